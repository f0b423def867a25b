// Verify attention of speculative decoding: the T = k + 1 new tokens of each of S sequences against the paged KV cache
// (layout of attention.hip: [num_blocks, Hkv, 64 tokens, 128]; bf16, or -- KV8 -- the fp8 cache), head_dim 128.
//
//   attn_verify_kernel   split-KV like attn_decode_kernel, grid (Hkv, nsplit, S), 4 waves.  Sequence s = blockIdx.z
//                        reads pos0[s], block-table row s and query rows s T .. s T + T - 1, and owns output rows,
//                        split partials ((s T H + row) nsplit + split) and tickets (s Hkv + hk) of its own: no word is
//                        read by a workgroup of another sequence, and each sequence takes eff_split from its own
//                        context (unsplit, split and early return side by side in one launch).  S = 1 is the
//                        one-sequence launch: same grid, same offsets.  Per sequence: all R = T * G query rows
//                        (row r = t * G + g: token t, head hk * G + g; R <= 16) of a kv head are the 16-wide side of
//                        the bf16 16x16x32 MFMA, so a workgroup reads every K / V byte of its block range once for
//                        all rows -- the cost of a verify step's attention is close to one decode step's, not T.
//                        Wave w owns keys 16 w .. 16 w + 15 of each 64-key block:
//                          S^T = K Q^T   the cache row [token][128] is the A-operand layout (a lane's 8 k-elements are
//                                        16 contiguous bytes): K goes global -> VGPR -> MFMA, no LDS; a lane then owns
//                                        one query row (attn_prefill_kernel's softmax: 4 values + 2 lane exchanges);
//                          O += P V      P stays in registers as the A operand (its upper 16 k-slots are zero: a wave
//                                        has 16 keys per block); V is staged by the wave itself into the XOR-swizzled
//                                        LDS image of attention.hip (v_off) and read transposed (ds_read_b64_tr_b16).
//                        Causality: row (t, g) sees key j iff j <= pos0 + t; the T new tokens' K / V are already in
//                        the cache (a rope_append launch precedes).  Online softmax in the exp2 domain with the finite
//                        LSA_NEG sentinel; a masked score contributes p = 0 explicitly, so a (row, split) whose every
//                        key is masked carries (m = LSA_NEG, l = 0, o = 0) and combines to exactly zero weight.
//                        The 4 waves merge through LDS; one split writes the output, more publish (o, m, l) partials
//                        and the last-arriving split of the kv head combines them in the same launch (the ticket
//                        protocol of attn_decode_kernel; the ticket word is left zeroed).
//                        Everything data-dependent (pos0, the block table) is read from device memory: a captured
//                        graph replays.  Fixed reduction order: two runs are bitwise equal.
//   attn_verify_kernel<true>   the same kernel over the fp8 cache (attn_decode_kernel<.., KV8>'s layout: 8 KiB of e4m3
//                        bytes per (block, kv-head) tile in the token-pair order of common.h kv8_off, f32 scales
//                        ksc / vsc [blocks, Hkv, 64] in token order).  Same grid, wave / key ownership, split combine
//                        and reduction order; half the K / V bytes:
//                          K   lane (g, r) loads the four 8-byte halves of key 16 w + r's chunks (dims 32 s + 8 g .. + 7)
//                              and widens them exactly to bf16 (v_cvt_scalef32_pk_bf16_fp8 at scale 1) as the A operand;
//                              the key's scale x the softmax scale multiplies the score (one float4 load per lane: the
//                              scales of keys 16 w + 4 g .. + 3, the four scores the lane owns);
//                          V   two 16-byte units per lane (token pair 8 w + 4 i + g, dims 8 r .. + 7), each half widened
//                              to bf16 into the same XOR-swizzled LDS image; the value's scale is folded into p before P
//                              is packed to bf16, the row sum l keeps the unscaled p.  A masked key (past a row's limit,
//                              the pair partner of the last visible key included) contributes p = 0 and its scales are
//                              never used.
//
// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage: 164 VGPRs + 32 AGPRs, 51 SGPRs, scratch 0,
// no spills, LDS 49668 bytes per workgroup, occupancy 2 waves per SIMD (the grid is Hkv x nsplit x S workgroups of
// 4 waves, planned at about 256: at most one workgroup per CU is resident then; registers admit two, LDS three).
// KV8: 134 VGPRs + 32 AGPRs, 56 SGPRs, scratch 0, no spills, LDS 49668 bytes, occupancy 3.  (The sequence index cost
// 7 / 6 SGPRs and no vector register over the one-sequence kernel.)
#include "common.h"

#define LSA_NEG (-1.0e30f)
#define LSA_SC1 16  // buffer cache-policy aux bit: sc1 (write-through store / L1-bypassing load)

typedef __attribute__((address_space(1))) unsigned long long av_g_u64;
typedef __attribute__((address_space(1))) int av_g_i32;
typedef short av_s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) av_s16x4_t* av_lds_s4_ptr;

__device__ __forceinline__ uint2 av_read_tr16(const uint16_t* p) {
  av_s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((av_lds_s4_ptr)(p));
  return __builtin_bit_cast(uint2, v);
}
// V image (attention.hip v_off): 16 B chunk ch of row r at chunk (ch ^ ((r & 7) << 1))
__device__ __forceinline__ int av_v_off(int r, int col) {
  return r * 128 + ((((col >> 3) ^ ((r & 7) << 1))) << 3) + (col & 7);
}

typedef uint32_t av_u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 av_ldg_nt8(const uint8_t* p) {
  const av_u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const av_u32x2_t*>(p));
  return make_uint2(v[0], v[1]);
}

template <bool KV8>
__global__ __launch_bounds__(256) void attn_verify_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
                                                          const uint16_t* __restrict__ vc,
                                                          const int* __restrict__ bt_all, int max_blocks,
                                                          const int* __restrict__ pos0_p, int T, int G, int Hkv,
                                                          float scale_log2, int chunk_blocks, int nsplit, int unsplit_max,
                                                          uint16_t* __restrict__ out, float* __restrict__ opart,
                                                          float* __restrict__ mlpart, int* __restrict__ counters,
                                                          const float* __restrict__ ksc, const float* __restrict__ vsc) {
  constexpr int D = 128;
  __shared__ __attribute__((aligned(16))) uint16_t Vs[64 * D];   // wave w writes and reads rows 16 w .. 16 w + 15 only
  __shared__ __attribute__((aligned(16))) float so[4][16][D];    // per-wave partial outputs
  __shared__ float sm[4][16], sl[4][16];
  __shared__ int s_last;
  const int hk = blockIdx.x, split = blockIdx.y, seq = blockIdx.z;
  const int H = Hkv * G, R = T * G;
  const size_t row0 = (size_t)seq * T * H;  // the sequence's first [S * T, H] row: queries, output and partials
  const int* __restrict__ bt = bt_all + (size_t)seq * max_blocks;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, r = lane & 15;
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(opart, 0, 0x7fffffff, 0x00020000);

  const int pos0 = pos0_p[seq];
  const int ctx = pos0 + T;
  const int nblk = min((ctx + 63) >> 6, max_blocks);
  int ech, nse;
  eff_split(nblk, chunk_blocks, nsplit, unsplit_max, ech, nse);
  if (split >= nse) return;  // whole workgroup: this context needs fewer splits
  const int blk0 = split * ech;
  const int blk1 = min(nblk, blk0 + ech);

  // query row r of this lane (rows >= R repeat row R - 1; never stored): B operand, k = 32 s + 8 g .. + 7
  const int rr = min(r, R - 1);
  const int qt = rr / G, qg = rr - qt * G;
  const int qpos = pos0 + qt;
  uint4 qf[4];
  {
    const uint16_t* qrow = q + (row0 + (size_t)qt * H + hk * G + qg) * D;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const uint4*>(qrow + 32 * s + 8 * g);
  }

  f32x4_t o[8];
  float mrow = LSA_NEG, lrow = 0.f;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // register staging of the next block's K (A operand rows) and V (row-major chunks for the LDS image), issued
  // right after the current block's registers are consumed (block index clamped: no conditional refill)
  uint4 kr[4], vr[4];
  // KV8: the lane's K chunks are the 8-byte halves of four token-pair units (kv8_off: key 16 w + r, dims 32 s + 8 g);
  // a V unit carries dims 8 r .. 8 r + 7 of the token pair 8 w + 4 i + g; one float4 holds the scales of keys
  // 16 w + 4 g .. + 3, the keys whose scores (and p) this lane owns
  uint2 kr8[4];
  uint4 vr8[2];
  float4 ksr, vsr;
  auto fetch = [&](int blk) {
    if constexpr (KV8) {
      const size_t rowb = ((size_t)__builtin_amdgcn_readfirstlane(bt[blk]) * Hkv + hk) * 64;
      const uint8_t* k8 = reinterpret_cast<const uint8_t*>(kc) + rowb * D;
      const uint8_t* v8 = reinterpret_cast<const uint8_t*>(vc) + rowb * D;
#pragma unroll
      for (int s = 0; s < 4; ++s) kr8[s] = av_ldg_nt8(k8 + kv8_off(16 * w + r, 32 * s + 8 * g));
#pragma unroll
      for (int i = 0; i < 2; ++i)
        vr8[i] = ldg_nt(reinterpret_cast<const uint4*>(v8 + kv8_off(16 * w + 8 * i + 2 * g, 8 * r)));
      ksr = *reinterpret_cast<const float4*>(ksc + rowb + 16 * w + 4 * g);
      vsr = *reinterpret_cast<const float4*>(vsc + rowb + 16 * w + 4 * g);
    } else {
      const size_t base = ((size_t)__builtin_amdgcn_readfirstlane(bt[blk]) * Hkv + hk) * 64 * D;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        kr[s] = ldg_nt(reinterpret_cast<const uint4*>(kc + base + (16 * w + r) * D + 32 * s + 8 * g));
#pragma unroll
      for (int i = 0; i < 4; ++i)
        vr[i] = ldg_nt(reinterpret_cast<const uint4*>(vc + base + (16 * w + 4 * i + g) * D + 8 * r));
    }
  };
  if (blk0 < blk1) fetch(blk0);
  const int qq = r >> 2, pp = r & 3;
  for (int blk = blk0; blk < blk1; ++blk) {
    __syncthreads();  // the previous block's transposed V reads are done
    uint4 kq[4];
    float ksl[4], vsl[4];  // KV8: key scale x softmax scale, value scale of keys 16 w + 4 g + i
    if constexpr (KV8) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {  // both tokens of the pair widened exactly to bf16 rows of the same LDS image
        const int row = 16 * w + 8 * i + 2 * g;
        *reinterpret_cast<uint4*>(&Vs[av_v_off(row, 8 * r)]) = fp8x8_to_bf16x8(make_uint2(vr8[i].x, vr8[i].y));
        *reinterpret_cast<uint4*>(&Vs[av_v_off(row + 1, 8 * r)]) = fp8x8_to_bf16x8(make_uint2(vr8[i].z, vr8[i].w));
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) kq[s] = fp8x8_to_bf16x8(kr8[s]);
      ksl[0] = ksr.x * scale_log2; ksl[1] = ksr.y * scale_log2; ksl[2] = ksr.z * scale_log2; ksl[3] = ksr.w * scale_log2;
      vsl[0] = vsr.x; vsl[1] = vsr.y; vsl[2] = vsr.z; vsl[3] = vsr.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<uint4*>(&Vs[av_v_off(16 * w + 4 * i + g, 8 * r)]) = vr[i];
        kq[i] = kr[i];
      }
    }
    __syncthreads();
    fetch(min(blk + 1, blk1 - 1));

    // S^T[key 4 g + i][query r] over the wave's 16 keys
    f32x4_t st = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) st = mfma16x16x32(kq[s], qf[s], st);
    float tmax = LSA_NEG;
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = blk * 64 + 16 * w + 4 * g + i;
      ok[i] = key <= qpos;
      if constexpr (KV8) st[i] = ok[i] ? st[i] * ksl[i] : LSA_NEG;
      else st[i] = ok[i] ? st[i] * scale_log2 : LSA_NEG;
      tmax = fmaxf(tmax, st[i]);
    }
    tmax = lsa_max_x32(lsa_max_x16(tmax));
    const float mnew = fmaxf(mrow, tmax);
    const float alpha = __builtin_amdgcn_exp2f(mrow - mnew);
    mrow = mnew;
    float p[4], psum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = ok[i] ? __builtin_amdgcn_exp2f(st[i] - mnew) : 0.f;  // (an all-masked row has mnew = LSA_NEG: exp2(0))
      psum += p[i];
    }
    lrow = lrow * alpha + psum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ai = __shfl(alpha, 4 * g + i, 64);
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) o[dt][i] *= ai;
    }
    // O[query 4 g + i][d 16 dt + r] += P V: A = P (k-slot 8 g + j <-> key 4 g + j, j < 4; slots j >= 4 zero),
    // B = V read transposed: lane (g, r) gets V[keys 4 g .. 4 g + 3][d = 16 dt + r]
    uint4 pa;
    if constexpr (KV8) {  // V's row scale rides in p (l keeps the unscaled p); a masked key's scale is never used
      pa.x = pack2bf(ok[0] ? p[0] * vsl[0] : 0.f, ok[1] ? p[1] * vsl[1] : 0.f);
      pa.y = pack2bf(ok[2] ? p[2] * vsl[2] : 0.f, ok[3] ? p[3] * vsl[3] : 0.f);
    } else {
      pa.x = pack2bf(p[0], p[1]);
      pa.y = pack2bf(p[2], p[3]);
    }
    pa.z = 0u;
    pa.w = 0u;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const uint2 v1 = av_read_tr16(&Vs[av_v_off(16 * w + 4 * g + qq, 16 * dt + 4 * pp)]);
      uint4 vb;
      vb.x = v1.x; vb.y = v1.y; vb.z = 0u; vb.w = 0u;
      o[dt] = mfma16x16x32(pa, vb, o[dt]);
    }
  }

  // merge the 4 waves: each publishes (m, l, o) of its key quarter for all 16 rows
  const float lt = lsa_sum_x32(lsa_sum_x16(lrow));
  if (g == 0) {
    sm[w][r] = mrow;
    sl[w][r] = lt;
  }
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) so[w][4 * g + i][16 * dt + r] = o[dt][i];
  __syncthreads();
  // each thread finishes 4 consecutive dims of one row
  for (int e = tid; e < R * 32; e += 256) {
    const int row = e >> 5, d0 = (e & 31) * 4;
    float M = LSA_NEG;
#pragma unroll
    for (int k = 0; k < 4; ++k) M = fmaxf(M, sm[k][row]);
    float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float wgt = __builtin_amdgcn_exp2f(sm[k][row] - M);
      L += sl[k][row] * wgt;
      const float4 v = *reinterpret_cast<const float4*>(&so[k][row][d0]);
      O[0] += v.x * wgt; O[1] += v.y * wgt; O[2] += v.z * wgt; O[3] += v.w * wgt;
    }
    const int t = row / G;
    const size_t orow = row0 + (size_t)t * H + hk * G + (row - t * G);  // [S * T, H] row of the output and partials
    if (nse == 1) {
      const float inv = L > 0.f ? 1.f / L : 0.f;
      uint2 pk;
      pk.x = pack2bf(O[0] * inv, O[1] * inv);
      pk.y = pack2bf(O[2] * inv, O[3] * inv);
      *reinterpret_cast<uint2*>(out + orow * D + d0) = pk;
    } else {
      // publish the partial write-through (sc1): the reducing workgroup may sit on another XCD
      const size_t pi = orow * nsplit + split;
      const u32x4_t v = {__float_as_uint(O[0]), __float_as_uint(O[1]), __float_as_uint(O[2]), __float_as_uint(O[3])};
      __builtin_amdgcn_raw_buffer_store_b128(v, rs_o, (int)((pi * D + d0) * 4), 0, LSA_SC1);
      if (d0 == 0)
        __hip_atomic_store((av_g_u64*)(mlpart) + pi,
                           ((unsigned long long)__float_as_uint(L) << 32) | __float_as_uint(M), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (nse == 1) return;

  // split-KV combine inside the launch (attn_decode_kernel's protocol: sc1 stores drained -> barrier -> one relaxed
  // agent ticket add; the reducer reads every partial with sc1 loads and resets the ticket for the next launch)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  av_g_i32* ctr = (av_g_i32*)(counters) + seq * Hkv + hk;
  if (tid == 0) s_last = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nse - 1;
  __syncthreads();
  if (!s_last) return;
  if (tid == 0) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int e = tid; e < R * 32; e += 256) {
    const int row = e >> 5, d0 = (e & 31) * 4;
    const int t = row / G;
    const size_t orow = row0 + (size_t)t * H + hk * G + (row - t * G);
    const size_t pi0 = orow * nsplit;
    float M = LSA_NEG, L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int sp = 0; sp < nse; ++sp) {
      const unsigned long long ml =
          __hip_atomic_load((av_g_u64*)(mlpart) + pi0 + sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_o, (int)(((pi0 + sp) * D + d0) * 4), 0, LSA_SC1);
      const float mi = __uint_as_float((uint32_t)ml), li = __uint_as_float((uint32_t)(ml >> 32));
      const float mn = fmaxf(M, mi);
      const float a = __builtin_amdgcn_exp2f(M - mn), wgt = __builtin_amdgcn_exp2f(mi - mn);
      M = mn;
      L = L * a + li * wgt;
      O[0] = O[0] * a + __uint_as_float(v[0]) * wgt; O[1] = O[1] * a + __uint_as_float(v[1]) * wgt;
      O[2] = O[2] * a + __uint_as_float(v[2]) * wgt; O[3] = O[3] * a + __uint_as_float(v[3]) * wgt;
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
    uint2 pk;
    pk.x = pack2bf(O[0] * inv, O[1] * inv);
    pk.y = pack2bf(O[2] * inv, O[3] * inv);
    *reinterpret_cast<uint2*>(out + orow * D + d0) = pk;
  }
}

// q [S, T, H, 128] bf16 (rotated); bt: the sequences' block-table rows [S, max_blocks]; pos0 [S]: device int32, position
// of each sequence's row 0; ks / vs: the fp8 cache's scale arrays [blocks, Hkv, 64] f32 (kc / vc are then e4m3 bytes),
// null for the bf16 cache; out [S * T, H * 128] bf16; workspace for S * T * H rows x nsplit partials and S * Hkv zeroed
// tickets (ops.verify_workspace).  1 <= S <= 8 and S * T <= 32 rows.
extern "C" int lsa_attn_verify(const void* q, const void* kc, const void* vc, const int* bt, int max_blocks,
                               const int* pos0, int S, int T, int H, int Hkv, float scale, int chunk_blocks, int nsplit,
                               int unsplit_max, void* out, float* opart, float* mlpart, int* counters, hipStream_t s,
                               const float* ks = nullptr, const float* vs = nullptr) {
  if (Hkv <= 0 || H <= 0 || H % Hkv) return -1;
  const int G = H / Hkv;
  if (T < 1 || T > 8 || T * G > 16) return -2;
  if (nsplit < 1 || nsplit > 256 || chunk_blocks < 1) return -3;
  if (max_blocks < 1) return -4;
  if ((ks == nullptr) != (vs == nullptr)) return -5;  // the fp8 cache needs both scale arrays
  if (S < 1 || S > 8) return -6;
  if (S * T > 32) return -7;
#define LSA_AVL(KV8)                                                                                                  \
  hipLaunchKernelGGL((attn_verify_kernel<KV8>), dim3(Hkv, nsplit, S), dim3(256), 0, s,                                \
                     reinterpret_cast<const uint16_t*>(q), reinterpret_cast<const uint16_t*>(kc),                     \
                     reinterpret_cast<const uint16_t*>(vc), bt, max_blocks, pos0, T, G, Hkv,                          \
                     scale * 1.4426950408889634f, chunk_blocks, nsplit, unsplit_max, reinterpret_cast<uint16_t*>(out), \
                     opart, mlpart, counters, ks, vs)
  if (ks != nullptr) LSA_AVL(true);
  else LSA_AVL(false);
#undef LSA_AVL
  return (int)hipGetLastError();
}
