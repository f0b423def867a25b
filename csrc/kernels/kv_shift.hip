// Context shift (ops.kv_shift): move KV rows between blocks of the paged cache and re-rotate the keys.
//
// The cache stores K already rotated by RoPE, so a token that moves from position p to p - delta needs its K row
// rotated by -delta; V does not depend on the position.  The arena is kv [L, 2, NB, Hkv, 64, 128] bf16.  A move is
// (src, dst, row_lo, row_hi, delta): in every layer and KV head, for rows row_lo <= r < row_hi,
//   K row r of dst = K row r of src rotated by -delta   (delta 0: a plain copy)
//   V row r of dst = V row r of src                     (src == dst: V is not touched at all)
// Rotate-half convention (norm_rope.hip, ops/reference.py rope_append): the pair is (i, i + 64), and with
// c = cos[delta][i], s = sin[delta][i] from the model's own f32 tables
//   lo' = lo * c + hi * s,   hi' = hi * c - lo * s
// computed in f32 from the stored bf16 with every product and sum rounded on its own (no fused multiply-add, so the
// host twin's torch arithmetic gives the same bits), then rounded once to nearest-even bf16.
//
// grid (move, layer, 2 * Hkv * 2), 256 threads: a workgroup takes 32 rows of one (K | V, head) tile, a lane the two
// 16-byte pieces that hold dims 8j .. 8j+7 and 64+8j .. 64+8j+7 of one row -- both halves of its 8 pairs, so an
// in-place move has no hazard between lanes and needs no LDS.  Every lane issues its loads (two pieces, and for K
// the 8 cos and 8 sin values) before its stores; every K / V byte is read once and written at most once.  Plain
// 16-byte vector loads and stores only.  The host refuses move lists in which a destination row range overlaps
// another destination or another move's source (ops.kv_shift), so no workgroup reads a word that another one
// writes.  A move with an id outside (0, NB), rows outside 0 <= lo <= hi <= 64 or a delta outside the tables is
// skipped here, as kv_copy_blocks_kernel skips a bad pair.  kv_shift8_kernel, further down, is the same on the fp8
// cache.
#include "common.h"

constexpr int KVS_THREADS = 256, KVS_ROWS = KVS_THREADS / 8;

// A product as its own rounded f32: the empty asm makes the value opaque, so the build's -ffp-contract=fast (which
// ignores a contract(off) pragma) cannot fuse it into the sum that follows as v_fma / v_pk_fma.
__device__ __forceinline__ float kvs_rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(KVS_THREADS) void kv_shift_kernel(uint4* kv, const int* __restrict__ moves, int nb,
                                                               int hkv, const float4* __restrict__ cos_t,
                                                               const float4* __restrict__ sin_t, int table_rows) {
  const int* mv = moves + 5 * blockIdx.x;
  const int src = mv[0], dst = mv[1], lo = mv[2], hi = mv[3], delta = mv[4];
  if (src <= 0 || src >= nb || dst <= 0 || dst >= nb || lo < 0 || hi > 64 || lo > hi || delta < 0 ||
      delta >= table_rows)
    return;
  const int z = blockIdx.z, half = z & 1, h = (z >> 1) % hkv, is_v = (z >> 1) / hkv;
  if (src == dst && (is_v || delta == 0)) return;  // nothing moves
  const int row = half * KVS_ROWS + (threadIdx.x >> 3), j = threadIdx.x & 7;
  if (row < lo || row >= hi) return;
  const size_t plane = ((size_t)blockIdx.y * 2 + is_v) * nb;
  const size_t in_tile = ((size_t)h * 64 + row) * 16 + j;  // 16-byte units: a row is 16 of them
  const uint4* ps = kv + (plane + src) * (size_t)hkv * 1024 + in_tile;
  uint4* pd = kv + (plane + dst) * (size_t)hkv * 1024 + in_tile;
  const uint4 a = ps[0], b = ps[8];
  if (is_v || delta == 0) {
    pd[0] = a;
    pd[8] = b;
    return;
  }
  const float4* pc = cos_t + (size_t)delta * 16 + 2 * j;  // a table row is 64 f32 = 16 float4
  const float4* pn = sin_t + (size_t)delta * 16 + 2 * j;
  const float4 c0 = pc[0], c1 = pc[1], s0 = pn[0], s1 = pn[1];
  const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float x[8], y[8], xo[8], yo[8];
  unpack8(a, x);
  unpack8(b, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    xo[i] = kvs_rounded(x[i] * c[i]) + kvs_rounded(y[i] * s[i]);
    yo[i] = kvs_rounded(y[i] * c[i]) - kvs_rounded(x[i] * s[i]);
  }
  pd[0] = pack8(xo);
  pd[8] = pack8(yo);
}

// kv: the [L, 2, NB, Hkv, 64, 128] bf16 arena; moves: device int32 [n, 5]; cos / sin: f32 [table_rows, 64]
extern "C" int lsa_kv_shift(void* kv, const int* moves, int n, int layers, int nb, int hkv, const float* cos_t,
                            const float* sin_t, int table_rows, hipStream_t s) {
  if (n <= 0) return 0;
  if (layers <= 0 || layers > 65535 || n > 65535 || nb < 2 || hkv <= 0 || 4 * hkv > 65535 || table_rows <= 0 ||
      kv == nullptr || moves == nullptr || cos_t == nullptr || sin_t == nullptr)
    return -1;
  hipLaunchKernelGGL(kv_shift_kernel, dim3(n, layers, 4 * hkv), dim3(KVS_THREADS), 0, s, reinterpret_cast<uint4*>(kv),
                     moves, nb, hkv, reinterpret_cast<const float4*>(cos_t), reinterpret_cast<const float4*>(sin_t),
                     table_rows);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The same on the fp8 cache (ops.kv_shift8): kv [L, 2, NB, Hkv, 64, 128] e4m3 bytes, every (block, head) tile in
// token-pair order (common.h kv8_off), with the f32 row scales sc [L, 2, NB, Hkv, 64] in token order.  A rotated K
// row is dequantised (x = f32(byte) * scale), rotated as above, and quantised again by the rule of the fused append
// (norm_rope.hip; ops/reference.py quant_kv_rows): amax = the row's max |x'| over its 128 values, bytes =
// e4m3(x' * (448 / amax)), new scale = amax / 448; amax 0 stores zeros and scale 0.  V rows and delta-0 K rows are
// copied with their scales, bit for bit, when src != dst, and not touched when src == dst.
//
// grid (move, layer, 2 * Hkv), 256 threads: a workgroup takes one whole (K | V, head) tile.  The 8 lanes of token
// pair p take chunks j and j + 8 of the pair, that is dims 8j .. 8j+7 and 64+8j .. 64+8j+7 of tokens 2p and 2p + 1:
// both halves of 8 rotate-half pairs of two rows, whose amax is a DPP reduction over the 8 lanes (no LDS).  A token
// out of [row_lo, row_hi) is neither read nor written: a lane loads the two 16-byte units when both tokens of its
// pair are in range and the in-range token's two 8-byte halves otherwise, and it stores 8-byte halves only, so a
// 16-byte unit is never read, modified and written back, and tokens 2p and 2p + 1 may belong to two moves (rows
// [0, 5) beside rows [5, 64) of one block).  Lanes 0 and 1 of the 8 store the two scales.  Every load of a lane
// (bytes, scales, cos and sin) is issued before its first store.
__device__ __forceinline__ float kvs8_max8(float d) {  // max over the aligned 8 lanes, in each of them
  d = fmaxf(d, lsa_dpp<LSA_DPP_HALF_MIRROR>(d));
  d = fmaxf(d, lsa_dpp<LSA_DPP_XOR1>(d));
  return fmaxf(d, lsa_dpp<LSA_DPP_XOR2>(d));
}

// one row's 16 values of a lane: dequantise, rotate, and the lane's share of the row's amax
__device__ __forceinline__ float kvs8_rotate(const uint2 a, const uint2 b, float scale, const float* c, const float* s,
                                             float* xo, float* yo) {
  float x[8], y[8], m = 0.f;
  fp8x8_to_f32(a, x);
  fp8x8_to_f32(b, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float xv = kvs_rounded(x[i] * scale), yv = kvs_rounded(y[i] * scale);
    xo[i] = kvs_rounded(xv * c[i]) + kvs_rounded(yv * s[i]);
    yo[i] = kvs_rounded(yv * c[i]) - kvs_rounded(xv * s[i]);
    m = fmaxf(m, fmaxf(fabsf(xo[i]), fabsf(yo[i])));
  }
  return m;
}

__global__ __launch_bounds__(KVS_THREADS) void kv_shift8_kernel(uint2* kv, float* sc, const int* __restrict__ moves,
                                                                int nb, int hkv, const float4* __restrict__ cos_t,
                                                                const float4* __restrict__ sin_t, int table_rows) {
  const int* mv = moves + 5 * blockIdx.x;
  const int src = mv[0], dst = mv[1], lo = mv[2], hi = mv[3], delta = mv[4];
  if (src <= 0 || src >= nb || dst <= 0 || dst >= nb || lo < 0 || hi > 64 || lo > hi || delta < 0 ||
      delta >= table_rows)
    return;
  const int h = blockIdx.z % hkv, is_v = blockIdx.z / hkv;
  if (src == dst && (is_v || delta == 0)) return;  // nothing moves
  const int p = threadIdx.x >> 3, j = threadIdx.x & 7, r0 = 2 * p, r1 = r0 + 1;
  const bool in0 = r0 >= lo && r0 < hi, in1 = r1 >= lo && r1 < hi;
  if (!in0 && !in1) return;  // (the 8 lanes of a pair leave together: the reduction below stays inside them)
  const size_t plane = ((size_t)blockIdx.y * 2 + is_v) * nb;
  const size_t ts = ((plane + src) * hkv + h) * 64, td = ((plane + dst) * hkv + h) * 64;  // tile offsets, in rows
  const int u = (p * 16 + j) * 2;  // 8-byte halves: chunk j of token 2p; + 1: of token 2p + 1; + 16: chunk j + 8
  const uint2* ps = kv + ts * 16 + u;
  uint2* pd = kv + td * 16 + u;
  uint2 a0 = make_uint2(0, 0), b0 = a0, a1 = a0, b1 = a0;
  if (in0 && in1) {
    const uint4 ua = *reinterpret_cast<const uint4*>(ps), ub = *reinterpret_cast<const uint4*>(ps + 16);
    a0 = make_uint2(ua.x, ua.y); a1 = make_uint2(ua.z, ua.w);
    b0 = make_uint2(ub.x, ub.y); b1 = make_uint2(ub.z, ub.w);
  } else if (in0) {
    a0 = ps[0]; b0 = ps[16];
  } else {
    a1 = ps[1]; b1 = ps[17];
  }
  float s0 = in0 ? sc[ts + r0] : 0.f, s1 = in1 ? sc[ts + r1] : 0.f;
  if (!(is_v || delta == 0)) {
    const float4* pc = cos_t + (size_t)delta * 16 + 2 * j;  // a table row is 64 f32 = 16 float4
    const float4* pn = sin_t + (size_t)delta * 16 + 2 * j;
    const float4 c0 = pc[0], c1 = pc[1], n0 = pn[0], n1 = pn[1];
    const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float s[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    float x0[8], y0[8], x1[8], y1[8];
    const float m0 = kvs8_max8(kvs8_rotate(a0, b0, s0, c, s, x0, y0));
    const float m1 = kvs8_max8(kvs8_rotate(a1, b1, s1, c, s, x1, y1));
    const float i0 = kv8_inv(m0), i1 = kv8_inv(m1);
    a0 = pack8_fp8(x0, i0); b0 = pack8_fp8(y0, i0);
    a1 = pack8_fp8(x1, i1); b1 = pack8_fp8(y1, i1);
    s0 = m0 * LSA_KV8_RMAX; s1 = m1 * LSA_KV8_RMAX;
  }
  if (in0) {
    pd[0] = a0; pd[16] = b0;
    if (j == 0) sc[td + r0] = s0;
  }
  if (in1) {
    pd[1] = a1; pd[17] = b1;
    if (j == 1) sc[td + r1] = s1;
  }
}

// kv: the [L, 2, NB, Hkv, 64, 128] e4m3 arena; kv_scale: f32 [L, 2, NB, Hkv, 64]; the rest as lsa_kv_shift
extern "C" int lsa_kv_shift8(void* kv, float* kv_scale, const int* moves, int n, int layers, int nb, int hkv,
                             const float* cos_t, const float* sin_t, int table_rows, hipStream_t s) {
  if (n <= 0) return 0;
  if (layers <= 0 || layers > 65535 || n > 65535 || nb < 2 || hkv <= 0 || 2 * hkv > 65535 || table_rows <= 0 ||
      kv == nullptr || kv_scale == nullptr || moves == nullptr || cos_t == nullptr || sin_t == nullptr)
    return -1;
  hipLaunchKernelGGL(kv_shift8_kernel, dim3(n, layers, 2 * hkv), dim3(KVS_THREADS), 0, s, reinterpret_cast<uint2*>(kv),
                     kv_scale, moves, nb, hkv, reinterpret_cast<const float4*>(cos_t),
                     reinterpret_cast<const float4*>(sin_t), table_rows);
  return (int)hipGetLastError();
}
