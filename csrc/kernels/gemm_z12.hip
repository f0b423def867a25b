// Decode GEMM at 17-32 rows over a lossless 12-bit weight stream ("z12"):  out[M, N] = X[M, K] @ W[N, K]^T with the
// bf16 values of W, bit for bit, read as 784 bytes per 16 x 32 MFMA fragment instead of 1024.
//
// z12 (ops.pack_z12) is derived per tensor from the fragment-major bf16 layout Wf[nb][kb][lane][8] of gemm.hip; lane
// 16 g + r owns the same 8 elements W[16 nb + r][32 kb + 8 g + i]:
//   LO  [N/16][K/32][64 lanes][8 B]  byte i = the low byte of element i (exponent bit 0 + the 7 mantissa bits)
//   HI  [N/16][K/32][64 lanes][4 B]  one nibble per element, sign << 3 | (exp[7:1] - base); element j in the low and
//                                    element 4 + j in the high nibble of byte j.  base is one integer per tensor: the
//                                    start of the 8-value window of exp[7:1] (16 binades) that covers most elements
//   ESC [N/16][K/32][4] u32          up to four exact patches per fragment for elements outside the window (zeros,
//                                    outliers): valid << 31 | lane << 20 | slot << 16 | bf16 bits
// A wave loads LO (8 B per lane) and HI (4 B per lane) of each fragment and, once per k-step, the ESC records of all its
// NB fragments (lane l entry l & 3 of fragment min(l >> 2, NB - 1): a vector load, so the records arrive in order with
// the planes and waiting for them does not wait for the next chunk's, as a scalar load's out-of-order counter would;
// one ballot per k-step, nibble i of it says whether fragment i has patches, and the entries are read back with
// v_readlane at lanes 4 i .. 4 i + 3: 2 NB + 3 vector loads per k-step, 15 at nb 6, where a record load per fragment
// made 20), rebuilds exactly the uint4 gemm_skinny_kernel would have loaded, and issues the same MFMAs.  The chunk depth
// (SkinnyCfg), the work split, the peeled two-deep pipeline, the cross-wave reduction and the epilogues are the code of
// gemm_skinny.h that gemm_skinny_kernel runs too, so at equal (nb, splitk, waves, div) the output is bit-identical to
// the bf16 kernel's.
//
// Fragment-major activations (ops.to_xfrag) and two row tiles (MT = 2) only; epilogues bf16, f32 slabs, SiLU(gate)*up.
#include "gemm_skinny.h"

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint2 ldg_nt2(const uint2* p) {
  const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
  return make_uint2(v[0], v[1]);
}
__device__ __forceinline__ uint32_t ldg_nt1(const uint32_t* p) { return __builtin_nontemporal_load(p); }

// One fragment-lane: 8 low bytes + 8 codes -> the lane's 8 bf16.  The high byte of a code c is
// (c & 8) << 4 | ((c & 7) + base), formed for four codes at a time on a dword (base4 = base in every byte; (c & 7) +
// base <= 127, no carry between bytes), then two byte permutes per high-byte dword interleave it with the low bytes.
// v_perm_b32 selects from {src0 (bytes 4..7), src1 (bytes 0..3)}.
__device__ __forceinline__ uint4 z12_decode(const uint2 lo, const uint32_t hi, const uint32_t base4) {
  const uint32_t ha = ((hi & 0x07070707u) + base4) | ((hi & 0x08080808u) << 4);
  const uint32_t hb = (((hi >> 4) & 0x07070707u) + base4) | (hi & 0x80808080u);
  uint4 r;
  r.x = __builtin_amdgcn_perm(ha, lo.x, 0x05010400u);
  r.y = __builtin_amdgcn_perm(ha, lo.x, 0x07030602u);
  r.z = __builtin_amdgcn_perm(hb, lo.y, 0x05010400u);
  r.w = __builtin_amdgcn_perm(hb, lo.y, 0x07030602u);
  return r;
}

// one patch entry (wave-uniform) into the owning lane's fragment: unrolled selects, no register indexing
__device__ __forceinline__ void z12_patch1(uint4& w, const uint32_t e, const int lane) {
  const bool mine = (e >> 31) != 0u && ((e >> 20) & 63u) == (uint32_t)lane;
  const uint32_t slot = (e >> 16) & 7u, d = slot >> 1;
  const uint32_t keep = (slot & 1u) ? 0x0000ffffu : 0xffff0000u;
  const uint32_t ins = (slot & 1u) ? (e << 16) : (e & 0xffffu);
  w.x = (mine && d == 0u) ? ((w.x & keep) | ins) : w.x;
  w.y = (mine && d == 1u) ? ((w.y & keep) | ins) : w.y;
  w.z = (mine && d == 2u) ? ((w.z & keep) | ins) : w.z;
  w.w = (mine && d == 3u) ? ((w.w & keep) | ins) : w.w;
}

template <int NB, int EPI, int WAVES, int DIV>
__global__ __launch_bounds__(64 * WAVES) void gemm_z12_kernel(const uint16_t* __restrict__ X, int M, int KB,
                                                              const uint2* __restrict__ Lo,
                                                              const uint32_t* __restrict__ Hi,
                                                              const uint32_t* __restrict__ Esc, uint32_t base4,
                                                              void* __restrict__ out, int ldo, int kb_per_split,
                                                              LsaEpi ep) {
  constexpr int MT = 2;
  constexpr int U = SkinnyCfg<MT, NB, DIV>::U;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: chunk indices stay scalar
  const int r = lane & 15;
  int nb0, cnt;  // this workgroup's n-blocks (ragged grids: common.h skinny_nblocks)
  skinny_nblocks<NB, EPI == EPI_SILU ? 2 : 1>(EPI == EPI_SILU ? ldo / 8 : ldo / 16, nb0, cnt);
  const SkinnySplit ks = skinny_split<U, WAVES>(KB, kb_per_split, w);
  const int kbA = ks.kbA, kbB = ks.kbB;

  f32x4_t acc[NB][MT];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const uint16_t* xp[MT];
  bool xvalid[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    xvalid[j] = j * 16 + r < M;
    xp[j] = X + ((size_t)j * 64 + lane) * 8;
  }
  size_t fb[NB];  // first record of n-block i (blocks >= cnt re-read the workgroup's last block and are never stored)
#pragma unroll
  for (int i = 0; i < NB; ++i) fb[i] = (size_t)(nb0 + min(i, cnt - 1)) * KB;
  // this lane's patch entry: entry lane & 3 of the record of fragment min(lane >> 2, NB - 1), n-block as in fb[]
  const uint32_t* escp = Esc + (size_t)(nb0 + min(min(lane >> 2, NB - 1), cnt - 1)) * KB * 4 + (lane & 3);

  struct Chunk {
    uint2 lo[U][NB];
    uint32_t hi[U][NB];
    uint32_t esc[U];  // lanes 4 i .. 4 i + 3 hold the record of fragment i
    uint4 x[U][MT];
  };
  auto load = [&](Chunk& c, int ci) {
    const int kb = kbA + ci * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const size_t f = fb[i] + kk;
        c.lo[u][i] = ldg_nt2(Lo + f * 64 + lane);
        c.hi[u][i] = ldg_nt1(Hi + f * 64 + lane);
      }
      c.esc[u] = escp[(size_t)kk * 4];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int j = 0; j < MT; ++j) c.x[u][j] = *reinterpret_cast<const uint4*>(xp[j] + (size_t)kk * MT * 512);
    }
  };
  auto comp = [&](const Chunk& c, int ci) {
    const int kb = kbA + ci * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = (kb + u) < kbB;
      uint4 wv[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) wv[i] = z12_decode(c.lo[u][i], c.hi[u][i], base4);
      const uint32_t e = c.esc[u];
      // nibble i: the valid bits of fragment i's four entries (lanes >= 4 NB repeat the last record: masked off)
      const uint64_t pm = __builtin_amdgcn_ballot_w64((e >> 31) != 0u) & ((1ull << (4 * NB)) - 1ull);
      if (pm) {  // wave-uniform, rare
#pragma unroll
        for (int i = 0; i < NB; ++i)
          if ((pm >> (4 * i)) & 15ull) {
            z12_patch1(wv[i], __builtin_amdgcn_readlane(e, 4 * i + 0), lane);
            z12_patch1(wv[i], __builtin_amdgcn_readlane(e, 4 * i + 1), lane);
            z12_patch1(wv[i], __builtin_amdgcn_readlane(e, 4 * i + 2), lane);
            z12_patch1(wv[i], __builtin_amdgcn_readlane(e, 4 * i + 3), lane);
          }
      }
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const bool ok = live && xvalid[j];
        uint4 xv = c.x[u][j];
        xv.x = ok ? xv.x : 0u; xv.y = ok ? xv.y : 0u; xv.z = ok ? xv.z : 0u; xv.w = ok ? xv.w : 0u;
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[i][j] = mfma16x16x32(wv[i], xv, acc[i][j]);
      }
    }
  };

  // Two chunks in flight.  (Three and four, with counted vmcnt waits, measured equal or slower on every 7B shape and
  // slower inside the decode step, and were removed, ARCHITECTURE.md section 4.)
  if (ks.n_it > 0) {
    Chunk A, B;
    load(A, w);
    skinny_pipe_peeled<WAVES>(A, B, w, ks.n_it, load, comp);
  }
  skinny_epilogue<MT, NB, EPI, WAVES, true>(acc, w, lane, M, nb0, cnt, out, ldo, ep);
}

// ------------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------------
struct Z12Args {
  const uint16_t* X;
  int M, KB;
  const uint2* lo;
  const uint32_t* hi;
  const uint32_t* esc;
  uint32_t base4;
  int NBtot;
  void* out;
  int ldo, splitk, waves, div;
  LsaEpi ep;
  hipStream_t s;
};

template <int NB, int EPI, int WV, int DV>
static void launch_z12_d(const Z12Args& a) {
  const int kbps = (a.KB + a.splitk - 1) / a.splitk;
  dim3 grid((a.NBtot + NB - 1) / NB, a.splitk);  // ragged when NB does not divide NBtot (kernel deals the blocks)
  hipLaunchKernelGGL((gemm_z12_kernel<NB, EPI, WV, DV>), grid, dim3(64 * WV), 0, a.s, a.X, a.M, a.KB, a.lo, a.hi, a.esc,
                     a.base4, a.out, a.ldo, kbps, a.ep);
}

template <int NB, int EPI>
static void launch_z12_n(const Z12Args& a) {
  skinny_variant<NB>(a.waves, a.div, [&](auto wv, auto dv) { launch_z12_d<NB, EPI, decltype(wv)::value, decltype(dv)::value>(a); });
}

template <int EPI>
static int launch_z12_e(const Z12Args& a, int nb) {
  if (nb == 2) launch_z12_n<2, EPI>(a);
  else if (nb == 4) launch_z12_n<4, EPI>(a);
  else if (nb == 6) launch_z12_n<6, EPI>(a);
  else return -2;
  return 0;
}

// X fragment-major (ops.to_xfrag, two row tiles); lo / hi / esc / base: ops.pack_z12 of the [N, K] weight.
// ep (nullable): row scale only (no residual epilogue).
extern "C" int lsa_gemm_z12(const void* X, int M, int K, const void* lo, const void* hi, const void* esc, int base, int N,
                            void* out, int epi, int nb, int splitk, int waves, int div, const LsaEpi* ep,
                            hipStream_t stream) {
  if (K % 32 != 0 || N % 16 != 0 || M <= 16 || M > 32) return -1;
  if (base < 1 || base > 120) return -1;
  if (ep && (ep->h || ep->xout || ep->ss_out)) return -8;
  if (epi != EPI_BF16 && epi != EPI_F32 && epi != EPI_SILU) return -4;
  const int NBtot = N / 16;
  if (nb != 2 && nb != 4 && nb != 6) return -2;
  if (!skinny_grid_ok(NBtot, nb, epi == EPI_SILU)) return -2;
  if (splitk < 1) splitk = 1;
  if (splitk > K / 32) return -3;
  if (epi != EPI_F32 && splitk != 1) return -3;
  Z12Args a;
  a.X = reinterpret_cast<const uint16_t*>(X);
  a.M = M;
  a.KB = K / 32;
  a.lo = reinterpret_cast<const uint2*>(lo);
  a.hi = reinterpret_cast<const uint32_t*>(hi);
  a.esc = reinterpret_cast<const uint32_t*>(esc);
  a.base4 = (uint32_t)base * 0x01010101u;
  a.NBtot = NBtot;
  a.out = out;
  a.ldo = epi == EPI_SILU ? N / 2 : N;
  a.splitk = splitk;
  a.waves = waves == 8 ? 8 : 4;
  a.div = (div == 1 || div == 2) ? div : 4;
  a.ep = ep ? *ep : LsaEpi{};
  a.s = stream;
  int rc;
  switch (epi) {
    case EPI_BF16: rc = launch_z12_e<EPI_BF16>(a, nb); break;
    case EPI_F32: rc = launch_z12_e<EPI_F32>(a, nb); break;
    default: rc = launch_z12_e<EPI_SILU>(a, nb); break;
  }
  if (rc) return rc;
  return (int)hipGetLastError();
}
