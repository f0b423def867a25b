// GGUF Q4_0 (ggml block_q4_0: 32 consecutive k share one f16 scale d, elements are 4-bit codes q, value d * (q - 8))
// weight-only linear layers, served with the file's own codes and scales:
//   out = X[M, K] @ dequant(Wq, D)^T     (bf16 activations, f32 accumulate on MFMA 16x16x32 bf16)
//
// The value rule (ops.dequantize_q4_0 is its host twin): w = bf16_rne(f32(d) * f32(q - 8)).  The f32 product is exact
// (11 significand bits x 4 bits), so the only rounding is the one to bf16.  The kernels form it as
// fma(f32(q), d, -8 d): q d, -8 d and their sum are all exact in f32, the fma rounds nothing, and v_cvt_pk_bf16_f32
// rounds to nearest even -- the same value; a zero (d = 0, or q = 8) comes out as +0 where the product form can give
// -0, which no sum and no comparison of values can tell apart.
//
// Weight layout (ops.pack_q4_0): Wq[nb][kb128][lane][16 B], lane = 16 g + r holds W[16 nb + r][128 kb + 32 g .. + 31],
// exactly one Q4_0 block per lane and 128-k step, so one 16-B load per lane feeds FOUR mfma_f32_16x16x32_bf16 k-steps:
// step s uses the lane's elements 8 s .. 8 s + 7 (the k order inside an MFMA step only has to agree between A and B,
// as in gemm_fp4.hip).  Nibble order inside the 16 bytes: dword s holds elements 8 s .. 8 s + 7, byte i of it element
// 8 s + i in its low nibble and element 8 s + 4 + i in its high nibble.  w & 0x0f0f0f0f and (w >> 4) & 0x0f0f0f0f are
// then elements 0..3 and 4..7 as bytes in order: v_cvt_f32_ubyte0..3 reads each without a further shift, and the
// pairs (0,1) (2,3) (4,5) (6,7) that v_cvt_pk_bf16_f32 packs are neighbours.  3 mask/shift + 8 cvt + 8 fma + 4 pack
// VALU ops per 8 weights.
// Scales: D[nb][ceil(kb128 / 2)][lane][4 B] -- the lane's f16 d of two consecutive 128-k steps in one word (even step
// in the low half).
// Work split, pipeline (clamped tail: a dead step runs with d = 0 and contributes zeros), reduction and epilogues:
// gemm_skinny.h -- bf16, f32 split-K slabs, SiLU * up (gate / up rows interleaved per 16), and the LsaEpi row scale
// that comes with the skeleton (the residual epilogue is not instantiated).  Prefill (M > 64) dequantises the layer
// into a bf16 fragment-layout scratch (lsa_q4_dequant) for the tile GEMM.  Plain vector loads and stores only.
#include "gemm_skinny.h"

namespace {

__device__ __forceinline__ float f16_f32(uint32_t h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);  // v_cvt_f32_f16: exact, subnormals included
}

// 8 codes (one dword, the nibble order above) -> one bf16 MFMA fragment (8 values) by the value rule; m8d = -8 d
__device__ __forceinline__ uint4 q4x8_to_bf16(uint32_t w, float d, float m8d) {
  const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
  auto v = [&](uint32_t b, int i) { return __builtin_fmaf((float)((b >> (8 * i)) & 0xffu), d, m8d); };
  return make_uint4(pack2bf(v(lo, 0), v(lo, 1)), pack2bf(v(lo, 2), v(lo, 3)), pack2bf(v(hi, 0), v(hi, 1)),
                    pack2bf(v(hi, 2), v(hi, 3)));
}

}  // namespace

// XF: X in the fragment-major decode layout (common.h xf_off): lane (r, g)'s 8 activations of step s,
// k = 128 kb + 32 g + 8 s .. + 7, are lane (16 s + r) of bf16 k-step 4 kb + g
template <int MT, int NB, int EPI, int WAVES, int U, bool XF = false>
__global__ __launch_bounds__(64 * WAVES) void gemm_q4_skinny_kernel(const uint16_t* __restrict__ X, int ldx, int M,
                                                                    int KB128, const uint4* __restrict__ Wq,
                                                                    const uint32_t* __restrict__ Dw,
                                                                    void* __restrict__ out, int ldo, int kb_per_split,
                                                                    LsaEpi ep) {
  // chunks of U 128-k steps
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  int nb0, cnt;  // this workgroup's n-blocks (ragged grids: common.h skinny_nblocks)
  skinny_nblocks<NB, EPI == EPI_SILU ? 2 : 1>(EPI == EPI_SILU ? ldo / 8 : ldo / 16, nb0, cnt);
  const SkinnySplit ks = skinny_split<U, WAVES>(KB128, kb_per_split, w);
  const int kbA = ks.kbA, kbB = ks.kbB;
  const int last_c = w + WAVES * (ks.n_it - 1);  // this wave's last chunk: the clamped pipeline's bound (gemm_skinny.h)
  const int KB2 = (KB128 + 1) >> 1;

  f32x4_t acc[NB][MT];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  bool xvalid[MT];
  // row-major X: padding rows (>= M) read zeros from past the buffer range, no memory request (gemm.hip)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, XF ? 0x7fffffff : M * ldx * 2, 0x00020000);
  uint32_t xoff[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = j * 16 + r;
    xvalid[j] = m < M;
    xoff[j] = XF ? (uint32_t)((((size_t)g * MT + j) * 64 + r) * 16)
                 : (xvalid[j] ? (uint32_t)(((size_t)m * ldx + 32 * g) * 2) : 0x80000000u);
  }
  const uint4* wp[NB];
  const uint32_t* dp[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    wp[i] = Wq + (size_t)(nb0 + min(i, cnt - 1)) * KB128 * 64 + lane;
    dp[i] = Dw + (size_t)(nb0 + min(i, cnt - 1)) * KB2 * 64 + lane;
  }

  struct Chunk {
    uint4 w[U][NB], x[U][MT][4];
    uint32_t d[U][NB];  // the block's f16 d, as loaded
  };
  auto load = [&](Chunk& ch, int c) {
    uint4(&wr)[U][NB] = ch.w;
    uint32_t(&dr)[U][NB] = ch.d;
    uint4(&xr)[U][MT][4] = ch.x;
    const int kb = kbA + c * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        wr[u][i] = ldg_nt(wp[i] + (size_t)kk * 64);
        dr[u][i] = (dp[i][(size_t)(kk >> 1) * 64] >> (16 * (kk & 1))) & 0xffffu;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int j = 0; j < MT; ++j) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          // XF: bf16 k-step 4 kk + g, lane 16 s + r; row-major: x[m][128 kk + 32 g + 8 s]
          const uint32_t o = XF ? xoff[j] + (uint32_t)(((size_t)kk * 4 * MT * 64 + 16 * s) * 16)
                                : xoff[j] + (uint32_t)kk * 256u + 16u * s;
          const u32x4_t a = __builtin_amdgcn_raw_buffer_load_b128(xrs, o, 0, 0);
          xr[u][j][s] = make_uint4(a[0], a[1], a[2], a[3]);
        }
      }
    }
  };
  auto comp = [&](const Chunk& ch, int c) {
    const uint4(&wr)[U][NB] = ch.w;
    const uint32_t(&dr)[U][NB] = ch.d;
    const uint4(&xr)[U][MT][4] = ch.x;
    const int kb = kbA + c * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = (kb + u) < kbB;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const float d = live ? f16_f32(dr[u][i]) : 0.f;  // a dead (clamped) step contributes zeros
        const float m8d = -8.f * d;
        const uint32_t q[4] = {wr[u][i].x, wr[u][i].y, wr[u][i].z, wr[u][i].w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const uint4 a = q4x8_to_bf16(q[s], d, m8d);
#pragma unroll
          for (int j = 0; j < MT; ++j) acc[i][j] = mfma16x16x32(a, xr[u][j][s], acc[i][j]);  // padding rows:
          // their own (discarded) output rows only
        }
      }
    }
  };
  if (ks.n_it > 0) {
    Chunk A, B;
    load(A, w);
    skinny_pipe_clamped<WAVES>(A, B, w, ks.n_it, last_c, load, comp);
  }
  skinny_epilogue<MT, NB, EPI, WAVES, XF>(acc, w, lane, M, nb0, cnt, out, ldo, ep);
}

// q4_0 [nb][kb128][lane][16 B] + d -> bf16 fragment layout [nb][kb32][lane][8] (ops.shuffle_weight), the same value
// rule by the same instruction sequence
__global__ __launch_bounds__(256) void q4_dequant_kernel(const uint4* __restrict__ Wq, const uint32_t* __restrict__ Dw,
                                                         int KB128, long nfrag, uint4* __restrict__ Wf) {
  const int KB2 = (KB128 + 1) >> 1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nfrag * 64; i += (long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const long f = i >> 6;  // (nb, kb128)
    const long nb = f / KB128;
    const int kb = (int)(f % KB128);
    const int r = lane & 15, g = lane >> 4;
    const float d = f16_f32((Dw[(nb * KB2 + (kb >> 1)) * 64 + lane] >> (16 * (kb & 1))) & 0xffffu);
    const float m8d = -8.f * d;
    const uint4 q = Wq[i];
    const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
    // element k = 128 kb + 32 g + 8 s + e -> bf16 fragment kb32 = 4 kb + g, lane' = 16 s + r
#pragma unroll
    for (int s = 0; s < 4; ++s) Wf[((nb * 4L * KB128) + 4L * kb + g) * 64 + 16 * s + r] = q4x8_to_bf16(qw[s], d, m8d);
  }
}

static thread_local int g_q4_xfrag = 0;
static thread_local LsaEpi g_q4_epi = {};

template <int MT, int NB, int EPI, int WV, int U>
static void launch_qx(const uint16_t* X, int ldx, int M, int KB128, const uint4* Wq, const uint32_t* D, int NBtot,
                      void* out, int ldo, int kbps, int splitk, hipStream_t s) {
  if (g_q4_xfrag)
    hipLaunchKernelGGL((gemm_q4_skinny_kernel<MT, NB, EPI, WV, U, true>), dim3((NBtot + NB - 1) / NB, splitk), dim3(64 * WV), 0,
                       s, X, ldx, M, KB128, Wq, D, out, ldo, kbps, g_q4_epi);
  else
    hipLaunchKernelGGL((gemm_q4_skinny_kernel<MT, NB, EPI, WV, U, false>), dim3((NBtot + NB - 1) / NB, splitk), dim3(64 * WV), 0,
                       s, X, ldx, M, KB128, Wq, D, out, ldo, kbps, g_q4_epi);
}

// The instantiation set: row tiles mt 1 | 2 x nb 1 | 2 | 4 | 8, mt 4 x nb 1 | 2 (the launcher clamps nb to 2 above 32
// rows), each at 4 and 8 waves, nb 8 at 4 waves only (two row tiles of it spill at 8; the 16-bit kernels keep their
// wide n-groups to 4 waves too); SiLU needs gate / up pairs, so no nb 1.  Any other nb runs nb 2 (lsa_q4_gemm_ex
// rewrites it before its grid check).  Chunk depth: U = 2 128-k steps, 1 where the registers of a wide n-group, of
// four row tiles (two steps of them left the accumulators' AGPRs as spill space inside the loop) or of 8-wave
// workgroups ask for it.
template <int EPI>
static void launch_qe(const uint16_t* X, int ldx, int M, int KB128, const uint4* Wq, const uint32_t* D, int NBtot,
                      void* out, int ldo, int nb, int splitk, int waves, hipStream_t s) {
  const int mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  const int kbps = (KB128 + splitk - 1) / splitk;
#define LSA_Q4(MTV, NBV)                                                                                         \
  if (mt == MTV && nb == NBV) {                                                                                  \
    constexpr int U4 = (NBV >= 8 || MTV >= 4) ? 1 : 2;                                                           \
    constexpr int U8 = (MTV >= 4 || NBV >= 4) ? 1 : U4;                                                          \
    if constexpr (NBV < 8) {                                                                                     \
      if (waves == 8) {                                                                                          \
        launch_qx<MTV, NBV, EPI, 8, U8>(X, ldx, M, KB128, Wq, D, NBtot, out, ldo, kbps, splitk, s);              \
        return;                                                                                                  \
      }                                                                                                          \
    }                                                                                                            \
    launch_qx<MTV, NBV, EPI, 4, U4>(X, ldx, M, KB128, Wq, D, NBtot, out, ldo, kbps, splitk, s);                  \
    return;                                                                                                      \
  }
  LSA_Q4(1, 4) LSA_Q4(2, 4) LSA_Q4(1, 8) LSA_Q4(2, 8)
  if constexpr (EPI != EPI_SILU) { LSA_Q4(1, 1) LSA_Q4(2, 1) LSA_Q4(4, 1) }
  LSA_Q4(1, 2) LSA_Q4(2, 2) LSA_Q4(4, 2)
#undef LSA_Q4
}

extern "C" int lsa_q4_dequant(const void* Wq, const void* D, int N, int K, void* Wf, hipStream_t s) {
  if (K % 128 || N % 16 || N <= 0 || K <= 0) return -1;
  const int KB128 = K / 128;
  const long nfrag = (long)(N / 16) * KB128;
  const long gl = (nfrag * 64 + 255) / 256;
  hipLaunchKernelGGL(q4_dequant_kernel, dim3((unsigned)(gl < 8192 ? gl : 8192)), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(Wq), reinterpret_cast<const uint32_t*>(D), KB128, nfrag,
                     reinterpret_cast<uint4*>(Wf));
  return (int)hipGetLastError();
}

// M <= 64 decode GEMM.  xfrag = 1: X in the fragment-major decode layout (a SiLU output is written in it too);
// ep (nullable): decode epilogue extensions (common.h LsaEpi).  Argument checks and error codes: lsa_fp4_gemm_ex's.
extern "C" int lsa_q4_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const void* D, int N, void* out,
                              int epi, int nb, int splitk, int waves, int xfrag, const LsaEpi* ep, hipStream_t stream) {
  g_q4_epi = ep ? *ep : LsaEpi{};
  if ((ep || epi == EPI_RES) && (M > 64 || (splitk > 1 && epi != EPI_F32 && epi != EPI_RES))) return -7;
  if (epi == EPI_RES && (!ep || !ep->h || !ep->xout || !ep->ss_out || ep->ldh != N || (splitk > 1 && !ep->tickets)))
    return -8;
  if (K <= 0 || N <= 0 || K % 128 != 0 || N % 16 != 0 || M <= 0 || M > 64) return -1;
  g_q4_xfrag = xfrag ? 1 : 0;
  const int KB128 = K / 128, NBtot = N / 16;
  const int ldo = (epi == EPI_SILU) ? N / 2 : N;
  // the nb that will run: 2 above 32 rows and for any nb without an instantiation; the grid check is made on it
  if (!(nb == 1 || nb == 2 || nb == 4 || nb == 8) || (M > 32 && nb > 2)) nb = 2;
  if (epi == EPI_SILU && nb < 2) nb = 2;
  if (!skinny_grid_ok(NBtot, nb, epi == EPI_SILU)) return -2;
  if (splitk < 1) splitk = 1;
  if (epi != EPI_F32 && epi != EPI_RES && splitk != 1) return -3;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
  const uint4* w = reinterpret_cast<const uint4*>(Wq);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(D);
  switch (epi) {
    case EPI_BF16: launch_qe<EPI_BF16>(x, ldx, M, KB128, w, d, NBtot, out, ldo, nb, splitk, waves, stream); break;
    case EPI_F32: launch_qe<EPI_F32>(x, ldx, M, KB128, w, d, NBtot, out, ldo, nb, splitk, waves, stream); break;
    case EPI_SILU: launch_qe<EPI_SILU>(x, ldx, M, KB128, w, d, NBtot, out, ldo, nb, splitk, waves, stream); break;
    default: return -4;  // the residual epilogue is not instantiated: a q4_0 engine takes the norm-launch step
  }
  return (int)hipGetLastError();
}
