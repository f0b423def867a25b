// fp8 (OCP e4m3fn, gfx950-native) weight-only linear layers:  out = X[M,K] @ (Wq[N,K] * scale[n])^T
//
// Weight layout (ops.shuffle_weight_fp8): Wq[nb][kb64][lane][16 B], lane = 16*g + r holds
// W[16*nb + r][64*kb64 + 16*g + 0..15].  One 16 B load per lane = 1 KiB per wave-instruction feeds TWO
// mfma_f32_16x16x32_bf16 k-steps: step 0 uses k-slots 16g + 0..7, step 1 uses 16g + 8..15 (the k order
// inside an MFMA step only has to agree between A and B, so the activation fragment of lane (m, g) is
// simply x[m][64*kb64 + 16g .. +15] as two uint4).  fp8 -> bf16 with v_cvt_scalef32_pk_bf16_fp8
// (one VALU op per 2 weights, far below the HBM-bound budget), per-output-channel scale in the epilogue.
// Decode therefore streams half the bytes of the bf16 path.  For prefill (M > 64) the layer is
// dequantised (lsa_fp8_dequant) into a bf16 fragment-layout scratch buffer owned by the caller
// and run through the bf16 tile GEMM.  Work split, pipeline (clamped tail), reduction and epilogues: gemm_skinny.h,
// the epilogues with the per-channel scale policy.
#include "gemm_skinny.h"

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

template <bool HI>
__device__ __forceinline__ uint32_t cvt2(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, HI));
}
// 16 fp8 -> two bf16 fragments (k-slots 0..7 and 8..15)
__device__ __forceinline__ void fp8x16_to_bf16(const uint4 q, uint4& a, uint4& b) {
  a.x = cvt2<false>(q.x); a.y = cvt2<true>(q.x); a.z = cvt2<false>(q.y); a.w = cvt2<true>(q.y);
  b.x = cvt2<false>(q.z); b.y = cvt2<true>(q.z); b.z = cvt2<false>(q.w); b.w = cvt2<true>(q.w);
}

// XF: X in the fragment-major decode layout (common.h xf_off): lane (r, g)'s 16 activations
// k = 64 kb64 + 16 g .. +15 are the two 16-B pieces (g' = 2 (g & 1), g' + 1) of bf16 k-step 2 kb64 + g / 2
template <int MT, int NB, int EPI, int WAVES, int U, bool XF = false>
__global__ __launch_bounds__(64 * WAVES) void gemm_fp8_skinny_kernel(const uint16_t* __restrict__ X, int ldx, int M,
                                                                     int KB64, const uint4* __restrict__ Wq,
                                                                     const float* __restrict__ wscale,
                                                                     void* __restrict__ out, int ldo, int kb_per_split,
                                                                     LsaEpi ep) {
  // chunks of U k64-steps
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int nb0 = blockIdx.x * NB;  // exact grids only (the host rejects a ragged one)
  const SkinnySplit ks = skinny_split<U, WAVES>(KB64, kb_per_split, w);
  const int kbA = ks.kbA, kbB = ks.kbB;
  const int last_c = w + WAVES * (ks.n_it - 1);  // this wave's last chunk: the clamped pipeline's bound (gemm_skinny.h)

  f32x4_t acc[NB][MT];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const uint16_t* xp[MT];
  bool xvalid[MT];
  // row-major X: padding rows (>= M) read zeros from past the buffer range, no memory request (gemm.hip)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, XF ? 0 : M * ldx * 2, 0x00020000);
  uint32_t xoff[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = j * 16 + r;
    xvalid[j] = m < M;
    xp[j] = XF ? X + (((size_t)(g >> 1) * MT + j) * 64 + 32 * (g & 1) + r) * 8
               : X + (size_t)(xvalid[j] ? m : 0) * ldx + 16 * g;
    xoff[j] = xvalid[j] ? (uint32_t)(((size_t)m * ldx + 16 * g) * 2) : 0x80000000u;
  }
  const uint4* wp[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) wp[i] = Wq + (size_t)(nb0 + i) * KB64 * 64 + lane;

  struct Chunk {
    uint4 w[U][NB], x[U][MT][2];
  };
  auto load = [&](Chunk& ch, int c) {
    uint4(&wr)[U][NB] = ch.w;
    uint4(&xr)[U][MT][2] = ch.x;
    const int kb = kbA + c * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int i = 0; i < NB; ++i) wr[u][i] = ldg_nt(wp[i] + (size_t)kk * 64);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u, kbB - 1);
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        if constexpr (XF) {
          const uint4* px = reinterpret_cast<const uint4*>(xp[j] + (size_t)kk * 2 * MT * 512);
          xr[u][j][0] = px[0];
          xr[u][j][1] = px[16];
        } else {
          const uint32_t o = xoff[j] + (uint32_t)kk * 128u;
          const u32x4_t a = __builtin_amdgcn_raw_buffer_load_b128(xrs, o, 0, 0);
          const u32x4_t b = __builtin_amdgcn_raw_buffer_load_b128(xrs, o + 16u, 0, 0);
          xr[u][j][0] = make_uint4(a[0], a[1], a[2], a[3]);
          xr[u][j][1] = make_uint4(b[0], b[1], b[2], b[3]);
        }
      }
    }
  };
  auto comp = [&](const Chunk& ch, int c) {
    const uint4(&wr)[U][NB] = ch.w;
    const uint4(&xr)[U][MT][2] = ch.x;
    const int kb = kbA + c * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = (kb + u) < kbB;
      uint4 x0[MT], x1[MT];
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const bool ok = live && xvalid[j];
        x0[j] = xr[u][j][0];
        x1[j] = xr[u][j][1];
        x0[j].x = ok ? x0[j].x : 0u; x0[j].y = ok ? x0[j].y : 0u; x0[j].z = ok ? x0[j].z : 0u; x0[j].w = ok ? x0[j].w : 0u;
        x1[j].x = ok ? x1[j].x : 0u; x1[j].y = ok ? x1[j].y : 0u; x1[j].z = ok ? x1[j].z : 0u; x1[j].w = ok ? x1[j].w : 0u;
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        uint4 a0, a1;
        fp8x16_to_bf16(wr[u][i], a0, a1);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          acc[i][j] = mfma16x16x32(a0, x0[j], acc[i][j]);
          acc[i][j] = mfma16x16x32(a1, x1[j], acc[i][j]);
        }
      }
    }
  };
  if (ks.n_it > 0) {
    Chunk A, B;
    load(A, w);
    skinny_pipe_clamped<WAVES>(A, B, w, ks.n_it, last_c, load, comp);
  }
  skinny_epilogue<MT, NB, EPI, WAVES, XF, true>(acc, w, lane, M, nb0, NB, out, ldo, ep, wscale);
}

// fp8 [nb][kb64][lane][16] -> bf16 fragment layout [nb][kb32][lane][8] with the channel scale applied
__global__ __launch_bounds__(256) void fp8_dequant_kernel(const uint4* __restrict__ Wq, const float* __restrict__ wscale,
                                                          int KB64, long nfrag, uint4* __restrict__ Wf) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nfrag * 64; i += (long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const long f = i >> 6;  // (nb, kb64)
    const long nb = f / KB64;
    const int kb64 = (int)(f % KB64);
    const int r = lane & 15, g = lane >> 4;
    const float sc = wscale[nb * 16 + r];
    uint4 a0, a1;
    fp8x16_to_bf16(Wq[i], a0, a1);
    // elements k = 64*kb64 + 16g + e  (e = 0..15) -> bf16 fragment kb32 = 2*kb64 + (16g + e) / 32,
    // lane' = 16 * (((16g + e) % 32) / 8) + r
    float f0[8], f1[8];
    unpack8(a0, f0);
    unpack8(a1, f1);
#pragma unroll
    for (int j = 0; j < 8; ++j) { f0[j] *= sc; f1[j] *= sc; }
    const int k0 = 16 * g;  // e = 0..7 -> k0 .. k0+7 ; e = 8..15 -> k0+8 ..
    const long kb32 = 2 * kb64 + (k0 >> 5);
    const int lane0 = 16 * ((k0 & 31) >> 3) + r;
    const int lane1 = 16 * (((k0 + 8) & 31) >> 3) + r;
    Wf[((nb * (2L * KB64)) + kb32) * 64 + lane0] = pack8(f0);
    Wf[((nb * (2L * KB64)) + kb32) * 64 + lane1] = pack8(f1);
  }
}

static thread_local int g_fp8_xfrag = 0;
static thread_local LsaEpi g_fp8_epi = {};

// Per-call knobs (ops.pick_gemm_config, fp8 tuning entries): waves 4 | 8 per workgroup; depth 1 | 2
// multiplies the chunk of k64-steps each wave keeps in flight (U0 = 4 / NB fragments per chunk: the
// shallow point; depth 2 doubles the weight bytes in flight per wave for grids with few waves per CU).
static thread_local int g_fp8_waves = 4;
static thread_local int g_fp8_depth = 1;

template <int MT, int NB, int EPI, int WV, int U>
static void launch_tx(const uint16_t* X, int ldx, int M, int KB64, const uint4* Wq, const float* sc, int NBtot,
                      void* out, int ldo, int kbps, int splitk, hipStream_t s) {
  if (g_fp8_xfrag)
    hipLaunchKernelGGL((gemm_fp8_skinny_kernel<MT, NB, EPI, WV, U, true>), dim3(NBtot / NB, splitk), dim3(64 * WV), 0,
                       s, X, ldx, M, KB64, Wq, sc, out, ldo, kbps, g_fp8_epi);
  else
    hipLaunchKernelGGL((gemm_fp8_skinny_kernel<MT, NB, EPI, WV, U, false>), dim3(NBtot / NB, splitk), dim3(64 * WV), 0,
                       s, X, ldx, M, KB64, Wq, sc, out, ldo, kbps, g_fp8_epi);
}

template <int MT, int NB, int EPI>
static void launch_t(const uint16_t* X, int ldx, int M, int KB64, const uint4* Wq, const float* sc, int NBtot, void* out,
                     int ldo, int splitk, hipStream_t s) {
  // default: 4 waves, 4 fragments (NB * U) per chunk (the shallow-chunk / high-occupancy point that won the
  // bf16 sweeps: each fp8 fragment feeds twice the MFMA work of a bf16 one)
  constexpr int U = (4 / NB) < 1 ? 1 : (4 / NB);
  const int kbps = (KB64 + splitk - 1) / splitk;
  if constexpr (EPI == EPI_BF16 || NB >= 6) {
    // bf16 out: not on the decode hot path, one configuration.  Wide n-groups (NB 6 / 8: one pair of
    // activation fragments feeds 6-8 weight fragments, the activation traffic is 2 * MT / NB of the weight
    // bytes): 4 waves only (the reduction buffer is WAVES * NB * MT KiB), depth 1 | 2
    if (EPI != EPI_BF16 && g_fp8_depth == 2) launch_tx<MT, NB, EPI, 4, 2 * U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
    else launch_tx<MT, NB, EPI, 4, U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
  } else {
    if (g_fp8_waves == 8) {
      if (g_fp8_depth == 2) launch_tx<MT, NB, EPI, 8, 2 * U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
      else launch_tx<MT, NB, EPI, 8, U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
    } else {
      if (g_fp8_depth == 2) launch_tx<MT, NB, EPI, 4, 2 * U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
      else launch_tx<MT, NB, EPI, 4, U>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, kbps, splitk, s);
    }
  }
}

template <int EPI>
static void launch_e(const uint16_t* X, int ldx, int M, int KB64, const uint4* Wq, const float* sc, int NBtot, void* out,
                     int ldo, int nb, int splitk, hipStream_t s) {
  const int mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
#define LSA_F8(MTV, NBV)                                                       \
  if (mt == MTV && nb == NBV) {                                                \
    launch_t<MTV, NBV, EPI>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, splitk, s); \
    return;                                                                    \
  }
  LSA_F8(1, 2) LSA_F8(1, 4) LSA_F8(2, 2) LSA_F8(2, 4) LSA_F8(4, 2) LSA_F8(2, 6) LSA_F8(2, 8) LSA_F8(1, 8)
  if constexpr (EPI != EPI_SILU) { LSA_F8(1, 1) LSA_F8(2, 1) LSA_F8(4, 1) }
#undef LSA_F8
  // fallback (unsupported nb): nb = 2 at the same row-tile count
  if (mt == 1) launch_t<1, 2, EPI>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, splitk, s);
  else if (mt == 2) launch_t<2, 2, EPI>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, splitk, s);
  else launch_t<4, 2, EPI>(X, ldx, M, KB64, Wq, sc, NBtot, out, ldo, splitk, s);
}

extern "C" int lsa_fp8_dequant(const void* Wq, const float* wscale, int N, int K, void* Wf, hipStream_t s) {
  if (K % 64 || N % 16) return -1;
  const int KB64 = K / 64;
  const long nfrag = (long)(N / 16) * KB64;
  const long tot = nfrag * 64;
  const long gl = (tot + 255) / 256;
  hipLaunchKernelGGL(fp8_dequant_kernel, dim3((unsigned)(gl < 8192 ? gl : 8192)), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(Wq), wscale, KB64, nfrag, reinterpret_cast<uint4*>(Wf));
  return (int)hipGetLastError();
}

extern "C" int lsa_fp8_gemm_cfg(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N,
                                void* out, int epi, int nb, int splitk, int xfrag, hipStream_t stream);

extern "C" int lsa_fp8_gemm(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N, void* out,
                            int epi, int nb, int splitk, hipStream_t stream) {
  return lsa_fp8_gemm_cfg(X, ldx, M, K, Wq, wscale, N, out, epi, nb, splitk, 0, stream);
}

// xfrag = 1: X in the fragment-major decode layout (M <= 64); a SiLU output is written in it too
extern "C" int lsa_fp8_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N,
                               void* out, int epi, int nb, int splitk, int xfrag, const LsaEpi* ep, hipStream_t stream);

extern "C" void lsa_fp8_gemm_knobs(int waves, int depth) {
  g_fp8_waves = waves == 8 ? 8 : 4;
  g_fp8_depth = depth == 2 ? 2 : 1;
}

extern "C" int lsa_fp8_gemm_cfg(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N,
                                void* out, int epi, int nb, int splitk, int xfrag, hipStream_t stream) {
  return lsa_fp8_gemm_ex(X, ldx, M, K, Wq, wscale, N, out, epi, nb, splitk, xfrag, nullptr, stream);
}

// ep (nullable): decode epilogue extensions (common.h LsaEpi), M <= 64
extern "C" int lsa_fp8_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N,
                               void* out, int epi, int nb, int splitk, int xfrag, const LsaEpi* ep, hipStream_t stream) {
  g_fp8_epi = ep ? *ep : LsaEpi{};
  if ((ep || epi == EPI_RES) && (M > 64 || (splitk > 1 && epi != EPI_F32 && epi != EPI_RES))) return -7;
  if (epi == EPI_RES && (!ep || !ep->h || !ep->xout || !ep->ss_out || ep->ldh != N || (splitk > 1 && !ep->tickets)))
    return -8;
  if (K % 64 != 0 || N % 16 != 0 || M <= 0) return -1;
  if (xfrag && M > 64) return -5;
  g_fp8_xfrag = xfrag ? 1 : 0;
  const int KB64 = K / 64, NBtot = N / 16;
  const int ldo = (epi == EPI_SILU) ? N / 2 : N;
  if (M <= 64) {
    if (nb <= 0) nb = 1;
    if (epi == EPI_SILU && nb < 2) nb = 2;
    if (NBtot % nb != 0) return -2;
    if (splitk < 1) splitk = 1;
    if (epi != EPI_F32 && epi != EPI_RES && splitk != 1) return -3;
    if (M > 32 && nb > 2) nb = 2;
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const uint4* w = reinterpret_cast<const uint4*>(Wq);
    switch (epi) {
      case EPI_BF16: launch_e<EPI_BF16>(x, ldx, M, KB64, w, wscale, NBtot, out, ldo, nb, splitk, stream); break;
      case EPI_F32: launch_e<EPI_F32>(x, ldx, M, KB64, w, wscale, NBtot, out, ldo, nb, splitk, stream); break;
      case EPI_SILU: launch_e<EPI_SILU>(x, ldx, M, KB64, w, wscale, NBtot, out, ldo, nb, splitk, stream); break;
      case EPI_RES: launch_e<EPI_RES>(x, ldx, M, KB64, w, wscale, NBtot, out, ldo, nb, splitk, stream); break;
      default: return -4;
    }
    return (int)hipGetLastError();
  }
  return -6;  // M > 64: caller dequantises (lsa_fp8_dequant) and runs the bf16 tile GEMM
}
