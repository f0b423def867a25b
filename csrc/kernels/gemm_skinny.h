// The skeleton of the decode ("skinny", M <= 64) GEMM kernels: gemm_skinny (gemm.hip), gemm_z12 (gemm_z12.hip),
// gemm_fp8_skinny (gemm_fp8.hip), gemm_fp4_skinny (gemm_fp4.hip) and gemm_a8_skinny (gemm_fp8a.hip).  A kernel
// keeps its operand pointers, the contents of a pipeline chunk and the load / compute callables that fetch and
// decode one chunk; everything around that step is here, once: the work split, the chunk-depth rule, the two-deep
// register pipeline, the cross-wave reduction, the epilogues and, on the host, the grid check and the
// (waves, div) -> variant map.  gemm_a8_skinny takes the split, the reduction and the grid check from here and keeps
// its own pipeline loop (measured slower through the shared driver, gemm_fp8a.hip) and its own quantising epilogues.  gemm_z12's output is bit-identical to gemm_skinny's at equal (nb, split-K, waves,
// div) because both run this code.
//
// Work split: workgroup = WAVES waves over NB n-blocks (16 rows each; common.h skinny_nblocks) and one split-K
// range; the range is cut into chunks of U k-steps dealt round-robin to the waves.  Each wave streams its chunks
// with a two-deep register pipeline: chunk i+1's NB*U weight fragments (+ the activation fragments) are in flight
// while chunk i's MFMAs run, so the memory pipe never drains between chunks.  Out-of-range k-steps of a chunk are
// clamped by the kernel's load (duplicate L2 hits) and masked in its compute by zeroing the activation fragment
// (or the scale), never by a per-load branch (which would force vmcnt(0) per element).
#pragma once
#include <type_traits>

#include "common.h"

// Chunk depth of the 16-bit kernels: U k-steps per chunk, DIV 1|2|4 divides it (fewer VGPRs -> more resident
// waves).  The k-step -> (split, wave, order) assignment follows from it.
template <int MT, int NB, int DIV = 1>
struct SkinnyCfg {
  static constexpr int U0 = (16 / (NB > 2 * MT ? NB : 2 * MT)) < 2 ? 2 : (16 / (NB > 2 * MT ? NB : 2 * MT));
  static constexpr int U = (U0 / DIV) < 1 ? 1 : (U0 / DIV);
};

// This workgroup's split-K range [kbA, kbB) of the KB k-steps and wave w's share of its chunks: chunk c of the
// range is k-steps kbA + c U .. + U - 1, wave w owns chunks w, w + WAVES, ... (n_it of them, 0 for an idle
// wave).
struct SkinnySplit {
  int kbA, kbB, nk, nch, n_it;
};
template <int U, int WAVES>
__device__ __forceinline__ SkinnySplit skinny_split(int KB, int kb_per_split, int w) {
  SkinnySplit s;
  s.kbA = blockIdx.y * kb_per_split;
  s.kbB = min(KB, s.kbA + kb_per_split);
  s.nk = s.kbB - s.kbA;
  s.nch = (s.nk + U - 1) / U;                                     // chunks in this split
  s.n_it = s.nch > w ? (s.nch - w + WAVES - 1) / WAVES : 0;  // chunks of this wave
  return s;
}

// The two-deep pipeline over wave w's n_it chunks; load(chunk, c) requests chunk c into a register buffer,
// comp(chunk, c) consumes it.  Called with n_it > 0 and the wave's first chunk (w) already requested into A
// (so a prologue that does not depend on all of it can sit between its parts).  sched_barrier(0) pins the issue
// order: the next chunk's loads all leave before this chunk's MFMAs (hipcc otherwise interleaves them and keeps only
// ~8 loads in flight).
//
// Two forms.  Peeled (gemm_skinny, gemm_z12): the last iteration is peeled, so the steady-state loop always has a
// chunk i + 2 to request and the tail requests nothing it does not use (an even chunk count used to re-request its
// last chunk, weights and activations, and drop it: one load in eight of the o projection's at batch 32).  Clamped
// (gemm_fp8_skinny, gemm_fp4_skinny; gemm_a8_skinny's own loop has this form): the request after the last chunk is clamped to the wave's
// last chunk last_c = w + WAVES (n_it - 1) and dropped.  The kernel computes last_c beside its split and passes it
// in: computed here instead, it moves the compiler's register allocation, and some of these kernels sit at an
// occupancy or spill boundary.  Moving those kernels to the peeled tail changes which loads are issued: a performance
// change that needs its own A/B, so both forms stay.
template <int WAVES, class Chunk, class Load, class Comp>
__device__ __forceinline__ void skinny_pipe_peeled(Chunk& A, Chunk& B, int w, int n_it, Load&& load, Comp&& comp) {
  int i = 0;
  for (; i + 2 < n_it; i += 2) {
    load(B, w + WAVES * (i + 1));
    __builtin_amdgcn_sched_barrier(0);
    comp(A, w + WAVES * i);
    __builtin_amdgcn_sched_barrier(0);
    load(A, w + WAVES * (i + 2));
    __builtin_amdgcn_sched_barrier(0);
    comp(B, w + WAVES * (i + 1));
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i + 1 < n_it) {
    load(B, w + WAVES * (i + 1));
    __builtin_amdgcn_sched_barrier(0);
    comp(A, w + WAVES * i);
    __builtin_amdgcn_sched_barrier(0);
    comp(B, w + WAVES * (i + 1));
  } else {
    comp(A, w + WAVES * i);
  }
}

template <int WAVES, class Chunk, class Load, class Comp>
__device__ __forceinline__ void skinny_pipe_clamped(Chunk& A, Chunk& B, int w, int n_it, int last_c, Load&& load,
                                                    Comp&& comp) {
  int i = 0;
  for (; i + 1 < n_it; i += 2) {
    load(B, w + WAVES * (i + 1));
    __builtin_amdgcn_sched_barrier(0);
    comp(A, w + WAVES * i);
    __builtin_amdgcn_sched_barrier(0);
    load(A, min(w + WAVES * (i + 2), last_c));
    __builtin_amdgcn_sched_barrier(0);
    comp(B, w + WAVES * (i + 1));
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i < n_it) comp(A, w + WAVES * i);
}

// Cross-wave reduction through LDS: every wave stores its accumulators to red[w][tile i * MT + j][lane]; after the
// caller's __syncthreads() (it may initialise LDS of its own before it) tile_sum adds a tile's WAVES partials in
// wave order.  tile_sum2 sums two tiles with their LDS reads interleaved wave by wave (a SiLU epilogue's gate and up
// tile); written out and not built on tile_sum because the read order moves the register allocation of the kernels
// that spill.
template <int WAVES, int NB, int MT>
using SkinnyRed = f32x4_t[WAVES][NB * MT][64];

template <int WAVES, int NB, int MT>
__device__ __forceinline__ SkinnyRed<WAVES, NB, MT>& skinny_red_store(const f32x4_t (&acc)[NB][MT], int w, int lane) {
  __shared__ __attribute__((aligned(16))) f32x4_t red[WAVES][NB * MT][64];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) red[w][i * MT + j][lane] = acc[i][j];
  return red;
}

template <int WAVES, int NT>
__device__ __forceinline__ f32x4_t tile_sum(const f32x4_t (&red)[WAVES][NT][64], int t, int l) {
  f32x4_t s = red[0][t][l];
#pragma unroll
  for (int ww = 1; ww < WAVES; ++ww) s += red[ww][t][l];
  return s;
}
template <int WAVES, int NT>
__device__ __forceinline__ void tile_sum2(const f32x4_t (&red)[WAVES][NT][64], int t0, int t1, int l, f32x4_t& s0,
                                          f32x4_t& s1) {
  s0 = red[0][t0][l];
  s1 = red[0][t1][l];
#pragma unroll
  for (int ww = 1; ww < WAVES; ++ww) {
    s0 += red[ww][t0][l];
    s1 += red[ww][t1][l];
  }
}

// four consecutive columns n .. n + 3 of row m as bf16
__device__ __forceinline__ void skinny_store_bf16x4(void* out, size_t elem, f32x4_t v) {
  uint2 p;
  p.x = pack2bf(v[0], v[1]);
  p.y = pack2bf(v[2], v[3]);
  *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + elem) = p;
}

// The epilogues over the reduced tile (epilogue modes: common.h EPI_*): reduction, then
//   EPI_BF16 -> bf16 [M, N];  EPI_F32 -> f32 [splitk][M][N];
//   EPI_SILU -> bf16 [M, N/2] = silu(gate) * up, gate / up n-blocks interleaved, row-major or (XF: fragment-major
//               in -> fragment-major out, the down projection's input) in the layout of common.h xf_off;
//   EPI_RES  -> the residual epilogue (common.h epi_residual4); with split-K (grid.y > 1) every split publishes its
//               partial, takes a ticket, and the last arriver of the column sums the slabs and finishes it
//               (common.h res_publish_and_ticket).
// nb0 / cnt: the workgroup's n-blocks (tiles i >= cnt are never stored).  Every output row is scaled by the LsaEpi
// row scale and, RF, by the kernel's own row factor rowf (the residual-reduce prologue's RMS scale).  CS: a
// per-output-channel scale wscale[n] (gemm_fp8_skinny), applied before a split-K partial is published and, in SiLU,
// as gs * (sc * wscale[..]).  Without RF / CS no multiply by one is written: the floating-point operations and their
// association are exactly those listed here.
template <int MT, int NB, int EPI, int WAVES, bool XF, bool CS = false, bool RF = false>
__device__ __forceinline__ void skinny_epilogue(const f32x4_t (&acc)[NB][MT], int w, int lane, int M, int nb0, int cnt,
                                                void* out, int ldo, const LsaEpi& ep, const float* wscale = nullptr,
                                                float rowf = 1.f) {
  constexpr int NT = 64 * WAVES;
  auto& red = skinny_red_store<WAVES>(acc, w, lane);
  __shared__ unsigned long long ssw[16 * MT];  // EPI_RES: per-row sum of h^2 over this workgroup's columns (Q24)
  if constexpr (EPI == EPI_RES) {
    if (threadIdx.x < 16 * MT) ssw[threadIdx.x] = 0ull;
  }
  __syncthreads();
  auto row_scale = [&](int m) {
    if constexpr (RF) return epi_row_scale(ep, m) * rowf;
    else return epi_row_scale(ep, m);
  };

  if constexpr (EPI == EPI_SILU) {
    for (int idx = threadIdx.x; idx < (NB / 2) * MT * 64; idx += NT) {
      const int l = idx & 63, t = idx >> 6;
      const int j = t % MT, p = t / MT;
      f32x4_t gs, us;
      tile_sum2(red, (2 * p) * MT + j, (2 * p + 1) * MT + j, l, gs, us);
      const int m = j * 16 + (l & 15);
      if (m < M && 2 * p < cnt) {
        const int n = ((nb0 + 2 * p) >> 1) * 16 + 4 * (l >> 4);
        const float sc = row_scale(m);
        f32x4_t v;
        if constexpr (CS) {
          const float* cg = wscale + (nb0 + 2 * p) * 16 + 4 * (l >> 4);  // gate rows; the up rows are the next block
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = silu(gs[q] * (sc * cg[q])) * (us[q] * (sc * cg[16 + q]));
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = silu(gs[q] * sc) * (us[q] * sc);
        }
        skinny_store_bf16x4(out, XF ? xf_off(m, n, MT) : (size_t)m * ldo + n, v);
      }
    }
  } else {
    const size_t slab = (size_t)blockIdx.y * M * ldo;
    if constexpr (EPI == EPI_RES) {
      if (gridDim.y > 1) {  // split-K: publish, ticket, the last split finishes the column
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, 0x7fffffff, 0x00020000);
        for (int idx = threadIdx.x; idx < NB * MT * 64; idx += NT) {
          const int l = idx & 63, t = idx >> 6;
          const int j = t % MT, i = t / MT;
          f32x4_t s = tile_sum(red, t, l);
          const int m = j * 16 + (l & 15);
          if (m < M && i < cnt) {
            if constexpr (CS) {
              const float4 sc = *reinterpret_cast<const float4*>(wscale + (nb0 + i) * 16 + 4 * (l >> 4));
              s[0] *= sc.x; s[1] *= sc.y; s[2] *= sc.z; s[3] *= sc.w;
            }
            res_store_partial(rs, slab + (size_t)m * ldo + (nb0 + i) * 16 + 4 * (l >> 4), s);
          }
        }
        __shared__ int s_last;
        if (!res_publish_and_ticket<NT>(ep, &s_last)) return;
        for (int idx = threadIdx.x; idx < NB * MT * 64; idx += NT) {
          const int l = idx & 63, t = idx >> 6;
          const int j = t % MT, i = t / MT;
          const int m = j * 16 + (l & 15);
          if (m < M && i < cnt) {
            const int n = (nb0 + i) * 16 + 4 * (l >> 4);
            atomicAdd(&ssw[m], (unsigned long long)ss_to_q24(
                epi_residual4(ep, m, n, res_slab_sum(rs, (size_t)m * ldo + n, (size_t)M * ldo, gridDim.y) *
                                        epi_row_scale(ep, m))));
          }
        }
        __syncthreads();
        if (threadIdx.x < M) atomicAdd(reinterpret_cast<unsigned long long*>(ep.ss_out) + threadIdx.x, ssw[threadIdx.x]);
        return;
      }
    }
    for (int idx = threadIdx.x; idx < NB * MT * 64; idx += NT) {
      const int l = idx & 63, t = idx >> 6;
      const int j = t % MT, i = t / MT;
      f32x4_t s = tile_sum(red, t, l);
      const int m = j * 16 + (l & 15);
      if (m < M && i < cnt) {
        const int n = (nb0 + i) * 16 + 4 * (l >> 4);
        if constexpr (CS) {
          const float4 sc = *reinterpret_cast<const float4*>(wscale + n);
          const float rs = row_scale(m);
          s[0] *= sc.x * rs; s[1] *= sc.y * rs; s[2] *= sc.z * rs; s[3] *= sc.w * rs;
        } else {
          s *= row_scale(m);
        }
        if constexpr (EPI == EPI_RES) {
          atomicAdd(&ssw[m], (unsigned long long)ss_to_q24(epi_residual4(ep, m, n, s)));
        } else if constexpr (EPI == EPI_F32) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + slab + (size_t)m * ldo + n) =
              make_float4(s[0], s[1], s[2], s[3]);
        } else {
          skinny_store_bf16x4(out, (size_t)m * ldo + n, s);
        }
      }
    }
    if constexpr (EPI == EPI_RES) {
      __syncthreads();
      if (threadIdx.x < M) atomicAdd(reinterpret_cast<unsigned long long*>(ep.ss_out) + threadIdx.x, ssw[threadIdx.x]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// A grid of ceil(NBtot / nb) workgroups over NBtot n-blocks: exact when nb divides NBtot, else ragged (the kernel
// deals the blocks, common.h skinny_nblocks), which needs >= 1 column unit per workgroup; SiLU units are pairs.
static inline bool skinny_grid_ok(int NBtot, int nb, bool silu) {
  if (NBtot % nb == 0) return true;
  const int wgs = (NBtot + nb - 1) / nb;
  return silu ? !(nb % 2 || NBtot % 2 || NBtot / 2 < wgs) : NBtot >= wgs;
}

// The (waves 4|8, div 1|2|4) -> <WAVES, DIV> variants of the 16-bit kernels: f(WAVES, DIV) is called with two
// std::integral_constant.  Wide n-groups (NB >= 6: one activation fragment feeds NB weight fragments) run 4 waves
// only (the cross-wave reduction buffer is WAVES * NB * MT KiB) at div 1|2; div 4 has a 4-wave variant only.
template <int NB, class F>
static inline void skinny_variant(int waves, int div, F&& f) {
  using W4 = std::integral_constant<int, 4>;
  using W8 = std::integral_constant<int, 8>;
  using D1 = std::integral_constant<int, 1>;
  using D2 = std::integral_constant<int, 2>;
  using D4 = std::integral_constant<int, 4>;
  if constexpr (NB >= 6) {
    if (div == 1) f(W4{}, D1{});
    else f(W4{}, D2{});
  } else if (div == 2) {
    if (waves == 8) f(W8{}, D2{});
    else f(W4{}, D2{});
  } else if (div == 4) {
    f(W4{}, D4{});
  } else {
    if (waves == 8) f(W8{}, D1{});
    else f(W4{}, D1{});
  }
}
