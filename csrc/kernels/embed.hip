// Embeddings (ops.embed_rowscale / embed_pool / embed_finish): pool the final-norm rows of a prefill on the device.
//
// A prefill holds the f32 residual stream h [T, D] of every prompt row (plus, in calls of at most 64 rows, the split-K
// slabs parts [np, T, D] of the last down projection that the final add_rmsnorm would sum).  The vector of an
// embedding request is y_t = (v_t * rs_t) * gamma, v_t = h_t (+ slab 0 + slab 1 ..., left to right as
// add_rmsnorm_kernel sums them), rs_t = rsqrt(sum(v_t^2) / D + eps), pooled over the input's tokens (their mean, or
// the last token's row alone) and divided by its Euclidean norm.  Per sequence i of the call, meta [5, n] int32:
//   emode[i]  0 none, 1 mean, 2 last        estart[i]  the segment's start_pos
//   eslot[i]  the request's slot            efinal[i]  1 when this call holds the input's last row
//   ecount[i] the input's total tokens
// and cu [n + 1] / tseq [T] are the prefill's own row offsets and row -> sequence map.
//
//   embed_rowscale_kernel  grid (T): rs[t] of every row that is pooled (all rows of a mean sequence, the last row of
//       an efinal last sequence).  Reads h and parts only.
//   embed_pool_kernel      grid (ceil(D / 256), n), one thread per column: a = estart == 0 ? +0 : acc[slot, c]; for
//       the sequence's rows of this call in position order a = a + y_t[c] (last: a = y of the last row of an efinal
//       segment, nothing otherwise); acc[slot, c] = a.  The sum is strictly left to right with every product and sum
//       rounded on its own, so it is the same bits however the prompt was chunked, and the host twin
//       (ops/reference.py embed_pool) reproduces them.  The loads of 8 rows are issued ahead of their 8 dependent adds.
//   embed_finish_kernel    grid (n), efinal sequences: m = acc / ecount (mean) or acc (last); ss = sum(m^2) in a fixed
//       order (thread i sums columns i, i + 256, ... in order; then a halving tree over the 256 partial sums);
//       out[slot] = m / sqrt(ss), zeros when ss == 0.
//
// Plain vector loads and stores only, no atomics, no scratch.  A thread of the pool kernel reads and writes its own
// acc word; the finish kernel reads acc and writes out; the host refuses two embedding sequences with one slot
// (ops._embed_check), so no workgroup reads a word that another workgroup of its launch writes.  A sequence with mode 0
// returns after the scalar load of its mode (a row: after its sequence index and that mode).  A sequence index, a slot
// or a row range outside its bounds is skipped, as kv_shift_kernel skips a bad move.
#include "common.h"

#pragma clang fp contract(off)

constexpr int EMB_THREADS = 256;

// A product as its own rounded f32 (kv_shift.hip kvs_rounded): opaque to the build's -ffp-contract=fast, which ignores
// the pragma above, so the sum that follows cannot become a v_fma.
__device__ __forceinline__ float emb_rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

__device__ __forceinline__ float emb_bf16(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

__global__ __launch_bounds__(EMB_THREADS) void embed_rowscale_kernel(const float* __restrict__ h,
                                                                     const float* __restrict__ parts, int nparts,
                                                                     size_t part_stride, const int* __restrict__ tseq,
                                                                     const int* __restrict__ cu,
                                                                     const int* __restrict__ meta, int n, int D,
                                                                     float eps, float* __restrict__ rs) {
  __shared__ float red[16];
  const int t = blockIdx.x, s = tseq[t];
  if ((unsigned)s >= (unsigned)n) return;
  const int mode = meta[s];
  if (mode == 0) return;
  if (mode != 1 && !(mode == 2 && meta[3 * n + s] != 0 && t == cu[s + 1] - 1)) return;
  const float4* hr = reinterpret_cast<const float4*>(h + (size_t)t * D);
  float ss = 0.f;
  for (int c4 = threadIdx.x; c4 < D / 4; c4 += EMB_THREADS) {
    float4 v = hr[c4];
    for (int p = 0; p < nparts; ++p) {
      const float4 q = *reinterpret_cast<const float4*>(parts + p * part_stride + (size_t)t * D + 4 * c4);
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    ss += v.x * v.x;
    ss += v.y * v.y;
    ss += v.z * v.z;
    ss += v.w * v.w;
  }
  const float tot = block_sum(ss, red);
  if (threadIdx.x == 0) rs[t] = rsqrtf(tot / (float)D + eps);
}

// v of (row t, column c): h + slab 0 + slab 1 + ...
#define EMB_ROWS 8

template <bool PARTS>
__global__ __launch_bounds__(EMB_THREADS) void embed_pool_kernel(const float* __restrict__ h,
                                                                 const float* __restrict__ parts, int nparts,
                                                                 size_t part_stride, const int* __restrict__ cu,
                                                                 const int* __restrict__ meta, int n, int T, int D,
                                                                 const float* __restrict__ rs,
                                                                 const uint16_t* __restrict__ gamma, float* acc,
                                                                 int nslots) {
  const int s = blockIdx.y;
  const int mode = meta[s];
  if (mode == 0) return;
  const int start = meta[n + s], slot = meta[2 * n + s], fin = meta[3 * n + s];
  int r0 = cu[s];
  const int r1 = cu[s + 1];
  if ((unsigned)slot >= (unsigned)nslots || r0 < 0 || r1 > T || r0 >= r1) return;
  if (mode == 2) {
    if (!fin) return;
    r0 = r1 - 1;
  } else if (mode != 1) {
    return;
  }
  const int c = blockIdx.x * EMB_THREADS + threadIdx.x;
  if (c >= D) return;
  const float g = emb_bf16(gamma[c]);
  float* pa = acc + (size_t)slot * D + c;
  const float* hc = h + c;
  const float* pc = parts + c;
  int t = r0;
  if (mode == 2) {  // the last row's y itself (not 0 + y: a -0 stays -0)
    float v = hc[(size_t)t * D];
    if constexpr (PARTS)
      for (int p = 0; p < nparts; ++p) v += pc[p * part_stride + (size_t)t * D];
    *pa = emb_rounded(emb_rounded(v * rs[t]) * g);
    return;
  }
  float a = start == 0 ? 0.f : *pa;
  for (; t + EMB_ROWS <= r1; t += EMB_ROWS) {
    float v[EMB_ROWS], sc[EMB_ROWS];
#pragma unroll
    for (int j = 0; j < EMB_ROWS; ++j) {
      v[j] = hc[(size_t)(t + j) * D];
      sc[j] = rs[t + j];
    }
    if constexpr (PARTS) {
      for (int p = 0; p < nparts; ++p) {
        float q[EMB_ROWS];
#pragma unroll
        for (int j = 0; j < EMB_ROWS; ++j) q[j] = pc[p * part_stride + (size_t)(t + j) * D];
#pragma unroll
        for (int j = 0; j < EMB_ROWS; ++j) v[j] += q[j];
      }
    }
#pragma unroll
    for (int j = 0; j < EMB_ROWS; ++j) a = a + emb_rounded(emb_rounded(v[j] * sc[j]) * g);
  }
  for (; t < r1; ++t) {
    float v = hc[(size_t)t * D];
    if constexpr (PARTS)
      for (int p = 0; p < nparts; ++p) v += pc[p * part_stride + (size_t)t * D];
    a = a + emb_rounded(emb_rounded(v * rs[t]) * g);
  }
  *pa = a;
}

__global__ __launch_bounds__(EMB_THREADS) void embed_finish_kernel(const int* __restrict__ meta, int n, int D,
                                                                   const float* __restrict__ acc,
                                                                   float* __restrict__ out, int nslots) {
  __shared__ float red[EMB_THREADS];
  const int s = blockIdx.x;
  const int mode = meta[s];
  if (mode == 0) return;
  const int slot = meta[2 * n + s], fin = meta[3 * n + s], count = meta[4 * n + s];
  if (!fin || (mode != 1 && mode != 2) || (unsigned)slot >= (unsigned)nslots || count <= 0) return;
  const float* pa = acc + (size_t)slot * D;
  float* po = out + (size_t)slot * D;
  const float cnt = (float)count;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += EMB_THREADS) {
    const float m = mode == 1 ? pa[c] / cnt : pa[c];
    ss = ss + emb_rounded(m * m);
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int w = EMB_THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
    __syncthreads();
  }
  const float tot = red[0];
  const float nrm = sqrtf(tot);
  for (int c = threadIdx.x; c < D; c += EMB_THREADS) {
    const float m = mode == 1 ? pa[c] / cnt : pa[c];
    po[c] = tot == 0.f ? 0.f : m / nrm;
  }
}

// h [T, D] f32; parts: nparts f32 slabs of [T, D], part_stride floats apart (nparts 0: none); tseq [T], cu [n + 1],
// meta [5, n] int32 on the device; rs [>= T] f32
extern "C" int lsa_embed_rowscale(const float* h, const float* parts, int nparts, long part_stride, const int* tseq,
                                  const int* cu, const int* meta, int n, int T, int D, float eps, float* rs,
                                  hipStream_t s) {
  if (T <= 0 || n <= 0) return 0;
  if (D <= 0 || D % 4 != 0 || nparts < 0 || (nparts > 0 && parts == nullptr) || h == nullptr || tseq == nullptr ||
      cu == nullptr || meta == nullptr || rs == nullptr)
    return -1;
  hipLaunchKernelGGL(embed_rowscale_kernel, dim3(T), dim3(EMB_THREADS), 0, s, h, parts, parts ? nparts : 0,
                     (size_t)part_stride, tseq, cu, meta, n, D, eps, rs);
  return (int)hipGetLastError();
}

// gamma: the final norm's bf16 weights [D]; acc [nslots, D] f32
extern "C" int lsa_embed_pool(const float* h, const float* parts, int nparts, long part_stride, const int* cu,
                              const int* meta, int n, int T, int D, const float* rs, const void* gamma, float* acc,
                              int nslots, hipStream_t s) {
  if (T <= 0 || n <= 0) return 0;
  if (D <= 0 || n > 65535 || nslots <= 0 || nparts < 0 || (nparts > 0 && parts == nullptr) || h == nullptr ||
      cu == nullptr || meta == nullptr || rs == nullptr || gamma == nullptr || acc == nullptr)
    return -1;
  const dim3 grid((D + EMB_THREADS - 1) / EMB_THREADS, n);
  const uint16_t* g = reinterpret_cast<const uint16_t*>(gamma);
  if (parts && nparts > 0)
    hipLaunchKernelGGL(embed_pool_kernel<true>, grid, dim3(EMB_THREADS), 0, s, h, parts, nparts, (size_t)part_stride,
                       cu, meta, n, T, D, rs, g, acc, nslots);
  else
    hipLaunchKernelGGL(embed_pool_kernel<false>, grid, dim3(EMB_THREADS), 0, s, h, parts, 0, (size_t)0, cu, meta, n, T,
                       D, rs, g, acc, nslots);
  return (int)hipGetLastError();
}

// acc, out [nslots, D] f32
extern "C" int lsa_embed_finish(const int* meta, int n, int D, const float* acc, float* out, int nslots,
                                hipStream_t s) {
  if (n <= 0) return 0;
  if (D <= 0 || nslots <= 0 || meta == nullptr || acc == nullptr || out == nullptr) return -1;
  hipLaunchKernelGGL(embed_finish_kernel, dim3(n), dim3(EMB_THREADS), 0, s, meta, n, D, acc, out, nslots);
  return (int)hipGetLastError();
}
