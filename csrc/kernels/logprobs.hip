// Per-token log-probabilities of the model's own distribution: log-softmax over the whole vocabulary of the logits as
// the lm_head wrote them (before the regex mask, the penalties and temperature / top-k / top-p / min-p), recorded on
// the device next to the commit.  Two launches, no workgroup reads a word another workgroup of its launch wrote:
//
//   lsa_logprob_scan    grid (ceil(V / 2048), B), after the lm_head and ahead of dfa_mask / the penalties.  A row that
//                       did not ask (lp_k[b] < 0) or is finished returns at once (a finished row that asked: lp_n0[b]
//                       = -1, no record this step).  Otherwise workgroup (c, b) reads its
//                       chunk of the row ONCE into registers and writes the chunk's (m_c, s_c = sum exp(l - m_c)), its
//                       best min(32, chunk length) packed keys (pack_key order: value descending, index ascending; 0 =
//                       none) and the chunk itself into lp_raw[b] (the mask and the penalties overwrite `logits` in
//                       place before the token is known); workgroup 0 of the row stores n0 = gen_len[b] into lp_n0[b].
//   lsa_logprob_commit  grid (B), after argmax_commit / sample_commit.  A row records exactly when it asked, lp_n0[b]
//                       was written by this step's scan and gen_len[b] == n0 + 1 (the commit appended one token; a row
//                       that finishes in this very step still records it); lp_n0[b] is consumed (-1), so a row
//                       finished earlier never records again.  M = max m_c, S = sum_c s_c exp(m_c - M) in chunk order,
//                       lse = M + log S: the result depends on the row and V alone and repeats bitwise.  lp_tok[b, n0]
//                       = lp_raw[b, tok] - lse for tok = out_tokens[b, n0]; for K = lp_k[b] > 0 the K best of the
//                       chunk candidates by K rounds of a block-wide max with the winner knocked out (never a sort of
//                       all 4096), lp_ids[b, n0, j] and lp_top[b, n0, j] = l_j - lse -- the expression of the chosen
//                       token, so the two are bitwise equal when it is among them.  j >= V: id -1, -inf.  Nothing is
//                       written at n0 >= max_new.
// Plain vector stores only.  ops/reference.py logprob_scan / logprob_commit are the host twins.
#include "common.h"

#define LP_CHUNK 2048
#define LP_CAND 32
#define LP_KMAX 20
#define LP_MAXCH 128  // V <= 262144: at most 4096 candidates per row

__device__ __forceinline__ unsigned long long lp_pack_key(float v, int idx) {  // sampling.hip pack_key
  return ((unsigned long long)float_key(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)idx);
}

// block-wide max of a packed key over 4 waves; red: 4 words the caller does not reuse before its next barrier
__device__ __forceinline__ unsigned long long lp_block_max_u64(unsigned long long v, unsigned long long* red) {
  v = wave_max_u64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return lsa_umax64(lsa_umax64(red[0], red[1]), lsa_umax64(red[2], red[3]));
}

__global__ __launch_bounds__(256) void logprob_scan_kernel(const float* __restrict__ logits, int V, int vec,
                                                           const int* __restrict__ lp_k,
                                                           const int* __restrict__ finished,
                                                           const int* __restrict__ gen_len, float* __restrict__ lp_raw,
                                                           float* __restrict__ lp_ms,
                                                           unsigned long long* __restrict__ lp_cand,
                                                           int* __restrict__ lp_n0, int nch) {
  const int c = blockIdx.x, b = blockIdx.y;
  if (lp_k[b] < 0) return;
  const int t = threadIdx.x;
  if (finished[b]) {  // no record this step, whatever an earlier step left in lp_n0
    if (c == 0 && t == 0) lp_n0[b] = -1;
    return;
  }
  const float* row = logits + (size_t)b * V;
  float* raw = lp_raw + (size_t)b * V;
  const int lo = c * LP_CHUNK;
  // element j of this thread: lo + 1024 * (j / 4) + 4 * t + j % 4 (two 16-byte accesses per thread when rows are aligned)
  float v[8];
  int idx[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i0 = lo + 1024 * h + 4 * t;
    if (vec && i0 + 4 <= V) {
      const float4 x = *reinterpret_cast<const float4*>(row + i0);
      *reinterpret_cast<float4*>(raw + i0) = x;
      v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < V;
        const float x = in ? row[i0 + j] : 0.f;
        if (in) raw[i0 + j] = x;
        v[4 * h + j] = x;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[4 * h + j] = i0 + j;
  }
  __shared__ float fred[8];
  __shared__ unsigned long long kred[2][4];
  // chunk max, then the sum of exp(l - m_c) from the registers: the row is read once
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = idx[j] < V ? fmaxf(m, v[j]) : m;
  m = wave_max(m);
  if ((t & 63) == 0) fred[t >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(fred[0], fred[1]), fmaxf(fred[2], fred[3]));
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += idx[j] < V ? expf(v[j] - m) : 0.f;
  s = wave_sum(s);
  if ((t & 63) == 0) fred[4 + (t >> 6)] = s;
  __syncthreads();
  if (t == 0) {
    float* ms = lp_ms + ((size_t)b * nch + c) * 2;
    ms[0] = m;
    ms[1] = (fred[4] + fred[5]) + (fred[6] + fred[7]);
    if (c == 0) lp_n0[b] = gen_len[b];
  }
  // the chunk's best LP_CAND keys: LP_CAND rounds of a block-wide max, the winner knocked out of its owner's registers
  unsigned long long key[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) key[j] = idx[j] < V ? lp_pack_key(v[j], idx[j]) : 0ull;
  unsigned long long* out = lp_cand + ((size_t)b * nch + c) * LP_CAND;
  for (int r = 0; r < LP_CAND; ++r) {
    unsigned long long best = key[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) best = lsa_umax64(best, key[j]);
    best = lp_block_max_u64(best, kred[r & 1]);  // (two buffers: round r + 1 writes while a slow wave still reads r)
    if (t == 0) out[r] = best;
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = key[j] == best ? 0ull : key[j];
  }
}

__global__ __launch_bounds__(256) void logprob_commit_kernel(const float* __restrict__ lp_raw, int V,
                                                             const float* __restrict__ lp_ms,
                                                             const unsigned long long* __restrict__ lp_cand, int nch,
                                                             const int* __restrict__ lp_k, int* __restrict__ lp_n0,
                                                             const int* __restrict__ gen_len,
                                                             const int* __restrict__ out_tokens, int max_new,
                                                             float* __restrict__ lp_tok, int* __restrict__ lp_ids,
                                                             float* __restrict__ lp_top, int kcap) {
  const int b = blockIdx.x, t = threadIdx.x;
  int K = lp_k[b];
  if (K < 0) return;
  const int n0 = lp_n0[b];
  if (n0 < 0) return;  // no scan of this step: the row was finished before it
  __syncthreads();     // every thread has read lp_n0[b] before it is consumed
  if (t == 0) lp_n0[b] = -1;
  if (gen_len[b] != n0 + 1 || n0 >= max_new) return;
  K = min(K, kcap);
  __shared__ float term[LP_MAXCH];
  __shared__ float fred[4];
  __shared__ unsigned long long kred[2][4];
  __shared__ unsigned long long win[LP_KMAX];
  const float* ms = lp_ms + (size_t)b * nch * 2;
  // lse: M = max m_c (order-free), S = sum s_c exp(m_c - M) serially in chunk order
  float m = -INFINITY;
  for (int c = t; c < nch; c += 256) m = fmaxf(m, ms[2 * c]);
  m = wave_max(m);
  if ((t & 63) == 0) fred[t >> 6] = m;
  __syncthreads();
  const float M = fmaxf(fmaxf(fred[0], fred[1]), fmaxf(fred[2], fred[3]));
  for (int c = t; c < nch; c += 256) term[c] = ms[2 * c + 1] * expf(ms[2 * c] - M);
  __syncthreads();
  float S = 0.f;
  for (int c = 0; c < nch; ++c) S += term[c];
  const float lse = M + logf(S);
  if (t == 0) {
    const int tok = out_tokens[(size_t)b * max_new + n0];
    lp_tok[(size_t)b * max_new + n0] = (tok >= 0 && tok < V) ? lp_raw[(size_t)b * V + tok] - lse : -INFINITY;
  }
  if (K <= 0) return;
  // the K best of the nch * LP_CAND candidates (<= 16 per thread, in registers)
  const int ncand = nch * LP_CAND;
  const unsigned long long* cand = lp_cand + (size_t)b * ncand;
  unsigned long long key[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) key[j] = (t + 256 * j) < ncand ? cand[t + 256 * j] : 0ull;
  for (int r = 0; r < K; ++r) {
    unsigned long long best = key[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) best = lsa_umax64(best, key[j]);
    best = lp_block_max_u64(best, kred[r & 1]);
    if (t == 0) win[r] = best;
#pragma unroll
    for (int j = 0; j < 16; ++j) key[j] = key[j] == best ? 0ull : key[j];
  }
  __syncthreads();
  if (t < K) {
    const unsigned long long w = win[t];
    const size_t o = ((size_t)b * max_new + n0) * kcap + t;
    lp_ids[o] = w ? (int)(0xffffffffu - (uint32_t)(w & 0xffffffffull)) : -1;
    lp_top[o] = w ? key_float((uint32_t)(w >> 32)) - lse : -INFINITY;
  }
}

// workspace: lp_ms (B * ceil(V / 2048) * 2 f32) + lp_cand (B * ceil(V / 2048) * 32 u64).  Refused before any launch:
// B < 1, V < 1 or V > 262144 (4096 candidates: lsa_sample_commit's bound).
extern "C" int lsa_logprob_scan(const float* logits, int B, int V, const int* lp_k, const int* finished,
                                const int* gen_len, float* lp_raw, float* lp_ms, unsigned long long* lp_cand, int* lp_n0,
                                hipStream_t s) {
  if (B < 1 || V < 1 || V > LP_MAXCH * LP_CHUNK) return -1;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  const int vec = (V % 4 == 0) && (((uintptr_t)logits | (uintptr_t)lp_raw) % 16 == 0);
  hipLaunchKernelGGL(logprob_scan_kernel, dim3(nch, B), dim3(256), 0, s, logits, V, vec, lp_k, finished, gen_len, lp_raw,
                     lp_ms, lp_cand, lp_n0, nch);
  return (int)hipGetLastError();
}

// kcap: the record width of lp_ids / lp_top [B, max_new, kcap], 0 .. 20 (-2 otherwise)
extern "C" int lsa_logprob_commit(const float* lp_raw, int B, int V, const float* lp_ms,
                                  const unsigned long long* lp_cand, const int* lp_k, int* lp_n0, const int* gen_len,
                                  const int* out_tokens, int max_new, float* lp_tok, int* lp_ids, float* lp_top, int kcap,
                                  hipStream_t s) {
  if (B < 1 || V < 1 || V > LP_MAXCH * LP_CHUNK || max_new < 1) return -1;
  if (kcap < 0 || kcap > LP_KMAX) return -2;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  hipLaunchKernelGGL(logprob_commit_kernel, dim3(B), dim3(256), 0, s, lp_raw, V, lp_ms, lp_cand, nch, lp_k, lp_n0,
                     gen_len, out_tokens, max_new, lp_tok, lp_ids, lp_top, kcap);
  return (int)hipGetLastError();
}
