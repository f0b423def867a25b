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
//
// The verify step of speculative decoding (S sequences of T rows, S * T <= 32; ``spec_logprobs``) runs the same two
// bodies (lp_scan_chunk, lp_commit_row: one expression per value, so a verify row records bit for bit what the plain
// pair records for the same row values and token) over its own 32-row raw buffer and chunk workspace:
//
//   lsa_spec_logprob_scan    grid (ceil(V / 2048), T, S), after the verify lm_head and ahead of dfa_mask_verify and the
//                            verify commit.  Sequence s = blockIdx.z, row r = s T + blockIdx.y.  lp_k[s] < 0: return;
//                            finished[s]: workgroup (0, 0, s) stores lp_n0[s] = -1, all return; else the plain scan of
//                            row r into the spec-side buffers, and workgroup (0, 0, s) stores lp_n0[s] = gen_len[s].
//   lsa_spec_logprob_commit  grid (T, S), after spec_commit / spec_sample_commit and dfa_spec_advance.  Workgroup
//                            (t, s): K = lp_k[s], n0 = lp_n0[s], c = gen_len[s] - n0 (the tokens this step committed
//                            into s, 0 .. T, already cut by EOS / limit).  It records exactly when K >= 0, n0 >= 0,
//                            t < c and n0 + t < max_new: index n0 + t from row s T + t and out_tokens[s, n0 + t] (row
//                            t is the distribution of generated token n0 + t), straight into the per-slot records.
//
// Prompt-token logprobs (teacher-forced scoring in the prefill): the target token of every scored row is known before
// the lm_head runs and nothing overwrites the rows, so the pair below runs the same two bodies without what a decode
// step needs only because its token comes later: no raw-row copy, and no candidate rounds when no row asked for K > 0.
//
//   lsa_prompt_logprob_scan    grid (ceil(V / 2048), R) over logits [R, V] (read only), targets [R], row_k [R].  A row
//                              with targets[r] < 0 returns after one scalar load.  Otherwise workgroup (c, r) writes
//                              the chunk's (m_c, s_c) by lp_scan_chunk's very expressions, and the chunk's best 32
//                              keys only in the launch form that was told some row has K > 0 (a template argument,
//                              not a per-lane branch).
//   lsa_prompt_logprob_commit  grid (R).  A row with a target runs lp_commit_row(raw = the logits row itself, tok =
//                              targets[r], K = min(row_k[r], kcap)) into dst_tok [R], dst_ids / dst_top [R, kcap]; rows
//                              without a target write nothing.  ``logits`` must stay intact between the two launches.
//
// A prompt record is therefore one expression with a generated-token record: for equal row values and token the two
// are bitwise equal, chosen value and top-K alike.
//
// Invariant: the verify commit does NOT consume lp_n0[s] -- T workgroups read it, and no workgroup reads a word another
// workgroup of its launch writes.  It need not: every step in which a row asks rewrites lp_n0 in its scan (n0, or -1
// for a finished row), the verify scan and the plain scan alike.  The plain commit's own consume is unaffected.
// Plain vector stores only.  ops/reference.py logprob_scan / logprob_commit / spec_logprob_scan / spec_logprob_commit
// are the host twins.
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

// One chunk of one raw row, the body of every scan kernel: chunk c of ``row`` (V words) is read ONCE into registers and
// (COPY) copied into ``raw``; (m_c, s_c) goes to ms[0 .. 1] and (CAND) the chunk's best LP_CAND packed keys to
// out[0 .. 31].  The one workgroup that announces the record index gets n0_dst (else nullptr): *n0_dst = *n0_src, the
// gen_len before the commit.  COPY / CAND are compile-time: the decode and verify scans take both, the prompt scan
// neither (K = 0 everywhere) or the candidates alone; the expressions of m_c, s_c and the keys are the same in all.
template <bool COPY, bool CAND>
__device__ __forceinline__ void lp_scan_chunk(const float* __restrict__ row, float* __restrict__ raw, int V, int vec,
                                              int c, float* __restrict__ ms, unsigned long long* __restrict__ out,
                                              int* __restrict__ n0_dst, const int* __restrict__ n0_src) {
  const int t = threadIdx.x;
  const int lo = c * LP_CHUNK;
  // element j of this thread: lo + 1024 * (j / 4) + 4 * t + j % 4 (two 16-byte accesses per thread when rows are aligned)
  float v[8];
  int idx[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i0 = lo + 1024 * h + 4 * t;
    if (vec && i0 + 4 <= V) {
      const float4 x = *reinterpret_cast<const float4*>(row + i0);
      if (COPY) *reinterpret_cast<float4*>(raw + i0) = x;
      v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < V;
        const float x = in ? row[i0 + j] : 0.f;
        if (COPY && in) raw[i0 + j] = x;
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
    ms[0] = m;
    ms[1] = (fred[4] + fred[5]) + (fred[6] + fred[7]);
    if (n0_dst != nullptr) *n0_dst = *n0_src;
  }
  if (!CAND) return;
  // the chunk's best LP_CAND keys: LP_CAND rounds of a block-wide max, the winner knocked out of its owner's registers
  unsigned long long key[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) key[j] = idx[j] < V ? lp_pack_key(v[j], idx[j]) : 0ull;
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

__global__ __launch_bounds__(256) void logprob_scan_kernel(const float* __restrict__ logits, int V, int vec,
                                                           const int* __restrict__ lp_k,
                                                           const int* __restrict__ finished,
                                                           const int* __restrict__ gen_len, float* __restrict__ lp_raw,
                                                           float* __restrict__ lp_ms,
                                                           unsigned long long* __restrict__ lp_cand,
                                                           int* __restrict__ lp_n0, int nch) {
  const int c = blockIdx.x, b = blockIdx.y;
  if (lp_k[b] < 0) return;
  if (finished[b]) {  // no record this step, whatever an earlier step left in lp_n0
    if (c == 0 && threadIdx.x == 0) lp_n0[b] = -1;
    return;
  }
  lp_scan_chunk<true, true>(logits + (size_t)b * V, lp_raw + (size_t)b * V, V, vec, c,
                            lp_ms + ((size_t)b * nch + c) * 2, lp_cand + ((size_t)b * nch + c) * LP_CAND,
                            c == 0 ? lp_n0 + b : nullptr, gen_len + b);
}

// The verify-step scan: sequence s = blockIdx.z, verify row r = s * T + blockIdx.y of logits [S * T, V]; the raw rows and
// the chunk partials go into the spec-side buffers of 32 rows (sp_raw [32, V], sp_ms, sp_cand), indexed by r.
__global__ __launch_bounds__(256) void spec_logprob_scan_kernel(const float* __restrict__ logits, int V, int vec, int T,
                                                                const int* __restrict__ lp_k,
                                                                const int* __restrict__ finished,
                                                                const int* __restrict__ gen_len,
                                                                float* __restrict__ sp_raw, float* __restrict__ sp_ms,
                                                                unsigned long long* __restrict__ sp_cand,
                                                                int* __restrict__ lp_n0, int nch) {
  const int c = blockIdx.x, s = blockIdx.z;
  if (lp_k[s] < 0) return;
  if (finished[s]) {
    if (c == 0 && blockIdx.y == 0 && threadIdx.x == 0) lp_n0[s] = -1;
    return;
  }
  const int r = s * T + blockIdx.y;
  // workgroup (0, 0, s) alone announces n0 = gen_len[s]: one writer per word
  lp_scan_chunk<true, true>(logits + (size_t)r * V, sp_raw + (size_t)r * V, V, vec, c,
                            sp_ms + ((size_t)r * nch + c) * 2, sp_cand + ((size_t)r * nch + c) * LP_CAND,
                            (c == 0 && blockIdx.y == 0) ? lp_n0 + s : nullptr, gen_len + s);
}

// One record, the body of both commit kernels: from a row's chunk partials ``ms`` / ``cand`` (nch chunks) and its raw copy
// ``raw``, *tok_dst = raw[tok] - lse and, for K > 0, the K best into ids_dst / top_dst[0 .. K - 1].
__device__ __forceinline__ void lp_commit_row(const float* __restrict__ raw, int V, const float* __restrict__ ms,
                                              const unsigned long long* __restrict__ cand, int nch, int K, int tok,
                                              float* __restrict__ tok_dst, int* __restrict__ ids_dst,
                                              float* __restrict__ top_dst) {
  const int t = threadIdx.x;
  __shared__ float term[LP_MAXCH];
  __shared__ float fred[4];
  __shared__ unsigned long long kred[2][4];
  __shared__ unsigned long long win[LP_KMAX];
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
  if (t == 0) *tok_dst = (tok >= 0 && tok < V) ? raw[tok] - lse : -INFINITY;
  if (K <= 0) return;
  // the K best of the nch * LP_CAND candidates (<= 16 per thread, in registers)
  const int ncand = nch * LP_CAND;
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
    ids_dst[t] = w ? (int)(0xffffffffu - (uint32_t)(w & 0xffffffffull)) : -1;
    top_dst[t] = w ? key_float((uint32_t)(w >> 32)) - lse : -INFINITY;
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
  const size_t o = (size_t)b * max_new + n0;
  lp_commit_row(lp_raw + (size_t)b * V, V, lp_ms + (size_t)b * nch * 2, lp_cand + (size_t)b * nch * LP_CAND, nch, K,
                out_tokens[o], lp_tok + o, lp_ids + o * kcap, lp_top + o * kcap);
}

// The verify-step commit, after spec_commit / spec_sample_commit (and dfa_spec_advance): workgroup (t, s) records
// generated token n0 + t of sequence s from verify row s * T + t exactly when the sequence asked, this step's scan
// announced n0 = lp_n0[s] >= 0 and the step committed more than t tokens (c = gen_len[s] - n0, 0 .. T, already cut by EOS
// and the limit), at index n0 + t < max_new.  Row t is the distribution of generated token n0 + t: row 0 follows the
// input token, row t draft t.  lp_n0[s] is NOT consumed here: T workgroups read it, and no workgroup reads a word
// another workgroup of its launch writes.  It need not be: every step in which a row asks rewrites lp_n0 in its scan
// (n0, or -1 for a finished row), the verify scan and the plain scan alike, so a stale n0 is never read.
__global__ __launch_bounds__(256) void spec_logprob_commit_kernel(const float* __restrict__ sp_raw, int V, int T,
                                                                  const float* __restrict__ sp_ms,
                                                                  const unsigned long long* __restrict__ sp_cand,
                                                                  int nch, const int* __restrict__ lp_k,
                                                                  const int* __restrict__ lp_n0,
                                                                  const int* __restrict__ gen_len,
                                                                  const int* __restrict__ out_tokens, int max_new,
                                                                  float* __restrict__ lp_tok, int* __restrict__ lp_ids,
                                                                  float* __restrict__ lp_top, int kcap) {
  const int t = blockIdx.x, s = blockIdx.y;
  int K = lp_k[s];
  if (K < 0) return;
  const int n0 = lp_n0[s];
  if (n0 < 0) return;
  if (t >= gen_len[s] - n0 || n0 + t >= max_new) return;
  K = min(K, kcap);
  const int r = s * T + t;
  const size_t o = (size_t)s * max_new + n0 + t;
  lp_commit_row(sp_raw + (size_t)r * V, V, sp_ms + (size_t)r * nch * 2, sp_cand + (size_t)r * nch * LP_CAND, nch, K,
                out_tokens[o], lp_tok + o, lp_ids + o * kcap, lp_top + o * kcap);
}

// The prompt pair: R scored prefill rows, each with its target token (< 0: the row records nothing) and its K.  CAND:
// the launch was told that some row has K > 0.  Nothing but ms / cand is written by the scan: ``logits`` is the raw row
// the commit reads.
template <bool CAND>
__global__ __launch_bounds__(256) void prompt_logprob_scan_kernel(const float* __restrict__ logits, int V, int vec,
                                                                  const int* __restrict__ targets,
                                                                  float* __restrict__ ms,
                                                                  unsigned long long* __restrict__ cand, int nch) {
  const int c = blockIdx.x, r = blockIdx.y;
  if (targets[r] < 0) return;
  lp_scan_chunk<false, CAND>(logits + (size_t)r * V, nullptr, V, vec, c, ms + ((size_t)r * nch + c) * 2,
                             cand + ((size_t)r * nch + c) * LP_CAND, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void prompt_logprob_commit_kernel(const float* __restrict__ logits, int V,
                                                                    const float* __restrict__ ms,
                                                                    const unsigned long long* __restrict__ cand,
                                                                    int nch, const int* __restrict__ targets,
                                                                    const int* __restrict__ row_k,
                                                                    float* __restrict__ dst_tok,
                                                                    int* __restrict__ dst_ids,
                                                                    float* __restrict__ dst_top, int kcap) {
  const int r = blockIdx.x;
  const int tok = targets[r];
  if (tok < 0) return;
  const int K = min(row_k[r], kcap);
  lp_commit_row(logits + (size_t)r * V, V, ms + (size_t)r * nch * 2, cand + (size_t)r * nch * LP_CAND, nch, K, tok,
                dst_tok + r, dst_ids + (size_t)r * kcap, dst_top + (size_t)r * kcap);
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

// The verify-step pair.  sp_raw f32 [32, V], sp_ms (32 * ceil(V / 2048) * 2 f32), sp_cand (32 * ceil(V / 2048) * 32 u64):
// the spec-side workspace of the S * T <= 32 verify rows.  Refused before any launch: T or S outside 1 .. 8 (-3),
// S * T > 32 (-3), V outside 1 .. 262144 (-1), kcap outside 0 .. 20 (-2).
#define LP_SPEC_ROWS 32
extern "C" int lsa_spec_logprob_scan(const float* logits, int S, int T, int V, const int* lp_k, const int* finished,
                                     const int* gen_len, float* sp_raw, float* sp_ms, unsigned long long* sp_cand,
                                     int* lp_n0, hipStream_t st) {
  if (V < 1 || V > LP_MAXCH * LP_CHUNK) return -1;
  if (T < 1 || T > 8 || S < 1 || S > 8 || S * T > LP_SPEC_ROWS) return -3;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  const int vec = (V % 4 == 0) && (((uintptr_t)logits | (uintptr_t)sp_raw) % 16 == 0);
  hipLaunchKernelGGL(spec_logprob_scan_kernel, dim3(nch, T, S), dim3(256), 0, st, logits, V, vec, T, lp_k, finished,
                     gen_len, sp_raw, sp_ms, sp_cand, lp_n0, nch);
  return (int)hipGetLastError();
}

extern "C" int lsa_spec_logprob_commit(const float* sp_raw, int S, int T, int V, const float* sp_ms,
                                       const unsigned long long* sp_cand, const int* lp_k, const int* lp_n0,
                                       const int* gen_len, const int* out_tokens, int max_new, float* lp_tok,
                                       int* lp_ids, float* lp_top, int kcap, hipStream_t st) {
  if (V < 1 || V > LP_MAXCH * LP_CHUNK || max_new < 1) return -1;
  if (kcap < 0 || kcap > LP_KMAX) return -2;
  if (T < 1 || T > 8 || S < 1 || S > 8 || S * T > LP_SPEC_ROWS) return -3;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  hipLaunchKernelGGL(spec_logprob_commit_kernel, dim3(T, S), dim3(256), 0, st, sp_raw, V, T, sp_ms, sp_cand, nch, lp_k,
                     lp_n0, gen_len, out_tokens, max_new, lp_tok, lp_ids, lp_top, kcap);
  return (int)hipGetLastError();
}

// The prompt pair.  ms (R * ceil(V / 2048) * 2 f32), cand (R * ceil(V / 2048) * 32 u64; written and read only when
// any_k).  any_k: some row_k[r] > 0 -- with any_k = 0 the commit must be given kcap = 0 or rows with row_k <= 0 only.
// Refused before any launch: R < 1, V outside 1 .. 262144 (-1), kcap outside 0 .. 20 (-2).
extern "C" int lsa_prompt_logprob_scan(const float* logits, int R, int V, const int* targets, int any_k, float* ms,
                                       unsigned long long* cand, hipStream_t s) {
  if (R < 1 || V < 1 || V > LP_MAXCH * LP_CHUNK) return -1;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  const int vec = (V % 4 == 0) && ((uintptr_t)logits % 16 == 0);
  if (any_k)
    hipLaunchKernelGGL(prompt_logprob_scan_kernel<true>, dim3(nch, R), dim3(256), 0, s, logits, V, vec, targets, ms,
                       cand, nch);
  else
    hipLaunchKernelGGL(prompt_logprob_scan_kernel<false>, dim3(nch, R), dim3(256), 0, s, logits, V, vec, targets, ms,
                       cand, nch);
  return (int)hipGetLastError();
}

// any_k = 0: the scan wrote no candidates, so every row commits with K = 0 whatever row_k says
extern "C" int lsa_prompt_logprob_commit(const float* logits, int R, int V, const float* ms,
                                         const unsigned long long* cand, const int* targets, const int* row_k,
                                         int any_k, float* dst_tok, int* dst_ids, float* dst_top, int kcap,
                                         hipStream_t s) {
  if (R < 1 || V < 1 || V > LP_MAXCH * LP_CHUNK) return -1;
  if (kcap < 0 || kcap > LP_KMAX) return -2;
  const int nch = (V + LP_CHUNK - 1) / LP_CHUNK;
  hipLaunchKernelGGL(prompt_logprob_commit_kernel, dim3(R), dim3(256), 0, s, logits, V, ms, cand, nch, targets, row_k,
                     dst_tok, dst_ids, dst_top, any_k ? kcap : 0);
  return (int)hipGetLastError();
}
