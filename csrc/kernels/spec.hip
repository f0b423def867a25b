// Prompt-lookup (n-gram) drafter of speculative decoding (graph-capturable: everything is read from device memory).
//
//   spec_draft_kernel   one 256-thread workgroup per speculating row.  The row's context is
//                       ctx = prompt_tok[row, :prompt_len] (+) out_tokens[row, :gen_len] of length L, with
//                       ctx[L - 1] == input_ids[row] and positions[row] == L - 1.  Every candidate end j in
//                       [0, L - 2] is scored by m(j) = the number of i < n_max with ctx[j - i] == ctx[L - 1 - i],
//                       counted from i = 0 to the first mismatch (or j - i < 0); candidates need m >= n_min and the
//                       lexicographic maximum of (m, full, j) wins, full = (j + 1 + k <= L): the longest match, then a
//                       match whose whole k-token continuation exists, then the most recent.
//                       draft[i] = ctx[j + 1 + i] (or -1 past the end; all -1 without a candidate).
//                       Writes spec_ids[T] = [input_ids[row], max(draft, 0) ...], spec_pos[T] = positions[row] + t and
//                       spec_draft[k].  forced [nf, k] (optional) skips the search: the draft is row
//                       min(gen_len[row], nf - 1) of it (nf = 1: one fixed draft; tests plant per-step drafts, and it
//                       is the hook of a later drafter).  Row r reads the table at forced + r * forced_ld: 0 for one
//                       [nf, k] table that serves every row, nf * k for per-sequence tables [rows, nf, k].
//                       ops/reference.py spec_draft is the host twin.
#include "common.h"

__global__ __launch_bounds__(256) void spec_draft_kernel(const int* __restrict__ prompt_tok, int prompt_ld,
                                                         const int* __restrict__ prompt_len,
                                                         const int* __restrict__ out_tokens, int max_new,
                                                         const int* __restrict__ gen_len,
                                                         const int* __restrict__ input_ids,
                                                         const int* __restrict__ positions, int k, int n_max, int n_min,
                                                         const int* __restrict__ forced, int nf, int forced_ld,
                                                         int* __restrict__ spec_ids, int* __restrict__ spec_pos,
                                                         int* __restrict__ spec_draft) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int T = k + 1;
  const int* pt = prompt_tok + (size_t)row * prompt_ld;
  const int* ot = out_tokens + (size_t)row * max_new;
  const int pl = min(max(prompt_len[row], 0), prompt_ld);
  const int gl = min(max(gen_len[row], 0), max_new);
  const int L = pl + gl;
  auto ctx = [&](int i) { return i < pl ? pt[i] : ot[i - pl]; };
  __shared__ unsigned long long red[4];
  __shared__ int s_j;
  if (forced == nullptr) {
    // key = m << 33 | full << 32 | j (j < 2^31); 0 = no candidate (m >= n_min >= 1 makes every candidate non-zero)
    unsigned long long best = 0ull;
    for (int j = tid; j <= L - 2; j += 256) {
      int m = 0;
      while (m < n_max && j - m >= 0 && ctx(j - m) == ctx(L - 1 - m)) ++m;
      if (m >= n_min && m > 0) {
        const unsigned long long key = ((unsigned long long)m << 33) | ((unsigned long long)(j + 1 + k <= L) << 32) |
                                       (unsigned long long)(uint32_t)j;
        best = key > best ? key : best;
      }
    }
    best = wave_max_u64(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned long long b2 = red[0];
      for (int i = 1; i < 4; ++i) b2 = red[i] > b2 ? red[i] : b2;
      s_j = b2 ? (int)(uint32_t)(b2 & 0xffffffffull) : -1;
    }
    __syncthreads();
  }
  if (tid < T) {
    int d = -1;
    if (tid > 0) {
      const int i = tid - 1;
      if (forced != nullptr) {
        d = forced[(size_t)row * forced_ld + (size_t)min(gl, nf - 1) * k + i];
      } else if (s_j >= 0 && s_j + 1 + i < L) {
        d = ctx(s_j + 1 + i);
      }
      spec_draft[(size_t)row * k + i] = d;
    }
    spec_ids[(size_t)row * T + tid] = tid == 0 ? input_ids[row] : max(d, 0);
    spec_pos[(size_t)row * T + tid] = positions[row] + tid;
  }
}

extern "C" int lsa_spec_draft(const int* prompt_tok, int prompt_ld, const int* prompt_len, const int* out_tokens,
                              int max_new, const int* gen_len, const int* input_ids, const int* positions, int rows,
                              int k, int n_max, int n_min, const int* forced, int nf, int forced_ld, int* spec_ids,
                              int* spec_pos, int* spec_draft, hipStream_t s) {
  if (rows < 1 || k < 1 || k > 255 || n_max < 1 || n_min < 1 || n_min > n_max) return -1;
  if (forced != nullptr && (nf < 1 || (forced_ld != 0 && forced_ld != nf * k))) return -2;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(rows), dim3(256), 0, s, prompt_tok, prompt_ld, prompt_len, out_tokens,
                     max_new, gen_len, input_ids, positions, k, n_max, n_min, forced, nf, forced_ld, spec_ids, spec_pos,
                     spec_draft);
  return (int)hipGetLastError();
}
