// Token selection + device-side decode-state update (graph-capturable: no host round trip).
//
//   lsa_argmax_partial   [B, V] f32 logits -> per-chunk packed (orderable key << 32 | ~index) maxima
//   lsa_sample_commit    per row: greedy (temperature <= 0) = reduce the argmax partials; otherwise
//                        repetition / presence / frequency penalties (last `window` tokens, llama.cpp semantics),
//                        top-k (<= 64) by a per-chunk bitonic sort in LDS, temperature softmax, top-p nucleus and
//                        min-p on the same probabilities, and a counter-based RNG draw.  Then the decode state is
//                        advanced in place:
//                        out_tokens[b, gen_len[b]] = tok, gen_len++, input_ids = tok, positions++,
//                        finished on EOS / length.  A finished row keeps its position (its KV slot is
//                        re-written, never a new block), so a replayed graph can never walk past the
//                        blocks reserved for it.
//   lsa_spec_commit / lsa_spec_sample_commit   the verify rows of a speculative-decoding step: greedy / sampled
//                        (penalty, draw) pick per row and the in-order commit of the accepted run (see below)
#include "common.h"

#define LSA_TOPK 64
#define LSA_CHUNK 2048

__device__ __forceinline__ unsigned long long pack_key(float v, int idx) {
  return ((unsigned long long)float_key(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)idx);
}

__global__ __launch_bounds__(256) void argmax_partial_kernel(const float* __restrict__ logits, int V, int chunk,
                                                             unsigned long long* __restrict__ part, int nch) {
  const int c = blockIdx.x, b = blockIdx.y;
  const float* row = logits + (size_t)b * V;
  const int lo = c * chunk, hi = min(V, lo + chunk);
  unsigned long long best = 0ull;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const unsigned long long k = pack_key(row[i], i);
    best = k > best ? k : best;
  }
  best = wave_max_u64(best);
  __shared__ unsigned long long red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b2 = red[0];
    for (int i = 1; i < 4; ++i) b2 = red[i] > b2 ? red[i] : b2;
    part[(size_t)b * nch + c] = b2;
  }
}

struct DecodeState {
  int* out_tokens;  // [B, max_new]
  int max_new;
  int* gen_len;     // [B]
  int* input_ids;   // [B]
  int* positions;   // [B]
  int* finished;    // [B]
  const int* eos;   // [neos]
  int neos;
  const int* limit;   // [B] per-row max new tokens (<= max_new)
  const int* eos_on;  // [B] 0 = ignore EOS for this row
  int* hist;          // [B, window] ring of the context's last tokens (slot = position % window), or null
  int window;
};

__device__ void commit_token(const DecodeState& st, int b, int tok) {
  if (st.finished[b]) return;
  const int n = st.gen_len[b];
  if (n < st.max_new) st.out_tokens[(size_t)b * st.max_new + n] = tok;
  st.gen_len[b] = n + 1;
  bool done = (n + 1) >= min(st.max_new, st.limit[b]);
  if (st.eos_on[b])
    for (int e = 0; e < st.neos; ++e) done |= (tok == st.eos[e]);
  st.input_ids[b] = tok;
  if (st.hist) st.hist[(size_t)b * st.window + (st.positions[b] + 1) % st.window] = tok;  // its position
  if (done) {
    st.finished[b] = 1;
  } else {
    st.positions[b] += 1;
  }
}

__global__ __launch_bounds__(64) void argmax_commit_kernel(const unsigned long long* __restrict__ part, int nch,
                                                           DecodeState st) {
  const int b = blockIdx.x;
  unsigned long long best = 0ull;
  for (int i = threadIdx.x; i < nch; i += 64) {
    const unsigned long long k = part[(size_t)b * nch + i];
    best = k > best ? k : best;
  }
  best = wave_max_u64(best);
  if (threadIdx.x == 0) commit_token(st, b, (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull)));
}

// ---------------------------------------------------------------- sampling path
// bitonic sort (descending by key) of n (power of two) packed keys in LDS with the whole block
__device__ void bitonic_desc(unsigned long long* a, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      // the compare-exchange loop starts on an instruction-cache line, wherever the code before the sort puts it (a
      // few bytes more ahead of it moved the sort of 4096 candidates by 5%: README, "Sampling options")
      asm volatile(".p2align 6");
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int ix = i ^ j;
        if (ix > i) {
          const unsigned long long x = a[i], y = a[ix];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) {
            a[i] = y;
            a[ix] = x;
          }
        }
      }
      __syncthreads();
    }
  }
}

// repetition penalty applied in place (llama.cpp / Ollama semantics: logit / pen if > 0, else * pen) to
// each distinct token among the row's last `last_n` context tokens (prompt + generated), read from the
// position-indexed ring `hist` ending at the current input position.  Then llama.cpp's presence / frequency penalties
// over the same window: a token that occurs c times in it loses fma(c, frequency, presence) (one rounding of the
// subtrahend, one of the subtraction; ops/reference.py repeat_penalty is the exact host twin).  penalty / presence /
// frequency: per row, null = off (1 / 0 / 0); a row with all three off is left alone.
__device__ __forceinline__ float penalised(float v, float pen, float pres, float freq, int c) {
#pragma clang fp contract(off)  // v * pen and the subtraction round separately: no second fused multiply-add
  v = v > 0.f ? v / pen : v * pen;
  return v - __fmaf_rn((float)c, freq, pres);
}

__global__ __launch_bounds__(64) void repeat_penalty_kernel(float* __restrict__ logits, int V,
                                                            const int* __restrict__ hist, int window,
                                                            const float* __restrict__ penalty,
                                                            const int* __restrict__ last_n,
                                                            const int* __restrict__ positions,
                                                            const float* __restrict__ presence,
                                                            const float* __restrict__ frequency) {
  const int b = blockIdx.x;
  const float pen = penalty ? penalty[b] : 1.0f;
  const float pres = presence ? presence[b] : 0.f;
  const float freq = frequency ? frequency[b] : 0.f;
  if (pen == 1.0f && pres == 0.f && freq == 0.f) return;
  const bool counted = freq != 0.f;  // (the count multiplies nothing else)
  const int* hrow = hist + (size_t)b * window;
  const int p = positions[b];
  const int n = min(min(last_n ? last_n[b] : window, window), p + 1);
  for (int i = threadIdx.x; i < n; i += 64) {
    const int t = hrow[(p - i) % window];
    if (t < 0 || t >= V) continue;
    bool first = true;  // the most recent occurrence applies the penalties, once per distinct token
    for (int k = 0; k < i; ++k) first &= (hrow[(p - k) % window] != t);
    if (!first) continue;
    int c = 1;  // its occurrences in the window: itself and the older ones
    if (counted)
      for (int k = i + 1; k < n; ++k) c += (hrow[(p - k) % window] == t);
    float* q = logits + (size_t)b * V + t;
    *q = penalised(*q, pen, pres, freq, c);
  }
}

// stage 1: per (chunk, row) top-LSA_TOPK keys of temperature-free logits
__global__ __launch_bounds__(256) void topk_partial_kernel(const float* __restrict__ logits, int V,
                                                           unsigned long long* __restrict__ cand, int nch) {
  __shared__ unsigned long long a[LSA_CHUNK];
  const int c = blockIdx.x, b = blockIdx.y;
  const int lo = c * LSA_CHUNK;
  for (int i = threadIdx.x; i < LSA_CHUNK; i += 256) {
    const int gi = lo + i;
    a[i] = gi < V ? pack_key(logits[(size_t)b * V + gi], gi) : 0ull;
  }
  __syncthreads();
  bitonic_desc(a, LSA_CHUNK);
  for (int i = threadIdx.x; i < LSA_TOPK; i += 256) cand[((size_t)b * nch + c) * LSA_TOPK + i] = a[i];
}

// splitmix64 finalizer of a stream key
__device__ __forceinline__ unsigned long long lsa_key_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float uniform01(unsigned long long seed, unsigned long long ctr) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// the greedy pick of one row: the first wave reduces the row's argmax partials (the token on every lane of it)
__device__ __forceinline__ int argmax_pick(const unsigned long long* __restrict__ part_row, int nch) {
  unsigned long long best = 0ull;
  for (int i = threadIdx.x; i < nch; i += 64) {
    const unsigned long long k = part_row[i];
    best = k > best ? k : best;
  }
  best = wave_max_u64(best);
  return (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
}

// THE sampler: the sampled pick of one row by its whole block (a: ncand_pow2 keys of dynamic LDS) -- merge the row's
// candidates, softmax(T), top-k / top-p, inverse-CDF pick at draw counter `ctr` of the seed word `sv`.  The token is
// returned on the first wave (-1 on the others).  sample_commit_kernel and spec_sample_pick_kernel both call it.
// min_p: next to the nucleus rule, candidate i > 0 stays only if e_i >= min_p; e_0 is exactly 1, so that is p_i >= min_p
// * p_max on the temperature-scaled probabilities, with no division.  min_p = 0 keeps every lane's `keep` as it is.
__device__ int sample_pick(unsigned long long* a, const unsigned long long* __restrict__ cand_row, int ncand_pow2,
                           int ncand, float T, int k, float tp, float min_p, unsigned long long sv,
                           unsigned long long ctr) {
  for (int i = threadIdx.x; i < ncand_pow2; i += blockDim.x) a[i] = i < ncand ? cand_row[i] : 0ull;
  __syncthreads();
  bitonic_desc(a, ncand_pow2);
  if (threadIdx.x >= 64) return -1;
  if (k <= 0 || k > LSA_TOPK) k = LSA_TOPK;
  const int i = threadIdx.x;
  const uint32_t* a32 = reinterpret_cast<const uint32_t*>(a);
  const float lmax = key_float(a32[1]);
  const float li = key_float(a32[2 * i + 1]);
  float e = (i < k && a[i] != 0ull) ? __expf((li - lmax) / T) : 0.f;
  const float tot = wave_sum(e);
  float p = e / tot;
  // inclusive prefix sum over the (sorted) probabilities
  float cum = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float x = __shfl_up(cum, o, 64);
    if (i >= o) cum += x;
  }
  // keep token i if the mass before it is < top_p and it reaches min_p of the best one (always keeps the first)
  const bool keep = (i < k) && (i == 0 || ((cum - p) < tp && e >= min_p)) && e > 0.f;
  const float pk = keep ? p : 0.f;
  const float ktot = wave_sum(pk);
  const float pn = pk / ktot;
  float cumk = pn;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float x = __shfl_up(cumk, o, 64);
    if (i >= o) cumk += x;
  }
  // draw g of a request: the request's seed is the stream KEY (scrambled, so seeds 0, 1, 2, ... give unrelated
  // streams) and the draw index the counter; the seed word packs the key (low 40 bits) with a counter offset (high 24
  // bits: the tokens a preempted request already generated, so its re-admission continues the same stream
  // whatever slot it lands in).  ops/reference.py device_uniform is the exact host twin (sample_pick of the pick).
  const float u = uniform01(lsa_key_mix(sv & 0xFFFFFFFFFFull), (sv >> 40) + ctr);
  // first kept index whose cumulative mass exceeds u (fallback: last kept index)
  int first_hit = (keep && u < cumk) ? i : 64;
  int last_kept = keep ? i : -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    first_hit = min(first_hit, __shfl_xor(first_hit, o, 64));
    last_kept = max(last_kept, __shfl_xor(last_kept, o, 64));
  }
  const int pick = first_hit < 64 ? first_hit : (last_kept >= 0 ? last_kept : 0);
  return (int)(0xffffffffu - (uint32_t)(a[pick] & 0xffffffffull));
}

// stage 2: one block per row — merge candidates, softmax(T), top-k/top-p, draw, commit
__global__ __launch_bounds__(1024) void sample_commit_kernel(const unsigned long long* __restrict__ cand, int ncand_pow2,
                                                             int ncand, const unsigned long long* __restrict__ amax_part,
                                                             int nch_amax, const float* __restrict__ temperature,
                                                             const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                             const unsigned long long* __restrict__ seeds,
                                                             const float* __restrict__ min_p, DecodeState st) {
  extern __shared__ unsigned long long a[];
  const int b = blockIdx.x;
  const float T = temperature[b];
  if (T <= 0.f) {  // greedy row inside a sampled batch
    if (threadIdx.x < 64) {
      const int tok = argmax_pick(amax_part + (size_t)b * nch_amax, nch_amax);
      if (threadIdx.x == 0) commit_token(st, b, tok);
    }
    return;
  }
  // the draw counter, read by every thread before the pick's first barrier: thread 0 commits (and advances it) after
  const int g = st.gen_len[b];
  const int tok = sample_pick(a, cand + (size_t)b * ncand, ncand_pow2, ncand, T, top_k[b], top_p[b],
                              min_p ? min_p[b] : 0.f, seeds[b], (unsigned long long)g);
  if (threadIdx.x == 0) commit_token(st, b, tok);
}

extern "C" int lsa_argmax_commit(const float* logits, int B, int V, unsigned long long* part, int* out_tokens,
                                 int max_new, int* gen_len, int* input_ids, int* positions, int* finished,
                                 const int* eos, int neos, const int* limit, const int* eos_on, hipStream_t s) {
  const int chunk = 4096;
  const int nch = (V + chunk - 1) / chunk;
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(nch, B), dim3(256), 0, s, logits, V, chunk, part, nch);
  DecodeState st{out_tokens, max_new, gen_len, input_ids, positions, finished, eos, neos, limit, eos_on, nullptr, 0};
  hipLaunchKernelGGL(argmax_commit_kernel, dim3(B), dim3(64), 0, s, part, nch, st);
  return (int)hipGetLastError();
}

// Speculative decoding (spec.hip drafts): logits [S * T, V] are the T = k + 1 verify rows of each of S sequences;
// workgroup s verifies rows s T .. s T + T - 1 against draft[s k ..] into state row s of st.  tok_i = argmax(logits[s T
// + i]); a = the number of leading i < k with draft[i] == tok_i (a -1 draft never matches); tok_0 .. tok_a are
// committed in order through commit_token, so nothing follows a finishing token (EOS / length).  stats [S, 3]: row s is
// written by workgroup s alone (plain stores), stats[s] += (1 step, drafts >= 0, tokens committed beyond the first).
// A finished row changes nothing and counts nothing.
__global__ __launch_bounds__(64) void spec_commit_kernel(const unsigned long long* __restrict__ part, int nch, int k,
                                                         const int* __restrict__ draft, long long* __restrict__ stats,
                                                         DecodeState st) {
  const int s = blockIdx.x;
  part += (size_t)s * (k + 1) * nch;
  draft += (size_t)s * k;
  stats += (size_t)s * 3;
  int tok = 0;
  bool run = true;  // tok_0 .. tok_{i-1} matched their drafts
  int committed = 0, drafted = 0;
  const bool live = !st.finished[s];
  for (int i = 0; i <= k; ++i) {
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < nch; c += 64) {
      const unsigned long long key = part[(size_t)i * nch + c];
      best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    tok = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
    if (threadIdx.x == 0 && run && live && !st.finished[s]) {
      commit_token(st, s, tok);
      ++committed;
    }
    if (i < k) {
      const int d = draft[i];
      drafted += d >= 0;
      run = run && d >= 0 && d == tok;
    }
  }
  if (threadIdx.x == 0 && live) {
    stats[0] += 1;
    stats[1] += drafted;
    stats[2] += committed > 0 ? committed - 1 : 0;
  }
}

extern "C" int lsa_spec_commit(const float* logits, int S, int T, int V, unsigned long long* part, const int* draft,
                               long long* stats, int* out_tokens, int max_new, int* gen_len, int* input_ids,
                               int* positions, int* finished, const int* eos, int neos, const int* limit,
                               const int* eos_on, hipStream_t s) {
  if (T < 2) return -1;
  if (S < 1 || (S > 1 && S * T > 32)) return -2;
  const int chunk = 4096;
  const int nch = (V + chunk - 1) / chunk;
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(nch, S * T), dim3(256), 0, s, logits, V, chunk, part, nch);
  DecodeState st{out_tokens, max_new, gen_len, input_ids, positions, finished, eos, neos, limit, eos_on, nullptr, 0};
  hipLaunchKernelGGL(spec_commit_kernel, dim3(S), dim3(64), 0, s, part, nch, T - 1, draft, stats, st);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- speculative decoding of sampled requests
// lsa_spec_sample_commit: logits [S * T, V] are the T = k + 1 verify rows of each of S sequences.  Sequence s owns rows
// s T .. s T + T - 1 of logits / part / cand / picks, draft + s k, ring row s, entry s of every sampling parameter,
// state row s and stats + 3 s; p = positions[s] and n = gen_len[s] at the launch.  Verify row i of a sequence makes the
// very draw the plain step would make for its generated token n + i -- penalised over the ring as it would stand had
// drafts 0 .. i-1 been committed, drawn at counter n + i -- and a draft is accepted exactly when it equals that draw,
// so the committed sequence is the plain sampled sequence of the same seed, whatever slot it runs in and whatever its
// neighbours are (a greedy request is a sequence with temperature 0 and penalty 1).  Four launches after the partials:
// penalty (grid T x S) -> argmax / top-k partials (B = S T) -> pick (grid T x S, picks[s T + i]) -> in-order commit
// (one wave per sequence).  No workgroup reads a word another workgroup of its launch writes.

// Penalties of verify row i, in place, with repeat_penalty_kernel's rule (counts included) over the tokens at positions
// (p + i - m, p + i], m = min(last_n, window, p + i + 1): the token at position p + j, 1 <= j <= i, is draft[j - 1];
// the token at a position <= p is hist[pos % window].  (A ring slot whose position is > p still holds the token
// `window` positions older; m <= window, so no such slot is ever read for it.)  A draft < 0 or >= V penalises nothing.
__global__ __launch_bounds__(64) void spec_repeat_penalty_kernel(float* __restrict__ logits, int V,
                                                                 const int* __restrict__ hist, int window,
                                                                 const float* __restrict__ penalty,
                                                                 const int* __restrict__ last_n,
                                                                 const int* __restrict__ positions,
                                                                 const int* __restrict__ draft,
                                                                 const float* __restrict__ presence,
                                                                 const float* __restrict__ frequency) {
  const int row = blockIdx.x, s = blockIdx.y, T = gridDim.x;
  const float pen = penalty ? penalty[s] : 1.0f;
  const float pres = presence ? presence[s] : 0.f;
  const float freq = frequency ? frequency[s] : 0.f;
  if (pen == 1.0f && pres == 0.f && freq == 0.f) return;
  const bool counted = freq != 0.f;
  hist += (size_t)s * window;
  draft += (size_t)s * (T - 1);
  const int p = positions[s];
  const int P = p + row;
  const int n = min(min(last_n ? last_n[s] : window, window), P + 1);
  auto tok_at = [&](int pos) { return pos > p ? draft[pos - p - 1] : hist[pos % window]; };
  for (int i = threadIdx.x; i < n; i += 64) {
    const int t = tok_at(P - i);
    if (t < 0 || t >= V) continue;
    bool first = true;  // the most recent occurrence applies the penalties, once per distinct token
    for (int k = 0; k < i; ++k) first &= (tok_at(P - k) != t);
    if (!first) continue;
    int c = 1;  // its occurrences in the row's window, the drafts before the row included
    if (counted)
      for (int k = i + 1; k < n; ++k) c += (tok_at(P - k) == t);
    float* q = logits + ((size_t)s * T + row) * V + t;
    *q = penalised(*q, pen, pres, freq, c);
  }
}

// per verify row of sequence s: the token the plain step would commit for its generated token n + row (the sampler of
// sample_commit_kernel at draw counter n + row; temperature <= 0: the row's argmax) -> picks[s T + row]
__global__ __launch_bounds__(1024) void spec_sample_pick_kernel(const unsigned long long* __restrict__ cand,
                                                                int ncand_pow2, int ncand,
                                                                const unsigned long long* __restrict__ amax_part,
                                                                int nch_amax, const float* __restrict__ temperature,
                                                                const int* __restrict__ top_k,
                                                                const float* __restrict__ top_p,
                                                                const unsigned long long* __restrict__ seeds,
                                                                const float* __restrict__ min_p,
                                                                const int* __restrict__ gen_len, int* __restrict__ picks) {
  extern __shared__ unsigned long long a[];
  const int s = blockIdx.y;
  const int row = s * gridDim.x + blockIdx.x;  // of logits / part / cand / picks
  const float T = temperature[s];
  if (T <= 0.f) {  // greedy, with or without a repetition penalty
    if (threadIdx.x < 64) {
      const int tok = argmax_pick(amax_part + (size_t)row * nch_amax, nch_amax);
      if (threadIdx.x == 0) picks[row] = tok;
    }
    return;
  }
  const int tok = sample_pick(a, cand + (size_t)row * ncand, ncand_pow2, ncand, T, top_k[s], top_p[s],
                              min_p ? min_p[s] : 0.f, seeds[s], (unsigned long long)(gen_len[s] + blockIdx.x));
  if (threadIdx.x == 0) picks[row] = tok;
}

// one wave per sequence s: a = the number of leading i < k with draft[i] >= 0 && draft[i] == picks[i] (its own k drafts
// and k + 1 picks); picks[0 .. a] are committed in order through commit_token (ring included), so nothing follows a
// finishing token; stats row s as spec_commit_kernel.  A finished sequence changes nothing and counts nothing.
__global__ __launch_bounds__(64) void spec_sample_commit_kernel(const int* __restrict__ picks, int k,
                                                                const int* __restrict__ draft,
                                                                long long* __restrict__ stats, DecodeState st) {
  if (threadIdx.x != 0) return;
  const int s = blockIdx.x;
  picks += (size_t)s * (k + 1);
  draft += (size_t)s * k;
  stats += (size_t)s * 3;
  const bool live = !st.finished[s];
  bool run = true;  // picks[0 .. i-1] matched their drafts
  int committed = 0, drafted = 0;
  for (int i = 0; i <= k; ++i) {
    const int tok = picks[i];
    if (run && live && !st.finished[s]) {
      commit_token(st, s, tok);
      ++committed;
    }
    if (i < k) {
      const int d = draft[i];
      drafted += d >= 0;
      run = run && d >= 0 && d == tok;
    }
  }
  if (live) {
    stats[0] += 1;
    stats[1] += drafted;
    stats[2] += committed > 0 ? committed - 1 : 0;
  }
}

// workspace: part (S T * ceil(V/4096) u64) + cand (S T * ceil(V/2048) * 64 u64) + picks (S T int)
extern "C" int lsa_spec_sample_commit(float* logits, int S, int T, int V, const int* draft, long long* stats, int* hist,
                                      int window, const float* penalty, const int* last_n, const float* temperature,
                                      const int* top_k, const float* top_p, const unsigned long long* seeds,
                                      int* out_tokens, int max_new, int* gen_len, int* input_ids, int* positions,
                                      int* finished, const int* eos, int neos, const int* limit, const int* eos_on,
                                      unsigned long long* part, unsigned long long* cand, int* picks,
                                      const float* presence, const float* frequency, const float* min_p, hipStream_t s) {
  // sizes refused before anything is launched or written: 2 <= T <= 8 verify rows per sequence, S T <= 32 rows (the
  // verify buffers), V <= 262144 (lsa_sample_commit)
  if (T < 2 || T > 8 || V < 1) return -1;
  if (S < 1 || S * T > 32) return -2;
  const int nch2 = (V + LSA_CHUNK - 1) / LSA_CHUNK;
  const int ncand = nch2 * LSA_TOPK;
  int p2 = 64;
  while (p2 < ncand) p2 <<= 1;
  if (p2 > 8192) return -1;
  if (hist && window > 0 && (penalty || presence || frequency))
    hipLaunchKernelGGL(spec_repeat_penalty_kernel, dim3(T, S), dim3(64), 0, s, logits, V, hist, window, penalty,
                       last_n, positions, draft, presence, frequency);
  const int chunk = 4096;
  const int nch = (V + chunk - 1) / chunk;
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(nch, S * T), dim3(256), 0, s, logits, V, chunk, part, nch);
  hipLaunchKernelGGL(topk_partial_kernel, dim3(nch2, S * T), dim3(256), 0, s, logits, V, cand, nch2);
  hipLaunchKernelGGL(spec_sample_pick_kernel, dim3(T, S), dim3(1024), p2 * sizeof(unsigned long long), s, cand, p2,
                     ncand, part, nch, temperature, top_k, top_p, seeds, min_p, gen_len, picks);
  DecodeState st{out_tokens, max_new, gen_len, input_ids, positions, finished, eos, neos, limit, eos_on,
                 window > 0 ? hist : nullptr, window};
  hipLaunchKernelGGL(spec_sample_commit_kernel, dim3(S), dim3(64), 0, s, picks, T - 1, draft, stats, st);
  return (int)hipGetLastError();
}

// workspace: part (B * ceil(V/4096) u64) + cand (B * ceil(V/2048) * 64 u64)
extern "C" int lsa_sample_commit(float* logits, int B, int V, unsigned long long* part, unsigned long long* cand,
                                 int* hist, int window, const float* penalty, const int* last_n,
                                 const float* temperature,
                                 const int* top_k, const float* top_p, const unsigned long long* seeds,
                                 int* out_tokens, int max_new, int* gen_len, int* input_ids, int* positions,
                                 int* finished, const int* eos, int neos, const int* limit, const int* eos_on,
                                 const float* presence, const float* frequency, const float* min_p, hipStream_t s) {
  const int nch2 = (V + LSA_CHUNK - 1) / LSA_CHUNK;
  const int ncand = nch2 * LSA_TOPK;
  int p2 = 64;
  while (p2 < ncand) p2 <<= 1;
  // V > 262144 unsupported (8192 candidates = 64 KiB of dynamic LDS); refused before anything is launched, so
  // neither the logits (penalty) nor the workspace is touched
  if (p2 > 8192) return -1;
  if (hist && window > 0 && (penalty || presence || frequency))
    hipLaunchKernelGGL(repeat_penalty_kernel, dim3(B), dim3(64), 0, s, logits, V, hist, window, penalty, last_n,
                       positions, presence, frequency);
  const int chunk = 4096;
  const int nch = (V + chunk - 1) / chunk;
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(nch, B), dim3(256), 0, s, logits, V, chunk, part, nch);
  hipLaunchKernelGGL(topk_partial_kernel, dim3(nch2, B), dim3(256), 0, s, logits, V, cand, nch2);
  DecodeState st{out_tokens, max_new, gen_len, input_ids, positions, finished, eos, neos, limit, eos_on,
                 window > 0 ? hist : nullptr, window};
  hipLaunchKernelGGL(sample_commit_kernel, dim3(B), dim3(1024), p2 * sizeof(unsigned long long), s, cand, p2, ncand,
                     part, nch, temperature, top_k, top_p, seeds, min_p, st);
  return (int)hipGetLastError();
}
