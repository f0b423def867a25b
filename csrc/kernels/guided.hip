// Regex-constrained decoding: the device-side token mask (graph-capturable: everything is read from device memory).
//
//   dfa_mask_kernel   grid (ceil(V / 2048), B), 256 threads.  Row b of logits [B, V] belongs to table row
//                     r = rows ? rows[b] : b (decode: the slot itself; prefill tail: the sequence's slot).
//                     The row returns at once when g_on[r] == 0 or finished[b] != 0.
//
//   Tables of row r (engine/guided.py compiles them): cls[r][256] u8 byte -> class, trans[r][S * C] u16 with
//   trans[s * C + cls[byte]] the next state or DEAD (0xFFFF), accept[r][S] u8, g_dim[r] = (S, C), S * C <= 32768.
//   The token bytes are CSR: tok_off[V + 1] / tok_blob.
//
//   Lazy advance (the commit kernels know nothing of the DFA).  n = gen_len[b]:
//     n == g_base[r]:  cur = g_state[r][n & 1]                     (the host wrote both slots at admission)
//     otherwise:       cur = walk(g_state[r][(n - 1) & 1], bytes(input_ids[b]))
//   Every workgroup computes cur for itself (every lane, from the token's bytes parked in LDS: no second barrier);
//   workgroup 0 of the row stores it to slot n & 1, whose value no workgroup uses in this launch (they use slot
//   (n - 1) & 1), with a plain vector store.  The next launch finds it across
//   the kernel boundary.  A launch that sees the same n again recomputes the same value from the same slot.
//
//   The workgroup stages cls and the live S * C entries of trans into LDS (static 64 KiB + 256 B: two workgroups
//   per CU), then each thread walks 8 tokens (ids chunk * 2048 + j * 256 + tid: coalesced logits stores) in lockstep,
//   so the 8 dependent LDS chains of a lane overlap; the loads that do not depend on the state (offsets, state words,
//   the next byte of every token) are issued ahead of the step that needs them.  A token stays when its length is 1..32 bytes and the walk from
//   cur never reaches DEAD; an id of eos[] stays when accept[cur] (or when cur is DEAD, which only a token committed
//   outside the mask can cause: the row may then only stop).  Every other logit becomes -inf; an allowed one is not
//   touched.  ops/reference.py dfa_mask is the host twin.
//
// Speculative decoding of constrained requests (the verify step's T = k + 1 logits rows of each of S sequences):
//
//   dfa_mask_verify_kernel   grid (ceil(V / 2048), T, S), 256 threads.  Sequence s = blockIdx.z is the sequence of state
//                     row s (gen_len[s], input_ids[s], finished[s]) and table row r + s; it reads its drafts at
//                     draft + s * k, masks logits rows s * T + t and writes g_spec + 9 * s (g_spec is [S, 1 + 8]).  The
//                     one-sequence form is S = 1 with any r (state row 0, table row r: the speculating slot is 0); the
//                     form over S sequences is r = 0, so table row = state row = slot, as in the plain decode mask.  The
//                     workgroups of a sequence return at once when g_on[r + s] == 0 or finished[s] != 0 (uniform per
//                     workgroup: one scalar load each for an unconstrained, finished or released slot, whose logits
//                     rows, state words and g_spec row stay untouched).
//                     Row t is masked exactly as dfa_mask_kernel masks a row whose current state is s_t, with
//                     s_0 = cur of the lazy advance above (workgroup (0, 0, s) stores it to slot n & 1 of table row
//                     r + s when n != g_base[r + s]) and s_t = walk(s_{t-1}, bytes(draft[t - 1])).
//                     A draft of -1, outside [0, V), of 0 or more than
//                     32 bytes, or one whose walk dies makes s_t and every later state DEAD: such a row can only be
//                     reached through a draft the previous row's mask already set to -inf, and it is masked by the same
//                     rule (EOS only) instead of skipped.  The draft bytes (at most 7 x 32 B) are parked in LDS beside
//                     the input token's and walked by every lane with broadcast reads.  Workgroup (0, t, s) stores s_t
//                     to g_spec[9 s + 1 + t], workgroup (0, 0, s) stores n to g_spec[9 s].
//                     What the S-form keeps of the one-sequence kernel: the shared __device__ helpers (dfa_stage,
//                     dfa_tok_spans, dfa_walk_mask); the static LDS footprint of 64 KiB + 256 B + the input token's and
//                     the drafts' bytes (32 B + 7 x 32 B); plain vector stores only; no workgroup reads a word that
//                     another workgroup of the same launch writes (a sequence touches only its own state row, table
//                     row, logits rows and g_spec row, and within a sequence the rule above holds as before); nothing
//                     ever waits on another workgroup.  Sequence s runs the instructions of its own one-sequence
//                     launch on the same operands, so it computes the same bits.
//                     ops/reference.py dfa_mask_verify / dfa_mask_verify_batch are the twins.
//
//   dfa_spec_advance_kernel  after spec_commit: grid (S), one wave per sequence.  n' = gen_len[s], n0 = g_spec[9 s],
//                     a = n' - n0 - 1 accepted drafts: with g_on[r + s] set and 0 <= a <= k it stores
//                     g_spec[9 s + 1 + a] & 0xFFFF to g_state[r + s][(n' - 1) & 1].  So after a verify step slot
//                     (n' - 1) & 1 holds the state after n' - 1 generated tokens, and the next launch's lazy advance over
//                     input_ids[s] is right whether it is dfa_mask_verify -- over one sequence or several -- or the
//                     plain dfa_mask (after the acceptance guard's fallback, or when another request arrives or
//                     leaves).  A replay on a finished row (the mask returned at once, gen_len stands still) rewrites
//                     the same value, or -- with a g_spec row left by an earlier request -- a dead word into a row
//                     nobody masks; admission and resume rewrite both slots (ModelRunner._set_guided).
#include "common.h"

#define DFA_DEAD 0xFFFFu
#define DFA_MAX_TABLE 32768
#define DFA_MAX_TOKEN_BYTES 32
#define DFA_CHUNK 2048
#define DFA_TPT 8  // tokens per thread
#define DFA_MAX_VERIFY 8  // verify rows T = k + 1 of a sequence in dfa_mask_verify_kernel
#define DFA_MAX_SEQS 8    // sequences of one dfa_mask_verify_kernel launch ...
#define DFA_MAX_ROWS 32   // ... and their rows S * T (the verify step's limits)

// The table of one row in LDS: step() is one transition; s == DEAD lands past SC and stays DEAD.
struct DfaLds {
  const uint16_t* trans;
  const uint8_t* cls;
  uint32_t C, SC;
  __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t bt) const {
    const uint32_t idx = s * C + cls[bt];
    return idx < SC ? (uint32_t)trans[idx] : DFA_DEAD;
  }
};

// CSR offsets / lengths of the thread's 8 tokens (0 / 0 for ids past V and for lengths outside 1..32); returns the
// longest length.
__device__ __forceinline__ int dfa_tok_spans(int V, const int* __restrict__ tok_off, int tok0, int (&off)[DFA_TPT],
                                             int (&len)[DFA_TPT]) {
  int maxlen = 0;
#pragma unroll
  for (int j = 0; j < DFA_TPT; ++j) {
    const int tok = tok0 + j * 256;
    off[j] = 0;
    len[j] = 0;
    if (tok < V) {
      const int o = tok_off[tok], l = tok_off[tok + 1] - o;
      if (l >= 1 && l <= DFA_MAX_TOKEN_BYTES) {
        off[j] = o;
        len[j] = l;
        maxlen = max(maxlen, l);
      }
    }
  }
  return maxlen;
}

// cls and the live S * C entries of trans of table row r into LDS (the caller's barrier publishes them).
__device__ __forceinline__ void dfa_stage(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ cls, int r,
                                          uint32_t SC, uint16_t* s_trans, uint8_t* s_cls, int tid) {
  // rows of trans are 64 KiB apart, so 16-byte loads are aligned; the last one may run past S * C but stays
  // inside the row (S * C <= 32768 = the row length)
  const uint4* src = reinterpret_cast<const uint4*>(trans + (size_t)r * DFA_MAX_TABLE);
  uint4* dst = reinterpret_cast<uint4*>(s_trans);
  const int n16 = (int)((SC + 7u) >> 3);
  for (int i = tid; i < n16; i += 256) dst[i] = src[i];
  s_cls[tid] = cls[(size_t)r * 256 + tid];
}

// The per-token walk both kernels share: the thread's 8 tokens (ids tok0 + j * 256) walk from cur in lockstep; -inf
// into row[tok] of every token that dies, has no bytes or too many, and of every EOS id unless eos_ok.  byte[] holds
// the first byte of each token (loaded by the caller ahead of its barrier).
__device__ __forceinline__ void dfa_walk_mask(const DfaLds& t, uint32_t cur, bool eos_ok, float* __restrict__ row,
                                              int V, int tok0, const uint8_t* __restrict__ tok_blob,
                                              const int (&off)[DFA_TPT], const int (&len)[DFA_TPT], int maxlen,
                                              uint32_t (&byte)[DFA_TPT], const int* __restrict__ eos, int neos) {
  uint32_t st[DFA_TPT];
#pragma unroll
  for (int j = 0; j < DFA_TPT; ++j) st[j] = len[j] > 0 ? cur : DFA_DEAD;
  for (int i = 0; i < maxlen; ++i) {
    uint32_t next[DFA_TPT];  // byte i + 1 is fetched while byte i walks the table
#pragma unroll
    for (int j = 0; j < DFA_TPT; ++j) {
      next[j] = (i + 1 < len[j] && st[j] != DFA_DEAD) ? (uint32_t)tok_blob[off[j] + i + 1] : 0u;
    }
#pragma unroll
    for (int j = 0; j < DFA_TPT; ++j) {
      if (i < len[j] && st[j] != DFA_DEAD) st[j] = t.step(st[j], byte[j]);
      byte[j] = next[j];
    }
  }
#pragma unroll
  for (int j = 0; j < DFA_TPT; ++j) {
    const int tok = tok0 + j * 256;
    if (tok >= V) continue;
    bool allowed = st[j] != DFA_DEAD;
    for (int e = 0; e < neos; ++e) {
      if (eos[e] == tok) allowed = eos_ok;
    }
    if (!allowed) row[tok] = -INFINITY;
  }
}

__global__ __launch_bounds__(256) void dfa_mask_kernel(float* __restrict__ logits, int V,
                                                       const int* __restrict__ tok_off,
                                                       const uint8_t* __restrict__ tok_blob,
                                                       const uint8_t* __restrict__ cls,
                                                       const uint16_t* __restrict__ trans,
                                                       const uint8_t* __restrict__ accept,
                                                       const int* __restrict__ g_dim, const int* __restrict__ g_on,
                                                       int* __restrict__ g_state, const int* __restrict__ g_base,
                                                       const int* __restrict__ rows, const int* __restrict__ gen_len,
                                                       const int* __restrict__ input_ids,
                                                       const int* __restrict__ finished, const int* __restrict__ eos,
                                                       int neos) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int r = rows != nullptr ? rows[b] : b;
  if (g_on[r] == 0 || finished[b] != 0) return;  // uniform per workgroup

  __shared__ __attribute__((aligned(16))) uint16_t s_trans[DFA_MAX_TABLE];
  __shared__ uint8_t s_cls[256];
  __shared__ uint8_t s_in[DFA_MAX_TOKEN_BYTES];  // the bytes of the row's last committed token

  // Every load whose address is known now is issued before anything waits: the row's dims and state words (uniform
  // addresses: scalar loads, repeated by every wave) and the CSR offsets of this thread's 8 tokens.
  const int S = min(max(g_dim[2 * r], 0), DFA_MAX_TABLE);
  const uint32_t C = (uint32_t)min(max(g_dim[2 * r + 1], 1), 256);
  const uint32_t SC = min((uint32_t)S * C, (uint32_t)DFA_MAX_TABLE);
  const int n = gen_len[b];
  const bool at_base = n == g_base[r] || n <= 0;
  const uint32_t slot_even = (uint32_t)g_state[2 * r] & 0xFFFFu, slot_odd = (uint32_t)g_state[2 * r + 1] & 0xFFFFu;
  const int in_tok = input_ids[b];

  const int tok0 = blockIdx.x * DFA_CHUNK + tid;
  int off[DFA_TPT], len[DFA_TPT];
  const int maxlen = dfa_tok_spans(V, tok_off, tok0, off, len);
  dfa_stage(trans, cls, r, SC, s_trans, s_cls, tid);
  // lazy advance, first half: the committed token's bytes, one per lane of the first half-wave
  int in_len = 0;
  if (!at_base && in_tok >= 0 && in_tok < V) {
    const int o = tok_off[in_tok], l = tok_off[in_tok + 1] - o;
    if (l >= 1 && l <= DFA_MAX_TOKEN_BYTES) {
      in_len = l;
      if (tid < l) s_in[tid] = tok_blob[o + tid];
    }
  }
  // the first byte of each of the thread's tokens, in flight across the barrier
  uint32_t byte[DFA_TPT];
#pragma unroll
  for (int j = 0; j < DFA_TPT; ++j) byte[j] = len[j] > 0 ? (uint32_t)tok_blob[off[j]] : 0u;
  __syncthreads();

  const DfaLds t{s_trans, s_cls, C, SC};

  // second half: every lane walks the same bytes (broadcast LDS reads), so cur needs no second barrier
  uint32_t cur;
  if (at_base) {
    cur = (n & 1) ? slot_odd : slot_even;
  } else {
    cur = in_len > 0 ? (((n - 1) & 1) ? slot_odd : slot_even) : DFA_DEAD;
    for (int i = 0; i < in_len; ++i) cur = t.step(cur, s_in[i]);
    if (blockIdx.x == 0 && tid == 0) g_state[2 * r + (n & 1)] = (int)cur;
  }
  // (consumed after the walk below, which hides this load)
  const bool eos_ok = cur == DFA_DEAD || (cur < (uint32_t)S && accept[(size_t)r * DFA_MAX_TABLE + cur] != 0);
  dfa_walk_mask(t, cur, eos_ok, logits + (size_t)b * V, V, tok0, tok_blob, off, len, maxlen, byte, eos, neos);
}

__global__ __launch_bounds__(256) void dfa_mask_verify_kernel(
    float* __restrict__ logits, int V, const int* __restrict__ tok_off, const uint8_t* __restrict__ tok_blob,
    const uint8_t* __restrict__ cls, const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept,
    const int* __restrict__ g_dim, const int* __restrict__ g_on, int* __restrict__ g_state,
    const int* __restrict__ g_base, int r, const int* __restrict__ gen_len, const int* __restrict__ input_ids,
    const int* __restrict__ finished, const int* __restrict__ eos, int neos, const int* __restrict__ draft,
    int* __restrict__ g_spec) {
  const int row = blockIdx.y, tid = threadIdx.x;  // verify row t = row: masked in the state after drafts 1..row
  const int T = gridDim.y, seq = blockIdx.z;      // sequence seq: state row seq, table row r + seq
  r += seq;
  if (g_on[r] == 0 || finished[seq] != 0) return;  // uniform per workgroup
  draft += seq * (T - 1);
  g_spec += 9 * seq;

  __shared__ __attribute__((aligned(16))) uint16_t s_trans[DFA_MAX_TABLE];
  __shared__ uint8_t s_cls[256];
  __shared__ uint8_t s_in[DFA_MAX_TOKEN_BYTES];                           // the input token's bytes
  __shared__ uint8_t s_dr[(DFA_MAX_VERIFY - 1) * DFA_MAX_TOKEN_BYTES];    // the bytes of drafts 1..row

  const int S = min(max(g_dim[2 * r], 0), DFA_MAX_TABLE);
  const uint32_t C = (uint32_t)min(max(g_dim[2 * r + 1], 1), 256);
  const uint32_t SC = min((uint32_t)S * C, (uint32_t)DFA_MAX_TABLE);
  const int n = gen_len[seq];
  const bool at_base = n == g_base[r] || n <= 0;
  const uint32_t slot_even = (uint32_t)g_state[2 * r] & 0xFFFFu, slot_odd = (uint32_t)g_state[2 * r + 1] & 0xFFFFu;
  const int in_tok = input_ids[seq];

  const int tok0 = blockIdx.x * DFA_CHUNK + tid;
  int off[DFA_TPT], len[DFA_TPT];
  const int maxlen = dfa_tok_spans(V, tok_off, tok0, off, len);
  dfa_stage(trans, cls, r, SC, s_trans, s_cls, tid);
  int in_len = 0;
  if (!at_base && in_tok >= 0 && in_tok < V) {
    const int o = tok_off[in_tok], l = tok_off[in_tok + 1] - o;
    if (l >= 1 && l <= DFA_MAX_TOKEN_BYTES) {
      in_len = l;
      if (tid < l) s_in[tid] = tok_blob[o + tid];
    }
  }
  // the drafts this row walks (uniform addresses); lane i of 32-lane group j parks byte i of draft j + 1.
  // d_len[j] == 0: no draft, an id outside [0, V), or a byte length outside 1..32 -- the state dies there
  int d_len[DFA_MAX_VERIFY - 1];
#pragma unroll
  for (int j = 0; j < DFA_MAX_VERIFY - 1; ++j) {
    d_len[j] = 0;
    if (j < row) {
      const int d = draft[j];
      if (d >= 0 && d < V) {
        const int o = tok_off[d], l = tok_off[d + 1] - o;
        if (l >= 1 && l <= DFA_MAX_TOKEN_BYTES) {
          d_len[j] = l;
          if ((tid >> 5) == j && (tid & 31) < l) s_dr[j * DFA_MAX_TOKEN_BYTES + (tid & 31)] = tok_blob[o + (tid & 31)];
        }
      }
    }
  }
  uint32_t byte[DFA_TPT];
#pragma unroll
  for (int j = 0; j < DFA_TPT; ++j) byte[j] = len[j] > 0 ? (uint32_t)tok_blob[off[j]] : 0u;
  __syncthreads();

  const DfaLds t{s_trans, s_cls, C, SC};
  const bool writer = blockIdx.x == 0 && tid == 0;

  uint32_t cur;  // s_0, by the plain kernel's lazy advance
  if (at_base) {
    cur = (n & 1) ? slot_odd : slot_even;
  } else {
    cur = in_len > 0 ? (((n - 1) & 1) ? slot_odd : slot_even) : DFA_DEAD;
    for (int i = 0; i < in_len; ++i) cur = t.step(cur, s_in[i]);
    if (writer && row == 0) g_state[2 * r + (n & 1)] = (int)cur;
  }
  // s_row: DEAD stays DEAD through step(), so one dead draft kills every later state
#pragma unroll
  for (int j = 0; j < DFA_MAX_VERIFY - 1; ++j) {
    if (j < row) {
      if (d_len[j] == 0) cur = DFA_DEAD;
      for (int i = 0; i < d_len[j]; ++i) cur = t.step(cur, s_dr[j * DFA_MAX_TOKEN_BYTES + i]);
    }
  }
  if (writer) {
    g_spec[1 + row] = (int)cur;
    if (row == 0) g_spec[0] = n;
  }
  const bool eos_ok = cur == DFA_DEAD || (cur < (uint32_t)S && accept[(size_t)r * DFA_MAX_TABLE + cur] != 0);
  dfa_walk_mask(t, cur, eos_ok, logits + ((size_t)seq * T + row) * V, V, tok0, tok_blob, off, len, maxlen, byte, eos,
                neos);
}

__global__ __launch_bounds__(64) void dfa_spec_advance_kernel(const int* __restrict__ g_on, int* __restrict__ g_state,
                                                              const int* __restrict__ g_spec,
                                                              const int* __restrict__ gen_len, int r, int k) {
  const int seq = blockIdx.x;  // sequence seq: gen_len[seq], g_spec row seq, table row r + seq
  r += seq;
  if (threadIdx.x != 0 || g_on[r] == 0) return;
  g_spec += 9 * seq;
  const int n1 = gen_len[seq], a = n1 - g_spec[0] - 1;
  if (a >= 0 && a <= k) g_state[2 * r + ((n1 - 1) & 1)] = g_spec[1 + a] & 0xFFFF;
}

extern "C" int lsa_dfa_mask(float* logits, int B, int V, const int* tok_off, const uint8_t* tok_blob,
                            const uint8_t* cls, const uint16_t* trans, const uint8_t* accept, const int* g_dim,
                            const int* g_on, int* g_state, const int* g_base, const int* rows, const int* gen_len,
                            const int* input_ids, const int* finished, const int* eos, int neos, hipStream_t s) {
  if (B < 1 || B > 65535 || V < 1 || neos < 0) return -1;
  hipLaunchKernelGGL(dfa_mask_kernel, dim3((V + DFA_CHUNK - 1) / DFA_CHUNK, B), dim3(256), 0, s, logits, V, tok_off,
                     tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, rows, gen_len, input_ids, finished,
                     eos, neos);
  return (int)hipGetLastError();
}

// logits [S * T, V]: the verify rows of the sequences in state rows 0 .. S - 1, table rows r .. r + S - 1; draft
// [S * (T - 1)]; g_spec [S, 1 + 8].  The callers have checked the sizes.
static int dfa_mask_verify_launch(float* logits, int S, int T, int V, const int* tok_off, const uint8_t* tok_blob,
                                  const uint8_t* cls, const uint16_t* trans, const uint8_t* accept, const int* g_dim,
                                  const int* g_on, int* g_state, const int* g_base, int r, const int* gen_len,
                                  const int* input_ids, const int* finished, const int* eos, int neos,
                                  const int* draft, int* g_spec, hipStream_t s) {
  hipLaunchKernelGGL(dfa_mask_verify_kernel, dim3((V + DFA_CHUNK - 1) / DFA_CHUNK, T, S), dim3(256), 0, s, logits, V,
                     tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, r, gen_len, input_ids,
                     finished, eos, neos, draft, g_spec);
  return (int)hipGetLastError();
}

// logits [T, V]: the verify rows of the sequence in state row 0, table row r; draft [T - 1]; g_spec [1 + 8].
extern "C" int lsa_dfa_mask_verify(float* logits, int T, int V, const int* tok_off, const uint8_t* tok_blob,
                                   const uint8_t* cls, const uint16_t* trans, const uint8_t* accept, const int* g_dim,
                                   const int* g_on, int* g_state, const int* g_base, int r, const int* gen_len,
                                   const int* input_ids, const int* finished, const int* eos, int neos,
                                   const int* draft, int* g_spec, hipStream_t s) {
  if (T < 2 || T > DFA_MAX_VERIFY || V < 1 || neos < 0 || r < 0) return -1;
  return dfa_mask_verify_launch(logits, 1, T, V, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, r,
                                gen_len, input_ids, finished, eos, neos, draft, g_spec, s);
}

// The form over S sequences (sequence s: state row s, table row r + s, logits rows s T .., drafts s (T - 1) .., g_spec
// row s).  Refused before any launch: S outside 1..8, T outside 2..8, S * T > 32.
extern "C" int lsa_dfa_mask_verify_batch(float* logits, int S, int T, int V, const int* tok_off,
                                         const uint8_t* tok_blob, const uint8_t* cls, const uint16_t* trans,
                                         const uint8_t* accept, const int* g_dim, const int* g_on, int* g_state,
                                         const int* g_base, int r, const int* gen_len, const int* input_ids,
                                         const int* finished, const int* eos, int neos, const int* draft, int* g_spec,
                                         hipStream_t s) {
  if (S < 1 || S > DFA_MAX_SEQS || T < 2 || T > DFA_MAX_VERIFY || S * T > DFA_MAX_ROWS || V < 1 || neos < 0 || r < 0) {
    return -1;
  }
  return dfa_mask_verify_launch(logits, S, T, V, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, r,
                                gen_len, input_ids, finished, eos, neos, draft, g_spec, s);
}

extern "C" int lsa_dfa_spec_advance(const int* g_on, int* g_state, const int* g_spec, const int* gen_len, int r, int k,
                                    hipStream_t s) {
  if (k < 1 || k > DFA_MAX_VERIFY - 1 || r < 0) return -1;
  hipLaunchKernelGGL(dfa_spec_advance_kernel, dim3(1), dim3(64), 0, s, g_on, g_state, g_spec, gen_len, r, k);
  return (int)hipGetLastError();
}

// The form over S sequences: g_spec [S, 1 + 8], gen_len [S], table rows r .. r + S - 1.
extern "C" int lsa_dfa_spec_advance_batch(const int* g_on, int* g_state, const int* g_spec, const int* gen_len, int r,
                                          int S, int k, hipStream_t s) {
  if (S < 1 || S > DFA_MAX_SEQS || k < 1 || k > DFA_MAX_VERIFY - 1 || S * (k + 1) > DFA_MAX_ROWS || r < 0) return -1;
  hipLaunchKernelGGL(dfa_spec_advance_kernel, dim3(S), dim3(64), 0, s, g_on, g_state, g_spec, gen_len, r, k);
  return (int)hipGetLastError();
}
