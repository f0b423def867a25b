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
#include "common.h"

#define DFA_DEAD 0xFFFFu
#define DFA_MAX_TABLE 32768
#define DFA_MAX_TOKEN_BYTES 32
#define DFA_CHUNK 2048
#define DFA_TPT 8  // tokens per thread

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
  {
    // rows of trans are 64 KiB apart, so 16-byte loads are aligned; the last one may run past S * C but stays
    // inside the row (S * C <= 32768 = the row length)
    const uint4* src = reinterpret_cast<const uint4*>(trans + (size_t)r * DFA_MAX_TABLE);
    uint4* dst = reinterpret_cast<uint4*>(s_trans);
    const int n16 = (int)((SC + 7u) >> 3);
    for (int i = tid; i < n16; i += 256) dst[i] = src[i];
    s_cls[tid] = cls[(size_t)r * 256 + tid];
  }
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

  auto step = [&](uint32_t s, uint32_t bt) -> uint32_t {
    const uint32_t idx = s * C + s_cls[bt];
    return idx < SC ? (uint32_t)s_trans[idx] : DFA_DEAD;  // s == DEAD lands past SC and stays DEAD
  };

  // second half: every lane walks the same bytes (broadcast LDS reads), so cur needs no second barrier
  uint32_t cur;
  if (at_base) {
    cur = (n & 1) ? slot_odd : slot_even;
  } else {
    cur = in_len > 0 ? (((n - 1) & 1) ? slot_odd : slot_even) : DFA_DEAD;
    for (int i = 0; i < in_len; ++i) cur = step(cur, s_in[i]);
    if (blockIdx.x == 0 && tid == 0) g_state[2 * r + (n & 1)] = (int)cur;
  }
  // (consumed after the walk below, which hides this load)
  const bool eos_ok = cur == DFA_DEAD || (cur < (uint32_t)S && accept[(size_t)r * DFA_MAX_TABLE + cur] != 0);

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
      if (i < len[j] && st[j] != DFA_DEAD) st[j] = step(st[j], byte[j]);
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
    if (!allowed) logits[(size_t)b * V + tok] = -INFINITY;
  }
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
