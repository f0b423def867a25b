"""Plain-PyTorch fp32 reference of every fused op in ``csrc/kernels`` (the numerics oracle).

Each function here has exactly the signature and in-place semantics of its HIP counterpart in
``ops/__init__.py`` so that (a) the GPU tests compare the kernel against this file op-by-op and (b) the
whole engine can step on CPU for the CPU-only test suite.  Nothing here is used on a GPU tensor in
production: ``ops`` refuses to fall back when the extension is missing on a GPU box.
"""
from __future__ import annotations

import contextlib
import math
import struct

import torch

BLOCK = 64  # tokens per KV-cache block (kernels assume 64)


# Row-stable host prefill (``row_stable``): torch's CPU matmul sums a row's products in an order that depends on how
# many rows the call has (below about 16 rows it takes another path), so a prompt's residual rows differ in their last
# bits with the packing and the chunking of the call.  While the flag is set, ``linear`` multiplies one row at a time and
# ``attn_prefill`` attends one query row at a time over exactly the keys it sees: every row is then computed by calls
# whose shapes depend on that row alone.  The host prefill sets it for calls that pool embeddings (engine/runner.py),
# whose vectors are then the same bits alone, packed or chunked; no other call changes.
_ROW_STABLE = False


@contextlib.contextmanager
def row_stable(on: bool = True):
    global _ROW_STABLE
    old, _ROW_STABLE = _ROW_STABLE, bool(on) or _ROW_STABLE
    try:
        yield
    finally:
        _ROW_STABLE = old


def linear(x: torch.Tensor, w: torch.Tensor, epi: str = "bf16", splitk: int = 1) -> torch.Tensor:
    """x [M,K] @ w[N,K]^T.  epi: bf16 | f32 | silu (w rows interleaved gate/up per 16)."""
    if _ROW_STABLE:
        xf, wt = x.float(), w.float().t()
        y = torch.cat([xf[i:i + 1] @ wt for i in range(xf.shape[0])]) if xf.shape[0] else xf @ wt
    else:
        y = x.float() @ w.float().t()
    if epi == "f32":
        return y
    if epi == "silu":
        M, N = y.shape
        y4 = y.view(M, N // 32, 2, 16)
        g, u = y4[:, :, 0, :].reshape(M, N // 2), y4[:, :, 1, :].reshape(M, N // 2)
        return (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
    return y.to(torch.bfloat16)


def slab_sum(v: torch.Tensor, parts) -> torch.Tensor:
    """v + parts[0] + parts[1] + ... in f32, left to right: the order in which every kernel that consumes split-K slabs
    adds them (``torch.sum`` promises no order), so the host paths reproduce the residual stream bit for bit."""
    for s in range(parts.shape[0]):
        v = v + parts[s].float()
    return v


def add_rmsnorm_f32(h, w, eps, rows, parts=None, ids=None, emb=None, row_idx=None, write_h=True):
    """The f32 rows of ``add_rmsnorm`` before their rounding to bf16 (what the kernel quantises for its fp8 output)."""
    idx = row_idx.long() if row_idx is not None else torch.arange(rows, device=h.device)
    if ids is not None:
        v = emb[ids.long()[idx]].float()
    else:
        v = h[idx].float()
    if parts is not None:
        v = slab_sum(v, parts[:, idx])
    if write_h:
        h[idx] = v
    inv = torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return v * inv * w.float()


def add_rmsnorm(h, w, eps, xn, parts=None, ids=None, emb=None, row_idx=None, write_h=True):
    xn.copy_(add_rmsnorm_f32(h, w, eps, xn.shape[0], parts, ids, emb, row_idx, write_h).to(torch.bfloat16))
    return xn


def rope_tables(head_dim: int, max_pos: int, theta: float, scaling: dict | None = None, device="cpu"):
    """cos/sin [max_pos, head_dim/2] f32 with optional llama3 frequency scaling."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling["low_freq_factor"], scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = (wl >= hi_wl) & (wl <= lo_wl)
        inv = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def _slots(pos, tok_seq, block_tables):
    seq = tok_seq.long() if tok_seq is not None else torch.arange(pos.shape[0], device=pos.device)
    p = pos.long()
    blk = block_tables.long()[seq, p // BLOCK]
    return blk, p % BLOCK


# fp8 KV cache rows (csrc/kernels/common.h kv8_inv / LSA_KV8_RMAX): e4m3(x * (448 / amax)) with scale amax * (1/448)
KV8_RMAX = torch.tensor(1.0 / 448.0, dtype=torch.float32)


def quant_kv_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x f32 [..., 128] -> (e4m3 bytes as uint8 [..., 128], f32 scales [...]) per row of 128 values."""
    x = x.float()
    a = x.abs().amax(-1)
    inv = torch.where(a > 0, torch.tensor(448.0, dtype=torch.float32, device=x.device) / a.clamp_min(1e-38),
                      torch.zeros_like(a))
    q = (x * inv.unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, a * KV8_RMAX.to(x.device)


def dequant_kv_rows(q: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).float() * sc.float().unsqueeze(-1)


# The fp8 cache tensors keep the [.., 64 tokens, 128] shape but store each (block, kv-head) tile in token-pair order
# (csrc/kernels/common.h kv8_off): the 8-byte chunk c of tokens 2p and 2p + 1 side by side, so one 16-byte lane load
# in decode attention carries two keys.  Scales stay in token order.
def kv8_physical(logical: torch.Tensor) -> torch.Tensor:
    """token-order e4m3 bytes [..., 64, 128] -> the cache's token-pair order (same shape)."""
    sh = logical.shape
    return logical.reshape(*sh[:-2], 32, 2, 16, 8).transpose(-3, -2).reshape(sh)


def kv8_logical(physical: torch.Tensor) -> torch.Tensor:
    """the cache's token-pair order [..., 64, 128] -> token-order e4m3 bytes (same shape)."""
    sh = physical.shape
    return physical.reshape(*sh[:-2], 32, 16, 2, 8).transpose(-3, -2).reshape(sh)


def rope_append(qkv, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv, kv_scales=None):
    if qkv.dtype == torch.float32 and qkv.dim() == 3:  # f32 split-K slabs [S, T, n]
        qkv = slab_sum(qkv[0], qkv[1:])
    T = qkv.shape[0]
    D = 128
    x = qkv.float().view(T, H + 2 * Hkv, D)
    p = pos.long()
    c = cos_t[p].unsqueeze(1)
    s = sin_t[p].unsqueeze(1)
    qk = x[:, : H + Hkv]
    lo, hi = qk[..., :64], qk[..., 64:]
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)
    q_out.copy_(rot[:, :H].to(torch.bfloat16).view_as(q_out))
    blk, off = _slots(pos, tok_seq, block_tables)
    if kv_scales is not None:  # fp8 cache: quantise each (token, kv-head) row
        ks, vs = kv_scales
        k8, ksc = quant_kv_rows(rot[:, H:])
        v8, vsc = quant_kv_rows(x[:, H + Hkv:])
        ub = blk.unique()
        idx = torch.searchsorted(ub, blk)
        for cache, rows in ((kc, k8), (vc, v8)):
            tiles = kv8_logical(cache[ub])
            tiles[idx, :, off] = rows
            cache[ub] = kv8_physical(tiles)
        ks[blk, :, off] = ksc
        vs[blk, :, off] = vsc
        return
    kc[blk, :, off] = rot[:, H:].to(kc.dtype)
    vc[blk, :, off] = x[:, H + Hkv:].to(vc.dtype)


def _gather_kv(cache, table_row, n, scales=None):
    nb = (n + BLOCK - 1) // BLOCK
    blocks = cache[table_row[:nb].long()]  # [nb, Hkv, 64, D]
    if scales is not None:
        blocks = dequant_kv_rows(kv8_logical(blocks), scales[table_row[:nb].long()])
    return blocks.permute(1, 0, 2, 3).reshape(cache.shape[1], nb * BLOCK, cache.shape[3])[:, :n]


def attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, out, kv_scales=None):
    B = pos.shape[0]
    G = H // Hkv
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    for b in range(B):
        n = int(pos[b]) + 1
        k = _gather_kv(kc, block_tables[b], n, ks).float().repeat_interleave(G, 0)
        v = _gather_kv(vc, block_tables[b], n, vs).float().repeat_interleave(G, 0)
        s = torch.einsum("hd,hnd->hn", q[b].float(), k) * scale
        o = torch.einsum("hn,hnd->hd", s.softmax(-1), v)
        out[b] = o.to(out.dtype).view_as(out[b])
    return out


def attn_prefill(q, kc, vc, block_tables, cu_q, ctx_lens, H, Hkv, scale, out, kv_scales=None):
    G = H // Hkv
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    cu = cu_q.tolist()
    for sq in range(len(cu) - 1):
        q0, q1 = cu[sq], cu[sq + 1]
        ql = q1 - q0
        if ql == 0:
            continue
        n = int(ctx_lens[sq])
        k = _gather_kv(kc, block_tables[sq], n, ks).float().repeat_interleave(G, 0)
        v = _gather_kv(vc, block_tables[sq], n, vs).float().repeat_interleave(G, 0)
        qq = q[q0:q1].float().transpose(0, 1)  # [H, ql, D]
        if _ROW_STABLE:  # one query row at a time over exactly its n - ql + r + 1 keys
            for r in range(ql):
                m = n - ql + r + 1
                p = (torch.einsum("hqd,hnd->hqn", qq[:, r:r + 1], k[:, :m]) * scale).softmax(-1)
                o = torch.einsum("hqn,hnd->hqd", p, v[:, :m])
                out[q0 + r] = o[:, 0].to(out.dtype).view_as(out[q0 + r])
            continue
        s = torch.einsum("hqd,hnd->hqn", qq, k) * scale
        qpos = torch.arange(n - ql, n, device=q.device).view(ql, 1)
        kpos = torch.arange(n, device=q.device).view(1, n)
        s = s.masked_fill(kpos > qpos, float("-inf"))
        o = torch.einsum("hqn,hnd->hqd", s.softmax(-1), v)
        out[q0:q1] = o.transpose(0, 1).to(out.dtype).view_as(out[q0:q1])
    return out


# fp64 attention with its componentwise error scale, for the elementwise tests (tests/attn_exact.py): next to the output
# o = sum_j p_j v_j every function returns a = sum_j p_j |v_j| per (row, head, column).  A kernel that rounds P, the row
# sum or the output to bf16 is off by a small multiple of 2^-9 a in EVERY element, whatever cancels in o; a wrong or
# missing key is off by about p_j |v_j|, which the whole-tensor norm ratio does not see.  fp8 caches: over the
# dequantised cache (e4m3 value times the f32 row scale, exact in fp64).
def _attn_rows_f64(q, k, v, scale, limits):
    """q [H, R, D], k / v [H, n, D] (fp64); row r sees keys j < limits[r] -> (o, a) [R, H, D]."""
    s = torch.einsum("hrd,hnd->hrn", q, k) * scale
    hidden = torch.arange(k.shape[1], device=q.device).view(1, -1) >= limits.view(-1, 1)
    p = s.masked_fill(hidden, float("-inf")).softmax(-1)
    return (torch.einsum("hrn,hnd->rhd", p, v), torch.einsum("hrn,hnd->rhd", p, v.abs()))


def _gather_kv_f64(cache, table_row, n, scales, G):
    if scales is None:
        return _gather_kv(cache, table_row, n).double().repeat_interleave(G, 0)
    nb = (n + BLOCK - 1) // BLOCK
    idx = table_row[:nb].long()
    blocks = kv8_logical(cache[idx]).view(torch.float8_e4m3fn).double() * scales[idx].double().unsqueeze(-1)
    return blocks.permute(1, 0, 2, 3).reshape(cache.shape[1], nb * BLOCK, cache.shape[3])[:, :n].repeat_interleave(G, 0)


def attn_decode_f64(q, kc, vc, block_tables, pos, H, Hkv, scale, kv_scales=None):
    """``attn_decode`` in fp64 -> (o, a), both [B, H, D] float64."""
    B, G = pos.shape[0], H // Hkv
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    o = torch.zeros(B, H, q.shape[-1], dtype=torch.float64, device=q.device)
    a = torch.zeros_like(o)
    for b in range(B):
        n = int(pos[b]) + 1
        k = _gather_kv_f64(kc, block_tables[b], n, ks, G)
        v = _gather_kv_f64(vc, block_tables[b], n, vs, G)
        ob, ab = _attn_rows_f64(q[b].double().view(H, 1, -1), k, v, scale, torch.tensor([n], device=q.device))
        o[b], a[b] = ob[0], ab[0]
    return o, a


def attn_prefill_f64(q, kc, vc, block_tables, cu_q, ctx_lens, H, Hkv, scale, kv_scales=None):
    """``attn_prefill`` in fp64 -> (o, a), both [T, H, D] float64 (rows of a zero-length sequence: none)."""
    G = H // Hkv
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    o = torch.zeros(q.shape[0], H, q.shape[-1], dtype=torch.float64, device=q.device)
    a = torch.zeros_like(o)
    cu = cu_q.tolist()
    for sq in range(len(cu) - 1):
        q0, q1 = cu[sq], cu[sq + 1]
        if q1 == q0:
            continue
        n = int(ctx_lens[sq])
        k = _gather_kv_f64(kc, block_tables[sq], n, ks, G)
        v = _gather_kv_f64(vc, block_tables[sq], n, vs, G)
        limits = torch.arange(n - (q1 - q0), n, device=q.device) + 1
        o[q0:q1], a[q0:q1] = _attn_rows_f64(q[q0:q1].double().transpose(0, 1), k, v, scale, limits)
    return o, a


def attn_verify_f64(q, kc, vc, block_table, pos0, H, Hkv, scale, kv_scales=None):
    """``attn_verify`` in fp64 -> (o, a), both [S * T, H, D] float64."""
    S, T = (q.shape[0], q.shape[1]) if q.dim() == 4 else (1, q.shape[0])
    G = H // Hkv
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    qs = q.reshape(S, T, H, -1)
    o = torch.zeros(S * T, H, q.shape[-1], dtype=torch.float64, device=q.device)
    a = torch.zeros_like(o)
    for s in range(S):
        p0 = int(pos0.reshape(-1)[s])
        row = block_table.reshape(S, -1)[s]
        k = _gather_kv_f64(kc, row, p0 + T, ks, G)
        v = _gather_kv_f64(vc, row, p0 + T, vs, G)
        limits = torch.arange(p0, p0 + T, device=q.device) + 1
        o[s * T:(s + 1) * T], a[s * T:(s + 1) * T] = _attn_rows_f64(qs[s].double().transpose(0, 1), k, v, scale, limits)
    return o, a


def commit(tok, out_tokens, gen_len, input_ids, positions, finished, eos, limit=None, eos_on=None, hist=None):
    eos_set = set(eos.tolist()) if eos is not None else set()
    max_new = out_tokens.shape[1]
    for b in range(tok.shape[0]):
        if int(finished[b]):
            continue
        n = int(gen_len[b])
        t = int(tok[b])
        if n < max_new:
            out_tokens[b, n] = t
        gen_len[b] = n + 1
        input_ids[b] = t
        if hist is not None:  # position-indexed ring of the context's last tokens
            hist[b, (int(positions[b]) + 1) % hist.shape[1]] = t
        lim = min(max_new, int(limit[b])) if limit is not None else max_new
        use_eos = bool(int(eos_on[b])) if eos_on is not None else True
        if n + 1 >= lim or (use_eos and t in eos_set):
            finished[b] = 1
        else:
            positions[b] += 1


def argmax_commit(logits, out_tokens, gen_len, input_ids, positions, finished, eos, limit=None, eos_on=None):
    commit(logits.float().argmax(-1), out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on)


# ----------------------------------------------------------------------------------- per-token logprobs
LOGPROB_KMAX = 20
LOGPROB_VMAX = 262144


def logprob_rows(logits, tok, k: int):
    """The model's own log-probabilities of rows ``logits`` [R, V]: the float64 log-softmax over the whole row of the
    logits as given (raw: no mask, penalty or temperature), rounded once to f32.

    -> (lp f32 [R]: that of ``tok[r]``; ids int32 [R, k], top f32 [R, k]: the k most likely tokens by (value
    descending, index ascending) with theirs; entries beyond V are id -1 and -inf)."""
    R, V = logits.shape
    lp = torch.log_softmax(logits.double(), dim=-1)
    t = torch.as_tensor(tok, dtype=torch.int64, device=logits.device).reshape(R, 1)
    chosen = lp.gather(1, t).reshape(R).float()
    ids = torch.full((R, k), -1, dtype=torch.int32, device=logits.device)
    top = torch.full((R, k), float("-inf"), dtype=torch.float32, device=logits.device)
    kk = min(k, V)
    if kk > 0:
        order = torch.sort(logits.float(), dim=-1, descending=True, stable=True).indices[:, :kk]
        ids[:, :kk] = order.int()
        top[:, :kk] = lp.gather(1, order).float()
    return chosen, ids, top


def logprob_scan(logits, lp_k, finished, gen_len, lp_raw, lp_n0):
    """Host twin of kernels/logprobs.hip logprob_scan_kernel (state level): a row b that asked (``lp_k[b] >= 0``) and
    is not finished keeps its raw row in ``lp_raw[b]`` and n0 = gen_len[b] in ``lp_n0[b]``; a finished row that asked
    gets ``lp_n0[b] = -1`` (no record this step); a row that did not ask is left alone.  ``logits`` is not modified."""
    for b in range(logits.shape[0]):
        if int(lp_k[b]) < 0:
            continue
        if int(finished[b]) != 0:
            lp_n0[b] = -1
            continue
        lp_raw[b].copy_(logits[b])
        lp_n0[b] = int(gen_len[b])


def logprob_commit(lp_raw, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, B: int):
    """Host twin of logprob_commit_kernel, after the token commit of the step.  Row b records exactly when it asked,
    ``lp_n0[b]`` was written by this step's scan (>= 0; it is consumed: set to -1) and ``gen_len[b] == n0 + 1``, at
    index n0 < max_new: ``lp_tok[b, n0]`` and, for K = min(lp_k[b], lp_ids.shape[2]) > 0, ``lp_ids / lp_top[b, n0, :K]``
    (``logprob_rows`` of the raw row and ``out_tokens[b, n0]``).  Nothing else is written."""
    max_new = out_tokens.shape[1]
    for b in range(B):
        K = int(lp_k[b])
        n0 = int(lp_n0[b])
        if K < 0 or n0 < 0:
            continue
        lp_n0[b] = -1
        if int(gen_len[b]) != n0 + 1 or n0 >= max_new:
            continue
        K = min(K, lp_ids.shape[2])
        chosen, ids, top = logprob_rows(lp_raw[b:b + 1], out_tokens[b:b + 1, n0], K)
        lp_tok[b, n0] = chosen[0]
        if K > 0:
            lp_ids[b, n0, :K] = ids[0]
            lp_top[b, n0, :K] = top[0]


LOGPROB_SPEC_ROWS = 32  # the rows of the spec-side raw buffer and chunk workspace: S * T <= 32


def spec_logprob_scan(logits, T: int, lp_k, finished, gen_len, lp_n0, sp_raw):
    """Host twin of spec_logprob_scan_kernel (state level), over the S = len(lp_k) sequences of a verify step with T
    rows each (``logits`` [S * T, V]): a sequence s that asked and is not finished keeps its T raw rows in
    ``sp_raw[s T .. s T + T - 1]`` (the spec-side buffer of 32 rows, not the per-slot ``lp_raw``) and n0 = gen_len[s]
    in ``lp_n0[s]``; a finished sequence that asked gets ``lp_n0[s] = -1``; one that did not ask is left alone."""
    for s in range(lp_k.shape[0]):
        if int(lp_k[s]) < 0:
            continue
        if int(finished[s]) != 0:
            lp_n0[s] = -1
            continue
        sp_raw[s * T:(s + 1) * T].copy_(logits[s * T:(s + 1) * T])
        lp_n0[s] = int(gen_len[s])


def spec_logprob_commit(T: int, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, sp_raw):
    """Host twin of spec_logprob_commit_kernel, after the verify commit.  Sequence s records exactly when it asked and
    ``lp_n0[s]`` = n0 >= 0: with c = gen_len[s] - n0 the tokens this step committed (0 .. T, already cut by EOS and the
    limit), for t < min(c, T) and n0 + t < max_new, index n0 + t gets ``logprob_rows`` of verify row s T + t (the
    distribution of generated token n0 + t: row 0 follows the input token, row t draft t) and ``out_tokens[s, n0 + t]``,
    K = min(lp_k[s], lp_ids.shape[2]).  Nothing else is written.

    Invariant: ``lp_n0`` is NOT consumed (on the device T workgroups read it).  It need not be: every step in which a
    row asks rewrites ``lp_n0`` in its scan (n0, or -1 for a finished row), the verify scan and the plain scan alike."""
    max_new = out_tokens.shape[1]
    for s in range(lp_k.shape[0]):
        K = int(lp_k[s])
        n0 = int(lp_n0[s])
        if K < 0 or n0 < 0:
            continue
        K = min(K, lp_ids.shape[2])
        c = int(gen_len[s]) - n0
        for t in range(min(c, T)):
            n = n0 + t
            if n >= max_new:
                break
            r = s * T + t
            chosen, ids, top = logprob_rows(sp_raw[r:r + 1], out_tokens[s:s + 1, n], K)
            lp_tok[s, n] = chosen[0]
            if K > 0:
                lp_ids[s, n, :K] = ids[0]
                lp_top[s, n, :K] = top[0]


def prompt_logprob_scan(logits, targets, row_k):
    """Host twin of prompt_logprob_scan_kernel (state level): the scan of scored prefill rows keeps nothing but chunk
    partials the commit reads, so on the host it is the statement that ``logits`` is not modified."""
    return None


def prompt_logprob_commit(logits, targets, row_k, dst_tok, dst_ids, dst_top):
    """Host twin of prompt_logprob_commit_kernel.  Row r of ``logits`` [R, V] records exactly when it has a target
    (``targets[r] >= 0``): ``dst_tok[r]`` and, for K = min(row_k[r], dst_ids.shape[1]) > 0, ``dst_ids / dst_top
    [r, :K]`` -- ``logprob_rows`` of the row as it stands and ``targets[r]``, the rule of a generated-token record.
    Nothing else is written."""
    for r in range(logits.shape[0]):
        tok = int(targets[r])
        if tok < 0:
            continue
        K = max(0, min(int(row_k[r]), dst_ids.shape[1]))
        chosen, ids, top = logprob_rows(logits[r:r + 1], [tok], K)
        dst_tok[r] = chosen[0]
        if K > 0:
            dst_ids[r, :K] = ids[0]
            dst_top[r, :K] = top[0]


# ----------------------------------------------------------------------------------- regex-constrained decoding
DFA_DEAD = 0xFFFF
DFA_MAX_TABLE = 32768
DFA_MAX_TOKEN_BYTES = 32


def dfa_mask(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len, input_ids,
             finished, eos, rows=None):
    """Host twin of csrc/kernels/guided.hip.  Per row b of ``logits`` [B, V] (table row r = rows[b], or b):

    * nothing happens when ``g_on[r] == 0`` or ``finished[b]``;
    * the DFA state after n = gen_len[b] tokens is ``cur = g_state[r, n & 1]`` when n == g_base[r] (written at
      admission), else the walk of input_ids[b]'s bytes from ``g_state[r, (n - 1) & 1]``, stored to slot n & 1;
    * token t stays when its 1..32 bytes walk from ``cur`` to a state other than DEAD; an id of ``eos`` stays when
      ``accept[r, cur]`` (or when cur is DEAD: the row can only stop); every other logit becomes -inf.

    Tables: tok_off int32 [V + 1] / tok_blob uint8 (CSR token bytes), cls uint8 [Bmax, 256], trans int16 [Bmax, 32768]
    (the u16 table's bits), accept uint8 [Bmax, 32768], g_dim int32 [Bmax, 2] = (S, C), g_state int32 [Bmax, 2]."""
    B, V = logits.shape
    tk = _dfa_tokens(V, tok_off, tok_blob, eos)
    for b in range(B):
        r = b if rows is None else int(rows[b])
        if int(g_on[r]) == 0 or int(finished[b]) != 0:
            continue
        tab = _DfaRow(r, cls, trans, accept, g_dim)
        cur = _dfa_lazy_advance(tab, tk, g_state, g_base, int(gen_len[b]), int(input_ids[b]))
        _dfa_mask_row(logits[b], tab, tk, cur)


def _dfa_tokens(V, tok_off, tok_blob, eos):
    """(V, off, lens, blob, eos ids) of the CSR token byte table, on the host."""
    off = tok_off.to(torch.int64).cpu()
    lens = off[1:V + 1] - off[:V]
    blob = tok_blob.cpu().to(torch.int64)
    eos_ids = [int(e) for e in eos.reshape(-1).tolist() if 0 <= int(e) < V]
    return V, off, lens, blob, eos_ids


class _DfaRow:
    """Table row r: ``step`` is one transition, vectorised over tokens; s == DEAD stays DEAD."""

    def __init__(self, r, cls, trans, accept, g_dim):
        self.r, self.accept = r, accept
        self.S, self.C = int(g_dim[r, 0]), int(g_dim[r, 1])
        self.SC = min(max(self.S * self.C, 0), DFA_MAX_TABLE)
        self.tr = trans[r].cpu().to(torch.int64) & 0xFFFF
        self.cl = cls[r].cpu().to(torch.int64)

    def step(self, s, byte):
        idx = s * self.C + self.cl[byte]
        ok = (s != DFA_DEAD) & (idx < self.SC)
        return torch.where(ok, self.tr[idx.clamp(0, DFA_MAX_TABLE - 1)], torch.full_like(s, DFA_DEAD))

    def walk_token(self, tk, s, t):
        """The state after token t's bytes from state s; DEAD for an id outside [0, V) or of 0 / more than 32 bytes."""
        V, off, lens, blob, _ = tk
        if not (0 <= t < V and 1 <= int(lens[t]) <= DFA_MAX_TOKEN_BYTES):
            return DFA_DEAD
        s = torch.tensor([int(s) & 0xFFFF])
        for i in range(int(lens[t])):
            s = self.step(s, blob[int(off[t]) + i].reshape(1))
        return int(s)


def _dfa_lazy_advance(tab, tk, g_state, g_base, n, t):
    """cur after n generated tokens: slot n & 1 at the base, else the walk of token t from slot (n - 1) & 1, stored."""
    r = tab.r
    if n == int(g_base[r]) or n <= 0:
        return int(g_state[r, n & 1]) & 0xFFFF
    cur = tab.walk_token(tk, int(g_state[r, (n - 1) & 1]), t)
    g_state[r, n & 1] = cur
    return cur


def _dfa_mask_row(row, tab, tk, cur):
    """-inf into every logit of ``row`` [V] that the state ``cur`` rules out."""
    V, off, lens, blob, eos_ids = tk
    nb = max(1, blob.numel())
    ok_len = (lens >= 1) & (lens <= DFA_MAX_TOKEN_BYTES)
    s = torch.full((V,), cur, dtype=torch.int64)
    for i in range(int(lens[ok_len].max()) if bool(ok_len.any()) else 0):
        act = ok_len & (lens > i)
        byte = blob[(off[:V] + i).clamp(max=nb - 1)] if blob.numel() else torch.zeros(V, dtype=torch.int64)
        s = torch.where(act, tab.step(s, byte), s)
    allowed = ok_len & (s != DFA_DEAD)
    eos_ok = cur == DFA_DEAD or (cur < tab.S and int(tab.accept[tab.r, cur]) != 0)
    for e in eos_ids:
        allowed[e] = eos_ok
    row[~allowed.to(row.device)] = float("-inf")


def dfa_mask_verify(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len, input_ids,
                    finished, eos, draft, g_spec, r=0):
    """Host twin of dfa_mask_verify_kernel: ``logits`` [T, V] are the verify rows of the sequence in state row 0 (table
    row r).  Nothing happens when ``g_on[r] == 0`` or ``finished[0]``.  s_0 is ``dfa_mask``'s lazily advanced state
    (stored to slot n & 1 away from the base); s_t = walk(s_{t-1}, bytes(draft[t - 1])), DEAD -- and every later state
    with it -- when the draft is -1, outside [0, V), of 0 or more than 32 bytes, or kills the walk.  Row t is masked as
    ``dfa_mask`` masks a row in state s_t.  g_spec[0] = n = gen_len[0], g_spec[1 + t] = s_t."""
    T, V = logits.shape
    if int(g_on[r]) == 0 or int(finished[0]) != 0:
        return
    tk = _dfa_tokens(V, tok_off, tok_blob, eos)
    tab = _DfaRow(r, cls, trans, accept, g_dim)
    n = int(gen_len[0])
    cur = _dfa_lazy_advance(tab, tk, g_state, g_base, n, int(input_ids[0]))
    g_spec[0] = n
    for t in range(T):
        if t:
            cur = tab.walk_token(tk, cur, int(draft[t - 1])) if cur != DFA_DEAD else DFA_DEAD
        g_spec[1 + t] = cur
        _dfa_mask_row(logits[t], tab, tk, cur)


def dfa_spec_advance(g_on, g_state, g_spec, gen_len, k, r=0):
    """Host twin of dfa_spec_advance_kernel (after ``spec_commit``): a = gen_len[0] - g_spec[0] - 1 accepted drafts;
    with g_on[r] set and 0 <= a <= k, g_state[r, (gen_len[0] - 1) & 1] = g_spec[1 + a]."""
    if int(g_on[r]) == 0:
        return
    n1 = int(gen_len[0])
    a = n1 - int(g_spec[0]) - 1
    if 0 <= a <= k:
        g_state[r, (n1 - 1) & 1] = int(g_spec[1 + a]) & 0xFFFF


def dfa_mask_verify_batch(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len,
                          input_ids, finished, eos, draft, g_spec, r=0):
    """Host twin of dfa_mask_verify_kernel over S = g_spec.shape[0] sequences: ``logits`` [S * T, V], ``draft`` [S * k],
    ``g_spec`` [S, 1 + 8].  Sequence s is one application of ``dfa_mask_verify`` -- the single statement of the rule --
    to its own slices: state row s, table row r + s, logits rows s T .. s T + T - 1, drafts s k .. s k + k - 1 and
    g_spec[s].  An unconstrained (g_on[r + s] == 0) or finished sequence is left as it is, with its g_spec row."""
    S = g_spec.shape[0]
    T = logits.shape[0] // S
    for s in range(S):
        dfa_mask_verify(logits[s * T:(s + 1) * T], tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base,
                        gen_len[s:s + 1], input_ids[s:s + 1], finished[s:s + 1], eos, draft[s * (T - 1):(s + 1) * (T - 1)],
                        g_spec[s], r + s)


def dfa_spec_advance_batch(g_on, g_state, g_spec, gen_len, k, r=0):
    """Host twin of dfa_spec_advance_kernel over S = g_spec.shape[0] sequences: ``dfa_spec_advance`` of sequence s on
    gen_len[s], g_spec[s] and table row r + s."""
    for s in range(g_spec.shape[0]):
        dfa_spec_advance(g_on, g_state, g_spec[s], gen_len[s:s + 1], k, r + s)


# ----------------------------------------------------------------------------------- prefix cache
def kv_copy_blocks(kv, kv_scale, pairs):
    """Copy the whole KV block src to dst, with its scales, in every layer for K and V (csrc/kernels/kv_copy.hip);
    kv [L, 2, NB, Hkv, 64, D], kv_scale [L, 2, NB, Hkv, 64] or None, pairs a validated list of (src, dst)."""
    if not pairs:
        return
    src = torch.tensor([s for s, _ in pairs], dtype=torch.long, device=kv.device)
    dst = torch.tensor([d for _, d in pairs], dtype=torch.long, device=kv.device)
    kv.index_copy_(2, dst, kv.index_select(2, src))
    if kv_scale is not None:
        kv_scale.index_copy_(2, dst, kv_scale.index_select(2, src))


# ----------------------------------------------------------------------------------- context shift
def kv_shift(kv, kv_scale, moves, cos_t, sin_t):
    """Host twin of kv_shift_kernel (csrc/kernels/kv_shift.hip) and its oracle; kv [L, 2, NB, Hkv, 64, 128] bf16,
    moves a validated list of (src, dst, row_lo, row_hi, delta), cos_t / sin_t the f32 RoPE tables [rows, 64].  For
    every layer and KV head, rows row_lo <= r < row_hi: K row r of dst = K row r of src rotated by -delta (the pair
    is (i, i + 64): lo' = lo*c + hi*s, hi' = hi*c - lo*s with c, s = cos_t / sin_t[delta, i], in f32 with each
    product and sum rounded on its own, then one rounding to bf16; delta 0 is a copy), V row r of dst = V row r of
    src when src != dst; the V of an in-place move is not touched."""
    assert kv_scale is None
    for src, dst, lo, hi, delta in moves:
        if hi <= lo:
            continue
        k = kv[:, 0, src, :, lo:hi]
        if delta == 0:
            if src != dst:
                kv[:, 0, dst, :, lo:hi] = k
        else:
            x, y = k[..., :64].float(), k[..., 64:].float()
            c, s = cos_t[delta].float(), sin_t[delta].float()
            kv[:, 0, dst, :, lo:hi] = torch.cat([x * c + y * s, y * c - x * s], dim=-1).to(kv.dtype)
        if src != dst:
            kv[:, 1, dst, :, lo:hi] = kv[:, 1, src, :, lo:hi]


def kv_shift8(kv, kv_scale, moves, cos_t, sin_t):
    """Host twin of kv_shift8_kernel (csrc/kernels/kv_shift.hip) and its oracle: ``kv_shift`` on the fp8 cache, kv
    [L, 2, NB, Hkv, 64, 128] uint8 with every tile in token-pair order, kv_scale [L, 2, NB, Hkv, 64] f32.  A K row
    with delta > 0 is dequantised, rotated in f32 as in ``kv_shift`` and quantised again (``quant_kv_rows``), which
    gives it a new scale; V rows and delta-0 K rows are copied with their scales when src != dst, and not touched
    when src == dst."""
    for src, dst, lo, hi, delta in moves:
        if hi <= lo:
            continue
        planes = ([0] if delta == 0 else []) + [1]
        if delta:
            k = dequant_kv_rows(kv8_logical(kv[:, 0, src])[:, :, lo:hi], kv_scale[:, 0, src, :, lo:hi])
            x, y = k[..., :64], k[..., 64:]
            c, s = cos_t[delta].float(), sin_t[delta].float()
            q, sc = quant_kv_rows(torch.cat([x * c + y * s, y * c - x * s], dim=-1))
            tile = kv8_logical(kv[:, 0, dst]).clone()
            tile[:, :, lo:hi] = q
            kv[:, 0, dst] = kv8_physical(tile)
            kv_scale[:, 0, dst, :, lo:hi] = sc
        if src != dst:
            for pl in planes:
                tile = kv8_logical(kv[:, pl, dst]).clone()
                tile[:, :, lo:hi] = kv8_logical(kv[:, pl, src])[:, :, lo:hi]
                kv[:, pl, dst] = kv8_physical(tile)
                kv_scale[:, pl, dst, :, lo:hi] = kv_scale[:, pl, src, :, lo:hi]


# ----------------------------------------------------------------------------------- embeddings
EMBED_NONE, EMBED_MEAN, EMBED_LAST = 0, 1, 2
EMBED_FINISH_LANES = 256  # threads of embed_finish_kernel: the partial sums its fixed-order reduction starts from


def _embed_rows(cu, meta, i):
    """(mode, start, slot, final, count, first row, end row) of sequence i; the rows are those the kernels visit: all of
    a mean sequence, the last row of a final last-mode segment, none otherwise."""
    mode, start, slot, fin, count = (int(meta[k][i]) for k in range(5))
    r0, r1 = int(cu[i]), int(cu[i + 1])
    if mode == EMBED_LAST:
        r0 = r1 - 1 if fin else r1
    elif mode != EMBED_MEAN:
        r0 = r1
    return mode, start, slot, fin, count, r0, r1


def _embed_v(h, parts, t):
    v = h[t].float()
    return slab_sum(v, parts[:, t]) if parts is not None else v


def embed_rowscale(h, parts, tseq, cu, meta, eps, rs):
    """Host twin of embed_rowscale_kernel (csrc/kernels/embed.hip): rs[t] = rsqrt(sum(v_t^2) / D + eps) in f32 for
    every pooled row t, v_t = h[t] + parts[0][t] + parts[1][t] + ... left to right; other entries of rs are not
    written.  cu [n + 1] and meta [5, n] are host lists (or CPU tensors); ``tseq`` is implied by cu here."""
    D = h.shape[1]
    for i in range(len(cu) - 1):
        *_, r0, r1 = _embed_rows(cu, meta, i)
        for t in range(r0, r1):
            v = _embed_v(h, parts, t)
            rs[t] = torch.rsqrt((v * v).sum() / D + eps)


def embed_pool(h, parts, cu, meta, rs, gamma, acc):
    """Host twin of embed_pool_kernel: per embedding sequence a = +0 when estart == 0 else acc[slot]; then for its rows
    of this call in position order a = a + (v_t * rs[t]) * gamma, every product and sum a rounded f32; acc[slot] = a.
    A last-mode sequence stores the y of the last row of its final segment and nothing before it.  Bit for bit what the
    kernel gives for the same rs."""
    g = gamma.float()
    for i in range(len(cu) - 1):
        mode, start, slot, _, _, r0, r1 = _embed_rows(cu, meta, i)
        if r0 >= r1:
            continue
        if mode == EMBED_LAST:
            acc[slot] = (_embed_v(h, parts, r0) * rs[r0]) * g
            continue
        a = torch.zeros_like(acc[slot]) if start == 0 else acc[slot].clone()
        for t in range(r0, r1):
            a = a + (_embed_v(h, parts, t) * rs[t]) * g
        acc[slot] = a


def embed_finish(meta, acc, out):
    """Host twin of embed_finish_kernel, for final sequences: m = acc[slot] / ecount (mean) or acc[slot] (last); ss =
    sum(m^2) in the kernel's order (lane i of 256 sums columns i, i + 256, ... in order, then a halving tree over the
    lanes); out[slot] = m / sqrt(ss), zeros when ss == 0.  ``meta`` [5, n] is a host list (or CPU tensor)."""
    n, D, W = len(meta[0]), acc.shape[1], EMBED_FINISH_LANES
    for i in range(n):
        mode, slot, fin, count = int(meta[0][i]), int(meta[2][i]), int(meta[3][i]), int(meta[4][i])
        if mode not in (EMBED_MEAN, EMBED_LAST) or not fin or count <= 0:
            continue
        m = acc[slot] / torch.tensor(float(count), dtype=torch.float32) if mode == EMBED_MEAN else acc[slot].clone()
        sq = torch.zeros((D + W - 1) // W * W, dtype=torch.float32, device=acc.device)
        sq[:D] = m * m
        lanes = torch.zeros(W, dtype=torch.float32, device=acc.device)
        for k in range(sq.numel() // W):
            lanes = lanes + sq[k * W:(k + 1) * W]
        w = W // 2
        while w > 0:
            lanes = lanes[:w] + lanes[w:2 * w]
            w //= 2
        tot = float(lanes[0])
        # the correctly rounded f32 square root, as the kernel's sqrtf: the float64 root rounded to f32 (53 bits are more
        # than the 2 * 24 + 2 that make the double rounding harmless); torch.sqrt on the CPU is off by an ulp now and then
        nrm = torch.tensor(math.sqrt(tot), dtype=torch.float32)
        out[slot] = torch.zeros_like(m) if tot == 0.0 else m / nrm


# ----------------------------------------------------------------------------------- speculative decoding
def attn_verify(q, kc, vc, block_table, pos0, H, Hkv, scale, out, kv_scales=None):
    """Attention of the T new tokens of each sequence (their K / V already appended): q [T, H, D] with one block-table
    row, or q [S, T, H, D] with block_table [S, max_blocks] and pos0 [S].  Row t of sequence s is a decode query at
    position pos0[s] + t, so it sees keys j <= pos0[s] + t.  ``kv_scales``: the fp8 cache's (ks, vs)."""
    S, T = (q.shape[0], q.shape[1]) if q.dim() == 4 else (1, q.shape[0])
    qs, o = q.reshape(S, T, H, -1), out.view(-1)[: q.numel()].view(S, T, H, -1)
    for s in range(S):  # one sequence after the other: nothing of a sequence depends on its neighbours
        p0 = int(pos0.reshape(-1)[s])
        pos = torch.arange(p0, p0 + T, dtype=torch.int32, device=q.device)
        bt = block_table.reshape(S, -1)[s:s + 1].expand(T, -1)
        attn_decode(qs[s], kc, vc, bt, pos, H, Hkv, scale, o[s], kv_scales)
    return out


def spec_draft(prompt_tok, prompt_len, out_tokens, gen_len, input_ids, positions, k, n_max, n_min, forced,
               spec_ids, spec_pos, spec_draft_out):
    """Prompt-lookup drafter (csrc/kernels/spec.hip): per row, the k tokens that followed the best earlier occurrence
    of the context's last tokens -- the lexicographic maximum of (match length m <= n_max, the whole continuation
    exists, end index j) over the candidate ends j <= L - 2 with m >= n_min; -1 where there is none."""
    rows = prompt_len.numel()
    T = k + 1
    for row in range(rows):
        pl = min(max(int(prompt_len[row]), 0), prompt_tok.shape[1])
        gl = min(max(int(gen_len[row]), 0), out_tokens.shape[1])
        draft = [-1] * k
        if forced is not None:
            f = forced[row] if forced.dim() == 3 else forced.reshape(-1, k)  # [rows, nf, k]: row s plants table s
            draft = [int(x) for x in f[min(gl, f.shape[0] - 1)]]
        else:
            ctx = torch.cat([prompt_tok[row, :pl], out_tokens[row, :gl]]).long()
            L = ctx.numel()
            if L >= 2:
                j = torch.arange(L - 1)
                m = torch.zeros(L - 1, dtype=torch.long)
                run = torch.ones(L - 1, dtype=torch.bool)
                for i in range(min(n_max, L)):
                    run = run & (j - i >= 0) & (ctx[(j - i).clamp_min(0)] == ctx[L - 1 - i])
                    m += run
                key = (m << 33) | ((j + 1 + k <= L).long() << 32) | j
                key = torch.where(m >= max(n_min, 1), key, torch.zeros_like(key))
                best = int(key.max())
                if best:
                    jb = best & 0xFFFFFFFF
                    draft = [int(ctx[jb + 1 + i]) if jb + 1 + i < L else -1 for i in range(k)]
        spec_draft_out.view(-1)[row * k:(row + 1) * k] = torch.tensor(draft, dtype=spec_draft_out.dtype)
        ids = [int(input_ids[row])] + [max(d, 0) for d in draft]
        spec_ids.view(-1)[row * T:(row + 1) * T] = torch.tensor(ids, dtype=spec_ids.dtype)
        spec_pos.view(-1)[row * T:(row + 1) * T] = int(positions[row]) + torch.arange(T, dtype=spec_pos.dtype)


def spec_commit(logits, draft, stats, out_tokens, gen_len, input_ids, positions, finished, eos, limit=None,
                eos_on=None):
    """stats [3]: logits [T, V] are the verify rows of the sequence in state row 0; stats [S, 3]: logits [S * T, V],
    rows s T .. s T + T - 1 belong to state row s and are verified against draft[s (T - 1) ..].  Per sequence: commits
    tok_0 .. tok_a in order (a = leading drafts equal to the argmax of their row), stopping after a finishing token;
    stats[s] += (1, drafts >= 0, tokens committed beyond the first).  A finished row changes and counts nothing."""
    S = stats.shape[0] if stats.dim() == 2 else 1
    T = logits.shape[0] // S
    k = T - 1
    toks = logits.float().argmax(-1)
    for s in range(S):
        if int(finished[s]):
            continue
        row = lambda t: t[s:s + 1] if t is not None else None  # noqa: E731  (commit works on row 0 of what it is given)
        dr = draft.reshape(-1)[s * k:(s + 1) * k]
        committed = 0
        for i in range(T):
            if int(finished[s]):
                break
            commit(toks[s * T + i:s * T + i + 1], out_tokens[s:s + 1], gen_len[s:s + 1], input_ids[s:s + 1],
                   positions[s:s + 1], finished[s:s + 1], eos, row(limit), row(eos_on))
            committed += 1
            if i >= T - 1 or int(dr[i]) < 0 or int(dr[i]) != int(toks[s * T + i]):
                break
        st = stats.view(-1, 3)[s]
        st[0] += 1
        st[1] += int((dr >= 0).sum())
        st[2] += max(committed - 1, 0)


def sample_probs(logits_row: torch.Tensor, temperature: float, top_k: int, top_p: float, topk_cap: int = 64, *,
                 min_p: float = 0.0):
    """Distribution the sampler draws from (top-k capped at 64, nucleus within it; ``min_p`` > 0: and only the
    candidates with ``exp((l_i - l_0) / T) >= min_p``, i.e. p_i >= min_p * p_max, next to the best one)."""
    k = top_k if 0 < top_k <= topk_cap else topk_cap
    vals, idx = logits_row.float().topk(min(topk_cap, logits_row.numel()))
    vals, idx = vals[:k], idx[:k]
    p = torch.softmax(vals / temperature, -1)
    before = torch.cumsum(p, 0) - p
    keep = before < top_p
    if min_p > 0:
        keep &= torch.exp((vals - vals[0]) / temperature) >= min_p
    keep[0] = True
    p = torch.where(keep, p, torch.zeros_like(p))
    return idx, p / p.sum()


def fma_f32(a: float, b: float, c: float) -> float:
    """The correctly rounded f32 of a * b + c for f32 operands whose product is exact in f64 (here: a count <= 64
    times an f32), as the device's one fused multiply-add gives it.  The f64 sum is made round-to-odd (the exact error
    of the addition picks the odd neighbour when the sum is inexact), so the second rounding, to f32, is the correct
    one of the exact value."""
    x = float(a) * float(b)
    y = float(c)
    s = x + y
    if not math.isfinite(s):
        return s
    yy = s - x
    err = (x - (s - yy)) + (y - yy)
    if err != 0.0 and not (struct.unpack("<Q", struct.pack("<d", s))[0] & 1):
        s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return float(torch.tensor(s, dtype=torch.float64).to(torch.float32))


def _penalise(row, counts: dict, pen: float, presence: float, frequency: float):
    """The two-step rule of the penalty kernels on ``row`` (f32, in place) for the in-range tokens of ``counts``
    (token -> occurrences c in the window): l = l / pen if l > 0 else l * pen, then l -= fma(c, frequency, presence)."""
    for t, c in counts.items():
        if 0 <= t < row.numel():
            row[t] = row[t] / pen if row[t] > 0 else row[t] * pen
            row[t] = row[t] - fma_f32(float(c), frequency, presence)
    return row


def repeat_penalty(row, hist_row, pen, pos, last_n, presence: float = 0.0, frequency: float = 0.0):
    """llama.cpp/Ollama penalties on one row of logits over the distinct tokens at context positions
    (pos - last_n, pos] of the position-indexed ring ``hist_row``: the repetition penalty ``pen`` (l / pen if l > 0
    else l * pen), then l -= c * frequency + presence for a token that occurs c times in that window (the subtrahend
    is one fused multiply-add, rounded once to f32).  pen == 1 with presence == frequency == 0 changes nothing."""
    if float(pen) == 1.0 and float(presence) == 0.0 and float(frequency) == 0.0:
        return row
    W = hist_row.numel()
    n = min(W if last_n is None else int(last_n), W, pos + 1)
    counts: dict = {}
    for i in range(n):
        t = int(hist_row[(pos - i) % W])
        counts[t] = counts.get(t, 0) + 1
    return _penalise(row, counts, pen, float(presence), float(frequency))


_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def pack_seed(key: int, offset: int = 0) -> int:
    """Device seed word of a request: the stream key (low 40 bits) and the draw-counter offset (high 24 bits, the
    tokens a preempted request already generated), as sampling.hip unpacks it."""
    assert 0 <= offset < (1 << 23), offset
    return (offset << 40) | (int(key) & ((1 << 40) - 1))


def draw_seed(packed: int, gen_len: int) -> int:
    """Generator seed of draw gen_len of a request, for the CPU path's ``torch.multinomial`` draw: the scrambled
    key plus the counter, so nearby keys give unrelated streams and the offset continues a resumed stream.  It has
    the shape of sampling.hip's keyed counter but not its bits (it mixes once more and only seeds a generator);
    the exact host twin of the device draw is ``device_uniform``."""
    packed &= _M64
    key, off = packed & ((1 << 40) - 1), packed >> 40
    return _mix64((_mix64(key) + 0x9E3779B97F4A7C15 * (off + gen_len + 1)) & _M64) & ((1 << 63) - 1)


# --------------------------------------------------------------- exact host twin of sampling.hip's sampled draw
_GOLDEN = 0x9E3779B97F4A7C15
SAMPLE_TOPK_CAP = 64     # LSA_TOPK
SAMPLE_MARGIN = 1e-4     # slack on u and top_p that covers the device's f32 arithmetic (see sample_pick_set)


def device_uniform(packed_seed: int, gen_len: int) -> float:
    """The uniform of draw ``gen_len`` of a request, bit for bit as sample_commit_kernel computes it:
    ``uniform01(lsa_key_mix(sv & (2^40 - 1)), (sv >> 40) + gen_len)`` in 64-bit wrapping integers.  The result is
    a multiple of 2^-24 in [0, 1)."""
    sv = int(packed_seed) & _M64
    # lsa_key_mix: the golden constant, then two multiply-xorshift rounds
    z = ((sv & ((1 << 40) - 1)) + _GOLDEN) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    seed = z ^ (z >> 31)
    # uniform01: golden * (counter + 1) onto the seed, then the two rounds with no further add
    ctr = ((sv >> 40) + int(gen_len)) & _M64
    z = (seed + _GOLDEN * (ctr + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def sample_candidates(row_f32: torch.Tensor, top_k: int):
    """(values f32, indices) of the sampler's candidates in the device's order: descending value, equal values
    lower index first (the packed key is ``float_key(v) << 32 | ~index``), cut at ``k = top_k if 0 < top_k <= 64
    else 64`` (fewer when the row is shorter).  The per-chunk top-64 and the merge of sampling.hip select exactly
    the first 64 of this order.

    Two device conventions are NOT modelled, so keep both out of inputs: the device keys order +0.0 above -0.0
    (torch compares them equal), and a NaN with the sign bit clear sorts above every number."""
    row = row_f32.detach().float().cpu()
    k = top_k if 0 < top_k <= SAMPLE_TOPK_CAP else SAMPLE_TOPK_CAP
    vals, idx = torch.sort(row, stable=True, descending=True)
    return vals[:k], idx[:k]


def sample_pick(row: torch.Tensor, T: float, top_k: int, top_p: float, u: float, *, min_p: float = 0.0) -> int:
    """The token sample_commit_kernel commits for uniform ``u``, computed in float64:

    * ``e_i = exp((l_i - l_0) / T)`` over the candidates of ``sample_candidates``, ``p = e / sum(e)``;
    * candidate i is kept iff ``(i == 0 or (mass before i < top_p and e_i >= min_p)) and e_i > 0`` -- the best token
      is always kept, ``top_p <= 0`` keeps nothing else, a -inf logit is never kept; e_0 is exactly 1, so the ``min_p``
      rule is p_i >= min_p * p_max on the temperature-scaled probabilities, and ``min_p`` = 0 keeps what it finds;
    * the kept mass is renormalised and the pick is the first kept i whose inclusive cumulative mass exceeds u
      (``u < cum_i``); when no cumulative value exceeds u (rounding left the last one below u) it is the LAST
      kept candidate -- a deliberate device convention, never a token outside the nucleus."""
    return _pick(*sample_candidates(row, top_k), T, top_p, u, min_p=min_p)


def _pick(vals, idx, T, top_p, u, *, min_p: float = 0.0) -> int:
    l = vals.double()
    e = torch.exp((l - l[0]) / float(T))
    p = e / e.sum()
    before = torch.cumsum(p, 0) - p
    keep = (before < float(top_p)) & (e > 0)
    if min_p > 0:
        keep &= e >= float(min_p)
    keep[0] = bool(e[0] > 0)
    pk = torch.where(keep, p, torch.zeros_like(p))
    cum = torch.cumsum(pk / pk.sum(), 0)
    hit = torch.nonzero(keep & (cum > float(u)))
    kept = torch.nonzero(keep)
    if hit.numel():
        return int(idx[int(hit[0])])
    return int(idx[int(kept[-1])]) if kept.numel() else int(idx[0])


def sample_pick_set(row: torch.Tensor, T: float, top_k: int, top_p: float, u: float, m: float = SAMPLE_MARGIN, *,
                    min_p: float = 0.0) -> set:
    """Tokens the device may commit: ``sample_pick`` over u in {u - m, u, u + m} x top_p in {top_p - m, top_p,
    top_p + m} and, with ``min_p`` > 0, x min_p in {min_p (1 - m), min_p, min_p (1 + m)}: the device compares its
    f32 ``__expf`` value e_i with min_p, and the relative error of that value (about (|x| + 4) * 2^-23, below 1e-5 for
    every e_i that is not far under any min_p worth setting) is a tenth of the relative margin m.  The device evaluates the same quantities in f32 (``__expf``, shuffle prefix sums); over <= 64
    candidates the absolute error of any cumulative boundary stays below about 1e-5 (per-term relative error about
    (|x| + 4) * 2^-23 weighted by p, six levels of prefix rounding, two normalisations), so m = 1e-4 is more than
    ten times the bound.  A draw is DECIDED when the set has one element: the device must then commit it."""
    vals, idx = sample_candidates(row, top_k)
    mps = (min_p * (1 - m), min_p, min_p * (1 + m)) if min_p > 0 else (0.0,)
    return {_pick(vals, idx, T, tp, uu, min_p=mp) for uu in (u - m, u, u + m) for tp in (top_p - m, top_p, top_p + m)
            for mp in mps}


def _row_opt(t, b: int, default: float = 0.0) -> float:
    """Entry b of an optional per-row f32 operand (None = ``default``)."""
    return default if t is None else float(t[b])


def sample_commit(logits, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len, input_ids,
                  positions, finished, eos, limit=None, eos_on=None, generator: torch.Generator | None = None,
                  last_n=None, presence=None, frequency=None, min_p=None):
    """``presence`` / ``frequency`` / ``min_p``: per-row f32 options, None = off (0); with all three off the call is
    what it is without them."""
    B = logits.shape[0]
    toks = torch.empty(B, dtype=torch.long)
    for b in range(B):
        row = logits[b].float().clone()
        pen, pres, freq = _row_opt(penalty, b, 1.0), _row_opt(presence, b), _row_opt(frequency, b)
        if hist is not None and (pen != 1.0 or pres != 0.0 or freq != 0.0):
            row = repeat_penalty(row, hist[b].cpu(), pen, int(positions[b]),
                                 None if last_n is None else int(last_n[b]), pres, freq)
        T = float(temperature[b])
        if T <= 0:
            toks[b] = int(row.argmax())
            continue
        idx, p = sample_probs(row, T, int(top_k[b]), float(top_p[b]), min_p=_row_opt(min_p, b))
        # draw g of a row comes from (seed key, g + offset) alone (one generator per row: a generator shared across
        # rows made a row's draws depend on the rows sampled before it in the batch)
        g = generator if generator is not None else torch.Generator().manual_seed(draw_seed(int(seeds[b]), int(gen_len[b])))
        toks[b] = int(idx[torch.multinomial(p.cpu(), 1, generator=g)])
    commit(toks, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on, hist=hist)


# --------------------------------------------------------------- speculative decoding of a sampled request
def spec_penalised_row(row, hist_row, draft, i, pen, pos, last_n, presence: float = 0.0, frequency: float = 0.0):
    """Verify row ``i`` of a sampled verify step with its penalties (spec_repeat_penalty_kernel): ``row``
    (modified and returned) is penalised with ``repeat_penalty``'s rule (repetition penalty, then the frequency /
    presence subtrahend of the token's count in the window) over the distinct tokens at context positions
    (pos + i - m, pos + i], m = min(last_n, W, pos + i + 1), where ``pos`` is the row's position at the launch: the
    token at position pos + j, 1 <= j <= i, is ``draft[j - 1]``, the token at a position <= pos is
    ``hist_row[position % W]`` -- the ring the plain step at position pos + i would see had drafts 0 .. i-1 been
    committed.  (A ring slot whose position is > pos holds a token W positions older; m <= W, so it is never read for
    it.)  A draft < 0 or >= V penalises nothing and counts for nothing; pen == 1 with presence == frequency == 0
    changes nothing."""
    if float(pen) == 1.0 and float(presence) == 0.0 and float(frequency) == 0.0:
        return row
    W = hist_row.numel()
    P = pos + i
    m = min(W if last_n is None else int(last_n), W, P + 1)
    counts: dict = {}
    for j in range(m):
        q = P - j
        t = int(draft[q - pos - 1]) if q > pos else int(hist_row[q % W])
        counts[t] = counts.get(t, 0) + 1
    return _penalise(row, counts, pen, float(presence), float(frequency))


def _spec_rows(logits, draft, hist, penalty, last_n, positions, presence=None, frequency=None):
    """The T verify rows (f32 clones) with the penalties of ``spec_penalised_row``."""
    rows = []
    pen, pres, freq = _row_opt(penalty, 0, 1.0), _row_opt(presence, 0), _row_opt(frequency, 0)
    for i in range(logits.shape[0]):
        row = logits[i].float().clone()
        if hist is not None and (pen != 1.0 or pres != 0.0 or freq != 0.0):
            row = spec_penalised_row(row, hist[0].cpu(), draft.cpu(), i, pen, int(positions[0]),
                                     None if last_n is None else int(last_n[0]), pres, freq)
        rows.append(row)
    return rows


def _seq_views(s, T, logits, draft, stats, per_seq):
    """Sequence ``s`` of an S-sequence sampled verify step as the one-sequence operands: its T logits rows, its T - 1
    drafts, its stats row and row ``s`` (kept as a [1, ...] view, so writes land in the caller's tensors) of every
    per-sequence tensor of ``per_seq`` (None stays None)."""
    row = lambda t: t[s:s + 1] if t is not None else None  # noqa: E731
    return (logits[s * T:(s + 1) * T], draft.reshape(-1)[s * (T - 1):(s + 1) * (T - 1)], stats.view(-1, 3)[s],
            [row(t) for t in per_seq])


def spec_sample_commit(logits, draft, stats, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len,
                       input_ids, positions, finished, eos, limit=None, eos_on=None, last_n=None, presence=None,
                       frequency=None, min_p=None):
    """The CPU engine's twin of lsa_spec_sample_commit.  stats [S, 3], S > 1: logits [S * T, V] are the rows of S
    sequences, and the call is a loop of the one-sequence call below over the row views of sequence s (rows s T .. s T
    + T - 1, draft[s (T - 1) ..], ring / parameter / state row s, stats[s]).  Otherwise logits [T, V]: the verify rows
    of the sequence in state row 0, n = gen_len[0] at the call.  Row i is penalised as ``spec_penalised_row`` says
    (written back into ``logits``) and
    draws as ``sample_commit`` draws for gen_len = n + i (``sample_probs`` and ``torch.multinomial`` under
    ``draw_seed(seed, n + i)``; temperature <= 0: the argmax), so a verify step is bit-equal to the plain sampled
    steps.  Commits picks[0 .. a] in order, ring included (a = leading drafts >= 0 equal to their row's pick),
    stopping after a finishing token; stats += (1, drafts >= 0, tokens committed beyond the first).  A finished row
    changes no state.  ``presence`` / ``frequency`` / ``min_p``: the per-sequence options of ``sample_commit``."""
    S = stats.shape[0] if stats.dim() == 2 else 1
    if S > 1:
        T = logits.shape[0] // S
        for s in range(S):
            lg, dr, st, (h, pen, tmp, tk, tp, sd, ot, gl, ii, ps, fin, lim, eon, ln, pr, fr, mp) = _seq_views(
                s, T, logits, draft, stats, (hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len,
                                             input_ids, positions, finished, limit, eos_on, last_n, presence, frequency,
                                             min_p))
            spec_sample_commit(lg, dr, st, h, pen, tmp, tk, tp, sd, ot, gl, ii, ps, fin, eos, lim, eon, last_n=ln,
                               presence=pr, frequency=fr, min_p=mp)
        return
    stats = stats.view(-1)
    T = logits.shape[0]
    n = int(gen_len[0])
    rows = _spec_rows(logits, draft, hist, penalty, last_n, positions, presence, frequency)
    Tmp = float(temperature[0])
    picks = []
    for i, row in enumerate(rows):
        logits[i].copy_(row)
        if Tmp <= 0:
            picks.append(int(row.argmax()))
            continue
        idx, p = sample_probs(row, Tmp, int(top_k[0]), float(top_p[0]), min_p=_row_opt(min_p, 0))
        g = torch.Generator().manual_seed(draw_seed(int(seeds[0]), n + i))
        picks.append(int(idx[torch.multinomial(p.cpu(), 1, generator=g)]))
    if int(finished[0]):
        return
    committed = 0
    for i in range(T):
        if int(finished[0]):
            break
        commit(torch.tensor([picks[i]]), out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on,
               hist=hist)
        committed += 1
        if i >= T - 1 or int(draft[i]) < 0 or int(draft[i]) != picks[i]:
            break
    stats[0] += 1
    stats[1] += int((draft[:T - 1] >= 0).sum())
    stats[2] += max(committed - 1, 0)


def spec_sample_pick_sets(logits, draft, hist, penalty, temperature, top_k, top_p, seeds, gen_len, positions,
                          last_n=None, m: float = SAMPLE_MARGIN, S: int = 1, presence=None, frequency=None,
                          min_p=None) -> list:
    """The exact device twin of the picks of lsa_spec_sample_commit: per verify row i the set of tokens the device
    may write to picks[i] -- ``sample_pick_set`` of the penalised row at ``device_uniform(seed, gen_len[0] + i)``, or
    the plain argmax for temperature <= 0.  A one-element set is a decided draw.  ``S`` > 1: logits [S * T, V], draft
    [S, T - 1] and row s of every other operand belong to sequence s; the list has S * T sets, sequence s at s T ..."""
    if S > 1:
        T = logits.shape[0] // S
        out = []
        for s in range(S):
            lg, dr, _, (h, pen, tmp, tk, tp, sd, gl, ps, ln, pr, fr, mp) = _seq_views(
                s, T, logits, draft, torch.zeros(S, 3), (hist, penalty, temperature, top_k, top_p, seeds, gen_len,
                                                         positions, last_n, presence, frequency, min_p))
            out += spec_sample_pick_sets(lg, dr, h, pen, tmp, tk, tp, sd, gl, ps, last_n=ln, m=m, presence=pr,
                                         frequency=fr, min_p=mp)
        return out
    n = int(gen_len[0])
    Tmp = float(temperature[0])
    out = []
    for i, row in enumerate(_spec_rows(logits, draft, hist, penalty, last_n, positions, presence, frequency)):
        if Tmp <= 0:
            out.append({int(row.argmax())})
        else:
            out.append(sample_pick_set(row, Tmp, int(top_k[0]), float(top_p[0]), device_uniform(int(seeds[0]), n + i), m,
                                       min_p=_row_opt(min_p, 0)))
    return out
