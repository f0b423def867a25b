"""Case builders and checkers of the exact attention tests (test_attn_exact_cpu.py runs them over ``ops.reference``,
test_attn_exact_gpu.py over the HIP kernels).  Everything is built on the host and moved to ``device``; every runner
takes the attention function as an argument, so a deliberately wrong host function goes through the same checker.

Two instruments:

* the COUNT construction: visible K rows are zero, so every visible score is 0, p = 1 and l = n exactly; the visible V
  row of key j, kv head h, sequence s is one-hot at column (j + 7 h + 31 s) mod 128.  The output element is c / n with c
  the number of visible keys of that residue class, and ``check_count`` asserts round(out * n) == c for every element
  against c computed in integers.  bf16 moves out * n by at most c * 2^-8 with c <= n / 128 + 1, so the rounding is
  safe for n < 16384 (the cases keep n <= 4096).  Everything a correct kernel must not read is finite poison (K = 8 in
  every column against a positive q, V = 1024): the tail of each last block, block 0 (the padding target of unused
  table entries), the other sequences' blocks (they are one-hot in another residue class or poison) and one spare
  block that no table names.
* the componentwise BOUND on random data: |got - o| <= c * 2^-9 * a per element against the fp64 reference
  (``ops.reference.attn_*_f64``), a = sum_j p_j |v_j|.
"""
import math

import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

D = 128
SCALE = 1 / math.sqrt(D)
POISON_K, POISON_V = 8.0, 1024.0
I32 = dict(dtype=torch.int32)

# the componentwise bound counts three roundings to bf16 -- P where it is an MFMA operand, the rounded P against the f32
# row sum, and the output -- of about 2^-9 relative each (half an ulp, 2^-8, at worst): 3 units of 2^-9 a, and a model of
# such a kernel (online softmax in 64-key tiles) stays below 2.7.  8 leaves room for the f32 accumulation order, the
# split combine and v_exp_f32.  Not fitted to any kernel's output.
BOUND_C = 8.0
UNIT = 2.0 ** -9
FLOOR = 2.0 ** -126  # below the smallest normal bf16 nothing is asked

RATIOS: dict = {}  # worst |err| / (2^-9 a) per "kernel/case" key, filled by check_bound


# ------------------------------------------------------------------------------------------------ caches
def _tables(ctx, seed):
    """Shuffled block tables [S, max blocks + 1] (unused entries 0) over blocks 1 .. total - 2; block 0 is the padding
    target, block total - 1 the spare that no table names."""
    g = torch.Generator().manual_seed(seed)
    nb = [(n + 63) // 64 for n in ctx]
    total = sum(nb) + 2
    perm = (torch.randperm(total - 2, generator=g) + 1).tolist()
    bt = torch.zeros(len(ctx), max(nb + [1]) + 1, **I32)
    i = 0
    for s, n in enumerate(nb):
        for j in range(n):
            bt[s, j] = perm[i]
            i += 1
    return bt, total, g


def _finish(kf, vf, bt, fp8, device):
    """f32 caches [blocks, Hkv, 64, D] -> dict(kc, vc, kvs, bt) on ``device``: bf16, or e4m3 bytes in the cache's
    token-pair order with their row scales."""
    if fp8:
        k8, ks = ref.quant_kv_rows(kf)
        v8, vs = ref.quant_kv_rows(vf)
        kc, vc = ref.kv8_physical(k8).contiguous().to(device), ref.kv8_physical(v8).contiguous().to(device)
        kvs = (ks.contiguous().to(device), vs.contiguous().to(device))
    else:
        kc, vc, kvs = kf.to(torch.bfloat16).to(device), vf.to(torch.bfloat16).to(device), None
    return dict(kc=kc, vc=vc, kvs=kvs, bt=bt.to(device))


def onehot_rows(j, Hkv, s):
    """The V rows of keys ``j`` (int64 [n]) of sequence s: [n, Hkv, D] with 1.0 at column (j + 7 h + 31 s) mod 128."""
    col = (j.view(-1, 1) + 7 * torch.arange(Hkv).view(1, -1) + 31 * s) % D
    return torch.nn.functional.one_hot(col, D).float()


def count_cache(ctx, Hkv, fp8, device, seed=0, visible=None):
    """The count construction for sequences of ``ctx`` keys (``visible[s]`` <= ctx[s] of them written, default all: the
    others stay poison, like the rest of the arena)."""
    bt, total, _ = _tables(ctx, seed)
    kf = torch.full((total, Hkv, 64, D), POISON_K)
    vf = torch.full((total, Hkv, 64, D), POISON_V)
    for s, n in enumerate(ctx if visible is None else visible):
        j = torch.arange(n)
        blk, off = bt[s, j // 64].long(), j % 64
        kf[blk, :, off] = 0.0
        vf[blk, :, off] = onehot_rows(j, Hkv, s)
    return _finish(kf, vf, bt, fp8, device)


def rand_cache(ctx, Hkv, fp8, device, seed=0):
    """Random normal K and V with a per-block magnitude ramp logspace(-1, 1) on V (a wrong block shows up)."""
    bt, total, g = _tables(ctx, seed)
    mag = torch.logspace(-1, 1, total).view(total, 1, 1, 1)
    kf = torch.randn(total, Hkv, 64, D, generator=g).to(torch.bfloat16).float()
    vf = (torch.randn(total, Hkv, 64, D, generator=g) * mag).to(torch.bfloat16).float()
    return _finish(kf, vf, bt, fp8, device)


def pos_q(shape, seed, device):
    """|randn| in bf16: positive, so a poison key (8.0 in every column) would dominate the softmax if admitted."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).abs().to(torch.bfloat16).to(device)


def rand_q(shape, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(device)


# ------------------------------------------------------------------------------------------------ checkers
def count_want(n, s, H, Hkv):
    """c [R, H, D] int64: the keys j < n[r] of sequence s[r] with (j + 7 (h // G) + 31 s[r]) mod 128 == column."""
    n, s = torch.as_tensor(n, dtype=torch.int64).view(-1, 1, 1), torch.as_tensor(s, dtype=torch.int64).view(-1, 1, 1)
    hk = (torch.arange(H) // (H // Hkv)).view(1, -1, 1)
    r = (torch.arange(D).view(1, 1, -1) - 7 * hk - 31 * s) % D
    return (n + (D - 1) - r) // D


def check_count(out, n, s, H, Hkv, tag=""):
    """round(out * n) == c on EVERY element; returns max |out * n - c|."""
    n = torch.as_tensor(n, dtype=torch.int64)
    want = count_want(n, s, H, Hkv)
    got = out.detach().cpu().double().reshape(want.shape) * n.double().view(-1, 1, 1)
    bad = ~(torch.isfinite(got) & (got.round() == want.double()))
    if bool(bad.any()):
        r, h, c = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{tag}: {int(bad.sum())} elements off, first at row {r} (n = {int(n[r])}) head {h} "
                             f"column {c}: out * n = {float(got[r, h, c]):.4f}, count {int(want[r, h, c])}")
    return float((got - want.double()).abs().max())


def check_bound(got, o, a, key, c=BOUND_C):
    """|got - o| <= c 2^-9 a + FLOOR on EVERY element; records and returns the worst |err| / (2^-9 a)."""
    err = (got.detach().cpu().double().reshape(o.shape) - o.cpu()).abs()
    a = a.cpu()
    ratio = float((err / (UNIT * a + FLOOR)).max()) if err.numel() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    bad = ~(err <= c * UNIT * a + FLOOR)  # a NaN is bad
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{key}: {int(bad.sum())} elements beyond {c} * 2^-9 * a (worst {ratio:.2f}), first at "
                             f"{i}: err {float(err[i]):.3e}, a {float(a[i]):.3e}")
    return ratio


# ------------------------------------------------------------------------------------------------ decode
DECODE_LENS = [1, 2, 63, 64, 65, 128, 129, 257, 700, 2100]
DECODE_HH = [(4, 4), (4, 2), (6, 2), (8, 2), (8, 1)]  # G = 1, 2, 3, 4, 8
SB_LENS = [(37 * i) % 300 + 1 for i in range(16)]   # B = 16, H = Hkv = 32: 512 workgroups, the single-buffer variant
BOUND_LENS = [1, 5, 65, 129, 700]


def decode_plans(B, Hkv, max_blocks):
    return {"default": None, "unsplit": (max_blocks, 1), "one_block_per_split": (1, max_blocks, 0),
            "16k": ops.decode_split_plan(B, Hkv, 16384), "chunk3x4": (3, 4, 0)}


def _positions(lens, device):
    return torch.tensor([n - 1 for n in lens], **I32).to(device)


def decode_count(device, H, Hkv, lens, fp8=False, plans=None, fn=None, xf=False, seed=0):
    """The count check of decode attention over ``lens`` in one launch, under every plan of ``plans``."""
    fn = fn or ops.attn_decode
    c = count_cache(lens, Hkv, fp8, device, seed)
    B = len(lens)
    q, pos = pos_q((B, H, D), seed + 1, device), _positions(lens, device)
    worst = 0.0
    for name, plan in (plans or {"default": None}).items():
        if xf:
            buf = torch.zeros(ops.xfrag_tiles(B) * 16 * H * D, dtype=torch.bfloat16, device=device)
            fn(q, c["kc"], c["vc"], c["bt"], pos, H, Hkv, SCALE, buf, plan=plan, xf=True, kv_scales=c["kvs"])
            out = ops.from_xfrag(buf, B, H * D)
        else:
            out = torch.full((B, H, D), 7.0, dtype=torch.bfloat16, device=device)
            fn(q, c["kc"], c["vc"], c["bt"], pos, H, Hkv, SCALE, out, plan=plan, kv_scales=c["kvs"])
        worst = max(worst, check_count(out, lens, list(range(B)), H, Hkv, f"decode {(H, Hkv)} fp8={fp8} plan {name}"))
    return worst


def fused_slabs(lens, H, Hkv, nparts, cos, sin, seed):
    """f32 split-K slabs [nparts, B, (H + 2 Hkv) * D] of the new token of every sequence: the k slices sum to exactly
    0, the v slices to exactly the one-hot row of key lens[b] - 1, the q slices to the inverse rotation of a positive
    vector (so the rotated q is positive).  The k and v slab values are multiples of 1/8 whose partial sums stay below
    64: every f32 sum of them is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    p = torch.tensor([n - 1 for n in lens])
    qt = torch.randn(B, H, D, generator=g).abs()
    c, s = cos[p].unsqueeze(1), sin[p].unsqueeze(1)
    lo, hi = qt[..., :64], qt[..., 64:]
    total = torch.zeros(B, H + 2 * Hkv, D)
    total[:, :H] = torch.cat([lo * c + hi * s, hi * c - lo * s], -1)  # rotating this gives qt back
    for b in range(B):
        total[b, H + Hkv:] = onehot_rows(p[b:b + 1], Hkv, b)[0]
    parts = torch.randint(-32, 33, (nparts, B, H + 2 * Hkv, D), generator=g).float() / 8
    parts[:, :, :H] *= 0.125
    parts[nparts - 1] = 0
    parts[nparts - 1] = total - parts.sum(0)
    return parts.view(nparts, B, -1).contiguous()


def decode_fused_count(device, H, Hkv, lens, nparts, fp8=False, fn=None, seed=0):
    """Fused RoPE + append: the cache row at ``pos`` holds poison before the call; afterwards the counts include the new
    key exactly once, the row holds exactly the new K (zero) and V (its one-hot row) and no other row has changed."""
    fn = fn or ops.attn_decode
    B = len(lens)
    c = count_cache(lens, Hkv, fp8, device, seed, visible=[n - 1 for n in lens])
    cos, sin = ref.rope_tables(D, c["bt"].shape[1] * 64, 500000.0)
    parts = fused_slabs(lens, H, Hkv, nparts, cos, sin, seed + 2).to(device)
    pos = _positions(lens, device)
    before = [t.clone() for t in (c["kc"], c["vc"]) + (c["kvs"] or ())]
    out = torch.full((B, H, D), 7.0, dtype=torch.bfloat16, device=device)
    fn(torch.zeros(B, H, D, dtype=torch.bfloat16, device=device), c["kc"], c["vc"], c["bt"], pos, H, Hkv, SCALE, out,
       qkv_parts=parts, cos=cos.to(device), sin=sin.to(device), kv_scales=c["kvs"])
    tag = f"fused decode {(H, Hkv)} nparts={nparts} fp8={fp8}"
    worst = check_count(out, lens, list(range(B)), H, Hkv, tag)
    # the cache: row pos of every sequence is the new token, every other row is what it was
    after = [t.detach().cpu() for t in (c["kc"], c["vc"]) + (c["kvs"] or ())]
    before = [t.cpu() for t in before]
    bt = c["bt"].cpu()
    if fp8:  # token order, so that a row is a row
        after[:2] = [ref.kv8_logical(t) for t in after[:2]]
        before[:2] = [ref.kv8_logical(t) for t in before[:2]]
    new = torch.zeros(before[0].shape[:3], dtype=torch.bool)
    for b, n in enumerate(lens):
        blk, off = int(bt[b, (n - 1) // 64]), (n - 1) % 64
        new[blk, :, off] = True
        v_row = onehot_rows(torch.tensor([n - 1]), Hkv, b)[0]
        if fp8:
            k_got = ref.dequant_kv_rows(after[0][blk, :, off], after[2][blk, :, off])
            v_got = ref.dequant_kv_rows(after[1][blk, :, off], after[3][blk, :, off])
            v8, vsc = ref.quant_kv_rows(v_row)
            assert torch.equal(after[1][blk, :, off], v8) and torch.equal(after[3][blk, :, off], vsc), (tag, b, "V bytes")
            assert bool((after[2][blk, :, off] == 0).all()), (tag, b, "K scale")
        else:
            k_got, v_got = after[0][blk, :, off].float(), after[1][blk, :, off].float()
        assert torch.equal(k_got, torch.zeros(Hkv, D)), (tag, b, "new K row")
        assert torch.equal(v_got, v_row), (tag, b, "new V row")
    for got, was in zip(after, before):
        keep = ~new if got.dim() == 3 else ~new.unsqueeze(-1).expand_as(got)
        assert torch.equal(got[keep], was[keep]), (tag, "a cache row other than the new token's changed")
    return worst


def decode_bound(device, H, Hkv, lens, fp8, plans, key, fn=None, f64=None, seed=0, spike=False):
    """The componentwise bound of decode attention on random data; ``spike``: key ctx - 2 of the last sequence (its
    last split under every plan) is 4 q of the kv head's first query head."""
    fn, f64 = fn or ops.attn_decode, f64 or ref.attn_decode_f64
    host = rand_cache(lens, Hkv, fp8, "cpu", seed)
    B = len(lens)
    q = rand_q((B, H, D), seed + 1, "cpu")
    if spike:
        _plant_spike(host, q[B - 1, ::H // Hkv], B - 1, lens[B - 1] - 2, fp8)
    o, a = f64(q, host["kc"], host["vc"], host["bt"], _positions(lens, "cpu"), H, Hkv, SCALE, kv_scales=host["kvs"])
    c = {k: _to(v, device) for k, v in host.items()}
    q, pos = q.to(device), _positions(lens, device)
    worst = 0.0
    for name, plan in plans.items():
        out = torch.full((B, H, D), 7.0, dtype=torch.bfloat16, device=device)
        fn(q, c["kc"], c["vc"], c["bt"], pos, H, Hkv, SCALE, out, plan=plan, kv_scales=c["kvs"])
        worst = max(worst, check_bound(out, o, a, f"{key}/{name}"))
    return worst


def _to(x, device):
    if x is None:
        return None
    return tuple(t.to(device) for t in x) if isinstance(x, tuple) else x.to(device)


def _plant_spike(c, qrow, s, j, fp8):
    """K row j of sequence s (host cache ``c``) := 4 * qrow [Hkv, D] for every kv head."""
    blk, off = int(c["bt"][s, j // 64]), j % 64
    row = (qrow.float() * 4).to(torch.bfloat16).float()
    if not fp8:
        c["kc"][blk, :, off] = row.to(torch.bfloat16)
        return
    k8, ksc = ref.quant_kv_rows(row)
    tile = ref.kv8_logical(c["kc"][blk])
    tile[:, off] = k8
    c["kc"][blk] = ref.kv8_physical(tile)
    c["kvs"][0][blk, :, off] = ksc


# ------------------------------------------------------------------------------------------------ prefill
PREFILL_HH = [(2, 2), (4, 2), (6, 2), (8, 2)]
PREFILL_CASES = {
    "fresh": ([1, 63, 64, 65, 127, 128, 129, 200], [1, 63, 64, 65, 127, 128, 129, 200]),
    "chunked": ([10, 64, 130], [200 + 10, 37 + 64, 300 + 130]),  # start positions 200, 37, 300: no multiple of 64
    "empty_mid": ([70, 0, 129], [70, 40, 129 + 37]),             # a zero-length sequence in the middle of cu_q
}


def _prefill_args(qlens, ctx, device):
    cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), **I32).to(device)
    return cu, torch.tensor(ctx, **I32).to(device)


def _prefill_rows(qlens, ctx):
    """(visible keys, sequence) of every packed query row."""
    n = [c - ql + t + 1 for ql, c in zip(qlens, ctx) for t in range(ql)]
    s = [i for i, ql in enumerate(qlens) for _ in range(ql)]
    return n, s


def prefill_count(device, H, Hkv, case, fp8=False, fn=None, seed=0):
    """Row t of a sequence counts exactly the keys 0 .. ctx - qlen + t."""
    fn = fn or ops.attn_prefill
    qlens, ctx = PREFILL_CASES[case]
    c = count_cache(ctx, Hkv, fp8, device, seed)
    T = sum(qlens)
    q = pos_q((T, H, D), seed + 1, device)
    cu, cl = _prefill_args(qlens, ctx, device)
    out = torch.full((T, H, D), 7.0, dtype=torch.bfloat16, device=device)
    fn(q, c["kc"], c["vc"], c["bt"], cu, cl, H, Hkv, SCALE, out, kv_scales=c["kvs"])
    n, s = _prefill_rows(qlens, ctx)
    return check_count(out, n, s, H, Hkv, f"prefill {(H, Hkv)} {case} fp8={fp8}")


def prefill_bound(device, H, Hkv, case, fp8, key, fn=None, f64=None, seed=0):
    fn, f64 = fn or ops.attn_prefill, f64 or ref.attn_prefill_f64
    qlens, ctx = PREFILL_CASES[case]
    c = rand_cache(ctx, Hkv, fp8, device, seed)
    T = sum(qlens)
    q = rand_q((T, H, D), seed + 1, device)
    cu, cl = _prefill_args(qlens, ctx, device)
    o, a = f64(q.cpu(), _to(c["kc"], "cpu"), _to(c["vc"], "cpu"), c["bt"].cpu(), cu.cpu(), cl.cpu(), H, Hkv, SCALE,
               kv_scales=_to(c["kvs"], "cpu"))
    out = torch.full((T, H, D), 7.0, dtype=torch.bfloat16, device=device)
    fn(q, c["kc"], c["vc"], c["bt"], cu, cl, H, Hkv, SCALE, out, kv_scales=c["kvs"])
    return check_bound(out, o, a, key)


# ------------------------------------------------------------------------------------------------ verify
VERIFY_HH = [(4, 4), (6, 2), (8, 2)]
VERIFY_POS0 = [0, 62, 63, 64, 700, 2100]
VERIFY_S_FORMS = {(2, 8): [0, 63], (4, 2): [63, 0, 700, 64], (8, 4): [0, 63, 62, 64, 700, 1, 2100, 130]}


def verify_T(H, Hkv):
    return [T for T in (2, 4, 8) if T * (H // Hkv) <= 16]


def verify_plans(Hkv, pos0, T, S=1):
    nblk = (pos0 + T + 63) // 64
    return {"default": None, "unsplit": (nblk, 1), "one_block_per_split": (1, nblk, 0),
            "16k": ops.verify_split_plan(Hkv, 16384, S)}


def _verify_rows(pos0s, T):
    return [p + t + 1 for p in pos0s for t in range(T)], [s for s in range(len(pos0s)) for _ in range(T)]


def verify_count(device, H, Hkv, T, pos0s, fp8=False, batched=False, fn=None, seed=0):
    """Row t of sequence s counts exactly the keys 0 .. pos0[s] + t.  ``batched``: one launch of the S-form; else one
    one-sequence launch per entry of ``pos0s`` (over the same cache), under the four plans."""
    fn = fn or ops.attn_verify
    S = len(pos0s)
    c = count_cache([p + T for p in pos0s], Hkv, fp8, device, seed)
    q = pos_q((S, T, H, D), seed + 1, device)
    pos0 = torch.tensor(pos0s, **I32).to(device)
    n, s = _verify_rows(pos0s, T)
    worst = 0.0
    if batched:
        for name, plan in verify_plans(Hkv, max(pos0s), T, S).items():
            out = torch.full((S * T, H * D), 7.0, dtype=torch.bfloat16, device=device)
            fn(q, c["kc"], c["vc"], c["bt"], pos0, H, Hkv, SCALE, out, plan=plan, kv_scales=c["kvs"])
            worst = max(worst, check_count(out, n, s, H, Hkv, f"verify S-form {(H, Hkv)} T={T} fp8={fp8} plan {name}"))
        return worst
    for i, p0 in enumerate(pos0s):
        for name, plan in verify_plans(Hkv, p0, T).items():
            out = torch.full((T, H * D), 7.0, dtype=torch.bfloat16, device=device)
            fn(q[i], c["kc"], c["vc"], c["bt"][i:i + 1].contiguous(), pos0[i:i + 1], H, Hkv, SCALE, out, plan=plan,
               kv_scales=c["kvs"])
            worst = max(worst, check_count(out, n[i * T:(i + 1) * T], s[i * T:(i + 1) * T], H, Hkv,
                                           f"verify {(H, Hkv)} T={T} pos0={p0} fp8={fp8} plan {name}"))
    return worst


def verify_bound(device, H, Hkv, T, pos0s, fp8, key, plans=None, fn=None, f64=None, seed=0, spike=False):
    """The componentwise bound of one-sequence verify launches; ``spike``: key pos0 (every row sees it; with pos0 a
    multiple of 64 it lies in the last block, so in the last split under every plan) is 4 q of the last row's first
    query head per kv head."""
    fn, f64 = fn or ops.attn_verify, f64 or ref.attn_verify_f64
    S = len(pos0s)
    c = rand_cache([p + T for p in pos0s], Hkv, fp8, "cpu", seed)
    q = rand_q((S, T, H, D), seed + 1, "cpu")
    if spike:
        for i, p0 in enumerate(pos0s):
            _plant_spike(c, q[i, T - 1, ::H // Hkv], i, p0, fp8)
    host = c
    c = {k: _to(v, device) for k, v in c.items()}
    q = q.to(device)
    pos0 = torch.tensor(pos0s, **I32).to(device)
    worst = 0.0
    for i, p0 in enumerate(pos0s):
        bt = c["bt"][i:i + 1].contiguous()
        o, a = f64(q[i].cpu(), host["kc"], host["vc"], bt.cpu(), pos0[i:i + 1].cpu(), H, Hkv, SCALE,
                   kv_scales=host["kvs"])
        for name, plan in (plans(p0) if plans else verify_plans(Hkv, p0, T)).items():
            out = torch.full((T, H * D), 7.0, dtype=torch.bfloat16, device=device)
            fn(q[i], c["kc"], c["vc"], bt, pos0[i:i + 1], H, Hkv, SCALE, out, plan=plan, kv_scales=c["kvs"])
            worst = max(worst, check_bound(out, o, a, f"{key}/{name}"))
    return worst
