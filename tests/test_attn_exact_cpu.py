"""CPU twins of test_attn_exact_gpu.py: the case builders and both checkers of attn_exact.py, run against
``ops.reference`` (through the ``ops`` entry points, which step on the reference for host tensors), and mutation checks:
a deliberately wrong HOST function goes through the same checker and must be rejected.  Nothing faulty is ever
launched on a GPU."""
import pytest
import torch

import attn_exact as ax
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ the builders hold
def test_count_want_is_a_plain_count():
    """The integer formula of ``count_want`` against counting key by key."""
    H, Hkv = 6, 2
    for n, s in ((1, 0), (65, 1), (129, 3), (700, 2)):
        want = torch.zeros(H, ax.D, dtype=torch.int64)
        for j in range(n):
            for h in range(H):
                want[h, (j + 7 * (h // 3) + 31 * s) % ax.D] += 1
        assert torch.equal(ax.count_want([n], [s], H, Hkv)[0], want)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (8, 1)])
def test_decode_count_reference(H, Hkv, fp8):
    assert ax.decode_count(CPU, H, Hkv, ax.DECODE_LENS, fp8) < 0.25
    assert ax.decode_count(CPU, H, Hkv, ax.DECODE_LENS[:6], fp8, xf=True) < 0.25


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("nparts", [1, 2, 3])
def test_decode_fused_count_reference(nparts, fp8):
    assert ax.decode_fused_count(CPU, 6, 2, [1, 2, 64, 65, 300], nparts, fp8) < 0.25


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("case", sorted(ax.PREFILL_CASES))
def test_prefill_count_reference(case, fp8):
    assert ax.prefill_count(CPU, 4, 2, case, fp8) < 0.25


@pytest.mark.parametrize("fp8", [False, True])
def test_verify_count_reference(fp8):
    assert ax.verify_count(CPU, 6, 2, 4, ax.VERIFY_POS0, fp8) < 0.25
    assert ax.verify_count(CPU, 4, 4, 2, ax.VERIFY_S_FORMS[(4, 2)], fp8, batched=True) < 0.25


@pytest.mark.parametrize("fp8", [False, True])
def test_bound_reference(fp8):
    """The fp32 reference, rounded to bf16, sits within one bf16 rounding of the fp64 one: at most half an ulp, which is
    2^-8 |o| <= 2 units of 2^-9 a, plus f32 noise."""
    one = {"default": None}
    assert ax.decode_bound(CPU, 6, 2, ax.BOUND_LENS, fp8, one, "cpu/decode") < 2.01
    assert ax.decode_bound(CPU, 4, 4, [5, 700], fp8, one, "cpu/decode_spike", spike=True) < 2.01
    assert ax.prefill_bound(CPU, 4, 2, "chunked", fp8, "cpu/prefill") < 2.01
    assert ax.verify_bound(CPU, 6, 2, 4, [0, 63, 700], fp8, "cpu/verify", plans=lambda p0: one) < 2.01
    assert ax.verify_bound(CPU, 4, 4, 4, [704], fp8, "cpu/verify_spike", plans=lambda p0: one, spike=True) < 2.01


def test_f64_reference_matches_f32_reference():
    """``attn_*_f64`` state the same operation as the fp32 reference (random data, both caches)."""
    for fp8 in (False, True):
        c = ax.rand_cache([5, 129, 300], 2, fp8, CPU, seed=3)
        q = ax.rand_q((3, 4, ax.D), 4, CPU)
        pos = torch.tensor([4, 128, 299], **ax.I32)
        want = ref.attn_decode(q, c["kc"], c["vc"], c["bt"], pos, 4, 2, ax.SCALE, torch.empty(3, 4, ax.D), c["kvs"])
        o, a = ref.attn_decode_f64(q, c["kc"], c["vc"], c["bt"], pos, 4, 2, ax.SCALE, c["kvs"])
        assert torch.allclose(o.float(), want, rtol=1e-4, atol=1e-5)
        assert bool((a >= o.abs() * (1 - 1e-12)).all())
        cu, cl = torch.tensor([0, 3, 3, 70], **ax.I32), torch.tensor([5, 129, 300], **ax.I32)
        qp = ax.rand_q((70, 4, ax.D), 5, CPU)
        want = ref.attn_prefill(qp, c["kc"], c["vc"], c["bt"], cu, cl, 4, 2, ax.SCALE, torch.zeros(70, 4, ax.D), c["kvs"])
        o, _ = ref.attn_prefill_f64(qp, c["kc"], c["vc"], c["bt"], cu, cl, 4, 2, ax.SCALE, c["kvs"])
        assert torch.allclose(o.float(), want, rtol=1e-4, atol=1e-5)
        qv = ax.rand_q((3, 2, 4, ax.D), 6, CPU)
        p0 = torch.tensor([3, 127, 200], **ax.I32)
        want = ref.attn_verify(qv, c["kc"], c["vc"], c["bt"], p0, 4, 2, ax.SCALE, torch.zeros(6, 4 * ax.D), c["kvs"])
        o, _ = ref.attn_verify_f64(qv, c["kc"], c["vc"], c["bt"], p0, 4, 2, ax.SCALE, c["kvs"])
        assert torch.allclose(o.float().view(6, -1), want, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the checkers bite
# Each planted fault is a host function with the signature of the entry point it replaces.
def _drop_newest(q, kc, vc, bt, pos, H, Hkv, scale, out, plan=None, kv_scales=None, **kw):
    return ref.attn_decode(q, kc, vc, bt, (pos - 1).clamp_min(0), H, Hkv, scale, out, kv_scales)


def _one_extra(q, kc, vc, bt, pos, H, Hkv, scale, out, plan=None, kv_scales=None, **kw):
    return ref.attn_decode(q, kc, vc, bt, pos + 1, H, Hkv, scale, out, kv_scales)


def _next_kv_group(q, kc, vc, bt, pos, H, Hkv, scale, out, plan=None, kv_scales=None, **kw):
    return ref.attn_decode(q, kc.roll(-1, 1), vc.roll(-1, 1), bt, pos, H, Hkv, scale, out)  # head h: (h // G + 1) % Hkv


def _neighbour_table(q, kc, vc, bt, pos, H, Hkv, scale, out, plan=None, kv_scales=None, **kw):
    bad = bt.clone()
    bad[:, 1] = bt.roll(1, 0)[:, 1]  # block 1 of every sequence through the neighbouring sequence's table row
    return ref.attn_decode(q, kc, vc, bad, pos, H, Hkv, scale, out, kv_scales)


def _new_token_twice(q, kc, vc, bt, pos, H, Hkv, scale, out, qkv_parts=None, cos=None, sin=None, kv_scales=None, **kw):
    """The appended row written (and attended) at pos and again at pos + 1."""
    ref.rope_append(qkv_parts, pos, None, bt, cos, sin, q, kc, vc, H, Hkv, kv_scales)
    k2, v2 = kc.clone(), vc.clone()
    for b in range(pos.shape[0]):
        p = int(pos[b])
        src, dst = (int(bt[b, p // 64]), p % 64), (int(bt[b, (p + 1) // 64]), (p + 1) % 64)
        k2[dst[0], :, dst[1]] = kc[src[0], :, src[1]]
        v2[dst[0], :, dst[1]] = vc[src[0], :, src[1]]
    return ref.attn_decode(q, k2, v2, bt, pos + 1, H, Hkv, scale, out)


def _tile_edge_blind(q, kc, vc, bt, cu_q, ctx_lens, H, Hkv, scale, out, kv_scales=None, **kw):
    """Rows with t % 64 == 63 of a sequence do not see their own key."""
    ref.attn_prefill(q, kc, vc, bt, cu_q, ctx_lens, H, Hkv, scale, out, kv_scales)
    cu = cu_q.tolist()
    for s in range(len(cu) - 1):
        ql, n = cu[s + 1] - cu[s], int(ctx_lens[s])
        for t in range(63, ql, 64):
            p = n - ql + t  # the row's own position: it sees keys < p only
            if p > 0:
                ref.attn_decode(q[cu[s] + t:cu[s] + t + 1], kc, vc, bt[s:s + 1], torch.tensor([p - 1], **ax.I32), H, Hkv,
                                scale, out[cu[s] + t:cu[s] + t + 1], kv_scales)
    return out


def _verify_drop_newest(q, kc, vc, bt, pos0, H, Hkv, scale, out, plan=None, kv_scales=None, **kw):
    """Every verify row blind to its own key (rows at position 0 keep it)."""
    T = q.shape[-3]
    pos = (pos0.view(-1, 1) + torch.arange(T, **ax.I32).view(1, -1) - 1).clamp_min(0).reshape(-1)
    table = bt.reshape(pos0.numel(), -1).repeat_interleave(T, 0)
    o = out.view(-1)[: q.numel()].view(-1, H, ax.D)
    return ref.attn_decode(q.reshape(-1, H, ax.D), kc, vc, table, pos, H, Hkv, scale, o, kv_scales)


def test_count_rejects_dropped_newest_key():
    with pytest.raises(AssertionError, match="elements off"):
        ax.decode_count(CPU, 6, 2, ax.DECODE_LENS, fn=_drop_newest)
    with pytest.raises(AssertionError, match="elements off"):  # one key among 2100, alone in the launch
        ax.decode_count(CPU, 6, 2, [2100], fn=_drop_newest)
    with pytest.raises(AssertionError, match="elements off"):
        ax.verify_count(CPU, 6, 2, 4, [700], fn=_verify_drop_newest)


def test_count_rejects_one_extra_key():
    for lens in (ax.DECODE_LENS, [63], [64], [2100]):  # the extra key: a poison row, or block 0 through a padding entry
        with pytest.raises(AssertionError, match="elements off"):
            ax.decode_count(CPU, 6, 2, lens, fn=_one_extra)


def test_count_rejects_tile_edge_rows_blind_to_themselves():
    for case in ("fresh", "chunked"):
        with pytest.raises(AssertionError, match="elements off"):
            ax.prefill_count(CPU, 4, 2, case, fn=_tile_edge_blind)


def test_count_rejects_wrong_kv_group():
    for H, Hkv in ((4, 2), (6, 2), (8, 2)):
        with pytest.raises(AssertionError, match="elements off"):
            ax.decode_count(CPU, H, Hkv, ax.DECODE_LENS, fn=_next_kv_group)


def test_count_rejects_new_token_counted_twice():
    with pytest.raises(AssertionError, match="elements off"):
        ax.decode_fused_count(CPU, 6, 2, [5, 65, 300], 2, fn=_new_token_twice)


def test_count_rejects_neighbouring_table_row():
    with pytest.raises(AssertionError, match="elements off"):
        ax.decode_count(CPU, 6, 2, [65, 129, 257, 700], fn=_neighbour_table)


def test_bound_rejects_planted_faults_on_random_data():
    """The componentwise bound rejects a dropped newest key, a block read through the neighbour's table row and tile-edge
    rows blind to themselves on random data."""
    one = {"default": None}
    with pytest.raises(AssertionError, match="beyond"):
        ax.decode_bound(CPU, 6, 2, ax.BOUND_LENS, False, one, "mut/drop", fn=_drop_newest)
    with pytest.raises(AssertionError, match="beyond"):
        ax.decode_bound(CPU, 6, 2, [129, 700], False, one, "mut/table", fn=_neighbour_table)
    with pytest.raises(AssertionError, match="beyond"):
        ax.prefill_bound(CPU, 4, 2, "fresh", False, "mut/edge", fn=_tile_edge_blind)
    for k in [k for k in ax.RATIOS if k.startswith("mut/")]:
        del ax.RATIOS[k]


def test_cpu_entry_points_are_the_reference():
    """The twins above go through ``ops``: for host tensors that is ``ops.reference``, plans ignored."""
    c = ax.count_cache([65], 2, False, CPU)
    q, pos = ax.pos_q((1, 4, ax.D), 1, CPU), torch.tensor([64], **ax.I32)
    a = ops.attn_decode(q, c["kc"], c["vc"], c["bt"], pos, 4, 2, ax.SCALE, torch.empty(1, 4, ax.D), plan=(3, 4, 0))
    b = ref.attn_decode(q, c["kc"], c["vc"], c["bt"], pos, 4, 2, ax.SCALE, torch.empty(1, 4, ax.D))
    assert torch.equal(a, b)
