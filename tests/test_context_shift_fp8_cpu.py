"""Context shift on the fp8 KV cache, on the CPU: the host twin of kv_shift8_kernel (``ops.reference.kv_shift8``)
against a float64 transcription, planted tables, untouched bytes and scales and the op's refusals; and the engine
generating past ``num_ctx`` on the fp8 cache with ``context_shift_fp8`` (kv_shift8_cases.py holds the builders and
checkers; test_context_shift_fp8_gpu.py runs them over the HIP kernel and the captured graphs).

Margins of the twin under the bounds of kv_shift8_cases.py (nsql, llama3 and mistral tables, deltas 64 / 128 / 4033 /
8128, wide magnitudes): worst element error / bound 0.94, worst relative scale error 2.4e-7 (bound 3.8e-6)."""
import pytest
import torch

import kv_shift8_cases as k8
import kv_shift_cases as ks
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.ops import reference as ref


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("kind", ["nsql", "llama3", "mistral"])
@pytest.mark.parametrize("Hkv,wide", [(1, True), (8, False)])
def test_twin_against_float64(kind, Hkv, wide):
    cos, sin = ks.tables(kind)
    kv0, sc0 = k8.arena8(Hkv, seed=Hkv + len(kind), wide=wide)
    moves = ks.moves_for() + [(1, 2, 0, 64, 4033)]  # (the engine's deltas are multiples of 64; the op takes any)
    kv1, sc1 = k8.run_op(kv0, sc0, moves, cos, sin)
    ratio, serr = k8.check_against(kv0, sc0, kv1, sc1, moves, cos, sin)
    print(f"worst element error / bound: {ratio:.3f}, worst relative scale error: {serr:.3g}")
    assert 0.0 < ratio <= 1.0
    # the planted rows: all zeros stays zeros with scale 0; one element becomes the two of its rotated pair
    x1 = k8.dequant(kv1, sc1)
    assert not x1[:, 0, 3, :, k8.ZERO_ROW].any() and not sc1[:, 0, 3, :, k8.ZERO_ROW].any()
    assert not k8.codes(kv1)[:, 0, 3, :, k8.ZERO_ROW].any()
    assert int((x1[0, 0, 3, 0, k8.ONE_ROW] != 0).sum()) == 2 and bool((sc1[:, 0, 3, :, k8.ONE_ROW] > 0).all())


def test_planted_tables():
    """cos and sin in {0, +-1}: as e4m3 values the codes are exactly the permuted, sign-flipped source codes, and the
    scale is the source's within 2^-22 relative (448 * scale, rounded, times 1 / 448, rounded)."""
    rows, d = 512, 192
    cos, sin = ks.planted(rows, d)
    kv0, sc0 = k8.arena8(2, seed=3)
    moves = [(3, 3, 0, 64, d), (4, 5, 10, 64, d)]
    kv1, sc1 = k8.run_op(kv0, sc0, moves, cos, sin)
    c0, c1 = k8.codes(kv0), k8.codes(kv1)
    assert torch.equal(c1[:, 0, 3], ks.planted_expect(c0[:, 0, 3]))
    assert torch.equal(c1[:, 0, 5, :, 10:], ks.planted_expect(c0[:, 0, 4, :, 10:]))
    for got, src in ((sc1[:, 0, 3], sc0[:, 0, 3]), (sc1[:, 0, 5, :, 10:], sc0[:, 0, 4, :, 10:])):
        assert bool(((got.double() - src.double()).abs() <= 2.0 ** -22 * src.double()).all())
    k8.check_against(kv0, sc0, kv1, sc1, moves, cos, sin)  # and everything else is a copy or untouched
    ident = (torch.ones(rows, 64), torch.zeros(rows, 64))
    for t in ident:
        t[d - 64], t[d + 64] = 0.5, -0.5
    kv2, sc2 = k8.run_op(kv0, sc0, [(3, 3, 0, 64, d)], *ident)
    assert torch.equal(k8.codes(kv2), c0) and torch.equal(kv2[:, :, :3], kv0[:, :, :3])


@pytest.mark.parametrize("Hkv", [1, 8])
def test_untouched_bytes_and_copies(Hkv):
    cos, sin = ks.tables("nsql", 512)
    kv0, sc0 = k8.arena8(Hkv, seed=11)
    moves = ks.moves_for(512)
    kv1, sc1 = k8.run_op(kv0, sc0, moves, cos, sin)
    k8.check_against(kv0, sc0, kv1, sc1, moves, cos, sin)
    lg = ref.kv8_logical
    assert torch.equal(kv1[:, 1, 3], kv0[:, 1, 3]) and torch.equal(sc1[:, 1, 3], sc0[:, 1, 3])  # in place: V untouched
    assert torch.equal(kv1[:, 1, 5], kv0[:, 1, 4]) and torch.equal(sc1[:, 1, 5], sc0[:, 1, 4])  # copied V rows
    assert torch.equal(lg(kv1)[:, :, 7, :, :5], lg(kv0)[:, :, 6, :, :5])   # delta 0: K and V rows copied
    assert torch.equal(sc1[:, :, 7, :, :5], sc0[:, :, 6, :, :5])
    assert torch.equal(lg(kv1)[:, 1, 7, :, 5:], lg(kv0)[:, 1, 8, :, 5:])
    assert not torch.equal(kv1[:, 0, 3], kv0[:, 0, 3]) and not torch.equal(sc1[:, 0, 3], sc0[:, 0, 3])
    assert k8.same(k8.run_op(kv0, sc0, moves, cos, sin), (kv1, sc1))       # repeatable
    one = (kv0.clone(), sc0.clone())
    for m in moves:  # each move alone
        ops.kv_shift8(*one, [m], cos, sin)
    assert k8.same(one, (kv1, sc1))
    odd = [(4, 4, 7, 33, 64), (5, 4, 0, 7, 0), (4, 6, 33, 47, 64)]  # odd bounds; reads beside an in-place write
    k8.check_against(kv0, sc0, *k8.run_op(kv0, sc0, odd, cos, sin), odd, cos, sin)


def test_refusals_leave_the_arena_unchanged():
    cos, sin = ks.tables("nsql", 512)
    kv, sc = k8.arena8(1, seed=5)
    kv0, sc0 = kv.clone(), sc.clone()
    for name, moves in ks.refusals(kv.shape[2], 512):
        with pytest.raises(ValueError):
            ops.kv_shift8(kv, sc, moves, cos, sin)
        assert k8.same((kv, sc), (kv0, sc0)), name
    ok = [(3, 4, 0, 64, 64)]
    for bad_kv in (ks.arena(1, seed=5), kv[0], kv.view(torch.int8), kv.float()):  # a bf16 arena; 5-d; not uint8
        with pytest.raises(ValueError):
            ops.kv_shift8(bad_kv, sc, ok, cos, sin)
    for bad_sc in (None, sc[0], sc[..., :32], sc.unsqueeze(-1), sc.double(), sc.to(torch.bfloat16)):
        with pytest.raises(ValueError):
            ops.kv_shift8(kv, bad_sc, ok, cos, sin)
    with pytest.raises(ValueError):
        ops.kv_shift8(kv, sc, ok, cos.double(), sin.double())
    with pytest.raises(ValueError):
        ops.kv_shift8(kv, sc, ok, cos[:, :32], sin[:, :32])
    assert k8.same((kv, sc), (kv0, sc0))
    ops.kv_shift8(kv, sc, [], cos, sin)  # an empty list is a no-op
    assert k8.same((kv, sc), (kv0, sc0))
    with pytest.raises(ValueError):  # and kv_shift still refuses the fp8 cache
        ops.kv_shift(kv, sc, ok, cos, sin)


def test_requantisation_error_grows_slowly():
    """Gaussian rows, llama3 tables, repeated delta-64 shifts against the exact rotation of the original dequantised
    rows: relative RMS error of K after 1 .. 4 re-quantisations (measured: 2.2 %, 3.2 %, 3.9 %, 4.6 %)."""
    cos, sin = ks.tables("llama3")
    kv, sc = k8.arena8(2, seed=21, NB=3, L=1)
    x0 = k8.dequant(kv, sc)[:, 0, 1].double()
    got = []
    for n in range(1, 5):
        ops.kv_shift8(kv, sc, [(1, 1, 0, 64, 64)], cos, sin)
        c, s = cos[64 * n].double(), sin[64 * n].double()
        a, b = x0[..., :64], x0[..., 64:]
        exact = torch.cat([a * c + b * s, b * c - a * s], dim=-1)
        err = k8.dequant(kv, sc)[:, 0, 1].double() - exact
        got.append(float(err.pow(2).mean().sqrt() / exact.pow(2).mean().sqrt()))
    print("relative RMS error after 1 .. 4 re-quantisations:", [f"{100 * g:.2f} %" for g in got])
    # one e4m3 rounding of a Gaussian row is 2^-4 / sqrt(3) relative at worst = 3.6 %; n independent ones add in
    # quadrature, so sqrt(n) * 3.6 % bounds n of them
    assert all(0.0 < g <= 0.036 * (n + 1) ** 0.5 for n, g in enumerate(got)) and got == sorted(got)


# ------------------------------------------------------------------------------------------------ the engine
PROMPT = [1] + list(range(3, 43))
KW = dict(device="cpu", max_slots=3, max_model_len=512, kv_dtype="fp8")
LONG = dict(max_tokens=300, ignore_eos=True, num_ctx=256)


@pytest.fixture(scope="module")
def eng():
    return build_engine("tiny-nsql", context_shift=True, context_shift_fp8=True, **KW)


@pytest.fixture(scope="module")
def greedy(eng):
    """The 300-token request on the fp8 engine with both flags, its shifts checked as they happen, and the same request
    opted out (it ends at the window)."""
    spy = k8.ShiftSpy8(eng, twin=True)
    try:
        on = eng.generate([PROMPT], SamplingParams(**LONG))[0]
    finally:
        spy.restore()
    off = eng.generate([PROMPT], SamplingParams(shift=False, **LONG))[0]
    return on, off, spy


def test_engine_generates_past_the_window(eng, greedy):
    on, off, spy = greedy
    assert eng.context_shift and eng.context_shift_fp8 and eng.runner.kv_fp8 and eng.runner.kv.dtype == torch.uint8
    assert on.eval_count == 300 and len(on.token_ids) == 300 and on.done_reason == "length"
    assert on.context_shifts >= 2 and spy.checked == on.context_shifts and spy.keeps == [4] * spy.checked
    assert eng.stats["context_shifts"] == on.context_shifts and eng.stats["context_shift_tokens"] == 64 * on.context_shifts
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == eng.runner.num_kv_blocks - 1


def test_tokens_up_to_the_first_shift_equal_the_opted_out_run(greedy):
    on, off, _ = greedy
    assert off.eval_count == 215 and off.context_shifts == 0 and off.done_reason == "length"
    assert on.token_ids[:215] == off.token_ids
    plain = build_engine("tiny-nsql", **KW)
    assert plain.generate([PROMPT], SamplingParams(**LONG))[0].token_ids == off.token_ids


def test_two_requests_shift_in_one_launch(eng, greedy):
    spy, calls = k8.ShiftSpy8(eng, twin=True), []
    inner = spy._orig
    spy._orig = lambda entries: (calls.append(len(entries)), inner(entries))[1]
    try:
        rs = eng.generate([PROMPT, PROMPT], SamplingParams(**LONG))
    finally:
        spy.restore()
    assert rs[0].token_ids == rs[1].token_ids and [r.eval_count for r in rs] == [300, 300]
    assert calls and set(calls) == {2} and spy.checked == 2 * len(calls) == rs[0].context_shifts + rs[1].context_shifts


def test_preemption_after_a_shift(eng, greedy):
    q = eng.add_request(PROMPT, SamplingParams(**LONG))
    eng.run_ahead = 16
    try:
        while not q.drops:
            eng.step()
    finally:
        eng.run_ahead = None
    with eng._lock:
        eng._preempt(q)
        eng._admit_hold = False
    assert q.gen_host == 0 and len(q.resumed) == 215 + 16
    kept = q.kept_ids
    assert q.shifted == 64 and len(kept) == len(q.ctx_ids) - 64 and kept[:4] == PROMPT[:4] and kept[4:] == q.ctx_ids[68:]
    eng.run_until_done([q])
    res = eng.result(q)
    assert res.eval_count == 300 and res.done_reason == "length" and q.preemptions == 1 and res.context_shifts >= 2
    assert res.token_ids[:215] == greedy[0].token_ids[:215]  # every generated token is reported
    assert eng.sched.free_blocks == eng.runner.num_kv_blocks - 1


def test_prefix_cache_tail_is_forked_and_never_written():
    """A prompt of 200 tokens whose first three blocks the prefix-cache index holds: the shift forks the shared blocks
    it would rotate, and the indexed blocks keep their bytes and scales -- a second request still hits them."""
    e = build_engine("tiny-nsql", context_shift=True, context_shift_fp8=True, prefix_cache=True, **KW)
    prompt = [1] + [3 + (7 * i) % 90 for i in range(199)]
    sp = SamplingParams(max_tokens=100, ignore_eos=True, num_ctx=256)
    first = e.generate([prompt], SamplingParams(max_tokens=8, ignore_eos=True, num_ctx=256))[0]
    assert e.sched.cached_blocks >= 3
    q = e.add_request(prompt, sp)
    while q.slot < 0 or q.gen_host == 0:
        e.step()
    shared = e.runner.block_tables[q.slot, :3].tolist()
    assert q.cached_tokens >= 128 and all(shared)
    kv0, sc0 = e.runner.kv[:, :, shared].clone(), e.runner.kv_scale[:, :, shared].clone()
    spy, forks = k8.ShiftSpy8(e, twin=True), []
    inner = spy._orig
    spy._orig = lambda entries: (forks.extend(m for en in entries for m in en[1] if m[0] != m[1]), inner(entries))[1]
    try:
        e.run_until_done([q])
    finally:
        spy.restore()
    res = e.result(q)
    assert res.eval_count == 100 and res.context_shifts >= 1 and spy.checked == res.context_shifts
    assert forks and all(dst not in shared for _, dst, _, _, _ in forks) and {m[0] for m in forks} <= set(shared)
    assert torch.equal(e.runner.kv[:, :, shared], kv0) and torch.equal(e.runner.kv_scale[:, :, shared], sc0)
    again = e.generate([prompt], SamplingParams(max_tokens=8, ignore_eos=True, num_ctx=256))[0]
    assert again.token_ids == first.token_ids and again.cached_prompt_tokens >= 128


# ------------------------------------------------------------------------------------------------ the flags
def _today(e, sp):
    r = e.generate([PROMPT], sp)[0]
    return r.token_ids, r.done_reason, r.context_shifts, {k: v for k, v in e.stats.items() if not k.endswith("_s")}


def test_context_shift_alone_is_still_inert():
    want = _today(build_engine("tiny-nsql", **KW), SamplingParams(**LONG))
    assert len(want[0]) == 215 and "context_shifts" not in want[3]
    e = build_engine("tiny-nsql", context_shift=True, **KW)
    assert not e.context_shift and not e.context_shift_fp8
    assert _today(e, SamplingParams(**LONG)) == want
    e = build_engine("tiny-nsql", context_shift_fp8=True, **KW)  # the new flag without the old one
    assert not e.context_shift and not e.context_shift_fp8
    assert _today(e, SamplingParams(**LONG)) == want
    bf16 = build_engine("tiny-nsql", context_shift=True, context_shift_fp8=True, **dict(KW, kv_dtype="bf16"))
    assert bf16.context_shift and not bf16.context_shift_fp8  # the bf16 cache shifts as before, with kv_shift


def test_settings_cli_and_health(monkeypatch, eng, tmp_path):
    import argparse

    from llm_based_apache_spark_optimization_amd.client import EngineService
    from llm_based_apache_spark_optimization_amd.config import Settings

    assert Settings().context_shift_fp8 is False
    monkeypatch.setenv("LSA_CONTEXT_SHIFT_FP8", "1")
    assert Settings().context_shift_fp8 is True and Settings().context_shift is False
    monkeypatch.delenv("LSA_CONTEXT_SHIFT_FP8")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    s = Settings.from_cli(ap.parse_args(["--context-shift", "--context-shift-fp8"]))
    assert s.context_shift is True and s.context_shift_fp8 is True
    assert Settings.from_cli(ap.parse_args(["--context-shift"])).context_shift_fp8 is False
    inert = build_engine("tiny-nsql", context_shift=True, **KW)
    svc = EngineService(lambda model: eng if model == "fp8shift" else inert,
                        defaults={"num_predict": 150, "ignore_eos": True, "num_ctx": 128})
    try:
        on = svc.generate("fp8shift", "hi")
        off = svc.generate("inert", "hi")
        assert on.eval_count == 150 and on.context_shifts >= 1 and on.to_dict()["context_shifts"] == on.context_shifts
        assert off.eval_count < 128 and "context_shifts" not in off.to_dict()
        h = svc.health()["engines"]
        assert h["fp8shift"]["context_shift"] is True and h["fp8shift"]["context_shift_fp8"] is True
        assert h["inert"]["context_shift"] is False and h["inert"]["context_shift_fp8"] is False
        assert h["fp8shift"]["context_shifts"] >= 1 and "context_shifts" not in h["inert"]
    finally:
        for m in svc.models():
            svc.loop(m).close()


def test_service_factory_passes_the_flag(monkeypatch):
    from llm_based_apache_spark_optimization_amd.config import Settings
    from llm_based_apache_spark_optimization_amd import engine
    from llm_based_apache_spark_optimization_amd.serving import service

    seen = {}
    monkeypatch.setattr(engine, "build_engine", lambda model, **kw: seen.update(kw) or _Stub())
    s = Settings(context_shift=True, context_shift_fp8=True)
    service.engine_factory(s)("tiny-nsql")
    assert seen["context_shift"] is True and seen["context_shift_fp8"] is True


class _Stub:
    class runner:
        spec_min_accept = 0
