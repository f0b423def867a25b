"""Context shift on the CPU: the host twin of the re-rotation kernel (``ops.reference.kv_shift``) against a float64
transcription, the rotation identity, planted tables, untouched bytes and the op's refusals; ``Scheduler.shift`` on
both scheduler implementations; and the engine generating past ``num_ctx`` (kv_shift_cases.py holds the builders and
checkers; test_context_shift_gpu.py runs them over the HIP kernel and the captured graphs)."""
import dataclasses
import os

import pytest
import torch

import kv_shift_cases as ks
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.engine import SamplingOptionError
from llm_based_apache_spark_optimization_amd.ops import reference as ref
from llm_based_apache_spark_optimization_amd.runtime import native

U = ks.U


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("kind", ["nsql", "llama3", "mistral"])
@pytest.mark.parametrize("Hkv", [1, 8])
def test_twin_against_float64(kind, Hkv):
    """|out - exact| <= u |exact| + 2^-20 (|a| + |b|) on every element, magnitudes 1e-3 .. 1e2, deltas up to 8128."""
    cos, sin = ks.tables(kind)
    kv0 = ks.arena(Hkv, seed=Hkv + len(kind), wide=True)
    moves = ks.moves_for() + [(1, 2, 0, 64, 4033)]  # (the engine's deltas are multiples of 64; the op takes any)
    worst = ks.check_against(kv0, ks.run_op(kv0, moves, cos, sin), moves, cos, sin)
    print(f"worst error / bound: {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("kind", ["nsql", "llama3"])
def test_rotation_identity(kind):
    """A cache written by ``rope_append`` at positions p and shifted by d holds R(p - d) k: every element within
    3u hypot(k_i, k_{i+64}) of the float64 rotation of the unrounded k (one rounding at the append, one at the shift,
    and the tables' angle error; positions < 8192)."""
    H, Hkv, T = 2, 2, 192
    cos, sin = ks.tables(kind)
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(T, (H + 2 * Hkv) * 128, generator=g)
    worst = 0.0
    for p0, d in ((64, 64), (1000, 960), (8000, 128), (7999, 7936)):
        pos = torch.arange(p0, p0 + T, dtype=torch.int32)
        first = p0 // 64
        bt = torch.zeros(1, 130, dtype=torch.int32)
        bt[0, first:first + 4] = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
        kc, vc = torch.zeros(6, Hkv, 64, 128, dtype=torch.bfloat16), torch.zeros(6, Hkv, 64, 128, dtype=torch.bfloat16)
        q_out = torch.zeros(T, H * 128, dtype=torch.bfloat16)
        ref.rope_append(qkv, pos, torch.zeros(T, dtype=torch.int32), bt, cos, sin, q_out, kc, vc, H, Hkv)
        kv = torch.stack([kc, vc])[None].contiguous()  # [1, 2, NB, Hkv, 64, 128]
        ops.kv_shift(kv, None, [(b, b, 0, 64, d) for b in (1, 2, 3, 4)], cos, sin)
        k = qkv.view(T, H + 2 * Hkv, 128)[:, H:H + Hkv].double()
        ang = (pos.double() - d)[:, None] * ks.inv_freq64(kind)[None]
        c, s = ang.cos()[:, None], ang.sin()[:, None]
        lo, hi = k[..., :64], k[..., 64:]
        exact = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)
        bound = 3 * U * torch.hypot(lo, hi).repeat(1, 1, 2)
        got = ks.rows_of(kv[:, 0], bt[0][(pos // 64).long()].long(), (pos % 64).long())[:, 0].double()
        err = (got - exact).abs()
        assert bool((err <= bound).all()), (p0, d, float((err / bound).max()))
        worst = max(worst, float((err / (U * torch.hypot(lo, hi).repeat(1, 1, 2))).max()))
    print(f"worst error: {worst:.2f} u hypot")


def test_planted_tables():
    """Row d = (cos 0, sin 1) gives lo' = hi, hi' = -lo and (1, 0) the identity, exactly; the rows 64 above and below
    d carry other plants, and every other row garbage."""
    rows, d = 512, 192
    cos, sin = ks.planted(rows, d)
    kv0 = ks.arena(2, seed=3)
    kv1 = ks.run_op(kv0, [(3, 3, 0, 64, d), (4, 5, 10, 64, d)], cos, sin)
    assert torch.equal(kv1[:, 0, 3], ks.planted_expect(kv0[:, 0, 3]))
    assert torch.equal(kv1[:, 0, 5, :, 10:], ks.planted_expect(kv0[:, 0, 4, :, 10:]))
    assert torch.equal(kv1[:, 0, 5, :, :10], kv0[:, 0, 5, :, :10]) and torch.equal(kv1[:, 1, 5, :, 10:], kv0[:, 1, 4, :, 10:])
    ident = (torch.ones(rows, 64), torch.zeros(rows, 64))
    for t in ident:
        t[d - 64], t[d + 64] = 0.5, -0.5
    kv2 = ks.run_op(kv0, [(3, 3, 0, 64, d)], *ident)
    assert torch.equal(kv2.view(torch.int16), kv0.view(torch.int16))  # the identity, bit for bit


@pytest.mark.parametrize("Hkv", [1, 8])
def test_untouched_bytes_and_copies(Hkv):
    cos, sin = ks.tables("nsql", 512)
    kv0 = ks.arena(Hkv, seed=11)
    moves = ks.moves_for(512)
    kv1 = ks.run_op(kv0, moves, cos, sin)
    ks.check_against(kv0, kv1, moves, cos, sin)  # every byte outside the destination rows is bit-unchanged
    b = lambda t: t.view(torch.int16)  # noqa: E731
    assert torch.equal(b(kv1[:, 1, 3]), b(kv0[:, 1, 3]))                 # the V of an in-place move
    assert torch.equal(b(kv1[:, 1, 5]), b(kv0[:, 1, 4]))                 # copied V rows
    assert torch.equal(b(kv1[:, :, 7, :, :5]), b(kv0[:, :, 6, :, :5]))   # delta 0: K and V rows copied
    assert torch.equal(b(kv1[:, 1, 7, :, 5:]), b(kv0[:, 1, 8, :, 5:]))
    assert not torch.equal(b(kv1[:, 0, 3]), b(kv0[:, 0, 3]))
    assert torch.equal(b(ks.run_op(kv0, moves, cos, sin)), b(kv1))       # repeatable
    one = kv0.clone()
    for m in moves:  # each move alone
        ops.kv_shift(one, None, [m], cos, sin)
    assert torch.equal(b(one), b(kv1))
    ok = ks.run_op(kv0, [(4, 4, 0, 9, 64), (4, 6, 9, 20, 64)], cos, sin)  # reads next to an in-place write: accepted
    ks.check_against(kv0, ok, [(4, 4, 0, 9, 64), (4, 6, 9, 20, 64)], cos, sin)


def test_refusals_leave_the_arena_unchanged():
    cos, sin = ks.tables("nsql", 512)
    kv = ks.arena(1, seed=5)
    kv0 = kv.clone()
    for name, moves in ks.refusals(kv.shape[2], 512):
        with pytest.raises(ValueError):
            ops.kv_shift(kv, None, moves, cos, sin)
        assert torch.equal(kv.view(torch.int16), kv0.view(torch.int16)), name
    ok = [(3, 4, 0, 64, 64)]
    for bad_kv in (kv[0], kv.float(), kv.view(torch.int16)):  # not 6-dimensional; not bf16
        with pytest.raises(ValueError):
            ops.kv_shift(bad_kv, None, ok, cos, sin)
    with pytest.raises(ValueError):  # the fp8 cache
        ops.kv_shift(kv, torch.ones(kv.shape[:5]), ok, cos, sin)
    with pytest.raises(ValueError):
        ops.kv_shift(kv, None, ok, cos.double(), sin.double())
    with pytest.raises(ValueError):
        ops.kv_shift(kv, None, ok, cos[:, :32], sin[:, :32])
    assert torch.equal(kv.view(torch.int16), kv0.view(torch.int16))
    ops.kv_shift(kv, None, [], cos, sin)


# ------------------------------------------------------------------------------------------------ the scheduler
SCHEDS = [native._PyScheduler] + ([native._mod.Scheduler] if native.NATIVE else [])


def _plan(old, shared, keep, d, fresh):
    """The rule, written out: (moves, table) for an old table whose first ``shared`` blocks the index holds."""
    k0, rem, m = keep // 64, keep % 64, d // 64
    moves, table, fresh = [], list(old[:k0]), list(fresh)
    for j in range(k0, len(old) - m):
        src = old[j + m]
        dst = fresh.pop(0) if j + m < shared else src
        if j == k0 and rem:
            moves += [(old[k0], dst, 0, rem, 0), (src, dst, rem, 64, d)]
        else:
            moves.append((src, dst, 0, 64, d))
        table.append(dst)
    return moves, table


@pytest.mark.parametrize("S", SCHEDS)
@pytest.mark.parametrize("keep", [0, 4, 64, 70])
@pytest.mark.parametrize("d", [64, 192])
def test_scheduler_plans_private(S, keep, d):
    s = S(12, 64, 2, 1000, 8)
    s.add(1, 300, 212)
    assert s.admit() == [1] and s.grow(1, 511) >= 0
    old = s.block_table(1)
    assert old == list(range(1, 9)) and s.free_blocks == 3
    moves, table = s.shift(1, keep, d)
    assert ([tuple(m) for m in moves], list(table)) == _plan(old, 0, keep, d, [])
    assert s.block_table(1) == list(table) == old[:keep // 64] + old[keep // 64 + d // 64:]
    assert s.free_blocks == 3  # the released blocks are still read by the moves ...
    s.shift_done()
    assert s.free_blocks == 3 + d // 64  # ... until the engine has enqueued them
    assert s.grow(1, 511) == d // 64 and len(s.block_table(1)) == 8
    s.finish(1)
    assert s.free_blocks == 11


def test_scheduler_plan_by_hand():
    for S in SCHEDS:
        s = S(12, 64, 2, 1000, 8)
        s.add(1, 250, 6)
        s.admit()
        assert s.block_table(1) == [1, 2, 3, 4]
        moves, table = s.shift(1, 4, 64)
        assert [tuple(m) for m in moves] == [(1, 2, 0, 4, 0), (2, 2, 4, 64, 64), (3, 3, 0, 64, 64), (4, 4, 0, 64, 64)]
        assert list(table) == [2, 3, 4]
        for bad in ((1, 4, 63), (1, -1, 64), (1, 4, 0), (1, 4, 192), (1, 128, 64)):
            with pytest.raises(Exception):
                s.shift(*bad)
        assert s.block_table(1) == [2, 3, 4]
        s.add(2, 10, 10)
        with pytest.raises(Exception):
            s.shift(2, 0, 64)  # not running


def _cached(S, blocks=20):
    """A scheduler whose index holds the three full blocks of a 200-token prompt, nobody referencing them."""
    s = S(blocks, 64, 3, 1000, 8, prefix_cache=True)
    toks = list(range(1000, 1200))
    s.add(1, 200, 10, toks)
    assert s.admit() == [1]
    s.publish(1)
    s.finish(1)
    assert s.cached_blocks == 3 and all(n[1] == 0 for n in s.prefix_nodes())
    return s, toks


@pytest.mark.parametrize("S", SCHEDS)
@pytest.mark.parametrize("keep", [4, 64, 70])
def test_scheduler_plans_shared(S, keep):
    """A shared head stays shared below keep // 64; a shared tail is forked to fresh blocks and never written; every
    block from keep // 64 on is private afterwards; the references are back at zero after ``finish``."""
    s, toks = _cached(S)
    s.add(2, 250, 6, toks[:192] + list(range(58)))
    assert s.admit() == [2] and s.shared_blocks(2) == 3
    old, free0 = s.block_table(2), s.free_blocks
    cached = {n[0] for n in s.prefix_nodes()}
    assert set(old[:3]) == cached and len(old) == 4
    k0 = keep // 64
    moves, table = s.shift(2, keep, 64)
    fresh = [b for b in table if b not in old]
    assert len(fresh) == 2 - k0 and ([tuple(m) for m in moves], list(table)) == _plan(old, 3, keep, 64, fresh)
    assert not {m[1] for m in moves} & cached  # no block of the index is written
    assert s.shared_blocks(2) == k0 and s.block_table(2)[:k0] == old[:k0]
    assert all(n[1] == 1 for n in s.prefix_nodes())  # still pinned: the moves read them
    s.shift_done()
    refs = {n[0]: n[1] for n in s.prefix_nodes()}
    assert [refs[b] for b in old[:3]] == [1] * k0 + [0] * (3 - k0)
    assert s.free_blocks == free0 - len(fresh) + (3 - k0)  # fresh blocks taken, the dropped nodes evictable again
    assert s.publish(2) == 0  # a shifted cache is never published
    s.finish(2)
    assert all(n[1] == 0 for n in s.prefix_nodes()) and s.free_blocks == 19  # cached blocks count as allocatable
    s.reset_prefix_cache()
    assert s.free_blocks == 19 and s.cached_blocks == 0


@pytest.mark.parametrize("S", SCHEDS)
def test_scheduler_refuses_when_blocks_are_short(S):
    s, toks = _cached(S, blocks=6)  # 5 usable blocks: 3 cached + the sharer's private block + 1
    s.add(2, 250, 6, toks[:192] + list(range(58)))
    assert s.admit() == [2] and s.free_blocks == 1
    before = (s.block_table(2), s.shared_blocks(2), s.prefix_nodes(), s.free_blocks)
    assert s.shift(2, 4, 64) is None  # two fresh blocks needed, one there
    assert (s.block_table(2), s.shared_blocks(2), s.prefix_nodes(), s.free_blocks) == before
    moves, table = s.shift(2, 64, 64)  # one fresh block is enough here
    assert len(moves) == 2 and s.free_blocks == 0
    s.shift_done()
    s.finish(2)
    s.reset_prefix_cache()
    assert s.free_blocks == 5


def test_scheduler_implementations_agree():
    if not native.NATIVE:
        pytest.skip("no native runtime")
    g = torch.Generator().manual_seed(5)
    rnd = lambda n: int(torch.randint(0, n, (1,), generator=g))  # noqa: E731
    pair = [S(30, 64, 4, 1000, 10, prefix_cache=True) for S in SCHEDS]
    live, nxt = [], 1
    for _ in range(300):
        op = rnd(6)
        if op == 0:
            n, new, cut = 1 + rnd(400), 1 + rnd(200), 64 * rnd(5)
            toks = [(3 * i) % 7 if i < cut else (5 * i + nxt) % 11 for i in range(n)]
            [s.add(nxt, n, new, toks) for s in pair]
            live.append(nxt)
            nxt += 1
        elif op == 1:
            assert pair[0].admit() == pair[1].admit()
            [(s.take_copies(), s.copies_done()) for s in pair]
        elif op == 2 and pair[0].running():
            rid = pair[0].running()[rnd(len(pair[0].running()))]
            assert pair[0].publish(rid) == pair[1].publish(rid)
            t = 1 + rnd(640)
            assert pair[0].grow(rid, t) == pair[1].grow(rid, t)
        elif op in (3, 4) and pair[0].running():
            rid = pair[0].running()[rnd(len(pair[0].running()))]
            keep, d, done = rnd(140), 64 * (1 + rnd(3)), rnd(2)
            out = []
            for s in pair:
                try:
                    p = s.shift(rid, keep, d)
                    out.append(None if p is None else ([tuple(m) for m in p[0]], list(p[1])))
                except Exception:  # noqa: BLE001 - both must refuse the same calls
                    out.append("raised")
                if done:
                    s.shift_done()
            assert out[0] == out[1]
        elif op == 5 and live:
            rid = live.pop(rnd(len(live)))
            [s.finish(rid) for s in pair]
        assert pair[0].free_blocks == pair[1].free_blocks and pair[0].prefix_nodes() == pair[1].prefix_nodes()
        assert [pair[0].block_table(r) for r in pair[0].running()] == [pair[1].block_table(r) for r in pair[1].running()]


# ------------------------------------------------------------------------------------------------ the engine
PROMPT = [1] + list(range(3, 43))
KW = dict(device="cpu", max_slots=3, max_model_len=512)
LONG = dict(max_tokens=300, ignore_eos=True, num_ctx=256)


@pytest.fixture(scope="module")
def eng():
    return build_engine("tiny-nsql", context_shift=True, guided=True, logprobs=True, **KW)


@pytest.fixture(scope="module")
def plain():
    return build_engine("tiny-nsql", guided=True, logprobs=True, **KW)


@pytest.fixture(scope="module")
def greedy(eng):
    """The 300-token request on the feature engine, its shifts checked as they happen, and the same request opted
    out (it ends at the window)."""
    spy = ks.ShiftSpy(eng)
    try:
        on = eng.generate([PROMPT], SamplingParams(**LONG))[0]
    finally:
        spy.restore()
    off = eng.generate([PROMPT], SamplingParams(shift=False, **LONG))[0]
    return on, off, spy


def test_engine_generates_past_the_window(eng, greedy):
    """300 tokens through a 256-token window: on the parent commit the engine stops at the window (215 tokens)."""
    on, off, spy = greedy
    assert on.eval_count == 300 and len(on.token_ids) == 300 and on.done_reason == "length"
    assert on.context_shifts >= 2 and spy.checked == on.context_shifts and spy.keeps == [4] * spy.checked
    assert eng.stats["context_shifts"] == on.context_shifts and eng.stats["context_shift_tokens"] == 64 * on.context_shifts
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == eng.runner.num_kv_blocks - 1


def test_tokens_up_to_the_first_shift_equal_the_opted_out_run(greedy, plain):
    on, off, _ = greedy
    assert off.eval_count == 256 - len(PROMPT) and off.context_shifts == 0 and off.done_reason == "length"
    assert on.token_ids[:off.eval_count] == off.token_ids
    assert plain.generate([PROMPT], SamplingParams(**LONG))[0].token_ids == off.token_ids


def test_sampled_request_with_repeat_penalty(eng):
    sp = SamplingParams(temperature=0.8, top_k=30, top_p=0.95, seed=5, repeat_penalty=1.3, num_keep=70, **LONG)
    spy = ks.ShiftSpy(eng)  # checks the ring rows too
    try:
        on = eng.generate([PROMPT], sp)[0]
    finally:
        spy.restore()
    off = eng.generate([PROMPT], dataclasses.replace(sp, shift=False))[0]
    assert on.eval_count == 300 and spy.checked == on.context_shifts >= 2 and spy.keeps[0] == len(PROMPT)
    assert on.token_ids[:off.eval_count] == off.token_ids and off.eval_count == 215


def test_guided_request(eng):
    sp = SamplingParams(max_tokens=300, num_ctx=256, regex="[a-z]{4000,}")
    on = eng.generate([PROMPT], sp)[0]
    off = eng.generate([PROMPT], dataclasses.replace(sp, shift=False))[0]
    assert on.eval_count == 300 and on.context_shifts >= 2 and on.done_reason == "length"
    assert on.text and all("a" <= ch <= "z" for ch in on.text)
    assert on.token_ids[:off.eval_count] == off.token_ids and off.eval_count == 215


def test_logprobs_and_streaming(eng, greedy):
    on = greedy[0]
    res = eng.generate([PROMPT], SamplingParams(logprobs=True, top_logprobs=2, **LONG))[0]
    assert res.token_ids == on.token_ids and len(res.logprobs) == res.eval_count == 300
    req = eng.add_request(PROMPT, SamplingParams(**LONG), stream=True)
    eng.run_ahead = 16
    try:
        import threading

        t = threading.Thread(target=eng.run_until_done, args=([req],))
        t.start()
        pieces = list(eng.stream_text(req, timeout_s=120))
        t.join()
    finally:
        eng.run_ahead = None
    assert len(pieces) > 4 and "".join(pieces) == on.text == eng.result(req).text


def test_neighbour_is_not_disturbed(eng, greedy):
    other = [1] + list(range(60, 90))
    solo = eng.generate([other], SamplingParams(max_tokens=120, ignore_eos=True))[0].token_ids
    a = eng.add_request(PROMPT, SamplingParams(**LONG))
    b = eng.add_request(other, SamplingParams(max_tokens=120, ignore_eos=True))
    eng.run_ahead = 8
    try:
        eng.run_until_done([a, b])
    finally:
        eng.run_ahead = None
    assert b.output_ids == solo and a.output_ids == greedy[0].token_ids and len(a.drops) >= 2


def test_two_requests_shift_in_one_launch(eng, greedy):
    """Two requests that fill their windows at the same boundary: one ``shift_slots`` call, so one kernel launch, for
    both; each slot's cache is checked as in the solo run.  (Their tokens are those of a batch-2 run, which on the CPU
    path differ from the solo run's in the last bits of the GEMMs long before the first shift.)"""
    spy, calls = ks.ShiftSpy(eng), []
    inner = spy._orig
    spy._orig = lambda entries: (calls.append(len(entries)), inner(entries))[1]
    try:
        rs = eng.generate([PROMPT, PROMPT], SamplingParams(**LONG))
    finally:
        spy.restore()
    assert rs[0].token_ids == rs[1].token_ids and [r.eval_count for r in rs] == [300, 300]
    assert rs[0].token_ids[:100] == greedy[0].token_ids[:100]
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
    assert q.shifted == 64 and len(kept) == len(q.ctx_ids) - 64 and kept[:4] == PROMPT[:4]
    assert kept[4:] == q.ctx_ids[68:]
    eng.run_until_done([q])
    res = eng.result(q)
    assert res.eval_count == 300 and res.done_reason == "length" and q.preemptions == 1 and res.context_shifts >= 2
    assert res.token_ids[:215] == greedy[0].token_ids[:215]  # every generated token is reported
    assert eng.sched.free_blocks == eng.runner.num_kv_blocks - 1


def test_spec_engine_takes_plain_steps_after_a_shift():
    e = build_engine("tiny-nsql", context_shift=True, spec_tokens=3, **KW)
    base = build_engine("tiny-nsql", context_shift=True, **KW)
    want = base.generate([PROMPT], SamplingParams(**LONG))[0]
    e.run_ahead = 8  # (a run to the window's end has no room for verify steps: each may commit spec_tokens + 1)
    q = e.add_request(PROMPT, SamplingParams(**LONG))
    while not q.drops:
        assert not q.spec_off or q.spec_steps >= 16
        e.step()
    assert q.spec_off
    steps = e.stats["spec_steps"]
    e.run_until_done([q])
    assert e.stats["spec_steps"] == steps > 0
    assert e.result(q).token_ids == want.token_ids and e.result(q).context_shifts == want.context_shifts


# ------------------------------------------------------------------------------------------------ ineligible cases
def _today(e, sp):
    r = e.generate([PROMPT], sp)[0]
    return r.token_ids, r.done_reason, r.context_shifts, {k: v for k, v in e.stats.items() if not k.endswith("_s")}


def test_flag_off_and_opt_out_are_todays_engine(eng, plain):
    want = _today(build_engine("tiny-nsql", **KW), SamplingParams(**LONG))
    assert len(want[0]) == 215 and "context_shifts" not in want[3]
    assert not plain.context_shift and "context_shifts" not in plain.stats
    e = build_engine("tiny-nsql", context_shift=True, **KW)
    got = _today(e, SamplingParams(shift=False, **LONG))
    assert got[3].pop("context_shifts") == 0 and got[3].pop("context_shift_tokens") == 0
    assert got == want


def test_small_window_is_ineligible():
    sp = SamplingParams(max_tokens=300, ignore_eos=True, num_ctx=127)
    want = _today(build_engine("tiny-nsql", **KW), sp)
    e = build_engine("tiny-nsql", context_shift=True, **KW)
    got = _today(e, sp)
    assert got[3].pop("context_shifts") == 0 and got[3].pop("context_shift_tokens") == 0
    assert got == want and len(want[0]) == 127 - len(PROMPT)
    at128 = e.generate([PROMPT], dataclasses.replace(sp, num_ctx=128, max_tokens=150))[0]
    assert at128.eval_count == 150 and at128.context_shifts >= 1  # W = 128: keep 0, d = 64


def test_fp8_cache_is_inert():
    want = _today(build_engine("tiny-nsql", kv_dtype="fp8", **KW), SamplingParams(**LONG))
    e = build_engine("tiny-nsql", kv_dtype="fp8", context_shift=True, **KW)
    assert not e.context_shift
    assert _today(e, SamplingParams(**LONG)) == want and len(want[0]) == 215


def _tp_worker(rank, world, port, q):
    import torch.distributed as dist

    from llm_based_apache_spark_optimization_amd.parallel import TPGroup

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tp = TPGroup(dist.group.WORLD, rank, world, torch.device("cpu"))
    sp = SamplingParams(max_tokens=150, ignore_eos=True, num_ctx=128)
    out = []
    for flag in (False, True):
        e = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=256, tp=tp, context_shift=flag)
        r = e.generate([PROMPT], sp)[0]
        out.append((r.token_ids, r.done_reason, r.context_shifts, e.context_shift, sorted(e.stats)))
    q.put((rank, out))
    dist.destroy_process_group()


def test_tensor_parallel_is_inert():
    import socket

    import torch.multiprocessing as tmp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = tmp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = dict(q.get(timeout=240) for _ in ps)
    [p.join(timeout=60) for p in ps]
    assert res[0] == res[1]
    off, on = res[0]
    assert on == off and len(off[0]) == 128 - len(PROMPT) and off[3] is False and "context_shifts" not in off[4]


# ------------------------------------------------------------------------------------------------ plumbing, HTTP
def test_options_and_settings(monkeypatch):
    import argparse

    from llm_based_apache_spark_optimization_amd.config import Settings

    assert SamplingParams().shift is True and SamplingParams.from_ollama_options({}).shift is True
    assert SamplingParams.from_ollama_options({"shift": False}).shift is False
    for bad in ("no", 0, 1, None, [False]):
        with pytest.raises(SamplingOptionError):
            SamplingParams.from_ollama_options({"shift": bad})
    assert Settings().context_shift is False
    monkeypatch.setenv("LSA_CONTEXT_SHIFT", "1")
    assert Settings().context_shift is True
    monkeypatch.delenv("LSA_CONTEXT_SHIFT")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--context-shift"])).context_shift is True


def test_client_and_http(eng, plain, tmp_path):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.client import EngineService, GenerateResponse
    from llm_based_apache_spark_optimization_amd.config import Settings
    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context
    from llm_based_apache_spark_optimization_amd.utils.metrics import REGISTRY

    svc = EngineService(lambda model: eng if model == "shift" else plain,
                        defaults={"num_predict": 230, "ignore_eos": True, "num_ctx": 128})
    try:
        s = Settings(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"),
                     history_dsn="sqlite:///" + str(tmp_path / "h.db"), engine="hip", secret_key="test",
                     nl2sql_model="shift", explain_model="shift")
        c = TestClient(create_app(make_context(s, backend=svc)))
        on = c.post("/api/generate", json={"model": "shift", "prompt": "hi"})
        assert on.status_code == 200 and on.json()["eval_count"] == 230 and on.json()["context_shifts"] >= 2
        out = c.post("/api/generate", json={"model": "shift", "prompt": "hi", "options": {"shift": False}}).json()
        assert out["context_shifts"] == 0 and out["eval_count"] < 128 and out["done_reason"] == "length"
        off = c.post("/api/generate", json={"model": "plain", "prompt": "hi"}).json()
        assert "context_shifts" not in off and off["eval_count"] == out["eval_count"]
        assert set(off) == set(out) - {"context_shifts"}
        for bad in ("false", 0, None):
            r = c.post("/api/generate", json={"model": "shift", "prompt": "hi", "options": {"shift": bad}})
            assert r.status_code == 400 and "shift" in r.json()["detail"]
        h = svc.health()["engines"]
        assert h["shift"]["context_shift"] is True and h["plain"]["context_shift"] is False
        assert h["shift"]["context_shifts"] >= 2 and "context_shifts" not in h["plain"]
        text = REGISTRY.render() if hasattr(REGISTRY, "render") else c.get("/metrics").text
        assert "lsa_context_shifts_total" in text and "lsa_context_shift_tokens_total" in text
    finally:
        for m in svc.models():
            svc.loop(m).close()
    assert "context_shifts" not in GenerateResponse(model="m", response="").to_dict()
    assert GenerateResponse(model="m", response="", context_shifts=2).to_dict()["context_shifts"] == 2
