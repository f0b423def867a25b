"""Prompt-token logprobs (teacher-forced scoring in the prefill) on the CPU: the host twins of the prompt kernel pair
against an independent float64 transcription, the engine's list against the float64 oracle and across every route a
prompt can take (whole, chunked, prefix-cached, preempted), the scheduler's ``match_limit``, and the client, HTTP and
evaluation-harness layers on the tiny model."""
import dataclasses
import json
import pathlib
import shutil
import subprocess
import types

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops, prompts
from llm_based_apache_spark_optimization_amd.client import EngineService, FakeBackend, GenerateResponse
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.engine import SamplingOptionError
from llm_based_apache_spark_optimization_amd.eval.harness import evaluate_multi, evaluate_single, summarize
from llm_based_apache_spark_optimization_amd.models.llama import reference_forward
from llm_based_apache_spark_optimization_amd.ops import reference as ref
from llm_based_apache_spark_optimization_amd.runtime import native

U = 2.0 ** -24
POISON = -777.25


def f64_rows(logits, tok, k):
    """Independent transcription: l - logsumexp(l) in double, one rounding; top-k by (value desc, index asc)."""
    R, V = logits.shape
    d = logits.double()
    lp = d - torch.logsumexp(d, dim=-1, keepdim=True)
    chosen = torch.tensor([float(lp[r, int(tok[r])]) for r in range(R)]).float()
    ids = torch.full((R, k), -1, dtype=torch.int32)
    top = torch.full((R, k), float("-inf"))
    for r in range(R):
        order = sorted(range(V), key=lambda i: (-float(logits[r, i]), i))[:k]
        for j, i in enumerate(order):
            ids[r, j] = i
            top[r, j] = float(lp[r, i])
    return chosen, ids, top


def _dst(R, K=20):
    return (torch.full((R,), POISON), torch.full((R, K), -9, dtype=torch.int32), torch.full((R, K), POISON))


def _pair(logits, targets, row_k, dst, any_k=True):
    ops.prompt_logprob_scan(logits, targets, row_k, any_k=any_k)
    ops.prompt_logprob_commit(logits, targets, row_k, *dst, any_k=any_k)


# ----------------------------------------------------------------------------------- host twins
def test_twins_against_float64_and_which_rows_record():
    torch.manual_seed(0)
    for V, sigma in ((50, 1.0), (2049, 12.0)):
        R = 6
        lg = torch.randn(R, V) * sigma
        raw = lg.clone()
        # rows 1 and 4 have no target; K mixed per row, one row with K = 0
        targets = torch.tensor([0, -1, V - 1, V // 2, -1, 7], dtype=torch.int32)
        row_k = torch.tensor([3, 5, 0, 20, 0, 1], dtype=torch.int32)
        dst = _dst(R)
        _pair(lg, targets, row_k, dst)
        assert torch.equal(lg, raw)  # the rows are only read
        for r in range(R):
            if int(targets[r]) < 0:  # no target: every destination word keeps its sentinel
                assert dst[0][r] == POISON and torch.all(dst[1][r] == -9) and torch.all(dst[2][r] == POISON)
                continue
            K = int(row_k[r])
            chosen, ids, top = f64_rows(lg[r:r + 1], targets[r:r + 1], K)
            assert torch.equal(dst[1][r, :K], ids[0])
            # two float64 evaluations of one formula, each rounded once to f32: at most an ulp of the result apart
            assert abs(float(dst[0][r]) - float(chosen[0])) <= 2 * U * abs(float(chosen[0]))
            if K:
                assert float((dst[2][r, :K].double() - top[0].double()).abs().max()) <= 2 * U * float(top[0].abs().max())
            assert torch.all(dst[1][r, K:] == -9) and torch.all(dst[2][r, K:] == POISON)
        # "no row has K > 0": the launch form without candidates records every chosen value, and no top entry
        dst0 = _dst(R)
        _pair(lg, targets, row_k, dst0, any_k=False)
        assert torch.equal(dst0[0], dst[0]) and torch.all(dst0[1] == -9) and torch.all(dst0[2] == POISON)


def test_twins_tie_order_and_k_above_v():
    lg = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5]])
    dst = _dst(1)
    _pair(lg, torch.tensor([2], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), dst)
    assert dst[1][0, :4].tolist() == [1, 2, 4, 0]  # equal values: the lower index first
    assert dst[2][0, 0] == dst[2][0, 1] == dst[2][0, 2] == dst[0][0]  # the chosen token is among them, bitwise
    dst = _dst(1)
    _pair(torch.zeros(1, 10), torch.tensor([3], dtype=torch.int32), torch.tensor([20], dtype=torch.int32), dst)
    assert dst[1][0, :10].tolist() == list(range(10)) and dst[1][0, 10:].tolist() == [-1] * 10
    assert torch.all(dst[2][0, 10:] == float("-inf")) and torch.all(dst[2][0, :10] == dst[0][0])
    # one expression with a generated-token record: the twin of the decode pair gives the same bits for the same row
    chosen, ids, top = ref.logprob_rows(lg, torch.tensor([2]), 4)
    d2 = _dst(1)
    _pair(lg, torch.tensor([2], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), d2)
    assert d2[0][0] == chosen[0] and torch.equal(d2[1][0, :4], ids[0]) and torch.equal(d2[2][0, :4], top[0])


def test_ops_refusals():
    lg = torch.randn(3, 64)
    t = torch.zeros(3, dtype=torch.int32)
    k = torch.zeros(3, dtype=torch.int32)
    dst = _dst(3)
    _pair(lg, t, k, dst)
    bad_scan = [
        (lg.double(), t, k),                       # dtype
        (lg.t().contiguous().t(), t, k),           # contiguity
        (lg, t.long(), k),                         # targets dtype
        (lg, t[:2], k),                            # targets shape
        (lg, t, torch.zeros(3, 1, dtype=torch.int32)),  # row_k shape
        (lg[0], t, k),                             # logits rank
        (torch.zeros(0, 64), t[:0], k[:0]),        # R < 1
    ]
    for args in bad_scan:
        with pytest.raises(ValueError):
            ops.prompt_logprob_scan(*args)
    with pytest.raises(ValueError):  # V above the sampler's bound
        ops.prompt_logprob_scan(torch.zeros(1, 262145), t[:1], k[:1])
    cm = lambda **kw: ops.prompt_logprob_commit(  # noqa: E731
        kw.get("lg", lg), kw.get("t", t), kw.get("k", k), kw.get("tok", dst[0]), kw.get("ids", dst[1]),
        kw.get("top", dst[2]))
    cm()
    with pytest.raises(ValueError):  # K outside 0 .. 20
        cm(ids=torch.zeros(3, 21, dtype=torch.int32), top=torch.zeros(3, 21))
    with pytest.raises(ValueError):  # records of another row count
        cm(tok=torch.zeros(4))
    with pytest.raises(ValueError):
        cm(ids=torch.zeros(2, 20, dtype=torch.int32), top=torch.zeros(2, 20))
    with pytest.raises(ValueError):
        cm(top=torch.zeros(3, 20, dtype=torch.float64))
    with pytest.raises(ValueError):
        cm(ids=torch.zeros(3, 20, dtype=torch.int64))
    ms, cand = ops.prompt_logprob_workspace(3, 5000, "cpu")
    assert ms.numel() == 3 * 3 * 2 and cand.numel() == 3 * 3 * 32 and cand.dtype == torch.int64


# ----------------------------------------------------------------------------------- engine (tiny model, CPU)
KW = dict(device="cpu", max_slots=4, max_model_len=512)
PROMPT = [1] + list(range(5, 45))
LONG = [1] + [5 + (7 * i) % 400 for i in range(150)]


@pytest.fixture(scope="module")
def eng():
    return build_engine("tiny-nsql", logprobs=True, **KW)


@pytest.fixture(scope="module")
def plain():
    return build_engine("tiny-nsql", **KW)


def _gen(e, prompts_, sps):
    reqs = [e.add_request(p, sp) for p, sp in zip(prompts_, sps)]
    e.run_until_done(reqs)
    return [e.result(q) for q in reqs]


def _check_shape(res, n, lo):
    """len == prompt_eval_count, null exactly below max(1, from)."""
    assert len(res.prompt_logprobs) == res.prompt_tokens == n
    assert [x is None for x in res.prompt_logprobs] == [j < max(1, lo) for j in range(n)]


@pytest.fixture(scope="module")
def whole(eng):
    """The whole-prompt list of LONG, computed once: the reference of the route tests."""
    sp = SamplingParams(max_tokens=3, ignore_eos=True, prompt_logprobs=True, top_logprobs=2)
    return _gen(eng, [LONG], [sp])[0]


def test_engine_against_the_float64_oracle(eng, plain, whole):
    """Every entry within 0.125 nats of the float64 log-softmax of ``reference_forward`` over the same ids: the bound
    and derivation of tests/test_logprobs_cpu.py::test_engine_values_against_teacher_forced_float64 (the oracle keeps
    f32 activations where the engine rounds to bf16, relative step 2^-8, layer after layer; a log-probability of
    magnitude <= 8 built from logits a few bf16 steps apart is held to 8 * 4 * 2^-8 = 0.125)."""
    _check_shape(whole, len(LONG), 0)
    lp64 = torch.log_softmax(reference_forward(eng.runner.w, LONG).double(), dim=-1)
    for j in range(1, len(LONG)):
        ent = whole.prompt_logprobs[j]
        want = float(lp64[j - 1, LONG[j]])
        print(f"prompt index {j}: engine {ent['logprob']:.6f} oracle {want:.6f}")
        assert abs(ent["logprob"] - want) <= 0.125, (j, ent["logprob"], want)
        assert ent["token"] == eng.tok.decode([LONG[j]]) and bytes(ent["bytes"]) == eng._bytes_of([LONG[j]])
        tops = ent["top_logprobs"]
        assert len(tops) == 2 and tops[0]["logprob"] >= tops[1]["logprob"] and tops[0]["logprob"] >= ent["logprob"]
        assert abs(tops[0]["logprob"] - float(lp64[j - 1].max())) <= 0.125  # the most likely token's value too
    # asking changes no generated token, and not asking gives no key
    base = _gen(plain, [LONG], [SamplingParams(max_tokens=3, ignore_eos=True)])[0]
    assert base.token_ids == whole.token_ids and base.prompt_logprobs is None
    assert eng.stats["prompt_logprob_requests"] >= 1 and eng.stats["prompt_logprob_rows"] >= len(LONG) - 1


def test_consistency_with_generation(eng):
    """Generate N greedy tokens with logprobs, then score prompt + those tokens from len(prompt).

    The issue expects bitwise equality on the CPU path.  It does not hold, for a reason in torch's CPU matmul and not in
    this change: a decode step runs its GEMMs over one row, the prefill over all rows at once, and torch's CPU matmul
    sums in another order at M = 1 (ops.linear of one layer differs in the last bit between M = 1 and M = 47 for all 47
    rows), which flips bf16 roundings of activations further down; the values then differ by up to ~5e-4.  So, as the
    issue provides for this case, both lists are held to the 0.125 oracle bound instead (and record 0, which the
    prefill computes in both runs over rows of the same call shape, is still compared, to 2^-8 as the existing tests
    compare runs at different batch sizes)."""
    N = 8
    gen = _gen(eng, [PROMPT], [SamplingParams(max_tokens=N, ignore_eos=True, logprobs=True)])[0]
    full = PROMPT + gen.token_ids
    sc = _gen(eng, [full], [SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=True,
                                           prompt_logprobs_from=len(PROMPT))])[0]
    _check_shape(sc, len(full), len(PROMPT))
    lp64 = torch.log_softmax(reference_forward(eng.runner.w, full).double(), dim=-1)
    for j in range(N):
        want = float(lp64[len(PROMPT) + j - 1, gen.token_ids[j]])
        a, b = gen.logprobs[j]["logprob"], sc.prompt_logprobs[len(PROMPT) + j]["logprob"]
        print(f"token {j}: generated {a:.6f} scored {b:.6f} oracle {want:.6f}")
        assert abs(a - want) <= 0.125 and abs(b - want) <= 0.125
        assert gen.logprobs[j]["token"] == sc.prompt_logprobs[len(PROMPT) + j]["token"]
    assert abs(gen.logprobs[0]["logprob"] - sc.prompt_logprobs[len(PROMPT)]["logprob"]) <= 2.0 ** -8


def test_same_list_chunked_and_from_the_middle(whole):
    sp = SamplingParams(max_tokens=3, ignore_eos=True, prompt_logprobs=True, top_logprobs=2)
    ch = _gen(build_engine("tiny-nsql", logprobs=True, prefill_chunk=64, **KW), [LONG], [sp])[0]
    assert ch.prompt_logprobs == whole.prompt_logprobs and ch.token_ids == whole.token_ids
    e = build_engine("tiny-nsql", logprobs=True, max_prefill_tokens=64, **KW)  # a prompt above max_prefill_tokens
    e.runner.score_tile_rows = 32
    mp = _gen(e, [LONG], [sp])[0]
    assert mp.prompt_logprobs == whole.prompt_logprobs
    mid = _gen(e, [LONG], [dataclasses.replace(sp, prompt_logprobs_from=70)])[0]
    _check_shape(mid, len(LONG), 70)
    assert mid.prompt_logprobs[70:] == whole.prompt_logprobs[70:]
    past = _gen(e, [LONG], [dataclasses.replace(sp, prompt_logprobs_from=len(LONG) + 5)])[0]
    assert past.prompt_logprobs == [None] * len(LONG)


def test_same_list_prefix_cached(whole):
    sp = SamplingParams(max_tokens=3, ignore_eos=True, prompt_logprobs=True, top_logprobs=2)
    e = build_engine("tiny-nsql", logprobs=True, prefix_cache=True, **KW)
    first = _gen(e, [LONG], [sp])[0]
    assert first.cached_prompt_tokens == 0 and first.prompt_logprobs == whole.prompt_logprobs
    # the same prompt again, asking from 0: every row must be computed, so nothing may come from the cache
    again = _gen(e, [LONG], [sp])[0]
    assert again.cached_prompt_tokens == 0 and again.prompt_logprobs == whole.prompt_logprobs
    # from 100: the rows from 99 on are computed; the 99 tokens before may be cached (one full block and a fork)
    mid = _gen(e, [LONG], [dataclasses.replace(sp, prompt_logprobs_from=100)])[0]
    assert 64 <= mid.cached_prompt_tokens <= 99
    _check_shape(mid, len(LONG), 100)
    assert mid.prompt_logprobs[100:] == whole.prompt_logprobs[100:]
    # a request that does not ask keeps today's match: all but the last token's block
    none = _gen(e, [LONG], [SamplingParams(max_tokens=3, ignore_eos=True)])[0]
    assert none.cached_prompt_tokens >= 128 and none.token_ids == whole.token_ids


def test_same_list_preempted_and_resumed():
    """A small arena (tests/test_kv_lazy.py): requests are preempted after their prompt completed; one is preempted
    by hand in the middle of its chunked prompt.  Every list equals, entry for entry and bit for bit, the list of the
    same requests run the same way on an arena large enough not to preempt; ``resumed`` tokens are never scored."""
    ps = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    sp = SamplingParams(max_tokens=150, ignore_eos=True, prompt_logprobs=True, top_logprobs=1)

    def run(**arena):
        e = build_engine("tiny-nsql", device="cpu", max_slots=3, max_model_len=512, logprobs=True, **arena)
        e.runner.rr_decode = False  # (tests/test_kv_lazy.py)
        e.run_ahead = 16
        reqs = [e.add_request(p, sp) for p in ps]
        e.run_until_done(reqs)
        return e, reqs, [e.result(q) for q in reqs]

    big, _, want = run()
    assert big.stats["preempted"] == 0
    e, reqs, got = run(num_kv_blocks=9)
    assert e.stats["preempted"] >= 1 and any(q.preemptions for q in reqs)
    assert e.stats["prompt_logprob_rows"] == sum(len(p) - 1 for p in ps)  # each index scored exactly once
    for r, w, p in zip(got, want, ps):
        _check_shape(r, len(p), 0)
        assert r.token_ids == w.token_ids
        assert r.prompt_logprobs == w.prompt_logprobs  # the whole list: values, tokens, bytes and top_logprobs
        assert all(len(x["top_logprobs"]) == 1 for x in r.prompt_logprobs[1:])
    # mid-prompt: chunks of 16, preempted after the second chunk; the re-admitted request scores the rest only
    c = build_engine("tiny-nsql", logprobs=True, prefill_chunk=16, **KW)
    sp = SamplingParams(max_tokens=3, ignore_eos=True, prompt_logprobs=True, top_logprobs=2)
    want = _gen(c, [PROMPT], [sp])[0]
    rows0 = c.stats["prompt_logprob_rows"]
    q = c.add_request(PROMPT, sp)
    c.step()
    c.step()
    assert 0 < q.prefilled < len(PROMPT) and q.plp_pending
    c._preempt(q)
    assert not q.plp_pending and q.plp_next == 33 and all(x is not None for x in q.prompt_lp[1:33])
    c.run_until_done([q])
    got = c.result(q)
    assert got.prompt_logprobs == want.prompt_logprobs and got.token_ids == want.token_ids
    assert c.stats["prompt_logprob_rows"] - rows0 == len(PROMPT) - 1


def test_refusals_and_fields(eng, plain):
    with pytest.raises(SamplingOptionError) as ei:
        plain.add_request(PROMPT, SamplingParams(prompt_logprobs=True))
    assert "LSA_LOGPROBS" in str(ei.value)
    for bad in (dict(prompt_logprobs=True, prompt_logprobs_from=-1), dict(prompt_logprobs=True, prompt_logprobs_from=2.5),
                dict(prompt_logprobs=True, prompt_logprobs_from=True), dict(top_logprobs=3),
                dict(prompt_logprobs=True, top_logprobs=21)):
        with pytest.raises(SamplingOptionError):
            eng.add_request(PROMPT, SamplingParams(**bad))
    for bad in (-3, "7", 1.5, True):
        with pytest.raises(SamplingOptionError):
            SamplingParams.from_ollama_options({"prompt_logprobs": True, "prompt_logprobs_from": bad})
    sp = SamplingParams.from_ollama_options({"prompt_logprobs": True, "prompt_logprobs_from": 9, "top_logprobs": 2})
    assert sp.prompt_logprobs and sp.prompt_logprobs_from == 9 and sp.top_logprobs == 2 and not sp.logprobs
    d = SamplingParams.from_ollama_options({})
    assert not d.prompt_logprobs and d.prompt_logprobs_from == 0
    # top_logprobs with prompt_logprobs alone is served
    r = _gen(eng, [PROMPT], [SamplingParams(max_tokens=2, ignore_eos=True, prompt_logprobs=True, top_logprobs=3)])[0]
    assert r.logprobs is None and len(r.prompt_logprobs[5]["top_logprobs"]) == 3
    # tensor parallelism: refused at the request (the sequence-parallel prefill keeps T / tp rows per rank)
    assert eng.prompt_logprobs_supported and not plain.prompt_logprobs_supported
    eng.runner.tp = types.SimpleNamespace(size=2, rank=0)
    try:
        assert not eng.prompt_logprobs_supported
        with pytest.raises(SamplingOptionError):
            eng.add_request(PROMPT, SamplingParams(prompt_logprobs=True))
    finally:
        eng.runner.tp = None
    # the tile workspace is accounted for once a prefill has scored
    S, cap, V = eng.runner.max_slots, eng.runner.max_new_cap, eng.runner.V
    nch = -(-V // 2048)
    base = S * (8 + cap * 4 * (1 + 2 * 20) + V * 4 + nch * (8 + 32 * 8))
    ws = eng.runner.prompt_lp_ws
    assert eng.runner.logprobs_bytes() == base + ws[0].numel() * 4 + ws[1].numel() * 8
    assert eng.runner.score_tile_rows == 256 and ws[0].numel() <= 256 * nch * 2


def test_nobody_asks_calls_the_runner_as_before(eng):
    """A request that does not ask reaches the runner through today's calls: no ``score`` argument, no records."""
    calls, pf, pc = [], eng.runner.prefill, eng.runner.prefill_chunk
    eng.runner.prefill = lambda *a, **kw: (calls.append(("prefill", len(a), sorted(kw))), pf(*a, **kw))[1]
    eng.runner.prefill_chunk = lambda *a, **kw: (calls.append(("chunk", len(a), sorted(kw))), pc(*a, **kw))[1]
    try:
        rows = eng.stats["prompt_logprob_rows"]
        _gen(eng, [PROMPT], [SamplingParams(max_tokens=2, ignore_eos=True)])
        assert calls == [("prefill", 2, [])] and eng.stats["prompt_logprob_rows"] == rows
        _gen(eng, [PROMPT, LONG], [SamplingParams(max_tokens=2, ignore_eos=True, prompt_logprobs=True),
                                   SamplingParams(max_tokens=2, ignore_eos=True)])
        assert calls[-1] == ("prefill", 2, ["score"])
    finally:
        del eng.runner.prefill, eng.runner.prefill_chunk


# ----------------------------------------------------------------------------------- scheduler
@pytest.mark.parametrize("cls", [native.Scheduler, native._PyScheduler], ids=["native", "python"])
def test_scheduler_match_limit(cls):
    bs = 4
    toks = list(range(100, 118))  # 18 tokens: four full blocks and two tokens

    def sched(cow=1):
        s = cls(64, bs, 4, 4096, 16, 8, prefix_cache=True, cow_min_tokens=cow)
        s.add(1, len(toks), 4, toks, True)
        assert s.admit() == [1] and s.cached_tokens(1) == 0
        s.publish(1)
        s.finish(1)
        return s

    def hit(s, rid, *extra, tokens=toks):
        s.add(rid, len(tokens), 4, tokens, True, *extra)
        assert s.admit() == [rid]
        n = s.cached_tokens(rid)
        s.copies_done() if not s.take_copies() else s.copies_done()
        s.finish(rid)
        return n

    s = sched()
    today = hit(s, 2)
    assert today == 16  # (18 - 1) // 4 full blocks; nothing of a fifth block is cached
    assert hit(s, 3, -1) == today and hit(s, 4, len(toks) - 1) == today and hit(s, 5, 1000) == today
    assert hit(s, 6, 0) == 0                    # every row computed
    assert hit(s, 7, 8) == 8                    # a full-prompt hit cut at the limit: two full blocks
    assert hit(s, 8, 10) == 10                  # ... and the fork (partial block) cut too: 8 + 2 of the third block
    assert hit(s, 9, 11) == 11 and hit(s, 10, 12) == 12
    assert hit(s, 11, 3) == 3                   # a fork of the first block alone
    assert hit(sched(cow=3), 12, 10) == 8       # a fork shorter than cow_min_tokens is not taken
    assert hit(s, 13) == today                  # the default reproduces today's match, after all of the above
    # a preempted request takes its limit for the resumed prompt
    s = sched()
    s.add(20, len(toks), 8, toks, True, 8)
    assert s.admit() == [20] and s.cached_tokens(20) == 8
    s.copies_done()
    longer = toks + [7, 8, 9]
    s.preempt(20, len(longer), 5, longer, 5)
    assert s.admit() == [20] and s.cached_tokens(20) == 5
    s.take_copies()
    s.copies_done()
    s.preempt(20, len(longer), 5, longer)
    assert s.admit() == [20] and s.cached_tokens(20) == 16


def test_match_limit_selftest_under_sanitizers(tmp_path):
    """csrc/tests/match_limit_selftest.cpp: the scheduler's cap over random block sizes, fork thresholds and prompt
    lengths, as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = pathlib.Path(__file__).resolve().parent.parent / "csrc" / "tests" / "match_limit_selftest.cpp"
    exe = tmp_path / "match_limit_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match_limit selftest ok" in r.stdout


def test_engine_passes_the_match_limit():
    e = build_engine("tiny-nsql", logprobs=True, prefix_cache=True, **KW)
    seen, add = [], e.sched.add
    e.sched = types.SimpleNamespace(**{n: getattr(e.sched, n) for n in dir(e.sched) if not n.startswith("_")})
    e.sched.add = lambda *a: (seen.append(a[5:]), add(*a))[1]
    for lo, want in ((0, (0,)), (1, (0,)), (2, (1,)), (30, (29,)), (40, (39,)), (41, ()), (400, ())):
        e.add_request(PROMPT, SamplingParams(prompt_logprobs=True, prompt_logprobs_from=lo))
        assert seen[-1] == want, (lo, seen[-1])
    e.add_request(PROMPT, SamplingParams())
    assert seen[-1] == ()


# ----------------------------------------------------------------------------------- client and HTTP
@pytest.fixture(scope="module")
def svc(eng, plain):
    s = EngineService(lambda model: eng if model == "lp" else plain, defaults={"num_predict": 6, "ignore_eos": True})
    yield s
    for m in s.models():
        s.loop(m).close()


def _consistent(sc, eng, completion):
    lps = [e["logprob"] for e in sc["token_logprobs"]]
    assert sc["completion"] == completion
    assert sc["tokens"] == len(lps) == len(eng.tok.encode(completion, add_bos=False))
    assert sc["logprob"] == pytest.approx(sum(lps)) and sc["mean_logprob"] == pytest.approx(sum(lps) / len(lps))
    assert sc["min_logprob"] == min(lps) <= sc["mean_logprob"] <= 0.0


def test_response_key_and_streaming(svc):
    r = svc.generate("lp", "select all rows")
    assert "prompt_logprobs" not in r.to_dict() and r.prompt_logprobs is None
    assert set(r.to_dict()) == {f.name for f in dataclasses.fields(GenerateResponse)} - {"logprobs"}
    r = svc.generate("lp", "select all rows", options={"prompt_logprobs": True, "top_logprobs": 2})
    d = r.to_dict()
    assert "logprobs" not in d and len(d["prompt_logprobs"]) == r.prompt_eval_count
    assert d["prompt_logprobs"][0] is None
    assert set(d["prompt_logprobs"][1]) == {"token", "logprob", "bytes", "top_logprobs"}
    json.dumps(d)
    both = svc.generate("lp", "select all rows", options={"prompt_logprobs": True, "logprobs": True})
    assert len(both.logprobs) == both.eval_count and "top_logprobs" not in both.prompt_logprobs[1]
    assert [e["logprob"] for e in both.prompt_logprobs[1:]] == [e["logprob"] for e in r.prompt_logprobs[1:]]
    assert both.response == r.response  # asking does not change what is generated
    # streamed: the whole list rides in the final chunk, and only there
    chunks = list(svc.generate_stream("lp", "select all rows", options={"prompt_logprobs": True, "top_logprobs": 2}))
    assert chunks[-1].done and chunks[-1].prompt_logprobs == r.prompt_logprobs
    assert all(c.prompt_logprobs is None and "prompt_logprobs" not in c.to_dict() for c in chunks[:-1])
    assert "prompt_logprobs" in chunks[-1].to_dict()
    assert all("prompt_logprobs" not in c.to_dict() for c in svc.generate_stream("lp", "select all rows"))
    back = GenerateResponse(**chunks[-1].to_dict())  # how the replica router rebuilds the final chunk
    assert back.prompt_logprobs == r.prompt_logprobs


def test_score_service(svc, eng):
    one = svc.score("lp", "how many rows", "SELECT COUNT(*) FROM t;", system="Table t")
    assert set(one) == {"model", "prompt_eval_count", "scores", "total_duration"} and len(one["scores"]) == 1
    ids = eng.tok.encode(eng.render("how many rows", "Table t", False), add_bos=True)
    assert one["prompt_eval_count"] == len(ids)
    _consistent(one["scores"][0], eng, "SELECT COUNT(*) FROM t;")
    assert "top_logprobs" not in one["scores"][0]["token_logprobs"][0]
    comps = ["SELECT COUNT(*) FROM t;", "SELECT 1;", "DROP TABLE t"]
    many = svc.score("lp", "how many rows", comps, system="Table t", top_logprobs=2)
    assert [s["completion"] for s in many["scores"]] == comps
    for s, c in zip(many["scores"], comps):
        _consistent(s, eng, c)
        assert len(s["token_logprobs"][0]["top_logprobs"]) == 2
    # scored in a batch beside others the values are the solo run's up to the CPU GEMMs' batch-size dependence
    assert many["scores"][0]["logprob"] == pytest.approx(one["scores"][0]["logprob"], abs=2.0 ** -8 * one["scores"][0]["tokens"])
    # the scores are the entries an ordinary request over prompt + completion reports
    cids = eng.tok.encode(comps[1], add_bos=False)
    r = _gen(eng, [ids + cids], [SamplingParams(max_tokens=1, prompt_logprobs=True, prompt_logprobs_from=len(ids))])[0]
    assert [e["token"] for e in r.prompt_logprobs[len(ids):]] == [e["token"] for e in many["scores"][1]["token_logprobs"]]
    for bad in ("", []):
        with pytest.raises(SamplingOptionError):
            svc.score("lp", "q", bad)
    # submitted together, all or none: a refused prompt withdraws the ones queued before it
    live = eng._plp_live
    with pytest.raises(ValueError):
        eng.add_requests([PROMPT, [1] * 600], SamplingParams(max_tokens=1, prompt_logprobs=True))
    assert not eng.has_work() and eng._plp_live == live
    with pytest.raises(SamplingOptionError):
        svc.score("lp", "q", ["x"] * 65)
    with pytest.raises(SamplingOptionError):
        svc.score("lp", "q", ["ok", ""])
    with pytest.raises(SamplingOptionError):
        svc.score("plain", "q", "SELECT 1")
    with pytest.raises(SamplingOptionError):  # never truncated: refused
        svc.score("lp", "q " * 40, "SELECT 1", options={"num_ctx": 32})
    with pytest.raises(SamplingOptionError):
        svc.score("lp", "q", "SELECT 1", top_logprobs=21)
    with pytest.raises(SamplingOptionError):
        FakeBackend().score("duckdb-nsql", "q", "SELECT 1")
    with pytest.raises(SamplingOptionError):
        FakeBackend().generate("duckdb-nsql", "q", options={"prompt_logprobs": True})
    h = svc.health()["engines"]
    assert h["lp"]["prompt_logprobs"] is True and h["plain"]["prompt_logprobs"] is False
    assert h["lp"]["prompt_logprob_requests"] >= 4 and h["lp"]["prompt_logprob_rows"] > 0


def test_http_layer(svc, eng, tmp_path):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context

    s = Settings(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"),
                 history_dsn="sqlite:///" + str(tmp_path / "h.db"), engine="hip", secret_key="test",
                 nl2sql_model="lp", explain_model="lp", logprobs=True)
    c = TestClient(create_app(make_context(s, backend=svc)))
    r = c.post("/api/score", json={"model": "lp", "prompt": "how many rows", "completion": "SELECT COUNT(*) FROM t;"})
    assert r.status_code == 200, r.text
    body = r.json()
    assert set(body) == {"model", "prompt_eval_count", "scores", "total_duration"}
    _consistent(body["scores"][0], eng, "SELECT COUNT(*) FROM t;")
    r = c.post("/api/score", json={"model": "lp", "prompt": "how many rows", "top_logprobs": 1,
                                   "completions": ["SELECT 1;", "SELECT COUNT(*) FROM t;"]})
    assert r.status_code == 200 and len(r.json()["scores"]) == 2
    _consistent(r.json()["scores"][1], eng, "SELECT COUNT(*) FROM t;")
    assert r.json()["scores"][1]["logprob"] == pytest.approx(body["scores"][0]["logprob"], abs=0.05)
    bad = [
        {"model": "lp", "prompt": "q", "completion": ""},                                    # empty completion
        {"model": "lp", "prompt": "q", "completions": ["x"] * 65},                           # more than 64
        {"model": "lp", "prompt": "q", "completions": []},
        {"model": "lp", "prompt": "q"},                                                      # neither
        {"model": "lp", "prompt": "q", "completion": "a", "completions": ["a"]},             # both
        {"model": "lp", "prompt": "q " * 40, "completion": "SELECT 1", "options": {"num_ctx": 32}},  # does not fit
        {"model": "plain", "prompt": "q", "completion": "SELECT 1"},                         # engine without logprobs
        {"model": "lp", "prompt": "q", "completion": "SELECT 1", "top_logprobs": 21},
    ]
    for b in bad:
        assert c.post("/api/score", json=b).status_code == 400, b
    # /api/generate: top level and inside options; the key is absent when not asked
    g = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "prompt_logprobs": True, "top_logprobs": 1})
    assert g.status_code == 200 and len(g.json()["prompt_logprobs"]) == g.json()["prompt_eval_count"]
    assert g.json()["prompt_logprobs"][0] is None and "logprobs" not in g.json()
    g2 = c.post("/api/generate", json={"model": "lp", "prompt": "hi",
                                       "options": {"prompt_logprobs": True, "top_logprobs": 1}})
    assert g2.json()["prompt_logprobs"] == g.json()["prompt_logprobs"]
    g3 = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "prompt_logprobs": True,
                                       "options": {"prompt_logprobs_from": 3}}).json()
    assert g3["prompt_logprobs"][:3] == [None] * 3 and g3["prompt_logprobs"][3] is not None
    assert "prompt_logprobs" not in c.post("/api/generate", json={"model": "lp", "prompt": "hi"}).json()
    lines = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "prompt_logprobs": True, "top_logprobs": 1,
                                          "stream": True}).text.strip().split("\n")
    last = json.loads(lines[-1])
    assert last["done"] and last["prompt_logprobs"] == g.json()["prompt_logprobs"]
    assert all("prompt_logprobs" not in json.loads(x) for x in lines[:-1])
    for b in ({"model": "plain", "prompt": "hi", "prompt_logprobs": True},
              {"model": "lp", "prompt": "hi", "prompt_logprobs": True, "options": {"prompt_logprobs_from": -1}},
              {"model": "lp", "prompt": "hi", "prompt_logprobs": True, "options": {"prompt_logprobs_from": 1.5}},
              {"model": "lp", "prompt": "hi", "top_logprobs": 2},
              {"model": "lp", "prompt": "hi", "prompt_logprobs": True, "top_logprobs": 21}):
        assert c.post("/api/generate", json=b).status_code == 400, b
    assert "lsa_prompt_logprob_tokens_total" in c.get("/metrics").text


# ----------------------------------------------------------------------------------- evaluation harness
def test_harness_score(capsys):
    # the evaluation prompts are ~900 byte-level tokens and the expected statements up to ~190: scoring never truncates,
    # so the harness engine gets a window that holds them
    big = build_engine("tiny-nsql", logprobs=True, device="cpu", max_slots=4, max_model_len=2048)
    svc = EngineService(lambda model: big, defaults={"ignore_eos": True})
    try:
        _harness_score(svc, capsys)
    finally:
        for m in svc.models():
            svc.loop(m).close()


def _harness_score(svc, capsys):
    gen = lambda **kw: svc.generate(kw["model"], kw["prompt"], kw["system"], kw["options"])  # noqa: E731
    score = lambda **kw: svc.score(kw["model"], kw["prompt"], kw["completions"], kw["system"], kw["options"])  # noqa: E731
    opts = {"num_predict": 4}
    off1 = evaluate_single(gen, "lp", opts, verbose=False)
    off = evaluate_multi(gen, ["lp"], options=opts, verbose=False)
    s_off = summarize(off, len(prompts.EVAL_QUERIES))
    out_off = capsys.readouterr().out
    new = {"expected_logprob", "expected_mean_logprob", "expected_tokens"}
    assert not new & set(off1) and not new & set(off["lp"]["queries"][0]) and not new & set(s_off["lp"])
    assert "Expected SQL" not in out_off
    on1 = evaluate_single(gen, "lp", opts, verbose=False, score=score)
    on = evaluate_multi(gen, ["lp"], options=opts, verbose=False, score=score)
    s_on = summarize(on, len(prompts.EVAL_QUERIES))
    out_on = capsys.readouterr().out
    assert set(on1) - set(off1) == new and set(s_on["lp"]) - set(s_off["lp"]) == new
    assert on1["expected_tokens"] == len(svc.loop("lp").engine.tok.encode(prompts.EVAL_EXPECTED_SQL, add_bos=False))
    assert on1["expected_logprob"] < 0 and on1["expected_mean_logprob"] == pytest.approx(
        on1["expected_logprob"] / on1["expected_tokens"])
    for q_on, q_off, q in zip(on["lp"]["queries"], off["lp"]["queries"], prompts.EVAL_QUERIES):
        assert set(q_on) - set(q_off) == new and q_on["generated_sql"] == q_off["generated_sql"]
        assert q_on["expected_tokens"] == len(svc.loop("lp").engine.tok.encode(q["expected_sql"].strip(), add_bos=False))
    qs = on["lp"]["queries"]
    assert s_on["lp"]["expected_tokens"] == sum(q["expected_tokens"] for q in qs)
    assert s_on["lp"]["expected_logprob"] == pytest.approx(sum(q["expected_logprob"] for q in qs) / len(qs))
    # one extra line per model; every other line of the summary is the line printed without the flag, latencies aside
    extra = [ln for ln in out_on.splitlines() if ln.startswith("Expected SQL log-likelihood:")]
    assert len(extra) == 1
    strip = lambda out: [ln for ln in out.splitlines() if "Latency" not in ln and "decode tok/s" not in ln]  # noqa: E731
    assert [ln for ln in strip(out_on) if ln not in extra] == strip(out_off)
    json.dumps({"single": [on1], "multi": on, "summary": s_on})
