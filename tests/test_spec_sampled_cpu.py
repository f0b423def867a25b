"""Speculative decoding for requests that need the sampler, on the CPU (``spec_sampled``): the host twin of the sampled
verify commit (ops.reference.spec_sample_commit) against the plain rule -- successive ``ref.sample_commit`` steps over
the same rows -- and the engine's sampled verify steps against its plain sampled steps of the same seed: the same
tokens, whatever is drafted.  The GPU file shares the engine case defined here."""
import argparse
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.eval import numerics
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_cpu import K, PROMPT, SYSTEM, forced_table

I32 = dict(dtype=torch.int32)
BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"  # test_guided_cpu.py's pattern
M = ref.SAMPLE_MARGIN
NAMES = ("out_tokens", "gen_len", "input_ids", "positions", "finished", "hist")

# ---------------------------------------------------------------------------------------------- twin vs plain steps
V, W, T, N0, MAX_NEW = 300, 64, K + 1, 2, 16
SAMPLED = (0.8, 40, 0.9)  # temperature, top_k, top_p


def make_case(pos, pen, last_n, temp=SAMPLED[0], finished=0, limit=MAX_NEW, eos=(-1,)):
    """T verify rows over V tokens, a full ring of recent tokens drawn from the 40 ids whose logits lead the rows (so a
    penalty moves the draws), and the decode state of a row at position ``pos`` that has generated N0 tokens."""
    g = torch.Generator().manual_seed(7 + pos)
    logits = torch.randn(T, V, generator=g) * 2
    logits[:, :40] += 3.0
    hist = torch.randint(0, 40, (1, W), generator=g, dtype=torch.int32)
    if pos + 1 < W:  # the slots of positions the context has not reached are empty
        for p in range(pos + 1, W):
            hist[0, p] = -1
    st = dict(out_tokens=torch.full((1, MAX_NEW), -1, **I32), gen_len=torch.tensor([N0], **I32),
              input_ids=torch.tensor([5], **I32), positions=torch.tensor([pos], **I32),
              finished=torch.tensor([finished], **I32), hist=hist)
    par = dict(penalty=torch.tensor([pen]), temperature=torch.tensor([temp]), top_k=torch.tensor([SAMPLED[1]], **I32),
               top_p=torch.tensor([SAMPLED[2]]), seeds=torch.tensor([ref.pack_seed(1234 + pos, 3)], dtype=torch.int64),
               last_n=torch.tensor([last_n], **I32), eos=torch.tensor(list(eos), **I32),
               limit=torch.tensor([limit], **I32), eos_on=torch.ones(1, **I32))
    return logits, st, par


def clone(st):
    return {k: v.clone() for k, v in st.items()}


def plain_steps(logits, st, par, n):
    """n successive plain sampled steps over rows 0 .. n-1 (the state is advanced in place); returns the tokens."""
    toks = []
    for i in range(n):
        g0, fin = int(st["gen_len"]), int(st["finished"])
        ref.sample_commit(logits[i:i + 1].clone(), st["hist"], par["penalty"], par["temperature"], par["top_k"],
                          par["top_p"], par["seeds"], st["out_tokens"], st["gen_len"], st["input_ids"],
                          st["positions"], st["finished"], par["eos"], par["limit"], par["eos_on"],
                          last_n=par["last_n"])
        toks.append(None if fin else int(st["out_tokens"][0, g0]))
    return toks


def verify_step(logits, st, par, draft, device="cpu"):
    """One ``ops.spec_sample_commit`` over all T rows (the state is advanced in place); returns the stats."""
    d = lambda t: t.to(device)  # noqa: E731
    dst = {k: d(v) for k, v in st.items()}
    stats = torch.zeros(3, dtype=torch.int64, device=device)
    ops.spec_sample_commit(d(logits.clone()), d(torch.tensor(draft, **I32)), stats, dst["hist"], d(par["penalty"]),
                           d(par["temperature"]), d(par["top_k"]), d(par["top_p"]), d(par["seeds"]),
                           dst["out_tokens"], dst["gen_len"], dst["input_ids"], dst["positions"], dst["finished"],
                           d(par["eos"]), d(par["limit"]), d(par["eos_on"]), last_n=d(par["last_n"]))
    for k in st:
        st[k].copy_(dst[k].cpu())
    return stats.tolist()


def assert_same(got, want, what=""):
    for name in NAMES:
        assert torch.equal(got[name], want[name]), f"{what}{name}: {got[name].tolist()} != {want[name].tolist()}"


def plain_tokens(logits, st, par):
    """The T tokens the plain steps draw over the rows (no EOS, no limit in the way)."""
    free = dict(par, eos=torch.tensor([-1], **I32), limit=torch.tensor([MAX_NEW], **I32))
    return plain_steps(logits, clone(st), free, T)


def drafts_accepting(toks, a):
    """k drafts of which exactly the first ``a`` are the rows' own picks."""
    return [toks[i] if i < a else (toks[i] + 1) % V for i in range(K)]


@pytest.mark.parametrize("pos", [0, 62, 63, 64, 127])
@pytest.mark.parametrize("pen,last_n,temp", [(1.0, 64, 0.8), (1.3, 0, 0.8), (1.3, 1, 0.8), (1.3, 5, 0.8), (1.3, 64, 0.8),
                                             (1.3, 64, 0.0)])
def test_twin_equals_plain_steps(pos, pen, last_n, temp):
    logits, st0, par = make_case(pos, pen, last_n, temp)
    toks = plain_tokens(logits, st0, par)
    for a in range(K + 1):
        want, got = clone(st0), clone(st0)
        assert plain_steps(logits, want, par, a + 1) == toks[:a + 1]
        stats = verify_step(logits, got, par, drafts_accepting(toks, a))
        assert_same(got, want, f"a = {a}: ")
        assert stats == [1, K, a]
        assert int(got["gen_len"]) == N0 + a + 1 and int(got["positions"]) == pos + a + 1


def test_penalty_moves_the_draws_and_the_ring_wraps():
    """The cases above check what they claim: with the penalty the plain tokens differ from the unpenalised ones, a
    later row's penalty depends on an accepted draft, and from position 62 the ring slot of an accepted token wraps."""
    moved = 0
    for pos in (0, 62, 63, 64, 127):
        logits, st0, par = make_case(pos, 1.3, 64)
        moved += plain_tokens(logits, st0, par) != plain_tokens(logits, st0, dict(par, penalty=torch.tensor([1.0])))
    assert moved >= 3
    logits, st0, par = make_case(62, 1.3, 64)
    toks = plain_tokens(logits, st0, par)
    st = clone(st0)
    verify_step(logits, st, par, drafts_accepting(toks, K))
    assert [int(st["hist"][0, (63 + i) % W]) for i in range(T)] == toks  # slots 63, 0, 1, 2
    # row 2 penalises draft 0 and draft 1, whatever the ring holds: a row whose drafts differ draws from other logits
    row = lambda d: ref.spec_penalised_row(logits[2].clone(), st0["hist"][0], torch.tensor(d, **I32), 2, 1.3, 62, 64)  # noqa: E731
    unseen = [t for t in range(40) if t not in set(st0["hist"][0].tolist())] or [41]
    assert not torch.equal(row([unseen[0], 41, 0]), row([42, 43, 0]))


@pytest.mark.parametrize("pos", [0, 62, 63, 64, 127])
@pytest.mark.parametrize("last_n", [0, 1, 5, 64])
def test_penalised_row_is_the_ring_after_the_drafts(pos, last_n):
    """spec_penalised_row(row i) == ref.repeat_penalty over a ring into which drafts 0 .. i-1 were written."""
    logits, st0, _ = make_case(pos, 1.3, last_n)
    draft = torch.tensor([3, V + 5, 7], **I32)  # an out-of-range draft penalises nothing
    for i in range(T):
        ring = st0["hist"][0].clone()
        for j in range(i):
            ring[(pos + 1 + j) % W] = draft[j]
        want = ref.repeat_penalty(logits[i].clone(), ring, 1.3, pos + i, last_n)
        got = ref.spec_penalised_row(logits[i].clone(), st0["hist"][0], draft, i, 1.3, pos, last_n)
        assert torch.equal(got, want), i
    minus = torch.tensor([3, -1, 7], **I32)
    assert torch.equal(ref.spec_penalised_row(logits[3].clone(), st0["hist"][0], minus, 3, 1.3, pos, 2),
                       ref.repeat_penalty(logits[3].clone(), torch.full((W,), 7, **I32), 1.3, pos + 3, 1))


@pytest.mark.parametrize("pen", [1.0, 1.3])
def test_stop_rules(pen):
    logits, st0, par = make_case(63, pen, 64)
    toks = plain_tokens(logits, st0, par)
    right = drafts_accepting(toks, K)
    # EOS drawn at an accepted row: nothing follows it
    pe = dict(par, eos=torch.tensor([toks[1], V + 1], **I32))
    want, got = clone(st0), clone(st0)
    plain_steps(logits, want, pe, T)
    e = toks.index(toks[1])  # 1, unless row 0 drew the same token
    assert verify_step(logits, got, pe, right) == [1, K, e]
    assert_same(got, want, "eos: ")
    assert int(got["finished"]) == 1 and int(got["gen_len"]) == N0 + e + 1 and int(got["positions"]) == 63 + e
    # ... unless the row ignores EOS
    pn = dict(pe, eos_on=torch.zeros(1, **I32))
    want, got = clone(st0), clone(st0)
    plain_steps(logits, want, pn, T)
    assert e < K and verify_step(logits, got, pn, right) == [1, K, K]
    assert_same(got, want, "eos_on = 0: ")
    # a length limit reached mid-step
    pl = dict(par, limit=torch.tensor([N0 + 3], **I32))
    want, got = clone(st0), clone(st0)
    plain_steps(logits, want, pl, T)
    assert verify_step(logits, got, pl, right) == [1, K, 2]
    assert_same(got, want, "limit: ")
    assert int(got["finished"]) == 1 and int(got["gen_len"]) == N0 + 3
    # a finished row: nothing changes
    lf, sf, pf = make_case(63, pen, 64, finished=1)
    got = clone(sf)
    assert verify_step(lf, got, pf, right) == [0, 0, 0]
    assert_same(got, sf, "finished: ")


@pytest.mark.parametrize("pen", [1.0, 1.3])
@pytest.mark.parametrize("j", range(K))
@pytest.mark.parametrize("bad", [-1, V + 5])
def test_unusable_draft_is_never_accepted(pen, j, bad):
    logits, st0, par = make_case(64, pen, 64)
    toks = plain_tokens(logits, st0, par)
    draft = drafts_accepting(toks, K)
    draft[j] = bad
    want, got = clone(st0), clone(st0)
    plain_steps(logits, want, par, j + 1)
    assert verify_step(logits, got, par, draft) == [1, K - (bad < 0), j]
    assert_same(got, want)


def test_sizes_refused():
    logits, st, par = make_case(5, 1.0, 64)
    for rows in (logits[:1], torch.cat([logits, logits, logits[:1]])):
        with pytest.raises(RuntimeError):
            verify_step(rows, clone(st), par, [1] * 8)


# ------------------------------------------------------------------------------------------------------- engine
PARAM_SETS = {
    "ollama": dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1),  # Ollama's default option set
    "pure": dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0),
    "greedy_pen": dict(temperature=0.0, repeat_penalty=1.3),
}
SEED = 11
# the case of the GPU file's engine tests (shared, so that the decided share below is measured on its rows)
GPU_CASE = dict(temperature=0.8, top_k=40, top_p=0.9, seed=SEED)


def make(**kw):
    return build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, seed=0, **kw)


def gen(eng, n=96, **opts):
    sp = SamplingParams(max_tokens=n, ignore_eos=True, **opts)
    return eng.generate([PROMPT], sp, system=SYSTEM)[0].token_ids


def counts(eng):
    return [eng.stats[k] for k in ("spec_steps", "spec_drafted", "spec_accepted")]


@pytest.fixture(scope="module")
def plain():
    """The plain sampled tokens of every parameter set (an engine without speculation)."""
    eng = make()
    out = {name: gen(eng, seed=SEED, **ps) for name, ps in PARAM_SETS.items()}
    assert eng.stats["spec_steps"] == 0
    assert len({tuple(v) for v in out.values()}) == len(out)  # the sets draw different sequences
    return out


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_engine_ngram_equals_plain(plain, name):
    eng = make(spec_tokens=K, spec_sampled=True)
    assert gen(eng, seed=SEED, **PARAM_SETS[name]) == plain[name]
    steps, drafted, accepted = counts(eng)
    assert steps > 0 and steps + accepted == 95  # every token after the prefill's is a step's first or accepted
    assert eng.stats["generated_tokens"] == 96


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
@pytest.mark.parametrize("kind,per_step", [("right", K), ("wrong", 0), ("first", 1)])
def test_engine_forced_drafts(plain, name, kind, per_step):
    eng = make(spec_tokens=K, spec_sampled=True)
    eng.runner.set_spec_forced(forced_table(plain[name], kind, eng.runner.V))
    assert gen(eng, seed=SEED, **PARAM_SETS[name]) == plain[name]
    steps = -(-95 // (per_step + 1))
    assert counts(eng) == [steps, K * steps, 95 - steps]


def test_engine_gating(plain):
    ps = PARAM_SETS["ollama"]
    # the flag off (the default): a request that needs the sampler takes plain steps
    eng = make(spec_tokens=K)
    assert eng.runner.spec_sampled is False
    assert gen(eng, seed=SEED, **ps) == plain["ollama"] and eng.stats["spec_steps"] == 0
    # "speculate": false
    eng = make(spec_tokens=K, spec_sampled=True)
    sp = SamplingParams.from_ollama_options({"num_predict": 96, "speculate": False, "ignore_eos": True, "seed": SEED, **ps})
    assert eng.generate([PROMPT], sp, system=SYSTEM)[0].token_ids == plain["ollama"]
    assert eng.stats["spec_steps"] == 0
    # ... and the same engine speculates for the request that does not opt out, sampled or greedy
    assert gen(eng, seed=SEED, **ps) == plain["ollama"] and eng.stats["spec_steps"] > 0
    s0 = eng.stats["spec_steps"]
    assert gen(eng, 24) == gen(make(), 24) and eng.stats["spec_steps"] > s0
    # inert without spec_tokens
    eng = make(spec_sampled=True)
    assert gen(eng, seed=SEED, **ps) == plain["ollama"] and eng.stats["spec_steps"] == 0


def test_engine_second_request_mid_run(plain):
    """verify steps -> bucket-2 plain sampled steps (a second request joins) -> verify steps again."""
    ps, want = PARAM_SETS["ollama"], plain["ollama"]
    eng = make(spec_tokens=K, spec_sampled=True)
    eng.runner.set_spec_forced(forced_table(want, "first", eng.runner.V))  # two tokens per verify step
    ids = eng.encode(eng.render(PROMPT, SYSTEM, False))
    a = eng.add_request(ids, SamplingParams(max_tokens=96, ignore_eos=True, seed=SEED, **ps))
    eng.run_ahead = 8
    eng.step()
    s0 = eng.stats["spec_steps"]
    assert 0 < s0 < 48 and not a.done.is_set()
    spb = SamplingParams(max_tokens=5, ignore_eos=True, temperature=0.7, seed=3)
    b = eng.add_request(ids[:20], spb)
    eng.run_until_done([b])
    assert eng.stats["spec_steps"] == s0 and not a.done.is_set()  # both ran plain sampled steps of bucket 2
    eng.run_until_done([a])
    assert eng.stats["spec_steps"] > s0
    assert a.output_ids == want
    assert b.output_ids == make().generate([ids[:20]], spb)[0].token_ids


def test_preempted_request_resumes_its_stream():
    """Two sampled requests in an arena too small for both: the younger is preempted mid-run and re-admitted alone;
    its verify steps continue the draw stream through the seed word's offset.  The reference is the same workload on
    the engine without speculation (a sampled row of a two-row CPU step is not bit-equal to its solo run, so solo
    runs are no reference here): the preemption falls on the same token in both."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(2)]
    sp = SamplingParams(max_tokens=150, ignore_eos=True, seed=SEED, **PARAM_SETS["ollama"])
    runs = []
    for kw in (dict(), dict(spec_tokens=K, spec_sampled=True)):
        eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, num_kv_blocks=6, **kw)
        eng.run_ahead = 16
        reqs = [eng.add_request(p, sp) for p in prompts]
        eng.run_until_done(reqs)
        runs.append((eng, reqs))
    (peng, preqs), (eng, reqs) = runs
    assert [q.output_ids for q in reqs] == [q.output_ids for q in preqs]
    assert [len(q.resumed) for q in reqs] == [len(q.resumed) for q in preqs]
    assert peng.stats["spec_steps"] == 0 and peng.stats["preempted"] >= 1
    assert eng.stats["preempted"] >= 1 and any(q.preemptions for q in reqs)
    victim = next(q for q in reqs if q.preemptions)
    assert 0 < len(victim.resumed) < 150 and victim.spec_steps > 0  # it speculated after its re-admission
    assert eng.sched.free_blocks == 5 and eng.sched.num_running == 0


def test_engine_guided_and_sampled():
    ps = dict(seed=SEED, **PARAM_SETS["ollama"])
    run = lambda e: e.generate([PROMPT], SamplingParams(max_tokens=64, regex=BOUNDED, **ps), system=SYSTEM)[0]  # noqa: E731
    want = run(make(guided=True))
    assert re.fullmatch(BOUNDED, want.text)
    eng = make(guided=True, spec_tokens=K, spec_guided=True, spec_sampled=True)
    res = run(eng)
    assert res.token_ids == want.token_ids and res.done_reason == "stop"
    assert eng.stats["spec_steps"] > 0 and eng.stats["spec_steps"] + eng.stats["spec_accepted"] == len(want.token_ids) - 1
    # planted drafts: every one accepted, the DFA state handed over after them
    eng = make(guided=True, spec_tokens=K, spec_guided=True, spec_sampled=True)
    eng.runner.set_spec_forced(forced_table(want.token_ids, "right", eng.runner.V))
    assert run(eng).token_ids == want.token_ids
    n = len(want.token_ids) - 1
    assert counts(eng)[0] == -(-n // (K + 1)) and counts(eng)[2] == n - counts(eng)[0]
    # a constrained sampled request needs both flags
    for kw in (dict(spec_sampled=True), dict(spec_guided=True)):
        eng = make(guided=True, spec_tokens=K, **kw)
        assert run(eng).token_ids == want.token_ids and eng.stats["spec_steps"] == 0


def test_flag_plumbing(monkeypatch):
    assert Settings().spec_sampled is False
    monkeypatch.setenv("LSA_SPEC_SAMPLED", "1")
    assert Settings().spec_sampled is True
    monkeypatch.delenv("LSA_SPEC_SAMPLED")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-sampled"])).spec_sampled is True
    assert Settings.from_cli(ap.parse_args([])).spec_sampled is False
    assert make().runner.spec_sampled is False
    eng = make(spec_tokens=K, spec_sampled=True)
    assert eng.runner.spec_sampled is True
    with pytest.raises(AssertionError, match="spec_sampled"):
        make(spec_tokens=K).runner.decode_spec(1, sample=True)


# ------------------------------------------------------------------------------------------------ decided share
def recorded_draws(eng, n_tokens=95):
    """``record_spec_logits`` of the GPU file's engine case.  Returns the tokens and, per verify step, one (row, the
    twin's pick set of that row at the token's draw, committed token, the row's draft or None) per committed token."""
    ids = eng.encode(eng.render(PROMPT, SYSTEM, False))
    sp = SamplingParams(**GPU_CASE)
    toks, logits, steps = numerics.record_spec_logits(eng, ids, n_tokens, hidden=False, params=sp)
    logits = logits.cpu()
    seed = ref.pack_seed(SEED, 0)
    out = []
    for s in steps:
        if not s["spec"]:
            continue
        rows = []
        for i in range(s["committed"]):
            j = s["first"] + i
            want = ref.sample_pick_set(logits[0, j - 1], sp.temperature, sp.top_k, sp.top_p, ref.device_uniform(seed, j), M)
            rows.append((i, want, toks[j], s["draft"][i] if i < len(s["draft"]) else None))
        out.append(rows)
    return toks, out


def test_decided_share_of_the_gpu_engine_case():
    """The reference alone, over the CPU engine's verify rows of the GPU engine test's prompt and parameters (n-gram
    drafts, then planted all-right drafts so that rows 1 .. k are drawn from too): at most 5% of the draws may be left
    undecided by the margin (the rule of test_decided_share_of_gpu_families), so the GPU test, which allows 10%,
    cannot hide behind its slack."""
    want = gen(make(), seed=SEED, temperature=0.8, top_k=40, top_p=0.9)
    for planted in (False, True):
        eng = make(spec_tokens=K, spec_sampled=True)
        if planted:
            eng.runner.set_spec_forced(forced_table(want, "right", eng.runner.V))
        toks, steps = recorded_draws(eng)
        assert toks == want
        sets = [w for rows in steps for _, w, _, _ in rows]
        undecided = sum(len(w) > 1 for w in sets) / len(sets)
        print(f"GPU engine case on the CPU (planted={planted}): {len(sets)} draws in {len(steps)} verify steps, "
              f"undecided share {undecided:.4f}")
        assert len(sets) == 95 and undecided <= 0.05
        assert not planted or len(steps) == -(-95 // (K + 1))
