"""Speculative decoding for several concurrent requests of which some need the sampler, on the CPU
(``spec_batch_sampled``): the S-sequence form of the sampled verify commit's host twin against S one-sequence calls, and
the engine's mixed runs -- sampled and greedy requests in one verify step -- against each request generated alone
without speculation: the same tokens, whatever is drafted, whoever else runs.  The GPU file shares the engine case."""
import argparse

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams
from llm_based_apache_spark_optimization_amd.eval import numerics
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_batch_cpu import PROMPTS, forced_tables, ids_of, make
from test_spec_cpu import K
from test_spec_sampled_cpu import M, NAMES, T, drafts_accepting, make_case, plain_tokens

I32 = dict(dtype=torch.int32)
PAR_SEQ = ("penalty", "temperature", "top_k", "top_p", "seeds", "last_n", "limit", "eos_on")  # one entry per sequence


# ------------------------------------------------------------------------------------------------ twin
def stack_cases(cases):
    """S one-sequence cases of ``make_case`` as the operands of one S-sequence call: (logits [S * T, V], state, par)."""
    logits = torch.cat([c[0] for c in cases])
    st = {k: torch.cat([c[1][k] for c in cases]) for k in NAMES}
    par = {k: torch.cat([c[2][k] for c in cases]) for k in PAR_SEQ}
    par["eos"] = cases[0][2]["eos"]
    return logits, st, par


def commit_call(logits, draft, stats, st, par):
    ops.spec_sample_commit(logits, draft, stats, st["hist"], par["penalty"], par["temperature"], par["top_k"],
                           par["top_p"], par["seeds"], st["out_tokens"], st["gen_len"], st["input_ids"],
                           st["positions"], st["finished"], par["eos"], par["limit"], par["eos_on"],
                           last_n=par["last_n"])


def test_ref_rows_equal_one_sequence_calls():
    """stats [S, 3] == S one-sequence calls: a sampled sequence with penalty 1.3 at position 62 that accepts every
    draft (its ring wraps inside the rows), a greedy one with penalty 1 that accepts one, and a finished one."""
    cases = [make_case(62, 1.3, 64), make_case(5, 1.0, 64, temp=0.0), make_case(63, 1.3, 64, finished=1)]
    toks = [plain_tokens(*c) for c in cases[:2]]
    drafts = [drafts_accepting(toks[0], K), drafts_accepting(toks[1], 1), [1, 2, 3]]
    logits, st, par = stack_cases(cases)
    stats = torch.zeros(3, 3, dtype=torch.int64)
    commit_call(logits, torch.tensor(drafts, **I32), stats, st, par)
    for s, (lg, st1, par1) in enumerate(cases):
        lg, st1, stats1 = lg.clone(), {k: v.clone() for k, v in st1.items()}, torch.zeros(3, dtype=torch.int64)
        commit_call(lg, torch.tensor(drafts[s], **I32), stats1, st1, par1)
        for name in NAMES:
            assert torch.equal(st[name][s:s + 1], st1[name]), (s, name)
        assert torch.equal(stats[s], stats1), s
        assert torch.equal(logits[s * T:(s + 1) * T], lg), s  # the penalised rows, written back
    assert stats.tolist() == [[1, K, K], [1, K, 1], [0, 0, 0]]
    assert [int(st["hist"][0, (63 + i) % 64]) for i in range(T)] == toks[0]  # slots 63, 0, 1, 2 of ring 0
    assert not torch.equal(logits[:T], cases[0][0]) and torch.equal(logits[T:2 * T], cases[1][0])
    assert st["gen_len"].tolist() == [2 + T, 2 + 2, 2] and st["positions"].tolist() == [62 + T, 5 + 2, 63]
    assert torch.equal(st["hist"][2:], cases[2][1]["hist"]) and int(st["out_tokens"][2].max()) == -1
    # the pick sets of the exact device twin take the same form: sequence s at s T ..
    l0, s0, p0 = stack_cases(cases)
    sets = ref.spec_sample_pick_sets(l0, torch.tensor(drafts, **I32), s0["hist"], p0["penalty"], p0["temperature"],
                                     p0["top_k"], p0["top_p"], p0["seeds"], s0["gen_len"], s0["positions"],
                                     last_n=p0["last_n"], S=3)
    assert len(sets) == 3 * T
    for s, (lg, st1, par1) in enumerate(cases):
        assert sets[s * T:(s + 1) * T] == ref.spec_sample_pick_sets(
            lg, torch.tensor(drafts[s], **I32), st1["hist"], par1["penalty"], par1["temperature"], par1["top_k"],
            par1["top_p"], par1["seeds"], st1["gen_len"], st1["positions"], last_n=par1["last_n"])
    assert sets[T:2 * T] == [{int(r.argmax())} for r in cases[1][0]]


def test_ref_sizes_refused():
    cases = [make_case(5, 1.0, 64), make_case(6, 1.0, 64)]
    logits, st, par = stack_cases(cases)
    two = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError):  # rows not divisible by S
        commit_call(logits[:7].clone(), torch.zeros(6, **I32), two, st, par)
    with pytest.raises(RuntimeError):  # T = 1 per sequence
        commit_call(logits[:2].clone(), torch.zeros(6, **I32), two, st, par)
    with pytest.raises(RuntimeError):  # a parameter tensor of one entry for two sequences
        commit_call(logits.clone(), torch.zeros(6, **I32), two, st, dict(par, temperature=par["temperature"][:1]))
    big = torch.zeros(40, logits.shape[1])
    with pytest.raises(RuntimeError):  # 40 rows (S = 5, T = 8)
        commit_call(big, torch.zeros(35, **I32), torch.zeros(5, 3, dtype=torch.int64), st, par)
    assert int(two.abs().sum()) == 0 and st["gen_len"].tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------ engine
SEED = 11
OLLAMA = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1, seed=SEED)  # Ollama's default option set
OTHER = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.0, seed=5)
# the engine case, shared with the GPU file: request s of PROMPTS runs with MIXED[s] -- sampled with Ollama's defaults,
# greedy, sampled with another seed and no penalty
MIXED = [OLLAMA, {}, OTHER]
ON = dict(spec_tokens=K, spec_batch=4, spec_sampled=True, spec_batch_sampled=True)


def params(opts, n):
    return SamplingParams(**{"max_tokens": n, "ignore_eos": True, **opts})


_SOLO = {}


def solo(model, prompt, n, opts, **kw):
    """The request's tokens generated alone by an engine without speculation (computed once per request)."""
    key = (model, prompt if isinstance(prompt, str) else tuple(prompt), tuple(sorted(opts.items())), tuple(sorted(kw.items())))
    if key not in _SOLO or len(_SOLO[key]) < n:
        eng = make(model, **kw)
        ids = ids_of(eng, prompt) if isinstance(prompt, str) else list(prompt)
        _SOLO[key] = eng.generate([ids], params(opts, n))[0].token_ids
    return _SOLO[key][:n]


def spy(eng):
    """Record (sample, S) of every ``decode_spec`` call of the engine's runner."""
    calls, inner = [], eng.runner.decode_spec

    def decode_spec(steps, max_ctx=None, guided=False, sample=False, S=1):
        calls.append((bool(sample), S))
        return inner(steps, max_ctx=max_ctx, guided=guided, sample=sample, S=S)

    eng.runner.decode_spec = decode_spec
    return calls


def run(eng, prompts, n, opts, watch=None, tweak=None):
    """Send the requests at once, request i with ``opts[i]`` and n (an int or one per request) tokens; step to the end.
    Returns (requests, batched): batched = the engine iterations in which the verify-step counters of two or more
    requests advanced.  ``tweak(reqs)`` runs before the first step, ``watch(eng, reqs)`` after each."""
    ns = [n] * len(prompts) if isinstance(n, int) else list(n)
    reqs = [eng.add_request(ids_of(eng, p) if isinstance(p, str) else list(p), params(o, m))
            for p, o, m in zip(prompts, opts, ns)]
    if tweak is not None:
        tweak(reqs)
    batched = 0
    while not all(q.done.is_set() for q in reqs):
        before = [q.spec_steps for q in reqs]
        eng.step()
        batched += sum(q.spec_steps > b for q, b in zip(reqs, before)) >= 2
        if watch is not None:
            watch(eng, reqs)
    return reqs, batched


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_mixed_run_equals_solo_plain(model):
    n = 40
    eng = make(model, **ON)
    calls = spy(eng)
    reqs, batched = run(eng, PROMPTS, n, MIXED)
    for q, p, o in zip(reqs, PROMPTS, MIXED):
        assert q.output_ids == solo(model, p, n, o), o
        assert q.spec_steps > 0 and q.spec_steps + q.spec_accepted <= n - 1
    assert batched > 0
    assert (True, 4) in calls and (False, 4) not in calls  # the runs over several sequences took the sampled step
    assert eng.stats["spec_steps"] == sum(q.spec_steps for q in reqs)
    rows = eng.runner.spec_row_counts()
    assert rows[3] == [0, 0, 0] and [rows[q.slot][0] for q in reqs] == [q.spec_steps for q in reqs]


# (the slower drafts sit in the lower slots, as in test_engine_planted_drafts_per_sequence, so every count is exact)
@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
@pytest.mark.parametrize("kinds", [("wrong", "right", "first"), ("wrong", "wrong", "wrong"), ("first", "right", "right")])
def test_engine_planted_drafts_per_sequence(model, kinds):
    n = 48
    want = [solo(model, p, n, o) for p, o in zip(PROMPTS, MIXED)]
    eng = make(model, **ON)
    calls = spy(eng)
    eng.runner.set_spec_forced(forced_tables(want, kinds, eng.runner.V))
    reqs, batched = run(eng, PROMPTS, n, MIXED)
    per = {"right": K, "wrong": 0, "first": 1}
    for q, w, kind in zip(reqs, want, kinds):
        assert q.output_ids == w, kind
        steps = -(-(n - 1) // (per[kind] + 1))
        assert (q.spec_steps, q.spec_accepted) == (steps, n - 1 - steps), kind
    assert batched > 0 and (True, 4) in calls and (False, 4) not in calls
    total = sum(q.spec_steps for q in reqs)
    assert eng.stats["spec_steps"] == total and eng.stats["spec_drafted"] == K * total
    assert eng.stats["spec_accepted"] == 3 * (n - 1) - total


def test_all_greedy_run_takes_the_greedy_batched_step():
    eng = make(**ON)
    calls = spy(eng)
    reqs, batched = run(eng, PROMPTS, 24, [{}, {}, {}])
    assert batched > 0 and (False, 4) in calls and not any(sample and S > 1 for sample, S in calls)
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 24, {}) for p in PROMPTS]
    # ... and the same engine takes the sampled step for the next, mixed run
    reqs, _ = run(eng, PROMPTS, 24, MIXED)
    assert (True, 4) in calls
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 24, o) for p, o in zip(PROMPTS, MIXED)]


def assert_plain(eng, prompts, opts, n=16, tweak=None, **solo_kw):
    """While two or more of the requests run, no verify step is taken; every request's tokens are its solo tokens."""
    def watch(eng, reqs):
        seen.append((sum(not q.done.is_set() for q in reqs), eng.stats["spec_steps"]))

    seen = [(len(prompts), eng.stats["spec_steps"])]
    reqs, batched = run(eng, prompts, n, opts, watch=watch, tweak=tweak)
    assert batched == 0
    assert all(b[1] == a[1] for a, b in zip(seen, seen[1:]) if a[0] >= 2), seen
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, n, o, **solo_kw) for p, o in zip(prompts, opts)]
    return reqs


def test_gating():
    """(The sampled request runs on PROMPTS[0]: the CPU's plain two-row step is not bit-equal to the one-row step for
    every sampled request -- see test_preempted_request_resumes_its_stream -- and for this one it is.)"""
    two, opts = PROMPTS[:2], [OLLAMA, {}]
    # the flag off: the situation of test_gating_sampled_constrained_and_opted_out
    eng = make(spec_tokens=K, spec_batch=4, spec_sampled=True)
    assert eng.runner.spec_batch_sampled is False
    assert_plain(eng, two, opts)
    with pytest.raises(AssertionError, match="spec_batch_sampled"):
        eng.runner.decode_spec(1, sample=True, S=2)
    # the flag on without spec_sampled
    assert_plain(make(spec_tokens=K, spec_batch=4, spec_batch_sampled=True), two, opts)
    # inert without spec_tokens, and without spec_batch > 1
    assert_plain(make(spec_sampled=True, spec_batch=4, spec_batch_sampled=True), two, opts)
    assert_plain(make(spec_tokens=K, spec_sampled=True, spec_batch_sampled=True), two, opts)
    # a constrained request in the run (even with spec_guided)
    eng = make(guided=True, spec_guided=True, **ON)
    assert_plain(eng, two, [OLLAMA, dict(regex="[a-z ]{40,60}", ignore_eos=False)], guided=True)
    # "speculate": false on one request; the acceptance guard's verdict on one request
    assert_plain(eng, two, [OLLAMA, dict(speculate=False)])

    def drop(reqs):
        reqs[1].spec_off = True

    assert_plain(eng, two, opts, tweak=drop)
    # a guided verify step over several sequences stays refused
    with pytest.raises(AssertionError):
        eng.runner.decode_spec(1, guided=True, sample=True, S=2)
    # the same engine speculates once both requests may
    reqs, batched = run(eng, two, 16, opts)
    assert batched > 0 and [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 16, o) for p, o in zip(two, opts)]


def test_acceptance_guard_drops_one_sampled_request_then_plain():
    n, opts = 120, [OLLAMA, {}]
    want = [solo("tiny-nsql", p, n, o) for p, o in zip(PROMPTS[:2], opts)]
    eng = make(**dict(ON, spec_batch=2))
    eng.runner.set_spec_forced(forced_tables(want, ("wrong", "right"), eng.runner.V, S=2))
    eng.runner.spec_min_accept = 0.5
    eng.run_ahead = 8
    (a, b), batched = run(eng, PROMPTS[:2], n, opts)
    assert [a.output_ids, b.output_ids] == want
    # the sampled request: 16 verify steps at zero acceptance (checked every 8 steps), then dropped on its own counts;
    # the greedy one accepted everything, is not dropped, and takes plain steps from then on all the same
    assert a.spec_off and 16 <= a.spec_steps < 24 and a.spec_accepted == 0
    assert not b.spec_off and b.spec_steps == a.spec_steps and b.spec_accepted == K * b.spec_steps
    assert eng.stats["spec_steps"] == a.spec_steps + b.spec_steps


def test_preempted_sampled_request_resumes_in_a_batch():
    """The scenario of test_preempted_request_resumes_in_a_batch with a sampled youngest request: it is preempted by the
    plain run's growth, re-admitted next to a request that still runs and speculates again there, its draws continuing
    at the counter offset of the seed word.  Up to its preemption the victim's tokens are its solo tokens; after it the
    context is re-prefilled, another computation than the decode steps that first produced it, so the reference for
    the rest is the stream itself: solo generation from the re-prefilled context, continued at the same draw -- as far
    as the victim's verify steps go (left alone in slot 2 it ends on plain steps of bucket 4, which on the CPU are not
    bit-equal to the one-row steps of the solo run)."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    ns, opts = [200, 120, 200], [{}, {}, OLLAMA]
    eng = make(num_kv_blocks=8, **ON)
    eng.run_ahead = 8
    seen = []

    def watch(eng, reqs):
        v = reqs[2]
        seen.append([(q.preemptions, q.spec_steps) for q in reqs])
        have.append(len(v.output_ids) if v.done.is_set() else len(v.resumed) + v.gen_host)

    have = [0]
    calls = spy(eng)
    reqs, batched = run(eng, prompts, ns, opts, watch=watch)
    assert eng.stats["preempted"] >= 1 and reqs[2].preemptions and not reqs[0].preemptions
    assert (True, 4) in calls
    for i, (q, p, n, o) in enumerate(zip(reqs, prompts, ns, opts)):
        m = len(q.resumed) if q.preemptions else n
        assert len(q.output_ids) == n and m > 0 and q.output_ids[:m] == solo("tiny-nsql", p, n, o)[:m], i
    resumed = [j for j in range(1, len(seen)) if seen[j][2][0] and seen[j][2][1] > seen[j - 1][2][1]
               and any(seen[j][o][1] > seen[j - 1][o][1] for o in (0, 1))]
    assert resumed, seen[-1]
    # the stream after the re-admission: a plain engine that is given the victim's context as its prompt and the
    # draws' offset in its seed word makes the same draws
    v = reqs[2]
    m = len(v.resumed)
    plain = make()
    q = plain.add_request(prompts[2], params(OLLAMA, ns[2]))
    q.resumed, q.params = list(v.output_ids[:m]), params(OLLAMA, ns[2] - m)
    plain.run_until_done([q])
    # (iteration j produced tokens have[j] .. have[j + 1] - 1 of the victim; `upto`: the end of its run of iterations
    # after the re-admission that were verify steps)
    it = [(have[j + 1], seen[j][2][1] > (seen[j - 1][2][1] if j else 0)) for j in range(len(seen)) if have[j + 1] > m + 1]
    upto = next((it[j - 1][0] for j in range(1, len(it)) if not it[j][1]), it[-1][0])
    assert it[0][1] and upto >= m + 32, (m, it)
    assert q.output_ids[:upto] == v.output_ids[:upto]
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == 7


def test_flag_plumbing(monkeypatch):
    assert Settings().spec_batch_sampled is False
    monkeypatch.setenv("LSA_SPEC_BATCH_SAMPLED", "1")
    assert Settings().spec_batch_sampled is True
    monkeypatch.delenv("LSA_SPEC_BATCH_SAMPLED")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-batch-sampled"])).spec_batch_sampled is True
    assert Settings.from_cli(ap.parse_args([])).spec_batch_sampled is False
    assert make().runner.spec_batch_sampled is False
    eng = make(**ON)
    assert eng.runner.spec_batch_sampled is True and eng.runner.spec_sampled is True and eng.spec_batch == 4
    from llm_based_apache_spark_optimization_amd.client import EngineService
    from llm_based_apache_spark_optimization_amd.serving.service import engine_factory
    svc = EngineService(lambda m: eng)
    try:
        svc.generate("tiny-nsql", "hi", options={"num_predict": 2})
        assert svc.health()["engines"]["tiny-nsql"]["spec_batch_sampled"] is True
    finally:
        for lp in svc._loops.values():
            lp.close()
    assert callable(engine_factory)


# ------------------------------------------------------------------------------------------------ decided share
UNUSABLE = torch.full((4, 1, K), -1, **I32)  # planted drafts no row can accept (-1: out of range, embedded as id 0)
GPU_TOKENS = 47  # tokens after the prefill's, the same budget for every request (so S never changes during a run)


def recorded_draws_batch(eng, n_tokens=GPU_TOKENS, prompts=PROMPTS, opts=MIXED):
    """``record_spec_logits_batch`` of the engine case.  Returns (tokens per request, rows per request): per token a
    verify step committed, (the twin's pick set of its recorded row at the token's draw, the committed token).  The
    recorded rows carry the request's penalty, so the set of a sampled request is ``sample_pick_set`` of the row at
    ``device_uniform(seed, j)``, and that of a greedy request the row's argmax."""
    ids = [ids_of(eng, p) for p in prompts]
    sps = [SamplingParams(**o) for o in opts]
    toks, logits, steps = numerics.record_spec_logits_batch(eng, ids, n_tokens, hidden=False, params=sps)
    logits = logits.cpu()
    out = []
    for i, sp in enumerate(sps):
        rows = []
        for s in steps[i]:
            if not s["spec"]:
                continue
            for t in range(s["committed"]):
                j = s["first"] + t
                row = logits[i, j - 1]
                if sp.temperature > 0:
                    u = ref.device_uniform(ref.pack_seed(sp.seed, 0), j)
                    rows.append((ref.sample_pick_set(row, sp.temperature, sp.top_k, sp.top_p, u, M), toks[i][j]))
                else:
                    rows.append(({int(row.argmax())}, toks[i][j]))
        out.append(rows)
    return toks, out


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_decided_share_of_the_gpu_engine_case(model):
    """The reference alone, over the CPU engine's verify rows of the GPU engine test's prompts, seeds and planted
    drafts (none usable, then all right so that rows 1 .. k are drawn from too): at most 5% of the sampled requests'
    draws may be left undecided by the margin, so the GPU test, which allows 10%, cannot hide behind its slack."""
    want = [solo(model, p, GPU_TOKENS + 1, o) for p, o in zip(PROMPTS, MIXED)]
    for kind in ("unusable", "right"):
        eng = make(model, **ON)
        eng.runner.set_spec_forced(UNUSABLE if kind == "unusable" else forced_tables(want, ("right",) * 3, eng.runner.V))
        toks, rows = recorded_draws_batch(eng)
        assert toks == want
        sets = [w for i, o in enumerate(MIXED) if o for w, _ in rows[i]]
        undecided = sum(len(w) > 1 for w in sets) / len(sets)
        print(f"{model}, GPU engine case on the CPU ({kind} drafts): {len(sets)} sampled draws, "
              f"undecided share {undecided:.4f}")
        assert len(sets) == 2 * GPU_TOKENS and undecided <= 0.05
