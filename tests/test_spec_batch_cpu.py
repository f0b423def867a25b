"""Speculative decoding for several concurrent greedy requests on the CPU (``spec_batch``): the host twins of the
S-row commit and the per-sequence planted drafts, and the engine's batched verify runs against each request decoded
alone without speculation -- the tokens must be identical, whatever is drafted, whoever else runs."""
import argparse

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

from test_spec_cpu import CONTEXTS, K, SYSTEM, draft_inputs, forced_table, planted_logits

I32 = dict(dtype=torch.int32)

# three different prompts.  The random-init tiny models answer each with spans that repeat (their own loops and the
# system prompt they all share), so the n-gram drafter has something to accept for every one of them: recorded over 40
# tokens, tiny-nsql accepts 2 / 2 / 5 drafts and tiny-llama3 28 each
PROMPTS = ["How many rows are there?", "List the names and ages of all people older than 30", "Select all records"]


# ------------------------------------------------------------------------------------------------ kernel twins
def commit_rows_state(S, max_new=16):
    return dict(out_tokens=torch.zeros(S, max_new, **I32), gen_len=torch.tensor([2, 5, 1, 3][:S], **I32),
                input_ids=torch.tensor([5, 6, 7, 8][:S], **I32), positions=torch.tensor([9, 40, 3, 77][:S], **I32),
                finished=torch.tensor([0, 1, 0, 0][:S], **I32), eos=torch.tensor([99], **I32),
                limit=torch.tensor([16, 16, 3, 16][:S], **I32), eos_on=torch.tensor([1, 1, 1, 0][:S], **I32))


# per row: (argmax of its T rows, its drafts): row 0 accepts two; row 1 is finished; row 2 accepts all but hits its
# length limit (3) after two tokens; row 3 has no draft at all (-1) and ignores the EOS it commits
COMMIT_ROWS = [([10, 11, 12, 13], [10, 11, 7]), ([20, 21, 22, 23], [20, 21, 22]), ([30, 31, 32, 33], [30, 31, 32]),
               ([99, 41, 42, 43], [-1, -1, -1])]


def run_commit_rows(S, device="cpu", V=128):
    """One S-row launch and S one-row launches on equal states: (state, stats) of both."""
    toks = [t for row in COMMIT_ROWS[:S] for t in row[0]]
    lg = planted_logits(toks, V).to(device)
    dr = torch.tensor([d for row in COMMIT_ROWS[:S] for d in row[1]], **I32).to(device)
    st = {k: v.to(device) for k, v in commit_rows_state(S).items()}
    stats = torch.zeros(S, 3, dtype=torch.int64, device=device)
    ops.spec_commit(lg, dr, stats, st["out_tokens"], st["gen_len"], st["input_ids"], st["positions"], st["finished"],
                    st["eos"], st["limit"], st["eos_on"])
    one = {k: v.to(device) for k, v in commit_rows_state(S).items()}
    one_stats = torch.zeros(S, 3, dtype=torch.int64, device=device)
    T = K + 1
    for s in range(S):
        row = lambda k: one[k][s:s + 1]  # noqa: E731
        ops.spec_commit(lg[s * T:(s + 1) * T].contiguous(), dr[s * K:(s + 1) * K].contiguous(), one_stats[s],
                        row("out_tokens"), row("gen_len"), row("input_ids"), row("positions"), row("finished"),
                        one["eos"], row("limit"), row("eos_on"))
    return ({k: v.cpu() for k, v in st.items()}, stats.cpu()), ({k: v.cpu() for k, v in one.items()}, one_stats.cpu())


def test_ref_spec_commit_rows_equal_one_row_calls():
    (st, stats), (one, one_stats) = run_commit_rows(3)
    for key in st:
        assert torch.equal(st[key], one[key]), key
    assert torch.equal(stats, one_stats)
    assert stats.tolist() == [[1, 3, 2], [0, 0, 0], [1, 3, 1]]  # the finished row counts nothing
    assert st["out_tokens"][0, 2:6].tolist() == [10, 11, 12, 0] and st["gen_len"].tolist() == [5, 5, 3]
    assert st["out_tokens"][1].abs().sum() == 0 and st["finished"].tolist() == [0, 1, 1]


def run_draft_rows(forced, device="cpu"):
    """Two rows with different contexts through one spec_draft call: (ids, pos, drafts)."""
    rows = [draft_inputs(CONTEXTS["constant"], 5, max_len=16, max_new=16),
            draft_inputs(CONTEXTS["tail_only"], 3, max_len=16, max_new=16)]
    ins = [torch.cat([r[i] for r in rows]).to(device) for i in range(6)]
    ids = torch.full((2 * (K + 1),), -7, **I32).to(device)
    pos = torch.full((2 * (K + 1),), -7, **I32).to(device)
    dr = torch.full((2 * K,), -7, **I32).to(device)
    ops.spec_draft(*ins, K, ids, pos, dr, forced=None if forced is None else forced.to(device))
    return ids.tolist(), pos.tolist(), dr.tolist()


def test_ref_spec_draft_per_sequence_forced():
    tables = torch.arange(2 * 10 * K, **I32).view(2, 10, K) + 100
    ids, pos, dr = run_draft_rows(tables)
    # row 0 has generated 7 tokens, row 1 4: each reads its own table at row min(gen_len, 9)
    assert dr == tables[0, 7].tolist() + tables[1, 4].tolist()
    assert ids == [4] + tables[0, 7].tolist() + [2] + tables[1, 4].tolist()
    assert pos == [11, 12, 13, 14, 6, 7, 8, 9]
    # one [nf, k] table serves every row, as before
    assert run_draft_rows(tables[0])[2] == tables[0, 7].tolist() + tables[0, 4].tolist()
    with pytest.raises(ValueError):
        run_draft_rows(tables[:1])  # fewer tables than rows


def test_ref_attn_verify_loops_over_sequences():
    """ref.attn_verify over [S, T, H, D] equals its one-sequence form per sequence; the S / row limits are refused."""
    g = torch.Generator().manual_seed(0)
    H, Hkv, D, T, S, MB = 4, 2, 128, 3, 2, 3
    kc = torch.randn(8, Hkv, 64, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(8, Hkv, 64, D, generator=g).to(torch.bfloat16)
    q = torch.randn(S, T, H, D, generator=g).to(torch.bfloat16)
    bt = torch.tensor([[1, 2, 3], [4, 5, 6]], **I32)
    pos0 = torch.tensor([5, 70], **I32)
    out = torch.zeros(S * T, H * D, dtype=torch.bfloat16)
    ops.attn_verify(q, kc, vc, bt, pos0, H, Hkv, D ** -0.5, out)
    for s in range(S):
        one = torch.zeros(T, H * D, dtype=torch.bfloat16)
        ops.attn_verify(q[s], kc, vc, bt[s], pos0[s:s + 1], H, Hkv, D ** -0.5, one)
        assert torch.equal(out[s * T:(s + 1) * T], one)
    with pytest.raises(ValueError):
        ops.attn_verify(torch.zeros(9, 2, H, D, dtype=torch.bfloat16), kc, vc, bt[:1].expand(9, MB).contiguous(),
                        torch.zeros(9, **I32), H, Hkv, 1.0, torch.zeros(18, H * D, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.attn_verify(torch.zeros(5, 8, H, D, dtype=torch.bfloat16), kc, vc, bt[:1].expand(5, MB).contiguous(),
                        torch.zeros(5, **I32), H, Hkv, 1.0, torch.zeros(40, H * D, dtype=torch.bfloat16))


# ------------------------------------------------------------------------------------------------ engine
def make(model="tiny-nsql", max_slots=4, max_model_len=512, **kw):
    return build_engine(model, device="cpu", max_slots=max_slots, max_model_len=max_model_len, seed=0, **kw)


def ids_of(eng, prompt):
    return eng.encode(eng.render(prompt, SYSTEM, False))


def run(eng, prompts, n=40, watch=None, **opts):
    """Send ``prompts`` (texts or token lists) at once, n tokens each (an int or one per request); step to the end.
    Returns (requests, batched): batched = the engine iterations in which the verify-step counters of two or more
    requests advanced, i.e. runs of verify steps over several sequences.  ``watch(eng, reqs)`` runs after each step."""
    ns = [n] * len(prompts) if isinstance(n, int) else list(n)
    reqs = [eng.add_request(ids_of(eng, p) if isinstance(p, str) else list(p),
                            SamplingParams(max_tokens=m, ignore_eos=True, **opts)) for p, m in zip(prompts, ns)]
    batched = 0
    while not all(q.done.is_set() for q in reqs):
        before = [q.spec_steps for q in reqs]
        eng.step()
        batched += sum(q.spec_steps > b for q, b in zip(reqs, before)) >= 2
        if watch is not None:
            watch(eng, reqs)
    return reqs, batched


_SOLO = {}


def solo(model, prompt, n, max_model_len=512):
    """The request's tokens generated alone by an engine without speculation (computed once per prompt)."""
    key = (model, prompt if isinstance(prompt, str) else tuple(prompt), max_model_len)
    if key not in _SOLO or len(_SOLO[key]) < n:
        eng = make(model, max_model_len=max_model_len)
        ids = ids_of(eng, prompt) if isinstance(prompt, str) else list(prompt)
        _SOLO[key] = eng.generate([ids], SamplingParams(max_tokens=n, ignore_eos=True))[0].token_ids
    return _SOLO[key][:n]


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_batch_tokens_equal_solo_plain(model):
    eng = make(model, spec_tokens=K, spec_batch=4)
    reqs, batched = run(eng, PROMPTS, 40)
    for q, p in zip(reqs, PROMPTS):
        assert q.output_ids == solo(model, p, 40)
        assert q.spec_steps > 0 and q.spec_accepted >= 1  # the drafter found something for every request
        assert q.spec_steps + q.spec_accepted <= 39   # (a request left alone in a slot other than 0 ends on plain steps)
    assert batched > 0
    st = eng.stats
    assert st["spec_steps"] == sum(q.spec_steps for q in reqs) and st["spec_accepted"] == sum(q.spec_accepted for q in reqs)
    rows = eng.runner.spec_row_counts()
    assert len(rows) == 4 and rows[3] == [0, 0, 0]  # the idle row of bucket 4 counts nothing
    assert eng.runner.spec_counts() == tuple(sum(c) for c in zip(*rows))
    assert [rows[q.slot][0] for q in reqs] == [q.spec_steps for q in reqs]


def forced_tables(tokens, kinds, V, S=4):
    """[S, nf, K]: table s plants drafts of ``kinds[s]`` for the request whose plain tokens are ``tokens[s]``."""
    tabs = [forced_table(t, kind, V) for t, kind in zip(tokens, kinds)]
    out = torch.zeros(S, tabs[0].shape[0], K, **I32)
    for s, t in enumerate(tabs):
        out[s] = t
    return out


# (the slower drafts sit in the lower slots: once the faster requests have finished, the rest keep speculating -- around
# the hole at S = 4, then alone in slot 0 -- so every count is exact; a request left alone in another slot ends plain)
@pytest.mark.parametrize("kinds", [("wrong", "right", "first"), ("wrong", "wrong", "wrong"), ("first", "right", "right")])
def test_engine_planted_drafts_per_sequence(kinds):
    n = 48
    want = [solo("tiny-nsql", p, n) for p in PROMPTS]
    eng = make(spec_tokens=K, spec_batch=4)
    eng.runner.set_spec_forced(forced_tables(want, kinds, eng.runner.V))
    reqs, batched = run(eng, PROMPTS, n)
    per = {"right": K, "wrong": 0, "first": 1}
    for q, w, kind in zip(reqs, want, kinds):
        assert q.output_ids == w
        steps = -(-(n - 1) // (per[kind] + 1))
        assert (q.spec_steps, q.spec_accepted) == (steps, n - 1 - steps), kind
    assert batched > 0
    total = sum(q.spec_steps for q in reqs)
    assert eng.stats["spec_steps"] == total and eng.stats["spec_drafted"] == K * total
    assert eng.stats["spec_accepted"] == 3 * (n - 1) - total


def test_gating_spec_batch_1_and_too_many_requests():
    eng = make(spec_tokens=K)  # spec_batch left at 1
    reqs, batched = run(eng, PROMPTS[:2], 16)
    assert batched == 0 and eng.stats["spec_steps"] == 0
    eng = make(spec_tokens=K, spec_batch=2)
    four = PROMPTS + [PROMPTS[0]]
    reqs, batched = run(eng, four, 16)
    assert batched == 0 and eng.stats["spec_steps"] == 0  # four equally long requests over spec_batch = 2
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 16) for p in four]
    reqs, batched = run(eng, PROMPTS[:2], 16)  # ... and two of them do speculate on the same engine
    assert batched > 0 and [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 16) for p in PROMPTS[:2]]


def test_gating_sampled_constrained_and_opted_out():
    eng = make(spec_tokens=K, spec_batch=4, spec_sampled=True, guided=True, spec_guided=True)
    sp = SamplingParams(max_tokens=16, ignore_eos=True)
    # a sampled request in the run (even with spec_sampled: sampled verification is one-sequence)
    a = eng.add_request(ids_of(eng, PROMPTS[0]), sp)
    b = eng.add_request(ids_of(eng, PROMPTS[1]), SamplingParams(max_tokens=16, ignore_eos=True, temperature=0.8, seed=1))
    eng.run_until_done([a, b])
    assert eng.stats["spec_steps"] == 0 and a.output_ids == solo("tiny-nsql", PROMPTS[0], 16)
    # a constrained request in the run (even with spec_guided)
    a = eng.add_request(ids_of(eng, PROMPTS[0]), sp)
    c = eng.add_request(ids_of(eng, PROMPTS[1]), SamplingParams(max_tokens=16, regex="[a-z ]{40,60}"))
    while not (a.done.is_set() and c.done.is_set()):
        both = not a.done.is_set() and not c.done.is_set()
        s0 = eng.stats["spec_steps"]
        eng.step()
        assert not both or eng.stats["spec_steps"] == s0
    assert a.output_ids == solo("tiny-nsql", PROMPTS[0], 16) and c.spec_steps == 0
    # "speculate": false on one request; the acceptance guard's verdict on one request
    s0 = eng.stats["spec_steps"]
    a = eng.add_request(ids_of(eng, PROMPTS[0]), sp)
    b = eng.add_request(ids_of(eng, PROMPTS[1]), SamplingParams(max_tokens=16, ignore_eos=True, speculate=False))
    eng.run_until_done([a, b])
    a = eng.add_request(ids_of(eng, PROMPTS[0]), sp)
    b = eng.add_request(ids_of(eng, PROMPTS[1]), sp)
    b.spec_off = True
    eng.run_until_done([a, b])
    assert eng.stats["spec_steps"] == s0
    assert (a.output_ids, b.output_ids) == (solo("tiny-nsql", PROMPTS[0], 16), solo("tiny-nsql", PROMPTS[1], 16))
    # the same engine speculates once both requests may
    reqs, batched = run(eng, PROMPTS[:2], 16)
    assert batched > 0


def test_gating_mid_chunked_prefill():
    """While a third request's prompt is being prefilled chunk by chunk, the two running requests take plain steps;
    once it runs, all three speculate together."""
    eng = make(spec_tokens=K, spec_batch=4, prefill_chunk=16)
    eng.run_ahead = 4
    sp = SamplingParams(max_tokens=64, ignore_eos=True)
    short = [[1] + list(range(3 + k, 40 + k)) for k in range(2)]  # 38 tokens: three chunks each
    long_ids = [1] + list(range(50, 149))                            # 100 tokens: seven chunks
    a, b = (eng.add_request(p, sp) for p in short)
    for _ in range(12):  # until both run and speculate together
        eng.step()
        if a.spec_steps and b.spec_steps:
            break
    assert a.spec_steps and b.spec_steps and not a.done.is_set()
    c = eng.add_request(long_ids, sp)
    held = 0
    for _ in range(200):
        if all(q.done.is_set() for q in (a, b, c)):
            break
        s0 = eng.stats["spec_steps"]
        eng.step()
        if eng._prefilling:  # still mid-prefill after the step: its decode run was plain
            held += 1
            assert eng.stats["spec_steps"] == s0
    assert all(q.done.is_set() for q in (a, b, c))
    assert held >= 2 and c.spec_steps > 0
    assert [q.output_ids for q in (a, b)] == [solo("tiny-nsql", p, 64) for p in short]
    assert c.output_ids == solo("tiny-nsql", long_ids, 64)


def test_gating_window_room():
    """One request whose window leaves fewer than steps * T + T positions makes the run plain."""
    eng = make(max_model_len=128, spec_tokens=K, spec_batch=2, max_slots=2)
    tight = [1] + list(range(3, 127))     # 125 tokens: 3 positions left
    short = [[1] + list(range(3 + k, 40 + k)) for k in range(2)]
    reqs, batched = run(eng, [tight, short[0]], [3, 3])
    assert batched == 0 and eng.stats["spec_steps"] == 0
    assert reqs[0].output_ids == solo("tiny-nsql", tight, 3, 128) and reqs[1].output_ids == solo("tiny-nsql", short[0], 3, 128)
    reqs, batched = run(eng, short, [8, 8])  # with room, the same engine speculates
    assert batched > 0 and [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 8, 128) for p in short]


def test_gating_kv_arena_too_small():
    """Three usable KV blocks, two requests of one block each that both need a second one for the verify run's
    lookahead: the run is plain (no run of verify steps serves both), the younger is preempted by the plain run's own
    growth, and each speculates only while it runs alone."""
    prompts = [[1] + list(range(3 + k, 52 + k)) for k in range(2)]  # 50 tokens
    eng = make(max_slots=2, num_kv_blocks=4, kv_reserve_tokens=0, spec_tokens=K, spec_batch=2)
    eng.run_ahead = 16
    reqs, batched = run(eng, prompts, 40)
    assert batched == 0
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, 40) for p in prompts]
    assert eng.stats["preempted"] >= 1 and eng.stats["spec_steps"] > 0
    assert eng.sched.free_blocks == 3 and eng.sched.num_running == 0


def test_hole_below_S_keeps_the_others_speculating():
    """The request in slot 1 finishes early: slots 0 and 2 keep speculating at S = 4 around the empty row."""
    eng = make(spec_tokens=K, spec_batch=4)
    eng.run_ahead = 4
    after = []

    def watch(eng, reqs):
        if reqs[1].done.is_set():
            after.append((reqs[0].spec_steps, reqs[2].spec_steps))

    reqs, batched = run(eng, PROMPTS, [48, 6, 48], watch=watch)
    assert [q.slot for q in reqs] == [0, 1, 2]
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, n) for p, n in zip(PROMPTS, (48, 6, 48))]
    # both survivors' counters advance together after the hole appears
    assert len(after) >= 3 and after[-1][0] > after[0][0] and after[-1][1] > after[0][1]
    assert eng.runner.spec_row_counts()[1][0] == reqs[1].spec_steps <= 5


def test_preempted_request_resumes_in_a_batch():
    """Three requests in an arena too small for all: the youngest is preempted by the plain run's growth, re-admitted
    next to a request that still runs, and speculates again there.  The requests that were never preempted decode their
    solo tokens, the victim does up to its preemption; after it the victim's context is re-prefilled, which is another
    computation than the decode steps that first produced it -- an engine without speculation leaves the solo tokens
    there as well in this scenario (token 122 of 150, at a near-tie), so nothing is asserted about them here."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    ns = [150, 100, 150]  # the middle request finishes while the oldest still runs: its blocks re-admit the victim
    eng = make(num_kv_blocks=8, spec_tokens=K, spec_batch=4)
    eng.run_ahead = 8
    seen = []

    def watch(eng, reqs):
        seen.append([(q.preemptions, q.spec_steps) for q in reqs])

    reqs, batched = run(eng, prompts, ns, watch=watch)
    assert eng.stats["preempted"] >= 1
    victim = next(i for i, q in enumerate(reqs) if q.preemptions)
    for i, (q, p, n) in enumerate(zip(reqs, prompts, ns)):
        m = len(q.resumed) if i == victim else n
        assert len(q.output_ids) == n and m > 0 and q.output_ids[:m] == solo("tiny-nsql", p, n)[:m], i
    # after its preemption the victim's counter advances in an iteration in which another request's advances too
    resumed = [j for j in range(1, len(seen)) if seen[j][victim][0] and seen[j][victim][1] > seen[j - 1][victim][1]
               and any(seen[j][o][1] > seen[j - 1][o][1] for o in range(3) if o != victim)]
    assert resumed, seen[-1]
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == 7


def test_acceptance_guard_drops_one_request_then_plain():
    n = 120
    want = [solo("tiny-nsql", p, n) for p in PROMPTS[:2]]
    eng = make(spec_tokens=K, spec_batch=2)
    eng.runner.set_spec_forced(forced_tables(want, ("wrong", "right"), eng.runner.V, S=2))
    eng.runner.spec_min_accept = 0.5
    eng.run_ahead = 8
    reqs, batched = run(eng, PROMPTS[:2], n)
    a, b = reqs
    assert [q.output_ids for q in reqs] == want
    # request a: 16 verify steps at zero acceptance (checked every 8 steps), then dropped on its own counters; request
    # b accepted everything, is not dropped, and takes plain steps from then on all the same (all or nothing)
    assert a.spec_off and 16 <= a.spec_steps < 24 and a.spec_accepted == 0
    assert not b.spec_off and b.spec_steps == a.spec_steps and b.spec_accepted == K * b.spec_steps
    assert eng.stats["spec_steps"] == a.spec_steps + b.spec_steps


def test_spec_batch_clamp_settings_and_health(monkeypatch, caplog):
    assert Settings().spec_batch == 1
    monkeypatch.setenv("LSA_SPEC_BATCH", "4")
    assert Settings().spec_batch == 4
    monkeypatch.delenv("LSA_SPEC_BATCH")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-batch", "2"])).spec_batch == 2
    assert Settings.from_cli(ap.parse_args([])).spec_batch == 1
    assert make().runner.spec_batch == 1 and make().spec_batch == 1
    assert make(spec_tokens=K).runner.spec_s() == 1
    with caplog.at_level("WARNING"):
        eng = make(spec_tokens=K, spec_batch=3)  # a power of two
        assert eng.runner.spec_s() == 2 and eng.spec_batch == 2
    assert any("spec_batch=3 clamped to 2" in r.getMessage() for r in caplog.records)
    assert make(spec_tokens=7, spec_batch=8, max_slots=8).runner.spec_s() == 4    # T = 8: 4 * 8 = 32 rows
    assert make(spec_tokens=1, spec_batch=16, max_slots=16).runner.spec_s() == 8  # at most 8 sequences
    assert make(spec_tokens=K, spec_batch=8, max_slots=2).runner.spec_s() == 2    # <= max_slots
    assert make("tiny-llama3", spec_tokens=9, spec_batch=8, max_slots=8).runner.spec_s() == 4  # T clamped to 5: 4 * 5
    # the plan and the workspace of S sequences
    assert ops.verify_split_plan(8, 2048, 4) == ops.decode_split_plan(4, 8, 2048)
    ws = ops.verify_workspace(4, 24, 8, 5, "cpu", S=3)
    assert ws[0].numel() == 3 * 4 * 24 * 5 * 128 and ws[2].numel() >= 3 * 8
    # health() of the serving backend carries the clamped spec_batch beside the engine's counters
    from llm_based_apache_spark_optimization_amd.client import EngineService
    svc = EngineService(lambda m: eng)
    try:
        svc.generate("tiny-nsql", "hi", options={"num_predict": 2})
        h = svc.health()["engines"]["tiny-nsql"]
        assert h["spec_batch"] == 2 and {"spec_steps", "spec_drafted", "spec_accepted"} <= set(h)
    finally:
        for lp in svc._loops.values():
            lp.close()
