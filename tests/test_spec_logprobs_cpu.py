"""Per-token logprobs for speculating requests on the CPU (``spec_logprobs``): the host twins of the verify-step pair
(ops/reference.py spec_logprob_scan / spec_logprob_commit) against ``logprob_rows`` over a list of sequence kinds and
against successive plain logprob steps fed the same rows, and the engine on the tiny model: a request that asked
speculates, and its tokens and its whole logprobs list are those of the engine without speculation, bit for bit.  The
sequence kinds and the step helper are shared with the GPU file."""
import argparse
import dataclasses

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.client import EngineService
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_batch_cpu import PROMPTS, ids_of
from test_spec_cpu import K, forced_table

I32 = dict(dtype=torch.int32)
POISON = -777.25
EOS = 7
SHAPES = [(1, 2), (1, 4), (2, 4), (4, 8)]


# ------------------------------------------------------------------------------------------------ sequence kinds
def kinds(T, max_new):
    """The sequences a launch is made of.  Per kind: lp_k, the state before the step (n0 = gen_len, finished, a stale
    lp_n0), how the verify commit goes (a = accepted drafts, eos_row = the verify row whose argmax is EOS, limit) and
    ``gen_after``: a gen_len planted after the real commit where no commit can produce the state (nothing committed by a
    live row; more tokens than the record has room for).  ``c`` is the number of tokens the commit rule sees."""
    full = T - 1
    return {
        "one_token": dict(k=1, n0=1, a=0, limit=max_new, c=1),
        "all_rows": dict(k=20, n0=0, a=full, limit=max_new, c=min(T, max_new)),           # c = T (T = 8: cut by limit)
        "finished_before": dict(k=5, n0=2, a=full, limit=max_new, fin=1, stale=2, c=None),  # lp_n0 = -1, no record
        "limit_in_step": dict(k=0, n0=3, a=full, limit=5, c=2),
        "eos_in_step": dict(k=3, n0=2, a=full, eos_row=1, limit=max_new, c=2),             # the EOS token is recorded
        "did_not_ask": dict(k=-1, n0=1, a=min(1, full), limit=max_new, stale=3, c=None),
        "nothing_committed": dict(k=2, n0=2, a=0, limit=max_new, gen_after=2, c=0),
        "past_max_new": dict(k=4, n0=max_new - 1, a=full, limit=max_new, gen_after=max_new - 1 + T, c=T),
        "idle_slot": dict(k=-1, n0=0, a=0, limit=max_new, fin=1, c=None),                  # what release_slot leaves
        "all_rows_k0": dict(k=0, n0=1, a=full, limit=max_new, c=min(T, max_new - 1)),
    }


def groups(S, T, max_new):
    """The kinds in launches of S sequences (the list repeats cyclically to fill the last launch)."""
    names = sorted(kinds(T, max_new))
    n = -(-len(names) // S) * S
    names = [names[i % len(names)] for i in range(n)]
    return [names[i:i + S] for i in range(0, n, S)]


def planted(S, T, V, seqs, gen):
    """logits [S * T, V] whose row argmax is a token of our choosing, and drafts of which sequence s accepts a."""
    lg = torch.randn(S * T, V, generator=gen)
    toks = torch.randint(8, V, (S, T), generator=gen)  # (never EOS = 7 unless planted)
    draft = torch.zeros(S, T - 1, **I32)
    for s, q in enumerate(seqs):
        if q.get("eos_row") is not None:
            toks[s, q["eos_row"]] = EOS
        for t in range(T):
            lg[s * T + t, toks[s, t]] = 8.0 + 0.25 * t
        for i in range(T - 1):
            draft[s, i] = toks[s, i] if i < q["a"] else (int(toks[s, i]) + 1) % V
    return lg, draft.reshape(-1)


def state(S, max_new, seqs, dev="cpu", kcap=20):
    st = dict(out_tokens=torch.full((S, max_new), -3, **I32), gen_len=torch.tensor([q["n0"] for q in seqs], **I32),
              input_ids=torch.zeros(S, **I32), positions=torch.tensor([5 + q["n0"] for q in seqs], **I32),
              finished=torch.tensor([q.get("fin", 0) for q in seqs], **I32),
              lp_k=torch.tensor([q["k"] for q in seqs], **I32),
              lp_n0=torch.tensor([q.get("stale", -1) for q in seqs], **I32),
              lp_tok=torch.full((S, max_new), POISON), lp_ids=torch.full((S, max_new, kcap), -9, **I32),
              lp_top=torch.full((S, max_new, kcap), POISON),
              limit=torch.tensor([q["limit"] for q in seqs], **I32), eos_on=torch.ones(S, **I32),
              eos=torch.tensor([EOS], **I32))
    return {k: v.to(dev) for k, v in st.items()}


def verify_step(st, logits, draft, T, ws, seqs=None, between=None):
    """scan -> (``between``: the mask / penalty stand-in) -> the real greedy verify commit -> planted gen_len -> commit,
    through the public ops."""
    S = st["lp_k"].shape[0]
    ops.spec_logprob_scan(logits, T, st["lp_k"], st["finished"], st["gen_len"], st["lp_n0"], ws)
    if between is not None:
        between(logits)
    stats = torch.zeros(S, 3, dtype=torch.int64, device=logits.device)
    ops.spec_commit(logits, draft, stats if S > 1 else stats[0], st["out_tokens"], st["gen_len"], st["input_ids"],
                    st["positions"], st["finished"], st["eos"], st["limit"], st["eos_on"])
    for s, q in enumerate(seqs or []):
        if q.get("gen_after") is not None:
            st["gen_len"][s] = q["gen_after"]
    ops.spec_logprob_commit(T, st["lp_k"], st["lp_n0"], st["gen_len"], st["out_tokens"], st["lp_tok"], st["lp_ids"],
                            st["lp_top"], ws)


def expected_records(st0, st, raw, T, seqs, rows=ref.logprob_rows):
    """The record tensors the rule asks for: poison everywhere but the records of ``logprob_rows``."""
    want = {k: st0[k].clone().cpu() for k in ("lp_tok", "lp_ids", "lp_top")}
    max_new = st0["out_tokens"].shape[1]
    n0s = []
    for s, q in enumerate(seqs):
        if q["k"] < 0:
            n0s.append(q.get("stale", -1))
            continue
        if q.get("fin", 0):
            n0s.append(-1)
            continue
        n0 = q["n0"]
        n0s.append(n0)
        c = int(st["gen_len"][s]) - n0
        assert c == q["c"], (q, c)
        for t in range(min(c, T)):
            n = n0 + t
            if n >= max_new:
                break
            Kq = q["k"]
            chosen, ids, top = rows(raw[s * T + t:s * T + t + 1].cpu(), st["out_tokens"][s:s + 1, n].cpu(), Kq)
            want["lp_tok"][s, n] = chosen[0]
            want["lp_ids"][s, n, :Kq] = ids[0]
            want["lp_top"][s, n, :Kq] = top[0]
    return want, n0s


@pytest.mark.parametrize("S,T", SHAPES)
def test_twin_rule_over_the_kinds(S, T):
    V, max_new = 50, 6
    gen = torch.Generator().manual_seed(10 * S + T)
    seen = set()
    for names in groups(S, T, max_new):
        seqs = [kinds(T, max_new)[n] for n in names]
        seen |= set(names)
        lg, draft = planted(S, T, V, seqs, gen)
        raw = lg.clone()
        st = state(S, max_new, seqs)
        st0 = {k: v.clone() for k, v in st.items()}
        ws = ops.spec_logprob_workspace(V, "cpu")
        verify_step(st, lg, draft, T, ws, seqs)
        assert torch.equal(lg, raw)  # the scan only reads
        want, n0s = expected_records(st0, st, raw, T, seqs)
        for k in want:
            assert torch.equal(st[k], want[k]), (names, k)
        assert st["lp_n0"].tolist() == n0s, names  # announced, never consumed; -1 for a finished row that asked
        # the commit itself writes nothing but the records: the state is what the verify commit (and the planted
        # gen_len) left
        st2 = state(S, max_new, seqs)
        stats = torch.zeros(S, 3, dtype=torch.int64)
        ops.spec_commit(raw.clone(), draft, stats if S > 1 else stats[0], st2["out_tokens"], st2["gen_len"],
                        st2["input_ids"], st2["positions"], st2["finished"], st2["eos"], st2["limit"], st2["eos_on"])
        for s, q in enumerate(seqs):
            if q.get("gen_after") is not None:
                st2["gen_len"][s] = q["gen_after"]
        for k in ("out_tokens", "gen_len", "input_ids", "positions", "finished"):
            assert torch.equal(st[k], st2[k]), (names, k)
        fin = {n: int(st["finished"][s]) for s, n in enumerate(names)}
        for n in ("limit_in_step", "eos_in_step"):
            assert fin.get(n, 1) == 1
    assert seen == set(kinds(T, max_new))


def test_case_list_is_what_it_says():
    for S, T in SHAPES:
        ks = kinds(T, 6)
        assert {q["k"] for q in ks.values()} >= {-1, 0, 1, 20}
        assert {q["c"] for q in ks.values()} >= {None, 0, 1, min(T, 6)}
        assert ks["past_max_new"]["n0"] + ks["past_max_new"]["c"] > 6
        assert S * T <= 32 and all(len(g) == S for g in groups(S, T, 6))


@pytest.mark.parametrize("S,T", SHAPES)
def test_equal_to_successive_plain_steps(S, T):
    """The verify twins record bit for bit what c successive plain scan / commit steps record when they are fed the
    same rows: plain step t of sequence s gets verify row s T + t, whose argmax the greedy commit appends."""
    V, max_new = 50, 16
    gen = torch.Generator().manual_seed(7 * S + T)
    accepts = [T - 1, 0, min(1, T - 1), T - 2]
    seqs = [dict(k=(20, 0, 3, 1)[s % 4], n0=1 + s, a=accepts[s % 4], limit=max_new) for s in range(S)]
    if S > 1:
        seqs[1].update(a=T - 1, limit=seqs[1]["n0"] + 2)   # ends by its limit inside the step
    if S > 2:
        seqs[2].update(a=T - 1, eos_row=2)                  # ends by EOS inside the step
        seqs[3].update(k=-1)
    lg, draft = planted(S, T, V, seqs, gen)
    st = state(S, max_new, seqs)
    ws = ops.spec_logprob_workspace(V, "cpu")
    verify_step(st, lg.clone(), draft, T, ws)
    pl = state(S, max_new, seqs)
    pl["lp_raw"] = torch.full((S, V), POISON)
    c0 = pl["gen_len"].clone()
    for s in range(S):
        sl = slice(s, s + 1)
        for t in range(int(st["gen_len"][s]) - int(c0[s])):
            row = lg[s * T + t:s * T + t + 1].clone()
            ops.logprob_scan(row, pl["lp_k"][sl], pl["finished"][sl], pl["gen_len"][sl], pl["lp_raw"][sl],
                             pl["lp_n0"][sl])
            ops.argmax_commit(row, pl["out_tokens"][sl], pl["gen_len"][sl], pl["input_ids"][sl], pl["positions"][sl],
                              pl["finished"][sl], pl["eos"], limit=pl["limit"][sl], eos_on=pl["eos_on"][sl])
            ops.logprob_commit(pl["lp_raw"][sl], pl["lp_k"][sl], pl["lp_n0"][sl], pl["gen_len"][sl],
                               pl["out_tokens"][sl], pl["lp_tok"][sl], pl["lp_ids"][sl], pl["lp_top"][sl], 1)
    for k in ("out_tokens", "gen_len", "finished", "lp_tok", "lp_ids", "lp_top"):
        assert torch.equal(st[k], pl[k]), k
    assert int((st["lp_tok"] != POISON).sum()) == sum(int(st["gen_len"][s]) - int(c0[s]) for s in range(S)
                                                       if seqs[s]["k"] >= 0) > 0


def test_ops_refusals_cpu():
    refusals("cpu")


def refusals(dev):
    """Every bad size, dtype and short buffer raises ValueError before anything is written."""
    V, max_new = 64, 6

    def call(S=2, T=4, ws=None, **bad):
        seqs = [dict(k=3, n0=1, a=0, limit=max_new) for _ in range(S)]
        st = state(S, max_new, seqs, dev)
        lg = torch.ones(S * T, V, device=dev)
        ws = ops.spec_logprob_workspace(V, dev) if ws is None else ws
        for w in ws:
            w.fill_(3)
        st.update({k: v.to(dev) for k, v in bad.items()})
        before = {k: v.clone() for k, v in st.items()}
        wb = [w.clone() for w in ws]
        with pytest.raises(ValueError):
            ops.spec_logprob_scan(lg, T, st["lp_k"], st["finished"], st["gen_len"], st["lp_n0"], ws)
        with pytest.raises(ValueError):
            ops.spec_logprob_commit(T, st["lp_k"], st["lp_n0"], st["gen_len"], st["out_tokens"], st["lp_tok"],
                                    st["lp_ids"], st["lp_top"], ws)
        for k, v in st.items():
            assert torch.equal(v, before[k]), k
        assert all(torch.equal(a, b) for a, b in zip(ws, wb))

    call(T=0)
    call(T=9)
    call(S=9, T=2)
    call(S=5, T=8)            # S * T = 40
    call(S=8, T=8)
    call(lp_k=torch.zeros(0, **I32))   # S = 0
    small = ops.spec_logprob_workspace(V, dev)
    call(ws=(small[0][:16], small[1], small[2]))      # a raw buffer of fewer than 32 rows
    call(ws=(small[0], small[1][:-1], small[2]))      # short chunk workspaces
    call(ws=(small[0], small[1], small[2][:-1]))
    call(ws=(small[0].double(), small[1], small[2]))
    call(ws=(small[0], small[1], small[2].int()))
    call(lp_k=torch.zeros(2, dtype=torch.int64))
    call(lp_n0=torch.zeros(1, **I32), gen_len=torch.zeros(1, **I32))  # state of fewer than S rows
    # what only one of the two reads
    seqs = [dict(k=3, n0=1, a=0, limit=max_new)] * 2
    st = state(2, max_new, seqs, dev)
    ws = ops.spec_logprob_workspace(V, dev)
    scan = lambda lg, **kw: ops.spec_logprob_scan(lg, 4, *[kw.get(k, st[k]) for k in (  # noqa: E731
        "lp_k", "finished", "gen_len", "lp_n0")], ws)
    for lg in (torch.ones(8, V + 1, device=dev), torch.ones(7, V, device=dev), torch.ones(8, V, device=dev).double(),
               torch.ones(V, 8, device=dev).t()):
        with pytest.raises(ValueError):
            scan(lg)
    with pytest.raises(ValueError):
        ops.spec_logprob_scan(torch.ones(2, 262145, device=dev), 2, st["lp_k"][:1], st["finished"], st["gen_len"],
                              st["lp_n0"], ws)
    cm = lambda **kw: ops.spec_logprob_commit(4, *[kw.get(k, st[k]) for k in (  # noqa: E731
        "lp_k", "lp_n0", "gen_len", "out_tokens", "lp_tok", "lp_ids", "lp_top")], ws)
    z = lambda *shape, **kw: torch.zeros(*shape, device=dev, **kw)  # noqa: E731
    for kw in (dict(lp_ids=z(2, max_new, 21, **I32), lp_top=z(2, max_new, 21)),  # kcap outside 0 .. 20
               dict(lp_tok=z(2, max_new + 1)), dict(lp_ids=z(2, max_new - 1, 20, **I32), lp_top=z(2, max_new - 1, 20)),
               dict(lp_top=z(2, max_new, 20, dtype=torch.float64)), dict(out_tokens=z(1, max_new, **I32)),
               dict(out_tokens=z(2, max_new, dtype=torch.int64))):
        with pytest.raises(ValueError):
            cm(**kw)
    assert bool((st["lp_tok"] == POISON).all()) and bool((st["lp_top"] == POISON).all())
    assert st["lp_n0"].tolist() == [-1, -1]
    cm()  # ... and the good call goes through (nothing announced: nothing recorded)
    assert bool((st["lp_tok"] == POISON).all())


# ------------------------------------------------------------------------------------------------ engine (tiny model)
BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"
OLLAMA = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1, seed=11)
LP = dict(logprobs=True, spec_logprobs=True)
N = 30


def make(**kw):
    return build_engine("tiny-nsql", device="cpu", max_slots=4, max_model_len=512, seed=0, **kw)


def params(opts, n=N):
    return SamplingParams(**{"max_tokens": n, "ignore_eos": "regex" not in opts, **opts})


_SOLO = {}


def solo(prompt, opts, n=N):
    """The request generated alone by an engine without speculation: its result (tokens and logprobs)."""
    key = (prompt if isinstance(prompt, str) else tuple(prompt), tuple(sorted(opts.items())), n)
    if key not in _SOLO:
        if "eng" not in _SOLO:
            _SOLO["eng"] = make(guided=True, logprobs=True)
        eng = _SOLO["eng"]
        ids = ids_of(eng, prompt) if isinstance(prompt, str) else list(prompt)
        _SOLO[key] = eng.generate([ids], params(opts, n))[0]
        assert eng.stats["spec_steps"] == 0
    return _SOLO[key]


def run(eng, reqs_spec, n=N):
    ns = [n] * len(reqs_spec) if isinstance(n, int) else list(n)
    reqs = [eng.add_request(ids_of(eng, p) if isinstance(p, str) else list(p), params(o, m))
            for (p, o), m in zip(reqs_spec, ns)]
    eng.run_until_done(reqs)
    return reqs


def check(eng, reqs, reqs_spec, n=N, speculated=True):
    for q, (p, o) in zip(reqs, reqs_spec):
        got, want = eng.result(q), solo(p, o, n)
        assert got.token_ids == want.token_ids, o
        assert got.logprobs == want.logprobs, o  # bit for bit: the CPU verify rows are the plain step's rows
        if o.get("logprobs"):
            assert len(got.logprobs) == got.eval_count == len(got.token_ids)
        else:
            assert got.logprobs is None
        if speculated:
            assert q.spec_steps > 0, o  # (fails without the feature: a request that asks never speculates)


ASK5 = dict(logprobs=True, top_logprobs=5)
ASK0 = dict(logprobs=True)


def test_engine_greedy_ngram_drafts():
    eng = make(spec_tokens=K, **LP)
    spec = [(PROMPTS[0], ASK5)]
    reqs = run(eng, spec, 40)
    check(eng, reqs, spec, 40)
    st = eng.stats
    assert st["spec_steps"] > 0 and st["spec_accepted"] >= 1 and st["spec_steps"] + st["spec_accepted"] == 39
    assert st["logprob_steps"] == st["decode_steps"] == st["spec_steps"]  # the verify steps count as logprob steps


@pytest.mark.parametrize("kind,per_step", [("right", K), ("wrong", 0), ("first", 1)])
def test_engine_greedy_planted_drafts(kind, per_step):
    spec = [(PROMPTS[0], ASK5)]
    want = solo(PROMPTS[0], ASK5, 40)
    eng = make(spec_tokens=K, **LP)
    eng.runner.set_spec_forced(forced_table(want.token_ids, kind, eng.runner.V))
    reqs = run(eng, spec, 40)
    check(eng, reqs, spec, 40)
    steps = -(-39 // (per_step + 1))
    assert (reqs[0].spec_steps, reqs[0].spec_accepted) == (steps, 39 - steps)


def test_engine_sampled():
    spec = [(PROMPTS[1], dict(ASK5, **OLLAMA))]
    eng = make(spec_tokens=K, spec_sampled=True, **LP)
    check(eng, run(eng, spec), spec)
    # raw rule: what is reported is the model's own distribution, whatever the penalty and the sampler did to it
    lps = eng.result(run(eng, spec)[0]).logprobs
    assert all(e["logprob"] <= e["top_logprobs"][0]["logprob"] for e in lps)
    assert any(e["token"] != e["top_logprobs"][0]["token"] for e in lps)


def test_engine_guided_lists_masked_tokens():
    spec = [(PROMPTS[0], dict(ASK5, regex=BOUNDED))]
    eng = make(spec_tokens=K, guided=True, spec_guided=True, **LP)
    reqs = run(eng, spec)
    check(eng, reqs, spec)
    lps = eng.result(reqs[0]).logprobs
    # greedy over the allowed tokens: where the raw top-1 is another token, that token was masked out -- and is listed
    assert any(e["top_logprobs"][0]["token"] != e["token"] and e["top_logprobs"][0]["logprob"] > e["logprob"]
               for e in lps)


BATCH = {
    "greedy": ([(PROMPTS[0], ASK5), (PROMPTS[1], ASK0), (PROMPTS[2], {})], dict(spec_batch=4)),
    "sampled": ([(PROMPTS[0], ASK5), (PROMPTS[1], dict(ASK0, **OLLAMA)), (PROMPTS[2], {})],
                dict(spec_batch=4, spec_sampled=True, spec_batch_sampled=True)),
    "guided": ([(PROMPTS[0], dict(ASK5, regex=BOUNDED)), (PROMPTS[1], ASK0), (PROMPTS[2], {})],
               dict(spec_batch=4, guided=True, spec_guided=True, spec_batch_guided=True)),
    "all": ([(PROMPTS[0], dict(ASK5, regex=BOUNDED)), (PROMPTS[1], ASK0), (PROMPTS[2], OLLAMA)],
            dict(spec_batch=4, guided=True, spec_guided=True, spec_batch_guided=True, spec_sampled=True,
                 spec_batch_sampled=True)),
}


def spy(eng):
    calls, inner = [], eng.runner.decode_spec

    def decode_spec(steps, **kw):
        calls.append(dict(kw))
        return inner(steps, **kw)

    eng.runner.decode_spec = decode_spec
    return calls


@pytest.mark.parametrize("name", sorted(BATCH))
def test_engine_spec_batch(name):
    spec, flags = BATCH[name]
    eng = make(spec_tokens=K, **flags, **LP)
    calls = spy(eng)
    reqs = run(eng, spec)
    check(eng, reqs, spec)
    big = [c for c in calls if c.get("S", 1) > 1]
    assert big and all(c.get("logprobs") is True for c in big)  # one asking request no longer makes the run plain
    assert eng.stats["spec_steps"] == sum(q.spec_steps for q in reqs)


def test_preemption_mid_run():
    """The scenario of test_spec_batch_cpu.test_preempted_request_resumes_in_a_batch with every request asking: each
    list is complete and in order, what was read before the slot went stays bit for bit, and the victim speculates
    again after it resumes."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    ns = [150, 100, 150]
    eng = make(num_kv_blocks=8, spec_tokens=K, spec_batch=4, **LP)
    eng.run_ahead = 8
    sp = dict(logprobs=True, top_logprobs=1)
    reqs = [eng.add_request(p, params(sp, n)) for p, n in zip(prompts, ns)]
    kept, preempt, after = {}, eng._preempt, {}

    def hook(q):
        preempt(q)
        assert len(q.logprobs) == len(q.resumed) and q.lp_read == 0
        kept[q.rid] = list(q.logprobs)
        after[q.rid] = q.spec_steps

    eng._preempt = hook
    eng.run_until_done(reqs)
    assert eng.stats["preempted"] >= 1 and kept and eng.stats["spec_steps"] > 0
    for q, p, n in zip(reqs, prompts, ns):
        r = eng.result(q)
        assert len(r.token_ids) == n == len(r.logprobs)
        assert [x["token"] for x in r.logprobs] == [eng.tok.decode([t]) for t in r.token_ids]
        assert all(x["top_logprobs"][0]["logprob"] == x["logprob"] for x in r.logprobs)  # greedy: top-1, none shifted
        if q.rid in kept:
            assert q.logprobs[:len(kept[q.rid])] == kept[q.rid] and q.spec_steps > after[q.rid]
        else:  # up to the CPU GEMMs' batch-size dependence in the plain runs of bucket 4 (tests/test_logprobs_cpu.py)
            w = solo(p, sp, n)
            assert r.token_ids == w.token_ids
            assert all(abs(x["logprob"] - y["logprob"]) <= 2.0 ** -8 for x, y in zip(r.logprobs, w.logprobs))


def test_second_request_arrives_mid_run():
    """verify steps with records -> plain logprob steps of bucket 2 -> verify steps again: one list, nothing lost."""
    want = solo(PROMPTS[0], ASK5, 60)
    eng = make(spec_tokens=K, **LP)
    eng.runner.set_spec_forced(forced_table(want.token_ids, "first", eng.runner.V))
    a = eng.add_request(ids_of(eng, PROMPTS[0]), params(ASK5, 60))
    eng.step()
    m, s0 = a.gen_host, a.spec_steps
    assert s0 > 0 and len(a.logprobs) == m and not a.done.is_set()
    b = eng.add_request(ids_of(eng, PROMPTS[1])[:20], params(dict(speculate=False), 3))
    eng.run_until_done([b])
    assert a.spec_steps == s0 and len(a.logprobs) == a.gen_host > m  # plain steps of two rows, recorded all the same
    eng.run_until_done([a])
    got = eng.result(a)
    assert a.spec_steps > s0 and got.token_ids == want.token_ids and len(got.logprobs) == 60
    assert got.logprobs[:m] == want.logprobs[:m]
    assert [x["token"] for x in got.logprobs] == [x["token"] for x in want.logprobs]
    assert all(abs(x["logprob"] - y["logprob"]) <= 2.0 ** -8 for x, y in zip(got.logprobs, want.logprobs))


@pytest.fixture(scope="module")
def svc():
    engs = {"spec": make(spec_tokens=K, **LP), "plain": make(logprobs=True)}
    s = EngineService(lambda model: engs[model], defaults={"num_predict": 12, "ignore_eos": True})
    s.engs = engs
    yield s
    for m in s.models():
        s.loop(m).close()


def test_streamed_pieces_concatenate(svc):
    opts = {"logprobs": True, "top_logprobs": 3, "num_predict": 40}
    s0 = svc.engs["spec"].stats["spec_steps"]
    whole = svc.generate("spec", "count the rows", options=opts)
    chunks = list(svc.generate_stream("spec", "count the rows", options=opts))
    cat = [e for c in chunks for e in (c.logprobs or [])]
    assert cat == whole.logprobs and len(cat) == 40 == whole.eval_count
    assert "".join(c.response for c in chunks) == whole.response
    assert sum(1 for c in chunks if c.logprobs) > 1
    assert svc.engs["spec"].stats["spec_steps"] > s0
    base = svc.generate("plain", "count the rows", options=opts)
    assert svc.engs["plain"].stats["spec_steps"] == 0
    assert base.logprobs == whole.logprobs and base.response == whole.response


# ------------------------------------------------------------------------------------------------ gating
def test_without_the_flag_an_asking_request_never_speculates():
    eng = make(spec_tokens=K, spec_batch=4, logprobs=True)
    assert eng.runner.spec_logprobs is False and "spec_lp_ws" not in eng.runner.__dict__
    spec = [(PROMPTS[0], ASK5)]
    check(eng, run(eng, spec), spec, speculated=False)
    assert eng.stats["spec_steps"] == 0
    three = BATCH["greedy"][0]  # ... and makes a spec_batch run plain for its neighbours
    reqs = run(eng, three)
    assert eng.stats["spec_steps"] == 0 and [q.output_ids for q in reqs] == [solo(p, o).token_ids for p, o in three]
    free = [(PROMPTS[2], {})]
    assert run(eng, free)[0].spec_steps > 0
    with pytest.raises(AssertionError, match="spec_logprobs"):
        eng.runner.decode_spec(1, logprobs=True)
    with pytest.raises(AssertionError, match="spec_logprobs"):
        eng.runner._verify_step(logprobs=True)
    with pytest.raises(AssertionError, match="enable_logprobs"):
        make(spec_tokens=K).runner.decode_spec(1, logprobs=True)
    # inert without logprobs and without spec_tokens
    eng = make(spec_logprobs=True, spec_tokens=K)
    assert not eng.logprobs and eng.runner.logprobs_bytes() == 0 and run(eng, free)[0].spec_steps > 0
    eng = make(**LP)
    check(eng, run(eng, spec), spec, speculated=False)


def test_a_run_in_which_nobody_asked_keeps_its_verify_steps():
    eng = make(spec_tokens=K, spec_batch=4, **LP)
    calls = spy(eng)
    n = eng.stats["logprob_steps"]
    reqs = run(eng, [(p, {}) for p in PROMPTS])
    assert calls and all("logprobs" not in c for c in calls) and eng.stats["logprob_steps"] == n
    assert [q.output_ids for q in reqs] == [solo(p, {}).token_ids for p in PROMPTS]
    del calls[:]
    run(eng, [(PROMPTS[0], ASK0)])
    assert calls and all(c.get("logprobs") is True for c in calls)


def test_graph_keys():
    """Every existing verify key is unchanged; the logprob variant is that key with a trailing "lp" (after S)."""
    eng = make(spec_tokens=K, spec_batch=4, guided=True, spec_guided=True, spec_sampled=True, spec_batch_sampled=True,
               spec_batch_guided=True, **LP)
    r = eng.runner
    seen = []

    class Recorder(dict):
        def __contains__(self, key):
            seen.append(key)
            raise KeyError  # stop before any capture: the CPU has no graphs

    r.use_graphs, r.graphs = True, Recorder()
    T, plan = r.spec_k() + 1, None
    for kw in (dict(), dict(guided=True), dict(sample=True), dict(guided=True, sample=True), dict(S=4),
               dict(S=2, sample=True), dict(S=4, guided=True, sample=True)):
        for lp in (False, True):
            with pytest.raises(KeyError):
                r.decode_spec(1, logprobs=lp, **kw)
        base, with_lp = seen[-2], seen[-1]
        plan = tuple(r.ctx_plan(kw.get("S", 1), None))
        want = ("spec", T, plan, 0) + ((True,) if kw.get("guided") else ())
        want += (("sample",) if kw.get("sample") else ()) + ((kw["S"],) if kw.get("S", 1) > 1 else ())
        assert base == want and with_lp == want + ("lp",)


def test_flag_plumbing_memory_and_health(monkeypatch):
    assert Settings().spec_logprobs is False
    monkeypatch.setenv("LSA_SPEC_LOGPROBS", "1")
    assert Settings().spec_logprobs is True
    monkeypatch.delenv("LSA_SPEC_LOGPROBS")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-logprobs"])).spec_logprobs is True
    assert Settings.from_cli(ap.parse_args([])).spec_logprobs is False
    off, on = make(spec_tokens=K, logprobs=True), make(spec_tokens=K, **LP)
    assert off.runner.spec_logprobs is False and on.runner.spec_logprobs is True
    V = on.runner.V
    nch = -(-V // 2048)
    assert on.runner.logprobs_bytes() - off.runner.logprobs_bytes() == 32 * (V * 4 + nch * (8 + 32 * 8))
    raw, ms, cand = ops.spec_logprob_workspace(V, "cpu")
    assert tuple(raw.shape) == (32, V) and ms.numel() == 32 * nch * 2 and cand.numel() == 32 * nch * 32
    assert tuple(on.runner.spec_lp_raw().shape) == (K + 1, V) and tuple(on.runner.spec_lp_raw(2).shape) == (2, K + 1, V)
    s = EngineService(lambda m: on if m == "on" else off)
    try:
        s.generate("on", "hi", options={"num_predict": 2})
        s.generate("off", "hi", options={"num_predict": 2})
        h = s.health()["engines"]
        assert h["on"]["spec_logprobs"] is True and h["off"]["spec_logprobs"] is False
    finally:
        for m in s.models():
            s.loop(m).close()
    from llm_based_apache_spark_optimization_amd.serving.service import engine_factory
    built = {}

    def fake_build(model, **kw):
        built.update(kw)
        raise RuntimeError("stop")

    import llm_based_apache_spark_optimization_amd.engine as engine_pkg
    monkeypatch.setattr(engine_pkg, "build_engine", fake_build)
    with pytest.raises(RuntimeError, match="stop"):
        engine_factory(dataclasses.replace(Settings(), logprobs=True, spec_tokens=K, spec_logprobs=True))("tiny-nsql")
    assert built["spec_logprobs"] is True and built["logprobs"] is True


def test_nl2sql_confidence_from_a_speculating_request(svc, tmp_path):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context

    s = Settings(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"),
                 history_dsn="sqlite:///" + str(tmp_path / "h.db"), engine="hip", secret_key="test",
                 nl2sql_model="spec", explain_model="spec", logprobs=True, sql_logprobs=True, spec_tokens=K,
                 spec_logprobs=True)
    c = TestClient(create_app(make_context(s, backend=svc)))
    s0 = svc.engs["spec"].stats["spec_steps"]
    body = {"question": "how many rows", "table_schema": "Name (string)", "options": {"num_predict": 16}}
    r = c.post("/nl2sql", json=body).json()
    assert r["sql_min_logprob"] <= r["sql_mean_logprob"] <= 0.0
    assert svc.engs["spec"].stats["spec_steps"] > s0  # the operator keeps the verify steps on /nl2sql
    s2 = dataclasses.replace(s, nl2sql_model="plain", explain_model="plain")
    r2 = TestClient(create_app(make_context(s2, backend=svc))).post("/nl2sql", json=body).json()
    assert (r2["sql_query"], r2["sql_mean_logprob"], r2["sql_min_logprob"]) == \
        (r["sql_query"], r["sql_mean_logprob"], r["sql_min_logprob"])
