"""Speculative decoding for several concurrent requests of which some are regex-constrained, on the CPU
(``spec_batch_guided``): the S-sequence forms of the verify-row mask and the state hand-over (ops.reference
dfa_mask_verify_batch / dfa_spec_advance_batch) against S one-sequence calls and against the plain rule, and the engine's
batched guided verify steps against each request generated alone without speculation: the same tokens, whatever is
drafted, whoever else runs.  The sequence mixes and their runner are shared with the GPU file."""
import argparse
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams
from llm_based_apache_spark_optimization_amd.engine.guided import DEAD

from test_spec_batch_cpu import PROMPTS, ids_of, make
from test_spec_cpu import K, forced_table
from test_spec_guided_cpu import BOUNDED, EOS, Env, _tables, _vocab, cases, expected

I32 = dict(dtype=torch.int32)

# ------------------------------------------------------------------------------------------------ sequence mixes
# (S, T) -> the mixes launched at that shape, each a list of S case names of test_spec_guided_cpu.cases ("idle" = the
# row release_slot leaves).  Sequence s of a mix runs in state row s on table row s = the DFA of its case.  No mix of
# two or four sequences can hold every kind of sequence the list below names, so a shape has several mixes, and
# ``check_mix_list`` asserts that those of each shape together hold all of them -- and each one a TINY and a LIMIT row.
SHAPES = {
    (2, 8): [["tiny_base_even_illegal_first", "limit_adv_odd_legal"], ["limit_off", "tiny_adv_even_legal"],
             ["tiny_finished", "limit_base_odd_legal"], ["limit_minus_one", "tiny_adv_odd_illegal_first"]],
    (4, 2): [["tiny_base_even_illegal_first", "limit_adv_odd_legal", "tiny_off", "limit_finished"],
             ["limit_minus_one", "tiny_adv_even_legal", "limit_base_odd_legal", "tiny_dead_input"]],
    (4, 8): [["limit_base_even_legal", "tiny_adv_odd_illegal_first", "limit_off", "tiny_finished"],
             ["tiny_minus_one", "limit_adv_even_legal", "tiny_base_odd_legal", "limit_adv_odd_illegal_last"]],
    (8, 4): [["tiny_base_even_legal", "limit_adv_odd_illegal_first", "tiny_off", "limit_finished", "limit_minus_one",
              "tiny_adv_even_legal", "idle", "limit_base_odd_legal"]],
}
MIXES = [(S, T, i) for (S, T), ms in SHAPES.items() for i in range(len(ms))]


def mix_cases(env, S, T, i):
    """The S case dicts of mix i of shape (S, T), drafts of k = T - 1 tokens."""
    cs = cases(env, T - 1)
    cs["idle"] = dict(cs["tiny_finished"], n=0, base=0, in_tok=0)
    out = [dict(cs[name], name=name) for name in SHAPES[(S, T)][i]]
    assert len(out) == S
    return out


def check_mix_list(env):
    """The mixes hold what the module comment claims (a list that silently degenerates would check nothing)."""
    for (S, T), ms in SHAPES.items():
        assert S * T <= 32
        union = []
        for i in range(len(ms)):
            mix = mix_cases(env, S, T, i)
            assert {c["r"] for c in mix} == {0, 1}  # a TINY and a LIMIT sequence: two tables in one launch
            union += mix
        live = [c for c in union if c["on"] and not c["finished"]]
        assert any(not c["on"] for c in union) and any(c["finished"] for c in union)
        assert any(c["n"] == c["base"] for c in live)
        assert {c["n"] & 1 for c in live if c["n"] != c["base"]} == {0, 1}  # lazy advances into both slots
        first_dead = [c for c in live if expected(env, c, T)[0][0] != DEAD and expected(env, c, T)[0][1] == DEAD]
        assert any(c["name"].endswith("illegal_first") for c in first_dead)
        assert any(c["name"].endswith("minus_one") for c in union)


class MixEnv:
    """One vocabulary on ``dev`` with the plain rule's masks (``Env.allowed``) and, per mix, S table rows."""

    def __init__(self, V, dev="cpu"):
        self.env, self.V, self.dev = Env(V, dev), V, dev

    def tables(self, mix):
        e = self.env
        cls, trans, accept, dim = _tables([e.dfas[c["r"]] for c in mix], len(mix))
        d = dict(off=e.host["off"], blob=e.host["blob"], cls=cls, trans=trans, accept=accept, dim=dim, eos=e.host["eos"])
        return {k: v.to(self.dev) for k, v in d.items()}


def operands(me, mix, T, fill=-7):
    """The state of a mix before the launch: dict of device tensors, and per sequence (states, g_state before, after)."""
    env, dev, S, k = me.env, me.dev, len(mix), T - 1
    exp = [expected(env, c, T) for c in mix]
    mk = lambda v: torch.tensor(v, **I32).to(dev)  # noqa: E731
    return dict(on=mk([c["on"] for c in mix]), base=mk([c["base"] for c in mix]),
                g_state=mk([e[1] for e in exp]), g_spec=torch.full((S, 9), fill, **I32).to(dev),
                gl=mk([c["n"] for c in mix]), ii=mk([c["in_tok"] for c in mix]), fin=mk([c["finished"] for c in mix]),
                dr=mk([t for c in mix for t in c["draft"][:k]])), exp


def verify_call(d, logits, o, g_state=None, g_spec=None, s=None):
    """ops.dfa_mask_verify on the mix's operands: the form over S sequences, or (``s``) the one-sequence form on
    sequence s's slices with table row s."""
    g_state = o["g_state"] if g_state is None else g_state
    g_spec = o["g_spec"] if g_spec is None else g_spec
    if s is None:
        return ops.dfa_mask_verify(logits, d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"], o["on"],
                                   g_state, o["base"], o["gl"], o["ii"], o["fin"], d["eos"], o["dr"], g_spec)
    k = o["dr"].numel() // o["gl"].numel()
    return ops.dfa_mask_verify(logits, d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"], o["on"],
                               g_state, o["base"], o["gl"][s:s + 1], o["ii"][s:s + 1], o["fin"][s:s + 1], d["eos"],
                               o["dr"][s * k:(s + 1) * k], g_spec, r=s)


def run_mix(me, mix, T, gen):
    """One launch of the S-form of ops.dfa_mask_verify on me.dev (twice: the second repeats the first bit for bit),
    checked against the plain-rule masks of the states walked token by token and, per sequence, against that sequence's
    own one-sequence launch; then the S-form of ops.dfa_spec_advance for a = 0, 1, k and another a per sequence, each
    checked against S one-sequence calls and followed by a plain ops.dfa_mask launch over the S rows with an arbitrary
    next token, checked against the mask of the state walked from scratch."""
    env, dev, S, k, V = me.env, me.dev, len(mix), T - 1, me.V
    d = me.tables(mix)
    o, exp = operands(me, mix, T)
    live = [c["on"] == 1 and c["finished"] == 0 for c in mix]
    logits = torch.randn(S * T, V, generator=gen)
    want = logits.clone()
    for s, c in enumerate(mix):
        if live[s]:
            for t in range(T):
                want[s * T + t][~env.allowed(c["r"], exp[s][0][t])] = float("-inf")
    want_state = torch.tensor([e[2] if lv else e[1] for e, lv in zip(exp, live)], **I32)
    want_spec = torch.tensor([([c["n"]] + e[0] + [-7] * (8 - T)) if lv else [-7] * 9
                              for c, e, lv in zip(mix, exp, live)], **I32)
    for _ in range(2):
        got = logits.to(dev)
        verify_call(d, got, o)
        assert torch.equal(got.cpu(), want)  # allowed: bit-unchanged; the others: -inf; untouched rows: bit-unchanged
        assert torch.equal(o["g_state"].cpu(), want_state) and torch.equal(o["g_spec"].cpu(), want_spec)
    for s in range(S):  # the sequence's own one-sequence launch: table row s, its slices of everything else
        o1, _ = operands(me, mix, T)
        rows, spec1 = logits[s * T:(s + 1) * T].to(dev), torch.full((9,), -7, **I32).to(dev)
        verify_call(d, rows, o1, g_spec=spec1, s=s)
        assert torch.equal(rows.cpu(), got[s * T:(s + 1) * T].cpu()), s
        assert torch.equal(spec1.cpu(), o["g_spec"][s].cpu()) and torch.equal(o1["g_state"][s].cpu(), o["g_state"][s].cpu())
        others = [j for j in range(S) if j != s]
        assert torch.equal(o1["g_state"][others].cpu(), operands(me, mix, T)[0]["g_state"][others].cpu())
    nxt = [env.tok[b"c"] if c["r"] == 0 else env.tok[b"d"] for c in mix]  # an arbitrary next token per sequence
    mk = lambda v: torch.tensor(v, **I32).to(dev)  # noqa: E731
    for accepted in ([0] * S, [min(1, k)] * S, [k] * S, [(s + 1) % (k + 1) for s in range(S)]):
        st = o["g_state"].clone()
        gl2 = mk([c["n"] + a + 1 if lv else c["n"] for c, a, lv in zip(mix, accepted, live)])  # (a dead row stands still)
        ops.dfa_spec_advance(o["on"], st, o["g_spec"], gl2, k)
        one = o["g_state"].clone()
        for s in range(S):
            ops.dfa_spec_advance(o["on"], one, o["g_spec"][s], gl2[s:s + 1], k, r=s)
        assert torch.equal(st.cpu(), one.cpu())
        for s, (c, a) in enumerate(zip(mix, accepted)):
            if live[s]:
                assert int(st[s, (c["n"] + a) & 1]) == exp[s][0][a], (s, a)
            else:
                assert torch.equal(st[s].cpu(), o["g_state"][s].cpu())
        rows = torch.randn(S, V, generator=gen)
        got = rows.to(dev)
        ops.dfa_mask(got, d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"], o["on"], st, o["base"], gl2,
                     mk(nxt), o["fin"], d["eos"])
        want_rows = rows.clone()
        for s, (c, a) in enumerate(zip(mix, accepted)):
            if live[s]:
                s_next = env.tok_walk(c["r"], exp[s][0][a], nxt[s])  # input, drafts 1..a and that token, from scratch
                want_rows[s][~env.allowed(c["r"], s_next)] = float("-inf")
                assert int(st[s, (c["n"] + a + 1) & 1]) == s_next, (s, a)
        assert torch.equal(got.cpu(), want_rows), accepted


def refusals(dev):
    """Every bad size raises ValueError before anything is written (the ops-level check comes before the extension's
    TORCH_CHECKs, which guard the same sizes for a direct caller)."""
    V = 64
    _, off, blob = _vocab(V)
    env = Env(V)

    def call(S, T, spec_rows=None, draft_n=None, slots=None, r=0, state_n=None, advance=True):
        slots = max(S, 1) if slots is None else slots
        cls, trans, accept, dim = _tables([env.dfas[s & 1] for s in range(slots)], slots)
        n = S if state_n is None else state_n
        t = lambda x: x.to(dev)  # noqa: E731
        outs = dict(logits=t(torch.ones(S * T, V)), g_state=t(torch.full((slots, 2), 3, **I32)),
                    g_spec=t(torch.full((S if spec_rows is None else spec_rows, 9), -7, **I32)))
        before = {k: v.clone() for k, v in outs.items()}
        z = lambda m: t(torch.zeros(m, **I32))  # noqa: E731
        args = (t(off), t(blob), t(cls), t(trans), t(accept), t(dim), t(torch.ones(slots, **I32)), outs["g_state"],
                z(slots), z(n), z(n), z(n), t(torch.tensor(EOS, **I32)),
                z(S * (T - 1) if draft_n is None else draft_n), outs["g_spec"])
        with pytest.raises(ValueError):
            ops.dfa_mask_verify(outs["logits"], *args, r=r)
        if advance:  # (the hand-over sees no logits: a g_spec of fewer rows is a smaller launch to it)
            with pytest.raises(ValueError):
                ops.dfa_spec_advance(args[6], outs["g_state"], outs["g_spec"], args[9], max(T - 1, 0), r=r)
        for k, v in outs.items():
            assert torch.equal(v, before[k]), k

    call(5, 8)                 # S * T = 40
    call(9, 2)                 # S = 9
    call(2, 1)                 # T = 1
    call(2, 9)                 # T = 9
    call(4, 4, spec_rows=3, advance=False)  # g_spec [S - 1, 9]: 16 rows do not divide among 3 sequences
    call(4, 4, slots=3)        # more sequences than table rows
    call(2, 4, slots=4, r=1)   # the form over S sequences is r = 0
    # operands that only the mask reads
    cls, trans, accept, dim = _tables([env.dfas[0], env.dfas[1]], 2)
    t = lambda x: x.to(dev)  # noqa: E731
    z = lambda m: t(torch.zeros(m, **I32))  # noqa: E731
    for draft_n, state_n in ((5, 2), (6, 1)):  # a short draft; one state row for two sequences
        logits, g_state, g_spec = t(torch.ones(8, V)), t(torch.full((2, 2), 3, **I32)), t(torch.full((2, 9), -7, **I32))
        with pytest.raises(ValueError):
            ops.dfa_mask_verify(logits, t(off), t(blob), t(cls), t(trans), t(accept), t(dim), t(torch.ones(2, **I32)),
                                g_state, z(2), z(state_n), z(state_n), z(state_n), t(torch.tensor(EOS, **I32)),
                                z(draft_n), g_spec)
        assert bool((logits == 1).all()) and bool((g_state == 3).all()) and bool((g_spec == -7).all())


# ------------------------------------------------------------------------------------------------ twins
_ME = MixEnv(2500)


def test_mix_list_is_what_it_says():
    check_mix_list(_ME.env)


@pytest.mark.parametrize("S,T,i", MIXES)
def test_ref_rows_equal_one_sequence_calls_and_plain_rule(S, T, i):
    run_mix(_ME, mix_cases(_ME.env, S, T, i), T, torch.Generator().manual_seed(100 * S + 10 * T + i))


def test_ops_refuse_bad_sizes():
    refusals("cpu")


# ------------------------------------------------------------------------------------------------ engine
LONG = r"(?i)(select|with) [a-c]{40,48} from temp_view;"  # an answer of 60-odd tokens, for the hand-overs
WORDS = r"[a-z ]{20,26}"                                   # another DFA in the neighbouring slot
OLLAMA = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1, seed=11)
ON = dict(guided=True, spec_tokens=K, spec_batch=4, spec_guided=True, spec_batch_guided=True)
ALL = dict(ON, spec_sampled=True, spec_batch_sampled=True)
# the engine cases: per request (prompt, options); a request with "regex" stops at its EOS, a free one runs to max_tokens
PAIR = [(PROMPTS[0], dict(regex=BOUNDED)), (PROMPTS[1], dict(regex=BOUNDED))]
WITH_FREE = [(PROMPTS[0], dict(regex=BOUNDED)), (PROMPTS[1], {})]
THREE = [(PROMPTS[0], dict(regex=BOUNDED)), (PROMPTS[1], {}), (PROMPTS[2], OLLAMA)]
SAMPLED_CONSTRAINED = [(PROMPTS[0], dict(regex=BOUNDED, **OLLAMA)), (PROMPTS[1], {}), (PROMPTS[2], dict(regex=WORDS))]
CASES = {"pair": (PAIR, ON), "with_free": (WITH_FREE, ON), "three": (THREE, ALL),
         "sampled_constrained": (SAMPLED_CONSTRAINED, ALL)}
N_FREE = 30  # tokens of a free request: the length of BOUNDED's answers, so that all requests of a case end together


def params(opts, n):
    return SamplingParams(**{"max_tokens": n, "ignore_eos": "regex" not in opts, **opts})


_SOLO = {}


def solo(model, prompt, opts, n, device="cpu", **kw):
    """The request generated alone by an engine without speculation (computed once per request): its result."""
    key = (model, device, prompt if isinstance(prompt, str) else tuple(prompt), tuple(sorted(opts.items())), n,
           tuple(sorted(kw.items())))
    if key not in _SOLO:
        from llm_based_apache_spark_optimization_amd.engine import build_engine
        eng = build_engine(model, device=device, max_slots=4, max_model_len=512, seed=0, guided=True, **kw)
        ids = ids_of(eng, prompt) if isinstance(prompt, str) else list(prompt)
        _SOLO[key] = eng.generate([ids], params(opts, n))[0]
        assert eng.stats["spec_steps"] == 0
    return _SOLO[key]


def spy(eng):
    """Record (guided, sample, S) of every ``decode_spec`` call of the engine's runner."""
    calls, inner = [], eng.runner.decode_spec

    def decode_spec(steps, max_ctx=None, guided=False, sample=False, S=1):
        calls.append((bool(guided), bool(sample), S))
        return inner(steps, max_ctx=max_ctx, guided=guided, sample=sample, S=S)

    eng.runner.decode_spec = decode_spec
    return calls


def run(eng, reqs_spec, n=N_FREE, watch=None, tweak=None):
    """Send the requests at once; step to the end.  Returns (requests, batched): batched = the engine iterations in
    which the verify-step counters of two or more requests advanced."""
    ns = [n] * len(reqs_spec) if isinstance(n, int) else list(n)
    reqs = [eng.add_request(ids_of(eng, p) if isinstance(p, str) else list(p), params(o, m))
            for (p, o), m in zip(reqs_spec, ns)]
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


def planted(tokens, kinds, V, S=4):
    """[S, nf, K]: table s plants drafts of ``kinds[s]`` for the request whose plain tokens are ``tokens[s]`` (answers
    of different lengths: the shorter tables are padded with rows no step reads)."""
    tabs = [forced_table(t, kind, V) for t, kind in zip(tokens, kinds)]
    out = torch.zeros(S, max(t.shape[0] for t in tabs), K, **I32)
    for s, t in enumerate(tabs):
        out[s, : t.shape[0]] = t
    return out


def check_results(eng, reqs, reqs_spec, want):
    for q, (p, o), w in zip(reqs, reqs_spec, want):
        assert q.output_ids == w.token_ids, o
        if "regex" in o:
            res = eng.result(q)
            assert re.fullmatch(o["regex"], res.text), res.text
            assert res.done_reason == "stop" and q.output_ids[-1] in eng.runner.eos_list
            assert w.done_reason == "stop" and w.text == res.text


def engine_case(model, name, kinds=None, device="cpu", **kw):
    """One case of CASES on a fresh engine, with n-gram drafts or (``kinds``: one kind for every request) planted ones:
    every request's tokens are its solo plain tokens; with planted drafts the counters are exact.  Returns the engine and
    the recorded decode_spec calls."""
    from llm_based_apache_spark_optimization_amd.engine import build_engine
    reqs_spec, flags = CASES[name]
    want = [solo(model, p, o, N_FREE, device=device, **kw) for p, o in reqs_spec]
    eng = build_engine(model, device=device, max_slots=4, max_model_len=512, seed=0, **flags, **kw)
    calls = spy(eng)
    if kinds is not None:
        eng.runner.set_spec_forced(planted([w.token_ids for w in want], [kinds] * len(want), eng.runner.V)
                                   .to(eng.runner.device))
    g0 = eng.stats["guided_steps"]
    reqs, batched = run(eng, reqs_spec)
    check_results(eng, reqs, reqs_spec, want)
    sampled = any(params(o, 1).needs_sampler for _, o in reqs_spec)
    big = [c for c in calls if c[2] > 1]
    assert batched > 0 and eng.stats["spec_steps"] > 0 and big
    # while a constrained request runs the batched steps are the guided ones, sampled exactly when one needs the sampler
    assert big[0] == (True, sampled, 2 if len(reqs_spec) == 2 else 4)
    assert all(c[:2] == (True, sampled) for c in big if c == big[0])
    assert eng.stats["guided_steps"] > g0 and eng.stats["spec_steps"] == sum(q.spec_steps for q in reqs)
    if kinds is not None:
        per = {"right": K, "wrong": 0, "first": 1}[kinds]
        for q, w in zip(reqs, want):
            n = len(w.token_ids)
            steps = -(-(n - 1) // (per + 1))
            assert (q.spec_steps, q.spec_accepted) == (steps, n - 1 - steps), (kinds, n)
    return eng, calls


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("kinds", [None, "right", "wrong", "first"])
def test_engine_batch_equals_solo_plain(name, kinds):
    engine_case("tiny-nsql", name, kinds)


def test_case_answers_end_together():
    """The planted-draft counters above are exact because no request of a case is left alone in a slot other than 0
    (where it would end on plain steps): BOUNDED's answers and the free requests have the same length."""
    for name, (reqs_spec, _) in CASES.items():
        lens = [len(solo("tiny-nsql", p, o, N_FREE).token_ids) for p, o in reqs_spec if o.get("regex") != WORDS]
        assert set(lens) == {N_FREE}, (name, lens)


def test_all_unconstrained_run_takes_the_unguided_batched_step():
    from llm_based_apache_spark_optimization_amd.engine import build_engine
    eng = build_engine("tiny-nsql", device="cpu", max_slots=4, max_model_len=512, seed=0, **ALL)
    calls = spy(eng)
    free = [(p, {}) for p in PROMPTS]
    g0 = eng.stats["guided_steps"]
    reqs, batched = run(eng, free, 24)
    assert batched > 0 and (False, False, 4) in calls and not any(g for g, _, _ in calls)
    assert eng.stats["guided_steps"] == g0
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, {}, 24).token_ids for p in PROMPTS]
    # ... and the same engine takes the guided step for the next run, which holds a constrained request
    reqs, _ = run(eng, WITH_FREE)
    assert (True, False, 2) in calls
    check_results(eng, reqs, WITH_FREE, [solo("tiny-nsql", p, o, N_FREE) for p, o in WITH_FREE])


# ------------------------------------------------------------------------------------------------ hand-overs
def build(**kw):
    from llm_based_apache_spark_optimization_amd.engine import build_engine
    return build_engine("tiny-nsql", device="cpu", max_slots=4, max_model_len=512, seed=0, **kw)


def test_third_request_arrives_mid_run():
    """batched guided verify steps -> plain guided steps of bucket 4 (a request that has opted out of speculation joins)
    -> batched guided verify steps again."""
    two = [(PROMPTS[0], dict(regex=LONG)), (PROMPTS[1], dict(regex=BOUNDED))]
    want = [solo("tiny-nsql", p, o, 96) for p, o in two]
    eng = build(**ON)
    eng.runner.set_spec_forced(planted([w.token_ids for w in want], ["wrong", "wrong"], eng.runner.V))  # one token a step
    a, b = (eng.add_request(ids_of(eng, p), params(o, 96)) for p, o in two)
    eng.step()
    s0 = eng.stats["spec_steps"]
    assert a.spec_steps > 0 and b.spec_steps > 0 and not a.done.is_set() and not b.done.is_set()
    short = ids_of(eng, PROMPTS[2])[:20]
    c = eng.add_request(short, SamplingParams(max_tokens=3, ignore_eos=True, speculate=False))
    eng.run_until_done([c])
    assert eng.stats["spec_steps"] == s0 and not a.done.is_set() and not b.done.is_set()  # all three ran plain steps
    g0 = eng.stats["guided_steps"]
    assert g0 >= s0 // 2 + 2
    eng.step()
    assert a.spec_steps + b.spec_steps > s0  # ... and the two are back on the batched guided verify steps
    eng.run_until_done([a, b])
    check_results(eng, [a, b], two, want)
    assert c.output_ids == solo("tiny-nsql", short, dict(speculate=False), 3).token_ids


def test_acceptance_guard_drops_one_constrained_request_then_plain_guided():
    two = [(PROMPTS[0], dict(regex=LONG)), (PROMPTS[1], dict(regex=LONG))]
    want = [solo("tiny-nsql", p, o, 96) for p, o in two]
    assert min(len(w.token_ids) for w in want) > 2 * 24
    eng = build(**dict(ON, spec_batch=2))
    eng.runner.set_spec_forced(planted([w.token_ids for w in want], ["wrong", "first"], eng.runner.V, S=2))
    eng.runner.spec_min_accept = 0.5
    (a, b), batched = run(eng, two, 96)
    check_results(eng, [a, b], two, want)
    # a: 16 verify steps at zero acceptance (checked every sync_every = 8 steps), then dropped on its own counters; b
    # accepted one draft a step, is not dropped, and takes plain guided steps of bucket 2 from then on all the same
    assert batched > 0 and a.spec_off and 16 <= a.spec_steps < 24 and a.spec_accepted == 0
    assert not b.spec_off and b.spec_steps == a.spec_steps and b.spec_accepted == b.spec_steps
    assert eng.stats["spec_steps"] == a.spec_steps + b.spec_steps
    assert eng.stats["guided_steps"] >= a.spec_steps + (len(want[0].token_ids) - 1 - a.spec_steps)


def test_one_request_finishes_early_then_one_sequence_guided_steps():
    """S = 2 -> the one-sequence guided verify step, when the request in slot 1 ends."""
    two = [(PROMPTS[0], dict(regex=LONG)), (PROMPTS[1], dict(regex=BOUNDED))]
    want = [solo("tiny-nsql", p, o, 96) for p, o in two]
    eng = build(**ON)
    calls = spy(eng)
    eng.runner.set_spec_forced(planted([w.token_ids for w in want], ["first", "first"], eng.runner.V))
    (a, b), batched = run(eng, two, 96)
    check_results(eng, [a, b], two, want)
    assert batched > 0 and (True, False, 2) in calls and (True, False, 1) in calls
    assert calls.index((True, False, 2)) < calls.index((True, False, 1))
    for q, w in zip((a, b), want):  # both speculated all their lives: the counters are those of one draft a step
        n = len(w.token_ids)
        assert (q.spec_steps, q.spec_accepted) == (-(-(n - 1) // 2), n - 1 - -(-(n - 1) // 2))


PREEMPT_RE = r"[a-c]{150,170};"


def test_preempted_constrained_request_resumes_in_a_batch():
    """Three constrained requests in an arena too small for all (the scenario of
    test_spec_batch_cpu.test_preempted_request_resumes_in_a_batch): the youngest is preempted by the plain run's growth,
    re-admitted in the DFA state its tokens reached (``_set_guided`` rewrites both slots) next to a request that still
    runs, and speculates again there."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    three = [(p, dict(regex=PREEMPT_RE)) for p in prompts]
    ns = [200, 120, 200]
    eng = build(num_kv_blocks=8, **ON)
    eng.run_ahead = 8
    seen = []

    def watch(eng, reqs):
        seen.append([(q.preemptions, q.spec_steps) for q in reqs])

    calls = spy(eng)
    reqs, batched = run(eng, three, ns, watch=watch)
    assert eng.stats["preempted"] >= 1 and batched > 0 and (True, False, 4) in calls
    victim = next(i for i, q in enumerate(reqs) if q.preemptions)
    for i, (q, (p, o), n) in enumerate(zip(reqs, three, ns)):
        w = solo("tiny-nsql", p, o, n)
        assert q.output_ids == w.token_ids, i
        text = eng.result(q).text
        if q.output_ids[-1] in eng.runner.eos_list:
            assert re.fullmatch(PREEMPT_RE, text), i
        else:  # stopped by its length limit: a prefix of a match
            assert re.fullmatch(r"[a-c]{1,170};?", text), i
    resumed = [j for j in range(1, len(seen)) if seen[j][victim][0] and seen[j][victim][1] > seen[j - 1][victim][1]
               and any(seen[j][o][1] > seen[j - 1][o][1] for o in range(3) if o != victim)]
    assert resumed, seen[-1]
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == 7


# ------------------------------------------------------------------------------------------------ flag
def assert_plain(eng, reqs_spec, n=16, **solo_kw):
    """While two or more of the requests run, no verify step is taken; every request's tokens are its solo tokens."""
    def watch(eng, reqs):
        seen.append((sum(not q.done.is_set() for q in reqs), eng.stats["spec_steps"]))

    seen = [(len(reqs_spec), eng.stats["spec_steps"])]
    reqs, batched = run(eng, reqs_spec, n, watch=watch)
    assert batched == 0
    assert all(b[1] == a[1] for a, b in zip(seen, seen[1:]) if a[0] >= 2), seen
    assert [q.output_ids for q in reqs] == [solo("tiny-nsql", p, o, n, **solo_kw).token_ids for p, o in reqs_spec]


def test_flag_plumbing(monkeypatch):
    assert Settings().spec_batch_guided is False
    monkeypatch.setenv("LSA_SPEC_BATCH_GUIDED", "1")
    assert Settings().spec_batch_guided is True
    monkeypatch.delenv("LSA_SPEC_BATCH_GUIDED")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-batch-guided"])).spec_batch_guided is True
    assert Settings.from_cli(ap.parse_args([])).spec_batch_guided is False
    assert make().runner.spec_batch_guided is False
    eng = build(**ON)
    assert eng.runner.spec_batch_guided is True and tuple(eng.runner.g_spec.shape) == (8, 9)
    from llm_based_apache_spark_optimization_amd.client import EngineService
    from llm_based_apache_spark_optimization_amd.serving.service import engine_factory
    svc = EngineService(lambda m: eng)
    try:
        svc.generate("tiny-nsql", "hi", options={"num_predict": 2})
        assert svc.health()["engines"]["tiny-nsql"]["spec_batch_guided"] is True
    finally:
        for lp in svc._loops.values():
            lp.close()
    assert callable(engine_factory)


def test_flag_off_and_prerequisites():
    # the flag off (the default): a constrained request makes the run plain, the buffers are the one-sequence ones
    eng = build(guided=True, spec_tokens=K, spec_batch=4, spec_guided=True)
    assert eng.runner.spec_batch_guided is False and eng.runner.g_spec.numel() == 9
    assert_plain(eng, WITH_FREE)
    eng.runner._spec_bufs()
    with pytest.raises(AssertionError, match="one-sequence"):
        eng.runner._verify_step(guided=True, S=2)
    with pytest.raises(AssertionError, match="spec_batch_guided"):
        eng.runner.decode_spec(1, guided=True, S=2)
    # inert without each prerequisite: spec_guided, spec_tokens, spec_batch > 1 ...
    assert_plain(build(guided=True, spec_tokens=K, spec_batch=4, spec_batch_guided=True), WITH_FREE)
    assert_plain(build(guided=True, spec_batch=4, spec_guided=True, spec_batch_guided=True), WITH_FREE)
    assert_plain(build(guided=True, spec_tokens=K, spec_guided=True, spec_batch_guided=True), WITH_FREE)
    # ... and guided: the constrained request is rejected as before, free requests speculate together as before
    eng = build(spec_tokens=K, spec_batch=4, spec_guided=True, spec_batch_guided=True)
    with pytest.raises(ValueError, match="guided"):
        eng.add_request([1, 2, 3], SamplingParams(regex=BOUNDED))
    reqs, batched = run(eng, [(p, {}) for p in PROMPTS[:2]], 16)
    assert batched > 0
    # a constrained request that needs the sampler needs spec_batch_sampled and spec_sampled too
    sampled = [(PROMPTS[0], dict(regex=BOUNDED, **OLLAMA)), (PROMPTS[1], {})]
    assert_plain(build(spec_sampled=True, **ON), sampled, N_FREE)
    # "speculate": false on a constrained request, and the acceptance guard's verdict on one, still make the run plain
    eng = build(**ON)
    assert_plain(eng, [(PROMPTS[0], dict(regex=BOUNDED, speculate=False)), (PROMPTS[1], {})], N_FREE)
    reqs, batched = run(eng, WITH_FREE)  # the same engine speculates once both requests may
    assert batched > 0
