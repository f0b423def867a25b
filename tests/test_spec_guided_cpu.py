"""Speculative decoding for regex-constrained requests on the CPU (``spec_guided``): the host twins of the verify-row mask
and the state hand-over (ops.reference.dfa_mask_verify / dfa_spec_advance) against the plain rule -- T single-row
``ref.dfa_mask`` calls in states walked token by token -- and the engine's guided verify steps against its plain guided
steps: the same tokens, whatever is drafted.  The case list and its runner are shared with the GPU file."""
import argparse
import itertools
import random
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.guided import DEAD, MAX_TABLE, compile_regex
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_cpu import K, PROMPT, SYSTEM, forced_table

BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"  # test_guided_cpu.py's pattern
ALPHA = b"abcdefghijklmnopqrstuvwxyz01234"
TINY = r"(ab|c)+(d?;)?"
LIMIT = r"(abcdefghijklmnopqrstuvwxyz01234){33}"  # 1024 states x 32 classes = the table-size limit
EOS = [5, 40]  # id 5 has zero bytes, id 40 has bytes: an EOS id is ruled by accept[cur] alone
I32 = dict(dtype=torch.int32)


def _vocab(V):
    """Synthetic token table (the one of test_guided_gpu.py): lengths 0, 1, 2, 7, 32 and 33, tokens that die on their
    last byte, for both DFAs."""
    tail = ALPHA[3:] + ALPHA[:3]  # what follows "...abc" in LIMIT
    words = [b"", b"a", b"ab", b"c", b"abc", b"", b"abababc", b"c" * 32, b"c" * 33, b"abx", b"cc;x", b"d;", b";",
             b"cd;", b"d", b"de", tail[:7], (tail + tail)[:32], (tail + tail)[:33], b"defghiX", b"dx", b"x", b"ab;",
             b"abd", b"cab", b"k"]
    rng = random.Random(V)
    while len(words) < V:
        k = rng.random()
        if k < 0.05:
            words.append(b"")
        elif k < 0.5:
            words.append(bytes(rng.choice(b"abcd;x") for _ in range(rng.randint(1, 6))))
        else:  # runs of the LIMIT cycle from a random phase, sometimes broken at the end
            p, n = rng.randrange(31), rng.randint(1, 12)
            w = (ALPHA * 2)[p:p + n]
            words.append(w + b"#" if rng.random() < 0.2 else w)
    lens = [len(w) for w in words]
    off = torch.tensor([0] + list(itertools.accumulate(lens)), **I32)
    blob = torch.tensor(list(b"".join(words)), dtype=torch.uint8)
    return words, off, blob


def _tables(dfas, slots):
    cls = torch.zeros(slots, 256, dtype=torch.uint8)
    trans = torch.full((slots, MAX_TABLE), -1, dtype=torch.int16)
    accept = torch.zeros(slots, MAX_TABLE, dtype=torch.uint8)
    dim = torch.zeros(slots, 2, **I32)
    for r, d in enumerate(dfas):
        sc = d.n_states * d.n_classes
        cls[r] = torch.from_numpy(d.cls)
        trans[r, :sc] = torch.from_numpy(d.trans.view("int16"))
        accept[r, : d.n_states] = torch.from_numpy(d.accept)
        dim[r] = torch.tensor([d.n_states, d.n_classes], **I32)
    return cls, trans, accept, dim


class Env:
    """The tables of one vocabulary size on the host and on ``dev``: table row 0 = TINY, row 1 = LIMIT (the kernel takes
    the table row as an argument; the state row is always 0).  ``allowed(r, s)`` is the plain rule's mask of state s:
    one single-row ``ref.dfa_mask`` launch at its base, cached -- the reference every case shares."""

    def __init__(self, V, dev="cpu"):
        self.V, self.dev = V, dev
        self.words, off, blob = _vocab(V)
        self.dfas = (compile_regex(TINY), compile_regex(LIMIT))
        assert self.dfas[1].n_states * self.dfas[1].n_classes == MAX_TABLE
        cls, trans, accept, dim = _tables(self.dfas, 2)
        self.host = dict(off=off, blob=blob, cls=cls, trans=trans, accept=accept, dim=dim,
                         eos=torch.tensor(EOS, **I32), base0=torch.zeros(2, **I32), on1=torch.ones(2, **I32))
        self.d = {k: v.to(dev) for k, v in self.host.items()}
        self.tok = {w: i for i, w in reversed(list(enumerate(self.words)))}  # first id of each word
        self._allowed = {}

    def tok_walk(self, r, s, t):
        """The state after token id t from state s, by the Python DFA: DEAD for no / an unknown / a 0- or > 32-byte token."""
        if s == DEAD or not 0 <= t < self.V or not 1 <= len(self.words[t]) <= 32:
            return DEAD
        return self.dfas[r].walk(s, self.words[t])

    def allowed(self, r, s):
        if (r, s) not in self._allowed:
            h = self.host
            row = torch.zeros(1, self.V)
            z = torch.zeros(1, **I32)
            ref.dfa_mask(row, h["off"], h["blob"], h["cls"], h["trans"], h["accept"], h["dim"], h["on1"],
                         torch.full((2, 2), s, **I32), h["base0"], z, z, z, h["eos"], rows=torch.tensor([r], **I32))
            self._allowed[(r, s)] = torch.isfinite(row[0])
        return self._allowed[(r, s)]

    def legal(self, r, s, k, skip=0):
        """k drafts that are each legal after the one before, from state s (varied: the (skip + i)-th candidate)."""
        out = []
        for i in range(k):
            # (nothing with 'd' or ';': TINY's statement must stay open for the drafts that follow)
            closes = (lambda w: b"d" in w or b";" in w) if r == 0 else (lambda w: False)
            cand = [t for t, w in enumerate(self.words) if t not in EOS and not closes(w)
                    and self.tok_walk(r, s, t) != DEAD]
            t = cand[(skip + i) % len(cand)]
            out.append(t)
            s = self.tok_walk(r, s, t)
        return out

    def illegal(self, r, s):
        return next(t for t, w in enumerate(self.words) if 1 <= len(w) <= 32 and self.dfas[r].walk(s, w) == DEAD)


def cases(env, k):
    """name -> dict(r, n, base, prev (the state the slots hold), in_tok, draft [k], on, finished): the issue's list,
    for both DFAs where the DFA matters."""
    tk = env.tok
    out = {}
    for r, name, prefix in ((0, "tiny", b"ab"), (1, "limit", ALPHA * 5 + b"abc")):
        d = env.dfas[r]
        s = d.walk(d.start, prefix)
        assert s != DEAD
        first = env.legal(r, s, 1)[0]                 # an input token, legal from s
        s1 = env.tok_walk(r, s, first)
        for n, base, tag in ((4, 4, "base_even"), (3, 3, "base_odd"), (6, 0, "adv_even"), (7, 0, "adv_odd")):
            cur = s if n == base else s1
            c = dict(r=r, n=n, base=base, prev=s, in_tok=first, on=1, finished=0)
            out[f"{name}_{tag}_legal"] = dict(c, draft=env.legal(r, cur, k, skip=n))
            if tag in ("base_even", "adv_odd"):
                lg = env.legal(r, cur, k)
                out[f"{name}_{tag}_illegal_first"] = dict(c, draft=[env.illegal(r, cur)] + lg[:k - 1])
                mid = cur
                for t in lg[:k - 1]:
                    mid = env.tok_walk(r, mid, t)
                out[f"{name}_{tag}_illegal_last"] = dict(c, draft=lg[:k - 1] + [env.illegal(r, mid)])
        c = dict(r=r, n=5, base=0, prev=s, in_tok=first, on=1, finished=0)
        lg = env.legal(r, s1, k)
        at = min(1, k - 1)
        out[f"{name}_minus_one"] = dict(c, draft=lg[:at] + [-1] + lg[at + 1:])
        out[f"{name}_zero_bytes"] = dict(c, draft=lg[:at] + [tk[b""]] + lg[at + 1:])
        out[f"{name}_out_of_range"] = dict(c, draft=lg[:at] + [env.V + 3] + lg[at + 1:])
        out[f"{name}_dead_input"] = dict(c, in_tok=tk[b"x"], draft=lg)   # a token from outside the mask: EOS only
        out[f"{name}_finished"] = dict(c, draft=lg, finished=1)
        out[f"{name}_off"] = dict(c, draft=lg, on=0)
    t0 = env.dfas[0]
    s = t0.walk(t0.start, b"ab")
    c = dict(r=0, n=2, base=0, prev=t0.start, in_tok=tk[b"ab"], on=1, finished=0)
    # 33 bytes of "c": the DFA would take them, the length rule does not
    out["tiny_33_bytes"] = dict(c, draft=env.legal(0, s, k - 1) + [tk[b"c" * 33]])
    out["tiny_32_bytes"] = dict(c, draft=([tk[b"c" * 32]] + env.legal(0, s, k))[:k])
    # "d;" ends the statement: every later row is EOS-only (the drafts after it die, whatever they are)
    out["tiny_ends"] = dict(c, draft=([tk[b"d;"], tk[b"c"], EOS[1], tk[b"ab"]] + [tk[b"c"]] * k)[:k])
    return out


def expected(env, c, T):
    """(states s_0..s_{T-1}, g_state after the launch) by the plain rule and the Python DFA."""
    r, n = c["r"], c["n"]
    slots = [c["prev"], c["prev"]]
    if n == c["base"]:
        other = env.dfas[r].start
        slots[(n - 1) & 1] = other  # a different state in the slot the launch must not read
        s = slots[n & 1]
    else:
        slots[n & 1] = env.dfas[r].start  # overwritten by the launch
        s = env.tok_walk(r, slots[(n - 1) & 1], c["in_tok"])
    before = list(slots)
    if n != c["base"]:
        slots[n & 1] = s
    states = [s]
    for t in c["draft"][:T - 1]:
        states.append(env.tok_walk(r, states[-1], t))
    return states, before, slots


def run_case(env, c, T, gen, advance_for=None):
    """One launch of ops.dfa_mask_verify on env.dev (twice: the second repeats the first bit for bit), checked against T
    single-row plain masks; then, for every a in ``advance_for``, ops.dfa_spec_advance at gen_len = n + a + 1 followed by
    a plain ops.dfa_mask launch with an arbitrary next token, checked against the mask of the state walked from scratch."""
    d, dev, r, n, k = env.d, env.dev, c["r"], c["n"], T - 1
    states, before, after = expected(env, c, T)
    live = c["on"] == 1 and c["finished"] == 0
    logits = torch.randn(T, env.V, generator=gen)
    want = logits.clone()
    if live:
        for t in range(T):
            want[t][~env.allowed(r, states[t])] = float("-inf")
    on = torch.ones(2, **I32)
    on[r] = c["on"]
    base = torch.zeros(2, **I32)
    base[r] = c["base"]
    mk = lambda v: torch.tensor(v, **I32).to(dev)  # noqa: E731
    g_state = torch.zeros(2, 2, **I32)
    g_state[r] = torch.tensor(before, **I32)
    g_state, g_spec = g_state.to(dev), torch.full((9,), -7, **I32).to(dev)
    on, base = on.to(dev), base.to(dev)
    gl, ii, fin, dr = mk([n]), mk([c["in_tok"]]), mk([c["finished"]]), mk(c["draft"][:k])
    want_state = torch.zeros(2, 2, **I32)
    want_state[r] = torch.tensor(after if live else before, **I32)
    want_spec = torch.tensor(([n] + states + [-7] * (8 - T)) if live else [-7] * 9, **I32)
    for _ in range(2):
        got = logits.to(dev)
        ops.dfa_mask_verify(got, d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"], on, g_state, base,
                            gl, ii, fin, d["eos"], dr, g_spec, r=r)
        assert torch.equal(got.cpu(), want)  # allowed: bit-unchanged; the others: -inf
        assert torch.equal(g_state.cpu(), want_state) and torch.equal(g_spec.cpu(), want_spec)
    if not live:
        assert torch.equal(want, logits)
        return
    nxt = env.tok[b"c"] if r == 0 else env.tok[b"d"]  # an arbitrary next token
    for a in (advance_for if advance_for is not None else range(k + 1)):
        st, gl2 = g_state.clone(), mk([n + a + 1])
        ops.dfa_spec_advance(on, st, g_spec, gl2, k, r=r)
        assert int(st[r, (n + a) & 1]) == states[a]
        row = torch.randn(1, env.V, generator=gen)
        got = row.to(dev)
        ops.dfa_mask(got, d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"], on, st, base, gl2,
                     mk([nxt]), mk([0]), d["eos"], rows=mk([r]))
        s_next = env.tok_walk(r, states[a], nxt)  # input, drafts 1..a and that token, from scratch
        want_row = row.clone()
        want_row[0][~env.allowed(r, s_next)] = float("-inf")
        assert torch.equal(got.cpu(), want_row), (a, states[a], s_next)
        assert int(st[r, (n + a + 1) & 1]) == s_next


# ------------------------------------------------------------------------------------------------ twins
_ENV = Env(2500)
CASE_NAMES = sorted(cases(_ENV, K))  # the names depend on neither V nor k


@pytest.fixture(scope="module")
def env():
    return _ENV


@pytest.mark.parametrize("name", CASE_NAMES)
def test_ref_verify_mask_equals_plain_rule(env, name):
    c = cases(env, K)[name]
    run_case(env, c, K + 1, torch.Generator().manual_seed(len(name)))


def test_ref_case_list_is_what_it_says(env):
    """The cases exercise what their names claim (a list that silently degenerates would check nothing)."""
    cs = cases(env, K)
    for name, c in cs.items():
        states, _, _ = expected(env, c, K + 1)
        if name.endswith("_legal") or name == "tiny_32_bytes":
            assert DEAD not in states, name
        if name.endswith("illegal_first"):
            assert states[0] != DEAD and states[1] == DEAD, name
        if name.endswith("dead_input"):
            assert set(states) == {DEAD}, name
        if name.endswith("illegal_last"):
            assert DEAD not in states[:-1] and states[-1] == DEAD, name
        if name.split("_", 1)[1] in ("minus_one", "zero_bytes", "out_of_range"):
            at = min(1, K - 1)
            assert DEAD not in states[:at + 1] and set(states[at + 1:]) == {DEAD}, name
    s33 = expected(env, cs["tiny_33_bytes"], K + 1)[0]
    assert s33[-1] == DEAD and s33[-2] != DEAD
    ends = expected(env, cs["tiny_ends"], K + 1)[0]
    assert env.allowed(0, ends[1]).nonzero().flatten().tolist() == EOS and ends[2] == DEAD
    assert env.allowed(0, DEAD).nonzero().flatten().tolist() == EOS  # a DEAD row: EOS only, by the plain rule
    assert {c["n"] & 1 for c in cs.values()} == {0, 1}
    assert any(c["n"] == c["base"] for c in cs.values()) and any(c["n"] != c["base"] for c in cs.values())


def test_ops_validate_rows():
    e = Env(64)
    d = e.d
    z = torch.zeros(1, **I32)
    for T in (1, 9):
        with pytest.raises(ValueError, match="2 <= T <= 8"):
            ops.dfa_mask_verify(torch.zeros(T, 64), d["off"], d["blob"], d["cls"], d["trans"], d["accept"], d["dim"],
                                d["on1"], torch.zeros(2, 2, **I32), d["base0"], z, z, z, d["eos"],
                                torch.zeros(8, **I32), torch.zeros(9, **I32))


# ------------------------------------------------------------------------------------------------ engine
def make(**kw):
    return build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, seed=0, **kw)


def gen(eng, n=64, **opts):
    return eng.generate([PROMPT], SamplingParams(max_tokens=n, regex=BOUNDED, **opts), system=SYSTEM)[0]


def counters(n, per_step):
    """(spec_steps, spec_accepted) of an n-token answer whose every verify step accepts per_step drafts until the EOS
    ends the last one early: the prefill commits token 0, every later token is a step's first or an accepted draft."""
    steps = -(-(n - 1) // (per_step + 1))
    return steps, (n - 1) - steps


@pytest.fixture(scope="module")
def plain_guided():
    eng = make(guided=True)
    res = gen(eng)
    assert eng.stats["spec_steps"] == 0 and re.fullmatch(BOUNDED, res.text)
    return eng, res.token_ids


def test_engine_ngram_equals_plain_guided(plain_guided):
    _, want = plain_guided
    eng = make(guided=True, spec_tokens=K, spec_guided=True)
    assert eng.runner.spec_guided and eng.runner.g_spec.numel() == 9
    res = gen(eng)
    assert res.token_ids == want  # bit for bit: the CPU twins compute a verify row as the plain step does
    assert re.fullmatch(BOUNDED, res.text) and res.done_reason == "stop" and res.token_ids[-1] in eng.runner.eos_list
    st = eng.stats
    assert st["spec_steps"] > 0 and st["guided_steps"] > 0
    assert st["spec_steps"] + st["spec_accepted"] == len(want) - 1
    # an unconstrained request on the same engine takes the unguided verify step
    g0, s0 = st["guided_steps"], st["spec_steps"]
    eng.generate([PROMPT], SamplingParams(max_tokens=16, ignore_eos=True), system=SYSTEM)
    assert eng.stats["guided_steps"] == g0 and eng.stats["spec_steps"] > s0


@pytest.mark.parametrize("kind,per_step", [("right", K), ("wrong", 0), ("first", 1)])
def test_engine_forced_drafts(plain_guided, kind, per_step):
    _, want = plain_guided
    eng = make(guided=True, spec_tokens=K, spec_guided=True)
    eng.runner.set_spec_forced(forced_table(want, kind, eng.runner.V))
    res = gen(eng)
    assert res.token_ids == want and re.fullmatch(BOUNDED, res.text)
    steps, accepted = counters(len(want), per_step)
    assert (eng.stats["spec_steps"], eng.stats["spec_accepted"]) == (steps, accepted)
    assert eng.stats["guided_steps"] >= steps


def test_engine_acceptance_guard_falls_back_to_plain_guided_steps(plain_guided):
    _, want = plain_guided
    assert len(want) - 1 > 16
    eng = make(guided=True, spec_tokens=K, spec_guided=True)
    eng.runner.set_spec_forced(forced_table(want, "wrong", eng.runner.V))
    eng.runner.spec_min_accept = 1.5
    res = gen(eng)
    assert res.token_ids == want and re.fullmatch(BOUNDED, res.text)
    # 16 verify steps at zero acceptance (two runs of sync_every = 8), then plain guided steps: the hand-over
    assert eng.stats["spec_steps"] == 16 and eng.stats["spec_accepted"] == 0
    assert eng.stats["guided_steps"] >= len(want) - 1


def test_engine_second_request_mid_run(plain_guided):
    """verify steps -> bucket-2 plain guided steps (an unconstrained request joins) -> verify steps again."""
    _, want = plain_guided
    eng = make(guided=True, spec_tokens=K, spec_guided=True)
    eng.runner.set_spec_forced(forced_table(want, "wrong", eng.runner.V))  # one token per verify step
    ids = eng.encode(eng.render(PROMPT, SYSTEM, False))
    a = eng.add_request(ids, SamplingParams(max_tokens=64, regex=BOUNDED))
    eng.step()
    s0 = eng.stats["spec_steps"]
    assert 0 < s0 < len(want) - 1 and not a.done.is_set()
    b = eng.add_request(ids[:20], SamplingParams(max_tokens=3, ignore_eos=True))
    eng.run_until_done([b])
    assert eng.stats["spec_steps"] == s0 and not a.done.is_set()  # both ran plain steps of bucket 2
    eng.run_until_done([a])
    assert eng.stats["spec_steps"] > s0
    assert a.output_ids == want
    solo = make()
    assert b.output_ids == solo.generate([ids[:20]], SamplingParams(max_tokens=3, ignore_eos=True))[0].token_ids


def test_flag_plumbing(monkeypatch, plain_guided):
    _, want = plain_guided
    assert Settings().spec_guided is False
    monkeypatch.setenv("LSA_SPEC_GUIDED", "1")
    assert Settings().spec_guided is True
    monkeypatch.delenv("LSA_SPEC_GUIDED")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-guided"])).spec_guided is True
    assert Settings.from_cli(ap.parse_args([])).spec_guided is False
    # off (the default): a constrained request never speculates
    eng = make(guided=True, spec_tokens=K)
    assert eng.runner.spec_guided is False
    assert gen(eng).token_ids == want and eng.stats["spec_steps"] == 0
    # inert without guided (the request is rejected as before) or without spec_tokens
    eng = make(spec_tokens=K, spec_guided=True)
    with pytest.raises(ValueError, match="guided"):
        eng.add_request([1, 2, 3], SamplingParams(regex=BOUNDED))
    eng = make(guided=True, spec_guided=True)
    assert gen(eng).token_ids == want and eng.stats["spec_steps"] == 0
