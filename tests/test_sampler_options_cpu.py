"""The sampler options min_p, presence_penalty and frequency_penalty on the CPU: the host twins of the two device rules
(ops.reference repeat_penalty / spec_penalised_row and sample_probs / sample_pick) against independent statements of
the rules, the defaults (zeros are the call without the options), the verify commit against successive plain steps with
the options on, and the engine: the options change a seeded request's tokens, the tokens are the twins applied to the
engine's own logits, a greedy request with only a frequency penalty takes the sampling path with its ring seeded from
the prompt, and the speculating engines commit the plain engine's tokens.  tests/test_sampler_options_gpu.py pins the
kernels to these twins and shares the cases defined here."""
import collections
import math
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams
from llm_based_apache_spark_optimization_amd.engine.engine import SamplingOptionError
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_sampling_cpu import FAMILIES, M, family_case
from test_spec_batch_cpu import PROMPTS, forced_tables, ids_of, make
from test_spec_cpu import K, PROMPT, forced_table

I32 = dict(dtype=torch.int32)
W = 64
BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"  # test_guided_cpu.py's pattern
NAMES = ("out_tokens", "gen_len", "input_ids", "positions", "finished", "hist")


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def dyadic(shape, g, scale=2.0):
    """Random logits in multiples of 2^-4 (no -0.0: the device orders it below +0.0, torch does not)."""
    return torch.round(torch.randn(shape, generator=g) * scale * 16) / 16 + 0.0


# ---------------------------------------------------------------------------------------------------- penalty twin
def window_of(ring, pos, last_n):
    """The tokens at context positions (pos - n, pos], n = min(last_n, 64, pos + 1), of the position-indexed ring."""
    return [int(ring[(pos - i) % W]) for i in range(min(last_n, W, pos + 1))]


def penalised_f64(row, tokens, pen, pres, freq):
    """The two-step rule written out in float64 for dyadic operands: step 1 rounds to f32 (a division by 1.5 is not
    exact), the subtrahend c * freq + pres and the subtraction are exact in f64, and the result is rounded once."""
    out = row.clone()
    for t, c in collections.Counter(tokens).items():
        if 0 <= t < row.numel():
            l = float(row[t])
            l = f32(l / pen if l > 0 else l * pen)
            out[t] = l - (c * freq + pres)
    return out


# (repeat_penalty, presence, frequency): each alone with the other two off, mixed signs, all off
PENALTIES = [(1.0, 0.5, 0.0), (1.0, 0.0, 0.25), (1.0, -0.5, 1.5), (1.5, 0.25, -0.5), (0.5, 1.5, 0.25), (2.0, 0.0, 0.0),
             (1.0, 0.0, 0.0)]
V_PEN = 300


def rings(g):
    """name -> ring: a few distinct tokens (counts 1, 2, many), with -1 and out-of-range entries; one token 64 times."""
    mixed = torch.randint(0, 24, (W,), generator=g, dtype=torch.int32)
    mixed[5], mixed[17], mixed[40], mixed[63] = -1, V_PEN, V_PEN + 7, -1
    return {"mixed": mixed, "constant": torch.full((W,), 7, **I32)}


@pytest.mark.parametrize("pos", [3, 62, 63, 64, 130])
@pytest.mark.parametrize("last_n", [0, 1, 5, 64, 100])
def test_penalty_twin_equals_the_float64_rule(pos, last_n):
    g = torch.Generator().manual_seed(100 * pos + last_n)
    seen = set()
    for name, ring in rings(g).items():
        row = dyadic(V_PEN, g)
        toks = window_of(ring, pos, last_n)
        seen |= set(collections.Counter(t for t in toks if 0 <= t < V_PEN).values())
        for pen, pres, freq in PENALTIES:
            got = ref.repeat_penalty(row.clone(), ring, pen, pos, last_n, pres, freq)
            want = penalised_f64(row, toks, pen, pres, freq)
            assert torch.equal(got, want), (name, pen, pres, freq)
            if (pen, pres, freq) == (1.0, 0.0, 0.0) or not toks:
                assert torch.equal(got, row)
        # the positional form (no presence / frequency) is the repetition penalty alone
        assert torch.equal(ref.repeat_penalty(row.clone(), ring, 1.5, pos, last_n),
                           penalised_f64(row, toks, 1.5, 0.0, 0.0))
    if last_n >= 64 and pos >= 63:
        assert {1, 2, 64} <= seen  # single, repeated and the whole ring one token
    if pos == 3:
        assert len(toks) == min(last_n, 4)  # p + 1 < last_n: the window stops at position 0


def test_subtrahend_is_one_fused_multiply_add():
    """fma_f32 rounds c * f + p once: against exact rational arithmetic, on operands where the product alone, or the
    f64 sum, would round differently."""
    from fractions import Fraction

    def nearest_f32(x: Fraction) -> float:
        lo = f32(float(x))
        cands = {lo, float(torch.nextafter(torch.tensor(lo), torch.tensor(math.inf))),
                 float(torch.nextafter(torch.tensor(lo), torch.tensor(-math.inf)))}
        best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(torch.tensor(c).view(torch.int32)) & 1))
        return best

    g = torch.Generator().manual_seed(3)
    vals = (torch.randn(200, generator=g) * 0.7).tolist() + [0.1, 0.3, 1.1, -0.7, 2.0 ** -20, 1.0 + 2.0 ** -23]
    vals = [f32(v) for v in vals]
    for i, f in enumerate(vals):
        p = vals[(7 * i + 3) % len(vals)]
        for c in (1, 2, 3, 7, 63, 64):
            assert ref.fma_f32(c, f, p) == nearest_f32(Fraction(c) * Fraction(f) + Fraction(p)), (c, f, p)


@pytest.mark.parametrize("pos", [3, 62, 63, 64, 130])
@pytest.mark.parametrize("last_n", [0, 1, 5, 64, 100])
def test_spec_penalised_row_is_the_ring_after_the_drafts(pos, last_n):
    """Row i < 8 equals the plain twin over a ring into which drafts 0 .. i-1 were committed: the counts include the
    drafts, an out-of-range or -1 draft counts for nothing."""
    g = torch.Generator().manual_seed(pos + last_n)
    ring = rings(g)["mixed"]
    rows = dyadic((8, V_PEN), g)
    draft = torch.tensor([3, V_PEN + 5, 3, int(ring[pos % W]), -1, 7, 3], **I32)
    for pen, pres, freq in PENALTIES:
        for i in range(8):
            after = ring.clone()
            for j in range(i):
                after[(pos + 1 + j) % W] = draft[j]
            want = ref.repeat_penalty(rows[i].clone(), after, pen, pos + i, last_n, pres, freq)
            got = ref.spec_penalised_row(rows[i].clone(), ring, draft, i, pen, pos, last_n, pres, freq)
            assert torch.equal(got, want), (pen, pres, freq, i)


# ---------------------------------------------------------------------------------------------------------- min_p
@pytest.mark.parametrize("T,K_,P", [(0.8, 40, 0.9), (1.0, 0, 1.0), (1.5, 10, 0.5), (0.3, 64, 0.95)])
@pytest.mark.parametrize("mp", [0.02, 0.3, 0.77])
def test_min_p_support(T, K_, P, mp):
    g = torch.Generator().manual_seed(11)
    row = torch.randn(300, generator=g) * 2
    idx0, p0 = ref.sample_probs(row, T, K_, P)
    idx, p = ref.sample_probs(row, T, K_, P, min_p=mp)
    assert torch.equal(idx, idx0)
    e = torch.exp((row[idx0].double() - float(row[idx0[0]])) / T)
    assert float(((e - mp).abs() / mp).min()) > 1e-3  # no candidate on the boundary, whatever the precision
    want = {int(idx0[i]) for i in range(idx0.numel()) if float(p0[i]) > 0 and (i == 0 or float(e[i]) >= mp)}
    assert set(idx[p > 0].tolist()) == want and int(idx0[0]) in want
    assert abs(float(p.sum()) - 1) < 1e-5
    # the exact twin of the device pick draws from the same support
    picks = {ref.sample_pick(row, T, K_, P, (j + 0.5) / 512, min_p=mp) for j in range(512)} | \
            {ref.sample_pick(row, T, K_, P, u, min_p=mp) for u in (0.0, 1 - 2.0 ** -24, 1.0, 1.5)}
    assert picks == want
    assert ref.sample_pick(row, T, K_, P, 1.5, min_p=mp) == int(idx[torch.nonzero(p > 0)[-1]])  # fallback: last kept


def test_min_p_one_keeps_only_ties_of_the_maximum():
    g = torch.Generator().manual_seed(12)
    row = torch.randn(300, generator=g)
    row[5] = row[9] = float(row.max()) + 1.0
    row[200] = float(row[5]) - 2.0 ** -10  # the closest loser
    idx, p = ref.sample_probs(row, 0.8, 0, 1.0, min_p=1.0)
    assert set(idx[p > 0].tolist()) == {5, 9} and p[p > 0].tolist() == [0.5, 0.5]
    assert {ref.sample_pick(row, 0.8, 0, 1.0, u, min_p=1.0) for u in (0.0, 0.3, 0.6, 0.99, 1.5)} == {5, 9}


@pytest.mark.parametrize("fi", range(len(FAMILIES)))
def test_min_p_zero_is_the_call_without_it(fi):
    logits, temp, topk, topp, seeds, gen0 = family_case(fi, V=2049, B=6)
    for b in range(6):
        a = ref.sample_probs(logits[b], float(temp[b]), int(topk[b]), float(topp[b]))
        z = ref.sample_probs(logits[b], float(temp[b]), int(topk[b]), float(topp[b]), min_p=0.0)
        assert torch.equal(a[0], z[0]) and torch.equal(a[1], z[1])
        u = ref.device_uniform(int(seeds[b]), int(gen0[b]))
        args = (logits[b], float(temp[b]), int(topk[b]), float(topp[b]), u)
        assert ref.sample_pick(*args) == ref.sample_pick(*args, min_p=0.0)
        assert ref.sample_pick_set(*args, M) == ref.sample_pick_set(*args, M, min_p=0.0)
    assert ref.sample_pick(logits[0], 0.0 + 1e-6, 40, 0.9, 0.7, min_p=0.9) == int(logits[0].argmax())


# ------------------------------------------------------------------------------------------------------- defaults
def commit_inputs(fi, B, V=2049):
    """B rows of family ``fi`` with a ring from the rows' best tokens, every other row with a repetition penalty."""
    logits, temp, topk, topp, seeds, gen0 = family_case(fi, V=V, B=B)
    g = torch.Generator().manual_seed(fi)
    pool = logits.max(0).values.topk(32).indices.to(torch.int32)
    hist = pool[torch.randint(0, 32, (B, W), generator=g)].contiguous()
    pos = torch.tensor([(61 + 3 * b) % 140 for b in range(B)], **I32)
    st = dict(out_tokens=torch.full((B, 16), -1, **I32), gen_len=gen0.clone(), input_ids=torch.zeros(B, **I32),
              positions=pos, finished=torch.zeros(B, **I32), hist=hist)
    par = dict(penalty=torch.tensor([1.0 if b % 2 else 1.3 for b in range(B)]), temperature=temp, top_k=topk, top_p=topp,
               seeds=seeds, last_n=torch.tensor([(64, 8, 33)[b % 3] for b in range(B)], **I32))
    return logits, st, par


def clone(st):
    return {k: v.clone() for k, v in st.items()}


def plain_call(logits, st, par, **opt):
    ref.sample_commit(logits, st["hist"], par["penalty"], par["temperature"], par["top_k"], par["top_p"], par["seeds"],
                      st["out_tokens"], st["gen_len"], st["input_ids"], st["positions"], st["finished"],
                      par.get("eos", torch.tensor([-1], **I32)), par.get("limit"), par.get("eos_on"),
                      last_n=par["last_n"], **opt)


def verify_call(logits, draft, stats, st, par, device="cpu", **opt):
    d = lambda t: None if t is None else t.to(device)  # noqa: E731
    ops.spec_sample_commit(logits, d(draft), stats, st["hist"], d(par["penalty"]), d(par["temperature"]), d(par["top_k"]),
                           d(par["top_p"]), d(par["seeds"]), st["out_tokens"], st["gen_len"], st["input_ids"],
                           st["positions"], st["finished"], d(par.get("eos", torch.tensor([-1], **I32))),
                           d(par.get("limit")), d(par.get("eos_on")), last_n=d(par["last_n"]),
                           **{k: d(v) for k, v in opt.items()})


@pytest.mark.parametrize("fi", range(len(FAMILIES)))
def test_explicit_zeros_are_the_call_without_the_options(fi):
    B = 8
    logits, st0, par = commit_inputs(fi, B)
    zeros = dict(presence=torch.zeros(B), frequency=torch.zeros(B), min_p=torch.zeros(B))
    a, z, la, lz = clone(st0), clone(st0), logits.clone(), logits.clone()
    plain_call(la, a, par)
    plain_call(lz, z, par, **zeros)
    for name in NAMES:
        assert torch.equal(a[name], z[name]), name
    assert torch.equal(la, lz)
    # the verify commit: two sequences of four rows
    a, z, la, lz = clone(st0), clone(st0), logits.clone(), logits.clone()
    two = lambda st: {k: v[:2] for k, v in st.items()}  # noqa: E731
    draft = torch.tensor([[1, 2, 3], [-1, 5, 2050]], **I32)
    sa, sz = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    par2 = {k: v[:2] for k, v in par.items()}
    verify_call(la, draft, sa, two(a), par2)
    verify_call(lz, draft, sz, two(z), par2, **{k: v[:2] for k, v in zeros.items()})
    for name in NAMES:
        assert torch.equal(a[name], z[name]), name
    assert torch.equal(la, lz) and torch.equal(sa, sz) and int(sa[:, 0].sum()) == 2


# ------------------------------------------------------------------------- the verify commit vs successive plain steps
V_SPEC, MAX_NEW, N0 = 300, 16, 2
# per-sequence options (repeat_penalty, presence, frequency, min_p, temperature, last_n)
SEQ_OPTS = [(1.0, 0.5, 0.25, 0.3, 0.8, 64), (1.3, -0.5, 1.5, 0.0, 0.8, 5), (1.0, 0.0, 0.25, 0.0, 0.0, 64),
            (1.0, 0.0, 0.0, 0.0, 0.8, 64)]


def spec_case(T, pos, opt, salt=0):
    """T verify rows over V_SPEC tokens whose 40 leading ids fill the ring (so the penalties move the draws), and the
    state of a row at position ``pos`` with N0 tokens generated, with the options ``opt`` (a row of SEQ_OPTS)."""
    pen, pres, freq, mp, temp, last_n = opt
    g = torch.Generator().manual_seed(7 + pos + 1000 * salt + T)
    logits = torch.randn(T, V_SPEC, generator=g) * 2
    logits[:, :40] += 3.0
    hist = torch.randint(0, 40, (1, W), generator=g, dtype=torch.int32)
    if pos + 1 < W:
        hist[0, pos + 1:] = -1
    st = dict(out_tokens=torch.full((1, MAX_NEW), -1, **I32), gen_len=torch.tensor([N0], **I32),
              input_ids=torch.tensor([5], **I32), positions=torch.tensor([pos], **I32), finished=torch.zeros(1, **I32),
              hist=hist)
    par = dict(penalty=torch.tensor([pen]), temperature=torch.tensor([temp]), top_k=torch.tensor([40], **I32),
               top_p=torch.tensor([0.9]), seeds=torch.tensor([ref.pack_seed(1234 + pos + salt, 3)], dtype=torch.int64),
               last_n=torch.tensor([last_n], **I32), limit=torch.tensor([MAX_NEW], **I32), eos_on=torch.ones(1, **I32))
    opts = dict(presence=torch.tensor([pres]), frequency=torch.tensor([freq]), min_p=torch.tensor([mp]))
    return logits, st, par, opts


def plain_steps(logits, st, par, opts, n):
    toks = []
    for i in range(n):
        g0 = int(st["gen_len"])
        plain_call(logits[i:i + 1].clone(), st, par, **opts)
        toks.append(int(st["out_tokens"][0, g0]))
    return toks


def accepting(toks, a, k):
    return [toks[i] if i < a else (toks[i] + 1) % V_SPEC for i in range(k)]


@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("pos", [5, 62, 63, 64])
@pytest.mark.parametrize("oi", range(len(SEQ_OPTS)))
def test_verify_commit_equals_plain_steps_with_the_options(T, pos, oi):
    logits, st0, par, opts = spec_case(T, pos, SEQ_OPTS[oi])
    toks = plain_steps(logits, clone(st0), par, opts, T)
    for a in range(T):
        want, got = clone(st0), clone(st0)
        assert plain_steps(logits, want, par, opts, a + 1) == toks[:a + 1]
        stats = torch.zeros(3, dtype=torch.int64)
        verify_call(logits.clone(), torch.tensor(accepting(toks, a, T - 1), **I32), stats, got, par, **opts)
        for name in NAMES:
            assert torch.equal(got[name], want[name]), (a, name)
        assert stats.tolist() == [1, T - 1, a]


def test_the_options_move_the_draws_of_these_cases():
    """The cases above check what they claim: with the options most of them draw other tokens than without."""
    moved = 0
    for pos in (5, 62, 63, 64):
        for oi in range(3):
            logits, st0, par, opts = spec_case(8, pos, SEQ_OPTS[oi])
            off = {k: torch.zeros(1) for k in opts}
            moved += plain_steps(logits, clone(st0), par, opts, 8) != \
                plain_steps(logits, clone(st0), dict(par, penalty=torch.ones(1)), off, 8)
    assert moved >= 9


def stack(cases):
    logits = torch.cat([c[0] for c in cases])
    st = {k: torch.cat([c[1][k] for c in cases]) for k in NAMES}
    par = {k: torch.cat([c[2][k] for c in cases]) for k in cases[0][2]}
    opts = {k: torch.cat([c[3][k] for c in cases]) for k in cases[0][3]}
    return logits, st, par, opts


@pytest.mark.parametrize("S,T", [(2, 4), (4, 8)])
def test_verify_commit_of_several_sequences_equals_plain_steps(S, T):
    """Sequence s of one S-sequence call commits what its own plain steps commit, with its own options and its own
    number of accepted drafts; ring positions 62 .. 64 straddle the rows."""
    cases = [spec_case(T, (62, 63, 5, 64)[s], SEQ_OPTS[s], salt=s) for s in range(S)]
    toks = [plain_steps(c[0], clone(c[1]), c[2], c[3], T) for c in cases]
    acc = [(T - 1, 1, 0, 2)[s] for s in range(S)]
    drafts = torch.tensor([accepting(toks[s], acc[s], T - 1) for s in range(S)], **I32)
    logits, st, par, opts = stack(cases)
    stats = torch.zeros(S, 3, dtype=torch.int64)
    verify_call(logits, drafts, stats, st, par, **opts)
    for s, c in enumerate(cases):
        want = clone(c[1])
        plain_steps(c[0], want, c[2], c[3], acc[s] + 1)
        for name in NAMES:
            assert torch.equal(st[name][s:s + 1], want[name]), (s, name)
    assert stats.tolist() == [[1, T - 1, a] for a in acc]


# ------------------------------------------------------------------- the cases of the GPU file, and their decided share
# row: (repeat_penalty, presence, frequency, min_p, temperature); repeat penalties are powers of two, so that every
# operation of the penalty is exact on dyadic logits and the device's logits can be compared bit for bit
GPU_ROWS = [(1.0, 0.0, 0.0, 0.0, 0.8),     # everything off
            (2.0, 0.0, 0.0, 0.0, 0.8),     # the repetition penalty alone
            (1.0, 0.5, 0.0, 0.0, 0.8),     # presence alone
            (1.0, 0.0, 0.25, 0.0, 0.8),    # frequency alone
            (1.0, 0.0, 0.0, 0.3, 0.8),     # min_p alone
            (0.5, -0.5, 1.5, 0.3, 1.0),    # all of them
            (1.0, 0.0, 1.5, 0.3, 0.0),     # a greedy row with a frequency penalty (min_p inert)
            (2.0, 0.5, 0.25, 0.3, 0.8)]    # a finished row
GPU_POS = [62, 63, 64, 130, 3, 63, 64, 62]
GPU_LAST_N = [64, 64, 5, 100, 64, 64, 1, 64]


def gpu_case(V, key0=0):
    """The B = 8 rows of the GPU file's ``sample_commit`` case at vocabulary V: dyadic logits, per row a ring of tokens
    from among its 24 best (each several times, with a -1 and an out-of-range entry), the options of GPU_ROWS."""
    B = len(GPU_ROWS)
    g = torch.Generator().manual_seed(V)
    logits = dyadic((B, V), g)
    hist = torch.zeros(B, W, **I32)
    for b in range(B):
        pool = logits[b].topk(24).indices.to(torch.int32)
        hist[b] = pool[torch.randint(0, 24, (W,), generator=g)]
        hist[b, 9], hist[b, 33] = -1, V + 2
        if GPU_POS[b] + 1 < W:
            hist[b, GPU_POS[b] + 1:] = -1
    col = lambda i: torch.tensor([r[i] for r in GPU_ROWS])  # noqa: E731
    par = dict(penalty=col(0), temperature=col(4), top_k=torch.full((B,), 40, **I32), top_p=torch.full((B,), 0.9),
               seeds=torch.tensor([ref.pack_seed(key0 + 7919 * b + 17, b % 3) for b in range(B)], dtype=torch.int64),
               last_n=torch.tensor(GPU_LAST_N, **I32))
    opts = dict(presence=col(1), frequency=col(2), min_p=col(3))
    fin = torch.zeros(B, **I32)
    fin[7] = 1
    st = dict(out_tokens=torch.full((B, 8), -1, **I32), gen_len=torch.tensor([b % 3 for b in range(B)], **I32),
              input_ids=torch.arange(B, **I32) + 100, positions=torch.tensor(GPU_POS, **I32), finished=fin, hist=hist)
    return logits, st, par, opts


def gpu_case_rows(logits, st, par, opts):
    """The twin's penalised rows of ``gpu_case`` (every row, finished or not: the penalty kernel does not look)."""
    return torch.stack([ref.repeat_penalty(logits[b].clone(), st["hist"][b], float(par["penalty"][b]),
                                           int(st["positions"][b]), int(par["last_n"][b]),
                                           float(opts["presence"][b]), float(opts["frequency"][b]))
                        for b in range(logits.shape[0])])


def gpu_case_sets(logits, st, par, opts):
    """Per row the twin's admissible tokens (None for the finished row)."""
    rows = gpu_case_rows(logits, st, par, opts)
    out = []
    for b in range(logits.shape[0]):
        if int(st["finished"][b]):
            out.append(None)
        elif float(par["temperature"][b]) <= 0:
            out.append({int(rows[b].argmax())})
        else:
            out.append(ref.sample_pick_set(rows[b], float(par["temperature"][b]), int(par["top_k"][b]),
                                           float(par["top_p"][b]),
                                           ref.device_uniform(int(par["seeds"][b]), int(st["gen_len"][b])), M,
                                           min_p=float(opts["min_p"][b])))
    return out


GPU_KEY0 = {5000: 0, 2049: 0}  # seed bases for which the twin alone decides at least 95% of the draws (checked below)


@pytest.mark.parametrize("V", [5000, 2049])
def test_decided_share_of_the_gpu_case(V):
    case = gpu_case(V, GPU_KEY0[V])
    sets = [s for s in gpu_case_sets(*case) if s is not None]
    undecided = sum(len(s) > 1 for s in sets) / len(sets)
    print(f"V = {V}: {len(sets)} draws, undecided share {undecided:.4f}")
    assert undecided <= 0.05
    # the options move the draws of this case: other sets than the rows have with everything off
    logits, st, par, opts = case
    off = {k: torch.zeros_like(v) for k, v in opts.items()}
    plain = gpu_case_sets(logits, st, dict(par, penalty=torch.ones(len(GPU_ROWS))), off)
    moved = [b for b in range(len(GPU_ROWS)) if plain[b] != gpu_case_sets(*case)[b]]
    print("rows whose set the options change:", moved)
    assert len(moved) >= 3 and 0 not in moved


def gpu_spec_case(S, T, V=2049):
    """The S-sequence verify case of the GPU file: sequence s has the options SEQ_OPTS[s], its ring position among 62 ..
    64 (so the drafts straddle the wrap), and a seed scanned until every row of the all-right launch is decided.
    Returns (logits [S T, V], state, par, opts, picks [S][T])."""
    cases, picks = [], []
    for s in range(S):
        pen, pres, freq, mp, temp, last_n = SEQ_OPTS[s]
        pos = (62, 63, 64, 63)[s]
        g = torch.Generator().manual_seed(100 * S + 10 * T + s + V)
        logits = dyadic((T, V), g)
        pool = logits.max(0).values.topk(32).indices.to(torch.int32)
        hist = pool[torch.randint(0, 32, (1, W), generator=g)].contiguous()
        st = dict(out_tokens=torch.full((1, MAX_NEW), -1, **I32), gen_len=torch.tensor([N0 + s], **I32),
                  input_ids=torch.tensor([5], **I32), positions=torch.tensor([pos], **I32),
                  finished=torch.zeros(1, **I32), hist=hist)
        par = dict(penalty=torch.tensor([2.0 if pen != 1.0 else 1.0]), temperature=torch.tensor([temp]),
                   top_k=torch.tensor([40], **I32), top_p=torch.tensor([0.9]), last_n=torch.tensor([last_n], **I32),
                   limit=torch.tensor([MAX_NEW], **I32), eos_on=torch.ones(1, **I32))
        opts = dict(presence=torch.tensor([pres]), frequency=torch.tensor([freq]), min_p=torch.tensor([mp]))
        for key in range(1000 * s, 1000 * s + 5000):
            par["seeds"] = torch.tensor([ref.pack_seed(key, 3)], dtype=torch.int64)
            got = []
            for i in range(T):  # row i's penalty reads drafts 0 .. i-1 only
                d = torch.tensor((got + [0] * T)[:T - 1], **I32)
                sets = ref.spec_sample_pick_sets(logits, d, hist, par["penalty"], par["temperature"], par["top_k"],
                                                 par["top_p"], par["seeds"], st["gen_len"], st["positions"],
                                                 last_n=par["last_n"], **opts)
                if len(sets[i]) != 1:
                    break
                got.append(next(iter(sets[i])))
            if len(got) == T:
                break
        else:
            raise AssertionError("no seed decides every row")
        cases.append((logits, st, par, opts))
        picks.append(got)
    return stack(cases) + (picks,)


# ---------------------------------------------------------------------------------------------------------- engine
N = 32
SEED = 11
BASE = {"temperature": 0.8, "seed": SEED}
OPTS = {"temperature": 0.8, "min_p": 0.3, "presence_penalty": 0.5, "frequency_penalty": 0.25, "seed": SEED}
# (a negative frequency penalty rewards what the context holds: tiny-nsql's greedy tokens never repeat on their own, so
# a positive one would leave them where they are)
GREEDY_FREQ = {"temperature": 0.0, "repeat_penalty": 1.0, "frequency_penalty": -1.5, "seed": 5}
MODELS = ["tiny-nsql", "tiny-llama3"]
# tiny-llama3's random-init logits put the token it has just read 300 to 350 above every other one (404.7 against 54.9
# on PROMPT, the same lead on every prompt tried), and the three options of OPTS can take at most 64 * 0.25 + 0.5 = 16.5
# off a logit: with OPTS as they stand it generates token 13 for ever, with or without them.  Its sampled requests
# therefore carry a repetition penalty that breaks that loop (404.7 / 8 = 50.6) -- both the request with the three
# options and the one without them, so the three options are still the only difference between the two.
EXTRA = {"tiny-nsql": {}, "tiny-llama3": {"repeat_penalty": 8.0}}


def params(opts, n=N):
    return SamplingParams.from_ollama_options({"num_predict": n, "ignore_eos": True, **opts})


def spy_commits(monkeypatch):
    """Record the operands of every ``ops.sample_commit`` call (cloned before the call) the engines make."""
    calls, inner = [], ops.sample_commit

    def sample_commit(logits, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len, input_ids,
                      positions, finished, *a, **kw):
        calls.append(dict(logits=logits.float().cpu().clone(), hist=hist.cpu().clone(), seeds=seeds.cpu().clone(),
                          gen_len=gen_len.cpu().clone(), positions=positions.cpu().clone(),
                          finished=finished.cpu().clone()))
        return inner(logits, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len, input_ids,
                     positions, finished, *a, **kw)

    monkeypatch.setattr(ops, "sample_commit", sample_commit)
    return calls


def host_loop(calls, key, prompt, tokens, sp):
    """The request with seed ``key`` replayed on the host: at every recorded commit of one of its live rows, the twins
    applied to the engine's own logits of that row -- the penalties over the window of its context so far (the prompt
    and the tokens before this one: not the engine's ring), min_p in the distribution, the draw at the token's index
    -- must give the token the engine committed.  Returns the number of tokens checked."""
    n = 0
    for c in calls:
        for b in range(c["logits"].shape[0]):
            word = int(c["seeds"][b]) & ((1 << 64) - 1)
            if word & ((1 << 40) - 1) != key or int(c["finished"][b]):
                continue
            g = (word >> 40) + int(c["gen_len"][b])
            ctx = list(prompt) + list(tokens[:g])
            assert int(c["positions"][b]) == len(ctx) - 1
            row = c["logits"][b].clone()
            if sp.needs_sampler and (sp.repeat_penalty != 1.0 or sp.presence_penalty or sp.frequency_penalty):
                win = ctx[-min(sp.repeat_last_n, W):] if sp.repeat_last_n > 0 else []
                for t, cnt in collections.Counter(win).items():
                    row[t] = row[t] / f32(sp.repeat_penalty) if row[t] > 0 else row[t] * f32(sp.repeat_penalty)
                    row[t] = row[t] - ref.fma_f32(cnt, f32(sp.frequency_penalty), f32(sp.presence_penalty))
            if sp.temperature <= 0:
                tok = int(row.argmax())
            else:
                idx, p = ref.sample_probs(row, f32(sp.temperature), sp.top_k, f32(sp.top_p), min_p=f32(sp.min_p))
                gen = torch.Generator().manual_seed(ref.draw_seed(ref.pack_seed(key, 0), g))
                tok = int(idx[torch.multinomial(p, 1, generator=gen)])
            assert tok == tokens[g], (g, tok, tokens[g])
            n += 1
    return n


def generate(eng, opts, prompt=PROMPT, n=N):
    ids = ids_of(eng, prompt) if isinstance(prompt, str) else list(prompt)
    return eng.generate([ids], params(opts, n))[0].token_ids


_PLAIN = {}


def opts_of(model, name):
    return {"base": {**BASE, **EXTRA[model]}, "opts": {**OPTS, **EXTRA[model]}, "greedy_freq": GREEDY_FREQ}[name]


def plain(model, name):
    """The plain engine's tokens of BASE / OPTS / GREEDY_FREQ (computed once per model)."""
    if (model, name) not in _PLAIN:
        _PLAIN[model, name] = generate(make(model), opts_of(model, name))
    return _PLAIN[model, name]


@pytest.mark.parametrize("model", MODELS)
def test_engine_options_change_a_seeded_request(model):
    """(This is the test the engine without the feature fails: it ignored the three options.)"""
    assert plain(model, "opts") != plain(model, "base")
    assert generate(make(model), opts_of(model, "opts")) == plain(model, "opts")  # two runs agree
    if model != "tiny-nsql":
        return
    # each option alone moves the tokens too (tiny-nsql's logits are nearly flat: only at a low temperature do its
    # candidates fall below 0.3 of the best one, with top_p = 1 leaving that tail to min_p)
    flat = {"temperature": 0.1, "top_k": 0, "top_p": 1.0, "seed": SEED}
    base = generate(make(model), flat)
    for name in ("min_p", "presence_penalty", "frequency_penalty"):
        assert generate(make(model), {**flat, name: OPTS[name]}) != base, name


@pytest.mark.parametrize("model", MODELS)
def test_engine_tokens_are_the_twins_on_its_own_logits(model, monkeypatch):
    calls = spy_commits(monkeypatch)
    eng = make(model)
    toks = generate(eng, opts_of(model, "opts"))
    assert toks == plain(model, "opts")
    assert host_loop(calls, SEED, ids_of(eng, PROMPT), toks, params(opts_of(model, "opts"))) == N


@pytest.mark.parametrize("model", MODELS)
def test_greedy_request_with_a_frequency_penalty(model, monkeypatch):
    sp = params(GREEDY_FREQ)
    assert sp.needs_sampler and sp.temperature == 0 and sp.repeat_penalty == 1.0
    assert not params({"temperature": 0.0, "min_p": 0.5}).needs_sampler  # min_p is inert on a greedy request
    assert params({"presence_penalty": -0.5}).needs_sampler
    calls = spy_commits(monkeypatch)
    eng = make(model)
    ids = ids_of(eng, PROMPT)
    toks = generate(eng, GREEDY_FREQ)
    assert len(calls) == N  # the prefill's commit and every decode step took the sampling path
    # the ring the first commit read: the prompt's last 64 tokens, each at its position's slot
    ring = torch.full((W,), -1, **I32)
    for p in range(max(0, len(ids) - W), len(ids)):
        ring[p % W] = ids[p]
    assert torch.equal(calls[0]["hist"][0], ring) and int(calls[0]["positions"][0]) == len(ids) - 1
    raw = calls[0]["logits"][0]
    pen = ref.repeat_penalty(raw.clone(), ring, 1.0, len(ids) - 1, 64, 0.0, GREEDY_FREQ["frequency_penalty"])
    assert toks[0] == int(pen.argmax()) and not torch.equal(pen, raw)  # the first token is already penalised
    assert host_loop(calls, 5, ids, toks, sp) == N
    assert toks != generate(make(model), {"temperature": 0.0}) or model == "tiny-llama3"  # (see EXTRA)


def test_preempted_request_resumes_with_its_options(monkeypatch):
    """Two requests with the options in an arena too small for both (the scenario of test_spec_sampled_cpu's
    preemption test): the younger is preempted and re-admitted.  Its ring is re-seeded from the prompt and the tokens
    it had generated, and its draws continue at their counter: every token of both requests is the twins' token on
    the engine's own logits over the request's whole context -- before and after the preemption -- and up to the
    preemption both requests' tokens are those of the same workload in an arena that never runs dry.  (After it the
    context is re-prefilled, another computation than the decode steps that first produced it, so the unpreempted
    run is no bit-exact reference for the rest; the host loop is.)"""
    from llm_based_apache_spark_optimization_amd.engine import build_engine

    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(2)]
    opts = [dict(OPTS, seed=21), dict(GREEDY_FREQ, seed=22)]
    runs = []
    for blocks in (6, 64):
        calls = spy_commits(monkeypatch)
        eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, num_kv_blocks=blocks)
        eng.run_ahead = 16
        reqs = [eng.add_request(p, params(o, 150)) for p, o in zip(prompts, opts)]
        eng.run_until_done(reqs)
        monkeypatch.undo()
        runs.append((eng, reqs, calls))
    (eng, reqs, calls), (big, breqs, _) = runs
    assert eng.stats["preempted"] >= 1 and big.stats["preempted"] == 0
    victim = next(q for q in reqs if q.preemptions)
    m = len(victim.resumed)
    assert 0 < m < 150
    for q, b, p, o in zip(reqs, breqs, prompts, opts):
        assert len(q.output_ids) == 150
        assert q.output_ids[:m] == b.output_ids[:m], m  # (both ran in step until then; then the survivor ran alone)
        # (the victim's re-prefill commits token m a second time: one more recorded commit than tokens)
        assert host_loop(calls, o["seed"], p, q.output_ids, params(o, 150)) >= 150


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["opts", "greedy_freq"])
def test_speculating_engine_commits_the_plain_tokens(model, name):
    opts = opts_of(model, name)
    want = plain(model, name)
    eng = make(model, spec_tokens=K, spec_sampled=True)
    assert generate(eng, opts) == want  # n-gram drafts
    assert eng.stats["spec_steps"] > 0 and eng.stats["spec_steps"] + eng.stats["spec_accepted"] == N - 1
    for kind, per in (("right", K), ("first", 1), ("wrong", 0)):
        eng = make(model, spec_tokens=K, spec_sampled=True)
        eng.runner.set_spec_forced(forced_table(want, kind, eng.runner.V))
        assert generate(eng, opts) == want, kind
        steps = -(-(N - 1) // (per + 1))
        assert [eng.stats[k] for k in ("spec_steps", "spec_accepted")] == [steps, N - 1 - steps], kind


@pytest.mark.parametrize("model", MODELS)
def test_batched_speculation_next_to_a_greedy_neighbour(model):
    """spec_batch = 4 with spec_batch_sampled: a request with the options, a greedy neighbour and a greedy request with
    a frequency penalty in one run of verify steps, each committing the tokens it generates alone on a plain engine."""
    mixed = [opts_of(model, "opts"), {}, GREEDY_FREQ]
    want = [generate(make(model), o, prompt=p) for p, o in zip(PROMPTS, mixed)]
    for kinds in (None, ("first", "right", "wrong")):
        eng = make(model, spec_tokens=K, spec_batch=4, spec_sampled=True, spec_batch_sampled=True)
        if kinds:
            eng.runner.set_spec_forced(forced_tables(want, kinds, eng.runner.V))
        reqs = [eng.add_request(ids_of(eng, p), params(o)) for p, o in zip(PROMPTS, mixed)]
        batched = 0
        while not all(q.done.is_set() for q in reqs):
            before = [q.spec_steps for q in reqs]
            eng.step()
            batched += sum(q.spec_steps > b for q, b in zip(reqs, before)) >= 2
        assert [q.output_ids for q in reqs] == want, kinds
        assert batched > 0 and all(q.spec_steps > 0 for q in reqs)


def test_guided_speculation_with_the_options():
    opts = dict(OPTS, regex=BOUNDED)
    run = lambda e: e.generate([ids_of(e, PROMPT)], SamplingParams.from_ollama_options({"num_predict": 64, **opts}))[0]  # noqa: E731
    want = run(make(guided=True))
    assert re.fullmatch(BOUNDED, want.text)
    eng = make(guided=True, spec_tokens=K, spec_guided=True, spec_sampled=True)
    res = run(eng)
    assert res.token_ids == want.token_ids and res.done_reason == "stop"
    assert eng.stats["spec_steps"] > 0
    eng = make(guided=True, spec_tokens=K, spec_guided=True, spec_sampled=True)
    eng.runner.set_spec_forced(forced_table(want.token_ids, "right", eng.runner.V))
    assert run(eng).token_ids == want.token_ids


def test_neighbour_without_options_is_unchanged():
    """A greedy request and a sampled request without the options, each next to a request with them: their tokens are
    those they have next to the same request with the options off (the rows of a step do not read each other)."""
    out = {}
    for name, first in (("on", OPTS), ("off", BASE)):
        eng = make()
        reqs = [eng.add_request(ids_of(eng, p), params(o)) for p, o in zip(PROMPTS, [first, {}, dict(BASE, seed=3)])]
        eng.run_until_done(reqs)
        out[name] = [q.output_ids for q in reqs]
    assert out["on"][0] != out["off"][0]
    assert out["on"][1:] == out["off"][1:]


def test_from_ollama_options_round_trip_and_defaults():
    sp = SamplingParams.from_ollama_options({"min_p": 0.05, "presence_penalty": 1.5, "frequency_penalty": -0.25})
    assert (sp.min_p, sp.presence_penalty, sp.frequency_penalty) == (0.05, 1.5, -0.25)
    sp = SamplingParams.from_ollama_options({})
    assert (sp.min_p, sp.presence_penalty, sp.frequency_penalty) == (0.0, 0.0, 0.0) and not sp.needs_sampler
    assert SamplingParams() == SamplingParams(min_p=0.0, presence_penalty=0.0, frequency_penalty=0.0)


@pytest.mark.parametrize("bad", [{"min_p": float("nan")}, {"min_p": 1.5}, {"min_p": -0.1}, {"min_p": float("inf")},
                                 {"presence_penalty": float("nan")}, {"presence_penalty": float("inf")},
                                 {"frequency_penalty": float("-inf")}, {"frequency_penalty": float("nan")}])
def test_bad_values_are_rejected_at_add_request(bad):
    eng = engine_for_rejects()
    before = eng.sched.num_waiting
    with pytest.raises(SamplingOptionError):
        eng.add_request([1, 2, 3], params(bad))
    assert isinstance(SamplingOptionError("x"), ValueError) and eng.sched.num_waiting == before
    eng.add_request([1, 2, 3], params({"min_p": 1.0, "presence_penalty": -2.0}))  # the ends of the range are allowed


_REJECT = []


def engine_for_rejects():
    if not _REJECT:
        _REJECT.append(make())
    return _REJECT[0]
