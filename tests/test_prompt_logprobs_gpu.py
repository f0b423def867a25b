"""Prompt-token logprobs on the GPU: the prompt kernel pair (csrc/kernels/logprobs.hip prompt_logprob_scan_kernel /
prompt_logprob_commit_kernel) against float64 -- every element, no tolerated share --, bitwise against the decode pair
(one expression), repeatability, untouched state and refusals; then the runner / engine on the tiny models: alignment of
the list with the rows the engine scored, every route a prompt takes, and an engine in which nobody asks."""
import collections
import dataclasses

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON = -777.25
KMAX = 20


def _distinct(V, sigma, gen):
    """V distinct f32 values ~ N(0, sigma^2) in random order."""
    x = torch.unique(torch.randn(V + V // 4 + 64, generator=gen) * sigma)
    assert x.numel() >= V
    return x[torch.randperm(x.numel(), generator=gen)[:V]].contiguous()


def _rows(R, V, seed):
    """Row r is of kind r % 5: N(0, 1) | N(0, 144) | largest logit at V - 1 | all equal | a tie of the two largest
    across the 2048 boundary (V <= 2048: across the middle), the lower index first."""
    gen = torch.Generator().manual_seed(seed)
    out = torch.empty(R, V)
    for r in range(R):
        kind = r % 5
        x = _distinct(V, 12.0 if kind == 1 else 1.0, gen)
        if kind == 2:
            x[V - 1] = float(x.max()) + 9.0
        elif kind == 3:
            x[:] = 0.75
        elif kind == 4 and V >= 4:
            i, j = (2047, 2048) if V > 2048 else (V // 2 - 1, V // 2)
            x[i] = x[j] = float(x.max()) + 0.5
        out[r] = x
    return out


def _targets(R, V, seed):
    """Targets at 0, 2047, 2048 and V - 1 (where they exist), random ids, and every fourth row (1, 5, 9, ...) without a
    target -- interleaved with rows that have one."""
    gen = torch.Generator().manual_seed(seed)
    fixed = [t for t in (0, 2047, 2048, V - 1) if t < V]
    out = []
    for r in range(R):
        if r % 4 == 1 and R > 1:
            out.append(-1)
        elif r < 2 * len(fixed):
            out.append(fixed[r // 2 % len(fixed)] if r % 2 == 0 else fixed[(r // 2 + 1) % len(fixed)])
        else:
            out.append(int(torch.randint(V, (1,), generator=gen)))
    if R == 1:
        out[0] = fixed[-1]
    return torch.tensor(out, dtype=torch.int32)


def _dst(R, dev, K=KMAX):
    return (torch.full((R,), POISON, device=dev), torch.full((R, K), -9, dtype=torch.int32, device=dev),
            torch.full((R, K), POISON, device=dev))


def _pair(dl, targets, row_k, dev, any_k, K=KMAX, ws=None):
    R, V = dl.shape
    ws = ws or ops.prompt_logprob_workspace(R, V, dev)
    dst = _dst(R, dev, K)
    t, k = targets.to(dev), row_k.to(dev)
    ops.prompt_logprob_scan(dl, t, k, workspace=ws, any_k=any_k)
    ops.prompt_logprob_commit(dl, t, k, *dst, workspace=ws, any_k=any_k)
    torch.cuda.synchronize()
    return [x.cpu() for x in dst]


_REF: dict = {}


def _reference(V, R):
    """Rows, targets, float64 lse and the stable descending order of a case: computed once, shared, never modified."""
    if (V, R) not in _REF:
        lg = _rows(R, V, seed=2000 + V + R)
        _REF[(V, R)] = (lg, _targets(R, V, seed=V + R), torch.logsumexp(lg.double(), dim=-1),
                        torch.sort(lg, dim=-1, descending=True, stable=True).indices[:, :KMAX])
    return _REF[(V, R)]


def _check(got, lg, tg, lse, order, ks, tag):
    """Every chosen value and every top-K value within 8 * 2^-24 * (1 + |lse| + |l|) of float64; ids exact; words past K
    and rows without a target at their sentinels."""
    got_tok, got_ids, got_top = got
    R, V = lg.shape
    d = lg.double()
    worst = 0.0
    for r in range(R):
        t, k = int(tg[r]), int(ks[r])
        if t < 0:
            assert got_tok[r] == POISON and torch.all(got_ids[r] == -9) and torch.all(got_top[r] == POISON), (tag, r)
            continue
        kk = min(k, V)
        assert got_ids[r, :kk].tolist() == order[r, :kk].tolist(), (tag, r)
        for j in range(kk, k):  # entries beyond V
            assert int(got_ids[r, j]) == -1 and float(got_top[r, j]) == float("-inf")
        assert torch.all(got_ids[r, k:] == -9) and torch.all(got_top[r, k:] == POISON), (tag, r)
        pairs = [(t, float(got_tok[r]))] + [(int(i), float(v)) for i, v in zip(order[r, :kk], got_top[r, :kk])]
        for i, v in pairs:
            l = float(d[r, i])
            unit = U * (1.0 + abs(float(lse[r])) + abs(l))
            err = abs(v - (l - float(lse[r])))
            worst = max(worst, err / unit)
            assert err <= 8 * unit, (tag, r, i, v, l - float(lse[r]), err / unit)
        hit = (order[r, :kk] == t).nonzero().flatten()
        if hit.numel():  # bitwise: one expression for the chosen token and its top-K entry
            assert got_top[r, int(hit[0])].view(torch.int32) == got_tok[r].view(torch.int32), (tag, r)
        if r % 5 == 4 and V >= 4 and k >= 2:  # the planted tie across the chunk boundary: the lower index first
            i, j = (2047, 2048) if V > 2048 else (V // 2 - 1, V // 2)
            assert got_ids[r, :2].tolist() == [i, j] and got_top[r, 0] == got_top[r, 1], (tag, r)
    print(f"{tag}: worst |err| / (2^-24 (1 + |lse| + |l|)) = {worst:.3f}")
    return worst


# V: 50 one partial chunk; 2049 odd (the unaligned path, one element in the second chunk); 5000; 128,256 (63 chunks)
CASES = [(50, 1), (50, 5), (2049, 5), (2049, 70), (5000, 1), (5000, 70), (128256, 3)]


@pytest.mark.parametrize("V,R", CASES)
def test_exact_against_float64(gpu, V, R):
    lg, tg, lse, order = _reference(V, R)
    dl = lg.to(gpu)
    mixed = torch.tensor([(0, 1, 5, 20)[r % 4] for r in range(R)], dtype=torch.int32)
    for name, ks, any_k in (("mixed", mixed, True), ("K=20", torch.full((R,), 20, dtype=torch.int32), True),
                            ("K=1", torch.ones(R, dtype=torch.int32), True),
                            ("K=0, some-row form", torch.zeros(R, dtype=torch.int32), True),
                            ("K=0, no-row form", torch.zeros(R, dtype=torch.int32), False)):
        got = _pair(dl, tg, ks, gpu, any_k)
        _check(got, lg, tg, lse, order, ks, f"V={V} R={R} {name}")
        assert torch.equal(dl.cpu(), lg)  # logits bitwise unchanged after both launches
    # the no-row form ignores a K the host mis-stated: chosen values only, no top word written
    got = _pair(dl, tg, mixed, gpu, False)
    _check(got, lg, tg, lse, order, torch.zeros(R, dtype=torch.int32), f"V={V} R={R} no-row form, K stated")
    # a narrower record (kcap = 4) caps K
    got = _pair(dl, tg, mixed, gpu, True, K=4)
    _check(got, lg, tg, lse, order, mixed.clamp(max=4), f"V={V} R={R} kcap=4")


@pytest.mark.parametrize("K", [0, 20])
@pytest.mark.parametrize("B", [5, 32])
def test_one_expression_with_the_decode_pair(gpu, K, B):
    """The same rows and tokens through the plain logprob_scan / logprob_commit pair: lp_tok, ids and top bitwise equal."""
    V, max_new, n0 = 5000, 4, 2
    lg, tg, _, _ = _reference(V, 70)
    lg = lg[:B].contiguous()
    tok = tg[:B].clone()
    tok[tok < 0] = 17  # (the decode pair has no row without a token)
    dl = lg.to(gpu)
    i32 = dict(dtype=torch.int32, device=gpu)
    f32 = dict(dtype=torch.float32, device=gpu)
    lp_k, lp_n0 = torch.full((B,), K, **i32), torch.full((B,), -1, **i32)
    gen_len, fin = torch.full((B,), n0, **i32), torch.zeros(B, **i32)
    out_tokens = torch.zeros(B, max_new, **i32)
    lp_tok, lp_ids = torch.full((B, max_new), POISON, **f32), torch.full((B, max_new, KMAX), -9, **i32)
    lp_top, lp_raw = torch.full((B, max_new, KMAX), POISON, **f32), torch.full((B, V), POISON, **f32)
    ws = ops.logprob_workspace(B, V, gpu)
    ops.logprob_scan(dl, lp_k, fin, gen_len, lp_raw, lp_n0, workspace=ws)
    out_tokens[:, n0] = tok.to(gpu)
    gen_len.fill_(n0 + 1)
    ops.logprob_commit(lp_raw, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, B, workspace=ws)
    for any_k in ((True, False) if K == 0 else (True,)):
        got = _pair(dl, tok, torch.full((B,), K, dtype=torch.int32), gpu, any_k)
        assert torch.equal(got[0].view(torch.int32), lp_tok[:, n0].cpu().view(torch.int32))
        assert torch.equal(got[1], lp_ids[:, n0].cpu())
        assert torch.equal(got[2].view(torch.int32), lp_top[:, n0].cpu().view(torch.int32))


def test_repeatability_and_row_independence(gpu):
    """Two launches give bitwise equal results; a row's record depends neither on its neighbours nor on R."""
    V = 5000
    lg, tg, _, _ = _reference(V, 70)
    dl = lg.to(gpu)
    ks = torch.tensor([(0, 1, 5, 20)[r % 4] for r in range(70)], dtype=torch.int32)
    a, b = _pair(dl, tg, ks, gpu, True), _pair(dl, tg, ks, gpu, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a workspace that held another launch's partials, rows in another order
    ws = ops.prompt_logprob_workspace(70, V, gpu)
    _pair(dl.flip(0).contiguous(), tg.flip(0), ks.flip(0), gpu, True, ws=ws)
    c = _pair(dl, tg, ks, gpu, True, ws=ws)
    for x, y in zip(a, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for r in (0, 3, 4, 13, 34, 69):  # alone at R = 1, and inside R = 5 at another place
        solo = _pair(dl[r:r + 1].contiguous(), tg[r:r + 1], ks[r:r + 1], gpu, True)
        sel = torch.tensor([2, r, 7, 8, 11])
        five = _pair(dl[sel.to(gpu)].contiguous(), tg[sel], ks[sel], gpu, True)
        for x, y, z in zip(solo, a, five):
            assert torch.equal(x[0].view(torch.int32), y[r].view(torch.int32)), r
            assert torch.equal(z[1].view(torch.int32), y[r].view(torch.int32)), r
    # the chosen value does not depend on the launch form
    z = _pair(dl, tg, torch.zeros(70, dtype=torch.int32), gpu, False)
    assert torch.equal(z[0].view(torch.int32), a[0].view(torch.int32))


def test_refusals_before_any_launch(gpu):
    R, V = 2, 64
    lg = torch.randn(R, V, device=gpu)
    t = torch.tensor([3, 5], dtype=torch.int32, device=gpu)
    k = torch.tensor([2, 2], dtype=torch.int32, device=gpu)
    ws = ops.prompt_logprob_workspace(R, V, gpu)
    dst = _dst(R, gpu)
    ext = ops.ext()

    def scan(**kw):
        a = dict(logits=lg, targets=t, row_k=k, any_k=True, ms=ws[0], cand=ws[1])
        a.update(kw)
        ext.prompt_logprob_scan(**a)

    def commit(**kw):
        a = dict(logits=lg, ms=ws[0], cand=ws[1], targets=t, row_k=k, any_k=True, dst_tok=dst[0], dst_ids=dst[1],
                 dst_top=dst[2])
        a.update(kw)
        ext.prompt_logprob_commit(**a)

    big = torch.zeros(1, 262145, device=gpu)
    bad_scan = [dict(logits=lg.double()), dict(logits=lg.t().contiguous().t()), dict(logits=lg[0]), dict(ms=ws[0][:3]),
                dict(cand=ws[1][:5]), dict(targets=t.long()), dict(targets=t[:1]), dict(row_k=k[:1]),
                dict(logits=big, targets=t[:1], row_k=k[:1]),
                dict(logits=lg[:0], targets=t[:0], row_k=k[:0])]
    bad_commit = [dict(dst_ids=torch.zeros(R, 21, dtype=torch.int32, device=gpu), dst_top=torch.zeros(R, 21, device=gpu)),
                  dict(dst_tok=torch.zeros(3, device=gpu)), dict(dst_tok=dst[0].double()),
                  dict(dst_ids=torch.zeros(3, KMAX, dtype=torch.int32, device=gpu),
                       dst_top=torch.zeros(3, KMAX, device=gpu)),
                  dict(dst_top=dst[2].double()), dict(dst_ids=dst[1].t().contiguous().t()), dict(cand=ws[1][:5]),
                  dict(logits=big, targets=t[:1], row_k=k[:1])]
    for kw in bad_scan:
        with pytest.raises(RuntimeError):
            scan(**kw)
    for kw in bad_commit:
        with pytest.raises(RuntimeError):
            commit(**kw)
    with pytest.raises(ValueError):  # the ops layer refuses the same before the binding
        ops.prompt_logprob_commit(lg, t, k, dst[0], torch.zeros(R, 21, dtype=torch.int32, device=gpu),
                                  torch.zeros(R, 21, device=gpu), workspace=ws)
    with pytest.raises(ValueError):
        ops.prompt_logprob_scan(lg, t, k)  # no workspace
    with pytest.raises(ValueError):
        ops.prompt_logprob_scan(lg, t, k, workspace=ops.prompt_logprob_workspace(1, V, gpu))  # too small
    with pytest.raises(ValueError):
        ops.prompt_logprob_scan(lg.double(), t, k, workspace=ws)
    with pytest.raises(ValueError):
        ops.prompt_logprob_scan(big, t[:1], k[:1], workspace=ws)
    torch.cuda.synchronize()
    for x in dst:
        assert torch.all(x.cpu() == (POISON if x.dtype == torch.float32 else -9))  # nothing was launched


# ------------------------------------------------------------------------------------------- runner and engine
def _prompt(n, k=0, mod=500):
    return [1] + [5 + (7 * i + 13 * k) % mod for i in range(n - 1)]


def _gen(e, prompts, sps):
    reqs = [e.add_request(p, sp) for p, sp in zip(prompts, sps)]
    e.run_until_done(reqs)
    return [e.result(q) for q in reqs]


class Spy:
    """Keeps the rows the engine actually scored, in scoring order, as ``_prompt_logprob_scan`` was given them."""

    def __init__(self, eng):
        self.eng, self.rows, self.targets, self.calls = eng, [], [], []

    def __enter__(self):
        scan = self.eng.runner._prompt_logprob_scan

        def spy(logits, targets, row_k, *a, **kw):
            self.rows.append(logits.clone())
            self.targets.append(targets.clone())
            self.calls.append(logits.shape[0])
            scan(logits, targets, row_k, *a, **kw)

        self.eng.runner._prompt_logprob_scan = spy
        return self

    def __exit__(self, *exc):
        del self.eng.runner._prompt_logprob_scan


def _check_entries(eng, res, prompt, lo, rows, targets, top=True):
    """Entry j == rows[j - 1][prompt[j]] - lse in float64 over the scored rows, under the kernels' bound; top_logprobs[0]
    is that row's argmax.  ``rows`` / ``targets``: the scored rows of prompt indices lo .. len(prompt) - 1, in order."""
    assert len(res.prompt_logprobs) == res.prompt_tokens == len(prompt)
    assert [x is None for x in res.prompt_logprobs] == [j < lo for j in range(len(prompt))]
    assert targets.tolist() == prompt[lo:] and rows.shape[0] == len(prompt) - lo
    d = rows.double().cpu()
    lse = torch.logsumexp(d, dim=-1)
    worst = 0.0
    for j in range(lo, len(prompt)):
        ent, r = res.prompt_logprobs[j], j - lo
        l = float(d[r, prompt[j]])
        unit = U * (1 + abs(float(lse[r])) + abs(l))
        err = abs(ent["logprob"] - (l - float(lse[r])))
        worst = max(worst, err / unit)
        assert err <= 8 * unit, (j, ent["logprob"], l - float(lse[r]), err / unit)
        assert ent["token"] == eng.tok.decode([prompt[j]])
        if top:
            best = int(torch.sort(rows[r].cpu(), descending=True, stable=True).indices[0])
            assert ent["top_logprobs"][0]["token"] == eng.tok.decode([best]), j
            lb = float(d[r, best])
            assert abs(ent["top_logprobs"][0]["logprob"] - (lb - float(lse[r]))) <= 8 * U * (1 + abs(float(lse[r])) + abs(lb))
    print(f"worst |err| / unit over {len(prompt) - lo} entries: {worst:.3f}")


ENGINE_CASES = [
    # model, engine kwargs, score_tile_rows, prompt length, from, expected scan calls (rows per tile)
    ("tiny-nsql", {}, 256, 30, 0, [29]),                       # skinny lm_head
    ("tiny-nsql", {}, 256, 150, 0, [149]),                     # more than 64 scored rows: the stream-K kernel
    ("tiny-nsql", {}, 64, 150, 0, [64, 64, 21]),               # the same in 64-row tiles
    ("tiny-llama3", {}, 256, 150, 70, [80]),                   # from the middle
    ("tiny-llama3", dict(prefill_chunk=64), 256, 150, 0, [64, 64, 21]),   # chunks: each call scores the rows it holds
    ("tiny-llama3", dict(prefill_chunk=64), 64, 150, 100, [29, 21]),      # a chunk seam inside the scored range
    ("tiny-llama3", dict(dtype="fp8"), 256, 150, 0, [149]),    # fp8 weights: another lm_head kernel at M > 64
    ("tiny-llama3", dict(dtype="fp8"), 256, 30, 0, [29]),
    # MXFP4 weights: tiles above 64 rows multiply by the lm_head dequantised once for the call, the last tile is skinny
    ("tiny-nsql", dict(dtype="mxfp4", seed=1), 70, 150, 0, [70, 70, 9]),
]


@pytest.mark.parametrize("model,kw,tile,n,lo,calls", ENGINE_CASES)
def test_engine_alignment_and_exactness(gpu, model, kw, tile, n, lo, calls):
    eng = build_engine(model, device=str(gpu), max_slots=4, max_model_len=512, logprobs=True, **kw)
    eng.runner.score_tile_rows = tile
    p = _prompt(n)
    sp = SamplingParams(max_tokens=2, ignore_eos=True, prompt_logprobs=True, prompt_logprobs_from=lo, top_logprobs=2)
    deq, dq = [], ops._dequant_scratch
    ops._dequant_scratch = lambda w, dev: (deq.append(w is eng.runner.w.lm_head), dq(w, dev))[1]
    try:
        with Spy(eng) as spy:
            res = _gen(eng, [p], [sp])[0]
    finally:
        ops._dequant_scratch = dq
    assert spy.calls == calls
    assert sum(deq) <= 1  # a quantised lm_head is dequantised at most once for all the tiles of a call
    if kw.get("dtype") == "mxfp4":
        assert sum(deq) == 1
    _check_entries(eng, res, p, max(1, lo), torch.cat(spy.rows), torch.cat(spy.targets))
    assert eng.stats["prompt_logprob_rows"] == n - max(1, lo) and eng.stats["prompt_logprob_requests"] == 1
    nch = -(-eng.runner.V // 2048)
    assert eng.runner.prompt_lp_ws[0].numel() == min(tile, max(calls)) * nch * 2  # the tile workspace, accounted for
    assert eng.runner.logprobs_bytes() >= sum(t.numel() * t.element_size() for t in eng.runner.prompt_lp_ws)


@pytest.fixture(scope="module")
def engines(gpu):
    kw = dict(device=str(gpu), max_slots=4, max_model_len=512)
    return build_engine("tiny-nsql", logprobs=True, guided=True, **kw), build_engine("tiny-nsql", guided=True, **kw)


def test_engine_two_sequences_packed_one_asks(engines):
    eng, _ = engines
    ps = [_prompt(30, 1), _prompt(150, 2)]
    free = SamplingParams(max_tokens=2, ignore_eos=True)
    ask = SamplingParams(max_tokens=2, ignore_eos=True, prompt_logprobs=True, prompt_logprobs_from=40, top_logprobs=3)
    with Spy(eng) as spy:
        got = _gen(eng, ps, [free, ask])
    assert spy.calls == [110] and got[0].prompt_logprobs is None
    _check_entries(eng, got[1], ps[1], 40, torch.cat(spy.rows), torch.cat(spy.targets))
    with Spy(eng) as spy:  # both ask, with their own K and from: the rows of each land in its own list
        both = _gen(eng, ps, [dataclasses.replace(ask, prompt_logprobs_from=0, top_logprobs=1), ask])
    rows, tg = torch.cat(spy.rows), torch.cat(spy.targets)
    assert rows.shape[0] == 29 + 110
    _check_entries(eng, both[0], ps[0], 1, rows[:29], tg[:29])
    _check_entries(eng, both[1], ps[1], 40, rows[29:], tg[29:])
    assert len(both[0].prompt_logprobs[3]["top_logprobs"]) == 1 and len(both[1].prompt_logprobs[50]["top_logprobs"]) == 3
    assert [r.token_ids for r in both] == [r.token_ids for r in got]


class OpCounter:
    """Profiler-free launch counter: every call the runner makes into ``ops`` while it is inside ``_prefill``."""

    def __init__(self, runner):
        self.runner, self.names, self.on = runner, [], False

    def __enter__(self):
        self.saved = {}
        for name in dir(ops):
            f = getattr(ops, name)
            if name.startswith("_") or not callable(f) or isinstance(f, type) or getattr(f, "__module__", "") != ops.__name__:
                continue
            self.saved[name] = f
            setattr(ops, name, self._wrap(name, f))
        pre = self.runner._prefill

        def prefill(*a, **kw):
            self.on = True
            try:
                return pre(*a, **kw)
            finally:
                self.on = False

        self.runner._prefill = prefill
        return self

    def _wrap(self, name, f):
        def g(*a, **kw):
            if self.on:
                self.names.append(name)
            return f(*a, **kw)
        return g

    def __exit__(self, *exc):
        for name, f in self.saved.items():
            setattr(ops, name, f)
        del self.runner._prefill


def test_nobody_asks(engines):
    """Tokens, graph keys and count_step_kernels are those of an engine without the feature in use; a prefill in which
    nobody asks makes the calls it makes on an engine that never scored, and asking adds exactly the tiles' launches."""
    eng, plain = engines
    ps = [_prompt(30, 3), _prompt(150, 4)]
    free = SamplingParams(max_tokens=12)
    with OpCounter(eng.runner) as before:
        a = _gen(eng, ps, [free, free])
    b = _gen(plain, ps, [free, free])
    assert [r.token_ids for r in a] == [r.token_ids for r in b] and all(r.prompt_logprobs is None for r in a)
    keys = {k for k in plain.runner.graphs}
    assert keys and {k for k in eng.runner.graphs if len(k) == 3} >= keys
    for B in (1, 4):
        assert eng.runner.count_step_kernels(B) == plain.runner.count_step_kernels(B)
        assert eng.runner.count_step_kernels(B, sample=True) == plain.runner.count_step_kernels(B, True)
    graphs = set(eng.runner.graphs)
    ask = SamplingParams(max_tokens=12, prompt_logprobs=True, top_logprobs=2)
    with OpCounter(eng.runner) as asked:
        c = _gen(eng, ps, [free, ask])
    assert [r.token_ids for r in c] == [r.token_ids for r in b]
    assert set(eng.runner.graphs) == graphs  # scoring is prefill work: no graph, no key
    with OpCounter(eng.runner) as after:
        d = _gen(eng, ps, [free, free])
    assert [r.token_ids for r in d] == [r.token_ids for r in b]
    # not asking adds zero launches, before and after a prefill that scored; asking adds one lm_head GEMM, one scan and
    # one commit per tile (149 rows: one tile) -- the final norm gathers the scored rows in the launch it has, and no
    # layer op is called once more
    assert before.names == after.names and not any(n.startswith("prompt_logprob") for n in before.names)
    extra = collections.Counter(asked.names) - collections.Counter(before.names)
    assert not collections.Counter(before.names) - collections.Counter(asked.names)
    assert extra["linear"] == 1 and extra["prompt_logprob_scan"] == 1 and extra["prompt_logprob_commit"] == 1
    helpers = {"gemm_sk", "sk_config", "ext", "pick_gemm_config", "tile_splitk", "logprob_workspace",
               "prompt_logprob_workspace", "tile_weight"}  # what ops.linear, the workspace and the tile loop call inside
    # ops with no launch of their own (tile_weight of a bf16 weight is the weight itself)
    assert set(extra) <= {"linear", "prompt_logprob_scan", "prompt_logprob_commit"} | helpers, extra


def test_asking_does_not_change_generated_tokens(engines):
    """A mixed batch of greedy, sampled and regex-constrained requests, all asking (one also for generated-token
    logprobs): the tokens are those of the engine without the feature."""
    eng, plain = engines
    ps = [_prompt(40, 5), _prompt(90, 6), _prompt(33, 7), _prompt(70, 8)]
    sps = [SamplingParams(max_tokens=16, ignore_eos=True),
           SamplingParams(max_tokens=16, ignore_eos=True, temperature=0.8, seed=5, repeat_penalty=1.3),
           SamplingParams(max_tokens=16, regex=r"(ab|c)+;"),
           SamplingParams(max_tokens=16, ignore_eos=True, temperature=0.6, seed=9, min_p=0.05)]
    want = _gen(plain, ps, sps)
    on = [dataclasses.replace(s, prompt_logprobs=True, top_logprobs=(0, 20, 3, 1)[i], logprobs=(i == 1),
                              prompt_logprobs_from=(0, 10, 0, 69)[i]) for i, s in enumerate(sps)]
    with Spy(eng) as spy:
        got = _gen(eng, ps, on)
    assert [r.token_ids for r in got] == [r.token_ids for r in want]
    rows, tg = torch.cat(spy.rows), torch.cat(spy.targets)
    o = 0
    for i, (r, p) in enumerate(zip(got, ps)):
        lo = max(1, on[i].prompt_logprobs_from)
        n = len(p) - lo
        _check_entries(eng, r, p, lo, rows[o:o + n], tg[o:o + n], top=on[i].top_logprobs > 0)
        o += n
    assert o == rows.shape[0]
    assert len(got[1].logprobs) == got[1].eval_count and got[0].logprobs is None
    assert "top_logprobs" not in got[0].prompt_logprobs[1] and len(got[1].prompt_logprobs[10]["top_logprobs"]) == 20


def test_prefix_cache_two_completions(gpu):
    """The same prompt with two completions, one after the other: the second is served the prompt's blocks up to the
    first scored row, and every completion token has an entry that obeys the bound over the rows scored."""
    eng = build_engine("tiny-llama3", device=str(gpu), max_slots=4, max_model_len=512, logprobs=True, prefix_cache=True)
    base = _prompt(100, 9, mod=600)
    comps = [[7 + (11 * i) % 600 for i in range(20)], [9 + (17 * i) % 600 for i in range(33)]]
    out = []
    for c in comps:
        sp = SamplingParams(max_tokens=1, prompt_logprobs=True, prompt_logprobs_from=len(base), top_logprobs=2)
        with Spy(eng) as spy:
            res = _gen(eng, [base + c], [sp])[0]
        _check_entries(eng, res, base + c, len(base), torch.cat(spy.rows), torch.cat(spy.targets))
        assert sum(x is not None for x in res.prompt_logprobs) == len(c)
        out.append(res)
    assert out[0].cached_prompt_tokens == 0
    assert 64 <= out[1].cached_prompt_tokens <= len(base) - 1
    # a request that does not ask still takes everything the cache holds of its prompt
    free = _gen(eng, [base + comps[1]], [SamplingParams(max_tokens=1)])[0]
    assert free.cached_prompt_tokens >= 128 and free.prompt_logprobs is None
