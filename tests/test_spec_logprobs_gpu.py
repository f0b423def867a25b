"""Per-token logprobs for speculating requests on the GPU (``spec_logprobs``): the verify-step pair of
csrc/kernels/logprobs.hip against float64 and the host twin, bitwise against the plain pair, the raw rule through the
real mask and sampled commit, refusals, graph replay, and the engine with captured graphs on the tiny model."""
import json
import os

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.guided import MAX_TABLE, compile_regex
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_logprobs_gpu import KMAX, POISON, U, Bufs, _rows
from test_spec_cpu import K, forced_table
from test_spec_logprobs_cpu import refusals

pytestmark = pytest.mark.gpu

I32 = dict(dtype=torch.int32)
RATIOS: dict = {}  # case -> worst |err| / (2^-24 (1 + |lse| + |l|)); merged into LSA_LOGPROBS_EXACT_OUT when it is set
SHAPES = [(1, 2), (1, 8), (2, 4), (4, 8), (8, 4)]
KS = (20, 0, 5, -1, 1, 20, 3, 0)  # lp_k of sequence s


class SpecBufs:
    """Decode state of S sequences, poisoned per-slot records and the spec-side workspace."""

    def __init__(self, S, T, V, max_new, dev, kcap=KMAX):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        R = S
        self.S, self.T, self.V, self.dev = S, T, V, dev
        self.out_tokens = torch.full((R, max_new), -3, **i32)
        self.gen_len = torch.zeros(S, **i32)
        self.input_ids = torch.zeros(S, **i32)
        self.positions = torch.full((S,), 7, **i32)
        self.finished = torch.zeros(S, **i32)
        self.limit = torch.full((S,), max_new, **i32)
        self.eos_on = torch.ones(S, **i32)
        self.eos = torch.tensor([-1], **i32)
        self.lp_k = torch.full((S,), -1, **i32)
        self.lp_n0 = torch.full((S,), -1, **i32)
        self.lp_tok = torch.full((R, max_new), POISON, **f32)
        self.lp_ids = torch.full((R, max_new, kcap), -9, **i32)
        self.lp_top = torch.full((R, max_new, kcap), POISON, **f32)
        self.ws = ops.spec_logprob_workspace(V, dev)
        self.ws[0].fill_(POISON)
        self.stats = torch.zeros(S, 3, dtype=torch.int64, device=dev)

    def scan(self, logits):
        ops.spec_logprob_scan(logits, self.T, self.lp_k, self.finished, self.gen_len, self.lp_n0, self.ws)

    def lp_commit(self):
        ops.spec_logprob_commit(self.T, self.lp_k, self.lp_n0, self.gen_len, self.out_tokens, self.lp_tok, self.lp_ids,
                                self.lp_top, self.ws)

    def greedy(self, logits, draft):
        ops.spec_commit(logits, draft, self.stats if self.S > 1 else self.stats[0], self.out_tokens, self.gen_len,
                        self.input_ids, self.positions, self.finished, self.eos, self.limit, self.eos_on)

    def state(self):
        return [t.clone() for t in (self.out_tokens, self.gen_len, self.input_ids, self.positions, self.finished,
                                    self.lp_n0)]

    def records(self):
        return [t.clone() for t in (self.lp_tok, self.lp_ids, self.lp_top)]


def hand_commit(S, T, V, lg, seed):
    """A different c per sequence, n0 per sequence, and tokens set by hand: the raw top-1, the runner-up or any id."""
    cs = [(T, 1, 0, T - 1, 2 % (T + 1), T, 1, T // 2)[s] for s in range(S)]
    n0s = [s % 3 for s in range(S)]
    order = torch.sort(lg, dim=-1, descending=True, stable=True).indices
    gen = torch.Generator().manual_seed(seed)
    tok = torch.tensor([int(order[r, 0]) if r % 3 == 0 else int(order[r, min(1, V - 1)]) if r % 3 == 1
                        else int(torch.randint(V, (1,), generator=gen)) for r in range(S * T)], **I32)
    return cs, n0s, tok


def run_hand(S, T, V, lg, dev, ks, cs, n0s, tok, max_new):
    bf = SpecBufs(S, T, V, max_new, dev)
    bf.lp_k.copy_(torch.tensor(ks[:S], **I32))
    bf.gen_len.copy_(torch.tensor(n0s, **I32))
    dl = lg.to(dev)
    bf.scan(dl)
    for s in range(S):
        for t in range(cs[s]):
            bf.out_tokens[s, n0s[s] + t] = int(tok[s * T + t])
    bf.gen_len.copy_(torch.tensor([n + c for n, c in zip(n0s, cs)], **I32))
    bf.lp_commit()
    torch.cuda.synchronize()
    assert torch.equal(dl.cpu(), lg)
    return bf


EXACT = [(V, S, T) for V in (50, 2049, 5000) for S, T in SHAPES] + [(128256, 1, 4), (10, 1, 2)]


@pytest.mark.parametrize("V,S,T", EXACT)
def test_exact_against_float64(gpu, V, S, T):
    """|err| <= 8 * 2^-24 * (1 + |lse| + |l|) for every recorded value, lse and l from float64; ids equal the twin's;
    the chosen token's value is bitwise its top-K entry; entries beyond V are id -1 / -inf; the rest is poison."""
    max_new = 2 + T
    lg = _rows(S * T, V, seed=2000 + V + 10 * S + T)
    cs, n0s, tok = hand_commit(S, T, V, lg, V + S)
    assert S == 1 or len(set(cs)) > 1
    bf = run_hand(S, T, V, lg, gpu, KS, cs, n0s, tok, max_new)
    got_tok, got_ids, got_top = bf.lp_tok.cpu(), bf.lp_ids.cpu(), bf.lp_top.cpu()
    touched = torch.zeros(S, max_new, dtype=torch.bool)
    d = lg.double()
    lse = torch.logsumexp(d, dim=-1)
    worst = 0.0
    for s in range(S):
        k = KS[s]
        assert int(bf.lp_n0[s]) == (n0s[s] if k >= 0 else -1)
        if k < 0:
            continue
        for t in range(cs[s]):
            r, n = s * T + t, n0s[s] + t
            touched[s, n] = True
            assert torch.equal(bf.ws[0][r].cpu(), lg[r])  # the raw copy of a scanned row
            _, ids, _ = ref.logprob_rows(lg[r:r + 1], tok[r:r + 1], k)
            assert torch.equal(got_ids[s, n, :k], ids[0]), (s, t)
            assert torch.all(got_ids[s, n, k:] == -9) and torch.all(got_top[s, n, k:] == POISON)
            pairs = [(int(tok[r]), float(got_tok[s, n]))]
            pairs += [(int(i), float(v)) for i, v in zip(ids[0], got_top[s, n, :k]) if int(i) >= 0]
            for i, v in pairs:
                l = float(d[r, i])
                unit = U * (1.0 + abs(float(lse[r])) + abs(l))
                err = abs(v - (l - float(lse[r])))
                worst = max(worst, err / unit)
                assert err <= 8 * unit, (s, t, i, v, l - float(lse[r]), err / unit)
            for j in range(min(k, V), k):
                assert int(got_ids[s, n, j]) == -1 and float(got_top[s, n, j]) == float("-inf")
            hit = (ids[0] == tok[r]).nonzero().flatten()
            if hit.numel():
                assert got_top[s, n, int(hit[0])].view(torch.int32) == got_tok[s, n].view(torch.int32)
    assert touched.any()
    assert torch.all(got_tok[~touched] == POISON) and torch.all(got_top[~touched] == POISON)
    assert torch.all(got_ids[~touched] == -9)
    RATIOS[f"spec V={V},S={S},T={T}"] = round(worst, 4)
    print(f"worst |err| / unit at V={V} S={S} T={T}: {worst:.3f}")
    out = os.environ.get("LSA_LOGPROBS_EXACT_OUT")
    if out:
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc.setdefault("unit", "2^-24 * (1 + |lse| + |l|), lse and l in float64")
        doc.setdefault("bound", 8)
        doc.setdefault("spec_worst_ratio", {}).update(RATIOS)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


@pytest.mark.parametrize("V", [2049, 5000])
@pytest.mark.parametrize("S,T", SHAPES)
def test_bitwise_against_the_plain_kernels(gpu, V, S, T):
    """Every record equals, bit for bit, what logprob_scan + logprob_commit at B = S * T record for the same row values
    and token; each sequence's records equal its own one-sequence launch; a repeat is bitwise."""
    max_new = 2 + T
    lg = _rows(S * T, V, seed=3000 + V + 10 * S + T)
    cs, n0s, tok = hand_commit(S, T, V, lg, 2 * V + S)
    a = run_hand(S, T, V, lg, gpu, KS, cs, n0s, tok, max_new)
    b = run_hand(S, T, V, lg, gpu, KS, cs, n0s, tok, max_new)
    for x, y in zip(a.records() + a.state(), b.records() + b.state()):
        assert torch.equal(x, y)
    # the plain pair over the S * T rows: row r = s T + t records index n0[s] + t of its own record row
    B = S * T
    pl = Bufs(B, V, max_new, gpu)
    pl.lp_k.copy_(torch.tensor([KS[r // T] for r in range(B)], **I32))
    idx = [n0s[r // T] + r % T for r in range(B)]
    pl.gen_len.copy_(torch.tensor(idx, **I32))
    pl.scan(lg.to(gpu))
    for r in range(B):
        pl.out_tokens[r, idx[r]] = int(tok[r])
    pl.gen_len.add_(1)
    pl.lp_commit()
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32)  # noqa: E731
    n = 0
    for s in range(S):
        for t in range(cs[s] if KS[s] >= 0 else 0):
            r, i = s * T + t, n0s[s] + t
            assert bits(a.lp_tok[s, i]) == bits(pl.lp_tok[r, i]), (s, t)
            assert torch.equal(a.lp_ids[s, i], pl.lp_ids[r, i])
            assert torch.equal(bits(a.lp_top[s, i]), bits(pl.lp_top[r, i]))
            n += 1
    assert n > 0
    for s in range(S):  # the sequence's own one-sequence launch
        one = run_hand(1, T, V, lg[s * T:(s + 1) * T].contiguous(), gpu, KS[s:s + 1], cs[s:s + 1], n0s[s:s + 1],
                       tok[s * T:(s + 1) * T], max_new)
        for x, y in zip(one.records(), a.records()):
            assert torch.equal(bits(x[0]), bits(y[s])), s
        assert int(one.lp_n0[0]) == int(a.lp_n0[s])


def _ab_tables(V, dev):
    """Tokens with even ids spell "a", odd ids "b"; the pattern b+ masks every even id (tests/test_logprobs_gpu.py)."""
    dfa = compile_regex("b+")
    cls = torch.zeros(1, 256, dtype=torch.uint8)
    trans = torch.full((1, MAX_TABLE), -1, dtype=torch.int16)
    accept = torch.zeros(1, MAX_TABLE, dtype=torch.uint8)
    cls[0] = torch.from_numpy(dfa.cls)
    trans[0, : dfa.n_states * dfa.n_classes] = torch.from_numpy(dfa.trans.view("int16"))
    accept[0, : dfa.n_states] = torch.from_numpy(dfa.accept)
    t = dict(off=torch.arange(V + 1, **I32), blob=torch.tensor([ord("a"), ord("b")] * (V // 2), dtype=torch.uint8),
             cls=cls, trans=trans, accept=accept, dim=torch.tensor([[dfa.n_states, dfa.n_classes]], **I32),
             on=torch.ones(1, **I32), base=torch.zeros(1, **I32))
    return {k: v.to(dev) for k, v in t.items()}, dfa.start


def _tail(dev, lg, draft, V, T, max_new, with_lp=True):
    """scan -> dfa_mask_verify -> spec_sample_commit (greedy draws, penalised ring) -> dfa_spec_advance -> commit."""
    tb, start = _ab_tables(V, dev)
    bf = SpecBufs(1, T, V, max_new, dev)
    bf.lp_k.fill_(3)
    dl = lg.clone().to(dev)
    g_state = torch.tensor([[start, start]], **I32).to(dev)
    g_spec = torch.zeros(9, **I32).to(dev)
    hist = torch.full((1, 64), -1, **I32)
    hist[0, :8] = torch.arange(1, 16, 2, **I32)  # the ring holds odd ids 1 .. 15: the penalty lowers them
    hist = hist.to(dev)
    f = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
    dr = torch.tensor(draft, **I32).to(dev)
    if with_lp:
        bf.scan(dl)
    ops.dfa_mask_verify(dl, tb["off"], tb["blob"], tb["cls"], tb["trans"], tb["accept"], tb["dim"], tb["on"], g_state,
                        tb["base"], bf.gen_len, bf.input_ids, bf.finished, bf.eos, dr, g_spec)
    ops.spec_sample_commit(dl, dr, bf.stats[0], hist, f([50.0]), f([0.0]), f([40], torch.int32), f([0.9]),
                           f([1], torch.int64), bf.out_tokens, bf.gen_len, bf.input_ids, bf.positions, bf.finished,
                           bf.eos, bf.limit, bf.eos_on)
    ops.dfa_spec_advance(tb["on"], g_state, g_spec, bf.gen_len, T - 1)
    if with_lp:
        bf.lp_commit()
    if dev != "cpu":
        torch.cuda.synchronize()
    return bf, dl


def test_raw_rule_through_the_real_tail(gpu):
    """The mask removes every row's raw top-1 (an even id) and the penalty its best odd ids, so the committed tokens are
    neither; the records are those of the raw rows all the same, and the masked token is listed first."""
    V, T, max_new = 5000, 4, 8
    lg = _rows(5 * T, V, seed=9)[::5].contiguous()  # N(0, 1) rows
    for t in range(T):
        lg[t, 100 + 2 * t] = float(lg[t].max()) + 6.0       # the raw top-1: even, masked
        lg[t, 1 + 2 * t] = float(lg[t].max()) - 1.0         # the best odd id: in the ring, penalised away
    draft = [9999 % V | 1] * (T - 1)
    for i in range(T - 1):  # the drafts the commit accepts, from the host twins of the same tail
        cpu, _ = _tail("cpu", lg, draft, V, T, max_new, with_lp=False)
        draft[i] = int(cpu.out_tokens[0, i])
    cpu, _ = _tail("cpu", lg, draft, V, T, max_new)
    bf, dl = _tail(gpu, lg, draft, V, T, max_new)
    toks = bf.out_tokens[0, :T].cpu()
    assert int(bf.gen_len[0]) == T and torch.equal(toks, cpu.out_tokens[0, :T])  # every draft accepted: c = T
    assert not torch.equal(dl.cpu(), lg)  # the mask and the penalty did rewrite the logits
    base, _ = _tail(gpu, lg, draft, V, T, max_new, with_lp=False)
    assert torch.equal(base.out_tokens, bf.out_tokens)  # the two launches only read what the tail reads
    for t in range(T):
        top1 = 100 + 2 * t
        assert int(toks[t]) % 2 == 1 and int(toks[t]) != 1 + 2 * t
        chosen, ids, tp = ref.logprob_rows(lg[t:t + 1], toks[t:t + 1], 3)
        assert torch.equal(bf.lp_ids[0, t, :3].cpu(), ids[0]) and int(ids[0, 0]) == top1
        assert torch.equal(cpu.lp_ids[0, t, :3], ids[0])
        lse = float(torch.logsumexp(lg[t].double(), 0))
        for got, i in [(float(bf.lp_tok[0, t]), int(toks[t]))] + [(float(v), int(i)) for v, i in
                                                                   zip(bf.lp_top[0, t, :3], ids[0])]:
            l = float(lg[t, i])
            assert abs(got - (l - lse)) <= 8 * U * (1 + abs(lse) + abs(l))
    assert torch.all(bf.lp_tok[0, T:] == POISON)


def test_refusals_before_any_launch(gpu):
    refusals(gpu)  # the ops layer: ValueError, nothing written
    V, max_new = 64, 6
    ext = ops.ext()

    def fresh(S, T, V=V, kcap=KMAX):
        bf = SpecBufs(S, T, V, max_new, gpu, kcap=kcap)
        bf.lp_k.fill_(2)
        return bf

    def scan(bf, T, **kw):
        a = dict(logits=torch.ones(bf.S * T, bf.V, device=gpu), T=T, lp_k=bf.lp_k, finished=bf.finished,
                 gen_len=bf.gen_len, sp_raw=bf.ws[0], sp_ms=bf.ws[1], sp_cand=bf.ws[2], lp_n0=bf.lp_n0)
        a.update(kw)
        ext.spec_logprob_scan(**a)

    def commit(bf, T, **kw):
        a = dict(T=T, sp_raw=bf.ws[0], sp_ms=bf.ws[1], sp_cand=bf.ws[2], lp_k=bf.lp_k, lp_n0=bf.lp_n0,
                 gen_len=bf.gen_len, out_tokens=bf.out_tokens, lp_tok=bf.lp_tok, lp_ids=bf.lp_ids, lp_top=bf.lp_top)
        a.update(kw)
        ext.spec_logprob_commit(**a)

    def untouched(bf):
        torch.cuda.synchronize()
        z = SpecBufs(bf.S, bf.T, bf.V, max_new, gpu, kcap=bf.lp_ids.shape[2])
        for x, y in zip(bf.records() + [bf.lp_n0, bf.ws[0]], z.records() + [z.lp_n0, z.ws[0]]):
            assert torch.equal(x, y)

    for S, T in ((2, 0), (2, 9), (9, 2), (5, 8)):  # T, S, S * T
        bf = fresh(S, max(T, 1))
        with pytest.raises(RuntimeError):
            scan(bf, T, logits=torch.ones(max(S * T, 1), V, device=gpu))
        with pytest.raises(RuntimeError):
            commit(bf, T)
        untouched(bf)
    bf = fresh(2, 4)
    bad_scan = [dict(logits=torch.ones(8, V, device=gpu).double()), dict(logits=torch.ones(V, 8, device=gpu).t()),
                dict(logits=torch.ones(7, V, device=gpu)), dict(logits=torch.ones(8, V + 1, device=gpu)),
                dict(sp_raw=bf.ws[0][:31]), dict(sp_ms=bf.ws[1][:-1]), dict(sp_cand=bf.ws[2][:-1]),
                dict(sp_cand=bf.ws[2].int()), dict(lp_k=bf.lp_k.long()), dict(finished=bf.finished[:1]),
                dict(lp_n0=bf.lp_n0[:1])]
    bad_commit = [dict(lp_ids=torch.zeros(2, max_new, 21, device=gpu, **I32),
                       lp_top=torch.zeros(2, max_new, 21, device=gpu)),
                  dict(lp_tok=torch.zeros(2, max_new + 1, device=gpu)), dict(lp_top=bf.lp_top.double()),
                  dict(out_tokens=bf.out_tokens[:1]), dict(out_tokens=bf.out_tokens.long()),
                  dict(sp_raw=bf.ws[0][:31]), dict(sp_ms=bf.ws[1][:-1]), dict(gen_len=bf.gen_len[:1])]
    for kw in bad_scan:
        with pytest.raises(RuntimeError):
            scan(bf, 4, **kw)
    for kw in bad_commit:
        with pytest.raises(RuntimeError):
            commit(bf, 4, **kw)
    untouched(bf)
    big = 262145  # V above the sampler's bound
    raw = torch.zeros(32, big, device=gpu)
    ms, cand = ops.logprob_workspace(32, big, gpu)
    one = fresh(1, 2)
    with pytest.raises(RuntimeError):
        scan(one, 2, logits=torch.zeros(2, big, device=gpu), sp_raw=raw, sp_ms=ms, sp_cand=cand)
    with pytest.raises(RuntimeError):
        commit(one, 2, sp_raw=raw, sp_ms=ms, sp_cand=cand)
    untouched(one)
    assert float(raw.abs().sum()) == 0.0


def test_graph_replay_equals_eager(gpu):
    """scan -> spec_commit -> commit, captured once and replayed three times with planted drafts (sequence 0 accepts
    two a step, sequence 1 none): records and state are those of three eager steps."""
    S, T, V, max_new = 2, 4, 5000, 16
    lg = _rows(S * T, V, seed=21)
    top = lg.argmax(-1)
    draft = torch.tensor([int(top[0]), int(top[1]), (int(top[2]) + 2) % V,
                          (int(top[4]) + 2) % V, int(top[5]), int(top[6])], **I32).to(gpu)

    def fresh():
        bf = SpecBufs(S, T, V, max_new, gpu)
        bf.lp_k.copy_(torch.tensor([20, 0], **I32))
        bf.gen_len.copy_(torch.tensor([1, 2], **I32))
        return bf, lg.to(gpu)

    def step(bf, dl):
        bf.scan(dl)
        bf.greedy(dl, draft)
        bf.lp_commit()

    eager, dl = fresh()
    for _ in range(3):
        step(eager, dl)
    cap, dl2 = fresh()
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step(cap, dl2)
    torch.cuda.current_stream(gpu).wait_stream(s)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert eager.gen_len.tolist() == [1 + 3 * 3, 2 + 3 * 1] == cap.gen_len.tolist()
    for x, y in zip(eager.records() + eager.state(), cap.records() + cap.state()):
        assert torch.equal(x, y)
    assert int((eager.lp_tok[0] != POISON).sum()) == 9 and int((eager.lp_tok[1] != POISON).sum()) == 3
    # step j of sequence 0 recorded rows 0 .. 2 at indices 1 + 3 j ..: three copies of three distributions
    assert torch.equal(eager.lp_tok[0, 1:4], eager.lp_tok[0, 4:7])
    assert torch.equal(eager.lp_top[0, 1:4], eager.lp_top[0, 7:10])
    assert eager.lp_n0.tolist() == [7, 4]  # announced by the last step's scan, not consumed


# ------------------------------------------------------------------------------------------- engine, captured graphs
PROMPT = [1] + list(range(40, 70))


def test_engine_with_captured_graphs(gpu):
    kw = dict(device=str(gpu), max_slots=4, max_model_len=512, seed=0, spec_tokens=K)
    eng = build_engine("tiny-nsql", logprobs=True, spec_logprobs=True, **kw)
    r = eng.runner
    free = SamplingParams(max_tokens=24, ignore_eos=True)
    ask = SamplingParams(max_tokens=24, ignore_eos=True, logprobs=True, top_logprobs=5)
    base = eng.generate([PROMPT], free)[0]
    assert eng.stats["spec_steps"] > 0
    spec_keys = {k for k in r.graphs if k[0] == "spec"}
    assert spec_keys and not any("lp" in k for k in r.graphs)  # nobody asked: the verify graphs of today
    # one verify step per engine step, planted drafts (one right, the rest wrong), and the raw rows after every step
    r.set_spec_forced(forced_table(base.token_ids, "first", r.V).to(gpu))
    eng.run_ahead = 1
    q = eng.add_request(PROMPT, ask)
    worst, seen_c = 0.0, set()
    while not q.done.is_set():
        n_before, s_before = len(q.logprobs), q.spec_steps
        eng.step()
        if q.spec_steps == s_before:
            continue
        raw = r.spec_lp_raw().double().cpu()
        n_before = max(n_before, 1)  # (record 0 is the prefill tail's)
        new = q.logprobs[n_before:]
        toks = r.tokens_of(q.slot, len(q.logprobs)) if not q.done.is_set() else q.output_ids[len(q.resumed):]
        seen_c.add(len(new))
        for t, (lpv, tops) in enumerate(new):  # row t of the step is the distribution of its t-th committed token
            lse = float(torch.logsumexp(raw[t], 0))
            for i, v in [(toks[n_before + t], lpv)] + list(tops):
                l = float(raw[t, int(i)])
                unit = U * (1 + abs(lse) + abs(l))
                worst = max(worst, abs(float(v) - (l - lse)) / unit)
                assert abs(float(v) - (l - lse)) <= 8 * unit
            order = torch.sort(raw[t].float(), descending=True, stable=True).indices[:5]
            assert [int(i) for i, _ in tops] == order.tolist()
    print(f"engine records: worst |err| / unit {worst:.3f}, tokens per verify step {sorted(seen_c)}")
    res = eng.result(q)
    assert q.spec_steps > 0 and 2 in seen_c
    assert res.token_ids == base.token_ids  # the scan only reads: the tokens with and without logprobs
    assert len(res.logprobs) == res.eval_count == 24
    lp_keys = {k for k in r.graphs if k[0] == "spec" and k[-1] == "lp"}
    assert lp_keys and {k for k in r.graphs if k[0] == "spec"} - lp_keys >= spec_keys
    assert r.count_verify_kernels(logprobs=True) == r.count_verify_kernels() + 2
