"""Speculative decoding for several concurrent requests of which some need the sampler, on the GPU
(``spec_batch_sampled``): lsa_spec_sample_commit over S sequences pinned, per sequence, to the exact host twin, to the
in-order commit rule and -- bitwise -- to that sequence's own one-sequence launch; its refusals, determinism and graph
replay; and the engine's mixed verify steps through captured graphs: the same tokens whatever is drafted, and every
committed token the twin's draw of its own verify row."""
import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import build_engine
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_batch_cpu import PROMPTS, forced_tables, ids_of
from test_spec_batch_sampled_cpu import GPU_TOKENS, MIXED, ON, UNUSABLE, params, recorded_draws_batch
from test_spec_cpu import K
from test_spec_sampled_gpu import NAMES, Case

pytestmark = pytest.mark.gpu

I32 = dict(dtype=torch.int32)
PAR_SEQ = ("penalty", "temperature", "top_k", "top_p", "seeds", "last_n", "limit", "eos_on")  # one entry per sequence
NPICKS = 40  # the picks buffer of the launches below: entries beyond S * T must stay as they were (-7)
STATE = tuple(n for n in NAMES if n != "hist")


def mix(V, T, kinds):
    """One ``Case`` per kind, of different logits families: ``sampled`` (penalty 1.3 at position 62 / 63, so the ring
    wraps inside the rows), ``greedy`` (temperature 0, penalty 1), ``greedy_pen`` (temperature 0, penalty 1.3),
    ``finished`` (a finished sequence with stale sampling parameters)."""
    make = {"sampled": lambda fi, s: Case(fi, V, T, pos=62 + s % 2, pen=1.3),
            "greedy": lambda fi, s: Case(fi, V, T, pos=10 + s, temp=0.0),
            "greedy_pen": lambda fi, s: Case(fi, V, T, pos=63, pen=1.3, temp=0.0),
            "finished": lambda fi, s: Case(fi, V, T, pos=63, pen=1.3, finished=1)}
    return [make[kind]((0, 1, 3)[s % 3], s) for s, kind in enumerate(kinds)]


class Stack:
    """S ``Case``s as the operands of one S-sequence launch."""

    def __init__(self, cases):
        self.cases, self.S, self.T, self.V = cases, len(cases), cases[0].T, cases[0].V
        self.logits = torch.cat([c.logits for c in cases])
        self.st = {k: torch.cat([c.st[k] for c in cases]) for k in NAMES}
        self.par = {k: torch.cat([c.par[k] for c in cases]) for k in PAR_SEQ}
        self.par["eos"] = cases[0].par["eos"]

    def drafts(self, name):
        """Pattern ``name`` of every sequence: ``right``, or wrong / minus (-1) / oor (out of range) at a j that
        differs from sequence to sequence."""
        k = self.T - 1
        return [c.drafts()["right" if name == "right" else f"{name}{(s + 1) % k}"] for s, c in enumerate(self.cases)]

    def workspace(self, gpu, rows=None):
        rows = self.S * self.T if rows is None else rows
        return (torch.zeros(rows * ((self.V + 4095) // 4096), dtype=torch.int64, device=gpu),
                torch.zeros(rows * ((self.V + 2047) // 2048) * 64, dtype=torch.int64, device=gpu),
                torch.full((NPICKS,), -7, dtype=torch.int32, device=gpu))

    def call(self, lg, dr, stats, st, par, ws):
        ops.spec_sample_commit(lg, dr, stats, st["hist"], par["penalty"], par["temperature"], par["top_k"],
                               par["top_p"], par["seeds"], st["out_tokens"], st["gen_len"], st["input_ids"],
                               st["positions"], st["finished"], par["eos"], par["limit"], par["eos_on"], workspace=ws,
                               last_n=par["last_n"])

    def device(self, gpu):
        d = lambda t: t.to(gpu).clone()  # noqa: E731
        return ({k: d(v) for k, v in self.st.items()}, {k: d(v) for k, v in self.par.items()},
                torch.zeros(self.S, 3, dtype=torch.int64, device=gpu))

    def launch(self, gpu, drafts):
        """One launch with stats [S, 3] from the start state; (state + ring, stats, picks, logits) on the host."""
        st, par, stats = self.device(gpu)
        lg, ws = self.logits.to(gpu).clone(), self.workspace(gpu)
        self.call(lg, torch.tensor(drafts, **I32).to(gpu), stats, st, par, ws)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in st.items()}, stats.tolist(), ws[2].cpu().tolist(), lg.cpu()

    def check(self, gpu, patterns=("right", "wrong", "minus", "oor")):
        S, T, k = self.S, self.T, self.T - 1
        for name in patterns:
            drafts = self.drafts(name)
            got, stats, picks, lg = self.launch(gpu, drafts)
            assert picks[S * T:] == [-7] * (NPICKS - S * T), (name, picks)
            for s, (c, draft) in enumerate(zip(self.cases, drafts)):
                sets, mine = c.sets(draft), picks[s * T:(s + 1) * T]
                for i in range(T):
                    assert mine[i] in sets[i], (name, s, i, mine[i], sorted(sets[i]))
                a = next((i for i in range(k) if draft[i] != c.picks[i]), k)
                assert mine[:a + 1] == c.picks[:a + 1], (name, s, mine, c.picks)  # decided by construction
                want, wstats = c.expect(draft, mine)
                for key in NAMES:
                    assert torch.equal(got[key][s:s + 1], want[key]), (name, s, key)
                assert stats[s] == wstats, (name, s, stats[s], wstats)
                if not int(c.st["finished"]):
                    assert stats[s] == [1, k - (name == "minus"), a], (name, s, stats[s])
                rows = ref._spec_rows(c.logits, torch.tensor(draft, **I32), c.st["hist"], c.par["penalty"],
                                      c.par["last_n"], c.st["positions"])
                # (bitwise but for the last bit of a penalised positive logit: the device's f32 division)
                assert torch.allclose(lg[s * T:(s + 1) * T], torch.stack(rows), rtol=2.5e-7, atol=0.0), (name, s)
                # the sequence's own one-sequence launch: bitwise
                one, ostats, opicks, olg = c.launch(gpu, draft)
                for key in NAMES:
                    assert torch.equal(got[key][s:s + 1], one[key]), (name, s, key)
                assert stats[s] == ostats and mine == opicks[:T] and torch.equal(lg[s * T:(s + 1) * T], olg), (name, s)


# ------------------------------------------------------------------------------------------------ kernel, exact
@pytest.mark.parametrize("V,T,kinds", [(2049, 2, ("sampled", "greedy")),
                                       (5000, 4, ("sampled", "greedy_pen", "finished")),
                                       (2049, 8, ("sampled", "greedy", "greedy_pen", "finished"))])
def test_sequences_equal_the_twin_and_their_own_launch(gpu, V, T, kinds):
    stack = Stack(mix(V, T, kinds))
    assert stack.S * T <= 32
    stack.check(gpu)


def test_llama3_vocabulary(gpu):
    Stack(mix(128256, 4, ("sampled", "greedy_pen"))).check(gpu, patterns=("right",))


def test_greedy_sequence_commits_what_spec_commit_commits(gpu):
    """Temperature 0 and penalty 1: the sequence's state and stats after the sampled commit are those of
    ``ops.spec_commit`` over the same rows and drafts."""
    stack = Stack(mix(2049, 4, ("sampled", "greedy")))
    c = stack.cases[1]
    for name in ("right", "wrong", "minus"):
        drafts = stack.drafts(name)
        got, stats, _, lg = stack.launch(gpu, drafts)
        assert torch.equal(lg[4:], c.logits)  # penalty 1: the rows are left as they are
        d = lambda t: t.to(gpu).clone()  # noqa: E731
        st = {key: d(c.st[key]) for key in STATE}
        gstats = torch.zeros(3, dtype=torch.int64, device=gpu)
        ops.spec_commit(d(c.logits), d(torch.tensor(drafts[1], **I32)), gstats, st["out_tokens"], st["gen_len"],
                        st["input_ids"], st["positions"], st["finished"], d(c.par["eos"]), d(c.par["limit"]),
                        d(c.par["eos_on"]))
        torch.cuda.synchronize()
        for key in STATE:
            assert torch.equal(got[key][1:2], st[key].cpu()), (name, key)
        assert stats[1] == gstats.tolist(), name


def test_sizes_refused_before_any_launch(gpu):
    """40 rows (S = 5, T = 8), T = 1 per sequence, rows not divisible by S, a workspace and a parameter tensor too small
    for S: an error, with the logits, the workspace, the state, the ring and the stats untouched."""
    stack = Stack(mix(2049, 4, ("sampled", "greedy")))
    five = Stack(mix(2049, 8, ("greedy",) * 5))
    cases = [(five, 40, 5, {}, None), (stack, 2, 2, {}, None), (stack, 7, 2, {}, None),
             (stack, 8, 2, {}, 4), (stack, 8, 2, dict(temperature=1), None), (stack, 8, 2, dict(seeds=1), None),
             (stack, 8, 2, dict(penalty=1), None)]
    for sk, rows, S, short, ws_rows in cases:
        logits = torch.randn(rows, sk.V, generator=torch.Generator().manual_seed(rows))
        st, par, _ = sk.device(gpu)
        stats = torch.zeros(S, 3, dtype=torch.int64, device=gpu)
        par = {k: (v[:short[k]] if k in short else v) for k, v in par.items()}
        n = 40 if ws_rows is None else ws_rows
        ws = (torch.full((n * 1,), 11, dtype=torch.int64, device=gpu),
              torch.full((n * 2 * 64,), 12, dtype=torch.int64, device=gpu),
              torch.full((n,), 13, dtype=torch.int32, device=gpu))
        lg = logits.to(gpu)
        with pytest.raises(RuntimeError):
            sk.call(lg, torch.zeros(40, dtype=torch.int32, device=gpu), stats, st, par, ws)
        torch.cuda.synchronize()
        what = (rows, S, short, ws_rows)
        assert torch.equal(lg.cpu(), logits), what
        assert [int(w.min()) for w in ws] == [11, 12, 13] and [int(w.max()) for w in ws] == [11, 12, 13], what
        for key in NAMES:
            assert torch.equal(st[key].cpu(), sk.st[key]), (what, key)
        assert int(stats.abs().sum()) == 0, what


def test_two_launches_are_bitwise_equal(gpu):
    stack = Stack(mix(5000, 4, ("sampled", "greedy_pen", "sampled")))
    drafts = stack.drafts("wrong")
    a, b = stack.launch(gpu, drafts), stack.launch(gpu, drafts)
    for key in NAMES:
        assert torch.equal(a[0][key], b[0][key]), key
    assert a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------ captured graph
def test_captured_graph_replays_the_eager_launches(gpu):
    """Four replays of a graph holding the S = 2 commit equal four eager launches: every sequence's draw counter,
    position and ring are read on the device at replay time (the drafts are all wrong, so each launch commits one
    token per sequence, at a new counter, and the ring of sequence 0 wraps from position 62)."""
    stack = Stack(mix(2049, 4, ("sampled", "greedy_pen")))
    dr = torch.tensor([[stack.V + 5, -1, 0], [-1, stack.V + 5, 1]], **I32).to(gpu)

    def fresh():
        st, par, stats = stack.device(gpu)
        return st, par, stats, stack.workspace(gpu)

    est, par, estats, ews = fresh()
    for _ in range(4):
        stack.call(stack.logits.to(gpu).clone(), dr, estats, est, par, ews)
    torch.cuda.synchronize()
    gst, gpar, gstats, gws = fresh()
    static = torch.zeros(2 * stack.T, stack.V, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # recorded, not executed
            stack.call(static, dr, gstats, gst, gpar, gws)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for _ in range(4):
        static.copy_(stack.logits)  # the penalty is applied in place
        graph.replay()
    torch.cuda.synchronize()
    for key in NAMES:
        assert torch.equal(gst[key], est[key]), key
    assert gstats.tolist() == estats.tolist() == [[4, 8, 0], [4, 8, 0]]
    assert est["gen_len"].tolist() == [2 + 4, 2 + 4] and est["positions"].tolist() == [62 + 4, 63 + 4]
    toks = est["out_tokens"][0, 2:6].tolist()
    assert est["hist"][0, [63, 0, 1, 2]].tolist() == toks and toks[0] == stack.cases[0].picks[0]
    assert est["hist"][1, [0, 1, 2, 3]].tolist() == est["out_tokens"][1, 2:6].tolist()


# ------------------------------------------------------------------------------------------------------- engine
def make(gpu, model, **kw):
    return build_engine(model, device=gpu, max_slots=4, max_model_len=512, seed=0, **kw)


def send(eng, n, **more):
    reqs = [eng.add_request(ids_of(eng, p), params({**o, **more}, n)) for p, o in zip(PROMPTS, MIXED)]
    eng.run_until_done(reqs)
    return reqs


def sampled_keys(eng):
    """The graph keys of sampled verify steps over several sequences: ("spec", T, plan, forced, "sample", S)."""
    return [key for key in eng.runner.graphs if key[0] == "spec" and len(key) >= 2 and key[-2] == "sample"]


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_mixed_verify_steps(gpu, model):
    """The three requests of the engine case -- Ollama's defaults, greedy, another seed without a penalty -- with equal
    budgets and drafts that are alike for all three, so that all finish together and S never changes during a run (a
    change of S changes the GEMM shapes, and with them the logits' last bits).  The baseline is the run whose planted
    drafts are all unusable: one token per request and step.  Planted all-right and first-right drafts repeat its
    tokens with exact counts; a recorded all-right run shows every committed token in the twin's pick set of its own
    row (undecided share printed, at most 10%: the CPU file keeps the reference alone within 5% on this case); a
    plain sampled batch before and after repeats its own tokens; with the flag off the run is the parent's."""
    n = GPU_TOKENS + 1
    eng = make(gpu, model, **ON)
    assert eng.runner.use_graphs and eng.runner.spec_k() == K
    V = eng.runner.V
    p1 = [q.output_ids for q in send(eng, n, speculate=False)]
    assert eng.stats["spec_steps"] == 0 and not sampled_keys(eng)
    eng.runner.set_spec_forced(UNUSABLE)
    base = send(eng, n)
    want = [q.output_ids for q in base]
    assert [(q.spec_steps, q.spec_accepted) for q in base] == [(n - 1, 0)] * 3 and eng.stats["spec_drafted"] == 0
    assert sampled_keys(eng) and all(key[-1] == 4 for key in sampled_keys(eng)), list(eng.runner.graphs)
    per = {"right": K, "first": 1}
    for kind in ("right", "first"):
        s0 = dict(eng.stats)
        eng.runner.set_spec_forced(forced_tables(want, (kind,) * 3, V))
        reqs = send(eng, n)
        assert [q.output_ids for q in reqs] == want, kind
        steps = -(-(n - 1) // (per[kind] + 1))
        assert [(q.spec_steps, q.spec_accepted) for q in reqs] == [(steps, n - 1 - steps)] * 3, kind
        assert eng.stats["spec_steps"] - s0["spec_steps"] == 3 * steps
        assert eng.stats["spec_drafted"] - s0["spec_drafted"] == 3 * K * steps
    # every committed token is the twin's draw of its own recorded row
    eng.runner.set_spec_forced(forced_tables(want, ("right",) * 3, V))
    toks, rows = recorded_draws_batch(eng)
    assert toks == want
    draws = undecided = 0
    for i, opts in enumerate(MIXED):
        assert len(rows[i]) == GPU_TOKENS, i
        for pick_set, tok in rows[i]:
            assert tok in pick_set, (i, tok, sorted(pick_set))
            if opts:  # (a greedy request's rows are always decided)
                draws += 1
                undecided += len(pick_set) > 1
    print(f"{model}: {draws} sampled draws, undecided share {undecided / draws:.4f}")
    assert draws == 2 * GPU_TOKENS and undecided <= 0.10 * draws
    # an all-greedy run on the same engine keeps the greedy batched graph
    before = sampled_keys(eng)
    eng.runner.set_spec_forced(None)
    greedy = [eng.add_request(ids_of(eng, p), params({}, n)) for p in PROMPTS]
    eng.run_until_done(greedy)
    assert sampled_keys(eng) == before
    assert any(key[0] == "spec" and key[-1] == 4 and "sample" not in key for key in eng.runner.graphs)
    # the plain sampled batch after the verify runs repeats its own tokens
    s0 = eng.stats["spec_steps"]
    assert [q.output_ids for q in send(eng, n, speculate=False)] == p1 and eng.stats["spec_steps"] == s0
    # the flag off: the parent's graphs and tokens -- the mixed run is the plain sampled batch
    off = make(gpu, model, **dict(ON, spec_batch_sampled=False))
    assert [q.output_ids for q in send(off, n)] == p1
    assert off.stats["spec_steps"] == 0 and not [key for key in off.runner.graphs if key[0] == "spec"]
    off_greedy = [off.add_request(ids_of(off, p), params({}, n)) for p in PROMPTS]
    off.run_until_done(off_greedy)
    assert [q.output_ids for q in off_greedy] == [q.output_ids for q in greedy]
    assert {key for key in off.runner.graphs if key[0] == "spec"} == \
        {key for key in eng.runner.graphs if key[0] == "spec" and "sample" not in key and key[3] == 0}
