"""Per-token logprobs on the CPU: the host twins (ops/reference.py logprob_rows / logprob_scan / logprob_commit) against
an independent float64 transcription, the recording rule, the raw rule (mask and penalties do not move the values), and
the engine, client and HTTP layers on the tiny model."""
import dataclasses
import json
import math

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.client import EngineService, FakeBackend, GenerateResponse
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.engine import SamplingOptionError
from llm_based_apache_spark_optimization_amd.models.llama import reference_forward
from llm_based_apache_spark_optimization_amd.ops import reference as ref

U = 2.0 ** -24
POISON = -777.25


def f64_rows(logits, tok, k):
    """Independent transcription: l - logsumexp(l) in double, one rounding; top-k by (value desc, index asc)."""
    R, V = logits.shape
    d = logits.double()
    lp = d - torch.logsumexp(d, dim=-1, keepdim=True)
    chosen = torch.tensor([float(lp[r, int(tok[r])]) for r in range(R)]).float()
    ids = torch.full((R, k), -1, dtype=torch.int32)
    top = torch.full((R, k), float("-inf"))
    for r in range(R):
        order = sorted(range(V), key=lambda i: (-float(logits[r, i]), i))[:k]
        for j, i in enumerate(order):
            ids[r, j] = i
            top[r, j] = float(lp[r, i])
    return chosen, ids, top


def test_logprob_rows_against_float64():
    torch.manual_seed(0)
    for V, sigma in ((50, 1.0), (2049, 12.0), (5000, 4.0)):
        lg = torch.randn(3, V) * sigma
        tok = torch.tensor([0, V - 1, V // 2])
        got = ref.logprob_rows(lg, tok, 5)
        want = f64_rows(lg, tok, 5)
        assert torch.equal(got[1], want[1])
        # two float64 evaluations of one formula, each rounded once to f32: at most an ulp of the f32 result apart
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            assert float((g.double() - w.double()).abs().max()) <= 2 * U * float(w.abs().max())
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32


def test_tie_order_and_k_above_v():
    lg = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5]])
    _, ids, top = ref.logprob_rows(lg, torch.tensor([1]), 4)
    assert ids.tolist() == [[1, 2, 4, 0]]  # equal values: the lower index first
    assert top[0, 0] == top[0, 1] == top[0, 2]
    chosen, ids, top = ref.logprob_rows(torch.zeros(1, 10), torch.tensor([3]), 20)
    assert ids[0, :10].tolist() == list(range(10)) and ids[0, 10:].tolist() == [-1] * 10
    assert torch.all(top[0, 10:] == float("-inf"))
    assert float(chosen[0]) == pytest.approx(-math.log(10), abs=1e-6)
    assert torch.all(top[0, :10] == chosen[0])


def _state(B, max_new, V, K=20):
    i32 = dict(dtype=torch.int32)
    return dict(out_tokens=torch.zeros(B, max_new, **i32), gen_len=torch.zeros(B, **i32),
                input_ids=torch.zeros(B, **i32), positions=torch.full((B,), 5, **i32), finished=torch.zeros(B, **i32),
                lp_k=torch.full((B,), -1, **i32), lp_n0=torch.full((B,), -1, **i32),
                lp_tok=torch.full((B, max_new), POISON), lp_ids=torch.full((B, max_new, K), -9, **i32),
                lp_top=torch.full((B, max_new, K), POISON), lp_raw=torch.full((B, V), POISON))


def _step(st, logits, eos, limit, mutate=None):
    """scan -> (mask / penalty stand-in) -> greedy commit -> logprob commit through the public ops (CPU twins)."""
    B = logits.shape[0]
    ops.logprob_scan(logits, st["lp_k"], st["finished"], st["gen_len"], st["lp_raw"], st["lp_n0"])
    if mutate is not None:
        mutate(logits)
    ops.argmax_commit(logits, st["out_tokens"], st["gen_len"], st["input_ids"], st["positions"], st["finished"], eos,
                      limit=limit)
    ops.logprob_commit(st["lp_raw"], st["lp_k"], st["lp_n0"], st["gen_len"], st["out_tokens"], st["lp_tok"],
                       st["lp_ids"], st["lp_top"], B)


def test_which_rows_record_and_where():
    torch.manual_seed(1)
    B, V, max_new = 5, 300, 4
    st = _state(B, max_new, V)
    # row 0 did not ask; row 1 finished before the step; row 2 finishes in the step (limit); row 3 plain, K = 3;
    # row 4 sits at n0 == max_new (unfinished: only a malformed state gets there, and nothing may be written)
    st["lp_k"][:] = torch.tensor([-1, 2, 0, 3, 1], dtype=torch.int32)
    st["finished"][1] = 1
    st["gen_len"][:] = torch.tensor([1, 2, 3, 1, 4], dtype=torch.int32)
    st["lp_n0"][1] = 1  # what the row's last live step left behind must not make it record again
    limit = torch.tensor([4, 4, 4, 4, 9], dtype=torch.int32)
    lg = torch.randn(B, V)
    raw = lg.clone()
    before = {k: st[k].clone() for k in ("lp_tok", "lp_ids", "lp_top")}
    _step(st, lg, torch.tensor([-1], dtype=torch.int32), limit)
    assert torch.equal(lg, raw)
    assert st["gen_len"].tolist() == [2, 2, 4, 2, 5] and st["finished"].tolist() == [0, 1, 1, 0, 1]
    for b in (0, 1, 4):
        for k in before:
            assert torch.equal(st[k][b], before[k][b]), (b, k)
    assert st["lp_n0"].tolist()[2:] == [-1, -1, -1]
    for b, n0, K in ((2, 3, 0), (3, 1, 3)):
        tok = st["out_tokens"][b, n0:n0 + 1]
        chosen, ids, top = ref.logprob_rows(raw[b:b + 1], tok, K)
        assert st["lp_tok"][b, n0] == chosen[0]
        assert torch.equal(st["lp_ids"][b, n0, :K], ids[0]) and torch.equal(st["lp_top"][b, n0, :K], top[0])
        assert torch.all(st["lp_top"][b, n0, K:] == POISON) and torch.all(st["lp_ids"][b, n0, K:] == -9)
        keep = torch.ones(max_new, dtype=torch.bool)
        keep[n0] = False
        assert torch.all(st["lp_tok"][b][keep] == POISON)
    # greedy: the chosen token is top-1, bitwise
    assert st["lp_ids"][3, 1, 0] == st["out_tokens"][3, 1] and st["lp_top"][3, 1, 0] == st["lp_tok"][3, 1]


def test_mask_and_penalty_do_not_move_the_values():
    """The same logits with and without a penalty / a mask between scan and commit.  The tokens are equal by
    construction: greedy rows, and what is rewritten is never the argmax."""
    torch.manual_seed(2)
    B, V = 2, 400
    lg = torch.randn(B, V)
    top2 = lg.topk(2, dim=-1).indices

    def mutate(x):  # a penalty on the runner-up of row 0, a mask (-inf) over the runner-up of row 1
        x[0, top2[0, 1]] = x[0, top2[0, 1]] / 1.7 - 0.4
        x[1, top2[1, 1]] = float("-inf")

    out = []
    for m in (None, mutate):
        st = _state(B, 4, V)
        st["lp_k"][:] = 5
        _step(st, lg.clone(), torch.tensor([-1], dtype=torch.int32), torch.full((B,), 4, dtype=torch.int32), m)
        out.append(st)
    a, b = out
    assert torch.equal(a["out_tokens"], b["out_tokens"])
    for k in ("lp_tok", "lp_ids", "lp_top"):
        assert torch.equal(a[k], b[k]), k
    assert b["lp_ids"][1, 0, 1] == top2[1, 1]  # the masked-out token is still reported, with its raw probability


def test_ops_refusals():
    st = _state(2, 4, 64)
    lg = torch.randn(2, 64)
    args = (st["lp_k"], st["finished"], st["gen_len"], st["lp_raw"], st["lp_n0"])
    with pytest.raises(ValueError):
        ops.logprob_scan(lg.double(), *args)
    with pytest.raises(ValueError):
        ops.logprob_scan(lg.t().contiguous().t(), *args)
    with pytest.raises(ValueError):
        ops.logprob_scan(torch.randn(2, 65), *args)  # lp_raw of another V
    cm = lambda **kw: ops.logprob_commit(*[kw.get(k, st[k]) for k in (  # noqa: E731
        "lp_raw", "lp_k", "lp_n0", "gen_len", "out_tokens", "lp_tok", "lp_ids", "lp_top")], 2)
    cm()
    with pytest.raises(ValueError):  # K outside 0 .. 20
        cm(lp_ids=torch.zeros(2, 4, 21, dtype=torch.int32), lp_top=torch.zeros(2, 4, 21))
    with pytest.raises(ValueError):  # records that do not match out_tokens
        cm(lp_tok=torch.zeros(2, 5))
    with pytest.raises(ValueError):
        cm(lp_ids=torch.zeros(2, 3, 20, dtype=torch.int32), lp_top=torch.zeros(2, 3, 20))
    with pytest.raises(ValueError):
        cm(lp_top=torch.zeros(2, 4, 20, dtype=torch.float64))
    with pytest.raises(ValueError):  # V above the sampler's bound
        ops.logprob_commit(torch.zeros(1, 262145), st["lp_k"], st["lp_n0"], st["gen_len"], st["out_tokens"],
                           st["lp_tok"], st["lp_ids"], st["lp_top"], 1)


# ----------------------------------------------------------------------------------- engine (tiny model, CPU)
KW = dict(device="cpu", max_slots=4, max_model_len=512)
PROMPTS = [[1] + list(range(5 + 3 * k, 30 + 3 * k)) for k in range(3)]


@pytest.fixture(scope="module")
def eng():
    return build_engine("tiny-nsql", logprobs=True, **KW)


@pytest.fixture(scope="module")
def plain():
    return build_engine("tiny-nsql", **KW)


def _gen(e, prompts, sps):
    reqs = [e.add_request(p, sp) for p, sp in zip(prompts, sps)]
    e.run_until_done(reqs)
    return [e.result(q) for q in reqs]


def test_engine_values_against_teacher_forced_float64(eng, plain):
    sp = SamplingParams(max_tokens=12, ignore_eos=True, logprobs=True, top_logprobs=5)
    seen, scan = [], eng.runner._logprob_scan

    def spy(logits, *a):  # the raw rows the engine scanned, in step order (prefill tail first)
        seen.append(logits[0].clone())
        scan(logits, *a)

    eng.runner._logprob_scan = spy
    try:
        res = _gen(eng, PROMPTS[:1], [sp])[0]
    finally:
        del eng.runner._logprob_scan
    assert res.eval_count == 12 and len(res.logprobs) == 12 and len(seen) == 12
    # against float64 over the very rows the engine scanned: |err| <= 8 * 2^-24 * (1 + |lse| + |l|)
    for j, ent in enumerate(res.logprobs):
        d = seen[j].double()
        lse = float(torch.logsumexp(d, 0))
        for tid, got in [(res.token_ids[j], ent["logprob"])] + [
                (int(i), t["logprob"]) for i, t in zip(d.float().sort(descending=True, stable=True).indices[:5],
                                                       ent["top_logprobs"])]:
            l = float(d[tid])
            err = abs(got - (l - lse))
            print(f"step {j} token {tid}: err / (2^-24 (1 + |lse| + |l|)) = {err / (U * (1 + abs(lse) + abs(l))):.3f}")
            assert err <= 8 * U * (1 + abs(lse) + abs(l))
    base = _gen(plain, PROMPTS[:1], [dataclasses.replace(sp, logprobs=False, top_logprobs=0)])[0]
    assert base.token_ids == res.token_ids and base.logprobs is None
    # and against the teacher-forced oracle.  Its logits are not the engine's (the oracle keeps f32 activations where the
    # engine rounds to bf16, relative step 2^-8, layer after layer), so the bound above cannot apply to them: a
    # log-probability of magnitude <= 8 built from logits that differ by a few bf16 steps is held to 8 * 4 * 2^-8 =
    # 0.125, far below what a wrong row, index or distribution gives (nats)
    p = PROMPTS[0]
    lg = reference_forward(eng.runner.w, p + res.token_ids[:-1])[len(p) - 1:]
    lp64 = torch.log_softmax(lg.double(), dim=-1)
    for j, ent in enumerate(res.logprobs):
        tid = res.token_ids[j]
        assert ent["token"] == eng.tok.decode([tid]) and bytes(ent["bytes"]) == eng._bytes_of([tid])
        print(f"step {j}: engine {ent['logprob']:.6f} oracle {float(lp64[j, tid]):.6f}")
        assert abs(ent["logprob"] - float(lp64[j, tid])) <= 0.125, (j, ent["logprob"], float(lp64[j, tid]))
        tops = ent["top_logprobs"]
        assert len(tops) == 5 and all(a["logprob"] >= b["logprob"] for a, b in zip(tops, tops[1:]))
        # greedy: the chosen token is top-1 with the very same value
        assert tops[0]["logprob"] == ent["logprob"] and tops[0]["token"] == ent["token"]
        assert sum(math.exp(t["logprob"]) for t in tops) <= 1.0 + 1e-6


def test_neighbour_and_tokens_unchanged(eng, plain):
    """A mixed batch: requests that ask beside ones that do not, greedy and sampled.  Every request's tokens are
    those of the engine without the feature, and its values those of its own run alone."""
    ask = SamplingParams(max_tokens=10, ignore_eos=True, logprobs=True, top_logprobs=3)
    no = SamplingParams(max_tokens=10, ignore_eos=True)
    smp = SamplingParams(max_tokens=10, ignore_eos=True, temperature=0.8, seed=11, repeat_penalty=1.2, logprobs=True,
                         top_logprobs=2)
    for e in (eng, plain):
        e.runner.rr_decode = False  # solo runs on the batched runs' step (tests/test_kv_lazy.py)
    sps = [ask, no, smp]
    mixed = _gen(eng, PROMPTS, sps)
    off = [dataclasses.replace(s, logprobs=False, top_logprobs=0) for s in sps]
    want = _gen(plain, PROMPTS, off)
    assert [r.token_ids for r in mixed] == [r.token_ids for r in want]
    assert mixed[1].logprobs is None and len(mixed[0].logprobs) == 10 and len(mixed[2].logprobs) == 10
    for i in (0, 2):
        solo = _gen(eng, [PROMPTS[i]], [sps[i]])[0]
        assert solo.token_ids == mixed[i].token_ids
        # the values are those of the row's own logits, and those are not bitwise the same at another batch size on the
        # CPU: the GEMMs sum in another order, and where that flips the bf16 rounding of an activation (relative step
        # 2^-8) the logits, of a few units, move by up to that fraction.  So 2^-8 here; bitwise independence of the
        # neighbours is the kernels' property (tests/test_logprobs_gpu.py)
        assert [x["token"] for x in solo.logprobs] == [x["token"] for x in mixed[i].logprobs]
        assert all(abs(x["logprob"] - y["logprob"]) <= 2.0 ** -8 for x, y in zip(solo.logprobs, mixed[i].logprobs))
    # a sampled, penalised row reports the raw distribution: top-1 is the raw argmax, whatever was drawn
    assert all(len(e["top_logprobs"]) == 2 and e["logprob"] <= e["top_logprobs"][0]["logprob"]
               for e in mixed[2].logprobs)
    # no request asks: the engine replays the graphs (CPU: takes the steps) it takes without the feature
    n = eng.stats["logprob_steps"]
    again = _gen(eng, PROMPTS[:2], [no, no])
    assert [r.token_ids for r in again] == [r.token_ids for r in want[:2]]
    assert eng.stats["logprob_steps"] == n


def test_preemption_keeps_the_list_complete_and_ordered():
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    e = build_engine("tiny-nsql", device="cpu", max_slots=3, max_model_len=512, num_kv_blocks=9, logprobs=True)
    sp = SamplingParams(max_tokens=150, ignore_eos=True, logprobs=True, top_logprobs=1)
    solo = [_gen(e, [p], [sp])[0] for p in prompts]
    e.run_ahead = 16
    reqs = [e.add_request(p, sp) for p in prompts]
    kept, preempt = {}, e._preempt

    def spy(q):  # what the request holds on the host once its slot is gone
        preempt(q)
        assert len(q.logprobs) == len(q.resumed) and q.lp_read == 0
        kept[q.rid] = list(q.logprobs)

    e._preempt = spy
    e.run_until_done(reqs)
    assert e.stats["preempted"] >= 1 and any(q.preemptions for q in reqs) and kept
    for q, s in zip(reqs, solo):
        r = e.result(q)
        assert r.token_ids == s.token_ids and len(r.logprobs) == 150
        # greedy: every entry is its step's top-1, for the token at that place -- none lost, doubled or shifted
        assert [x["token"] for x in r.logprobs] == [e.tok.decode([t]) for t in r.token_ids]
        assert all(x["top_logprobs"][0]["logprob"] == x["logprob"] for x in r.logprobs)
        # entries from before a preemption are the values recorded when the token was first generated, bitwise
        if q.rid in kept:
            assert q.logprobs[:len(kept[q.rid])] == kept[q.rid]
        # and all of them are the solo run's up to the CPU GEMMs' batch-size dependence (see above)
        assert all(abs(x["logprob"] - y["logprob"]) <= 2.0 ** -8 for x, y in zip(r.logprobs, s.logprobs))


def test_refusals_and_flags(eng, plain):
    with pytest.raises(SamplingOptionError) as ei:
        plain.add_request(PROMPTS[0], SamplingParams(logprobs=True))
    assert "LSA_LOGPROBS" in str(ei.value)
    for bad in (dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1), dict(top_logprobs=3)):
        with pytest.raises(SamplingOptionError):
            eng.add_request(PROMPTS[0], SamplingParams(**bad))
    with pytest.raises(SamplingOptionError):
        SamplingParams.from_ollama_options({"logprobs": True, "top_logprobs": "many"})
    sp = SamplingParams.from_ollama_options({"logprobs": True, "top_logprobs": 4})
    assert sp.logprobs and sp.top_logprobs == 4
    assert not SamplingParams.from_ollama_options({}).logprobs
    assert eng.logprobs and eng.runner.logprobs and not plain.logprobs and not plain.runner.logprobs
    assert not hasattr(plain.runner, "lp_raw")
    assert Settings().logprobs is False and Settings().sql_logprobs is False
    r = plain.runner
    assert r.graph_key(4, True, (1, 2, 3)) == (4, True, (1, 2, 3))
    assert r.graph_key(4, False, (1, 2, 3), True) == (4, False, (1, 2, 3), True)
    assert r.graph_key(4, False, (1, 2, 3), False, True) == (4, False, (1, 2, 3), False, "lp")
    assert r.graph_key(4, False, (1, 2, 3), True, True) == (4, False, (1, 2, 3), True, "lp")
    # the memory enable_logprobs takes, computed: records + raw rows + chunk workspaces
    S, cap, V = eng.runner.max_slots, eng.runner.max_new_cap, eng.runner.V
    nch = -(-V // 2048)
    assert eng.runner.logprobs_bytes() == S * (8 + cap * 4 * (1 + 2 * 20) + V * 4 + nch * (8 + 32 * 8))


# ----------------------------------------------------------------------------------- client and HTTP
@pytest.fixture(scope="module")
def svc(eng, plain):
    s = EngineService(lambda model: eng if model == "lp" else plain, defaults={"num_predict": 12, "ignore_eos": True})
    yield s
    for m in s.models():
        s.loop(m).close()


def test_response_key_only_when_asked(svc):
    r = svc.generate("lp", "select all rows")
    assert "logprobs" not in r.to_dict() and r.logprobs is None
    assert set(r.to_dict()) == {f.name for f in dataclasses.fields(GenerateResponse)} - {"logprobs"}
    r = svc.generate("lp", "select all rows", options={"logprobs": True, "top_logprobs": 2})
    d = r.to_dict()
    assert len(d["logprobs"]) == r.eval_count == 12
    assert set(d["logprobs"][0]) == {"token", "logprob", "bytes", "top_logprobs"}
    assert set(d["logprobs"][0]["top_logprobs"][0]) == {"token", "logprob", "bytes"}
    json.dumps(d)
    r0 = svc.generate("lp", "select all rows", options={"logprobs": True})
    assert "top_logprobs" not in r0.logprobs[0] and [e["logprob"] for e in r0.logprobs] == [e["logprob"] for e in r.logprobs]


def test_streaming_concatenates_to_the_whole_list(svc):
    opts = {"logprobs": True, "top_logprobs": 3, "num_predict": 30}
    whole = svc.generate("lp", "count the rows", options=opts)
    chunks = list(svc.generate_stream("lp", "count the rows", options=opts))
    assert chunks[-1].done and not any(c.done for c in chunks[:-1])
    cat = [e for c in chunks for e in (c.logprobs or [])]
    assert cat == whole.logprobs and len(cat) == 30
    assert "".join(c.response for c in chunks) == whole.response
    assert sum(1 for c in chunks if c.logprobs) > 1  # they arrive with the syncs, not at the end
    plain_chunks = list(svc.generate_stream("lp", "count the rows", options={"num_predict": 8}))
    assert all("logprobs" not in c.to_dict() for c in plain_chunks)


def test_stop_string_keeps_one_entry_per_counted_token(svc):
    """A stop string cuts the text; the engine's token accounting (eval_count) is what it is without logprobs, and
    the list has one entry per counted token."""
    base = svc.generate("lp", "list the names", options={"logprobs": True, "num_predict": 20})
    assert len(base.response) > 4
    stop = base.response[len(base.response) // 2:][:3]
    cut = svc.generate("lp", "list the names", options={"logprobs": True, "num_predict": 20, "stop": [stop]})
    assert len(cut.response) < len(base.response) and stop not in cut.response
    assert len(cut.logprobs) == cut.eval_count
    assert cut.logprobs == base.logprobs[:cut.eval_count]


def test_http_layer(svc, tmp_path):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context

    def app(**kw):
        s = Settings(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"),
                     history_dsn="sqlite:///" + str(tmp_path / "h.db"), engine="hip", secret_key="test",
                     nl2sql_model="lp", explain_model="lp", logprobs=True, **kw)
        return TestClient(create_app(make_context(s, backend=svc)))

    c = app()
    r = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "logprobs": True, "top_logprobs": 2})
    assert r.status_code == 200 and len(r.json()["logprobs"]) == r.json()["eval_count"]
    assert len(r.json()["logprobs"][0]["top_logprobs"]) == 2
    r2 = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "options": {"logprobs": True, "top_logprobs": 2}})
    assert r2.json()["logprobs"] == r.json()["logprobs"]
    assert "logprobs" not in c.post("/api/generate", json={"model": "lp", "prompt": "hi"}).json()
    r = c.post("/api/generate", json={"model": "plain", "prompt": "hi", "logprobs": True})
    assert r.status_code == 400 and "logprobs" in r.json()["detail"]
    r = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "logprobs": True, "top_logprobs": 21})
    assert r.status_code == 400
    r = c.post("/api/generate", json={"model": "lp", "prompt": "hi", "top_logprobs": 2})
    assert r.status_code == 400
    assert c.get("/health").status_code == 200
    assert svc.health()["engines"]["lp"]["logprobs"] is True and svc.health()["engines"]["plain"]["logprobs"] is False
    # /nl2sql: the two fields exist exactly with sql_logprobs
    body = {"question": "how many rows", "table_schema": "Name (string)", "options": {"num_predict": 6}}
    off = c.post("/nl2sql", json=body).json()
    on = app(sql_logprobs=True).post("/nl2sql", json=body).json()
    assert set(on) - set(off) == {"sql_mean_logprob", "sql_min_logprob"} and set(off) <= set(on)
    assert on["sql_query"] == off["sql_query"]
    assert on["sql_min_logprob"] <= on["sql_mean_logprob"] <= 0.0
    with pytest.raises(ValueError):
        make_context(Settings(engine="hip", sql_logprobs=True, secret_key="t"), backend=svc)


def test_fake_backend_refuses():
    with pytest.raises(SamplingOptionError):
        FakeBackend().generate("duckdb-nsql", "q", options={"logprobs": True})
    assert "logprobs" not in FakeBackend().generate("duckdb-nsql", "q").to_dict()
