"""Embeddings on the CPU: the host twins of the three kernels (``ops.reference.embed_*``) under the checks of
embed_cases.py, the engine's vectors however a request is run, the float64 oracle, and the HTTP / client plumbing.
test_embed_gpu.py runs the same builders over the kernels of csrc/kernels/embed.hip and the captured engine."""
import argparse
import dataclasses
import io
import json
import types
import urllib.error

import pytest
import torch

import embed_cases as ec
from llm_based_apache_spark_optimization_amd import client as lsa_client
from llm_based_apache_spark_optimization_amd.client import Backend, EngineService, FakeBackend, RemoteBackend
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.engine import SamplingOptionError
from llm_based_apache_spark_optimization_amd.eval import numerics
from llm_based_apache_spark_optimization_amd.utils.metrics import REGISTRY

CPU = "cpu"


# ----------------------------------------------------------------------------------- the twins
@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_twin_rowscale(D, nslab):
    ec.check_rowscale(D, nslab, CPU)


@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_twin_pool(D, nslab):
    ec.check_pool(D, nslab, CPU)


@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_twin_chunk_invariance(D, nslab):
    ec.check_chunk_invariance(D, nslab, CPU)


@pytest.mark.parametrize("nslab", (0, 3))
@pytest.mark.parametrize("D", ec.DS)
def test_twin_last(D, nslab):
    ec.check_last(D, nslab, CPU)


@pytest.mark.parametrize("D", ec.DS)
def test_twin_finish(D):
    ec.check_finish(D, CPU)


def test_ops_refusals():
    ec.check_refusals(CPU)


# ----------------------------------------------------------------------------------- engine (tiny models, CPU)
KW = dict(device="cpu", max_slots=8, max_model_len=512)
MODELS = ("tiny-nsql", "tiny-llama3")
INPUTS = [ec.input_ids(n, k=k) for k, n in enumerate(ec.IN_LENS)]


def embed_many(e, inputs, pooling):
    reqs = [e.add_request(ids, SamplingParams(embed=pooling)) for ids in inputs]
    e.run_until_done(reqs)
    return [e.result(q) for q in reqs]


def vec(res):
    return torch.tensor(res.embedding, dtype=torch.float32)


@pytest.fixture(scope="module", params=MODELS)
def world(request):
    """(model, engine with embeddings, {(pooling, input index): vector of the input embedded alone})."""
    e = build_engine(request.param, embeddings=True, **KW)
    alone = {}
    for pooling in ("mean", "last"):
        for i, ids in enumerate(INPUTS):
            r = embed_many(e, [ids], pooling)[0]
            assert r.eval_count == 1 and r.prompt_tokens == len(ids) and r.logprobs is None
            assert len(r.embedding) == e.runner.d
            alone[(pooling, i)] = vec(r)
    return request.param, e, alone


def test_unit_norm_and_poolings_differ(world):
    _, e, alone = world
    for (pooling, i), v in alone.items():
        assert abs(float(v.double().norm()) - 1.0) < 2.0 ** -20, (pooling, i)
    for i in range(len(INPUTS)):
        assert not ec.same_bits(alone[("mean", i)], alone[("last", i)])
        assert float((alone[("mean", i)] - alone[("last", i)]).norm()) > 1e-3
    assert e.stats["embed_requests"] == 2 * len(INPUTS)
    assert e.stats["embed_tokens"] == 2 * sum(ec.IN_LENS)


def test_same_bits_packed_and_beside_a_generation(world):
    model, e, alone = world
    for pooling in ("mean", "last"):
        for i, r in enumerate(embed_many(e, INPUTS, pooling)):
            assert ec.same_bits(vec(r), alone[(pooling, i)]), (pooling, i)
    # beside a running generate request, whose tokens are those it generates alone
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    prompt = ec.input_ids(40, k=9)
    solo = e.add_request(prompt, sp)
    e.run_until_done([solo])
    gen = e.add_request(prompt, sp)
    e.run_ahead = 2  # (a run of decode steps ends after 2, so that the request is still running when the inputs arrive)
    try:
        e.step()
        assert not gen.done.is_set() and gen.gen_host >= 1
        reqs = [e.add_request(ids, SamplingParams(embed="mean")) for ids in INPUTS[:3]]
        e.run_until_done(reqs + [gen])
    finally:
        e.run_ahead = None
    assert gen.output_ids == solo.output_ids and e.result(gen).embedding is None
    for i, q in enumerate(reqs):
        assert ec.same_bits(q.embedding, alone[("mean", i)])
    # mixed poolings and a generate request in one packed prefill
    mixed = [e.add_request(INPUTS[3], SamplingParams(embed="last")), e.add_request(prompt, sp),
             e.add_request(INPUTS[1], SamplingParams(embed="mean"))]
    e.run_until_done(mixed)
    assert ec.same_bits(mixed[0].embedding, alone[("last", 3)]) and ec.same_bits(mixed[2].embedding, alone[("mean", 1)])
    assert mixed[1].output_ids == solo.output_ids


@pytest.mark.parametrize("chunk", (16, 64))
def test_same_bits_chunked_and_preempted(world, chunk):
    model, _, alone = world
    c = build_engine(model, embeddings=True, prefill_chunk=chunk, **KW)
    for pooling in ("mean", "last"):
        for i, r in enumerate(embed_many(c, INPUTS, pooling)):
            assert ec.same_bits(vec(r), alone[(pooling, i)]), (pooling, i)
        for i, ids in enumerate(INPUTS):  # one at a time: other call shapes again
            assert ec.same_bits(vec(embed_many(c, [ids], pooling)[0]), alone[(pooling, i)]), (pooling, i)
    # preempted by hand in the middle of its chunked prompt: the re-admitted request pools again from position 0
    for pooling in ("mean", "last"):
        q = c.add_request(INPUTS[3], SamplingParams(embed=pooling))
        c.step()
        c.step()
        assert 0 < q.prefilled < len(INPUTS[3])
        c._preempt(q)
        assert q.prefilled == 0 and q.embedding is None
        c.run_until_done([q])
        assert q.preemptions == 1 and ec.same_bits(q.embedding, alone[(pooling, 3)])


def test_prefix_cache(world):
    model, _, alone = world
    e = build_engine(model, embeddings=True, prefix_cache=True, **KW)
    for k in range(2):  # a mean request computes every row, both times
        r = embed_many(e, [INPUTS[3]], "mean")[0]
        assert r.cached_prompt_tokens == 0 and ec.same_bits(vec(r), alone[("mean", 3)])
    first = embed_many(e, [INPUTS[3]], "last")[0]
    again = embed_many(e, [INPUTS[3]], "last")[0]
    assert again.cached_prompt_tokens >= 64, "a last request keeps today's match rule"
    assert ec.same_bits(vec(first), alone[("last", 3)]) and ec.same_bits(vec(again), alone[("last", 3)])


def _logged(e, run):
    calls, pf, pc = [], e.runner.prefill, e.runner.prefill_chunk

    def norm(a):
        return [[(s, list(ids), p0) for s, ids, p0 in x] if isinstance(x, list) else x for x in a]

    e.runner.prefill = lambda *a, **kw: (calls.append(("prefill", norm(a), sorted(kw.items()))), pf(*a, **kw))[1]
    e.runner.prefill_chunk = lambda *a, **kw: (calls.append(("chunk", norm(a), sorted(kw.items()))), pc(*a, **kw))[1]
    try:
        out = run(e)
    finally:
        del e.runner.prefill, e.runner.prefill_chunk
    return calls, out


@pytest.mark.parametrize("chunk", (None, 16))
def test_nobody_asks_calls_the_runner_as_before(chunk):
    """An engine with embeddings on and no embedding request makes the prefill / prefill_chunk calls, arguments
    included, of an engine without; and its tokens are the same."""
    def run(e):
        sp = SamplingParams(max_tokens=4, ignore_eos=True)
        reqs = [e.add_request(INPUTS[0], sp), e.add_request(INPUTS[2], sp)]
        e.run_until_done(reqs)
        return [q.output_ids for q in reqs]

    on = build_engine("tiny-nsql", embeddings=True, prefill_chunk=chunk, **KW)
    off = build_engine("tiny-nsql", prefill_chunk=chunk, **KW)
    assert on.runner.embeddings and not off.runner.embeddings and not hasattr(off.runner, "emb_acc")
    a, b = _logged(on, run), _logged(off, run)
    assert a == b and a[0] and all(not kw for _, _, kw in a[0])
    # and once somebody asks, the embed tuples ride along
    calls, _ = _logged(on, lambda e: embed_many(e, [INPUTS[0]], "mean"))
    assert dict(calls[-1][2])["embed"] == [("mean", len(INPUTS[0]), True)]


@pytest.mark.parametrize("pooling", ("mean", "last"))
def test_against_the_float64_oracle(world, pooling):
    """||e - e_o||_2 <= 2 kappa rel_max, e_o from the oracle's final-norm rows pooled and normalised in float64, kappa =
    mean ||y_o,t|| / ||pooled y_o||, rel_max the hidden-state bound of eval/numerics.py for the runner's class."""
    model, e, alone = world
    rel_max = numerics.hidden_rel_max(numerics.numerics_class(e.runner, 1), len(e.runner.w.layers))
    for i, ids in enumerate(INPUTS):
        e_o, kappa = ec.oracle_vector(e.runner.w, ids, pooling)
        err = float((alone[(pooling, i)].double() - e_o).norm())
        print(f"{model} {pooling} {len(ids)} tokens: error {err:.3e}, bound {2 * kappa * rel_max:.3e} (kappa {kappa:.2f})")
        assert err <= 2 * kappa * rel_max


# ----------------------------------------------------------------------------------- refusals, client, HTTP
def test_engine_refusals():
    plain = build_engine("tiny-nsql", **KW)
    e = build_engine("tiny-nsql", embeddings=True, **KW)
    with pytest.raises(SamplingOptionError) as ei:
        plain.add_request(INPUTS[0], SamplingParams(embed="mean"))
    assert "LSA_EMBEDDINGS" in str(ei.value)
    with pytest.raises(SamplingOptionError):
        e.add_request(INPUTS[0], SamplingParams(embed="max"))
    with pytest.raises(SamplingOptionError):
        e.add_request([1], SamplingParams(embed="last"))
    assert SamplingParams.from_ollama_options({"embed": "mean", "pooling": "mean"}).embed is None
    assert e.embeddings_supported and not plain.embeddings_supported
    e.runner.tp = types.SimpleNamespace(size=2, rank=0)
    try:
        assert not e.embeddings_supported
        with pytest.raises(SamplingOptionError) as ei:
            e.add_request(INPUTS[0], SamplingParams(embed="mean"))
        assert "tensor parallelism" in str(ei.value)
    finally:
        e.runner.tp = None
    live = e._emb_live
    with pytest.raises(ValueError):
        e.add_requests([INPUTS[0], [1] * 600], SamplingParams(embed="mean"))
    assert not e.has_work() and e._emb_live == live == 0
    # a runner without the buffers refuses the call itself
    with pytest.raises(AssertionError):
        plain.runner.prefill([(0, INPUTS[0], 0)], embed=[("mean", 5, True)])


@pytest.fixture(scope="module")
def svc():
    on = build_engine("tiny-nsql", embeddings=True, **KW)
    off = build_engine("tiny-nsql", **KW)
    s = EngineService(lambda model: on if model == "emb" else off, defaults={"num_predict": 6, "ignore_eos": True})
    s.on = on
    yield s
    for m in s.models():
        s.loop(m).close()


def text_of(n: int) -> str:
    """A text of n tokens under the tiny models' byte tokenizer (BOS + one token per ASCII byte)."""
    return ("select name, age from temp_view where age > 21 order by name; " * 8)[: n - 1]


def test_service_and_client(svc):
    texts = [text_of(n) for n in ec.IN_LENS]
    out = svc.embed("emb", texts)
    assert set(out) == {"model", "embeddings", "total_duration", "load_duration", "prompt_eval_count"}
    assert out["load_duration"] == 0 and out["prompt_eval_count"] == sum(ec.IN_LENS) and len(out["embeddings"]) == 4
    for v in out["embeddings"]:
        assert len(v) == svc.on.runner.d and abs(sum(x * x for x in v) ** 0.5 - 1.0) < 2.0 ** -20
    one = svc.embed("emb", texts[2])
    assert one["embeddings"] == [out["embeddings"][2]] and one["prompt_eval_count"] == 65
    mean = svc.embed("emb", texts, options={"pooling": "mean"})
    assert all(a != b for a, b in zip(mean["embeddings"], out["embeddings"]))
    assert svc.embed("emb", texts, options={"pooling": "last"})["embeddings"] == out["embeddings"]
    json.dumps(out)
    # the module-level call goes through the configured backend
    old = lsa_client._backend
    lsa_client.set_backend(svc)
    try:
        assert lsa_client.embed(model="emb", input=texts[0])["embeddings"] == [out["embeddings"][0]]
    finally:
        lsa_client.set_backend(old)
    # truncate: the window is min(max_model_len, num_ctx) less the request's one token
    long = text_of(130)
    cut = svc.embed("emb", long, options={"num_ctx": 65, "pooling": "mean"})
    assert cut["prompt_eval_count"] == 64
    assert cut["embeddings"] == svc.embed("emb", long[:63], options={"pooling": "mean"})["embeddings"]
    with pytest.raises(SamplingOptionError):
        svc.embed("emb", long, truncate=False, options={"num_ctx": 65})
    assert svc.embed("emb", long[:63], truncate=False, options={"num_ctx": 65})["prompt_eval_count"] == 64
    for bad in ([], ["x"] * 65, "", ["ok", ""], 7, ["ok", 3]):
        with pytest.raises(SamplingOptionError):
            svc.embed("emb", bad)
    with pytest.raises(SamplingOptionError):
        svc.embed("emb", "x y", options={"pooling": "max"})
    with pytest.raises(SamplingOptionError):
        svc.embed("plain", "x y")
    h = svc.health()["engines"]
    assert h["emb"]["embeddings"] is True and h["plain"]["embeddings"] is False
    assert h["emb"]["embed_requests"] >= 4 and h["emb"]["embed_tokens"] >= sum(ec.IN_LENS)
    assert "embed_requests" not in h["plain"]
    # /api/generate cannot make an embedding request
    r = svc.generate("emb", "hi", options={"embed": "mean", "pooling": "mean"})
    assert r.eval_count == 6
    with pytest.raises(NotImplementedError):
        Backend().embed("m", "x")


def test_fake_backend():
    f = FakeBackend()
    a = f.embed("duckdb-nsql", ["one text", "another"])
    assert len(a["embeddings"]) == 2 and all(len(v) == FakeBackend.EMBED_DIM for v in a["embeddings"])
    assert all(abs(sum(x * x for x in v) - 1.0) < 1e-9 for v in a["embeddings"])
    assert f.embed("duckdb-nsql", "one text")["embeddings"][0] == a["embeddings"][0] != a["embeddings"][1]
    assert f.embed("duckdb-nsql", "one text", options={"pooling": "mean"})["embeddings"][0] != a["embeddings"][0]
    for bad in ([], ["x"] * 65, " "):
        with pytest.raises(SamplingOptionError):
            f.embed("duckdb-nsql", bad)
    with pytest.raises(SamplingOptionError):
        f.embed("duckdb-nsql", "x", options={"pooling": "cls"})


class NoEmbed(Backend):
    pass


def test_http_layer(svc, tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context

    def app_for(backend):
        s = Settings(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"),
                     history_dsn="sqlite:///" + str(tmp_path / "h.db"), engine="hip", secret_key="test",
                     nl2sql_model="emb", explain_model="emb", embeddings=True)
        return TestClient(create_app(make_context(s, backend=backend)))

    c = app_for(svc)
    r = c.post("/api/embed", json={"model": "emb", "input": "select 1"})
    assert r.status_code == 200, r.text
    body = r.json()
    assert set(body) == {"model", "embeddings", "total_duration", "load_duration", "prompt_eval_count"}
    assert body["model"] == "emb" and body["prompt_eval_count"] == 9 and len(body["embeddings"]) == 1
    assert body["embeddings"] == svc.embed("emb", "select 1")["embeddings"]
    r = c.post("/api/embed", json={"model": "emb", "input": ["select 1", "select 2 from t"], "options": {"pooling": "mean"}})
    assert r.status_code == 200 and len(r.json()["embeddings"]) == 2
    long = text_of(130)
    r = c.post("/api/embed", json={"model": "emb", "input": long, "options": {"num_ctx": 65}})
    assert r.status_code == 200 and r.json()["prompt_eval_count"] == 64
    assert r.json()["embeddings"] == svc.embed("emb", long[:63])["embeddings"]
    bad = [
        {"model": "emb", "input": long, "truncate": False, "options": {"num_ctx": 65}},
        {"model": "emb", "input": ["x"] * 65},
        {"model": "emb", "input": []},
        {"model": "emb", "input": ""},
        {"model": "emb", "input": "x y", "options": {"pooling": "max"}},
        {"model": "plain", "input": "x y"},
    ]
    for b in bad:
        assert c.post("/api/embed", json=b).status_code == 400, b
    svc.on.runner.tp = types.SimpleNamespace(size=2, rank=0)
    try:
        r = c.post("/api/embed", json={"model": "emb", "input": "x y"})
        assert r.status_code == 400 and "tensor parallelism" in r.text
    finally:
        svc.on.runner.tp = None
    assert app_for(NoEmbed()).post("/api/embed", json={"model": "m", "input": "x"}).status_code == 501
    text = c.get("/metrics").text
    for name in ("lsa_embed_requests_total", "lsa_embed_tokens_total"):
        assert name in text
    assert 'route="api_embed"' in text and "lsa_request_seconds" in text
    assert c.get("/health").json()["engines"]["emb"]["embeddings"] is True

    # RemoteBackend round trip, over the app instead of a socket
    def urlopen(req, timeout=None):
        resp = c.post(req.full_url.replace("http://test", ""), content=req.data, headers=dict(req.header_items()))
        if resp.status_code >= 400:
            raise urllib.error.HTTPError(req.full_url, resp.status_code, "error", {}, io.BytesIO(resp.content))
        return io.BytesIO(resp.content)

    monkeypatch.setattr("urllib.request.urlopen", urlopen)
    rb = RemoteBackend("http://test")
    got = rb.embed("emb", ["select 1", "select 2 from t"], options={"pooling": "mean"})
    assert got["embeddings"] == svc.embed("emb", ["select 1", "select 2 from t"], options={"pooling": "mean"})["embeddings"]
    with pytest.raises(SamplingOptionError):
        rb.embed("emb", "x y", options={"pooling": "max"})
    with pytest.raises(SamplingOptionError):
        rb.embed("emb", long, truncate=False, options={"num_ctx": 65})


def test_flag_from_the_environment_and_the_command_line(monkeypatch):
    assert Settings().embeddings is False
    monkeypatch.setenv("LSA_EMBEDDINGS", "1")
    assert Settings().embeddings is True
    monkeypatch.delenv("LSA_EMBEDDINGS")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--embeddings"])).embeddings is True
    assert Settings.from_cli(ap.parse_args([])).embeddings is False
    # the service factory hands the flag to build_engine
    from llm_based_apache_spark_optimization_amd.serving import service

    seen = {}
    monkeypatch.setattr("llm_based_apache_spark_optimization_amd.engine.build_engine",
                        lambda model, **kw: seen.update(kw) or types.SimpleNamespace(runner=types.SimpleNamespace()))
    s = Settings(embeddings=True, spec_min_accept=-1.0)
    service.engine_factory(s)("duckdb-nsql")
    assert seen["embeddings"] is True
    assert dataclasses.replace(SamplingParams(), embed="mean").embed == "mean"
