"""Embeddings on the GPU: the three kernels of csrc/kernels/embed.hip under the checks of embed_cases.py (bit-equal to
the host twins for the same row scales, chunk invariance on the device, the float64 bounds, the untouched-words rule,
the refusals), the engine's vectors against the float64 oracle with bf16 and fp8 weights, and the captured engine
against the twins applied to what the runner passed to the ops.  The CPU twins are test_embed_cpu.py.

The worst measured error / bound ratios are kept in profiles/embed/embed_exact_mi355x.json (written when
LSA_EMBED_EXACT_OUT names a file)."""
import json
import os

import pytest
import torch

import embed_cases as ec
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.eval import numerics
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

KW = dict(max_slots=8, max_model_len=512)
INPUTS = [ec.input_ids(n, k=k) for k, n in enumerate(ec.IN_LENS)]


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("LSA_EMBED_EXACT_OUT")
    if path and ec.RATIOS:
        with open(path, "w") as f:
            json.dump({"unit": "measured error / bound, worst case (rowscale: |rs - exact| / ((c + 6) 2^-24 exact); "
                               "finish: |out - e| / ((c + 6) 2^-24 |e|); oracle: ||e - e_o|| / (2 kappa rel_max))",
                       "device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
                       "worst": {k: round(v, 4) for k, v in sorted(ec.RATIOS.items())}}, f, indent=1)
            f.write("\n")


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_rowscale_against_float64(gpu, D, nslab):
    ec.check_rowscale(D, nslab, gpu)


@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_pool_bit_equal_to_twin(gpu, D, nslab):
    ec.check_pool(D, nslab, gpu)


@pytest.mark.parametrize("nslab", ec.SLABS)
@pytest.mark.parametrize("D", ec.DS)
def test_chunk_invariance_on_the_device(gpu, D, nslab):
    ec.check_chunk_invariance(D, nslab, gpu)


@pytest.mark.parametrize("nslab", (0, 3))
@pytest.mark.parametrize("D", ec.DS)
def test_last(gpu, D, nslab):
    ec.check_last(D, nslab, gpu)


@pytest.mark.parametrize("D", ec.DS)
def test_finish_against_float64(gpu, D):
    ec.check_finish(D, gpu)


def test_refusals(gpu):
    ec.check_refusals(gpu)


# ------------------------------------------------------------------------------------------------ the engine
def embed_many(e, inputs, pooling):
    reqs = [e.add_request(ids, SamplingParams(embed=pooling)) for ids in inputs]
    e.run_until_done(reqs)
    return [e.result(q) for q in reqs]


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_against_the_float64_oracle(gpu, model, dtype):
    """||e - e_o||_2 <= 2 kappa rel_max per input and pooling (embed_cases.oracle_vector).  rel_max is the hidden-state
    bound of eval/numerics.py for the class of the prefill that made the rows: fp8 weights run an input of more than 64
    rows W8A8 (the oracle rounds its activations per token too: act_quant_rows), class w8a8; otherwise the runner's
    batch-1 class."""
    e = build_engine(model, device=str(gpu), dtype=dtype, embeddings=True, **KW)
    r = e.runner
    nl = len(r.w.layers)
    for pooling in ("mean", "last"):
        for ids in INPUTS:
            got = torch.tensor(embed_many(e, [ids], pooling)[0].embedding, dtype=torch.float64)
            assert abs(float(got.norm()) - 1.0) < 2.0 ** -20
            aq = len(ids) if (dtype == "fp8" and len(ids) > 64 and ops.FP8_W8A8) else 0
            cls = "w8a8" if aq else numerics.numerics_class(r, 1)
            rel_max = numerics.hidden_rel_max(cls, nl)
            e_o, kappa = ec.oracle_vector(r.w, ids, pooling, act_quant_rows=aq, kv_fp8=r.kv_fp8)
            ratio = float((got - e_o).norm()) / (2 * kappa * rel_max)
            print(f"{model} {dtype} {pooling} {len(ids)} tokens ({cls}): error / bound = {ratio:.4f} (kappa {kappa:.2f})")
            ec.note(f"oracle_{model}_{dtype}_{pooling}_{len(ids)}", ratio)
            assert ratio <= 1.0


def _capture(monkeypatch, log):
    """Wrap the three ops entry points: keep host copies of what the runner passed (rs as the device wrote it)."""
    rowscale, pool, finish = ops.embed_rowscale, ops.embed_pool, ops.embed_finish

    def w_rowscale(h, parts, tseq, cu, meta, eps, rs, host=None):
        rowscale(h, parts, tseq, cu, meta, eps, rs, host=host)
        torch.cuda.synchronize()
        log.append(dict(h=h.cpu().clone(), parts=None if parts is None else parts.cpu().clone(), cu=list(host[0]),
                        meta=[list(x) for x in host[1]], rs=rs.cpu().clone(), dev_meta=meta.cpu().tolist(),
                        dev_cu=cu.cpu().tolist()))

    def w_pool(h, parts, cu, meta, rs, gamma, acc, host=None):
        log[-1]["gamma"] = gamma.cpu().clone()
        pool(h, parts, cu, meta, rs, gamma, acc, host=host)

    def w_finish(meta, acc, out, host=None):
        log[-1]["finished"] = True
        finish(meta, acc, out, host=host)

    monkeypatch.setattr(ops, "embed_rowscale", w_rowscale)
    monkeypatch.setattr(ops, "embed_pool", w_pool)
    monkeypatch.setattr(ops, "embed_finish", w_finish)


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_captured_engine_against_the_twins(gpu, model, monkeypatch):
    """A captured engine with chunked prefill (chunks of 64 rows take the split-K GEMMs: the pool sums their slabs):
    every vector equals, bit for bit, the pool and finish twins run over the rows, slabs and row scales that the runner
    handed to the ops, call after call; the transfer's meta words are what the host built."""
    e = build_engine(model, device=str(gpu), embeddings=True, prefill_chunk=64, **KW)
    r = e.runner
    assert r.use_graphs and r.embeddings
    log: list = []
    _capture(monkeypatch, log)
    acc_t = torch.zeros(r.max_slots, r.d)
    out_t = torch.zeros(r.max_slots, r.d)
    slabs = 0
    for pooling, inputs in (("mean", [INPUTS[3]]), ("last", [INPUTS[3]]), ("mean", INPUTS), ("last", INPUTS[:2])):
        del log[:]
        reqs = [e.add_request(ids, SamplingParams(embed=pooling)) for ids in inputs]
        slots = {}
        while not all(q.done.is_set() for q in reqs):
            e.step()
            for q in reqs:
                if q.slot >= 0:
                    slots[q.rid] = q.slot
        assert log and all(c.get("finished") and "gamma" in c for c in log)
        slabs += sum(c["parts"].shape[0] for c in log if c["parts"] is not None)
        for c in log:
            assert c["dev_meta"] == c["meta"] and c["dev_cu"] == c["cu"]
            ref.embed_pool(c["h"], c["parts"], c["cu"], c["meta"], c["rs"], c["gamma"], acc_t)
            ref.embed_finish(c["meta"], acc_t, out_t)
        for q in reqs:
            assert ec.same_bits(q.embedding, out_t[slots[q.rid]]), (pooling, len(q.prompt_ids))
    assert slabs > 0, "no call handed split-K slabs to the pool"


def test_decode_graphs_and_kernel_counts_unchanged(gpu):
    """With embeddings enabled, and even after embedding requests ran, the decode graph keys and the kernels per
    decode step are those of an engine without; and the generated tokens are the same."""
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    prompts = [ec.input_ids(40, k=9), ec.input_ids(33, k=4)]

    def gen(e):
        reqs = [e.add_request(p, sp) for p in prompts]
        e.run_until_done(reqs)
        return [q.output_ids for q in reqs]

    off = build_engine("tiny-nsql", device=str(gpu), **KW)
    on = build_engine("tiny-nsql", device=str(gpu), embeddings=True, **KW)
    want = gen(off)
    embed_many(on, INPUTS[:2], "mean")
    assert gen(on) == want
    assert set(on.runner.graphs) == set(off.runner.graphs) and on.runner.graphs
    for B in (1, 2, 8):
        for sample in (False, True):
            assert on.runner.count_step_kernels(B, sample) == off.runner.count_step_kernels(B, sample)
