"""Speculative decoding with fp8 / MXFP4 weights and the fp8 KV cache on the GPU (``spec_quantized``): attn_verify over
the e4m3 cache against the reference, and the engine's verify steps (weight-only GEMMs, captured graphs) against
their own oracle plan and threshold class."""
import dataclasses

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams
from llm_based_apache_spark_optimization_amd.eval import numerics as nm
from llm_based_apache_spark_optimization_amd.models import get_spec
from llm_based_apache_spark_optimization_amd.models.llama import init_random, reference_forward
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_cpu import K, PROMPT, SYSTEM, forced_table
from test_spec_gpu import _rel, equal_up_to_margin, gen, make, prompt_ids

pytestmark = pytest.mark.gpu

I32 = dict(dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ attn_verify
@pytest.mark.parametrize("H,Hkv", [(32, 32), (24, 8), (32, 8)])
@pytest.mark.parametrize("pos0", [0, 62, 63, 700, 2100])
def test_attn_verify_fp8_matches_decode_reference(gpu, H, Hkv, pos0):
    """attn_verify(kv_scales=) == ref.attn_decode(kv_scales) called per row with pos = pos0 + t, over the e4m3 cache
    after rope_append(kv_scales=) of the T rows; the shapes of test_attn_verify_matches_decode_reference.  pos0 = 62 /
    63 also put the first new token on the even / odd half of a token pair.  The whole arena holds finite random e4m3
    rows with positive scales (no NaN codes)."""
    G = H // Hkv
    D, MB = 128, 40
    g = torch.Generator().manual_seed(1000 * H + pos0)
    nblocks = MB + 3
    k8, ks = ref.quant_kv_rows(torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5)
    v8, vs = ref.quant_kv_rows(torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5)
    assert ((k8 & 0x7F) != 0x7F).all() and ((v8 & 0x7F) != 0x7F).all() and (ks > 0).all() and (vs > 0).all()
    k8, v8 = ref.kv8_physical(k8).contiguous().to(gpu), ref.kv8_physical(v8).contiguous().to(gpu)
    ks, vs = ks.contiguous().to(gpu), vs.contiguous().to(gpu)
    bt = (torch.randperm(nblocks - 1, generator=g)[:MB] + 1).to(torch.int32).view(1, MB).to(gpu)
    cos, sin = ref.rope_tables(D, MB * 64, 10000.0, None, device=gpu)
    scale = D ** -0.5
    for T in sorted({2, 4, min(8, 16 // G)}):
        if T * G > 16:
            continue
        qkv = (torch.randn(T, (H + 2 * Hkv) * D, generator=g) * 0.7).to(torch.bfloat16).to(gpu)
        pos = torch.arange(pos0, pos0 + T, **I32).to(gpu)
        q = torch.zeros(T, H, D, dtype=torch.bfloat16, device=gpu)
        ops.rope_append(qkv, pos, torch.zeros(T, **I32).to(gpu), bt, cos, sin, q, k8, v8, H, Hkv, kv_scales=(ks, vs))
        want = torch.zeros(T, H, D, dtype=torch.bfloat16, device=gpu)
        ref.attn_decode(q, k8, v8, bt.expand(T, MB), pos, H, Hkv, scale, want, kv_scales=(ks, vs))
        nblk = (pos0 + T + 63) // 64
        plans = {"default": None, "unsplit": (nblk, 1), "one_block_per_split": (1, nblk, 0),
                 "16k": ops.verify_split_plan(Hkv, 16384)}
        for name, plan in plans.items():
            out = torch.full((T, H * D), 7.0, dtype=torch.bfloat16, device=gpu)
            ops.attn_verify(q, k8, v8, bt, pos[:1], H, Hkv, scale, out, plan=plan, kv_scales=(ks, vs))
            assert torch.isfinite(out.float()).all(), (T, name)
            e = _rel(out.view(T, H, D), want)
            assert e < 1e-2, (T, name, e)
            for t in range(T):  # per row too: a wrong causal limit on one row hides in the whole-tensor norm
                assert _rel(out.view(T, H, D)[t], want[t]) < 1e-2, (T, name, t)
            out2 = torch.zeros_like(out)
            ops.attn_verify(q, k8, v8, bt, pos[:1], H, Hkv, scale, out2, plan=plan, kv_scales=(ks, vs))
            assert torch.equal(out, out2), (T, name)


def test_attn_verify_checks_cache_dtype_against_scales(gpu):
    k8 = torch.zeros(3, 8, 64, 128, dtype=torch.uint8, device=gpu)
    ks = torch.ones(3, 8, 64, device=gpu)
    kb = torch.zeros(3, 8, 64, 128, dtype=torch.bfloat16, device=gpu)
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16, device=gpu)
    out = torch.zeros(2, 8 * 128, dtype=torch.bfloat16, device=gpu)
    bt = torch.tensor([[1, 2]], **I32).to(gpu)
    pos = torch.zeros(1, **I32).to(gpu)
    with pytest.raises(RuntimeError):
        ops.attn_verify(q, k8, k8, bt, pos, 8, 8, 0.1, out)  # e4m3 bytes without scales
    with pytest.raises(RuntimeError):
        ops.attn_verify(q, kb, kb, bt, pos, 8, 8, 0.1, out, kv_scales=(ks, ks))  # scales with the bf16 cache


# ------------------------------------------------------------------------------------------------ engine
CONFIGS = [("fp8", "bf16"), ("fp8", "fp8"), ("mxfp4", "bf16"), ("bf16", "fp8"), ("mxfp4", "fp8")]
GATED = CONFIGS[:3]  # the configurations tests/test_numerics_gpu.py gates for the plain path


def qmake(gpu, model, dtype, kv, **kw):
    return make(gpu, model, dtype=dtype, kv_dtype=kv, spec_tokens=K, spec_quantized=True, **kw)


@pytest.mark.parametrize("dtype,kv", CONFIGS)
@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_verify_steps_self_consistent_and_numerics(gpu, model, dtype, kv):
    """Exact by construction, per recorded step: the committed tokens are the argmax of verify rows 0 .. a, drafts
    0 .. a - 1 equal those argmaxes, and draft a does not (or a = k).  No plain step runs while the window has room.
    Then the verify rows against the oracle under the verify plan and class over >= 64 tokens: asserted for the
    configurations whose plain path tests/test_numerics_gpu.py gates; for the other two only if the plain engine of the
    same configuration passes its own check here (their thresholds are otherwise uncalibrated for that cache)."""
    eng = qmake(gpu, model, dtype, kv)
    assert eng.runner.spec_supported()
    k = eng.runner.spec_k()
    ids = prompt_ids(eng)
    toks, elog, steps = nm.record_spec_logits(eng, ids, 64)
    assert len(toks) == 65 and sum(s["spec"] for s in steps) >= 8
    for s in steps:
        if not s["spec"]:
            continue
        c, am, dr = s["committed"], s["row_argmax"], s["draft"]
        assert toks[s["first"]:s["first"] + c] == am[:c]
        assert dr[:c - 1] == am[:c - 1]
        if s["first"] + c < 65:  # not truncated by the length limit
            assert c - 1 == k or dr[c - 1] != am[c - 1]
    good = nm.check_recorded(eng, [ids], [toks], elog, 64, (0,), spec_steps=steps)
    print({"good": good})
    assert good["plain_tokens_skipped"] == 0 and good["tokens_checked"] >= 64, good
    assert good["class"] == nm.spec_numerics_class(eng.runner)
    if (dtype, kv) in GATED:
        assert good["ok"], good
    else:
        peng = make(gpu, model, dtype=dtype, kv_dtype=kv)
        pgood = nm.teacher_forced_check(peng, [ids], 64)
        print({"plain": pgood})
        if pgood["ok"]:
            assert good["ok"], (good, pgood)
    if model == "tiny-llama3":
        assert good["tied_head"], good


@pytest.mark.parametrize("base,dtype,kv", [("duckdb-nsql", "fp8", "fp8"), ("llama3.2", "mxfp4", "bf16")])
def test_spec_numerics_check_catches_kv_fault(gpu, base, dtype, kv):
    """Production widths, 4 layers (test_spec_gpu.py::test_spec_numerics_check_catches_kv_fault): the verify steps pass
    their criterion over 64 committed tokens and fail it with a swapped key pair in the cache layout (the fault moves
    the fp8 cache's per-token scales with their rows)."""
    spec = dataclasses.replace(get_spec(base), n_layers=4, name=base + "-4l")
    r = ModelRunner(init_random(spec, gpu, seed=5, kind=dtype), max_slots=2, max_model_len=512, num_kv_blocks=17,
                    kv_dtype=kv, spec_tokens=K, spec_quantized=True)
    eng = LLMEngine(r, name=spec.name)
    g = torch.Generator().manual_seed(3)
    ids = [1] + torch.randint(3, 30000, (100,), generator=g).tolist()
    good = nm.teacher_forced_check_spec(eng, ids, 64)
    print({"good": good})
    assert good["ok"] and good["tokens_checked"] >= 64 and good["verify_steps"] >= 16, good
    assert good["plain_tokens_skipped"] == 0, good
    truth = init_random(spec, gpu, seed=5, kind=dtype)
    with nm.kv_swap_fault(eng):
        bad = nm.teacher_forced_check_spec(eng, ids, 64, weights=truth)
    print({"bad_kv": bad})
    assert not bad["ok"], (good, bad)


def test_engine_forced_drafts(gpu):
    """Planted drafts, MXFP4 weights with the fp8 cache: the tokens are the verify path's own greedy tokens whatever is
    drafted (all runs take the same verify kernels, so they agree exactly), and the acceptance counts are exact."""
    base = qmake(gpu, "tiny-nsql", "mxfp4", "fp8")
    want = gen(base)
    assert base.stats["spec_steps"] > 0
    for kind, per_step in (("right", K), ("wrong", 0), ("first", 1)):
        eng = qmake(gpu, "tiny-nsql", "mxfp4", "fp8")
        eng.runner.set_spec_forced(forced_table(want, kind, eng.runner.V))
        assert gen(eng) == want, kind
        steps = -(-95 // (per_step + 1))
        assert eng.stats["spec_steps"] == steps and eng.stats["spec_accepted"] == 95 - steps, kind
        assert eng.stats["spec_drafted"] == K * steps, kind


def test_engine_graph_replay_and_mixed_runs(gpu):
    """fp8 weights with the fp8 cache: the verify step replays from a captured graph; a repeated run is identical; a
    request that opts out adds no verify steps and decodes the plain engine's tokens."""
    eng = qmake(gpu, "tiny-nsql", "fp8", "fp8")
    r = eng.runner
    assert r.use_graphs
    a = gen(eng, 48)
    assert any(key[0] == "spec" for key in r.graphs), list(r.graphs)
    assert gen(eng, 48) == a
    sp_off = SamplingParams(max_tokens=48, ignore_eos=True, speculate=False)
    s0 = eng.stats["spec_steps"]
    assert s0 > 0
    p1 = eng.generate([PROMPT], sp_off, system=SYSTEM)[0].token_ids
    assert eng.stats["spec_steps"] == s0
    assert gen(eng, 48) == a
    assert p1 == gen(make(gpu, dtype="fp8", kv_dtype="fp8"), 48)  # the engine's plain path is the plain engine's


def test_production_shape_3b_fp8_cache(gpu):
    """Llama-3.2-3B shape (GQA 3:1), 2 layers, a 2048-token prompt, the fp8 cache with bf16 weights, 32 tokens with
    forced all-right drafts at k = 3: equal to the plain fp8-cache run under the margin rule of
    test_spec_gpu.py::test_production_shape_3b (both values printed)."""
    spec = dataclasses.replace(get_spec("llama3.2"), n_layers=2, name="llama3.2-2l")
    w = init_random(spec, gpu, seed=5)
    g = torch.Generator().manual_seed(9)
    ids = [1] + torch.randint(3, 30000, (2047,), generator=g).tolist()
    sp = SamplingParams(max_tokens=32, ignore_eos=True)
    kw = dict(max_slots=2, max_model_len=2304, num_kv_blocks=80, kv_dtype="fp8")
    peng = LLMEngine(ModelRunner(w, **kw), name=spec.name)
    toks = peng.generate([ids], sp)[0].token_ids
    rtoks, elog = nm.record_decode_logits(peng, [ids], 31, hidden=False)
    lg = reference_forward(w, ids + toks[:31])[len(ids):len(ids) + 31].float()
    top2 = lg.topk(2, -1).values
    margins = (top2[:, 0] - top2[:, 1]).tolist()
    bound = 10.0 * (elog[0].float() - lg.to(elog.device)).abs().max().item()
    eng = LLMEngine(ModelRunner(w, spec_tokens=3, spec_quantized=True, **kw), name=spec.name)
    eng.runner.set_spec_forced(forced_table(toks, "right", spec.vocab_size))
    got = eng.generate([ids], sp)[0].token_ids
    ok, n = equal_up_to_margin(got, toks, margins, bound)
    print({"min_margin": min(margins), "bound_10x_max_logit_diff": bound, "compared_tokens": n + 1})
    assert ok, (got, toks, n)
    assert eng.stats["spec_steps"] > 0
