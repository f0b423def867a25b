"""fp8 KV cache kernels (ops.KV_FP8) vs the plain-PyTorch reference over the same e4m3 cache
(csrc/kernels/norm_rope.hip rope_append_kernel<., KV8>, attention.hip attn_decode_kernel<., KV8>, kv8.hip), and
the engine at production shapes with kv_dtype="fp8" vs the oracle's fp8-cache emulation."""
import dataclasses
import math

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams
from llm_based_apache_spark_optimization_amd.models import get_spec
from llm_based_apache_spark_optimization_amd.models.llama import init_random, reference_forward
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _paged8(kv_lens, Hkv, device, seed=0):
    """Random e4m3 cache (+ scales) with shuffled block tables; block 0 stays unused (padding rows)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    nb_per = [(n + 63) // 64 for n in kv_lens]
    total = sum(nb_per) + 1
    perm = (torch.randperm(total - 1, generator=g) + 1).tolist()
    bt = torch.zeros(len(kv_lens), max(nb_per) + 1, dtype=torch.int32)
    i = 0
    for s, nb in enumerate(nb_per):
        for j in range(nb):
            bt[s, j] = perm[i]
            i += 1
    mag = torch.logspace(-1, 1, total).view(total, 1, 1, 1)  # per-block magnitudes: the scales matter
    k8, ks = ref.quant_kv_rows(torch.randn(total, Hkv, 64, 128, generator=g) * mag)
    v8, vs = ref.quant_kv_rows(torch.randn(total, Hkv, 64, 128, generator=g) * mag)
    k8, v8 = ref.kv8_physical(k8), ref.kv8_physical(v8)  # the cache's token-pair byte order
    return k8.to(device), v8.to(device), ks.to(device), vs.to(device), bt.to(device)


def _deq_close(k8a, ksa, k8b, ksb, rtol=1e-5):
    """Two e4m3 caches written by different code (fma contraction may flip a rounding): scales equal to f32
    rounding, bytes equal except for rare 1-code flips."""
    assert torch.allclose(ksa, ksb, rtol=rtol, atol=0)
    assert (k8a != k8b).float().mean().item() < 0.01
    assert _rel(ref.dequant_kv_rows(ref.kv8_logical(k8a), ksa), ref.dequant_kv_rows(ref.kv8_logical(k8b), ksb)) < 1e-2


@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
@pytest.mark.parametrize("src", ["bf16", "parts"])
def test_rope_append_fp8(gpu, HH, src):
    H, Hkv = HH
    T, D, nblk = 9, 128, 6
    torch.manual_seed(5)
    cos, sin = ref.rope_tables(D, 512, 10000.0, device=gpu)
    if src == "bf16":
        qkv = torch.randn(T, (H + 2 * Hkv) * D, device=gpu).to(torch.bfloat16)
    else:  # f32 split-K slabs of the decode QKV projection
        qkv = torch.randn(3, T, (H + 2 * Hkv) * D, device=gpu)
    pos = torch.tensor([0, 1, 2, 63, 64, 65, 130, 5, 200], device=gpu, dtype=torch.int32)
    tok_seq = torch.tensor([0, 0, 0, 0, 0, 0, 0, 1, 1], device=gpu, dtype=torch.int32)
    bt = torch.tensor([[2, 4, 5, 0], [1, 3, 0, 0]], device=gpu, dtype=torch.int32)
    out = []
    for fn in (ops.rope_append, ref.rope_append):
        k8 = torch.zeros(nblk, Hkv, 64, D, device=gpu, dtype=torch.uint8)
        v8 = torch.zeros_like(k8)
        ks = torch.zeros(nblk, Hkv, 64, device=gpu)
        vs = torch.zeros_like(ks)
        q = torch.empty(T, H, D, device=gpu, dtype=torch.bfloat16)
        fn(qkv, pos, tok_seq, bt, cos, sin, q, k8, v8, H, Hkv, kv_scales=(ks, vs))
        out.append((q, k8, v8, ks, vs))
    (q, k8, v8, ks, vs), (q2, k82, v82, ks2, vs2) = out
    torch.cuda.synchronize()
    assert _rel(q, q2) < 1e-2
    _deq_close(k8, ks, k82, ks2, rtol=2.0 ** -20)
    _deq_close(v8, vs, v82, vs2, rtol=2.0 ** -20)
    assert ks.count_nonzero().item() == T * Hkv  # exactly the T appended rows per kv head


@pytest.mark.parametrize("HH", [(32, 32), (24, 8), (32, 8), (16, 2)])
@pytest.mark.parametrize("lens", [[1, 63, 64, 65], [700, 5, 2100]])
def test_attn_decode_fp8(gpu, HH, lens):
    H, Hkv = HH
    D = 128
    k8, v8, ks, vs, bt = _paged8(lens, Hkv, gpu, seed=len(lens) + H)
    B = len(lens)
    q = torch.randn(B, H, D, device=gpu).to(torch.bfloat16)
    pos = torch.tensor([n - 1 for n in lens], device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    want = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ref.attn_decode(q, k8, v8, bt, pos, H, Hkv, scale, want, kv_scales=(ks, vs))
    plans = [None, (bt.shape[1], 1), ops.decode_split_plan(B, Hkv, 16384), (1, bt.shape[1], 0)]
    for plan in plans:  # default, single split, long-context grid, one block per split (in-launch combine)
        out = torch.empty_like(want)
        ops.attn_decode(q, k8, v8, bt, pos, H, Hkv, scale, out, plan=plan, kv_scales=(ks, vs))
        assert _rel(out, want) < 1e-2, plan
    xf = torch.zeros(ops.xfrag_tiles(B) * 16 * H * D, device=gpu, dtype=torch.bfloat16)
    ops.attn_decode(q, k8, v8, bt, pos, H, Hkv, scale, xf, xf=True, kv_scales=(ks, vs))
    out = torch.empty_like(want)
    ops.attn_decode(q, k8, v8, bt, pos, H, Hkv, scale, out, kv_scales=(ks, vs))
    assert torch.equal(ops.from_xfrag(xf, B, H * D), out.view(B, -1))


@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
@pytest.mark.parametrize("lens", [[1, 64, 65, 300], [2000]])
@pytest.mark.parametrize("nparts", [1, 3, 8])
def test_attn_decode_fp8_fused_rope(gpu, HH, lens, nparts):
    """RoPE + fp8 KV append fused into decode attention == rope_append then attn_decode (cache and output)."""
    H, Hkv = HH
    D = 128
    k8, v8, ks, vs, bt = _paged8(lens, Hkv, gpu, seed=7)
    B = len(lens)
    pos = torch.tensor([n - 1 for n in lens], device=gpu, dtype=torch.int32)
    cos, sin = ref.rope_tables(D, 4096, 500000.0, device=gpu)
    parts = torch.randn(nparts, B, (H + 2 * Hkv) * D, device=gpu)
    scale = 1 / math.sqrt(D)
    c1 = [t.clone() for t in (k8, v8, ks, vs)]
    q1 = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ops.rope_append(parts, pos, None, bt, cos, sin, q1, c1[0], c1[1], H, Hkv, kv_scales=(c1[2], c1[3]))
    o1 = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ops.attn_decode(q1, c1[0], c1[1], bt, pos, H, Hkv, scale, o1, kv_scales=(c1[2], c1[3]))
    c2 = [t.clone() for t in (k8, v8, ks, vs)]
    o2 = torch.empty_like(o1)
    ops.attn_decode(torch.empty_like(q1), c2[0], c2[1], bt, pos, H, Hkv, scale, o2, qkv_parts=parts, cos=cos,
                    sin=sin, kv_scales=(c2[2], c2[3]))
    torch.cuda.synchronize()
    _deq_close(c2[0], c2[2], c1[0], c1[2])
    _deq_close(c2[1], c2[3], c1[1], c1[3])
    assert _rel(o2, o1) < 1e-2
    # and the output matches the reference over the cache the fused kernel left behind
    want = torch.empty_like(o1)
    ref.attn_decode(q1, c2[0], c2[1], bt, pos, H, Hkv, scale, want, kv_scales=(c2[2], c2[3]))
    assert _rel(o2, want) < 1e-2


def test_kv8_dequant_exact(gpu):
    Hkv = 8
    ctx = [1, 130, 64, 700]
    k8, v8, ks, vs, bt = _paged8(ctx, Hkv, gpu, seed=3)
    cl = torch.tensor(ctx, device=gpu, dtype=torch.int32)
    ko, vo, table = ops.kv8_scratch(ctx, Hkv, gpu)
    ops.ext().kv8_dequant(k8, v8, ks, vs, bt, cl, table.shape[1], ko, vo)
    torch.cuda.synchronize()
    for s, n in enumerate(ctx):
        for j in range((n + 63) // 64):
            b = int(bt[s, j])
            i = int(table[s, j])
            assert torch.equal(ko[i], ref.dequant_kv_rows(ref.kv8_logical(k8[b]), ks[b]).to(torch.bfloat16))
            assert torch.equal(vo[i], ref.dequant_kv_rows(ref.kv8_logical(v8[b]), vs[b]).to(torch.bfloat16))


@pytest.mark.parametrize("kernel", ["16", "32", "32pair"])
@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
@pytest.mark.parametrize("case", ["fresh", "chunked", "long"])
def test_attn_prefill_fp8(gpu, HH, case, kernel, monkeypatch):
    monkeypatch.setattr(ops, "PREFILL_ATTN", kernel[:2])
    monkeypatch.setattr(ops, "PREFILL_PAIR", "1" if kernel == "32pair" else "0")
    H, Hkv = HH
    D = 128
    if case == "fresh":
        qlens, ctx = [1, 70, 130, 64], [1, 70, 130, 64]
    elif case == "chunked":
        qlens, ctx = [10, 64, 100], [200, 64, 400]
    else:
        qlens, ctx = [300, 257], [300, 400]
    k8, v8, ks, vs, bt = _paged8(ctx, Hkv, gpu, seed=H)
    T = sum(qlens)
    q = torch.randn(T, H, D, device=gpu).to(torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0).tolist()), device=gpu, dtype=torch.int32)
    cl = torch.tensor(ctx, device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    out = torch.empty(T, H, D, device=gpu, dtype=torch.bfloat16)
    out2 = torch.empty_like(out)
    ops.attn_prefill(q, k8, v8, bt, cu, cl, H, Hkv, scale, out, kv_scales=(ks, vs))
    ref.attn_prefill(q, k8, v8, bt, cu, cl, H, Hkv, scale, out2, kv_scales=(ks, vs))
    assert _rel(out, out2) < 1e-2


def test_cache_dtype_checked_on_host(gpu):
    k8, v8, ks, vs, bt = _paged8([100], 8, gpu)
    q = torch.randn(1, 8, 128, device=gpu).to(torch.bfloat16)
    pos = torch.tensor([99], device=gpu, dtype=torch.int32)
    out = torch.empty_like(q)
    with pytest.raises(RuntimeError, match="kc"):  # e4m3 bytes without scales
        ops.attn_decode(q, k8, v8, bt, pos, 8, 8, 0.1, out)
    with pytest.raises(RuntimeError, match="scales"):
        ops.attn_decode(q, k8, v8, bt, pos, 8, 8, 0.1, out, kv_scales=(ks[:1], vs[:1]))


_ENG = {}


def _engine(gpu, model, dtype):
    key = (model, dtype)
    if key not in _ENG:
        _ENG.clear()
        torch.cuda.empty_cache()
        spec = dataclasses.replace(get_spec(model), n_layers=2, name=f"{model}-2l")
        w = init_random(spec, gpu, seed=11, kind=dtype)
        runner = ModelRunner(w, max_slots=64, max_model_len=512, use_graphs=True, kv_dtype="fp8")
        _ENG[key] = LLMEngine(runner, name=spec.name)
    return _ENG[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", ["duckdb-nsql", "llama3.2"])
@pytest.mark.parametrize("B", [1, 20, 32])
def test_decode_tokens_kv_fp8_prod_shapes(gpu, model, dtype, B):
    """Production-shape decode (2 layers, captured graphs) with the fp8 cache: every greedy token within the
    test_prod_shapes_gpu margin of the oracle run with the same fp8-cache rounding (and the same W8A8 roundings
    the fp8-weight buckets use)."""
    eng = _engine(gpu, model, dtype)
    r = eng.runner
    assert r.kv.dtype == torch.uint8
    g = torch.Generator().manual_seed(300 + B)
    prompts = [[1] + torch.randint(3, min(r.V, 30000), (int(40 + 13 * i % 170),), generator=g).tolist()
               for i in range(B)]
    res = eng.generate(prompts, SamplingParams(max_tokens=12, ignore_eos=True))
    rows = sum(len(q) for q in prompts)
    bk = r.bucket(B)
    plan = r.oracle_plan(bk)
    worst = 0.0
    for p, out in zip(prompts, res[: min(B, 6)]):
        lg = reference_forward(r.w, p + out.token_ids[:-1], act_quant_rows=len(p) if rows > 64 else 0,
                               decode_a8=plan, kv_fp8=True)[len(p) - 1:]
        chosen = lg.gather(1, torch.tensor(out.token_ids, device=lg.device).view(-1, 1)).squeeze(1)
        worst = max(worst, ((lg.max(1).values - chosen) / lg.std(1)).max().item())
    assert worst < 0.15, (model, dtype, B, worst)
