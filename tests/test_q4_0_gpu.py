"""GGUF Q4_0 on the GPU (csrc/kernels/gemm_q4.hip): the dequant kernel against the value rule, value for value (torch.equal:
the kernels write a zero as +0 where the rule's product can be -0), the decode
GEMM exact on every element over data whose sums are exact in f32, the SiLU epilogue and random data under the
project's tolerance for this class of kernel, the refusals, the two-stream prefill scratch, and q4_0 engines against
their fp32 oracle."""
import math

import pytest
import torch

import gguf_cases as gc
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.eval import numerics as nm
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(16, 128), (48, 384), (96, 1408)]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-12))


@pytest.mark.parametrize("N,K", [(96, 1408), (16, 128)])  # K / 128 = 11: the last scale word is half used
def test_q4_dequant_kernel_exact(gpu, N, K):
    g = torch.Generator().manual_seed(N)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    d = (torch.randn(N, K // 32, generator=g) * 0.02).to(torch.float16)
    edge = torch.tensor(gc.EDGE_SCALES).to(torch.float16)
    d.view(-1)[: edge.numel()] = edge          # zero, negative, subnormal, 65504 ...
    d.view(-1)[-edge.numel():] = edge          # ... in the first and in the last rows
    pw = ops.PackedWeight.from_q4_0(codes.to(gpu), d.to(gpu))
    assert pw.kind == "q4_0" and pw.nbytes == N * K // 2 + (N // 16) * ((K // 128 + 1) // 2) * 256
    buf = torch.full((N * K + 64,), 7.0, device=gpu, dtype=torch.bfloat16)
    ops.ext().q4_dequant(pw.data, pw.scale, N, K, buf)
    want = ops.dequantize_q4_0(pw.data, pw.scale, N, K)
    rule = (d.float()[..., None] * (codes.view(N, K // 32, 32).float() - 8.0)).to(torch.bfloat16).float().view(N, K)
    assert torch.equal(want.cpu(), rule)
    assert torch.equal(ops.unshuffle_weight(buf[: N * K], N, K).float(), want)
    assert bool((buf[N * K:] == 7.0).all())
    assert torch.equal(pw.dense().float(), want)


_exact = {}


def _exact_case(gpu, N, K):
    """(x [64, K] integers in [-4, 4], the packed weight, the f64 product [64, N]) -- made once per shape.  Scales are
    powers of two that differ per row and per block, so every product and partial sum is exact in f32."""
    if (N, K) not in _exact:
        g = torch.Generator().manual_seed(N * 7 + K)
        x = torch.randint(-4, 5, (64, K), generator=g).to(torch.bfloat16).to(gpu)
        codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8).to(gpu)
        row = torch.arange(N, device=gpu)[:, None]
        blk = torch.arange(K // 32, device=gpu)[None, :]
        d = torch.exp2(-2.0 - ((row + 3 * blk) % 5).float()).to(torch.float16)
        pw = ops.PackedWeight.from_q4_0(codes, d)
        w64 = d.double()[..., None] * (codes.view(N, K // 32, 32).double() - 8.0)
        _exact[(N, K)] = (x, pw, x.double() @ w64.view(N, K).t())
    return _exact[(N, K)]


def _variants(M):
    """Every (nb, waves) the launcher instantiates at M's row-tile count, and one nb it has no kernel for (6 -> 2)."""
    nbs = (1, 2) if M > 32 else (1, 2, 4, 8, 6)
    return [(nb, wv) for nb in nbs for wv in (4, 8)]


@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64])
def test_q4_gemm_exact_on_every_element(gpu, M):
    SENT = -1232.0  # a bf16 value
    for N, K in SHAPES:  # N / 16 = 1, 3, 6: nb 2, 4, 8 make ragged grids of them
        x64, pw, y64 = _exact_case(gpu, N, K)
        x, want = x64[:M].contiguous(), y64[:M]
        xf = ops.to_xfrag(x)
        for nb, waves in _variants(M):
            for epi, sk in (("f32", 1), ("f32", 2), ("f32", 4), ("bf16", 1)):
                for frag in (False, True):
                    outs = []
                    for _ in range(2):
                        flat = torch.full(((sk + 1) * M * N + 16 * N,), SENT, device=gpu,
                                          dtype=torch.float32 if epi == "f32" else torch.bfloat16)
                        if frag:
                            ops.linear_xf(xf, M, pw, epi, out=flat, splitk=sk, nb=nb, waves=waves)
                        else:
                            ops.linear(x, pw, epi, out=flat, splitk=sk, nb=nb, waves=waves)
                        outs.append(flat)
                    tag = (M, N, K, nb, waves, epi, sk, frag)
                    assert torch.equal(outs[0], outs[1]), tag
                    y = outs[0][: sk * M * N].view(sk, M, N)
                    if epi == "f32":
                        assert torch.equal(y.sum(0).double(), want), tag
                    else:
                        assert torch.equal(y[0], want.to(torch.bfloat16)), tag
                    assert bool((outs[0][sk * M * N:] == SENT).all()), tag  # rows >= M, slabs >= splitk


@pytest.mark.parametrize("M", [1, 20, 64, 130])
@pytest.mark.parametrize("epi", ["bf16", "f32", "silu"])
def test_q4_gemm(gpu, M, epi):
    N, K = 1024, 4096
    torch.manual_seed(M)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w, "q4_0")
    assert pw.kind == "q4_0"
    wd = ops.dequantize_q4_0(pw.data, pw.scale, N, K)
    # sanity of the quantiser, not of the kernel: step d = max / 8 ~ 0.26 sigma for 32 normal values, so an rms error of
    # d / sqrt(12) ~ 0.08 sigma plus the clipped top code
    assert _rel(wd, w) < 0.15
    yr = ref.linear(x, wd, epi)
    for nb, sk, waves in ((1, 1, 4), (2, 2, 8), (4, 4, 4), (8, 1, 4), (4, 1, 8)):
        if epi != "f32" and sk > 1:
            sk = 1
        if epi == "silu" and nb < 2:
            nb = 2
        y = ops.linear(x, pw, epi, splitk=sk, nb=nb, waves=waves)
        if epi == "f32":
            y = y.sum(0)
        assert _rel(y, yr) < 1e-2, (M, epi, nb, sk, waves)
        if M <= 64:  # fragment-major activations (the decode path at B > 16)
            yx = ops.linear_xf(ops.to_xfrag(x), M, pw, epi, splitk=sk, nb=nb, waves=waves)
            if epi == "f32":
                yx = yx.sum(0)
            elif epi == "silu":
                yx = ops.from_xfrag(yx, M, N // 2)
            assert _rel(yx, yr) < 1e-2, (M, epi, nb, sk, waves, "xf")
    if M <= 64 and epi == "f32":  # the row scale that comes with the skeleton's epilogue
        ss = ops.ss_q24(x.float().pow(2).sum(1))
        y = ops.linear(x, pw, "f32", splitk=1, rownorm=(ss, 1e-5))[0]
        xs = x.float() * torch.rsqrt(x.float().pow(2).sum(1, keepdim=True) / K + 1e-5)
        assert _rel(y, xs @ wd.t()) < 1e-2


def test_q4_refusals_raise_before_any_launch(gpu):
    N, K = 32, 256
    pw = ops.PackedWeight.from_q4_0(torch.randint(0, 16, (N, K), dtype=torch.uint8, device=gpu),
                                    torch.full((N, K // 32), 0.5, dtype=torch.float16, device=gpu))
    x = torch.ones(4, K, device=gpu, dtype=torch.bfloat16)
    e = ops.ext()

    def untouched(fn, out, rc=None):
        """fn raises -- with the launcher's own error code where it is the launcher that refuses -- and writes nothing"""
        with pytest.raises((RuntimeError, ValueError), match=f"rc={rc}$" if rc is not None else None):
            fn(out)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())

    f32 = lambda n: torch.full((n,), 3.0, device=gpu)  # noqa: E731
    b16 = lambda n: torch.full((n,), 3.0, device=gpu, dtype=torch.bfloat16)  # noqa: E731
    # K not a multiple of 128, N not a multiple of 16: lsa_q4_gemm_ex returns -1
    bad_k = ops.PackedWeight(N, 192, "q4_0", pw.data, pw.scale)
    x192 = torch.ones(4, 192, device=gpu, dtype=torch.bfloat16)
    untouched(lambda o: ops.linear(x192, bad_k, "f32", out=o, splitk=1), f32(4 * N), -1)
    bad_n = ops.PackedWeight(24, K, "q4_0", pw.data, pw.scale)
    untouched(lambda o: ops.linear(x, bad_n, "f32", out=o, splitk=1), f32(4 * N), -1)
    untouched(lambda o: ops.linear_xf(ops.to_xfrag(x), 4, bad_n, "f32", out=o, splitk=1), f32(4 * N), -1)
    # M = 0, and M > 64 into the skinny entry point: -1
    untouched(lambda o: ops.linear(x[:0], pw, "f32", out=o, splitk=1), f32(4 * N), -1)
    x65 = torch.ones(65, K, device=gpu, dtype=torch.bfloat16)
    untouched(lambda o: e.q4_gemm(x65, pw.data, pw.scale, N, o, ops.EPI["f32"], 1, 1, 4), f32(65 * N), -1)
    untouched(lambda o: e.q4_gemm_xf(ops.to_xfrag(x65[:64]), 65, K, pw.data, pw.scale, N, o, ops.EPI["f32"], 1, 1, 4),
              f32(65 * N), -1)
    # split-K with an epilogue that is not f32 slabs: -3
    untouched(lambda o: ops.linear(x, pw, "bf16", out=o, splitk=2), b16(2 * 4 * N), -3)
    untouched(lambda o: ops.linear(x, pw, "silu", out=o, splitk=2), b16(2 * 4 * N), -3)
    untouched(lambda o: ops.linear_xf(ops.to_xfrag(x), 4, pw, "bf16", out=o, splitk=2), b16(2 * 4 * N), -3)
    # a grid the nb that would run cannot cover: nb 3 has no kernel and runs as nb 2, whose SiLU pairs do not tile an
    # odd number of n-blocks: -2
    pw48 = ops.PackedWeight.from_q4_0(torch.randint(0, 16, (48, K), dtype=torch.uint8, device=gpu),
                                      torch.full((48, K // 32), 0.5, dtype=torch.float16, device=gpu))
    untouched(lambda o: ops.linear(x, pw48, "silu", out=o, nb=3), b16(4 * 48), -2)
    # no residual epilogue for this kind; buffers that do not match the shape (the bindings' own checks)
    h, so = torch.zeros(4, N, device=gpu), torch.zeros(4, device=gpu, dtype=torch.int64)
    with pytest.raises((RuntimeError, ValueError)):
        ops.linear(x, pw, "res", res=(h, b16(4 * N), so))
    untouched(lambda o: e.q4_gemm(x, pw.data[:1], pw.scale, N, o, ops.EPI["f32"], 1, 1, 4), f32(4 * N))
    untouched(lambda o: e.q4_gemm(x, pw.data, pw.scale[:1], N, o, ops.EPI["f32"], 1, 1, 4), f32(4 * N))
    untouched(lambda o: e.q4_dequant(pw.data, pw.scale, N, K, o), b16(N * K - 1))


def test_q4_prefill_two_streams_match_serial(gpu):
    """Co-served engines prefill on their own streams: each stream has its own dequant scratch, so interleaved
    prefill GEMMs of two different q4_0 models give the results of serial runs."""
    torch.manual_seed(3)
    M, K = 256, 2048
    wa = ops.PackedWeight.from_dense(torch.randn(2048, K, device=gpu) / math.sqrt(K), "q4_0")
    wb = ops.PackedWeight.from_dense(torch.randn(4096, K, device=gpu) / math.sqrt(K), "q4_0")  # regrows the scratch
    xa = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    xb = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    ya0, yb0 = ops.linear(xa, wa, "bf16"), ops.linear(xb, wb, "bf16")
    assert _rel(ya0, ref.linear(xa, wa.dense().float(), "bf16")) < 1e-2
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(sa):
            ya = ops.linear(xa, wa, "bf16")
        with torch.cuda.stream(sb):
            yb = ops.linear(xb, wb, "bf16")
        outs.append((ya, yb))
    torch.cuda.synchronize()
    for ya, yb in outs:
        assert torch.equal(ya, ya0) and torch.equal(yb, yb0)


def _prompts(eng, batch):
    g = torch.Generator().manual_seed(batch)
    return [[1] + torch.randint(3, eng.spec.vocab_size, (30 + 3 * i,), generator=g).tolist() for i in range(batch)]


def _check_engine(eng, batches):
    r = eng.runner
    assert r.w.layers[0].wqkv.kind == "q4_0" and not r.w.layers[0].norms_folded
    assert not r.fused_norm and not r.wide_norm and not r.rr_decode and not r.a8 and not r.spec_supported()
    for batch in batches:  # 2: the row-major step; 20: the fragment-major step
        assert r.use_xfrag(r.bucket(batch)) == (batch > 16)
        prompts = _prompts(eng, batch)
        res = nm.teacher_forced_check(eng, prompts, 32, check_rows=(0, batch - 1))
        assert res["ok"] and res["class"] == "bf16", res
    out = eng.generate(_prompts(eng, 2), SamplingParams(max_tokens=8, ignore_eos=True))
    assert [o.eval_count for o in out] == [8, 8]


def test_q4_0_engines(gpu, tmp_path):
    kw = dict(device=str(gpu), max_slots=32, max_model_len=512)
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    bf = build_engine("tiny-nsql", dtype="bf16", seed=1, **kw)
    prompts = _prompts(bf, 2)
    want = [r.token_ids for r in bf.generate(prompts, sp)]
    keys = set(bf.runner.graphs)
    counts = {(B, s): bf.runner.count_step_kernels(B, s) for B in (1, 2, 8) for s in (False, True)}
    assert keys

    p = tmp_path / "nsql.gguf"
    gc.build_checkpoint(p, "tiny-nsql", output="Q6_K")
    eng = build_engine("tiny-nsql", checkpoint=str(p), dtype="q4_0", **kw)
    assert eng.runner.w.lm_head.kind == "bf16" and eng.runner.w.source["tensor_types"]["Q4_0"] == 15
    _check_engine(eng, (2, 20))
    cpu = build_engine("tiny-nsql", device="cpu", checkpoint=str(p), dtype="q4_0", max_slots=4, max_model_len=512)
    for a, b in zip(eng.runner.w.layers, cpu.runner.w.layers):  # the GPU engine holds the file's values
        for x, y in ((a.wqkv, b.wqkv), (a.wo, b.wo), (a.w_gate_up, b.w_gate_up), (a.w_down, b.w_down)):
            assert torch.equal(x.dense().cpu(), y.dense())
    del eng, cpu

    rnd = build_engine("tiny-nsql", dtype="q4_0", seed=1, **kw)  # no file: quantised on load, the head too
    assert rnd.runner.w.lm_head.kind == "q4_0"
    _check_engine(rnd, (2, 20))
    del rnd

    p3 = tmp_path / "l3.gguf"
    gc.build_checkpoint(p3, "tiny-llama3", embd="Q8_0", rope_freqs=True)  # hidden 384, G = 3, tied
    l3 = build_engine("tiny-llama3", checkpoint=str(p3), dtype="q4_0", **kw)
    assert l3.runner.w.lm_head.kind == "bf16"
    _check_engine(l3, (2,))
    del l3

    # the bf16 engine built beside them: same graphs, same kernels per step, same tokens
    assert [r.token_ids for r in bf.generate(prompts, sp)] == want
    assert set(bf.runner.graphs) == keys
    assert counts == {(B, s): bf.runner.count_step_kernels(B, s) for B in (1, 2, 8) for s in (False, True)}
