"""Numerics of every gfx950 kernel against the plain-PyTorch fp32 reference (ops/reference.py)."""
import math

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ----------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M", [1, 3, 16, 17, 32, 40, 64])
@pytest.mark.parametrize("NK", [(1024, 4096), (4096, 1024), (1536, 11008), (256, 1376)])
def test_gemm_skinny_bf16(gpu, M, NK):
    N, K = NK
    torch.manual_seed(M * 7 + N)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    y = ops.linear(x, pw, "bf16")
    yr = ref.linear(x, w, "bf16")
    assert y.shape == (M, N)
    assert _rel(y, yr) < 1e-2


@pytest.mark.parametrize("M", [1, 8, 33])
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_gemm_skinny_f32_splitk(gpu, M, splitk):
    N, K = 2048, 4096
    torch.manual_seed(1)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    y = ops.linear(x, pw, "f32", splitk=splitk)
    assert y.shape == (splitk, M, N)
    yr = x.float() @ w.float().t()
    assert _rel(y.sum(0), yr) < 1e-4


@pytest.mark.parametrize("M", [1, 20, 64, 100, 257, 1100, 2100])
def test_gemm_silu(gpu, M):
    """Fused SiLU(gate) * up through ops.linear: the skinny decode kernel (M <= 64) and the stream-K prefill kernel."""
    F, K = 1024, 2048
    torch.manual_seed(2)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    wg = (torch.randn(F, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    wu = (torch.randn(F, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(ops.interleave_gate_up(wg, wu))
    y = ops.linear(x, pw, "silu")
    yr = torch.nn.functional.silu(x.float() @ wg.float().t()) * (x.float() @ wu.float().t())
    assert y.shape == (M, F)
    assert _rel(y, yr) < 1e-2


@pytest.mark.parametrize("M", [1, 9, 20, 32, 48, 64])
@pytest.mark.parametrize("epi", ["bf16", "f32", "silu"])
@pytest.mark.parametrize("nb,waves,div", [(2, 4, 4), (4, 8, 2), (1, 4, 1), (6, 4, 2), (8, 4, 1)])
def test_gemm_xfrag(gpu, M, epi, nb, waves, div):
    """Fragment-major activations (ops.to_xfrag) through every epilogue and tuning knob vs fp32
    (nb 6 / 8: wide n-groups, one activation fragment per 6 / 8 weight fragments)."""
    if epi == "silu" and nb == 1:
        pytest.skip("silu needs nb >= 2")
    N, K = (1536 if nb >= 6 else 1024), 2048
    torch.manual_seed(M * 3 + nb)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    if epi == "silu":
        wg = (torch.randn(N // 2, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
        wu = (torch.randn(N // 2, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
        pw = ops.PackedWeight.from_dense(ops.interleave_gate_up(wg, wu))
        yr = torch.nn.functional.silu(x.float() @ wg.float().t()) * (x.float() @ wu.float().t())
    else:
        w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
        pw = ops.PackedWeight.from_dense(w)
        yr = x.float() @ w.float().t()
    xf = ops.to_xfrag(x)
    sk = 2 if epi == "f32" else 1
    y = ops.linear_xf(xf, M, pw, epi, splitk=sk, nb=nb, waves=waves, div=div)
    if epi == "f32":
        y = y.sum(0)
    elif epi == "silu":  # fragment-major in -> fragment-major out
        y = ops.from_xfrag(y, M, N // 2)
    assert _rel(y, yr) < (1e-4 if epi == "f32" else 1e-2)


@pytest.mark.parametrize("M", [1, 9, 16, 30])
@pytest.mark.parametrize("nb", [6, 8])
def test_gemm_wide_nb_rowmajor(gpu, M, nb):
    """Wide n-groups with row-major activations (the batch <= 16 decode layout) vs fp32."""
    N, K = 1536, 2048
    torch.manual_seed(M + nb)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    for div in (1, 2):
        y = ops.linear(x, pw, "f32", splitk=2, nb=nb, waves=4, div=div)
        assert _rel(y.sum(0), x.float() @ w.float().t()) < 1e-4


@pytest.mark.parametrize("M", [17, 32, 48, 64])
@pytest.mark.parametrize("splitk", [1, 4, 8])
def test_gemm_f32_mid_batch(gpu, M, splitk):
    """16 < M <= 64, f32 slabs, every chunk-depth divisor vs fp32."""
    N, K = 1024, 4096
    torch.manual_seed(M + splitk)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    for div in (1, 2, 4):
        y2 = ops.linear(x, pw, "f32", splitk=splitk, div=div)
        assert _rel(y2.sum(0), x.float() @ w.float().t()) < 1e-4


@pytest.mark.parametrize("M", [1, 32])
def test_silu_parts(gpu, M):
    F, K = 512, 1024
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    wg = (torch.randn(F, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    wu = (torch.randn(F, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(ops.interleave_gate_up(wg, wu))
    parts = ops.linear(x, pw, "f32", splitk=2)
    act = torch.empty(M, F, device=gpu, dtype=torch.bfloat16)
    ops.silu_parts(parts, act)
    yr = torch.nn.functional.silu(x.float() @ wg.float().t()) * (x.float() @ wu.float().t())
    assert _rel(act, yr) < 1e-2


def _sk_ref(x, w, epi, h0=None):
    yr = x.float() @ w.float().t()
    if epi == "silu":
        M, N = yr.shape
        r3 = yr.view(M, N // 32, 2, 16)
        return (torch.nn.functional.silu(r3[:, :, 0]) * r3[:, :, 1]).reshape(M, N // 2)
    return yr + h0 if epi == "res" else yr


def _sk_case(gpu, M, N, K, epi, share, ncu=None, seed=0, cfg=-1):
    torch.manual_seed(seed + M + N + K)
    x = (torch.rand(M, K, device=gpu) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, device=gpu) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    h0 = torch.randn(M, N, device=gpu) if epi == "res" else None
    ncol = N // 2 if epi == "silu" else N
    dt = torch.float32 if epi in ("f32", "res") else torch.bfloat16
    out = h0.clone() if epi == "res" else torch.full((M, ncol), float("nan"), device=gpu, dtype=dt)
    ws, tk, ncu0 = ops._sk_workspace(gpu)
    grid = ops.ext().gemm_sk(x, pw.data, N, out, ops._SK_EPI[epi], ws, tk, ncu or ncu0, share, cfg)
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0  # every call leaves the tickets zero
    yr = _sk_ref(x, w, epi, h0)
    assert not torch.isnan(out).any()  # every output element written
    assert _rel(out, yr) < (1e-5 if dt == torch.float32 else 1e-2), (M, N, K, epi, share, grid)
    return x, pw, out, h0, grid


@pytest.mark.parametrize("M", [65, 300, 777, 2048])
@pytest.mark.parametrize("NK", [(800, 4096), (1024, 1376), (4096, 512), (3072, 3072), (256, 96)])
@pytest.mark.parametrize("epi", ["bf16", "f32", "silu", "res"])
def test_gemm_stream_k(gpu, M, NK, epi):
    """Stream-K prefill kernel (the cost model's tile pick) vs the fp32 product: M / N tile edges (N = 800: a
    partial column tile), odd K / 32 (1376 -> 43 k-steps), every epilogue (the residual one accumulates into h),
    grids from 4 tiles to a full chip of K-range shares."""
    N, K = NK
    _sk_case(gpu, M, N, K, epi, ops.SK_MIN_SHARE)


@pytest.mark.parametrize("nbuf", [3, 2])
@pytest.mark.parametrize("cfg", list(range(8)) + [8, 11, 13, 14, 15])
@pytest.mark.parametrize("MNK", [(300, 3072, 1376), (2048, 5120, 1024), (1100, 800, 512), (640, 1536, 2048)])
@pytest.mark.parametrize("epi", ["bf16", "silu", "res"])
def test_gemm_stream_k_tile_shapes(gpu, cfg, MNK, epi, nbuf):
    """Every tile configuration (BM 128 / 256 x BN 128 / 192 / 256; + 8: whole tiles only) on shapes whose edges cut
    every tile kind, with the three-buffer K-tile pipeline (where it fits) and the two-buffer one; K-tile counts 22,
    16, 8 and 32 exercise every tail of the three-way unrolled loop."""
    M, N, K = MNK
    if epi == "silu" and not ops.sk_cfg_pairs(cfg):
        pytest.skip("SiLU needs an even n-block count per wave")
    ops.ext().gemm_sk_nbuf(nbuf)
    try:
        _sk_case(gpu, M, N, K, epi, 4, cfg=cfg)
    finally:
        ops.ext().gemm_sk_nbuf(3)


@pytest.mark.parametrize("share", [1, 2, 5])
@pytest.mark.parametrize("MNK", [(300, 3072, 3072), (2048, 3072, 8192), (128, 4096, 4096)])
def test_gemm_stream_k_many_partials(gpu, share, MNK):
    """Small stream-K shares: tiles cut among many workgroups (up to 64-way at share 1), every partial summed by the
    last to arrive in contributor order, so a repeated call is bitwise identical."""
    M, N, K = MNK
    x, pw, out, h0, _ = _sk_case(gpu, M, N, K, "f32", share)
    first = out.clone()
    ws, tk, ncu = ops._sk_workspace(gpu)
    for _ in range(3):
        ops.ext().gemm_sk(x, pw.data, N, out, 1, ws, tk, ncu, share, -1)
        torch.cuda.synchronize()
        assert torch.equal(out, first)


@pytest.mark.parametrize("cfg", [-1, 0, 2, 4, 5, 6, 12])
@pytest.mark.parametrize("MNK", [(300, 3072, 1376), (2048, 6144, 1024), (1100, 800, 512)])
@pytest.mark.parametrize("epi", ["bf16", "res"])
def test_gemm_stream_k_epilogues(gpu, cfg, MNK, epi):
    """The stream-K prefill GEMM's bf16 and residual (h += y) epilogues vs the fp32 reference over the direct
    (LDS-free) and LDS-image epilogues of several tile configurations: every element written, tickets left zero."""
    M, N, K = MNK
    torch.manual_seed(M + N + K + cfg)
    x = (torch.rand(M, K, device=gpu) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, device=gpu) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    ws, tk, ncu = ops._sk_workspace(gpu)
    yr = x.float() @ w.float().t()
    if epi == "res":
        h0 = torch.randn(M, N, device=gpu)
        h = h0.clone()
        ops.ext().gemm_sk(x, pw.data, N, h, 3, ws, tk, ncu, 4, cfg)
        torch.cuda.synchronize()
        assert int(tk.abs().sum()) == 0
        assert _rel(h, h0 + yr) < 1e-5
        return
    out = torch.full((M, N), float("nan"), device=gpu, dtype=torch.bfloat16)
    ops.ext().gemm_sk(x, pw.data, N, out, ops._SK_EPI[epi], ws, tk, ncu, 4, cfg)
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0
    assert not torch.isnan(out.float()).any()
    assert _rel(out, _sk_ref(x.float(), w, epi)) < 1e-2, (M, N, K, epi, cfg)


@pytest.mark.parametrize("cfg", [-1, 0, 3, 5, 6, 7, 8, 12])
@pytest.mark.parametrize("MNK", [(300, 3072, 1376), (2048, 5120, 1024), (1100, 800, 512), (65, 1536, 2048)])
@pytest.mark.parametrize("epi", ["bf16", "silu", "res"])
def test_gemm_stream_k_fragment_major(gpu, cfg, MNK, epi):
    """Fragment-major X (ops.to_xfrag, ceil(M / 16) row tiles; the pad rows of the last tile hold NaN, which must not
    reach a real row) and, for SiLU, a fragment-major output: bitwise equal to the row-major call of the same
    configuration (the same MFMAs in the same order), every element written, tickets left zero.  K = 1376: an odd
    k-step count, the last K-tile's missing step staged from past the buffer end."""
    M, N, K = MNK
    if epi == "silu" and cfg >= 0 and not ops.sk_cfg_pairs(cfg):
        pytest.skip("SiLU needs an even n-block count per wave")
    if epi == "silu" and N % 64:
        pytest.skip("a fragment-major SiLU output holds whole 32-column k-steps")
    torch.manual_seed(M + N + K)
    x = (torch.rand(M, K, device=gpu) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, device=gpu) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    mt = ops.xfrag_tiles(M)
    xp = torch.full((mt * 16, K), float("nan"), device=gpu, dtype=torch.bfloat16)
    xp[:M] = x
    xf = xp.view(mt, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)
    assert torch.equal(ops.from_xfrag(xf, M, K), x)
    ws, tk, ncu = ops._sk_workspace(gpu)
    ncol = N // 2 if epi == "silu" else N
    if epi == "res":
        h0 = torch.randn(M, N, device=gpu)
        a, b = h0.clone(), h0.clone()
        ops.ext().gemm_sk(x, pw.data, N, a, 3, ws, tk, ncu, 4, cfg)
        ops.ext().gemm_sk(xf, pw.data, N, b, 3, ws, tk, ncu, 4, cfg, 1, M)
    else:
        a = torch.full((M, ncol), float("nan"), device=gpu, dtype=torch.bfloat16)
        ops.ext().gemm_sk(x, pw.data, N, a, ops._SK_EPI[epi], ws, tk, ncu, 4, cfg)
        xo = epi == "silu"
        b = torch.full(((mt * 16 if xo else M) * ncol,), float("nan"), device=gpu, dtype=torch.bfloat16)
        ops.ext().gemm_sk(xf, pw.data, N, b, ops._SK_EPI[epi], ws, tk, ncu, 4, cfg, 3 if xo else 1, M)
        b = ops.from_xfrag(b, M, ncol) if xo else b.view(M, ncol)
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0
    assert not torch.isnan(b.float()).any()
    assert torch.equal(a, b), (M, N, K, epi, cfg, _rel(b, a))
    assert _rel(b, _sk_ref(x.float(), w, epi, h0 if epi == "res" else None)) < (1e-5 if epi == "res" else 1e-2)


@pytest.mark.parametrize("ncu", [8, 24, 40])
@pytest.mark.parametrize("MN", [(777, 1280), (2048, 10240), (1024, 4096)])
def test_gemm_stream_k_dp_rounds(gpu, ncu, MN):
    """A plan on a grid smaller than the chip (ncu workgroups): several data-parallel rounds of whole tiles plus the
    stream-K remainder (tiles mod ncu + ncu), and grids whose size is not a multiple of the 8 XCDs."""
    M, N = MN
    for epi in ("bf16", "res"):
        _sk_case(gpu, M, N, 1024, epi, 4, ncu=ncu)


def test_gemm_asymmetric_exact(gpu):
    """Small-integer operands: the result is exact, so any lane/row/col map error shows up."""
    M, N, K = 7, 48, 64
    x = torch.zeros(M, K, device=gpu)
    for m in range(M):
        x[m, m] = 1.0  # rows of identity
    w = torch.arange(N * K, device=gpu).reshape(N, K).remainder(13).float() - 6
    pw = ops.PackedWeight.from_dense(w.to(torch.bfloat16))
    y = ops.linear(x.to(torch.bfloat16), pw, "f32")[0]
    assert torch.equal(y, (x @ w.t()))


# ----------------------------------------------------------------------------------------- fp8
def test_fp8_cvt_matches_torch(gpu):
    w = torch.randn(64, 128, device=gpu) * 3
    q, s = ops.quantize_fp8(w)
    deq = ops.dequantize_fp8(q, s, 64, 128)
    assert _rel(deq, w) < 0.05
    pw = ops.PackedWeight(64, 128, "fp8", q, s)
    x = torch.eye(64, 128, device=gpu).to(torch.bfloat16)  # picks rows of W^T
    y = ops.linear(x, pw, "f32")[0]
    assert torch.allclose(y, (x.float() @ deq.t()), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("M", [1, 16, 20, 32, 40, 64, 130])
@pytest.mark.parametrize("epi", ["bf16", "f32", "silu"])
def test_fp8_gemm(gpu, M, epi):
    N, K = 1024, 4096
    torch.manual_seed(3)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w, kind="fp8")
    wd = ops.dequantize_fp8(pw.data, pw.scale, N, K)
    y = ops.linear(x, pw, epi)
    yr = ref.linear(x, wd, epi)
    if epi == "f32":
        y = y.sum(0)
    # M > 64 runs W8A8 (per-token fp8 activations, ~2.5 % e4m3 rounding); decode M <= 64 is weight-only
    assert _rel(y, yr) < (4e-2 if M > 64 and ops.FP8_W8A8 else 1e-2)
    if M <= 64:  # fragment-major activations (the decode path at B > 16)
        yx = ops.linear_xf(ops.to_xfrag(x), M, pw, epi, splitk=2 if epi == "f32" else 1)
        if epi == "f32":
            yx = yx.sum(0)
        elif epi == "silu":
            yx = ops.from_xfrag(yx, M, N // 2)
        assert _rel(yx, yr) < 1e-2


@pytest.mark.parametrize("M", [1, 9, 20, 32])
@pytest.mark.parametrize("epi", ["f32", "silu"])
@pytest.mark.parametrize("nb,depth", [(6, 1), (8, 2), (8, 1)])
def test_fp8_gemm_wide_nb(gpu, M, epi, nb, depth):
    """W8A16 decode GEMM with wide n-groups (row-major and fragment-major activations) vs fp32."""
    if nb == 6 and M <= 16:
        pytest.skip("nb 6 is instantiated for the 17..32-row tile only")
    N, K = 1536, 4096
    torch.manual_seed(M + nb)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w if epi == "f32" else ops.interleave_gate_up(w[: N // 2], w[N // 2:]), "fp8")
    wd = ops.dequantize_fp8(pw.data, pw.scale, N, K)
    yr = ref.linear(x, wd, epi)
    xf = 16 < M
    xin = ops.to_xfrag(x) if xf else x
    sk = 2 if epi == "f32" else 1
    kw = dict(splitk=sk, nb=nb, waves=4, div=2 if depth == 2 else 4)
    y = ops.linear_xf(xin, M, pw, epi, **kw) if xf else ops.linear(xin, pw, epi, **kw)
    if epi == "f32":
        y = y.sum(0)
    elif xf:
        y = ops.from_xfrag(y, M, N // 2)
    assert _rel(y, yr) < 1e-2


# ----------------------------------------------------------------------------------------- norm / rope
@pytest.mark.parametrize("D", [3072, 4096, 8192, 1024])
def test_add_rmsnorm(gpu, D):
    rows, S = 5, 3
    torch.manual_seed(D)
    h = torch.randn(rows, D, device=gpu)
    parts = torch.randn(S, rows, D, device=gpu)
    w = torch.randn(D, device=gpu).to(torch.bfloat16)
    xn = torch.empty(rows, D, device=gpu, dtype=torch.bfloat16)
    h2, xn2 = h.clone(), xn.clone()
    ops.add_rmsnorm(h, w, 1e-5, xn, parts=parts)
    ref.add_rmsnorm(h2, w, 1e-5, xn2, parts=parts)
    assert torch.allclose(h, h2, atol=1e-5)
    assert _rel(xn, xn2) < 1e-2
    # embedding gather form
    V = 100
    emb = torch.randn(V, D, device=gpu).to(torch.bfloat16)
    ids = torch.tensor([3, 99, 0, 5, 7], device=gpu, dtype=torch.int32)
    ops.add_rmsnorm(h, w, 1e-5, xn, ids=ids, emb=emb)
    assert torch.allclose(h, emb[ids.long()].float())
    # gathered rows, no write-back
    ri = torch.tensor([4, 1], device=gpu, dtype=torch.int32)
    xs = torch.empty(2, D, device=gpu, dtype=torch.bfloat16)
    hb = h.clone()
    ops.add_rmsnorm(h, w, 1e-5, xs, row_idx=ri, write_h=False)
    assert torch.equal(h, hb)
    ref_xs = torch.empty_like(xs)
    ref.add_rmsnorm(h.clone(), w, 1e-5, ref_xs, row_idx=ri, write_h=False)
    assert _rel(xs, ref_xs) < 1e-2


@pytest.mark.parametrize("rows", [3, 20, 33])
def test_add_rmsnorm_xfrag(gpu, rows):
    """Fragment-major output of the norm (decode GEMM input) == to_xfrag of the row-major output."""
    D = 4096
    h = torch.randn(rows, D, device=gpu)
    parts = torch.randn(2, rows, D, device=gpu)
    w = torch.randn(D, device=gpu).to(torch.bfloat16)
    xr = torch.empty(rows, D, device=gpu, dtype=torch.bfloat16)
    h2 = h.clone()
    ops.add_rmsnorm(h2, w, 1e-5, xr, parts=parts)
    xf = torch.zeros(ops.xfrag_tiles(rows) * 16 * D, device=gpu, dtype=torch.bfloat16)
    ops.add_rmsnorm(h, w, 1e-5, xf, parts=parts, rows=rows, xf=True)
    assert torch.equal(h, h2)
    assert torch.equal(ops.from_xfrag(xf, rows, D), xr)


@pytest.mark.parametrize("kernel", ["rows8", "row_per_wg"])
@pytest.mark.parametrize("rows", [65, 300, 777, 2048])
@pytest.mark.parametrize("D", [3072, 4096, 160])
def test_add_rmsnorm_xfrag_prefill(gpu, rows, D, kernel):
    """The prefill norm of h alone into the fragment-major layout (the 8-row LDS-staged kernel, forced at every size
    here, and the row-per-workgroup one; partial last tiles at 65 / 300 / 777 rows; D = 160: an odd k-step count)
    vs the fp32 reference, h untouched."""
    ops.ext().rmsnorm_xf_tile_min(65 if kernel == "rows8" else 1 << 30)
    try:
        _norm_xf_case(gpu, rows, D)
    finally:
        ops.ext().rmsnorm_xf_tile_min(512)


def _norm_xf_case(gpu, rows, D):
    torch.manual_seed(rows + D)
    h = torch.randn(rows, D, device=gpu) * 3
    w = torch.randn(D, device=gpu).to(torch.bfloat16)
    h0 = h.clone()
    xf = torch.full((ops.xfrag_tiles(rows) * 16 * D,), float("nan"), device=gpu, dtype=torch.bfloat16)
    ops.add_rmsnorm(h, w, 1e-5, xf, write_h=False, rows=rows, xf=True)
    torch.cuda.synchronize()
    assert torch.equal(h, h0)
    want = h0 * torch.rsqrt(h0.pow(2).mean(1, keepdim=True) + 1e-5) * w.float()
    got = ops.from_xfrag(xf, rows, D).float()
    assert torch.isfinite(got).all()
    assert _rel(got, want) < 1e-2


@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
def test_rope_append(gpu, HH):
    H, Hkv = HH
    T, D, nblk = 9, 128, 6
    torch.manual_seed(5)
    cos, sin = ref.rope_tables(D, 512, 10000.0, device=gpu)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, device=gpu).to(torch.bfloat16)
    pos = torch.tensor([0, 1, 2, 63, 64, 65, 130, 5, 200], device=gpu, dtype=torch.int32)
    tok_seq = torch.tensor([0, 0, 0, 0, 0, 0, 0, 1, 1], device=gpu, dtype=torch.int32)
    bt = torch.tensor([[2, 4, 5, 0], [1, 3, 0, 0]], device=gpu, dtype=torch.int32)
    kc = torch.zeros(nblk, Hkv, 64, D, device=gpu, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q = torch.empty(T, H, D, device=gpu, dtype=torch.bfloat16)
    kc2, vc2, q2 = kc.clone(), vc.clone(), q.clone()
    ops.rope_append(qkv, pos, tok_seq, bt, cos, sin, q, kc, vc, H, Hkv)
    ref.rope_append(qkv, pos, tok_seq, bt, cos, sin, q2, kc2, vc2, H, Hkv)
    assert _rel(q, q2) < 1e-2
    assert _rel(kc, kc2) < 1e-2
    assert torch.equal(vc, vc2)
    # f32 split-K slab input (the decode path): the kernel sums the slabs while rotating
    parts = torch.randn(3, T, (H + 2 * Hkv) * D, device=gpu)
    kc3, vc3, q3 = kc.clone(), vc.clone(), q.clone()
    kc4, vc4, q4 = kc.clone(), vc.clone(), q.clone()
    ops.rope_append(parts, pos, tok_seq, bt, cos, sin, q3, kc3, vc3, H, Hkv)
    ref.rope_append(parts, pos, tok_seq, bt, cos, sin, q4, kc4, vc4, H, Hkv)
    assert _rel(q3, q4) < 1e-2 and _rel(kc3, kc4) < 1e-2
    v32 = parts[0]
    for s in range(1, parts.shape[0]):  # the kernel adds the slabs in this order, in f32
        v32 = v32 + parts[s]
    blk, off = ref._slots(pos, tok_seq, bt)
    vc_want = vc.clone()
    vc_want[blk, :, off] = v32.view(T, H + 2 * Hkv, D)[:, H + Hkv:].to(torch.bfloat16)
    assert torch.equal(vc3, vc_want)


# ----------------------------------------------------------------------------------------- attention
def _paged(kv_lens, Hkv, D, device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nb_per = [(n + 63) // 64 for n in kv_lens]
    total = sum(nb_per) + 1
    perm = (torch.randperm(total - 1, generator=g) + 1).tolist()
    maxb = max(nb_per) + 1
    bt = torch.zeros(len(kv_lens), maxb, dtype=torch.int32)
    i = 0
    for s, nb in enumerate(nb_per):
        for j in range(nb):
            bt[s, j] = perm[i]
            i += 1
    kc = (torch.randn(total, Hkv, 64, D, generator=g)).to(torch.bfloat16).to(device)
    vc = (torch.randn(total, Hkv, 64, D, generator=g)).to(torch.bfloat16).to(device)
    return kc, vc, bt.to(device)


@pytest.mark.parametrize("HH", [(32, 32), (24, 8), (32, 8), (16, 2)])
@pytest.mark.parametrize("lens", [[1, 63, 64, 65], [700, 5, 2100]])
def test_attn_decode(gpu, HH, lens):
    H, Hkv = HH
    D = 128
    kc, vc, bt = _paged(lens, Hkv, D, gpu, seed=len(lens) + H)
    B = len(lens)
    q = torch.randn(B, H, D, device=gpu).to(torch.bfloat16)
    pos = torch.tensor([n - 1 for n in lens], device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    out = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    out2 = torch.empty_like(out)
    ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, out)
    ref.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, out2)
    assert _rel(out, out2) < 1e-2
    # forced single split (no combine kernel)
    out3 = torch.empty_like(out)
    ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, out3, plan=(bt.shape[1], 1))
    assert _rel(out3, out2) < 1e-2
    # a grid planned for a much longer context (graph capture at max_model_len): per-sequence splits
    out4 = torch.empty_like(out)
    ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, out4, plan=ops.decode_split_plan(B, Hkv, 16384))
    assert _rel(out4, out2) < 1e-2
    # unsplit threshold 0: every context of >= 2 blocks splits one block per workgroup (in-launch combine)
    out5 = torch.empty_like(out)
    ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, out5, plan=(1, bt.shape[1], 0))
    assert _rel(out5, out2) < 1e-2
    # fragment-major output (O-projection input), split and single-split paths
    for plan in (None, (bt.shape[1], 1)):
        xf = torch.zeros(ops.xfrag_tiles(B) * 16 * H * D, device=gpu, dtype=torch.bfloat16)
        ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, xf, plan=plan, xf=True)
        ro = out if plan is None else out3
        assert torch.equal(ops.from_xfrag(xf, B, H * D), ro.view(B, -1))
    # e4m3 output (the W8A8 / W4A8 o projection's input): one E8M0 scale per (row, head), vs the fp32 oracle
    for plan in (None, (bt.shape[1], 1)):
        mt = ops.xfrag_tiles(B)
        x8 = torch.zeros(mt * 16 * H * D, device=gpu, dtype=torch.uint8)
        s8 = torch.full((mt * 64 * H,), 127, device=gpu, dtype=torch.uint8)
        ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, scale, x8, plan=plan, xf=True, out_s8=s8)
        got = ops.xf8_dequant(x8, B, H * D, None, s8)
        want = out2.view(B, -1).float()
        assert _rel(got, want) < 4e-2, plan
        # the scale is the head's own: its amax lands in the top binade of e4m3 ([224, 448])
        se = ops.from_xs8(s8, B, H * D).view(B, H, 4).cpu().int()
        assert (se == se[:, :, :1]).all()
        amax = want.view(B, H, D).abs().amax(-1).cpu()
        ratio = amax / torch.exp2(se[:, :, 0].float() - 127)
        assert ((ratio > 200) & (ratio <= 448)).all(), ratio


@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
@pytest.mark.parametrize("lens", [[1, 64, 65, 300], [2000]])
@pytest.mark.parametrize("nparts", [1, 3, 8])
def test_attn_decode_fused_rope(gpu, HH, lens, nparts):
    """RoPE + KV append fused into decode attention == rope_append then attn_decode (cache and output)."""
    H, Hkv = HH
    D = 128
    kc, vc, bt = _paged(lens, Hkv, D, gpu, seed=7)
    B = len(lens)
    pos = torch.tensor([n - 1 for n in lens], device=gpu, dtype=torch.int32)
    cos, sin = ref.rope_tables(D, 4096, 500000.0, device=gpu)
    parts = torch.randn(nparts, B, (H + 2 * Hkv) * D, device=gpu)
    scale = 1 / math.sqrt(D)
    k1, v1 = kc.clone(), vc.clone()
    q1 = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ops.rope_append(parts, pos, None, bt, cos, sin, q1, k1, v1, H, Hkv)
    o1 = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ops.attn_decode(q1, k1, v1, bt, pos, H, Hkv, scale, o1)
    k2, v2 = kc.clone(), vc.clone()
    o2 = torch.empty_like(o1)
    ops.attn_decode(torch.empty_like(q1), k2, v2, bt, pos, H, Hkv, scale, o2, qkv_parts=parts, cos=cos, sin=sin)
    torch.cuda.synchronize()
    assert torch.equal(v1, v2)  # v is copied
    assert torch.allclose(k1.float(), k2.float(), rtol=1e-2, atol=1e-2)  # fma contraction may differ by 1 ulp
    assert (k1 != k2).float().mean() < 0.01
    assert _rel(o2, o1) < 1e-2


@pytest.mark.parametrize("B", [2, 16, 20])
def test_attn_decode_g1_single_buffer_grids(gpu, B):
    """G = 1 (7B MHA) decode attention with fused RoPE / KV append on both sides of the single-buffer grid
    threshold (B x 32 heads >= 512 workgroups: one K/V register set at 8 waves / SIMD; below it the two-set
    pipeline) vs the fp32 reference over the rope_append-written cache."""
    H = Hkv = 32
    D = 128
    lens = [(37 * i) % 300 + 1 for i in range(B)]
    kc, vc, bt = _paged(lens, Hkv, D, gpu, seed=11)
    pos = torch.tensor([n - 1 for n in lens], device=gpu, dtype=torch.int32)
    cos, sin = ref.rope_tables(D, 4096, 500000.0, device=gpu)
    parts = torch.randn(2, B, (H + 2 * Hkv) * D, device=gpu)
    scale = 1 / math.sqrt(D)
    k1, v1 = kc.clone(), vc.clone()
    q1 = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ops.rope_append(parts, pos, None, bt, cos, sin, q1, k1, v1, H, Hkv)
    o_ref = torch.empty(B, H, D, device=gpu, dtype=torch.bfloat16)
    ref.attn_decode(q1, k1, v1, bt, pos, H, Hkv, scale, o_ref)
    o = torch.empty_like(o_ref)
    ops.attn_decode(torch.empty_like(q1), kc, vc, bt, pos, H, Hkv, scale, o, qkv_parts=parts, cos=cos, sin=sin)
    torch.cuda.synchronize()
    assert _rel(o, o_ref) < 1e-2
    assert torch.equal(vc, v1)


P_KERNELS = ["16", "32", "32pair"]


def _set_prefill_kernel(monkeypatch, kernel):
    monkeypatch.setattr(ops, "PREFILL_ATTN", kernel[:2])
    monkeypatch.setattr(ops, "PREFILL_PAIR", "1" if kernel.endswith("pair") else "0")


@pytest.mark.parametrize("kernel", P_KERNELS)
@pytest.mark.parametrize("HH", [(32, 32), (24, 8)])
@pytest.mark.parametrize("case", ["fresh", "chunked", "long", "longer"])
def test_attn_prefill(gpu, HH, case, kernel, monkeypatch):
    """The prefill attention kernels (16 x 16 MFMA, 64 rows per workgroup; 32 x 32 MFMA, 128 rows, single or
    heavy/light paired query blocks per workgroup) vs
    the fp32 reference: packed variable-length sequences, chunked continuation, multi-block causal tiles."""
    _set_prefill_kernel(monkeypatch, kernel)
    H, Hkv = HH
    D = 128
    if case == "fresh":
        qlens, ctx = [1, 70, 130, 64], [1, 70, 130, 64]
    elif case == "chunked":  # chunked prefill: context already holds earlier chunks
        qlens, ctx = [10, 64, 100], [200, 64, 400]
    elif case == "long":  # several 128-row query blocks and 64-key tiles per sequence, ragged ends
        qlens, ctx = [300, 257], [300, 400]
    else:  # one long prompt (many tiles through the 3-deep V ring) next to a short one
        qlens, ctx = [1100, 40], [1100, 700]
    kc, vc, bt = _paged(ctx, Hkv, D, gpu, seed=H)
    T = sum(qlens)
    q = torch.randn(T, H, D, device=gpu).to(torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0).tolist()), device=gpu, dtype=torch.int32)
    cl = torch.tensor(ctx, device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    out = torch.empty(T, H, D, device=gpu, dtype=torch.bfloat16)
    out2 = torch.empty_like(out)
    ops.attn_prefill(q, kc, vc, bt, cu, cl, H, Hkv, scale, out)
    ref.attn_prefill(q, kc, vc, bt, cu, cl, H, Hkv, scale, out2)
    assert _rel(out, out2) < 1e-2
    # the fragment-major output (the o projection's stream-K input): the same values, rearranged
    of = torch.full((ops.xfrag_tiles(T) * 16 * H * D,), float("nan"), device=gpu, dtype=torch.bfloat16)
    ops.attn_prefill(q, kc, vc, bt, cu, cl, H, Hkv, scale, of, xf=True)
    torch.cuda.synchronize()
    assert torch.equal(ops.from_xfrag(of, T, H * D), out.view(T, H * D))


@pytest.mark.parametrize("kernel", P_KERNELS)
def test_attn_prefill_spike(gpu, kernel, monkeypatch):
    """Force the online-softmax rescale branch: one very large score late in the sequence."""
    _set_prefill_kernel(monkeypatch, kernel)
    H, Hkv, D = 8, 8, 128
    n = 300
    kc, vc, bt = _paged([n], Hkv, D, gpu, seed=9)
    q = torch.randn(n, H, D, device=gpu).to(torch.bfloat16)
    blk = int(bt[0, 250 // 64])
    kc[blk, :, 250 % 64] = (q[299].float() * 4).to(torch.bfloat16)
    cu = torch.tensor([0, n], device=gpu, dtype=torch.int32)
    cl = torch.tensor([n], device=gpu, dtype=torch.int32)
    out = torch.empty(n, H, D, device=gpu, dtype=torch.bfloat16)
    out2 = torch.empty_like(out)
    ops.attn_prefill(q, kc, vc, bt, cu, cl, H, Hkv, 1 / math.sqrt(D), out)
    ref.attn_prefill(q, kc, vc, bt, cu, cl, H, Hkv, 1 / math.sqrt(D), out2)
    assert _rel(out, out2) < 1e-2


# ----------------------------------------------------------------------------------------- sampling
def _state(B, max_new, device):
    z = lambda: torch.zeros(B, dtype=torch.int32, device=device)  # noqa: E731
    return (torch.full((B, max_new), -1, dtype=torch.int32, device=device), z(), z(),
            torch.arange(B, dtype=torch.int32, device=device) + 10, z())


@pytest.mark.parametrize("V", [32000, 128256, 1000])
def test_argmax_commit(gpu, V):
    B = 5
    logits = torch.randn(B, V, device=gpu)
    logits[1, 777 % V] = 100.0
    logits[2, :] = 0.0  # ties -> first index
    eos = torch.tensor([int(logits[3].argmax())], device=gpu, dtype=torch.int32)
    st = _state(B, 4, gpu)
    st2 = tuple(t.clone() for t in st)
    ops.argmax_commit(logits, *st, eos)
    ref.argmax_commit(logits, *st2, eos)
    for a, b in zip(st, st2):
        assert torch.equal(a, b)
    assert int(st[4][3]) == 1 and int(st[3][3]) == 13  # finished on EOS, position not advanced


def test_sample_commit_distribution(gpu):
    V, B = 5000, 64
    torch.manual_seed(0)
    base = torch.randn(V, device=gpu) * 2
    logits = base.repeat(B, 1)
    T, K, P = 0.8, 40, 0.9
    temp = torch.full((B,), T, device=gpu)
    topk = torch.full((B,), K, device=gpu, dtype=torch.int32)
    topp = torch.full((B,), P, device=gpu)
    counts = torch.zeros(V)
    eos = torch.tensor([-1], device=gpu, dtype=torch.int32)
    rounds = 40
    for r in range(rounds):
        seeds = torch.randint(0, 2**62, (B,), device=gpu, dtype=torch.int64)
        st = _state(B, 2, gpu)
        ops.sample_commit(logits.clone(), None, None, temp, topk, topp, seeds, *st, eos)
        toks = st[0][:, 0].cpu()
        counts += torch.bincount(toks.long(), minlength=V).float()
    idx, p = ref.sample_probs(base.cpu(), T, K, P)
    emp = counts[idx] / counts.sum()
    assert counts[idx].sum() == counts.sum()  # never outside the nucleus
    assert (emp - p).abs().max() < 0.05


def test_sample_greedy_rows(gpu):
    V, B = 32000, 4
    logits = torch.randn(B, V, device=gpu)
    temp = torch.tensor([0.0, 0.0, 1.0, 1.0], device=gpu)
    topk = torch.tensor([1, 1, 1, 1], device=gpu, dtype=torch.int32)  # top-k 1 == greedy
    topp = torch.ones(B, device=gpu)
    seeds = torch.arange(B, device=gpu, dtype=torch.int64)
    eos = torch.tensor([-1], device=gpu, dtype=torch.int32)
    st = _state(B, 3, gpu)
    ops.sample_commit(logits, None, None, temp, topk, topp, seeds, *st, eos)
    assert torch.equal(st[0][:, 0].long(), logits.argmax(-1))


def test_repeat_penalty_ring_matches_reference(gpu):
    """Repetition penalty over the position-indexed history ring (greedy rows, so deterministic) and the
    ring write of the committed token, vs the fp32 reference."""
    V, B, W = 32000, 6, 64
    torch.manual_seed(3)
    logits = torch.randn(B, V) * 3
    hist = torch.randint(0, V, (B, W), dtype=torch.int32)
    hist[1, 10:] = -1
    hist[2, :] = hist[2, 0]                                   # one token repeated: penalised once
    pos = torch.tensor([5, 9, 200, 63, 64, 1000], dtype=torch.int32)
    pen = torch.tensor([1.3, 2.0, 1.5, 1.0, 0.7, 1.1])
    last_n = torch.tensor([64, 64, 64, 64, 8, 3], dtype=torch.int32)
    # make the penalty decide the argmax: each row's top logit sits on one of its recent tokens
    for b in range(B):
        t = int(hist[b, int(pos[b]) % W])
        if t >= 0:
            logits[b, t] = logits[b].max() + 0.1
    temp = torch.zeros(B)
    topk = torch.full((B,), 40, dtype=torch.int32)
    topp = torch.ones(B)
    seeds = torch.zeros(B, dtype=torch.int64)
    eos = torch.tensor([-1], dtype=torch.int32)

    def run(dev):
        st = [x.to(dev) for x in _state(B, 4, "cpu")]
        st[3].copy_(pos.to(dev))
        h = hist.to(dev).clone()
        ops.sample_commit(logits.to(dev).clone(), h, pen.to(dev), temp.to(dev), topk.to(dev), topp.to(dev),
                          seeds.to(dev), *st, eos.to(dev), last_n=last_n.to(dev))
        return st[0][:, 0].cpu(), h.cpu()

    tg, hg = run(gpu)
    tc, hc = run("cpu")
    assert torch.equal(tg, tc)
    assert torch.equal(hg, hc)
    for b in range(B):  # the committed token landed at column (pos + 1) % W
        assert int(hg[b, (int(pos[b]) + 1) % W]) == int(tg[b])


def test_rope_table_bound_checked_on_host(gpu):
    """Positions live on the device, so the host checks the rope tables cover every position the block
    tables can address (a short table would otherwise be read out of bounds by the fused kernels)."""
    H, Hkv, D = 8, 2, 128
    kc, vc, bt = _paged([100, 300], Hkv, D, gpu)
    pos = torch.tensor([99, 299], device=gpu, dtype=torch.int32)
    cos, sin = ref.rope_tables(D, 256, 10000.0, device=gpu)  # bt addresses 6 * 64 = 384 positions
    parts = torch.randn(1, 2, (H + 2 * Hkv) * D, device=gpu)
    q = torch.empty(2, H, D, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="rope tables"):
        ops.attn_decode(q, kc, vc, bt, pos, H, Hkv, 0.1, torch.empty_like(q), qkv_parts=parts, cos=cos, sin=sin)
    with pytest.raises(RuntimeError, match="rope tables"):
        ops.rope_append(parts, pos, None, bt, cos, sin, q, kc, vc, H, Hkv)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ norm-folded decode epilogues
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("xf", [False, True])
@pytest.mark.parametrize("M", [1, 7, 20, 32, 64])
def test_gemm_rownorm_and_residual_epilogues(gpu, kind, xf, M):
    """rownorm (rows scaled by rsqrt(ss/K + eps)) on the f32-slab and SiLU epilogues, and the residual
    epilogue (h += y, xout = bf16(h), ss_out += sum h^2) vs the fp32 PyTorch definition."""
    if xf and M <= 16:
        pytest.skip("fragment-major activations are the 16 < M <= 64 decode layout")
    torch.manual_seed(M + 3 * xf)
    d, F = 1024, 512
    eps = 1e-5
    h0 = torch.randn(M, d, device=gpu) * 3
    x = h0.to(torch.bfloat16)
    ss = h0.pow(2).sum(1)
    wq = (torch.randn(768, d, device=gpu) / math.sqrt(d)).to(torch.bfloat16)
    wg = (torch.randn(F, d, device=gpu) / math.sqrt(d)).to(torch.bfloat16)
    wu = (torch.randn(F, d, device=gpu) / math.sqrt(d)).to(torch.bfloat16)
    wo = (torch.randn(d, F, device=gpu) / math.sqrt(F)).to(torch.bfloat16)
    pq, pgu, po = (ops.PackedWeight.from_dense(t, kind) for t in (wq, ops.interleave_gate_up(wg, wu), wo))
    xin = ops.to_xfrag(x) if xf else x

    def lin(a, w, epi, **kw):
        return ops.linear_xf(a, M, w, epi, **kw) if xf else ops.linear(a, w, epi, **kw)

    inv = torch.rsqrt(ss / d + eps)[:, None]
    xs = x.float() * inv  # what the un-folded path feeds the GEMM (before its bf16 rounding)
    ssq = ops.ss_q24(ss)  # the kernels' int64 Q24 fixed point
    y = lin(xin, pq, "f32", splitk=2, rownorm=(ssq, eps))
    assert _rel(y.sum(0), xs @ pq.dense().float().t()) < 2e-2
    act = lin(xin, pgu, "silu", rownorm=(ssq, eps))
    act = ops.from_xfrag(act, M, F) if xf else act
    gd, ud = pgu.dense().float().view(F // 16, 2, 16, d)[:, 0].reshape(F, d), pgu.dense().float().view(F // 16, 2, 16, d)[:, 1].reshape(F, d)
    want_act = torch.nn.functional.silu(xs @ gd.t()) * (xs @ ud.t())
    assert _rel(act, want_act) < 2e-2
    # residual epilogue from the bf16 activations
    a16 = want_act.to(torch.bfloat16)
    h = torch.randn(M, d, device=gpu)
    h_ref = h + a16.float() @ po.dense().float().t()
    tickets = torch.zeros(d // 16, device=gpu, dtype=torch.int32)
    for splitk in (1, 4):  # one workgroup per column, and split-K finished by the last-arriving split
        runs = []
        for _ in range(3):
            hh = h.clone()
            xout = torch.zeros(ops.xfrag_tiles(M) * 16 * d if xf else M * d, device=gpu, dtype=torch.bfloat16)
            ss_out = torch.full((M,), 1 << 23, device=gpu, dtype=torch.int64)  # 0.5 in Q24
            lin(ops.to_xfrag(a16) if xf else a16, po, "res", splitk=splitk,
                res=(hh, xout if xf else xout.view(M, d), ss_out, tickets))
            torch.cuda.synchronize()
            assert _rel(hh, h_ref) < 1e-2, splitk
            got_x = ops.from_xfrag(xout, M, d) if xf else xout.view(M, d)
            assert torch.equal(got_x, hh.to(torch.bfloat16)), splitk
            assert torch.allclose(ops.ss_float(ss_out), 0.5 + hh.pow(2).sum(1), rtol=1e-4), splitk
            assert torch.all(tickets == 0), "the last arriver must reset its column counter"
            runs.append(ss_out)
        # integer accumulation: bit-identical whatever order the workgroups finished in
        assert all(torch.equal(runs[0], r) for r in runs[1:]), splitk


@pytest.mark.parametrize("xf", [False, True])
def test_add_rmsnorm_raw_mode(gpu, xf):
    """raw mode: h = emb[ids]; x = bf16(h); ss_out[m] = sum h^2; the next nzero accumulators zeroed."""
    B, d, V, S = 20, 512, 1000, 32
    torch.manual_seed(5)
    emb = torch.randn(V, d, device=gpu).to(torch.bfloat16)
    ids = torch.randint(0, V, (B,), device=gpu, dtype=torch.int32)
    h = torch.zeros(S, d, device=gpu)
    xn = torch.zeros(ops.xfrag_tiles(B) * 16 * d if xf else B * d, device=gpu, dtype=torch.bfloat16)
    ss = torch.full((4, S), 7, device=gpu, dtype=torch.int64)
    ops.add_rmsnorm(h[:B], torch.ones(d, device=gpu, dtype=torch.bfloat16), 1e-5, xn if xf else xn.view(B, d),
                    ids=ids, emb=emb, rows=B, xf=xf, ss_out=ss.view(-1), ss_ld=S, ss_nzero=2)
    torch.cuda.synchronize()
    hv = emb[ids.long()].float()
    assert torch.equal(h[:B], hv)
    got = ops.from_xfrag(xn, B, d) if xf else xn.view(B, d)
    assert torch.equal(got, hv.to(torch.bfloat16))
    assert torch.allclose(ops.ss_float(ss[0, :B]), hv.pow(2).sum(1), rtol=1e-5)
    assert torch.all(ss[1:3, :B] == 0) and torch.all(ss[3] == 7) and torch.all(ss[0, B:] == 7)


@pytest.mark.parametrize("case", [(1, 3072, 4, False), (32, 4096, 2, True), (20, 4096, 3, True), (5, 2560, 0, False),
                                  (64, 4096, 5, True)])
def test_res_add_ss(gpu, case):
    """Wide raw residual add (ops.res_add_ss) vs the fp32 PyTorch definition: h += sum of the split-K slabs,
    x = bf16(h) (row-major or fragment-major), ss += sum h^2 in Q24 on top of what the accumulator holds; rows
    past B and the slab padding untouched; bitwise identical across repeats (integer atomics)."""
    B, d, S, xf = case
    torch.manual_seed(B * d + S)
    Sl = 64
    h = torch.randn(Sl, d, device=gpu) * 4
    parts = torch.randn(max(S, 1), B, d, device=gpu) if S else None
    runs = []
    for _ in range(2):
        hh = h.clone()
        xn = torch.zeros(ops.xfrag_tiles(B) * 16 * d if xf else B * d, device=gpu, dtype=torch.bfloat16)
        ss = torch.full((Sl,), 1 << 23, device=gpu, dtype=torch.int64)  # 0.5 in Q24
        ops.res_add_ss(hh[:B], parts, xn if xf else xn.view(B, d), B, ss, xf=xf)
        torch.cuda.synchronize()
        hv = h[:B] + (parts.sum(0) if parts is not None else 0)
        assert torch.allclose(hh[:B], hv, atol=1e-5, rtol=1e-6)
        assert torch.equal(hh[B:], h[B:])
        got = ops.from_xfrag(xn, B, d) if xf else xn.view(B, d)
        assert torch.equal(got, hh[:B].to(torch.bfloat16))
        assert torch.allclose(ops.ss_float(ss[:B]), 0.5 + hv.pow(2).sum(1), rtol=1e-5)
        assert torch.all(ss[B:] == 1 << 23)
        runs.append(ss)
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------ W8A8 fp8 prefill GEMM (block-scaled MFMA)
def test_fp8_tile_gemm_exact_integers(gpu):
    """Small integers are exact in e4m3 and in every partial sum: the 16x16x128 f8f6f4 MFMA tile GEMM must
    match the integer product exactly (checks the lane/k pairing of A and B and the epilogue row/col map);
    asymmetric operands and scales."""
    torch.manual_seed(0)
    M, N, K = 300, 512, 1024
    xi = torch.randint(-4, 5, (M, K), device=gpu).float()
    wi = torch.randint(-4, 5, (N, K), device=gpu).float()
    x8 = xi.to(torch.float8_e4m3fn).view(torch.uint8)
    sx = torch.linspace(0.5, 2.0, M, device=gpu)
    sw = torch.linspace(1.0, 3.0, N, device=gpu)
    wq = ops.pack_fp8(wi.to(torch.float8_e4m3fn))
    want = (xi @ wi.t()) * sx[:, None] * sw[None, :]
    out = torch.empty(M, N, device=gpu)
    ops.ext().fp8_gemm_t256(x8, sx, wq, sw, N, out, 1, 1)
    torch.cuda.synchronize()
    assert torch.allclose(out, want, rtol=1e-6, atol=1e-3), (out - want).abs().max().item()
    for sk in (2, 4):  # split-K slabs sum to the same product
        o = torch.empty(sk, M, N, device=gpu)
        ops.ext().fp8_gemm_t256(x8, sx, wq, sw, N, o, 1, sk)
        torch.cuda.synchronize()
        assert torch.allclose(o.sum(0), want, rtol=1e-6, atol=1e-3), sk


def test_quant_rows_fp8_matches_torch(gpu):
    torch.manual_seed(1)
    x = (torch.randn(77, 3072, device=gpu) * torch.linspace(0.1, 30, 77, device=gpu)[:, None]).to(torch.bfloat16)
    x8, sx = ops.quantize_rows_fp8(x)
    torch.cuda.synchronize()
    amax = x.float().abs().amax(1)
    assert torch.allclose(sx, amax / 448.0, rtol=1e-6)
    want = (x.float() / sx[:, None]).to(torch.float8_e4m3fn)
    got = x8.view(torch.float8_e4m3fn)
    # same OCP e4m3fn encoding and round-to-nearest-even (the 1/s multiply vs divide may flip a tie)
    mism = (got.view(torch.uint8) != want.view(torch.uint8)).float().mean().item()
    assert mism < 1e-3, mism
    assert torch.allclose(got.float(), want.float(), rtol=0.13, atol=2 ** -8)  # a tie flip: one e4m3 ulp


@pytest.mark.parametrize("M", [100, 384, 1000])
@pytest.mark.parametrize("epi", ["bf16", "f32", "silu"])
def test_fp8_w8a8_linear(gpu, M, epi):
    """ops.linear on fp8 weights at M > 64 runs W8A8 (per-token activation scales) on the fp8 MFMA: vs the
    fp32 product of the bf16 activations and the dequantised weights, within fp8 activation rounding."""
    torch.manual_seed(M)
    N, K = (1024, 2048) if epi != "silu" else (2048, 1024)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w, "fp8")
    wd = pw.dense().float()
    y = ops.linear(x, pw, epi)
    if epi == "f32":
        y = y.sum(0)
        want = x.float() @ wd.t()
    elif epi == "bf16":
        want = x.float() @ wd.t()
    else:
        F = N // 2
        g = wd.view(F // 16, 2, 16, K)[:, 0].reshape(F, K)
        u = wd.view(F // 16, 2, 16, K)[:, 1].reshape(F, K)
        want = torch.nn.functional.silu(x.float() @ g.t()) * (x.float() @ u.t())
    assert _rel(y, want) < 4e-2


# ------------------------------------------------------------------ W8A8 decode GEMM (fp8 activations)
@pytest.mark.parametrize("M", [1, 9, 20, 32, 48, 64])
def test_quant_xf8(gpu, M):
    """GPU per-row e4m3 quantisation into the xf8 layout vs the CPU definition (one e4m3 ulp apart at most)."""
    torch.manual_seed(M)
    K = 512
    x = (torch.randn(M, K, device=gpu) * 3).to(torch.bfloat16)
    x8, sx = ops.quantize_xf8(x)
    c8, csx = ops.quantize_xf8(x.cpu())
    assert torch.allclose(sx.cpu(), csx, rtol=1e-6)
    a = ops.from_xf8(x8, M, K).cpu().view(torch.float8_e4m3fn).float()
    b = ops.from_xf8(c8, M, K).view(torch.float8_e4m3fn).float()
    assert torch.allclose(a, b, rtol=0.13, atol=2 ** -8)


@pytest.mark.parametrize("M", [1, 9, 20, 32, 48, 64])
@pytest.mark.parametrize("epi", ["f32", "silu"])
@pytest.mark.parametrize("nb", [2, 4, 6, 8])
def test_fp8a_gemm(gpu, M, epi, nb):
    """W8A8 decode GEMM on the fp8 MFMA vs the fp32 product of the dequantised operands (the kernel is exact
    up to f32 accumulation order: the quantisation itself is the caller's)."""
    if nb >= 6 and not 16 < M <= 32:
        pytest.skip("nb 8 is instantiated for the 17..32-row tile")
    torch.manual_seed(M + nb)
    N, K = 1536, 1536
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w if epi == "f32" else ops.interleave_gate_up(w[: N // 2], w[N // 2:]), "fp8")
    x8, sx = ops.quantize_xf8(x)
    xd = ops.from_xf8(x8, M, K).view(torch.float8_e4m3fn).float() * sx[:, None]
    yr = xd @ ops.dequantize_fp8(pw.data, pw.scale, N, K).float().t()
    if epi == "f32":
        for sk in (1, 3):
            y = ops.linear_a8(x8, sx, M, pw, "f32", splitk=sk, nb=nb)
            assert _rel(y.sum(0), yr) < 1e-4, sk
    else:
        y3 = yr.view(M, N // 32, 2, 16)
        want = (torch.nn.functional.silu(y3[:, :, 0]) * y3[:, :, 1]).reshape(M, N // 2)
        for xfo in (True, False):
            y = ops.linear_a8(x8, sx, M, pw, "silu", nb=nb, xfo=xfo)
            got = ops.from_xfrag(y, M, N // 2) if xfo else y.view(M, N // 2)
            assert _rel(got, want) < 1e-2, xfo


def _blocky(M, K, gen_dev, seed):
    """[M, K] bf16 whose 32-column blocks span 2^-8 .. 2^6 in magnitude (exercises per-block scales)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mag = torch.exp2(torch.randint(-8, 7, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
    return (torch.randn(M, K, generator=g) * mag).to(torch.bfloat16).to(gen_dev)


@pytest.mark.parametrize("M", [1, 9, 20, 32, 48, 64])
def test_quant_xf8_blocks(gpu, M):
    """GPU block-scaled e4m3 quantisation (E8M0 per 32 / 128 columns) vs the CPU definition."""
    K = 1024
    x = _blocky(M, K, gpu, M)
    for blk in (32, 128):
        x8, s8 = ops.quantize_xf8_blocks(x, blk)
        c8, cs8 = ops.quantize_xf8_blocks(x.cpu(), blk)
        assert torch.equal(ops.from_xs8(s8, M, K).cpu(), ops.from_xs8(cs8, M, K)), blk
        a = ops.xf8_dequant(x8, M, K, None, s8).cpu()
        b = ops.xf8_dequant(c8, M, K, None, cs8)
        assert torch.allclose(a, b, rtol=0.13, atol=0), blk
        assert _rel(a, x.float().cpu()) < 4e-2


@pytest.mark.parametrize("M", [1, 9, 20, 32, 48, 64])
@pytest.mark.parametrize("wkind", ["fp8", "mxfp4"])
def test_a8_gemm_block_scales(gpu, M, wkind):
    """W8A8 / W4A8 decode GEMM (ops.linear_a8) with per-block E8M0 activation scales (the MFMA's B scale operand) and,
    for MXFP4, the weights' own E8M0 block scales (A operand, e2m1 elements straight into the MFMA) vs the fp32
    product of the dequantised operands; f32 split-K slabs, the bf16 SiLU epilogue, and the e4m3 SiLU epilogue
    (E8M0 per (row, 32 columns): the down projection's input) vs the CPU quantisation of the fp32 product."""
    N, K = 2048, 1536
    torch.manual_seed(M)
    x = _blocky(M, K, gpu, 7 * M)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    x8, s8 = ops.quantize_xf8_blocks(x, 32)
    xd = ops.xf8_dequant(x8, M, K, None, s8)
    sx = torch.full((M,), 0.5, device=gpu)  # a per-row scale on top of the blocks multiplies in
    for epi in ("f32", "silu"):
        pw = ops.PackedWeight.from_dense(w if epi == "f32" else ops.interleave_gate_up(w[: N // 2], w[N // 2:]), wkind)
        wd = (ops.dequantize_fp8(pw.data, pw.scale, N, K) if wkind == "fp8"
              else ops.dequantize_mxfp4(pw.data, pw.scale, N, K)).float()
        yr = xd @ wd.t()
        if epi == "f32":
            for sk in (1, 3):
                y = ops.linear_a8(x8, None, M, pw, "f32", splitk=sk, s8=s8)
                assert _rel(y.sum(0), yr) < 1e-4, sk
            y = ops.linear_a8(x8, sx, M, pw, "f32", s8=s8)
            assert _rel(y.sum(0), 0.5 * yr) < 1e-4
            continue
        y3 = yr.view(M, N // 32, 2, 16)
        want = (torch.nn.functional.silu(y3[:, :, 0]) * y3[:, :, 1]).reshape(M, N // 2)
        got = ops.from_xfrag(ops.linear_a8(x8, None, M, pw, "silu", s8=s8), M, N // 2)
        assert _rel(got, want) < 1e-2
        mt = ops.xfrag_tiles(M)
        for nb in (4, 8):
            if nb == 8 and M > 32:
                continue
            o8 = torch.zeros(mt * 16 * N // 2, device=gpu, dtype=torch.uint8)
            os8 = torch.full((mt * 64 * (N // 2 // 128),), 0, device=gpu, dtype=torch.uint8)
            ops.linear_a8(x8, None, M, pw, "silu", out=o8, out_s8=os8, s8=s8, nb=nb)
            got8 = ops.xf8_dequant(o8, M, N // 2, None, os8)
            assert _rel(got8, want) < 4e-2, nb
            _, ws = ops.quantize_blocks_fp8(want.cpu(), 32)
            # the block exponents agree except where f32 accumulation order moves an amax across a binade
            assert (ops.from_xs8(os8, M, N // 2).cpu() != ws).float().mean() < 0.02, nb


@pytest.mark.parametrize("M", [20, 32, 64])
def test_add_rmsnorm_fp8_output(gpu, M):
    """add_rmsnorm's xf8 output: the normalised rows (f32, before the bf16 rounding) as per-row e4m3."""
    torch.manual_seed(M)
    d = 1024
    h = torch.randn(M, d, device=gpu) * 2
    g = (torch.rand(d, device=gpu) + 0.5).to(torch.bfloat16)
    want = h * torch.rsqrt(h.pow(2).mean(1, keepdim=True) + 1e-5) * g.float()
    xn = torch.zeros(ops.xfrag_tiles(M) * 16 * d, device=gpu, dtype=torch.bfloat16)
    x8 = torch.zeros(ops.xfrag_tiles(M) * 16 * d, device=gpu, dtype=torch.uint8)
    sx = torch.zeros(M, device=gpu)
    ops.add_rmsnorm(h.clone(), g, 1e-5, xn, rows=M, xf=True, x8=x8, sx8=sx)
    assert torch.allclose(sx, want.abs().amax(1) / 448, rtol=1e-3)
    got = ops.from_xf8(x8, M, d).view(torch.float8_e4m3fn).float() * sx[:, None]
    assert _rel(got, want) < 4e-2
    assert _rel(ops.from_xfrag(xn, M, d).float(), want) < 1e-2  # the bf16 copy is still written



@pytest.mark.parametrize("kind", ["bf16", "mxfp4", "fp8a"])
@pytest.mark.parametrize("M", [1, 9, 32])
@pytest.mark.parametrize("nb", [4, 6, 8])
def test_gemm_ragged_grid(gpu, kind, M, nb):
    """Ragged decode-GEMM grids (common.h skinny_nblocks): 172 n-blocks (86 gate/up pairs; the 7B gate_up's 1376 / 8)
    are not a multiple of nb = 6 or 8, so ceil(172 / nb) workgroups share them 1-2 blocks / pairs apart (nb 4: the
    divisible grid); every column written exactly once, vs fp32, for the bf16, MXFP4 and W8A8 decode kernels (f32
    split-K slabs and the SiLU epilogue)."""
    if kind == "fp8a" and M <= 16:
        pytest.skip("W8A8 decode runs the fragment-major buckets above 16 rows")
    if nb == 6 and M <= 16:
        pytest.skip("nb 6 is instantiated for the two-row-tile kernels")
    N, K = 16 * 172, 1024
    torch.manual_seed(M * 31 + nb)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) / math.sqrt(K)).to(torch.bfloat16)
    wkind = "fp8" if kind == "fp8a" else kind
    pw = ops.PackedWeight.from_dense(w, wkind)
    # the exact weights the kernel multiplies (fp8: e4m3 x f32 channel scale, not rounded to bf16)
    wd = ops.dequantize_fp8(pw.data, pw.scale, N, K).float() if wkind == "fp8" else pw.dense().float()
    xf = 16 < M <= 64
    if kind == "fp8a":
        x8, sx = ops.quantize_xf8(x)
        xe = ops.from_xf8(x8, M, K).view(torch.float8_e4m3fn).float() * sx[:, None]
    else:
        xe = x.float()
    yr = xe @ wd.t()
    y3 = yr.view(M, N // 32, 2, 16)
    want_silu = (torch.nn.functional.silu(y3[:, :, 0]) * y3[:, :, 1]).reshape(M, N // 2)
    for epi in ("f32", "silu"):
        sk = 2 if epi == "f32" else 1
        if kind == "fp8a":
            y = ops.linear_a8(x8, sx, M, pw, epi, splitk=sk, nb=nb, xfo=True)
        elif xf:
            y = ops.linear_xf(ops.to_xfrag(x), M, pw, epi, splitk=sk, nb=nb)
        else:
            y = ops.linear(x, pw, epi, splitk=sk, nb=nb)
        if epi == "f32":
            assert y.shape[0] == sk and _rel(y.sum(0), yr) < 1e-4, (kind, epi)
        else:
            got = ops.from_xfrag(y, M, N // 2) if (xf or kind == "fp8a") else y.view(M, N // 2)
            assert _rel(got, want_silu) < 1e-2, (kind, epi)



@pytest.mark.parametrize("H,Hkv", [(24, 8), (32, 32), (4, 2), (16, 4)])
@pytest.mark.parametrize("T", [65, 300, 1100])
@pytest.mark.parametrize("cfg", [-1, 0, 3, 5, 6, 7, 8, 11])
def test_gemm_rope_epilogue(gpu, H, Hkv, T, cfg):
    """Prefill qkv GEMM with RoPE + the paged KV-cache append in its epilogue (ops.linear_rope / EPI_ROPE) vs the
    fp32 product rotated by the reference: q_out, and every appended cache row at its (block, kv-head, slot) --
    two sequences packed, the second starting mid-block (chunked-prefill continuation), scattered block tables."""
    K, D = 512, 128
    N = (H + 2 * Hkv) * D
    torch.manual_seed(T + H + cfg)
    x = (torch.rand(T, K, device=gpu) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, device=gpu) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    t0 = T // 3
    pos = torch.cat([torch.arange(t0), torch.arange(37, 37 + T - t0)]).to(torch.int32)
    tok_seq = torch.cat([torch.zeros(t0), torch.ones(T - t0)]).to(torch.int32)
    nblk = 64
    perm = torch.randperm(nblk - 1) + 1
    bt = torch.stack([perm[:24], perm[24:48]]).to(torch.int32)
    cos, sin = ref.rope_tables(128, 4096, 10000.0, None)
    kc = torch.zeros(nblk, Hkv, 64, D, device=gpu, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q = torch.zeros(T, H, D, device=gpu, dtype=torch.bfloat16)
    ws, tk, ncu = ops._sk_workspace(gpu)
    ops.ext().gemm_sk_rope(x, pw.data, ws, tk, ncu, 4, cfg, pos.to(gpu), tok_seq.to(gpu), bt.to(gpu), cos.to(gpu),
                           sin.to(gpu), q, kc, vc, H, Hkv)
    torch.cuda.synchronize()
    assert int(tk.abs().sum()) == 0
    qkv = x.float().cpu() @ w.float().cpu().t()
    q_r = torch.zeros(T, H, D, dtype=torch.bfloat16)
    kc_r, vc_r = torch.zeros(nblk, Hkv, 64, D, dtype=torch.bfloat16), torch.zeros(nblk, Hkv, 64, D, dtype=torch.bfloat16)
    ref.rope_append(qkv, pos, tok_seq, bt, cos, sin, q_r, kc_r, vc_r, H, Hkv)
    assert _rel(q.cpu(), q_r) < 4e-3
    assert _rel(kc.cpu(), kc_r) < 4e-3 and _rel(vc.cpu(), vc_r) < 4e-3
    assert int((kc.cpu() != 0).any(-1).sum()) == T * Hkv  # exactly one appended row per token and kv-head



@pytest.mark.parametrize("cfg", [4, 5, 12, 13, -2])
@pytest.mark.parametrize("MK", [(300, 64), (2048, 96), (128, 320), (1100, 1024), (2048, 3072)])
@pytest.mark.parametrize("epi", ["bf16", "f32", "res", "silu"])
def test_gemm_stream_k_one_phase(gpu, cfg, MK, epi):
    """The one-phase four-buffer schedule of the 128-row tiles (ext.gemm_sk_one_phase) vs the fp32 product: short K
    (fewer K-tiles than buffers), an odd k-step count, stream-K partial tiles and whole tiles (cfg + 8), every
    epilogue; and bit-identical to the four-phase schedule (same MFMA order per accumulator)."""
    M, K = MK
    N = 1536
    torch.manual_seed(M + K + max(cfg, 0))
    x = (torch.rand(M, K, device=gpu) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, device=gpu) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    pw = ops.PackedWeight.from_dense(w)
    shape = (M, N // 2 if epi == "silu" else N)
    dt = torch.float32 if epi in ("f32", "res") else torch.bfloat16
    h0 = torch.randn(*shape, device=gpu) if epi == "res" else None
    outs = []
    for one in (1, 0):
        ops.ext().gemm_sk_one_phase(one)
        out = h0.clone() if epi == "res" else torch.empty(*shape, device=gpu, dtype=dt)
        ops.gemm_sk(x, pw.data, N, out, epi, cfg=None if cfg == -2 else cfg)
        outs.append(out)
    ops.ext().gemm_sk_one_phase(1)  # the default
    torch.cuda.synchronize()
    y = x.float() @ w.float().t()
    got = outs[0] - h0 if epi == "res" else outs[0]
    if epi == "silu":
        g, u = y.view(M, -1, 2, 16)[:, :, 0].reshape(M, -1), y.view(M, -1, 2, 16)[:, :, 1].reshape(M, -1)
        y = torch.nn.functional.silu(g) * u
    assert _rel(got, y) < 1e-2
    assert torch.equal(outs[0], outs[1])
