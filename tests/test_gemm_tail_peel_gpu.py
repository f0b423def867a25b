"""Decode GEMM (csrc/kernels/gemm.hip gemm_skinny_kernel) with the pipeline's last iteration peeled: every chunk count
a wave can end on, against the fp32 reference at test_gemm_xfrag's tolerances.  K 64 gives waves with no chunk at all,
K 2048 equal even counts, K 2144 a ragged last chunk with unequal counts of both parities across the waves; uneven
split-K slices (split-K 3) and ragged grids (N 320 at nb 6) ride along.  Fragment-major and row-major activations."""
import math

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops

pytestmark = pytest.mark.gpu

N = 320
_cache: dict = {}


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _weights(gpu, K):
    """Dense and packed weights of one K, made once: a plain [N, K] matrix and a gate/up pair for the SiLU epilogue."""
    if K not in _cache:
        g = torch.Generator(device="cpu").manual_seed(K)
        w, wg, wu = ((torch.randn(n, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(gpu)
                     for n in (N, N // 2, N // 2))
        _cache[K] = dict(w=w, wg=wg, wu=wu, pw=ops.PackedWeight.from_dense(w),
                         pgu=ops.PackedWeight.from_dense(ops.interleave_gate_up(wg, wu)))
    return _cache[K]


@pytest.mark.parametrize("K", [64, 2048, 2144])
@pytest.mark.parametrize("M", [1, 9, 17, 32, 48])
def test_tail_peel_every_chunk_count(gpu, M, K):
    W = _weights(gpu, K)
    g = torch.Generator(device="cpu").manual_seed(1000 * M + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(gpu)
    xf = ops.to_xfrag(x)
    lin = x.float() @ W["w"].float().t()
    act = torch.nn.functional.silu(x.float() @ W["wg"].float().t()) * (x.float() @ W["wu"].float().t())
    for nb in (2, 4, 6):
        for waves, div in ((4, 1), (4, 2), (4, 4), (8, 2)):
            tag = (M, K, nb, waves, div)
            for splitk in (1, 2, 3):
                y = ops.linear_xf(xf, M, W["pw"], "f32", splitk=splitk, nb=nb, waves=waves, div=div)
                assert y.shape == (splitk, M, N)
                assert _rel(y.sum(0), lin) < 1e-4, tag + (splitk, "xf")
                y = ops.linear(x, W["pw"], "f32", splitk=splitk, nb=nb, waves=waves, div=div)
                assert _rel(y.sum(0), lin) < 1e-4, tag + (splitk, "row")
            y = ops.linear_xf(xf, M, W["pw"], "bf16", splitk=1, nb=nb, waves=waves, div=div)
            assert _rel(y, lin) < 1e-2, tag
            y = ops.linear_xf(xf, M, W["pgu"], "silu", splitk=1, nb=nb, waves=waves, div=div)
            assert _rel(ops.from_xfrag(y, M, N // 2), act) < 1e-2, tag
