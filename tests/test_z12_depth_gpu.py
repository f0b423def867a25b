"""The 12-bit decode GEMM (csrc/kernels/gemm_z12.hip) over every wave chunk count, with one patch-record load and one
ballot per k-step: for every (nb, waves, div) the launcher tells apart, ops.linear_xf(z12=True) is bit-equal to the bf16
kernel at the same (nb, splitk, waves, div).  (Written with the pipeline-depth experiment; depths 3 and 4 passed these
cases, lost inside the decode step and were removed, so the shipped depth 2 is what runs here.)
K = 32 x {1, 3, 4, 5, 9, 13, 17, 21, 25, 29, 33} gives a wave of a 4-wave workgroup 0 .. 9 chunks at one k-step per chunk
(no chunk, the prologue alone, both tails of the two-deep pipeline) and unequal split-K ranges; N 96 / 224 are an exact
and a ragged grid at nb 4 and 6; 17 and 32 rows; f32 slabs at split-K 1 / 2 / 3, SiLU and bf16, each with and without the
row scale.  Weights: N(0, 0.02^2), and the same with planted patch entries: the corners of the first and the last
fragment, four entries in one fragment, and one entry in every other n-block at the middle k-step (middle and last
n-blocks of exact and ragged workgroups, where the n-block clamp and the nibble-to-fragment mapping act; several fragments
of one k-step of one workgroup under one ballot).  A captured-graph replay at the longest K."""
import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops

pytestmark = pytest.mark.gpu

KS = [32 * k for k in (1, 3, 4, 5, 9, 13, 17, 21, 25, 29, 33)]
VARIANTS = [(2, 4, 1), (2, 4, 2), (2, 4, 4), (2, 8, 1), (2, 8, 2), (4, 4, 1), (4, 4, 2), (4, 4, 4), (4, 8, 1), (4, 8, 2),
            (6, 4, 1), (6, 4, 2)]  # (nb, waves, div) the launcher tells apart
EPIS = (("f32", 1), ("f32", 2), ("f32", 3), ("silu", 1), ("bf16", 1))

_cache: dict = {}


def _dense(kind, N, K):
    # seeds at which no escape of the draw itself lands in the fragment that gets four planted entries (a fifth would
    # make the weight not compressible)
    g = torch.Generator().manual_seed(11 * N + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    if kind == "planted":
        # lane 16 g + r, slot i of fragment (nb, kb) is W[16 nb + r][32 kb + 8 g + i]
        bits = w.view(torch.int16)
        nbl, kbl = N // 16 - 1, K // 32 - 1
        plant = [((0, 0, 0, 0), 0x0000), ((0, 0, 63, 7), 0x4080), ((0, 0, 0, 7), 0x0001), ((0, 0, 63, 0), 0xC080),
                 ((nbl, kbl, 0, 0), 0x3080), ((nbl, kbl, 63, 7), 0x8000), ((nbl, kbl, 0, 7), 0xC080)]
        plant += [((j, (kbl + 1) // 2, (7 * j + 3) % 64, j % 8), 0x4300 + j) for j in range(1, nbl)]
        for (nb, kb, lane, slot), b in plant:
            bits[16 * nb + (lane & 15), 32 * kb + 8 * (lane >> 4) + slot] = b - 0x10000 if b >= 0x8000 else b
    return w


def _weight(gpu, kind, N, K):
    key = (kind, N, K)
    if key not in _cache:
        pw = ops.PackedWeight.from_dense(_dense(kind, N, K).to(gpu)).add_z12()
        assert pw.z12 is not None
        z = pw.z12
        assert torch.equal(ops.unpack_z12(z).view(torch.int16).reshape(-1), pw.data.view(torch.int16).reshape(-1))
        if kind == "planted":  # every planted value lies outside the 16-binade window of N(0, 0.02^2)
            rec = (z.esc.view(N // 16, K // 32, 4) < 0).sum(-1)
            mid = (K // 32) // 2
            assert int(rec[0, 0]) == 4 and int(rec[-1, -1]) >= 3
            assert all(int(rec[j, mid]) >= 1 for j in range(1, N // 16 - 1))
        _cache[key] = pw
    return _cache[key]


@pytest.mark.parametrize("kind", ["randn", "planted"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [96, 224])
def test_every_chunk_count_bit_equal_to_bf16(gpu, N, K, kind):
    pw = _weight(gpu, kind, N, K)
    for M in (17, 32):
        g = torch.Generator().manual_seed(1000 * M + K)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(gpu)
        xf = ops.to_xfrag(x)
        ss = ops.ss_q24(x.float().pow(2).sum(1))
        for nb, waves, div in VARIANTS:
            for epi, splitk in EPIS:
                if splitk > K // 32:
                    continue
                for scale in (False, True):
                    kw = dict(splitk=splitk, nb=nb, waves=waves, div=div)
                    if scale:
                        kw["rownorm"] = (ss, 1e-5)
                    want = ops.linear_xf(xf, M, pw, epi, **kw)
                    got = ops.linear_xf(xf, M, pw, epi, z12=True, **kw)
                    assert got.shape == want.shape and got.dtype == want.dtype
                    assert torch.equal(got, want), (M, N, K, kind, nb, waves, div, epi, splitk, scale)


@pytest.mark.parametrize("nb,waves,div", [(6, 4, 2), (4, 4, 4)])
def test_graph_replay_at_the_longest_k(gpu, nb, waves, div):
    M, N, K = 32, 224, 32 * 33
    pw = _weight(gpu, "planted", N, K)
    g = torch.Generator().manual_seed(11)
    xs = [ops.to_xfrag(torch.randn(M, K, generator=g).to(torch.bfloat16).to(gpu)) for _ in range(3)]
    xf = torch.zeros_like(xs[0])
    out = torch.zeros(2, M, N, device=gpu, dtype=torch.float32)
    kw = dict(splitk=2, nb=nb, waves=waves, div=div)
    ops.linear_xf(xf, M, pw, "f32", out=out, z12=True, **kw)  # loads the kernel before the capture
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.linear_xf(xf, M, pw, "f32", out=out, z12=True, **kw)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for x in xs:
        xf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.linear_xf(x, M, pw, "f32", **kw))
