"""Decode GEMM at 32 rows: the 12-bit weight stream (gemm_z12.hip) against the bf16 kernel (gemm.hip) on the 7B shapes
and the lm_head, weights cold from HBM (rotating over > 600 MiB of bf16 copies, the z12 planes of the same copies).
Every arm is a captured graph of 60 launches; the arms' windows alternate (bf16, z12 nb 2, z12 nb 4, ..., bf16, ...),
5 windows each, median reported.  Arms: the bf16 table pick, and z12 at the same (splitk, waves, div) with nb 2 / 4 / 6
(nb does not change the summation order).  Each z12 arm is first checked bit-equal to the bf16 kernel at its config.
One JSON line per shape.  Usage: python scripts/bench_z12.py [shape,shape,..]"""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from llm_based_apache_spark_optimization_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"7b_qkv": (12288, 4096, "f32"), "7b_o": (4096, 4096, "f32"), "7b_gateup": (22016, 4096, "silu"),
          "7b_down": (4096, 11008, "f32"), "7b_head": (32000, 4096, "f32")}
if len(sys.argv) > 1:
    SHAPES = {k: v for k, v in SHAPES.items() if k in sys.argv[1].split(",")}
M, LAUNCHES, WINDOWS = 32, 60, 5


def capture(fn):
    fn(0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for i in range(LAUNCHES):
                fn(i)
    torch.cuda.current_stream(dev).wait_stream(side)
    return g


for name, (N, K, epi) in SHAPES.items():
    ncopy = max(2, (600 << 20) // (N * K * 2) + 1)
    ws = []
    for _ in range(ncopy):
        ws.append(ops.PackedWeight.from_dense((torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)).add_z12())
        assert ws[-1].z12 is not None
    xf = ops.to_xfrag(torch.randn(M, K, device=dev).to(torch.bfloat16))
    nb0, sk, wv, dv = ops.pick_gemm_config(M, N, K, epi, xf=True)

    def out_buf():
        if epi == "silu":
            return torch.zeros(ops.xfrag_tiles(M) * 16 * (N // 2), device=dev, dtype=torch.bfloat16)
        return torch.zeros(sk, M, N, device=dev)

    arms = {"bf16": dict(nb=nb0, z12=False)}
    for nb in (2, 4, 6):
        arms[f"z12_nb{nb}"] = dict(nb=nb, z12=True)
    graphs, equal = {}, {}
    for tag, a in arms.items():
        o = out_buf()
        kw = dict(out=o, splitk=sk, nb=a["nb"], waves=wv, div=dv)
        if a["z12"]:
            ref = ops.linear_xf(xf, M, ws[0], epi, splitk=sk, nb=a["nb"], waves=wv, div=dv).clone()
            ops.linear_xf(xf, M, ws[0], epi, z12=True, **kw)
            equal[tag] = bool(torch.equal(o.view(-1)[: ref.numel()], ref.view(-1)))
        graphs[tag] = capture(lambda i, kw=kw, a=a: ops.linear_xf(xf, M, ws[i % ncopy], epi, z12=a["z12"], **kw))
    torch.cuda.synchronize()
    win = {t: [] for t in arms}
    for _ in range(WINDOWS + 1):  # the first round warms up
        for tag, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            win[tag].append(round(e0.elapsed_time(e1) * 1000 / LAUNCHES, 2))
    us = {t: statistics.median(v[1:]) for t, v in win.items()}
    print(json.dumps(dict(shape=name, M=M, N=N, K=K, epi=epi, pick=dict(nb=nb0, splitk=sk, waves=wv, div=dv),
                          us=us, windows={t: v[1:] for t, v in win.items()}, bit_identical=equal,
                          speedup_same_nb=round(us["bf16"] / us[f"z12_nb{nb0}"], 4),
                          TBps_bf16=round(N * K * 2 / us["bf16"] / 1e6, 3))), flush=True)
    del ws, graphs
    torch.cuda.empty_cache()
