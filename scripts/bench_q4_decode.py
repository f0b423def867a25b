"""GGUF Q4_0 W4A16 decode GEMM (csrc/kernels/gemm_q4.hip) over (nb, splitk, waves) at the 7B / 3B decode shapes, with
the MXFP4 kernel (csrc/kernels/gemm_fp4.hip) at the same configuration beside it: us per call and the weight stream's
rate (codes + f16 scales: 4.5 bits per weight).  The two kernels walk the same operands; the difference is the
in-register decode (about 23 VALU ops per 8 weights against 4), so the ratio says whether that decode hides behind the
stream.  Weights rotate over > 600 MiB so they stream from HBM.  One JSON line per (shape, M) with the best config and
a ready "tune" entry ("NxK:epi:b<M>:q4"); scripts/merge_tuning.py folds them into ops/gemm_tuning.json.

    python scripts/bench_q4_decode.py [Ms] [shape,shape,...]
"""
import json
import sys

import torch

sys.path.insert(0, ".")
from llm_based_apache_spark_optimization_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"7b_qkv": (12288, 4096, "f32"), "7b_o": (4096, 4096, "f32"), "7b_gateup": (22016, 4096, "silu"),
          "7b_down": (4096, 11008, "f32"), "7b_lm_head": (32000, 4096, "f32"), "3b_qkv": (5120, 3072, "f32"),
          "3b_o": (3072, 3072, "f32"), "3b_gateup": (16384, 3072, "silu"), "3b_down": (3072, 8192, "f32")}
Ms = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 32]
names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(SHAPES)


def timeit(fn, it=30):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    reps = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(it):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) * 1000 / it)
    return sorted(reps)[1]


for name in names:
    N, K, epi = SHAPES[name]
    nbytes = N * K // 2 + (N // 16) * ((K // 128 + 1) // 2) * 256
    ncopy = max(2, (600 << 20) // nbytes + 1)
    ws = {kind: [ops.PackedWeight.from_dense(torch.randn(N, K, device=dev) * 0.02, kind) for _ in range(ncopy)]
          for kind in ("q4_0", "mxfp4")}
    for M in Ms:
        xf = 16 < M <= 64
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        xin = ops.to_xfrag(x) if xf else x
        pick = ops.pick_gemm_config(M, N, K, epi, xf=xf, kind="q4_0")
        res = {"shape": name, "M": M, "xf": xf, "pick": list(pick[:3])}
        best = None
        for nb in (1, 2, 4, 8):
            if (epi == "silu" and nb < 2) or (N // 16) % nb or (M > 32 and nb > 2):
                continue
            for sk in ((1, 2, 4, 8) if epi == "f32" else (1,)):
                for waves in ((4,) if nb == 8 else (4, 8)):
                    out = (torch.empty(sk, M, N, device=dev) if epi == "f32" else
                           torch.empty(ops.xfrag_tiles(M) * 16 * N // 2 if xf else M * N // 2, device=dev,
                                       dtype=torch.bfloat16))
                    us = {}
                    for kind in ("q4_0", "mxfp4"):
                        def run(i, w=ws[kind], nb=nb, sk=sk, waves=waves, out=out):
                            if xf:
                                ops.linear_xf(xin, M, w[i % ncopy], epi, out=out, splitk=sk, nb=nb, waves=waves)
                            else:
                                ops.linear(xin, w[i % ncopy], epi, out=out, splitk=sk, nb=nb, waves=waves)

                        us[kind] = timeit(run)
                    if best is None or us["q4_0"] < best[0]:
                        best = (us["q4_0"], nb, sk, waves, us["mxfp4"])
                    if (nb, sk, waves) == tuple(pick[:3]):
                        res["pick_us"] = round(us["q4_0"], 2)
        us, nb, sk, waves, fp4_us = best
        res.update(best_us=round(us, 2), best=[nb, sk, waves], TBps=round(nbytes / us / 1e6, 2),
                   mxfp4_same_cfg_us=round(fp4_us, 2), q4_over_mxfp4=round(us / fp4_us, 3))
        b = 1
        while b < M:
            b *= 2
        res["tune"] = {f"{N}x{K}:{epi}:b{b}:q4": {"nb": nb, "splitk": sk, "waves": waves, "us": round(us, 2),
                                                   "note": "scripts/bench_q4_decode.py"}}
        print(json.dumps(res), flush=True)
    del ws
    torch.cuda.empty_cache()
