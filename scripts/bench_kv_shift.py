"""Context shift on MI355X: what one shift costs, beside the prefill it avoids.

  shift    device time of one ``ops.kv_shift`` launch with the moves of one request that fills a window of c = 2048
           and c = 4096 tokens with num_keep = 4 (d = 64 * ((c - 4) // 128) tokens dropped, every surviving block
           rotated in place, the kept head copied), on a 7B-shaped and a 3B-shaped bf16 arena.
  prefill  time to first token of the same engine for a prompt of the c - d tokens that survive: the alternative to
           shifting the cache is to prefill them again.

The shift is timed with device events around windows of --calls launches (the arena is far larger than one block, the
launches of a window rotate the same blocks again and again), the prefill with the host clock around a max_tokens = 1
request that ends in the token's read-back; both report the median and the spread of --reps windows.  Writes JSON
lines to profiles/kv_shift/kv_shift_mi355x.jsonl.  Needs a GPU.

  --fp8    also time ``kv_shift8`` (the fp8 cache: dequantise, rotate, quantise again) on the same move lists, on an
           e4m3 arena of the same shape filled with random codes and scales; it moves half the K bytes of the bf16
           launch plus 8 scale bytes per row ("kv_shift8" records, beside the "kv_shift" ones).

  python scripts/bench_kv_shift.py [--layers N] [--reps 9] [--calls 10] [--skip prefill] [--fp8]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llm_based_apache_spark_optimization_amd import ops  # noqa: E402
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams  # noqa: E402
from llm_based_apache_spark_optimization_amd.models import get_spec  # noqa: E402
from llm_based_apache_spark_optimization_amd.models.llama import init_random  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "kv_shift")
MODELS = {"7b": "duckdb-nsql", "3b": "llama3.2"}
KEEP = 4


def emit(rec: dict) -> None:
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "kv_shift_mi355x.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def plan(c: int) -> tuple:
    """(moves, d) of a request whose cache holds rows 0 .. c - 2 in blocks 1, 2, ..., all private, keep = 4."""
    d = 64 * ((c - KEEP) // 128)
    m, nb = d // 64, -(-(c - 1) // 64)
    moves = [(1, 1 + m, 0, KEEP, 0), (1 + m, 1 + m, KEEP, 64, d)] + [(1 + j, 1 + j, 0, 64, d) for j in range(m + 1, nb)]
    return moves, d


def fp8_arena(r: ModelRunner) -> tuple:
    """An e4m3 arena of the runner's shape: random finite codes (0x7f and 0xff are NaN) and scales near 1."""
    g = torch.Generator(device=r.device).manual_seed(8)
    kv = torch.randint(0, 0x7f, tuple(r.kv.shape), generator=g, device=r.device, dtype=torch.uint8)
    kv |= torch.randint(0, 2, tuple(r.kv.shape), generator=g, device=r.device, dtype=torch.uint8) << 7
    sc = torch.rand(tuple(r.kv.shape[:5]), generator=g, device=r.device) + 0.5
    return kv, sc


def bench_shift(r: ModelRunner, tag: str, c: int, reps: int, calls: int, fp8=None) -> None:
    moves, d = plan(c)
    host = torch.tensor(moves, dtype=torch.int32).pin_memory().to(r.device)
    if fp8 is None:
        launch = lambda: ops.ext().kv_shift(r.kv, host, r.cos, r.sin)  # noqa: E731
    else:
        launch = lambda: ops.ext().kv_shift8(fp8[0], fp8[1], host, r.cos, r.sin)  # noqa: E731
    for _ in range(3):
        launch()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    rows = (c - 1 - d - KEEP)  # rotated rows; K read and written (fp8: one byte per value and a 4-byte scale per row)
    nbytes = 2 * rows * r.L * r.Hkv * (128 * 2 if fp8 is None else 128 + 4)
    us = statistics.median(ts)
    emit({"bench": "kv_shift" if fp8 is None else "kv_shift8", "model": tag, "layers": r.L, "kv_heads": r.Hkv, "ctx": c, "keep": KEEP, "discard": d,
          "moves": len(moves), "k_bytes_read_plus_written": nbytes, "us_median": round(us, 1),
          "us_min": round(min(ts), 1), "us_max": round(max(ts), 1), "gbps": round(nbytes / us / 1e3, 1)})


def bench_prefill(eng: LLMEngine, tag: str, c: int, reps: int) -> None:
    _, d = plan(c)
    g = torch.Generator().manual_seed(c)
    ts = []
    for i in range(reps + 1):
        ids = [1] + torch.randint(3, 30000, (c - d - 1,), generator=g).tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate([ids], SamplingParams(max_tokens=1, ignore_eos=True))
        if i:  # the first request warms the shapes up
            ts.append((time.perf_counter() - t0) * 1e3)
    emit({"bench": "prefill_of_kept", "model": tag, "layers": eng.runner.L, "ctx": c, "tokens": c - d,
          "ms_median": round(statistics.median(ts), 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's (0 = all)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip", default="")
    ap.add_argument("--fp8", action="store_true", help="also time kv_shift8 on an fp8 arena of the same shape")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_shift.py needs a GPU: nothing here can be measured without one")
    dev = torch.device("cuda")
    for tag, name in MODELS.items():
        spec = get_spec(name)
        if a.layers:
            spec = dataclasses.replace(spec, n_layers=a.layers, name=f"{name}-{a.layers}l")
        r = ModelRunner(init_random(spec, dev, seed=0), max_slots=2, max_model_len=4096, num_kv_blocks=72)
        eng = LLMEngine(r, name=spec.name, context_shift=True)
        fp8 = fp8_arena(r) if a.fp8 else None
        for c in (2048, 4096):
            bench_shift(r, tag, c, a.reps, a.calls)
            if fp8 is not None:
                bench_shift(r, tag, c, a.reps, a.calls, fp8)
            if "prefill" not in a.skip:
                bench_prefill(eng, tag, c, a.reps)
        del eng, r, fp8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
