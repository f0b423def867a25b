"""Prefix caching on MI355X: what a block fork costs, where it pays, and what a cache hit saves.

  copy   device time of ops.kv_copy_blocks for one (src, dst) pair on a 7B-shaped and a 3B-shaped arena (bf16 and fp8).
  cow    time to first token of hit requests behind a 256-token cached prefix whose suffix is 32 tokens, 32 + p
         tokens (what a request pays when a p-token partial match is NOT forked) and 32 tokens after a fork of p, for
         p in 8 16 32 48: saved = t(32 + p) - t(32).  The default of cow_min_tokens is the smallest p whose saved
         time is at least twice the copy time on both models (64 = never fork, if none is).
  ttft   hit against miss: 7B 300-token prompt with a 256-token shared schema; 3B 2k-token prompt repeated; 7B batch
         of 32 x 128 tokens with 64 shared, the donor run first.  A miss is a request with "cache_prompt": false,
         which takes the path of an engine without the cache.

Times to first token are host wall clock around a max_tokens = 1 request (prefill + the first token's read-back), the
median of --reps requests with fresh random suffixes; the copy is timed with device events.  Writes JSON lines to
profiles/prefix_cache/{kv_copy,cow_sweep,ttft}_mi355x.jsonl.  Needs a GPU.

  python scripts/bench_prefix_cache.py [--layers N] [--skip copy,cow,ttft] [--reps 9] [--out DIR]
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

OUT = os.path.join(ROOT, "profiles", "prefix_cache")
MODELS = {"7b": "duckdb-nsql", "3b": "llama3.2"}


def emit(name: str, rec: dict) -> None:
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, name + "_mi355x.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def bench_copy(dev, reps: int) -> dict:
    """us per kv_copy_blocks call of one pair, the data warm (the same pair again and again), median of reps
    event-timed batches of 20 calls."""
    out = {}
    for tag, name in MODELS.items():
        spec = get_spec(name)
        L, Hkv = spec.n_layers, spec.n_kv_heads
        for fp8 in (False, True):
            kv = torch.zeros(L, 2, 4, Hkv, 64, 128, dtype=torch.uint8 if fp8 else torch.bfloat16, device=dev)
            sc = torch.ones(L, 2, 4, Hkv, 64, dtype=torch.float32, device=dev) if fp8 else None
            pairs = torch.tensor([[1, 2]], dtype=torch.int32, device=dev)
            for _ in range(5):
                ops.ext().kv_copy_blocks(kv, sc, pairs)
            ts = []
            for _ in range(max(reps, 15)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    ops.ext().kv_copy_blocks(kv, sc, pairs)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / 20)
            nbytes = kv[:, :, 0].numel() * kv.element_size() + (sc[:, :, 0].numel() * 4 if fp8 else 0)
            us = statistics.median(ts)
            rec = {"bench": "kv_copy_blocks", "model": tag, "layers": L, "kv_heads": Hkv, "kv": "fp8" if fp8 else "bf16",
                   "block_bytes": nbytes, "us_median": round(us, 2), "us_min": round(min(ts), 2),
                   "us_max": round(max(ts), 2), "gbps_read_plus_write": round(2 * nbytes / us / 1e3, 1)}
            emit("kv_copy", rec)
            out[(tag, fp8)] = us
            del kv, sc
    return out


def engine(name: str, dev, layers: int, cow_min: int, max_slots: int = 32) -> LLMEngine:
    spec = get_spec(name)
    if layers:
        spec = dataclasses.replace(spec, n_layers=layers, name=f"{name}-{layers}l")
    r = ModelRunner(init_random(spec, dev, seed=0), max_slots=max_slots, max_model_len=4096, num_kv_blocks=1024)
    return LLMEngine(r, name=spec.name, prefix_cache=True, prefix_cow_min_tokens=cow_min)


def rand(g, n: int) -> list:
    return torch.randint(3, 30000, (n,), generator=g).tolist()


def ttft_ms(eng: LLMEngine, prompts: list, cache: bool = True) -> tuple:
    """(ms until every prompt's first token is on the host, prompt tokens served from the cache)"""
    sp = SamplingParams(max_tokens=1, ignore_eos=True, cache_prompt=cache)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = eng.generate(prompts, sp)
    return (time.perf_counter() - t0) * 1e3, sum(r.cached_prompt_tokens for r in res)


def med(eng, make_prompts, reps: int, cache: bool = True, warm: int = 2) -> tuple:
    ts, cached = [], 0
    for i in range(warm + reps):
        t, cached = ttft_ms(eng, make_prompts(), cache)
        if i >= warm:
            ts.append(t)
    return statistics.median(ts), min(ts), max(ts), cached


def bench_cow(dev, layers: int, reps: int, copy_us: dict) -> None:
    rows = {}
    for tag, name in MODELS.items():
        eng = engine(name, dev, layers, cow_min=1, max_slots=2)
        g = torch.Generator().manual_seed(11)
        shared, block = [1] + rand(g, 255), rand(g, 64)
        ttft_ms(eng, [shared + block + rand(g, 10)])  # the donor: 4 shared blocks and the block that gets forked
        base = med(eng, lambda: [shared + rand(g, 32)], reps)
        assert base[3] == 256, base
        for p in (8, 16, 32, 48):
            nofork = med(eng, lambda: [shared + rand(g, p + 32)], reps)
            fork = med(eng, lambda: [shared + block[:p] + rand(g, 32)], reps)
            assert nofork[3] == 256 and fork[3] == 256 + p, (nofork, fork)
            saved_us = (nofork[0] - base[0]) * 1e3
            cu = copy_us.get((tag, False))
            rec = {"bench": "cow_sweep", "model": tag, "layers": eng.runner.L, "p": p,
                   "ttft_ms_suffix_32": round(base[0], 3), "ttft_ms_suffix_32_plus_p": round(nofork[0], 3),
                   "ttft_ms_fork_then_32": round(fork[0], 3), "saved_us": round(saved_us, 1),
                   "copy_us": None if cu is None else round(cu * eng.runner.L / get_spec(name).n_layers, 2),
                   "spread_ms": [round(base[2] - base[1], 3), round(nofork[2] - nofork[1], 3), round(fork[2] - fork[1], 3)]}
            rec["saved_over_copy"] = None if not rec["copy_us"] else round(saved_us / rec["copy_us"], 2)
            emit("cow_sweep", rec)
            rows.setdefault(p, []).append(rec["saved_over_copy"])
        del eng
        torch.cuda.empty_cache()
    ok = [p for p, v in sorted(rows.items()) if len(v) == len(MODELS) and all(x is not None and x >= 2.0 for x in v)]
    emit("cow_sweep", {"bench": "cow_min_default", "rule": "smallest p with saved >= 2 x copy on both models, else 64",
                       "qualifying_p": ok, "default": ok[0] if ok else 64})


def bench_ttft(dev, layers: int, reps: int) -> None:
    g = torch.Generator().manual_seed(23)
    for tag, name, kind in (("7b", MODELS["7b"], "schema_300"), ("3b", MODELS["3b"], "repeat_2k"),
                            ("7b", MODELS["7b"], "batch_32x128")):
        eng = engine(name, dev, layers, cow_min=16)
        if kind == "schema_300":
            shared = [1] + rand(g, 255)
            ttft_ms(eng, [shared + rand(g, 44)])
            make = lambda: [shared + rand(g, 44)]  # noqa: E731
        elif kind == "repeat_2k":
            prompt = [1] + rand(g, 2047)
            ttft_ms(eng, [prompt])
            make = lambda: [prompt]  # noqa: E731
        else:
            shared = [1] + rand(g, 63)
            ttft_ms(eng, [shared + rand(g, 64)])
            make = lambda: [shared + rand(g, 64) for _ in range(32)]  # noqa: E731
        miss = med(eng, make, reps, cache=False)
        hit = med(eng, make, reps)
        emit("ttft", {"bench": "ttft_hit_vs_miss", "model": tag, "layers": eng.runner.L, "case": kind,
                      "prompt_tokens": sum(len(p) for p in make()), "cached_tokens_hit": hit[3],
                      "cached_tokens_miss": miss[3], "ttft_ms_miss": round(miss[0], 3), "ttft_ms_hit": round(hit[0], 3),
                      "hit_over_miss": round(hit[0] / miss[0], 3),
                      "spread_ms": [round(miss[2] - miss[1], 3), round(hit[2] - hit[1], 3)]})
        del eng
        torch.cuda.empty_cache()


def main() -> None:
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="truncate the models to N layers (0 = full depth)")
    ap.add_argument("--skip", default="")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    OUT = a.out
    skip = set(filter(None, a.skip.split(",")))
    dev = torch.device("cuda:0")
    ops.ext()
    copy_us = bench_copy(dev, a.reps) if "copy" not in skip else {}
    if "cow" not in skip:
        bench_cow(dev, a.layers, a.reps, copy_us)
    if "ttft" not in skip:
        bench_ttft(dev, a.layers, a.reps)


if __name__ == "__main__":
    main()
