#!/usr/bin/env python
"""Device time of the sampled commits with the sampler options off, with the penalties on and with all of them on:
``sample_commit`` at B = 1 and 32 and ``spec_sample_commit`` at T = 4, V = 32000 and 128256.

  python scripts/bench_sampler_options.py --out sampler_options.jsonl [--ext-so PATH/_lsa_hip.so --no-options --tag T]

``--ext-so``: time another build of the extension (for instance the parent commit's) instead of this tree's;
``--no-options``: call it the way a build without the options is called, without the three option operands (cases
``off`` and ``repeat`` only).  Rows are appended to ``--out`` with ``--tag`` in them, so runs of two builds can be
alternated in one session and compared round by round.

Cases: ``off`` (repetition penalty 1, the options zero: the early return of the penalty kernel), ``repeat`` (repetition
penalty 1.1 alone: the ring scan both builds have), ``penalties`` (presence 0.5 and frequency 0.25 on top of it: the
scan with the count), ``all`` (min_p = 0.05 as well).  Each window is ITERS launches between two device events; the
windows of the cases of a shape are interleaved; a row reports the median window and the spread (min,
max) in microseconds per launch."""
import argparse
import importlib.util
import json
import statistics
import sys

import torch

from llm_based_apache_spark_optimization_amd import ops

W = 64


def load(path):
    spec = importlib.util.spec_from_file_location("_lsa_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def operands(B, V, T, dev):
    """Rows of random logits (T = 0: B plain rows; else one sequence of T verify rows), a full ring of tokens from
    among each row's best, the decode state and the workspace."""
    R = B if T == 0 else T
    S = B if T == 0 else 1
    g = torch.Generator().manual_seed(V + R)
    logits = torch.randn(R, V, generator=g) * 2
    pool = logits.max(0).values.topk(40).indices.to(torch.int32)
    i32 = dict(dtype=torch.int32, device=dev)
    o = dict(logits0=logits.to(dev), logits=torch.empty(R, V, device=dev),
             hist=pool[torch.randint(0, 40, (S, W), generator=g)].contiguous().to(dev),
             temperature=torch.full((S,), 0.8, device=dev), top_k=torch.full((S,), 40, **i32),
             top_p=torch.full((S,), 0.9, device=dev), seeds=torch.arange(S, dtype=torch.int64, device=dev) * 7919 + 17,
             out_tokens=torch.zeros(S, 512, **i32), gen_len=torch.zeros(S, **i32), input_ids=torch.zeros(S, **i32),
             positions=torch.full((S,), 200, **i32), finished=torch.zeros(S, **i32), eos=torch.tensor([-1], **i32),
             limit=torch.full((S,), 1 << 30, **i32), eos_on=torch.zeros(S, **i32), last_n=torch.full((S,), W, **i32),
             part=torch.empty(R * ((V + 4095) // 4096), dtype=torch.int64, device=dev),
             cand=torch.empty(R * ((V + 2047) // 2048) * 64, dtype=torch.int64, device=dev),
             picks=torch.empty(R, **i32), draft=torch.full((max(T - 1, 1),), -1, **i32),
             stats=torch.zeros(3, dtype=torch.int64, device=dev))
    return o, S


CASES = {"off": (1.0, 0.0, 0.0, 0.0), "repeat": (1.1, 0.0, 0.0, 0.0), "penalties": (1.1, 0.5, 0.25, 0.0),
         "all": (1.1, 0.5, 0.25, 0.05)}


def launcher(ext, o, S, T, case, with_options, dev):
    pen, pres, freq, mp = CASES[case]
    f = lambda v: torch.full((S,), v, device=dev)  # noqa: E731
    penalty = f(pen)
    extra = (f(pres), f(freq), f(mp)) if with_options else ()
    if T == 0:
        def run():
            ext.sample_commit(o["logits"], o["part"], o["cand"], o["hist"], penalty, o["last_n"], o["temperature"],
                              o["top_k"], o["top_p"], o["seeds"], o["out_tokens"], o["gen_len"], o["input_ids"],
                              o["positions"], o["finished"], o["eos"], o["limit"], o["eos_on"], *extra)
    else:
        def run():
            ext.spec_sample_commit(o["logits"], o["draft"], o["stats"], o["hist"], penalty, o["last_n"],
                                   o["temperature"], o["top_k"], o["top_p"], o["seeds"], o["out_tokens"], o["gen_len"],
                                   o["input_ids"], o["positions"], o["finished"], o["eos"], o["limit"], o["eos_on"],
                                   o["part"], o["cand"], o["picks"], *extra)
    return run


def window(run, o, iters):
    """Microseconds per launch over ``iters`` launches from the start state (each launch commits one token per row
    or sequence; the out_tokens rows are wider than a window is long, so no row finishes inside one)."""
    o["logits"].copy_(o["logits0"])
    o["gen_len"].zero_()
    o["positions"].fill_(200)
    o["finished"].zero_()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ext-so", default=None)
    ap.add_argument("--no-options", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--vocab", type=int, nargs="*", default=[32000, 128256])
    ap.add_argument("--ops", nargs="*", default=["sample_commit", "spec_sample_commit"])
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert args.iters < 512
    if not torch.cuda.is_available():
        print("needs a GPU", file=sys.stderr)
        return 2
    dev = "cuda:0"
    builds = {args.tag: (load(args.ext_so) if args.ext_so else ops.ext(), not args.no_options)}
    with open(args.out, "a") as out:
        for V in args.vocab:
            for op, B, T in (("sample_commit", 1, 0), ("sample_commit", 32, 0), ("spec_sample_commit", 1, 4)):
                if op not in args.ops:
                    continue
                o, S = operands(B, V, T, dev)
                runs = {(bn, case): launcher(ext, o, S, T, case, with_opts, dev)
                        for bn, (ext, with_opts) in builds.items() for case in args.cases
                        if with_opts or case in ("off", "repeat")}
                for run in runs.values():  # warm-up of every pair
                    window(run, o, 20)
                times = {k: [] for k in runs}
                for _ in range(args.windows):
                    for k, run in runs.items():
                        times[k].append(window(run, o, args.iters))
                for (bn, case), ts in times.items():
                    row = dict(op=op, V=V, B=B, T=T, build=bn, case=case, us_median=round(statistics.median(ts), 3),
                               us_min=round(min(ts), 3), us_max=round(max(ts), 3), windows=len(ts), iters=args.iters)
                    print(json.dumps(row), flush=True)
                    out.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
