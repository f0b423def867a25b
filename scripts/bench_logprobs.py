#!/usr/bin/env python
"""Device time of per-token logprobs: the two kernels standalone (``logprob_scan``, ``logprob_commit``) and the
captured decode step with and without the logprob variant, at V = 32000 (duckdb-nsql) and 128256 (llama3.2), B = 1 and
32, K = 0 and 20.

  python scripts/bench_logprobs.py --out profiles/logprobs/logprobs_mi355x.jsonl [--no-steps] [--table]

Each window is ITERS launches (or graph replays) between two device events; the arms of a shape are alternated window
by window in one process; a row reports the median window and its spread (min, max) in microseconds per launch.
Scan rows also report the bytes the scan moves (it reads V * 4 and writes V * 4 per row) over its median time, as a
share of ``--hbm-gbs`` (the MI355X's 8 TB/s by default).  The cost is reported, not gated.  ``--table`` prints the README table
from the rows of ``--out`` instead of measuring.

  python scripts/bench_logprobs.py --spec --out profiles/logprobs/spec_logprobs_mi355x.jsonl

``--spec`` measures the verify-step pair instead (``spec_logprobs``): ``spec_logprob_scan`` / ``spec_logprob_commit``
standalone at (S, T) = (1, 4) and (4, 8) with every sequence recording all T rows, and the captured verify step of the
two models (k = 3 drafts; one sequence, and four with ``spec_batch``) with nobody asking (the plain verify graph and the
"lp" graph with lp_k = -1), all asking K = 0 and all asking K = 20, next to the plain decode step of the same bucket
with and without logprobs -- same windows, arms alternated, same state restored before every window.

  python scripts/bench_logprobs.py --prompt --out profiles/logprobs/prompt_logprobs_mi355x.jsonl \
      [--exact-out profiles/logprobs/prompt_logprobs_exact_mi355x.json]

``--prompt`` measures prompt-token logprobs: the prompt pair standalone (``prompt_logprob_scan`` in its K = 0 form
without candidates and in its K = 20 form, ``prompt_logprob_commit``) at R = 32 and 256 rows, beside the plain
``logprob_scan`` at 32 rows in the same windows (its body is the parent commit's: the yardstick of the K = 0 form), with
the bytes the K = 0 scan reads over its time; the time to first token of a 2k-token prompt on llama3.2 (3B) and a
300-token prompt on duckdb-nsql (7B) with nobody asking, scored from the middle and scored whole, arms interleaved;
and a scoring call of 8 completions of 32 tokens against a cached prompt (the requests ``EngineService.score`` submits).
``--exact-out`` also writes the worst |err| / (2^-24 (1 + |lse| + |l|)) of the pair against float64."""
import argparse
import json
import statistics
import sys

import torch

from llm_based_apache_spark_optimization_amd import ops


def timed(run, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(arms, iters, windows, reset=None):
    """arms: name -> callable; -> name -> list of us per launch, the arms taking turns window by window."""
    for run in arms.values():
        if reset:
            reset()
        timed(run, max(4, iters // 10))
    times = {k: [] for k in arms}
    for _ in range(windows):
        for k, run in arms.items():
            if reset:
                reset()
            times[k].append(timed(run, iters))
    return times


def row_of(ts, **kw):
    return dict(kw, us_median=round(statistics.median(ts), 3), us_min=round(min(ts), 3), us_max=round(max(ts), 3),
                windows=len(ts))


def kernels(V, B, dev, iters, windows, hbm_gbs):
    """The two launches standalone.  Arms: every row asks with K = 0 / K = 20, and no row asks (the early return)."""
    g = torch.Generator().manual_seed(V + B)
    logits = (torch.randn(B, V, generator=g) * 2).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    max_new = 8
    st = dict(gen_len=torch.zeros(B, **i32), finished=torch.zeros(B, **i32), out_tokens=torch.zeros(B, max_new, **i32),
              lp_n0=torch.full((B,), -1, **i32), lp_tok=torch.zeros(B, max_new, device=dev),
              lp_ids=torch.zeros(B, max_new, ops.LOGPROB_KMAX, **i32),
              lp_top=torch.zeros(B, max_new, ops.LOGPROB_KMAX, device=dev), lp_raw=torch.zeros(B, V, device=dev))
    ws = ops.logprob_workspace(B, V, dev)
    ks = {"k0": torch.zeros(B, **i32), "k20": torch.full((B,), 20, **i32), "off": torch.full((B,), -1, **i32)}
    ones = torch.ones(B, **i32)
    rows = []

    def scan(k):
        return lambda: ops.logprob_scan(logits, ks[k], st["finished"], st["gen_len"], st["lp_raw"], st["lp_n0"],
                                        workspace=ws)

    t = alternate({k: scan(k) for k in ks}, iters, windows)
    for k, ts in t.items():
        r = row_of(ts, what="logprob_scan", V=V, B=B, case=k, iters=iters)
        if k != "off":
            r["bytes"] = 2 * 4 * V * B
            r["hbm_share"] = round(r["bytes"] / (r["us_median"] * 1e-6) / (hbm_gbs * 1e9), 4)
        rows.append(r)

    # the commit records only after a scan of the same step: each timed launch is preceded, outside the timing of the
    # other arm, by a state that makes it record -- lp_n0 = 0 and gen_len = 1 are restored by a tiny copy per launch,
    # measured alone as the arm "restore" and subtracted by the reader
    ops.logprob_scan(logits, ks["k20"], st["finished"], st["gen_len"], st["lp_raw"], st["lp_n0"], workspace=ws)
    zeros = torch.zeros(B, **i32)

    def commit(k):
        def run():
            st["lp_n0"].copy_(zeros)
            ops.logprob_commit(st["lp_raw"], ks[k], st["lp_n0"], ones, st["out_tokens"], st["lp_tok"], st["lp_ids"],
                               st["lp_top"], B, workspace=ws)
        return run

    arms = {k: commit(k) for k in ks}
    arms["restore"] = lambda: st["lp_n0"].copy_(zeros)
    t = alternate(arms, iters, windows)
    base = statistics.median(t["restore"])
    for k, ts in t.items():
        r = row_of(ts, what="logprob_commit" if k != "restore" else "restore_copy", V=V, B=B, case=k, iters=iters)
        if k != "restore":
            r["us_median_less_restore"] = round(r["us_median"] - base, 3)
        rows.append(r)
    return rows


def steps(model, B, dev, iters, windows):
    """The captured decode step of ``model`` over B running rows: the plain graph, and the logprob variant with no row
    asking, with every row asking K = 0, and K = 20."""
    from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

    arms = ("plain", "lp_off", "lp_k0", "lp_k20")
    budget = iters + 64
    eng = build_engine(model, device=dev, max_slots=B, max_model_len=budget + 64, kv_reserve_tokens=-1, logprobs=True)
    r = eng.runner
    sp = SamplingParams(max_tokens=budget, ignore_eos=True, logprobs=True, top_logprobs=20)
    for i in range(B):
        eng.add_request([1] + list(range(10 + i, 26 + i)), sp)
    eng.run_ahead = 1
    eng.step()  # admission, prefill and one decode step; the rows keep running
    assert eng.sched.num_running == B
    i32 = dict(dtype=torch.int32, device=dev)
    ks = {"lp_off": torch.full((B,), -1, **i32), "lp_k0": torch.zeros(B, **i32), "lp_k20": torch.full((B,), 20, **i32)}
    max_ctx = budget + 32
    # every window decodes the same ``iters`` steps from the same state (a later window would otherwise attend to a
    # longer context than an earlier one): the decode state is put back before each
    state = (r.gen_len, r.positions, r.input_ids, r.finished)
    snap = [t.clone() for t in state]

    def restore():
        for t, s0 in zip(state, snap):
            t.copy_(s0)

    def arm(name):
        def run():
            r.decode(B, 1, False, max_ctx=max_ctx, logprobs=name != "plain")
        return run

    runs = {name: arm(name) for name in arms}
    times = {k: [] for k in arms}
    for w in range(windows + 1):  # window 0 warms every graph up
        for name in arms:
            restore()
            if name != "plain":
                r.lp_k[:B].copy_(ks[name])
            t = timed(runs[name], iters)
            if w:
                times[name].append(t)
    V = r.V
    out = [row_of(ts, what="decode_step", model=model, V=V, B=B, case=k, iters=iters) for k, ts in times.items()]
    eng.abort_all("measurement over")
    del eng, r
    torch.cuda.empty_cache()
    return out


def spec_kernels(V, S, T, dev, iters, windows, hbm_gbs):
    """The verify-step pair standalone: every sequence asks K = 0 / K = 20 and records all T rows, or nobody asks."""
    g = torch.Generator().manual_seed(V + S * T)
    logits = (torch.randn(S * T, V, generator=g) * 2).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    max_new = 16
    st = dict(gen_len=torch.zeros(S, **i32), finished=torch.zeros(S, **i32), out_tokens=torch.zeros(S, max_new, **i32),
              lp_n0=torch.full((S,), -1, **i32), lp_tok=torch.zeros(S, max_new, device=dev),
              lp_ids=torch.zeros(S, max_new, ops.LOGPROB_KMAX, **i32),
              lp_top=torch.zeros(S, max_new, ops.LOGPROB_KMAX, device=dev))
    ws = ops.spec_logprob_workspace(V, dev)
    ks = {"k0": torch.zeros(S, **i32), "k20": torch.full((S,), 20, **i32), "off": torch.full((S,), -1, **i32)}
    rows = []

    def scan(k):
        return lambda: ops.spec_logprob_scan(logits, T, ks[k], st["finished"], st["gen_len"], st["lp_n0"], ws)

    for k, ts in alternate({k: scan(k) for k in ks}, iters, windows).items():
        r = row_of(ts, what="spec_logprob_scan", V=V, S=S, T=T, case=k, iters=iters)
        if k != "off":
            r["bytes"] = 2 * 4 * V * S * T
            r["hbm_share"] = round(r["bytes"] / (r["us_median"] * 1e-6) / (hbm_gbs * 1e9), 4)
        rows.append(r)
    # the verify commit does not consume lp_n0: after one scan (n0 = 0) every launch records T tokens per sequence
    scan("k20")()
    after = torch.full((S,), T, **i32)

    def commit(k):
        return lambda: ops.spec_logprob_commit(T, ks[k], st["lp_n0"], after, st["out_tokens"], st["lp_tok"],
                                               st["lp_ids"], st["lp_top"], ws)

    for k, ts in alternate({k: commit(k) for k in ks}, iters, windows).items():
        rows.append(row_of(ts, what="spec_logprob_commit", V=V, S=S, T=T, case=k, iters=iters))
    return rows


def spec_steps(model, S, dev, iters, windows, k=3):
    """The captured verify step of ``model`` over S sequences of T = k + 1 rows: the plain verify graph, the "lp" graph
    with nobody asking, all asking K = 0 and all asking K = 20; and the plain decode step of bucket S without and with
    logprobs (K = 20), for the acceptance a speculating request with logprobs needs."""
    from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

    arms = ("verify", "verify_lp_off", "verify_lp_k0", "verify_lp_k20", "plain", "plain_lp_k20")
    T = k + 1
    budget = iters * T + 64  # a window of ``iters`` verify steps commits at most iters * T tokens: nobody finishes
    eng = build_engine(model, device=dev, max_slots=max(S, 2), max_model_len=256 + budget, kv_reserve_tokens=-1,
                       logprobs=True, spec_tokens=k, spec_batch=S, spec_logprobs=True)
    r = eng.runner
    assert T == r.spec_k() + 1
    sp = SamplingParams(max_tokens=budget, ignore_eos=True, logprobs=True, top_logprobs=20)
    for i in range(S):
        eng.add_request([1] + list(range(10 + i, 138 + i)), sp)
    eng.run_ahead = 1
    eng.step()
    assert eng.sched.num_running == S and eng.stats["spec_steps"] > 0
    i32 = dict(dtype=torch.int32, device=dev)
    ks = {"off": torch.full((S,), -1, **i32), "k0": torch.zeros(S, **i32), "k20": torch.full((S,), 20, **i32)}
    max_ctx = 160 + budget
    state = (r.gen_len, r.positions, r.input_ids, r.finished)
    snap = [t.clone() for t in state]

    def restore():
        for t, s0 in zip(state, snap):
            t.copy_(s0)

    def run(name):
        if name.startswith("verify"):
            return lambda: r.decode_spec(1, max_ctx=max_ctx, S=r.bucket(S), logprobs=name != "verify")
        return lambda: r.decode(r.bucket(S), 1, False, max_ctx=max_ctx, logprobs=name != "plain")

    runs = {name: run(name) for name in arms}
    times = {name: [] for name in arms}
    for w in range(windows + 1):  # window 0 warms every graph up
        for name in arms:
            r.lp_k[:S].copy_(ks[name.rsplit("_", 1)[-1]] if "lp_" in name else ks["off"])
            restore()  # every window runs the same ``iters`` steps from the same state
            t = timed(runs[name], iters)
            if w:
                times[name].append(t)
    out = [row_of(ts, what="spec_step", model=model, V=r.V, S=S, T=T, case=name, iters=iters)
           for name, ts in times.items()]
    eng.abort_all("measurement over")
    del eng, r
    torch.cuda.empty_cache()
    return out


def prompt_kernels(V, dev, iters, windows, hbm_gbs):
    """The prompt pair standalone at R = 32 and 256, beside the plain scan at 32 rows, all in the same windows."""
    i32 = dict(dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(V)
    arms, meta = {}, {}
    for R in (32, 256):
        logits = (torch.randn(R, V, generator=g) * 2).to(dev)
        tg = torch.randint(V, (R,), generator=g).to(dev, torch.int32)
        ws = ops.prompt_logprob_workspace(R, V, dev)
        dst = (torch.zeros(R, device=dev), torch.zeros(R, ops.LOGPROB_KMAX, **i32),
               torch.zeros(R, ops.LOGPROB_KMAX, device=dev))
        for case, k, any_k in (("k0", torch.zeros(R, **i32), False), ("k20", torch.full((R,), 20, **i32), True)):
            def scan(logits=logits, tg=tg, k=k, ws=ws, any_k=any_k):
                ops.prompt_logprob_scan(logits, tg, k, workspace=ws, any_k=any_k)

            def commit(logits=logits, tg=tg, k=k, ws=ws, any_k=any_k, dst=dst):
                ops.prompt_logprob_commit(logits, tg, k, *dst, workspace=ws, any_k=any_k)

            ops.prompt_logprob_scan(logits, tg, k, workspace=ws, any_k=True)  # partials and candidates for the commit
            arms[f"scan R={R} {case}"], meta[f"scan R={R} {case}"] = scan, ("prompt_logprob_scan", R, case)
            arms[f"commit R={R} {case}"], meta[f"commit R={R} {case}"] = commit, ("prompt_logprob_commit", R, case)
    B = 32
    pl = (torch.randn(B, V, generator=g) * 2).to(dev)
    st = dict(gen_len=torch.zeros(B, **i32), finished=torch.zeros(B, **i32), lp_n0=torch.full((B,), -1, **i32),
              lp_raw=torch.zeros(B, V, device=dev), k0=torch.zeros(B, **i32))
    pws = ops.logprob_workspace(B, V, dev)
    arms["plain"] = lambda: ops.logprob_scan(pl, st["k0"], st["finished"], st["gen_len"], st["lp_raw"], st["lp_n0"],
                                             workspace=pws)
    meta["plain"] = ("logprob_scan (plain, the parent's body)", B, "k0")
    rows = []
    for name, ts in alternate(arms, iters, windows).items():
        what, R, case = meta[name]
        r = row_of(ts, what=what, V=V, R=R, case=case, iters=iters)
        r["us_per_row"] = round(r["us_median"] / R, 4)
        if what == "prompt_logprob_scan" and case == "k0":
            r["bytes"] = 4 * V * R  # one read of the rows; the partials are 8 bytes a chunk
            r["gb_per_s"] = round(r["bytes"] / (r["us_median"] * 1e-6) / 1e9, 1)
            r["hbm_share"] = round(r["gb_per_s"] / hbm_gbs, 4)
        rows.append(r)
    return rows


def prompt_exact(dev):
    """Worst |err| / (2^-24 (1 + |lse| + |l|)) of the prompt pair against float64, chosen and top-20 values."""
    out = {}
    for V, R in ((32000, 32), (128256, 32), (5000, 70)):
        g = torch.Generator().manual_seed(7 * V + R)
        lg = torch.randn(R, V, generator=g) * 3
        tg = torch.randint(V, (R,), generator=g).to(torch.int32)
        d = lg.double()
        lse = torch.logsumexp(d, -1)
        order = torch.sort(lg, dim=-1, descending=True, stable=True).indices[:, :20]
        dl = lg.to(dev)
        ws = ops.prompt_logprob_workspace(R, V, dev)
        dst = (torch.zeros(R, device=dev), torch.zeros(R, 20, dtype=torch.int32, device=dev), torch.zeros(R, 20, device=dev))
        k = torch.full((R,), 20, dtype=torch.int32, device=dev)
        ops.prompt_logprob_scan(dl, tg.to(dev), k, workspace=ws)
        ops.prompt_logprob_commit(dl, tg.to(dev), k, *dst, workspace=ws)
        tok, ids, top = (x.cpu() for x in dst)
        assert torch.equal(ids.long(), order)
        want_tok = d.gather(1, tg.long()[:, None])[:, 0] - lse
        want_top = d.gather(1, order) - lse[:, None]
        unit_tok = 2.0 ** -24 * (1 + lse.abs() + d.gather(1, tg.long()[:, None])[:, 0].abs())
        unit_top = 2.0 ** -24 * (1 + lse.abs()[:, None] + d.gather(1, order).abs())
        worst = max(float(((tok.double() - want_tok).abs() / unit_tok).max()),
                    float(((top.double() - want_top).abs() / unit_top).max()))
        out[f"prompt V={V},R={R},K=20"] = round(worst, 4)
    return {"unit": "2^-24 * (1 + |lse| + |l|), lse and l in float64", "bound": 8, "prompt_worst_ratio": out}


def prompt_ttft(model, n_prompt, dev, windows):
    """Time to first token of one ``n_prompt``-token prompt (max_tokens 1: prefill, first-token commit, host read):
    nobody asks / scored from the middle / scored whole, interleaved."""
    import time

    from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

    eng = build_engine(model, device=dev, max_slots=4, max_model_len=n_prompt + 64, logprobs=True)
    V = eng.runner.V
    g = torch.Generator().manual_seed(n_prompt)
    ids = [1] + torch.randint(5, min(V, 30000), (n_prompt - 1,), generator=g).tolist()
    arms = {"nobody": SamplingParams(max_tokens=1, ignore_eos=True),
            "from_middle": SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=True,
                                          prompt_logprobs_from=n_prompt // 2),
            "whole": SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=True)}
    times = {k: [] for k in arms}
    for w in range(windows + 1):  # window 0 warms up
        for name, sp in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = eng.add_request(ids, sp)
            eng.run_until_done([q])
            dt = (time.perf_counter() - t0) * 1e6
            res = eng.result(q)
            assert (res.prompt_logprobs is None) == (name == "nobody")
            if w:
                times[name].append(dt)
    out = [row_of(ts, what="ttft", model=model, V=V, prompt_tokens=n_prompt, case=k,
                  scored_rows={"nobody": 0, "from_middle": n_prompt - n_prompt // 2, "whole": n_prompt - 1}[k])
           for k, ts in times.items()]
    del eng
    torch.cuda.empty_cache()
    return out


def prompt_score_call(model, dev, windows, n_prompt=300, n_comp=8, comp_len=32):
    """The requests of one scoring call: ``n_comp`` completions of ``comp_len`` tokens after one ``n_prompt``-token
    prompt, submitted together (max_tokens 1, scored from the prompt's end), with the prompt's blocks in the prefix
    cache and, for comparison, on an engine without the cache."""
    import time

    from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

    out = []
    for cache in (True, False):
        eng = build_engine(model, device=dev, max_slots=8, max_model_len=n_prompt + comp_len + 64, logprobs=True,
                           prefix_cache=cache)
        V = eng.runner.V
        g = torch.Generator().manual_seed(3)
        ids = [1] + torch.randint(5, min(V, 30000), (n_prompt - 1,), generator=g).tolist()
        comps = [torch.randint(5, min(V, 30000), (comp_len,), generator=g).tolist() for _ in range(n_comp)]
        sp = SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=True, prompt_logprobs_from=n_prompt)
        ts, cached = [], 0
        for w in range(windows + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reqs = [eng.add_request(ids + c, sp) for c in comps]
            eng.run_until_done(reqs)
            res = [eng.result(q) for q in reqs]
            dt = (time.perf_counter() - t0) * 1e6
            assert all(sum(x is not None for x in r.prompt_logprobs) == comp_len for r in res)
            if w:
                ts.append(dt)
                cached = sum(r.cached_prompt_tokens for r in res)
        out.append(row_of(ts, what="score_call", model=model, V=V, prompt_tokens=n_prompt, completions=n_comp,
                          completion_tokens=comp_len, case="prefix_cache" if cache else "no_cache",
                          cached_prompt_tokens=cached))
        del eng
        torch.cuda.empty_cache()
    return out


def table(path):
    rows = [json.loads(x) for x in open(path)]
    print("| what | V | B | case | us median (min .. max) |")
    print("|---|---|---|---|---|")
    for r in rows:
        extra = f", {100 * r['hbm_share']:.1f} % of HBM" if "hbm_share" in r else ""
        rows_of = r["B"] if "B" in r else r["R"] if "R" in r else f"{r['S']} x {r['T']}" if "S" in r else "-"
        what = r["what"] + (f" {r['model']}" if "model" in r else "")
        print(f"| {what} | {r['V']} | {rows_of} | {r['case']} | {r['us_median']} ({r['us_min']} .. {r['us_max']})"
              f"{extra} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--spec", action="store_true", help="measure the verify-step pair (spec_logprobs) instead")
    ap.add_argument("--prompt", action="store_true", help="measure prompt-token logprobs (the prompt pair) instead")
    ap.add_argument("--exact-out", default="", help="--prompt: write the pair's worst exactness ratios here")
    args = ap.parse_args()
    if args.table:
        table(args.out)
        return 0
    if not torch.cuda.is_available():
        print("needs a GPU", file=sys.stderr)
        return 2
    dev = "cuda:0"
    with open(args.out, "a") as out:
        def emit(rows):
            for r in rows:
                print(json.dumps(r), flush=True)
                out.write(json.dumps(r) + "\n")
            out.flush()

        if args.prompt:
            if not args.no_kernels:
                for V in (32000, 128256):
                    emit(prompt_kernels(V, dev, args.iters, args.windows, args.hbm_gbs))
                if args.exact_out:
                    with open(args.exact_out, "w") as f:
                        json.dump(prompt_exact(dev), f, indent=1)
            if not args.no_steps:
                emit(prompt_ttft("llama3.2", 2048, dev, args.windows))
                emit(prompt_ttft("duckdb-nsql", 300, dev, args.windows))
                emit(prompt_score_call("duckdb-nsql", dev, args.windows))
            return 0
        if args.spec:
            if not args.no_kernels:
                for V in (32000, 128256):
                    for S, T in ((1, 4), (4, 8)):
                        emit(spec_kernels(V, S, T, dev, args.iters, args.windows, args.hbm_gbs))
            if not args.no_steps:
                for model in ("duckdb-nsql", "llama3.2"):
                    for S in (1, 4):
                        emit(spec_steps(model, S, dev, args.step_iters, args.windows))
            return 0
        if not args.no_kernels:
            for V in (32000, 128256):
                for B in (1, 32):
                    emit(kernels(V, B, dev, args.iters, args.windows, args.hbm_gbs))
        if not args.no_steps:
            for model in ("duckdb-nsql", "llama3.2"):
                for B in (1, 32):
                    emit(steps(model, B, dev, args.step_iters, args.windows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
