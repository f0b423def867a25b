"""Speculative decoding on MI355X: what a verify step costs and what it can gain.

  kernel   attn_verify (T rows of one sequence, one pass over the cache) against attn_decode over a bucket of T rows
           (T sequences' worth of cache reads) and against single-token attn_decode; achieved KV bytes/s.  The same
           shapes over the fp8 KV cache (e4m3 rows + per-row scales) beside the bf16 cache.
  step     device time of a verify step (k drafted tokens) against the plain batch-1 step on the same engine, with
           planted all-wrong drafts so both arms decode the same tokens; break-even acceptance = ratio - 1.
  e2e      tokens/s of a request at planted acceptance 0, about half, and all: the envelope.  (Random-init weights
           give no meaningful natural acceptance; real acceptance needs a checkpoint, LSA_CHECKPOINT_DIR.)

With --sampled: speculative decoding of requests that need the sampler (``spec_sampled``) instead, appended to
profiles/spec/spec_sampled_mi355x.jsonl:

  commit   device time of the sampled verify commit (ops.spec_sample_commit: penalty, partials, per-row pick, in-order
           commit) against the greedy one (ops.spec_commit) at the same T, and next to it the plain step's
           sample_commit minus argmax_commit at B = 1 from the same run: the extra cost should be of that order.
  e2e      tokens/s of ONE sampled request with Ollama's default options (temperature 0.8, top_k 40, top_p 0.9,
           repeat_penalty 1.1) and a fixed seed on the two prompts above: spec_sampled off (the plain sampled steps)
           against on with the n-gram drafter (its acceptance counts recorded) and with planted acceptance 0, about
           half, and all.

With --batch 2,4,8: speculative decoding of several greedy requests at once (``spec_batch``), k = 3, appended to
profiles/spec/spec_batch_mi355x.jsonl:

  kernel   attn_verify over S sequences in one launch beside S one-sequence launches and beside attn_decode at
           batch S (one row per sequence).
  step     device time of a verify step over S sequences (S x 4 rows, planted all-wrong drafts) against the plain
           step of bucket S decoding the same S requests; ratio - 1 = the accepted drafts per step and request at
           which the verify step breaks even.
  e2e      decode tokens/s of the S requests together: plain, and planted acceptance none / about half / all.

With --batch 2,4,8 --sampled: the same for requests that need the sampler (``spec_batch_sampled``), k = 3, Ollama's
default options and one seed per request, appended to profiles/spec/spec_batch_sampled_mi355x.jsonl:

  commit   device time of the sampled verify commit over S sequences (S x 4 rows) against the greedy ``spec_commit``
           at the same rows and against the plain step's ``sample_commit`` at batch S.
  step     device time of the sampled verify step over S sequences (planted all-wrong drafts) against the plain sampled
           step of bucket S; ratio - 1 = the break-even accepted drafts per step and request.
  e2e      decode tokens/s of the S sampled requests together: plain, and planted acceptance none / about half / all,
           planted from the verify path's own tokens.

Every graph is warmed, times are device events, the arms alternate within one process.  Appends JSON lines to
profiles/spec/spec_decode_mi355x.jsonl, or -- with quantised weights or the fp8 cache (``spec_quantized`` engines) --
to profiles/spec/spec_decode_quant_mi355x.jsonl (--out overrides).  Needs a GPU.

  python scripts/bench_spec.py [--layers N] [--skip kernel,step,e2e] [--reps 5] [--dtype bf16|fp8|mxfp4]
                               [--kv-dtype bf16|fp8] [--models duckdb-nsql,llama3.2] [--out FILE] [--sampled]
                               [--batch 2,4,8 [--sampled]]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llm_based_apache_spark_optimization_amd import ops  # noqa: E402
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams  # noqa: E402
from llm_based_apache_spark_optimization_amd.models import get_spec  # noqa: E402
from llm_based_apache_spark_optimization_amd.models.llama import init_random  # noqa: E402
from llm_based_apache_spark_optimization_amd.ops import reference as ref  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "spec", "spec_decode_mi355x.jsonl")
OUT_QUANT = os.path.join(ROOT, "profiles", "spec", "spec_decode_quant_mi355x.jsonl")
OUT_SAMPLED = os.path.join(ROOT, "profiles", "spec", "spec_sampled_mi355x.jsonl")
OUT_BATCH = os.path.join(ROOT, "profiles", "spec", "spec_batch_mi355x.jsonl")
OUT_BATCH_SAMPLED = os.path.join(ROOT, "profiles", "spec", "spec_batch_sampled_mi355x.jsonl")
OLLAMA = dict(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.1)  # Ollama's default option set


def emit(rec: dict) -> None:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def time_graph(fn, iters: int = 50) -> float:
    """us per call of fn, replayed from a captured graph of 10 calls (device events)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(10):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * 10)


def bench_kernel(dev, reps: int) -> None:
    D = 128
    for name, H, Hkv, ctxs in (("llama3.2-3b", 24, 8, (2048,)), ("duckdb-nsql-7b", 32, 32, (256, 2048))):
        G = H // Hkv
        for ctx in ctxs:
            for T in sorted({2, 4, min(8, 16 // G)}):
                mb = (ctx + T + 63) // 64 + 1
                g = torch.Generator().manual_seed(ctx + T)
                kc = (torch.randn(T * mb + 1, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
                vc = (torch.randn(T * mb + 1, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
                # the same rows in the fp8 cache: e4m3 bytes in the token-pair order + per-(token, kv-head) scales
                (k8, ks), (v8, vs) = ref.quant_kv_rows(kc.float()), ref.quant_kv_rows(vc.float())
                k8, v8 = ref.kv8_physical(k8).contiguous(), ref.kv8_physical(v8).contiguous()
                ks, vs = ks.contiguous(), vs.contiguous()
                bts = (torch.arange(T * mb, dtype=torch.int32) + 1).view(T, mb).to(dev)  # T disjoint sequences
                q = (torch.randn(T, H, D, generator=g) * 0.7).to(torch.bfloat16).to(dev)
                out = torch.zeros(T, H * D, dtype=torch.bfloat16, device=dev)
                pos0 = torch.tensor([ctx - T], dtype=torch.int32, device=dev)
                posT = torch.full((T,), ctx - 1, dtype=torch.int32, device=dev)
                plan = ops.verify_split_plan(Hkv, ctx)
                ws = ops.verify_workspace(T, H, Hkv, plan[1], dev)
                planT = ops.decode_split_plan(T, Hkv, ctx)
                wsT = ops.decode_workspace(T, H, Hkv, planT[1], dev)
                arms = {
                    "verify": lambda: ops.attn_verify(q, kc, vc, bts[:1], pos0, H, Hkv, D ** -0.5, out, workspace=ws,
                                                      plan=plan),
                    "verify_fp8": lambda: ops.attn_verify(q, k8, v8, bts[:1], pos0, H, Hkv, D ** -0.5, out,
                                                          workspace=ws, plan=plan, kv_scales=(ks, vs)),
                    "decode_T_rows": lambda: ops.attn_decode(q, kc, vc, bts, posT, H, Hkv, D ** -0.5, out.view(T, H, D),
                                                             workspace=wsT, plan=planT),
                    "decode_1_row": lambda: ops.attn_decode(q[:1], kc, vc, bts[:1], posT[:1], H, Hkv, D ** -0.5,
                                                            out[:1].view(1, H, D), workspace=ws, plan=plan),
                }
                us = {k: [] for k in arms}
                for _ in range(reps):  # alternate the arms
                    for k, fn in arms.items():
                        us[k].append(time_graph(fn))
                med = {k: round(statistics.median(v), 2) for k, v in us.items()}
                kv_bytes = 2 * Hkv * ctx * D * 2
                emit(dict(bench="kernel", model=name, H=H, Hkv=Hkv, ctx=ctx, T=T, us=med,
                          verify_over_decode1=round(med["verify"] / med["decode_1_row"], 3),
                          verify_over_decodeT=round(med["verify"] / med["decode_T_rows"], 3),
                          verify_kv_GBps=round(kv_bytes / med["verify"] / 1e3, 1),
                          verify_fp8_over_bf16=round(med["verify_fp8"] / med["verify"], 3),
                          verify_fp8_kv_GBps=round(kv_bytes * (D + 4) / (2 * D) / med["verify_fp8"] / 1e3, 1)))


def forced(toks, kind: str, k: int, V: int) -> torch.Tensor:
    n = len(toks)
    right = lambda i: toks[i] if i < n else 0  # noqa: E731
    rows = []
    for g in range(n + 1):
        if kind == "all":
            rows.append([right(g + i) for i in range(k)])
        elif kind == "none":
            rows.append([(right(g + i) + 1) % V for i in range(k)])
        else:  # about half: the first ceil(k / 2) right
            h = (k + 1) // 2
            rows.append([right(g + i) if i < h else (right(g + i) + 1) % V for i in range(k)])
    return torch.tensor(rows, dtype=torch.int32)


def bench_engine(dev, layers, reps: int, skip, dtype: str = "bf16", kv_dtype: str = "bf16", models=()) -> None:
    for base, plen, new in (("duckdb-nsql", 128, 128), ("llama3.2", 2048, 128)):
        if models and base not in models:
            continue
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5, kind=dtype)
        # quantised weights / the fp8 cache: the verify rows run the weight-only GEMMs (opt-in, spec_quantized)
        r = ModelRunner(w, max_slots=2, max_model_len=plen + new + 64, num_kv_blocks=2 * ((plen + new) // 64 + 3),
                        kv_dtype=kv_dtype, spec_quantized=(dtype, kv_dtype) != ("bf16", "bf16"))
        eng = LLMEngine(r, name=spec.name)
        g = torch.Generator().manual_seed(7)
        ids = [1] + torch.randint(3, 30000, (plen - 1,), generator=g).tolist()
        sp = SamplingParams(max_tokens=new, ignore_eos=True)

        def run(k: int, kind: str, toks=None):
            """(tokens, decode device s, decode steps, tokens / s of the decode phase) of one request."""
            r.spec_tokens = k
            r.set_spec_forced(None if not k else forced(toks, kind, r.spec_k(), spec.vocab_size))
            d0, n0 = eng.stats["decode_device_s"], eng.stats["decode_steps"]
            out = eng.generate([ids], sp)[0].token_ids
            ds, ns = eng.stats["decode_device_s"] - d0, eng.stats["decode_steps"] - n0
            return out, ds, ns, (len(out) - 1) / ds

        toks = run(0, "")[0]  # warms the plain graphs
        kmax = min(7, 16 // (r.H // r.Hkv) - 1)
        ks = sorted({1, 3, kmax})
        for k in ks:
            run(k, "none", toks)  # warms the verify graphs
        if "step" not in skip:
            plain, ver = [], {k: [] for k in ks}
            for _ in range(reps):
                _, ds, ns, _ = run(0, "")
                plain.append(ds / ns)
                for k in ks:
                    out, ds, ns, _ = run(k, "none", toks)
                    assert ns == new - 1, (ns, "all-wrong drafts commit one token per step")
                    ver[k].append(ds / ns)
            p = statistics.median(plain)
            for k in ks:
                v = statistics.median(ver[k])
                emit(dict(bench="step", model=spec.name, dtype=dtype, kv_dtype=kv_dtype, a8_plan_b1=list(r.a8_plan(1)),
                          rr_a8=bool(r.rr_decode and r.rr_a8), layers=spec.n_layers, prompt=plen, new=new, k=k,
                          plain_step_ms=round(p * 1e3, 4), verify_step_ms=round(v * 1e3, 4),
                          break_even_accept=round(v / p - 1, 3), tokens_equal=out == toks))
        if "e2e" not in skip:
            res = {}
            # the planted drafts follow the verify path's own greedy tokens (at random-init margins they can leave the
            # plain run's after a few tokens, and drafts built from the plain run would then never be accepted)
            toks = run(3, "none", toks)[0]
            for _ in range(reps):
                res.setdefault("plain", []).append(run(0, "")[3])
                for kind in ("none", "half", "all"):
                    out, _, ns, tps = run(3, kind, toks)
                    res.setdefault(kind, []).append(tps)
                    res[kind + "_steps"] = ns
            emit(dict(bench="e2e", model=spec.name, dtype=dtype, kv_dtype=kv_dtype, layers=spec.n_layers, prompt=plen,
                      new=new, k=3,
                      decode_tok_s={k: round(statistics.median(v), 1) for k, v in res.items() if not k.endswith("_steps")},
                      verify_steps={k[:-6]: v for k, v in res.items() if k.endswith("_steps")}))
        del eng, r, w
        torch.cuda.empty_cache()


def bench_sampled_commit(dev, reps: int, models=()) -> None:
    """The verify commits alone, over static rows: every launch commits one token (the drafts are -1)."""
    W, max_new = 64, 8192  # ~520 launches per arm and measurement: no row reaches its limit
    for base in ("duckdb-nsql", "llama3.2"):
        if models and base not in models:
            continue
        V = get_spec(base).vocab_size
        g = torch.Generator().manual_seed(V)
        logits0 = (torch.randn(8, V, generator=g) * 2).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        par = dict(hist=torch.randint(0, V, (1, W), generator=g, dtype=torch.int32).to(dev),
                   pen=torch.tensor([OLLAMA["repeat_penalty"]], device=dev), last_n=torch.tensor([W], **i32),
                   temp=torch.tensor([OLLAMA["temperature"]], device=dev), top_k=torch.tensor([OLLAMA["top_k"]], **i32),
                   top_p=torch.tensor([OLLAMA["top_p"]], device=dev),
                   seeds=torch.tensor([ref.pack_seed(17, 0)], dtype=torch.int64, device=dev))
        eos = torch.tensor([-1], **i32)
        draft = torch.full((8,), -1, **i32)
        part = torch.zeros(8 * ((V + 4095) // 4096), dtype=torch.int64, device=dev)
        cand = torch.zeros(8 * ((V + 2047) // 2048) * 64, dtype=torch.int64, device=dev)
        picks = torch.zeros(8, **i32)

        def state():
            return (torch.zeros(1, max_new, **i32), torch.zeros(1, **i32), torch.zeros(1, **i32),
                    torch.full((1,), 100, **i32), torch.zeros(1, **i32))

        def arm(kind: str, T: int):
            st, stats, lg = state(), torch.zeros(3, dtype=torch.int64, device=dev), logits0[:T].clone()
            if kind == "spec_sampled":
                return lambda: ops.spec_sample_commit(lg, draft[:T - 1], stats, par["hist"], par["pen"], par["temp"],
                                                      par["top_k"], par["top_p"], par["seeds"], *st, eos,
                                                      workspace=(part, cand, picks), last_n=par["last_n"])
            if kind == "spec_greedy":
                return lambda: ops.spec_commit(lg, draft[:T - 1], stats, *st, eos, part=part)
            if kind == "plain_sampled":
                return lambda: ops.sample_commit(lg, par["hist"], par["pen"], par["temp"], par["top_k"], par["top_p"],
                                                 par["seeds"], *st, eos, workspace=(part, cand), last_n=par["last_n"])
            return lambda: ops.argmax_commit(lg, *st, eos, part=part)

        us = {}
        for _ in range(reps):  # alternate the arms
            for kind, T in [("plain_greedy", 1), ("plain_sampled", 1)] + [(k, T) for T in (2, 4, 8)
                                                                         for k in ("spec_greedy", "spec_sampled")]:
                us.setdefault(f"{kind}_T{T}", []).append(time_graph(arm(kind, T)))
        med = {k: round(statistics.median(v), 2) for k, v in us.items()}
        plain_extra = med["plain_sampled_T1"] - med["plain_greedy_T1"]
        emit(dict(bench="sampled_commit", model=base, V=V, us=med, plain_extra_us=round(plain_extra, 2),
                  verify_extra_us={T: round(med[f"spec_sampled_T{T}"] - med[f"spec_greedy_T{T}"], 2) for T in (2, 4, 8)},
                  verify_extra_over_plain_extra={T: round((med[f"spec_sampled_T{T}"] - med[f"spec_greedy_T{T}"])
                                                          / plain_extra, 2) for T in (2, 4, 8)}))


def bench_sampled_engine(dev, layers, reps: int, models=(), k: int = 3, seed: int = 11) -> None:
    for base, plen, new in (("duckdb-nsql", 128, 128), ("llama3.2", 2048, 128)):
        if models and base not in models:
            continue
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5)
        r = ModelRunner(w, max_slots=2, max_model_len=plen + new + 64, num_kv_blocks=2 * ((plen + new) // 64 + 3),
                        spec_tokens=k, spec_sampled=True)
        eng = LLMEngine(r, name=spec.name)
        g = torch.Generator().manual_seed(7)
        ids = [1] + torch.randint(3, 30000, (plen - 1,), generator=g).tolist()
        sp = SamplingParams(max_tokens=new, ignore_eos=True, seed=seed, **OLLAMA)

        def run(on: bool, kind: str = "", toks=None):
            """(tokens, decode steps, tokens / s of the decode phase, (verify steps, drafted, accepted))."""
            r.spec_sampled = on
            r.set_spec_forced(None if not kind else forced(toks, kind, r.spec_k(), spec.vocab_size))
            d0, n0, c0 = eng.stats["decode_device_s"], eng.stats["decode_steps"], r.spec_counts()
            out = eng.generate([ids], sp)[0].token_ids
            ds, ns = eng.stats["decode_device_s"] - d0, eng.stats["decode_steps"] - n0
            return out, ns, (len(out) - 1) / ds, [a - b for a, b in zip(r.spec_counts(), c0)]

        plain = run(False)[0]     # warms the plain sampled graphs
        toks = run(True)[0]       # ... and the sampled verify graph (n-gram drafts): the verify path's own tokens
        res, counts, same = {}, {}, {}
        for _ in range(reps):
            for name, args in (("off", (False,)), ("ngram", (True,)), ("none", (True, "none", toks)),
                               ("half", (True, "half", toks)), ("all", (True, "all", toks))):
                out, ns, tps, c = run(*args)
                res.setdefault(name, []).append(tps)
                counts[name] = dict(decode_steps=ns, verify_steps=c[0], drafted=c[1], accepted=c[2])
                same[name] = out == (plain if name == "off" else toks)
        tok_s = {n: round(statistics.median(v), 1) for n, v in res.items()}
        emit(dict(bench="sampled_e2e", model=spec.name, layers=spec.n_layers, prompt=plen, new=new, k=r.spec_k(),
                  options=OLLAMA, seed=seed, decode_tok_s=tok_s, counts=counts, tokens_repeat=same,
                  verify_tokens_equal_plain=toks == plain,
                  speedup_over_off={n: round(v / tok_s["off"], 3) for n, v in tok_s.items()}))
        del eng, r, w
        torch.cuda.empty_cache()


def bench_batch_kernel(dev, reps: int, Ss, T: int = 4) -> None:
    """attn_verify over S sequences of T rows: one launch, S one-sequence launches, and attn_decode at batch S."""
    D = 128
    for name, H, Hkv, ctx in (("duckdb-nsql-7b", 32, 32, 256), ("llama3.2-3b", 24, 8, 2176)):
        for S in Ss:
            mb = (ctx + 63) // 64 + 1
            g = torch.Generator().manual_seed(ctx + S)
            kc = (torch.randn(S * mb + 1, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            vc = (torch.randn(S * mb + 1, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            bts = (torch.arange(S * mb, dtype=torch.int32) + 1).view(S, mb).to(dev)  # S disjoint sequences
            q = (torch.randn(S, T, H, D, generator=g) * 0.7).to(torch.bfloat16).to(dev)
            out = torch.zeros(S * T, H * D, dtype=torch.bfloat16, device=dev)
            pos0 = torch.full((S,), ctx - T, dtype=torch.int32, device=dev)
            posS = torch.full((S,), ctx - 1, dtype=torch.int32, device=dev)
            planS, plan1 = ops.verify_split_plan(Hkv, ctx, S), ops.verify_split_plan(Hkv, ctx)
            wsS = ops.verify_workspace(T, H, Hkv, planS[1], dev, S=S)
            ws1 = ops.verify_workspace(T, H, Hkv, plan1[1], dev)
            planD = ops.decode_split_plan(S, Hkv, ctx)
            wsD = ops.decode_workspace(S, H, Hkv, planD[1], dev)
            q1 = q[:, 0].contiguous()

            def one_by_one():
                for s_ in range(S):
                    ops.attn_verify(q[s_], kc, vc, bts[s_:s_ + 1], pos0[s_:s_ + 1], H, Hkv, D ** -0.5,
                                    out[s_ * T:(s_ + 1) * T], workspace=ws1, plan=plan1)

            arms = {
                "verify_S": lambda: ops.attn_verify(q, kc, vc, bts, pos0, H, Hkv, D ** -0.5, out, workspace=wsS, plan=planS),
                "verify_1_x_S": one_by_one,
                "decode_batch_S": lambda: ops.attn_decode(q1, kc, vc, bts, posS, H, Hkv, D ** -0.5,
                                                          out[:S].view(S, H, D), workspace=wsD, plan=planD),
            }
            us = {k: [] for k in arms}
            for _ in range(reps):  # alternate the arms
                for k, fn in arms.items():
                    us[k].append(time_graph(fn))
            med = {k: round(statistics.median(v), 2) for k, v in us.items()}
            emit(dict(bench="batch_kernel", model=name, H=H, Hkv=Hkv, ctx=ctx, S=S, T=T, plan=list(planS), us=med,
                      verify_S_over_1_x_S=round(med["verify_S"] / med["verify_1_x_S"], 3),
                      verify_S_over_decode_S=round(med["verify_S"] / med["decode_batch_S"], 3)))


def bench_batch_sampled_commit(dev, reps: int, Ss, models=(), T: int = 4) -> None:
    """The commits alone, over static rows: every launch commits one token per sequence (the drafts are -1)."""
    W, max_new = 64, 8192  # ~520 launches per arm and measurement: no row reaches its limit
    for base in ("duckdb-nsql", "llama3.2"):
        if models and base not in models:
            continue
        V = get_spec(base).vocab_size
        g = torch.Generator().manual_seed(V)
        SM = max(Ss)
        logits0 = (torch.randn(SM * T, V, generator=g) * 2).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        hist = torch.randint(0, V, (SM, W), generator=g, dtype=torch.int32).to(dev)
        pen, last_n = torch.full((SM,), OLLAMA["repeat_penalty"], device=dev), torch.full((SM,), W, **i32)
        temp = torch.full((SM,), OLLAMA["temperature"], device=dev)
        top_p = torch.full((SM,), OLLAMA["top_p"], device=dev)
        top_k = torch.full((SM,), OLLAMA["top_k"], **i32)
        seeds = torch.tensor([ref.pack_seed(17 + s_, 0) for s_ in range(SM)], dtype=torch.int64, device=dev)
        eos = torch.tensor([-1], **i32)
        draft = torch.full((SM * T,), -1, **i32)
        part = torch.zeros(SM * T * ((V + 4095) // 4096), dtype=torch.int64, device=dev)
        cand = torch.zeros(SM * T * ((V + 2047) // 2048) * 64, dtype=torch.int64, device=dev)
        picks = torch.zeros(SM * T, **i32)
        for S in Ss:
            def state():
                return (torch.zeros(S, max_new, **i32), torch.zeros(S, **i32), torch.zeros(S, **i32),
                        torch.full((S,), 100, **i32), torch.zeros(S, **i32))

            def arm(kind: str):
                st, stats = state(), torch.zeros(S, 3, dtype=torch.int64, device=dev)
                if kind == "spec_sampled":
                    lg = logits0[:S * T].clone()
                    return lambda: ops.spec_sample_commit(lg, draft[:S * (T - 1)], stats if S > 1 else stats[0],
                                                          hist[:S], pen[:S], temp[:S], top_k[:S], top_p[:S], seeds[:S], *st, eos,
                                                          workspace=(part, cand, picks), last_n=last_n[:S])
                if kind == "spec_greedy":
                    lg = logits0[:S * T].clone()
                    return lambda: ops.spec_commit(lg, draft[:S * (T - 1)], stats if S > 1 else stats[0], *st, eos,
                                                   part=part)
                lg = logits0[:S].clone()
                return lambda: ops.sample_commit(lg, hist[:S], pen[:S], temp[:S], top_k[:S], top_p[:S], seeds[:S], *st,
                                                 eos, workspace=(part, cand), last_n=last_n[:S])

            us = {}
            for _ in range(reps):  # alternate the arms
                for kind in ("spec_greedy", "spec_sampled", "plain_sampled"):
                    us.setdefault(kind, []).append(time_graph(arm(kind)))
            med = {k_: round(statistics.median(v), 2) for k_, v in us.items()}
            emit(dict(bench="batch_sampled_commit", model=base, V=V, S=S, T=T, rows=S * T, us=med,
                      sampled_over_greedy_us=round(med["spec_sampled"] - med["spec_greedy"], 2),
                      sampled_over_plain_batch_S_us=round(med["spec_sampled"] - med["plain_sampled"], 2)))


def bench_batch_engine(dev, layers, reps: int, skip, Ss, models=(), k: int = 3, sampled: bool = False,
                       seed: int = 11) -> None:
    """The verify step over S sequences against the plain step of bucket S, and the planted-draft envelope.  ``sampled``:
    every request runs with Ollama's default options and its own seed (``spec_batch_sampled``): the sampled verify step
    against the plain sampled step."""
    for base, plen, new in (("duckdb-nsql", 128, 128), ("llama3.2", 2048, 128)):
        if models and base not in models:
            continue
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5)
        SM = max(Ss)
        r = ModelRunner(w, max_slots=SM, max_model_len=plen + new + 64, num_kv_blocks=SM * ((plen + new) // 64 + 3) + 1,
                        spec_tokens=k, spec_batch=SM, spec_sampled=sampled, spec_batch_sampled=sampled)
        eng = LLMEngine(r, name=spec.name, max_prefill_tokens=SM * plen + 64)
        T = r.spec_k() + 1
        g = torch.Generator().manual_seed(7)
        prompts = [[1] + torch.randint(3, 30000, (plen - 1,), generator=g).tolist() for _ in range(SM)]
        for S in Ss:
            if S > r.spec_s():
                continue
            ids = prompts[:S]

            def run(kind: str, toks=None):
                """(tokens per request, decode device s, decode steps, decode tokens / s of the S requests)."""
                sps = [SamplingParams(max_tokens=new, ignore_eos=True, speculate=bool(kind),
                                      **(dict(seed=seed + s_, **OLLAMA) if sampled else {})) for s_ in range(S)]
                if kind:
                    tab = torch.zeros(r.spec_s(), new + 1, T - 1, dtype=torch.int32)
                    for s_ in range(S):
                        tab[s_] = forced(toks[s_], kind, T - 1, spec.vocab_size)
                    r.set_spec_forced(tab)
                d0, n0 = eng.stats["decode_device_s"], eng.stats["decode_steps"]
                reqs = [eng.add_request(p_, sp) for p_, sp in zip(ids, sps)]
                eng.run_until_done(reqs)
                out = [q.output_ids for q in reqs]
                ds, ns = eng.stats["decode_device_s"] - d0, eng.stats["decode_steps"] - n0
                return out, ds, ns, sum(len(o) - 1 for o in out) / ds

            plain_toks = run("")[0]               # warms the plain graphs of bucket S
            toks = run("none", plain_toks)[0]     # warms the verify graph; the verify path's own greedy tokens
            if "step" not in skip:
                plain, ver, steps, same = [], [], 0, True
                for _ in range(reps):
                    _, ds, ns, _ = run("")
                    plain.append(ds / ns)
                    out, ds, steps, _ = run("none", toks)
                    ver.append(ds / steps)
                    same = same and out == toks
                p, v = statistics.median(plain), statistics.median(ver)
                emit(dict(bench="batch_sampled_step" if sampled else "batch_step", model=spec.name,
                          layers=spec.n_layers, prompt=plen, new=new, k=T - 1, S=S,
                          rows=S * T, plain_step_ms=round(p * 1e3, 4), verify_step_ms=round(v * 1e3, 4),
                          break_even_accept=round(v / p - 1, 3), verify_steps=steps, tokens_repeat=same,
                          verify_tokens_equal_plain=toks == plain_toks))
            if "e2e" not in skip:
                res = {}
                for _ in range(reps):
                    res.setdefault("plain", []).append(run("")[3])
                    for kind in ("none", "half", "all"):
                        _, _, ns, tps = run(kind, toks)
                        res.setdefault(kind, []).append(tps)
                        res[kind + "_steps"] = ns
                tok_s = {n: round(statistics.median(v), 1) for n, v in res.items() if not n.endswith("_steps")}
                emit(dict(bench="batch_sampled_e2e" if sampled else "batch_e2e", model=spec.name,
                          layers=spec.n_layers, prompt=plen, new=new, k=T - 1, S=S,
                          decode_tok_s=tok_s, speedup_over_plain={n: round(v / tok_s["plain"], 3) for n, v in tok_s.items()},
                          verify_steps={n[:-6]: v for n, v in res.items() if n.endswith("_steps")}))
        del eng, r, w
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="truncate the models to this many layers (0 = full depth)")
    ap.add_argument("--skip", default="", help="comma list of kernel,step,e2e")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8", "mxfp4"), help="weight format of the engines")
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"), help="KV cache dtype of the engines")
    ap.add_argument("--models", default="", help="comma list of duckdb-nsql,llama3.2 (default both)")
    ap.add_argument("--out", default="", help="JSON-lines file to append to")
    ap.add_argument("--sampled", action="store_true", help="measure spec_sampled (sampled verify commit, sampled request)")
    ap.add_argument("--batch", default="", help="comma list of S: measure spec_batch at S concurrent greedy requests")
    a = ap.parse_args()
    global OUT
    OUT = a.out or (OUT_BATCH_SAMPLED if a.batch and a.sampled else OUT_BATCH if a.batch
                    else OUT_SAMPLED if a.sampled else OUT if (a.dtype, a.kv_dtype) == ("bf16", "bf16") else OUT_QUANT)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec.py needs a GPU")
    ops.ext()
    dev = torch.device("cuda:0")
    skip = set(a.skip.split(",")) if a.skip else set()
    if a.batch:
        Ss = [int(x) for x in a.batch.split(",") if x]
        models = tuple(m for m in a.models.split(",") if m)
        if "kernel" not in skip and a.sampled:
            bench_batch_sampled_commit(dev, a.reps, Ss, models)
        elif "kernel" not in skip:
            bench_batch_kernel(dev, a.reps, Ss)
        if not {"step", "e2e"} <= skip:
            bench_batch_engine(dev, a.layers, a.reps, skip, Ss, models, sampled=a.sampled)
        return
    if a.sampled:
        models = tuple(m for m in a.models.split(",") if m)
        if "kernel" not in skip:
            bench_sampled_commit(dev, a.reps, models)
        if "e2e" not in skip:
            bench_sampled_engine(dev, a.layers, a.reps, models)
        return
    if "kernel" not in skip:
        bench_kernel(dev, a.reps)
    if not {"step", "e2e"} <= skip:
        bench_engine(dev, a.layers, a.reps, skip, a.dtype, a.kv_dtype,
                     tuple(m for m in a.models.split(",") if m))


if __name__ == "__main__":
    main()
