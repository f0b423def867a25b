"""Regex-constrained decoding on MI355X: what the device-side token mask costs.

  kernel   ops.dfa_mask standalone (device us, captured-graph replays) at V = 32,000 and 128,256, B = 1 and 32, for
           prompts.SQL_STATEMENT_REGEX (nearly every token stays alive, so every token is walked to its end) and for a
           pattern at the table-size limit (S * C = 32768: the whole 64 KiB table is staged, most tokens die on their
           first byte), beside ops.argmax_commit over the same logits (argmax_partial_kernel + the commit: one read
           of the same rows).  The vocabulary is synthetic with the length profile of a BPE vocabulary: the 256
           single bytes, then space-prefixed words of 2..12 bytes.
  step     device time of a decode step replayed from the guided graph against the plain graph of the same engine, on
           the same rows: duckdb-nsql-7B at batch 1 and batch 32 (128-token prompts), Llama-3.2-3B at batch 1 with a
           2k-token prompt (the explain shape).  Every row carries the SQL pattern; 16-step runs in the order guided,
           plain, plain, guided (the context grows with every run; the order cancels it), means of 2 x --reps runs
           each.  The plain graph commits tokens the DFA never saw, so every guided run restarts the rows' lazy
           advance inside the statement, as a re-admission would.

With --spec: speculative decoding of constrained requests (``spec_guided``) instead, appended to
profiles/spec/spec_guided_mi355x.jsonl:

  kernel   ops.dfa_mask_verify over the T verify rows (T = 2 / 4 / 8 at V = 32,000, T = 2 / 4 / 5 at V = 128,256) beside
           the unchanged ops.dfa_mask at B = T on the same logits, every row in the state the verify row is in (the
           baseline: the new kernel adds only the draft walk), for both patterns, with drafts the pattern allows.
  step     one constrained request per model and k, planted drafts that the pattern allows (rows 1..k are masked in
           live states; the random-init model accepts next to none, so every arm commits about one token per step):
           the guided verify step against the unguided verify step (what the mask of T rows and the hand-over cost),
           and against the plain guided step (what a constrained request pays today): the break-even accepted drafts
           per step of a constrained request = guided verify / plain guided - 1.  16-step runs in a mirrored order.

With --spec-batch: speculative decoding of several requests of which some are constrained (``spec_batch_guided``),
appended to profiles/spec/spec_batch_guided_mi355x.jsonl:

  kernel   the S-sequence form of ops.dfa_mask_verify beside the unchanged ops.dfa_mask at B = S * T on the same logits,
           every baseline row in the state its verify row is in: (S, T) = (2, 4), (4, 4), (4, 8) at V = 32,000 and (4, 5)
           at V = 128,256, both patterns, every sequence constrained; and one record per shape with half the sequences
           unconstrained (g_on = 0 in both arms), which shows the early return.
  step     S constrained requests per model (duckdb-nsql-7B 128-token prompts, Llama-3.2-3B 2k-token prompts; S = 2 and
           4, k = 3), planted drafts that the pattern allows: the guided batched verify step against the unguided
           batched verify step (what the mask of S * T rows and the hand-over cost) and against the plain guided step
           of bucket S (what S constrained requests pay without the flag): the break-even accepted drafts per step and
           request of a constrained batch = guided batched verify / plain guided - 1.  16-step runs, mirrored order.

Appends JSON lines to profiles/guided/guided_mask_mi355x.jsonl (--out overrides).  Needs a GPU.

  python scripts/bench_guided.py [--spec | --spec-batch] [--layers N] [--skip kernel,step] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llm_based_apache_spark_optimization_amd import ops, prompts  # noqa: E402
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams  # noqa: E402
from llm_based_apache_spark_optimization_amd.engine.guided import DEAD, MAX_TABLE, compile_regex  # noqa: E402
from llm_based_apache_spark_optimization_amd.models import get_spec  # noqa: E402
from llm_based_apache_spark_optimization_amd.models.llama import init_random  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "guided", "guided_mask_mi355x.jsonl")
OUT_SPEC = os.path.join(ROOT, "profiles", "spec", "spec_guided_mi355x.jsonl")
OUT_SPEC_BATCH = os.path.join(ROOT, "profiles", "spec", "spec_batch_guided_mi355x.jsonl")
LIMIT_PATTERN = r"(abcdefghijklmnopqrstuvwxyz01234){33}"  # 1024 states x 32 classes


def emit(rec: dict) -> None:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def time_graph(fn, iters: int = 30) -> float:
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


def synthetic_vocab(V: int, seed: int = 0):
    """(offsets int32 [V + 1], blob uint8) of a BPE-like vocabulary: ids 0..2 empty (specials), 256 single bytes,
    then words of 2..12 bytes (mean ~6), half of them space-prefixed."""
    rng = random.Random(seed)
    letters = b"etaoinsrhldcumfpgwybvkxjqzETAOINSRHLDCUM0123456789_(),.*=<>'\""
    words = [b"", b"", b""] + [bytes([b]) for b in range(256)]
    while len(words) < V:
        n = min(12, max(2, int(rng.gauss(6, 2.5))))
        w = bytes(rng.choice(letters) for _ in range(n))
        words.append(b" " + w[:-1] if rng.random() < 0.5 else w)
    lens = [len(w) for w in words]
    off = torch.cumsum(torch.tensor([0] + lens, dtype=torch.int64), 0).to(torch.int32)
    blob = torch.frombuffer(bytearray(b"".join(words)), dtype=torch.uint8).clone()
    return off, blob


def tables(dfa, slots: int, dev, state: int):
    cls = torch.zeros(slots, 256, dtype=torch.uint8)
    trans = torch.full((slots, MAX_TABLE), -1, dtype=torch.int16)
    accept = torch.zeros(slots, MAX_TABLE, dtype=torch.uint8)
    sc = dfa.n_states * dfa.n_classes
    cls[:] = torch.from_numpy(dfa.cls)
    trans[:, :sc] = torch.from_numpy(dfa.trans.view("int16"))
    accept[:, : dfa.n_states] = torch.from_numpy(dfa.accept)
    dim = torch.tensor([[dfa.n_states, dfa.n_classes]] * slots, dtype=torch.int32)
    st = torch.full((slots, 2), state, dtype=torch.int32)
    return [t.to(dev) for t in (cls, trans, accept, dim, torch.ones(slots, dtype=torch.int32), st,
                                torch.zeros(slots, dtype=torch.int32))]


def bench_kernel(dev) -> None:
    sql = compile_regex(prompts.SQL_STATEMENT_REGEX)
    lim = compile_regex(LIMIT_PATTERN)
    cases = (("sql", sql, sql.walk(sql.start, b"SELECT ")), ("limit", lim, lim.walk(lim.start, b"abc")))
    for V in (32000, 128256):
        off, blob = synthetic_vocab(V)
        off, blob = off.to(dev), blob.to(dev)
        for B in (1, 32):
            i32 = dict(dtype=torch.int32, device=dev)
            logits = torch.randn(B, V, device=dev)
            z = torch.zeros(B, **i32)
            eos = torch.tensor([2], **i32)
            out_tokens = torch.zeros(B, 8, **i32)
            part = torch.zeros(B * ((V + 4095) // 4096), dtype=torch.int64, device=dev)
            st = [out_tokens, torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32), torch.ones(B, **i32)]
            t_arg = time_graph(lambda: ops.argmax_commit(logits, *st, eos, part=part))
            for name, dfa, state in cases:
                cls, trans, accept, dim, on, gst, base = tables(dfa, B, dev, state)
                work = logits.clone()
                t = time_graph(lambda: ops.dfa_mask(work, off, blob, cls, trans, accept, dim, on, gst, base, z, z, z,
                                                    eos))
                alive = int(torch.isfinite(work).sum()) // B
                emit(dict(bench="kernel", V=V, B=B, pattern=name, states=dfa.n_states, classes=dfa.n_classes,
                          table_bytes=2 * dfa.n_states * dfa.n_classes, blob_bytes=int(blob.numel()),
                          tokens_alive_per_row=alive, dfa_mask_us=round(t, 2), argmax_commit_us=round(t_arg, 2),
                          ratio=round(t / t_arg, 2)))


def bench_step(dev, layers: int, reps: int) -> None:
    for base, B, plen in (("duckdb-nsql", 1, 128), ("duckdb-nsql", 32, 128), ("llama3.2", 1, 2048)):
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5, kind="bf16")
        new, run = 1024, 16
        r = ModelRunner(w, max_slots=B, max_model_len=plen + new + 64, num_kv_blocks=B * ((plen + new) // 64 + 2) + 1)
        r.enable_guided(*synthetic_vocab(spec.vocab_size))
        eng = LLMEngine(r, name=spec.name, kv_reserve_tokens=-1, guided=True)  # every KV block reserved at admission
        g = torch.Generator().manual_seed(7)
        sp = SamplingParams(max_tokens=new, regex=prompts.SQL_STATEMENT_REGEX)
        for _ in range(B):
            eng.add_request([1] + torch.randint(3, spec.vocab_size, (plen - 1,), generator=g).tolist(), sp)
        eng.step()  # prefill (the first token obeys the pattern) + one guided decode run
        ctx = plen + new

        def timed(guided: bool) -> float:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.decode(B, run, False, max_ctx=ctx, guided=guided)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / run

        dfa = compile_regex(prompts.SQL_STATEMENT_REGEX)
        inside = dfa.walk(dfa.start, b"SELECT ")  # the state inside the statement: nearly every token stays alive

        def rebase() -> None:
            """The plain graph commits tokens the DFA never saw: restart every row's lazy advance inside the statement,
            at its current gen_len (what a re-admission writes)."""
            r.g_base[:B].copy_(r.gen_len[:B])
            r.g_state[:B].fill_(inside)

        rebase(), timed(True), timed(False)
        gd, pl = [], []
        for _ in range(reps):  # guided, plain, plain, guided: the context grows by 16 per run, the order cancels it
            for guided in (True, False, False, True):
                if guided:
                    rebase()
                (gd if guided else pl).append(timed(guided))
        live = B - int(r.finished[:B].sum())
        gm, pm = statistics.mean(gd), statistics.mean(pl)
        emit(dict(bench="step", model=spec.name, layers=spec.n_layers, B=B, prompt=plen, vocab=spec.vocab_size,
                  rows_live_after_guided_runs=live, plain_step_ms=round(pm, 4), guided_step_ms=round(gm, 4),
                  mask_cost_us=round((gm - pm) * 1e3, 1), ratio=round(gm / pm, 4)))
        eng.abort_all("bench over")
        del eng, r, w
        torch.cuda.empty_cache()


def legal_drafts(dfa, state: int, off, blob, k: int) -> list:
    """k token ids (of >= 4 bytes where one exists) that the pattern allows one after the other from ``state``."""
    offs, data = off.tolist(), bytes(blob.tolist())
    out = []
    for i in range(k):
        best = None
        for t in range(259 + 97 * i, len(offs) - 1):  # past the specials and the single bytes, another word per draft
            w = data[offs[t]:offs[t + 1]]
            if 4 <= len(w) <= 32 and dfa.walk(state, w) != DEAD:
                best = t
                break
        if best is None:  # a pattern that takes no word: the single byte it does take
            best = next(t for t in range(3, 259) if dfa.walk(state, data[offs[t]:offs[t + 1]]) != DEAD)
        out.append(best)
        state = dfa.walk(state, data[offs[best]:offs[best + 1]])
    return out


def bench_spec_kernel(dev, reps: int) -> None:
    sql = compile_regex(prompts.SQL_STATEMENT_REGEX)
    lim = compile_regex(LIMIT_PATTERN)
    pats = (("sql", sql, sql.walk(sql.start, b"SELECT ")), ("limit", lim, lim.walk(lim.start, b"abc")))
    for V, Ts in ((32000, (2, 4, 8)), (128256, (2, 4, 5))):
        off_h, blob_h = synthetic_vocab(V)
        off, blob = off_h.to(dev), blob_h.to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        eos = torch.tensor([2], **i32)
        for name, dfa, state in pats:
            for T in Ts:
                drafts = legal_drafts(dfa, state, off_h, blob_h, T - 1)
                states = [state]
                for t in drafts:
                    states.append(dfa.walk(states[-1], bytes(blob_h[off_h[t]:off_h[t + 1]].tolist())))
                assert DEAD not in states
                cls, trans, accept, dim, on, gst, base = tables(dfa, T, dev, state)
                gst.copy_(torch.tensor([[s, s] for s in states], **i32))  # row t of the baseline sits in state s_t
                z = torch.zeros(T, **i32)
                logits = torch.randn(T, V, device=dev)
                wv, wm = logits.clone(), logits.clone()
                dr, g_spec = torch.tensor(drafts, **i32), torch.zeros(9, **i32)
                gst0 = torch.full((T, 2), state, **i32)
                arms = {
                    "dfa_mask_verify": lambda: ops.dfa_mask_verify(wv, off, blob, cls, trans, accept, dim, on, gst0, base,
                                                                   z, z, z, eos, dr, g_spec),
                    "dfa_mask_B_T": lambda: ops.dfa_mask(wm, off, blob, cls, trans, accept, dim, on, gst, base, z, z, z,
                                                         eos),
                }
                us = {k: [] for k in arms}
                for _ in range(reps):  # alternate the arms
                    for k, fn in arms.items():
                        us[k].append(time_graph(fn))
                assert torch.equal(wv, wm) and g_spec[1:1 + T].tolist() == states  # the same mask, by both kernels
                med = {k: round(statistics.median(v), 2) for k, v in us.items()}
                emit(dict(bench="spec_kernel", V=V, T=T, pattern=name, states=dfa.n_states, classes=dfa.n_classes,
                          draft_bytes=[int(off_h[t + 1] - off_h[t]) for t in drafts],
                          tokens_alive_per_row=int(torch.isfinite(wv).sum()) // T, us=med,
                          draft_walk_us=round(med["dfa_mask_verify"] - med["dfa_mask_B_T"], 2),
                          ratio=round(med["dfa_mask_verify"] / med["dfa_mask_B_T"], 3)))


def bench_spec_step(dev, layers: int, reps: int) -> None:
    dfa = compile_regex(prompts.SQL_STATEMENT_REGEX)
    inside = dfa.walk(dfa.start, b"SELECT ")
    for base, plen, ks in (("duckdb-nsql", 128, (1, 3, 7)), ("llama3.2", 2048, (1, 3, 4))):
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5, kind="bf16")
        new, run = 1024, 16
        r = ModelRunner(w, max_slots=2, max_model_len=plen + new + 64, num_kv_blocks=(plen + new) // 64 + 4,
                        spec_tokens=max(ks), spec_guided=True)
        off_h, blob_h = synthetic_vocab(spec.vocab_size)
        r.enable_guided(off_h, blob_h)
        eng = LLMEngine(r, name=spec.name, kv_reserve_tokens=-1, guided=True)
        g = torch.Generator().manual_seed(7)
        ids = [1] + torch.randint(3, spec.vocab_size, (plen - 1,), generator=g).tolist()
        ctx = plen + new
        for k in ks:
            r.spec_tokens = k
            assert r.spec_k() == k, (k, r.spec_k())
            r.set_spec_forced(torch.tensor([legal_drafts(dfa, inside, off_h, blob_h, k)], dtype=torch.int32))
            eng.add_request(ids, SamplingParams(max_tokens=new, regex=prompts.SQL_STATEMENT_REGEX))
            eng.step()  # prefill + one run of guided verify steps
            assert eng.stats["spec_steps"] > 0

            def rebase() -> None:
                """The unguided arms commit tokens the DFA never saw: restart the lazy advance inside the statement."""
                r.g_base[:1].copy_(r.gen_len[:1])
                r.g_state[:1].fill_(inside)

            def timed(arm: str) -> float:
                if arm in ("guided_verify", "guided"):
                    rebase()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if arm.endswith("verify"):
                    r.decode_spec(run, max_ctx=ctx, guided=arm == "guided_verify")
                else:
                    r.decode(1, run, False, max_ctx=ctx, guided=arm == "guided")
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / run

            order = ("guided_verify", "verify", "guided", "plain")
            for arm in order:
                timed(arm)  # warms the four graphs
            ms = {arm: [] for arm in order}
            n0 = int(r.gen_len[0])
            for _ in range(reps):  # mirrored: the context grows with every run, the order cancels it
                for arm in order + order[::-1]:
                    ms[arm].append(timed(arm))
            steps = reps * 8 * run
            m = {arm: statistics.mean(v) for arm, v in ms.items()}
            emit(dict(bench="spec_step", model=spec.name, layers=spec.n_layers, prompt=plen, vocab=spec.vocab_size, k=k,
                      T=k + 1, row_live_after=1 - int(r.finished[0]), steps=steps, tokens=int(r.gen_len[0]) - n0,
                      plain_step_ms=round(m["plain"], 4), guided_step_ms=round(m["guided"], 4),
                      verify_step_ms=round(m["verify"], 4), guided_verify_step_ms=round(m["guided_verify"], 4),
                      mask_verify_cost_us=round((m["guided_verify"] - m["verify"]) * 1e3, 1),
                      mask_plain_cost_us=round((m["guided"] - m["plain"]) * 1e3, 1),
                      break_even_unconstrained=round(m["verify"] / m["plain"] - 1, 3),
                      break_even_constrained=round(m["guided_verify"] / m["guided"] - 1, 3)))
            eng.abort_all("bench over")
        del eng, r, w
        torch.cuda.empty_cache()


def bench_spec_batch_kernel(dev, reps: int) -> None:
    sql = compile_regex(prompts.SQL_STATEMENT_REGEX)
    lim = compile_regex(LIMIT_PATTERN)
    pats = (("sql", sql, sql.walk(sql.start, b"SELECT ")), ("limit", lim, lim.walk(lim.start, b"abc")))
    for V, shapes in ((32000, ((2, 4), (4, 4), (4, 8))), (128256, ((4, 5),))):
        off_h, blob_h = synthetic_vocab(V)
        off, blob = off_h.to(dev), blob_h.to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        eos = torch.tensor([2], **i32)
        for name, dfa, state in pats:
            for S, T in shapes:
                drafts = legal_drafts(dfa, state, off_h, blob_h, T - 1)
                states = [state]
                for t in drafts:
                    states.append(dfa.walk(states[-1], bytes(blob_h[off_h[t]:off_h[t + 1]].tolist())))
                assert DEAD not in states
                B = S * T
                cls, trans, accept, dim, on, gst, base = tables(dfa, B, dev, state)
                gst.copy_(torch.tensor([[s, s] for s in states] * S, **i32))  # baseline row s T + t sits in state s_t
                z = torch.zeros(B, **i32)
                logits = torch.randn(B, V, device=dev)
                dr = torch.tensor(drafts * S, **i32)
                gst0 = torch.full((B, 2), state, **i32)
                for half in (False, True):  # half: the odd sequences carry no constraint, in both arms
                    wv, wm = logits.clone(), logits.clone()
                    g_spec = torch.zeros(S, 9, **i32)
                    on_v, on_m = on.clone(), on.clone()
                    if half:
                        on_v[1:S:2] = 0
                        on_m.view(S, T)[1::2] = 0
                    arms = {
                        "dfa_mask_verify_S": lambda: ops.dfa_mask_verify(wv, off, blob, cls, trans, accept, dim, on_v,
                                                                         gst0, base, z, z, z, eos, dr, g_spec),
                        "dfa_mask_B_ST": lambda: ops.dfa_mask(wm, off, blob, cls, trans, accept, dim, on_m, gst, base, z,
                                                              z, z, eos),
                    }
                    us = {k: [] for k in arms}
                    for _ in range(reps):  # alternate the arms
                        for k, fn in arms.items():
                            us[k].append(time_graph(fn))
                    live = [s for s in range(S) if not (half and s & 1)]
                    assert torch.equal(wv, wm) and all(g_spec[s, 1:1 + T].tolist() == states for s in live)
                    assert all(torch.equal(wv[s * T:(s + 1) * T], logits[s * T:(s + 1) * T]) for s in range(S) if s not in live)
                    med = {k: round(statistics.median(v), 2) for k, v in us.items()}
                    emit(dict(bench="spec_batch_kernel", V=V, S=S, T=T, rows=B, pattern=name, states=dfa.n_states,
                              classes=dfa.n_classes, constrained_sequences=len(live),
                              draft_bytes=[int(off_h[t + 1] - off_h[t]) for t in drafts],
                              tokens_alive_per_masked_row=int(torch.isfinite(wv[:T]).sum()) // T, us=med,
                              draft_walk_us=round(med["dfa_mask_verify_S"] - med["dfa_mask_B_ST"], 2),
                              ratio=round(med["dfa_mask_verify_S"] / med["dfa_mask_B_ST"], 3)))


def bench_spec_batch_step(dev, layers: int, reps: int, Ss=(2, 4), k: int = 3, models=None) -> None:
    dfa = compile_regex(prompts.SQL_STATEMENT_REGEX)
    inside = dfa.walk(dfa.start, b"SELECT ")
    for base, plen in (("duckdb-nsql", 128), ("llama3.2", 2048)):
        if models and base not in models:
            continue
        spec = get_spec(base)
        if layers:
            spec = dataclasses.replace(spec, n_layers=layers, name=f"{base}-{layers}l")
        w = init_random(spec, dev, seed=5, kind="bf16")
        new, run, SM = 1024, 16, max(Ss)
        r = ModelRunner(w, max_slots=SM, max_model_len=plen + new + 64, num_kv_blocks=SM * ((plen + new) // 64 + 3) + 1,
                        spec_tokens=k, spec_guided=True, spec_batch=SM, spec_batch_guided=True)
        off_h, blob_h = synthetic_vocab(spec.vocab_size)
        r.enable_guided(off_h, blob_h)
        eng = LLMEngine(r, name=spec.name, kv_reserve_tokens=-1, guided=True, max_prefill_tokens=SM * plen + 64)
        assert r.spec_k() == k and r.spec_s() == SM, (r.spec_k(), r.spec_s())
        g = torch.Generator().manual_seed(7)
        ids = [[1] + torch.randint(3, spec.vocab_size, (plen - 1,), generator=g).tolist() for _ in range(SM)]
        ctx = plen + new
        r.set_spec_forced(torch.tensor([legal_drafts(dfa, inside, off_h, blob_h, k)], dtype=torch.int32))
        for S in Ss:
            for p in ids[:S]:
                eng.add_request(p, SamplingParams(max_tokens=new, regex=prompts.SQL_STATEMENT_REGEX))
            s0 = eng.stats["spec_steps"]
            eng.step()  # prefill + one run of guided verify steps over the S sequences
            assert eng.stats["spec_steps"] > s0

            def rebase() -> None:
                """The unguided arms commit tokens the DFA never saw: restart the lazy advance inside the statement."""
                r.g_base[:S].copy_(r.gen_len[:S])
                r.g_state[:S].fill_(inside)

            def timed(arm: str) -> float:
                if arm in ("guided_verify", "guided"):
                    rebase()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if arm.endswith("verify"):
                    r.decode_spec(run, max_ctx=ctx, guided=arm == "guided_verify", S=S)
                else:
                    r.decode(S, run, False, max_ctx=ctx, guided=arm == "guided")
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / run

            order = ("guided_verify", "verify", "guided", "plain")
            for arm in order:
                timed(arm)  # warms the four graphs
            ms = {arm: [] for arm in order}
            n0 = r.gen_len[:S].tolist()
            for _ in range(reps):  # mirrored: the context grows with every run, the order cancels it
                for arm in order + order[::-1]:
                    ms[arm].append(timed(arm))
            m = {arm: statistics.mean(v) for arm, v in ms.items()}
            emit(dict(bench="spec_batch_step", model=spec.name, layers=spec.n_layers, prompt=plen, vocab=spec.vocab_size,
                      k=k, T=k + 1, S=S, rows=S * (k + 1), rows_live_after=S - int(r.finished[:S].sum()),
                      steps=reps * 8 * run, tokens=[a - b for a, b in zip(r.gen_len[:S].tolist(), n0)],
                      plain_step_ms=round(m["plain"], 4), guided_step_ms=round(m["guided"], 4),
                      verify_step_ms=round(m["verify"], 4), guided_verify_step_ms=round(m["guided_verify"], 4),
                      mask_verify_cost_us=round((m["guided_verify"] - m["verify"]) * 1e3, 1),
                      mask_plain_cost_us=round((m["guided"] - m["plain"]) * 1e3, 1),
                      break_even_unconstrained=round(m["verify"] / m["plain"] - 1, 3),
                      break_even_constrained=round(m["guided_verify"] / m["guided"] - 1, 3)))
            eng.abort_all("bench over")
        del eng, r, w
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="truncate the models to this many layers (0 = full depth)")
    ap.add_argument("--skip", default="", help="comma list of kernel,step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spec", action="store_true", help="measure spec_guided (verify-row mask, guided verify step)")
    ap.add_argument("--spec-batch", action="store_true",
                    help="measure spec_batch_guided (the mask over S sequences, the guided batched verify step)")
    ap.add_argument("--models", default="", help="comma list of duckdb-nsql,llama3.2 (--spec-batch step; default both)")
    ap.add_argument("--out", default="", help="JSON-lines file to append to")
    a = ap.parse_args()
    global OUT
    OUT = a.out or (OUT_SPEC_BATCH if a.spec_batch else OUT_SPEC if a.spec else OUT)
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided.py needs a GPU")
    ops.ext()
    dev = torch.device("cuda:0")
    skip = set(a.skip.split(",")) if a.skip else set()
    if a.spec_batch:
        if "kernel" not in skip:
            bench_spec_batch_kernel(dev, a.reps)
        if "step" not in skip:
            bench_spec_batch_step(dev, a.layers, a.reps, models=set(a.models.split(",")) if a.models else None)
        return
    if a.spec:
        if "kernel" not in skip:
            bench_spec_kernel(dev, a.reps)
        if "step" not in skip:
            bench_spec_step(dev, a.layers, a.reps)
        return
    if "kernel" not in skip:
        bench_kernel(dev)
    if "step" not in skip:
        bench_step(dev, a.layers, a.reps)


if __name__ == "__main__":
    main()
