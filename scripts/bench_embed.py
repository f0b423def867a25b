"""Embeddings on MI355X: what the three pooling launches cost, beside the prefill call they follow.

Two cases, each with both poolings: one 2048-token input on the Llama-3.2-3B spec, and 32 inputs of 128 tokens on the
duckdb-nsql-7B spec (one packed prefill of 4096 rows).  Per case and pooling the engine embeds the inputs --reps times;
device events are recorded around the runner's prefill call and between the three launches inside it
(ops.embed_rowscale, embed_pool, embed_finish), so every record carries

  prefill_ms          the whole prefill call of the embedding requests, launches included
  prefill_plain_ms    the same inputs as ordinary max_tokens = 1 requests (no pooling)
  embed_us            the three launches together (event before the first, event after the last)
  rowscale_us / pool_us / finish_us   each launch apart

as medians over the repetitions, with the minimum and maximum of embed_us.  Writes JSON lines to
profiles/embed/embed_mi355x.jsonl.  Needs a GPU.

  python scripts/bench_embed.py [--layers N] [--reps 9]
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

OUT = os.path.join(ROOT, "profiles", "embed")
CASES = [("3b", "llama3.2", 1, 2048), ("7b", "duckdb-nsql", 32, 128)]


def emit(rec: dict) -> None:
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "embed_mi355x.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


class Probe:
    """Device events around ``runner.prefill`` and between the three embedding launches inside it."""

    def __init__(self, runner: ModelRunner):
        self.r, self.calls, self.marks = runner, [], []
        self._prefill = runner.prefill
        self._ops = (ops.embed_rowscale, ops.embed_pool, ops.embed_finish)

    def __enter__(self):
        rowscale, pool, finish = self._ops

        def prefill(*a, **kw):
            e0 = ev()
            out = self._prefill(*a, **kw)
            self.calls.append((e0, ev()))
            return out

        def w_rowscale(*a, **kw):
            self.marks.append([ev()])
            rowscale(*a, **kw)
            self.marks[-1].append(ev())

        def w_pool(*a, **kw):
            pool(*a, **kw)
            self.marks[-1].append(ev())

        def w_finish(*a, **kw):
            finish(*a, **kw)
            self.marks[-1].append(ev())

        self.r.prefill = prefill
        ops.embed_rowscale, ops.embed_pool, ops.embed_finish = w_rowscale, w_pool, w_finish
        return self

    def __exit__(self, *exc):
        del self.r.prefill
        ops.embed_rowscale, ops.embed_pool, ops.embed_finish = self._ops

    def take(self):
        torch.cuda.synchronize()
        pf = sum(a.elapsed_time(b) for a, b in self.calls)
        parts = [[m[i].elapsed_time(m[i + 1]) * 1e3 for i in range(3)] + [m[0].elapsed_time(m[3]) * 1e3] for m in self.marks]
        self.calls, self.marks = [], []
        return pf, [sum(p[i] for p in parts) for i in range(4)] if parts else None


def run_case(eng: LLMEngine, tag: str, n: int, tokens: int, reps: int) -> None:
    g = torch.Generator().manual_seed(tokens)
    vocab = eng.spec.vocab_size
    inputs = [[1] + torch.randint(3, min(vocab, 30000), (tokens - 1,), generator=g).tolist() for _ in range(n)]
    med = statistics.median
    with Probe(eng.runner) as probe:
        plain = []
        for i in range(reps + 1):
            reqs = eng.add_requests(inputs, SamplingParams(max_tokens=1, ignore_eos=True))
            eng.run_until_done(reqs)
            pf, _ = probe.take()
            if i:  # the first run warms the shapes up
                plain.append(pf)
        for pooling in ("last", "mean"):
            pfs, parts = [], []
            for i in range(reps + 1):
                reqs = eng.add_requests(inputs, SamplingParams(embed=pooling))
                eng.run_until_done(reqs)
                pf, p = probe.take()
                assert all(q.embedding is not None for q in reqs)
                if i:
                    pfs.append(pf)
                    parts.append(p)
            tog = [p[3] for p in parts]
            emit({"bench": "embed", "model": tag, "layers": eng.runner.L, "hidden": eng.runner.d, "inputs": n,
                  "tokens_per_input": tokens, "pooling": pooling, "prefill_ms": round(med(pfs), 3),
                  "prefill_plain_ms": round(med(plain), 3), "embed_us": round(med(tog), 1),
                  "embed_us_min": round(min(tog), 1), "embed_us_max": round(max(tog), 1),
                  "rowscale_us": round(med([p[0] for p in parts]), 1), "pool_us": round(med([p[1] for p in parts]), 1),
                  "finish_us": round(med([p[2] for p in parts]), 1),
                  "embed_share_of_prefill": round(med(tog) / 1e3 / med(pfs), 5)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's (0 = all)")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed.py needs a GPU: nothing here can be measured without one")
    dev = torch.device("cuda")
    for tag, name, n, tokens in CASES:
        spec = get_spec(name)
        if a.layers:
            spec = dataclasses.replace(spec, n_layers=a.layers, name=f"{name}-{a.layers}l")
        r = ModelRunner(init_random(spec, dev, seed=0), max_slots=max(2, n), max_model_len=4096,
                        num_kv_blocks=n * (tokens // 64 + 1) + 8)
        eng = LLMEngine(r, name=spec.name, embeddings=True)
        run_case(eng, tag, n, tokens, a.reps)
        del eng, r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
