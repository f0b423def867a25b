"""NL->SQL accuracy / latency comparison across models.

Reproduces Model_Evaluation_&_Comparision.py: the single-query evaluation (taxi schema, one question,
an 8-line expected SQL; C21) and the 4-query evaluation (C22) over ``mistral``, ``llama3.2`` and
``duckdb-nsql``, with the same metrics — exact match after ``strip()``, Levenshtein distance
(native C++ ``_lsa_runtime.levenshtein`` in place of the python-Levenshtein extension) and end-to-end
client wall-clock latency around each ``generate`` call — and the same printed summary.  Additions:
p50 latency, output tokens and tokens/s per model (from the engine's ``eval_count`` /
``eval_duration``, which the reference discarded), a JSON report, and the Markdown model-comparison report of
``eval.report`` (the reference's hand-written ``Model_Comparision_Report.docx``).  ``--score`` (an engine with
per-token logprobs) adds the likelihood metric: the log-likelihood the model gives the *expected* SQL after the very
prompt it was sent (``client.score``: teacher-forced through the prefill), per query ``expected_logprob`` (sum over the
expected statement's tokens), ``expected_mean_logprob`` and ``expected_tokens`` -- the one metric that does not tie when
every answer is wrong in its own way.  Without the flag the printed summary and the JSON are what they are without it.

    python -m llm_based_apache_spark_optimization_amd.eval.harness --engine hip --max-tokens 128
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from typing import Callable, Optional, Sequence

from .. import prompts
from ..runtime.native import levenshtein

GenerateFn = Callable[..., object]
ScoreFn = Callable[..., dict]


def _expected(score: Optional[ScoreFn], model: str, system: str, prompt: str, expected_sql: str,
              options: Optional[dict]) -> dict:
    """The three likelihood fields of one query ({} without ``score``)."""
    if score is None:
        return {}
    keep = {k: v for k, v in (options or {}).items() if k in ("num_ctx",)}
    sc = score(model=model, system=system, prompt=prompt, completions=[expected_sql], options=keep)["scores"][0]
    return {"expected_logprob": sc["logprob"], "expected_mean_logprob": sc["mean_logprob"],
            "expected_tokens": sc["tokens"]}


def _gen(generate: GenerateFn, model: str, system: str, prompt: str, options: Optional[dict]):
    t0 = time.time()
    res = generate(model=model, system=system, prompt=prompt, options=options)
    return res, time.time() - t0


def evaluate_single(generate: GenerateFn, model_name: str, options: Optional[dict] = None, verbose: bool = True,
                    score: Optional[ScoreFn] = None):
    res, latency = _gen(generate, model_name, prompts.EVAL_SINGLE_SYSTEM, prompts.EVAL_SINGLE_PROMPT, options)
    generated_sql = res.response.strip()
    exact_match = 1 if generated_sql == prompts.EVAL_EXPECTED_SQL else 0
    edit_distance = levenshtein(generated_sql, prompts.EVAL_EXPECTED_SQL)
    if verbose:
        print(f"Model: {model_name}")
        print(f"Generated SQL:\n{generated_sql}")
        print(f"Exact Match: {exact_match}")
        print(f"Edit Distance: {edit_distance}")
        print(f"Latency: {latency:.4f} sec")
        print("=" * 80)
    return {"model": model_name, "generated_sql": generated_sql, "exact_match": exact_match,
            "edit_distance": edit_distance, "latency": latency,
            "eval_count": getattr(res, "eval_count", 0), "eval_duration": getattr(res, "eval_duration", 0),
            **_expected(score, model_name, prompts.EVAL_SINGLE_SYSTEM, prompts.EVAL_SINGLE_PROMPT,
                        prompts.EVAL_EXPECTED_SQL, options)}


def evaluate_multi(generate: GenerateFn, models: Sequence[str], queries=prompts.EVAL_QUERIES,
                   options: Optional[dict] = None, verbose: bool = True, score: Optional[ScoreFn] = None) -> dict:
    results = {m: {"exact_match": 0, "total_edit_distance": 0, "total_latency": 0, "queries": []} for m in models}
    for model in models:
        if verbose:
            print(f"Evaluating model: {model}\n" + "=" * 80)
        for query in queries:
            res, latency = _gen(generate, model, prompts.EVAL_MULTI_SYSTEM, query["nl"], options)
            generated_sql = res.response.strip()
            expected_sql = query["expected_sql"].strip()
            exact_match = int(generated_sql == expected_sql)
            edit_distance = levenshtein(generated_sql, expected_sql)
            r = results[model]
            r["exact_match"] += exact_match
            r["total_edit_distance"] += edit_distance
            r["total_latency"] += latency
            r["queries"].append({"query": query["nl"], "generated_sql": generated_sql, "expected_sql": expected_sql,
                                 "exact_match": exact_match, "edit_distance": edit_distance, "latency": latency,
                                 "eval_count": getattr(res, "eval_count", 0),
                                 "eval_duration": getattr(res, "eval_duration", 0),
                                 **_expected(score, model, prompts.EVAL_MULTI_SYSTEM, query["nl"], expected_sql,
                                             options)})
            if verbose:
                print(f"Query: {query['nl']}")
                print(f"Generated SQL: {generated_sql}")
                print(f"Expected SQL: {expected_sql}")
                print(f"Exact Match: {exact_match}, Edit Distance: {edit_distance}, Latency: {latency:.4f} sec")
                print("-" * 80)
    return results


def summarize(results: dict, n_queries: int, verbose: bool = True) -> dict:
    out = {}
    if verbose:
        print("\n\nFinal Evaluation Summary:\n" + "=" * 100)
    for model, data in results.items():
        lats = [q["latency"] for q in data["queries"]]
        toks = sum(q["eval_count"] for q in data["queries"])
        dur = sum(q["eval_duration"] for q in data["queries"]) / 1e9
        s = {"exact_match_rate": data["exact_match"] / n_queries * 100,
             "avg_edit_distance": data["total_edit_distance"] / n_queries,
             "avg_latency": data["total_latency"] / n_queries,
             "p50_latency": statistics.median(lats) if lats else 0.0,
             "output_tokens": toks, "decode_tokens_per_s": (toks / dur) if dur else 0.0}
        scored = [q for q in data["queries"] if "expected_logprob" in q]
        if scored:  # --score: the likelihood of the expected statements (sum per query averaged; per-token mean)
            n_tok = sum(q["expected_tokens"] for q in scored)
            total = sum(q["expected_logprob"] for q in scored)
            s.update(expected_logprob=total / len(scored), expected_mean_logprob=total / max(1, n_tok),
                     expected_tokens=n_tok)
        out[model] = s
        if verbose:
            print(f"Model: {model}")
            print(f"Exact Match Rate: {s['exact_match_rate']:.2f}%")
            print(f"Average Edit Distance: {s['avg_edit_distance']:.2f}")
            print(f"Average Latency: {s['avg_latency']:.4f} sec")
            print(f"p50 Latency: {s['p50_latency']:.4f} sec   output tokens: {toks}   "
                  f"decode tok/s: {s['decode_tokens_per_s']:.1f}")
            if scored:
                print(f"Expected SQL log-likelihood: {s['expected_logprob']:.3f} per query   "
                      f"{s['expected_mean_logprob']:.4f} per token   tokens: {s['expected_tokens']}")
            print("=" * 100)
    return out


def main(argv=None) -> int:
    from .. import client
    from ..config import Settings

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--engine", default="hip", choices=["hip", "fake", "remote"])
    ap.add_argument("--remote-url", default="http://127.0.0.1:8000")
    ap.add_argument("--models", default=",".join(prompts.EVAL_MODELS))
    ap.add_argument("--max-tokens", type=int, default=128, help="num_predict per request")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--json", default="", help="write the report here")
    ap.add_argument("--report", default="", help="write the Markdown model-comparison report here (eval.report)")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--score", action="store_true",
                    help="add the log-likelihood of the expected SQL (needs an engine with per-token logprobs)")
    a = ap.parse_args(argv)
    s = Settings(engine=a.engine, remote_url=a.remote_url, **({"logprobs": True} if a.score else {}))
    from ..serving.service import backend_from_settings

    client.set_backend(backend_from_settings(s))
    opts = {"num_predict": a.max_tokens, "temperature": a.temperature}
    models = [m for m in a.models.split(",") if m]
    sc = dict(score=client.score) if a.score else {}
    single = [evaluate_single(client.generate, m, opts, verbose=not a.quiet, **sc) for m in models]
    multi = evaluate_multi(client.generate, models, options=opts, verbose=not a.quiet, **sc)
    summary = summarize(multi, len(prompts.EVAL_QUERIES), verbose=not a.quiet)
    report = {"single": single, "multi": multi, "summary": summary, "options": opts}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    if a.report:
        from .report import render

        with open(a.report, "w") as f:
            f.write(render(report, random_weights=a.engine != "remote"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
