"""FastAPI JSON service.

Reference-compatible route (FastAPI/app.py:62-144): ``POST /process-data/`` with body
``{"input_text": str, "file_name": str}``; the CSV is resolved under the configured input directory;
responses keep the reference's keys and its HTTP-200-with-"error" convention:

* success  ``{"message": "Query executed successfully!", "input_file_name", "input_data", "sql_query",
  "output_file"}``
* SQL error ``{"error": "SQL execution failed", "sql_query", "error_details"}`` (LLM#2's explanation)
* missing  ``{"error": "CSV file not found at <path>"}``

North-star endpoints (BASELINE.json): ``POST /nl2sql`` and ``POST /explain_error``.  Plus an
Ollama-compatible ``POST /api/generate`` / ``GET /api/tags`` (so ``ollama``-style clients, including
the reference's own harness pointed at this host, work unchanged), ``/health``, ``/ready``,
``/metrics`` (Prometheus) and ``/status/{request_id}``.

Handlers are plain ``def`` (run in FastAPI's threadpool): the reference's ``async def`` handlers
made blocking calls and serialised every request on the event loop (SURVEY.md §2.6 P-DP); here
concurrent requests reach the engine together and share decode steps.
"""
from __future__ import annotations

import json
import os
import time
from typing import Optional, Union

from fastapi import FastAPI, HTTPException, Request
from fastapi.responses import JSONResponse, PlainTextResponse, StreamingResponse
from pydantic import BaseModel

from .. import prompts
from ..client import EngineUnavailable
from ..engine.engine import SamplingOptionError
from ..engine.guided import GuidedRequestError
from ..utils.metrics import REGISTRY, record_generation
from ..utils.tracing import new_request_id
from .pipeline import resolve_input, sql_logprob_summary
from .service import AppContext, make_context


class InputString(BaseModel):
    input_text: str
    file_name: str


class NL2SQLRequest(BaseModel):
    question: Optional[str] = None
    input_text: Optional[str] = None
    table_schema: Optional[str] = None
    schema_text: Optional[str] = None
    file_name: Optional[str] = None
    options: Optional[dict] = None


class ExplainRequest(BaseModel):
    error_message: str
    options: Optional[dict] = None


class GenerateRequest(BaseModel):
    model: str
    prompt: str = ""
    system: str = ""
    options: Optional[dict] = None
    stream: bool = False
    raw: bool = False
    # per-token logprobs: Ollama's top-level request fields (also accepted inside ``options``)
    logprobs: Optional[bool] = None
    top_logprobs: Optional[int] = None
    # prompt-token logprobs (OpenAI's echo + logprobs), next to them; prompt_logprobs_from travels in ``options``
    prompt_logprobs: Optional[bool] = None

    def merged_options(self) -> Optional[dict]:
        if self.logprobs is None and self.top_logprobs is None and self.prompt_logprobs is None:
            return self.options
        top = {k: v for k, v in (("logprobs", self.logprobs), ("top_logprobs", self.top_logprobs),
                                 ("prompt_logprobs", self.prompt_logprobs)) if v is not None}
        return dict(self.options or {}, **top)


class ScoreRequest(BaseModel):
    """Teacher-forced scoring: the log-likelihood of ``completion`` / each of ``completions`` after the prompt."""
    model: str
    prompt: str = ""
    system: str = ""
    raw: bool = False
    completion: Optional[str] = None
    completions: Optional[list[str]] = None
    top_logprobs: int = 0
    options: Optional[dict] = None


class EmbedRequest(BaseModel):
    """Ollama's ``/api/embed``: ``input`` is one text or a list of them; ``options`` may carry ``num_ctx`` and the
    extension ``pooling`` ("last", the default, or "mean")."""
    model: str
    input: Union[str, list[str]] = ""
    truncate: bool = True
    options: Optional[dict] = None


def create_app(ctx: Optional[AppContext] = None) -> FastAPI:
    ctx = ctx or make_context()
    app = FastAPI(title="MI355X NL->SQL / Spark-error service")
    app.state.ctx = ctx
    s = ctx.settings

    @app.exception_handler(EngineUnavailable)
    def engine_down(request: Request, exc: EngineUnavailable):
        # a dead engine answers at once (SURVEY.md §5 failure detection) instead of after the request timeout
        REGISTRY.inc("lsa_requests_total", 1, "requests", route=request.url.path.strip("/"), outcome="unavailable")
        return JSONResponse(status_code=503, content={"error": "engine unavailable", "detail": str(exc)})

    @app.exception_handler(GuidedRequestError)
    def bad_regex(request: Request, exc: GuidedRequestError):
        # a pattern the engine cannot serve (unsupported syntax, too large, guided decoding off) is the caller's error
        REGISTRY.inc("lsa_requests_total", 1, "requests", route=request.url.path.strip("/"), outcome="bad_regex")
        return JSONResponse(status_code=400, content={"error": "invalid regex constraint", "detail": str(exc)})

    @app.exception_handler(SamplingOptionError)
    def bad_option(request: Request, exc: SamplingOptionError):
        # a sampler option the engine refuses (a NaN penalty, min_p outside [0, 1]) is the caller's error too
        REGISTRY.inc("lsa_requests_total", 1, "requests", route=request.url.path.strip("/"), outcome="bad_option")
        return JSONResponse(status_code=400, content={"error": "invalid sampling option", "detail": str(exc)})

    @app.post("/process-data/")
    def modify_string(data: InputString):
        t0 = time.perf_counter()
        file_path = resolve_input(s.input_dir, data.file_name)
        if file_path is None:
            REGISTRY.inc("lsa_requests_total", 1, "requests", route="process-data", outcome="bad_name")
            return {"error": "Invalid file name: " + data.file_name}
        if not os.path.exists(file_path):
            REGISTRY.inc("lsa_requests_total", 1, "requests", route="process-data", outcome="not_found")
            return {"error": "CSV file not found at " + file_path}
        res = ctx.pipeline.run(file_path, data.file_name, data.input_text,
                               output_name=lambda ts: f"{ts}_{os.path.basename(file_path)}.csv")
        REGISTRY.observe("lsa_request_seconds", time.perf_counter() - t0, "e2e latency", route="process-data")
        if not res.ok:
            REGISTRY.inc("lsa_requests_total", 1, "requests", route="process-data", outcome="sql_error")
            return {"error": "SQL execution failed", "sql_query": res.sql_query, "error_details": res.explanation}
        REGISTRY.inc("lsa_requests_total", 1, "requests", route="process-data", outcome="ok")
        body = {
            "message": "Query executed successfully!",
            "input_file_name": data.file_name,
            "input_data": data.input_text,
            "sql_query": res.sql_query,
            "output_file": res.output_file,
        }
        if res.sql_mean_logprob is not None:  # Settings.sql_logprobs only
            body.update(sql_mean_logprob=res.sql_mean_logprob, sql_min_logprob=res.sql_min_logprob)
        return body

    @app.post("/nl2sql")
    def nl2sql(req: NL2SQLRequest):
        t0 = time.perf_counter()
        question = req.question or req.input_text
        if not question:
            raise HTTPException(422, "question (or input_text) is required")
        schema = req.table_schema or req.schema_text
        if schema is None and req.file_name:
            path = resolve_input(s.input_dir, req.file_name)
            if path is None:
                raise HTTPException(400, "invalid file_name: " + req.file_name)
            if not os.path.exists(path):
                return {"error": "CSV file not found at " + path}
            table = ctx.pipeline.executor.table_of(ctx.pipeline.executor.load_csv(path))
            schema = prompts.table_schema_text(table.dtypes)
        if schema is None:
            raise HTTPException(422, "table_schema or file_name is required")
        rid = new_request_id()
        r = ctx.pipeline.nl2sql(schema, question, req.options, rid)
        dt = time.perf_counter() - t0
        REGISTRY.observe("lsa_request_seconds", dt, "e2e latency", route="nl2sql")
        REGISTRY.inc("lsa_requests_total", 1, "requests", route="nl2sql", outcome="ok")
        body = {"sql_query": r.response, "model": r.model, "request_id": rid, "table_schema": schema,
                "eval_count": r.eval_count, "eval_duration": r.eval_duration,
                "prompt_eval_count": r.prompt_eval_count, "total_duration": r.total_duration, "latency_s": dt}
        if getattr(s, "sql_logprobs", False):  # (unset: the body is key for key what it was)
            body.update(sql_logprob_summary(r) or {})
        return body

    @app.post("/explain_error")
    def explain_error(req: ExplainRequest):
        t0 = time.perf_counter()
        rid = new_request_id()
        r = ctx.pipeline.explain(req.error_message, req.options, rid)
        dt = time.perf_counter() - t0
        REGISTRY.observe("lsa_request_seconds", dt, "e2e latency", route="explain_error")
        REGISTRY.inc("lsa_requests_total", 1, "requests", route="explain_error", outcome="ok")
        return {"explanation": r.response, "model": r.model, "request_id": rid, "eval_count": r.eval_count,
                "eval_duration": r.eval_duration, "prompt_eval_count": r.prompt_eval_count,
                "total_duration": r.total_duration, "latency_s": dt}

    @app.post("/api/generate")
    def api_generate(req: GenerateRequest):
        if req.stream:  # Ollama's NDJSON framing: response pieces as decoded, then the done chunk
            chunks = ctx.backend.generate_stream(req.model, req.prompt, req.system, req.merged_options(), req.raw)

            def ndjson():
                for c in chunks:
                    if c.done:
                        record_generation(c, "api_generate")
                    yield json.dumps(c.to_dict()) + "\n"
            return StreamingResponse(ndjson(), media_type="application/x-ndjson")
        r = ctx.backend.generate(req.model, req.prompt, req.system, req.merged_options(), req.raw)
        record_generation(r, "api_generate")
        return r.to_dict()

    @app.post("/api/score")
    def api_score(req: ScoreRequest):
        # what the engine refuses (no logprobs, TP > 1, an empty completion, more than 64 of them, a sequence that does
        # not fit the context window: scoring never truncates) is a SamplingOptionError: 400 through the handler above
        t0 = time.perf_counter()
        if (req.completion is None) == (req.completions is None):
            raise HTTPException(400, "exactly one of completion and completions is required")
        comps = [req.completion] if req.completions is None else list(req.completions)
        if not comps:
            raise HTTPException(400, "completions is empty")
        try:
            out = ctx.backend.score(req.model, req.prompt, comps, req.system, req.options, req.raw, req.top_logprobs)
        except NotImplementedError:
            raise HTTPException(501, "this backend does not score completions") from None
        REGISTRY.observe("lsa_request_seconds", time.perf_counter() - t0, "e2e latency", route="api_score")
        REGISTRY.inc("lsa_requests_total", 1, "requests", route="api_score", outcome="ok")
        return out

    @app.post("/api/embed")
    def api_embed(req: EmbedRequest):
        # what the engine refuses (no embeddings, TP > 1, an unknown pooling, no input or more than 64, an empty input,
        # an over-long one with truncate false) is a SamplingOptionError: 400 through the handler above
        t0 = time.perf_counter()
        try:
            out = ctx.backend.embed(req.model, req.input, req.truncate, req.options)
        except NotImplementedError:
            raise HTTPException(501, "this backend does not embed") from None
        REGISTRY.observe("lsa_request_seconds", time.perf_counter() - t0, "e2e latency", route="api_embed")
        REGISTRY.inc("lsa_requests_total", 1, "requests", route="api_embed", outcome="ok")
        return out

    @app.get("/api/tags")
    def api_tags():
        return {"models": [{"name": m, "model": m} for m in (ctx.backend.models() or
                                                              [s.nl2sql_model, s.explain_model])]}

    @app.get("/api/version")
    def api_version():
        return {"version": "lsa-mi355x-0.1"}

    @app.get("/status/{request_id}")
    def status(request_id: str):
        return ctx.status.get(request_id)

    @app.get("/health")
    def health():
        return ctx.backend.health()

    @app.get("/ready")
    def ready():
        h = ctx.backend.health()
        if not h.get("ok", False):
            raise HTTPException(503, "engine not healthy")
        return {"ready": True}

    @app.get("/metrics", response_class=PlainTextResponse)
    def metrics():
        export_backend_gauges(ctx.backend)
        return REGISTRY.render()

    return app


def export_backend_gauges(backend) -> None:
    """Engine gauges (running / waiting / KV usage / restarts per model) and, under DP, per-replica load
    (alive, in-flight, served) plus each replica's engine gauges (``ReplicaRouter.health(deep=True)``)."""
    try:
        h = backend.health(deep=True)
    except Exception:  # noqa: BLE001 - metrics must render even when the backend is down
        h = {}

    def engines(eng: dict, **lbl):
        for m, e in (eng or {}).items():
            REGISTRY.set("lsa_engine_running", e.get("running", 0), "running requests", model=m, **lbl)
            REGISTRY.set("lsa_engine_waiting", e.get("waiting", 0), "queued requests", model=m, **lbl)
            REGISTRY.set("lsa_engine_kv_usage", e.get("kv_usage", 0.0), "KV cache fraction in use", model=m, **lbl)
            REGISTRY.set("lsa_engine_prefix_cached_blocks", e.get("prefix_cached_blocks", 0),
                         "KV blocks held by the prefix cache's index", model=m, **lbl)
            REGISTRY.set("lsa_engine_alive", 1.0 if e.get("alive", True) else 0.0, "engine loop alive", model=m, **lbl)
            REGISTRY.set("lsa_engine_restarts", e.get("restarts", 0) + e.get("rebuilds", 0),
                         "engine recoveries (loop restarts + rebuilds)", model=m, **lbl)
    engines(h.get("engines"))
    for r in h.get("replicas") or []:
        rid = str(r.get("id"))
        REGISTRY.set("lsa_replica_alive", 1.0 if r.get("alive") else 0.0, "DP replica alive", replica=rid)
        REGISTRY.set("lsa_replica_inflight", r.get("inflight", 0), "requests in flight on the replica", replica=rid)
        REGISTRY.set("lsa_replica_served", r.get("served", 0), "requests served by the replica", replica=rid)
        engines((r.get("health") or {}).get("engines"), replica=rid)


def main(argv=None) -> None:  # pragma: no cover - server entry point
    import argparse

    import uvicorn

    from ..config import Settings
    from ..utils import setup_logging

    ap = argparse.ArgumentParser(description="FastAPI NL->SQL service on MI355X")
    Settings.add_cli(ap)
    settings = Settings.from_cli(ap.parse_args(argv))
    setup_logging(settings.log_level)
    uvicorn.run(create_app(make_context(settings)), host=settings.host, port=settings.fastapi_port)


if __name__ == "__main__":  # pragma: no cover
    main()
