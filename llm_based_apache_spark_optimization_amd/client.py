"""Ollama-compatible client API.

The reference's only model interface is ``ollama.generate(model=..., system=..., prompt=...)`` and it
reads ``.response`` (FastAPI/app.py:85-90,105-111; Flask/app.py:102-107,160-165;
Model_Evaluation_&_Comparision.py:23,114).  This module keeps that call shape::

    from llm_based_apache_spark_optimization_amd import client
    res = client.generate(model="duckdb-nsql", system=..., prompt=...)
    sql = res.response            # or res["response"]

and returns the timing fields Ollama reports (``eval_count``, ``eval_duration``, ``prompt_eval_*``,
``load_duration``, ``total_duration``).  Backends (``set_backend``):

* ``EngineService`` — in-process MI355X engines (one ``LLMEngine`` per model, continuous batching on a
  background thread so concurrent callers share decode steps);
* ``FakeBackend`` — deterministic canned outputs for tests (with fault injection);
* ``RemoteBackend`` — HTTP ``POST /api/generate`` on an Ollama-compatible server (this package's
  FastAPI app, or a real Ollama daemon);
* ``parallel.router.ReplicaRouter`` — data-parallel dispatch across engine replica processes.
"""
from __future__ import annotations

import dataclasses
import datetime as _dt
import json
import queue
import threading
import time
from typing import Callable, Dict, Iterator, Optional

import torch

from .engine.engine import SamplingOptionError, SamplingParams


@dataclasses.dataclass
class GenerateResponse:
    model: str
    response: str
    done: bool = True
    done_reason: str = "stop"
    created_at: str = ""
    total_duration: int = 0
    load_duration: int = 0
    prompt_eval_count: int = 0
    prompt_eval_duration: int = 0
    eval_count: int = 0
    eval_duration: int = 0
    # of prompt_eval_count (the full prompt length), the tokens served from the engine's prefix cache
    prompt_cached_count: int = 0
    # per-token logprobs, when the request asked ("logprobs": true): one {"token", "logprob", "bytes", "top_logprobs":
    # [{"token", "logprob", "bytes"}]} per generated token (a streamed chunk: those of the tokens read at its sync)
    logprobs: Optional[list] = None
    # prompt-token logprobs, when the request asked ("prompt_logprobs": true): one entry per prompt token
    # (prompt_eval_count of them), null below max(1, prompt_logprobs_from), else the shape of a ``logprobs`` entry; a
    # streamed request carries the whole list in its final chunk.  An init-only argument kept as a plain attribute and
    # not a dataclass field, because tests/test_logprobs_cpu.py::test_response_key_only_when_asked pins the keys of a
    # response that did not ask to ``dataclasses.fields`` less ``logprobs``; ``to_dict`` adds the key when it is set, and
    # ``dataclasses.replace`` carries the attribute over (it reads an InitVar that has a default from the object)
    prompt_logprobs: dataclasses.InitVar[Optional[list]] = None
    # context shifts of the request, on an engine that runs context shift (None, and no key, on any other); an
    # init-only argument for the same reason
    context_shifts: dataclasses.InitVar[Optional[int]] = None

    def __post_init__(self, prompt_logprobs=None, context_shifts=None):
        self.prompt_logprobs = prompt_logprobs
        self.context_shifts = context_shifts

    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, default=None):
        return getattr(self, k, default)

    def to_dict(self) -> dict:
        d = dataclasses.asdict(self)
        if d["logprobs"] is None:  # nothing asked: the response is key for key what it is without the feature
            del d["logprobs"]
        if self.prompt_logprobs is not None:
            d["prompt_logprobs"] = self.prompt_logprobs
        if self.context_shifts is not None:
            d["context_shifts"] = self.context_shifts
        return d

    @property
    def tokens_per_second(self) -> float:
        return self.eval_count / (self.eval_duration / 1e9) if self.eval_duration else 0.0


def _now() -> str:
    return _dt.datetime.now(_dt.timezone.utc).isoformat()


class Backend:
    def generate(self, model: str, prompt: str, system: str = "", options: Optional[dict] = None,
                 raw: bool = False) -> GenerateResponse:
        raise NotImplementedError

    def generate_stream(self, model: str, prompt: str, system: str = "", options: Optional[dict] = None,
                        raw: bool = False) -> Iterator[GenerateResponse]:
        """Ollama's streaming shape: chunks with ``done=False`` carrying response pieces, then one
        ``done=True`` chunk with an empty response and the timing fields.  Backends without incremental
        output send the whole answer as one piece."""
        r = self.generate(model, prompt, system, options, raw)
        yield GenerateResponse(model=model, response=r.response, done=False, done_reason="", created_at=r.created_at)
        yield dataclasses.replace(r, response="")

    def score(self, model: str, prompt: str, completions, system: str = "", options: Optional[dict] = None,
              raw: bool = False, top_logprobs: int = 0) -> dict:
        """Teacher-forced scoring: the log-likelihood the model gives each of ``completions`` after the rendered prompt
        (``EngineService.score`` states the answer's shape)."""
        raise NotImplementedError

    def embed(self, model: str, input, truncate: bool = True, options: Optional[dict] = None) -> dict:
        """Ollama's ``/api/embed``: one unit vector per input text (``EngineService.embed`` states the semantics and
        the answer's shape)."""
        raise NotImplementedError

    def models(self) -> list:
        return []

    def health(self, deep: bool = False) -> dict:
        return {"ok": True}


# -------------------------------------------------------------------------------------- engines
class EngineUnavailable(RuntimeError):
    """The model's engine is down (its loop died and could not be restarted): the serving layer answers
    503 at once instead of letting requests wait for the timeout."""


def _fatal_device_error(e: BaseException) -> bool:
    """A GPU fault poisons the HIP context: the engine cannot be reset in this process."""
    from .engine.runner import TPCommError

    if isinstance(e, TPCommError):  # the lockstep TP group is out of sync: never step it again
        return True
    msg = str(e)
    return any(k in msg for k in ("HIP error", "hipError", "CUDA error", "illegal memory access",
                                  "device-side assert", "Memory access fault"))


class _EngineLoop:
    """Drives one LLMEngine from a background thread; callers block on their request's event.

    Failure handling: when a step raises, every queued / running request is failed at once
    (``LLMEngine.abort_all``) and the loop keeps serving -- up to ``max_errors`` failures inside
    ``error_window_s``.  A fatal device error, or too many failures, ends the loop; ``EngineService``
    then rebuilds the engine or answers ``EngineUnavailable``.

    ``every_error_fatal`` (the leader of a lockstep TP replica, parallel/lockstep.py): any step exception
    ends the loop, because a failure after a mirrored call left the followers inside collectives the leader
    never joins; ``on_fatal(e)`` then runs before any request is released (the TP leader exits, so the
    router re-dispatches its in-flight requests and terminates the followers)."""

    def __init__(self, engine, run_ahead: int = 16, max_errors: int = 3, error_window_s: float = 60.0,
                 every_error_fatal: bool = False, on_fatal: Optional[Callable[[BaseException], None]] = None):
        self.engine = engine
        self.max_errors, self.error_window_s = max_errors, error_window_s
        self.every_error_fatal, self.on_fatal = every_error_fatal, on_fatal
        self._errors: list = []
        self.restarts = 0
        engine.run_ahead = run_ahead  # serving: bound each decode run so arrivals are admitted promptly
        # each engine runs on its own HIP stream: co-served models overlap on the GPU, and one engine's
        # host syncs never wait for the other's queued kernels
        self.stream = None
        dev = getattr(getattr(engine, "runner", None), "device", None)
        if dev is not None and torch.device(dev).type == "cuda":
            self.stream = torch.cuda.Stream(device=dev)
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        self._cv = threading.Condition()
        self._stop = False
        self._err: Optional[BaseException] = None
        self._t = threading.Thread(target=self._run, name=f"engine-{engine.name}", daemon=True)
        self._t.start()

    def submit_many(self, prompts, params) -> list:
        """``submit`` for several prompts that should be admitted together (``LLMEngine.add_requests``)."""
        if not self.alive():
            raise EngineUnavailable(f"engine {self.engine.name} is down: {self._err!r}")
        reqs = self.engine.add_requests(prompts, params)
        with self._cv:
            self._cv.notify()
        return reqs

    def submit(self, ids, params, stream: bool = False):
        if not self.alive():
            raise EngineUnavailable(f"engine {self.engine.name} is down: {self._err!r}")
        req = self.engine.add_request(ids, params, stream=stream)
        with self._cv:
            self._cv.notify()
        return req

    def _run(self):
        from .utils.metrics import REGISTRY

        while not self._stop:
            with self._cv:
                while not self._stop and not self.engine.has_work():
                    self._cv.wait(timeout=0.5)
            if self._stop:
                return
            try:
                if self.stream is not None:
                    with torch.cuda.stream(self.stream):
                        self.engine.step()
                else:
                    self.engine.step()
            except BaseException as e:  # noqa: BLE001 - surface to waiting callers
                REGISTRY.inc("lsa_engine_errors_total", 1, "engine step failures", model=self.engine.name)
                now = time.monotonic()
                self._errors = [t for t in self._errors if now - t < self.error_window_s] + [now]
                fatal = (self.every_error_fatal or _fatal_device_error(e)
                         or len(self._errors) > self.max_errors)
                if fatal:
                    self._err = e  # alive() turns false before any caller is released
                    if self.on_fatal is not None:
                        self.on_fatal(e)
                try:
                    self.engine.abort_all(repr(e))
                except BaseException:  # noqa: BLE001
                    self._err = e
                    fatal = True
                if fatal:
                    return
                self.restarts += 1  # the engine is empty and consistent again: keep serving

    def alive(self) -> bool:
        return self._t.is_alive() and self._err is None

    def close(self):
        self._stop = True
        with self._cv:
            self._cv.notify_all()


class EngineService(Backend):
    """Named in-process engines (built lazily through ``factory``) behind the Ollama call shape."""

    def __init__(self, factory: Callable[[str], object], defaults: Optional[dict] = None,
                 timeout_s: float = 300.0, max_rebuilds: int = 2, every_error_fatal: bool = False,
                 on_fatal: Optional[Callable[[BaseException], None]] = None):
        self._factory = factory
        self._loop_kw = dict(every_error_fatal=every_error_fatal, on_fatal=on_fatal)
        self._loops: Dict[str, _EngineLoop] = {}
        self._lock = threading.Lock()
        self.defaults = defaults or {}
        self.timeout_s = timeout_s
        self.max_rebuilds = max_rebuilds
        self.rebuilds: Dict[str, int] = {}
        self._build_err: Dict[str, BaseException] = {}

    def loop(self, model: str) -> _EngineLoop:
        """The model's engine loop, built on first use and rebuilt (at most ``max_rebuilds`` times) after
        its loop died; a model that cannot be (re)built raises ``EngineUnavailable``."""
        with self._lock:
            lp = self._loops.get(model)
            if lp is not None and lp.alive():
                return lp
            if lp is not None:  # dead loop: rebuild the engine once the old one is released
                if self.rebuilds.get(model, 0) >= self.max_rebuilds:
                    raise EngineUnavailable(f"engine {model} is down after {self.rebuilds[model]} rebuilds: "
                                            f"{lp._err!r}")
                self.rebuilds[model] = self.rebuilds.get(model, 0) + 1
                lp.close()
                del self._loops[model]
                lp = None
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()
            try:
                self._loops[model] = _EngineLoop(self._factory(model), **self._loop_kw)
            except EngineUnavailable:
                raise
            except Exception as e:  # noqa: BLE001
                self._build_err[model] = e
                raise EngineUnavailable(f"engine {model} could not be built: {e!r}") from e
            return self._loops[model]

    def _submit(self, model, prompt, system, options, raw, stream=False):
        lp = self.loop(model)
        eng = lp.engine
        opts = dict(self.defaults)
        opts.update(options or {})
        # no num_predict (the reference's option-less calls): generate until EOS / the context window, as
        # Ollama does; the engine bounds it by num_ctx and its own max_new_cap
        params = SamplingParams.from_ollama_options(opts)
        ids = eng.encode(eng.render(prompt, system, raw))
        if params.num_ctx is not None:
            ids = eng.fit_context(ids, params.num_ctx, params.num_keep)
        return eng, lp.submit(ids, params, stream=stream)

    @staticmethod
    def _final(model, eng, req) -> GenerateResponse:
        r = eng.result(req)
        return GenerateResponse(model=model, response=r.text, done_reason=r.done_reason, created_at=_now(),
                                total_duration=r.total_duration_ns, load_duration=r.load_duration_ns,
                                prompt_eval_count=r.prompt_tokens, prompt_eval_duration=r.prompt_eval_duration_ns,
                                eval_count=r.eval_count, eval_duration=r.eval_duration_ns,
                                prompt_cached_count=r.cached_prompt_tokens, logprobs=r.logprobs,
                                prompt_logprobs=r.prompt_logprobs,
                                context_shifts=r.context_shifts if getattr(eng, "context_shift", False) else None)

    def generate(self, model, prompt, system="", options=None, raw=False) -> GenerateResponse:
        eng, req = self._submit(model, prompt, system, options, raw)
        if not req.done.wait(self.timeout_s):
            raise TimeoutError(f"generation on {model} timed out after {self.timeout_s}s")
        if req.error:
            raise RuntimeError(f"engine {model} failed: {req.error}")
        return self._final(model, eng, req)

    def generate_stream(self, model, prompt, system="", options=None, raw=False) -> Iterator[GenerateResponse]:
        """Pieces of the answer as the engine's decode runs complete (every ``sync_every`` steps, or
        ``run_ahead`` steps for requests that ignore EOS), then the final chunk with the timings."""
        eng, req = self._submit(model, prompt, system, options, raw, stream=True)
        try:
            sent = 0  # generated tokens whose logprob entries went out
            for piece in eng.stream_text(req, timeout_s=self.timeout_s):
                ents = None
                if req.params.logprobs:  # the entries of the tokens this sync revealed
                    toks = req.stream_toks
                    ents = eng.logprob_entries(req, toks[sent:], start=sent)
                    sent = len(toks)
                yield GenerateResponse(model=model, response=piece, done=False, done_reason="", created_at=_now(),
                                       logprobs=ents)
        except queue.Empty:
            raise TimeoutError(f"generation on {model} timed out after {self.timeout_s}s") from None
        except RuntimeError as e:
            raise RuntimeError(f"engine {model} failed: {e}") from None
        last = self._final(model, eng, req)
        if last.logprobs is not None:  # what no earlier chunk carried; over the chunks: the non-streamed list
            last = dataclasses.replace(last, logprobs=last.logprobs[sent:])
        yield dataclasses.replace(last, response="")  # (prompt_logprobs rides whole with this final chunk)

    MAX_SCORE_COMPLETIONS = 64

    def score(self, model, prompt, completions, system="", options=None, raw=False, top_logprobs=0) -> dict:
        """The log-likelihood of each completion given the prompt, through the prefill (prompt-token logprobs).

        The rendered prompt is tokenised as ``generate`` tokenises it; each completion is tokenised on its own, without
        BOS, and appended (the lm-eval-harness convention: a joint tokenisation of prompt + completion could merge
        across the seam and differ).  Each completion is one ordinary engine request -- max_tokens 1 (the token is
        discarded), prompt_logprobs_from = the prompt's length, logprobs off -- and all are submitted together, so they
        batch and, with the prefix cache, share the prompt's blocks.  Scoring never truncates: what does not fit the
        context window is refused (``SamplingOptionError``), as are an empty completion and more than 64 of them.

        -> {"model", "prompt_eval_count", "scores": [{"completion", "tokens", "logprob" (sum), "mean_logprob",
        "min_logprob", "token_logprobs": [entries]}], "total_duration"}"""
        t0 = time.perf_counter()
        if isinstance(completions, str):
            completions = [completions]
        completions = list(completions)
        if not completions:
            raise SamplingOptionError("score needs at least one completion")
        if len(completions) > self.MAX_SCORE_COMPLETIONS:
            raise SamplingOptionError(f"score takes at most {self.MAX_SCORE_COMPLETIONS} completions a call")
        lp = self.loop(model)
        eng = lp.engine
        opts = dict(self.defaults)
        opts.update(options or {})
        opts.update(num_predict=1, logprobs=False, prompt_logprobs=True, top_logprobs=top_logprobs)
        params = SamplingParams.from_ollama_options(opts)
        ids = eng.tok.encode(eng.render(prompt, system, raw), add_bos=True)
        window = eng.runner.max_model_len if params.num_ctx is None else min(eng.runner.max_model_len,
                                                                            int(params.num_ctx))
        seqs = []
        for c in completions:
            cids = eng.tok.encode(c, add_bos=False) if isinstance(c, str) else []
            if not cids:
                raise SamplingOptionError("score: a completion is empty (no tokens)")
            if len(ids) + len(cids) > window - 1:
                raise SamplingOptionError(f"score: prompt ({len(ids)} tokens) + completion ({len(cids)}) does not fit "
                                          f"the context window ({window}); scoring never truncates")
            seqs.append(ids + cids)
        params = dataclasses.replace(params, prompt_logprobs_from=len(ids), max_tokens=1)
        reqs = lp.submit_many(seqs, params)  # admitted together: one packed prefill, one shared prompt
        scores = []
        for c, req in zip(completions, reqs):
            if not req.done.wait(self.timeout_s):
                raise TimeoutError(f"scoring on {model} timed out after {self.timeout_s}s")
            if req.error:
                raise RuntimeError(f"engine {model} failed: {req.error}")
            ents = eng.result(req).prompt_logprobs[len(ids):]
            lps = [float(e["logprob"]) for e in ents]
            scores.append({"completion": c, "tokens": len(ents), "logprob": sum(lps), "mean_logprob": sum(lps) / len(lps),
                           "min_logprob": min(lps), "token_logprobs": ents})
        return {"model": model, "prompt_eval_count": len(ids), "scores": scores,
                "total_duration": int((time.perf_counter() - t0) * 1e9)}

    MAX_EMBED_INPUTS = 64

    @staticmethod
    def embed_inputs(input, limit: int) -> list:
        """``input`` (a string or a list of strings) as a list, refused when empty or longer than ``limit``."""
        texts = [input] if isinstance(input, str) else list(input) if isinstance(input, (list, tuple)) else None
        if texts is None or any(not isinstance(t, str) for t in texts):
            raise SamplingOptionError("embed: input must be a string or a list of strings")
        if not texts:
            raise SamplingOptionError("embed needs at least one input")
        if len(texts) > limit:
            raise SamplingOptionError(f"embed takes at most {limit} inputs a call")
        return texts

    @staticmethod
    def embed_pooling(options: Optional[dict]) -> str:
        """The option extension ``pooling``: "last" (the default) or "mean"."""
        pooling = (options or {}).get("pooling", "last")
        if pooling not in ("last", "mean"):
            raise SamplingOptionError('pooling must be "last" or "mean"')
        return pooling

    def embed(self, model, input, truncate=True, options=None) -> dict:
        """One vector per input: the final-norm output of the model (what the lm_head reads, in f32), pooled over the
        input's tokens -- the last token's row (``"pooling": "last"``, the default) or the mean over all of them, BOS
        included (``"mean"``) -- and divided by its Euclidean norm.

        Each input is tokenised on its own with BOS and no prompt template.  The window is min(max_model_len, num_ctx),
        less one position for the request's single discarded token: a longer input keeps its first window - 1 tokens
        when ``truncate`` (Ollama's default) and is refused otherwise.  Each input is one ordinary engine request of
        one token and all are submitted together, so they pack into one prefill.  Refused (``SamplingOptionError``):
        an engine without embeddings or under TP > 1, an unknown pooling, no input or more than 64, an input with no
        token besides BOS.

        -> {"model", "embeddings": [[float] * d] * n, "total_duration", "load_duration": 0, "prompt_eval_count"}"""
        t0 = time.perf_counter()
        texts = self.embed_inputs(input, self.MAX_EMBED_INPUTS)
        pooling = self.embed_pooling(options)
        lp = self.loop(model)
        eng = lp.engine
        opts = dict(self.defaults)
        opts.update(options or {})
        opts.update(num_predict=1, logprobs=False, prompt_logprobs=False, top_logprobs=0)
        for k in ("regex", "stop"):
            opts.pop(k, None)
        params = dataclasses.replace(SamplingParams.from_ollama_options(opts), embed=pooling, max_tokens=1)
        window = eng.runner.max_model_len if params.num_ctx is None else min(eng.runner.max_model_len,
                                                                            int(params.num_ctx))
        seqs = []
        for t in texts:
            ids = eng.tok.encode(t, add_bos=True)
            if len(ids) < 2:
                raise SamplingOptionError("embed: an input is empty (no tokens besides BOS)")
            if len(ids) > window - 1:
                if not truncate:
                    raise SamplingOptionError(f"embed: an input of {len(ids)} tokens does not fit the context window "
                                              f"({window}, less the request's one token) and truncate is false")
                ids = ids[:window - 1]
            if len(ids) < 2:
                raise SamplingOptionError(f"embed: the context window ({window}) leaves no room for an input")
            seqs.append(ids)
        reqs = lp.submit_many(seqs, params)  # admitted together: one packed prefill
        vecs = []
        for req in reqs:
            if not req.done.wait(self.timeout_s):
                raise TimeoutError(f"embedding on {model} timed out after {self.timeout_s}s")
            if req.error:
                raise RuntimeError(f"engine {model} failed: {req.error}")
            vecs.append(eng.result(req).embedding)
        return {"model": model, "embeddings": vecs, "total_duration": int((time.perf_counter() - t0) * 1e9),
                "load_duration": 0, "prompt_eval_count": sum(len(s) for s in seqs)}

    def models(self) -> list:
        return sorted(self._loops)

    def health(self, deep: bool = False) -> dict:
        return {"ok": all(lp.alive() for lp in self._loops.values()),
                "engines": {m: {"alive": lp.alive(), "running": lp.engine.sched.num_running,
                                "waiting": lp.engine.sched.num_waiting, "kv_usage": lp.engine.sched.kv_usage,
                                "prefix_cached_blocks": lp.engine.sched.cached_blocks,
                                "restarts": lp.restarts, "rebuilds": self.rebuilds.get(m, 0),
                                "spec_batch": getattr(lp.engine, "spec_batch", 1),
                                "spec_batch_sampled": bool(getattr(getattr(lp.engine, "runner", None),
                                                                   "spec_batch_sampled", False)),
                                "spec_batch_guided": bool(getattr(getattr(lp.engine, "runner", None),
                                                                  "spec_batch_guided", False)),
                                "logprobs": bool(getattr(lp.engine, "logprobs", False)),
                                "prompt_logprobs": bool(getattr(lp.engine, "prompt_logprobs_supported", False)),
                                "spec_logprobs": bool(getattr(getattr(lp.engine, "runner", None),
                                                              "spec_logprobs", False)),
                                "context_shift": bool(getattr(lp.engine, "context_shift", False)),
                                "context_shift_fp8": bool(getattr(lp.engine, "context_shift_fp8", False)),
                                "embeddings": bool(getattr(lp.engine, "embeddings_supported", False)),
                                **_weights_health(lp.engine),
                                **lp.engine.stats} for m, lp in self._loops.items()}}


def _weights_health(engine) -> dict:
    """The weight kind an engine serves (the kind it was built for, on the CPU too) and, for a GGUF load, the file's
    tensor count per ggml type."""
    w = getattr(getattr(engine, "runner", None), "w", None)
    if w is None:
        return {}
    pw = w.layers[0].wqkv
    out = {"weight_kind": getattr(pw, "requested", None) or pw.kind}
    src = getattr(w, "source", None)
    if src:
        out["checkpoint_format"] = src.get("format")
        out["gguf_tensor_types"] = dict(src.get("tensor_types") or {})
    return out


# -------------------------------------------------------------------------------------- fake
class FakeBackend(Backend):
    """Deterministic stand-in for tests: NL->SQL returns ``sql_for(prompt)``, explain returns a fixed
    analysis.  ``fail_next`` injects an exception (failure-path tests)."""

    def __init__(self, sql: Optional[Callable[[str, str], str]] = None, explanation: str = ""):
        self.sql = sql or (lambda prompt, system: "SELECT * FROM temp_view LIMIT 10;")
        self.explanation = explanation or ("The query references a column that does not exist in temp_view. "
                                           "Check the column names in the table schema and correct the query.")
        self.calls = []
        self.fail_next: Optional[BaseException] = None
        self._lock = threading.Lock()

    def generate(self, model, prompt, system="", options=None, raw=False) -> GenerateResponse:
        with self._lock:
            self.calls.append({"model": model, "prompt": prompt, "system": system, "options": options})
            if self.fail_next is not None:
                e, self.fail_next = self.fail_next, None
                raise e
        if options and (options.get("logprobs") or options.get("top_logprobs") or options.get("prompt_logprobs")):
            raise SamplingOptionError("the fake backend has no model distribution: logprobs cannot be served")
        t0 = time.perf_counter()
        if options and options.get("fake_delay"):
            time.sleep(float(options["fake_delay"]))
        text = self.explanation if "Spark error" in prompt or "troubleshoot" in system else self.sql(prompt, system)
        dt = int((time.perf_counter() - t0) * 1e9)
        return GenerateResponse(model=model, response=text, created_at=_now(), total_duration=dt,
                                eval_count=len(text.split()), eval_duration=dt, prompt_eval_count=len(prompt.split()))

    def score(self, model, prompt, completions, system="", options=None, raw=False, top_logprobs=0) -> dict:
        raise SamplingOptionError("the fake backend has no model distribution: completions cannot be scored")

    EMBED_DIM = 64

    def embed(self, model, input, truncate=True, options=None) -> dict:
        """Deterministic unit vectors of ``EMBED_DIM`` entries, a function of (model, text, pooling) alone."""
        import hashlib

        texts = EngineService.embed_inputs(input, EngineService.MAX_EMBED_INPUTS)
        pooling = EngineService.embed_pooling(options)
        with self._lock:
            self.calls.append({"model": model, "input": input, "truncate": truncate, "options": options})
        vecs = []
        for t in texts:
            if not t.strip():
                raise SamplingOptionError("embed: an input is empty (no tokens besides BOS)")
            raw = b"".join(hashlib.sha256(f"{model}\0{pooling}\0{i}\0{t}".encode()).digest()
                           for i in range(self.EMBED_DIM // 32))
            v = [b / 127.5 - 1.0 for b in raw[:self.EMBED_DIM]]
            nrm = sum(x * x for x in v) ** 0.5 or 1.0
            vecs.append([x / nrm for x in v])
        return {"model": model, "embeddings": vecs, "total_duration": 0, "load_duration": 0,
                "prompt_eval_count": sum(1 + len(t.split()) for t in texts)}

    def models(self):
        return ["duckdb-nsql", "llama3.2", "mistral"]


# -------------------------------------------------------------------------------------- remote
class RemoteBackend(Backend):
    def __init__(self, url: str = "http://127.0.0.1:8000", timeout_s: float = 300.0):
        self.url = url.rstrip("/")
        self.timeout_s = timeout_s

    def generate(self, model, prompt, system="", options=None, raw=False) -> GenerateResponse:
        import urllib.request

        body = json.dumps({"model": model, "prompt": prompt, "system": system, "options": options or {},
                           "stream": False, "raw": raw}).encode()
        req = urllib.request.Request(self.url + "/api/generate", data=body, headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=self.timeout_s) as f:
            d = json.loads(f.read())
        fields = {f.name for f in dataclasses.fields(GenerateResponse)} | {"prompt_logprobs", "context_shifts"}
        return GenerateResponse(**{k: v for k, v in d.items() if k in fields})

    def score(self, model, prompt, completions, system="", options=None, raw=False, top_logprobs=0) -> dict:
        import urllib.error
        import urllib.request

        body = json.dumps({"model": model, "prompt": prompt, "system": system, "options": options or {}, "raw": raw,
                           "completions": [completions] if isinstance(completions, str) else list(completions),
                           "top_logprobs": top_logprobs}).encode()
        req = urllib.request.Request(self.url + "/api/score", data=body, headers={"Content-Type": "application/json"})
        try:
            with urllib.request.urlopen(req, timeout=self.timeout_s) as f:
                return json.loads(f.read())
        except urllib.error.HTTPError as e:
            if e.code == 400:  # what the engine refused, as the in-process backend raises it
                raise SamplingOptionError(e.read().decode(errors="replace")) from None
            raise


    def embed(self, model, input, truncate=True, options=None) -> dict:
        import urllib.error
        import urllib.request

        body = json.dumps({"model": model, "input": input, "truncate": bool(truncate), "options": options or {}}).encode()
        req = urllib.request.Request(self.url + "/api/embed", data=body, headers={"Content-Type": "application/json"})
        try:
            with urllib.request.urlopen(req, timeout=self.timeout_s) as f:
                return json.loads(f.read())
        except urllib.error.HTTPError as e:
            if e.code == 400:  # what the engine refused, as the in-process backend raises it
                raise SamplingOptionError(e.read().decode(errors="replace")) from None
            if e.code == 501:
                raise NotImplementedError(e.read().decode(errors="replace")) from None
            raise


# -------------------------------------------------------------------------------------- module API
_backend: Optional[Backend] = None
_blk = threading.Lock()


def set_backend(b: Backend) -> None:
    global _backend
    with _blk:
        _backend = b


def get_backend() -> Backend:
    global _backend
    with _blk:
        if _backend is None:
            from .serving.service import backend_from_settings
            from .config import Settings

            _backend = backend_from_settings(Settings())
        return _backend


def generate(model: str, prompt: str = "", system: str = "", options: Optional[dict] = None, raw: bool = False,
             logprobs: bool = False, top_logprobs: int = 0, prompt_logprobs: bool = False,
             **_ignored) -> GenerateResponse:
    """Drop-in for ``ollama.generate(model=, system=, prompt=)``.  ``logprobs`` / ``top_logprobs`` (Ollama's top-level
    request fields) and ``prompt_logprobs`` travel to the backend inside ``options``."""
    if logprobs or top_logprobs:
        options = dict(options or {}, logprobs=bool(logprobs), top_logprobs=top_logprobs)
    if prompt_logprobs:
        options = dict(options or {}, prompt_logprobs=True)
    return get_backend().generate(model, prompt, system, options, raw)


def score(model: str, prompt: str = "", completions=(), system: str = "", options: Optional[dict] = None,
          raw: bool = False, top_logprobs: int = 0) -> dict:
    """The log-likelihood the model gives each of ``completions`` (a string or a list) after the prompt:
    ``EngineService.score`` through the configured backend."""
    return get_backend().score(model, prompt, completions, system, options, raw, top_logprobs)


def embed(model: str, input="", truncate: bool = True, options: Optional[dict] = None, **_ignored) -> dict:
    """Drop-in for ``ollama.embed(model=, input=)``: one unit vector per input text (a string or a list), through the
    configured backend (``EngineService.embed``)."""
    return get_backend().embed(model, input, truncate, options)
