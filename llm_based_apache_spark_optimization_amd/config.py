"""One settings object for the whole service (env vars ``LSA_*`` + CLI flags).

The reference hard-codes everything (SURVEY.md §5 "Config / flag system"): WSL input/output paths
(FastAPI/app.py:68,118; Flask/app.py:19-20), the MySQL DSN 172.23.131.215 root/root db ``project``
(FastAPI/app.py:31-36), model names (FastAPI/app.py:86,106), the Flask secret (Flask/app.py:12),
host/port (FastAPI/app.py:148, Flask default 5000) and the history page size 8 (Flask/app.py:214).
Defaults here keep the reference behaviour (model names, page size, ports) while making every value
configurable.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
from typing import Optional


def _env(name: str, default, cast=str):
    v = os.environ.get("LSA_" + name)
    if v is None:
        return default
    if cast is bool:
        return v.lower() in ("1", "true", "yes", "on")
    return cast(v)


@dataclasses.dataclass
class Settings:
    # paths
    input_dir: str = dataclasses.field(default_factory=lambda: _env("INPUT_DIR", os.path.abspath("data/Input")))
    output_dir: str = dataclasses.field(default_factory=lambda: _env("OUTPUT_DIR", os.path.abspath("data/Output")))
    # persistence: "sqlite:///path.db" (default) or "mysql://user:pw@host/db"
    history_dsn: str = dataclasses.field(default_factory=lambda: _env("HISTORY_DSN", "sqlite:///data/history.db"))
    history_page_size: int = dataclasses.field(default_factory=lambda: _env("HISTORY_PAGE_SIZE", 8, int))
    # SQL execution backend: "sqlite" (default) | "spark" (needs pyspark)
    sql_backend: str = dataclasses.field(default_factory=lambda: _env("SQL_BACKEND", "sqlite"))
    # models
    nl2sql_model: str = dataclasses.field(default_factory=lambda: _env("NL2SQL_MODEL", "duckdb-nsql"))
    explain_model: str = dataclasses.field(default_factory=lambda: _env("EXPLAIN_MODEL", "llama3.2"))
    # engine: "hip" (MI355X engine), "fake" (deterministic test engine), "remote" (HTTP to another server)
    engine: str = dataclasses.field(default_factory=lambda: _env("ENGINE", "hip"))
    remote_url: str = dataclasses.field(default_factory=lambda: _env("REMOTE_URL", "http://127.0.0.1:8000"))
    # checkpoints of the NL->SQL and the explain model: an HF directory (config.json + *.safetensors) or a GGUF file
    # (an Ollama blob); unset = seeded random weights
    checkpoint_dir: Optional[str] = dataclasses.field(default_factory=lambda: _env("CHECKPOINT_DIR", None))
    explain_checkpoint_dir: Optional[str] = dataclasses.field(
        default_factory=lambda: _env("EXPLAIN_CHECKPOINT_DIR", None))
    # weight kinds: "bf16" | "fp8" | "mxfp4" | "q4_0" (a GGUF file's own Q4_0 codes and scales, engine/factory.py)
    dtype: str = dataclasses.field(default_factory=lambda: _env("DTYPE", "bf16"))
    explain_dtype: str = dataclasses.field(default_factory=lambda: _env("EXPLAIN_DTYPE", "bf16"))
    # paged KV cache dtype of every engine: "bf16" | "fp8" (e4m3 rows + per-row scales, ops.KV_FP8)
    kv_dtype: str = dataclasses.field(default_factory=lambda: _env("KV_DTYPE", "bf16"))
    # prompt-lookup speculative decoding for batch-1 greedy requests: tokens drafted per verify step (0 = off; 3 works
    # for every served model), and the acceptance guard's break-even (accepted drafts per verify step below which a
    # request falls back to plain steps; < 0 = the runner's default)
    spec_tokens: int = dataclasses.field(default_factory=lambda: _env("SPEC_TOKENS", 0, int))
    spec_min_accept: float = dataclasses.field(default_factory=lambda: _env("SPEC_MIN_ACCEPT", -1.0, float))
    # speculate with fp8 / MXFP4 weights and the fp8 KV cache too (off: those engines take plain steps whatever
    # spec_tokens says).  Opt-in because their verify rows run weight-only GEMMs while the plain batch-1 step may run
    # e4m3 activations: a speculated request can leave the plain request's token sequence earlier than a near-tie
    spec_quantized: bool = dataclasses.field(default_factory=lambda: _env("SPEC_QUANTIZED", False, bool))
    # prefix cache (off by default): the KV blocks of full 64-token prompt blocks stay cached after their request and
    # are shared with later requests whose prompt starts with the same tokens; prompts of every caller of one engine
    # share KV then.  prefix_cow_min_tokens: the shortest common prefix with a cached block for which the block is
    # forked (copied, the rest prefilled) rather than prefilled whole; 64 = never fork.  Default 8: the smallest p of
    # the sweep 8 / 16 / 32 / 48 whose saved time to first token is >= 2x the block copy's device time on both models
    # (7B: copy 21.6 us, 8 more suffix tokens cost 921 us; 3B: 17.3 us against 609 us; scripts/bench_prefix_cache.py,
    # profiles/prefix_cache/cow_sweep_mi355x.jsonl)
    prefix_cache: bool = dataclasses.field(default_factory=lambda: _env("PREFIX_CACHE", False, bool))
    prefix_cow_min_tokens: int = dataclasses.field(default_factory=lambda: _env("PREFIX_COW_MIN_TOKENS", 8, int))
    # regex-constrained decoding (off by default): requests may carry the option "regex"; the answer is then a full
    # match of the pattern (engine/guided.py).  sql_guided (needs guided): /nl2sql constrains the NL->SQL model to
    # prompts.SQL_STATEMENT_REGEX -- one SELECT / WITH statement that ends at its first ';'
    guided: bool = dataclasses.field(default_factory=lambda: _env("GUIDED", False, bool))
    sql_guided: bool = dataclasses.field(default_factory=lambda: _env("SQL_GUIDED", False, bool))
    # constrained requests speculate too (off: a request with a regex takes plain guided steps whatever spec_tokens
    # says).  Needs guided and spec_tokens; the tokens are those of the plain guided steps
    spec_guided: bool = dataclasses.field(default_factory=lambda: _env("SPEC_GUIDED", False, bool))
    # requests that need the sampler speculate too (off: a request with temperature > 0 or a repetition penalty takes
    # plain steps whatever spec_tokens says).  Needs spec_tokens; verify row i makes the plain step's draw for its
    # token, so the tokens are those of the plain sampled steps of the same seed
    spec_sampled: bool = dataclasses.field(default_factory=lambda: _env("SPEC_SAMPLED", False, bool))
    # the largest number of running greedy, unconstrained requests whose decode run may be a run of verify steps (1:
    # only a request that runs alone speculates).  Needs spec_tokens; clamped to a power of two with spec_batch * T <= 32,
    # at most 8 and at most the engine's slots (max_batch).  All or nothing: one running request that cannot speculate makes the run plain
    spec_batch: int = dataclasses.field(default_factory=lambda: _env("SPEC_BATCH", 1, int))
    # requests that need the sampler speculate in such a run too, beside greedy ones (off: one of them makes the run
    # plain).  Needs spec_tokens, spec_sampled and spec_batch > 1; every request's tokens are those it generates alone
    spec_batch_sampled: bool = dataclasses.field(default_factory=lambda: _env("SPEC_BATCH_SAMPLED", False, bool))
    # regex-constrained requests speculate in such a run too, beside unconstrained ones (off: one of them makes the run
    # plain).  Needs guided, spec_guided, spec_tokens and spec_batch > 1 (and spec_batch_sampled for a constrained
    # request that needs the sampler); every request's tokens are those of its plain guided steps
    spec_batch_guided: bool = dataclasses.field(default_factory=lambda: _env("SPEC_BATCH_GUIDED", False, bool))
    # per-token logprobs (off by default): requests may carry "logprobs" / "top_logprobs" (0 .. 20) and get every
    # generated token's log-probability under the model's own distribution (raw logits: before the regex mask, the
    # penalties and temperature / top-k / top-p / min-p).  sql_logprobs (needs logprobs): /nl2sql and the pipeline's
    # job result add sql_mean_logprob / sql_min_logprob of the generated statement
    logprobs: bool = dataclasses.field(default_factory=lambda: _env("LOGPROBS", False, bool))
    sql_logprobs: bool = dataclasses.field(default_factory=lambda: _env("SQL_LOGPROBS", False, bool))
    # a request that asked for logprobs speculates too (off: it takes plain steps and makes a spec_batch run plain).
    # Needs logprobs and spec_tokens; the records are the log-softmax of the raw verify rows
    spec_logprobs: bool = dataclasses.field(default_factory=lambda: _env("SPEC_LOGPROBS", False, bool))
    # context shift (off by default): a request that fills its num_ctx window keeps its first num_keep tokens, drops
    # half of the rest and goes on generating, as Ollama does, instead of ending at the window; the option extension
    # "shift": false opts a request out.  Inert with tp > 1, and on the fp8 KV cache without context_shift_fp8
    context_shift: bool = dataclasses.field(default_factory=lambda: _env("CONTEXT_SHIFT", False, bool))
    # context shift on the fp8 KV cache too (off by default; needs context_shift): a surviving key is dequantised,
    # rotated and quantised again once per shift, with a new row scale.  Still inert with tp > 1
    context_shift_fp8: bool = dataclasses.field(default_factory=lambda: _env("CONTEXT_SHIFT_FP8", False, bool))
    # embeddings (off by default): POST /api/embed returns one unit vector per input, pooled on the device from the
    # final-norm rows of the prefill ("pooling": "last", the default, or "mean").  Refused with tp > 1
    embeddings: bool = dataclasses.field(default_factory=lambda: _env("EMBEDDINGS", False, bool))
    tp: int = dataclasses.field(default_factory=lambda: _env("TP", 1, int))
    dp: int = dataclasses.field(default_factory=lambda: _env("DP", 1, int))
    max_batch: int = dataclasses.field(default_factory=lambda: _env("MAX_BATCH", 32, int))
    max_model_len: int = dataclasses.field(default_factory=lambda: _env("MAX_MODEL_LEN", 4096, int))
    # share of the free GPU memory each engine's paged KV arena takes when it is built (two co-served
    # models: the first gets 45 %, the second 45 % of what is left)
    kv_memory_fraction: float = dataclasses.field(default_factory=lambda: _env("KV_MEMORY_FRACTION", 0.45, float))
    # default num_predict of a request that sets none: -1 = Ollama's default, generate until EOS or the context
    # window (the reference's option-less ollama.generate calls, FastAPI/app.py:85-90,105-109)
    max_new_tokens: int = dataclasses.field(default_factory=lambda: _env("MAX_NEW_TOKENS", -1, int))
    # server safety cap on generated tokens per request (0 = the model context window); far above any
    # typical NL->SQL or explanation answer, it only bounds a model that never emits EOS
    max_new_cap: int = dataclasses.field(default_factory=lambda: _env("MAX_NEW_CAP", 0, int))
    # KV reservation at admission: prompt + this many generated tokens; decode runs grow the tables block by block
    # and an exhausted arena preempts the youngest request (-1 = reserve prompt + max_new up front)
    kv_reserve_tokens: int = dataclasses.field(default_factory=lambda: _env("KV_RESERVE_TOKENS", 64, int))
    # chunked-prefill interleave: prompt tokens prefilled per engine iteration (0 = whole prompts); longer
    # prompts stall the running decode batch one chunk at a time.  The budget also caps prefill throughput
    # (one chunk per decode run): 512 collapsed co-serving at 16 QPS (nl2sql p50 0.56 -> 3.4 s), 2048 does not
    # (scripts/gpu_r2_serving_ab.sh)
    prefill_chunk: int = dataclasses.field(default_factory=lambda: _env("PREFILL_CHUNK", 2048, int))
    # sampling defaults: greedy (the reference sampled at Ollama defaults; pass options to match)
    temperature: float = dataclasses.field(default_factory=lambda: _env("TEMPERATURE", 0.0, float))
    top_k: int = dataclasses.field(default_factory=lambda: _env("TOP_K", 40, int))
    top_p: float = dataclasses.field(default_factory=lambda: _env("TOP_P", 0.9, float))
    request_timeout_s: float = dataclasses.field(default_factory=lambda: _env("REQUEST_TIMEOUT", 300.0, float))
    # servers
    host: str = dataclasses.field(default_factory=lambda: _env("HOST", "127.0.0.1"))
    fastapi_port: int = dataclasses.field(default_factory=lambda: _env("FASTAPI_PORT", 8000, int))
    flask_port: int = dataclasses.field(default_factory=lambda: _env("FLASK_PORT", 5000, int))
    secret_key: str = dataclasses.field(default_factory=lambda: _env("SECRET_KEY", os.urandom(16).hex()))
    log_level: str = dataclasses.field(default_factory=lambda: _env("LOG_LEVEL", "INFO"))
    trace: bool = dataclasses.field(default_factory=lambda: _env("TRACE", False, bool))

    def ensure_dirs(self) -> None:
        os.makedirs(self.input_dir, exist_ok=True)
        os.makedirs(self.output_dir, exist_ok=True)
        if self.history_dsn.startswith("sqlite:///"):
            d = os.path.dirname(self.history_dsn[len("sqlite:///"):])
            if d:
                os.makedirs(d, exist_ok=True)

    @staticmethod
    def add_cli(ap: argparse.ArgumentParser) -> None:
        for f in dataclasses.fields(Settings):
            t = {int: int, float: float, bool: None}.get(type(Settings().__getattribute__(f.name)), str)
            flag = "--" + f.name.replace("_", "-")
            if t is None:
                ap.add_argument(flag, action="store_true", default=None)
            else:
                ap.add_argument(flag, type=t, default=None)

    @staticmethod
    def from_cli(ns: argparse.Namespace) -> "Settings":
        s = Settings()
        for f in dataclasses.fields(Settings):
            v = getattr(ns, f.name, None)
            if v is not None:
                setattr(s, f.name, v)
        return s
