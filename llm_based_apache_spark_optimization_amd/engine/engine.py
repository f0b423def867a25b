"""LLMEngine: continuous-batching text generation over a ModelRunner.

The request lifecycle mirrors what the reference gets from the Ollama daemon behind
``ollama.generate(model=, system=, prompt=)`` (FastAPI/app.py:85-90,105-109; Flask/app.py:102-107,
160-164; Model_Evaluation_&_Comparision.py:23,114): template -> tokenize -> prefill -> decode loop ->
detokenize, with the timing fields Ollama reports (and the reference ignored).

Scheduling is native (``runtime/_lsa_runtime.Scheduler``): FCFS admission into fixed decode slots.  KV is
reserved lazily: admission takes the prompt plus one 64-token block, each decode run first grows the running
tables to the context the run will reach, and when the arena is exhausted the youngest running request is
preempted (blocks and slot released, re-queued first with its generated tokens folded into its prompt and
re-prefilled on re-admission).  Each engine iteration prefills newly admitted
requests (packed, one launch sequence) and then replays the captured decode graph for
``sync_every`` steps before reading the finished flags back — the host touches the GPU once per
``sync_every`` tokens, not once per token.
"""
from __future__ import annotations

import dataclasses
import itertools
import math
import queue
import threading
import time
from typing import Callable, Iterator, Optional, Sequence

import torch

from ..models.templates import STOP_STRINGS, apply_stops, render
from ..models.tokenizer import token_bytes, tokenizer_for
from ..ops.reference import pack_seed
from ..runtime import native
from ..utils import tracing
from ..utils.metrics import REGISTRY, TOKEN_BUCKETS
from .guided import GuidedRequestError, compile_regex
from .runner import BLOCK, ModelRunner


UNLIMITED = 1 << 30  # max_tokens of a request without num_predict: EOS / context window end it


class SamplingOptionError(ValueError):
    """A request's sampler option cannot be served (a non-finite penalty or min_p, min_p outside [0, 1]).  The HTTP
    layer answers it with 400, as it answers a ``GuidedRequestError``."""


def _top_logprobs_option(v) -> int:
    try:
        return int(v or 0)
    except (TypeError, ValueError):
        raise SamplingOptionError("top_logprobs must be an integer in 0 .. 20") from None


def _shift_option(v) -> bool:
    if not isinstance(v, bool):
        raise SamplingOptionError("shift must be a boolean")
    return v


def _prompt_logprobs_from_option(v) -> int:
    if v is None:
        return 0
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise SamplingOptionError("prompt_logprobs_from must be a non-negative integer")
    return v


@dataclasses.dataclass
class SamplingParams:
    """Ollama-compatible options (temperature 0 = greedy, as the benchmark configs require)."""

    max_tokens: int = 128
    temperature: float = 0.0
    top_k: int = 40
    top_p: float = 0.9
    seed: Optional[int] = None
    ignore_eos: bool = False
    stop: tuple = ()
    # llama.cpp/Ollama repetition penalty over the last repeat_last_n (<= 64) context tokens.  1.0 = off
    # unless a request sets it (Ollama's own default is 1.1; the benchmark configs are plain greedy)
    repeat_penalty: float = 1.0
    repeat_last_n: int = 64
    # llama.cpp's presence / frequency penalties over the same window (after the repetition penalty, a token that
    # occurs c times there loses c * frequency_penalty + presence_penalty; negative values reward repeats) and min_p
    # (a candidate stays only with probability >= min_p times the best one's, on the temperature-scaled probabilities,
    # next to top_p -- Ollama's order; inert on a greedy request).  0.0 = off
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_p: float = 0.0
    num_ctx: Optional[int] = None    # Ollama context window (prompt + generated tokens); None = model's
    num_keep: int = 4
    # prompt-lookup speculative decoding, where the engine runs it (LLMEngine(spec_tokens > 0), batch 1: a greedy
    # request, and -- on an engine built with spec_sampled (LSA_SPEC_SAMPLED=1) -- one with temperature > 0 and / or a
    # repetition penalty, whose verify rows make the plain steps' draws of the same seed); the Ollama option extension
    # "speculate": false opts a request out.  The tokens are the same either way.
    speculate: bool = True
    # prefix cache, where the engine runs it (LLMEngine(prefix_cache=True)): llama.cpp's "cache_prompt": false opts a
    # request out -- it neither reuses cached KV blocks nor publishes its own
    cache_prompt: bool = True
    # regex-constrained decoding, where the engine runs it (LLMEngine(guided=True)): the Ollama option extension
    # "regex".  The generated text -- its UTF-8 bytes -- is a full match of the pattern (engine/guided.py: the supported
    # syntax) when the request ends by EOS; EOS is allowed only then.  A request that ends at its length limit is
    # returned as it stands, possibly short of a match.  Not with ignore_eos.  A constrained request speculates only
    # on an engine built with spec_guided (LSA_SPEC_GUIDED=1); its tokens are those of its plain guided steps.
    regex: Optional[str] = None
    # per-token log-probabilities, where the engine runs them (LLMEngine(logprobs=True)): Ollama's / OpenAI's
    # "logprobs" (bool) and "top_logprobs" (K, 0 .. 20).  Every generated token comes back with its log-probability
    # and, K > 0, the K most likely tokens of its step with theirs -- under the model's own distribution: log-softmax
    # over the whole vocabulary of the logits as the lm_head wrote them, before the regex mask, the penalties and
    # temperature / top-k / top-p / min-p.  A request that asks never speculates; its tokens are what they are without.
    logprobs: bool = False
    top_logprobs: int = 0
    # prompt-token log-probabilities (OpenAI's echo + logprobs, vLLM's prompt_logprobs; same engine flag): entry j of
    # the response list is the log-probability the model gives prompt token j after prompt tokens 0 .. j - 1 -- the
    # raw rule above, at the prefill row of position j - 1 -- for max(1, prompt_logprobs_from) <= j < prompt length;
    # entries below are null.  top_logprobs applies to them as to generated tokens.  Generation is what it is without.
    prompt_logprobs: bool = False
    prompt_logprobs_from: int = 0
    # context shift, where the engine runs it (LLMEngine(context_shift=True)): a request that fills its num_ctx window
    # keeps its first num_keep tokens, drops half of the rest and goes on, as Ollama does; the Ollama option extension
    # "shift": false opts a request out -- it then ends at the window
    shift: bool = True
    # embeddings, where the engine runs them (LLMEngine(embeddings=True)): "mean" or "last" makes the request an
    # embedding request -- its prefill pools the final-norm rows of the prompt on the device and the result carries the
    # unit vector (GenerationResult.embedding); it generates one token, which is discarded.  Set by the embed route
    # (serving/executor.py); not an Ollama option: ``from_ollama_options`` never sets it
    embed: Optional[str] = None

    @property
    def needs_sampler(self) -> bool:
        """Rows that need the sampling path (draw and/or a penalty) rather than the argmax-only graph."""
        return (self.temperature > 0 or self.repeat_penalty != 1.0 or self.presence_penalty != 0.0
                or self.frequency_penalty != 0.0)

    @staticmethod
    def from_ollama_options(opts: Optional[dict], default_max: int = UNLIMITED) -> "SamplingParams":
        """Ollama option dict -> params.  ``num_predict`` absent, None or negative = Ollama's default: generate
        until EOS or the context window (``LLMEngine.add_request`` bounds it by num_ctx / max_new_cap)."""
        opts = opts or {}
        n = opts.get("num_predict", default_max)
        if n is None or int(n) < 0:
            n = default_max if default_max is not None and default_max >= 0 else UNLIMITED
        stop = opts.get("stop") or ()
        # ignore_eos: benchmark extension (fixed-length outputs from random-init weights), not an Ollama option
        return SamplingParams(max_tokens=int(n), temperature=float(opts.get("temperature", 0.0)),
                              top_k=int(opts.get("top_k", 40)), top_p=float(opts.get("top_p", 0.9)),
                              seed=opts.get("seed"), stop=tuple(stop), ignore_eos=bool(opts.get("ignore_eos", False)),
                              repeat_penalty=float(opts.get("repeat_penalty", 1.0)),
                              repeat_last_n=int(opts.get("repeat_last_n", 64)),
                              presence_penalty=float(opts.get("presence_penalty", 0.0)),
                              frequency_penalty=float(opts.get("frequency_penalty", 0.0)),
                              min_p=float(opts.get("min_p", 0.0)),
                              num_ctx=int(opts["num_ctx"]) if opts.get("num_ctx") else None,
                              num_keep=int(opts.get("num_keep", 4)), speculate=bool(opts.get("speculate", True)),
                              cache_prompt=bool(opts.get("cache_prompt", True)),
                              regex=(str(opts["regex"]) if opts.get("regex") else None),
                              logprobs=bool(opts.get("logprobs", False)),
                              top_logprobs=_top_logprobs_option(opts.get("top_logprobs", 0)),
                              prompt_logprobs=bool(opts.get("prompt_logprobs", False)),
                              prompt_logprobs_from=_prompt_logprobs_from_option(opts.get("prompt_logprobs_from")),
                              shift=_shift_option(opts.get("shift", True)))


@dataclasses.dataclass
class Request:
    rid: int
    prompt_ids: list
    params: SamplingParams
    arrival: float
    admitted: float = 0.0
    first_token: float = 0.0
    finished_at: float = 0.0
    output_ids: list = dataclasses.field(default_factory=list)
    done: threading.Event = dataclasses.field(default_factory=threading.Event)
    slot: int = -1
    gen_host: int = 0  # generated-token count as of the last device sync
    prefilled: int = 0  # prompt tokens already in the KV cache (chunked prefill in progress when < len)
    error: Optional[str] = None
    # streaming: ("tokens", ids-so-far) after every host sync that saw new tokens, then ("done", None)
    stream: Optional[queue.Queue] = None
    streamed: int = 0
    stream_toks: list = dataclasses.field(default_factory=list)  # the snapshot ``stream_text`` last took from it
    # tokens generated before a preemption (lazy KV growth ran the arena dry): the current incarnation's prompt is
    # prompt_ids + resumed and its params.max_tokens the remaining budget
    resumed: list = dataclasses.field(default_factory=list)
    preemptions: int = 0
    # speculative decoding: verify steps / accepted drafts of this request so far, and the acceptance guard's verdict
    spec_steps: int = 0
    spec_accepted: int = 0
    spec_off: bool = False
    # prefix cache: prompt tokens whose KV was found in the cache (summed over re-admissions of a preempted request)
    cached_tokens: int = 0
    # regex-constrained decoding: the compiled pattern (engine/guided.py Dfa) of params.regex
    dfa: Optional[object] = None
    # per-token logprobs (params.logprobs): one (logprob, [(token id, logprob)] * K) per generated token, in order,
    # kept on the host across preemptions; lp_read = device records of the current incarnation already read
    logprobs: list = dataclasses.field(default_factory=list)
    lp_read: int = 0
    # prompt-token logprobs (params.prompt_logprobs): prompt_lp[j] = None or the record of prompt token j, kept on the
    # host across preemptions; plp_next = the next prompt index to score (records are made in prompt order);
    # plp_pending = device records of prefill calls not read yet: (records, first row, rows, first prompt index)
    prompt_lp: list = dataclasses.field(default_factory=list)
    plp_next: int = 0
    plp_pending: list = dataclasses.field(default_factory=list)
    # context shift (LLMEngine(context_shift=True)): shift_w = the window W of an eligible request, 0 = it ends at its
    # window; shifted = tokens discarded from its cache so far; drops = the (keep, discard) of each shift, in order --
    # the host mirror of the context as the cache holds it is ``kept_ids``
    shift_w: int = 0
    shifted: int = 0
    drops: list = dataclasses.field(default_factory=list)
    # embeddings (params.embed): the unit vector [d] f32, read at the host sync that retires the request
    embedding: Optional[torch.Tensor] = None

    @property
    def ctx_ids(self) -> list:
        """The prompt plus anything generated before a preemption: what the current incarnation prefills, unless the
        request has shifted its context (``kept_ids``)."""
        return self.prompt_ids + self.resumed if self.resumed else self.prompt_ids

    @property
    def base(self) -> int:
        """Context length of the current incarnation less its generated tokens: context = base + gen_host."""
        return len(self.prompt_ids) + len(self.resumed) - self.shifted

    @property
    def kept_ids(self) -> list:
        """``ctx_ids`` as the cache holds it: every shift's slice [keep, keep + discard) dropped, in order.  It is what
        a preempted request re-prefills; len(kept_ids) == base once the shifted tokens are all in ``resumed``."""
        ids = self.ctx_ids
        for keep, d in self.drops:
            ids = ids[:keep] + ids[keep + d:]
        return ids


@dataclasses.dataclass
class GenerationResult:
    text: str
    token_ids: list
    prompt_tokens: int
    eval_count: int
    total_duration_ns: int
    load_duration_ns: int
    prompt_eval_duration_ns: int
    eval_duration_ns: int
    done_reason: str
    cached_prompt_tokens: int = 0  # prompt tokens served from the prefix cache instead of being prefilled
    context_shifts: int = 0  # times the request's context was shifted at its num_ctx window (context_shift engines)
    # params.logprobs: one {"token", "logprob", "bytes", "top_logprobs": [{"token", "logprob", "bytes"}]} per generated
    # token (len == eval_count); None when the request did not ask
    logprobs: Optional[list] = None
    # params.prompt_logprobs: one entry per prompt token (len == prompt_tokens): None below max(1, prompt_logprobs_from),
    # else the same shape as a ``logprobs`` entry; None when the request did not ask
    prompt_logprobs: Optional[list] = None
    # params.embed: the pooled, normalised final-norm vector [d] as a list of floats; None when the request did not ask
    embedding: Optional[list] = None


class LLMEngine:
    def __init__(self, runner: ModelRunner, tokenizer=None, max_prefill_tokens: int = 16384, sync_every: int = 8,
                 name: Optional[str] = None, prefill_chunk: Optional[int] = None, kv_reserve_tokens: int = BLOCK,
                 spec_tokens: int = 0, prefix_cache: bool = False, prefix_cow_min_tokens: Optional[int] = None,
                 guided: bool = False, spec_batch: int = 0, logprobs: bool = False, context_shift: bool = False,
                 context_shift_fp8: bool = False, embeddings: bool = False):
        self.runner = runner
        if spec_tokens:  # speculative decoding for batch-1 greedy requests (the runner clamps it to what it supports)
            runner.spec_tokens = int(spec_tokens)
        if spec_batch:  # ... and for up to spec_batch greedy requests at once (``_spec_run``; the runner clamps it too)
            runner.spec_batch = int(spec_batch)
        self.spec = runner.spec
        self.name = name or self.spec.name
        self.tok = tokenizer or tokenizer_for(self.spec)
        tok_eos = [e for e in getattr(self.tok, "eos_ids", ()) if 0 <= e < self.spec.vocab_size]
        if tok_eos and sorted(tok_eos) != sorted(runner.eos_list):
            runner.set_eos(sorted(set(tok_eos) | set(e for e in runner.eos_list if e >= 0)))
        # kv_reserve_tokens: generated tokens reserved at admission (< 0: prompt + max_new up front, no growth)
        # prefix_cache: KV blocks of full prompt blocks stay cached after their request and are shared with later
        # requests whose prompt starts with the same tokens (runtime_core.h: the index, its safety invariant and the
        # eviction rule).  Off by default; block ids, launches and statistics are then what they are without it.
        self.prefix_cache = bool(prefix_cache)
        if self.prefix_cache:  # a row finished by its prefill token must not rewrite a published block (runner.py)
            runner.park_past_prompt = True
        cow = {} if prefix_cow_min_tokens is None else {"cow_min_tokens": int(prefix_cow_min_tokens)}
        self.sched = native.Scheduler(runner.num_kv_blocks, BLOCK, runner.max_slots, max_prefill_tokens,
                                      runner.max_blocks, kv_reserve_tokens, prefix_cache=self.prefix_cache, **cow)
        # set by a preemption: no admissions while requests run and fewer than _admit_hold_blocks KV blocks are free
        # (the preempted request's re-admission plus one block of growth per running request), so the preempted
        # request is not re-admitted at once and evicted again by the same growth
        self._admit_hold = False
        self._admit_hold_blocks = 0
        self.sync_every = sync_every
        # decode steps per iteration when every running request ignores EOS: None = run to the first
        # length limit (offline batches); a server sets a bound so new arrivals are admitted promptly
        self.run_ahead: Optional[int] = None
        self.max_prefill_tokens = max_prefill_tokens
        # chunked-prefill interleave (serving): at most this many prompt tokens are prefilled per engine
        # iteration, so a long prompt (a 2k-token Spark error for /explain_error) is spread over several
        # iterations with decode runs of the already-running requests in between instead of stalling them
        # for its whole prefill.  None = prefill every admitted prompt at once (offline batches, bench.py).
        self.prefill_chunk = prefill_chunk
        self._prefilling: list = []  # admitted requests whose prompt is not fully in the KV cache yet
        self._ids = itertools.count(1)
        self._reqs: dict[int, Request] = {}
        self._lock = threading.RLock()
        self._slot_owner: dict[int, int] = {}
        self.load_time_s = 0.0
        self.stats = {"requests": 0, "prompt_tokens": 0, "generated_tokens": 0, "decode_steps": 0,
                      "prefill_s": 0.0, "decode_s": 0.0, "decode_device_s": 0.0, "aborted": 0, "preempted": 0,
                      "kv_grown_blocks": 0, "peak_running": 0, "spec_steps": 0, "spec_drafted": 0, "spec_accepted": 0,
                      # prefix cache: admissions that looked the prompt up, those that found something, and the
                      # prompt tokens not prefilled because of it (prompt_tokens counts the tokens that were)
                      "prefix_queries": 0, "prefix_hits": 0, "prefix_cached_tokens": 0}
        self._spec_seen = (0, 0, 0)  # runner.spec_counts() as of the last decode run
        self._spec_rows_seen: list = []  # runner.spec_row_counts() as of the last decode run over several sequences
        # the largest number of requests a run of verify steps may serve (the runner's clamped spec_batch; 1 = off)
        self.spec_batch = runner.spec_s() if getattr(runner, "spec_tokens", 0) > 0 else 1
        # regex-constrained decoding (SamplingParams.regex): the tokenizer's byte table goes to the device once and the
        # runner allocates its per-slot DFA tables; off (the default) nothing is allocated, launched or counted
        self.guided = bool(guided) or bool(getattr(runner, "guided", False))
        self._tok_bytes = None
        if self.guided:
            off, blob = token_bytes(self.tok, self.spec.vocab_size)
            self._tok_bytes = (off.tolist(), blob.tobytes())
            if not getattr(runner, "guided", False):
                runner.enable_guided(off, blob)
            self.stats.update(guided_requests=0, guided_steps=0)
        # per-token logprobs (SamplingParams.logprobs): the runner allocates its per-slot records and captures a variant
        # of each decode graph; off (the default) nothing is allocated, launched or counted
        self.logprobs = bool(logprobs) or bool(getattr(runner, "logprobs", False))
        self._lp_pieces: dict = {}  # token id -> (decoded piece, its bytes)
        if self.logprobs:
            if not getattr(runner, "logprobs", False):
                runner.enable_logprobs()
            self.stats.update(logprob_requests=0, logprob_steps=0, prompt_logprob_requests=0, prompt_logprob_rows=0)
        self._plp_live = 0  # live requests that asked for prompt-token logprobs: 0 = every prefill call is today's
        # embeddings (SamplingParams.embed): the runner allocates its per-slot accumulators; off (the default) nothing
        # is allocated, launched or counted.  Under tensor parallelism the flag is kept and every request refused
        self.embeddings = bool(embeddings) or bool(getattr(runner, "embeddings", False))
        if self.embeddings:
            if self.embeddings_supported and not getattr(runner, "embeddings", False):
                runner.enable_embeddings()
            self.stats.update(embed_requests=0, embed_tokens=0)
        self._emb_live = 0  # live embedding requests: 0 = every prefill call is today's
        # context shift (SamplingParams.shift): a request that fills its window drops half of its context and goes on
        # (``_shift_contexts``).  The flag is inert -- requests end at the window -- under tensor parallelism, and on the
        # fp8 KV cache unless ``context_shift_fp8`` opts in as well (ops.kv_shift8 then quantises every surviving key
        # again, once per shift); off (the default) nothing is launched or counted
        tp = getattr(runner, "tp", None)
        fp8 = getattr(runner, "kv_scale", None) is not None
        self.context_shift_fp8 = bool(context_shift) and bool(context_shift_fp8) and fp8 and \
            (tp is None or tp.size == 1)
        self.context_shift = bool(context_shift) and (not fp8 or self.context_shift_fp8) and \
            (tp is None or tp.size == 1)
        if self.context_shift:
            self.stats.update(context_shifts=0, context_shift_tokens=0)
        # per-decode-run device timing (hipEvents around the graph replays, read after the host sync the
        # run ends with anyway): lsa_decode_step_device_seconds{model} = GPU time per token step
        self.device_timing = runner.on_gpu

    # -------------------------------------------------------------------------------- prompts
    def render(self, prompt: str, system: str = "", raw: bool = False) -> str:
        return prompt if raw else render(self.spec.template, prompt, system)

    @staticmethod
    def fit_context(ids: Sequence[int], num_ctx: int, num_keep: int = 4) -> list[int]:
        """Ollama's ``num_ctx`` window: a prompt of more than num_ctx - 1 tokens keeps its
        first ``num_keep`` tokens (BOS + template head) and its tail, dropping the middle, so at least one
        token can be generated.  Generation then stops at the window (``add_request`` caps max_tokens) --
        unless the engine runs context shift (``context_shift=True``): an eligible request then drops half of the
        context past its first ``num_keep`` tokens and goes on, as Ollama does (``_shift_contexts``)."""
        limit = max(1, int(num_ctx) - 1)
        ids = list(ids)
        if len(ids) <= limit:
            return ids
        keep = max(0, min(int(num_keep), limit - 1))
        return ids[:keep] + ids[len(ids) - (limit - keep):]

    def encode(self, text: str) -> list[int]:
        ids = self.tok.encode(text, add_bos=True)
        limit = self.runner.max_model_len - 1
        return ids[-limit:] if len(ids) > limit else ids

    # -------------------------------------------------------------------------------- request API
    def add_request(self, prompt_ids: Sequence[int], params: SamplingParams, stream: bool = False) -> Request:
        window = self.runner.max_model_len if params.num_ctx is None else min(self.runner.max_model_len,
                                                                               int(params.num_ctx))
        room = window - len(prompt_ids)
        if room < 1:
            raise ValueError("prompt longer than the model context")
        if not isinstance(params.shift, bool):
            raise SamplingOptionError("shift must be a boolean")
        # context shift: an eligible request is not capped by the room -- it shifts when it fills the window; the
        # scheduler is told a max_new inside the window, the device ``limit`` carries the real budget
        shift_w = window if (self.context_shift and params.shift and window >= 128) else 0
        budget = min(params.max_tokens, self.runner.max_new_cap) if shift_w else \
            min(params.max_tokens, room, self.runner.max_new_cap)
        p = dataclasses.replace(params, max_tokens=max(1, budget))
        sched_new = min(p.max_tokens, room)
        for name in ("presence_penalty", "frequency_penalty", "min_p"):  # refused here, like a bad pattern below
            if not math.isfinite(float(getattr(p, name))):
                raise SamplingOptionError(f"{name} must be a finite number")
        if not 0.0 <= float(p.min_p) <= 1.0:
            raise SamplingOptionError("min_p must lie in [0, 1]")
        if not isinstance(p.top_logprobs, int) or isinstance(p.top_logprobs, bool) or not 0 <= p.top_logprobs <= 20:
            raise SamplingOptionError("top_logprobs must be an integer in 0 .. 20")
        if p.top_logprobs and not (p.logprobs or p.prompt_logprobs):
            raise SamplingOptionError("top_logprobs needs logprobs: true (or prompt_logprobs: true)")
        if (p.logprobs or p.prompt_logprobs) and not self.logprobs:
            raise SamplingOptionError("this engine was built without per-token logprobs (logprobs=True / "
                                      "LSA_LOGPROBS=1 enables it)")
        if (isinstance(p.prompt_logprobs_from, bool) or not isinstance(p.prompt_logprobs_from, int)
                or p.prompt_logprobs_from < 0):
            raise SamplingOptionError("prompt_logprobs_from must be a non-negative integer")
        if p.prompt_logprobs and not self.prompt_logprobs_supported:
            raise SamplingOptionError("prompt_logprobs is not served under tensor parallelism (the sequence-parallel "
                                      "prefill keeps a share of the rows per rank)")
        if p.embed is not None:
            if p.embed not in ("mean", "last"):
                raise SamplingOptionError('pooling must be "mean" or "last"')
            if not self.embeddings:
                raise SamplingOptionError("this engine was built without embeddings (embeddings=True / "
                                          "LSA_EMBEDDINGS=1 enables it)")
            if not self.embeddings_supported:
                raise SamplingOptionError("embeddings are not served under tensor parallelism (the sequence-parallel "
                                          "prefill keeps a share of the rows per rank)")
            if len(prompt_ids) < 2:
                raise SamplingOptionError("an embedding input needs at least one token besides BOS")
            # an ordinary request of one greedy token, which is discarded: no stop, logprobs, regex, stream or shift
            p = dataclasses.replace(p, max_tokens=1, temperature=0.0, repeat_penalty=1.0, presence_penalty=0.0,
                                    frequency_penalty=0.0, stop=(), regex=None, logprobs=False, top_logprobs=0,
                                    prompt_logprobs=False, shift=False, speculate=False)
            stream, shift_w, sched_new = False, 0, 1
        dfa = None
        if p.regex is not None:  # compiled here, so that a bad pattern fails the request, not the engine loop
            if not self.guided:
                raise GuidedRequestError("this engine was built without regex-constrained decoding (guided=True / "
                                         "LSA_GUIDED=1 enables it)")
            if p.ignore_eos:
                raise GuidedRequestError("regex cannot be combined with ignore_eos: a constrained request ends by EOS")
            dfa = compile_regex(p.regex)
        req = Request(next(self._ids), list(map(int, prompt_ids)), p, time.perf_counter(),
                      stream=queue.Queue() if stream else None, dfa=dfa, shift_w=shift_w)
        if p.logprobs:
            self.stats["logprob_requests"] += 1
        match_limit = -1
        if p.prompt_logprobs:
            self.stats["prompt_logprob_requests"] += 1
            req.prompt_lp = [None] * len(req.prompt_ids)
            req.plp_next = max(1, p.prompt_logprobs_from)
            match_limit = self._plp_match_limit(req)
        if p.embed is not None:
            self.stats["embed_requests"] += 1
            self.stats["embed_tokens"] += len(req.prompt_ids)
            REGISTRY.inc("lsa_embed_requests_total", 1, "embedding inputs", model=self.name)
            REGISTRY.inc("lsa_embed_tokens_total", len(req.prompt_ids), "tokens of embedding inputs", model=self.name)
            if p.embed == "mean":  # every row must be computed, not found in the cache
                match_limit = 0
        if dfa is not None:
            self.stats["guided_requests"] += 1
            REGISTRY.inc("lsa_guided_requests_total", 1, "requests with a regex constraint", model=self.name)
        with self._lock:
            if self.prefix_cache and match_limit >= 0:  # the scored rows must be computed, not found in the cache
                self.sched.add(req.rid, len(req.prompt_ids), sched_new, req.prompt_ids, bool(p.cache_prompt),
                               match_limit)
            elif self.prefix_cache:
                self.sched.add(req.rid, len(req.prompt_ids), sched_new, req.prompt_ids, bool(p.cache_prompt))
            else:
                self.sched.add(req.rid, len(req.prompt_ids), sched_new)
            self._reqs[req.rid] = req
            if p.prompt_logprobs:
                self._plp_live += 1
            if p.embed is not None:
                self._emb_live += 1
        return req

    def add_requests(self, prompts: Sequence[Sequence[int]], params: SamplingParams) -> list:
        """``add_request`` for several prompts under one hold of the engine's lock: a loop thread stepping the engine
        meanwhile admits them together (one packed prefill, one shared prefix), not the first one alone.  All or none:
        if a prompt is refused, the ones queued before it are withdrawn and the refusal is raised."""
        with self._lock:
            reqs = []
            try:
                for ids in prompts:
                    reqs.append(self.add_request(ids, params))
            except Exception:
                for q in reqs:  # still waiting: nothing was admitted while the lock was held
                    self.sched.finish(q.rid)
                    self._reqs.pop(q.rid, None)
                    if q.params.prompt_logprobs:
                        self._plp_live -= 1
                    if q.params.embed is not None:
                        self._emb_live -= 1
                raise
            return reqs

    @property
    def prompt_logprobs_supported(self) -> bool:
        """Prompt-token logprobs are served: the engine runs per-token logprobs and is not tensor-parallel."""
        tp = getattr(self.runner, "tp", None)
        return bool(self.logprobs) and (tp is None or tp.size == 1)

    @property
    def embeddings_supported(self) -> bool:
        """Embeddings are served: the engine was built with them and is not tensor-parallel."""
        tp = getattr(self.runner, "tp", None)
        return bool(self.embeddings) and (tp is None or tp.size == 1)

    def _plp_match_limit(self, q: Request) -> int:
        """Leading tokens of ``q``'s (resumed) prompt that may come from the prefix cache: the row of position
        plp_next - 1 is the first that must be computed; -1 = today's rule, once every prompt index is scored."""
        if q.plp_next >= len(q.prompt_ids):
            return -1
        return min(len(q.ctx_ids) - 1, max(0, q.plp_next - 1))

    def has_work(self) -> bool:
        return self.sched.num_waiting > 0 or self.sched.num_running > 0 or bool(self._prefilling)

    def step(self) -> list[Request]:
        """One engine iteration: admit + prefill new requests (at most ``prefill_chunk`` prompt tokens when
        set), run decode steps over the requests whose prompt is complete, retire finished ones."""
        r = self.runner
        with self._lock:
            # after a preemption, admit nothing while requests still run: the preempted one would otherwise be
            # re-admitted at once and evicted again by the same growth
            if self._admit_hold and (self.sched.num_running == 0 or self.sched.free_blocks >= self._admit_hold_blocks):
                self._admit_hold = False
            admitted = [] if self._admit_hold else self.sched.admit()
            self.stats["peak_running"] = max(self.stats["peak_running"], self.sched.num_running)
            t0 = time.perf_counter()
            entries = []
            for rid in admitted:
                req = self._reqs[rid]
                slot = self.sched.slot(rid)
                req.slot = slot
                req.admitted = req.admitted or t0
                self._slot_owner[slot] = rid
                sp = req.params
                if self.prefix_cache and sp.cache_prompt:
                    # the prefill starts past the cached tokens (they are not charged to prefill_chunk either); the
                    # full prompt still goes to set_slots for the drafter's history and the repetition-penalty ring
                    req.prefilled = hit = self.sched.cached_tokens(rid)
                    req.cached_tokens += hit
                    self.stats["prefix_queries"] += 1
                    self.stats["prefix_hits"] += 1 if hit else 0
                    self.stats["prefix_cached_tokens"] += hit
                    REGISTRY.inc("lsa_prefix_cache_queries_total", 1, "admissions that looked the prompt up in the "
                                 "prefix cache", model=self.name)
                    REGISTRY.inc("lsa_prefix_cache_hits_total", 1 if hit else 0, "admissions that reused cached KV "
                                 "blocks", model=self.name)
                    REGISTRY.inc("lsa_prefix_cached_tokens_total", hit, "prompt tokens served from the prefix cache",
                                 model=self.name)
                # a re-admitted (preempted) request continues its random stream where it stopped: the sampler draws
                # token g from the stream keyed by the seed at counter g + offset (ops/reference.py device_uniform,
                # sampling.hip), and this incarnation's g restarts at 0 after len(resumed) tokens
                seed = pack_seed(sp.seed if sp.seed is not None else (rid * 7919 + 17), len(req.resumed))
                entries.append(dict(slot=slot, blocks=self.sched.block_table(rid), limit=sp.max_tokens,
                                    temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, seed=seed,
                                    eos_on=not sp.ignore_eos, repeat_penalty=sp.repeat_penalty,
                                    repeat_last_n=sp.repeat_last_n, presence_penalty=sp.presence_penalty,
                                    frequency_penalty=sp.frequency_penalty, min_p=sp.min_p, prompt_ids=req.kept_ids,
                                    defer_table=self.prefill_chunk is not None))
                if sp.logprobs:  # the row records (runner.enable_logprobs): lp_k = its top_logprobs K
                    entries[-1].update(lp_k=int(sp.top_logprobs))
                    req.lp_read = 0  # the device record indices restart with the incarnation
                if req.dfa is not None:  # a re-admitted request resumes in the state its generated tokens reached
                    entries[-1].update(dfa=req.dfa, dfa_state=req.dfa.walk(req.dfa.start, self._bytes_of(req.resumed)))
                self._prefilling.append(req)
            r.set_slots(entries)  # one batched host -> device transfer for every admitted request
            if self.prefix_cache and admitted:
                # forks of partly matching cached blocks: one launch, ahead of the prefills on the same stream; the
                # sources stay pinned in the scheduler until the copy is enqueued
                copies = self.sched.take_copies()
                if copies:
                    r.copy_kv_blocks(copies)
                self.sched.copies_done()
            if self._prefilling:
                done_now = self._prefill_some()
                t1 = time.perf_counter()
                for q in done_now:
                    q.first_token = q.first_token or t1
                    q.gen_host = 1
                    if q.stream is not None:  # the prefill's token goes out now (one sync, streaming only)
                        q.streamed = len(q.resumed) + 1
                        if q.params.logprobs:  # its record too, ahead of the chunk that carries the token
                            self._read_logprobs([q], [1])
                        q.stream.put(("tokens", q.resumed + r.tokens_of(q.slot, 1)))
                self.stats["prefill_s"] += t1 - t0
            pending = {q.rid for q in self._prefilling}
            running = [rid for rid in self.sched.running() if rid not in pending]
            if not running:
                return []
            sample = any(self._reqs[rid].params.needs_sampler for rid in running)
            guided = self.guided and any(self._reqs[rid].dfa is not None for rid in running)
            # the logprob graph variant exactly while a running request asked; such a request speculates only with
            # the runner's ``spec_logprobs`` (the verify graph with the two logprob launches)
            lp = self.logprobs and any(self._reqs[rid].params.logprobs for rid in running)
            lp_spec = not lp or bool(getattr(r, "spec_logprobs", False))
            # steps until the earliest request can hit its length limit; with EOS possible, at most
            # sync_every steps between host checks
            reqs = [self._reqs[rid] for rid in running]
            if self.context_shift:  # requests that filled their window drop half of their context, in one launch
                self._shift_contexts(reqs)
            remaining = min(q.params.max_tokens - q.gen_host for q in reqs)
            if remaining <= 0:
                n_steps = 0  # a request finished with its prefill token (max_tokens 1): retire it first
            elif all(q.params.ignore_eos for q in reqs):
                n_steps = remaining if self.run_ahead is None else min(self.run_ahead, remaining)
            else:
                n_steps = min(self.sync_every, remaining)
            if self.context_shift and n_steps:  # no run takes an eligible row past its window: it shifts there first
                n_steps = min([n_steps] + [q.shift_w - q.base - q.gen_host for q in reqs if q.shift_w])
            spec_T = self._spec_run(reqs, n_steps, remaining) if (n_steps and lp_spec) else 0
            if spec_T:  # verify steps: each commits 1 .. spec_T tokens, so fewer cover the same budget
                n_steps = min(n_steps, -(-remaining // spec_T))
            elif n_steps:
                reqs = self._grow_kv(reqs, n_steps)  # lazy KV: grow the tables for this run, preempting if needed
                running = [q.rid for q in reqs]
                if not reqs:
                    return []
            B = r.bucket(self.sched.highest_slot + 1)
            # host-side bound on every row's context during the run (selects the decode graph's split plan)
            spec_S = r.bucket(self.sched.highest_slot + 1) if (spec_T and len(reqs) > 1) else 1
            if spec_T:
                max_ctx = max(q.base + q.gen_host for q in reqs) + n_steps * spec_T + spec_T
            else:
                max_ctx = max(q.base + min(q.gen_host + n_steps, q.params.max_tokens) for q in reqs) + 1
        # the decode run needs no scheduler state: new requests may be added meanwhile
        t0 = time.perf_counter()
        ev = None
        if n_steps:
            if self.device_timing:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            # verify steps of a run in which a request asked: the "lp" verify graph (spec_logprobs); a run in which
            # nobody asked keeps today's verify graphs and their call
            lpk = dict(logprobs=True) if (lp and spec_T) else {}
            if spec_T and spec_S > 1 and guided:  # spec_batch_guided: the mask of every constrained sequence's rows,
                # only while a running request is constrained (then the sampled commit, if one needs the sampler)
                r.decode_spec(n_steps, max_ctx=max_ctx, guided=True, sample=sample, S=spec_S, **lpk)
            elif spec_T and spec_S > 1 and sample:  # spec_batch_sampled: the sampled commit over the spec_S sequences
                r.decode_spec(n_steps, max_ctx=max_ctx, sample=True, S=spec_S, **lpk)
            elif spec_T and spec_S > 1:  # spec_batch: greedy, unconstrained verify steps over slots 0 .. spec_S - 1
                r.decode_spec(n_steps, max_ctx=max_ctx, S=spec_S, **lpk)
            elif spec_T:
                if sample:  # spec_sampled: the verify graph that ends in the sampled commit (masked too, if guided)
                    r.decode_spec(n_steps, max_ctx=max_ctx, guided=guided, sample=True, **lpk)
                elif guided:  # spec_guided: the verify graph with the mask of the T verify rows
                    r.decode_spec(n_steps, max_ctx=max_ctx, guided=True, **lpk)
                else:
                    r.decode_spec(n_steps, max_ctx=max_ctx, **lpk)
            elif lp:  # the variant with the two logprob launches (masked too, if a row is constrained)
                r.decode(B, n_steps, sample, max_ctx=max_ctx, guided=guided, logprobs=True)
            else:
                if guided:  # the graph variant with the mask launch, only while a running row is constrained
                    r.decode(B, n_steps, sample, max_ctx=max_ctx, guided=True)
                else:
                    r.decode(B, n_steps, sample, max_ctx=max_ctx)
            if ev is not None:
                ev[1].record()
        fin, gl, _ = r.read_rows([q.slot for q in reqs])
        with self._lock:
            self.stats["decode_s"] += time.perf_counter() - t0
            self.stats["decode_steps"] += n_steps
            if guided and n_steps:  # plain masked steps and (spec_guided, spec_batch_guided) masked verify steps
                self.stats["guided_steps"] += n_steps
                REGISTRY.inc("lsa_guided_steps_total", n_steps, "decode steps run with the regex mask", model=self.name)
            if spec_T and n_steps:
                self._spec_account(reqs)
            if lp:  # the records of this sync's new tokens (up to T per verify step), for the rows that asked, in one
                # transfer; logprob_steps counts plain and verify steps alike
                self.stats["logprob_steps"] += n_steps
                asked = [(q, min(int(gl[i]), q.params.max_tokens)) for i, q in enumerate(reqs) if q.params.logprobs]
                self._read_logprobs([q for q, _ in asked], [n for _, n in asked])
            if self._plp_live:  # prompt records of the requests whose first token this sync made host-visible
                self._read_prompt_logprobs(reqs)
            if ev is not None:
                dev_s = ev[0].elapsed_time(ev[1]) / 1e3  # both recorded before read_rows' sync
                self.stats["decode_device_s"] += dev_s
                REGISTRY.observe("lsa_decode_step_device_seconds", dev_s / n_steps, "GPU time per decode step",
                                 buckets=TOKEN_BUCKETS, model=self.name, batch=str(B))
            done = []
            now = time.perf_counter()
            # generated tokens of every finished row in one device -> host transfer
            fin_rows = [(self._reqs[rid].slot, min(int(gl[i]), self._reqs[rid].params.max_tokens))
                        for i, rid in enumerate(running) if int(fin[i])]
            fin_toks = dict(zip([s for s, _ in fin_rows], r.tokens_of_many([s for s, _ in fin_rows],
                                                                           [n for _, n in fin_rows])))
            if self._emb_live:  # the vectors of the finished embedding requests, before their slots are released
                emb = [self._reqs[rid] for i, rid in enumerate(running)
                       if int(fin[i]) and self._reqs[rid].params.embed is not None]
                if emb:
                    for q, vec in zip(emb, r.embeddings_of([q.slot for q in emb])):
                        q.embedding = vec
            for i, rid in enumerate(running):
                self._reqs[rid].gen_host = int(gl[i])
                q = self._reqs[rid]
                if q.stream is not None and not int(fin[i]):
                    n = min(int(gl[i]), q.params.max_tokens)
                    if len(q.resumed) + n > q.streamed:  # the rows are host-visible after read_rows' sync
                        q.streamed = len(q.resumed) + n
                        q.stream.put(("tokens", q.resumed + r.tokens_of(q.slot, n)))
                if int(fin[i]):
                    req = self._reqs.pop(rid)
                    if req.params.prompt_logprobs:
                        self._plp_live -= 1
                    if req.params.embed is not None:
                        self._emb_live -= 1
                    req.output_ids = req.resumed + fin_toks[req.slot]
                    n = len(req.output_ids)
                    self._admit_hold = False
                    req.finished_at = now
                    r.release_slot(req.slot)
                    self._slot_owner.pop(req.slot, None)
                    self.sched.finish(rid)
                    self.stats["generated_tokens"] += n
                    self.stats["requests"] += 1
                    self._trace_done(req, n)
                    req.done.set()
                    if req.stream is not None:
                        req.stream.put(("done", None))
                    done.append(req)
            return done

    def _shift_contexts(self, reqs: list) -> None:
        """Context shift, at a run boundary (the host knows every row's generated count): every unfinished eligible
        request whose context c = base + gen_host has reached its window W keeps its first
        keep = min(num_keep, prompt length, W - 128) tokens and drops the d = 64 * ((c - keep) // 128) after them --
        llama.cpp's half of the rest, in whole 64-token blocks, so the survivors keep their rows and move down d / 64
        table entries, their keys rotated by -d.  The scheduler plans the block moves (``Scheduler.shift``); all
        requests shifting now go into one kernel launch, followed on the same stream by the new table rows and
        positions (``ModelRunner.shift_slots``), so the next decode run reads the shifted state.  What counts
        generated tokens (gen_len, out_tokens, limit, seeds, DFA state, logprob records) does not change, nor does
        the penalty ring (indexed by position % 64).  A request that has shifted takes plain steps from then on (the
        drafter's context is not compacted).  When the arena cannot supply the fresh blocks of a shared tail, the
        request ends at the window, as it would without the feature."""
        entries = []
        for q in reqs:
            c = q.base + q.gen_host
            if not q.shift_w or c < q.shift_w or q.gen_host >= q.params.max_tokens:
                continue
            keep = max(0, min(int(q.params.num_keep), len(q.prompt_ids), q.shift_w - 128))
            d = BLOCK * ((c - keep) // (2 * BLOCK))
            plan = self.sched.shift(q.rid, keep, d)
            if plan is None:  # end it here: the budget becomes what it has generated, the row is marked finished
                q.params = dataclasses.replace(q.params, max_tokens=q.gen_host)
                q.shift_w = 0
                self.runner.end_slot(q.slot)
                continue
            moves, table = plan
            entries.append((q.slot, moves, table, d))
            q.shifted += d
            q.drops.append((keep, d))
            q.spec_off = True
            self.stats["context_shifts"] += 1
            self.stats["context_shift_tokens"] += d
            REGISTRY.inc("lsa_context_shifts_total", 1, "context shifts at the num_ctx window", model=self.name)
            REGISTRY.inc("lsa_context_shift_tokens_total", d, "tokens dropped by context shifts", model=self.name)
        if entries:
            self.runner.shift_slots(entries)
        self.sched.shift_done()

    def _grow_kv(self, reqs: list, n_steps: int) -> list:
        """Lazy KV reservation: before a decode run of ``n_steps`` every running request must own the blocks of
        every cache position the run writes (the context after the run, less the last generated token, which is
        never written).  Requests grow oldest admission first; when the arena runs dry the youngest running
        request is preempted (possibly the one growing).  Returns the requests that stay in the run; the device
        block tables of the grown ones are updated in one batched transfer."""
        need = {q.rid: q.base + min(q.gen_host - 1 + n_steps, q.params.max_tokens - 1) for q in reqs}
        order = self.sched.youngest_first()
        alive = set(need)
        grown = {}
        for rid in reversed(order):  # oldest first
            if rid not in alive:
                continue
            while True:
                got = self.sched.grow(rid, need[rid])
                if got >= 0:
                    if got > 0:
                        grown[rid] = got
                    break
                victim = next(v for v in order if v in alive)
                self._preempt(self._reqs[victim])
                alive.discard(victim)
                grown.pop(victim, None)
                if victim == rid:
                    break
        if grown:
            self.stats["kv_grown_blocks"] += sum(grown.values())
            self.runner.extend_tables([(self._reqs[rid].slot, self.sched.block_table(rid)) for rid in grown])
        return [q for q in reqs if q.rid in alive]

    def _spec_run(self, reqs: list, n_steps: int, remaining: int) -> int:
        """Whether this decode run is a run of verify steps (speculative decoding): returns T = drafted tokens + 1, or
        0 for the plain run.  Verify steps need the runner's support (``ModelRunner.spec_supported``), exactly one
        running request, greedy (or, ``spec_sampled``, one that needs the sampler), in slot 0 (decode bucket 1), that
        has not opted out or been dropped by the acceptance guard; room for every position the run may write inside the model window; and the KV blocks of those
        positions without preempting anyone: the worst case is T committed tokens per step plus T - 1 rows of
        lookahead (also reserved so that a finished row, which rewrites its last T positions while the graph replays,
        stays in its own blocks).  A run in which a request asked for per-token logprobs is one only with the runner's
        ``spec_logprobs`` (``step`` does not ask otherwise: the plain verify graphs record none, which for ``spec_batch``
        is one more reason of the all-or-nothing rule); with it, every other condition here holds unchanged."""
        r = self.runner
        if not (getattr(r, "spec_tokens", 0) > 0 and r.spec_supported()):
            return 0
        if len(reqs) != 1:
            return self._spec_run_batch(reqs, n_steps, remaining)
        q = reqs[0]
        sp = q.params
        if q.slot != 0 or self.sched.highest_slot != 0 or self.sched.num_running != 1 or not sp.speculate or q.spec_off:
            return 0
        if sp.needs_sampler and not getattr(r, "spec_sampled", False):
            return 0  # a request that needs the sampler speculates only with the opt-in (the sampled verify graph)
        if q.dfa is not None and not (getattr(r, "spec_guided", False) and getattr(r, "guided", False)):
            return 0  # a constrained request speculates only with the opt-in (the guided verify graph)
        T = r.spec_k() + 1
        steps = min(n_steps, -(-remaining // T))
        if q.base + q.gen_host + steps * T + T > (q.shift_w or r.max_model_len):
            return 0
        got = self.sched.grow(q.rid, q.base + q.gen_host - 1 + steps * T + T - 1)
        if got < 0:
            return 0
        if got > 0:
            self.stats["kv_grown_blocks"] += got
            r.extend_tables([(q.slot, self.sched.block_table(q.rid))])
        return T

    def _spec_run_batch(self, reqs: list, n_steps: int, remaining: int) -> int:
        """``_spec_run`` for n = len(reqs) > 1 running requests (``spec_batch``): T when the run is a run of verify
        steps over the sequences of slots 0 .. S - 1, S = bucket(highest slot + 1) <= spec_batch, else 0.  All or
        nothing -- a limit, not an oversight: one request that cannot speculate makes the whole run plain, because a
        mixed run would need rows of two kinds in one graph.  Every condition must hold: the scheduler runs no other
        request and none is mid-prefill; every request has ``speculate`` on and has not been dropped by the acceptance
        guard; every request is unconstrained -- or, with ``spec_batch_guided``, ``spec_guided`` and a guided runner,
        any mix of constrained and unconstrained requests: the run then takes the guided verify graph exactly when at
        least one running request is constrained; every request is greedy -- or, with ``spec_batch_sampled`` and
        ``spec_sampled``, any mix of greedy requests and requests that need the sampler: the run then takes the
        sampled verify graph exactly when at least one running request needs the sampler (a greedy request in it is a
        sequence with temperature 0 and penalty 1), and the greedy batched graph otherwise; every request has window
        room for steps * T + T more positions; and
        ``sched.grow`` gives every request the blocks of those positions without preempting anyone (blocks grown before
        a later request fails stay with their requests: the plain run that follows needs them too).  Slots below S
        without a request are idle rows of the step (``ModelRunner._verify_step``)."""
        r = self.runner
        SB = r.spec_s()
        if SB < 2 or len(reqs) > SB or self.sched.num_running != len(reqs) or self._prefilling:
            return 0
        if r.bucket(self.sched.highest_slot + 1) > SB or any(not 0 <= q.slot < SB for q in reqs):
            return 0
        sampled_ok = getattr(r, "spec_batch_sampled", False) and getattr(r, "spec_sampled", False)
        guided_ok = getattr(r, "spec_batch_guided", False) and getattr(r, "spec_guided", False) and \
            getattr(r, "guided", False)
        if any((q.params.needs_sampler and not sampled_ok) or (q.dfa is not None and not guided_ok)
               or not q.params.speculate or q.spec_off for q in reqs):
            return 0
        T = r.spec_k() + 1
        if SB * T > 32:
            return 0
        steps = min(n_steps, -(-remaining // T))
        if any(q.base + q.gen_host + steps * T + T > (q.shift_w or r.max_model_len) for q in reqs):
            return 0
        grown, ok = [], True
        for q in reqs:
            got = self.sched.grow(q.rid, q.base + q.gen_host - 1 + steps * T + T - 1)
            if got < 0:
                ok = False
                break
            if got > 0:
                self.stats["kv_grown_blocks"] += got
                grown.append((q.slot, self.sched.block_table(q.rid)))
        if grown:
            r.extend_tables(grown)
        return T if ok else 0

    def _read_logprobs(self, reqs: list, ns: list) -> None:
        """Append device records [q.lp_read, n) of each request's slot row to ``q.logprobs`` (one transfer)."""
        sel = [(q, n) for q, n in zip(reqs, ns) if n > q.lp_read]
        if not sel:
            return
        recs = self.runner.logprobs_of_many([q.slot for q, _ in sel], [q.lp_read for q, _ in sel], [n for _, n in sel])
        for (q, n), rec in zip(sel, recs):
            q.logprobs.extend(rec)
            q.lp_read = n

    def _read_prompt_logprobs(self, reqs: list) -> None:
        """Move the pending device records of prompt tokens to ``q.prompt_lp`` (one transfer for all of ``reqs``)."""
        sel = [(q, pend) for q in reqs for pend in q.plp_pending]
        if not sel:
            return
        got = self.runner.prompt_logprobs_of([(rec, a, n, int(q.params.top_logprobs)) for q, (rec, a, n, _) in sel])
        for (q, (_, _, n, j0)), rows in zip(sel, got):
            q.prompt_lp[j0:j0 + n] = rows
        for q in reqs:
            q.plp_pending = []

    def _score_seg(self, slot: int, a: int, b: int):
        """The rows of a prefill segment (positions [a, b) of the request in ``slot``) that a prompt-logprob request
        still has to score: (request, (first row in the segment, K, targets)) or None.  The row of position p gives
        prompt index p + 1, so the rows are plp_next - 1 .. prompt length - 2, never a row of ``resumed`` tokens."""
        q = self._reqs.get(self._slot_owner.get(slot, -1))
        if q is None or not q.params.prompt_logprobs:
            return None
        lo, hi = max(a, q.plp_next - 1), min(b, len(q.prompt_ids) - 1)
        if hi <= lo:
            return None
        return q, (lo - a, int(q.params.top_logprobs), q.ctx_ids[lo + 1:hi + 1])

    def _embed_seg(self, slot: int, end: int):
        """The ``embed`` entry of a prefill segment that ends at position ``end`` of the request in ``slot``: None, or
        (pooling, the input's tokens, whether the segment holds its last row)."""
        q = self._reqs.get(self._slot_owner.get(slot, -1))
        if q is None or q.params.embed is None:
            return None
        total = len(q.kept_ids)
        return q.params.embed, total, end == total

    def _run_prefill(self, batch: list, commit: bool, any_sample: bool = False) -> None:
        """One runner prefill call.  While no live request asked for prompt logprobs it is today's call; else the
        segments' rows to score ride along and the call's device records are kept with their requests, unread."""
        r = self.runner
        segs = [self._score_seg(slot, p0, p0 + len(ids)) for slot, ids, p0 in batch] if self._plp_live else []
        embs = [self._embed_seg(slot, p0 + len(ids)) for slot, ids, p0 in batch] if self._emb_live else []
        ekw = dict(embed=embs) if any(embs) else {}  # nobody embeds: the call, arguments included, is today's
        if not any(segs):
            if commit:
                r.prefill(batch, any_sample, **ekw)
            else:
                r.prefill_chunk(batch, **ekw)
            return
        score = [sg[1] if sg else None for sg in segs]
        recs = r.prefill(batch, any_sample, score=score, **ekw) if commit else \
            r.prefill_chunk(batch, score=score, **ekw)
        for i, row0, rows in recs[3]:
            q = segs[i][0]
            q.plp_pending.append((recs[:3], row0, rows, q.plp_next))
            q.plp_next += rows
            self.stats["prompt_logprob_rows"] += rows
            REGISTRY.inc("lsa_prompt_logprob_tokens_total", rows, "prompt tokens scored (prompt_logprobs)",
                         model=self.name)

    def _lp_piece(self, tid: int) -> tuple:
        """(decoded piece, byte values) of a token id: the bytes come from the tokenizer's ``token_bytes`` table."""
        got = self._lp_pieces.get(tid)
        if got is None:
            if self._tok_bytes is None:
                off, blob = token_bytes(self.tok, self.spec.vocab_size)
                self._tok_bytes = (off.tolist(), blob.tobytes())
            off, blob = self._tok_bytes
            raw = blob[off[tid]:off[tid + 1]] if 0 <= tid < len(off) - 1 else b""
            got = self._lp_pieces[tid] = (self.tok.decode([tid]), list(raw))
        return got

    def prompt_logprob_entries(self, req: Request) -> list:
        """The response list of a request that asked for prompt logprobs: one entry per prompt token, None where no
        record is defined (index 0 and below prompt_logprobs_from)."""
        return [None if rec is None else self.logprob_entries(req, [tid], records=[rec])[0]
                for tid, rec in zip(req.prompt_ids, req.prompt_lp)]

    def logprob_entries(self, req: Request, token_ids: Sequence[int], start: int = 0,
                        records: Optional[list] = None) -> list:
        """The response entries of generated tokens ``token_ids`` = output tokens [start, start + len) of ``req``
        (``records``: of these records instead of the generated tokens')."""
        out = []
        src = req.logprobs if records is None else records
        for j, tid in enumerate(token_ids):
            lpv, top = src[start + j]
            piece, raw = self._lp_piece(int(tid))
            ent = {"token": piece, "logprob": float(lpv), "bytes": raw}
            if req.params.top_logprobs:
                ent["top_logprobs"] = [dict(zip(("token", "bytes"), self._lp_piece(int(i))), logprob=float(v))
                                       for i, v in top]
            out.append(ent)
        return out

    def _bytes_of(self, ids: Sequence[int]) -> bytes:
        """The bytes the token ids decode to (the table regex-constrained decoding walks on the device)."""
        off, blob = self._tok_bytes
        return b"".join(blob[off[t]:off[t + 1]] for t in ids if 0 <= t < len(off) - 1)

    def _spec_account(self, reqs: list) -> None:
        """Fold the runner's verify-step counters into the engine's and the requests'; apply the acceptance guard: a
        request whose accepted-per-step mean is below break-even after 16 verify steps takes plain steps from now on.
        A run over several sequences reads the per-row counters: row s belongs to the request in slot s."""
        rows = self.runner.spec_row_counts()
        seen = self._spec_rows_seen + [[0, 0, 0]] * (len(rows) - len(self._spec_rows_seen))
        self._spec_rows_seen = rows
        now = tuple(int(sum(c)) for c in zip(*rows))
        d = [a - b for a, b in zip(now, self._spec_seen)]
        self._spec_seen = now
        for key, v in zip(("spec_steps", "spec_drafted", "spec_accepted"), d):
            self.stats[key] += v
        REGISTRY.inc("lsa_spec_steps_total", d[0], "speculative-decoding verify steps", model=self.name)
        REGISTRY.inc("lsa_spec_drafted_tokens_total", d[1], "tokens drafted by the prompt-lookup drafter", model=self.name)
        REGISTRY.inc("lsa_spec_accepted_tokens_total", d[2], "drafted tokens accepted by verification", model=self.name)
        for q in reqs:
            ds = [a - b for a, b in zip(rows[q.slot], seen[q.slot])]
            q.spec_steps += ds[0]
            q.spec_accepted += ds[2]
            if q.spec_steps >= 16 and q.spec_accepted / q.spec_steps < self.runner.spec_min_accept:
                q.spec_off = True

    def _preempt(self, q: Request) -> None:
        """Release a running request's slot and KV blocks and re-queue it first; its generated tokens become part
        of the prompt it re-prefills (recompute), its budget shrinks by as many."""
        n = min(q.gen_host, q.params.max_tokens)
        toks = self.runner.tokens_of(q.slot, n) if n else []
        if q.params.logprobs:  # its unread records, before the slot goes: they stay with the request on the host
            self._read_logprobs([q], [n])
            q.lp_read = 0
        if q.plp_pending:  # the prompt records too; the re-admitted request scores only indices from plp_next on
            self._read_prompt_logprobs([q])
        if q in self._prefilling:  # not reached by the engine itself: ``_grow_kv`` picks its victims among requests
            # whose prompt is complete.  A caller that preempts a request in the middle of its chunked prompt (the
            # tests do, to hold that such a request scores only the prompt indices it lacks) must not leave it there
            self._prefilling.remove(q)
        q.resumed = q.resumed + toks
        q.params = dataclasses.replace(q.params, max_tokens=q.params.max_tokens - n)
        self.runner.release_slot(q.slot)
        self._slot_owner.pop(q.slot, None)
        limit = self._plp_match_limit(q) if q.params.prompt_logprobs else -1
        if q.params.embed == "mean":  # the re-admitted request pools again from position 0: every row is computed
            limit = 0
        # a request that has shifted re-prefills the context as its cache held it (kept_ids; ctx_ids otherwise); an
        # eligible one tells the scheduler a max_new inside its window, as add_request does
        ids = q.kept_ids
        new = min(q.params.max_tokens, q.shift_w - len(ids)) if q.shift_w else q.params.max_tokens
        if self.prefix_cache and limit >= 0:  # prompt indices still to score: their rows must be computed again
            self.sched.preempt(q.rid, len(ids), new, ids, limit)
        elif self.prefix_cache:  # with its tokens, so that the resumed request can hit its own blocks if they survive
            self.sched.preempt(q.rid, len(ids), new, ids)
        else:
            self.sched.preempt(q.rid, len(ids), new)
        q.slot, q.gen_host, q.prefilled = -1, 0, 0
        q.preemptions += 1
        self.stats["preempted"] += 1
        reserve = self.sched.reserve_tokens
        gen = q.params.max_tokens if reserve < 0 else min(q.params.max_tokens, reserve)
        self._admit_hold = True
        self._admit_hold_blocks = -(-(q.base + gen) // BLOCK) + self.sched.num_running

    def _trace_done(self, req: Request, n: int) -> None:
        """Engine spans of a finished request (queue -> prefill -> decode), fed to lsa_stage_seconds and,
        with LSA_TRACE=1, to the JSONL trace (SURVEY.md §5 tracing)."""
        rid = f"{self.name}:{req.rid}"
        tracing.record("engine_queue", req.admitted - req.arrival, rid, model=self.name)
        tracing.record("engine_prefill", req.first_token - req.admitted, rid, model=self.name,
                       prompt_tokens=len(req.prompt_ids))
        tracing.record("engine_decode", req.finished_at - req.first_token, rid, model=self.name, tokens=n)

    def abort_all(self, reason: str) -> list:
        """Fail every queued and running request (engine recovery after a step raised): their callers are
        released with ``error`` set, slots and KV blocks are returned, the engine is empty again."""
        with self._lock:
            out = []
            now = time.perf_counter()
            for rid, req in list(self._reqs.items()):
                req.error = reason
                req.finished_at = now
                if req.slot >= 0:
                    try:
                        self.runner.release_slot(req.slot)
                    except Exception:  # noqa: BLE001 - a faulted device: the engine is rebuilt anyway
                        pass
                self.sched.finish(rid)
                req.done.set()
                if req.stream is not None:
                    req.stream.put(("done", None))
                out.append(req)
            if self.context_shift:
                self.sched.shift_done()
            if self.prefix_cache:  # the device state is suspect after a failed step: keep no KV from before it
                self.sched.copies_done()
                self.sched.reset_prefix_cache()
            self._reqs.clear()
            self._plp_live = 0
            self._emb_live = 0
            self._slot_owner.clear()
            self._prefilling.clear()
            self.stats["aborted"] += len(out)
            return out

    def _prefill_some(self) -> list:
        """Prefill the admitted-but-incomplete prompts FCFS within this iteration's token budget; returns the
        requests whose prompt completed (their first token is committed)."""
        budget = self.prefill_chunk if self.prefill_chunk else None
        final, partial, done = [], [], []
        any_sample = False
        for q in list(self._prefilling):
            ids = q.kept_ids
            rest = len(ids) - q.prefilled
            take = rest if budget is None else min(rest, budget)
            if take <= 0:
                break
            seg = (q.slot, ids[q.prefilled:q.prefilled + take], q.prefilled)
            q.prefilled += take
            if q.prefilled == len(ids):
                final.append(seg)
                done.append(q)
                any_sample |= q.params.needs_sampler
                self._prefilling.remove(q)
            else:
                partial.append(seg)
            self.stats["prompt_tokens"] += take
            if budget is not None:
                budget -= take
                if budget <= 0:
                    break
        if partial:  # KV only (no token commit); chunks of different requests pack into one launch sequence
            self._run_prefill(partial, False)
        if final:
            self._prefill_packed(final, any_sample)
        if self.prefix_cache:  # the prompt's last chunk is launched: its full blocks may be shared from now on
            for q in done:
                self.sched.publish(q.rid)
        return done

    def _prefill_packed(self, seqs, any_sample: bool) -> None:
        """Prefill in chunks of at most max_prefill_tokens tokens (long prompts split across calls)."""
        batch, tokens = [], 0
        for slot, ids, p0 in seqs:
            if len(ids) > self.max_prefill_tokens:  # chunked prefill of one long prompt
                if batch:
                    self._run_prefill(batch, True, any_sample)
                    batch, tokens = [], 0
                c = self.max_prefill_tokens
                for s in range(0, len(ids) - c, c):
                    self._run_prefill([(slot, ids[s:s + c], p0 + s)], False)
                s = ((len(ids) - 1) // c) * c
                self._run_prefill([(slot, ids[s:], p0 + s)], True, any_sample)
                continue
            if tokens + len(ids) > self.max_prefill_tokens and batch:
                self._run_prefill(batch, True, any_sample)
                batch, tokens = [], 0
            batch.append((slot, ids, p0))
            tokens += len(ids)
        if batch:
            self._run_prefill(batch, True, any_sample)

    def run_until_done(self, reqs: Sequence[Request]) -> None:
        while not all(q.done.is_set() for q in reqs):
            self.step()

    # -------------------------------------------------------------------------------- one-shot API
    def result(self, req: Request, template: Optional[str] = None) -> GenerationResult:
        t0 = time.perf_counter()
        text = self.tok.decode(req.output_ids)
        text = apply_stops(text, template or self.spec.template, req.params.stop)
        tracing.record("engine_detok", time.perf_counter() - t0, f"{self.name}:{req.rid}", model=self.name)
        ns = lambda s: int(max(0.0, s) * 1e9)  # noqa: E731
        ended_eos = bool(req.output_ids) and req.output_ids[-1] in self.runner.eos_list and not req.params.ignore_eos
        return GenerationResult(
            text=text, token_ids=req.output_ids, prompt_tokens=len(req.prompt_ids), eval_count=len(req.output_ids),
            total_duration_ns=ns(req.finished_at - req.arrival), load_duration_ns=ns(self.load_time_s),
            prompt_eval_duration_ns=ns(req.first_token - req.admitted),
            eval_duration_ns=ns(req.finished_at - req.first_token), done_reason="stop" if ended_eos else "length",
            cached_prompt_tokens=req.cached_tokens, context_shifts=len(req.drops),
            logprobs=self.logprob_entries(req, req.output_ids) if req.params.logprobs else None,
            prompt_logprobs=self.prompt_logprob_entries(req) if req.params.prompt_logprobs else None,
            embedding=req.embedding.tolist() if req.embedding is not None else None)

    def text_of(self, token_ids: Sequence[int], req: Request) -> str:
        """The response text of ``token_ids`` exactly as ``result`` builds it (stop strings applied)."""
        return apply_stops(self.tok.decode(list(token_ids)), self.spec.template, req.params.stop)

    def stream_text(self, req: Request, timeout_s: Optional[float] = None) -> Iterator[str]:
        """Text pieces of a request added with ``stream=True``, one per host sync that revealed tokens.
        The pieces concatenate to ``result(req).text``: a trailing incomplete UTF-8 sequence and any
        tail that could still grow into a stop string are held back until later tokens settle them, and
        nothing past a stop string is sent."""
        assert req.stream is not None, "add_request(..., stream=True)"
        stops = tuple(STOP_STRINGS.get(self.spec.template, ())) + tuple(req.params.stop)
        sent = 0
        while True:
            kind, toks = req.stream.get(timeout=timeout_s)
            if kind == "done":
                break
            req.stream_toks = toks
            raw = self.tok.decode(list(toks))
            text = self.text_of(toks, req)
            if len(text) < len(raw):  # a stop string appeared: only its prefix is ever sent
                safe = len(text)
            else:
                safe = len(text.rstrip("\ufffd"))
                hold = 0  # the longest tail that is a proper prefix of a stop string
                for st in stops:
                    for k in range(min(len(st) - 1, safe), hold, -1):
                        if text[safe - k:safe] == st[:k]:
                            hold = k
                            break
                safe -= hold
            # one piece per snapshot, empty while no new text is settled (tokens that decode to nothing,
            # held-back tails): the client sees progress at every sync, as with Ollama's per-token chunks
            piece = text[sent:safe] if safe > sent else ""
            sent = max(sent, safe)
            yield piece
        if req.error:
            raise RuntimeError(req.error)
        final = self.result(req).text
        if len(final) > sent:
            yield final[sent:]

    def generate(self, prompts: Sequence, params: Optional[SamplingParams] = None, system: str = "",
                 raw: bool = False) -> list[GenerationResult]:
        """Batch generate. ``prompts``: strings (templated + tokenized) or token-id lists."""
        params = params or SamplingParams()
        reqs = []
        for p in prompts:
            ids = self.encode(self.render(p, system, raw)) if isinstance(p, str) else list(p)
            if params.num_ctx is not None:
                ids = self.fit_context(ids, params.num_ctx, params.num_keep)
            reqs.append(self.add_request(ids, params))
        self.run_until_done(reqs)
        return [self.result(q) for q in reqs]

    def generate_text(self, prompt: str, system: str = "", params: Optional[SamplingParams] = None,
                      on_token: Optional[Callable[[str], None]] = None) -> GenerationResult:
        res = self.generate([prompt], params, system)[0]
        if on_token is not None:
            on_token(res.text)
        return res
