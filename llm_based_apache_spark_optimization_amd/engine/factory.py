"""Build an LLMEngine for a named model (random-init, a safetensors checkpoint directory or a GGUF file)."""
from __future__ import annotations

import time
from typing import Optional

import torch

from ..models import get_spec, tokenizer_for
from ..models.gguf import is_gguf
from ..models.llama import init_random, load_gguf, load_safetensors_dir
from .engine import LLMEngine
from .runner import ModelRunner


def build_engine(model: str, device: Optional[str] = None, checkpoint: Optional[str] = None, dtype: str = "bf16",
                 max_slots: int = 32, max_model_len: int = 4096, seed: int = 0, tp=None,
                 use_graphs: bool = True, sync_every: int = 8, num_kv_blocks: Optional[int] = None,
                 max_prefill_tokens: int = 16384, kv_memory_fraction: float = 0.85,
                 warm_graphs: bool = False, prefill_chunk: Optional[int] = None,
                 kv_dtype: Optional[str] = None, max_new_cap: Optional[int] = None,
                 kv_reserve_tokens: int = 64, spec_tokens: int = 0, prefix_cache: bool = False,
                 prefix_cow_min_tokens: Optional[int] = None, spec_quantized: bool = False,
                 guided: bool = False, spec_guided: bool = False, spec_sampled: bool = False,
                 spec_batch: int = 1, spec_batch_sampled: bool = False,
                 spec_batch_guided: bool = False, logprobs: bool = False,
                 spec_logprobs: bool = False, context_shift: bool = False,
                 context_shift_fp8: bool = False, embeddings: bool = False) -> LLMEngine:
    """checkpoint: an HF directory (config.json + *.safetensors) or a GGUF file (recognised by its magic; Ollama blobs
    carry no extension).  dtype: "bf16" | "fp8" | "mxfp4" | "q4_0"; "q4_0" serves a GGUF file's own Q4_0 codes and scales
    (``models.llama.load_gguf`` has the rules), quantises by ggml's rule where there is no such file, runs at TP = 1
    only (else bf16, with a warning) and takes plain steps whatever ``spec_tokens`` says.
    kv_dtype: paged KV cache dtype, "bf16" | "fp8" (None: LSA_KV_FP8, default bf16).
    max_new_cap: generated-token cap per request (None: the context window).
    kv_reserve_tokens: generated tokens whose KV is reserved at admission (the rest grows lazily; < 0 reserves
    prompt + max_new up front).
    spec_tokens: tokens drafted per step by prompt-lookup speculative decoding for batch-1 greedy requests (0 = off).
    spec_quantized: speculate with fp8 / MXFP4 weights and the fp8 KV cache too (off: those engines take plain steps);
    their verify rows run the weight-only GEMMs, a different numerics class from a W8A8 / W4A8 plain batch-1 step.
    prefix_cache: keep the KV blocks of full prompt blocks after their request and share them with later requests
    whose prompt starts with the same tokens (off by default); prefix_cow_min_tokens: the shortest common prefix
    with a cached block that is worth forking it (None: the scheduler's default).
    guided: regex-constrained decoding for requests that carry ``SamplingParams.regex`` (off by default: such a
    request is then rejected); allocates the per-slot DFA tables and captures a guided variant of each decode graph.
    spec_guided: regex-constrained requests speculate too (off: they take plain guided steps); needs guided and
    spec_tokens, and is inert without either.
    spec_sampled: requests that need the sampler (temperature > 0 and / or a repetition penalty) speculate too (off:
    they take plain steps); their tokens are those of the plain sampled steps of the same seed.  Needs spec_tokens; a
    constrained sampled request speculates only with spec_guided as well.
    spec_batch: the largest number of running greedy, unconstrained requests (in slots below it) whose decode run may
    be a run of verify steps (1, the default: one request in slot 0 only); clamped to a power of two with
    spec_batch * (spec_tokens + 1) <= 32 and <= max_slots.  All or nothing: one running request that cannot speculate
    makes the run plain.
    spec_batch_sampled: requests that need the sampler may be among the requests of such a run (off: one of them makes
    the run plain).  The run then ends each verify step in the sampled commit over its sequences, where a greedy
    request is a sequence with temperature 0 and penalty 1; every request's tokens are those it generates alone.  An
    all-greedy run keeps the greedy batched graph.  Needs spec_tokens, spec_sampled and spec_batch > 1, and is inert
    without any of them.
    spec_batch_guided: regex-constrained requests may be among the requests of such a run (off: one of them makes the
    run plain).  The run then masks the verify rows of every constrained sequence in that sequence's own DFA states
    and leaves an unconstrained sequence untouched; every request's tokens are those of its plain (guided) steps.  An
    all-unconstrained run keeps the unguided batched graph.  Needs guided, spec_guided, spec_tokens and spec_batch > 1
    (a constrained request that needs the sampler: spec_sampled and spec_batch_sampled too), and is inert without any
    of them.
    logprobs: per-token log-probabilities for requests that carry ``SamplingParams.logprobs`` (off by default: such a
    request is then rejected); allocates the per-slot record buffers and captures a logprob variant of each decode
    graph, replayed only while a running request asked.
    spec_logprobs: a request that asked for logprobs speculates wherever one that did not ask would (off: it takes plain
    steps, and makes a spec_batch run plain); its records are the log-softmax of the raw verify rows.  Needs logprobs
    and spec_tokens, and is inert without either.
    context_shift: a request that fills its num_ctx window keeps its first num_keep tokens, drops half of the rest and
    goes on generating, as Ollama does (off by default: it ends at the window); ``SamplingParams.shift`` = False opts
    a request out.  Inert on the fp8 KV cache and under tensor parallelism.
    context_shift_fp8: with ``context_shift``, shift on the fp8 KV cache too: a surviving key is dequantised, rotated
    and quantised again with a new row scale, once per shift (``ops.kv_shift8``).  Inert without ``context_shift``, on
    the bf16 cache (which shifts anyway) and under tensor parallelism.
    embeddings: serve embedding requests (``SamplingParams.embed``, ``EngineService.embed``, POST /api/embed): the
    prefill pools the final-norm rows of such a request on the device (off by default: such a request is then
    rejected); allocates two [max_slots, hidden] f32 buffers.  Requests are refused under tensor parallelism."""
    if device is None:
        device = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cpu"
    t0 = time.perf_counter()
    tpr, tps = (tp.rank, tp.size) if tp is not None else (0, 1)
    if dtype == "q4_0" and tps > 1 and not (checkpoint and is_gguf(checkpoint)):
        import warnings

        warnings.warn(f"dtype q4_0 runs at tp = 1 only (tp = {tps}): loading as bf16")
        dtype = "bf16"
    if checkpoint and is_gguf(checkpoint):
        w = load_gguf(checkpoint, device, kind=dtype, name=model, tp_rank=tpr, tp_size=tps)
        tok = tokenizer_for(w.spec, checkpoint, (w.source or {}).get("tokenizer"))
    elif checkpoint:
        w = load_safetensors_dir(checkpoint, device, kind=dtype, name=model, tp_rank=tpr, tp_size=tps)
        tok = tokenizer_for(w.spec, checkpoint)
    else:
        spec = get_spec(model)
        w = init_random(spec, device, seed=seed, kind=dtype, tp_rank=tpr, tp_size=tps)
        tok = tokenizer_for(spec)
    runner = ModelRunner(w, max_slots=max_slots, max_model_len=max_model_len, tp=tp, use_graphs=use_graphs,
                         num_kv_blocks=num_kv_blocks, kv_memory_fraction=kv_memory_fraction, kv_dtype=kv_dtype,
                         max_new_cap=max_new_cap, spec_tokens=spec_tokens, spec_quantized=spec_quantized,
                         spec_guided=spec_guided, spec_sampled=spec_sampled, spec_batch=spec_batch,
                         spec_batch_sampled=spec_batch_sampled, spec_batch_guided=spec_batch_guided,
                         spec_logprobs=spec_logprobs)
    eng = LLMEngine(runner, tok, sync_every=sync_every, max_prefill_tokens=max_prefill_tokens, name=model,
                    prefill_chunk=prefill_chunk or None, kv_reserve_tokens=kv_reserve_tokens, spec_tokens=spec_tokens,
                    prefix_cache=prefix_cache, prefix_cow_min_tokens=prefix_cow_min_tokens, guided=guided,
                    logprobs=logprobs, context_shift=context_shift, context_shift_fp8=context_shift_fp8,
                    embeddings=embeddings)
    if torch.device(device).type == "cuda":
        if warm_graphs:
            runner.capture_all()
        torch.cuda.synchronize(device)
    eng.load_time_s = time.perf_counter() - t0
    return eng
