"""ModelRunner: one model replica (optionally one tensor-parallel shard of it) on one device.

Owns the packed weights, the paged KV cache, the RoPE tables, every decode workspace and the
device-resident decode state, and executes

* ``prefill(seqs)`` — packed variable-length prefill (eager launches; shapes change per call),
  which also commits each sequence's first generated token into its decode slot;
* ``decode(B, steps)`` — ``steps`` decode steps over slot rows ``[0, B)``, replayed from a captured
  hipGraph (``torch.cuda.CUDAGraph``) per (batch bucket, sampler mode).  The whole step — 32 layers of
  fused kernels, the TP all-reduces, LM head, token selection and the state update — runs without
  the host: positions, context lengths, finished flags and the generated tokens live on the device, so
  a graph replays for as many steps as the host wants between synchronisations.

Decode-step kernel sequence per layer (``L`` layers, B tokens):
  add_rmsnorm(+embedding | +down partials) -> gemm qkv -> rope_append (RoPE + paged KV write)
  -> attn_decode (split-KV) -> gemm o (f32 split-K slabs) [-> all_reduce] -> add_rmsnorm(+o partials)
  -> gemm gate_up (fused SiLU*up) -> gemm down (f32 slabs) [-> all_reduce]
then add_rmsnorm(final) -> gemm lm_head [-> all_gather] -> argmax/sample + commit.
"""
from __future__ import annotations


import math
import os
from typing import Optional, Sequence

import torch

from .. import ops
from ..models.llama import LlamaWeights
from ..ops import reference as ref

BLOCK = 64
REPEAT_WINDOW = 64  # repetition-penalty ring (Ollama repeat_last_n default; larger values are clamped)
# norm-free attention input in prefill (Runner._prefill_layers), off by default: measured even with the norm launch
# it removes (3B 2k TTFT 14.38 vs 14.34 ms, profiles/r5/prefill_norm_free_ab.txt)
# batch-1 decode with the residual add folded into the next GEMM's prologue (ModelRunner._decode_step_rr)
RR_DECODE = os.environ.get("LSA_RR", "1") != "0"
# largest decode bucket whose bf16 GEMMs read the 12-bit weight stream (ModelRunner.z12_max_batch; 0 = off)
Z12_MAX_BATCH = 32


class TPCommError(RuntimeError):
    """A TP peer missed a one-shot all-reduce (the kernel poisoned the result with NaN and set err)."""


class ModelRunner:
    def __init__(self, weights: LlamaWeights, max_slots: int = 32, max_model_len: int = 4096,
                 num_kv_blocks: Optional[int] = None, kv_memory_fraction: float = 0.85,
                 max_new_cap: Optional[int] = None, tp=None, use_graphs: bool = True,
                 fuse_rope: Optional[bool] = None, seq_parallel: Optional[bool] = None, sp_min_tokens: Optional[int] = None,
                 kv_dtype: Optional[str] = None, spec_tokens: int = 0, spec_ngram: tuple = (3, 1),
                 spec_quantized: bool = False, spec_guided: bool = False, spec_sampled: bool = False,
                 spec_batch: int = 1, spec_batch_sampled: bool = False, spec_batch_guided: bool = False,
                 spec_logprobs: bool = False):
        self.w = weights
        # prompt-lookup speculative decoding (``_verify_step``): tokens drafted per step (0 = off) and the drafter's
        # (longest, shortest) n-gram.  Plain attributes: an experiment may set them on a built runner.
        self.spec_tokens = int(spec_tokens)
        self.spec_ngram = tuple(spec_ngram)
        # opt-in: verify steps for fp8 / MXFP4 weights and the fp8 KV cache too (``spec_supported``).  Their verify rows
        # run the weight-only GEMMs (bf16 activations), whatever the plain batch-1 step of the model runs.
        self.spec_quantized = bool(spec_quantized)
        # opt-in: verify steps for regex-constrained requests too (``_verify_step(guided=True)``: the mask of the T
        # verify rows and the DFA state's hand-over inside the verify graph).  Inert without ``enable_guided``.
        self.spec_guided = bool(spec_guided)
        # opt-in: verify steps for requests that need the sampler too (temperature > 0 and / or a repetition penalty;
        # ``_verify_step(sample=True)``: verify row i makes the plain step's draw for generated token n + i, so the
        # tokens are those of the plain sampled steps of the same seed)
        self.spec_sampled = bool(spec_sampled)
        # opt-in: the largest number S of running requests (slots 0 .. S - 1) whose decode run may be a run of verify
        # steps (``_verify_step(S=)``: S * T rows, ``spec_s`` clamps it).  1 = one request in slot 0 only.  Greedy,
        # unconstrained requests only: sampled and guided verify steps stay one-sequence without the next two flags.
        self.spec_batch = int(spec_batch)
        # opt-in: requests that need the sampler in the verify steps over S sequences too (``_verify_step(sample=True,
        # S=)``: the sampled commit over S sequences; a greedy request in such a step is a sequence with temperature 0
        # and penalty 1).  Inert without ``spec_sampled`` and ``spec_batch`` > 1.
        self.spec_batch_sampled = bool(spec_batch_sampled)
        # opt-in: regex-constrained requests in the verify steps over S sequences too (``_verify_step(guided=True,
        # S=)``: every constrained sequence's T rows are masked in that sequence's own DFA states, an unconstrained
        # sequence beside it is untouched).  Inert without ``enable_guided``, ``spec_guided`` and ``spec_batch`` > 1; a
        # constrained request that needs the sampler needs ``spec_batch_sampled`` as well.
        self.spec_batch_guided = bool(spec_batch_guided)
        # opt-in: verify steps for requests that asked for per-token logprobs too (``_verify_step(logprobs=True)``: the
        # scan of the S * T raw verify rows after the lm_head and the record of the tokens the step committed after its
        # commit, kernels/logprobs.hip).  Inert without ``enable_logprobs`` and ``spec_tokens``.
        self.spec_logprobs = bool(spec_logprobs)
        # acceptance guard of the engine: a request whose accepted-per-verify-step mean falls below this after 16
        # verify steps takes plain steps for the rest of its life.  Break-even = verify-step time / plain-step time - 1.
        # Measured on MI355X (scripts/bench_spec.py, profiles/spec/spec_decode_mi355x.jsonl; plain vs verify step, k = 3):
        # duckdb-nsql-7B 128 + 128: 2.575 vs 2.845 ms -> 0.105; Llama-3.2-3B 2k + 128: 1.559 vs 1.828 ms -> 0.172
        # (k = 1: 0.085 / 0.098; k = max: 0.133 at k = 7 / 0.224 at k = 4).  The default stays 0.0 = never drop until the
        # guard has run against real (checkpoint) acceptance; set it per deployment (LSA_SPEC_MIN_ACCEPT).
        # The figures above are the break-even of ONE sequence.  A verify step over S sequences (``spec_batch``) breaks
        # even against the plain step of bucket S at, per step and request (scripts/bench_spec.py --batch,
        # profiles/spec/spec_batch_mi355x.jsonl, k = 3): 7B 0.10 / 0.12 / 0.34 and 3B 0.13 / 0.18 / 0.25 at S = 2 / 4 / 8.
        # The guard compares every request with this one value whatever S it ran at: set it to the row of the
        # spec_batch in use.  Sampled requests in such a step (``spec_batch_sampled``, against the plain sampled step of
        # bucket S; --batch --sampled, profiles/spec/spec_batch_sampled_mi355x.jsonl): 7B 0.08 / 0.12 / 0.33, 3B 0.14 /
        # 0.16 / 0.25.  Constrained requests in such a step (``spec_batch_guided``, against the plain guided step of bucket
        # S; scripts/bench_guided.py --spec-batch, profiles/spec/spec_batch_guided_mi355x.jsonl): 7B 0.08 / 0.11, 3B 0.14 /
        # 0.16 at S = 2 / 4.
        self.spec_min_accept = 0.0
        self._spec = None           # device buffers of the verify step (allocated on first use)
        self._spec_forced = None    # [nf, k] int32 planted drafts (tests / a later drafter), see set_spec_forced
        self._spec_clamp_logged = False
        self._spec_batch_clamp_logged = False
        # paged KV cache dtype: "bf16" or "fp8" (e4m3 rows with per-(token, kv-head) scales, ops.KV_FP8)
        kv_dtype = kv_dtype or ("fp8" if ops.KV_FP8 else "bf16")
        assert kv_dtype in ("bf16", "fp8"), kv_dtype
        self.kv_fp8 = kv_dtype == "fp8"
        # Megatron sequence parallelism for TP prefill (SURVEY.md §2.6 P-SP): reduce-scatter the row-parallel
        # outputs, residual + RMSNorm on T/tp rows, all-gather the bf16 normalised activations
        self.seq_parallel = True if seq_parallel is None else seq_parallel
        # SP prefill collective payload: the row-parallel GEMMs write bf16 and the reduce-scatter moves bf16 (half the
        # xGMI bytes of f32; the TP partial sums are rounded once to bf16 before the sum, as the decode all-reduce's
        # bf16 payload does); False keeps f32 slabs
        self.sp_bf16 = os.environ.get("LSA_SP_BF16", "1") != "0"
        self.sp_min_tokens = 256 if sp_min_tokens is None else sp_min_tokens
        # decode RoPE + KV append inside the attention kernel (fuse_rope=False restores the separate launch)
        self.fuse_rope = True if fuse_rope is None else fuse_rope
        self.spec = spec = weights.spec
        self.device = weights.device
        self.tp = tp
        tps = tp.size if tp is not None else 1
        self.H = spec.n_heads // tps
        self.Hkv = spec.n_kv_heads // tps
        self.D = spec.head_dim
        assert self.D == 128, "kernels are specialised for head_dim 128"
        self.d = spec.hidden
        self.L = spec.n_layers
        self.V = spec.vocab_size
        self.Vl = weights.lm_head.N
        self.ffn_l = spec.ffn // tps
        self.eps = spec.rms_eps
        self.scale = 1.0 / math.sqrt(self.D)
        self.max_slots = max_slots
        self.max_model_len = min(max_model_len, spec.max_position)
        self.max_blocks = (self.max_model_len + BLOCK - 1) // BLOCK
        self.max_new_cap = max_new_cap or self.max_model_len
        self.on_gpu = self.device.type == "cuda"
        self.use_graphs = use_graphs and self.on_gpu
        dev = self.device

        # ---------------- KV cache: [L, 2, blocks, Hkv, 64, D] bf16, or e4m3 bytes + [L, 2, blocks, Hkv, 64] f32 scales
        per_block = self.L * 2 * self.Hkv * BLOCK * ((self.D + 4) if self.kv_fp8 else self.D * 2)
        want = max_slots * self.max_blocks + 1
        if num_kv_blocks is None:
            if self.on_gpu:
                free, _ = torch.cuda.mem_get_info(dev)
                budget = int(free * kv_memory_fraction) - (1 << 30)
                num_kv_blocks = max(2, min(want, budget // per_block))
            else:
                num_kv_blocks = want
        if tp is not None and tp.size > 1:
            # every rank's arena must hold every block id the leader's scheduler hands out: ranks that size
            # their arenas from their own free memory (shared GPUs, a rebuild beside a not-yet-freed engine)
            # agree on the smallest
            num_kv_blocks = tp.min_int(num_kv_blocks)
        self.num_kv_blocks = int(num_kv_blocks)
        self.kv = torch.zeros(self.L, 2, self.num_kv_blocks, self.Hkv, BLOCK, self.D,
                              dtype=torch.uint8 if self.kv_fp8 else torch.bfloat16, device=dev)
        self.kv_scale = (torch.zeros(self.L, 2, self.num_kv_blocks, self.Hkv, BLOCK, dtype=torch.float32, device=dev)
                         if self.kv_fp8 else None)
        # one row per position the block tables can address (the kernels check this bound on the host)
        cos, sin = ref.rope_tables(self.D, self.max_blocks * BLOCK, spec.rope_theta, spec.rope_scaling, device=dev)
        self.cos, self.sin = cos.contiguous(), sin.contiguous()

        # ---------------- device decode state (one row per slot)
        S = max_slots
        i32 = dict(dtype=torch.int32, device=dev)
        self.input_ids = torch.zeros(S, **i32)
        self.positions = torch.zeros(S, **i32)
        self.gen_len = torch.zeros(S, **i32)
        self.finished = torch.ones(S, **i32)
        self.limit = torch.full((S,), self.max_new_cap, **i32)
        self.eos_on = torch.ones(S, **i32)
        self.out_tokens = torch.zeros(S, self.max_new_cap, **i32)
        self.block_tables = torch.zeros(S, self.max_blocks, **i32)
        self.temperature = torch.zeros(S, dtype=torch.float32, device=dev)
        self.top_k = torch.full((S,), 40, **i32)
        self.top_p = torch.full((S,), 0.9, dtype=torch.float32, device=dev)
        self.seeds = torch.zeros(S, dtype=torch.int64, device=dev)
        # repetition penalty (Ollama repeat_penalty / repeat_last_n): per-row ring of the context's last
        # REPEAT_WINDOW tokens, indexed by position, written by the sampling commit
        self.penalty = torch.ones(S, dtype=torch.float32, device=dev)
        self.last_n = torch.full((S,), REPEAT_WINDOW, **i32)
        self.hist = torch.full((S, REPEAT_WINDOW), -1, **i32)
        # presence / frequency penalties over the same ring and the sampler's min_p (0 = off, the default: every
        # captured sampling graph reads them, and a zero changes no logit and no draw)
        self.presence = torch.zeros(S, dtype=torch.float32, device=dev)
        self.frequency = torch.zeros(S, dtype=torch.float32, device=dev)
        self.min_p = torch.zeros(S, dtype=torch.float32, device=dev)
        self.eos_list = list(spec.eos_ids) or [-1]
        self.eos = torch.tensor(self.eos_list, **i32)

        # ---------------- decode workspaces sized for S rows
        f32 = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=torch.bfloat16, device=dev)
        self.h = torch.zeros(S, self.d, **f32)
        self.xn = torch.zeros(S, self.d, **bf)
        self.qkv = torch.zeros(S, (self.H + 2 * self.Hkv) * self.D, **bf)
        self.q = torch.zeros(S, self.H, self.D, **bf)
        self.attn = torch.zeros(S, self.H * self.D, **bf)
        self.act = torch.zeros(S, self.ffn_l, **bf)
        # fragment-major decode activations (ops.to_xfrag) for 16 < B <= 64 bf16 buckets: the norm,
        # attention and gate_up kernels write the next GEMM's MFMA B-fragments directly
        xr = 16 * ops.xfrag_tiles(min(S, 64))
        self.xn_f = torch.zeros(xr * self.d, **bf)
        self.attn_f = torch.zeros(xr * self.H * self.D, **bf)
        self.act_f = torch.zeros(xr * self.ffn_l, **bf)
        # W8A8 / W4A8 decode (fp8 or MXFP4 weights, ops.linear_a8 on the block-scaled fp8 MFMA, activations in the
        # xf8 layout): the norm launches write the qkv / gate_up inputs as per-row-scaled e4m3, the decode attention
        # writes the o input as e4m3 with one E8M0 scale per (row, head), and the gate_up GEMM's SiLU epilogue writes
        # the down input as e4m3 with one E8M0 scale per (row, 32 columns)
        wkind = weights.layers[0].wqkv.kind
        self.a8 = (ops.FP8_A8_DECODE and self.on_gpu and wkind in ("fp8", "mxfp4") and self.d % 128 == 0)
        # the down projection W8A8 needs whole 32-column blocks per SiLU workgroup (gate_up n-blocks % 4 == 0)
        self.a8_down_ok = self.ffn_l % 128 == 0 and (2 * self.ffn_l // 16) % 4 == 0
        # Which projections take e4m3 activations, per weight format and bucket (standalone sweeps with weights
        # streaming from HBM: profiles/r4/bench_a8_decode_{fp8,mxfp4}_mi355x.jsonl, scripts/bench_a8_decode.py):
        #   qkv: fp8 above 32 rows -- at 32 the W8A8 GEMM ties / loses to W8A16 (7B 13.3 vs 12.4 us) and the 7B b32
        #        bench did not move while the e4m3 activations cost top-1 agreement (profiles/bench_fp8a_decode_mi355x.jsonl);
        #        MXFP4 at every bucket (7B 8.0 vs 10.2 us at 1 row, 9.4 vs 11.9 at 32: no VALU e2m1 widening);
        #   gate_up: fp8 from 17 rows (7B 19.0 vs 22.7 us at 32), MXFP4 at every bucket (11.2 vs 15.7, 13.0 vs 15.5);
        #   o and down: only where it pays -- MXFP4 up to 16 rows (7B o 6.1 vs 10.0 us, down 7.9 vs 10.0 at 1 row); at 32
        #        rows they tie or lose (o 6.3 vs 6.1, down 9.6 vs 10.5 but the e4m3 SiLU output it needs costs gate_up
        #        15.3 vs 13.0 us), and fp8 never gains (7B b32 step 2.80 vs 2.60 ms with them,
        #        profiles/r4/rocprof_fp8_b32_a8all_summary.txt)
        mx = wkind == "mxfp4"
        self.a8_min_batch = 0 if mx else 32
        self.a8_mlp_min_batch = 0 if mx else 16
        self.a8_od_max_batch = 16 if mx else 0  # o / down W8A8 (W4A8) up to this bucket
        self.x8 = torch.zeros(xr * self.d if self.a8 else 1, dtype=torch.uint8, device=dev)
        self.sx8 = torch.ones(max(S, 64), **f32)
        mt64 = ops.xfrag_tiles(min(S, 64))
        self.x8o = torch.zeros(xr * self.H * self.D if self.a8 else 1, dtype=torch.uint8, device=dev)
        self.s8o = torch.full((mt64 * 64 * (self.H * self.D // 128) if self.a8 else 1,), 127, dtype=torch.uint8,
                              device=dev)
        a8d = self.a8 and self.a8_down_ok
        self.x8d = torch.zeros(xr * self.ffn_l if a8d else 1, dtype=torch.uint8, device=dev)
        self.s8d = torch.full((mt64 * 64 * (self.ffn_l // 128) if a8d else 1,), 127, dtype=torch.uint8, device=dev)
        self.o_buf = torch.zeros(8 * S * self.d, **f32)
        self.down_buf = torch.zeros(8 * S * self.d, **f32)
        self.qkv_buf = torch.zeros(8 * S * (self.H + 2 * self.Hkv) * self.D, **f32)
        self.logits_l = torch.zeros(S, self.Vl, **f32)
        self.logits = self.logits_l if tps == 1 else torch.zeros(S, self.V, **f32)
        self.gather_buf = None if tps == 1 else torch.zeros(tps * S * self.Vl, **f32)
        nsplit_max = max(4, ops.decode_split_plan(1, self.Hkv, self.max_model_len)[1])
        self.attn_ws = ops.decode_workspace(S, self.H, self.Hkv, nsplit_max, dev)
        self.amax_part = torch.zeros(S * ((self.V + 4095) // 4096), dtype=torch.int64, device=dev)
        self.cand = torch.zeros(S * ((self.V + 2047) // 2048) * 64, dtype=torch.int64, device=dev)
        # norm-free decode (TP = 1, gammas folded into wqkv / w_gate_up): the GEMMs read the raw residual
        # stream and scale rows by its RMS; the row sums of squares are produced by the embedding kernel
        # and the o / down residual epilogues into ssq[2l], ssq[2l + 1], ssq[2l + 2]
        self.fused_norm = tps == 1 and all(lw.norms_folded for lw in weights.layers)
        # ... for decode buckets up to this batch: measured on MI355X (rocprofv3 decode-step spans,
        # profiles/rocprof_fused_norm_ab.txt) the norm-free step wins at batch 1 (3B 2k explain 1788 -> 1738 us,
        # 7B 2.77 -> 2.71 ms) but loses at batch 32 for the 3B (2029 -> 2087 us: the residual epilogue's
        # last-arriver tail costs more than the norm launch it replaces); the norm launches stay above it
        # The 3B (hidden 3072) lost it again in round 2 once its o / down residual epilogues were re-measured
        # inside the step: 192 output blocks per row-parallel GEMM leave CUs idle without split-K, and split-K
        # adds the last-arriver tail (3B 2k explain 1.733 vs 1.708 ms per step norm-free vs norm launches,
        # 7B b1 2.625 vs 2.69 ms) -- so the default is per hidden size
        # (o / down as non-split residual GEMMs on the decode block's ring engine (ops.res_gemm, removed in round 4), in the norm-free
        # step at batch 32 measured slower than the split-K GEMMs + norm launches: 7B 3.77 vs 3.49 ms per step,
        # profiles/r3/res_ring_ab_mi355x.txt -- a standalone full-K stream cannot ramp 128-352 KB per CU fast
        # enough with <= 63 KB of LDS-DMA in flight per loader wave; not wired in)
        self.fused_norm_max_batch = 16 if self.d >= 4096 else 0
        # 12-bit weight stream (ops.pack_z12, gemm_z12.hip) for the bf16 decode GEMMs and the lm_head of the buckets
        # 17..z12_max_batch (the kernel covers up to 32 rows); 0 = off.  Same tokens either way: the kernel forms the
        # bf16 values bit for bit and sums in the bf16 kernel's order.  Read when a step is captured.
        self.z12_max_batch = Z12_MAX_BATCH
        self.res_cfg = None # experiment hook: (nb, splitk, waves, div) of the norm-free step's o / down GEMMs
        self.ssq = torch.zeros(2 * self.L + 2, S, dtype=torch.int64, device=dev)  # Q24 fixed point (ops.ss_q24)
        # arrival counters of the split-K residual epilogues (one per 16 output columns; left zeroed)
        self.res_tickets = torch.zeros(max(64, self.d // 16), dtype=torch.int32, device=dev)
        # buckets that keep the norm launches (above fused_norm_max_batch): the norms as WIDE raw residual adds
        # (ops.res_add_ss: one wave per 512-column slice, Q24 row sums of squares by integer atomics) with the RMS
        # scaling moved into the qkv / gate_up GEMMs (rownorm; gammas folded into their weights) instead of one
        # 512-thread workgroup per row with a block reduction.  TP = 1; not with W8A8 inputs (their e4m3
        # quantisation needs the whole-row amax in the norm launch) or the MLP residual epilogue
        # Under TP the residual add rides in the one-shot all-reduce (TPGroup.reduce_add: the sum over ranks, h +=,
        # bf16 / fragment-major xn and the row sums in one launch), so a TP layer issues as many launches as TP = 1.
        self.wide_norm = all(lw.norms_folded for lw in weights.layers)
        # batch-1 residual-reduce step (_decode_step_rr): the qkv and gate_up GEMMs fold the residual add of the
        # previous row-parallel projection's slabs into their prologue (ops.linear_rr), so a layer issues 5 launches
        # (qkv, attention, o, gate_up, down) and no residual-add launch; TP = 1, bf16 weights, gammas folded
        self._plan_rr()
        self.zero_slab = torch.zeros(1, 1, self.d, **f32)  # layer 0's "previous projection" in the W8A8 RR step
        self.h_alt = torch.zeros(1, self.d, **f32)  # the residual stream's second buffer (h_out never aliases h)
        self.graphs: dict = {}
        self._pending_bt: dict = {}  # slot -> block-table row of a prompt still being prefilled in chunks
        # Prefix cache (set by LLMEngine(prefix_cache=True)): a row that finishes with its prefill token parks at
        # position prompt_len instead of prompt_len - 1.  A finished row keeps rewriting the KV row of its position
        # while the decode graph replays, and prompt_len - 1 lies in a published (shared) block when the prompt fills
        # its last block exactly; prompt_len is always in the request's own blocks (admission reserves it).
        self.park_past_prompt = False
        # regex-constrained decoding (``enable_guided``): off = no buffer, launch or graph differs
        self.guided = False
        self._g_host_on: set = set()  # slots whose current request carries a constraint (host mirror of g_on)
        # per-token logprobs (``enable_logprobs``): off = no buffer, launch or graph differs
        self.logprobs = False
        # embeddings (``enable_embeddings``): off = no buffer, launch or transfer word differs
        self.embeddings = False
        # prompt-token logprobs: the scored prefill rows go through the lm_head in tiles of at most this many rows (the
        # transient logits are tile x V x 4 bytes; <= 64 rows take the skinny GEMMs, more the stream-K kernel)
        self.score_tile_rows = 256
        if self.tp is not None and self.tp.size > 1 and self.on_gpu:
            self.tp.warmup()  # communicators (RCCL + the one-shot IPC all-reduce) before any launch
            if not self.tp.capturable():  # gloo without the IPC kernel (test boxes): eager decode steps
                self.use_graphs = False

    # ------------------------------------------------------------------------------------ helpers
    def _kv_scales(self, l: int):
        """(ks, vs) scale tensors of layer l's fp8 cache, None for a bf16 cache."""
        return (self.kv_scale[l, 0], self.kv_scale[l, 1]) if self.kv_fp8 else None

    def _reduce_add(self, parts: torch.Tensor, h: torch.Tensor, xn: torch.Tensor, ss: torch.Tensor, B: int,
                    xf: bool) -> None:
        """Wide residual add of a row-parallel projection's split-K slabs (+ the TP all-reduce, fused on the IPC
        kernel): h[:B] += sum; xn = bf16(h); ss[:B] += row sums of h^2."""
        if self.tp is None or self.tp.size == 1:
            ops.res_add_ss(h, parts, xn, B, ss, xf=xf)
        else:
            self.tp.reduce_add(parts, self.h, xn, ss, B, xf=xf)

    def _reduce_parts(self, parts: torch.Tensor) -> torch.Tensor:
        """TP all-reduce of a row-parallel GEMM's split-K slabs; returns what the next add_rmsnorm sums."""
        if self.tp is None or self.tp.size == 1:
            return parts
        return self.tp.reduce_parts(parts)

    def _splitk(self, M: int, K: int, N: Optional[int] = None, tp_reduced: bool = True, xf: bool = False) -> int:
        if not self.on_gpu:
            return 1
        if M > 64:  # prefill: split-K on small tile grids; TP prefill reduces single slabs over RCCL
            return 1 if (self.tp is not None and self.tp.size > 1) else ops.tile_splitk(
                M, N or self.d, K, self.w.layers[0].wo.kind)
        if tp_reduced and self.tp is not None and self.tp.size > 1 and not self.tp.can_fold_splitk(M * self.d):
            return 1  # RCCL reduces one slab; the one-shot kernel folds split-K slabs into the all-reduce
        return ops.pick_gemm_config(M, N or self.d, K, "f32", xf=xf, kind=self.w.layers[0].wo.kind)[1]

    def a8_plan(self, B: int) -> tuple[bool, bool, bool, bool]:
        """Which decode projections run W8A8 / W4A8 (e4m3 activations) at bucket B: (qkv, gate_up, o, down)."""
        if not self.a8 or B > 64:
            return (False, False, False, False)
        qkv, gu, od = B > self.a8_min_batch, B > self.a8_mlp_min_batch, B <= self.a8_od_max_batch
        return (qkv, gu, od, gu and od and self.a8_down_ok)

    def _plan_rr(self) -> None:
        """rr_a8 / rr_decode from the current a8 buckets (``set_a8_buckets`` re-plans)."""
        lw0 = self.w.layers[0]
        # quantised weights whose batch-1 step runs all four projections W8A8 / W4A8 (MXFP4): the qkv / gate_up GEMMs
        # quantise their own residual-reduced input (ops.linear_a8_rr), so the two quantising norm launches go too
        self.rr_a8 = all(self.a8_plan(1)) and ops.rr_a8_supported(lw0.wqkv, self.d) and ops.rr_a8_supported(
            lw0.w_gate_up, self.d) and self._a8_splitk_b1() <= 4  # the prologue sums at most 4 slabs
        tps = 1 if self.tp is None else self.tp.size
        self.rr_decode = (RR_DECODE and tps == 1 and self.wide_norm and (self.rr_a8 or (
            ops.rr_supported(lw0.wqkv, self.d) and ops.rr_supported(lw0.w_gate_up, self.d))))

    def set_a8_buckets(self, min_batch: int, mlp_min_batch: int, od_max_batch: int) -> None:
        """Re-plan which decode buckets run W8A8 / W4A8 (``a8_plan``) and the batch-1 residual-reduce step; drops
        captured graphs."""
        self.a8_min_batch, self.a8_mlp_min_batch, self.a8_od_max_batch = min_batch, mlp_min_batch, od_max_batch
        self._plan_rr()
        self.graphs.clear()

    def _a8_splitk_b1(self) -> int:
        """The larger split-K of the batch-1 W8A8 / W4A8 o and down GEMMs (the slabs a residual-reduce prologue sums;
        e.g. MXFP4 Llama-3.2-3B picks 8 and keeps the norm-launch step)."""
        kind = self.w.layers[0].wqkv.kind
        if kind not in ("fp8", "mxfp4"):
            return 1
        ak = "fp8a" if kind == "fp8" else "fp4a"
        return max(ops.pick_gemm_config(1, self.d, K, "f32", xf=True, kind=ak)[1] for K in (self.H * self.D, self.ffn_l))

    def oracle_plan(self, B: int) -> dict:
        """a8_plan(B) as the numerics oracle's ``decode_a8`` dict (models/llama.py reference_forward), plus ``rr``:
        the batch-1 residual-reduce step of fp8 / MXFP4 weights quantises the qkv / gate_up inputs per 32-block
        (E8M0) from the raw residual and applies the RMS row scale after the GEMM (_decode_step_rr)."""
        plan = dict(zip(("qkv", "gate_up", "o", "down"), self.a8_plan(B)))
        plan["rr"] = B == 1 and self.rr_decode and self.rr_a8
        return plan

    def use_xfrag(self, B: int) -> bool:
        """Fragment-major activations pay off once a decode batch spans >1 row tile (B > 16):
        measured 8-20 % faster GEMMs at B = 32 (scripts/bench_xf.py); every kind with fragment-major decode GEMMs."""
        return self.on_gpu and 16 < B <= 64 and self.w.layers[0].wqkv.kind in ("bf16", "fp8", "mxfp4", "q4_0")

    def _lm_head(self, xn: torch.Tensor, M: int, xf: bool = False, z12: bool = False) -> torch.Tensor:
        """logits [M, V] (f32) for the normalised rows xn [M, d] (fragment-major when xf)."""
        loc = self.logits_l[:M] if M <= self.max_slots else torch.empty(M, self.Vl, dtype=torch.float32,
                                                                         device=self.device)
        if xf:
            ops.linear_xf(xn, M, self.w.lm_head, "f32", out=loc, splitk=1, z12=z12)
        else:
            ops.linear(xn, self.w.lm_head, "f32", out=loc, splitk=1)
        return self._gather_logits(loc, M)

    def _gather_logits(self, loc: torch.Tensor, M: int) -> torch.Tensor:
        """vocab-parallel logits -> full [M, V] (all-gather over the TP group)."""
        if self.tp is None or self.tp.size == 1:
            return loc
        tps = self.tp.size
        gb = self.gather_buf[: tps * M * self.Vl] if M <= self.max_slots else torch.empty(
            tps * M * self.Vl, dtype=torch.float32, device=self.device)
        self.tp.all_gather(gb, loc.reshape(-1))
        full = self.logits[:M] if M <= self.max_slots else torch.empty(M, self.V, dtype=torch.float32,
                                                                      device=self.device)
        full.view(M, tps, self.Vl).copy_(gb.view(tps, M, self.Vl).transpose(0, 1))
        return full

    # ------------------------------------------------------------------------------------ decode
    def ctx_plan(self, B: int, max_ctx: Optional[int] = None) -> tuple[int, int]:
        """Split-KV grid plan for a decode run whose contexts stay <= max_ctx.  Contexts are rounded up to
        a power-of-two tier (>= 256) so only a few plans (= captured graphs) exist per bucket.  Any plan is
        correct for any context (the kernel widens its splits); the tier only avoids launching split
        workgroups that short contexts leave empty: B = 32 at ctx 200 costs 24 us planned for 512 keys,
        31 us for 4096 and 42 us for 8192 (scripts/attn_scaling.py)."""
        t = self.max_model_len if max_ctx is None else min(self.max_model_len, max(256, max_ctx))
        tier = 256
        while tier < t:
            tier *= 2
        tier = min(tier, self.max_model_len)
        return tuple(ops.decode_split_plan(B, self.Hkv, tier))

    def _decode_step(self, B: int, sample: bool, plan: Optional[tuple] = None, guided: bool = False,
                     logprobs: bool = False) -> None:
        a8, a8m, a8o, a8d = self.a8_plan(B)  # qkv / gate_up / o / down W8A8 (W4A8)
        if B == 1 and self.rr_decode and (self.rr_a8 or not (a8 or a8m or a8o)):
            return self._decode_step_rr(sample, plan, guided, logprobs)
        if self.fused_norm and B <= self.fused_norm_max_batch and not (a8 or a8m or a8o):
            return self._decode_step_fused(B, sample, plan, guided, logprobs)
        w, d = self.w, self.d
        ids, pos, bt = self.input_ids[:B], self.positions[:B], self.block_tables[:B]
        h = self.h[:B]
        # e4m3 activations live in the xf8 layout: every GEMM input of the step is then fragment-major
        xf = self.step_xfrag(B)
        ak = "fp8a" if w.layers[0].wo.kind == "fp8" else "fp4a"
        sk_o = (self._splitk(B, self.H * self.D, xf=xf) if not a8o else
                ops.pick_gemm_config(B, d, self.H * self.D, "f32", xf=True, kind=ak)[1])
        sk_d = (self._splitk(B, self.ffn_l, xf=xf) if not a8d else
                ops.pick_gemm_config(B, d, self.ffn_l, "f32", xf=True, kind=ak)[1])
        nqkv = (self.H + 2 * self.Hkv) * self.D
        sk_q = (ops.pick_gemm_config(B, nqkv, d, "f32", xf=True, kind=ak)[1] if a8
                else self._splitk(B, d, nqkv, tp_reduced=False, xf=xf))
        q8 = dict(x8=self.x8, sx8=self.sx8) if a8 else {}
        q8m = dict(x8=self.x8, sx8=self.sx8) if a8m else {}
        # each side of the layer: a wide residual add + row scale in the next GEMM unless that GEMM runs W8A8 (its
        # e4m3 input comes from the quantising norm launch)
        wna = self.wide_norm and not a8
        wnm = self.wide_norm and not a8m
        # the embedding launch writes raw rows + row sums and zeroes every later accumulator whenever any side uses them
        # (layer 0's qkv then row-scales, whatever its later layers do)
        raw0 = wna or wnm
        ssq = self.ssq
        rn_a = lambda l: dict(rownorm=(ssq[2 * l], self.eps)) if (wna or (l == 0 and raw0)) else {}  # noqa: E731
        assert not (a8 and wna), "a W8A8 qkv input comes from the quantising norm launch"
        rn_m = lambda l: dict(rownorm=(ssq[2 * l + 1], self.eps)) if wnm else {}  # noqa: E731
        o_parts = self.o_buf[: sk_o * B * d].view(sk_o, B, d)
        d_parts = self.down_buf[: sk_d * B * d].view(sk_d, B, d)
        qkv_parts = self.qkv_buf[: sk_q * B * nqkv].view(sk_q, B, nqkv)
        plan = plan or ops.decode_split_plan(B, self.Hkv, self.max_model_len)
        ws = self.attn_ws
        if xf:  # every GEMM input lives in the fragment-major layout, written by its producer
            xn, attn, act = self.xn_f, self.attn_f, self.act_f

            z12 = 16 < B <= self.z12_max_batch

            def lin(x, wt, epi, **kw):
                return ops.linear_xf(x, B, wt, epi, z12=z12, **kw)
        else:
            xn, attn, act = self.xn[:B], self.attn[:B], self.act[:B]
            lin = ops.linear
            z12 = False
        for l, lw in enumerate(w.layers):
            if l == 0 and raw0:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=B, xf=xf,
                                ss_out=ssq.view(-1), ss_ld=self.max_slots, ss_nzero=2 * self.L, **q8)
            elif l == 0:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=B, xf=xf, **q8)
            elif wna:
                self._reduce_add(d_parts, h, xn, ssq[2 * l], B, xf)
            else:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, parts=self._reduce_parts(d_parts), rows=B, xf=xf, **q8)
            # QKV as f32 split-K slabs; the attention kernel sums them, applies RoPE and appends the new
            # token's k/v to the paged cache itself (no separate rope/append launch)
            if a8:  # (layer 0 after a raw embedding launch: its e4m3 rows are un-normalised -> row scale)
                ops.linear_a8(self.x8, self.sx8, B, lw.wqkv, "f32", out=qkv_parts, splitk=sk_q, **rn_a(l))
            else:
                lin(xn, lw.wqkv, "f32", out=qkv_parts, splitk=sk_q, **rn_a(l))
            kc, vc = self.kv[l, 0], self.kv[l, 1]
            if not self.fuse_rope:
                ops.rope_append(qkv_parts, pos, None, bt, self.cos, self.sin, self.q[:B], kc, vc, self.H, self.Hkv,
                                kv_scales=self._kv_scales(l))
            fr = self.fuse_rope
            ops.attn_decode(self.q[:B], kc, vc, bt, pos, self.H, self.Hkv, self.scale,
                            (self.x8o if a8o else attn) if xf else attn.view(B, self.H, self.D), workspace=ws,
                            plan=plan, xf=xf, qkv_parts=qkv_parts if fr else None, cos=self.cos if fr else None,
                            sin=self.sin if fr else None, kv_scales=self._kv_scales(l),
                            out_s8=self.s8o if a8o else None)
            if a8o:
                ops.linear_a8(self.x8o, None, B, lw.wo, "f32", out=o_parts, splitk=sk_o, s8=self.s8o)
            else:
                lin(attn, lw.wo, "f32", out=o_parts, splitk=sk_o)
            if wnm:
                self._reduce_add(o_parts, h, xn, ssq[2 * l + 1], B, xf)
            else:
                ops.add_rmsnorm(h, lw.mlp_norm, self.eps, xn, parts=self._reduce_parts(o_parts), rows=B, xf=xf, **q8m)
            if a8m:
                ops.linear_a8(self.x8, self.sx8, B, lw.w_gate_up, "silu", out=self.x8d if a8d else act,
                              out_s8=self.s8d if a8d else None)
            else:
                lin(xn, lw.w_gate_up, "silu", out=act, **rn_m(l))
            if a8d:
                ops.linear_a8(self.x8d, None, B, lw.w_down, "f32", out=d_parts, splitk=sk_d, s8=self.s8d)
            else:
                lin(act, lw.w_down, "f32", out=d_parts, splitk=sk_d)
        ops.add_rmsnorm(h, w.final_norm, self.eps, xn, parts=self._reduce_parts(d_parts), rows=B, xf=xf)
        self._decode_tail(B, sample, xn, xf, guided, z12=z12, logprobs=logprobs)

    def _decode_step_fused(self, B: int, sample: bool, plan: Optional[tuple] = None, guided: bool = False,
                           logprobs: bool = False) -> None:
        """Norm-free decode step (TP = 1): 5 launches per layer instead of 7.

          embed (+ row sum of squares)  ->  per layer:
            gemm qkv (rows scaled by rsqrt(ss/d + eps), f32 split-K slabs) -> attn_decode (RoPE + KV append)
            -> gemm o (residual epilogue: h += y, x = bf16(h), ss += h^2)
            -> gemm gate_up (row-scaled, SiLU*up) -> gemm down (residual epilogue)
          -> final RMSNorm -> lm_head -> token commit
        """
        w, d = self.w, self.d
        ids, pos, bt = self.input_ids[:B], self.positions[:B], self.block_tables[:B]
        h = self.h[:B]
        xf = self.use_xfrag(B)
        nqkv = (self.H + 2 * self.Hkv) * self.D
        sk_q = self._splitk(B, d, nqkv, tp_reduced=False, xf=xf)
        # the residual-epilogue GEMMs run their own tuned split (ops/gemm_tuning.json "res" entries; the
        # f32 pick where none is tuned)
        sk_o = ops.pick_gemm_config(B, d, self.H * self.D, "res", xf=xf, kind=w.layers[0].wo.kind)[1]
        sk_d = ops.pick_gemm_config(B, d, self.ffn_l, "res", xf=xf, kind=w.layers[0].w_down.kind)[1]
        rc = {}
        if self.res_cfg is not None:  # experiment override (bench.py --set res_cfg=(nb,splitk,waves,div))
            nb_, sk_o, wv_, dv_ = self.res_cfg
            sk_d = sk_o
            rc = dict(nb=nb_, waves=wv_, div=dv_)
        qkv_parts = self.qkv_buf[: sk_q * B * nqkv].view(sk_q, B, nqkv)
        o_parts = self.o_buf[: sk_o * B * d].view(sk_o, B, d)
        d_parts = self.down_buf[: sk_d * B * d].view(sk_d, B, d)
        plan = plan or ops.decode_split_plan(B, self.Hkv, self.max_model_len)
        ws = self.attn_ws
        ssq, S, tk = self.ssq, self.max_slots, self.res_tickets
        if xf:
            xn, attn, act = self.xn_f, self.attn_f, self.act_f

            def lin(x, wt, epi, **kw):
                return ops.linear_xf(x, B, wt, epi, **kw)
        else:
            xn, attn, act = self.xn[:B], self.attn[:B], self.act[:B]
            lin = ops.linear
        ops.add_rmsnorm(h, w.layers[0].attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=B, xf=xf,
                        ss_out=ssq.view(-1), ss_ld=S, ss_nzero=2 * self.L)
        for l, lw in enumerate(w.layers):
            lin(xn, lw.wqkv, "f32", out=qkv_parts, splitk=sk_q, rownorm=(ssq[2 * l], self.eps))
            kc, vc = self.kv[l, 0], self.kv[l, 1]
            ops.attn_decode(self.q[:B], kc, vc, bt, pos, self.H, self.Hkv, self.scale,
                            attn if xf else attn.view(B, self.H, self.D), workspace=ws, plan=plan, xf=xf,
                            qkv_parts=qkv_parts, cos=self.cos, sin=self.sin, kv_scales=self._kv_scales(l))
            lin(attn, lw.wo, "res", out=o_parts, splitk=sk_o, res=(h, xn, ssq[2 * l + 1], tk), **rc)
            lin(xn, lw.w_gate_up, "silu", out=act, rownorm=(ssq[2 * l + 1], self.eps))
            lin(act, lw.w_down, "res", out=d_parts, splitk=sk_d, res=(h, xn, ssq[2 * l + 2], tk), **rc)
        ops.add_rmsnorm(h, w.final_norm, self.eps, xn, rows=B, xf=xf, write_h=False)
        self._decode_tail(B, sample, xn, xf, guided, logprobs=logprobs)

    def _decode_step_rr(self, sample: bool, plan: Optional[tuple] = None, guided: bool = False,
                        logprobs: bool = False) -> None:
        """Batch-1 decode step with the residual adds folded into the GEMM prologues (TP = 1, bf16, gammas folded):
        5 launches per layer.

          embed (raw h, bf16(h), sum h^2)  ->  per layer:
            gemm qkv  (layer 0: bf16 x, row-scaled slabs; later layers ops.linear_rr: x = h + sum(down slabs) formed
                       in the prologue, h_out = x, sum x^2 -> ssq[l], unscaled f32 slabs)
            -> attn_decode (slab sum, RMS row scale from ssq[l], RoPE, KV append, split-KV attention)
            -> gemm o (f32 split-K slabs)
            -> gemm gate_up (ops.linear_rr: x = h + sum(o slabs), its own full-row RMS scale, SiLU * up)
            -> gemm down (f32 split-K slabs)
          -> final RMSNorm (h + down slabs) -> lm_head -> token commit
        The residual stream alternates between self.h and self.h_alt (a prologue's other workgroups still read the
        buffer the column-0 workgroups replace).
        With fp8 / MXFP4 weights (``rr_a8``) every projection runs W8A8 / W4A8: qkv and gate_up quantise their
        residual-reduced input themselves (ops.linear_a8_rr; layer 0's qkv reduces the embedding row with a zero
        slab), attention writes the o input as e4m3 + E8M0 per head, gate_up the down input as e4m3 + E8M0 per 32."""
        w, d, B = self.w, self.d, 1
        ids, pos, bt = self.input_ids[:1], self.positions[:1], self.block_tables[:1]
        nqkv = (self.H + 2 * self.Hkv) * self.D
        a8 = self.rr_a8
        if a8:
            ak = "fp8a" if w.layers[0].wqkv.kind == "fp8" else "fp4a"
            sk_q = ops.rr_config(nqkv, d, "f32", w.layers[0].wqkv.kind)[1]
            sk_o = ops.pick_gemm_config(1, d, self.H * self.D, "f32", xf=True, kind=ak)[1]
            sk_d = ops.pick_gemm_config(1, d, self.ffn_l, "f32", xf=True, kind=ak)[1]
        else:
            sk_q = ops.rr_config(nqkv, d, "f32", w.layers[0].wqkv.kind)[1] if self.on_gpu else 1
            sk_o = self._splitk(1, self.H * self.D)
            sk_d = self._splitk(1, self.ffn_l)
        assert sk_o <= 4 and sk_d <= 4, "the residual-reduce prologue sums at most 4 slabs"
        qkv_parts = self.qkv_buf[: sk_q * nqkv].view(sk_q, 1, nqkv)
        o_parts = self.o_buf[: sk_o * d].view(sk_o, 1, d)
        d_parts = self.down_buf[: sk_d * d].view(sk_d, 1, d)
        plan = plan or ops.decode_split_plan(1, self.Hkv, self.max_model_len)
        ssq = self.ssq
        hs = (self.h[:1], self.h_alt)
        cur = 0
        xn, attn, act = self.xn[:1], self.attn[:1], self.act[:1]
        ops.add_rmsnorm(hs[0], w.layers[0].attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=1,
                        ss_out=ssq.view(-1), ss_ld=self.max_slots, ss_nzero=self.L)
        for l, lw in enumerate(w.layers):
            if a8:  # the qkv input (embedding row | h + down slabs) quantised in the GEMM's prologue
                ops.linear_a8_rr(hs[cur], self.zero_slab if l == 0 else d_parts, hs[1 - cur], lw.wqkv, "f32",
                                 out=qkv_parts, ss_out=ssq[l + 1], eps=self.eps, splitk=sk_q)
                cur = 1 - cur
                rn = (ssq[l + 1], self.eps, d)
            elif l == 0:
                ops.linear(xn, lw.wqkv, "f32", out=qkv_parts, splitk=sk_q, rownorm=(ssq[0], self.eps))
                rn = None
            else:
                ops.linear_rr(hs[cur], d_parts, hs[1 - cur], lw.wqkv, "f32", out=qkv_parts, ss_out=ssq[l + 1],
                              eps=self.eps, splitk=sk_q)
                cur = 1 - cur
                rn = (ssq[l + 1], self.eps, d)
            kc, vc = self.kv[l, 0], self.kv[l, 1]
            if a8:
                ops.attn_decode(self.q[:1], kc, vc, bt, pos, self.H, self.Hkv, self.scale, self.x8o, workspace=self.attn_ws,
                                plan=plan, xf=True, qkv_parts=qkv_parts, cos=self.cos, sin=self.sin,
                                kv_scales=self._kv_scales(l), out_s8=self.s8o, rownorm=rn)
                ops.linear_a8(self.x8o, None, 1, lw.wo, "f32", out=o_parts, splitk=sk_o, s8=self.s8o)
                ops.linear_a8_rr(hs[cur], o_parts, hs[1 - cur], lw.w_gate_up, "silu", out=self.x8d, out_s8=self.s8d,
                                 eps=self.eps)
                cur = 1 - cur
                ops.linear_a8(self.x8d, None, 1, lw.w_down, "f32", out=d_parts, splitk=sk_d, s8=self.s8d)
                continue
            ops.attn_decode(self.q[:1], kc, vc, bt, pos, self.H, self.Hkv, self.scale, attn.view(1, self.H, self.D),
                            workspace=self.attn_ws, plan=plan, qkv_parts=qkv_parts, cos=self.cos, sin=self.sin,
                            kv_scales=self._kv_scales(l), rownorm=rn)
            ops.linear(attn, lw.wo, "f32", out=o_parts, splitk=sk_o)
            ops.linear_rr(hs[cur], o_parts, hs[1 - cur], lw.w_gate_up, "silu", out=act, eps=self.eps)
            cur = 1 - cur
            ops.linear(act, lw.w_down, "f32", out=d_parts, splitk=sk_d)
        ops.add_rmsnorm(hs[cur], w.final_norm, self.eps, xn, parts=d_parts, rows=1, write_h=False)
        self._decode_tail(B, sample, xn, False, guided, logprobs=logprobs)

    def _decode_tail(self, B: int, sample: bool, xn, xf: bool, guided: bool = False, z12: bool = False,
                     logprobs: bool = False) -> None:
        logits = self._lm_head(xn, B, xf, z12)
        if logprobs:  # the raw rows: ahead of the mask and the penalties, which rewrite ``logits`` in place
            self._logprob_scan(logits, self.lp_k[:B], self.finished[:B], self.gen_len[:B], self.lp_n0[:B])
        if guided:  # -inf into every token that would kill a constrained row's DFA; the commits below run unchanged
            self._dfa_mask(logits, self.gen_len[:B], self.input_ids[:B], self.finished[:B])
        st = (self.out_tokens[:B], self.gen_len[:B], self.input_ids[:B], self.positions[:B], self.finished[:B])
        if sample:
            ops.sample_commit(logits, self.hist[:B], self.penalty[:B], self.temperature[:B], self.top_k[:B],
                              self.top_p[:B], self.seeds[:B], *st, self.eos, self.limit[:B], self.eos_on[:B],
                              workspace=(self.amax_part, self.cand) if self.on_gpu else None,
                              last_n=self.last_n[:B], presence=self.presence[:B], frequency=self.frequency[:B],
                              min_p=self.min_p[:B])
        else:
            ops.argmax_commit(logits, *st, self.eos, self.limit[:B], self.eos_on[:B],
                              part=self.amax_part if self.on_gpu else None)
        if logprobs:
            ops.logprob_commit(self.lp_raw, self.lp_k, self.lp_n0, self.gen_len, self.out_tokens, self.lp_tok,
                               self.lp_ids, self.lp_top, B, workspace=self.lp_ws)

    def final_hidden(self, B: int) -> torch.Tensor:
        """[B, d] bf16: the final-norm output rows of the last decode step (what the lm_head read), in row order
        whatever layout the step's bucket used (the numerics check of tied-embedding models reads it)."""
        if self.step_xfrag(B):
            return ops.from_xfrag(self.xn_f, B, self.d)
        return self.xn[:B]

    def step_xfrag(self, B: int) -> bool:
        """Whether the decode step of bucket B hands its activations on in the fragment-major layouts (use_xfrag,
        or -- any W8A8 / W4A8 projection -- the xf8 one, which forces it at any batch)."""
        a8, a8m, a8o, _ = self.a8_plan(B)
        return self.use_xfrag(B) or a8 or a8m or a8o

    def bucket(self, n: int) -> int:
        b = 1
        while b < n:
            b *= 2
        return min(b, self.max_slots) if n <= self.max_slots else self.max_slots

    @staticmethod
    def graph_key(B: int, sample: bool, plan: tuple, guided: bool = False, logprobs: bool = False) -> tuple:
        """Key of a decode graph: (B, sample, plan), and (B, sample, plan, True) for its guided variant (the same step
        with the ``dfa_mask`` launch between the lm_head and the commit).  The logprob variant of either (two launches
        more: ``logprob_scan`` after the lm_head, ``logprob_commit`` after the token commit) is (B, sample, plan,
        guided, "lp"); without the flag every key is what it was."""
        if logprobs:
            return (B, sample, plan, bool(guided), "lp")
        return (B, sample, plan, True) if guided else (B, sample, plan)

    def capture(self, B: int, sample: bool, plan: Optional[tuple] = None, guided: bool = False,
                logprobs: bool = False) -> None:
        """Capture the decode-step graph of (bucket, sampling mode, split plan).  (Several steps per graph were
        measured no faster -- no idle time at graph boundaries, profiles/decode_b32_normfree_spg_ab_mi355x.txt.)"""
        plan = tuple(plan or self.ctx_plan(B))
        assert self.guided or not guided, "guided decode graphs need enable_guided()"
        assert self.logprobs or not logprobs, "logprob decode graphs need enable_logprobs()"
        key = self.graph_key(B, sample, plan, guided, logprobs)
        if key in self.graphs:
            return
        if self.tp is not None and self.tp.size > 1:
            self.tp.warmup()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            # state must not change during capture: kernels are recorded, not executed
            with torch.cuda.graph(g, stream=s):
                self._decode_step(B, sample, plan, guided, logprobs)
        torch.cuda.current_stream(self.device).wait_stream(s)
        self.graphs[key] = g

    def count_step_kernels(self, B: int, sample: bool = False, logprobs: bool = False) -> int:
        """Kernel launches of one captured decode step of bucket B (a throw-away capture whose graph is kept and
        walked with hipGraphGetNodes): the launch-count check of the fused TP step (tests/test_tp_launches_gpu.py)."""
        assert self.use_graphs, "needs graph capture"
        plan = tuple(self.ctx_plan(B))
        if self.tp is not None and self.tp.size > 1:
            self.tp.warmup()
        return self._count_kernels(lambda: self._decode_step(B, sample, plan, False, logprobs))

    def count_verify_kernels(self, S: int = 1, guided: bool = False, sample: bool = False,
                             logprobs: bool = False) -> int:
        """Kernel launches of one captured verify step over S sequences (``count_step_kernels`` for ``_verify_step``)."""
        assert self.use_graphs, "needs graph capture"
        plan = tuple(self.ctx_plan(S))
        self._spec_bufs()
        if logprobs:
            self._spec_lp_ws()
        return self._count_kernels(lambda: self._verify_step(plan, guided, sample, S, logprobs))

    def _count_kernels(self, step) -> int:
        """The kernel nodes of a throw-away capture of ``step()``."""
        import ctypes

        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.current_stream(self.device).wait_stream(s)
        lib = ctypes.CDLL("libamdhip64.so")
        graph = ctypes.c_void_p(g.raw_cuda_graph())
        n = ctypes.c_size_t(0)
        assert lib.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
        nodes = (ctypes.c_void_p * n.value)()
        assert lib.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
        kernels = 0
        for nd in nodes:
            t = ctypes.c_int(-1)
            assert lib.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(t)) == 0
            kernels += t.value == 0  # hipGraphNodeTypeKernel
        g.reset()
        return kernels

    def buckets(self) -> list[int]:
        out, b = [], 1
        while b < self.max_slots:
            out.append(b)
            b *= 2
        return out + [self.max_slots]

    def plans(self, B: int) -> list[tuple]:
        """Distinct split plans over the context tiers 256, 512, ... max_model_len."""
        out, t = [], 256
        while True:
            p = self.ctx_plan(B, t)
            if p not in out:
                out.append(p)
            if t >= self.max_model_len:
                return out
            t *= 2

    def capture_all(self, sample_modes: Sequence[bool] = (False, True)) -> None:
        """Capture every (bucket, sampling mode, context tier) decode graph up front, so a server never
        pays a capture inside a request."""
        if not self.use_graphs:
            return
        for b in self.buckets():
            for sm in sample_modes:
                for p in self.plans(b):
                    self.capture(b, sm, p)
                    if self.guided:
                        self.capture(b, sm, p, guided=True)
                    if self.logprobs:
                        self.capture(b, sm, p, logprobs=True)
                        if self.guided:
                            self.capture(b, sm, p, guided=True, logprobs=True)
        torch.cuda.synchronize(self.device)

    def decode(self, B: int, steps: int, sample: bool = False, max_ctx: Optional[int] = None,
               guided: bool = False, logprobs: bool = False) -> None:
        """Run ``steps`` decode steps over slot rows [0, B) (B a bucket size); ``max_ctx`` bounds every
        row's context length during the run (picks the graph planned for that tier).  ``guided``: the variant with
        the regex mask, for runs in which a row is constrained; ``logprobs``: the variant that records per-token
        log-probabilities, for runs in which a row asked (``enable_logprobs``)."""
        plan = tuple(self.ctx_plan(B, max_ctx))
        if not self.use_graphs:
            for _ in range(steps):
                self._decode_step(B, sample, plan, guided, logprobs)
            return
        self.capture(B, sample, plan, guided, logprobs)
        g = self.graphs[self.graph_key(B, sample, plan, guided, logprobs)]
        for _ in range(steps):
            g.replay()

    # ------------------------------------------------------------------------------------ speculative decoding
    def spec_k(self) -> int:
        """Drafted tokens per verify step: ``spec_tokens`` clamped to what ``attn_verify`` takes (T = k + 1 <= 8
        rows and T * G <= 16 query rows per kv head)."""
        k = min(int(self.spec_tokens), 7, 16 // max(1, self.H // self.Hkv) - 1)
        if 0 <= k < self.spec_tokens and not self._spec_clamp_logged:
            self._spec_clamp_logged = True
            import logging
            logging.getLogger(__name__).warning("spec_tokens=%d clamped to %d (T <= 8, T * H / Hkv <= 16)",
                                                self.spec_tokens, k)
        return max(k, 0)

    def spec_s(self) -> int:
        """The most sequences a verify step may serve: ``spec_batch`` clamped to a power of two that is at most 8 (the
        sequences ``attn_verify`` takes), at most ``max_slots``, and keeps spec_batch * T <= 32 rows (T = 8 allows 4)."""
        want = max(1, int(self.spec_batch))
        T = self.spec_k() + 1
        s = 1
        while s * 2 <= min(want, self.max_slots, 8) and s * 2 * T <= 32:
            s *= 2
        if s != want and not self._spec_batch_clamp_logged:
            self._spec_batch_clamp_logged = True
            import logging
            logging.getLogger(__name__).warning("spec_batch=%d clamped to %d (a power of two, spec_batch * T <= 32, "
                                                "<= max_slots)", self.spec_batch, s)
        return s

    def spec_supported(self) -> bool:
        """Whether this runner can run verify steps: TP = 1, at least one drafted token, and either bf16 weights with
        the bf16 KV cache or -- ``spec_quantized`` -- bf16 / fp8 / MXFP4 weights with the bf16 or the fp8 cache."""
        tps = 1 if self.tp is None else self.tp.size
        bf16 = ("bf16", "dense")  # packed for the GPU / plain on the CPU
        # (a CPU engine keeps every weight dense; it is gated by the kind it was built for, like its GPU twin)
        kinds = [getattr(w, "requested", None) or w.kind for w in (self.w.layers[0].wqkv, self.w.lm_head)]
        if self.spec_quantized:
            dtypes = all(k in bf16 + ("fp8", "mxfp4") for k in kinds)
        else:
            dtypes = not self.kv_fp8 and all(k in bf16 for k in kinds)
        return self.spec_tokens > 0 and tps == 1 and dtypes and self.spec_k() >= 1

    def spec_oracle_plan(self) -> dict:
        """``oracle_plan`` of the verify rows: every projection weight-only (bf16 activations), no residual-reduce
        quantisation -- whatever the plain batch-1 step of the same runner runs."""
        return dict(qkv=False, gate_up=False, o=False, down=False, rr=False)

    def _spec_bufs(self) -> dict:
        """Device buffers of the verify step, sized for the most rows a step can have (32 = S * T), and the context
        history ``ctx`` / ``ctx_len`` of the ``spec_s()`` slots that may speculate."""
        if self._spec is not None:
            assert self._spec["ctx"].shape[0] >= self.spec_s(), "spec_batch must be set before the first verify step"
            return self._spec
        dev, TM, SB = self.device, 32, self.spec_s()
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=torch.bfloat16, device=dev)
        nqkv = (self.H + 2 * self.Hkv) * self.D
        nsplit_max = max([4] + [ops.verify_split_plan(self.Hkv, self.max_model_len, S)[1] for S in (1, 2, 4, 8)])
        self._spec = dict(
            # the prompt history of slots 0 .. SB - 1
            ctx=torch.zeros(SB, self.max_model_len, **i32), ctx_len=torch.zeros(SB, **i32),
            ids=torch.zeros(TM, **i32), pos=torch.zeros(TM, **i32), draft=torch.full((TM,), -1, **i32),
            # seq0[T]: the sequence (block-table row) of verify row i = i // T
            seq0={T: (torch.arange(TM, device=dev) // T).to(torch.int32) for T in range(1, 9)},
            stats=torch.zeros(max(SB, 1), 3, dtype=torch.int64, device=dev),
            h=torch.zeros(TM, self.d, **f32), xn=torch.zeros(TM, self.d, **bf), q=torch.zeros(TM, self.H, self.D, **bf),
            attn=torch.zeros(TM, self.H * self.D, **bf), act=torch.zeros(TM, self.ffn_l, **bf),
            o_buf=torch.zeros(8 * TM * self.d, **f32), down_buf=torch.zeros(8 * TM * self.d, **f32),
            qkv_buf=torch.zeros(8 * TM * nqkv, **f32), logits=torch.zeros(TM, self.Vl, **f32),
            ssq=torch.zeros(2 * self.L + 2, TM, dtype=torch.int64, device=dev),
            amax_part=torch.zeros(TM * ((self.V + 4095) // 4096), dtype=torch.int64, device=dev),
            # sampled verify steps (ops.spec_sample_commit): the rows' top-k candidates and their picked tokens
            cand=torch.zeros(TM * ((self.V + 2047) // 2048) * 64, dtype=torch.int64, device=dev),
            picks=torch.zeros(TM, **i32),
            attn_ws=ops.verify_workspace(TM, self.H, self.Hkv, nsplit_max, dev))  # (TM rows = S * T)
        return self._spec

    def set_spec_forced(self, table: Optional[torch.Tensor]) -> None:
        """Plant the drafts of the next verify steps instead of searching: ``table`` [nf, k] int32, a step whose row
        has generated g tokens drafts row min(g, nf - 1) (None restores the n-gram search); ``table`` [S, nf, k] plants
        table s in the sequence of slot s (S >= the S of the verify steps that read it).  One device buffer per
        table shape, rewritten in place: a captured verify graph is keyed by the buffer it reads."""
        if table is None:
            self._spec_forced = None
            return
        bufs = self.__dict__.setdefault("_spec_forced_bufs", {})
        buf = bufs.get(tuple(table.shape))
        if buf is None:
            buf = bufs[tuple(table.shape)] = torch.zeros(tuple(table.shape), dtype=torch.int32, device=self.device)
        buf.copy_(table.to(torch.int32))
        self._spec_forced = buf

    def _verify_step(self, plan: Optional[tuple] = None, guided: bool = False, sample: bool = False, S: int = 1,
                     logprobs: bool = False) -> None:
        """One speculative-decoding step of the request in slot 0: a forward pass over T = k + 1 rows -- the row's input
        token and k drafted tokens at positions p .. p + T - 1 -- and the in-order commit of the tokens greedy decoding
        would have produced (``ops.spec_commit``): between 1 and T per step, the same sequence as plain steps.

        ``S`` > 1 (``spec_batch``; unconstrained): the same launches over the S sequences of slots 0 .. S - 1,
        S * T rows with row-major activations throughout -- rows s T .. s T + T - 1 are sequence s: its state row,
        ``block_tables[s]``, ``positions[s]``; the GEMMs and their split-K are those of S * T rows, ``attn_verify`` runs
        the S sequences in one launch and ``spec_commit`` commits each into its own state row and counts in its own
        row of ``stats``.  A slot below S without a request is the row ``release_slot`` leaves -- finished, position 0,
        a block table of zeros: it rewrites T rows of scratch block 0, commits nothing and counts nothing.

          spec_draft -> embed -> per layer: gemm qkv (f32 slabs) -> rope_append (RoPE + the T K/V rows into the cache)
          -> attn_verify (all T rows share one pass over the cache) -> gemm o -> norm -> gemm gate_up -> gemm down
          -> final norm -> lm_head over T rows -> spec_commit

        KV invariant, per sequence (a sequence writes only the blocks of its own table, whatever its neighbours accept):
        a step writes cache positions p .. p + T - 1 and advances to p' = p + a + 1 (a accepted drafts).
        The stale rows p' .. p + T - 1 lie inside the next step's write range p' .. p' + T - 1, so the next step (or
        the next plain step, which writes p' before reading it) overwrites them before any query can see them: row t
        sees only keys <= p' + t.  A finished row keeps its position and rewrites the same T positions when the graph
        replays; the engine reserves those positions (LLMEngine._spec_run).
        With the fp8 cache a rejected row's e4m3 bytes and its f32 scale are both overwritten by that next step
        (rope_append writes a row's bytes and its scale together), so the invariant holds for the pair (bytes, scale).
        The 16-byte unit that a token pair shares (common.h kv8_off) is safe: each token writes only its own 8 bytes
        of it, so rewriting a stale odd token never touches its committed even partner, and the other way round.

        fp8 / MXFP4 weights: every verify row runs the weight-only GEMMs (W8A16 / W4A16) through ``ops.linear``, the
        lm_head included; there are no e4m3 activations in a verify step.

        ``guided`` (a constrained request, ``spec_guided``): ``dfa_mask_verify`` between the lm_head and spec_commit masks
        row t in the DFA state after the input token and drafts 1..t, so the commit accepts a draft only where the plain
        guided step would have chosen it; ``dfa_spec_advance`` after the commit leaves the state after the accepted
        drafts where the next mask launch -- verify or plain -- advances from.

        ``sample`` (a request that needs the sampler, ``spec_sampled``): the step ends in ``ops.spec_sample_commit``
        instead: row i is penalised over the ring as it would stand had drafts 0 .. i-1 been committed and makes the
        plain step's draw for generated token gen_len + i; a draft is accepted exactly when it equals that draw, so
        the committed tokens are the plain sampled tokens of the same seed.  A rejected row's draw counter is used
        again by the next step, as the plain path would use it.  With ``guided`` the mask runs before it (a -inf logit
        stays -inf under the penalty and is never kept by the sampler) and the DFA hand-over after it, unchanged.

        ``sample`` with ``S`` > 1 (``spec_batch_sampled``): the sampled commit over the S sequences -- sequence s reads
        ring row s and entry s of every sampling parameter and draws at its own counter gen_len[s] + i, so each
        request's tokens are those it generates alone; a greedy request among them is a sequence with temperature 0
        and penalty 1, whose rows the commit leaves as they are and whose picks are their argmax.

        ``guided`` with ``S`` > 1 (``spec_batch_guided``): the mask over the S sequences in one launch -- sequence s is
        masked in the states of table row s (= its slot, as in the plain decode mask) from its own drafts, and leaves
        gen_len and its T states in row s of ``g_spec`` for the hand-over after the commit; a sequence without a
        constraint (or finished, or an idle slot) is untouched, as an unconstrained row is in the plain ``dfa_mask``.
        Each request's tokens are those of its plain guided steps.  With ``sample`` the mask runs before the sampled
        commit over the S sequences, as in the one-sequence step.

        ``logprobs`` (a running request asked, ``spec_logprobs``): ``spec_logprob_scan`` between the lm_head and the mask
        keeps the raw rows of every sequence that asked (the raw rule: before ``dfa_mask_verify``, the penalties and
        the sampler) and announces n0 = gen_len[s]; ``spec_logprob_commit`` at the end records the c = gen_len[s] - n0
        tokens the step committed, token n0 + t from verify row t, into the per-slot records of slot s.  A sequence
        that did not ask (lp_k[s] < 0), a finished one and an idle slot record nothing."""
        w, d, Ts = self.w, self.d, self.spec_k() + 1
        sb = self._spec_bufs()
        assert not logprobs or (self.spec_logprobs and self.logprobs), \
            "logprob verify steps need spec_logprobs and enable_logprobs()"
        lp_ws = self._spec_lp_ws() if logprobs else None
        assert S == 1 or not guided or (self.spec_batch_guided and self.spec_guided and self.guided), \
            "guided verify steps are one-sequence"
        assert S == 1 or not sample or (self.spec_sampled and self.spec_batch_sampled), \
            "sampled verify steps over several sequences need spec_sampled and spec_batch_sampled"
        assert 1 <= S <= sb["ctx"].shape[0] and S * Ts <= 32, "verify step: S <= spec_batch sequences, S * T <= 32 rows"
        T = S * Ts  # rows of the step from here on
        n_max, n_min = self.spec_ngram
        st = (self.out_tokens[:S], self.gen_len[:S], self.input_ids[:S], self.positions[:S], self.finished[:S])
        ids, pos, bt = sb["ids"][:T], sb["pos"][:T], self.block_tables[:S]
        draft = sb["draft"][:S * (Ts - 1)]
        ops.spec_draft(sb["ctx"][:S], sb["ctx_len"][:S], st[0], st[1], st[2], st[3], Ts - 1, ids, pos, draft,
                       n_max=n_max, n_min=n_min, forced=self._spec_forced)
        h, xn, attn, act, q = sb["h"][:T], sb["xn"][:T], sb["attn"][:T], sb["act"][:T], sb["q"][:T]
        nqkv = (self.H + 2 * self.Hkv) * self.D
        sk_o = self._splitk(T, self.H * self.D)
        sk_d = self._splitk(T, self.ffn_l)
        sk_q = self._splitk(T, d, nqkv, tp_reduced=False)
        o_parts = sb["o_buf"][: sk_o * T * d].view(sk_o, T, d)
        d_parts = sb["down_buf"][: sk_d * T * d].view(sk_d, T, d)
        qkv_parts = sb["qkv_buf"][: sk_q * T * nqkv].view(sk_q, T, nqkv)
        plan = plan or ops.verify_split_plan(self.Hkv, self.max_model_len)
        wn = self.wide_norm  # raw residual adds + the RMS row scale in the next GEMM (gammas folded), as _decode_step
        ssq = sb["ssq"]
        rn = lambda i: dict(rownorm=(ssq[i], self.eps)) if wn else {}  # noqa: E731
        lin = ops.linear if self.on_gpu else self._verify_linear_cpu
        kvs = self._kv_scales
        # the CPU twin of the residual-reduce step's SiLU GEMM takes its RMS row scale from the residual row itself
        rr_cpu = wn and not self.on_gpu and self.rr_decode and not self.rr_a8
        for l, lw in enumerate(w.layers):
            if l == 0 and wn:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=T, ss_out=ssq.view(-1),
                                ss_ld=ssq.shape[1], ss_nzero=2 * self.L)
            elif l == 0:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=T)
            elif wn:
                ops.res_add_ss(h, d_parts, xn, T, ssq[2 * l])
            else:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, parts=d_parts, rows=T)
            pre = {} if (self.on_gpu or l) else dict(pre=True)
            lin(xn, lw.wqkv, "f32", out=qkv_parts, splitk=sk_q, **rn(2 * l), **pre)
            kc, vc = self.kv[l, 0], self.kv[l, 1]
            ops.rope_append(qkv_parts, pos, sb["seq0"][Ts][:T], bt, self.cos, self.sin, q, kc, vc, self.H, self.Hkv,
                            kv_scales=kvs(l))
            if S == 1:
                ops.attn_verify(q, kc, vc, bt, pos[:1], self.H, self.Hkv, self.scale, attn, workspace=sb["attn_ws"],
                                plan=plan, kv_scales=kvs(l))
            else:  # (positions[:S] are the sequences' pos0: spec_draft copied them into pos[s * Ts])
                ops.attn_verify(q.view(S, Ts, self.H, self.D), kc, vc, bt, st[3], self.H, self.Hkv, self.scale, attn,
                                workspace=sb["attn_ws"], plan=plan, kv_scales=kvs(l))
            lin(attn, lw.wo, "f32", out=o_parts, splitk=sk_o)
            if wn:
                ops.res_add_ss(h, o_parts, xn, T, ssq[2 * l + 1])
            else:
                ops.add_rmsnorm(h, lw.mlp_norm, self.eps, xn, parts=o_parts, rows=T)
            lin(xn, lw.w_gate_up, "silu", out=act, **(dict(rownorm=(h, self.eps)) if rr_cpu else rn(2 * l + 1)))
            lin(act, lw.w_down, "f32", out=d_parts, splitk=sk_d)
        ops.add_rmsnorm(h, w.final_norm, self.eps, xn, parts=d_parts, rows=T)
        logits = sb["logits"][:T]
        lin(xn, w.lm_head, "f32", out=logits, splitk=1)
        if logprobs:  # the raw rows: ahead of the mask and the sampled commit, which rewrite ``logits`` in place
            ops.spec_logprob_scan(logits, Ts, self.lp_k[:S], st[4], st[1], self.lp_n0[:S], lp_ws)
        if guided:
            ops.dfa_mask_verify(logits, self.g_tok_off, self.g_tok_blob, self.g_cls, self.g_trans, self.g_accept,
                                self.g_dim, self.g_on, self.g_state, self.g_base, st[1], st[2], st[4], self.eos,
                                draft, self.g_spec[0] if S == 1 else self.g_spec[:S])
        if sample:
            ops.spec_sample_commit(logits, draft, sb["stats"][0] if S == 1 else sb["stats"][:S], self.hist[:S],
                                   self.penalty[:S], self.temperature[:S], self.top_k[:S], self.top_p[:S],
                                   self.seeds[:S], *st, self.eos, self.limit[:S], self.eos_on[:S],
                                   workspace=(sb["amax_part"], sb["cand"], sb["picks"]) if self.on_gpu else None,
                                   last_n=self.last_n[:S], presence=self.presence[:S], frequency=self.frequency[:S],
                                   min_p=self.min_p[:S])
        else:
            ops.spec_commit(logits, draft, sb["stats"][0] if S == 1 else sb["stats"][:S], *st, self.eos, self.limit[:S],
                            self.eos_on[:S], part=sb["amax_part"] if self.on_gpu else None)
        if guided:
            ops.dfa_spec_advance(self.g_on, self.g_state, self.g_spec[0] if S == 1 else self.g_spec[:S], st[1], Ts - 1)
        if logprobs:
            ops.spec_logprob_commit(Ts, self.lp_k[:S], self.lp_n0[:S], st[1], self.out_tokens, self.lp_tok, self.lp_ids,
                                    self.lp_top, lp_ws)

    def _verify_linear_cpu(self, x, wt, epi, out, splitk=1, rownorm=None, pre=False):
        """CPU twin of the verify step's GEMMs, one row at a time with the rounding points of the plain batch-1 step's
        own CPU twins, so that a verify row computes bit for bit what the plain step computes for that token (the GPU
        kernels scale the GEMM's output rows; ``ops.linear``'s CPU twin scales its bf16 input rows instead).  With the
        residual-reduce plain step (``rr_decode``): the product of the raw bf16 row, then the RMS row scale -- from the
        Q24 row sum for an f32 epilogue (as ``attn_decode(rownorm=)`` applies it to the slabs), from the f32 residual
        row itself for the SiLU epilogue (as ``linear_rr`` does; ``rownorm[0]`` is then the residual stream).
        Quantised weights: on the CPU their plain step runs neither e4m3 activations nor the residual-reduce step, so
        every projection is the plain ``ops.linear`` call of that row."""
        post = rownorm is not None and self.rr_decode and not self.rr_a8
        for i in range(x.shape[0]):
            row = x[i:i + 1]
            if not post or pre:  # (pre: layer 0's qkv, where the plain step makes this very call)
                kw = {} if rownorm is None else dict(rownorm=(rownorm[0][i:i + 1], rownorm[1]))
                y = ops.linear(row, wt, epi, **kw)
            elif epi == "f32":
                r = torch.rsqrt(ops.ss_float(rownorm[0][i:i + 1]) / wt.K + rownorm[1])
                y = ref.linear(row, wt.dense(), "f32").unsqueeze(0) * r.view(1, 1, 1)
            else:
                r = torch.rsqrt(rownorm[0][i].float().pow(2).sum() / wt.K + rownorm[1])
                y = ref.linear(row, wt.dense(), "f32") * r
                g, u = y.view(-1, 2, 16)[:, 0].reshape(1, -1), y.view(-1, 2, 16)[:, 1].reshape(1, -1)
                y = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
            (out[0, i] if (epi == "f32" and out.dim() == 3) else out[i]).copy_(y.reshape(-1))
        return out

    def spec_logits(self, S: int = 1) -> torch.Tensor:
        """[T, V] f32: the verify rows of the last verify step (the numerics check reads them).  After a guided and /
        or sampled verify step they are the rows as the commit read them: masked (-inf) and with the repetition
        penalty of a sampled step applied.  ``S`` > 1: [S, T, V], the rows of a step over S sequences."""
        T = self.spec_k() + 1
        rows = self._spec_bufs()["logits"][: S * T]
        return rows if S == 1 else rows.view(S, T, -1)

    def spec_lp_raw(self, S: int = 1) -> torch.Tensor:
        """[T, V] f32: the raw verify rows ``spec_logprob_scan`` kept in the last logprob verify step, as the lm_head
        wrote them (rows of sequences that asked and were not finished; other rows are stale).  ``S`` > 1: [S, T, V]."""
        T = self.spec_k() + 1
        rows = self._spec_lp_ws()[0][: S * T]
        return rows if S == 1 else rows.view(S, T, -1)

    def spec_drafts(self, S: int = 1) -> torch.Tensor:
        """[k] int32: the drafts of the last verify step (-1 = none).  ``S`` > 1: [S, k]."""
        k = self.spec_k()
        d = self._spec_bufs()["draft"][: S * k]
        return d if S == 1 else d.view(S, k)

    def decode_spec(self, steps: int, max_ctx: Optional[int] = None, guided: bool = False,
                    sample: bool = False, S: int = 1, logprobs: bool = False) -> None:
        """Run ``steps`` verify steps of the request in slot 0 (the analogue of ``decode`` at bucket 1); ``max_ctx``
        bounds pos0 + T during the run (picks the split plan's tier).  ``guided``: the variant with the regex mask of
        the verify rows, for a constrained request (its graph key is the unguided one with a trailing True).
        ``sample``: the variant that ends in the sampled commit, for a request that needs the sampler (its graph key
        is the greedy one with a trailing "sample"; the greedy graphs and their keys are untouched).
        ``S`` > 1: verify steps over the sequences of slots 0 .. S - 1 (``_verify_step(S=)``), one graph per (S, T,
        plan, forced buffer): the split plan is the decode plan of bucket S, the key the one-sequence key with S
        appended.  ``sample`` with ``S`` > 1 needs ``spec_batch_sampled``; its key is the greedy key, then "sample",
        then S.  ``guided`` with ``S`` > 1 needs ``spec_batch_guided``; its key is the one-sequence key, then True, then
        "sample" if sampled, then S.  ``logprobs``: the variant with the two logprob launches of the verify step, for
        runs in which a request asked (``spec_logprobs``): its key is the key above with a trailing "lp" (after S where
        present); every other key is unchanged."""
        assert self.spec_supported(), ("speculative decoding: TP = 1, spec_tokens > 0, bf16 weights and KV cache "
                                       "(or spec_quantized)")
        assert not guided or (self.guided and self.spec_guided), "guided verify steps need enable_guided() and spec_guided"
        assert not sample or self.spec_sampled, "sampled verify steps need spec_sampled"
        assert not logprobs or (self.spec_logprobs and self.logprobs), \
            "logprob verify steps need spec_logprobs and enable_logprobs()"
        assert S == 1 or (S <= self.spec_s() and (not guided or self.spec_batch_guided)
                          and (not sample or self.spec_batch_sampled)), \
            "verify steps over several sequences: S <= spec_batch (clamped), constrained only with " \
            "spec_batch_guided, sampled only with spec_batch_sampled"
        plan = tuple(self.ctx_plan(S, max_ctx))
        if not self.use_graphs:
            for _ in range(steps):
                self._verify_step(plan, guided, sample, S, logprobs)
            return
        key = ("spec", self.spec_k() + 1, plan, 0 if self._spec_forced is None else self._spec_forced.data_ptr())
        if guided:
            key += (True,)
        if sample:
            key += ("sample",)
        if S > 1:
            key += (S,)
        if logprobs:
            key += ("lp",)
        if key not in self.graphs:
            self._spec_bufs()
            if logprobs:
                self._spec_lp_ws()
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    self._verify_step(plan, guided, sample, S, logprobs)
            torch.cuda.current_stream(self.device).wait_stream(s)
            self.graphs[key] = g
        g = self.graphs[key]
        for _ in range(steps):
            g.replay()

    def spec_counts(self) -> tuple[int, int, int]:
        """(verify steps, drafted tokens, accepted tokens) since the runner was built, summed over the sequences (a
        device -> host read: call it after the sync a decode run ends with)."""
        a, b, c = (sum(col) for col in zip(*self.spec_row_counts())) if self._spec is not None else (0, 0, 0)
        return int(a), int(b), int(c)

    def spec_row_counts(self) -> list[list[int]]:
        """[S, 3]: ``spec_counts`` per sequence (row s = the verify steps that ran with slot s live)."""
        if self._spec is None:
            return [[0, 0, 0] for _ in range(self.spec_s())]
        return self._spec["stats"].tolist()

    # ------------------------------------------------------------------------------------ regex-constrained decoding
    def enable_guided(self, tok_off, tok_blob) -> None:
        """Allocate the device side of regex-constrained decoding: the tokenizer's byte table (CSR: ``tok_off`` int32
        [>= V + 1], ``tok_blob`` uint8; numpy or torch, uploaded once) and one DFA table row per slot -- cls 256 B,
        trans 64 KiB, accept 32 KiB -- plus g_on, the two state slots, g_base and the (S, C) dims (ops.dfa_mask), and
        g_spec: gen_len and the states of the T <= 8 verify rows of a guided verify step (ops.dfa_mask_verify), one row
        of 1 + 8 words per sequence of the step: one row, or 8 with ``spec_batch_guided`` (the one-sequence step uses
        row 0)."""
        off = torch.as_tensor(tok_off).to(torch.int64).reshape(-1)
        blob = torch.as_tensor(tok_blob).to(torch.uint8).reshape(-1)
        V = self.V
        if off.numel() < V + 1:  # ids the tokenizer does not know decode to nothing
            off = torch.cat([off, off[-1:].expand(V + 1 - off.numel())])
        off = off[: V + 1]
        if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) > blob.numel():
            raise ValueError("token byte table: offsets must start at 0, not decrease, and end inside the blob")
        if blob.numel() == 0:
            blob = torch.zeros(1, dtype=torch.uint8)
        dev, S = self.device, self.max_slots
        i32 = dict(dtype=torch.int32, device=dev)
        self.g_tok_off = off.to(torch.int32).to(dev)
        self.g_tok_blob = blob.to(dev)
        self.g_cls = torch.zeros(S, 256, dtype=torch.uint8, device=dev)
        self.g_trans = torch.full((S, ref.DFA_MAX_TABLE), -1, dtype=torch.int16, device=dev)
        self.g_accept = torch.zeros(S, ref.DFA_MAX_TABLE, dtype=torch.uint8, device=dev)
        self.g_dim = torch.zeros(S, 2, **i32)
        self.g_on = torch.zeros(S, **i32)
        self.g_state = torch.zeros(S, 2, **i32)
        self.g_base = torch.zeros(S, **i32)
        self.g_spec = torch.zeros(8 if self.spec_batch_guided else 1, 1 + 8, **i32)
        self.guided = True
        self.graphs.clear()

    def _dfa_mask(self, logits, gen_len, input_ids, finished, rows=None) -> None:
        ops.dfa_mask(logits, self.g_tok_off, self.g_tok_blob, self.g_cls, self.g_trans, self.g_accept, self.g_dim,
                     self.g_on, self.g_state, self.g_base, gen_len, input_ids, finished, self.eos, rows=rows)

    def _set_guided(self, entries: Sequence[dict], idx: torch.Tensor) -> None:
        """The constraint part of ``set_slots``: g_on, both state slots (= the request's start state), g_base (the
        row's gen_len at admission, which restarts at 0) and the dims of every admitted slot in one transfer, then the
        tables of the constrained ones."""
        n = len(entries)
        meta = torch.zeros(n, 6, dtype=torch.int32)  # on | state, state | base | S, C
        for i, e in enumerate(entries):
            dfa = e.get("dfa")
            sl = int(e["slot"])
            if dfa is None:
                self._g_host_on.discard(sl)
                continue
            self._g_host_on.add(sl)
            st = int(e.get("dfa_state", dfa.start))
            meta[i] = torch.tensor([1, st, st, 0, dfa.n_states, dfa.n_classes], dtype=torch.int32)
            sc = dfa.n_states * dfa.n_classes
            assert sc <= ref.DFA_MAX_TABLE and dfa.n_classes <= 256
            self.g_cls[sl].copy_(torch.from_numpy(dfa.cls))
            self.g_trans[sl, :sc].copy_(torch.from_numpy(dfa.trans.view("int16")))
            self.g_accept[sl, : dfa.n_states].copy_(torch.from_numpy(dfa.accept))
        mv = (meta.pin_memory() if self.on_gpu else meta).to(self.device, non_blocking=True)
        self.g_on.index_copy_(0, idx, mv[:, 0])
        self.g_state.index_copy_(0, idx, mv[:, 1:3])
        self.g_base.index_copy_(0, idx, mv[:, 3])
        self.g_dim.index_copy_(0, idx, mv[:, 4:6])

    # ------------------------------------------------------------------------------------ per-token logprobs
    def enable_logprobs(self) -> None:
        """Allocate the device side of per-token logprobs (kernels/logprobs.hip), per slot: lp_k (-1 = the row did not
        ask, else its top_logprobs K), lp_n0 (the record index the step's scan announces, -1 = none), the records
        lp_tok [S, max_new_cap], lp_ids / lp_top [S, max_new_cap, 20], the raw-row copy lp_raw [S, V] and the chunk
        workspaces.  ``logprobs_bytes()`` is what it costs."""
        if self.logprobs:
            return
        dev, S, V, cap, K = self.device, self.max_slots, self.V, self.max_new_cap, ops.LOGPROB_KMAX
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.lp_k = torch.full((S,), -1, **i32)
        self.lp_n0 = torch.full((S,), -1, **i32)
        self.lp_tok = torch.zeros(S, cap, **f32)
        self.lp_ids = torch.full((S, cap, K), -1, **i32)
        self.lp_top = torch.zeros(S, cap, K, **f32)
        self.lp_raw = torch.zeros(S, V, **f32)
        self.lp_ws = ops.logprob_workspace(S, V, dev)
        self.logprobs = True
        if self.spec_logprobs:
            self._spec_lp_ws()

    def _spec_lp_ws(self) -> tuple:
        """The spec-side raw rows and chunk workspace of logprob verify steps (32 rows; ``ops.spec_logprob_workspace``):
        allocated only when both ``enable_logprobs()`` and ``spec_logprobs`` hold."""
        assert self.logprobs and self.spec_logprobs, "logprob verify steps need spec_logprobs and enable_logprobs()"
        ws = self.__dict__.get("spec_lp_ws")
        if ws is None:
            ws = self.spec_lp_ws = ops.spec_logprob_workspace(self.V, self.device)
        return ws

    def logprobs_bytes(self) -> int:
        """Device bytes ``enable_logprobs`` holds (records + raw rows + chunk workspaces; with ``spec_logprobs`` the
        32 raw rows and chunk workspace of the verify step too)."""
        if not self.logprobs:
            return 0
        ts = (self.lp_k, self.lp_n0, self.lp_tok, self.lp_ids, self.lp_top, self.lp_raw, *self.lp_ws,
              *(self.__dict__.get("spec_lp_ws") or ()), *(self.__dict__.get("prompt_lp_ws") or ()))
        return sum(t.numel() * t.element_size() for t in ts)

    def _logprob_scan(self, logits, lp_k, finished, gen_len, lp_n0) -> None:
        ops.logprob_scan(logits, lp_k, finished, gen_len, self.lp_raw, lp_n0, workspace=self.lp_ws)

    # ------------------------------------------------------------------------------------ embeddings
    def enable_embeddings(self) -> None:
        """Allocate the device side of embeddings (kernels/embed.hip), per slot: the pooled sum emb_acc [S, d] f32 that
        the prefills of a chunked prompt accumulate into (never cleared: a segment that starts at position 0 starts its
        sum from +0) and the normalised vector emb_out [S, d] f32; plus the per-call row scales, grown on demand."""
        if self.embeddings:
            return
        assert self.tp is None or self.tp.size == 1, "embeddings are not served under tensor parallelism"
        f32 = dict(dtype=torch.float32, device=self.device)
        self.emb_acc = torch.zeros(self.max_slots, self.d, **f32)
        self.emb_out = torch.zeros(self.max_slots, self.d, **f32)
        self.emb_rs = torch.zeros(256, **f32)
        self.embeddings = True

    def _embed_rows(self, h, d_parts, tsd, cud, meta_d, host) -> None:
        """The three embedding launches of one prefill call, on the prefill's stream: row scales of the pooled rows, the
        pool into emb_acc, and the final vectors of the inputs that end in this call into emb_out."""
        T = h.shape[0]
        if self.emb_rs.numel() < T:
            self.emb_rs = torch.zeros(max(T, 2 * self.emb_rs.numel()), dtype=torch.float32, device=self.device)
        ops.embed_rowscale(h, d_parts, tsd, cud, meta_d, self.eps, self.emb_rs, host=host)
        ops.embed_pool(h, d_parts, cud, meta_d, self.emb_rs, self.w.final_norm, self.emb_acc, host=host)
        ops.embed_finish(meta_d, self.emb_acc, self.emb_out, host=host)

    def embeddings_of(self, slots: Sequence[int]) -> torch.Tensor:
        """The vectors emb_out[slots] as a host [n, d] f32 tensor: one device -> host copy."""
        idx = torch.tensor(list(slots), dtype=torch.long, device=self.device)
        return self.emb_out.index_select(0, idx).cpu()

    # prompt-token logprobs: teacher-forced scoring of prefill rows (kernels/logprobs.hip, the prompt pair)
    def _prompt_lp_ws(self, rows: int) -> tuple:
        """The chunk workspace of one lm_head tile of scored rows (``ops.prompt_logprob_workspace``): allocated by the
        first prefill that scores, regrown if ``score_tile_rows`` was raised since."""
        ws = self.__dict__.get("prompt_lp_ws")
        nch = (self.V + ops.LOGPROB_CHUNK - 1) // ops.LOGPROB_CHUNK
        if ws is None or ws[0].numel() < rows * nch * 2:
            ws = self.prompt_lp_ws = ops.prompt_logprob_workspace(rows, self.V, self.device)
        return ws

    def _prompt_logprob_scan(self, logits, targets, row_k, any_k: bool = True) -> None:
        ops.prompt_logprob_scan(logits, targets, row_k, workspace=self._prompt_lp_ws(logits.shape[0]), any_k=any_k)

    def _score_rows(self, xs, targets, row_k, any_k: bool) -> tuple:
        """Records of R scored prefill rows: ``xs`` [R, d] are their final-norm states, ``targets`` / ``row_k`` [R] the
        token and the K of each.  The rows go through the lm_head in tiles of at most ``score_tile_rows``, each tile
        followed by the scan / commit pair over the tile's logits.  -> (tok f32 [R], ids int32 [R, 20], top f32
        [R, 20]) on the device; nothing is synchronised."""
        R, K, dev = xs.shape[0], ops.LOGPROB_KMAX, self.device
        tok = torch.zeros(R, dtype=torch.float32, device=dev)
        ids = torch.full((R, K), -1, dtype=torch.int32, device=dev)
        top = torch.zeros(R, K, dtype=torch.float32, device=dev)
        tile = max(1, int(self.score_tile_rows))
        ws = self._prompt_lp_ws(min(tile, R))
        # a quantised lm_head is dequantised once for all the tiles of more than 64 rows, not once per tile
        wf = ops.tile_weight(self.w.lm_head, dev) if min(tile, R) > 64 else None
        for a in range(0, R, tile):
            b = min(R, a + tile)
            logits = ops.linear(xs[a:b], self.w.lm_head, "f32", splitk=1, wf=wf).view(b - a, self.V)
            self._prompt_logprob_scan(logits, targets[a:b], row_k[a:b], any_k)
            ops.prompt_logprob_commit(logits, targets[a:b], row_k[a:b], tok[a:b], ids[a:b], top[a:b], workspace=ws,
                                      any_k=any_k)
        return tok, ids, top

    def prompt_logprobs_of(self, recs: Sequence[tuple]) -> list[list[tuple]]:
        """``recs``: (records of one ``prefill`` call, first row, rows, K) per wanted run of rows.  One device -> host
        transfer; per run a list of (logprob, [(token id, logprob)] * K), the shape ``logprobs_of_many`` gives."""
        if not recs:
            return []
        KM = ops.LOGPROB_KMAX
        pack = torch.cat([torch.cat([r[0][a:a + n].unsqueeze(-1), r[2][a:a + n], r[1][a:a + n].view(torch.float32)],
                                    dim=-1) for r, a, n, _ in recs]).cpu()
        tok, top = pack[:, 0].tolist(), pack[:, 1:1 + KM].tolist()
        ids = pack[:, 1 + KM:].contiguous().view(torch.int32).tolist()
        out, o = [], 0
        for _, _, n, k in recs:
            out.append([(tok[o + j], list(zip(ids[o + j][:k], top[o + j][:k]))) for j in range(n)])
            o += n
        return out

    def logprobs_of_many(self, slots: Sequence[int], lo: Sequence[int], hi: Sequence[int]) -> list[list[tuple]]:
        """Records [lo[i], hi[i]) of slot row ``slots[i]`` in one device -> host transfer: per row a list of
        (logprob, [(token id, logprob)] * K) with K the row's top_logprobs."""
        if not slots:
            return []
        a, m = min(lo), max(hi)
        if m <= a:
            return [[] for _ in slots]
        idx = torch.tensor(list(slots), dtype=torch.long, device=self.device)
        K = ops.LOGPROB_KMAX
        pack = torch.cat([self.lp_tok[:, a:m].index_select(0, idx).unsqueeze(-1),
                          self.lp_top[:, a:m].index_select(0, idx),
                          self.lp_ids[:, a:m].index_select(0, idx).view(torch.float32)], dim=-1)
        ks = self.lp_k.index_select(0, idx).view(torch.float32)
        host = torch.cat([pack.reshape(-1), ks]).cpu()
        n = len(slots)
        kh = host[-n:].view(torch.int32).tolist()
        rec = host[:-n].view(n, m - a, 1 + 2 * K)
        tok, top = rec[..., 0].tolist(), rec[..., 1:1 + K].tolist()
        ids = rec[..., 1 + K:].contiguous().view(torch.int32).tolist()
        out = []
        for i in range(n):
            k = max(0, kh[i])
            out.append([(tok[i][j - a], list(zip(ids[i][j - a][:k], top[i][j - a][:k])))
                        for j in range(lo[i], hi[i])])
        return out

    # ------------------------------------------------------------------------------------ slots
    def set_slot(self, slot: int, blocks: Sequence[int], limit: int, temperature: float = 0.0, top_k: int = 40,
                 top_p: float = 0.9, seed: int = 0, eos_on: bool = True, repeat_penalty: float = 1.0,
                 repeat_last_n: int = REPEAT_WINDOW, prompt_ids: Sequence[int] = (), defer_table: bool = False,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, min_p: float = 0.0) -> None:
        """``defer_table``: the slot's block table stays out of the decode-visible table until its prompt's
        final prefill chunk commits (chunked-prefill interleave: decode runs in between must not append
        the idle row's k/v into the blocks the prompt is being written to)."""
        self.set_slots([dict(slot=slot, blocks=blocks, limit=limit, temperature=temperature, top_k=top_k, top_p=top_p,
                             seed=seed, eos_on=eos_on, repeat_penalty=repeat_penalty, repeat_last_n=repeat_last_n,
                             prompt_ids=prompt_ids, defer_table=defer_table, presence_penalty=presence_penalty,
                             frequency_penalty=frequency_penalty, min_p=min_p)])

    def set_slots(self, entries: Sequence[dict]) -> None:
        """``set_slot`` for every admitted request at once (keyword dicts of set_slot's arguments): the per-slot
        parameters travel host -> device in ONE pinned int32 + one f32 + one int64 transfer and land with one
        index_copy per state tensor, instead of ~11 tiny copies / fills per slot (a 32-request bench round's
        admission was ~350 small launches of host time with the GPU idle)."""
        if not entries:
            return
        n, W, mb = len(entries), REPEAT_WINDOW, self.max_blocks
        # speculative decoding: the context history (its length, then the tokens) of every slot < spec_batch rides in
        # the same transfer
        SB = self.spec_s() if (self.spec_tokens > 0 and self.spec_supported()) else 0
        sx = (1 + self.max_model_len) if any(int(e["slot"]) < SB for e in entries) else 0
        ints = torch.zeros(n, mb + 5 + sx, dtype=torch.int32)  # block-table row | limit top_k eos_on last_n visible
        flts = torch.zeros(n, 6, dtype=torch.float32)     # temperature top_p penalty presence frequency min_p
        seeds = torch.zeros(n, dtype=torch.int64)
        hist = None
        # a request with any of the three penalties reads the ring from its first token on
        ringed = [float(e.get("repeat_penalty", 1.0)) != 1.0 or float(e.get("presence_penalty", 0.0)) != 0.0 or
                  float(e.get("frequency_penalty", 0.0)) != 0.0 for e in entries]
        for i, e in enumerate(entries):
            blocks = list(e["blocks"])
            ints[i, : len(blocks)] = torch.tensor(blocks, dtype=torch.int32)
            last_n = max(0, min(int(e.get("repeat_last_n", REPEAT_WINDOW)), W))
            ints[i, mb:mb + 5] = torch.tensor([min(int(e["limit"]), self.max_new_cap), int(e.get("top_k", 40)),
                                               1 if e.get("eos_on", True) else 0, last_n,
                                               0 if e.get("defer_table", False) else 1], dtype=torch.int32)
            if sx and int(e["slot"]) < SB:
                pids = list(e.get("prompt_ids", ()))[: self.max_model_len]
                ints[i, mb + 5] = len(pids)
                ints[i, mb + 6: mb + 6 + len(pids)] = torch.tensor(pids, dtype=torch.int32)
            flts[i] = torch.tensor([float(e.get("temperature", 0.0)), float(e.get("top_p", 0.9)),
                                    float(e.get("repeat_penalty", 1.0)), float(e.get("presence_penalty", 0.0)),
                                    float(e.get("frequency_penalty", 0.0)), float(e.get("min_p", 0.0))])
            seeds[i] = int(e.get("seed", 0))
            if ringed[i]:  # seed the ring with the prompt's last tokens (p -> p % W)
                if hist is None:
                    hist = torch.full((n, W), -1, dtype=torch.int32)
                ids = list(e.get("prompt_ids", ()))
                for p in range(max(0, len(ids) - W), len(ids)):
                    hist[i, p % W] = int(ids[p])
        if self.on_gpu:
            ints, flts, seeds = ints.pin_memory(), flts.pin_memory(), seeds.pin_memory()
        dv = ints.to(self.device, non_blocking=True)
        fv = flts.to(self.device, non_blocking=True)
        sv = seeds.to(self.device, non_blocking=True)
        slots = [int(e["slot"]) for e in entries]
        idx = torch.tensor(slots, dtype=torch.long).to(self.device, non_blocking=True)
        visible = ints[:, mb + 4].tolist()
        for i, sl in enumerate(slots):
            if visible[i]:
                self._pending_bt.pop(sl, None)
            else:
                self._pending_bt[sl] = dv[i, :mb].clone()
        self.block_tables.index_copy_(0, idx, dv[:, :mb] * dv[:, mb + 4:mb + 5])  # deferred rows stay zero
        if sx:
            sb = self._spec_bufs()
            for i, sl in enumerate(slots):
                if sl < SB:
                    sb["ctx_len"][sl:sl + 1].copy_(dv[i, mb + 5:mb + 6])
                    sb["ctx"][sl:sl + 1].copy_(dv[i:i + 1, mb + 6:])
        self.limit.index_copy_(0, idx, dv[:, mb])
        self.top_k.index_copy_(0, idx, dv[:, mb + 1])
        self.eos_on.index_copy_(0, idx, dv[:, mb + 2])
        self.last_n.index_copy_(0, idx, dv[:, mb + 3])
        self.temperature.index_copy_(0, idx, fv[:, 0])
        self.top_p.index_copy_(0, idx, fv[:, 1])
        self.penalty.index_copy_(0, idx, fv[:, 2])
        self.presence.index_copy_(0, idx, fv[:, 3])
        self.frequency.index_copy_(0, idx, fv[:, 4])
        self.min_p.index_copy_(0, idx, fv[:, 5])
        self.seeds.index_copy_(0, idx, sv)
        if self.logprobs:  # lp_k per entry: -1 = the request did not ask
            lk = torch.tensor([int(e.get("lp_k", -1)) for e in entries], dtype=torch.int32)
            self.lp_k.index_copy_(0, idx, (lk.pin_memory() if self.on_gpu else lk).to(self.device, non_blocking=True))
        elif any(int(e.get("lp_k", -1)) >= 0 for e in entries):
            raise RuntimeError("a request asks for logprobs but the runner was built without them")
        if self.guided:
            self._set_guided(entries, idx)
        elif any(e.get("dfa") is not None for e in entries):
            raise RuntimeError("a request carries a regex but the runner was built without guided decoding")
        if hist is not None:
            hv = hist.pin_memory() if self.on_gpu else hist
            hsel = torch.tensor([i for i in range(n) if ringed[i]], dtype=torch.long)
            self.hist.index_copy_(0, idx[hsel.to(self.device)], hv[hsel].to(self.device, non_blocking=True))

    def extend_tables(self, entries: Sequence[tuple]) -> None:
        """Lazy KV growth (engine._grow_kv): rewrite the decode-visible block-table rows of running slots,
        ``entries`` = [(slot, blocks)], whose tables gained blocks -- one pinned transfer + one index_copy for all
        of them, between decode runs (a captured graph reads the table from device memory at every replay)."""
        if not entries:
            return
        mb = self.max_blocks
        rows = torch.zeros(len(entries), mb, dtype=torch.int32)
        for i, (_, blocks) in enumerate(entries):
            assert len(blocks) <= mb, "block table longer than max_model_len"
            rows[i, : len(blocks)] = torch.tensor(list(blocks), dtype=torch.int32)
        if self.on_gpu:
            rows = rows.pin_memory()
        idx = torch.tensor([int(sl) for sl, _ in entries], dtype=torch.long)
        for sl, _ in entries:
            assert int(sl) not in self._pending_bt, "growing a slot whose prompt is still being prefilled"
        self.block_tables.index_copy_(0, idx.to(self.device, non_blocking=True), rows.to(self.device, non_blocking=True))

    def copy_kv_blocks(self, pairs: Sequence[tuple]) -> None:
        """Prefix cache: fork cached KV blocks, ``pairs`` = [(src, dst)] block ids of this runner's arena
        (ops.kv_copy_blocks).  Runs eagerly on the engine's stream, which orders it before the prefill that writes
        the rest of dst and attends to it, and before any later write of a src that is evicted meanwhile."""
        if pairs:
            ops.kv_copy_blocks(self.kv, self.kv_scale, pairs)

    def shift_slots(self, entries: Sequence[tuple]) -> None:
        """Context shift (engine.LLMEngine._shift_contexts): ``entries`` = [(slot, moves, blocks, discard)], the
        scheduler's plan for each running slot that drops ``discard`` tokens of its cache.  One ``ops.kv_shift``
        (on the fp8 cache ``ops.kv_shift8``) launch moves and re-rotates the rows of every entry; then each slot's decode-visible block-table row is
        rewritten (zero-filled past its end) and its position lowered by ``discard`` -- one pinned transfer for the
        rows and the deltas.  All of it runs on the engine's stream between decode runs, so a captured graph reads
        the shifted state at its next replay."""
        if not entries:
            return
        mb = self.max_blocks
        for sl, _, blocks, _ in entries:
            assert int(sl) not in self._pending_bt, "shifting a slot whose prompt is still being prefilled"
            assert len(blocks) <= mb, "block table longer than max_model_len"
        moves = [m for _, moves, _, _ in entries for m in moves]
        if self.kv_fp8:
            ops.kv_shift8(self.kv, self.kv_scale, moves, self.cos, self.sin)
        else:
            ops.kv_shift(self.kv, self.kv_scale, moves, self.cos, self.sin)
        rows = torch.zeros(len(entries), mb + 1, dtype=torch.int32)
        for i, (_, _, blocks, discard) in enumerate(entries):
            rows[i, : len(blocks)] = torch.tensor(list(blocks), dtype=torch.int32)
            rows[i, mb] = -int(discard)
        if self.on_gpu:
            rows = rows.pin_memory()
        idx = torch.tensor([int(e[0]) for e in entries], dtype=torch.long).to(self.device, non_blocking=True)
        dv = rows.to(self.device, non_blocking=True)
        self.block_tables.index_copy_(0, idx, dv[:, :mb])
        self.positions.index_add_(0, idx, dv[:, mb])

    def set_eos(self, ids: Sequence[int]) -> None:
        """Replace the stop-token set (same length keeps captured graphs valid; otherwise recapture)."""
        ids = list(ids) or [-1]
        if len(ids) != self.eos.numel():
            self.graphs.clear()
            self.eos = torch.tensor(ids, dtype=torch.int32, device=self.device)
        else:
            self.eos.copy_(torch.tensor(ids, dtype=torch.int32))
        self.eos_list = ids

    def end_slot(self, slot: int) -> None:
        """Mark a running row finished where it stands (a context shift the arena could not serve): the decode graphs
        skip it and the engine's next read of the finished flags retires it with the tokens it has."""
        self.finished[slot] = 1

    def release_slot(self, slot: int) -> None:
        self._pending_bt.pop(slot, None)
        self._g_host_on.discard(slot)
        self.finished[slot] = 1
        self.positions[slot] = 0
        self.gen_len[slot] = 0
        if self.logprobs:
            self.lp_k[slot] = -1
        self.block_tables[slot].zero_()

    # ------------------------------------------------------------------------------------ prefill
    def prefill(self, seqs: list[tuple[int, Sequence[int], int]], sample_any: bool = False,
                score: Optional[Sequence] = None, embed: Optional[Sequence] = None):
        """Prefill ``seqs`` = [(slot, token_ids, start_pos)] and commit each first token into its slot.

        ``start_pos`` > 0 continues a chunked prefill (the cache already holds positions < start_pos);
        only the final chunk of a prompt should be passed with ``commit=True`` semantics — a chunk whose
        prompt continues is passed through ``prefill_chunk``.

        ``score`` (prompt-token logprobs, ``enable_logprobs``): per sequence None or (first scored row, K, targets) --
        rows first .. first + len(targets) - 1 of the sequence's tokens in this call are scored, row first + k against
        ``targets[k]`` (the token that follows it in the prompt: the next token of this call, or for its last row the
        first token of the next chunk, which the caller knows).  Returns None, or the call's device records
        (tok, ids, top, [(sequence index, first record row, rows)]) for ``prompt_logprobs_of``; no host sync.

        ``embed`` (embeddings, ``enable_embeddings``): per sequence None or (pooling "mean" | "last", the input's total
        tokens, whether this call holds the input's last row).  The sequence's final-norm rows of this call are pooled
        into its slot's accumulator (a segment with start_pos 0 restarts it), and the call with the last row leaves
        the normalised vector in ``emb_out[slot]`` for ``embeddings_of``; no host sync.
        """
        return self._prefill(seqs, commit=True, sample_any=sample_any, score=score, embed=embed)

    def prefill_chunk(self, seqs: list[tuple[int, Sequence[int], int]], score: Optional[Sequence] = None,
                      embed: Optional[Sequence] = None):
        return self._prefill(seqs, commit=False, score=score, embed=embed)

    def _prefill(self, seqs, commit: bool, sample_any: bool = False, score: Optional[Sequence] = None,
                 embed: Optional[Sequence] = None):
        dev, w, d = self.device, self.w, self.d
        n = len(seqs)
        lens = [len(t) for _, t, _ in seqs]
        T = sum(lens)
        cu = [0]
        for x in lens:
            cu.append(cu[-1] + x)
        toks, pos, tseq = [], [], []
        for i, (_, t, p0) in enumerate(seqs):
            toks.extend(int(x) for x in t)
            pos.extend(range(p0, p0 + len(t)))
            tseq.extend([i] * len(t))
        ctx = [p0 + len(t) for _, t, p0 in seqs]
        slots = [s for s, _, _ in seqs]
        # scored rows (prompt-token logprobs): packed row index, target token and K of each, known before any launch
        srow, stgt, sk, smeta = [], [], [], []
        for i, sc in enumerate(score or ()):
            if sc is None or not len(sc[2]):
                continue
            first, K, tg = int(sc[0]), int(sc[1]), sc[2]
            assert self.logprobs, "a sequence asks for prompt logprobs but the runner was built without logprobs"
            assert self.tp is None or self.tp.size == 1, "prompt logprobs are not served under tensor parallelism"
            assert 0 <= first and first + len(tg) <= lens[i] and 0 <= K <= ops.LOGPROB_KMAX, (first, len(tg), lens[i], K)
            smeta.append((i, len(srow), len(tg)))
            srow.extend(range(cu[i] + first, cu[i] + first + len(tg)))
            stgt.extend(int(x) for x in tg)
            sk.extend([K] * len(tg))
        R = len(srow)
        # embedding sequences: meta [5, n] (emode, estart, eslot, efinal, ecount) behind the scored rows' words, only
        # when some sequence of this call embeds
        emeta = None
        if embed is not None and any(e is not None for e in embed):
            assert self.embeddings, "a sequence asks for an embedding but the runner was built without embeddings"
            assert self.tp is None or self.tp.size == 1, "embeddings are not served under tensor parallelism"
            assert len(embed) == n, (len(embed), n)
            emeta = [[0] * n for _ in range(5)]
            for i, e in enumerate(embed):
                if e is not None:
                    emeta[0][i], emeta[1][i], emeta[2][i] = ops.EMBED_MODES[e[0]], int(seqs[i][2]), int(slots[i])
                    emeta[3][i], emeta[4][i] = int(bool(e[2])), int(e[1])
        host = torch.tensor(toks + pos + tseq + cu + ctx + [c - 1 for c in cu[1:]] + srow + stgt + sk +
                            (sum(emeta, []) if emeta is not None else []), dtype=torch.int32)
        if self.on_gpu:
            host = host.pin_memory()
        dv = host.to(dev, non_blocking=True)
        o = 0
        ids = dv[o:o + T]; o += T
        posd = dv[o:o + T]; o += T
        tsd = dv[o:o + T]; o += T
        cud = dv[o:o + n + 1]; o += n + 1
        ctxd = dv[o:o + n]; o += n
        last = dv[o:o + n]
        if R:  # the final norm gathers the scored rows behind (commit) or instead of (chunk) the last rows, in one launch
            last = dv[o:o + n + R] if commit else dv[o + n:o + n + R]
            tgt_d, k_d = dv[o + n + R:o + n + 2 * R], dv[o + n + 2 * R:o + n + 3 * R]
        meta_d = dv[o + n + 3 * R:o + n + 3 * R + 5 * n].view(5, n) if emeta is not None else None
        slot_t = torch.tensor(slots, dtype=torch.long, device=dev)
        bt = self.block_tables.index_select(0, slot_t)
        for i, sl in enumerate(slots):  # deferred tables: prefill writes through them; the commit publishes
            pend = self._pending_bt.get(sl)
            if pend is not None:
                bt[i].copy_(pend)
                if commit:
                    self.block_tables[sl].copy_(pend)
                    del self._pending_bt[sl]
        work = None
        self._cu_host = cu  # host offsets: the prefill attention kernel choice (ops._prefill_kernel)
        # fp8 cache: the bf16 scratch every layer's prefill attention widens its blocks into (ops.kv8_scratch)
        self._kv8_scratch = ops.kv8_scratch(ctx, self.Hkv, dev) if (self.kv_fp8 and self.on_gpu) else None
        if self.on_gpu:
            work = ops.prefill_plan(cu, ctx=ctx, heads=self.H, device=dev)

        tps = self.tp.size if self.tp is not None else 1
        if self.seq_parallel and tps > 1 and T >= self.sp_min_tokens:
            assert emeta is None, "embeddings are not served under tensor parallelism"
            xl = self._prefill_layers_sp(T, ids, posd, tsd, bt, cud, ctxd, last, work, n, commit)
        else:
            # host path: a call that pools embeddings computes every row on its own (ops/reference.py row_stable), so
            # that a vector is the same bits however the call was packed or the prompt chunked
            with ref.row_stable(emeta is not None and not self.on_gpu):
                xl, h, d_parts = self._prefill_layers(T, ids, posd, tsd, bt, cud, ctxd, last, work,
                                                      last.numel() if R else n, commit or R > 0)
            if emeta is not None:
                self._embed_rows(h, d_parts, tsd, cud, meta_d, (cu, emeta))
        recs = None
        if R:
            recs = (*self._score_rows(xl[-R:], tgt_d, k_d, max(sk) > 0), smeta)
            xl = xl[:n]
        if not commit:
            return recs
        logits = self._lm_head(xl, n)
        # commit the first generated token of each sequence into its slot row
        i32 = dict(dtype=torch.int32, device=dev)
        out_t = torch.zeros(n, self.max_new_cap, **i32)
        gl = torch.zeros(n, **i32)
        iid = torch.zeros(n, **i32)
        pp = ctxd - 1
        fin = torch.zeros(n, **i32)
        lim = self.limit.index_select(0, slot_t)
        eon = self.eos_on.index_select(0, slot_t)
        lp = self.logprobs and commit
        if lp:  # record 0 of every sequence that asked: the same two ops, eagerly, on the gathered rows
            assert n <= self.max_slots, "one sequence per slot: lp_raw and the chunk workspaces hold max_slots rows"
            lpk = self.lp_k.index_select(0, slot_t)
            lpn = torch.full((n,), -1, **i32)
            self._logprob_scan(logits, lpk, fin, gl, lpn)
        if self.guided and any(sl in self._g_host_on for sl in slots):
            # the first generated token obeys the constraint too: gl = 0 = g_base, so each row reads the start state
            # the admission wrote; the table rows are the sequences' slots
            self._dfa_mask(logits, gl, iid, fin, rows=slot_t.to(torch.int32))
        if sample_any:
            hist = self.hist.index_select(0, slot_t)
            ops.sample_commit(logits, hist, self.penalty.index_select(0, slot_t),
                              self.temperature.index_select(0, slot_t),
                              self.top_k.index_select(0, slot_t), self.top_p.index_select(0, slot_t),
                              self.seeds.index_select(0, slot_t), out_t, gl, iid, pp, fin, self.eos, lim, eon,
                              last_n=self.last_n.index_select(0, slot_t),
                              presence=self.presence.index_select(0, slot_t),
                              frequency=self.frequency.index_select(0, slot_t),
                              min_p=self.min_p.index_select(0, slot_t))
            self.hist.index_copy_(0, slot_t, hist)
        else:
            ops.argmax_commit(logits, out_t, gl, iid, pp, fin, self.eos, lim, eon)
        if lp:  # every row committed its token 0; the records are one entry wide
            K = ops.LOGPROB_KMAX
            t0 = torch.zeros(n, 1, dtype=torch.float32, device=dev)
            i0 = torch.full((n, 1, K), -1, **i32)
            p0 = torch.zeros(n, 1, K, dtype=torch.float32, device=dev)
            ops.logprob_commit(self.lp_raw, lpk, lpn, gl, out_t[:, :1].contiguous(), t0, i0, p0, n, workspace=self.lp_ws)
            self.lp_tok[:, 0].index_copy_(0, slot_t, t0[:, 0])
            self.lp_ids[:, 0].index_copy_(0, slot_t, i0[:, 0])
            self.lp_top[:, 0].index_copy_(0, slot_t, p0[:, 0])
        self.out_tokens.index_copy_(0, slot_t, out_t)
        self.gen_len.index_copy_(0, slot_t, gl)
        self.input_ids.index_copy_(0, slot_t, iid)
        self.positions.index_copy_(0, slot_t, pp + fin if self.park_past_prompt else pp)
        self.finished.index_copy_(0, slot_t, fin)
        return recs

    def _prefill_layers(self, T, ids, posd, tsd, bt, cud, ctxd, last, work, n, commit):
        """Prefill layer stack with full-sequence residuals; returns (xl, h, d_parts): xl the normalised states of the n
        rows ``last`` names (each sequence's last row, and / or the rows a prompt-logprob request scores), None when not
        ``commit`` (a chunk that neither commits a token nor scores a row); h [T, d] the f32 residual stream and d_parts
        the last down projection's split-K slabs still to be added to it (None: already in h), which the embedding
        pool reads (``_embed_rows``)."""
        dev, w, d = self.device, self.w, self.d
        f32 = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=torch.bfloat16, device=dev)
        h = torch.empty(T, d, **f32)
        qkv = torch.empty(T, (self.H + 2 * self.Hkv) * self.D, **bf)
        q = torch.empty(T, self.H, self.D, **bf)
        sk_o = self._splitk(T, self.H * self.D)
        sk_d = self._splitk(T, self.ffn_l)
        d_parts = None
        # TP = 1: o / down accumulate into the f32 residual in the stream-K GEMM's epilogue (ops.linear_res), so the
        # norms after them read h alone (no f32 slab written by the GEMM and read back by the add)
        # (stream-K tile kernels: T > 64 rows; shorter chunks take the skinny split-K GEMMs, whose f32 slabs the next
        # add_rmsnorm sums).  The round-5 norm-free variant (the down epilogue also writing bf16(h) + row sums, the qkv
        # GEMM scaling its rows) measured a tie and was removed in round 6 (ARCHITECTURE.md section 4)
        tp1 = self.tp is None or self.tp.size == 1
        res_o = tp1 and T > 64 and ops.res_supported(w.layers[0].wo)
        res_d = tp1 and T > 64 and ops.res_supported(w.layers[0].w_down)
        # fragment-major activations (ops.to_xfrag, ceil(T / 16) row tiles): the norms, the attention and the gate_up
        # SiLU epilogue write every stream-K GEMM input in the order the GEMM stages it, one contiguous KiB per MFMA
        # fragment (ops.PREFILL_XF)
        xfp = res_o and res_d and ops.PREFILL_XF
        rows = T if xfp else None
        mt16 = 16 * ops.xfrag_tiles(T)
        xn = torch.empty(mt16 * d, **bf) if xfp else torch.empty(T, d, **bf)
        attn = torch.empty(mt16 * self.H * self.D, **bf) if xfp else torch.empty(T, self.H * self.D, **bf)
        act = torch.empty(mt16 * (w.layers[0].w_gate_up.N // 2), **bf) if xfp else None
        for l, lw in enumerate(w.layers):
            if l == 0:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, ids=ids, emb=w.embed, rows=rows, xf=xfp)
            else:
                ops.add_rmsnorm(h, lw.attn_norm, self.eps, xn, parts=d_parts, write_h=not res_d, rows=rows, xf=xfp)
            self._prefill_attention(xn, lw, l, qkv, q, attn, posd, tsd, bt, cud, ctxd, work, T, xfp)
            if res_o:
                ops.linear_res(attn, lw.wo, h, rows=rows)
                ops.add_rmsnorm(h, lw.mlp_norm, self.eps, xn, write_h=False, rows=rows, xf=xfp)
            else:
                o_parts = ops.linear(attn, lw.wo, "f32", splitk=sk_o)
                if not self.on_gpu:
                    o_parts = o_parts.view(1, T, d)
                o_parts = self._reduce_parts(o_parts)
                ops.add_rmsnorm(h, lw.mlp_norm, self.eps, xn, parts=o_parts)
            sk_g = self._splitk(T, self.d, lw.w_gate_up.N)
            if xfp:
                ops.linear_sk(xn, lw.w_gate_up, "silu", act, rows=T, xf_out=True)
            elif sk_g > 1:  # small tile grid: f32 split-K slabs, then silu(gate) * up over the slabs
                act = ops.silu_parts(ops.linear(xn, lw.w_gate_up, "f32", splitk=sk_g),
                                     torch.empty(T, lw.w_gate_up.N // 2, **bf))
            else:
                act = ops.linear(xn, lw.w_gate_up, "silu")
            if res_d:
                ops.linear_res(act, lw.w_down, h, rows=rows)
                d_parts = None
            else:
                d_parts = ops.linear(act, lw.w_down, "f32", splitk=sk_d)
                if not self.on_gpu:
                    d_parts = d_parts.view(1, T, d)
                d_parts = self._reduce_parts(d_parts)
        if not commit:
            return None, h, d_parts
        xl = torch.empty(n, d, **bf)
        ops.add_rmsnorm(h, w.final_norm, self.eps, xl, parts=d_parts, row_idx=last, write_h=False)
        return xl, h, d_parts

    def _prefill_attention(self, xn, lw, l, qkv, q, attn, posd, tsd, bt, cud, ctxd, work, T, xf=False):
        """qkv projection + RoPE + KV-cache append + causal attention of one prefill layer.  xf: xn and attn are
        flat fragment-major buffers of T rows (``_prefill_layers``)."""
        kc, vc = self.kv[l, 0], self.kv[l, 1]
        kvs = self._kv_scales(l)
        rows = T if xf else None
        out = attn if xf else attn.view(T, self.H, self.D)
        akw = dict(work=work, cu_list=self._cu_host, kv_scales=kvs, kv8_scratch_=self._kv8_scratch, xf=xf)
        if self.on_gpu and ops.rope_fusable(lw.wqkv, self.kv_fp8, T) and bt.shape[1] > 0:
            # RoPE + the KV-cache append in the qkv GEMM's epilogue: no qkv round trip, no rope_append launch
            ops.linear_rope(xn, lw.wqkv, posd, tsd, bt, self.cos, self.sin, q, kc, vc, self.H, self.Hkv, rows=rows)
            ops.attn_prefill(q, kc, vc, bt, cud, ctxd, self.H, self.Hkv, self.scale, out, **akw)
            return
        sk_q = self._splitk(T, self.d, (self.H + 2 * self.Hkv) * self.D)
        if xf:
            ops.linear_sk(xn, lw.wqkv, "bf16", qkv, rows=T)
            ops.rope_append(qkv, posd, tsd, bt, self.cos, self.sin, q, kc, vc, self.H, self.Hkv, kv_scales=kvs)
        elif sk_q > 1:  # small tile grid: f32 split-K slabs, summed by rope_append while it rotates
            parts = ops.linear(xn, lw.wqkv, "f32", splitk=sk_q)
            ops.rope_append(parts, posd, tsd, bt, self.cos, self.sin, q, kc, vc, self.H, self.Hkv, kv_scales=kvs)
        else:
            ops.linear(xn, lw.wqkv, "bf16", out=qkv)
            ops.rope_append(qkv, posd, tsd, bt, self.cos, self.sin, q, kc, vc, self.H, self.Hkv, kv_scales=kvs)
        ops.attn_prefill(q, kc, vc, bt, cud, ctxd, self.H, self.Hkv, self.scale, out, **akw)

    def _prefill_layers_sp(self, T, ids, posd, tsd, bt, cud, ctxd, last, work, n, commit):
        """Sequence-parallel prefill under TP: rank r owns rows [r*Tl, (r+1)*Tl) of the residual stream.
        Row-parallel outputs (O, down; [Tp, d], bf16 when ``sp_bf16`` else f32) are reduce-scattered instead of
        all-reduced, the residual add + RMSNorm runs on the local Tl rows only (in f32), and the bf16 normalised
        rows are all-gathered for the next column-parallel GEMM: with bf16 payloads both collectives move half the
        bytes of an f32 all-reduce's phases, and 1/tp of the norm work.  Rows past T (padding to a multiple of tp)
        are row-independent garbage that is never read back."""
        dev, w, d, tp = self.device, self.w, self.d, self.tp
        f32 = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=torch.bfloat16, device=dev)
        tps, r = tp.size, tp.rank
        Tl = (T + tps - 1) // tps
        Tp = Tl * tps
        ids_p = ids if Tp == T else torch.cat([ids, torch.zeros(Tp - T, dtype=ids.dtype, device=dev)])
        ids_l = ids_p[r * Tl:(r + 1) * Tl]
        h_l = torch.empty(Tl, d, **f32)
        xn_l = torch.empty(Tl, d, **bf)
        xn_full = torch.empty(Tp, d, **bf)
        xn = xn_full[:T]
        pay = dict(dtype=torch.bfloat16 if self.sp_bf16 else torch.float32, device=dev)
        epi = "bf16" if self.sp_bf16 else "f32"
        full = torch.zeros(Tp, d, **pay)  # row-parallel GEMM output (padding rows stay zero)
        loc = torch.empty(Tl, d, **f32)
        loc_p = torch.empty(Tl, d, **pay) if self.sp_bf16 else loc

        def rs():  # reduce-scatter of the row-parallel output into this rank's f32 residual slab
            tp.reduce_scatter(loc_p, full)
            if loc_p is not loc:
                loc.copy_(loc_p)

        qkv = torch.empty(T, (self.H + 2 * self.Hkv) * self.D, **bf)
        q = torch.empty(T, self.H, self.D, **bf)
        attn = torch.empty(T, self.H * self.D, **bf)
        parts = loc.view(1, Tl, d)
        for l, lw in enumerate(w.layers):
            if l == 0:
                ops.add_rmsnorm(h_l, lw.attn_norm, self.eps, xn_l, ids=ids_l, emb=w.embed)
            else:
                ops.add_rmsnorm(h_l, lw.attn_norm, self.eps, xn_l, parts=parts)
            tp.all_gather(xn_full.view(-1), xn_l.view(-1))
            self._prefill_attention(xn, lw, l, qkv, q, attn, posd, tsd, bt, cud, ctxd, work, T)
            ops.linear(attn, lw.wo, epi, out=full, splitk=1)
            rs()
            ops.add_rmsnorm(h_l, lw.mlp_norm, self.eps, xn_l, parts=parts)
            tp.all_gather(xn_full.view(-1), xn_l.view(-1))
            act = ops.linear(xn, lw.w_gate_up, "silu")
            ops.linear(act, lw.w_down, epi, out=full, splitk=1)
            rs()
        if not commit:
            return None
        ops.add_rmsnorm(h_l, w.final_norm, self.eps, xn_l, parts=parts)
        tp.all_gather(xn_full.view(-1), xn_l.view(-1))
        return xn_full.index_select(0, last.long())

    # ------------------------------------------------------------------------------------ readback
    def read_rows(self, slots: Sequence[int]):
        """(finished, gen_len, tokens) for ``slots`` (one device->host sync)."""
        idx = torch.tensor(list(slots), dtype=torch.long, device=self.device)
        n = idx.numel()
        parts = [self.finished.index_select(0, idx), self.gen_len.index_select(0, idx)]
        car = getattr(self.tp, "car", None) if self.tp is not None else None
        if car is not None:
            parts.append(car.err)  # one-shot all-reduce timeout flag, read in the same transfer
        host = torch.cat(parts).cpu()
        if car is not None and int(host[2 * n]):
            raise TPCommError("tensor-parallel all-reduce: a peer did not arrive within the timeout; "
                              "this replica's outputs since the last sync are invalid")
        return host[:n], host[n:2 * n], idx

    def tokens_of(self, slot: int, n: int) -> list[int]:
        return self.out_tokens[slot, :n].tolist()

    def tokens_of_many(self, slots: Sequence[int], ns: Sequence[int]) -> list[list[int]]:
        """``tokens_of`` for several rows in one device -> host transfer."""
        if not slots:
            return []
        m = max(ns)
        idx = torch.tensor(list(slots), dtype=torch.long, device=self.device)
        rows = self.out_tokens[:, :m].index_select(0, idx).cpu().tolist()
        return [r[:k] for r, k in zip(rows, ns)]
