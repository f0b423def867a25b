"""Prefix cache on the GPU: the KV block copy kernel (csrc/kernels/kv_copy.hip) bit for bit, and the engine with
cache hits: the KV a sharer attends to is the donor's, the donor's blocks are never written, the decode numerics of a
hit request pass the existing criterion (and fail it when the fork's copy is skipped), captured graphs replay."""
import dataclasses

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.eval import numerics as nm
from llm_based_apache_spark_optimization_amd.models import get_spec
from llm_based_apache_spark_optimization_amd.models.llama import init_random

from test_prefix_cache_cpu import QUESTIONS, SYS

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kv_copy_blocks
def arena(gpu, L, NB, Hkv, fp8, seed):
    """Random bit patterns (every bf16 / e4m3 encoding, NaNs included: the copy is compared as integers)."""
    g = torch.Generator().manual_seed(seed)
    if fp8:
        kv = torch.randint(0, 256, (L, 2, NB, Hkv, 64, 128), generator=g, dtype=torch.uint8).to(gpu)
        sc = torch.rand(L, 2, NB, Hkv, 64, generator=g).to(gpu)
        return kv, sc
    bits = torch.randint(-32768, 32768, (L, 2, NB, Hkv, 64, 128), generator=g, dtype=torch.int16)
    return bits.view(torch.bfloat16).to(gpu), None


def bits_of(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def check_copy(kv, sc, pairs):
    kv0 = bits_of(kv).clone()
    sc0 = bits_of(sc).clone() if sc is not None else None
    ops.kv_copy_blocks(kv, sc, pairs)
    torch.cuda.synchronize()
    dsts = {d for _, d in pairs}
    others = [b for b in range(kv.shape[2]) if b not in dsts]
    for now, was in ((bits_of(kv), kv0),) + (((bits_of(sc), sc0),) if sc is not None else ()):
        for s, d in pairs:  # every layer, K and V
            assert torch.equal(now[:, :, d], was[:, :, s]), (s, d)
        assert torch.equal(now[:, :, others], was[:, :, others])  # block 0 included


@pytest.mark.parametrize("pairs", [[(3, 5)], [(1, 8), (7, 2), (4, 6)]], ids=["one", "three"])
@pytest.mark.parametrize("Hkv", [1, 8])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_kv_copy_blocks_exact(gpu, fp8, Hkv, pairs):
    """Hkv = 1 with fp8 is the smallest tile (8 KiB + a 256 B scale tile): one workgroup per plane, guarded tail."""
    kv, sc = arena(gpu, 2, 9, Hkv, fp8, seed=17 * Hkv + fp8)
    check_copy(kv, sc, pairs)


def test_kv_copy_blocks_production_stride(gpu):
    kv, sc = arena(gpu, 28, 5, 8, False, seed=5)
    check_copy(kv, sc, [(4, 1), (2, 3)])


def test_kv_copy_blocks_rejects_bad_operands(gpu):
    kv, sc = arena(gpu, 2, 9, 1, True, seed=1)
    kv0, sc0 = kv.clone(), sc.clone()
    for bad in ([(0, 3)], [(3, 0)], [(3, 9)], [(9, 3)], [(3, 3)], [(1, 2), (3, 2)], [(1, 2), (2, 3)], [(-1, 2)]):
        with pytest.raises(ValueError):
            ops.kv_copy_blocks(kv, sc, bad)
    pairs = torch.tensor([[3, 5]], dtype=torch.int32, device=gpu)
    for args in ((kv.float(), sc, pairs), (kv, None, pairs), (kv, sc[:, :, :8].contiguous(), pairs),
                 (kv, sc, pairs.long()), (kv[:, :, :, :, :32], sc, pairs), (kv, sc, pairs.view(-1))):
        with pytest.raises(RuntimeError):
            ops.ext().kv_copy_blocks(*args)
    torch.cuda.synchronize()
    assert torch.equal(kv, kv0) and torch.equal(sc, sc0)  # nothing was launched
    ops.kv_copy_blocks(kv, sc, [])


# ------------------------------------------------------------------------------------------------ engine, exact part
def make(gpu, kv_dtype="bf16", **kw):
    return build_engine("tiny-nsql", device=str(gpu), max_slots=3, max_model_len=512, num_kv_blocks=33,
                        kv_dtype=kv_dtype, prefix_cache=True, **kw)


def rows_below(r, block, n):
    """The KV (and scales) of a block's first n token rows in every layer, as integers."""
    kv = bits_of(r.kv)[:, :, block]
    if not r.kv_fp8:
        return [kv[:, :, :, :n].clone()]
    assert n % 2 == 0  # e4m3 rows lie in token-pair order: pair p = the 256 bytes at 256 p of a head's tile
    L, _, Hkv = kv.shape[:3]
    return [kv.reshape(L, 2, Hkv, 64 * 128)[..., :128 * n].clone(), bits_of(r.kv_scale)[:, :, block, :, :n].clone()]


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_sharer_reads_the_donors_kv(gpu, kv_dtype):
    eng = make(gpu, kv_dtype)
    r = eng.runner
    assert r.use_graphs and r.kv_fp8 == (kv_dtype == "fp8")
    eng.run_ahead = 2
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    a, b = SYS + QUESTIONS[0], SYS + QUESTIONS[1]  # 199 and 204 tokens, 150 in common
    donor = eng.add_request(a, sp)
    eng.step()  # prefill, publish, two decode steps
    td = eng.sched.block_table(donor.rid)
    assert eng.sched.shared_blocks(donor.rid) == 3 and eng.sched.cached_tokens(donor.rid) == 0
    torch.cuda.synchronize()
    snap = [rows_below(r, blk, 64) for blk in td[:3]]
    eng.run_until_done([donor])
    sharer = eng.add_request(b, sp)
    eng.step()
    ts = eng.sched.block_table(sharer.rid)
    assert eng.sched.cached_tokens(sharer.rid) == 150 and sharer.cached_tokens == 150
    assert ts[:2] == td[:2] and ts[2] != td[2] and ts[2] not in td[:3]  # shared ids, then the private fork
    torch.cuda.synchronize()
    for x, y in zip(rows_below(r, ts[2], 22), rows_below(r, td[2], 22)):  # the fork's rows below p = 22
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(rows_below(r, ts[2], 64), rows_below(r, td[2], 64)))
    eng.run_until_done([sharer])
    torch.cuda.synchronize()
    for blk, was in zip(td[:3], snap):  # the donor's blocks are never written: not by its decode, not by the sharer
        for x, y in zip(rows_below(r, blk, 64), was):
            assert torch.equal(x, y), blk
    assert eng.stats["prefix_hits"] == 1 and eng.stats["prefix_cached_tokens"] == 150
    assert eng.stats["prompt_tokens"] == len(a) + len(b) - 150


def test_engine_graphs_replay_after_hits(gpu):
    """Cache hits change what is prefilled, not the decode step: the captured decode graphs replay, and the same
    sequence of requests run again (from an empty cache) gives the same tokens and the same hits."""
    eng = make(gpu)
    r = eng.runner
    sp = SamplingParams(max_tokens=24, ignore_eos=True)
    prompts = [SYS + q for q in QUESTIONS]

    def run():
        c0 = eng.stats["prefix_cached_tokens"]
        out = [eng.generate([p], sp)[0] for p in prompts]
        pair = [eng.add_request(p, sp) for p in prompts[1:]]  # two sharers decoding in one batch
        eng.run_until_done(pair)
        return ([x.token_ids for x in out] + [q.output_ids for q in pair],
                [x.cached_prompt_tokens for x in out] + [q.cached_tokens for q in pair],
                eng.stats["prefix_cached_tokens"] - c0)

    first = run()
    assert r.use_graphs and r.graphs
    graphs = set(r.graphs)
    assert first[1][:3] == [0, 150, 150] and first[1][3:] == [192, 192] and first[2] == sum(first[1])
    assert eng.sched.reset_prefix_cache() > 0 and eng.sched.cached_blocks == 0
    assert run() == first
    assert set(r.graphs) == graphs  # replayed, nothing recaptured


# ------------------------------------------------------------------------------------------------ engine, numerics
@pytest.mark.parametrize("base", ["duckdb-nsql", "llama3.2"])
def test_hit_request_numerics_and_skipped_copy_is_caught(gpu, base):
    """Production widths, 4 layers (the engines of test_spec_gpu.py::test_spec_numerics_check_catches_kv_fault; the
    256-wide models do not move under KV faults).  A 128-token prompt reuses 64 shared tokens and a fork of p = 40:
    the teacher-forced check over 64 decode steps of the hit request passes the existing thresholds, and fails them
    when the fork's block copy is skipped (the 40 forked rows are then whatever the block held)."""
    spec = dataclasses.replace(get_spec(base), n_layers=4, name=base + "-4l")
    g = torch.Generator().manual_seed(3)
    donor = [1] + torch.randint(3, 30000, (139,), generator=g).tolist()
    hit = donor[:104] + torch.randint(3, 30000, (24,), generator=g).tolist()
    assert hit[104] != donor[104]

    def engine():
        r = ModelRunner(init_random(spec, gpu, seed=5), max_slots=2, max_model_len=512, num_kv_blocks=17)
        eng = LLMEngine(r, name=spec.name, prefix_cache=True)
        eng.generate([donor], SamplingParams(max_tokens=4, ignore_eos=True))
        assert eng.sched.cached_blocks == 2
        return eng

    eng = engine()
    good = nm.teacher_forced_check(eng, [hit], 64)
    assert eng.stats["prefix_cached_tokens"] == 104 and eng.stats["prefix_hits"] == 1
    bad_eng = engine()
    bad_eng.runner.copy_kv_blocks = lambda pairs: None
    bad = nm.teacher_forced_check(bad_eng, [hit], 64)
    assert bad_eng.stats["prefix_cached_tokens"] == 104
    print({"good": good, "bad_skipped_copy": bad})
    assert good["ok"] and good["tokens_checked"] >= 64, good
    assert not bad["ok"], (good, bad)
