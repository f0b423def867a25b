"""Prefix cache on the CPU: the scheduler's block index (native and pure-Python twin, scenario by scenario and in a
seeded differential run) and the engine end to end on tiny-nsql, where chunked prefill is exact, so a request that
reuses cached KV blocks must produce exactly the tokens it produces without the cache."""
import os
import random

import pytest
import torch

from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.runtime import native

IMPLS = [pytest.param(native._PyScheduler, id="python")]
if native.NATIVE:
    IMPLS.append(pytest.param(native._mod.Scheduler, id="native"))


def sched(cls, num_blocks=17, slots=4, budget=100000, maxb=16, **kw):
    return cls(num_blocks, 64, slots, budget, maxb, prefix_cache=True, **kw)


def toks(n, salt=0, start=0):
    return [(7 * i + 13 * salt * (i + 1)) % 251 + 3 for i in range(start, start + n)]


def admit_one(s, rid):
    assert s.admit() == [rid]
    copies = s.take_copies()
    s.copies_done()
    return copies


# ------------------------------------------------------------------------------------------------ scheduler scenarios
@pytest.mark.parametrize("cls", IMPLS)
@pytest.mark.parametrize("cow,cached,copies", [(16, 150, [(3, 4)]), (64, 128, [])])
def test_miss_then_hit(cls, cow, cached, copies):
    s = sched(cls, cow_min_tokens=cow)
    a = toks(200)
    b = a[:150] + toks(50, salt=1)
    assert b[150] != a[150]
    s.add(1, 200, 10, a)
    assert admit_one(s, 1) == [] and s.cached_tokens(1) == 0
    assert s.block_table(1) == [1, 2, 3, 4] and s.shared_blocks(1) == 0
    assert s.publish(1) == 3 and s.shared_blocks(1) == 3 and s.cached_blocks == 3
    assert s.publish(1) == 0  # once per admission
    s.finish(1)
    assert s.cached_blocks == 3 and s.free_blocks == 16 and s.kv_usage == 0.0
    s.add(2, 200, 10, b)
    assert admit_one(s, 2) == copies
    assert s.cached_tokens(2) == cached and s.shared_blocks(2) == 2
    assert s.block_table(2) == [1, 2, 4, 5]  # two shared blocks, then private ones (the fork's target first)
    # B's third block (forked or not) differs from A's: published as a sibling
    assert s.publish(2) == 1 and s.block_table(2)[:3] == [1, 2, 4] and s.shared_blocks(2) == 3
    assert [n[0] for n in s.prefix_nodes()] == [1, 2, 3, 4]


@pytest.mark.parametrize("cls", IMPLS)
@pytest.mark.parametrize("cow,cached", [(16, 127), (64, 64)])
def test_last_token_cap(cls, cow, cached):
    """An identical prompt of exactly 2 blocks: at least its last token is computed, so its last block can only be
    reused through the fork (63 rows)."""
    s = sched(cls, cow_min_tokens=cow)
    p = toks(128)
    s.add(1, 128, 10, p)
    admit_one(s, 1)
    s.publish(1)
    s.finish(1)
    s.add(2, 128, 10, p)
    copies = admit_one(s, 2)
    assert s.cached_tokens(2) == cached and s.shared_blocks(2) == 1
    assert copies == ([(2, s.block_table(2)[1])] if cow == 16 else [])
    # publishing a duplicate keeps the duplicate private
    assert s.publish(2) == 0 and s.shared_blocks(2) == 1 and s.cached_blocks == 2
    t = s.block_table(2)
    s.finish(2)
    assert s.free_blocks == 16 and [n[0] for n in s.prefix_nodes()] == [1, 2] and t[1] not in (1, 2)


@pytest.mark.parametrize("cls", IMPLS)
def test_opt_out_and_token_checks(cls):
    s = sched(cls)
    p = toks(200)
    s.add(1, 200, 10, p)
    admit_one(s, 1)
    s.publish(1)
    s.finish(1)
    s.add(2, 200, 10, p, False)  # cacheable = False: neither matches nor publishes
    assert admit_one(s, 2) == [] and s.cached_tokens(2) == 0 and s.shared_blocks(2) == 0
    assert s.publish(2) == 0 and s.cached_blocks == 3
    s.add(3, 200, 10, [], False)  # tokens are ignored then
    with pytest.raises(Exception):
        s.add(4, 200, 10, p[:199])  # required and length-checked when the cache is on
    with pytest.raises(Exception):
        s.add(5, 200, 10)
    s.add(6, 200, 10, p)
    assert s.admit() == [3, 6] and s.cached_tokens(6) == 192 and s.take_copies() == []  # the donor's partial 4th block is not cached
    s.copies_done()
    with pytest.raises(Exception):
        s.preempt(6, 201, 9, p)
    s.preempt(6, 201, 9, p + [5])
    assert s.cached_tokens(6) == 0 and s.block_table(6) == []
    off = cls(17, 64, 4, 100000, 16)  # cache off: tokens are ignored altogether
    off.add(1, 200, 10, p[:5])
    off.add(2, 200, 10)
    assert off.admit() == [1, 2] and off.cached_tokens(1) == 0 and off.publish(1) == 0 and off.cached_blocks == 0


@pytest.mark.parametrize("cls", IMPLS)
def test_refcounts_and_eviction(cls):
    s = sched(cls, num_blocks=9, slots=3, maxb=8)  # 8 usable blocks
    p = toks(130)
    s.add(1, 130, 10, p)
    admit_one(s, 1)  # blocks 1 2 3
    s.publish(1)     # nodes 1 2
    s.add(2, 130, 10, p)
    s.add(3, 130, 10, p)
    assert s.admit() == [2, 3] and s.take_copies() == []
    s.copies_done()
    assert s.block_table(2)[:2] == [1, 2] == s.block_table(3)[:2]
    assert [n[:3] for n in s.prefix_nodes()] == [[1, 3, 1], [2, 3, 0]]
    assert s.free_blocks == 8 - 5 and abs(s.kv_usage - 5 / 8) < 1e-12
    # every other block goes to request 4; the shared ones are never handed out
    s.finish(1)
    s.finish(2)
    assert [n[1] for n in s.prefix_nodes()] == [1, 1] and s.free_blocks == 8 - 3
    s.add(4, 60, 440, toks(60, salt=3))
    assert s.admit() == [4]
    assert s.grow(4, 160) == 1 and s.grow(4, 64 * 5) == 2 and s.free_blocks == 0
    assert s.grow(4, 64 * 5 + 1) == -1  # private + referenced blocks fill the arena
    assert not {1, 2} & set(s.block_table(4))
    s.finish(3)  # both holders gone: the two nodes are evictable and count as free, with 3's private block
    assert s.cached_blocks == 2 and s.free_blocks == 3 and [n[1] for n in s.prefix_nodes()] == [0, 0]
    assert s.grow(4, 64 * 6 + 1) == 2  # one block from the free list, one evicted: the leaf, not its parent
    assert [n[0] for n in s.prefix_nodes()] == [1] and set(s.block_table(4)[-2:]) == {2, 5}
    assert s.grow(4, 64 * 7 + 1) == 1 and s.cached_blocks == 0 and s.block_table(4)[-1] == 1
    assert s.free_blocks == 0 and len(s.block_table(4)) == 8


@pytest.mark.parametrize("cls", IMPLS)
def test_eviction_is_lru_and_admission_evicts(cls):
    s = sched(cls, num_blocks=9, slots=2, maxb=8)
    for rid, salt in ((1, 1), (2, 2), (3, 3)):  # three unrelated 2-block chains, released in the order 1 2 3
        s.add(rid, 130, 1, toks(130, salt=salt))
        admit_one(s, rid)
        s.publish(rid)
        s.finish(rid)
    chains = {n[0]: n[4] for n in s.prefix_nodes()}
    assert len(chains) == 6 and s.free_blocks == 8
    s.add(4, 130, 1, toks(130, salt=2))  # touches chain 2: now the most recently used
    admit_one(s, 4)
    s.finish(4)
    s.add(5, 250, 1, toks(250, salt=9))  # needs 4 blocks, 2 are on the free list: evicts chain 1, leaf first
    admit_one(s, 5)
    left = {n[0] for n in s.prefix_nodes()}
    assert sorted(b for b in chains if b not in left) == [1, 2] and chains[2] == 1
    s.add(6, 60, 1, toks(60, salt=8))  # one more block: the leaf of chain 3, released after chain 2 but used before
    admit_one(s, 6)
    assert {n[0] for n in s.prefix_nodes()} == {3, 4, 5}
    s.finish(6)
    s.add(7, 130, 1, toks(130, salt=2))
    admit_one(s, 7)
    assert s.cached_tokens(7) == 128
    s.finish(7)
    s.add(8, 130, 1, toks(130, salt=1))
    admit_one(s, 8)
    assert s.cached_tokens(8) == 0  # chain 1 is gone


@pytest.mark.parametrize("cls", IMPLS)
def test_pending_copy_source_is_pinned(cls):
    """The source of a pending copy survives a later admission of the same admit() that needs every other block."""
    s = sched(cls, num_blocks=9, slots=3, maxb=8)
    a = toks(128)
    s.add(1, 128, 1, a)
    admit_one(s, 1)  # blocks 1 2 3
    s.publish(1)     # nodes 1 2
    s.finish(1)
    s.add(2, 100, 1, a[:100])  # chain [1], fork of block 2 with p = 35
    s.add(3, 300, 1, toks(300, salt=7))  # 5 blocks: everything else
    assert s.admit() == [2, 3]
    t2, t3 = s.block_table(2), s.block_table(3)
    assert s.cached_tokens(2) == 99 and t2[0] == 1 and len(t3) == 5
    assert s.take_copies() == [(2, t2[1])]
    assert 2 not in t3 and 1 not in t3 and not set(t2) & set(t3)
    assert [n[:2] for n in s.prefix_nodes()] == [[1, 2], [2, 1]]  # request 2 + the pin; the pin alone
    assert s.free_blocks == 0
    s.copies_done()
    assert [n[:2] for n in s.prefix_nodes()] == [[1, 1], [2, 0]] and s.free_blocks == 1
    # had request 3 come alone it would have evicted block 2
    s.finish(2)
    s.finish(3)
    s.add(4, 420, 1, toks(420, salt=8))
    assert s.admit() == [4] and s.cached_blocks == 1


@pytest.mark.parametrize("cls", IMPLS)
def test_reset_and_preempt_resume(cls):
    s = sched(cls, num_blocks=9, slots=2, maxb=8)
    p = toks(140)
    s.add(1, 140, 50, p)
    admit_one(s, 1)
    s.publish(1)
    assert s.reset_prefix_cache() == 0 and s.cached_blocks == 2  # referenced nodes stay
    gen = toks(60, salt=4)
    s.preempt(1, 200, 10, p + gen)  # resumed with its generated tokens folded in
    assert s.cached_blocks == 2 and s.free_blocks == 8
    assert s.admit() == [1] and s.cached_tokens(1) == 128 and s.block_table(1)[:2] == [1, 2]  # hits its own blocks
    s.copies_done()
    s.publish(1)
    assert s.cached_blocks == 3
    s.finish(1)
    assert s.reset_prefix_cache() == 3 and s.cached_blocks == 0 and s.free_blocks == 8 and s.prefix_nodes() == []


@pytest.mark.parametrize("cls", IMPLS)
def test_cache_off_block_ids_unchanged(cls):
    """prefix_cache=False (the default): the block ids of a scripted run are those of the scheduler before the
    prefix cache existed (free list popped from its end, released blocks appended in table order)."""
    for kw in ({}, {"prefix_cache": False}):
        s = cls(9, 64, 2, 1000, 8, **kw)
        s.add(1, 100, 100)
        s.add(2, 70, 100)
        assert s.admit() == [1, 2]
        assert s.block_table(1) == [1, 2, 3] and s.block_table(2) == [4, 5, 6] and s.free_blocks == 2
        assert s.grow(1, 193) == 1 and s.block_table(1) == [1, 2, 3, 7]
        s.finish(2)
        s.add(3, 10, 10)
        assert s.admit() == [3] and s.block_table(3) == [6]
        s.preempt(1, 150, 50)
        assert s.admit() == [1] and s.block_table(1) == [7, 3, 2, 1] and s.free_blocks == 3
        assert s.grow(3, 20) == 0 and s.grow(1, 10 ** 6) == 0
        assert s.cached_blocks == 0 and s.take_copies() == [] and abs(s.kv_usage - 5 / 8) < 1e-12
        s.finish(1)
        s.add(4, 200, 300)
        assert s.admit() == [4] and s.block_table(4) == [1, 2, 3, 7, 5]


# ------------------------------------------------------------------------------------------------ differential run
def _check_invariants(s, live, nb):
    nodes = s.prefix_nodes()
    index = {n[0] for n in nodes}
    holders, private = {}, []
    for rid in live:
        t, k = s.block_table(rid), s.shared_blocks(rid)
        assert set(t[:k]) <= index
        for b in t[:k]:
            holders[b] = holders.get(b, 0) + 1
        private += t[k:]
    assert len(private) == len(set(private)), "a block in two private tables"
    assert not set(private) & index, "a private block in the index"
    assert 0 not in private and 0 not in index
    for n in nodes:
        assert n[1] == holders.get(n[0], 0), "reference count != holders"
    evictable = sum(1 for n in nodes if n[1] == 0)
    assert (s.free_blocks - evictable) + len(private) + len(nodes) == nb - 1
    assert s.cached_blocks == len(nodes)


@pytest.mark.skipif(not native.NATIVE, reason="no native runtime to compare with")
@pytest.mark.parametrize("seed,cow", [(0, 16), (1, 1), (2, 64)])
def test_differential_native_vs_python(seed, cow):
    rng = random.Random(seed)
    nb = 24
    pair = [cls(nb, 64, 4, 400, 12, prefix_cache=True, cow_min_tokens=cow)
            for cls in (native._mod.Scheduler, native._PyScheduler)]
    bases = [toks(700, salt=k) for k in range(3)]
    reqs, waiting, running, next_id = {}, [], [], 1

    def prompt():
        base = bases[rng.randrange(3)]
        n = rng.choice([rng.randrange(1, 500), 64 * rng.randrange(1, 7), 64 * rng.randrange(1, 7) + 1])
        cut = rng.randrange(0, n + 1)
        return base[:cut] + toks(n - cut, salt=rng.randrange(4, 9), start=cut)

    def both(f):
        out = []
        for s in pair:
            try:
                out.append(("ok", f(s)))
            except Exception as e:  # noqa: BLE001 - both must fail alike
                out.append(("err", type(e).__name__ in ("ValueError", "RuntimeError", "IndexError", "KeyError")))
        assert out[0] == out[1] or (out[0][0] == out[1][0] == "err"), out
        return out[0]

    for _ in range(3000):
        op = rng.random()
        if op < 0.25:
            p, mx = prompt(), rng.randrange(1, 200)
            rid, next_id = next_id, next_id + 1
            cacheable = rng.random() < 0.9
            if both(lambda s: s.add(rid, len(p), mx, p, cacheable))[0] == "ok":
                reqs[rid] = [p, mx]
                waiting.append(rid)
        elif op < 0.5:
            kind, got = both(lambda s: s.admit())
            assert kind == "ok"
            for rid in got:
                waiting.remove(rid)
                running.append(rid)
                both(lambda s: (s.block_table(rid), s.cached_tokens(rid), s.slot(rid)))
                assert got and pair[0].cached_tokens(rid) <= len(reqs[rid][0]) - 1
            assert both(lambda s: s.take_copies())[0] == "ok"
            both(lambda s: s.copies_done())
        elif op < 0.65 and running:
            rid = rng.choice(running)
            both(lambda s: s.publish(rid))
        elif op < 0.8 and running:
            rid = rng.choice(running)
            want = rng.randrange(1, 900)
            both(lambda s: s.grow(rid, want))
        elif op < 0.88 and running:
            rid = rng.choice(running)
            p, mx = reqs[rid]
            p2 = p + toks(rng.randrange(0, 40), salt=rid % 5)
            mx2 = max(1, mx - (len(p2) - len(p)))
            if both(lambda s: s.preempt(rid, len(p2), mx2, p2))[0] == "ok":
                reqs[rid] = [p2, mx2]
                running.remove(rid)
                waiting.insert(0, rid)
        elif op < 0.98 and (running or waiting):
            rid = rng.choice(running + waiting)
            both(lambda s: s.finish(rid))
            (running if rid in running else waiting).remove(rid)
            del reqs[rid]
        else:
            both(lambda s: s.reset_prefix_cache())
        both(lambda s: (s.free_blocks, s.cached_blocks, s.kv_usage, s.prefix_nodes(), s.num_waiting, s.num_running,
                        s.youngest_first()))
        for s in pair:
            _check_invariants(s, running, nb)
    assert next_id > 300 and pair[0].cached_blocks >= 0


# ------------------------------------------------------------------------------------------------ engine
SYS = [1] + toks(149, salt=2)  # a 150-token "schema": two full blocks and 22 tokens of a third
QUESTIONS = [toks(n, salt=s) for n, s in ((49, 3), (54, 4), (45, 5))]  # prompts of three full blocks and a bit


def make(prefix_cache, **kw):
    kw.setdefault("max_slots", 3)
    kw.setdefault("max_model_len", 512)
    return build_engine("tiny-nsql", device="cpu", prefix_cache=prefix_cache, **kw)


def expected_cached(prompt, donors, cow=native._PyScheduler.COW_MIN_TOKENS):
    """Host model of the index for donors that were published whole and never evicted."""
    best = 0
    for d in donors:
        lcp = next((i for i, (x, y) in enumerate(zip(prompt, d)) if x != y), min(len(prompt), len(d)))
        lcp = min(lcp, len(prompt) - 1)
        full, p = divmod(lcp, 64)
        full = min(full, len(d) // 64)
        p = p if (full < len(d) // 64 and p >= cow) else 0
        best = max(best, 64 * full + p)
    return best


def run_sequence(eng, prompts, sp):
    return [eng.generate([p], sp)[0] for p in prompts]


@pytest.mark.parametrize("kw,spkw", [
    ({}, {}),
    ({"prefill_chunk": 40}, {}),
    ({"spec_tokens": 3}, {}),
    ({}, {"repeat_penalty": 1.1}),
    ({"kv_dtype": "fp8"}, {}),
], ids=["plain", "chunk40", "spec3", "penalty", "kv_fp8"])
def test_engine_tokens_equal_with_and_without_cache(kw, spkw):
    sp = SamplingParams(max_tokens=12, ignore_eos=True, **spkw)
    same = [1] + toks(127, salt=6)  # exactly two blocks: the repeat reuses 127 tokens through the fork
    prompts = [SYS + q for q in QUESTIONS] + [same, same]
    off, on = make(False, **kw), make(True, **kw)
    want = run_sequence(off, prompts, sp)
    got = run_sequence(on, prompts, sp)
    assert [r.token_ids for r in got] == [r.token_ids for r in want]
    exp = [expected_cached(p, prompts[:i]) for i, p in enumerate(prompts)]
    assert exp == [0, 150, 150, 0, 127]
    assert [r.cached_prompt_tokens for r in got] == exp and all(r.cached_prompt_tokens == 0 for r in want)
    assert [r.prompt_tokens for r in got] == [len(p) for p in prompts]  # the full prompt length, as before
    st = on.stats
    assert st["prefix_cached_tokens"] == sum(exp) and st["prefix_queries"] == 5 and st["prefix_hits"] == 3
    assert st["prompt_tokens"] == sum(len(p) for p in prompts) - sum(exp)  # a hit prefills only its suffix
    assert off.stats["prompt_tokens"] == sum(len(p) for p in prompts) and off.stats["prefix_queries"] == 0
    assert off.sched.cached_blocks == 0 and on.sched.cached_blocks > 0
    assert on.sched.num_running == 0 and on.sched.free_blocks == on.runner.num_kv_blocks - 1
    if kw.get("spec_tokens"):
        assert st["spec_steps"] > 0 and st["spec_steps"] == off.stats["spec_steps"]


def test_engine_two_sharers_in_one_batch():
    sp = SamplingParams(max_tokens=10, ignore_eos=True)
    prompts = [SYS + q for q in QUESTIONS]
    off, on = make(False), make(True)
    want = [r.token_ids for r in off.generate(prompts, sp)]
    donor = on.generate(prompts[:1], sp)[0]
    reqs = [on.add_request(p, sp) for p in prompts[1:]]
    on.run_ahead = 2  # as a server bounds each decode run
    on.step()
    assert on.sched.num_running == 2  # admitted by one admit(), decoding in one batch
    t1, t2 = (on.sched.block_table(q.rid) for q in reqs)
    assert t1[:2] == t2[:2] and t1[2] != t2[2] and not set(t1[2:]) & set(t2[2:])
    on.run_until_done(reqs)
    assert [donor.token_ids] + [q.output_ids for q in reqs] == want
    assert [on.result(q).cached_prompt_tokens for q in reqs] == [150, 150]


def test_engine_row_finished_by_prefill_token_leaves_published_block_alone():
    """A prompt that fills its last block exactly and ends with EOS as its first token: the finished row keeps
    rewriting the KV row of its position while the decode run replays, and that must not be row 63 of the published
    block (the runner parks it at prompt_len when the cache is on)."""
    p = [1] + toks(127, salt=6)
    probe = make(True)
    first = probe.generate([p], SamplingParams(max_tokens=1, ignore_eos=True))[0].token_ids[0]  # no decode run
    assert probe.sched.cached_blocks == 2
    eng = make(True)
    eng.runner.set_eos([first])
    r = eng.generate([p], SamplingParams(max_tokens=10))[0]
    assert r.token_ids == [first] and r.done_reason == "stop" and eng.stats["decode_steps"] > 0
    blocks = [n[0] for n in eng.sched.prefix_nodes()]
    assert blocks == [n[0] for n in probe.sched.prefix_nodes()] == [1, 2]
    assert torch.equal(eng.runner.kv[:, :, blocks], probe.runner.kv[:, :, blocks])
    off = make(False)  # without the cache nothing changes: the row stays at its last prompt position
    off.runner.set_eos([first])
    assert off.generate([p], SamplingParams(max_tokens=10))[0].token_ids == [first]
    assert not off.runner.park_past_prompt and not torch.equal(off.runner.kv[:, :, 2], probe.runner.kv[:, :, 2])
    # a longer prompt that extends it reads the whole cached block
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    longer = p + toks(30, salt=4)
    assert eng.generate([longer], sp)[0].token_ids == make(False).generate([longer], sp)[0].token_ids
    assert eng.stats["prefix_cached_tokens"] == 128


def test_engine_cache_prompt_false_never_hits():
    sp = SamplingParams.from_ollama_options({"num_predict": 6, "ignore_eos": True, "cache_prompt": False})
    assert sp.cache_prompt is False and SamplingParams.from_ollama_options({}).cache_prompt is True
    on = make(True)
    p = SYS + QUESTIONS[0]
    a, b = run_sequence(on, [p, p], sp)
    assert a.token_ids == b.token_ids and b.cached_prompt_tokens == 0
    assert on.stats["prefix_queries"] == 0 and on.sched.cached_blocks == 0
    c = on.generate([p], SamplingParams(max_tokens=6, ignore_eos=True))[0]  # nothing was published either
    assert c.cached_prompt_tokens == 0 and c.token_ids == a.token_ids and on.sched.cached_blocks == 3


def test_engine_small_arena_preempts_and_evicts():
    """8 usable blocks, 3 slots, long generations: lazy growth preempts, admissions evict cached blocks, resumed
    requests find some of their own blocks again -- the tokens are those of an engine with room for everything."""
    sp = SamplingParams(max_tokens=120, ignore_eos=True)
    prompts = [SYS[:100] + q for q in QUESTIONS] + [[1] + toks(70, salt=8)] + [SYS[:100] + QUESTIONS[0]]
    want = [r.token_ids for r in make(False).generate(prompts, sp)]
    on = make(True, num_kv_blocks=9)
    reqs = [on.add_request(p, sp) for p in prompts]
    on.run_until_done(reqs)
    assert [q.output_ids for q in reqs] == want
    assert on.stats["preempted"] > 0 and on.stats["prefix_hits"] > 0
    assert on.sched.num_running == 0 and on.sched.free_blocks == 8
    on.abort_all("test")
    assert on.sched.cached_blocks == 0  # abort_all drops the cache: the device state is suspect after a failed step


def test_settings_env_and_surface(monkeypatch):
    import argparse

    from llm_based_apache_spark_optimization_amd.client import EngineService, GenerateResponse
    from llm_based_apache_spark_optimization_amd.parallel.lockstep import MUTATORS

    assert Settings().prefix_cache is False
    assert Settings().prefix_cow_min_tokens == native._PyScheduler.COW_MIN_TOKENS
    monkeypatch.setenv("LSA_PREFIX_CACHE", "1")
    monkeypatch.setenv("LSA_PREFIX_COW_MIN_TOKENS", "24")
    s = Settings()
    assert s.prefix_cache is True and s.prefix_cow_min_tokens == 24
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    monkeypatch.delenv("LSA_PREFIX_CACHE")
    assert Settings.from_cli(ap.parse_args(["--prefix-cache"])).prefix_cache is True
    assert "copy_kv_blocks" in MUTATORS
    assert GenerateResponse(model="m", response="").prompt_cached_count == 0
    if native.NATIVE:
        assert native._mod.Scheduler(9, 64, 2, 100, 8, prefix_cache=True).cow_min_tokens == native._PyScheduler.COW_MIN_TOKENS

    svc = EngineService(lambda m: make(True, prefix_cow_min_tokens=24))
    opts = {"temperature": 0, "num_predict": 4, "ignore_eos": True}
    system = "Name (string), Fare (float), " * 4
    r1 = svc.generate("tiny-nsql", "Select all rows", system, opts)
    r2 = svc.generate("tiny-nsql", "Count the rows", system, opts)
    assert svc.loop("tiny-nsql").engine.sched.cow_min_tokens == 24
    assert r1.prompt_cached_count == 0 and r2.prompt_cached_count >= 64
    assert r2.prompt_eval_count > r2.prompt_cached_count and "prompt_cached_count" in r2.to_dict()
    h = svc.health()["engines"]["tiny-nsql"]
    assert h["prefix_queries"] == 2 and h["prefix_hits"] == 1 and h["prefix_cached_tokens"] == r2.prompt_cached_count
    assert h["prefix_cached_blocks"] > 0
    svc.loop("tiny-nsql").close()


def test_kv_copy_blocks_cpu():
    from llm_based_apache_spark_optimization_amd import ops

    g = torch.Generator().manual_seed(0)
    kv = torch.randint(0, 255, (2, 2, 9, 2, 64, 128), generator=g, dtype=torch.uint8)
    sc = torch.rand(2, 2, 9, 2, 64, generator=g)
    kv0, sc0 = kv.clone(), sc.clone()
    ops.kv_copy_blocks(kv, sc, [(1, 8), (7, 2)])
    assert torch.equal(kv[:, :, 8], kv0[:, :, 1]) and torch.equal(sc[:, :, 2], sc0[:, :, 7])
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert torch.equal(kv[:, :, keep], kv0[:, :, keep]) and torch.equal(sc[:, :, keep], sc0[:, :, keep])
    for bad in ([(0, 3)], [(3, 0)], [(3, 9)], [(3, 3)], [(1, 2), (3, 2)], [(1, 2), (2, 3)], [(-1, 2)]):
        with pytest.raises(ValueError):
            ops.kv_copy_blocks(kv, sc, bad)


# ------------------------------------------------------------------------------------------------ TP = 2 (gloo)
def _tp_worker(rank, world, port, q):
    import torch.distributed as dist

    from llm_based_apache_spark_optimization_amd.parallel import TPGroup

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tp = TPGroup(dist.group.WORLD, rank, world, torch.device("cpu"))
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    prompts = [SYS + q for q in QUESTIONS[:2]]
    out = []
    for cache in (False, True):
        e = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=256, tp=tp, prefix_cache=cache)
        out.append([e.generate([p], sp)[0].token_ids for p in prompts])
        out.append(e.stats["prefix_cached_tokens"])
    q.put((rank, out))
    dist.destroy_process_group()


def test_tensor_parallel_tokens_equal_with_cache():
    import socket

    import torch.multiprocessing as tmp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = tmp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = dict(q.get(timeout=240) for _ in ps)
    [p.join(timeout=60) for p in ps]
    assert res[0] == res[1]
    off, off_cached, on, on_cached = res[0]
    assert on == off and off_cached == 0 and on_cached == 150
