"""Speculative decoding for several concurrent requests of which some are regex-constrained, on the GPU
(``spec_batch_guided``): dfa_mask_verify_kernel and dfa_spec_advance_kernel over S sequences (csrc/kernels/guided.hip)
against the plain rule, their host twins' expectations and each sequence's own one-sequence launch -- exact: allowed logits
bit-unchanged, the others -inf, g_state and g_spec equal -- and the engine's batched guided verify steps with captured
graphs."""
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import build_engine

from test_spec_cpu import K
from test_spec_guided_cpu import EOS, cases
from test_spec_batch_cpu import PROMPTS
from test_spec_batch_guided_cpu import (ALL, CASES, MIXES, WITH_FREE, MixEnv, check_mix_list, mix_cases,
                                        operands, params, planted, refusals, run, run_mix, spy, verify_call)

pytestmark = pytest.mark.gpu
I32 = dict(dtype=torch.int32)

_ENVS = {}


def mix_env(gpu, V):
    return _ENVS.get(V) or _ENVS.setdefault(V, MixEnv(V, str(gpu)))  # (the plain-rule masks are computed once per V)


# V: three chunks with a partial last one | exactly one chunk
@pytest.mark.parametrize("S,T,i", MIXES)
@pytest.mark.parametrize("V", [5000, 2048])
def test_kernels_match_plain_rule_and_one_sequence_launches(gpu, V, S, T, i):
    me = mix_env(gpu, V)
    run_mix(me, mix_cases(me.env, S, T, i), T, torch.Generator().manual_seed(V + 100 * S + 10 * T + i))
    torch.cuda.synchronize()


def test_mix_list_is_what_it_says(gpu):
    check_mix_list(mix_env(gpu, 2048).env)


def test_refusals_leave_device_tensors_alone(gpu):
    refusals(str(gpu))
    torch.cuda.synchronize()


def test_captured_graph_equals_eager_launches(gpu):
    """mask -> spec_commit -> hand-over of two sequences (T = 4; the tiny table at its base, the 64 KiB one lazily
    advancing) captured once and replayed three times on a state that moves -- gen_len, the input token, both g_state
    slots, g_spec -- against the same launches made eagerly."""
    S, T, V, dev = 2, 4, 5000, str(gpu)
    me = mix_env(gpu, V)
    cs = cases(me.env, T - 1)
    mix = [cs["tiny_base_even_legal"], cs["limit_adv_odd_legal"]]
    d = me.tables(mix)
    gen = torch.Generator().manual_seed(7)
    srcs = [torch.randn(S * T, V, generator=gen) for _ in range(3)]
    for src in srcs:  # (no sequence ends during the replays)
        src[:, EOS] = -100.0
    for t in range(T - 1):  # first replay: sequence 0 accepts its k legal drafts, sequence 1 the first of them
        srcs[0][t, mix[0]["draft"][t]] = 100.0
    srcs[0][T, mix[1]["draft"][0]] = 100.0

    def state():
        o, _ = operands(me, mix, T)
        mk = lambda v: torch.tensor(v, **I32).to(dev)  # noqa: E731
        o.update(logits=torch.zeros(S * T, V, device=dev), src=torch.zeros(S * T, V, device=dev),
                 out=torch.zeros(S, 64, **I32).to(dev), pos=mk([40, 70]), limit=mk([64, 64]), eos_on=mk([1, 1]),
                 stats=torch.zeros(S, 3, dtype=torch.int64, device=dev),
                 part=torch.empty(S * T * ((V + 4095) // 4096), device=dev, dtype=torch.int64))
        return o

    def step(o):
        o["logits"].copy_(o["src"])
        verify_call(d, o["logits"], o)
        ops.spec_commit(o["logits"], o["dr"], o["stats"], o["out"], o["gl"], o["ii"], o["pos"], o["fin"], d["eos"],
                        o["limit"], o["eos_on"], part=o["part"])
        ops.dfa_spec_advance(o["on"], o["g_state"], o["g_spec"], o["gl"], T - 1)

    eager, snaps = state(), []
    for src in srcs:
        eager["src"].copy_(src)
        step(eager)
        snaps.append({k: v.clone() for k, v in eager.items()})
    torch.cuda.synchronize()
    o = state()
    o["src"].copy_(srcs[0])
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(o)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for src, want in zip(srcs, snaps):
        o["src"].copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for k in ("logits", "g_state", "g_spec", "gl", "ii", "fin", "out", "pos", "stats"):
            assert torch.equal(o[k], want[k]), k
    stats = o["stats"].tolist()
    assert stats[0][0] == 3 and stats[0][2] >= K and stats[1][2] >= 1 and o["gl"].tolist()[0] >= mix[0]["n"] + K + 3


# ------------------------------------------------------------------------------------------------ engine
def make(gpu, model, **flags):
    return build_engine(model, device=str(gpu), max_slots=4, max_model_len=512, seed=0, **flags)


def matches(eng, reqs, reqs_spec):
    for q, (p, o) in zip(reqs, reqs_spec):
        if "regex" in o:
            res = eng.result(q)
            assert re.fullmatch(o["regex"], res.text) and res.done_reason == "stop", res.text


def base_run(gpu, model, name):
    """The verify path's own tokens: the case on a spec_batch_guided engine with n-gram drafts."""
    reqs_spec, flags = CASES[name]
    eng = make(gpu, model, **flags)
    calls = spy(eng)
    reqs, batched = run(eng, reqs_spec)
    matches(eng, reqs, reqs_spec)
    sampled = any(params(o, 1).needs_sampler for _, o in reqs_spec)
    assert batched > 0 and (True, sampled, 2 if len(reqs_spec) == 2 else 4) in calls
    assert eng.stats["guided_steps"] > 0 and eng.stats["spec_steps"] == sum(q.spec_steps for q in reqs)
    return eng, [q.output_ids for q in reqs]


@pytest.mark.parametrize("name", ["pair", "with_free"])
@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_planted_drafts_repeat_the_base_run(gpu, model, name):
    """Planted drafts on fresh engines: every arm takes the same verify kernels, so the tokens agree exactly whatever is
    drafted (the argument of test_spec_gpu.py::test_engine_forced_drafts), and the acceptance counts are exact -- for
    the request in slot 0, which speculates all its life, and for every other one that does not outlive it (left alone
    in another slot a request ends on plain steps)."""
    reqs_spec, flags = CASES[name]
    _, want = base_run(gpu, model, name)
    for kind, per in (("right", K), ("wrong", 0), ("first", 1)):
        eng = make(gpu, model, **flags)
        eng.runner.set_spec_forced(planted(want, [kind] * len(want), eng.runner.V).to(gpu))
        reqs, batched = run(eng, reqs_spec)
        assert [q.output_ids for q in reqs] == want, kind
        matches(eng, reqs, reqs_spec)
        steps = [-(-(len(w) - 1) // (per + 1)) for w in want]
        for s, (q, w) in enumerate(zip(reqs, want)):
            if s == 0 or steps[s] <= steps[0]:
                assert (q.spec_steps, q.spec_accepted) == (steps[s], len(w) - 1 - steps[s]), (kind, s)
        assert batched > 0


def spec_keys(eng):
    return [k for k in eng.runner.graphs if k[0] == "spec"]


def batched_guided(k):
    """A key of the guided verify graph over several sequences: (.., True, S) or (.., True, "sample", S)."""
    return len(k) >= 6 and k[4] is True and isinstance(k[-1], int) and k[-1] > 1


def test_engine_graph_keys(gpu):
    eng, _ = base_run(gpu, "tiny-nsql", "pair")
    assert eng.runner.use_graphs
    assert any(len(k) == 6 and k[4] is True and k[5] == 2 for k in spec_keys(eng)), spec_keys(eng)
    eng, _ = base_run(gpu, "tiny-nsql", "three")  # a sampled neighbour: the guided graph that ends in the sampled commit
    assert any(len(k) == 7 and k[4:] == (True, "sample", 4) for k in spec_keys(eng)), spec_keys(eng)
    # an all-free run on that engine adds only the unguided batched key
    before = set(spec_keys(eng))
    g0 = eng.stats["guided_steps"]
    reqs, batched = run(eng, [(p, {}) for p in PROMPTS], 24)
    new = [k for k in spec_keys(eng) if k not in before and isinstance(k[-1], int) and len(k) > 4]
    assert batched > 0 and eng.stats["guided_steps"] == g0
    assert len(new) == 1 and len(new[0]) == 5 and new[0][4] == 4, new
    assert not any(batched_guided(k) for k in spec_keys(eng) if k not in before)
    # an engine built without the flag: a constrained request makes the run plain, and every key has a shape it had
    off = make(gpu, "tiny-nsql", **{k: v for k, v in ALL.items() if k != "spec_batch_guided"})
    assert off.runner.spec_batch_guided is False and off.runner.g_spec.numel() == 9
    run(off, WITH_FREE)
    run(off, [(p, {}) for p in PROMPTS[:2]], 16)
    run(off, WITH_FREE[:1])
    run(off, CASES["three"][0][1:])
    keys = spec_keys(off)
    assert keys and not any(batched_guided(k) for k in keys)
    shapes = {(len(k),) + tuple(x if isinstance(x, (bool, str)) else "S" for x in k[4:]) for k in keys}
    assert shapes <= {(4,), (5, True), (5, "sample"), (5, "S"), (6, True, "sample"), (6, "sample", "S")}, shapes
    assert (5, True) in shapes and (5, "S") in shapes and (6, "sample", "S") in shapes
    dec = [k for k in off.runner.graphs if k[0] != "spec"]
    assert dec and all(len(k) == 3 or (len(k) == 4 and k[3] is True) for k in dec), dec
