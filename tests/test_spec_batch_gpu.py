"""Speculative decoding for several concurrent greedy requests on the GPU (``spec_batch``): attn_verify over S
sequences against its own one-sequence launches (bitwise) and the decode reference, the S-row commit and the
per-sequence planted drafts against their host twins, and the engine's batched verify steps (captured graphs)."""
import dataclasses

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import LLMEngine, ModelRunner, SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.eval import numerics as nm
from llm_based_apache_spark_optimization_amd.models import get_spec
from llm_based_apache_spark_optimization_amd.models.llama import init_random
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_spec_batch_cpu import PROMPTS, forced_tables, run_commit_rows, run_draft_rows
from test_spec_cpu import K

pytestmark = pytest.mark.gpu

I32 = dict(dtype=torch.int32)
D, MB = 128, 16
POS0 = (0, 63, 700)  # no prior context | row 0 ends a block | several splits: three eff_split paths side by side


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ attn_verify
def verify_case(gpu, H, Hkv, T, pos0s, fp8=False, idle=()):
    """A cache holding the T appended rows of every sequence (sequence s owns its own blocks; an ``idle`` sequence is
    the released row: pos0 = 0 and a block table of zeros, i.e. scratch block 0).  Returns what attn_verify reads."""
    S = len(pos0s)
    g = torch.Generator().manual_seed(1000 * H + 10 * T + S)
    nblocks = S * MB + 1
    if fp8:
        k8, ks = ref.quant_kv_rows(torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5)
        v8, vs = ref.quant_kv_rows(torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5)
        kc, vc = ref.kv8_physical(k8).contiguous().to(gpu), ref.kv8_physical(v8).contiguous().to(gpu)
        kvs = (ks.contiguous().to(gpu), vs.contiguous().to(gpu))
    else:
        kc = (torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(gpu)
        vc = (torch.randn(nblocks, Hkv, 64, D, generator=g) * 0.5).to(torch.bfloat16).to(gpu)
        kvs = None
    bt = torch.zeros(S, MB, **I32)
    for s in range(S):
        if s not in idle:
            bt[s] = 1 + s * MB + torch.randperm(MB, generator=g).to(torch.int32)
    bt = bt.to(gpu)
    pos0 = torch.tensor(pos0s, **I32).to(gpu)
    cos, sin = ref.rope_tables(D, MB * 64, 10000.0, None, device=gpu)
    qkv = (torch.randn(S * T, (H + 2 * Hkv) * D, generator=g) * 0.7).to(torch.bfloat16).to(gpu)
    pos = (pos0.view(S, 1) + torch.arange(T, **I32).to(gpu).view(1, T)).reshape(-1).contiguous()
    seq = (torch.arange(S * T, device=gpu) // T).to(torch.int32)
    q = torch.zeros(S * T, H, D, dtype=torch.bfloat16, device=gpu)
    ops.rope_append(qkv, pos, seq, bt, cos, sin, q, kc, vc, H, Hkv, kv_scales=kvs)
    return dict(q=q.view(S, T, H, D), kc=kc, vc=vc, bt=bt, pos0=pos0, pos=pos, seq=seq, kvs=kvs)


def plans_for(Hkv, T):
    nblk = (max(POS0) + T + 63) // 64
    return {"default": ops.verify_split_plan(Hkv, MB * 64, 3), "unsplit": (nblk, 1, 4),
            "one_block_per_split": (1, nblk, 0), "16k": ops.verify_split_plan(Hkv, 16384)}


def launch(c, H, Hkv, plan, seqs=None):
    """attn_verify over the sequences ``seqs`` of the case (all, in one launch, by default) -> (out, tickets)."""
    S, T = c["q"].shape[:2]
    sel = list(range(S)) if seqs is None else list(seqs)
    ws = ops.verify_workspace(T, H, Hkv, plan[1], c["q"].device, S=len(sel))
    out = torch.full((len(sel) * T, H * D), 7.0, dtype=torch.bfloat16, device=c["q"].device)
    if seqs is not None and len(sel) == 1:  # the one-sequence form
        s = sel[0]
        ops.attn_verify(c["q"][s], c["kc"], c["vc"], c["bt"][s:s + 1], c["pos0"][s:s + 1], H, Hkv, D ** -0.5, out,
                        workspace=ws, plan=plan, kv_scales=c["kvs"])
    else:
        ops.attn_verify(c["q"][sel].contiguous(), c["kc"], c["vc"], c["bt"][sel].contiguous(), c["pos0"][sel].contiguous(),
                        H, Hkv, D ** -0.5, out, workspace=ws, plan=plan, kv_scales=c["kvs"])
    return out, ws[2]


def check_batch(gpu, H, Hkv, T, fp8):
    G = H // Hkv
    c = verify_case(gpu, H, Hkv, T, POS0, fp8)
    S = len(POS0)
    want = torch.zeros(S * T, H, D, dtype=torch.bfloat16, device=gpu)
    ref.attn_decode(c["q"].view(S * T, H, D), c["kc"], c["vc"], c["bt"][c["seq"].long()], c["pos"], H, Hkv, D ** -0.5,
                    want, c["kvs"])
    for name, plan in plans_for(Hkv, T).items():
        out, tickets = launch(c, H, Hkv, plan)
        assert torch.isfinite(out.float()).all(), (T, name)
        assert int(tickets.abs().sum()) == 0, (T, name)  # the tickets are left zeroed
        for s in range(S):
            one, _ = launch(c, H, Hkv, plan, seqs=[s])
            assert torch.equal(out[s * T:(s + 1) * T], one), (T, name, s)  # nothing depends on the neighbours
        for row in range(S * T):
            e = _rel(out.view(S * T, H, D)[row], want[row])
            assert e < 1e-2, (T, name, row, e, G)
        again, _ = launch(c, H, Hkv, plan)
        assert torch.equal(out, again), (T, name)


@pytest.mark.parametrize("H,Hkv", [(32, 32), (24, 8)])
def test_attn_verify_three_sequences_bf16(gpu, H, Hkv):
    for T in sorted({2, min(8, 16 // (H // Hkv))}):
        check_batch(gpu, H, Hkv, T, fp8=False)


def test_attn_verify_three_sequences_fp8(gpu):
    check_batch(gpu, 24, 8, 2, fp8=True)


def test_attn_verify_idle_sequence_and_limits(gpu):
    """A fourth, idle sequence (pos0 = 0, block table of zeros) leaves its neighbours' outputs unchanged; S * T > 32 and
    S > 8 are refused with an exception, not a launch."""
    H, Hkv, T = 8, 8, 4
    c = verify_case(gpu, H, Hkv, T, POS0 + (0,), idle=(3,))
    for name, plan in plans_for(Hkv, T).items():
        out, tickets = launch(c, H, Hkv, plan)
        three, _ = launch(c, H, Hkv, plan, seqs=[0, 1, 2])
        assert torch.equal(out[:3 * T], three), name
        assert torch.isfinite(out.float()).all() and int(tickets.abs().sum()) == 0, name
    ws = ops.verify_workspace(8, H, Hkv, 4, gpu, S=8)
    bf = dict(dtype=torch.bfloat16, device=gpu)
    for S, T_ in ((5, 8), (9, 2)):  # 40 rows | 9 sequences
        out = torch.full((S * T_, H * D), 7.0, **bf)
        for call in (ops.attn_verify, ops.ext().attn_verify):
            with pytest.raises((ValueError, RuntimeError)):
                args = (torch.zeros(S, T_, H, D, **bf), c["kc"], c["vc"], torch.zeros(S, MB, **I32).to(gpu),
                        torch.zeros(S, **I32).to(gpu), H, Hkv, D ** -0.5)
                if call is ops.attn_verify:
                    call(*args, out, workspace=ws, plan=(1, 4, 0))
                else:
                    call(*args, 1, 4, 0, out, *ws, None, None)
        assert bool((out == 7.0).all())  # nothing was launched


# ------------------------------------------------------------------------------------------------ commit / draft
@pytest.mark.parametrize("V", [512, 128256])
def test_spec_commit_kernel_rows(gpu, V):
    """S = 4 x T = 4 against ref.spec_commit: state, tokens and per-row stats; a finished row (1) and an all -1 draft
    row (3) among them; and equal to four one-row launches."""
    (st_g, stats_g), (one_g, one_stats_g) = run_commit_rows(4, device=gpu, V=V)
    (st_c, stats_c), _ = run_commit_rows(4, V=V)
    assert torch.equal(stats_g, stats_c) and torch.equal(stats_g, one_stats_g)
    assert stats_c.tolist() == [[1, 3, 2], [0, 0, 0], [1, 3, 1], [1, 0, 0]]
    for key in st_c:
        assert torch.equal(st_g[key], st_c[key]), key
        assert torch.equal(st_g[key], one_g[key]), key


def test_spec_draft_kernel_per_sequence_forced(gpu):
    tables = torch.arange(2 * 10 * K, **I32).view(2, 10, K) + 100
    assert run_draft_rows(tables, device=gpu) == run_draft_rows(tables)
    assert run_draft_rows(tables[0], device=gpu) == run_draft_rows(tables[0])
    assert run_draft_rows(None, device=gpu) == run_draft_rows(None)


# ------------------------------------------------------------------------------------------------ engine
def make(gpu, model="tiny-nsql", **kw):
    return build_engine(model, device=gpu, max_slots=4, max_model_len=512, seed=0, **kw)


def ids_of(eng, prompt):
    """The bare prompt (no template, no system text): with these byte-level tokenizers prompt + generated stays below
    256 tokens, so every split plan is unsplit or one block per split."""
    return eng.encode(prompt)


def send(eng, n, prompts=PROMPTS):
    reqs = [eng.add_request(ids_of(eng, p), SamplingParams(max_tokens=n, ignore_eos=True)) for p in prompts]
    eng.run_until_done(reqs)
    return reqs


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_batched_verify_steps_self_consistent_and_numerics(gpu, model):
    """Per recorded step and request: committed = argmax of verify rows 0 .. a, drafts 0 .. a - 1 equal them, draft a
    does not (or a = k).  Then the bf16 criterion over >= 64 committed tokens of every request.  Prompt + generated
    stays below 256 tokens, so every plan is unsplit or one block per split."""
    eng = make(gpu, model, spec_tokens=K, spec_batch=4)
    k = eng.runner.spec_k()
    ids = [ids_of(eng, p) for p in PROMPTS]
    assert max(map(len, ids)) + 65 <= 256
    toks, elog, steps = nm.record_spec_logits(eng, ids, 64)
    assert any(len(key) > 4 and key[0] == "spec" and key[-1] == 4 for key in eng.runner.graphs), list(eng.runner.graphs)
    for i in range(3):
        assert len(toks[i]) == 65 and sum(s["spec"] for s in steps[i]) >= 8
        for s in steps[i]:
            if not s["spec"]:
                continue
            c, am, dr = s["committed"], s["row_argmax"], s["draft"]
            assert toks[i][s["first"]:s["first"] + c] == am[:c]
            assert dr[:c - 1] == am[:c - 1]
            if s["first"] + c < 65:  # not truncated by the length limit
                assert c - 1 == k or dr[c - 1] != am[c - 1]
        one = tuple(e[i:i + 1] for e in elog) if isinstance(elog, tuple) else elog[i:i + 1]
        good = nm.check_recorded(eng, [ids[i]], [toks[i]], one, 64, (0,), spec_steps=steps[i])
        assert good["ok"] and good["tokens_checked"] >= 64, (i, good)
        if model == "tiny-llama3":
            assert good["tied_head"], good
        print({"request": i, "good": good})


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_planted_drafts_graph_replay_and_mixed_runs(gpu, model):
    """The baseline is the run with "wrong" drafts (wrong against a probe run's tokens; the counts show that every one
    was rejected): one token per row and step, so all rows finish together and every step has the same S * T shape.
    "right" and "first" drafts planted from it reproduce it exactly, with exact counts, all three requests alike, so
    every step of those runs has that shape too; the S > 1 verify graph is captured and a second identical run replays it to identical tokens; a plain run
    after a batched verify run, and the reverse, still match their own earlier outputs."""
    n = 48
    eng = make(gpu, model, spec_tokens=K, spec_batch=4)
    k = eng.runner.spec_k()
    assert k == K
    V = eng.runner.V
    probe = [q.output_ids for q in send(eng, n)]  # n-gram drafts: only something to be wrong against
    eng.runner.set_spec_forced(forced_tables(probe, ("wrong",) * 3, V))
    base = send(eng, n)
    want = [q.output_ids for q in base]
    assert [(q.spec_steps, q.spec_accepted) for q in base] == [(n - 1, 0)] * 3
    assert any(key[0] == "spec" and key[-1] == 4 for key in eng.runner.graphs), list(eng.runner.graphs)
    per = {"right": K, "first": 1, "wrong": 0}
    for kinds in (("right",) * 3, ("first",) * 3, ("wrong",) * 3):
        s0 = dict(eng.stats)
        eng.runner.set_spec_forced(forced_tables(want, kinds, V))
        reqs = send(eng, n)
        assert [q.output_ids for q in reqs] == want, kinds
        for q, kind in zip(reqs, kinds):
            steps = -(-(n - 1) // (per[kind] + 1))
            assert (q.spec_steps, q.spec_accepted) == (steps, n - 1 - steps), kinds
        total = sum(q.spec_steps for q in reqs)
        assert eng.stats["spec_steps"] - s0["spec_steps"] == total
        assert eng.stats["spec_drafted"] - s0["spec_drafted"] == K * total
    # n-gram drafts, twice: the captured graph replays to identical tokens
    eng.runner.set_spec_forced(None)
    a = [q.output_ids for q in send(eng, n)]
    assert [q.output_ids for q in send(eng, n)] == a
    # plain after batched verify, and the reverse, on one engine
    off = [eng.add_request(ids_of(eng, p), SamplingParams(max_tokens=n, ignore_eos=True, speculate=False)) for p in PROMPTS]
    s0 = eng.stats["spec_steps"]
    eng.run_until_done(off)
    p1 = [q.output_ids for q in off]
    assert eng.stats["spec_steps"] == s0
    assert [q.output_ids for q in send(eng, n)] == a
    off = [eng.add_request(ids_of(eng, p), SamplingParams(max_tokens=n, ignore_eos=True, speculate=False)) for p in PROMPTS]
    eng.run_until_done(off)
    assert [q.output_ids for q in off] == p1


@pytest.mark.parametrize("base", ["duckdb-nsql", "llama3.2"])
def test_spec_batch_numerics_check_catches_kv_fault(gpu, base):
    """Production widths, 4 layers, two requests: the batched verify steps pass the bf16 criterion over 64 committed
    tokens each, and fail it with a swapped key pair in the cache layout."""
    spec = dataclasses.replace(get_spec(base), n_layers=4, name=base + "-4l")

    def engine():
        r = ModelRunner(init_random(spec, gpu, seed=5), max_slots=2, max_model_len=512, num_kv_blocks=17, spec_tokens=K,
                        spec_batch=2)
        return LLMEngine(r, name=spec.name)

    g = torch.Generator().manual_seed(3)
    ids = [[1] + torch.randint(3, 30000, (100,), generator=g).tolist() for _ in range(2)]
    eng = engine()
    good = nm.teacher_forced_check_spec(eng, ids, 64)
    for res in good:
        assert res["ok"] and res["tokens_checked"] >= 64 and res["verify_steps"] >= 16, good
    truth = init_random(spec, gpu, seed=5)
    with nm.kv_swap_fault(eng):
        bad = nm.teacher_forced_check_spec(eng, ids, 64, weights=truth)
    assert not any(res["ok"] for res in bad), (good, bad)
    print({"good": good, "bad_kv": bad})
