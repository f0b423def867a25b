"""Context shift on the fp8 KV cache, on the GPU: kv_shift8_kernel (csrc/kernels/kv_shift.hip) against the float64
rule, planted tables, the untouched-bytes rule and the host twin; the op's refusals; and the engine generating past
``num_ctx`` on the fp8 cache with captured decode graphs on both tiny specs.  The builders and checkers are
kv_shift8_cases.py; their CPU twins are test_context_shift_fp8_cpu.py."""
import pytest
import torch

import kv_shift8_cases as k8
import kv_shift_cases as ks
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine

pytestmark = pytest.mark.gpu

ODD = [(1, 1, 7, 33, 64), (2, 1, 33, 64, 0)]  # odd bounds on both sides, in place; a copy into the rows behind them


def run(kv, sc, moves, cos, sin):
    out = k8.run_op(kv, sc, moves, cos, sin)
    torch.cuda.synchronize()
    return out


def against_twin(dev, host) -> int:
    """The project's rule for two e4m3 caches written by different code (test_kv_fp8_gpu.py): scales to 1e-5 relative,
    bytes equal except for 1-code differences.  Returns the count of differing bytes."""
    (kd, sd), (kh, sh) = dev, host
    kd, sd = kd.cpu(), sd.cpu()
    assert torch.allclose(sd, sh, rtol=1e-5, atol=0)
    diff = kd != kh
    a, b = kd[diff].int(), kh[diff].int()
    step = ((a & 0x80) == (b & 0x80)) & ((a - b).abs() == 1)   # neighbouring codes of one sign
    zero = ((a & 0x7f) <= 1) & ((b & 0x7f) <= 1)               # or the codes around zero
    assert bool((step | zero).all()), "a byte differs from the twin's by more than one code"
    assert diff.float().mean().item() < 0.01
    return int(diff.sum())


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("kind", ["nsql", "llama3", "mistral"])
@pytest.mark.parametrize("Hkv", [1, 8])
def test_kernel_against_float64(gpu, kind, Hkv):
    """L = 2, NB = 12; three sequences' moves in one launch (in place, forked, rows [5, 64) beside rows [0, 5) with
    delta 0, an empty range, deltas 64, 128 and rows - 64) and one plan with odd bounds on both sides.  Rotated rows
    within the bounds of kv_shift8_cases.py, every other destination byte and scale bit-equal to its source, every
    byte and scale outside the destination rows unchanged; repeatable; equal to each move launched alone; and the
    host twin's bytes and scales by the project's rule for two fp8 caches."""
    cos, sin = ks.tables(kind)
    kv0, sc0 = k8.arena8(Hkv, seed=Hkv + len(kind), wide=True)
    moves = ks.moves_for() + ODD
    dc, ds = cos.to(gpu), sin.to(gpu)
    dev = (kv0.to(gpu), sc0.to(gpu))
    out = run(*dev, moves, dc, ds)
    ratio, serr = k8.check_against(kv0, sc0, *out, moves, cos, sin)
    print(f"worst element error / bound: {ratio:.3f}, worst relative scale error: {serr:.3g}")
    assert 0.0 < ratio <= 1.0
    x1 = k8.dequant(*out)
    assert not x1[:, 0, 3, :, k8.ZERO_ROW].any() and not out[1][:, 0, 3, :, k8.ZERO_ROW].any()
    assert int((x1[0, 0, 3, 0, k8.ONE_ROW] != 0).sum()) == 2
    assert k8.same(run(*dev, moves, dc, ds), out)
    one = (dev[0].clone(), dev[1].clone())
    for m in moves:
        ops.kv_shift8(*one, [m], dc, ds)
    assert k8.same(one, out)
    n = against_twin(out, k8.run_op(kv0, sc0, moves, cos, sin))
    print(f"bytes that differ from the host twin's: {n} of {kv0.numel()}")


def test_kernel_planted_tables(gpu):
    rows, d = 512, 192
    cos, sin = ks.planted(rows, d, gpu)
    kv0, sc0 = k8.arena8(2, seed=3)
    moves = [(3, 3, 0, 64, d), (4, 5, 10, 64, d), (6, 6, 7, 33, d)]
    kv1, sc1 = run(kv0.to(gpu), sc0.to(gpu), moves, cos, sin)
    c0, c1, sc1 = k8.codes(kv0), k8.codes(kv1), sc1.cpu()
    for got, src, rows_ in ((3, 3, slice(0, 64)), (5, 4, slice(10, 64)), (6, 6, slice(7, 33))):
        assert torch.equal(c1[:, 0, got, :, rows_], ks.planted_expect(c0[:, 0, src, :, rows_]))
        a, b = sc1[:, 0, got, :, rows_].double(), sc0[:, 0, src, :, rows_].double()
        assert bool(((a - b).abs() <= 2.0 ** -22 * b).all())
    k8.check_against(kv0, sc0, kv1, sc1, moves, cos.cpu(), sin.cpu())


def test_kernel_production_stride(gpu):
    """28 layers, 4 KV heads (the 7B's arena stride) and a 4096-row table: one in-place move and one fork."""
    cos, sin = ks.tables("mistral", 4096)
    kv0, sc0 = k8.arena8(4, seed=9, NB=5, L=28)
    moves = [(2, 2, 0, 64, 4032), (3, 4, 3, 64, 1024), (1, 4, 0, 3, 0)]
    out = run(kv0.to(gpu), sc0.to(gpu), moves, cos.to(gpu), sin.to(gpu))
    ratio, _ = k8.check_against(kv0, sc0, *out, moves, cos, sin)
    assert 0.0 < ratio <= 1.0


def test_refusals_launch_nothing(gpu, monkeypatch):
    cos, sin = (t.to(gpu) for t in ks.tables("nsql", 512))
    kv, sc = (t.to(gpu) for t in k8.arena8(1, seed=5))
    kv0, sc0 = kv.clone(), sc.clone()
    launches = []
    real = ops.ext().kv_shift8
    monkeypatch.setattr(ops.ext(), "kv_shift8", lambda *a: (launches.append(1), real(*a))[1])
    for name, moves in ks.refusals(kv.shape[2], 512):
        with pytest.raises(ValueError):
            ops.kv_shift8(kv, sc, moves, cos, sin)
    ok = [(3, 4, 0, 64, 64)]
    for args in ((ks.arena(1, seed=5).to(gpu), sc, ok, cos, sin), (kv[0], sc, ok, cos, sin), (kv, None, ok, cos, sin),
                 (kv, sc[..., :32], ok, cos, sin), (kv, sc.double(), ok, cos, sin),
                 (kv, sc, ok, cos.double(), sin.double())):
        with pytest.raises(ValueError):
            ops.kv_shift8(*args)
    ops.kv_shift8(kv, sc, [], cos, sin)
    assert not launches
    mv = torch.tensor(ok, dtype=torch.int32, device=gpu)
    for args in ((kv.view(torch.int8), sc, mv, cos, sin), (kv, sc.double(), mv, cos, sin),
                 (kv, sc[..., :32].contiguous(), mv, cos, sin), (kv, sc, mv.long(), cos, sin),
                 (kv, sc, mv.view(-1), cos, sin), (kv, sc, mv, cos[:, :32].contiguous(), sin[:, :32].contiguous()),
                 (kv[:, :, :, :, :32], sc, mv, cos, sin), (kv, sc.cpu(), mv, cos, sin), (kv, sc, mv, cos.cpu(), sin.cpu())):
        with pytest.raises(RuntimeError):  # the binding repeats the operand checks
            real(*args)
    torch.cuda.synchronize()
    assert k8.same((kv, sc), (kv0, sc0))
    ops.kv_shift8(kv, sc, ok, cos, sin)
    assert launches == [1] and not torch.equal(kv, kv0) and not torch.equal(sc, sc0)


# ------------------------------------------------------------------------------------------------ the engine
PROMPT = [1] + list(range(3, 43))
KW = dict(max_slots=2, max_model_len=512, kv_dtype="fp8")
LONG = dict(max_tokens=300, ignore_eos=True, num_ctx=256)


class StepSpy(k8.ShiftSpy8):
    """``ShiftSpy8`` that also runs the first decode step after each shift twice from the same state -- replayed from
    the captured graph, and eagerly -- and compares everything the step writes, bit for bit."""

    STATE = ("kv", "kv_scale", "positions", "input_ids", "gen_len", "out_tokens", "finished")

    def __call__(self, entries):
        super().__call__(entries)
        r = self.eng.runner
        torch.cuda.synchronize()
        save = {n: getattr(r, n).clone() for n in self.STATE}
        plan = tuple(r.ctx_plan(1, 256))

        def run(step):
            step()
            torch.cuda.synchronize()
            got = {n: getattr(r, n).clone() for n in self.STATE}
            for n in self.STATE:
                getattr(r, n).copy_(save[n])
            return got

        graph = run(lambda: r.decode(1, 1, False, max_ctx=256))
        eager = run(lambda: r._decode_step(1, False, plan, False, False))
        assert r.graph_key(1, False, plan) in r.graphs
        for n in self.STATE:
            assert torch.equal(graph[n].view(torch.uint8), eager[n].view(torch.uint8)), n
        assert not torch.equal(graph["kv"], save["kv"]) and int(graph["gen_len"][0]) == int(save["gen_len"][0]) + 1
        self.stepped = getattr(self, "stepped", 0) + 1


@pytest.mark.parametrize("model", ["tiny-nsql", "tiny-llama3"])
def test_engine_generates_past_the_window(gpu, model):
    """300 tokens through a 256-token window on the fp8 cache with captured graphs: after each shift the cache is within
    the float64 bounds on the pre-shift snapshot (kept rows and V bit-equal), table and position are the rule's, the
    first step after it replays from the graph as it runs eagerly, and the tokens up to the first shift are those of
    the opted-out run."""
    eng = build_engine(model, device=str(gpu), context_shift=True, context_shift_fp8=True, **KW)
    assert eng.runner.use_graphs and eng.context_shift and eng.context_shift_fp8 and eng.runner.kv_fp8
    spy = StepSpy(eng, twin=False)
    try:
        on = eng.generate([PROMPT], SamplingParams(**LONG))[0]
    finally:
        spy.restore()
    off = eng.generate([PROMPT], SamplingParams(shift=False, **LONG))[0]
    print(f"worst element error / bound: {spy.worst[0]:.3f}, worst relative scale error: {spy.worst[1]:.3g}")
    assert on.eval_count == 300 and on.done_reason == "length" and on.context_shifts >= 2
    assert spy.checked == spy.stepped == on.context_shifts and spy.keeps == [4] * spy.checked
    assert 0.0 < spy.worst[0] <= 1.0
    assert off.eval_count == 215 and off.context_shifts == 0 and on.token_ids[:215] == off.token_ids
    assert eng.stats["context_shifts"] == on.context_shifts and eng.runner.graphs
    assert eng.sched.num_running == 0 and eng.sched.free_blocks == eng.runner.num_kv_blocks - 1


@pytest.mark.parametrize("flags", [dict(context_shift=True), dict(context_shift=True, context_shift_fp8=True)])
def test_flags_off_is_todays_fp8_engine(gpu, flags):
    """``context_shift`` alone (inert on the fp8 cache), and both flags while nobody shifts: the same graph keys, launch
    counts, tokens and statistics as the fp8 engine without them."""
    kw = dict(device=str(gpu), **KW)
    plain, eng = build_engine("tiny-nsql", **kw), build_engine("tiny-nsql", **flags, **kw)
    both = "context_shift_fp8" in flags
    assert eng.context_shift is both and eng.context_shift_fp8 is both
    a = plain.generate([PROMPT], SamplingParams(**LONG))[0]
    b = eng.generate([PROMPT], SamplingParams(shift=not both, **LONG))[0]
    assert a.token_ids == b.token_ids and len(a.token_ids) == 215 and a.done_reason == b.done_reason == "length"
    assert set(plain.runner.graphs) == set(eng.runner.graphs) and plain.runner.graphs
    for B in (1, 2):
        assert plain.runner.count_step_kernels(B) == eng.runner.count_step_kernels(B)
    drop = ("prefill_s", "decode_s", "decode_device_s")
    want = {k: v for k, v in plain.stats.items() if k not in drop}
    got = {k: v for k, v in eng.stats.items() if k not in drop}
    if both:
        assert got.pop("context_shifts") == 0 and got.pop("context_shift_tokens") == 0
    assert got == want and b.context_shifts == 0
    assert not plain.context_shift and "context_shifts" not in plain.stats
