"""Speculative decoding with fp8 / MXFP4 weights and the fp8 KV cache on the CPU (``spec_quantized``): the verify
steps decode exactly the plain engine's tokens -- the CPU twins compute every verify row as the plain step does -- and
the opt-in gates them."""
import argparse

import pytest
import torch

from llm_based_apache_spark_optimization_amd.config import Settings

from test_spec_cpu import K, PROMPT, SYSTEM, forced_table, gen, make

CONFIGS = [("bf16", "fp8"), ("fp8", "bf16"), ("mxfp4", "fp8")]  # (weights, KV cache)

_plain: dict = {}


def plain(dtype, kv, model="tiny-nsql", n=96):
    """(engine, tokens) of the plain engine of these dtypes, computed once and left unchanged."""
    key = (model, dtype, kv, n)
    if key not in _plain:
        eng = make(model, dtype=dtype, kv_dtype=kv)
        toks = gen(eng, n)
        assert eng.stats["spec_steps"] == 0 and eng.stats["decode_steps"] == n - 1
        _plain[key] = (eng, toks)
    return _plain[key]


@pytest.mark.parametrize("dtype,kv", CONFIGS)
def test_engine_spec_equals_plain_exactly(dtype, kv):
    _, toks = plain(dtype, kv)
    eng = make(dtype=dtype, kv_dtype=kv, spec_tokens=K, spec_quantized=True)
    assert eng.runner.spec_supported()
    assert gen(eng) == toks  # exact: a mismatch is a bug in a CPU twin
    st = eng.stats
    assert st["spec_steps"] + st["spec_accepted"] == 95 and st["spec_accepted"] >= 1


def test_forced_wrong_drafts_fp8_cache_leave_committed_kv_untouched():
    """Three rejected rows per step: the tokens are the plain run's, and the committed context's cache bytes and
    scales equal the plain engine's (a stale row's bytes and scale are both overwritten before any query sees them)."""
    peng, toks = plain("bf16", "fp8")
    eng = make(kv_dtype="fp8", spec_tokens=K, spec_quantized=True)
    eng.runner.set_spec_forced(forced_table(toks, "wrong", eng.runner.V))
    assert gen(eng) == toks
    st = eng.stats
    assert st["spec_steps"] == 95 and st["spec_accepted"] == 0 and st["spec_drafted"] == K * 95
    ctx = len(eng.encode(eng.render(PROMPT, SYSTEM, False))) + 95
    for e in (peng, eng):  # both engines are idle: their requests ran in the same blocks from a fresh arena
        assert e.sched.num_running == 0 and e.runner.kv_fp8
    blocks = list(range(1, 1 + -(-ctx // 64)))
    from llm_based_apache_spark_optimization_amd.ops import reference as ref

    def rows(r):  # token-order bytes [L, 2, Hkv, ctx, 128] and scales [L, 2, Hkv, ctx]
        b = ref.kv8_logical(r.kv[:, :, blocks]).transpose(2, 3).reshape(r.L, 2, r.Hkv, -1, 128)[:, :, :, :ctx]
        s = r.kv_scale[:, :, blocks].transpose(2, 3).reshape(r.L, 2, r.Hkv, -1)[:, :, :, :ctx]
        return b, s

    (a, sa), (b, sb) = rows(eng.runner), rows(peng.runner)
    assert torch.equal(a, b)
    assert torch.equal(sa, sb)


@pytest.mark.parametrize("dtype,kv", CONFIGS)
def test_gating_off_by_default(dtype, kv):
    _, toks = plain(dtype, kv)
    eng = make(dtype=dtype, kv_dtype=kv, spec_tokens=K)
    assert eng.runner.spec_quantized is False and eng.runner.spec_supported() is False
    assert gen(eng, 12) == toks[:12]
    assert eng.stats["spec_steps"] == 0


def test_setting_surfaces(monkeypatch):
    assert Settings().spec_quantized is False
    monkeypatch.setenv("LSA_SPEC_QUANTIZED", "1")
    assert Settings().spec_quantized is True
    monkeypatch.delenv("LSA_SPEC_QUANTIZED")
    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    assert Settings.from_cli(ap.parse_args(["--spec-quantized"])).spec_quantized is True
    assert Settings.from_cli(ap.parse_args([])).spec_quantized is False
    eng = make(spec_tokens=K, spec_quantized=True)  # bf16 weights and cache: supported either way
    assert eng.runner.spec_quantized is True and eng.runner.spec_supported()
    plan = eng.runner.spec_oracle_plan()
    assert plan == dict(qkv=False, gate_up=False, o=False, down=False, rr=False)


def test_gqa_clamp_fp8_cache():
    eng = make("tiny-llama3", kv_dtype="fp8", spec_tokens=9, spec_quantized=True)  # G = 3: T * G <= 16 -> T <= 5
    r = eng.runner
    assert r.H // r.Hkv == 3 and r.spec_k() == 4 and r.spec_supported()
    _, base = plain("bf16", "fp8", "tiny-llama3", 48)
    assert gen(eng, 48) == base and eng.stats["spec_steps"] > 0
