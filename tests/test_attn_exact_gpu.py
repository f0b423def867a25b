"""Exact tests of the attention kernels (attention.hip, attention_prefill32.hip, attention_verify.hip, kv8.hip): which
keys a row sees, and the error of every single output element.  The builders and checkers are attn_exact.py; their CPU
twins and the mutation checks that show they bite are test_attn_exact_cpu.py.

* ``*_count``: the count construction -- zero K rows, one-hot V rows, finite poison everywhere else -- makes the output
  c / n with c an integer count of the visible keys per residue class; round(out * n) == c is asserted on EVERY element,
  so one key too many, too few, of the wrong kv head or read through the wrong block-table row fails, at any context
  length.
* ``*_bound``: random data against the fp64 reference, |got - o| <= 8 * 2^-9 * sum_j p_j |v_j| on EVERY element
  (attn_exact.BOUND_C: 3 derived -- bf16 P as MFMA operand, rounded P against the f32 row sum, bf16 output -- plus slack
  for accumulation order, the split combine and v_exp_f32).  The worst ratio per kernel variant measured on an MI355X
  is kept in profiles/attn/attn_exact_mi355x.json (written when LSA_ATTN_EXACT_OUT names a file).
"""
import json
import os

import pytest
import torch

import attn_exact as ax
from llm_based_apache_spark_optimization_amd import ops

pytestmark = pytest.mark.gpu

P_KERNELS = ["16", "32", "32pair"]
CACHES = ["bf16", "fp8"]


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("LSA_ATTN_EXACT_OUT")
    if path and ax.RATIOS:
        with open(path, "w") as f:
            json.dump({"unit": "|got - o| / (2^-9 * sum_j p_j |v_j|), worst element", "bound": ax.BOUND_C,
                       "device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
                       "worst": {k: round(v, 3) for k, v in sorted(ax.RATIOS.items())}}, f, indent=1)
            f.write("\n")


def _set_prefill_kernel(monkeypatch, kernel):
    monkeypatch.setattr(ops, "PREFILL_ATTN", kernel[:2])
    monkeypatch.setattr(ops, "PREFILL_PAIR", "1" if kernel.endswith("pair") else "0")


def _max_blocks(lens):
    return (max(lens) + 63) // 64 + 1


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.DECODE_HH)
def test_attn_decode_count(gpu, H, Hkv, cache):
    """G = 1, 2, 3, 4, 8 over contexts on both sides of every block edge in one launch, under the default plan, one
    split, one block per split, the 16k-context grid and a chunk (3) that does not divide the block counts."""
    plans = ax.decode_plans(len(ax.DECODE_LENS), Hkv, _max_blocks(ax.DECODE_LENS))
    ax.decode_count(gpu, H, Hkv, ax.DECODE_LENS, cache == "fp8", plans)


@pytest.mark.parametrize("cache", CACHES)
def test_attn_decode_count_single_buffer(gpu, cache):
    """G = 1 at B = 16, H = Hkv = 32: 512 workgroups, the single-buffer variant."""
    ax.decode_count(gpu, 32, 32, ax.SB_LENS, cache == "fp8", {"default": None})


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.DECODE_HH)
def test_attn_decode_fused_count(gpu, H, Hkv, cache):
    """Fused RoPE + append from 1, 2, 4, 8 (specialised) and 3 (runtime loop) slabs: the new key is counted exactly
    once, its cache row holds exactly the new K and V, no other cache row changes."""
    for nparts in (1, 2, 4, 8, 3):
        ax.decode_fused_count(gpu, H, Hkv, ax.DECODE_LENS, nparts, cache == "fp8", seed=nparts)


@pytest.mark.parametrize("cache", CACHES)
def test_attn_decode_fused_count_single_buffer(gpu, cache):
    ax.decode_fused_count(gpu, 32, 32, ax.SB_LENS, 4, cache == "fp8")


def test_attn_decode_count_xf(gpu):
    """The fragment-major output layout carries the same counts (read back with ``from_xfrag``)."""
    plans = {"default": None, "unsplit": (_max_blocks(ax.DECODE_LENS), 1)}
    ax.decode_count(gpu, 6, 2, ax.DECODE_LENS, False, plans, xf=True)


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.DECODE_HH)
def test_attn_decode_bound(gpu, H, Hkv, cache):
    plans = ax.decode_plans(len(ax.BOUND_LENS), Hkv, _max_blocks(ax.BOUND_LENS))
    ax.decode_bound(gpu, H, Hkv, ax.BOUND_LENS, cache == "fp8", plans, f"decode_{cache}_G{H // Hkv}", seed=H)


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_attn_decode_bound_spike(gpu, H, Hkv, cache):
    """A key of the last split equal to 4 q: the split maxima differ by a large margin and the in-launch combine has to
    rescale; the same bound."""
    lens = [5, 700]
    nblk = _max_blocks(lens) - 1
    plans = {"one_block_per_split": (1, nblk, 0), "chunk2x4": (2, 4, 4)}
    ax.decode_bound(gpu, H, Hkv, lens, cache == "fp8", plans, f"decode_spike_{cache}_G{H // Hkv}", seed=H, spike=True)


# ------------------------------------------------------------------------------------------------ prefill
@pytest.mark.parametrize("kernel", P_KERNELS)
@pytest.mark.parametrize("H,Hkv", ax.PREFILL_HH)
@pytest.mark.parametrize("case", sorted(ax.PREFILL_CASES))
def test_attn_prefill_count(gpu, H, Hkv, case, kernel, monkeypatch):
    """Row t of a sequence counts exactly the keys 0 .. ctx - qlen + t: every row beside every tile and query-block
    edge, fresh and chunked (start positions that are no multiple of 64), and a zero-length sequence in the pack."""
    _set_prefill_kernel(monkeypatch, kernel)
    ax.prefill_count(gpu, H, Hkv, case)


@pytest.mark.parametrize("kernel", P_KERNELS)
@pytest.mark.parametrize("case", ["fresh", "chunked"])
def test_attn_prefill_count_fp8(gpu, case, kernel, monkeypatch):
    _set_prefill_kernel(monkeypatch, kernel)
    ax.prefill_count(gpu, 4, 2, case, fp8=True)


@pytest.mark.parametrize("kernel", P_KERNELS)
@pytest.mark.parametrize("H,Hkv", ax.PREFILL_HH)
@pytest.mark.parametrize("case", ["fresh", "chunked"])
def test_attn_prefill_bound(gpu, H, Hkv, case, kernel, monkeypatch):
    _set_prefill_kernel(monkeypatch, kernel)
    ax.prefill_bound(gpu, H, Hkv, case, False, f"prefill{kernel}_bf16_G{H // Hkv}/{case}", seed=H)


@pytest.mark.parametrize("kernel", P_KERNELS)
@pytest.mark.parametrize("case", ["fresh", "chunked"])
def test_attn_prefill_bound_fp8(gpu, case, kernel, monkeypatch):
    """The reference runs over the e4m3 values times their f32 row scales; the kernels attend to the bf16 scratch of
    kv8.hip, one more rounding of K and V than the bound counts.  It stays inside the same 8 units (measured worst 3.8,
    the largest of any variant)."""
    _set_prefill_kernel(monkeypatch, kernel)
    ax.prefill_bound(gpu, 4, 2, case, True, f"prefill{kernel}_fp8_G2/{case}", seed=4)


# ------------------------------------------------------------------------------------------------ verify
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.VERIFY_HH)
def test_attn_verify_count(gpu, H, Hkv, cache):
    """Row t counts exactly the keys 0 .. pos0 + t, for every T with T * G <= 16, pos0 on both sides of a block edge
    and deep into a context, under the four plans."""
    for T in ax.verify_T(H, Hkv):
        ax.verify_count(gpu, H, Hkv, T, ax.VERIFY_POS0, cache == "fp8", seed=T)


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.VERIFY_HH)
def test_attn_verify_count_batched(gpu, H, Hkv, cache):
    """The S-form: a different pos0 per sequence (0 and 63 side by side) in one launch."""
    for (S, T), pos0s in ax.VERIFY_S_FORMS.items():
        if T * (H // Hkv) <= 16:
            ax.verify_count(gpu, H, Hkv, T, pos0s, cache == "fp8", batched=True, seed=S)


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", ax.VERIFY_HH)
def test_attn_verify_bound(gpu, H, Hkv, cache):
    for T in ax.verify_T(H, Hkv):
        ax.verify_bound(gpu, H, Hkv, T, [0, 63, 700], cache == "fp8", f"verify_{cache}_G{H // Hkv}_T{T}", seed=H + T)


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_attn_verify_bound_spike(gpu, H, Hkv, cache):
    """Key pos0 = 704 (block 11, the last split) equal to 4 q of the last row: the combine has to rescale."""
    T = 4
    plans = lambda p0: {"one_block_per_split": (1, (p0 + T + 63) // 64, 0), "chunk2x4": (2, 4, 4)}  # noqa: E731
    ax.verify_bound(gpu, H, Hkv, T, [704], cache == "fp8", f"verify_spike_{cache}_G{H // Hkv}_T{T}", plans=plans,
                    seed=H, spike=True)
