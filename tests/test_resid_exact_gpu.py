"""Per-element and exact tests of the residual-stream kernels (csrc/kernels/norm_rope.hip: add_rmsnorm_kernel,
rmsnorm_xf_kernel, res_add_ss_kernel, rope_append_kernel with the bf16 and the fp8 cache, the three SiLU kernels) and of
the RoPE / KV-append epilogue of the prefill GEMM.  Builders and checkers are in tests/resid_exact.py, the same ones run
over the host paths with mutation checks in tests/test_resid_exact_cpu.py.

"Exact" = asserted on EVERY output element, no norm ratio and no tolerated share: ``torch.equal`` on the constructions
whose float64 result is representable (f32 sums from left to right, the planted rotation table on dyadic inputs, fp8 rows
that quantise exactly), sentinel-filled outputs whose every element outside the written set keeps its bits, and
``bf16(y - e) <= got <= bf16(y + e)`` against float64 on random data with the slack e derived in resid_exact.py.  The
worst share of e measured on an MI355X is kept in profiles/resid/resid_exact_mi355x.json
(scripts/resid_exact_margins.py)."""
import pytest
import torch

import resid_exact as rx
from llm_based_apache_spark_optimization_amd import ops

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("D", rx.NORM_D)
def test_add_rmsnorm_slab_counts(gpu, D):
    """Slab counts 0 .. 9 with 1 .. 5 rows at D = 8 (one vector, 63 idle lanes) .. 8192 (VPT 1) and 8200 / 16384 (VPT 4);
    rows of unit scale, of 1e-3 (eps decides), all zero and of 1e4; h the f32 sum from left to right bit for bit."""
    rx.norm_suite(gpu, D)


@pytest.mark.parametrize("form", rx.NORM_FORMS[1:])
def test_add_rmsnorm_forms(gpu, form):
    """ids + emb (a repeated id and id V - 1), row_idx (out of order, repeated, write_h False), raw mode with 0 and 2
    zeroed accumulators, the fragment-major output and the e4m3 output, at every D that takes them."""
    rx.norm_forms_suite(gpu, form)


def test_add_rmsnorm_spike_rows(gpu):
    """Sixteen rows at D = 8192, row k with one element 2^12 times the rest inside wave k's columns: a block reduction
    that misses any of the sixteen waves fails the bound on that row."""
    rx.norm_spike_suite(gpu)


@pytest.mark.parametrize("rows", [65, 71, 80])
def test_rmsnorm_xf_kernel(gpu, rows):
    """The 8-rows-per-workgroup prefill norm at D = 32 / 160 / 4096: partial last tiles, spike rows in every lane
    group, h bit-unchanged, the guard zone after the last tile untouched."""
    with rx.forced_xf_kernel():
        rx.norm_xf_suite(gpu, rows)


@pytest.mark.parametrize("D", rx.RES_D)
def test_res_add_ss(gpu, D):
    """h and its bf16 copy exact for 0 .. 9 slabs x 1 / 5 / 33 rows, the Q24 row sums within their bound and bitwise
    repeatable, rows and accumulators past ``rows`` untouched."""
    rx.res_suite(gpu, D)


# ------------------------------------------------------------------------------------------------ rope + append
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
@pytest.mark.parametrize("HH", rx.ROPE_HH)
def test_rope_append_exact(gpu, HH, cache):
    """The planted table on dyadic rows (fp8: rows that quantise exactly): q, the appended K / V rows, bytes and scales
    bit-equal to the float64 result for bf16 rows and 1 / 2 / 3 / 4 / 5 / 8 slabs, with and without tok_seq; every
    other slot of q_out, the caches and the scale planes keeps its sentinel."""
    rx.rope_suite(gpu, HH, "planted8" if cache == "fp8" else "planted")


@pytest.mark.parametrize("cache", ["bf16", "fp8"])
@pytest.mark.parametrize("HH", [(4, 2), (24, 8)])
def test_rope_append_bound(gpu, HH, cache):
    """Random data under the model's tables: q and K within 2^-22 (|x0 c| + |x1 s|) of float64 (fp8 K rows: the
    one-quantisation rule), V rows bit-equal to bf16(f32 slab sum) / ``quant_kv_rows`` of it."""
    rx.rope_suite(gpu, HH, "real8" if cache == "fp8" else "real")


@pytest.mark.parametrize("cfg", rx.GEMM_ROPE_CFGS)
def test_gemm_rope_epilogue_exact(gpu, cfg):
    """Prefill qkv GEMM with the RoPE + append epilogue on integer x and w and the planted table: q and every appended
    row equal the float64 result, every other slot keeps its sentinel."""
    rx.gemm_rope_run(rx.gemm_rope_case(), gpu, cfg)


# ------------------------------------------------------------------------------------------------ SiLU
def test_silu_kernels(gpu):
    """silu_parts (F 16 / 48 / 512, M 1 / 3, 1 - 3 slabs), silu_mul (n 8 / 2056), silu_bf16 (F 16 / 48): every element
    within 2^-12 |y| of float64, gate = +-100 planted, the guard zone untouched."""
    rx.silu_small_suite(gpu, bf16_fn=rx.silu_bf16_fn)


@pytest.mark.parametrize("kernel", ["parts", "mul", "bf16"])
def test_silu_past_the_grid_cap(gpu, kernel):
    """One case each just past what one pass of the capped grid covers: the stride loop's second trip, whole tensor."""
    if kernel == "parts":
        rx.silu_parts_check(ops.silu_parts, gpu, 1, rx.SILU_PARTS_CAP + 4096, 1, key="silu_parts/cap")
    elif kernel == "mul":
        rx.silu_mul_check(ops.silu_mul, gpu, rx.SILU_MUL_CAP + 2056, key="silu_mul/cap")
    else:
        rx.silu_bf16_check(rx.silu_bf16_fn, gpu, 1, rx.SILU_BF16_CAP + 4096, key="silu_bf16/cap")
