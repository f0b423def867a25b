"""Case builders and checkers of the exact tests of the residual-stream kernels (csrc/kernels/norm_rope.hip and the
RoPE / KV-append epilogue of the prefill GEMM): test_resid_exact_cpu.py runs them over the host paths of ``ops``,
test_resid_exact_gpu.py over the HIP kernels.  Every case is built on the host and moved to ``device``; every runner
takes the op as an argument, so a deliberately wrong host function goes through the same checker.

"Exact" here means: asserted on EVERY output element -- no norm ratio, no tolerated share.  Two instruments:

* exact constructions (``check_exact``, a ``torch.equal``): residual sums are f32 adds from left to right, which no
  contraction changes, so h is the same sum in torch bit for bit and the raw bf16 copy is ``h.to(bfloat16)``; the
  rotation runs over a planted cos / sin table with entries from {0, +-1, +-0.5} (another pattern at every (position,
  d), so the wrong table row or column changes the result) and dyadic inputs, so every product and sum is exact in f32
  with or without FMA and the result is the float64 one; fp8 rows are e4m3 values times 2^k with an amax of 448 * 2^k,
  so bytes (in token-pair order) and scales are those of ``ops.reference.quant_kv_rows``.  Every output buffer starts
  as a finite non-zero sentinel and ``check_untouched`` asserts that every element outside the written set, computed
  here from pos / tok_seq / block_tables, keeps its bits.
* bounds against float64 on random data (``within_bf16``): bf16(y - e) <= got <= bf16(y + e) with y the float64 result
  from the kernel's own exact inputs (for slabs: their f32 sum from left to right) and e the f32 slack
    RMSNorm   2^-16 |y|   (sum of squares: <= 32 sequential + ~10 tree roundings < 2^-18; rsqrtf and two multiplies < 2^-21)
    RoPE      2^-22 (|x0 c| + |x1 s|)   (two roundings, or one with FMA)
    SiLU * up 2^-12 |y| + 1e-30   (__expf has no written bound here; 8 times finer than bf16's half ulp 2^-9, so any
              intermediate bf16 rounding or a wrong pairing is separated from f32 arithmetic)
  fp8 rows (one quantisation): dequantised element within 2^-4 |y| + 2^-10 scale + 2^-20 amax, scale within 2^-20 of
  amax / 448 (the rule of tests/kv_shift8_cases.py for one rounding); Q24 row sums within 2^-18 sum + nwaves 2^-24.
  None of these is fitted to a kernel's output; ``RATIOS`` keeps the worst err / e per family.
"""
import contextlib

import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

HD = 128
BF16, F32, I32, I64, U8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8
SENTINEL = {F32: -777.25, BF16: -776.0, U8: 0x5A, I64: 0x5A5A5A5A5A5A, I32: 0x5A5A5A}
EPS = 1e-5

RATIOS: dict = {}  # worst err / e per family, filled by the bound checkers


def sentinel(shape, dtype, device="cpu"):
    return torch.full(shape if isinstance(shape, (tuple, list)) else (shape,), SENTINEL[dtype], dtype=dtype, device=device)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _record(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))
    return float(ratio)


# ------------------------------------------------------------------------------------------------ checkers
def check_exact(got, want, tag):
    """``torch.equal`` with the first differing index in the message."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"exact {tag}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if not torch.equal(got, want):
        bad = ~(got == want)
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"exact {tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got "
                             f"{got[i].item()!r}, want {want[i].item()!r}")


def check_untouched(got, init, written, tag):
    """Every element outside ``written`` (bool, broadcastable from the leading dims; None = nothing written) keeps the
    bits it had before the call."""
    g, b = _bits(got), _bits(init)
    bad = g != b
    if written is not None:
        w = written.detach().cpu()
        bad &= ~w.reshape(tuple(w.shape) + (1,) * (bad.dim() - w.dim()))
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"sentinel {tag}: {int(bad.sum())} elements outside the written set changed, first at {i}")


def _bf16_cell(got):
    """[lo, hi] in float64: the reals that round to the bf16 value ``got`` (ties included)."""
    mag = _bits(got.to(BF16)).to(torch.int32) & 0x7FFF
    val = lambda m: (m << 16).view(F32).double()
    a = val(mag)
    dn = torch.where(mag > 0, val((mag - 1).clamp_min(0)), -val(torch.ones_like(mag)))
    return (a + dn) / 2, (a + val(mag + 1)) / 2


def within_bf16(got, y, e, key, tag=""):
    """bf16(y - e) <= got <= bf16(y + e) on EVERY element (float64 -> f32 -> bf16 is monotonic, so an f32 value within e
    of y passes whatever it rounds to).  Records and returns the worst share of e that any element needs: the
    distance from y to the reals rounding to ``got``, over e."""
    got = got.detach().cpu()
    y, e = y.detach().cpu().double(), e.detach().cpu().double()
    g = got.double().reshape(y.shape)
    lo, hi = (y - e).to(F32).to(BF16).double(), (y + e).to(F32).to(BF16).double()
    sg = torch.where(torch.signbit(g), -1.0, 1.0)
    clo, chi = _bf16_cell(got.reshape(y.shape))
    d = torch.maximum(clo - sg * y, sg * y - chi).clamp_min(0)
    ratio = float((d / e.clamp_min(1e-300)).max()) if d.numel() else 0.0
    _record(key, ratio)
    bad = ~((lo <= g) & (g <= hi))  # a NaN is bad
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"bound {key} {tag}: {int(bad.sum())} of {bad.numel()} elements outside bf16(y -+ e) (worst "
                             f"needs {ratio:.3g} e), first at {i}: got {float(g[i])!r}, y {float(y[i])!r}, e {float(e[i]):.3e}")
    return ratio


def check_fp8_rows(codes, scale, y, key, tag=""):
    """One quantisation of the float64 rows ``y`` [..., n] into e4m3 ``codes`` (uint8, logical order) with row scales
    ``scale`` [...]: scale within 2^-20 of amax / 448 (rows with amax > 0; finite elsewhere), dequantised element within
    2^-4 |y| + 2^-10 scale + 2^-20 amax.  Returns the worst element error / bound."""
    codes, scale, y = codes.detach().cpu(), scale.detach().cpu().double(), y.detach().cpu().double()
    amax = y.abs().amax(-1)
    sc = amax / 448.0
    serr = (scale - sc).abs()
    bad = ~(torch.isfinite(scale) & ((serr <= 2.0 ** -20 * sc) | (amax == 0)))
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"bound {key} {tag}: {int(bad.sum())} scales beyond 2^-20 of amax / 448, first at {i}: got "
                             f"{float(scale[i])!r}, want {float(sc[i])!r}")
    got = codes.view(torch.float8_e4m3fn).double() * scale.unsqueeze(-1)
    bound = 2.0 ** -4 * y.abs() + (2.0 ** -10 * sc + 2.0 ** -20 * amax).unsqueeze(-1)
    err = (got - y).abs()
    bad = ~(err <= bound)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    _record(key, ratio)
    nz = amax > 0
    _record(key + "/scale", float((serr[nz] / (2.0 ** -20 * sc[nz])).max()) if bool(nz.any()) else 0.0)
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"bound {key} {tag}: {int(bad.sum())} elements past the fp8 bound (worst {ratio:.3g}), first at "
                             f"{i}: got {float(got[i])!r}, y {float(y[i])!r}")
    return ratio


def check_q24(ss, base, h32, nwaves, key, tag=""):
    """|ss_float - sum h^2| <= 2^-18 sum h^2 + nwaves 2^-24 per row (``base``: what the accumulator held, in Q24)."""
    want = h32.detach().cpu().double().pow(2).sum(-1)
    got = (ss.detach().cpu() - base).double() / ops.SS_SCALE
    e = 2.0 ** -18 * want + nwaves * 2.0 ** -24
    err = (got - want).abs()
    ratio = _record(key, float((err / e).max()))
    bad = ~(err <= e)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"bound {key} {tag}: row sum {i} off by {float(err[i]):.3e} (bound {float(e[i]):.3e})")
    return ratio


def slab_sum32(v, parts):
    """v + parts[0] + parts[1] + ... in f32 from left to right (v None: starts from parts[0])."""
    v = v.float() if v is not None else None
    for s in range(parts.shape[0] if parts is not None else 0):
        v = parts[s].float().clone() if v is None else v + parts[s].float()
    return v


# ------------------------------------------------------------------------------------------------ add_rmsnorm
NORM_D = [8, 136, 520, 4096, 8192, 8200, 16384]
NORM_MAGS = [1.0, 1e-3, 0.0, 1e4, 1.0]  # unit, eps matters (1e-5 against a variance of 1e-6), all-zero row, large
NORM_FORMS = ["plain", "ids", "row_idx", "raw0", "raw2", "xf", "x8"]


def norm_form_ok(form, D):
    return {"xf": D % 32 == 0, "x8": D % 128 == 0}.get(form, True)


def spike_rows(h, period):
    """Row k < 16 gets one element 2^12 times the rest at a column of the k-th ``period``-column stretch (the columns of
    wave k of the row-per-workgroup kernel at D = 8192, period 512): a reduction that loses that wave, or that lane,
    changes the row's scale by far more than any bound."""
    D = h.shape[1]
    for k in range(min(16, h.shape[0])):
        h[k, (k * period + 29 * k + 5) % D] = 4096.0 * (-1) ** k
    return h


def norm_case(D, nparts, rows, form="plain", seed=0, spikes=False, slab_mag=1.0, h_mag=1.0):
    """Host tensors of one add_rmsnorm call.  The slabs are a row-sliced view of a taller buffer (part_stride != rows * D);
    h is taller than the rows in use and every output has a guard zone."""
    g = torch.Generator().manual_seed(seed * 7919 + D * 31 + nparts)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(D=D, rows=rows, form=form, nparts=nparts)
    nh = 5 if form == "row_idx" else rows
    mags = torch.tensor([NORM_MAGS[(r + nparts) % 5] for r in range(nh)]).view(-1, 1)
    if spikes:
        mags = torch.ones(nh, 1)
    if form.startswith("raw"):  # the Q24 int64 row sum holds sum h^2 < 2^39: rows of 1e4 at D = 4096 are outside its range
        mags = mags.clamp_max(1e2)
    h = sentinel((nh + 2, D), F32)
    h[:nh] = rn(nh, D) * mags * h_mag
    if spikes:
        spike_rows(h[:nh], 512)
    c["h"], c["nh"] = h, nh
    c["w"] = (rn(D) * 0.5 + 1).to(BF16)
    if nparts:
        tall = rn(nparts, nh + 3, D) * slab_mag
        tall[:, :nh] *= mags
        c["parts"] = tall[:, :nh]
    else:
        c["parts"] = None
    c["ids"] = c["emb"] = c["row_idx"] = None
    if form == "ids":
        V = 11
        c["emb"] = rn(V, D).to(BF16)
        c["ids"] = torch.tensor([V - 1, 3, 3, 0, 7][:rows], dtype=I32)  # the last id and a repeated one
    if form == "row_idx":
        c["rows"] = rows = 4
        c["row_idx"] = torch.tensor([3, 0, 3, 1], dtype=I32)  # out of order, one repeated
    # the f32 rows the kernel norms: embedding or h, plus the slabs from left to right
    idx = c["row_idx"].long() if c["row_idx"] is not None else torch.arange(rows)
    v0 = c["emb"][c["ids"].long()[idx]].float() if form == "ids" else h[idx]
    c["v32"] = slab_sum32(v0, c["parts"][:, idx] if nparts else None)
    v = c["v32"].double()
    eps32 = torch.tensor(EPS, dtype=F32).double()
    c["y"] = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps32) * c["w"].double()
    return c


def norm_run(fn, c, device):
    """One call of ``fn`` (the signature of ops.add_rmsnorm) on sentinel-filled outputs; everything back on the host."""
    D, rows, form = c["D"], c["rows"], c["form"]
    dev = lambda t: None if t is None else t.to(device)
    h = c["h"].clone().to(device)
    tall = None
    if c["parts"] is not None:
        base = c["parts"]._base if c["parts"]._base is not None else c["parts"]
        tall = base.clone().to(device)
    parts = None if tall is None else tall[:, :c["nh"]]
    xf = form in ("xf", "x8")
    mt = ops.xfrag_tiles(rows)
    G = 64
    xn = sentinel((mt * 16 * D + G) if xf else (rows + 1) * D, BF16, device)
    o = dict(xf=xf)
    kw = dict(parts=parts, ids=dev(c["ids"]), emb=dev(c["emb"]), row_idx=dev(c["row_idx"]),
              write_h=form != "row_idx")
    if form.startswith("raw"):
        nz, ld = int(form[3:]), rows + 3
        ss = sentinel((nz + 2) * ld, I64, device)
        kw.update(ss_out=ss, ss_ld=ld, ss_nzero=nz)
        o.update(ss=ss, ss_ld=ld, nz=nz)
    if form == "x8":
        o["x8"], o["sx8"] = sentinel(mt * 16 * D + G, U8, device), sentinel(rows + 4, F32, device)
        kw.update(x8=o["x8"], sx8=o["sx8"])
    if xf:
        fn(h, dev(c["w"]), EPS, xn, rows=rows, xf=True, **kw)
    else:
        fn(h, dev(c["w"]), EPS, xn[: rows * D].view(rows, D), rows=rows, **kw)
    o.update(h=h, xn=xn, tall=tall)
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}


def norm_rows(c, o):
    """The bf16 output rows [rows, D] of a run (fragment-major layouts unpacked)."""
    D, rows = c["D"], c["rows"]
    return ops.from_xfrag(o["xn"], rows, D) if o["xf"] else o["xn"][: rows * D].view(rows, D)


def norm_check(c, o, key="add_rmsnorm"):
    """Everything one add_rmsnorm call promises.  Returns the worst share of the bound in use."""
    D, rows, form, nh = c["D"], c["rows"], c["form"], c["nh"]
    tag = f"D={D} nparts={c['nparts']} rows={rows} {form}"
    want_h = c["h"].clone()
    if form != "row_idx":
        want_h[:rows] = c["v32"]
    check_exact(o["h"], want_h, tag + " h")  # the left-to-right sum, bit for bit; rows past `rows` keep the sentinel
    if o["tall"] is not None:
        check_untouched(o["tall"], c["parts"]._base, None, tag + " slabs")
    got = norm_rows(c, o)
    mt = ops.xfrag_tiles(rows)
    guard = o["xn"][(mt * 16 * D if o["xf"] else rows * D):]
    check_untouched(guard, sentinel(guard.shape, BF16), None, tag + " xn guard")
    ratio = 0.0
    if form.startswith("raw"):
        check_exact(got, c["v32"].to(BF16), tag + " raw bf16 copy")
        ld, nz = o["ss_ld"], o["nz"]
        ss = o["ss"].view(nz + 2, ld)
        check_q24(ss[0, :rows], 0, c["v32"], 1, key + "/q24", tag)
        check_exact(ss[1: nz + 1, :rows], torch.zeros(nz, rows, dtype=I64), tag + " zeroed accumulators")
        written = torch.zeros(nz + 2, ld, dtype=torch.bool)
        written[: nz + 1, :rows] = True
        check_untouched(ss, sentinel((nz + 2, ld), I64), written, tag + " ss_out")
    else:
        ratio = within_bf16(got, c["y"], 2.0 ** -16 * c["y"].abs(), key, tag)
        zero = c["v32"].abs().amax(-1) == 0
        assert bool((got[zero] == 0).all()), f"exact {tag}: an all-zero row is not exactly zero"
    if form == "x8":
        check_fp8_rows(ops.from_xf8(o["x8"], rows, D), o["sx8"][:rows], c["y"], key + "/x8", tag)
        check_untouched(o["x8"][mt * 16 * D:], sentinel(64, U8), None, tag + " x8 guard")
        check_untouched(o["sx8"][rows:], sentinel(4, F32), None, tag + " sx8 guard")
    return ratio


# ------------------------------------------------------------------------------------------------ rmsnorm_xf (prefill)
def norm_xf_case(rows, D, seed=0):
    g = torch.Generator().manual_seed(seed + rows * 131 + D)
    h = torch.randn(rows, D, generator=g) * torch.tensor([NORM_MAGS[r % 5] for r in range(rows)]).view(-1, 1)
    h[:16] = torch.randn(16, D, generator=g)
    if D >= 64:
        spike_rows(h, 4)
    w = (torch.randn(D, generator=g) * 0.5 + 1).to(BF16)
    v = h.double()
    y = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + torch.tensor(EPS, dtype=F32).double()) * w.double()
    return dict(rows=rows, D=D, h=h, w=w, y=y)


def norm_xf_check(fn, c, device, key="rmsnorm_xf"):
    rows, D = c["rows"], c["D"]
    n = ops.xfrag_tiles(rows) * 16 * D
    h = c["h"].clone().to(device)
    xn = sentinel(n + 64, BF16, device)
    fn(h, c["w"].to(device), EPS, xn, write_h=False, rows=rows, xf=True)
    tag = f"rows={rows} D={D}"
    check_untouched(h, c["h"], None, tag + " h")
    check_untouched(xn[n:], sentinel(64, BF16), None, tag + " guard")  # pad rows of the last tile: unspecified
    return within_bf16(ops.from_xfrag(xn.cpu(), rows, D), c["y"], 2.0 ** -16 * c["y"].abs(), key, tag)


# ------------------------------------------------------------------------------------------------ res_add_ss
RES_D = [8, 520, 2560, 4104]
RES_ROWS = [1, 5, 33]
SS_BASE = 1 << 23  # 0.5 in Q24: the kernel adds on top of what the accumulator holds


def res_case(D, nparts, rows, seed=0, slab_mag=1.0, h_mag=4.0):
    g = torch.Generator().manual_seed(seed * 104729 + D * 17 + nparts * 3 + rows)
    h = sentinel((rows + 2, D), F32)
    h[:rows] = torch.randn(rows, D, generator=g) * h_mag
    # (contiguous slabs: ops.res_add_ss refuses a row-sliced view, its size check counts the view's elements)
    parts = torch.randn(nparts, rows, D, generator=g) * slab_mag if nparts else None
    return dict(D=D, rows=rows, nparts=nparts, h=h, parts=parts, v32=slab_sum32(h[:rows], parts))


def res_run(fn, c, device, xf):
    D, rows = c["D"], c["rows"]
    h = c["h"].clone().to(device)
    tall = c["parts"].clone().to(device) if c["parts"] is not None else None
    n = ops.xfrag_tiles(rows) * 16 * D if xf else rows * D
    xn = sentinel(n + 64, BF16, device)
    ss = sentinel(rows + 3, I64, device)
    ss[:rows] = SS_BASE
    fn(h, tall, xn[:n] if xf else xn[:n].view(rows, D), rows, ss, xf=xf)
    return dict(h=h.cpu(), xn=xn.cpu(), ss=ss.cpu(), xf=xf, n=n, tall=None if tall is None else tall.cpu())


def res_check(c, o, key="res_add_ss"):
    D, rows = c["D"], c["rows"]
    tag = f"D={D} nparts={c['nparts']} rows={rows} xf={o['xf']}"
    want_h = c["h"].clone()
    want_h[:rows] = c["v32"]
    check_exact(o["h"], want_h, tag + " h")
    got = ops.from_xfrag(o["xn"], rows, D) if o["xf"] else o["xn"][: rows * D].view(rows, D)
    check_exact(got, c["v32"].to(BF16), tag + " bf16 copy")
    check_untouched(o["xn"][o["n"]:], sentinel(64, BF16), None, tag + " xn guard")
    check_untouched(o["ss"][rows:], sentinel(3, I64), None, tag + " accumulators past rows")
    if o["tall"] is not None:
        check_untouched(o["tall"], c["parts"], None, tag + " slabs")
    return check_q24(o["ss"][:rows], SS_BASE, c["v32"], (D + 511) // 512, key + "/q24", tag)


# ------------------------------------------------------------------------------------------------ rope tables, layouts
ROPE_HH = [(1, 1), (4, 2), (24, 8), (32, 32), (64, 8)]  # (64, 8): 1152 rotation items, a second trip of the stride loop
ROPE_SLABS = [0, 1, 2, 3, 4, 5, 8]  # 0: bf16 rows
MAX_BLOCKS = 4
MAX_POS = 64 * MAX_BLOCKS


def planted_tables(P=MAX_POS, seed=0, axis=False):
    """cos / sin [P, 64] f32 with entries from {0, +-1, +-0.5}, drawn per (position, d).  axis=True: exactly one of the
    two is non-zero at every entry (a rotated value is then one input times +-1 or +-0.5, so e4m3 inputs stay e4m3),
    and column (3 p + 1) % 64 of row p is (+-1, 0)."""
    g = torch.Generator().manual_seed(1000 + seed)
    vals = torch.tensor([1.0, -1.0, 0.5, -0.5, 0.0])
    if not axis:
        return vals[torch.randint(0, 5, (P, 64), generator=g)], vals[torch.randint(0, 5, (P, 64), generator=g)]
    a = vals[torch.randint(0, 4, (P, 64), generator=g)]
    which = torch.randint(0, 2, (P, 64), generator=g).bool()
    cos, sin = torch.where(which, a, torch.zeros(())), torch.where(which, torch.zeros(()), a)
    p = torch.arange(P)
    cos[p, (3 * p + 1) % 64] = torch.where(p % 2 == 0, 1.0, -1.0)
    sin[p, (3 * p + 1) % 64] = 0.0
    return cos, sin


def slots(pos, tok_seq, bt):
    """(block, slot) of every token, from pos / tok_seq / block_tables alone."""
    seq = tok_seq.long() if tok_seq is not None else torch.arange(pos.shape[0])
    return bt.long()[seq, pos.long() // 64], pos.long() % 64


def rope_layout(decode, seed=0):
    """Positions 0, 63, 64, 127, the last table row, and two tokens in adjacent slots of one block.  Prefill form: three
    sequences, the second starting mid-block; decode form (tok_seq None): one token per sequence, sequences 5 and 6
    sharing a block.  Block ids are scattered and include nblk - 1; every unused table entry names a spare block that
    must keep its sentinel, and the tables are wider than most sequences use."""
    g = torch.Generator().manual_seed(77 + seed)
    nblk = 9
    order = [nblk - 1] + torch.randperm(nblk - 1, generator=g).tolist()
    spare = order[-1]
    if decode:
        pos, seqs, nseq = [0, 63, 64, 127, MAX_POS - 1, 37, 38], list(range(7)), 7
    else:
        pos, seqs, nseq = [0, 63, 64, 127, 37, 38, MAX_POS - 1], [0, 0, 0, 0, 1, 1, 2], 3
    bt = torch.full((nseq, MAX_BLOCKS), spare, dtype=I32)
    i = 0
    for p, s in zip(pos, seqs):
        if decode and s == 6:
            bt[6, 0] = bt[5, 0]
        elif int(bt[s, p // 64]) == spare:
            bt[s, p // 64] = order[i]
            i += 1
    return dict(pos=torch.tensor(pos, dtype=I32), tok_seq=None if decode else torch.tensor(seqs, dtype=I32), bt=bt,
                nblk=nblk, spare=spare, T=len(pos))


def _e4m3_values(shape, g):
    """Random normal e4m3 values with exponent field 5 .. 14: multiples of 2^-5 below 256 whose halves are e4m3 too."""
    m = torch.randint(0, 8, shape, generator=g).double()
    ex = torch.randint(5, 15, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * (1 + m / 8) * torch.exp2(ex - 7)


def rope_case(H, Hkv, S, decode, mode, seed=0):
    """One rope_append call.  S = 0: bf16 rows, S > 0: that many f32 slabs (a row-sliced view of a taller buffer).
    mode: 'planted' / 'planted8' (exact constructions for the bf16 / fp8 cache) or 'real' / 'real8' (random data, the
    model's tables, the float64 bounds)."""
    c = rope_layout(decode, seed)
    T, NH = c["T"], H + 2 * Hkv
    g = torch.Generator().manual_seed(seed * 31 + H * 1009 + Hkv * 13 + S)
    fp8, exact = mode.endswith("8"), mode.startswith("planted")
    if exact:
        c["cos"], c["sin"] = planted_tables(MAX_POS, seed, axis=fp8)
    else:
        c["cos"], c["sin"] = ref.rope_tables(HD, MAX_POS, 10000.0)
    if mode == "planted":
        x = torch.randint(-63, 64, (T, NH, HD), generator=g).double() / 64
        quantum = torch.full((T, NH, 1), 1.0 / 64, dtype=torch.float64)
    elif mode == "planted8":
        k = ((torch.arange(T).view(-1, 1) + 3 * torch.arange(NH).view(1, -1)) % 7 - 3).double().view(T, NH, 1)
        x = _e4m3_values((T, NH, HD), g)
        p = c["pos"].long()
        for t in range(T):  # amax 448 (x 2^k below): K rows where |cos| = 1 and sin = 0, V rows anywhere
            x[t, H:H + Hkv, (3 * int(p[t]) + 1) % 64] = 448.0
            x[t, H + Hkv:, (5 * t + 11) % HD] = -448.0
        x = x * torch.exp2(k)
        quantum = torch.exp2(k - 5)
    if exact:
        if S == 0:
            qkv = x.float().to(BF16).view(T, NH * HD)
            assert torch.equal(qkv.double().view(T, NH, HD), x)
        else:
            tall = torch.zeros(S, T + 2, NH, HD, dtype=torch.float64)
            tall[: S - 1, :T] = torch.randint(-32, 33, (S - 1, T, NH, HD), generator=g).double() * quantum
            tall[S - 1, :T] = x - tall[: S - 1, :T].sum(0)
            tall[:, T:] = SENTINEL[F32]
            qkv = tall.float().view(S, T + 2, NH * HD)[:, :T]
            assert torch.equal(qkv.double().sum(0).view(T, NH, HD), x)  # every order of the f32 adds is exact
        x32 = x.float()
    else:
        if S == 0:
            qkv = torch.randn(T, NH * HD, generator=g).to(BF16)
            x32 = qkv.float().view(T, NH, HD)
        else:
            tall = torch.randn(S, T + 2, NH * HD, generator=g)
            qkv = tall[:, :T]
            x32 = slab_sum32(None, qkv).view(T, NH, HD)
    x = x32.double()
    cs, sn = c["cos"][c["pos"].long()].double().unsqueeze(1), c["sin"][c["pos"].long()].double().unsqueeze(1)
    lo, hi = x[:, : H + Hkv, :64], x[:, : H + Hkv, 64:]
    c["rot"] = torch.cat([lo * cs - hi * sn, hi * cs + lo * sn], -1)
    c["e_rot"] = 2.0 ** -22 * torch.cat([(lo * cs).abs() + (hi * sn).abs(), (hi * cs).abs() + (lo * sn).abs()], -1)
    c.update(H=H, Hkv=Hkv, S=S, fp8=fp8, exact=exact, qkv=qkv, x32=x32, mode=mode, decode=decode)
    return c


def rope_run(fn, c, device, cos=None, sin=None):
    """One call of ``fn`` (the signature of ops.rope_append) on sentinel-filled q_out, caches and scale planes."""
    H, Hkv, T, nblk = c["H"], c["Hkv"], c["T"], c["nblk"]
    if c["S"]:
        qkv = c["qkv"]._base.clone().to(device).view(c["S"], T + 2, -1)[:, :T]
    else:
        qkv = c["qkv"].to(device)
    q = sentinel((T + 1, H, HD), BF16, device)
    cd = U8 if c["fp8"] else BF16
    kc, vc = sentinel((nblk, Hkv, 64, HD), cd, device), sentinel((nblk, Hkv, 64, HD), cd, device)
    kvs = (sentinel((nblk, Hkv, 64), F32, device), sentinel((nblk, Hkv, 64), F32, device)) if c["fp8"] else None
    dev = lambda t: None if t is None else t.to(device)
    fn(qkv, dev(c["pos"]), dev(c["tok_seq"]), dev(c["bt"]), dev(c["cos"] if cos is None else cos),
       dev(c["sin"] if sin is None else sin), q[:T], kc, vc, H, Hkv, kv_scales=kvs)
    o = dict(q=q.cpu(), kc=kc.cpu(), vc=vc.cpu())
    if kvs is not None:
        o.update(ks=kvs[0].cpu(), vs=kvs[1].cpu())
    return o


def rope_written(c):
    blk, off = slots(c["pos"], c["tok_seq"], c["bt"])
    m = torch.zeros(c["nblk"], c["Hkv"], 64, dtype=torch.bool)
    m[blk, :, off] = True
    return blk, off, m


def rope_check_untouched(c, o):
    """q_out past T, and every cache slot and scale outside the written set, keep the sentinel."""
    H, Hkv, T, nblk = c["H"], c["Hkv"], c["T"], c["nblk"]
    tag = f"rope {c['mode']} {(H, Hkv)} S={c['S']} decode={c['decode']}"
    _, _, m = rope_written(c)
    check_untouched(o["q"][T:], sentinel((1, H, HD), BF16), None, tag + " q_out guard row")
    if c["fp8"]:
        s8 = ref.kv8_logical(sentinel((nblk, Hkv, 64, HD), U8))
        check_untouched(ref.kv8_logical(o["kc"]), s8, m, tag + " K bytes")
        check_untouched(ref.kv8_logical(o["vc"]), s8, m, tag + " V bytes")
        check_untouched(o["ks"], sentinel((nblk, Hkv, 64), F32), m, tag + " K scales")
        check_untouched(o["vs"], sentinel((nblk, Hkv, 64), F32), m, tag + " V scales")
    else:
        check_untouched(o["kc"], sentinel((nblk, Hkv, 64, HD), BF16), m, tag + " K cache")
        check_untouched(o["vc"], sentinel((nblk, Hkv, 64, HD), BF16), m, tag + " V cache")


def rope_check_written(c, o, key="rope"):
    """q and the appended rows: bit-equal to the float64 result on the exact constructions, within the bounds on random
    data; V rows always bit-equal.  Returns the worst share of the RoPE bound (0 for the exact constructions)."""
    H, Hkv, T = c["H"], c["Hkv"], c["T"]
    tag = f"rope {c['mode']} {(H, Hkv)} S={c['S']} decode={c['decode']}"
    blk, off, _ = rope_written(c)
    rq, rk, v32 = c["rot"][:, :H], c["rot"][:, H:], c["x32"][:, H + Hkv:]
    ratio = 0.0
    if c["exact"]:
        check_exact(o["q"][:T], rq.float().to(BF16), tag + " q")
    else:
        ratio = within_bf16(o["q"][:T], rq, c["e_rot"][:, :H], key, tag + " q")
    if not c["fp8"]:
        if c["exact"]:
            check_exact(o["kc"][blk, :, off], rk.float().to(BF16), tag + " K rows")
        else:
            ratio = max(ratio, within_bf16(o["kc"][blk, :, off], rk, c["e_rot"][:, H:], key, tag + " K rows"))
        check_exact(o["vc"][blk, :, off], v32.to(BF16), tag + " V rows")
        return ratio
    k8, v8 = ref.kv8_logical(o["kc"])[blk, :, off], ref.kv8_logical(o["vc"])[blk, :, off]
    ksc, vsc = o["ks"][blk, :, off], o["vs"][blk, :, off]
    if c["exact"]:
        wk, wks = ref.quant_kv_rows(rk.float())
        check_exact(k8, wk, tag + " K bytes")
        check_exact(ksc, wks, tag + " K scales")
    else:
        check_fp8_rows(k8, ksc, rk, key + "/kv8", tag + " K rows")
    wv, wvs = ref.quant_kv_rows(v32)
    check_exact(v8, wv, tag + " V bytes")
    check_exact(vsc, wvs, tag + " V scales")
    return ratio


def rope_check(c, o, key="rope"):
    rope_check_untouched(c, o)
    return rope_check_written(c, o, key)


# ------------------------------------------------------------------------------------------------ prefill GEMM epilogue
GEMM_ROPE_CFGS = [-1, 0, 3, 5, 6, 7, 8, 11]  # the list of test_kernels_gpu.py::test_gemm_rope_epilogue


def gemm_rope_case(H=4, Hkv=2, T=65, K=64, seed=0):
    """Integer-valued x and w (the product is exact in f32 in any order) and the planted table: q and the appended rows
    are the float64 result.  Two packed sequences, the second starting mid-block, scattered block tables."""
    g = torch.Generator().manual_seed(seed + 5)
    N = (H + 2 * Hkv) * HD
    x = torch.randint(-2, 3, (T, K), generator=g).to(BF16)
    w = torch.randint(-1, 2, (N, K), generator=g).to(BF16)
    t0 = T // 3
    pos = torch.cat([torch.arange(t0), torch.arange(37, 37 + T - t0)]).to(I32)
    tok_seq = torch.cat([torch.zeros(t0), torch.ones(T - t0)]).to(I32)
    nblk = 8
    perm = (torch.randperm(nblk - 2, generator=g) + 1).tolist()  # block 0 and one more stay unnamed
    bt = torch.tensor([perm[:2] + [0], [nblk - 1, perm[2]] + [0]], dtype=I32)
    cos, sin = planted_tables(64 * bt.shape[1], seed)
    qkv = (x.double() @ w.double().t()).view(T, H + 2 * Hkv, HD)
    cs, sn = cos[pos.long()].double().unsqueeze(1), sin[pos.long()].double().unsqueeze(1)
    lo, hi = qkv[:, : H + Hkv, :64], qkv[:, : H + Hkv, 64:]
    rot = torch.cat([lo * cs - hi * sn, hi * cs + lo * sn], -1)
    return dict(H=H, Hkv=Hkv, T=T, K=K, x=x, w=w, pos=pos, tok_seq=tok_seq, bt=bt, nblk=nblk, cos=cos, sin=sin,
                want_q=rot[:, :H].float().to(BF16), want_k=rot[:, H:].float().to(BF16),
                want_v=qkv[:, H + Hkv:].float().to(BF16))


def gemm_rope_check(c, q, kc, vc, tag):
    H, Hkv, T, nblk = c["H"], c["Hkv"], c["T"], c["nblk"]
    blk, off = slots(c["pos"], c["tok_seq"], c["bt"])
    m = torch.zeros(nblk, Hkv, 64, dtype=torch.bool)
    m[blk, :, off] = True
    check_exact(q[:T], c["want_q"], tag + " q")
    check_exact(kc[blk, :, off], c["want_k"], tag + " K rows")
    check_exact(vc[blk, :, off], c["want_v"], tag + " V rows")
    check_untouched(q[T:], sentinel((1, H, HD), BF16), None, tag + " q_out guard row")
    check_untouched(kc, sentinel((nblk, Hkv, 64, HD), BF16), m, tag + " K cache")
    check_untouched(vc, sentinel((nblk, Hkv, 64, HD), BF16), m, tag + " V cache")


# ------------------------------------------------------------------------------------------------ SiLU
def silu_y(gate, up):
    g, u = gate.double(), up.double()
    y = g / (1 + torch.exp(-g)) * u
    return y, 2.0 ** -12 * y.abs() + 1e-30


def _gate_up(M, F, g, dtype):
    """gate (|gate| <= 20, +-100 planted) and up [M, F] in ``dtype``'s values, as f32."""
    gate = (torch.rand(M, F, generator=g) * 40 - 20).to(dtype).float()
    up = torch.randn(M, F, generator=g).to(dtype).float()
    gate.view(-1)[3], gate.view(-1)[-2] = 100.0, -100.0
    return gate, up


def interleave16(gate, up):
    """[M, F] x 2 -> [M, 2F]: column block 2j = gate columns 16j .. 16j + 15, block 2j + 1 = the up columns."""
    M, F = gate.shape
    return torch.stack([gate.view(M, F // 16, 16), up.view(M, F // 16, 16)], 2).reshape(M, 2 * F)


def silu_parts_check(fn, device, M, F, S, seed=0, key="silu_parts"):
    """fn = ops.silu_parts over S slabs [S, M, 2F] (a row-sliced view of a taller buffer)."""
    g = torch.Generator().manual_seed(seed + M * 7 + F + S)
    gate, up = _gate_up(M, F, g, F32)
    tall = torch.zeros(S, M + 1, 2 * F)
    tall[: S - 1, :M] = torch.randn(S - 1, M, 2 * F, generator=g)
    tall[S - 1, :M] = interleave16(gate, up) - (tall[: S - 1, :M].sum(0) if S > 1 else 0)
    y32 = slab_sum32(None, tall[:, :M])  # the kernel's own gate / up: the slabs from left to right
    y4 = y32.view(M, F // 16, 2, 16)
    y, e = silu_y(y4[:, :, 0].reshape(M, F), y4[:, :, 1].reshape(M, F))
    out = sentinel(M * F + 64, BF16, device)
    fn(tall.to(device)[:, :M], out[: M * F].view(M, F))
    check_untouched(out[M * F:], sentinel(64, BF16), None, f"silu_parts M={M} F={F} S={S} guard")
    return within_bf16(out[: M * F].view(M, F), y, e, key, f"M={M} F={F} S={S}")


def silu_mul_check(fn, device, n, seed=0, key="silu_mul"):
    """fn = ops.silu_mul over bf16 gate / up [n]."""
    g = torch.Generator().manual_seed(seed + n)
    gate, up = _gate_up(1, n, g, BF16)
    y, e = silu_y(gate, up)
    out = sentinel(n + 64, BF16, device)
    fn(gate.view(-1).to(BF16).to(device), up.view(-1).to(BF16).to(device), out[:n])
    check_untouched(out[n:], sentinel(64, BF16), None, f"silu_mul n={n} guard")
    return within_bf16(out[:n].view(1, n), y, e, key, f"n={n}")


def silu_bf16_check(fn, device, M, F, seed=0, key="silu_bf16"):
    """fn(y [M, 2F] bf16 interleaved, out): the prefill pass over the vendor GEMM's output."""
    g = torch.Generator().manual_seed(seed + M * 7 + F)
    gate, up = _gate_up(M, F, g, BF16)
    y, e = silu_y(gate, up)
    out = sentinel(M * F + 64, BF16, device)
    fn(interleave16(gate, up).to(BF16).to(device), out[: M * F].view(M, F))
    check_untouched(out[M * F:], sentinel(64, BF16), None, f"silu_bf16 M={M} F={F} guard")
    return within_bf16(out[: M * F].view(M, F), y, e, key, f"M={M} F={F}")


# ------------------------------------------------------------------------------------------------ suites
# One function per family: the GPU tests run them over the HIP kernels, scripts/resid_exact_margins.py runs the same
# ones once to record RATIOS.  Each returns its worst share of the bound.
@contextlib.contextmanager
def forced_xf_kernel():
    """rmsnorm_xf_kernel from 65 rows on (its production threshold is 512), restored afterwards."""
    ops.ext().rmsnorm_xf_tile_min(65)
    try:
        yield
    finally:
        ops.ext().rmsnorm_xf_tile_min(512)


def norm_suite(device, D, fn=None):
    """Every slab count 0 .. 9 (the switch's 0 / 1 / 2 / 3 / 4 / 6 / 8 and the runtime path) with 1 .. 5 rows."""
    fn = fn or ops.add_rmsnorm
    worst = 0.0
    for nparts in range(10):
        c = norm_case(D, nparts, 1 + nparts % 5)
        worst = max(worst, norm_check(c, norm_run(fn, c, device)))
    return worst


def norm_forms_suite(device, form, fn=None):
    fn = fn or ops.add_rmsnorm
    worst = 0.0
    for D in NORM_D:
        for nparts in (0, 3, 5):
            if norm_form_ok(form, D):
                c = norm_case(D, nparts, 5, form)
                worst = max(worst, norm_check(c, norm_run(fn, c, device)))
    return worst


def norm_spike_suite(device, fn=None):
    fn = fn or ops.add_rmsnorm
    worst = 0.0
    for nparts in (0, 2):
        c = norm_case(8192, nparts, 16, spikes=True)
        worst = max(worst, norm_check(c, norm_run(fn, c, device), "add_rmsnorm/spike"))
    return worst


def norm_xf_suite(device, rows, fn=None):
    fn = fn or ops.add_rmsnorm
    return max(norm_xf_check(fn, norm_xf_case(rows, D), device) for D in (32, 160, 4096))


def res_suite(device, D, fn=None):
    """Slab counts 0 .. 9 x rows 1 / 5 / 33, row-major and (D % 32 == 0) fragment-major; the Q24 sums repeat bitwise."""
    fn = fn or ops.res_add_ss
    worst = 0.0
    for nparts in range(10):
        for rows in RES_ROWS:
            c = res_case(D, nparts, rows)
            for xf in ([False, True] if D % 32 == 0 else [False]):
                o = res_run(fn, c, device, xf)
                worst = max(worst, res_check(c, o))
                again = res_run(fn, c, device, xf)
                check_exact(again["ss"], o["ss"], f"res_add_ss D={D} nparts={nparts} rows={rows} repeat")
    return worst


def rope_suite(device, HH, mode, fn=None):
    fn = fn or ops.rope_append
    worst = 0.0
    for S in ROPE_SLABS:
        for decode in (False, True):
            c = rope_case(*HH, S, decode, mode)
            worst = max(worst, rope_check(c, rope_run(fn, c, device)))
    return worst


def gemm_rope_run(c, device, cfg):
    H, Hkv, T, nblk = c["H"], c["Hkv"], c["T"], c["nblk"]
    pw = ops.PackedWeight.from_dense(c["w"].to(device))
    ws, tk, ncu = ops._sk_workspace(device)
    q = sentinel((T + 1, H, HD), BF16, device)
    kc, vc = sentinel((nblk, Hkv, 64, HD), BF16, device), sentinel((nblk, Hkv, 64, HD), BF16, device)
    ops.ext().gemm_sk_rope(c["x"].to(device), pw.data, ws, tk, ncu, 4, cfg, c["pos"].to(device), c["tok_seq"].to(device),
                           c["bt"].to(device), c["cos"].to(device), c["sin"].to(device), q, kc, vc, H, Hkv)
    assert int(tk.abs().sum()) == 0
    gemm_rope_check(c, q.cpu(), kc.cpu(), vc.cpu(), f"gemm_sk_rope cfg {cfg}")


SILU_PARTS_CAP = 4096 * 256 * 4  # elements one pass of each kernel's capped grid covers
SILU_MUL_CAP = 2048 * 256 * 8
SILU_BF16_CAP = 8192 * 256 * 8


def silu_bf16_fn(y, out):
    ops.ext().silu_bf16(y, out)


def silu_small_suite(device, parts_fn=None, mul_fn=None, bf16_fn=None):
    worst = 0.0
    for M in (1, 3):
        for F in (16, 48, 512):
            for S in (1, 2, 3):
                worst = max(worst, silu_parts_check(parts_fn or ops.silu_parts, device, M, F, S))
        for F in (16, 48):
            if bf16_fn is not None:
                worst = max(worst, silu_bf16_check(bf16_fn, device, M, F))
    for n in (8, 2056):
        worst = max(worst, silu_mul_check(mul_fn or ops.silu_mul, device, n))
    return worst
