"""Case builders and checkers of the fp8 context-shift tests (test_context_shift_fp8_cpu.py runs them over
``ops.reference.kv_shift8``, test_context_shift_fp8_gpu.py over kv_shift8_kernel and the captured graphs).  The tables,
move lists and refusals are those of kv_shift_cases.py; the float64 transcription below is the oracle of both files.

The bounds on a rotated K row.  ``exact`` = the float64 rotation of the dequantised source row, ``amax`` = its max
|exact|.  The row is stored again as e4m3(x' * 448 / amax') with scale amax' / 448, so
  * the new scale is amax / 448 up to the f32 arithmetic of the dequantisation, the rotation and the two scale
    products: within 2^-18 relative;
  * an element is off by at most e4m3's normal half-ulp, 2^-4 |exact|, or -- below the smallest normal code -- by its
    subnormal half-step, 2^-10 in code units, that is 2^-10 * (new scale); 2^-16 * amax covers the f32 arithmetic.
A row with amax 0 must come back as zeros with scale 0."""
import torch

import kv_shift_cases as ks
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

ZERO_ROW, ONE_ROW = 9, 10  # planted in the K plane of every block: an all-zero row, a row with one non-zero element


def arena8(Hkv: int, seed: int, NB: int = 12, L: int = 2, wide: bool = False):
    """A whole fp8 arena: (kv uint8 [L, 2, NB, Hkv, 64, 128] in token-pair order, kv_scale f32 [L, 2, NB, Hkv, 64]),
    random f32 rows through ``quant_kv_rows`` / ``kv8_physical``; ``wide``: magnitudes 1e-3 .. 1e2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, 2, NB, Hkv, 64, 128, generator=g)
    if wide:
        x = x * 10.0 ** (torch.rand(L, 2, NB, Hkv, 64, 1, generator=g) * 5.0 - 3.0)
    x[:, 0, :, :, ZERO_ROW] = 0.0
    x[:, 0, :, :, ONE_ROW] = 0.0
    for b in range(NB):
        x[:, 0, b, :, ONE_ROW, (7 * b + 5) % 128] = 1.7 * (b + 1)
    q, sc = ref.quant_kv_rows(x)
    return ref.kv8_physical(q).contiguous(), sc.contiguous()


def dequant(kv: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    """The arena's values in token order, f32."""
    return ref.dequant_kv_rows(ref.kv8_logical(kv.cpu()), sc.cpu())


def codes(kv: torch.Tensor) -> torch.Tensor:
    """The arena's e4m3 codes as f32 values, in token order."""
    return ref.kv8_logical(kv.cpu()).view(torch.float8_e4m3fn).float()


def expected64(kv0, sc0, moves, cos, sin):
    """float64 transcription of the rule over the stored cache: (exact, amax, rot, want_q, want_sc).  On the rotated
    K rows (``rot`` [L, 2, NB, Hkv, 64]) ``exact`` is the float64 rotation of the dequantised source and ``amax`` its
    row maximum; everywhere else the result must be the bytes ``want_q`` (token order) and scales ``want_sc``: the
    source's on copied rows, the arena's own on every row that is no destination."""
    kv0, sc0 = kv0.cpu(), sc0.cpu()
    x0 = dequant(kv0, sc0).double()
    exact = x0.clone()
    want_q, want_sc = ref.kv8_logical(kv0).clone(), sc0.clone()
    q0, s0 = want_q.clone(), sc0.clone()
    rot = torch.zeros(sc0.shape, dtype=torch.bool)
    amax = torch.zeros(sc0.shape, dtype=torch.float64)
    c64, s64 = cos.cpu().double(), sin.cpu().double()
    for src, dst, lo, hi, delta in moves:
        if hi <= lo:
            continue
        if delta:
            k = x0[:, 0, src, :, lo:hi]
            a, b = k[..., :64], k[..., 64:]
            c, s = c64[delta], s64[delta]
            out = torch.cat([a * c + b * s, b * c - a * s], dim=-1)
            exact[:, 0, dst, :, lo:hi] = out
            amax[:, 0, dst, :, lo:hi] = out.abs().amax(-1)
            rot[:, 0, dst, :, lo:hi] = True
        if src != dst:
            for pl in ([1] if delta else [0, 1]):
                want_q[:, pl, dst, :, lo:hi] = q0[:, pl, src, :, lo:hi]
                want_sc[:, pl, dst, :, lo:hi] = s0[:, pl, src, :, lo:hi]
                exact[:, pl, dst, :, lo:hi] = x0[:, pl, src, :, lo:hi]
    return exact, amax, rot, want_q, want_sc


def check_rows(got: torch.Tensor, got_sc: torch.Tensor, exact: torch.Tensor, amax: torch.Tensor):
    """Rotated rows: dequantised result ``got`` [..., 128] with its new scales ``got_sc`` [...] against ``exact`` and
    ``amax`` (same shapes, float64).  Returns (worst element error / bound, worst relative scale error)."""
    scale = amax / 448.0
    serr = (got_sc.double() - scale).abs()
    assert bool((serr <= 2.0 ** -18 * scale).all()), f"scale off by {float((serr / scale.clamp_min(1e-300)).max()):.3g}"
    bound = 2.0 ** -4 * exact.abs() + (2.0 ** -10 * scale + 2.0 ** -16 * amax).unsqueeze(-1)
    err = (got.double() - exact).abs()
    bad = err > bound
    assert not bad.any(), f"{int(bad.sum())} elements past their bound, first at {bad.nonzero()[0].tolist()}"
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    nz = scale > 0
    return ratio, (float((serr[nz] / scale[nz]).max()) if nz.any() else 0.0)


def check_against(kv0, sc0, kv1, sc1, moves, cos, sin):
    """The whole result against the rule: rotated K rows within their bounds, every other destination byte and scale
    bit-equal to its source, every byte and scale outside the destination rows unchanged.  Returns (worst element
    error / bound, worst relative scale error) over the rotated rows."""
    exact, amax, rot, want_q, want_sc = expected64(kv0, sc0, moves, cos, sin)
    got_q, got_sc = ref.kv8_logical(kv1.cpu()), sc1.cpu()
    assert torch.equal(got_q[~rot], want_q[~rot]), "a copied or untouched byte differs"
    assert torch.equal(got_sc[~rot].view(torch.int32), want_sc[~rot].view(torch.int32)), \
        "a copied or untouched scale differs"
    if not rot.any():
        return 0.0, 0.0
    return check_rows(dequant(kv1, sc1)[rot], got_sc[rot], exact[rot], amax[rot])


def run_op(kv, sc, moves, cos, sin):
    kv, sc = kv.clone(), sc.clone()
    ops.kv_shift8(kv, sc, moves, cos, sin)
    return kv, sc


def same(a, b) -> bool:
    """Two (kv, kv_scale) pairs, bit for bit."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def scales_of(plane: torch.Tensor, blocks: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Scales (blocks[i], rows[i]) of one K or V plane [L, NB, Hkv, 64] -> [n, L, Hkv]."""
    return plane.permute(1, 3, 0, 2)[blocks, rows].contiguous()


class ShiftSpy8(ks.ShiftSpy):
    """``ShiftSpy`` on the fp8 cache.  Through the block tables, after every shift: the kept head's K rows and every V
    row carry the snapshot's bytes and scales; the shifted K rows are, with ``twin``, bit-equal (bytes and scales) to
    ``ops.reference.kv_shift8`` applied to the snapshot, and otherwise within the bounds of ``expected64`` on the
    snapshot (``worst`` keeps the worst ratios seen).  Table, position and penalty ring as in the bf16 spy."""

    def __init__(self, eng, twin: bool):
        super().__init__(eng)
        self.twin, self.worst = twin, (0.0, 0.0)

    def __call__(self, entries):
        r = self.eng.runner
        kv0, sc0 = r.kv.clone().cpu(), r.kv_scale.clone().cpu()
        bt0, pos0 = r.block_tables.clone().cpu(), r.positions.clone().cpu()
        hist0 = r.hist.clone() if getattr(r, "hist", None) is not None else None
        self._orig(entries)
        if hist0 is not None:
            assert torch.equal(r.hist, hist0), "the penalty ring changed"
        bt1, pos1 = r.block_tables.cpu(), r.positions.cpu()
        touched = {int(e[0]) for e in entries}
        for s in range(bt0.shape[0]):
            if s not in touched:
                assert torch.equal(bt1[s], bt0[s]) and int(pos1[s]) == int(pos0[s])
        cos, sin = r.cos.cpu(), r.sin.cpu()
        snap_q, now_q, now_s = ref.kv8_logical(kv0), ref.kv8_logical(r.kv.cpu()), r.kv_scale.cpu()
        now_x = ref.dequant_kv_rows(now_q, now_s)
        for slot, moves, table, d in entries:
            q = self.eng._reqs[self.eng._slot_owner[slot]]
            keep, d2 = q.drops[-1]
            n = int(pos0[slot])  # cache rows before: positions 0 .. c - 2
            assert d2 == d and n + 1 == q.shift_w and d == 64 * ((n + 1 - keep) // 128) and d >= 64
            assert keep == max(0, min(q.params.num_keep, len(q.prompt_ids), q.shift_w - 128))
            assert int(pos1[slot]) == n - d
            assert bt1[slot].tolist() == list(table) + [0] * (bt1.shape[1] - len(table))
            rule = [(b, b, 0, 64, d) for b in bt0[slot].tolist() if b]  # every old block rotated in place (K only)
            newp = torch.arange(n - d)
            oldp = torch.where(newp < keep, newp, newp + d)
            nb, ob = bt1[slot][newp // 64].long(), bt0[slot][oldp // 64].long()
            nr, orow, head = newp % 64, oldp % 64, newp < keep
            assert torch.equal(ks.rows_of(now_q[:, 1], nb, nr), ks.rows_of(snap_q[:, 1], ob, orow)), "V rows differ"
            assert torch.equal(scales_of(now_s[:, 1], nb, nr).view(torch.int32),
                               scales_of(sc0[:, 1], ob, orow).view(torch.int32)), "V scales differ"
            got_k, got_ks = ks.rows_of(now_q[:, 0], nb, nr), scales_of(now_s[:, 0], nb, nr)
            assert torch.equal(got_k[head], ks.rows_of(snap_q[:, 0], ob, orow)[head]), "kept K rows changed"
            assert torch.equal(got_ks[head].view(torch.int32), scales_of(sc0[:, 0], ob, orow)[head].view(torch.int32))
            if self.twin:
                tq, ts = kv0.clone(), sc0.clone()
                ref.kv_shift8(tq, ts, rule, cos, sin)
                assert torch.equal(got_k[~head], ks.rows_of(ref.kv8_logical(tq)[:, 0], ob, orow)[~head]), \
                    "shifted K rows differ from the twin"
                assert torch.equal(got_ks[~head].view(torch.int32),
                                   scales_of(ts[:, 0], ob, orow)[~head].view(torch.int32)), "K scales differ"
            else:
                exact, amax, _, _, _ = expected64(kv0, sc0, rule, cos, sin)
                w = check_rows(ks.rows_of(now_x[:, 0], nb, nr)[~head], got_ks[~head],
                               ks.rows_of(exact[:, 0], ob, orow)[~head], scales_of(amax[:, 0], ob, orow)[~head])
                self.worst = (max(self.worst[0], w[0]), max(self.worst[1], w[1]))
            self.checked += 1
            self.keeps.append(keep)
