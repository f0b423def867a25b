"""Case builders and checkers of the context-shift tests (test_context_shift_cpu.py runs them over ``ops.reference``,
test_context_shift_gpu.py over the HIP kernel and the captured graphs).  Everything is built on the host from seeds
and moved to ``device``; the float64 transcription below is the oracle of both."""
import math

import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.models.spec import get_spec
from llm_based_apache_spark_optimization_amd.ops import reference as ref

U = 2.0 ** -8  # bf16 round-to-nearest bound
TABLE_ROWS = 8192

# theta 1e4, 5e5 with llama3 scaling (the two tiny specs' settings) and 1e6
ROPE = {"nsql": (get_spec("tiny-nsql").rope_theta, get_spec("tiny-nsql").rope_scaling),
        "llama3": (get_spec("tiny-llama3").rope_theta, get_spec("tiny-llama3").rope_scaling),
        "mistral": (1.0e6, None)}
assert ROPE["nsql"] == (1.0e4, None) and ROPE["llama3"][0] == 5.0e5 and ROPE["llama3"][1]["rope_type"] == "llama3"


def tables(kind: str, rows: int = TABLE_ROWS):
    theta, scaling = ROPE[kind]
    return ref.rope_tables(128, rows, theta, scaling)


def inv_freq64(kind: str) -> torch.Tensor:
    """float64 inverse frequencies [64] of a RoPE setting, transcribed from the published llama3 rule."""
    theta, sc = ROPE[kind]
    inv = [1.0 / theta ** (2 * i / 128) for i in range(64)]
    if sc:
        f, lo, hi, old = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"], \
            sc["original_max_position_embeddings"]
        for i, v in enumerate(inv):
            wl = 2 * math.pi / v
            if wl > old / lo:
                inv[i] = v / f
            elif wl >= old / hi:
                smooth = (old / wl - lo) / (hi - lo)
                inv[i] = (1 - smooth) * v / f + smooth * v
    return torch.tensor(inv, dtype=torch.float64)


def arena(Hkv: int, seed: int, NB: int = 12, L: int = 2, wide: bool = False) -> torch.Tensor:
    """A whole arena [L, 2, NB, Hkv, 64, 128] of random bf16, block 0 included; ``wide``: magnitudes 1e-3 .. 1e2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, 2, NB, Hkv, 64, 128, generator=g)
    if wide:
        x = x * 10.0 ** (torch.rand(L, 2, NB, Hkv, 64, 1, generator=g) * 5.0 - 3.0)
    return x.to(torch.bfloat16)


def moves_for(rows: int = TABLE_ROWS) -> list:
    """Three sequences' moves of one launch over blocks 1 .. 11 of a 12-block arena: an in-place whole block, a fork to
    a fresh block, rows [5, 64) next to rows [0, 5) with delta 0 (a kept head that ends inside a block), an empty
    range, and deltas 64, 128 and rows - 64.  Blocks 0, 1 and 2 are nobody's."""
    return [(3, 3, 0, 64, 64), (4, 5, 0, 64, 64),                              # sequence A: in place; fork
            (6, 7, 0, 5, 0), (8, 7, 5, 64, 128),                               # sequence B: keep = 5, its tail forked
            (9, 9, 7, 7, 64), (10, 10, 0, 64, rows - 64), (11, 11, 0, 64, 128)]  # sequence C: empty; far; in place


def expected64(kv0: torch.Tensor, moves, cos: torch.Tensor, sin: torch.Tensor):
    """float64 transcription of the rule over the stored cache ``kv0`` and the f32 tables: (exact, tol, written).
    exact = what every element must be; tol = u |exact| + 2^-20 (|a| + |b|) on rotated K elements (a, b the stored
    pair) and 0 everywhere else (copies and untouched elements are exact); written = the destination elements."""
    kv0 = kv0.cpu()
    exact = kv0.double().clone()
    tol = torch.zeros_like(exact)
    written = torch.zeros(kv0.shape, dtype=torch.bool)
    c64, s64 = cos.cpu().double(), sin.cpu().double()
    for src, dst, lo, hi, delta in moves:
        if hi <= lo:
            continue
        k = kv0[:, 0, src, :, lo:hi].double()
        a, b = k[..., :64], k[..., 64:]
        if delta:
            c, s = c64[delta], s64[delta]
            out = torch.cat([a * c + b * s, b * c - a * s], dim=-1)
            mag = (a.abs() + b.abs()).repeat(1, 1, 1, 2)
            tol[:, 0, dst, :, lo:hi] = U * out.abs() + 2.0 ** -20 * mag
        else:
            out = k
        if delta or src != dst:
            exact[:, 0, dst, :, lo:hi] = out
            written[:, 0, dst, :, lo:hi] = True
        if src != dst:
            exact[:, 1, dst, :, lo:hi] = kv0[:, 1, src, :, lo:hi].double()
            written[:, 1, dst, :, lo:hi] = True
    return exact, tol, written


def check_against(kv0: torch.Tensor, kv1: torch.Tensor, moves, cos, sin) -> float:
    """Every element of the result ``kv1`` within its bound of the float64 rule; every byte outside the destination
    rows bit-unchanged.  Returns the worst error / bound ratio over the rotated elements."""
    exact, tol, written = expected64(kv0, moves, cos, sin)
    got = kv1.cpu()
    err = (got.double() - exact).abs()
    bad = err > tol
    assert not bad.any(), f"{int(bad.sum())} elements past their bound, first at {bad.nonzero()[0].tolist()}"
    same = got.view(torch.int16) == kv0.cpu().view(torch.int16)
    assert bool(same[~written].all()), "a byte outside the destination rows changed"
    rot = tol > 0
    return float((err[rot] / tol[rot]).max()) if rot.any() else 0.0


def planted(rows: int, d: int, dev="cpu"):
    """Tables for which the result is exact.  Row d: even pairs (cos 0, sin 1) -- lo' = hi, hi' = -lo -- and odd pairs
    (1, 0), the identity; rows d - 64 and d + 64: (cos -1, sin 0) and (cos 0, sin -1); every other row garbage.  A wrong
    table row, a wrong pair mapping, a wrong column or a wrong sign gives different bits."""
    g = torch.Generator().manual_seed(rows + d)
    cos, sin = torch.randn(rows, 64, generator=g), torch.randn(rows, 64, generator=g)
    even = (torch.arange(64) % 2 == 0)
    cos[d], sin[d] = (~even).float(), even.float()
    for r, (c, s) in ((d - 64, (-1.0, 0.0)), (d + 64, (0.0, -1.0))):
        if 0 <= r < rows:
            cos[r], sin[r] = torch.full((64,), c), torch.full((64,), s)
    return cos.to(dev), sin.to(dev)


def planted_expect(k: torch.Tensor) -> torch.Tensor:
    """Rows k [..., 128] rotated with row d of ``planted``."""
    lo, hi = k[..., :64], k[..., 64:]
    even = (torch.arange(64, device=k.device) % 2 == 0)
    return torch.cat([torch.where(even, hi, lo), torch.where(even, -lo, hi)], dim=-1)


# move lists the op refuses before anything is uploaded or launched: (name, moves)
def refusals(NB: int, rows: int) -> list:
    ok = (3, 4, 0, 64, 64)
    return [("src 0", [(0, 4, 0, 64, 64)]), ("dst 0", [(3, 0, 0, 64, 64)]), ("src NB", [(NB, 4, 0, 64, 64)]),
            ("dst NB", [(3, NB, 0, 64, 64)]), ("negative id", [(-1, 4, 0, 64, 64)]),
            ("lo < 0", [(3, 4, -1, 64, 64)]), ("hi > 64", [(3, 4, 0, 65, 64)]), ("lo > hi", [(3, 4, 9, 8, 64)]),
            ("delta < 0", [(3, 4, 0, 64, -64)]), ("delta = rows", [(3, 4, 0, 64, rows)]),
            ("two moves, one destination", [ok, (5, 4, 63, 64, 64)]),
            ("destination read by another move", [ok, (4, 6, 0, 64, 64)]),
            ("in-place destination read by another move", [(4, 4, 0, 10, 64), (4, 6, 9, 20, 64)])]


def rows_of(plane: torch.Tensor, blocks: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Rows (blocks[i], rows[i]) of one K or V plane [L, NB, Hkv, 64, 128] -> [n, L, Hkv, 128]."""
    return plane.permute(1, 3, 0, 2, 4)[blocks, rows].contiguous()


class ShiftSpy:
    """Wraps ``runner.shift_slots`` of an engine: before each call it snapshots the arena and the slot state, after it
    checks the shifted cache, table, position and penalty ring of every entry against the rule, reading the rows
    through the block tables (not through the planned moves).  ``checked`` counts the shifts seen."""

    def __init__(self, eng):
        self.eng, self.checked, self.keeps = eng, 0, []
        self._orig = eng.runner.shift_slots
        eng.runner.shift_slots = self

    def restore(self):
        """Take the spy out again by deleting the instance attribute: assigning the bound method back would leave
        the runner in a reference cycle (runner -> its __dict__ -> bound method -> runner), and an engine whose
        captured graphs wait for the cyclic collector can be destroyed in the middle of a later graph capture."""
        del self.eng.runner.shift_slots

    def __call__(self, entries):
        r = self.eng.runner
        kv0 = r.kv.clone()
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
        for slot, moves, table, d in entries:
            q = self.eng._reqs[self.eng._slot_owner[slot]]
            keep, d2 = q.drops[-1]
            n = int(pos0[slot])  # cache rows before: positions 0 .. c - 2
            assert d2 == d and n + 1 == q.shift_w and d == 64 * ((n + 1 - keep) // 128) and d >= 64
            assert keep == max(0, min(q.params.num_keep, len(q.prompt_ids), q.shift_w - 128))
            assert int(pos1[slot]) == n - d
            assert bt1[slot].tolist() == list(table) + [0] * (bt1.shape[1] - len(table))
            # the rule on a twin arena: every old block of the slot rotated in place by d (K only)
            old = [b for b in bt0[slot].tolist() if b]
            twin = kv0.cpu().clone()
            ref.kv_shift(twin, None, [(b, b, 0, 64, d) for b in old], r.cos.cpu(), r.sin.cpu())
            snap, now = kv0.cpu(), r.kv.cpu()
            newp = torch.arange(n - d)
            oldp = torch.where(newp < keep, newp, newp + d)
            nb = bt1[slot][newp // 64].long()
            ob = bt0[slot][oldp // 64].long()
            got_k, got_v = rows_of(now[:, 0], nb, newp % 64), rows_of(now[:, 1], nb, newp % 64)
            want_k = torch.where((newp < keep)[:, None, None, None], rows_of(snap[:, 0], ob, oldp % 64),
                                 rows_of(twin[:, 0], ob, oldp % 64))
            assert torch.equal(got_k.view(torch.int16), want_k.view(torch.int16)), "kept K rows differ from the twin"
            assert torch.equal(got_v.view(torch.int16), rows_of(snap[:, 1], ob, oldp % 64).view(torch.int16)), \
                "V rows differ"
            self.checked += 1
            self.keeps.append(keep)


def run_op(kv: torch.Tensor, moves, cos, sin) -> torch.Tensor:
    out = kv.clone()
    ops.kv_shift(out, None, moves, cos, sin)
    return out
