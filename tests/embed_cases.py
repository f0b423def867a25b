"""Case builders and checkers of the embedding tests (test_embed_cpu.py runs them over the host twins of
``ops.reference``, test_embed_gpu.py over the kernels of csrc/kernels/embed.hip and the captured engine).

One pack of sequences, lengths 1, 2, 63, 64, 65 and 130 with the modes mean / last / none mixed, at D = 64, 384 (no
multiple of 256) and 4096 with 0, 1 and 3 split-K slabs; ``acc``, ``out`` and ``rs`` start from a sentinel so that every
word a launch must not write can be compared bit for bit."""
import math

import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

LENS = [1, 2, 63, 64, 65, 130]
MODES = [1, 2, 0, 1, 2, 1]        # mean, last, none, mean, last, mean (the 130-row sequence pools its mean)
SLOTS = [5, 2, 7, 0, 3, 6]        # of NSLOTS; slots 1, 4 and 8 belong to no sequence of the call
NSLOTS = 9
DS = (64, 384, 4096)
SLABS = (0, 1, 3)
EPS = 1e-5
SENTINEL = -1234.5
U = 2.0 ** -24
RATIOS: dict = {}  # worst measured error / bound per check, for profiles/embed/embed_exact_mi355x.json


def note(key: str, ratio: float) -> None:
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def meta_of(lens, modes, slots, starts=None, finals=None, counts=None):
    n = len(lens)
    return [list(modes), list(starts or [0] * n), list(slots), list(finals or [1] * n), list(counts or lens)]


def cu_of(lens):
    cu = [0]
    for x in lens:
        cu.append(cu[-1] + x)
    return cu


class Pack:
    """Operands of one call on ``device`` plus their host copies."""

    def __init__(self, D, nslab, device, lens=LENS, modes=MODES, slots=SLOTS, seed=0, **meta_kw):
        g = torch.Generator().manual_seed(1000 * D + 10 * nslab + seed)
        self.D, self.device, self.lens = D, torch.device(device), list(lens)
        self.cu = cu_of(lens)
        T = self.T = self.cu[-1]
        h = torch.randn(T, D, generator=g)
        parts = torch.randn(nslab, T, D, generator=g) * 0.25 if nslab else None
        if T > 70:  # rows of magnitude 1e4 and 1e-3 and an all-zero row, inside the mean sequences
            h[67] *= 1e4
            h[70] *= 1e-3
            h[200 if T > 200 else T - 1] = 0.0
            if parts is not None:
                parts[:, 67] *= 1e4
                parts[:, 70] *= 1e-3
                parts[:, 200 if T > 200 else T - 1] = 0.0
        self.zero_row = (200 if T > 200 else T - 1) if T > 70 else None
        self.h, self.parts = h, parts
        self.gamma = (1.0 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16)
        self.meta = meta_of(lens, modes, slots, **meta_kw)
        self.tseq = [i for i, x in enumerate(lens) for _ in range(x)]
        dev = self.device
        self.d = dict(h=h.to(dev), parts=parts.to(dev) if parts is not None else None, gamma=self.gamma.to(dev),
                      cu=torch.tensor(self.cu, dtype=torch.int32, device=dev),
                      tseq=torch.tensor(self.tseq, dtype=torch.int32, device=dev),
                      meta=torch.tensor(self.meta, dtype=torch.int32, device=dev))

    @property
    def host(self):
        return (self.cu, self.meta)

    def fresh(self, nslots=NSLOTS):
        """(acc, out, rs) on the device, all sentinel."""
        f = dict(dtype=torch.float32, device=self.device)
        return (torch.full((nslots, self.D), SENTINEL, **f), torch.full((nslots, self.D), SENTINEL, **f),
                torch.full((self.T + 3,), SENTINEL, **f))

    def rowscale(self, rs):
        d = self.d
        ops.embed_rowscale(d["h"], d["parts"], d["tseq"], d["cu"], d["meta"], EPS, rs, host=self.host)

    def pool(self, rs, acc):
        d = self.d
        ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"], rs, d["gamma"], acc, host=self.host)

    def finish(self, acc, out):
        ops.embed_finish(self.d["meta"], acc, out, host=self.host)

    def v(self):
        """The f32 rows the kernels form: h + slab 0 + slab 1 + ... left to right (adds only: the same bits anywhere)."""
        return ref.slab_sum(self.h.clone(), self.parts) if self.parts is not None else self.h.clone()

    def pooled_rows(self):
        """Row indices that get a row scale."""
        rows = []
        for i in range(len(self.lens)):
            *_, r0, r1 = ref._embed_rows(self.cu, self.meta, i)
            rows.extend(range(r0, r1))
        return rows


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def rowscale_chain(D: int, device) -> int:
    """The longest chain of f32 additions one sum of squares passes through.  embed_rowscale_kernel, grid (T) of 256
    threads: a thread takes the float4 groups tid, tid + 256, ... of the row, 4 * ceil(D / 1024) sequential adds; then
    the wave's DPP tree (6 levels over 64 lanes) and the sequential sum over the block's 4 waves: 4 * ceil(D / 1024) +
    6 + 4, 26 at D = 4096.  The host twin sums with torch.sum, whose order is not promised: D, the longest any has."""
    if torch.device(device).type == "cuda":
        return 4 * math.ceil(D / 1024) + 6 + 4
    return D


def finish_chain(D: int) -> int:
    """embed_finish_kernel (and its twin, which follows the same order): thread i of 256 sums columns i, i + 256, ...
    in order, ceil(D / 256) adds, then the halving tree over the 256 partial sums, 8 levels."""
    return math.ceil(D / 256) + 8


# ------------------------------------------------------------------------------------------------ checks
def check_rowscale(D, nslab, device):
    """|rs - exact| <= (c + 6) 2^-24 exact for every pooled row, exact from the f32 rows v in float64; an all-zero row
    gives rsqrt(eps); every entry of rs that no pooled row owns keeps its sentinel bits."""
    p = Pack(D, nslab, device)
    _, _, rs = p.fresh()
    p.rowscale(rs)
    sync(device)
    got = rs.cpu().double()
    v = p.v().double()
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    exact = 1.0 / torch.sqrt((v * v).sum(1) / D + eps32)
    rows = p.pooled_rows()
    assert 67 in rows and 70 in rows and p.zero_row in rows
    c = rowscale_chain(D, device)
    bound = (c + 6) * U * exact
    err = (got[: p.T] - exact).abs()
    idx = torch.tensor(rows)
    ratio = float((err[idx] / bound[idx]).max())
    print(f"rowscale D={D} slabs={nslab}: worst |rs - exact| / bound = {ratio:.4f} (c = {c})")
    note(f"rowscale_D{D}_slabs{nslab}", ratio)
    assert ratio <= 1.0
    assert abs(float(got[p.zero_row]) - eps32 ** -0.5) <= (c + 6) * U * eps32 ** -0.5
    others = torch.ones(rs.numel(), dtype=torch.bool)
    others[idx] = False
    assert bool((bits(rs)[others] == bits(torch.tensor([SENTINEL]))[0]).all()), "a row that is not pooled was written"
    return ratio


def check_pool(D, nslab, device):
    """acc bit-equal to the twin's for the same rs; rows of slots outside the call and of the mode-0 sequence keep the
    sentinel; a last-mode row is exactly that sequence's last y; two runs give the same bits."""
    p = Pack(D, nslab, device)
    acc, out, rs = p.fresh()
    p.rowscale(rs)
    p.pool(rs, acc)
    p.finish(acc, out)
    sync(device)
    rs_h = rs.cpu()
    acc_t = torch.full((NSLOTS, D), SENTINEL)
    out_t = torch.full((NSLOTS, D), SENTINEL)
    ref.embed_pool(p.h, p.parts, p.cu, p.meta, rs_h, p.gamma, acc_t)
    ref.embed_finish(p.meta, acc_t, out_t)
    assert same_bits(acc, acc_t), "pool differs from its twin"
    assert same_bits(out, out_t), "finish differs from its twin"
    sent = bits(torch.full((D,), SENTINEL))
    for slot in (1, 4, 8, SLOTS[2]):  # no sequence, or the mode-0 sequence
        assert torch.equal(bits(acc[slot]), sent) and torch.equal(bits(out[slot]), sent), slot
    v, g = p.v(), p.gamma.float()
    for i, mode in enumerate(MODES):
        if mode == 2:
            t = p.cu[i + 1] - 1
            assert same_bits(acc[SLOTS[i]], (v[t] * rs_h[t]) * g)
    acc2, out2, rs2 = p.fresh()
    p.rowscale(rs2)
    p.pool(rs2, acc2)
    p.finish(acc2, out2)
    sync(device)
    assert same_bits(rs2, rs) and same_bits(acc2, acc) and same_bits(out2, out), "not repeatable"
    nrm = out.cpu().double()[[s for s, m in zip(SLOTS, MODES) if m]].norm(dim=1)
    assert bool(((nrm - 1.0).abs() < 2.0 ** -20).all())


def check_chunk_invariance(D, nslab, device):
    """The 130-row sequence pooled whole, and as segments of 1, 63 and 66 rows in three launches (estart 0 / 1 / 64,
    efinal on the last only): acc and out bit-equal.  A continuation adds onto a planted acc; estart == 0 ignores a
    poisoned one.  A neighbour sequence rides in every launch."""
    whole = Pack(D, nslab, device, lens=[7, 130], modes=[2, 1], slots=[4, 1], seed=5)
    acc_w, out_w, rs_w = whole.fresh()
    acc_w[1] = float("nan")  # poisoned: estart == 0 must not read it
    whole.rowscale(rs_w)
    whole.pool(rs_w, acc_w)
    whole.finish(acc_w, out_w)
    sync(device)
    assert not bool(torch.isnan(acc_w[1]).any())
    acc_c, out_c, _ = whole.fresh()
    acc_c[1] = float("nan")
    a = 7
    for lo, hi in ((0, 1), (1, 64), (64, 130)):
        seg = Pack(D, nslab, device, lens=[7, hi - lo], modes=[2, 1], slots=[4, 1], seed=5, starts=[0, lo],
                   finals=[1, int(hi == 130)], counts=[7, 130])
        rows = list(range(7)) + list(range(a + lo, a + hi))
        seg.h = whole.h[rows].clone()
        seg.parts = whole.parts[:, rows].clone() if whole.parts is not None else None
        seg.d["h"] = seg.h.to(seg.device)
        seg.d["parts"] = seg.parts.to(seg.device) if seg.parts is not None else None
        seg.d["gamma"], seg.gamma = whole.d["gamma"], whole.gamma
        _, _, rs = seg.fresh()
        seg.rowscale(rs)
        if hi < 130:
            before = out_c.clone()
        seg.pool(rs, acc_c)
        seg.finish(acc_c, out_c)
        sync(device)
        if hi < 130:  # a segment that is not final leaves the mean sequence's out row alone
            assert same_bits(out_c[1], before[1])
    assert same_bits(acc_c[1], acc_w[1]) and same_bits(out_c[1], out_w[1]), "the chunked sum differs from the whole one"
    assert same_bits(acc_c[4], acc_w[4]) and same_bits(out_c[4], out_w[4])
    # a continuation onto a planted accumulator adds onto it: the twin, started from the same planted row
    plant = torch.linspace(-3.0, 5.0, D)
    seg = Pack(D, nslab, device, lens=[9], modes=[1], slots=[2], seed=9, starts=[40], finals=[0], counts=[60])
    acc, out, rs = seg.fresh()
    acc[2] = plant.to(seg.device)
    seg.rowscale(rs)
    seg.pool(rs, acc)
    seg.finish(acc, out)
    sync(device)
    acc_t = torch.full((NSLOTS, D), SENTINEL)
    acc_t[2] = plant
    ref.embed_pool(seg.h, seg.parts, seg.cu, seg.meta, rs.cpu(), seg.gamma, acc_t)
    assert same_bits(acc, acc_t) and not same_bits(acc[2], plant)
    assert torch.equal(bits(out), bits(torch.full((NSLOTS, D), SENTINEL))), "finish wrote for a segment that is not final"


def check_last(D, nslab, device):
    """Last pooling: a segment that is not final writes nothing at all; the final one stores exactly the last row's y."""
    p = Pack(D, nslab, device, lens=[5, 60], modes=[2, 2], slots=[0, 3], seed=3, starts=[0, 64], finals=[0, 1],
             counts=[20, 130])
    acc, out, rs = p.fresh()
    p.rowscale(rs)
    p.pool(rs, acc)
    p.finish(acc, out)
    sync(device)
    sent = bits(torch.full((D,), SENTINEL))
    assert torch.equal(bits(acc[0]), sent) and torch.equal(bits(out[0]), sent)
    assert torch.equal(bits(rs[:64]), bits(torch.full((64,), SENTINEL))), "only the final segment's last row is scaled"
    t = p.T - 1
    y = (p.v()[t] * rs.cpu()[t]) * p.gamma.float()
    assert same_bits(acc[3], y)
    e = y.double() / y.double().norm()
    assert float((out[3].cpu().double() - e).abs().max()) <= (finish_chain(D) + 6) * U * float(e.abs().max())


def check_finish(D, device):
    """out against float64 from the device's own acc: |out - e| <= (c + 6) 2^-24 |e| on every element, with the chain
    of the finish reduction; a zero acc row gives zeros; ecount 1; mean against last on one accumulator."""
    g = torch.Generator().manual_seed(D)
    acc_h = torch.randn(NSLOTS, D, generator=g) * 37.0
    acc_h[6] = 0.0
    acc_h[7] = acc_h[0]
    meta = meta_of([1] * 5, [1, 2, 1, 1, 2], [0, 7, 6, 3, 5], counts=[130, 130, 9, 1, 4])
    dev = torch.device(device)
    acc, out = acc_h.to(dev), torch.full((NSLOTS, D), SENTINEL, device=dev)
    ops.embed_finish(torch.tensor(meta, dtype=torch.int32, device=dev), acc, out, host=(None, meta))
    sync(device)
    got = out.cpu().double()
    c = finish_chain(D)
    worst = 0.0
    for mode, slot, count in zip(meta[0], meta[2], meta[4]):
        if slot == 6:
            assert not bool(out[6].cpu().any()), "a zero accumulator must give zeros"
            continue
        m = acc_h[slot].double() / (count if mode == 1 else 1)
        e = m / m.norm()
        ratio = float(((got[slot] - e).abs() / ((c + 6) * U * e.abs()).clamp(min=1e-300)).max())
        worst = max(worst, ratio)
    print(f"finish D={D}: worst |out - e| / bound = {worst:.4f} (c = {c})")
    note(f"finish_D{D}", worst)
    assert worst <= 1.0
    # ecount 1: the mean of one row is the row; mean (count 130) and last on the same accumulator agree to the bound
    assert same_bits(out[3], _finish_twin(acc_h, 3, 2))
    assert float((got[0] - got[7]).abs().max()) <= 2 * (c + 6) * U * float(got[7].abs().max())
    for slot in (1, 2, 4, 8):
        assert torch.equal(bits(out[slot]), bits(torch.full((D,), SENTINEL)))
    out_t = torch.full((NSLOTS, D), SENTINEL)
    ref.embed_finish(meta, acc_h, out_t)
    assert same_bits(out, out_t), "finish differs from its twin"
    return worst


def _finish_twin(acc_h, slot, mode):
    out = torch.zeros_like(acc_h)
    ref.embed_finish([[mode], [0], [slot], [1], [1]], acc_h, out)
    return out[slot]


def check_refusals(device):
    """A bad mode, a slot out of range, wrong dtypes and an rs that is too short raise ValueError before any launch:
    acc, out and rs keep their sentinel."""
    import pytest

    p = Pack(64, 1, device, lens=[3, 4], modes=[1, 2], slots=[0, 1])
    acc, out, rs = p.fresh(nslots=2)
    d = p.d

    def meta_t(m):
        return torch.tensor(m, dtype=torch.int32, device=p.device)

    bad_mode = meta_of([3, 4], [1, 3], [0, 1])
    bad_slot = meta_of([3, 4], [1, 2], [0, 2])
    twice = meta_of([3, 4], [1, 2], [1, 1])
    cases = [
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], meta_t(bad_mode), rs, d["gamma"], acc, host=(p.cu, bad_mode)),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], meta_t(bad_slot), rs, d["gamma"], acc, host=(p.cu, bad_slot)),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], meta_t(bad_slot), rs, d["gamma"], acc),  # read from the tensor
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], meta_t(twice), rs, d["gamma"], acc, host=(p.cu, twice)),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"], rs, d["gamma"].float(), acc, host=p.host),
        lambda: ops.embed_pool(d["h"].double(), d["parts"], d["cu"], d["meta"], rs, d["gamma"], acc, host=p.host),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"].long(), rs, d["gamma"], acc, host=p.host),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"], rs[:6], d["gamma"], acc, host=p.host),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"], rs, d["gamma"], acc.double(), host=p.host),
        lambda: ops.embed_pool(d["h"], d["parts"], d["cu"], d["meta"], rs, d["gamma"], acc, host=([0, 3, 8], p.meta)),
        lambda: ops.embed_rowscale(d["h"], d["parts"], d["tseq"], d["cu"], meta_t(bad_mode), EPS, rs, host=(p.cu, bad_mode)),
        lambda: ops.embed_rowscale(d["h"], d["parts"], d["tseq"], d["cu"], d["meta"], EPS, rs[:6], host=p.host),
        lambda: ops.embed_rowscale(d["h"], d["parts"], d["tseq"].long(), d["cu"], d["meta"], EPS, rs, host=p.host),
        lambda: ops.embed_rowscale(d["h"], d["parts"].double(), d["tseq"], d["cu"], d["meta"], EPS, rs, host=p.host),
        lambda: ops.embed_finish(meta_t(bad_mode), acc, out, host=(None, bad_mode)),
        lambda: ops.embed_finish(meta_t(bad_slot), acc, out, host=(None, bad_slot)),
        lambda: ops.embed_finish(d["meta"], acc, out[:1], host=p.host),
        lambda: ops.embed_finish(d["meta"], acc, out.double(), host=p.host),
    ]
    for k, case in enumerate(cases):
        with pytest.raises(ValueError):
            case()
            pytest.fail(f"refusal case {k} was accepted")
    sync(device)
    for t in (acc, out, rs):
        assert torch.equal(bits(t), bits(torch.full_like(t, SENTINEL).cpu())), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ engine level
IN_LENS = (5, 64, 65, 130)


def input_ids(n: int, vocab: int = 400, k: int = 0) -> list:
    """An input of n tokens, BOS first."""
    return [1] + [5 + (7 * i + 13 * k) % vocab for i in range(n - 1)]


def oracle_vector(weights, ids, pooling: str, **fwd):
    """(e_o, kappa): the oracle's final-norm rows y_o pooled and normalised in float64, and kappa = mean ||y_o,t|| /
    ||pooled y_o|| (1 for last pooling over one row... of that row alone)."""
    from llm_based_apache_spark_optimization_amd.models.llama import reference_forward

    _, y = reference_forward(weights, ids, return_hidden=True, **fwd)
    y = y.double().cpu()
    rows = y if pooling == "mean" else y[-1:]
    pooled = rows.mean(0)
    kappa = float(rows.norm(dim=1).mean() / pooled.norm())
    return pooled / pooled.norm(), kappa
