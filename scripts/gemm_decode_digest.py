"""One SHA-256 per decode-GEMM case over the raw output bytes, for bitwise A/B runs of two builds on one machine.

    python scripts/gemm_decode_digest.py > digest.txt        # needs a GPU; compares nothing itself
    python scripts/gemm_decode_digest.py --each              # also one line per call (to find what differs)

A case is one (entry point, weight kind, N, K, M, activation layout); its digest covers the outputs of all its calls:
every epilogue and split-K count, with and without the row scale, at every (nb, waves, div) -- about 37,000 calls in
all; one line each, --each, is several MB of text.

Every decode entry point (ops.linear, ops.linear_xf with and without z12, ops.linear_rr, ops.linear_a8,
ops.linear_a8_rr; bf16 / fp8 / mxfp4 weights), M 1..64, K 256 / 1408 (fewer chunks than waves; odd and even chunk
counts per wave, unequal splits), N 256 / 352 (exact and ragged grids), every epilogue (bf16, f32 slabs at split-K
1 / 2 / 3, SiLU in both layouts, the residual epilogue at split-K 1 / 4 -- h, xout and ss_out hashed), with and
without the row scale, over every (nb, waves, div) variant of the launchers.  Inputs come from seeded CPU generators; every
case is deterministic by design (slab sums in contributor order, Q24 integer atomics), so two runs of one build print
the same lines.  A call the host code rejects (fp8 ragged grids, uneven W8A8 splits, ...) enters its case's digest
as the return code.  Each line: the case, its calls, how many of them were such refusals, the SHA-256; the last line
gives the totals.
"""
import hashlib
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_based_apache_spark_optimization_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "gemm_decode_digest needs a GPU"
DEV = torch.device("cuda:0")
MS = (1, 16, 17, 32, 33, 64)
NKS = [(N, K) for N in (256, 352) for K in (256, 1408)]
# every (waves, div) variant the launchers tell apart: five at nb 1 / 2 / 4, two (4 waves, div 1 | 2) at nb 6 / 8; for
# the fp8 / W8A8 kernels div 2 is chunk depth 2, so these are also their waves x depth variants.  A superset of the
# combinations in tests/test_kernels_gpu.py, tests/test_z12_gpu.py and tests/test_z12_depth_gpu.py
CFGS = [(nb, wv, dv) for nb in (1, 2, 4) for wv, dv in ((4, 1), (4, 2), (4, 4), (8, 1), (8, 2))] + \
       [(nb, 4, dv) for nb in (6, 8) for dv in (1, 2)]
EPS = 1e-5


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


EACH = "--each" in sys.argv[1:]
_sub = []
_total = [0, 0]  # calls, host refusals


def case(name, fn):
    """One call of a case: its digest (or the host code's refusal) joins the case's line, printed by flush().  Only
    a launcher's own rejection of the arguments (a negative return code, before any launch) is a refusal: any other
    error ends the run."""
    try:
        out = fn()
        torch.cuda.synchronize()
        _sub.append(f"{name} {digest(*out)}")
    except RuntimeError as e:
        m = re.search(r"lsa kernel '\w+' failed: rc=-\d+", str(e))
        if m is None:
            raise
        _sub.append(f"{name} ERR {m.group(0)}")


def flush(name):
    """case, calls, of which refused by the host code, SHA-256 over the calls' lines"""
    if EACH:
        print("\n".join("  " + s for s in _sub))
    nerr = sum(" ERR " in s for s in _sub)
    _total[0] += len(_sub)
    _total[1] += nerr
    print(name, len(_sub), nerr, hashlib.sha256("\n".join(_sub).encode()).hexdigest())
    _sub.clear()


_w = {}


def weight(kind, N, K):
    if (kind, N, K) not in _w:
        w = rnd(N + K, N, K, scale=0.02).to(torch.bfloat16).to(DEV)  # gate / up interleaved or not: the same bytes
        pw = ops.PackedWeight.from_dense(w, kind)
        if kind == "bf16":
            pw.add_z12()
            assert pw.z12 is not None, "the bf16 test weight must have its 12-bit companion (the z1 cases run it)"
        _w[kind, N, K] = pw
    return _w[kind, N, K]


def cfgs(M, silu=False):
    for nb, wv, dv in CFGS:
        if nb >= 6 and not 16 < M <= 32:  # wide n-groups: the two-row-tile kernels
            continue
        if M > 32 and nb > 2:  # the host clamps these to nb 2
            continue
        if silu and nb < 2:
            continue
        yield nb, wv, dv


def run_linear(kind):
    for N, K in NKS:
        pw = weight(kind, N, K)
        for M in MS:
            x = rnd(1000 * M + K, M, K).to(torch.bfloat16).to(DEV)
            ss = ops.ss_q24(x.float().pow(2).sum(1))
            a16 = rnd(7 * M + N, M, K).to(torch.bfloat16).to(DEV)
            h0 = rnd(M + N + K, M, N).to(DEV)
            for xf in (False, True):
                if xf and M <= 16:
                    continue
                xin, ain = (ops.to_xfrag(x), ops.to_xfrag(a16)) if xf else (x, a16)
                for z12 in ((False, True) if xf and kind == "bf16" and M <= 32 else (False,)):
                    def lin(a, epi, **kw):
                        if xf:
                            return ops.linear_xf(a, M, pw, epi, z12=z12, **kw)
                        return ops.linear(a, pw, epi, **kw)

                    for rn in (False, True):
                        rkw = {"rownorm": (ss, EPS)} if rn else {}
                        tag = f"{kind} N{N} K{K} M{M} xf{int(xf)} z{int(z12)} rn{int(rn)}"
                        for nb, wv, dv in cfgs(M):
                            if z12 and nb not in (2, 4, 6):
                                continue
                            c = dict(nb=nb, waves=wv, div=dv)
                            ct = f"nb{nb} w{wv} d{dv}"
                            case(f"{tag} bf16 {ct}", lambda: [lin(xin, "bf16", splitk=1, **c, **rkw)])
                            for sk in (1, 2, 3):
                                case(f"{tag} f32 sk{sk} {ct}", lambda: [lin(xin, "f32", splitk=sk, **c, **rkw)])
                            if nb >= 2:
                                case(f"{tag} silu {ct}", lambda: [lin(xin, "silu", splitk=1, **c, **rkw)])
                            for sk in (() if z12 else (1, 4)):
                                def res():
                                    hh = h0.clone()
                                    xout = torch.zeros(ops.xfrag_tiles(M) * 16 * N if xf else M * N, device=DEV,
                                                       dtype=torch.bfloat16)
                                    ss_out = torch.full((M,), 1 << 23, device=DEV, dtype=torch.int64)
                                    tickets = torch.zeros(N // 16, device=DEV, dtype=torch.int32)
                                    lin(ain, "res", splitk=sk, res=(hh, xout if xf else xout.view(M, N), ss_out, tickets),
                                        **c, **rkw)
                                    return [hh, xout, ss_out, tickets]

                                case(f"{tag} res sk{sk} {ct}", res)
                    flush(f"{kind} N{N} K{K} M{M} xf{int(xf)} z{int(z12)}")


def run_rr():
    for N, K in NKS:
        pw = weight("bf16", N, K)
        for np_ in (1, 2, 4):
            h = rnd(K + np_, 1, K).to(DEV)
            parts = rnd(N + K + np_, np_, 1, K).to(DEV)
            for nb, wv, dv in [c for c in CFGS if c[0] <= 4]:
                ct = f"rr bf16 N{N} K{K} np{np_} nb{nb} w{wv} d{dv}"
                c = dict(nb=nb, waves=wv, div=dv)
                for sk in (1, 2, 3):
                    def f32():
                        h_out = torch.zeros(K, device=DEV)
                        ss_out = torch.zeros(1, device=DEV, dtype=torch.int64)
                        y = ops.linear_rr(h, parts, h_out, pw, "f32", ss_out=ss_out, eps=EPS, splitk=sk, **c)
                        return [y, h_out, ss_out]

                    case(f"{ct} f32 sk{sk}", f32)
                if nb >= 2:
                    def silu():
                        h_out = torch.zeros(K, device=DEV)
                        return [ops.linear_rr(h, parts, h_out, pw, "silu", eps=EPS, **c), h_out]

                    case(f"{ct} silu", silu)
            flush(f"rr bf16 N{N} K{K} np{np_}")


def run_a8(kind):
    for N, K in NKS:
        pw = weight(kind, N, K)
        for M in MS:
            x = rnd(1000 * M + K, M, K).to(torch.bfloat16).to(DEV)
            ss = ops.ss_q24(x.float().pow(2).sum(1))
            x8, sx = ops.quantize_xf8(x)
            xb8, s8 = ops.quantize_xf8_blocks(x, 32)
            mt = ops.xfrag_tiles(M)
            for asc in (False, True):
                a = dict(s8=s8) if asc else {}
                xa, sa = (xb8, None) if asc else (x8, sx)
                for rn in (False, True):
                    rkw = {"rownorm": (ss, EPS)} if rn else {}
                    tag = f"a8 {kind} N{N} K{K} M{M} asc{int(asc)} rn{int(rn)}"
                    for nb, wv, dv in cfgs(M):
                        c = dict(nb=nb, waves=wv, div=dv)
                        ct = f"nb{nb} w{wv} d{dv}"
                        for sk in (1, 2, 3):
                            case(f"{tag} f32 sk{sk} {ct}",
                                 lambda: [ops.linear_a8(xa, sa, M, pw, "f32", splitk=sk, **c, **a, **rkw)])
                        for xfo in ((True, False) if nb >= 2 else ()):
                            case(f"{tag} silu xfo{int(xfo)} {ct}",
                                 lambda: [ops.linear_a8(xa, sa, M, pw, "silu", xfo=xfo, **c, **a, **rkw)])

                        def silu8():
                            o8 = torch.zeros(mt * 16 * N // 2, device=DEV, dtype=torch.uint8)
                            os8 = torch.zeros(mt * 64 * -(-(N // 2) // 128), device=DEV, dtype=torch.uint8)
                            ops.linear_a8(xa, sa, M, pw, "silu", out=o8, out_s8=os8, **c, **a, **rkw)
                            return [o8, os8]

                        if nb % 4 == 0 and (N // 2) % 128 == 0:
                            case(f"{tag} silu8 {ct}", silu8)
                flush(f"a8 {kind} N{N} K{K} M{M} asc{int(asc)}")
        for np_ in (1, 2, 4):  # batch 1 with the residual-reduce prologue
            h = rnd(K + np_, 1, K).to(DEV)
            parts = rnd(N + K + np_, np_, 1, K).to(DEV)
            for nb, wv, dv in [c for c in CFGS if c[0] != 6]:
                ct = f"a8rr {kind} N{N} K{K} np{np_} nb{nb} w{wv} d{dv}"
                c = dict(nb=nb, waves=wv, div=dv)
                for sk in (1, 2):
                    def f32():
                        h_out = torch.zeros(K, device=DEV)
                        ss_out = torch.zeros(1, device=DEV, dtype=torch.int64)
                        y = ops.linear_a8_rr(h, parts, h_out, pw, "f32", ss_out=ss_out, eps=EPS, splitk=sk, **c)
                        return [y, h_out, ss_out]

                    case(f"{ct} f32 sk{sk}", f32)

                def silu8():
                    h_out = torch.zeros(K, device=DEV)
                    o8 = torch.zeros(16 * N // 2, device=DEV, dtype=torch.uint8)
                    os8 = torch.zeros(64 * (N // 2 // 128), device=DEV, dtype=torch.uint8)
                    ops.linear_a8_rr(h, parts, h_out, pw, "silu", out=o8, out_s8=os8, eps=EPS, **c)
                    return [o8, os8, h_out]

                if nb % 4 == 0 and (N // 2) % 128 == 0:
                    case(f"{ct} silu8", silu8)
            flush(f"a8rr {kind} N{N} K{K} np{np_}")


def main():
    ops.ext()
    for kind in ("bf16", "fp8", "mxfp4"):
        run_linear(kind)
    run_rr()
    for kind in ("fp8", "mxfp4"):
        run_a8(kind)
    print("# total", _total[0], "calls,", _total[1], "refused by the host code")


if __name__ == "__main__":
    main()
