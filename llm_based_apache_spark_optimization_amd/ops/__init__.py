"""Fused operators of the decode engine.

GPU tensors run the hand-written gfx950 kernels of ``csrc/kernels`` through the in-tree extension
``_lsa_hip``; there is no silent fallback — if the extension is missing while a GPU tensor is passed,
the op raises.  CPU tensors run ``ops.reference`` (the fp32 oracle the GPU tests compare against) so
the engine and its scheduler can be exercised on a machine without a GPU.

Weights are held as :class:`PackedWeight`: on the GPU in the MFMA fragment-major layout
(``shuffle_weight``) or fp8-e4m3fn with per-channel scales (``quantize_fp8``); on the CPU as the
plain ``[N, K]`` matrix.
"""
from __future__ import annotations

import dataclasses
import importlib
import importlib.util
import json
import math
import os
from typing import NamedTuple, Optional

import torch

from . import reference as ref

_ext = None
_ext_err: Optional[BaseException] = None

EPI = {"bf16": 0, "f32": 1, "silu": 2, "res": 3}


def ext():
    """The compiled gfx950 extension (raises if it cannot be loaded)."""
    global _ext, _ext_err
    if _ext is None and _ext_err is None:
        try:
            alt = os.environ.get("LSA_HIP_SO")  # experiment knob: an alternative build of the same extension
            if alt:
                spec = importlib.util.spec_from_file_location("_lsa_hip", alt)
                _ext = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(_ext)
            else:
                _ext = importlib.import_module(__name__ + "._lsa_hip")
        except BaseException as e:  # noqa: BLE001 - record and re-raise on use
            _ext_err = e
    if _ext is None:
        raise RuntimeError(
            "gfx950 extension _lsa_hip is not built/loadable; run "
            "`python -m llm_based_apache_spark_optimization_amd.ops.build`"
        ) from _ext_err
    if not BUILD_INFO:
        _check_provenance()
    return _ext


# build provenance of the loaded extension (ops/build.py writes _lsa_hip.provenance.json next to the .so): the
# sources hash it was built from, its own hash, and whether both still match the tree -- a stale .so (kernels
# edited, not rebuilt) fails loudly on load instead of silently running old kernels (LSA_ALLOW_STALE_EXT=1 to
# override, e.g. for A/B builds)
BUILD_INFO: dict = {}


def _check_provenance() -> None:
    import hashlib

    from . import build as _b

    so = getattr(_ext, "__file__", "") or ""
    info = {"so": os.path.basename(so)}
    try:
        rec = json.loads(_b.PROVENANCE.read_text())
    except (OSError, ValueError):
        rec = None
    info["provenance"] = rec
    if rec is not None and so and os.path.abspath(so) == str(_b.HIP_EXT):
        try:
            with open(so, "rb") as f:
                info["so_match"] = hashlib.sha256(f.read()).hexdigest()[:16] == rec.get("so_sha256")
        except OSError:
            info["so_match"] = False
        try:
            info["sources_match"] = _b.sources_sha() == rec.get("sources_sha")
        except OSError:  # sources not shipped with this tree
            info["sources_match"] = None
    BUILD_INFO.update(info)
    if (info.get("so_match") is False or info.get("sources_match") is False) and \
            os.environ.get("LSA_ALLOW_STALE_EXT") != "1":
        raise RuntimeError(f"_lsa_hip.so does not match its sources / provenance record ({info}); rebuild with "
                           "`python -m llm_based_apache_spark_optimization_amd.ops.build`")


def hip_available() -> bool:
    try:
        ext()
        return True
    except RuntimeError:
        return False


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ----------------------------------------------------------------------------------- weights
def shuffle_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> fragment-major [N/16, K/32, 64 lanes, 8]: lane = 16*((k%32)//8) + n%16."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    return w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def unshuffle_weight(wf: torch.Tensor, N: int, K: int) -> torch.Tensor:
    return wf.reshape(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K)


def interleave_gate_up(wg: torch.Tensor, wu: torch.Tensor) -> torch.Tensor:
    """Stack gate and up rows interleaved per 16 so one skinny-GEMM wave owns matching pairs."""
    F, K = wg.shape
    return torch.stack([wg.view(F // 16, 16, K), wu.view(F // 16, 16, K)], dim=1).reshape(2 * F, K)


def pack_fp8(q: torch.Tensor) -> torch.Tensor:
    """e4m3fn bytes [N, K] -> the fragment layout [N/16, K/64, 64 lanes, 16 B], lane = 16 g + r holding
    W[16 nb + r][64 kb + 16 g .. + 15]."""
    N, K = q.shape
    assert N % 16 == 0 and K % 64 == 0, (N, K)
    return q.view(torch.uint8).reshape(N // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous()


def quantize_fp8(w: torch.Tensor):
    """Per-output-channel e4m3fn quantisation -> (packed uint8 [N/16, K/64, 64, 16], scale f32 [N])."""
    N, K = w.shape
    assert N % 16 == 0 and K % 64 == 0, (N, K)
    wf = w.float()
    scale = (wf.abs().amax(dim=1) / 448.0).clamp(min=1e-12)
    q = (wf / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return pack_fp8(q), scale


def dequantize_fp8(packed: torch.Tensor, scale: torch.Tensor, N: int, K: int) -> torch.Tensor:
    q = packed.reshape(N // 16, K // 64, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K)
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


# MXFP4 (OCP MX): e2m1 elements, one E8M0 power-of-two scale per 32 consecutive k (csrc/kernels/gemm_fp4.hip)
FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_FP4_EDGES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)  # midpoints of the e2m1 magnitude grid


def quantize_mxfp4(w: torch.Tensor):
    """[N, K] -> (e2m1 codes uint8 [N, K] (sign in bit 3), E8M0 scale bytes uint8 [N, K/32]): per 32-element block
    scale 2^(floor(log2 amax) - 2) (e2m1 emax = 2, OCP MX), elements rounded to the e2m1 grid, saturated at 6."""
    N, K = w.shape
    assert K % 32 == 0, K
    wf = w.float().view(N, K // 32, 32)
    amax = wf.abs().amax(-1)
    e = (torch.floor(torch.log2(amax.clamp(min=2.0 ** -125))) - 2).clamp(-126, 127)
    e = torch.where(amax > 0, e, torch.full_like(e, -127))
    v = wf / torch.exp2(e.clamp(min=-126))[..., None]
    mag = torch.bucketize(v.abs().clamp(max=6.0), torch.tensor(_FP4_EDGES, device=w.device))
    codes = (mag | ((v < 0).to(mag.dtype) << 3)).to(torch.uint8).view(N, K)
    return codes, (e + 127).to(torch.uint8)


def pack_mxfp4(codes: torch.Tensor, sbytes: torch.Tensor):
    """codes [N, K], scale bytes [N, K/32] -> the gemm_fp4 layouts: Wq [N/16, K/128, 64 lanes, 16 B] (lane = 16 g + r
    holds W[16 nb + r][128 kb + 32 g .. + 31], element 2i in the low nibble of byte i) and S [N/16, ceil(K/512), 64, 4]
    (the lane's scale byte of four consecutive 128-k steps in one word)."""
    N, K = codes.shape
    assert N % 16 == 0 and K % 128 == 0, (N, K)
    c = codes.view(N, K // 2, 2)
    packed = (c[..., 0] | (c[..., 1] << 4)).contiguous()
    wq = packed.view(N // 16, 16, K // 128, 4, 16).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 128, 64, 16)
    kb = K // 128
    kb4 = (kb + 3) // 4
    sl = sbytes.view(N // 16, 16, kb, 4).permute(0, 2, 3, 1).reshape(N // 16, kb, 64)
    sp = torch.zeros(N // 16, kb4 * 4, 64, dtype=torch.uint8, device=codes.device)
    sp[:, :kb] = sl
    return wq, sp.view(N // 16, kb4, 4, 64).permute(0, 1, 3, 2).contiguous()


def dequantize_mxfp4(wq: torch.Tensor, sw: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """The exact f32 values the gemm_fp4 kernels multiply with (e2m1 value x 2^(e - 127))."""
    kb = K // 128
    packed = wq.reshape(N // 16, kb, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K // 2)
    codes = torch.stack([packed & 15, packed >> 4], dim=-1).view(N, K).long()
    vals = torch.tensor(FP4_VALUES, device=wq.device)[codes & 7] * (1.0 - 2.0 * (codes >> 3).float())
    sb = sw.reshape(N // 16, -1, 64, 4).permute(0, 1, 3, 2).reshape(N // 16, -1, 64)[:, :kb]
    sb = sb.reshape(N // 16, kb, 4, 16).permute(0, 3, 1, 2).reshape(N, K // 32).float()
    scale = torch.where(sb > 0, torch.exp2(sb - 127.0), torch.zeros_like(sb))
    return (vals.view(N, K // 32, 32) * scale[..., None]).view(N, K)


# GGUF Q4_0 (ggml block_q4_0): 32 consecutive k share one f16 scale d, elements are 4-bit codes q.  The value rule of
# every consumer (csrc/kernels/gemm_q4.hip, dequantize_q4_0): w = bf16_rne(f32(d) * f32(q - 8)); the f32 product is
# exact (11 significand bits x 4), so the one rounding is the one to bf16.
def _check_q4_shape(N: int, K: int) -> None:
    if N <= 0 or K <= 0 or N % 16 or K % 128:
        raise ValueError(f"q4_0 weights need N % 16 == 0 and K % 128 == 0, got N = {N}, K = {K}")


def quantize_q4_0(w: torch.Tensor):
    """[N, K] -> (codes uint8 [N, K] in 0..15, d f16 [N, K/32]) by ggml's reference rule, in f32: per block of 32,
    max = the first element of largest magnitude (with its sign), d = max / -8, id = 1 / d (0 for d = 0),
    q = min(15, trunc(x * id + 8.5)); d is stored as f16."""
    N, K = w.shape
    if K % 32:
        raise ValueError(f"q4_0 blocks are 32 wide, got K = {K}")
    x = w.float().reshape(N, K // 32, 32)
    a = x.abs()
    pos = torch.arange(32, device=x.device)
    first = torch.where(a == a.amax(-1, keepdim=True), pos, pos.new_full((), 32)).amin(-1, keepdim=True)
    d = x.gather(-1, first.clamp(max=31)).squeeze(-1) / -8.0
    inv = torch.where(d != 0, 1.0 / d, torch.zeros_like(d))
    q = ((x * inv[..., None]) + 8.5).to(torch.int32).clamp(max=15)
    return q.to(torch.uint8).reshape(N, K), d.to(torch.float16)


def q4_0_values(codes: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """The value rule on plain (codes [N, K], d [N, K/32]): bf16 [N, K]."""
    N, K = codes.shape
    v = d.float()[..., None] * (codes.reshape(N, K // 32, 32).float() - 8.0)
    return v.to(torch.bfloat16).reshape(N, K)


def pack_q4_0(codes: torch.Tensor, d: torch.Tensor):
    """codes [N, K], d f16 [N, K/32] -> the gemm_q4 layouts: Wq [N/16, K/128, 64 lanes, 16 B] (lane = 16 g + r holds
    W[16 nb + r][128 kb + 32 g .. + 31], one Q4_0 block; byte 4 s + i = element 8 s + i in the low nibble, element
    8 s + 4 + i in the high one) and D f16 [N/16, ceil(K/256), 64, 2] (the lane's d of two consecutive 128-k steps in
    one word)."""
    N, K = codes.shape
    _check_q4_shape(N, K)
    if tuple(d.shape) != (N, K // 32) or d.dtype != torch.float16 or codes.dtype != torch.uint8:
        raise ValueError(f"pack_q4_0: codes uint8 [N, K] and d f16 [N, K/32], got {codes.dtype} {tuple(codes.shape)}, "
                         f"{d.dtype} {tuple(d.shape)}")
    c = codes.reshape(N, K // 8, 2, 4)
    packed = (c[:, :, 0] | (c[:, :, 1] << 4)).reshape(N, K // 2)
    kb = K // 128
    wq = packed.view(N // 16, 16, kb, 4, 16).permute(0, 2, 3, 1, 4).reshape(N // 16, kb, 64, 16).contiguous()
    kb2 = (kb + 1) // 2
    dl = d.reshape(N // 16, 16, kb, 4).permute(0, 2, 3, 1).reshape(N // 16, kb, 64)
    dp = torch.zeros(N // 16, kb2 * 2, 64, dtype=torch.float16, device=codes.device)
    dp[:, :kb] = dl
    return wq, dp.view(N // 16, kb2, 2, 64).permute(0, 1, 3, 2).contiguous()


def unpack_q4_0(wq: torch.Tensor, dw: torch.Tensor, N: int, K: int):
    """The inverse of ``pack_q4_0``: (codes uint8 [N, K], d f16 [N, K/32])."""
    _check_q4_shape(N, K)
    kb = K // 128
    p = wq.reshape(N // 16, kb, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K // 8, 4)
    codes = torch.stack([p & 15, p >> 4], dim=2).reshape(N, K)
    dl = dw.reshape(N // 16, -1, 64, 2).permute(0, 1, 3, 2).reshape(N // 16, -1, 64)[:, :kb]
    return codes, dl.reshape(N // 16, kb, 4, 16).permute(0, 3, 1, 2).reshape(N, K // 32)


def dequantize_q4_0(wq: torch.Tensor, dw: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """The exact values the gemm_q4 kernels multiply with, from the packed layout, as f32: the value rule."""
    return q4_0_values(*unpack_q4_0(wq, dw, N, K)).float()


# "z12": the bf16 values of a weight as a lossless 12-bit stream for the 17-32-row decode GEMM (csrc/kernels/gemm_z12.hip
# documents the format).  The exponents of a weight matrix sit in a handful of binades, so per tensor one window of 8
# consecutive values of exp[7:1] (16 binades) covers all but ~1e-4 of the elements; those are patched exactly from a
# list of up to four entries per 16 x 32 fragment.  784 bytes per fragment instead of 1024.
# LSA_Z12=0 skips the packing at load (it costs 0.77 x the bf16 bytes on top of them: the bf16 copy stays for prefill and
# every other bucket).
Z12 = os.environ.get("LSA_Z12", "1") != "0"
Z12_WINDOW = 8      # values of exp[7:1] a HI code addresses
Z12_MAX_ESC = 4     # patch entries per fragment


class Z12Planes(NamedTuple):
    lo: torch.Tensor    # uint8 [N/16, K/32, 64, 8]: byte i = low byte of the lane's element i
    hi: torch.Tensor    # uint8 [N/16, K/32, 64, 4]: byte j = code(element j) | code(element 4 + j) << 4
    esc: torch.Tensor   # int32 [N/16, K/32, 4]: valid << 31 | lane << 20 | slot << 16 | bf16 bits
    base: int           # first exp[7:1] value of the window

    @property
    def nbytes(self) -> int:
        return self.lo.numel() + self.hi.numel() + 4 * self.esc.numel()


def z12_base(wf: torch.Tensor) -> int:
    """The window start (1..120) whose 8 consecutive exp[7:1] values cover the most elements (the first such).  Windows
    never hold exp[7:1] = 0: zeros and values below 2^-125 are always patch entries."""
    e7 = (wf.reshape(-1).view(torch.int16).to(torch.int32) >> 8) & 0x7F
    hist = torch.bincount(e7, minlength=128)[:128].to(torch.int64)
    c = torch.cat([hist.new_zeros(1), hist.cumsum(0)])
    cover = c[1 + Z12_WINDOW:129] - c[1:129 - Z12_WINDOW]  # cover[b - 1] = sum(hist[b : b + 8]), b = 1..120
    return int(cover.argmax().item()) + 1


def pack_z12(w: torch.Tensor) -> Optional[Z12Planes]:
    """bf16 weight ([N, K], or already fragment-major as ``shuffle_weight`` returns it) -> its z12 planes, or None when
    some fragment has more than four elements outside the tensor's window (not compressible: the weight keeps only its
    bf16 copy and kernel)."""
    wf = shuffle_weight(w) if w.dim() == 2 else w
    assert wf.dtype == torch.bfloat16 and wf[0, 0].numel() == 512, (wf.dtype, wf.shape)
    NB, KB = wf.shape[:2]
    wf = wf.reshape(NB, KB, 64, 8)
    base = z12_base(wf)
    bits = wf.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    hb = bits >> 8
    e7 = hb & 0x7F
    out = (e7 < base) | (e7 >= base + Z12_WINDOW)
    if int(out.sum(dim=(2, 3)).max().item()) > Z12_MAX_ESC:
        return None
    code = torch.where(out, torch.zeros_like(hb), ((hb >> 7) << 3) | (e7 - base))  # filler: +, first binade pair
    lo = (bits & 0xFF).to(torch.uint8)
    hi = (code[..., :4] | (code[..., 4:] << 4)).to(torch.uint8)
    esc = torch.zeros(NB * KB, Z12_MAX_ESC, dtype=torch.int64, device=wf.device)
    idx = out.nonzero()  # row-major order: a fragment's entries by (lane, slot)
    if idx.shape[0]:
        f = idx[:, 0] * KB + idx[:, 1]
        first = torch.searchsorted(f, f)  # f is sorted: the first entry of each fragment
        rank = torch.arange(f.numel(), device=f.device) - first
        val = bits[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].to(torch.int64)
        esc[f, rank] = (1 << 31) | (idx[:, 2] << 20) | (idx[:, 3] << 16) | val
    esc = torch.where(esc >= (1 << 31), esc - (1 << 32), esc).to(torch.int32)
    return Z12Planes(lo.contiguous(), hi.contiguous(), esc.view(NB, KB, Z12_MAX_ESC).contiguous(), base)


def unpack_z12(z: Z12Planes) -> torch.Tensor:
    """z12 planes -> the fragment-major bf16 tensor [N/16, K/32, 64, 8], formed the way the kernel forms it: high byte
    (c & 8) << 4 | ((c & 7) + base) over the low byte, then the valid patch entries."""
    hi = z.hi.to(torch.int32)
    code = torch.cat([hi & 0xF, hi >> 4], dim=-1)
    bits = ((((code & 8) << 4) | ((code & 7) + z.base)) << 8) | z.lo.to(torch.int32)
    e = z.esc.to(torch.int64) & 0xFFFFFFFF
    at = (e >> 31).nonzero()
    if at.shape[0]:
        ev = e[at[:, 0], at[:, 1], at[:, 2]]
        bits[at[:, 0], at[:, 1], (ev >> 20) & 63, (ev >> 16) & 7] = (ev & 0xFFFF).to(torch.int32)
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(torch.bfloat16)


@dataclasses.dataclass
class PackedWeight:
    """A linear layer's weight in the layout its kernel streams."""

    N: int
    K: int
    kind: str  # "dense" (CPU reference) | "bf16" (fragment layout) | "fp8" | "mxfp4" | "q4_0"
    data: torch.Tensor
    scale: Optional[torch.Tensor] = None
    requested: Optional[str] = None  # "dense" only: the kind the weight was packed for (the CPU keeps every kind dense)
    z12: Optional[Z12Planes] = None  # "bf16" only: the same values as a 12-bit stream (linear_xf at 17-32 rows)

    def add_z12(self) -> "PackedWeight":
        """Attach the z12 companion of a GPU bf16 weight (a no-op for other kinds, under LSA_Z12=0, and for tensors that
        are not compressible)."""
        if Z12 and self.kind == "bf16" and self.z12 is None:
            self.z12 = pack_z12(self.data)
        return self

    @staticmethod
    def from_dense(w: torch.Tensor, kind: str = "bf16") -> "PackedWeight":
        N, K = w.shape
        if kind == "q4_0":  # the CPU keeps the quantised-then-dequantised values: the GPU engine's numerics class
            _check_q4_shape(N, K)
            return PackedWeight.from_q4_0(*quantize_q4_0(w))
        if not w.is_cuda:
            return PackedWeight(N, K, "dense", w.to(torch.bfloat16).contiguous(), None, kind)
        if kind == "fp8":
            q, s = quantize_fp8(w)
            return PackedWeight(N, K, "fp8", q, s.contiguous())
        if kind == "mxfp4":
            wq, sw = pack_mxfp4(*quantize_mxfp4(w))
            return PackedWeight(N, K, "mxfp4", wq, sw)
        wb = w.to(torch.bfloat16)
        return PackedWeight(N, K, "bf16", shuffle_weight(wb))

    @staticmethod
    def from_q4_0(codes: torch.Tensor, d: torch.Tensor) -> "PackedWeight":
        """Q4_0 codes uint8 [N, K] and block scales f16 [N, K/32] taken verbatim (a GGUF tensor's own)."""
        N, K = codes.shape
        _check_q4_shape(N, K)
        if not codes.is_cuda:
            return PackedWeight(N, K, "dense", q4_0_values(codes, d).contiguous(), None, "q4_0")
        wq, dw = pack_q4_0(codes, d)
        return PackedWeight(N, K, "q4_0", wq, dw)

    def dense(self) -> torch.Tensor:
        if self.kind == "dense":
            return self.data
        if self.kind == "bf16":
            return unshuffle_weight(self.data, self.N, self.K)
        if self.kind == "mxfp4":
            return dequantize_mxfp4(self.data, self.scale, self.N, self.K).to(torch.bfloat16)
        if self.kind == "q4_0":
            return q4_0_values(*unpack_q4_0(self.data, self.scale, self.N, self.K))
        return dequantize_fp8(self.data, self.scale, self.N, self.K).to(torch.bfloat16)

    @property
    def nbytes(self) -> int:
        return self.data.numel() * self.data.element_size() + (
            self.scale.numel() * self.scale.element_size() if self.scale is not None else 0)


def pick_nb_splitk(M: int, N: int, K: int, epi: str) -> tuple[int, int]:
    """Skinny-GEMM decomposition (from scripts/bench_gemm.py sweeps on MI355X).

    M <= 16: one 16-row block per wave-group (x traffic is negligible), split-K until >= 1024
    workgroups.  M > 16: 4 blocks (64 rows) per workgroup so each activation fragment feeds 4 MFMAs,
    split-K until >= 256 workgroups.  Only the f32 epilogue (partial slabs summed by the consumer)
    can split K.
    """
    nbt = N // 16
    if M <= 16:
        nb, target = 1, 1024
    else:
        nb, target = (4 if M <= 32 else 2), 256
    if epi == "silu":
        nb = max(nb, 2)
    while nb > 1 and nbt % nb:
        nb //= 2
    splitk = 1
    if epi == "f32" and M <= 64:
        while (nbt // nb) * splitk < target and splitk < 8 and K // (32 * splitk * 2) >= 16:
            splitk *= 2
    return nb, splitk


# ----------------------------------------------------------------------------------- tuning
_TUNING_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuning.json")
_tuning: Optional[dict] = None


# experiment overrides of tuning entries (in-pipeline A/Bs: bench.py --set 'ops.TUNING_OVERRIDES={"key": {...}}'),
# consulted before the measured table; empty in production
TUNING_OVERRIDES: dict = {}


def _tuning_table() -> dict:
    """Measured best decode-GEMM configs on MI355X ({"NxK:epi:s|m": {nb, splitk, waves, div}}),
    produced by scripts/bench_gemm.py (median of 3 interleaved runs per config)."""
    global _tuning
    if _tuning is None:
        try:
            with open(_TUNING_PATH) as f:
                _tuning = json.load(f)
        except (OSError, ValueError):
            _tuning = {}
    return {**_tuning, **TUNING_OVERRIDES} if TUNING_OVERRIDES else _tuning


def pick_gemm_config(M: int, N: int, K: int, epi: str, xf: bool = False,
                     kind: str = "bf16") -> tuple[int, int, int, int]:
    """(nb, splitk, waves, div) for a decode GEMM: the tuning table when it has the shape (entries
    measured with fragment-major activations carry a ':xf' suffix, fp8-weight entries ':fp8'), else
    the heuristic below (div 4, 4-wave workgroups won most measured shapes)."""
    if kind in ("mxfp4", "q4_0"):  # W4A16 decode GEMM (gemm_fp4.hip): its own sweep entries (scripts/bench_fp4_decode.py);
        # Q4_0 (gemm_q4.hip) looks under ':q4' and, without an entry, takes the same heuristic: the same byte stream
        # per lane and the same MFMA count
        b = 1
        while b < M:
            b *= 2
        sfx = "fp4" if kind == "mxfp4" else "q4"
        e = _tuning_table().get(f"{N}x{K}:{epi}:b{b}:{sfx}") or _tuning_table().get(
            f"{N}x{K}:{'f32' if epi == 'res' else epi}:b{b}:{sfx}")
        if e is not None and M <= 64:
            return e["nb"], e["splitk"], e["waves"], 4
        nbt = N // 16
        nb = 2 if M <= 16 else (8 if M <= 32 else 2)
        while nb > 1 and nbt % nb:
            nb //= 2
        if epi == "silu":
            nb = max(nb, 2)
        sk, target = 1, (512 if M <= 16 else 256)
        if epi in ("f32", "res"):
            while (nbt // nb) * sk < target and sk < 8 and K // (128 * sk * 2) >= 4:
                sk *= 2
        return nb, sk, 4, 4
    if kind in ("fp8a", "fp4a"):  # W8A8 / W4A8 decode GEMM: its own sweep entries, else the 16-bit-activation
        # kernel's (nb, splitk) at default knobs; 'silu8' = the e4m3 SiLU output (whole 32-column blocks: nb % 4 == 0)
        b = 1
        while b < M:
            b *= 2
        e = _tuning_table().get(f"{N}x{K}:{epi}:b{b}:{kind}")
        if e is not None:
            return e["nb"], e["splitk"], e["waves"], e["div"]
        if epi == "silu8":
            nbt = N // 16
            nb = 8 if (M <= 16 and nbt % 8 == 0 and nbt // 8 >= 256) else 4
            assert nbt % nb == 0, f"e4m3 SiLU output needs N / 16 % 4 == 0 (N = {N})"
            return nb, 1, 4, 4
        nb, sk, _, _ = pick_gemm_config(M, N, K, epi, xf=xf, kind="fp8" if kind == "fp8a" else "mxfp4")
        return (2 if (M > 32 and nb > 2) else nb), sk, 4, 4
    if epi == "res":  # the residual epilogue runs the f32-slab main loop (split-K with a last-arriver finish):
        # its own measured entries (scripts/bench_res_epi.py --tune) first, else the f32 entries
        b = 1
        while b < M:
            b *= 2
        e = _tuning_table().get(f"{N}x{K}:res:b{b}" + (":fp8" if kind == "fp8" else ""))
        if e is not None and M <= 64 and not (M > 32 and e["nb"] > 2):
            return e["nb"], e["splitk"], e["waves"], e["div"]
        epi = "f32"
    if M <= 64:
        key = f"{N}x{K}:{epi}:{'s' if M <= 16 else 'm'}"
        tab = _tuning_table()
        e = None
        # per-batch-bucket entries (power-of-two M) where a sweep beat the s/m entry by > 3 %
        # (scripts/bench_gemm_buckets.py, profiles/gemm_buckets_mi355x.jsonl)
        b = 1
        while b < M:
            b *= 2
        e = tab.get(f"{N}x{K}:{epi}:b{b}" + (":fp8" if kind == "fp8" else ":xf" if xf else ""))
        if e is None and kind == "fp8":
            e = tab.get(key + ":fp8")
        fp8_entry = e is not None and kind == "fp8"
        if e is None and xf:
            e = tab.get(key + ":xf")
        e = e if e is not None else tab.get(key)
        if e is not None and not (M > 32 and e["nb"] > 2):
            if kind == "fp8" and not fp8_entry:  # a bf16 entry's nb / split only; fp8 knobs at their defaults
                return e["nb"], e["splitk"], 4, 4
            return e["nb"], e["splitk"], e["waves"], e["div"]
    nb, sk = pick_nb_splitk(M, N, K, epi)
    return nb, sk, 4, 4


# ----------------------------------------------------------------------------------- linear
_dq_scratch: dict = {}


def _fp8_depth(div) -> int:
    """fp8 skinny GEMM chunk depth from a config tuple's 4th field: entries measured for fp8 store the
    depth (1 | 2) there; the bf16 'div' defaults (4) mean the shallow default."""
    return 2 if div == 2 else 1


SS_SCALE = float(1 << 24)


def ss_q24(v: torch.Tensor) -> torch.Tensor:
    """f32 sums of squares -> the kernels' int64 Q24 fixed point (truncating, like the device conversion)."""
    return (v.float() * SS_SCALE).to(torch.int64)


def ss_float(q: torch.Tensor) -> torch.Tensor:
    return q.double().div(SS_SCALE).float()


def _epi_kw(rownorm, res, xmt: int) -> dict:
    """Keyword arguments of the kernels' decode epilogue extensions (csrc/kernels/lsa_epi.h).

    rownorm = (ss, eps): the input rows are the UN-normalised residual stream (RMSNorm gamma folded into
    the weight): output row m is scaled by rsqrt(ss[m] / K + eps).  Row sums of squares (``ss``, ``ss_out``)
    are int64 Q24 fixed point (value * 2^24, ``SS_SCALE``): the kernels add them with integer atomics, so the
    total does not depend on workgroup arrival order and batched decoding stays deterministic.
    res = (h, xout, ss_out[, tickets]) with epi='res': h += y (f32 [M, N]); xout = bf16(h) (fragment-major
    when the call is linear_xf, else row-major [M, N]); ss_out[m] += sum_n h[m, n]^2 (the next GEMM's
    rownorm).  With ``tickets`` (int32, >= N/16 zeroed counters) the GEMM may split K: the splits publish
    f32 partials into ``out`` ([splitk, M, N]) and the last to arrive finishes each column."""
    kw = {}
    if rownorm is not None:
        kw["rowss"], kw["eps"] = rownorm[0], float(rownorm[1])
    if res is not None:
        kw["h"], kw["xout"], kw["ss_out"] = res[:3]
        kw["xmt"] = xmt
        if len(res) > 3 and res[3] is not None:
            kw["tickets"] = res[3]
    return kw


def _res_split(res, splitk: int, out, M: int, N: int, device):
    """(splitk, out) of a residual-epilogue call: split-K needs the ticket counters and a slab buffer."""
    if len(res) < 4 or res[3] is None or splitk <= 1:
        return 1, res[0]
    if out is None:
        out = torch.empty(splitk, M, N, device=device, dtype=torch.float32)
    return splitk, out


def _epi_ref(y: torch.Tensor, M: int, K: int, epi: str, rownorm, res, xf: bool):
    """CPU semantics of the epilogue extensions on a reference result y (f32 [M, N] or bf16 silu output
    computed from row-scaled inputs)."""
    h, xout, ss_out = res[:3]
    hn = h[:M].float() + y.float()
    h[:M].copy_(hn)
    x16 = hn.to(torch.bfloat16)
    if xf:
        f = to_xfrag(x16)
        xout.view(-1)[: f.numel()].copy_(f)
    else:
        xout.view(-1)[: x16.numel()].copy_(x16.reshape(-1))
    ss_out[:M] += ss_q24(hn.pow(2).sum(1))


# ----------------------------------------------------------------------------------- prefill GEMM (M > 64)
# Every prefill projection runs on the stream-K 256^2 MFMA kernel (csrc/kernels/gemm_tile256.hip): a persistent grid
# of one workgroup per CU, whole tiles for the full rounds and K-range shares of the rest, partial tiles summed by the
# last workgroup to arrive.  Its workspace (partial slots + tickets) is per (device, HIP stream): co-served engines
# prefill on their own streams and must not share tickets.
_sk_ws: dict = {}
# fewest K-tiles (64 deep) a workgroup's stream-K share may hold: below it the grid shrinks instead (fewer partial
# tiles, each summed from fewer contributors)
SK_MIN_SHARE = int(os.environ.get("LSA_SK_MIN_SHARE", "8"))
_SK_EPI = {"bf16": 0, "f32": 1, "silu": 2, "res": 3}


def _sk_workspace(device) -> tuple:
    dev = torch.device(device)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    got = _sk_ws.get(key)
    if got is None:
        ncu = num_cus(dev)
        e = ext()
        ws = torch.empty(e.gemm_sk_ws_bytes(ncu) // 4, device=dev, dtype=torch.float32)
        tk = torch.zeros(e.gemm_sk_tickets(ncu), device=dev, dtype=torch.int32)
        got = _sk_ws[key] = (ws, tk, ncu)
    return got


# stream-K tile configurations (gemm_tile256.hip kSkCfgs, same order; + 8 = whole tiles only):
# (BM, BN, BK, waves per workgroup; 4 = two workgroups per CU)
SK_CFGS = ((256, 256, 64, 8), (256, 192, 64, 8), (256, 128, 64, 8), (128, 256, 64, 8), (128, 192, 64, 8),
           (128, 128, 64, 8), (128, 192, 64, 4), (128, 128, 64, 4))


def sk_cfg_pairs(cfg: int) -> bool:
    """Whether a configuration's waves hold an even n-block count (the SiLU epilogue pairs gate / up n-blocks)."""
    _, bn, _, nw = SK_CFGS[cfg & 7]
    return (bn // 16 // (nw // 2)) % 2 == 0


def sk_cfg_tag(cfg: int) -> str:
    """Name of a stream-K configuration code (bench arms, the tuning table): e.g. 128x192, 128x192w4dp."""
    bm, bn, bk, nw = SK_CFGS[cfg & 7]
    return f"{bm}x{bn}" + ("k128" if bk == 128 else "") + ("w4" if nw == 4 else "") + ("dp" if cfg & 8 else "")


_SK_TUNING_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_sk_tuning.json")
_sk_tuning: Optional[dict] = None
_SK_BUCKETS = (128, 256, 300, 512, 1024, 2048, 4096)


def sk_config(M: int, N: int, K: int, epi: str) -> int:
    """Tile configuration for a prefill GEMM: the measured table (scripts/bench_prefill_gemm.py --grid ->
    scripts/make_sk_tuning.py -> gemm_sk_tuning.json; the nearest measured M in log scale), else -1 (the kernel's
    tile-shape cost model)."""
    global _sk_tuning
    if _sk_tuning is None:
        try:
            with open(_SK_TUNING_PATH) as f:
                _sk_tuning = json.load(f)
        except (OSError, ValueError):
            _sk_tuning = {}
    b = min(_SK_BUCKETS, key=lambda c: abs(math.log2(c) - math.log2(max(M, 1))))
    e = _sk_tuning.get(f"{N}x{K}:{'res' if epi in ('res', 'f32') else epi}:m{b}")
    return int(e["cfg"]) if e is not None else -1


def gemm_sk(x: torch.Tensor, wf: torch.Tensor, N: int, out: torch.Tensor, epi: str,
            min_share: Optional[int] = None, cfg: Optional[int] = None, rows: Optional[int] = None,
            xf_out: bool = False) -> torch.Tensor:
    """out (epi 'bf16' / 'f32' / 'silu') or h (epi 'res': h[:M] += x @ W^T) from the stream-K prefill GEMM over the
    fragment-layout bf16 weight ``wf``.  cfg: None = the measured table (``sk_config``), -1 = the kernel's
    tile-shape cost model, else an SK_CFGS index (+ 8: whole tiles only).  rows: x is a flat buffer in the
    fragment-major layout (``to_xfrag``) of that many rows; xf_out: the SiLU output is written in it."""
    M, K = (rows, wf.numel() // N) if rows is not None else x.shape
    if cfg is None:
        cfg = sk_config(M, N, K, epi)
    ws, tk, ncu = _sk_workspace(x.device)
    ext().gemm_sk(x, wf, N, out, _SK_EPI[epi], ws, tk, ncu, SK_MIN_SHARE if min_share is None else min_share, cfg,
                  (1 if rows is not None else 0) + (2 if xf_out else 0), rows or 0)
    return out


def linear_sk(x: torch.Tensor, w: PackedWeight, epi: str, out: torch.Tensor, rows: Optional[int] = None,
              xf_out: bool = False) -> torch.Tensor:
    """Prefill projection (M > 64) on the stream-K kernel into ``out`` (epi 'bf16' | 'silu'), with fragment-major
    activations: rows = x is a flat ``to_xfrag`` buffer of that many rows; xf_out = the SiLU output is written in
    that layout too (flat, >= xfrag_tiles(rows) * 16 * N / 2), the down projection's input."""
    M = rows if rows is not None else x.shape[0]
    if not _gpu(x):
        y = ref.linear(from_xfrag(x, M, w.K) if rows is not None else x, w.dense(), epi)
        f = to_xfrag(y) if xf_out else y
        out.view(-1)[: f.numel()].copy_(f.reshape(-1))
        return out
    wf = w.data if w.kind == "bf16" else _dequant_scratch(w, x.device)
    return gemm_sk(x, wf, w.N, out, epi, rows=rows, xf_out=xf_out)


def linear_res(x: torch.Tensor, w: PackedWeight, h: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
    """h[:M] += x @ W^T in f32 (prefill o / down, M > 64, TP = 1): the residual add rides in the GEMM epilogue, so the
    norm after it reads h alone.  bf16 weights, or quantised ones through their bf16 dequantisation scratch; W8A8
    fp8 prefill keeps its slab path (``res_supported``).  rows: x is fragment-major (``to_xfrag``) with that many."""
    M = rows if rows is not None else x.shape[0]
    if not _gpu(x):
        xr = from_xfrag(x, M, w.K) if rows is not None else x
        h[:M] += ref.linear(xr, w.dense(), "f32")
        return h
    wf = w.data if w.kind == "bf16" else _dequant_scratch(w, x.device)
    return gemm_sk(x, wf, w.N, h, "res", rows=rows)


def linear_rope(x: torch.Tensor, w: PackedWeight, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc,
                H: int, Hkv: int, rows: Optional[int] = None) -> None:
    """The prefill qkv projection with RoPE and the paged bf16 KV-cache append fused into the GEMM epilogue (M > 64,
    bf16 cache): q_out [T, H, 128] = rotated q, the cache gets rotated k and v at each token's slot.  CPU: the
    unfused reference (bf16 qkv, then ``rope_append``).  rows: x is fragment-major (``to_xfrag``) with that many."""
    M = rows if rows is not None else x.shape[0]
    if not _gpu(x):
        qkv = linear(from_xfrag(x, M, w.K) if rows is not None else x, w, "bf16")
        return ref.rope_append(qkv, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv)
    wf = w.data if w.kind == "bf16" else _dequant_scratch(w, x.device)
    ws, tk, ncu = _sk_workspace(x.device)
    ext().gemm_sk_rope(x, wf, ws, tk, ncu, SK_MIN_SHARE, rope_config(M, w.N, w.K), pos, tok_seq,
                       block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv, 1 if rows is not None else 0, rows or 0)


def rope_config(M: int, N: int, K: int) -> int:
    """Tile configuration of the RoPE-epilogue qkv GEMM: the table's measured "rope" entry (scripts/rope_cfg_sweep.py,
    profiles/r5/rope_cfg_sweep_mi355x.jsonl: the bf16 entry's 192-column tile widened to 256 columns ran the 3B qkv at
    4096 rows in 185 us vs 147.5 us on 128 x 256), else the bf16 entry."""
    sk_config(M, N, K, "bf16")  # loads the table
    b = min(_SK_BUCKETS, key=lambda c: abs(math.log2(c) - math.log2(max(M, 1))))
    e = (_sk_tuning or {}).get(f"{N}x{K}:rope:m{b}")
    return int(e["cfg"]) if e is not None else sk_config(M, N, K, "bf16")


def rope_fusable(w: PackedWeight, kv_fp8: bool, M: int = 1 << 30) -> bool:
    """Whether the prefill qkv projection of M rows takes the fused RoPE / cache-append epilogue (``linear_rope``):
    bf16 cache, weights the stream-K kernel reads (bf16, or quantised ones through their bf16 dequantisation; the
    W8A8 fp8 prefill keeps its split-K path), and at least ROPE_FUSED_MIN_M rows."""
    return not kv_fp8 and res_supported(w) and ROPE_FUSED and M >= ROPE_FUSED_MIN_M


# The fused epilogue needs a whole-head (256-column) tile.  In the engine (rocprofv3 / scripts/ttft_ab.py,
# profiles/r5/ttft_ab_mi355x.jsonl, profiles/r5/rocprof_b32_gaps.txt) it wins where the qkv round trip it removes is
# large -- the 7B b32 bench prefill, 4096 rows: 361 us fused vs 320 + 65 (rope_append) -- and loses below, where the
# 192-column tile plus the separate launch is faster (3B 2k TTFT 14.41 vs 14.30 ms, 7B 300-token 11.29 vs 10.96 ms)
ROPE_FUSED = os.environ.get("LSA_ROPE_FUSED", "1") != "0"
ROPE_FUSED_MIN_M = int(os.environ.get("LSA_ROPE_FUSED_MIN_M", "4096"))


def res_supported(w: PackedWeight) -> bool:
    """Whether ``linear_res`` takes this weight (everything but W8A8 fp8 prefill, whose fp8 tile kernel writes
    split-K slabs)."""
    return RES_FUSED and not (w.kind == "fp8" and FP8_W8A8 and w.K % 128 == 0)


# prefill o / down: residual add in the GEMM epilogue (1) or an f32 GEMM output summed by the next add_rmsnorm (0)
RES_FUSED = os.environ.get("LSA_RES_FUSED", "1") != "0"
# TP = 1 prefill with every stream-K GEMM input in the fragment-major layout (engine.runner._prefill_layers): the
# producers (add_rmsnorm, the prefill attention, the gate_up SiLU epilogue) write it, the GEMM stages each MFMA
# fragment as one contiguous KiB instead of 16 half-lines
PREFILL_XF = os.environ.get("LSA_PREFILL_XF", "1") != "0"


def linear(x: torch.Tensor, w: PackedWeight, epi: str = "bf16", out: Optional[torch.Tensor] = None,
           splitk: Optional[int] = None, nb: Optional[int] = None, waves: Optional[int] = None,
           div: Optional[int] = None, rownorm=None, res=None, _xf: bool = False,
           wf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ W^T with a fused epilogue.  epi='f32' returns [splitk, M, N] partial slabs.
    rownorm / res (epi='res'): the decode epilogue extensions, see ``_epi_kw``.  wf: ``tile_weight(w, device)`` of a
    caller that runs several M > 64 products over one weight, so that a quantised weight is dequantised once."""
    M, K = x.shape
    assert K == w.K, (K, w.K)
    assert (epi == "res") == (res is not None), "epi='res' needs res=(h, xout, ss_out)"
    if not _gpu(x):
        if rownorm is not None:  # scale the rows before the product (the kernels scale the output rows)
            x = (x.float() * torch.rsqrt(ss_float(rownorm[0][:M]) / K + rownorm[1])[:, None]).to(x.dtype)
        if epi == "res":
            _epi_ref(ref.linear(x, w.dense(), "f32"), M, K, epi, rownorm, res, _xf)
            return res[0]
        y = ref.linear(x, w.dense(), epi)
        if epi == "f32":
            y = y.unsqueeze(0)
        if out is not None:
            out.view(-1)[: y.numel()].copy_(y.reshape(-1))
            return out
        return y
    if M > 64 and epi in ("bf16", "f32", "silu") and not (w.kind == "fp8" and FP8_W8A8 and K % 128 == 0):
        # prefill: the stream-K tile kernel (epi 'f32' returns one [1, M, N] slab whatever splitk asked for)
        assert rownorm is None and res is None, "epilogue extensions are decode-only (M <= 64)"
        if out is None:
            out = torch.empty(*((1, M, w.N) if epi == "f32" else (M, w.N // 2 if epi == "silu" else w.N)),
                              device=x.device, dtype=torch.float32 if epi == "f32" else torch.bfloat16)
        if wf is None:
            wf = w.data if w.kind == "bf16" else _dequant_scratch(w, x.device)
        return gemm_sk(x, wf, w.N, out, epi)
    nb0, sk0, wv0, dv0 = pick_gemm_config(M, w.N, K, epi, kind=w.kind)
    nb = nb0 if nb is None else nb
    if M > 64:  # prefill tile kernels: split-K (f32 slabs) only where the tile grid is small
        assert rownorm is None and res is None, "epilogue extensions are decode-only (M <= 64)"
        splitk = (tile_splitk(M, w.N, K, w.kind) if splitk is None else splitk) if epi == "f32" else 1
    splitk = sk0 if splitk is None else splitk
    waves = wv0 if waves is None else waves
    div = dv0 if div is None else div
    if epi == "res":
        splitk, out = _res_split(res, splitk, out, M, w.N, x.device)
    if out is None:
        if epi == "f32":
            out = torch.empty(splitk, M, w.N, device=x.device, dtype=torch.float32)
        else:
            out = torch.empty(M, w.N // 2 if epi == "silu" else w.N, device=x.device, dtype=torch.bfloat16)
    e = ext()
    kw = _epi_kw(rownorm, res, 0)
    if w.kind == "bf16":
        e.gemm(x, w.data, w.N, out, EPI[epi], nb, splitk, waves, div, **kw)
    elif w.kind == "fp8":
        if M <= 64:  # fp8 knobs: waves, and the tuning entry's "div" field is the chunk depth (1 | 2)
            e.fp8_gemm(x, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, _fp8_depth(div), **kw)
        else:  # W8A8 on the block-scaled fp8 MFMA: per-token activation scales, no weight dequantisation
            x8, sx = quantize_rows_fp8(x)
            e.fp8_gemm_t256(x8, sx, w.data, w.scale, w.N, out, EPI[epi], splitk)
    elif w.kind == "mxfp4":  # W4A16 decode GEMM, e2m1 -> bf16 in registers (v_cvt_scalef32_pk_bf16_fp4)
        e.fp4_gemm(x, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, **kw)
    elif w.kind == "q4_0":  # GGUF Q4_0 decode GEMM, codes -> bf16 in registers by the value rule (gemm_q4.hip)
        if res is not None:
            raise ValueError("q4_0 weights have no residual epilogue")
        e.q4_gemm(x, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, **kw)
    else:
        raise ValueError(f"weight kind {w.kind} on GPU")
    return out


FP8_W8A8 = os.environ.get("LSA_FP8_W8A8", "1") != "0"


def tile_weight(w: PackedWeight, device) -> Optional[torch.Tensor]:
    """The bf16 fragment-layout weight the stream-K route of ``linear`` (M > 64) multiplies by, for a caller that runs
    several such products over ``w`` back to back and passes it on as ``linear(..., wf=)``: the weight itself (bf16),
    one dequantisation into the stream's scratch (MXFP4, Q4_0; fp8 where the W8A8 tile kernel does not apply), or None where
    that route is not taken (CPU, W8A8 fp8).  Valid until the next dequantisation on the same stream."""
    if torch.device(device).type != "cuda" or (w.kind == "fp8" and FP8_W8A8 and w.K % 128 == 0):
        return None
    return w.data if w.kind == "bf16" else _dequant_scratch(w, device)


def _dequant_scratch(w: PackedWeight, device) -> torch.Tensor:
    """One layer's weight dequantised to the bf16 fragment layout in a scratch (prefill of quantised models: one
    pass over 0.5-1 byte per weight, then the bf16 tile GEMM).  One scratch per (device, HIP stream): co-served
    engines prefill on their own streams (client.py), and a scratch shared across streams would let one stream's
    dequant overwrite the weights another stream's GEMM is still reading.  A regrown scratch is freed on the same
    stream that used it, so the caching allocator orders its reuse behind that stream's pending kernels."""
    key = (torch.device(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _dq_scratch.get(key)
    if buf is None or buf.numel() < w.N * w.K:
        buf = torch.empty(w.N * w.K, device=device, dtype=torch.bfloat16)
        _dq_scratch[key] = buf
    if w.kind == "mxfp4":
        ext().fp4_dequant(w.data, w.scale, w.N, w.K, buf)
    elif w.kind == "q4_0":
        ext().q4_dequant(w.data, w.scale, w.N, w.K, buf)
    else:
        ext().fp8_dequant(w.data, w.scale, w.N, w.K, buf)
    return buf[: w.N * w.K]


def quantize_rows_fp8(x: torch.Tensor):
    """Per-token fp8: (x8 [M, K] uint8 e4m3fn bits, sx [M] f32) with x ~= e4m3(x / sx) * sx, sx = amax / 448."""
    M, K = x.shape
    if not _gpu(x):
        xf = x.float()
        sx = (xf.abs().amax(1) / 448.0).clamp(min=1e-30)
        sx = torch.where(xf.abs().amax(1) > 0, sx, torch.ones_like(sx))
        q = (xf / sx[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
        return q.view(torch.uint8), sx
    x8 = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    sx = torch.empty(M, device=x.device, dtype=torch.float32)
    ext().quant_rows_fp8(x, x8, sx)
    return x8, sx


def fp8_tile_splitk(M: int, N: int, K: int) -> int:
    """Split-K of a W8A8 prefill GEMM (f32 slab epilogue) on the 256^2 fp8 tile kernel: doubled until the
    grid has >= 256 workgroups, at most 8 slabs and >= 4 K-tiles (512 of K) per slab."""
    tiles = ((M + 255) // 256) * ((N // 16 + 15) // 16)
    if tiles >= 128:
        return 1
    sk = 1
    while tiles * sk < 256 and sk < 8 and (K // 128) // (sk * 2) >= 4:
        sk *= 2
    return sk


def tile_splitk(M: int, N: int, K: int, kind: str = "bf16") -> int:
    """Split-K (f32 slabs) of a prefill GEMM (M > 64): only the W8A8 fp8 tile kernel splits K (``fp8_tile_splitk``);
    every other prefill projection runs on the stream-K kernel, which balances the K ranges itself."""
    if kind == "fp8" and FP8_W8A8 and K % 128 == 0:
        return fp8_tile_splitk(M, N, K)
    return 1


_NUM_CUS: dict = {}


def num_cus(device) -> int:
    idx = torch.device(device).index or 0
    if idx not in _NUM_CUS:
        _NUM_CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _NUM_CUS[idx]


def xfrag_tiles(M: int) -> int:
    """Row tiles (16 rows each) of the fragment-major activation layout for M rows: decode (M <= 64) rounds up to
    1 | 2 | 4 tiles (the skinny kernels' MT), prefill (M > 64) to ceil(M / 16) (the stream-K GEMM's xf operands)."""
    return 1 if M <= 16 else (2 if M <= 32 else (4 if M <= 64 else (M + 15) // 16))


def to_xfrag(x: torch.Tensor) -> torch.Tensor:
    """[M, K] -> fragment-major activations Xf[K/32][MT][64 lanes][8] (lane = 16*((k%32)/8) + m%16,
    rows >= M zero): one MFMA B-fragment per (k-step, row tile) is 1 KiB lane-linear."""
    M, K = x.shape
    mt = xfrag_tiles(M)
    xp = torch.zeros(mt * 16, K, dtype=x.dtype, device=x.device)
    xp[:M] = x
    return xp.view(mt, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


def from_xfrag(xf: torch.Tensor, M: int, K: int) -> torch.Tensor:
    mt = xfrag_tiles(M)
    return xf[: mt * 16 * K].view(K // 32, mt, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(mt * 16, K)[:M]


def linear_xf(xf: torch.Tensor, M: int, w: PackedWeight, epi: str = "bf16", out: Optional[torch.Tensor] = None,
              splitk: Optional[int] = None, nb: Optional[int] = None, waves: Optional[int] = None,
              div: Optional[int] = None, rownorm=None, res=None, z12: bool = False) -> torch.Tensor:
    """``linear`` with the activations in the fragment-major layout (``to_xfrag``), M <= 64, bf16 or fp8 weights.
    epi='silu' writes its [M, N/2] output in the fragment-major layout too (the next GEMM's input);
    for that epilogue ``out`` is a flat buffer of at least xfrag_tiles(M) * 16 * N/2 elements.
    epi='res' writes its bf16 copy of the residual in the fragment-major layout.
    ``z12``: the caller allows the 12-bit weight stream (gemm_z12.hip) where the weight has one and 16 < M <= 32; same
    values, same summation order, fewer bytes.  A weight without it (not compressible) runs the bf16 kernel, as does
    a shape whose ':z12' tuning entry says "off" (measured slower) unless the call names its own ``nb``."""
    if not _gpu(xf) or w.kind not in ("bf16", "fp8", "mxfp4", "q4_0"):
        if epi != "silu":
            return linear(from_xfrag(xf, M, w.K), w, epi, out, splitk, nb, waves, div, rownorm, res, _xf=True)
        y = to_xfrag(linear(from_xfrag(xf, M, w.K), w, epi, None, splitk, nb, waves, div, rownorm))
        if out is None:
            return y
        out.view(-1)[: y.numel()].copy_(y)
        return out
    nb0, sk0, wv0, dv0 = pick_gemm_config(M, w.N, w.K, epi, xf=True, kind=w.kind)
    z12 = z12 and w.kind == "bf16" and w.z12 is not None and 16 < M <= 32 and epi in ("bf16", "f32", "silu")
    if z12:  # ':z12' entries: the bf16 pick's (splitk, waves, div) -- the summation order -- with their own nb
        e = _tuning_table().get(f"{w.N}x{w.K}:{epi}:b32:z12")
        if e is not None and e.get("off"):
            z12 = nb is not None
        elif e is not None:
            nb0, sk0, wv0, dv0 = e["nb"], e["splitk"], e["waves"], e["div"]
    nb = nb0 if nb is None else nb
    splitk = sk0 if splitk is None else splitk
    waves = wv0 if waves is None else waves
    div = dv0 if div is None else div
    z12 = z12 and nb in (2, 4, 6)
    if epi == "res":
        splitk, out = _res_split(res, splitk, out, M, w.N, xf.device)
    if out is None:
        if epi == "f32":
            out = torch.empty(splitk, M, w.N, device=xf.device, dtype=torch.float32)
        elif epi == "silu":  # whole 32-column k-steps of the fragment-major output
            out = torch.zeros(xfrag_tiles(M) * 16 * (-(-(w.N // 2) // 32) * 32), device=xf.device, dtype=torch.bfloat16)
        else:
            out = torch.empty(M, w.N, device=xf.device, dtype=torch.bfloat16)
    kw = _epi_kw(rownorm, res, xfrag_tiles(M))
    if z12:
        z = w.z12
        ext().z12_gemm_xf(xf, M, w.K, z.lo, z.hi, z.esc, z.base, w.N, out, EPI[epi], nb, splitk, waves, div, **kw)
    elif w.kind == "fp8":
        ext().fp8_gemm_xf(xf, M, w.K, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, _fp8_depth(div), **kw)
    elif w.kind == "mxfp4":
        ext().fp4_gemm_xf(xf, M, w.K, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, **kw)
    elif w.kind == "q4_0":
        if res is not None:
            raise ValueError("q4_0 weights have no residual epilogue")
        ext().q4_gemm_xf(xf, M, w.K, w.data, w.scale, w.N, out, EPI[epi], nb, splitk, waves, **kw)
    else:
        ext().gemm_xf(xf, M, w.K, w.data, w.N, out, EPI[epi], nb, splitk, waves, div, **kw)
    return out


# ----------------------------------------------------------------------------------- W8A8 decode
# LSA_FP8_A8=0 keeps the W8A16 decode GEMMs for the qkv / gate_up projections of fp8 models
FP8_A8_DECODE = os.environ.get("LSA_FP8_A8", "1") != "0"


def to_xf8(x8: torch.Tensor, mt: int) -> torch.Tensor:
    """uint8 [M, K] e4m3 bytes -> the flat xf8 layout X8[K/128][mt][64 lanes][32 B] of the W8A8 / W4A8 decode GEMM
    (csrc/kernels/gemm_fp8a.hip, common.h xf8_off; lane 16 g + r: row 16 t + r at k = 128 s + 16 g .. +15 and
    128 s + 64 + 16 g .. +15 -- the MFMA's own K order for an 8-bit operand), rows >= M zero."""
    M, K = x8.shape
    full = torch.zeros(16 * mt, K, dtype=torch.uint8, device=x8.device)
    full[:M] = x8
    v = full.view(mt, 16, K // 128, 2, 4, 16)  # t, r, s, h, g, e
    return v.permute(2, 0, 4, 1, 3, 5).contiguous().view(-1)  # s, t, g, r, h, e


def from_xf8(x8f: torch.Tensor, M: int, K: int) -> torch.Tensor:
    mt = xfrag_tiles(M)
    v = x8f.view(-1)[: mt * 16 * K].view(K // 128, mt, 4, 16, 2, 16)  # s, t, g, r, h, e
    return v.permute(1, 3, 0, 4, 2, 5).reshape(16 * mt, K)[:M]


def to_xs8(s: torch.Tensor, mt: int) -> torch.Tensor:
    """E8M0 bytes [M, K/32] (one per row and 32-column block) -> the block-scale layout S8[K/128][mt][64 lanes]
    (common.h xs8_off), rows >= M = 127 (2^0)."""
    M, nb32 = s.shape
    full = torch.full((16 * mt, nb32), 127, dtype=torch.uint8, device=s.device)
    full[:M] = s
    return full.view(mt, 16, nb32 // 4, 4).permute(2, 0, 3, 1).contiguous().view(-1)  # s, t, g, r


def from_xs8(s8: torch.Tensor, M: int, K: int) -> torch.Tensor:
    mt = xfrag_tiles(M)
    v = s8.view(-1)[: mt * 64 * (K // 128)].view(K // 128, mt, 4, 16)  # s, t, g, r
    return v.permute(1, 3, 0, 2).reshape(16 * mt, K // 32)[:M]


def e8m0_for_amax(amax: torch.Tensor) -> torch.Tensor:
    """E8M0 exponent (int32) of the smallest power of two s with amax / s <= 448, clamped to [1, 253] -- the host
    twin of common.h e8m0_for_amax (same f32 bit arithmetic)."""
    b = (amax.float() * (1.0 / 448.0)).contiguous().view(torch.int32)
    e = (b >> 23) + ((b & 0x7FFFFF) != 0).to(torch.int32)
    return e.clamp(1, 253)


def quantize_blocks_fp8(x: torch.Tensor, blk: int = 32):
    """[M, K] -> (e4m3 bytes [M, K] uint8, E8M0 bytes [M, K/32] uint8): one power-of-two scale per row and block of
    ``blk`` (32 | 128) consecutive columns (a 128-block's byte repeated for its four 32-blocks) -- what the decode
    attention (blk 128: per head) and the W8A8 SiLU epilogue (blk 32) write for the next W8A8 / W4A8 GEMM."""
    M, K = x.shape
    xf = x.float().view(M, K // blk, blk)
    e = e8m0_for_amax(xf.abs().amax(-1))
    inv = torch.exp2(127.0 - e.float())
    q = (xf * inv[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).view(M, K)
    return q, e.to(torch.uint8).repeat_interleave(blk // 32, dim=1)


def dequant_blocks_fp8(x8: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(e4m3 bytes [M, K], E8M0 [M, K/32]) -> f32 [M, K]."""
    M, K = x8.shape
    v = x8.view(torch.float8_e4m3fn).float().view(M, K // 32, 32)
    return (v * torch.exp2(s.float() - 127.0)[..., None]).view(M, K)


def quantize_xf8(x: torch.Tensor, mt: Optional[int] = None, out: Optional[torch.Tensor] = None,
                 sx: Optional[torch.Tensor] = None):
    """(x8 flat xf8 bytes, sx [M] f32): per-row e4m3 activations (scale amax / 448) for ``linear_a8``."""
    M, K = x.shape
    mt = mt or xfrag_tiles(M)
    if out is None:
        out = torch.zeros(mt * 16 * K, dtype=torch.uint8, device=x.device)
    if sx is None:
        sx = torch.empty(M, dtype=torch.float32, device=x.device)
    if not _gpu(x):
        q, s = quantize_rows_fp8(x)
        out.view(-1)[: mt * 16 * K].copy_(to_xf8(q, mt))
        sx[:M].copy_(s)
        return out, sx
    ext().quant_xf8(x, mt, out, sx)
    return out, sx


def quantize_xf8_blocks(x: torch.Tensor, blk: int = 32, mt: Optional[int] = None, out: Optional[torch.Tensor] = None,
                        s8: Optional[torch.Tensor] = None):
    """(x8 flat xf8 bytes, s8 flat block scales): block-scaled e4m3 activations (``quantize_blocks_fp8``) in the
    layouts ``linear_a8(..., s8=)`` reads."""
    M, K = x.shape
    mt = mt or xfrag_tiles(M)
    if out is None:
        out = torch.zeros(mt * 16 * K, dtype=torch.uint8, device=x.device)
    if s8 is None:
        s8 = torch.full((mt * 64 * (K // 128),), 127, dtype=torch.uint8, device=x.device)
    if not _gpu(x):
        q, s = quantize_blocks_fp8(x, blk)
        out.view(-1)[: mt * 16 * K].copy_(to_xf8(q, mt))
        s8.view(-1)[: mt * 64 * (K // 128)].copy_(to_xs8(s, mt))
        return out, s8
    ext().quant_xf8_blocks(x.contiguous(), mt, blk, out, s8)
    return out, s8


def xf8_dequant(x8: torch.Tensor, M: int, K: int, sx: Optional[torch.Tensor] = None,
                s8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The f32 [M, K] activations a W8A8 / W4A8 GEMM multiplies: xf8 bytes x per-row sx x per-block E8M0."""
    v = from_xf8(x8, M, K).view(torch.float8_e4m3fn).float()
    if s8 is not None:
        v = (v.view(M, K // 32, 32) * torch.exp2(from_xs8(s8, M, K).float() - 127.0)[..., None]).view(M, K)
    if sx is not None:
        v = v * sx[:M, None].float()
    return v


def linear_a8(x8: torch.Tensor, sx: Optional[torch.Tensor], M: int, w: PackedWeight, epi: str = "f32",
              out: Optional[torch.Tensor] = None, splitk: Optional[int] = None, nb: Optional[int] = None,
              waves: Optional[int] = None, div: Optional[int] = None, rownorm=None, xfo: bool = True,
              s8: Optional[torch.Tensor] = None, out_s8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W8A8 / W4A8 decode GEMM (M <= 64; fp8 or MXFP4 weights): out = (x8 . scales) @ w^T with the activations in
    the xf8 layout on the block-scaled fp8 MFMA.  Activation scales: per-row f32 ``sx`` (``quantize_xf8`` / the
    fp8 output of ``add_rmsnorm``) and / or per-block E8M0 ``s8`` (``quantize_xf8_blocks`` / the e4m3 outputs of
    ``attn_decode(out_s8=)`` and of this GEMM's SiLU epilogue).  epi 'f32' -> [splitk, M, N] slabs; 'silu' -> bf16
    [M, N/2] in the fragment-major layout (``xfo``) or row-major, or -- ``out_s8`` given -- e4m3 xf8 bytes in
    ``out`` with one E8M0 scale per (row, 32 columns) in ``out_s8`` (nb a multiple of 4)."""
    assert epi in ("f32", "silu")
    assert sx is not None or s8 is not None
    f8o = epi == "silu" and out_s8 is not None
    if not _gpu(x8):
        xd = xf8_dequant(x8, M, w.K, sx, s8)
        if rownorm is not None:
            xd = xd * torch.rsqrt(ss_float(rownorm[0][:M]) / w.K + rownorm[1])[:, None]
        y = xd @ w.dense().float().t()
        if epi == "f32":
            sk = splitk or 1
            o = out if out is not None else torch.empty(sk, M, w.N)
            o.view(-1)[: sk * M * w.N].zero_()
            o.view(sk, M, w.N)[0].copy_(y)
            return o
        F = w.N // 2
        y3 = y.view(M, F // 16, 2, 16)
        act = (torch.nn.functional.silu(y3[:, :, 0]) * y3[:, :, 1]).reshape(M, F)
        if f8o:
            q, s = quantize_blocks_fp8(act, 32)
            mt = xfrag_tiles(M)
            out.view(-1)[: mt * 16 * F].copy_(to_xf8(q, mt))
            out_s8.view(-1)[: mt * 64 * (F // 128)].copy_(to_xs8(s, mt))
            return out
        act = act.to(torch.bfloat16)
        act = to_xfrag(act) if xfo else act
        if out is None:
            return act
        out.view(-1)[: act.numel()].copy_(act.view(-1))
        return out
    assert w.kind in ("fp8", "mxfp4"), "linear_a8 runs fp8 / MXFP4 weights"
    kind = "fp8a" if w.kind == "fp8" else "fp4a"
    nb0, sk0, wv0, dv0 = pick_gemm_config(M, w.N, w.K, "silu8" if f8o else epi, xf=True, kind=kind)
    nb = nb0 if nb is None else nb
    splitk = sk0 if splitk is None else splitk
    waves = wv0 if waves is None else waves
    div = dv0 if div is None else div
    if out is None:
        if epi == "f32":
            out = torch.empty(splitk, M, w.N, device=x8.device, dtype=torch.float32)
        else:
            out = torch.zeros((xfrag_tiles(M) * 16 if xfo else M) * (w.N // 2), device=x8.device, dtype=torch.bfloat16)
    kw = _epi_kw(rownorm, None, 0)
    fp4 = w.kind == "mxfp4"
    ext().a8_gemm(x8, s8, sx, M, w.K, w.data, None if fp4 else w.scale, w.scale if fp4 else None, w.N, out, out_s8,
                  EPI[epi], nb, splitk, waves, _fp8_depth(div), 2 if f8o else (1 if xfo else 0), **kw)
    return out


def rr_config(N: int, K: int, epi: str, kind: str = "bf16") -> tuple[int, int, int, int]:
    """(nb, splitk, waves, div) of a batch-1 residual-reduce GEMM (``linear_rr`` / ``linear_a8_rr``): the measured
    "NxK:epi:b1:rr[:kind]" entry of the tuning table (scripts/sweep_rr_b1.py -- the prologue re-reads the residual
    slice once per workgroup, so the best n-block width differs from the plain kernel's), else the plain kernel's
    pick.  kind: 'bf16' or the weight kind ('fp8' / 'mxfp4': the W8A8 / W4A8 kernel)."""
    a8 = kind in ("fp8", "mxfp4")
    e = _tuning_table().get(f"{N}x{K}:{epi}:b1:rr" + (f":{kind}" if a8 else ""))
    if e is not None:
        return e["nb"], (1 if epi == "silu" else e["splitk"]), e["waves"], e["div"]
    if a8:
        ak = "fp8a" if kind == "fp8" else "fp4a"
        nb, sk, wv, dv = pick_gemm_config(1, N, K, "silu8" if epi == "silu" else epi, xf=True, kind=ak)
    else:
        nb, sk, wv, dv = pick_gemm_config(1, N, K, epi, kind=kind)
    return nb, (1 if epi == "silu" else sk), wv, dv


def linear_a8_rr(h: torch.Tensor, parts: torch.Tensor, h_out: torch.Tensor, w: PackedWeight, epi: str,
                 out: Optional[torch.Tensor] = None, out_s8: Optional[torch.Tensor] = None,
                 ss_out: Optional[torch.Tensor] = None, eps: float = 1e-5, splitk: Optional[int] = None,
                 nb: Optional[int] = None, waves: Optional[int] = None, div: Optional[int] = None) -> torch.Tensor:
    """Batch-1 W8A8 / W4A8 decode projection (fp8 or MXFP4 weights) with the residual add AND the activation
    quantisation in its prologue (gemm_fp8a.hip RR): x = h + sum_s parts[s] (h_out <- x), quantised to e4m3 with one
    E8M0 scale per 32 k -- no quantising norm launch before it.  The RMSNorm gamma is folded into W; the row scale
    r = rsqrt(mean(x^2) + eps) is applied
      * epi='silu' (gate_up): in the epilogue from the workgroup's own full-row sum; the output is the down
        projection's e4m3 input in the xf8 layout (``out``) with one E8M0 per 32 columns (``out_s8``);
      * epi='f32' (qkv): not here -- [splitk, 1, N] f32 slabs of W @ q(x), and sum x^2 goes to ss_out[0] (Q24) for
        the slab consumer (``attn_decode(rownorm=...)``)."""
    K = w.K
    assert epi in ("f32", "silu") and parts.dim() == 3 and parts.shape[1] == 1
    nb0, sk0, wv0, dv0 = rr_config(w.N, K, epi, w.kind)
    splitk = 1 if epi == "silu" else (sk0 if splitk is None else splitk)
    nb, waves, div = nb0 if nb is None else nb, wv0 if waves is None else waves, dv0 if div is None else div
    if not _gpu(h):
        x = ref.slab_sum(h.view(-1)[:K].float(), parts.reshape(parts.shape[0], -1)[:, :K])
        h_out.view(-1)[:K].copy_(x)
        q, s = quantize_blocks_fp8(x.view(1, K), 32)
        y = dequant_blocks_fp8(q, s) @ w.dense().float().t()
        if epi == "f32":
            ss_out.view(-1)[:1] += ss_q24(x.pow(2).sum().view(1))
            o = out if out is not None else torch.empty(splitk, 1, w.N)
            o.view(-1)[: splitk * w.N].zero_()
            o.view(splitk, 1, w.N)[0].copy_(y)
            return o
        y = y * torch.rsqrt(x.pow(2).sum() / K + eps)
        F = w.N // 2
        y3 = y.view(1, F // 16, 2, 16)
        act = (torch.nn.functional.silu(y3[:, :, 0]) * y3[:, :, 1]).reshape(1, F)
        qa, sa = quantize_blocks_fp8(act, 32)
        out.view(-1)[: 16 * F].copy_(to_xf8(qa, 1))
        out_s8.view(-1)[: 64 * (F // 128)].copy_(to_xs8(sa, 1))
        return out
    assert w.kind in ("fp8", "mxfp4"), "linear_a8_rr runs fp8 / MXFP4 weights"
    if out is None:
        assert epi == "f32"
        out = torch.empty(splitk, 1, w.N, device=h.device, dtype=torch.float32)
    fp4 = w.kind == "mxfp4"
    ext().a8_gemm_rr(h.view(-1)[:K], parts, h_out.view(-1), w.data, None if fp4 else w.scale, w.scale if fp4 else None,
                     w.N, out, out_s8, EPI[epi], nb, splitk, waves, _fp8_depth(div), ss_out=ss_out, eps=float(eps))
    return out


def rr_a8_supported(w: PackedWeight, K: int, splitk: int = 1) -> bool:
    """Whether a batch-1 W8A8 / W4A8 GEMM can take the residual-reduce prologue (``linear_a8_rr``): K slices that
    fit the kernel's LDS image (gemm_fp8a.hip A8_RR_KMAX)."""
    return w.kind in ("fp8", "mxfp4") and K % 128 == 0 and (K // 128 + splitk - 1) // splitk * 128 <= 8192


# ----------------------------------------------------------------------------------- norms / rope
def add_rmsnorm(h: torch.Tensor, w: torch.Tensor, eps: float, xn: torch.Tensor,
                parts: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
                emb: Optional[torch.Tensor] = None, row_idx: Optional[torch.Tensor] = None,
                write_h: bool = True, rows: Optional[int] = None, xf: bool = False,
                ss_out: Optional[torch.Tensor] = None, ss_ld: int = 0, ss_nzero: int = 0,
                x8: Optional[torch.Tensor] = None, sx8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """h[r] (= emb[ids[r]]) (+= sum parts[:, r]); xn[m] = rmsnorm(h[row_idx[m]]) * w.
    xf=True: xn is a flat buffer receiving the fragment-major layout (``to_xfrag``) of ``rows`` rows.
    ss_out (raw mode, the norm folded into the next GEMMs): xn = bf16(h) un-normalised, ss_out[m] = sum h^2,
    and ss_out[k * ss_ld + m] = 0 for k = 1..ss_nzero (the accumulators of the later residual epilogues).
    x8 / sx8: the same rows also as per-row-scaled e4m3 in the xf8 layout (``linear_a8`` input; quantised from
    the f32 values, before the bf16 rounding of xn)."""
    assert x8 is None or xf, "the fp8 output rides on the fragment-major (xf) decode layout"
    if x8 is not None and not _gpu(h):
        n = rows if rows is not None else xn.shape[0]
        hc = h.clone()  # the f32 rows, before the bf16 rounding of xn (raw mode: the un-normalised sums)
        y32 = ref.add_rmsnorm_f32(hc, w, eps, n, parts, ids, emb, row_idx, True)
        if ss_out is not None:
            y32 = hc[:n]
        add_rmsnorm(h, w, eps, xn, parts, ids, emb, row_idx, write_h, rows, xf, ss_out, ss_ld, ss_nzero)
        quantize_xf8(y32, xfrag_tiles(n), x8, sx8)
        return xn
    if rows is None:
        assert not xf, "xf output needs rows"
        rows = xn.shape[0]
    if ss_out is not None and not _gpu(h):
        tmp = torch.empty(rows, w.numel(), dtype=torch.bfloat16, device=h.device)
        ref.add_rmsnorm(h, torch.ones_like(w), eps, tmp, parts, ids, emb, row_idx, write_h)
        hv = h[:rows].float()
        raw = hv.to(torch.bfloat16)
        if xf:
            f = to_xfrag(raw)
            xn.view(-1)[: f.numel()].copy_(f)
        else:
            xn[:rows].copy_(raw)
        ss_out[:rows] = ss_q24(hv.pow(2).sum(1))
        for k in range(1, ss_nzero + 1):
            ss_out[k * ss_ld: k * ss_ld + rows] = 0
        return xn
    if not _gpu(h):
        if not xf:
            return ref.add_rmsnorm(h, w, eps, xn, parts, ids, emb, row_idx, write_h)
        tmp = torch.empty(rows, w.numel(), dtype=torch.bfloat16, device=h.device)
        ref.add_rmsnorm(h, w, eps, tmp, parts, ids, emb, row_idx, write_h)
        f = to_xfrag(tmp)
        xn.view(-1)[: f.numel()].copy_(f)
        return xn
    nparts = parts.shape[0] if parts is not None else 0
    stride = parts.stride(0) if parts is not None else 0
    ext().add_rmsnorm(h, parts, nparts, stride, ids, emb, row_idx, write_h, w, eps, xn, rows,
                      xfrag_tiles(rows) if (xf or x8 is not None) else 0, ss_out, ss_ld, ss_nzero, x8, sx8)
    return xn


def prefetch(tensors, nbytes=None, wgs: int = 512) -> None:
    """Infinity-Cache warm-up: stream (the first ``nbytes[k]`` bytes of) up to four tensors through the memory
    hierarchy with allocating loads and no stores, so the next kernel reading them hits the 256 MiB die-level cache.
    Issued on a side stream of the captured decode step (``ModelRunner.prefetch_plan``).  No-op off the GPU."""
    tensors = [t for t in tensors if t is not None]
    if not tensors or not _gpu(tensors[0]):
        return
    nb = list(nbytes) if nbytes is not None else [-1] * len(tensors)
    ext().prefetch(tensors, [int(b) for b in nb], int(wgs))


def rr_supported(w: PackedWeight, K: int, splitk: int = 1) -> bool:
    """Whether a batch-1 decode GEMM can take the residual-reduce prologue (``linear_rr``): bf16 weights and a K slice
    per split that fits the kernel's LDS image (gemm.hip RR_KMAX)."""
    return w.kind in ("bf16", "dense") and K % 32 == 0 and (K // 32 + splitk - 1) // splitk * 32 <= 8192


def linear_rr(h: torch.Tensor, parts: torch.Tensor, h_out: torch.Tensor, w: PackedWeight, epi: str,
              out: Optional[torch.Tensor] = None, ss_out: Optional[torch.Tensor] = None, eps: float = 1e-5,
              splitk: Optional[int] = None, nb: Optional[int] = None, waves: Optional[int] = None,
              div: Optional[int] = None) -> torch.Tensor:
    """Batch-1 decode projection with the residual add folded into its prologue (gemm.hip RR; lsa_epi.h LsaRr).

    x = h + sum_s parts[s] (h: f32 [1, K] residual stream, parts: f32 [S, 1, K] split-K slabs of the previous
    row-parallel projection); h_out <- x (the next residual stream, a different buffer than h).  The RMSNorm gamma is
    folded into W (``norms_folded``); the RMS row scale r = rsqrt(mean(x^2) + eps) is applied
      * epi='silu': in the epilogue (splitk 1; each workgroup reduces the whole row itself) -> bf16 [1, N/2];
      * epi='f32': NOT here -- the output is [splitk, 1, N] f32 slabs of W @ bf16(x), and sum x^2 is added to
        ss_out[0] (Q24 int64, must be zero on entry) for the slab consumer (``attn_decode(rownorm=...)``).
    Replaces the ``res_add_ss`` launch between the two projections (one kernel boundary less per layer side)."""
    K = w.K
    assert epi in ("f32", "silu") and h.numel() >= K and parts.dim() == 3 and parts.shape[1] == 1
    nb0, sk0, wv0, dv0 = rr_config(w.N, K, epi, w.kind)
    splitk = 1 if epi == "silu" else (sk0 if splitk is None else splitk)
    nb = nb0 if nb is None else nb
    if not _gpu(h):
        x = ref.slab_sum(h.view(-1)[:K].float(), parts.reshape(parts.shape[0], -1)[:, :K])
        h_out.view(-1)[:K].copy_(x)
        xb = x.to(torch.bfloat16).view(1, K)
        if epi == "silu":
            r = torch.rsqrt(x.pow(2).sum() / K + eps)
            y = ref.linear(xb, w.dense(), "f32") * r
            g, u = y.view(-1, 2, 16)[:, 0].reshape(1, -1), y.view(-1, 2, 16)[:, 1].reshape(1, -1)
            res = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
            if out is None:
                return res
            out.view(-1)[: res.numel()].copy_(res.view(-1))
            return out
        assert ss_out is not None
        ss_out.view(-1)[:1] += ss_q24(x.pow(2).sum().view(1))
        y = ref.linear(xb, w.dense(), "f32").unsqueeze(0)
        if out is None:
            return y
        out.view(-1)[: y.numel()].copy_(y.reshape(-1))
        return out
    waves = wv0 if waves is None else waves
    div = dv0 if div is None else div
    if out is None:
        out = (torch.empty(splitk, 1, w.N, device=h.device, dtype=torch.float32) if epi == "f32" else
               torch.empty(1, w.N // 2, device=h.device, dtype=torch.bfloat16))
    ext().gemm_rr(h.view(-1)[:K], parts, h_out.view(-1), w.data, w.N, out, EPI[epi], nb, splitk, waves, div,
                  ss_out=ss_out, eps=float(eps))
    return out


def res_add_ss(h: torch.Tensor, parts: Optional[torch.Tensor], xn: torch.Tensor, rows: int, ss_out: torch.Tensor,
               xf: bool = False) -> torch.Tensor:
    """Residual add of the folded-norm decode step (the RMSNorm gammas live in the next GEMM's weight, which scales
    its output rows by rsqrt(ss / d + eps), ``linear(..., rownorm=(ss_out, eps))``):
    h[:rows] += sum_s parts[s];  xn = bf16(h) (fragment-major when xf);  ss_out[:rows] += sum h^2 (Q24 int64).
    ss_out must be zero on entry.  One wave per 512-column slice on the GPU (norm_rope.hip res_add_ss_kernel)."""
    D = h.shape[1]
    if not _gpu(h):
        hv = h[:rows].float()
        if parts is not None:
            hv = ref.slab_sum(hv, parts[:, :rows])
        h[:rows].copy_(hv)
        x16 = hv.to(torch.bfloat16)
        if xf:
            f = to_xfrag(x16)
            xn.view(-1)[: f.numel()].copy_(f)
        else:
            xn[:rows].copy_(x16)
        ss_out[:rows] += ss_q24(hv.pow(2).sum(1))
        return xn
    nparts = parts.shape[0] if parts is not None else 0
    stride = parts.stride(0) if parts is not None else 0
    ext().res_add_ss(h, parts, nparts, stride, xn, rows, D, xfrag_tiles(rows) if xf else 0, ss_out)
    return xn


def rope_append(qkv, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv, kv_scales=None):
    """RoPE of q / k and the paged-cache append of k / v.  kv_scales = (ks, vs): fp8 cache (``KV_FP8``), kc / vc
    are uint8 e4m3 bytes and every (token, kv-head) row is stored with its own f32 scale."""
    if not _gpu(qkv):
        return ref.rope_append(qkv, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv, kv_scales)
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    ext().rope_append(qkv, pos, tok_seq, block_tables, cos_t, sin_t, q_out, kc, vc, H, Hkv, ks, vs)


def silu_parts(parts: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out [M, F] = silu(gate) * up from f32 split-K slabs [S, M, 2F] of the interleaved gate_up GEMM."""
    if not _gpu(parts):
        S, M, N = parts.shape
        y = ref.slab_sum(parts[0].float(), parts[1:]).view(M, N // 32, 2, 16)
        g, u = y[:, :, 0, :].reshape(M, N // 2), y[:, :, 1, :].reshape(M, N // 2)
        out.copy_((torch.nn.functional.silu(g) * u).to(out.dtype))
        return out
    ext().silu_parts(parts, out)
    return out


def silu_mul(g: torch.Tensor, u: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(g)
    if not _gpu(g):
        out.copy_((torch.nn.functional.silu(g.float()) * u.float()).to(out.dtype))
        return out
    ext().silu_mul(g, u, out)
    return out


# ----------------------------------------------------------------------------------- attention
# fp8 KV cache (LSA_KV_FP8=1 or ModelRunner(kv_dtype="fp8")): the paged cache holds e4m3 bytes with one f32 scale
# per (token, kv-head) row of 128 values (amax / 448) -- half the bytes of the memory-bound decode attention and
# twice the tokens per GiB of cache.  Decode attention reads the bytes directly; prefill widens the blocks it
# attends to into a bf16 scratch per layer (kv8_dequant).  Off by default: it is a lossy cache (relative error
# ~2^-4 per element), checked against the oracle's own fp8-cache emulation (models.llama.reference_forward kv_fp8).
KV_FP8 = os.environ.get("LSA_KV_FP8", "0") == "1"


def kv8_scratch(ctx: list[int], Hkv: int, device) -> tuple:
    """(ko, vo, table) for ``attn_prefill``'s fp8 path: compact bf16 scratch of every block the sequences with
    contexts ``ctx`` attend to (sequence i's block j at i * mb + j) and the matching [n, mb] block table."""
    mb = max(1, max((c + 63) // 64 for c in ctx))
    n = len(ctx)
    ko = torch.empty(n * mb, Hkv, 64, 128, dtype=torch.bfloat16, device=device)
    vo = torch.empty_like(ko)
    table = torch.arange(n * mb, dtype=torch.int32, device=device).view(n, mb)
    return ko, vo, table


# experiment overrides of the split-KV decode plan, {(B, Hkv): (chunk_blocks, nsplit, unsplit_max)} (in-engine A/Bs,
# scripts/ab_rr_cfg.py "plan:B:Hkv" keys); empty in production
DECODE_PLAN_OVERRIDES: dict = {}


def decode_split_plan(B: int, Hkv: int, max_ctx: int) -> tuple[int, int, int]:
    """(chunk_blocks, nsplit, unsplit_max) grid plan of split-KV decode for contexts up to max_ctx.  The
    kernel picks each sequence's own split from its length (csrc/kernels/attention.hip eff_split):
    <= unsplit_max blocks run unsplit, longer contexts are cut into nsplit pieces of at least chunk_blocks
    blocks, so a sequence shorter than max_ctx uses fewer, equally long splits.

    Measured on MI355X (scripts/bench_attn.py, profiles/attn_split_plans_mi355x.jsonl): the best grid is
    about 256 workgroups, i.e. one per CU of (sequence, kv-head) pairs x splits.  At >= 256 pairs (7B at
    batch >= 8, 3B at batch >= 32) every context runs unsplit (3B B=32 ctx 2048: 77.2 -> 46.4 us, 7B B=32
    ctx 512: 53.9 -> 44.6 us vs the earlier fixed 4-block chunks); 64 pairs -> 4 splits (3B B=8 ctx 2048:
    31.8 -> 16.8 us); 8 pairs (3B at batch 1) -> up to 32 splits of >= 2 blocks (17 at 2k context).
    Contexts of <= 4 blocks run unsplit (a combine costs more than it spreads), except on grids of <= 8
    pairs, where one block per split still wins (3B B=1 ctx 200: 8.65 -> 7.32 us)."""
    if (B, Hkv) in DECODE_PLAN_OVERRIDES:
        return tuple(DECODE_PLAN_OVERRIDES[(B, Hkv)])
    nblk = max(1, (max_ctx + 63) // 64)
    pairs = max(1, B * Hkv)
    if nblk <= 4:  # every sequence runs unsplit (eff_split): no empty split workgroups, no combine
        if pairs <= 8 and nblk > 1:
            return 1, nblk, 0
        return nblk, 1, 4
    nsplit = min(max(1, round(256 / pairs)), (nblk + 1) // 2, 256)
    if nsplit <= 1:
        return nblk, 1, 4
    return 2, nsplit, 4


def decode_workspace(B: int, H: int, Hkv: int, nsplit: int, device) -> tuple:
    """(opart, mlpart, counters) for split-KV decode: per-split partial outputs / (max, sum) pairs and the
    per-(sequence, kv-head) arrival tickets of the in-kernel combine (must start zeroed; the kernel
    leaves them zeroed)."""
    return (torch.empty(B * H * max(nsplit, 1) * 128, device=device, dtype=torch.float32),
            torch.empty(B * H * max(nsplit, 1) * 2, device=device, dtype=torch.float32),
            torch.zeros(B * Hkv, device=device, dtype=torch.int32))


def attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, out, workspace=None, plan=None, xf=False,
                qkv_parts=None, cos=None, sin=None, kv_scales=None, out_s8=None, rownorm=None):
    """q [B,H,128] vs paged cache, context = pos + 1.  workspace = decode_workspace(...) for split-KV.
    xf=True: out is a flat buffer receiving the fragment-major layout of the [B, H*128] output.
    qkv_parts ([S, B, (H+2Hkv)*128] f32 split-K slabs of the QKV projection) + cos/sin: RoPE and the
    KV-cache append of the new token are fused in (``q`` is then only a [B, H, 128] scratch buffer).
    kv_scales = (ks, vs): fp8 cache (see ``KV_FP8``).
    out_s8 (xf only): ``out`` is a uint8 buffer receiving the output as e4m3 in the xf8 layout with one E8M0 scale
    per (row, head) in ``out_s8`` -- the input of a W8A8 / W4A8 o projection (``linear_a8(s8=)``).
    rownorm = (ss, eps, hidden): the slabs are the projection of UN-normalised rows (``linear_rr``); row b's q / k / v
    are scaled by rsqrt(ss[b] / hidden + eps) (ss Q24 int64) before RoPE."""
    B = pos.shape[0]
    assert out_s8 is None or xf, "the e4m3 attention output lives in the xf8 layout"
    assert rownorm is None or qkv_parts is not None, "rownorm scales the fused-RoPE slabs"
    if not _gpu(pos):
        if rownorm is not None:
            r = torch.rsqrt(ss_float(rownorm[0][:B]) / rownorm[2] + rownorm[1])
            qkv_parts = qkv_parts[:, :B].sum(0, keepdim=True) * r.view(1, B, 1)
        if qkv_parts is not None:
            ref.rope_append(qkv_parts, pos, None, block_tables, cos, sin, q, kc, vc, H, Hkv, kv_scales)
        if out_s8 is not None:
            tmp = torch.empty(B, H, q.shape[-1], dtype=torch.bfloat16, device=q.device)
            ref.attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, tmp, kv_scales)
            quantize_xf8_blocks(tmp.view(B, -1), 128, xfrag_tiles(B), out, out_s8)
            return out
        if not xf:
            return ref.attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, out, kv_scales)
        tmp = torch.empty(B, H, q.shape[-1], dtype=torch.bfloat16, device=q.device)
        ref.attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, tmp, kv_scales)
        f = to_xfrag(tmp.view(B, -1))
        out.view(-1)[: f.numel()].copy_(f)
        return out
    plan = plan if plan is not None else decode_split_plan(B, Hkv, block_tables.shape[1] * 64)
    chunk, nsplit = plan[0], plan[1]
    unsplit_max = plan[2] if len(plan) > 2 else 4
    if workspace is None:
        workspace = decode_workspace(B, H, Hkv, nsplit, q.device)
    opart, mlpart, counters = workspace
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    ext().attn_decode(q, kc, vc, block_tables, pos, H, Hkv, scale, chunk, nsplit, out, opart, mlpart, counters,
                      xfrag_tiles(B) if xf else 0, qkv_parts, cos, sin, unsplit_max, ks, vs, out_s8=out_s8,
                      **({} if rownorm is None else dict(rowss=rownorm[0], eps=float(rownorm[1]),
                                                          hidden=int(rownorm[2]))))
    return out


# prefill attention kernel: "32" = 32 x 32 MFMA tiles, 128 query rows per workgroup (attention_prefill32.hip);
# "16" = the 16 x 16 kernel of attention.hip (64 rows per workgroup); "auto" = 32 when the longest packed
# sequence has >= 512 rows (measured, scripts/bench_attn_prefill.py: 7B 2k 146 -> 119 us, 3B 2k 118 -> 115 us,
# 8k 1051 -> 1021 us), else 16 (32 x 128-token prompts: 28 vs 31 us, twice the work items)
PREFILL_ATTN = "auto"


def _prefill_kernel(cu_q: list) -> str:
    if PREFILL_ATTN != "auto":
        return PREFILL_ATTN
    longest = max((cu_q[i + 1] - cu_q[i] for i in range(len(cu_q) - 1)), default=0)
    return "32" if longest >= 512 else "16"


def prefill_qblock(cu_q: Optional[list] = None) -> int:
    k = _prefill_kernel(cu_q or [0])
    return 128 if k == "32" else ext().prefill_qblock


def prefill_work(cu_q: list[int], qblock: Optional[int] = None, ctx: Optional[list[int]] = None,
                 kernel: Optional[str] = None, heads: int = 32) -> list:
    """Work items of the prefill attention kernel for packed sequences (cu_q offsets; ``ctx`` = per-sequence
    context length after this prefill, default = the chunk length, i.e. no cached prefix).

    16-row kernel: (seq, q_start) per workgroup, heaviest (latest) query blocks first.
    32-row kernel ('32'): NG items (seq, q_start, t0, t1) per workgroup -- the key tiles [t0, t1) = the whole causal
    range of a 128-row query block; NG = 2 pairs a heavy block with a light one (``_pair_blocks``).  (Cutting heavy
    blocks into KV-split pieces -- merged by a second launch, in LDS, or in the same launch through write-through
    partials -- was built three times and measured slower each time: profiles/attn_prefill_kv_split_mi355x.jsonl,
    profiles/attn_prefill_halves_mi355x.jsonl, profiles/r5/attn_prefill_kv_split_inlaunch_ab_mi355x.jsonl: a CU is
    throughput-bound on one busy group, so halving the longest chain only moves work between groups.)"""
    kernel = kernel or _prefill_kernel(cu_q)
    if qblock is None:
        qblock = 128 if kernel == "32" else ext().prefill_qblock
    items = []
    for s in range(len(cu_q) - 1):
        ql = cu_q[s + 1] - cu_q[s]
        pos0 = (ctx[s] - ql) if ctx is not None else 0
        for qs in range(0, ql, qblock):
            items.append(((pos0 + min(qs + qblock, ql) + 63) // 64, s, qs))
    items.sort(key=lambda t: -t[0])
    if kernel != "32":
        return [(s, qs) for _, s, qs in items]
    units = [(s, qs, 0, nt) for nt, s, qs in items]
    empty = (-1, 0, 0, 0)
    n = len(units)
    longest = max(cu_q[i + 1] - cu_q[i] for i in range(len(cu_q) - 1))
    if not _pair_blocks(n, heads, longest, qblock):
        return units
    out = []
    for i in range((n + 1) // 2):
        j = n - 1 - i
        b = units[j] if j > i else empty
        out.append(units[i] + b)
    return out


class PrefillPlan(NamedTuple):
    """Device-side plan of one prefill attention call (``prefill_plan``)."""
    kernel: str
    work: torch.Tensor  # int32 [n_workgroups, 2 | 4 * NG]


def prefill_plan(cu_q: list[int], ctx: Optional[list[int]] = None, heads: int = 32, device=None,
                 kernel: Optional[str] = None) -> PrefillPlan:
    """Work items of the prefill attention kernel for packed sequences, on ``device``."""
    kernel = kernel or _prefill_kernel(cu_q)
    rows = prefill_work(cu_q, ctx=ctx, kernel=kernel, heads=heads)
    w = torch.tensor(rows, dtype=torch.int32)
    if device is not None:
        w = w.to(device, non_blocking=True)
    return PrefillPlan(kernel, w)


# auto | 1 | 0 -- heavy/light paired query blocks in the 32-row prefill kernel
PREFILL_PAIR = "auto"


def _pair_blocks(n_items: int, heads: int, longest: int, qblock: int) -> bool:
    """Pair when every single block would be resident at once (<= 2 per CU on 256 CUs: the dispatch order
    then fixes which blocks share a CU, and heavy ones can land together) or for very long sequences; with
    more blocks than slots the hardware's dynamic dispatch balances them better (scripts/bench_attn_prefill.py,
    profiles/attn_prefill_pairing_mi355x.jsonl: 7B 2k 103 -> 89 us paired, 3B 2k 97 -> 84, 3B 8k 730 -> 695;
    4 x 1k 3B single 83 vs paired 90)."""
    if PREFILL_PAIR != "auto":
        return PREFILL_PAIR == "1"
    return n_items * heads <= 512 or longest >= 32 * qblock


def attn_prefill(q, kc, vc, block_tables, cu_q, ctx_lens, H, Hkv, scale, out, work=None, cu_list=None,
                 kv_scales=None, kv8_scratch_=None, xf: bool = False):
    """Causal prefill attention of packed sequences (cu_q offsets) over the paged cache.  ``work``: the
    ``prefill_plan`` of the same offsets (or None: planned here from ``cu_list`` / the device offsets).
    kv_scales = (ks, vs): fp8 cache -- the attended blocks are widened into ``kv8_scratch_`` (= kv8_scratch(ctx,
    ...), built from the host context list; made here when not given) and the bf16 kernels run on that.
    xf: ``out`` is a flat buffer receiving the fragment-major layout (``to_xfrag``) of the [T, H * 128] rows -- the
    o projection's stream-K input."""
    T = q.shape[0]
    if not _gpu(q):
        if not xf:
            return ref.attn_prefill(q, kc, vc, block_tables, cu_q, ctx_lens, H, Hkv, scale, out, kv_scales)
        tmp = ref.attn_prefill(q, kc, vc, block_tables, cu_q, ctx_lens, H, Hkv, scale, torch.empty_like(q), kv_scales)
        f = to_xfrag(tmp.reshape(T, -1))
        out.view(-1)[: f.numel()].copy_(f)
        return out
    if kv_scales is not None:
        ko, vo, table = kv8_scratch_ if kv8_scratch_ is not None else kv8_scratch(ctx_lens.tolist(), Hkv, q.device)
        ext().kv8_dequant(kc, vc, kv_scales[0], kv_scales[1], block_tables, ctx_lens, table.shape[1], ko, vo)
        kc, vc, block_tables = ko, vo, table
    cu = cu_list if cu_list is not None else cu_q.tolist()
    plan = work if isinstance(work, PrefillPlan) else None
    if plan is None:
        plan = (prefill_plan(cu, ctx=ctx_lens.tolist(), heads=H, device=q.device) if work is None
                else PrefillPlan(_prefill_kernel(cu), work))
    ext().attn_prefill(q, kc, vc, block_tables, cu_q, ctx_lens, plan.work, H, Hkv, scale, out,
                       1 if plan.kernel == "32" else 0, xfrag_tiles(T) if xf else 0)
    return out


# ----------------------------------------------------------------------------------- sampling
def _row_defaults(B, out_tokens, limit, eos_on):
    dev = out_tokens.device
    if limit is None:
        limit = torch.full((B,), out_tokens.shape[1], dtype=torch.int32, device=dev)
    if eos_on is None:
        eos_on = torch.ones(B, dtype=torch.int32, device=dev)
    return limit, eos_on


def argmax_commit(logits, out_tokens, gen_len, input_ids, positions, finished, eos, limit=None, eos_on=None,
                  part=None):
    """Greedy token + in-place decode-state update (see kernels/sampling.hip)."""
    B, V = logits.shape
    limit, eos_on = _row_defaults(B, out_tokens, limit, eos_on)
    if not _gpu(logits):
        return ref.argmax_commit(logits, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on)
    if part is None:
        part = torch.empty(B * ((V + 4095) // 4096), device=logits.device, dtype=torch.int64)
    ext().argmax_commit(logits, part, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on)


def sample_commit(logits, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len, input_ids,
                  positions, finished, eos, limit=None, eos_on=None, workspace=None, last_n=None, presence=None,
                  frequency=None, min_p=None):
    """Temperature / top-k / top-p / min-p draw (+ optional penalties) + decode-state update.

    ``hist`` [B, W] int32 is the ring of each row's last W context tokens (token at position p in column
    p % W, -1 = empty); with it, rows whose ``penalty`` != 1 have the logits of the distinct tokens among
    their last ``last_n`` (<= W, default W) positions penalised (Ollama ``repeat_penalty`` /
    ``repeat_last_n``), and the committed token is written into the ring.  ``logits`` is modified.

    ``presence`` / ``frequency`` / ``min_p``: optional f32 [B], None = off.  A token that occurs c times among those
    positions also loses c * frequency + presence (llama.cpp's ``penalties`` sampler, after the repetition penalty);
    a sampled row keeps, next to its best candidate, only the candidates of probability >= min_p times the best
    one's, on the temperature-scaled probabilities the nucleus rule reads.  Zeros are bit for bit the call without
    them (``ops.reference.repeat_penalty`` / ``sample_pick`` state the exact rules)."""
    B, V = logits.shape
    limit, eos_on = _row_defaults(B, out_tokens, limit, eos_on)
    if not _gpu(logits):
        return ref.sample_commit(logits, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len,
                                 input_ids, positions, finished, eos, limit, eos_on, last_n=last_n, presence=presence,
                                 frequency=frequency, min_p=min_p)
    if workspace is None:
        part = torch.empty(B * ((V + 4095) // 4096), device=logits.device, dtype=torch.int64)
        cand = torch.empty(B * ((V + 2047) // 2048) * 64, device=logits.device, dtype=torch.int64)
    else:
        part, cand = workspace
    ext().sample_commit(logits, part, cand, hist, penalty, last_n, temperature, top_k, top_p, seeds, out_tokens,
                        gen_len, input_ids, positions, finished, eos, limit, eos_on, presence, frequency, min_p)


# ----------------------------------------------------------------------------------- per-token logprobs
LOGPROB_KMAX = ref.LOGPROB_KMAX
LOGPROB_CHUNK = 2048
LOGPROB_CAND = 32


def logprob_workspace(B: int, V: int, device) -> tuple:
    """(lp_ms f32 [B * nch * 2], lp_cand int64 [B * nch * 32]), nch = ceil(V / 2048): what ``logprob_scan`` hands
    ``logprob_commit`` next to ``lp_raw``."""
    nch = (V + LOGPROB_CHUNK - 1) // LOGPROB_CHUNK
    return (torch.empty(B * nch * 2, device=device, dtype=torch.float32),
            torch.empty(B * nch * LOGPROB_CAND, device=device, dtype=torch.int64))


def _logprob_check(op: str, B: int, V: int, tensors: dict, lp_raw) -> None:
    """The refusals both ops make before any launch (the binding repeats them on the device path)."""
    if not (B >= 1 and 1 <= V <= ref.LOGPROB_VMAX):
        raise ValueError(f"{op}: V = {V} outside 1 .. {ref.LOGPROB_VMAX} (the sampler's bound)")
    for name, (t, dt) in tensors.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be a contiguous {dt} tensor")
    if lp_raw.dim() != 2 or lp_raw.shape[0] < B or lp_raw.shape[1] != V:
        raise ValueError(f"{op}: lp_raw must be [>= {B}, {V}]")


def logprob_scan(logits, lp_k, finished, gen_len, lp_raw, lp_n0, workspace=None):
    """First half of the per-token logprob record (kernels/logprobs.hip), right after the lm_head and ahead of the
    regex mask and the penalties: for every row that asked (``lp_k[b] >= 0``) and is not finished, the chunk partials
    of the raw row's log-sum-exp and its per-chunk best 32 go into ``workspace`` (``logprob_workspace``), the raw row
    into ``lp_raw[b]`` and ``gen_len[b]`` into ``lp_n0[b]``.  ``logits`` is only read."""
    if logits.dim() != 2:
        raise ValueError("logprob_scan: logits must be [B, V]")
    B, V = logits.shape
    i32, f32 = torch.int32, torch.float32
    _logprob_check("logprob_scan", B, V, {"logits": (logits, f32), "lp_k": (lp_k, i32), "finished": (finished, i32),
                                          "gen_len": (gen_len, i32), "lp_raw": (lp_raw, f32), "lp_n0": (lp_n0, i32)},
                   lp_raw)
    if not _gpu(logits):
        return ref.logprob_scan(logits, lp_k, finished, gen_len, lp_raw, lp_n0)
    if workspace is None:
        raise ValueError("logprob_scan: the device path needs the workspace logprob_commit will read")
    ext().logprob_scan(logits, lp_k, finished, gen_len, lp_raw, workspace[0], workspace[1], lp_n0)


def logprob_commit(lp_raw, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, B: int, workspace=None):
    """Second half, after the step's token commit: row b < B records ``lp_tok[b, n0]`` (the log-probability of
    ``out_tokens[b, n0]`` under the raw row's softmax) and its ``lp_k[b]`` most likely tokens into ``lp_ids / lp_top
    [b, n0, :K]`` exactly when it asked, this step's scan wrote ``lp_n0[b] = n0`` and the commit appended one token
    (``ops.reference.logprob_commit`` states the rule; ``logprob_rows`` the values)."""
    i32, f32 = torch.int32, torch.float32
    V = lp_raw.shape[1] if lp_raw.dim() == 2 else 0
    _logprob_check("logprob_commit", B, V, {"lp_raw": (lp_raw, f32), "lp_k": (lp_k, i32), "lp_n0": (lp_n0, i32),
                                            "gen_len": (gen_len, i32), "out_tokens": (out_tokens, i32),
                                            "lp_tok": (lp_tok, f32), "lp_ids": (lp_ids, i32), "lp_top": (lp_top, f32)},
                   lp_raw)
    if lp_ids.dim() != 3 or not 0 <= lp_ids.shape[2] <= LOGPROB_KMAX:
        raise ValueError(f"logprob_commit: top_logprobs K must be in 0 .. {LOGPROB_KMAX}")
    if (out_tokens.dim() != 2 or out_tokens.shape[0] < B or lp_tok.shape != out_tokens.shape
            or lp_ids.shape != lp_top.shape or tuple(lp_ids.shape[:2]) != tuple(out_tokens.shape)):
        raise ValueError("logprob_commit: record buffers must match out_tokens ([rows, max_new] / [rows, max_new, K])")
    if not _gpu(lp_raw):
        return ref.logprob_commit(lp_raw, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, B)
    if workspace is None:
        raise ValueError("logprob_commit: the device path needs logprob_scan's workspace")
    ext().logprob_commit(lp_raw, workspace[0], workspace[1], lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, B)


def prompt_logprob_workspace(R: int, V: int, device) -> tuple:
    """(ms f32 [R * nch * 2], cand int64 [R * nch * 32]), nch = ceil(V / 2048): what ``prompt_logprob_scan`` hands
    ``prompt_logprob_commit`` for up to R scored rows (the raw rows stay in ``logits``: no copy)."""
    return logprob_workspace(R, V, device)


def _prompt_logprob_check(op: str, logits, targets, row_k, extra: dict) -> tuple:
    """The refusals both prompt ops make before any launch (``_logprob_check``'s; the binding repeats them)."""
    if logits.dim() != 2:
        raise ValueError(f"{op}: logits must be [R, V]")
    R, V = logits.shape
    i32, f32 = torch.int32, torch.float32
    _logprob_check(op, R, V, dict({"logits": (logits, f32), "targets": (targets, i32), "row_k": (row_k, i32)}, **extra),
                   logits)
    if targets.dim() != 1 or row_k.dim() != 1 or targets.shape[0] != R or row_k.shape[0] != R:
        raise ValueError(f"{op}: targets / row_k must be [{R}]")
    return R, V


def _prompt_ws_check(op: str, R: int, V: int, workspace) -> None:
    nch = (V + LOGPROB_CHUNK - 1) // LOGPROB_CHUNK
    if (workspace is None or len(workspace) != 2 or workspace[0].dtype != torch.float32
            or workspace[1].dtype != torch.int64 or workspace[0].numel() < R * nch * 2
            or workspace[1].numel() < R * nch * LOGPROB_CAND):
        raise ValueError(f"{op}: the device path needs prompt_logprob_workspace of at least {R} rows")


def prompt_logprob_scan(logits, targets, row_k, workspace=None, any_k: bool = True):
    """First half of a prompt-token logprob record (kernels/logprobs.hip prompt_logprob_scan_kernel), right after the
    lm_head of R scored prefill rows: for every row with a target (``targets[r] >= 0``) the chunk partials of its
    log-sum-exp and -- ``any_k``: some ``row_k[r] > 0``, a launch-level switch the host decides -- its per-chunk best 32
    go into ``workspace`` (``prompt_logprob_workspace``).  ``logits`` is only read and must stay intact until
    ``prompt_logprob_commit`` has read it."""
    R, V = _prompt_logprob_check("prompt_logprob_scan", logits, targets, row_k, {})
    if not _gpu(logits):
        return ref.prompt_logprob_scan(logits, targets, row_k)
    _prompt_ws_check("prompt_logprob_scan", R, V, workspace)
    ext().prompt_logprob_scan(logits, targets, row_k, bool(any_k), workspace[0], workspace[1])


def prompt_logprob_commit(logits, targets, row_k, dst_tok, dst_ids, dst_top, workspace=None, any_k: bool = True):
    """Second half: row r with a target records ``dst_tok[r]`` (the log-probability of ``targets[r]`` under the row's
    softmax) and its K = min(row_k[r], dst_ids.shape[1]) most likely tokens into ``dst_ids / dst_top[r, :K]``
    (``ops.reference.prompt_logprob_commit`` states the rule, ``logprob_rows`` the values); rows without a target
    write nothing.  ``any_k`` must be what the scan was given: without it every row records with K = 0."""
    R, V = _prompt_logprob_check("prompt_logprob_commit", logits, targets, row_k,
                                 {"dst_tok": (dst_tok, torch.float32), "dst_ids": (dst_ids, torch.int32),
                                  "dst_top": (dst_top, torch.float32)})
    if dst_ids.dim() != 2 or not 0 <= dst_ids.shape[1] <= LOGPROB_KMAX:
        raise ValueError(f"prompt_logprob_commit: top_logprobs K must be in 0 .. {LOGPROB_KMAX}")
    if dst_tok.dim() != 1 or dst_tok.shape[0] != R or dst_ids.shape != dst_top.shape or dst_ids.shape[0] != R:
        raise ValueError("prompt_logprob_commit: record buffers must be [R] / [R, K]")
    if not _gpu(logits):
        if not any_k:
            row_k = torch.zeros_like(row_k)
        return ref.prompt_logprob_commit(logits, targets, row_k, dst_tok, dst_ids, dst_top)
    _prompt_ws_check("prompt_logprob_commit", R, V, workspace)
    ext().prompt_logprob_commit(logits, workspace[0], workspace[1], targets, row_k, bool(any_k), dst_tok, dst_ids,
                                dst_top)


LOGPROB_SPEC_ROWS = ref.LOGPROB_SPEC_ROWS


def spec_logprob_workspace(V: int, device) -> tuple:
    """(sp_raw f32 [32, V], ms f32 [32 * nch * 2], cand int64 [32 * nch * 32]): the raw rows and chunk partials of the
    S * T <= 32 rows of a verify step, between ``spec_logprob_scan`` and ``spec_logprob_commit`` (the per-slot
    ``lp_raw [max_slots, V]`` may have fewer rows than a verify step)."""
    R = LOGPROB_SPEC_ROWS
    return (torch.zeros(R, V, device=device, dtype=torch.float32),) + logprob_workspace(R, V, device)


def _spec_logprob_check(op: str, T: int, V: int, lp_k, tensors: dict, workspace) -> int:
    """The refusals of both verify-step ops before any launch: ``_logprob_check``'s, and T / S / S * T."""
    if lp_k.dim() != 1:
        raise ValueError(f"{op}: lp_k must be [S]")
    S = lp_k.shape[0]
    if not (isinstance(T, int) and 1 <= T <= 8 and 1 <= S <= 8 and S * T <= LOGPROB_SPEC_ROWS):
        raise ValueError(f"{op}: T = {T} and S = {S} must be in 1 .. 8 with S * T <= {LOGPROB_SPEC_ROWS}")
    if workspace is None or len(workspace) != 3:
        raise ValueError(f"{op}: needs spec_logprob_workspace (raw rows, ms, cand)")
    raw, ms, cand = workspace
    _logprob_check(op, LOGPROB_SPEC_ROWS, V, dict(tensors, sp_raw=(raw, torch.float32), ms=(ms, torch.float32),
                                                  cand=(cand, torch.int64)), raw)
    nch = (V + LOGPROB_CHUNK - 1) // LOGPROB_CHUNK
    if ms.numel() < LOGPROB_SPEC_ROWS * nch * 2 or cand.numel() < LOGPROB_SPEC_ROWS * nch * LOGPROB_CAND:
        raise ValueError(f"{op}: chunk workspaces too small for {LOGPROB_SPEC_ROWS} rows")
    for name, (t, _) in tensors.items():
        if name in ("lp_n0", "gen_len", "finished") and (t.dim() != 1 or t.shape[0] < S):
            raise ValueError(f"{op}: {name} must be [>= {S}]")
    return S


def spec_logprob_scan(logits, T: int, lp_k, finished, gen_len, lp_n0, workspace):
    """``logprob_scan`` of a verify step (kernels/logprobs.hip spec_logprob_scan_kernel), right after its lm_head and
    ahead of ``dfa_mask_verify`` and the verify commit: S = lp_k.shape[0] sequences of T rows, ``logits`` [S * T, V].
    The T raw rows of every sequence that asked and is not finished go into ``workspace`` (``spec_logprob_workspace``)
    and ``gen_len[s]`` into ``lp_n0[s]`` (-1 for a finished sequence that asked).  ``logits`` is only read."""
    if logits.dim() != 2:
        raise ValueError("spec_logprob_scan: logits must be [S * T, V]")
    i32, f32 = torch.int32, torch.float32
    S = _spec_logprob_check("spec_logprob_scan", T, logits.shape[1], lp_k,
                            {"logits": (logits, f32), "lp_k": (lp_k, i32), "finished": (finished, i32),
                             "gen_len": (gen_len, i32), "lp_n0": (lp_n0, i32)}, workspace)
    if logits.shape[0] != S * T:
        raise ValueError(f"spec_logprob_scan: logits must have S * T = {S * T} rows")
    if not _gpu(logits):
        return ref.spec_logprob_scan(logits, T, lp_k, finished, gen_len, lp_n0, workspace[0])
    ext().spec_logprob_scan(logits, T, lp_k, finished, gen_len, workspace[0], workspace[1], workspace[2], lp_n0)


def spec_logprob_commit(T: int, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, workspace):
    """``logprob_commit`` of a verify step, after its token commit (and ``dfa_spec_advance``): sequence s records the
    c = gen_len[s] - lp_n0[s] tokens the step committed, index n0 + t from verify row s T + t and
    ``out_tokens[s, n0 + t]``, straight into the per-slot records (``ops.reference.spec_logprob_commit`` states the
    rule).  ``lp_n0`` is only read."""
    i32, f32 = torch.int32, torch.float32
    raw = workspace[0] if workspace is not None and len(workspace) == 3 else None
    V = raw.shape[1] if raw is not None and raw.dim() == 2 else 0
    S = _spec_logprob_check("spec_logprob_commit", T, V, lp_k,
                            {"lp_k": (lp_k, i32), "lp_n0": (lp_n0, i32), "gen_len": (gen_len, i32),
                             "out_tokens": (out_tokens, i32), "lp_tok": (lp_tok, f32), "lp_ids": (lp_ids, i32),
                             "lp_top": (lp_top, f32)}, workspace)
    if lp_ids.dim() != 3 or not 0 <= lp_ids.shape[2] <= LOGPROB_KMAX:
        raise ValueError(f"spec_logprob_commit: top_logprobs K must be in 0 .. {LOGPROB_KMAX}")
    if (out_tokens.dim() != 2 or out_tokens.shape[0] < S or lp_tok.shape != out_tokens.shape
            or lp_ids.shape != lp_top.shape or tuple(lp_ids.shape[:2]) != tuple(out_tokens.shape)):
        raise ValueError("spec_logprob_commit: record buffers must match out_tokens ([rows, max_new] / "
                         "[rows, max_new, K])")
    if not _gpu(raw):
        return ref.spec_logprob_commit(T, lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids, lp_top, raw)
    ext().spec_logprob_commit(T, raw, workspace[1], workspace[2], lp_k, lp_n0, gen_len, out_tokens, lp_tok, lp_ids,
                              lp_top)


# ----------------------------------------------------------------------------------- speculative decoding
def verify_split_plan(Hkv: int, max_ctx: int, S: int = 1) -> tuple[int, int, int]:
    """(chunk_blocks, nsplit, unsplit_max) of ``attn_verify`` over S sequences for contexts (pos0 + T) up to max_ctx:
    the batch-S decode plan -- one workgroup per (sequence, kv head, split) either way."""
    return decode_split_plan(S, Hkv, max_ctx)


def verify_workspace(T: int, H: int, Hkv: int, nsplit: int, device, S: int = 1) -> tuple:
    """(opart, mlpart, counters) of ``attn_verify``: the split partials of S * T * H query rows and (at least) S * Hkv
    arrival tickets (start zeroed; the kernel leaves them zeroed)."""
    return decode_workspace(S * T, H, Hkv, nsplit, device)


def attn_verify(q, kc, vc, block_table, pos0, H, Hkv, scale, out, workspace=None, plan=None, kv_scales=None):
    """Speculative-decoding verify attention: q [T, H, 128] (rotated) are the T new tokens of ONE sequence whose block
    table row is ``block_table``, at positions pos0 .. pos0 + T - 1 (``pos0``: int32 tensor, read on the device); their
    K / V are already in the cache (``rope_append``): bf16, or -- ``kv_scales`` = (ks, vs) -- the fp8 cache's e4m3
    bytes with their per-(token, kv-head) scales.  Row t sees keys j <= pos0 + t.  out [T, H * 128] bf16.
    T <= 8 and T * H / Hkv <= 16.
    Several sequences in one launch: q [S, T, H, 128], block_table [S, max_blocks], pos0 [S], out [S * T, H * 128], with
    1 <= S <= 8 and S * T <= 32; every sequence computes exactly what its own one-sequence launch computes."""
    S, T = (q.shape[0], q.shape[1]) if q.dim() == 4 else (1, q.shape[0])
    if q.dim() not in (3, 4) or not 1 <= S <= 8 or S * T > 32:
        raise ValueError("attn_verify: q [T, H, 128] or [S, T, H, 128] with 1 <= S <= 8 and S * T <= 32")
    if q.dim() == 4 and (block_table.dim() != 2 or block_table.shape[0] != S or pos0.numel() < S):
        raise ValueError("attn_verify: q [S, T, H, 128] needs block_table [S, max_blocks] and pos0 [S]")
    if not _gpu(q):
        return ref.attn_verify(q, kc, vc, block_table, pos0, H, Hkv, scale, out, kv_scales)
    plan = plan if plan is not None else verify_split_plan(Hkv, block_table.numel() // S * 64, S)
    chunk, nsplit = plan[0], plan[1]
    unsplit_max = plan[2] if len(plan) > 2 else 4
    if workspace is None:
        workspace = verify_workspace(T, H, Hkv, nsplit, q.device, S)
    opart, mlpart, counters = workspace
    ks, vs = kv_scales if kv_scales is not None else (None, None)
    ext().attn_verify(q, kc, vc, block_table, pos0, H, Hkv, scale, chunk, nsplit, unsplit_max, out, opart, mlpart,
                      counters, ks, vs)
    return out


def kv_copy_blocks(kv: torch.Tensor, kv_scale: Optional[torch.Tensor], pairs) -> None:
    """Prefix cache: copy whole KV blocks inside the arena, ``pairs`` = host list of (src, dst) block ids
    (kernels/kv_copy.hip): for every layer, K and V, the [Hkv, 64, 128] tile of block src and its scale tile land in
    block dst.  kv [L, 2, NB, Hkv, 64, 128] bf16 or e4m3 bytes, kv_scale [L, 2, NB, Hkv, 64] f32 or None.  The ids
    are checked here, before anything is uploaded or launched: 0 < id < NB (block 0 is the idle rows' scratch),
    src != dst, no dst listed twice and no dst that is also a src (the copies of one launch run in no order)."""
    pairs = [(int(s), int(d)) for s, d in pairs]
    if not pairs:
        return
    if kv.dim() != 6:
        raise ValueError("kv must be the [L, 2, NB, Hkv, 64, 128] arena")
    NB = kv.shape[2]
    srcs, dsts = {s for s, _ in pairs}, [d for _, d in pairs]
    if any(not (0 < s < NB and 0 < d < NB) or s == d for s, d in pairs):
        raise ValueError(f"kv_copy_blocks: block ids must satisfy 0 < id < {NB} and src != dst: {pairs}")
    if len(set(dsts)) != len(dsts) or srcs & set(dsts):
        raise ValueError(f"kv_copy_blocks: a destination is listed twice or is also a source: {pairs}")
    if not _gpu(kv):
        return ref.kv_copy_blocks(kv, kv_scale, pairs)
    host = torch.tensor(pairs, dtype=torch.int32).pin_memory()  # the ids travel in one pinned transfer
    ext().kv_copy_blocks(kv, kv_scale, host.to(kv.device, non_blocking=True))


def _kv_shift_moves(name: str, kv: torch.Tensor, moves, cos: torch.Tensor, sin: torch.Tensor) -> list:
    """The checks ``kv_shift`` and ``kv_shift8`` share, on the tables and the move list of a 6-dimensional arena ``kv``
    (their docstrings state the rule); returns the moves as int tuples."""
    if cos.dim() != 2 or cos.shape[1] != 64 or cos.shape != sin.shape or cos.dtype != torch.float32 or \
            sin.dtype != torch.float32:
        raise ValueError(f"{name}: cos / sin must be f32 [rows, 64] tables")
    NB, rows = kv.shape[2], cos.shape[0]
    if any(len(m) != 5 for m in moves):
        raise ValueError(f"{name}: a move is (src, dst, row_lo, row_hi, delta)")
    if any(not (0 < s < NB and 0 < d < NB) for s, d, _, _, _ in moves):
        raise ValueError(f"{name}: block ids must satisfy 0 < id < {NB}: {moves}")
    if any(not 0 <= lo <= hi <= 64 for _, _, lo, hi, _ in moves):
        raise ValueError(f"{name}: rows must satisfy 0 <= row_lo <= row_hi <= 64: {moves}")
    if any(not 0 <= dl < rows for _, _, _, _, dl in moves):
        raise ValueError(f"{name}: delta must satisfy 0 <= delta < {rows}: {moves}")
    dsts: dict = {}
    for i, (_, d, lo, hi, _) in enumerate(moves):
        if hi > lo:
            dsts.setdefault(d, []).append((lo, hi, i))
    for rs in dsts.values():
        rs.sort()
        if any(a[1] > b[0] for a, b in zip(rs, rs[1:])):
            raise ValueError(f"{name}: two moves write overlapping rows of one block: {moves}")
    for i, (s, _, lo, hi, _) in enumerate(moves):
        if hi > lo and any(j != i and dlo < hi and lo < dhi for dlo, dhi, j in dsts.get(s, ())):
            raise ValueError(f"{name}: a move writes rows that another move reads: {moves}")
    return moves


def kv_shift(kv: torch.Tensor, kv_scale: Optional[torch.Tensor], moves, cos: torch.Tensor, sin: torch.Tensor) -> None:
    """Context shift: move KV rows between blocks of the arena and rotate the keys back (kernels/kv_shift.hip).
    ``moves`` = host list of (src, dst, row_lo, row_hi, delta): in every layer and KV head, for rows
    row_lo <= r < row_hi, K row r of block dst = K row r of block src rotated by -delta with the RoPE tables
    ``cos`` / ``sin`` [rows, 64] f32 (delta 0: a copy), and V row r of dst = V row r of src when src != dst (the V of
    an in-place move is not touched).  kv [L, 2, NB, Hkv, 64, 128] bf16; the fp8 cache (``kv_scale`` not None) is
    refused here -- ``kv_shift8`` takes it.  Everything is checked here, before anything is uploaded or launched:
    0 < id < NB, 0 <= row_lo <= row_hi <= 64, 0 <= delta < rows, no two moves with overlapping destination rows, and
    no move whose destination rows overlap the source rows of another move (the moves of one launch run in no order)."""
    moves = [tuple(int(v) for v in m) for m in moves]
    if kv.dim() != 6 or kv.dtype != torch.bfloat16:
        raise ValueError("kv_shift: kv must be the bf16 [L, 2, NB, Hkv, 64, 128] arena")
    if kv_scale is not None:
        raise ValueError("kv_shift: the fp8 KV cache is not supported")
    moves = _kv_shift_moves("kv_shift", kv, moves, cos, sin)
    if not moves:
        return
    if not _gpu(kv):
        return ref.kv_shift(kv, None, moves, cos, sin)
    host = torch.tensor(moves, dtype=torch.int32).pin_memory()  # the moves travel in one pinned transfer
    ext().kv_shift(kv, host.to(kv.device, non_blocking=True), cos, sin)


def kv_shift8(kv: torch.Tensor, kv_scale: torch.Tensor, moves, cos: torch.Tensor, sin: torch.Tensor) -> None:
    """``kv_shift`` on the fp8 cache (kv_shift8_kernel in kernels/kv_shift.hip): kv [L, 2, NB, Hkv, 64, 128] uint8, the
    e4m3 bytes of every (block, head) tile in token-pair order (``reference.kv8_physical``), and kv_scale
    [L, 2, NB, Hkv, 64] f32, the row scales in token order.  For rows row_lo <= r < row_hi of a move with delta > 0,
    K row r of src is dequantised (f32(byte) * scale), rotated by -delta as in ``kv_shift`` and quantised again by the
    append's rule (``reference.quant_kv_rows``: bytes e4m3(x * 448 / amax), new scale amax / 448 with amax the rotated
    row's max |x|; an all-zero row stays zeros with scale 0) into row r of dst.  V rows and delta-0 K rows are copied
    with their scales, bit for bit, when src != dst and not touched when src == dst.  The move list is checked as in
    ``kv_shift``; everything is refused before anything is uploaded or launched."""
    moves = [tuple(int(v) for v in m) for m in moves]
    if kv.dim() != 6 or kv.dtype != torch.uint8:
        raise ValueError("kv_shift8: kv must be the uint8 (e4m3) [L, 2, NB, Hkv, 64, 128] arena")
    if not isinstance(kv_scale, torch.Tensor) or kv_scale.dtype != torch.float32 or \
            tuple(kv_scale.shape) != tuple(kv.shape[:5]):
        raise ValueError("kv_shift8: kv_scale must be the f32 [L, 2, NB, Hkv, 64] row scales of kv")
    moves = _kv_shift_moves("kv_shift8", kv, moves, cos, sin)
    if not moves:
        return
    if not _gpu(kv):
        return ref.kv_shift8(kv, kv_scale, moves, cos, sin)
    host = torch.tensor(moves, dtype=torch.int32).pin_memory()  # the moves travel in one pinned transfer
    ext().kv_shift8(kv, kv_scale, host.to(kv.device, non_blocking=True), cos, sin)


# ----------------------------------------------------------------------------------- embeddings
EMBED_MODES = {"mean": ref.EMBED_MEAN, "last": ref.EMBED_LAST}


def _embed_host(name: str, cu, meta, host):
    """(cu, meta) as host lists: ``host`` when the caller has them (the runner: no device read), else read from the
    tensors (a synchronising read on the GPU; tests)."""
    if host is not None:
        cu_h, meta_h = host
    else:
        cu_h, meta_h = (cu.tolist() if cu is not None else None), meta.tolist()
    if len(meta_h) != 5 or any(len(r) != len(meta_h[0]) for r in meta_h) or not len(meta_h[0]):
        raise ValueError(f"{name}: meta is [5, n]: emode, estart, eslot, efinal, ecount per sequence")
    return ([int(v) for v in cu_h] if cu_h is not None else None), [[int(v) for v in r] for r in meta_h]


def _embed_check(name: str, cu_h, meta_h, T: Optional[int], nslots: Optional[int]) -> None:
    """The value checks the three embedding ops share, made on the host before any launch: modes 0 / 1 / 2; for an
    embedding sequence estart >= 0, efinal 0 / 1, ecount >= 1, 0 <= eslot < slots and no slot named twice (a second
    workgroup would read what the first writes); cu non-decreasing from 0 to T."""
    n = len(meta_h[0])
    mode, start, slot, fin, count = meta_h
    if any(m not in (0, 1, 2) for m in mode):
        raise ValueError(f"{name}: emode must be 0 (none), 1 (mean) or 2 (last): {mode}")
    on = [i for i in range(n) if mode[i]]
    if any(start[i] < 0 or fin[i] not in (0, 1) or count[i] < 1 for i in on):
        raise ValueError(f"{name}: estart >= 0, efinal 0 / 1 and ecount >= 1: {meta_h}")
    if nslots is not None and any(not 0 <= slot[i] < nslots for i in on):
        raise ValueError(f"{name}: eslot must satisfy 0 <= slot < {nslots}: {slot}")
    if len({slot[i] for i in on}) != len(on):
        raise ValueError(f"{name}: two embedding sequences of one call name one slot: {slot}")
    if cu_h is not None and (len(cu_h) != n + 1 or cu_h[0] != 0 or cu_h[-1] != T or
                             any(a > b for a, b in zip(cu_h, cu_h[1:]))):
        raise ValueError(f"{name}: cu must be [n + 1], non-decreasing from 0 to T = {T}: {cu_h}")


def _embed_operands(name: str, h, parts, cu, meta, rs):
    if h.dim() != 2 or h.dtype != torch.float32 or h.shape[1] % 4 or not h.is_contiguous():
        raise ValueError(f"{name}: h must be a contiguous f32 [T, D] tensor with D % 4 == 0")
    if parts is not None:
        if parts.dim() == 2:
            parts = parts.unsqueeze(0)
        if parts.dtype != torch.float32 or parts.dim() != 3 or tuple(parts.shape[1:]) != tuple(h.shape):
            raise ValueError(f"{name}: parts must be f32 [np, T, D] slabs")
    if meta.dtype != torch.int32 or meta.dim() != 2 or meta.shape[0] != 5 or cu.dtype != torch.int32 or \
            cu.dim() != 1 or cu.numel() != meta.shape[1] + 1:
        raise ValueError(f"{name}: meta must be int32 [5, n] and cu int32 [n + 1]")
    if rs.dtype != torch.float32 or rs.dim() != 1 or rs.numel() < h.shape[0]:
        raise ValueError(f"{name}: rs must be an f32 vector of at least T = {h.shape[0]} entries")
    return parts


def embed_rowscale(h: torch.Tensor, parts: Optional[torch.Tensor], tseq: torch.Tensor, cu: torch.Tensor,
                   meta: torch.Tensor, eps: float, rs: torch.Tensor, host=None) -> None:
    """Embeddings, step 1 (kernels/embed.hip): rs[t] = rsqrt(sum(v_t^2) / D + eps) for every row the pool visits, with
    v_t = h[t] + parts[0][t] + ... left to right (the sum the final add_rmsnorm forms).  h [T, D] f32, parts None or
    f32 [np, T, D], tseq [T] / cu [n + 1] / meta [5, n] int32 on h's device (meta rows: emode 0 none / 1 mean / 2 last,
    estart, eslot, efinal, ecount).  ``host`` = (cu, meta) as host lists when the caller has them.  Everything is
    checked before any launch."""
    parts = _embed_operands("embed_rowscale", h, parts, cu, meta, rs)
    if tseq.dtype != torch.int32 or tseq.dim() != 1 or tseq.numel() != h.shape[0]:
        raise ValueError("embed_rowscale: tseq must be int32 [T]")
    cu_h, meta_h = _embed_host("embed_rowscale", cu, meta, host)
    _embed_check("embed_rowscale", cu_h, meta_h, h.shape[0], None)
    if not _gpu(h):
        return ref.embed_rowscale(h, parts, tseq, cu_h, meta_h, eps, rs)
    ext().embed_rowscale(h, parts, tseq, cu, meta, float(eps), rs)


def embed_pool(h: torch.Tensor, parts: Optional[torch.Tensor], cu: torch.Tensor, meta: torch.Tensor, rs: torch.Tensor,
               gamma: torch.Tensor, acc: torch.Tensor, host=None) -> None:
    """Embeddings, step 2: per embedding sequence a = +0 when estart == 0 else acc[eslot]; a = a + (v_t * rs[t]) * gamma
    over the sequence's rows of this call in position order (every product and sum a rounded f32); acc[eslot] = a.  A
    last-mode sequence stores the y of the last row of its efinal segment, and nothing from an earlier segment.  gamma
    [D] bf16 (the final norm), acc [slots, D] f32.  The same bits as ``reference.embed_pool`` for the same rs, and
    the same bits however the rows were split over calls."""
    parts = _embed_operands("embed_pool", h, parts, cu, meta, rs)
    if gamma.dtype != torch.bfloat16 or gamma.dim() != 1 or gamma.numel() != h.shape[1]:
        raise ValueError("embed_pool: gamma must be the bf16 [D] norm weights")
    if acc.dtype != torch.float32 or acc.dim() != 2 or acc.shape[1] != h.shape[1] or not acc.is_contiguous():
        raise ValueError("embed_pool: acc must be a contiguous f32 [slots, D] tensor")
    cu_h, meta_h = _embed_host("embed_pool", cu, meta, host)
    _embed_check("embed_pool", cu_h, meta_h, h.shape[0], acc.shape[0])
    if not _gpu(h):
        return ref.embed_pool(h, parts, cu_h, meta_h, rs, gamma, acc)
    ext().embed_pool(h, parts, cu, meta, rs, gamma, acc)


def embed_finish(meta: torch.Tensor, acc: torch.Tensor, out: torch.Tensor, host=None) -> None:
    """Embeddings, step 3, for the sequences with efinal: m = acc[eslot] / ecount (mean) or acc[eslot] (last);
    out[eslot] = m / sqrt(sum(m^2)), zeros when the sum is 0.  The sum runs in a fixed order
    (``reference.embed_finish`` reproduces its bits).  acc, out [slots, D] f32."""
    if meta.dtype != torch.int32 or meta.dim() != 2 or meta.shape[0] != 5:
        raise ValueError("embed_finish: meta must be int32 [5, n]")
    if acc.dtype != torch.float32 or out.dtype != torch.float32 or acc.dim() != 2 or acc.shape != out.shape or \
            not acc.is_contiguous() or not out.is_contiguous():
        raise ValueError("embed_finish: acc and out must be contiguous f32 [slots, D] tensors of one shape")
    _, meta_h = _embed_host("embed_finish", None, meta, (None, host[1]) if host is not None else None)
    _embed_check("embed_finish", None, meta_h, None, acc.shape[0])
    if not _gpu(acc):
        return ref.embed_finish(meta_h, acc, out)
    ext().embed_finish(meta, acc, out)


def spec_draft(prompt_tok, prompt_len, out_tokens, gen_len, input_ids, positions, k, spec_ids, spec_pos, spec_draft_out,
               n_max: int = 3, n_min: int = 1, forced=None):
    """Prompt-lookup drafter, one row per entry of ``prompt_len`` (kernels/spec.hip).  forced [nf, k] int32 replaces
    the search: the draft is its row min(gen_len, nf - 1); forced [rows, nf, k] plants table s in row s."""
    if forced is not None and forced.dim() == 3 and (forced.shape[0] < prompt_len.numel() or forced.shape[2] != k):
        raise ValueError("spec_draft: forced [rows, nf, k] needs one table per row")
    if not _gpu(prompt_tok):
        return ref.spec_draft(prompt_tok, prompt_len, out_tokens, gen_len, input_ids, positions, k, n_max, n_min,
                              forced, spec_ids, spec_pos, spec_draft_out)
    ext().spec_draft(prompt_tok, prompt_len, out_tokens, gen_len, input_ids, positions, k, n_max, n_min, forced,
                     spec_ids, spec_pos, spec_draft_out)


def spec_commit(logits, draft, stats, out_tokens, gen_len, input_ids, positions, finished, eos, limit=None,
                eos_on=None, part=None):
    """Greedy verification of the T = k + 1 verify rows ``logits`` of the sequence in state row 0 and the in-order
    commit of the accepted tokens (kernels/sampling.hip spec_commit_kernel); stats int64 [3] += (steps, drafted,
    accepted).  stats [S, 3]: ``logits`` [S * T, V] and ``draft`` [S, k] are the rows of S sequences (S * T <= 32),
    sequence s commits into state row s and counts in stats[s]."""
    T, V = logits.shape  # (all S * T rows)
    S = stats.shape[0] if stats.dim() == 2 else 1
    if T % S or T // S < 2 or (S > 1 and T > 32):
        raise ValueError("spec_commit: logits [S * T, V] with T >= 2 and S * T <= 32")
    limit, eos_on = _row_defaults(S, out_tokens, limit, eos_on)
    if not _gpu(logits):
        return ref.spec_commit(logits, draft, stats, out_tokens, gen_len, input_ids, positions, finished, eos, limit,
                               eos_on)
    if part is None:
        part = torch.empty(T * ((V + 4095) // 4096), device=logits.device, dtype=torch.int64)
    ext().spec_commit(logits, part, draft, stats, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on)


def spec_sample_commit(logits, draft, stats, hist, penalty, temperature, top_k, top_p, seeds, out_tokens, gen_len,
                       input_ids, positions, finished, eos, limit=None, eos_on=None, workspace=None, last_n=None,
                       presence=None, frequency=None, min_p=None):
    """Sampled verification of the T = k + 1 verify rows ``logits`` (2 <= T <= 8, V <= 262144) of the sequence in
    state row 0 (kernels/sampling.hip lsa_spec_sample_commit).  Row i is penalised over the ring ``hist`` [1, W] as it
    would stand had drafts 0 .. i-1 been committed (``logits`` is modified) and makes the draw of the plain
    ``sample_commit`` step for generated token gen_len[0] + i (temperature <= 0: the argmax); a draft is accepted
    exactly when it equals that draw, and the accepted run is committed in order, ring included, so the tokens are
    those of the plain sampled steps of the same seed.  The parameters are row 0's; stats int64 [3] += (steps, drafted,
    accepted).  ``workspace`` = (part, cand, picks): int64 [T * ceil(V / 4096)], int64 [T * ceil(V / 2048) * 64],
    int32 [T] (the rows' tokens).

    stats [S, 3]: ``logits`` [S * T, V] and ``draft`` [S, T - 1] are the rows of S sequences (S * T <= 32, as
    ``spec_commit``); sequence s reads ring row s and entry s of every parameter, commits into state row s and counts
    in stats[s]; the workspace is sized for S * T rows.  A sequence with temperature 0 and penalty 1 commits what
    ``spec_commit`` commits for its rows.

    ``presence`` / ``frequency`` / ``min_p``: the optional per-sequence f32 options of ``sample_commit`` (>= S entries,
    None = off); row i counts a token's occurrences in the window it is penalised over, drafts 0 .. i-1 included."""
    R, V = logits.shape  # (all S * T rows)
    S = stats.shape[0] if stats.dim() == 2 else 1
    if S > 1 and (stats.shape[1] != 3 or R % S or R > 32):
        raise RuntimeError("spec_sample_commit: stats [S, 3], logits [S * T, V] with S * T <= 32")
    T = R // S
    limit, eos_on = _row_defaults(S, out_tokens, limit, eos_on)
    if not _gpu(logits):
        if not 2 <= T <= 8 or V > 262144:  # as the binding and the launcher refuse them
            raise RuntimeError("spec_sample_commit: 2 <= T <= 8 verify rows, V <= 262144")
        if S > 1:  # as the binding: one ring row, one parameter and one state row per sequence
            per_seq = [temperature, top_k, top_p, seeds, gen_len, input_ids, positions, finished] + \
                [t for t in (penalty, last_n, presence, frequency, min_p) if t is not None]
            if any(t.numel() < S for t in per_seq) or draft.numel() < S * (T - 1) or out_tokens.shape[0] < S or \
                    (hist is not None and hist.shape[0] < S):
                raise RuntimeError("spec_sample_commit: one row of every per-sequence operand per sequence")
        return ref.spec_sample_commit(logits, draft, stats, hist, penalty, temperature, top_k, top_p, seeds,
                                      out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on,
                                      last_n=last_n, presence=presence, frequency=frequency, min_p=min_p)
    if workspace is None:
        workspace = (torch.empty(R * ((V + 4095) // 4096), device=logits.device, dtype=torch.int64),
                     torch.empty(R * ((V + 2047) // 2048) * 64, device=logits.device, dtype=torch.int64),
                     torch.empty(R, device=logits.device, dtype=torch.int32))
    part, cand, picks = workspace
    ext().spec_sample_commit(logits, draft, stats, hist, penalty, last_n, temperature, top_k, top_p, seeds, out_tokens,
                             gen_len, input_ids, positions, finished, eos, limit, eos_on, part, cand, picks, presence,
                             frequency, min_p)


# ----------------------------------------------------------------------------------- regex-constrained decoding
def dfa_mask(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len, input_ids,
             finished, eos, rows=None):
    """Regex-constrained decoding (kernels/guided.hip): every logit of ``logits`` [B, V] whose token would leave the
    row's byte DFA without a possible match becomes -inf, in place; the EOS ids stay exactly in an accepting state.
    The DFA state is advanced lazily from ``input_ids`` / ``gen_len`` into ``g_state`` (two slots per row), so the
    commit kernels run unchanged after it.  ``rows`` int32 [B] maps logits rows to table rows (default: identity).
    Operands and the exact rule: ``ops.reference.dfa_mask``."""
    if not _gpu(logits):
        return ref.dfa_mask(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len,
                            input_ids, finished, eos, rows)
    ext().dfa_mask(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, rows, gen_len,
                   input_ids, finished, eos)


def dfa_mask_verify(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len, input_ids,
                    finished, eos, draft, g_spec, r: int = 0):
    """The regex mask of a verify step (kernels/guided.hip dfa_mask_verify_kernel): ``logits`` [T, V] are the T = k + 1
    verify rows of the sequence in state row 0 (table row ``r``), ``draft`` [k] int32 what ``spec_draft`` wrote.  Row t
    is masked as ``dfa_mask`` masks a row whose state is the one after the input token and drafts 1..t (DEAD from the
    first draft that is -1, unknown, of 0 or > 32 bytes, or kills the walk).  ``g_spec`` int32 [1 + 8] receives gen_len
    and the T states for ``dfa_spec_advance``.  The exact rule: ``ops.reference.dfa_mask_verify``.

    A 2-D ``g_spec`` [S, 1 + 8] selects the form over S sequences (``spec_batch_guided``; as the 2-D ``stats`` of
    ``spec_commit``): ``logits`` [S * T, V], ``draft`` [>= S * k]; sequence s is the sequence of state row s and table
    row s (``r`` must be 0: table row = state row = slot, as in ``dfa_mask``), masks its rows s T .. s T + T - 1 from
    its own drafts and fills g_spec[s].  A sequence whose g_on is 0 or that has finished is left untouched, g_spec row
    included.  1 <= S <= 8, 2 <= T <= 8, S * T <= 32.  The exact rule: ``ops.reference.dfa_mask_verify_batch``."""
    if g_spec.dim() == 2:
        S, R = g_spec.shape[0], logits.shape[0]
        if not (1 <= S <= 8 and g_spec.shape[1] == 9 and R % S == 0 and 2 <= R // S <= 8 and R <= 32):
            raise ValueError("dfa_mask_verify: g_spec [1 <= S <= 8, 9], logits [S * T, V] with 2 <= T <= 8 verify rows "
                             "per sequence and S * T <= 32")
        if draft.numel() < S * (R // S - 1) or min(gen_len.numel(), input_ids.numel(), finished.numel()) < S:
            raise ValueError("dfa_mask_verify: draft [S * (T - 1)] and one state row per sequence")
        if int(r) != 0 or S > cls.shape[0]:
            raise ValueError("dfa_mask_verify over S sequences: table row = state row (r = 0), S <= table rows")
        if not _gpu(logits):
            return ref.dfa_mask_verify_batch(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base,
                                             gen_len, input_ids, finished, eos, draft, g_spec, 0)
        return ext().dfa_mask_verify(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, 0,
                                     gen_len, input_ids, finished, eos, draft, g_spec)
    if not 2 <= logits.shape[0] <= 8:
        raise ValueError("dfa_mask_verify: 2 <= T <= 8 verify rows")
    if not _gpu(logits):
        return ref.dfa_mask_verify(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, gen_len,
                                   input_ids, finished, eos, draft, g_spec, r)
    ext().dfa_mask_verify(logits, tok_off, tok_blob, cls, trans, accept, g_dim, g_on, g_state, g_base, int(r), gen_len,
                          input_ids, finished, eos, draft, g_spec)


def dfa_spec_advance(g_on, g_state, g_spec, gen_len, k: int, r: int = 0):
    """After ``spec_commit`` (one wave): with a = gen_len[0] - g_spec[0] - 1 accepted drafts, 0 <= a <= k, the state
    g_spec[1 + a] goes to g_state[r, (gen_len[0] - 1) & 1] -- where the next mask launch, verify or plain, advances
    from.  A 2-D ``g_spec`` [S, 1 + 8] selects the form over S sequences (one launch): sequence s reads gen_len[s] and
    g_spec[s] and stores to g_state[s]; ``r`` must be 0."""
    if g_spec.dim() == 2:
        S = g_spec.shape[0]
        if not (1 <= S <= 8 and g_spec.shape[1] == 9 and 1 <= int(k) <= 7 and S * (int(k) + 1) <= 32):
            raise ValueError("dfa_spec_advance: g_spec [1 <= S <= 8, 9], 1 <= k <= 7, S * (k + 1) <= 32")
        if gen_len.numel() < S or int(r) != 0 or S > g_on.numel():
            raise ValueError("dfa_spec_advance over S sequences: gen_len [S], r = 0, S <= table rows")
        if not _gpu(g_state):
            return ref.dfa_spec_advance_batch(g_on, g_state, g_spec, gen_len, k, 0)
        return ext().dfa_spec_advance(g_on, g_state, g_spec, gen_len, 0, int(k))
    if not _gpu(g_state):
        return ref.dfa_spec_advance(g_on, g_state, g_spec, gen_len, k, r)
    ext().dfa_spec_advance(g_on, g_state, g_spec, gen_len, int(r), int(k))
