"""GGUF checkpoints (the file format of llama.cpp and of Ollama's model blobs): reader and dequantisation.

The reader is host-only (numpy + mmap): it parses the header, the metadata key/values and the tensor infos of GGUF
version 2 or 3 (little-endian) and hands each tensor out as a zero-copy ``uint8`` view of the mapped file.  Every count
and length is checked against the bytes that remain before anything is allocated, so a malformed file raises
``ValueError`` naming the field -- never a ``MemoryError`` or an out-of-range view.

``dequantize`` holds the torch twins of ggml's reference ``dequantize_row_*`` for the tensor types the served models
contain (F32, F16, BF16, Q8_0, Q4_0, Q4_K, Q6_K): raw block bytes in, f32 out, computed in f32 on whatever device the
bytes are on, so a load sends the 4.5-8.5 bits per weight to the GPU and widens them there.

File layout: magic ``GGUF`` | version u32 | tensor count u64 | kv count u64 | kv pairs (key string, value type u32,
value) | tensor infos (name string, n_dims u32, ne u64 x n_dims, ggml type u32, offset u64) | padding to
``general.alignment`` (default 32) | tensor data (offsets relative to its start, each a multiple of the alignment).
A string is a u64 length and that many bytes.  ``ne[0]`` is the contiguous dimension.
"""
from __future__ import annotations

import dataclasses
import mmap
import struct
from typing import Optional

import numpy as np
import torch

MAGIC = b"GGUF"
DEFAULT_ALIGNMENT = 32

# metadata value types
T_U8, T_I8, T_U16, T_I16, T_U32, T_I32, T_F32, T_BOOL, T_STR, T_ARR, T_U64, T_I64, T_F64 = range(13)
_SCALAR = {T_U8: "<u1", T_I8: "<i1", T_U16: "<u2", T_I16: "<i2", T_U32: "<u4", T_I32: "<i4", T_F32: "<f4",
           T_BOOL: "<u1", T_U64: "<u8", T_I64: "<i8", T_F64: "<f8"}
_MAX_ARRAY_DEPTH = 4

# ggml tensor types: number -> (name, elements per block, bytes per block)
F32, F16, Q4_0, Q8_0, Q4_K, Q6_K, BF16 = 0, 1, 2, 8, 12, 14, 30
GGML_TYPES = {F32: ("F32", 1, 4), F16: ("F16", 1, 2), Q4_0: ("Q4_0", 32, 18), Q8_0: ("Q8_0", 32, 34),
              Q4_K: ("Q4_K", 256, 144), Q6_K: ("Q6_K", 256, 210), BF16: ("BF16", 1, 2)}


@dataclasses.dataclass(frozen=True)
class TensorInfo:
    name: str
    ne: tuple        # ggml order: ne[0] is the contiguous dimension
    ggml_type: int
    offset: int      # relative to the start of the tensor data
    nbytes: int

    @property
    def type_name(self) -> str:
        return GGML_TYPES[self.ggml_type][0]

    @property
    def shape(self) -> tuple:
        """Row-major shape: ne reversed ([N, K] for a matrix with ne = [K, N])."""
        return tuple(reversed(self.ne))

    @property
    def numel(self) -> int:
        n = 1
        for d in self.ne:
            n *= d
        return n


class _Cursor:
    """Bounds-checked little-endian reads over the mapped file."""

    def __init__(self, buf, size: int):
        self.buf, self.size, self.pos = buf, size, 0

    def need(self, n: int, field: str) -> None:
        if n < 0 or n > self.size - self.pos:
            raise ValueError(f"GGUF: {field}: needs {n} bytes at offset {self.pos}, file has {self.size - self.pos} left")

    def take(self, n: int, field: str) -> bytes:
        self.need(n, field)
        b = bytes(self.buf[self.pos:self.pos + n])
        self.pos += n
        return b

    def u32(self, field: str) -> int:
        return struct.unpack("<I", self.take(4, field))[0]

    def u64(self, field: str) -> int:
        return struct.unpack("<Q", self.take(8, field))[0]

    def string(self, field: str) -> str:
        n = self.u64(field + " length")
        raw = self.take(n, field)
        try:
            return raw.decode("utf-8")
        except UnicodeDecodeError:  # vocabularies may hold raw byte pieces
            return raw.decode("utf-8", errors="surrogateescape")

    def value(self, vtype: int, field: str, depth: int = 0):
        if vtype in _SCALAR:
            dt = np.dtype(_SCALAR[vtype])
            v = np.frombuffer(self.take(dt.itemsize, field), dtype=dt)[0]
            return bool(v) if vtype == T_BOOL else v.item()
        if vtype == T_STR:
            return self.string(field)
        if vtype == T_ARR:
            if depth >= _MAX_ARRAY_DEPTH:
                raise ValueError(f"GGUF: {field}: arrays nested deeper than {_MAX_ARRAY_DEPTH}")
            et = self.u32(field + " element type")
            n = self.u64(field + " count")
            if et in _SCALAR:
                dt = np.dtype(_SCALAR[et])
                self.need(n * dt.itemsize, field + " count")
                a = np.frombuffer(self.take(n * dt.itemsize, field), dtype=dt)
                return [bool(x) for x in a] if et == T_BOOL else a.tolist()
            if et not in (T_STR, T_ARR):
                raise ValueError(f"GGUF: {field}: unknown metadata value type {et}")
            self.need(n * (8 if et == T_STR else 12), field + " count")  # the least its elements can take
            return [self.value(et, field, depth + 1) for _ in range(n)]
        raise ValueError(f"GGUF: {field}: unknown metadata value type {vtype}")


class GGUFFile:
    """A parsed, memory-mapped GGUF file.  ``metadata``: key -> Python value; ``tensors``: name -> TensorInfo (file
    order); ``raw(name)``: the tensor's bytes as a zero-copy uint8 view, valid until ``close()``."""

    def __init__(self, path: str):
        self.path = str(path)
        self._f = open(self.path, "rb")
        try:
            self._f.seek(0, 2)
            self.size = self._f.tell()
            if self.size < 4:
                raise ValueError(f"GGUF: magic: file has {self.size} bytes")
            self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        except BaseException:
            self._f.close()
            raise
        try:
            self._parse()
        except BaseException:
            self.close()
            raise

    def _parse(self) -> None:
        c = _Cursor(self._mm, self.size)
        magic = c.take(4, "magic")
        if magic != MAGIC:
            raise ValueError(f"GGUF: magic: {magic!r} is not {MAGIC!r}")
        v = c.u32("version")
        if v not in (2, 3):
            if v == 1:
                raise ValueError("GGUF: version: 1 is not supported (versions 2 and 3 are)")
            if v & 0xFFFF == 0 and (v >> 24) in (1, 2, 3):
                raise ValueError(f"GGUF: version: {v:#x} is byte-swapped: a big-endian file, not supported")
            raise ValueError(f"GGUF: version: {v} is not supported (versions 2 and 3 are)")
        self.version = v
        n_tensors = c.u64("tensor count")
        n_kv = c.u64("metadata kv count")
        c.need(n_kv * 13, "metadata kv count")      # key length + value type + one byte, at least
        self.metadata: dict = {}
        for _ in range(n_kv):
            key = c.string("metadata key")
            if key in self.metadata:
                raise ValueError(f"GGUF: metadata key: duplicate {key!r}")
            self.metadata[key] = c.value(c.u32(f"value type of {key!r}"), f"metadata value of {key!r}")
        align = self.metadata.get("general.alignment", DEFAULT_ALIGNMENT)
        if not isinstance(align, int) or isinstance(align, bool) or align <= 0 or align & (align - 1):
            raise ValueError(f"GGUF: general.alignment: {align!r} is not a power of two")
        self.alignment = align
        c.need(n_tensors * 24, "tensor count")      # name length + n_dims + type + offset, at least
        infos = []
        seen = set()
        for _ in range(n_tensors):
            name = c.string("tensor name")
            if name in seen:
                raise ValueError(f"GGUF: tensor name: duplicate {name!r}")
            seen.add(name)
            nd = c.u32(f"n_dims of {name!r}")
            if not 1 <= nd <= 4:
                raise ValueError(f"GGUF: n_dims of {name!r}: {nd} is not in 1..4")
            ne = tuple(c.u64(f"ne of {name!r}") for _ in range(nd))
            t = c.u32(f"ggml type of {name!r}")
            if t not in GGML_TYPES:
                raise ValueError(f"GGUF: ggml type of {name!r}: type {t} is not supported "
                                 f"(supported: {', '.join(f'{n} = {k}' for k, (n, _, _) in GGML_TYPES.items())})")
            _, blk, bpb = GGML_TYPES[t]
            if any(d <= 0 for d in ne) or ne[0] % blk:
                raise ValueError(f"GGUF: ne of {name!r}: ne[0] = {ne[0]} is not a positive multiple of the "
                                 f"{GGML_TYPES[t][0]} block size {blk}" if all(d > 0 for d in ne) else
                                 f"GGUF: ne of {name!r}: {ne} has an empty dimension")
            n = 1
            for d in ne:
                n *= d
            off = c.u64(f"offset of {name!r}")
            if off % align:
                raise ValueError(f"GGUF: offset of {name!r}: {off} is not a multiple of the alignment {align}")
            infos.append(TensorInfo(name, ne, t, off, n // blk * bpb))
        self.data_offset = (c.pos + align - 1) // align * align
        for ti in infos:
            if self.data_offset + ti.offset + ti.nbytes > self.size:
                raise ValueError(f"GGUF: tensor {ti.name!r}: {ti.nbytes} bytes at data offset {ti.offset} extend past "
                                 f"the end of the file ({self.size} bytes, data from {self.data_offset})")
        self.tensors = {ti.name: ti for ti in infos}
        self._np = np.frombuffer(self._mm, dtype=np.uint8)

    def raw(self, name: str) -> np.ndarray:
        ti = self.tensors[name]
        a = self.data_offset + ti.offset
        return self._np[a:a + ti.nbytes]

    def type_counts(self) -> dict:
        out: dict = {}
        for ti in self.tensors.values():
            out[ti.type_name] = out.get(ti.type_name, 0) + 1
        return out

    def tensor_f32(self, name: str, device="cpu") -> torch.Tensor:
        """The tensor dequantised to f32 in its row-major shape on ``device`` (the raw bytes travel, not the f32)."""
        ti = self.tensors[name]
        raw = torch.from_numpy(np.array(self.raw(name))).to(device)
        return dequantize(raw, ti.ggml_type).reshape(ti.shape)

    def close(self) -> None:
        self._np = None
        try:
            self._mm.close()
        except (AttributeError, BufferError, ValueError):
            pass
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def is_gguf(path) -> bool:
    """A file (Ollama blobs carry no extension) whose first four bytes are the GGUF magic."""
    import os

    if not path or not os.path.isfile(path):
        return False
    with open(path, "rb") as f:
        return f.read(4) == MAGIC


# ----------------------------------------------------------------------------------- dequantisation twins
def _f16(raw: torch.Tensor) -> torch.Tensor:
    """uint8 [..., 2] -> f32 [...] (the little-endian f16 they hold)."""
    return raw.contiguous().view(torch.float16).squeeze(-1).float()


def q4_0_split(raw: torch.Tensor):
    """Q4_0 blocks (uint8 [nblocks * 18]) -> (codes uint8 [nblocks, 32], d f16 [nblocks]): block = f16 d, 16 bytes qs;
    element j is the low nibble of qs[j], element 16 + j the high one."""
    b = raw.reshape(-1, 18)
    qs = b[:, 2:]
    return torch.cat([qs & 15, qs >> 4], dim=1), b[:, :2].contiguous().view(torch.float16).squeeze(-1)


def dequantize(raw: torch.Tensor, ggml_type: int) -> torch.Tensor:
    """Raw tensor bytes (uint8, 1-D) -> f32 [numel] by ggml's reference definitions, every step in f32."""
    if ggml_type == F32:
        return raw.contiguous().view(torch.float32).clone()
    if ggml_type == F16:
        return raw.contiguous().view(torch.float16).float()
    if ggml_type == BF16:
        return raw.contiguous().view(torch.bfloat16).float()
    if ggml_type == Q8_0:  # f16 d, 32 int8 qs: y = d * q
        b = raw.reshape(-1, 34)
        return (_f16(b[:, :2])[:, None] * b[:, 2:].contiguous().view(torch.int8).float()).reshape(-1)
    if ggml_type == Q4_0:  # y = d * (q - 8)
        codes, d = q4_0_split(raw)
        return (d.float()[:, None] * (codes.float() - 8.0)).reshape(-1)
    if ggml_type == Q4_K:
        # f16 d, f16 dmin, 12 bytes of 6-bit (scale, min) pairs, 128 bytes qs; eight sub-blocks of 32: sub-blocks
        # 2 c and 2 c + 1 are the low and high nibbles of qs[32 c .. 32 c + 31]; y = (d * sc) * q - (dmin * m)
        b = raw.reshape(-1, 144)
        d, dmin = _f16(b[:, 0:2]), _f16(b[:, 2:4])
        s = b[:, 4:16].to(torch.int32)
        sc = torch.cat([s[:, 0:4] & 63, (s[:, 8:12] & 15) | ((s[:, 0:4] >> 6) << 4)], dim=1).float()
        mn = torch.cat([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], dim=1).float()
        qs = b[:, 16:].reshape(-1, 4, 32)
        q = torch.stack([qs & 15, qs >> 4], dim=2).reshape(-1, 8, 32).float()
        return ((d[:, None] * sc)[..., None] * q - (dmin[:, None] * mn)[..., None]).reshape(-1)
    if ggml_type == Q6_K:
        # 128 bytes ql, 64 bytes qh, 16 int8 scales, f16 d; two halves of 128: element 32 t + l of a half (t = 0..3)
        # has low bits ql[l + 32 (t & 1)] >> 4 (t >> 1), high bits (qh[l] >> 2 t) & 3, scale index 2 t + l / 16;
        # y = (d * scale) * (q - 32)
        b = raw.reshape(-1, 210)
        ql = b[:, :128].reshape(-1, 2, 2, 32).to(torch.int32)   # half, t & 1, l
        qh = b[:, 128:192].reshape(-1, 2, 1, 32).to(torch.int32)
        sc = b[:, 192:208].contiguous().view(torch.int8).float().reshape(-1, 2, 4, 2)  # half, t, l / 16
        d = _f16(b[:, 208:210])
        lo = torch.cat([ql & 15, ql >> 4], dim=2)                # half, t, l
        sh = torch.arange(0, 8, 2, device=raw.device).view(1, 1, 4, 1)
        q = (lo | (((qh >> sh) & 3) << 4)) - 32
        ds = d[:, None, None, None] * sc                         # half, t, l / 16
        return (ds.repeat_interleave(16, dim=3) * q.float()).reshape(-1)
    raise ValueError(f"GGUF: ggml type {ggml_type} is not supported")


# ----------------------------------------------------------------------------------- model metadata
ARCH = "llama"


def _meta(md: dict, key: str, default=None, required: bool = False):
    if key not in md:
        if required:
            raise ValueError(f"GGUF: metadata key {key!r} is missing")
        return default
    return md[key]


def model_dims(g: GGUFFile) -> dict:
    """The model dimensions of a llama-architecture file, by spec field name."""
    md = g.metadata
    arch = _meta(md, "general.architecture", required=True)
    if arch != ARCH:
        raise ValueError(f"GGUF: general.architecture: {arch!r} is not supported (only {ARCH!r})")
    if "token_embd.weight" not in g.tensors:
        raise ValueError("GGUF: required tensor 'token_embd.weight' is missing")
    hidden = int(_meta(md, "llama.embedding_length", required=True))
    heads = int(_meta(md, "llama.attention.head_count", required=True))
    if heads <= 0 or hidden <= 0:
        raise ValueError(f"GGUF: llama.attention.head_count: {heads} heads over llama.embedding_length {hidden}")
    hd = _meta(md, "llama.attention.key_length", _meta(md, "llama.rope.dimension_count", hidden // heads))
    emb = g.tensors["token_embd.weight"]
    if len(emb.ne) != 2:
        raise ValueError(f"GGUF: ne of 'token_embd.weight': {emb.ne} is not a matrix")
    return {
        "n_layers": ("llama.block_count", int(_meta(md, "llama.block_count", required=True))),
        "hidden": ("llama.embedding_length", hidden),
        "ffn": ("llama.feed_forward_length", int(_meta(md, "llama.feed_forward_length", required=True))),
        "n_heads": ("llama.attention.head_count", heads),
        "n_kv_heads": ("llama.attention.head_count_kv", int(_meta(md, "llama.attention.head_count_kv", heads))),
        "head_dim": ("llama.attention.key_length", int(hd)),
        "vocab_size": ("token_embd.weight", int(emb.ne[1])),
        "rms_eps": ("llama.attention.layer_norm_rms_epsilon",
                    float(_meta(md, "llama.attention.layer_norm_rms_epsilon", 1e-5))),
        "rope_theta": ("llama.rope.freq_base", float(_meta(md, "llama.rope.freq_base", 10000.0))),
    }


def tokenizer_dict(md: dict) -> Optional[dict]:
    """The ``tokenizer.ggml.*`` metadata under the field names transformers' GGUF tokenizer converters read, or None
    when the file carries no vocabulary."""
    p = "tokenizer.ggml."
    if p + "model" not in md or p + "tokens" not in md:
        return None
    out = {k[len(p):]: v for k, v in md.items() if k.startswith(p)}
    out["tokenizer_type"] = out.pop("model")
    return out
