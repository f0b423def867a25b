"""Helpers of the GGUF tests: a minimal GGUF writer, scalar transcriptions of ggml's reference dequantisation (plain
loops over one block, written independently of the vectorised twins in models/gguf.py), and builders of tiny checkpoint
files from a seeded HF-layout state dict.  Files go to the test's tmp_path; nothing is committed."""
import dataclasses
import struct

import numpy as np
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.models import gguf as G
from llm_based_apache_spark_optimization_amd.models.spec import get_spec

# ----------------------------------------------------------------------------------- writer
U8, I8, U16, I16, U32, I32, F32V, BOOL, STR, ARR, U64, I64, F64 = range(13)
_FMT = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", F32V: "<f", BOOL: "<B", U64: "<Q", I64: "<q",
        F64: "<d"}


def _string(s) -> bytes:
    b = s if isinstance(s, bytes) else s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def encode_value(vtype: int, v) -> bytes:
    """A metadata value; an array is ``(element type, [values])``, nested arrays nest that pair."""
    if vtype in _FMT:
        return struct.pack(_FMT[vtype], v)
    if vtype == STR:
        return _string(v)
    if vtype == ARR:
        et, items = v
        return struct.pack("<IQ", et, len(items)) + b"".join(encode_value(et, x) for x in items)
    raise ValueError(vtype)


def write_gguf(path, metadata, tensors, version=3, alignment=None, magic=b"GGUF", tensor_count=None, kv_count=None,
               misalign=None):
    """metadata: [(key, value type, value)]; tensors: [(name, ne, ggml type, data bytes)].  ``alignment``: written as
    general.alignment when given (else the default 32 applies).  tensor_count / kv_count: lie in the header.
    misalign: {tensor name: bytes added to its offset}.  Returns the section boundaries
    {"header", "metadata", "infos", "data_start", "end"} as file offsets."""
    md = list(metadata)
    if alignment is not None:
        md.append(("general.alignment", U32, alignment))
    align = alignment or 32
    out = bytearray(magic + struct.pack("<I", version))
    out += struct.pack("<QQ", len(tensors) if tensor_count is None else tensor_count,
                       len(md) if kv_count is None else kv_count)
    marks = {"header": len(out)}
    for key, vt, v in md:
        out += _string(key) + struct.pack("<I", vt) + encode_value(vt, v)
    marks["metadata"] = len(out)
    off = 0
    offsets = []
    for name, ne, t, data in tensors:
        o = off + (misalign or {}).get(name, 0)
        offsets.append(o)
        out += _string(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne)
        out += struct.pack("<IQ", t, o)
        off = (o + len(data) + align - 1) // align * align
    marks["infos"] = len(out)
    out += b"\0" * (-len(out) % align)
    marks["data_start"] = len(out)
    for (name, ne, t, data), o in zip(tensors, offsets):
        out += b"\0" * (marks["data_start"] + o - len(out))
        out += data
    marks["end"] = len(out)
    with open(path, "wb") as f:
        f.write(bytes(out))
    return marks


# ----------------------------------------------------------------------------------- scalar transcriptions
f32 = np.float32


def _h(b) -> np.float32:
    return np.frombuffer(bytes(b[:2]), dtype="<f2")[0].astype(np.float32)


def _i8(v: int) -> int:
    return v - 256 if v > 127 else v


def scalar_f32(b):
    return [np.frombuffer(bytes(b), dtype="<f4")[0]]


def scalar_f16(b):
    return [_h(b)]


def scalar_bf16(b):
    return [np.frombuffer(bytes([0, 0, b[0], b[1]]), dtype="<f4")[0]]


def scalar_q8_0(b):
    d = _h(b[0:2])
    return [d * f32(_i8(b[2 + j])) for j in range(32)]


def scalar_q4_0(b):
    d = _h(b[0:2])
    y = [None] * 32
    for j in range(16):
        x0 = (b[2 + j] & 0x0F) - 8
        x1 = (b[2 + j] >> 4) - 8
        y[j] = f32(x0) * d
        y[j + 16] = f32(x1) * d
    return y


def _scale_min_k4(j, q):
    if j < 4:
        return q[j] & 63, q[j + 4] & 63
    return (q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4), (q[j + 4] >> 4) | ((q[j] >> 6) << 4)


def scalar_q4_k(b):
    d, dmin = _h(b[0:2]), _h(b[2:4])
    scales, q = b[4:16], b[16:144]
    y = []
    is_ = 0
    for j in range(0, 256, 64):
        sc, m = _scale_min_k4(is_, scales)
        d1, m1 = d * f32(sc), dmin * f32(m)
        sc, m = _scale_min_k4(is_ + 1, scales)
        d2, m2 = d * f32(sc), dmin * f32(m)
        qq = q[j // 2:j // 2 + 32]
        y += [d1 * f32(qq[l] & 0xF) - m1 for l in range(32)]
        y += [d2 * f32(qq[l] >> 4) - m2 for l in range(32)]
        is_ += 2
    return y


def scalar_q6_k(b):
    ql, qh, sc = b[0:128], b[128:192], [_i8(v) for v in b[192:208]]
    d = _h(b[208:210])
    y = [None] * 256
    for n in range(0, 256, 128):
        qlo, qho, sco = ql[n // 2:], qh[n // 4:], sc[n // 16:]
        for l in range(32):
            i = l // 16
            q1 = ((qlo[l] & 0xF) | (((qho[l] >> 0) & 3) << 4)) - 32
            q2 = ((qlo[l + 32] & 0xF) | (((qho[l] >> 2) & 3) << 4)) - 32
            q3 = ((qlo[l] >> 4) | (((qho[l] >> 4) & 3) << 4)) - 32
            q4 = ((qlo[l + 32] >> 4) | (((qho[l] >> 6) & 3) << 4)) - 32
            y[n + l] = d * f32(sco[i]) * f32(q1)
            y[n + l + 32] = d * f32(sco[i + 2]) * f32(q2)
            y[n + l + 64] = d * f32(sco[i + 4]) * f32(q3)
            y[n + l + 96] = d * f32(sco[i + 6]) * f32(q4)
    return y


SCALAR = {G.F32: scalar_f32, G.F16: scalar_f16, G.BF16: scalar_bf16, G.Q8_0: scalar_q8_0, G.Q4_0: scalar_q4_0,
          G.Q4_K: scalar_q4_k, G.Q6_K: scalar_q6_k}


def scalar_dequant(raw: bytes, ggml_type: int) -> torch.Tensor:
    bpb = G.GGML_TYPES[ggml_type][2]
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(0, len(raw), bpb):
            out += SCALAR[ggml_type](raw[i:i + bpb])
    return torch.from_numpy(np.array(out, dtype=np.float32))


def f16_bytes(v) -> bytes:
    return np.array([v], dtype="<f2").tobytes()


# f16 block scales every block type is tried with: zero, negative, subnormal (2^-24 and the largest), the largest finite
EDGE_SCALES = (0.0, -0.0, -0.375, 2.0 ** -24, -(2.0 ** -14 - 2.0 ** -24), 65504.0, -65504.0, 1.0, 0.0123)


# ----------------------------------------------------------------------------------- tensor encoders
TYPE_IDS = {"F32": G.F32, "F16": G.F16, "BF16": G.BF16, "Q8_0": G.Q8_0, "Q4_0": G.Q4_0, "Q4_K": G.Q4_K, "Q6_K": G.Q6_K}


def q4_0_blocks(codes: torch.Tensor, d: torch.Tensor) -> bytes:
    """(codes uint8 [N, K], d f16 [N, K/32]) -> ggml block_q4_0 bytes: qs[j] = code j | code 16 + j << 4."""
    c = codes.reshape(-1, 2, 16)
    qs = (c[:, 0] | (c[:, 1] << 4)).numpy()
    blk = np.concatenate([d.reshape(-1, 1).numpy().view(np.uint8), qs], axis=1)
    return blk.tobytes()


def encode_tensor(w: torch.Tensor, tname: str, gen: torch.Generator):
    """f32 tensor -> (ggml type, bytes, the f32 values the bytes dequantise to, in w's shape).  Q4_0 quantises by
    ``ops.quantize_q4_0``; Q8_0 by amax / 127; the K-quants are random codes under small finite scales (their values
    have nothing to do with ``w``: the tests only need the file and the model to agree)."""
    t = TYPE_IDS[tname]
    if tname == "F32":
        return t, w.float().numpy().astype("<f4").tobytes(), w.float().clone()
    if tname in ("F16", "BF16"):
        h = w.to(torch.float16 if tname == "F16" else torch.bfloat16)
        return t, h.view(torch.int16).numpy().astype("<i2").tobytes(), h.float()
    if tname == "Q4_0":
        w2 = w.reshape(-1, w.shape[-1])
        codes, d = ops.quantize_q4_0(w2)
        deq = d.float()[..., None] * (codes.reshape(w2.shape[0], -1, 32).float() - 8.0)
        return t, q4_0_blocks(codes, d), deq.reshape(w.shape)
    if tname == "Q8_0":
        x = w.float().reshape(-1, 32)
        d = (x.abs().amax(1) / 127.0).to(torch.float16)
        q = torch.where(d[:, None] != 0, x / d.float()[:, None], torch.zeros_like(x)).round().clamp(-127, 127).to(torch.int8)
        blk = np.concatenate([d.reshape(-1, 1).numpy().view(np.uint8), q.numpy().view(np.uint8)], axis=1)
        return t, blk.tobytes(), (d.float()[:, None] * q.float()).reshape(w.shape)
    _, blk_el, bpb = G.GGML_TYPES[t]
    nblk = w.numel() // blk_el
    raw = torch.randint(0, 256, (nblk, bpb), generator=gen, dtype=torch.uint8)
    small = torch.tensor(np.frombuffer(f16_bytes(2.0 ** -15), dtype=np.uint8).copy())
    if tname == "Q4_K":
        raw[:, 0:2] = small
        raw[:, 2:4] = small
    else:
        raw[:, 208:210] = small
    return t, raw.numpy().tobytes(), G.dequantize(raw.reshape(-1), t).reshape(w.shape)


# ----------------------------------------------------------------------------------- checkpoint builders
def hf_state_dict(spec, seed: int = 0) -> dict:
    """A seeded HF-layout (LlamaForCausalLM) f32 state dict of ``spec``."""
    g = torch.Generator().manual_seed(seed)
    d, hd = spec.hidden, spec.head_dim

    def rnd(*shape, s=0.05):
        return torch.randn(*shape, generator=g) * s

    sd = {"model.embed_tokens.weight": rnd(spec.vocab_size, d, s=1.0), "model.norm.weight": 1.0 + rnd(d, s=0.1)}
    for i in range(spec.n_layers):
        p = f"model.layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = rnd(spec.n_heads * hd, d)
        sd[p + "self_attn.k_proj.weight"] = rnd(spec.n_kv_heads * hd, d)
        sd[p + "self_attn.v_proj.weight"] = rnd(spec.n_kv_heads * hd, d)
        sd[p + "self_attn.o_proj.weight"] = rnd(d, spec.n_heads * hd)
        sd[p + "mlp.gate_proj.weight"] = rnd(spec.ffn, d)
        sd[p + "mlp.up_proj.weight"] = rnd(spec.ffn, d)
        sd[p + "mlp.down_proj.weight"] = rnd(d, spec.ffn)
        sd[p + "input_layernorm.weight"] = 1.0 + rnd(d, s=0.1)
        sd[p + "post_attention_layernorm.weight"] = 1.0 + rnd(d, s=0.1)
    if not spec.tie_embeddings:
        sd["lm_head.weight"] = rnd(spec.vocab_size, d)
    return sd


def converter_permute(w: torch.Tensor, n_head: int) -> torch.Tensor:
    """The row order llama.cpp's converter stores q and k in (HF half-split rotary -> interleaved pairs)."""
    n, k = w.shape
    return w.reshape(n_head, 2, n // n_head // 2, k).swapaxes(1, 2).reshape(n, k)


_HF_TO_GGUF = {"self_attn.q_proj": "attn_q", "self_attn.k_proj": "attn_k", "self_attn.v_proj": "attn_v",
               "self_attn.o_proj": "attn_output", "mlp.gate_proj": "ffn_gate", "mlp.up_proj": "ffn_up",
               "mlp.down_proj": "ffn_down", "input_layernorm": "attn_norm", "post_attention_layernorm": "ffn_norm"}


def gguf_name(hf_name: str) -> str:
    if hf_name == "model.embed_tokens.weight":
        return "token_embd.weight"
    if hf_name == "model.norm.weight":
        return "output_norm.weight"
    if hf_name == "lm_head.weight":
        return "output.weight"
    _, _, i, rest = hf_name.split(".", 3)
    return f"blk.{i}.{_HF_TO_GGUF[rest[:-len('.weight')]]}.weight"


def model_metadata(spec, arch="llama", **over) -> list:
    md = {"general.architecture": (STR, arch), "general.name": (STR, spec.name),
          "llama.block_count": (U32, spec.n_layers), "llama.context_length": (U32, spec.max_position),
          "llama.embedding_length": (U32, spec.hidden), "llama.feed_forward_length": (U32, spec.ffn),
          "llama.attention.head_count": (U32, spec.n_heads), "llama.attention.head_count_kv": (U32, spec.n_kv_heads),
          "llama.attention.key_length": (U32, spec.head_dim), "llama.rope.dimension_count": (U32, spec.head_dim),
          "llama.attention.layer_norm_rms_epsilon": (F32V, spec.rms_eps), "llama.rope.freq_base": (F32V, spec.rope_theta),
          "general.file_type": (U32, 2)}
    for k, v in over.items():
        if v is None:
            md.pop(k, None)
        else:
            md[k] = v
    return [(k, vt, v) for k, (vt, v) in md.items()]


def build_checkpoint(path, model="tiny-nsql", seed=0, proj="Q4_0", types=None, embd="Q4_0", output="Q4_0",
                     rope_freqs=False, meta=None, extra_metadata=(), drop=(), version=3, alignment=None, arch="llama",
                     vocab=None):
    """Write a tiny GGUF checkpoint of the named spec.  proj: the type of the seven projection tensors; types:
    {gguf tensor name: type} exceptions; embd / output: the types of token_embd / output.weight (a tied spec writes no
    output.weight); vocab: rows of token_embd / output.weight when not the spec's; meta: metadata overrides ({key: (value type, value) | None to drop}); drop: tensor names left out.
    Returns (src, deq): the seeded HF-layout state dict the file was made from, and the HF-layout state dict of the f32
    values the file's tensors dequantise to (q / k rows back in HF order)."""
    spec = get_spec(model)
    src = hf_state_dict(dataclasses.replace(spec, vocab_size=vocab) if vocab else spec, seed)
    g = torch.Generator().manual_seed(seed + 1)
    tensors, deq = [], {}
    for hf, w in src.items():
        name = gguf_name(hf)
        if w.dim() == 1:
            tname = "F32"
        elif name == "token_embd.weight":
            tname = embd
        elif name == "output.weight":
            tname = output
        else:
            tname = proj
        tname = (types or {}).get(name, tname)
        heads = spec.n_heads if ".attn_q." in name else spec.n_kv_heads if ".attn_k." in name else 0
        stored = converter_permute(w, heads) if heads else w
        t, data, dv = encode_tensor(stored, tname, g)
        if heads:  # back to HF row order: the inverse permutation
            n, k = dv.shape
            dv = dv.reshape(heads, n // heads // 2, 2, k).swapaxes(1, 2).reshape(n, k)
        deq[hf] = dv
        if name not in drop:
            tensors.append((name, tuple(reversed(w.shape)), t, data))
    if rope_freqs:
        tensors.append(("rope_freqs.weight", (spec.head_dim // 2,), G.F32,
                        np.ones(spec.head_dim // 2, dtype="<f4").tobytes()))
    write_gguf(path, model_metadata(spec, arch=arch, **(meta or {})) + list(extra_metadata), tensors, version=version,
               alignment=alignment)
    return src, deq


# ----------------------------------------------------------------------------------- synthetic vocabularies
def _gpt2_byte_chars():
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    out, n = [], 0
    for b in range(256):
        if b in keep:
            out.append(chr(b))
        else:
            out.append(chr(256 + n))
            n += 1
    return out


def gpt2_vocab_metadata() -> list:
    """A byte-level BPE vocabulary: the 256 byte tokens, a few merges, begin / end markers."""
    sp = "Ġ"  # the byte-level image of a space
    merges = ["h e", "l l", "he ll", "hell o", f"{sp} w", "o r", f"{sp}w or"]
    tokens = _gpt2_byte_chars() + [m.replace(" ", "") for m in merges] + ["<|begin|>", "<|end|>"]
    types = [1] * (len(tokens) - 2) + [3, 3]
    n = len(tokens)
    return [("tokenizer.ggml.model", STR, "gpt2"), ("tokenizer.ggml.pre", STR, "default"),
            ("tokenizer.ggml.tokens", ARR, (STR, tokens)), ("tokenizer.ggml.token_type", ARR, (I32, types)),
            ("tokenizer.ggml.merges", ARR, (STR, merges)), ("tokenizer.ggml.bos_token_id", U32, n - 2),
            ("tokenizer.ggml.eos_token_id", U32, n - 1)]


def llama_vocab_metadata() -> list:
    """A SentencePiece-style vocabulary: <unk> <s> </s>, the 256 byte tokens, letters and a few scored pieces."""
    tokens = ["<unk>", "<s>", "</s>"] + [f"<0x{b:02X}>" for b in range(256)]
    types = [2, 3, 3] + [6] * 256
    scores = [0.0] * len(tokens)
    pieces = ["▁"] + [chr(c) for c in range(ord("a"), ord("z") + 1)] + [
        "he", "ll", "hell", "hello", "▁hello", "wo", "▁wo", "rl", "▁worl", "wor", "▁wor", "worl"]
    for i, p in enumerate(pieces):
        tokens.append(p)
        types.append(1)
        scores.append(-1.0 - i if len(p) == 1 else -float(20 - len(p)) / 10.0)
    return [("tokenizer.ggml.model", STR, "llama"), ("tokenizer.ggml.tokens", ARR, (STR, tokens)),
            ("tokenizer.ggml.scores", ARR, (F32V, scores)), ("tokenizer.ggml.token_type", ARR, (I32, types)),
            ("tokenizer.ggml.bos_token_id", U32, 1), ("tokenizer.ggml.eos_token_id", U32, 2),
            ("tokenizer.ggml.unknown_token_id", U32, 0)]
