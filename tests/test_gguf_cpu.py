"""GGUF checkpoints on the CPU: the reader and its refusals, the dequantisation twins against scalar transcriptions of
ggml's definitions, the Q4_0 host functions, the tensor mapping, the dtype table, the tokenizer and the settings."""
import struct
import warnings

import numpy as np
import pytest
import torch

import gguf_cases as gc
from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.engine import LLMEngine
from llm_based_apache_spark_optimization_amd.engine.runner import ModelRunner
from llm_based_apache_spark_optimization_amd.models import gguf as G
from llm_based_apache_spark_optimization_amd.models import llama as llama_mod
from llm_based_apache_spark_optimization_amd.models import tokenizer as tok_mod
from llm_based_apache_spark_optimization_amd.models import tokenizer_for
from llm_based_apache_spark_optimization_amd.models.llama import from_hf_state_dict, load_gguf
from llm_based_apache_spark_optimization_amd.models.spec import get_spec

ONE = [("t", (32,), G.F32, np.arange(32, dtype="<f4").tobytes())]


# ----------------------------------------------------------------------------------- reader
def test_metadata_round_trip_every_type(tmp_path):
    md = [("u8", gc.U8, 250), ("i8", gc.I8, -7), ("u16", gc.U16, 65000), ("i16", gc.I16, -30000),
          ("u32", gc.U32, 4000000000), ("i32", gc.I32, -2000000000), ("f32", gc.F32V, 0.5), ("yes", gc.BOOL, 1),
          ("no", gc.BOOL, 0), ("s", gc.STR, "héllo"), ("empty", gc.STR, ""), ("u64", gc.U64, 2 ** 63 + 5),
          ("i64", gc.I64, -2 ** 62), ("f64", gc.F64, 1e-300), ("ints", gc.ARR, (gc.I32, [3, -1, 2])),
          ("floats", gc.ARR, (gc.F32V, [0.25, -2.0])), ("strs", gc.ARR, (gc.STR, ["a", "", "ccc"])),
          ("none", gc.ARR, (gc.U8, [])), ("bools", gc.ARR, (gc.BOOL, [1, 0])),
          ("nested", gc.ARR, (gc.ARR, [(gc.U16, [1, 2]), (gc.STR, ["x", ""]), (gc.ARR, [(gc.I8, [-1])])]))]
    p = tmp_path / "m.gguf"
    gc.write_gguf(p, md, ONE)
    with G.GGUFFile(p) as g:
        want = {"u8": 250, "i8": -7, "u16": 65000, "i16": -30000, "u32": 4000000000, "i32": -2000000000, "f32": 0.5,
                "yes": True, "no": False, "s": "héllo", "empty": "", "u64": 2 ** 63 + 5, "i64": -2 ** 62, "f64": 1e-300,
                "ints": [3, -1, 2], "floats": [0.25, -2.0], "strs": ["a", "", "ccc"], "none": [], "bools": [True, False],
                "nested": [[1, 2], ["x", ""], [[-1]]]}
        assert g.metadata == want
        assert type(g.metadata["yes"]) is bool and type(g.metadata["u8"]) is int
        assert g.version == 3 and g.alignment == 32
        assert np.array_equal(g.raw("t").view("<f4"), np.arange(32, dtype="<f4"))


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("alignment", [None, 64])
def test_versions_and_alignment(tmp_path, version, alignment):
    a = np.arange(40, dtype="<f4")
    b = np.arange(32, dtype="<f2")
    p = tmp_path / "a.gguf"
    marks = gc.write_gguf(p, [("k", gc.STR, "v")], [("a", (40,), G.F32, a.tobytes()), ("b", (8, 4), G.F16, b.tobytes())],
                          version=version, alignment=alignment)
    al = alignment or 32
    with G.GGUFFile(p) as g:
        assert g.version == version and g.alignment == al
        assert g.data_offset == marks["data_start"] and g.data_offset % al == 0
        assert g.tensors["b"].offset == 192 if al == 64 else g.tensors["b"].offset == 160
        assert g.tensors["b"].shape == (4, 8) and g.tensors["b"].type_name == "F16"
        ra = g.raw("a")
        assert not ra.flags.owndata and not ra.flags.writeable  # a view of the mapping, not a copy
        assert np.array_equal(ra.view("<f4"), a) and np.array_equal(g.raw("b").view("<f2"), b)
        assert torch.equal(g.tensor_f32("b"), torch.from_numpy(b.astype(np.float32)).reshape(4, 8))
        assert g.type_counts() == {"F32": 1, "F16": 1}


def _raises(p, field):
    with pytest.raises(ValueError, match=field):
        G.GGUFFile(p).close()


def test_refusals_name_the_field(tmp_path):
    p = tmp_path / "r.gguf"
    gc.write_gguf(p, [], ONE, magic=b"GGML")
    _raises(p, "magic")
    gc.write_gguf(p, [], ONE, version=1)
    _raises(p, "version")
    gc.write_gguf(p, [], ONE, version=3 << 24)  # a big-endian file read little-endian
    _raises(p, "version.*big-endian")
    gc.write_gguf(p, [], ONE, version=7)
    _raises(p, "version")
    gc.write_gguf(p, [], ONE)
    raw = bytearray(p.read_bytes())
    with open(p, "wb") as f:  # a metadata value of type 13
        f.write(raw[:16] + struct.pack("<Q", 1) + gc._string("bad") + struct.pack("<I", 13) + raw[24:])
    _raises(p, "unknown metadata value type 13")
    gc.write_gguf(p, [("arr", gc.ARR, (77, []))], ONE)
    _raises(p, "unknown metadata value type 77")
    gc.write_gguf(p, [], [("t", (32,), 3, b"\0" * 20)])  # Q4_1
    _raises(p, "ggml type of 't'.*type 3 ")
    gc.write_gguf(p, [], [("t", (32,), 99, b"\0" * 20)])
    _raises(p, "type 99 ")
    gc.write_gguf(p, [], [("t", (48, 2), G.Q4_0, b"\0" * 54)])
    _raises(p, r"ne of 't'.*ne\[0\] = 48.*block size 32")
    gc.write_gguf(p, [], [("t", (128, 2), G.Q4_K, b"\0" * 144)])
    _raises(p, r"ne\[0\] = 128.*block size 256")
    gc.write_gguf(p, [], ONE + [("u", (32,), G.F32, b"\0" * 128)], misalign={"u": 4})
    _raises(p, "offset of 'u'.*alignment")
    gc.write_gguf(p, [], ONE + [("t", (32,), G.F32, b"\0" * 128)])
    _raises(p, "tensor name: duplicate 't'")
    gc.write_gguf(p, [("k", gc.U8, 1), ("k", gc.U8, 2)], ONE)
    _raises(p, "metadata key: duplicate 'k'")
    gc.write_gguf(p, [], ONE, alignment=48)
    _raises(p, "general.alignment")
    gc.write_gguf(p, [], [("t", (32, 2, 2, 2, 2), G.F32, b"")])
    _raises(p, "n_dims")
    gc.write_gguf(p, [], [("t", (32, 0), G.F32, b"")])
    _raises(p, "ne of 't'")


def test_huge_counts_and_truncation(tmp_path):
    p = tmp_path / "h.gguf"
    gc.write_gguf(p, [("k", gc.STR, "v")], ONE, tensor_count=2 ** 60)
    _raises(p, "tensor count")
    gc.write_gguf(p, [("k", gc.STR, "v")], ONE, kv_count=2 ** 60)
    _raises(p, "kv count")
    gc.write_gguf(p, [("a", gc.ARR, (gc.U64, []))], ONE)
    raw = bytearray(p.read_bytes())
    i = raw.index(b"\x01\x00\x00\x00\x00\x00\x00\x00a") + 9 + 4 + 4  # the array's count field
    raw[i:i + 8] = struct.pack("<Q", 2 ** 61)
    p.write_bytes(bytes(raw))
    _raises(p, "'a' count")
    gc.write_gguf(p, [("a", gc.ARR, (gc.STR, []))], ONE)
    raw = bytearray(p.read_bytes())
    i = raw.index(b"\x01\x00\x00\x00\x00\x00\x00\x00a") + 9 + 4 + 4
    raw[i:i + 8] = struct.pack("<Q", 2 ** 59)
    p.write_bytes(bytes(raw))
    _raises(p, "'a' count")
    gc.write_gguf(p, [("s", gc.STR, "v")], ONE)
    raw = bytearray(p.read_bytes())
    i = raw.index(b"\x01\x00\x00\x00\x00\x00\x00\x00s") + 9 + 4  # the string's length field
    raw[i:i + 8] = struct.pack("<Q", 2 ** 62)
    p.write_bytes(bytes(raw))
    _raises(p, "metadata value of 's'")
    # a file cut at every section boundary, one byte short of it, and in the middle of the data
    md = [("k", gc.STR, "v"), ("n", gc.U32, 3)]
    tensors = ONE + [("u", (32, 2), G.Q4_0, b"\x11" * 36)]
    marks = gc.write_gguf(p, md, tensors)
    whole = p.read_bytes()
    G.GGUFFile(p).close()
    for cut in sorted({0, 3, 4, 8, 16, marks["header"] - 1, marks["header"], marks["metadata"] - 1, marks["metadata"],
                       marks["infos"] - 1, marks["infos"], marks["data_start"], marks["data_start"] + 128,
                       marks["end"] - 1}):
        p.write_bytes(whole[:cut])
        with pytest.raises(ValueError, match="GGUF: "):
            G.GGUFFile(p).close()


# ----------------------------------------------------------------------------------- dequantisation twins
def _same(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, 1.5, 2.5, 3.5), torch.nan_to_num(b, 1.5, 2.5, 3.5))


def _with_scales(raw, bpb, at):
    """Random blocks with the f16 fields at byte offsets ``at`` set to every edge scale in turn."""
    raw = raw.clone().reshape(-1, bpb)
    for i, s in enumerate(gc.EDGE_SCALES):
        for j, a in enumerate(at):
            sv = gc.EDGE_SCALES[(i + 3 * j) % len(gc.EDGE_SCALES)]
            raw[i, a:a + 2] = torch.tensor(np.frombuffer(gc.f16_bytes(sv), dtype=np.uint8).copy())
    return raw.reshape(-1)


@pytest.mark.parametrize("tname", ["F32", "F16", "BF16", "Q8_0", "Q4_0", "Q4_K", "Q6_K"])
def test_dequant_twins_equal_scalar_transcriptions(tname):
    t = gc.TYPE_IDS[tname]
    _, _, bpb = G.GGML_TYPES[t]
    g = torch.Generator().manual_seed(t)
    n = 24 if bpb > 4 else 256
    raw = torch.randint(0, 256, (n * bpb,), generator=g, dtype=torch.uint8)
    at = {"Q8_0": (0,), "Q4_0": (0,), "Q4_K": (0, 2), "Q6_K": (208,)}.get(tname)
    if at:
        raw = _with_scales(raw, bpb, at)
        b = raw.reshape(-1, bpb)
        if tname == "Q4_K":    # the 6-bit sub-scales and mins at their extremes
            b[10, 4:16] = 0
            b[11, 4:16] = 255
            b[12, 4:16] = torch.tensor([63, 0, 63, 0, 0, 63, 0, 63, 0xF0, 0x0F, 0xF0, 0x0F], dtype=torch.uint8)
            b[10:13, 0:2] = torch.tensor(np.frombuffer(gc.f16_bytes(0.0123), dtype=np.uint8).copy())
            b[10:13, 2:4] = torch.tensor(np.frombuffer(gc.f16_bytes(-0.5), dtype=np.uint8).copy())
        if tname == "Q6_K":    # int8 sub-scales -128, 127, 0 and codes 0 / 63
            b[10, 192:208] = 128
            b[11, 192:208] = 127
            b[12, 192:208] = 0
            b[13, 0:192] = 0
            b[14, 0:192] = 255
            b[10:15, 208:210] = torch.tensor(np.frombuffer(gc.f16_bytes(-0.0123), dtype=np.uint8).copy())
    got = G.dequantize(raw, t)
    assert got.dtype == torch.float32
    assert _same(got, gc.scalar_dequant(raw.numpy().tobytes(), t)), tname


def test_q4_0_block_by_hand():
    raw = bytes([0x00, 0x38]) + bytes(((15 - j) << 4) | j for j in range(16))  # d = 0x3800 = 0.5
    want = [(j - 8) / 2 for j in range(16)] + [(7 - j) / 2 for j in range(16)]
    got = G.dequantize(torch.tensor(list(raw), dtype=torch.uint8), G.Q4_0)
    assert got.tolist() == want
    assert gc.scalar_dequant(raw, G.Q4_0).tolist() == want
    codes, d = G.q4_0_split(torch.tensor(list(raw), dtype=torch.uint8))
    assert codes.tolist() == [list(range(16)) + list(range(15, -1, -1))] and d.tolist() == [0.5]


# ----------------------------------------------------------------------------------- Q4_0 host functions
def test_quantize_q4_0_rule():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 256, generator=g)
    w[3, 32:64] = 0.0
    w[5, 0] = 9.0      # the largest magnitude, positive
    w[6, 1] = -9.0     # and negative
    w[7, 0:32] = torch.tensor([2.0, -2.0] + [0.1] * 30)  # a tie: the first one counts
    codes, d = ops.quantize_q4_0(w)
    assert codes.dtype == torch.uint8 and d.dtype == torch.float16 and codes.shape == (64, 256) and d.shape == (64, 8)
    assert int(codes.max()) <= 15
    deq = d.float()[..., None] * (codes.view(64, 8, 32).float() - 8.0)
    err = (w.view(64, 8, 32) - deq).abs()
    assert bool((err <= d.float().abs()[..., None]).all())   # loose: the top code clips (|d| instead of |d| / 2)
    assert float(d[3, 1]) == 0.0 and bool((codes[3, 32:64] == 8).all())
    assert int(codes[5, 0]) == 0 and float(d[5, 0]) == -9.0 / 8 and int(codes[6, 1]) == 0 and float(d[6, 0]) == 9.0 / 8
    assert float(d[7, 0]) == -0.25 and int(codes[7, 0]) == 0 and int(codes[7, 1]) == 15
    # the scalar rule, block by block
    for r, b in ((0, 0), (5, 0), (9, 7)):
        x = w[r, 32 * b:32 * b + 32].numpy()
        i = int(np.argmax(np.abs(x)))
        dd = np.float32(x[i]) / np.float32(-8.0)
        inv = np.float32(1.0) / dd if dd != 0 else np.float32(0.0)
        q = [min(15, int(np.float32(np.float32(v) * inv) + np.float32(8.5))) for v in x]
        assert codes[r, 32 * b:32 * b + 32].tolist() == q
        assert float(d[r, b]) == float(np.float16(dd))


@pytest.mark.parametrize("N,K", [(16, 128), (96, 1408), (48, 384)])
def test_pack_q4_0_round_trip(N, K):
    g = torch.Generator().manual_seed(N + K)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    d = (torch.randn(N, K // 32, generator=g) * 0.01).to(torch.float16)
    d.view(-1)[: len(gc.EDGE_SCALES)] = torch.tensor(gc.EDGE_SCALES).to(torch.float16)
    wq, dw = ops.pack_q4_0(codes, d)
    assert wq.shape == (N // 16, K // 128, 64, 16) and dw.shape == (N // 16, (K // 128 + 1) // 2, 64, 2)
    assert wq.dtype == torch.uint8 and dw.dtype == torch.float16
    rule = (d.float()[..., None] * (codes.view(N, K // 32, 32).float() - 8.0)).to(torch.bfloat16).float().view(N, K)
    got = ops.dequantize_q4_0(wq, dw, N, K)
    assert got.dtype == torch.float32 and torch.equal(got, rule)
    c2, d2 = ops.unpack_q4_0(wq, dw, N, K)
    assert torch.equal(c2, codes) and torch.equal(d2.view(torch.int16), d.view(torch.int16))
    # the documented lane layout, element by element at a few places
    for n, k in ((0, 0), (N - 1, K - 1), (5, 77), (N - 3, K - 40)):
        nb, r, kb, g_, e = n // 16, n % 16, k // 128, (k % 128) // 32, k % 32
        byte = int(wq[nb, kb, 16 * g_ + r, 4 * (e // 8) + e % 4])
        assert (byte >> 4 if e % 8 >= 4 else byte & 15) == int(codes[n, k])
        assert dw[nb, kb // 2, 16 * g_ + r, kb % 2].view(torch.int16) == d[n, k // 32].view(torch.int16)
    pw = ops.PackedWeight.from_q4_0(codes, d)   # the CPU keeps the rule's values dense
    assert pw.kind == "dense" and pw.requested == "q4_0" and torch.equal(pw.dense().float(), rule)
    assert pw.add_z12() is pw and pw.z12 is None and pw.nbytes == N * K * 2


def test_q4_0_bad_shapes_raise():
    c = torch.zeros(16, 96, dtype=torch.uint8)
    with pytest.raises(ValueError, match="K % 128"):
        ops.pack_q4_0(c, torch.zeros(16, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match="N % 16"):
        ops.pack_q4_0(torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(8, 4, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.pack_q4_0(torch.zeros(16, 128, dtype=torch.uint8), torch.zeros(16, 4, dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.PackedWeight.from_dense(torch.zeros(24, 128), "q4_0")
    with pytest.raises(ValueError):
        ops.PackedWeight.from_q4_0(c, torch.zeros(16, 3, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.quantize_q4_0(torch.zeros(4, 40))
    pw = ops.PackedWeight.from_dense(torch.randn(16, 128), "q4_0")
    assert pw.requested == "q4_0" and pw.dense().dtype == torch.bfloat16


def test_pick_gemm_config_q4_suffix():
    assert ops.pick_gemm_config(1, 4096, 4096, "f32", kind="q4_0")[2] == 4
    ops.TUNING_OVERRIDES["4096x4096:f32:b1:q4"] = {"nb": 4, "splitk": 2, "waves": 8}
    try:
        assert ops.pick_gemm_config(1, 4096, 4096, "f32", kind="q4_0") == (4, 2, 8, 4)
        assert ops.pick_gemm_config(1, 4096, 4096, "f32", kind="mxfp4") != (4, 2, 8, 4)
    finally:
        ops.TUNING_OVERRIDES.clear()


# ----------------------------------------------------------------------------------- mapping
def _expected_packed(spec, src, i):
    """Test-side build of layer i: quantise, dequantise by the rule, fuse, interleave."""
    def qd(name):
        w = src[f"model.layers.{i}.{name}.weight"]
        return ops.q4_0_values(*ops.quantize_q4_0(w))

    wqkv = torch.cat([qd("self_attn.q_proj"), qd("self_attn.k_proj"), qd("self_attn.v_proj")], 0)
    gu = ops.interleave_gate_up(qd("mlp.gate_proj"), qd("mlp.up_proj"))
    return wqkv, qd("self_attn.o_proj"), gu, qd("mlp.down_proj")


def test_mapping_from_q4_0_file(tmp_path):
    p = tmp_path / "nsql.gguf"
    src, deq = gc.build_checkpoint(p, "tiny-nsql")
    spec = get_spec("tiny-nsql")
    w = load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    assert w.spec is spec and len(w.layers) == spec.n_layers
    for i, lw in enumerate(w.layers):
        for got, want in zip((lw.wqkv, lw.wo, lw.w_gate_up, lw.w_down), _expected_packed(spec, src, i)):
            assert got.requested == "q4_0" and torch.equal(got.dense(), want)
        assert lw.norms_folded is False
        assert torch.equal(lw.attn_norm, src[f"model.layers.{i}.input_layernorm.weight"].to(torch.bfloat16))
        assert torch.equal(lw.mlp_norm, src[f"model.layers.{i}.post_attention_layernorm.weight"].to(torch.bfloat16))
    assert torch.equal(w.final_norm, src["model.norm.weight"].to(torch.bfloat16))
    assert w.lm_head.requested == "q4_0"
    assert torch.equal(w.lm_head.dense(), ops.q4_0_values(*ops.quantize_q4_0(src["lm_head.weight"])))
    assert torch.equal(w.embed, ops.q4_0_values(*ops.quantize_q4_0(src["model.embed_tokens.weight"])))
    assert w.source["tensor_types"] == {"Q4_0": 16, "F32": 5} and w.source["format"] == "gguf v3"


def _greedy(eng, prompts, n=10):
    return [r.token_ids for r in eng.generate(prompts, SamplingParams(max_tokens=n, ignore_eos=True))]


def test_cpu_engine_matches_state_dict_engine(tmp_path, monkeypatch):
    p = tmp_path / "nsql.gguf"
    _, deq = gc.build_checkpoint(p, "tiny-nsql", seed=3)
    eng = build_engine("tiny-nsql", device="cpu", checkpoint=str(p), dtype="q4_0", max_slots=4, max_model_len=256)
    assert eng.runner.w.layers[0].wqkv.requested == "q4_0" and not eng.runner.fused_norm and not eng.runner.wide_norm
    monkeypatch.setattr(llama_mod, "FOLD_NORMS", False)
    w2 = from_hf_state_dict(get_spec("tiny-nsql"), deq, "cpu", "bf16")
    for a, b in zip(eng.runner.w.layers, w2.layers):
        assert torch.equal(a.wqkv.dense(), b.wqkv.dense()) and torch.equal(a.w_down.dense(), b.w_down.dense())
    eng2 = LLMEngine(ModelRunner(w2, max_slots=4, max_model_len=256), eng.tok, name="tiny-nsql")
    prompts = [[1, 17, 99, 250, 31], [1, 400, 3, 77]]
    got = _greedy(eng, prompts)
    assert got == _greedy(eng2, prompts) and all(len(o) == 10 for o in got)


# ----------------------------------------------------------------------------------- dtype table
def test_one_q8_0_projection_loads_whole_model_as_bf16(tmp_path):
    p = tmp_path / "mixed.gguf"
    _, deq = gc.build_checkpoint(p, "tiny-nsql", types={"blk.1.ffn_down.weight": "Q8_0"})
    with pytest.warns(UserWarning, match=r"blk\.1\.ffn_down\.weight.*Q8_0"):
        w = load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    assert all(pw.requested == "bf16" for lw in w.layers for pw in (lw.wqkv, lw.wo, lw.w_gate_up, lw.w_down))
    assert w.lm_head.requested == "bf16" and w.layers[0].norms_folded == llama_mod.FOLD_NORMS
    want = from_hf_state_dict(get_spec("tiny-nsql"), deq, "cpu", "bf16")
    for a, b in zip(w.layers, want.layers):
        assert torch.equal(a.w_down.dense(), b.w_down.dense()) and torch.equal(a.wqkv.dense(), b.wqkv.dense())


def test_q6_k_output_gives_bf16_head_beside_q4_0_layers(tmp_path):
    p = tmp_path / "q6.gguf"
    _, deq = gc.build_checkpoint(p, "tiny-nsql", output="Q6_K", embd="Q4_K")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w = load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    assert w.layers[0].wqkv.requested == "q4_0" and w.lm_head.requested == "bf16"
    assert torch.equal(w.lm_head.dense(), deq["lm_head.weight"].to(torch.bfloat16))
    assert torch.equal(w.embed, deq["model.embed_tokens.weight"].to(torch.bfloat16))
    assert w.source["tensor_types"] == {"Q4_0": 14, "F32": 5, "Q6_K": 1, "Q4_K": 1}


def test_bf16_dtype_on_q4_0_file_folds_as_today(tmp_path):
    p = tmp_path / "nsql.gguf"
    _, deq = gc.build_checkpoint(p, "tiny-nsql")
    w = load_gguf(str(p), "cpu", "bf16", "tiny-nsql")
    want = from_hf_state_dict(get_spec("tiny-nsql"), deq, "cpu", "bf16")
    assert llama_mod.FOLD_NORMS and w.layers[0].norms_folded
    for a, b in zip(w.layers, want.layers):
        for x, y in ((a.wqkv, b.wqkv), (a.wo, b.wo), (a.w_gate_up, b.w_gate_up), (a.w_down, b.w_down)):
            assert x.requested == "bf16" and torch.equal(x.dense(), y.dense())
        assert torch.equal(a.attn_norm, torch.ones_like(a.attn_norm))
    assert torch.equal(w.lm_head.dense(), want.lm_head.dense()) and torch.equal(w.embed, want.embed)


def test_tied_file_with_rope_freqs_and_other_types(tmp_path):
    p = tmp_path / "l3.gguf"
    src, deq = gc.build_checkpoint(p, "tiny-llama3", embd="Q8_0", rope_freqs=True,
                                   types={"blk.0.attn_v.weight": "Q4_0"})
    w = load_gguf(str(p), "cpu", "q4_0", "tiny-llama3")  # a known spec with rope scaling: rope_freqs is ignored
    spec = get_spec("tiny-llama3")
    assert w.spec is spec and w.layers[0].wqkv.requested == "q4_0"
    assert w.lm_head.requested == "bf16" and torch.equal(w.lm_head.dense(), w.embed)
    assert torch.equal(w.embed, deq["model.embed_tokens.weight"].to(torch.bfloat16))
    for i, lw in enumerate(w.layers):  # 3 query heads over 1 kv head: the un-permute uses each one's own count
        for got, want in zip((lw.wqkv, lw.wo, lw.w_gate_up, lw.w_down), _expected_packed(spec, src, i)):
            assert torch.equal(got.dense(), want)
    p2 = tmp_path / "untied.gguf"
    gc.build_checkpoint(p2, "tiny-nsql", drop=("output.weight",))
    with pytest.raises(ValueError, match="output.weight"):
        load_gguf(str(p2), "cpu", "q4_0", "tiny-nsql")
    p3 = tmp_path / "f16.gguf"
    _, deq3 = gc.build_checkpoint(p3, "tiny-llama3", proj="F16", embd="F16")
    w3 = load_gguf(str(p3), "cpu", "bf16", "tiny-llama3")
    want3 = from_hf_state_dict(spec, deq3, "cpu", "bf16")
    assert torch.equal(w3.layers[1].wqkv.dense(), want3.layers[1].wqkv.dense())


@pytest.mark.parametrize("key,val,field", [
    ("llama.block_count", (gc.U32, 3), "llama.block_count"),
    ("llama.embedding_length", (gc.U32, 512), "llama.embedding_length"),
    ("llama.feed_forward_length", (gc.U32, 1024), "llama.feed_forward_length"),
    ("llama.attention.head_count", (gc.U32, 4), "llama.attention.head_count"),
    ("llama.attention.head_count_kv", (gc.U32, 1), "llama.attention.head_count_kv"),
    ("llama.attention.key_length", (gc.U32, 64), "llama.attention.key_length"),
    ("llama.attention.layer_norm_rms_epsilon", (gc.F32V, 1e-6), "llama.attention.layer_norm_rms_epsilon"),
    ("llama.rope.freq_base", (gc.F32V, 500000.0), "llama.rope.freq_base"),
])
def test_dimension_mismatch_names_its_key(tmp_path, key, val, field):
    p = tmp_path / "bad.gguf"
    gc.build_checkpoint(p, "tiny-nsql", meta={key: val})
    with pytest.raises(ValueError, match=field.replace(".", r"\.")):
        load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")


def test_model_level_refusals(tmp_path):
    p = tmp_path / "bad.gguf"
    gc.build_checkpoint(p, "tiny-nsql", vocab=544)
    with pytest.raises(ValueError, match=r"token_embd\.weight.*vocab_size = 544"):   # vocab = rows of token_embd
        load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    gc.build_checkpoint(p, "tiny-nsql", arch="qwen2")
    with pytest.raises(ValueError, match="general.architecture.*qwen2"):
        load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    gc.build_checkpoint(p, "tiny-nsql", drop=("blk.1.ffn_up.weight",))
    with pytest.raises(ValueError, match=r"required tensor 'blk\.1\.ffn_up\.weight' is missing"):
        load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    gc.build_checkpoint(p, "tiny-nsql", meta={"llama.block_count": None})
    with pytest.raises(ValueError, match=r"llama\.block_count.*missing"):
        load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")


def test_unknown_name_builds_spec_from_metadata(tmp_path):
    p = tmp_path / "u.gguf"
    gc.build_checkpoint(p, "tiny-nsql", extra_metadata=[("tokenizer.ggml.bos_token_id", gc.U32, 7),
                                                        ("tokenizer.ggml.eos_token_id", gc.U32, 9)])
    w = load_gguf(str(p), "cpu", "q4_0", "somebody-elses-model")
    s, t = w.spec, get_spec("tiny-nsql")
    assert s.name == "somebody-elses-model" and s.template == "raw" and not s.tie_embeddings
    assert (s.vocab_size, s.hidden, s.n_layers, s.n_heads, s.n_kv_heads, s.ffn, s.head_dim, s.max_position) == (
        t.vocab_size, t.hidden, t.n_layers, t.n_heads, t.n_kv_heads, t.ffn, t.head_dim, t.max_position)
    assert s.rope_theta == t.rope_theta and abs(s.rms_eps - t.rms_eps) < 1e-9 and s.rope_scaling is None
    assert s.bos_id == 7 and s.eos_ids == (9,)
    assert w.layers[0].wqkv.requested == "q4_0"
    p2 = tmp_path / "u3.gguf"
    gc.build_checkpoint(p2, "tiny-llama3", rope_freqs=True)
    with pytest.raises(ValueError, match=r"rope_freqs\.weight"):
        load_gguf(str(p2), "cpu", "q4_0", "somebody-elses-model")


# ----------------------------------------------------------------------------------- tokenizer
def test_tokenizer_from_gpt2_metadata(tmp_path):
    p = tmp_path / "t.gguf"
    md = gc.gpt2_vocab_metadata()
    gc.build_checkpoint(p, "tiny-nsql", extra_metadata=md)
    eng = build_engine("tiny-nsql", device="cpu", checkpoint=str(p), dtype="q4_0", max_slots=2, max_model_len=128)
    tok = eng.tok
    assert isinstance(tok, tok_mod.HFTokenizer)
    text = "hello world, 42 + x!"
    ids = tok.encode(text, add_bos=False)
    tokens = md[2][2][1]
    assert ids[0] == tokens.index("hello") and tokens.index("Ġwor") in ids and len(ids) < len(text)
    assert tok.decode(ids) == text
    assert tok.encode(text)[0] == get_spec("tiny-nsql").bos_id


def test_tokenizer_from_llama_metadata(tmp_path):
    p = tmp_path / "t.gguf"
    md = gc.llama_vocab_metadata()
    gc.build_checkpoint(p, "tiny-nsql", extra_metadata=md)
    w = load_gguf(str(p), "cpu", "q4_0", "tiny-nsql")
    tok = tokenizer_for(w.spec, str(p), w.source["tokenizer"])
    assert isinstance(tok, tok_mod.HFTokenizer)
    text = "hello world 42"
    ids = tok.encode(text, add_bos=False)
    tokens = md[1][2][1]
    assert tokens.index("▁hello") in ids and tokens.index("<0x34>") in ids   # a scored piece, and byte fallback
    assert tok.decode(ids) == text


def test_tokenizer_failure_falls_back_to_bytes(tmp_path, monkeypatch):
    import transformers.integrations.ggml as tg

    p = tmp_path / "t.gguf"
    gc.build_checkpoint(p, "tiny-nsql", extra_metadata=gc.gpt2_vocab_metadata())

    def boom(*a, **k):
        raise RuntimeError("no converter today")

    monkeypatch.setattr(tg, "convert_gguf_tokenizer", boom)
    with pytest.warns(UserWarning, match="byte tokenizer"):
        eng = build_engine("tiny-nsql", device="cpu", checkpoint=str(p), dtype="q4_0", max_slots=2, max_model_len=128)
    assert isinstance(eng.tok, tok_mod.ByteTokenizer)
    (tmp_path / "sub").mkdir()   # no vocabulary at all: the byte tokenizer, silently
    p2 = tmp_path / "sub" / "blob"
    gc.build_checkpoint(p2, "tiny-nsql")
    w = load_gguf(str(p2), "cpu", "q4_0", "tiny-nsql")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert isinstance(tokenizer_for(w.spec, str(p2), w.source["tokenizer"]), tok_mod.ByteTokenizer)


# ----------------------------------------------------------------------------------- settings, service, health
def test_settings_and_service_plumbing(tmp_path, monkeypatch):
    from llm_based_apache_spark_optimization_amd import client as client_mod
    from llm_based_apache_spark_optimization_amd.serving import service

    monkeypatch.setenv("LSA_DTYPE", "q4_0")
    monkeypatch.setenv("LSA_EXPLAIN_DTYPE", "q4_0")
    monkeypatch.setenv("LSA_CHECKPOINT_DIR", "/models/nsql.gguf")
    monkeypatch.setenv("LSA_EXPLAIN_CHECKPOINT_DIR", "/models/llama-blob")
    s = Settings()
    assert (s.dtype, s.explain_dtype, s.checkpoint_dir, s.explain_checkpoint_dir) == (
        "q4_0", "q4_0", "/models/nsql.gguf", "/models/llama-blob")
    import argparse

    ap = argparse.ArgumentParser()
    Settings.add_cli(ap)
    s2 = Settings.from_cli(ap.parse_args(["--dtype", "q4_0", "--explain-checkpoint-dir", "/x/y"]))
    assert s2.dtype == "q4_0" and s2.explain_checkpoint_dir == "/x/y"
    seen = {}
    import llm_based_apache_spark_optimization_amd.engine as engine_pkg

    class _Eng:
        runner = type("R", (), {"spec_min_accept": 0})()

    def fake_build(model, checkpoint=None, dtype=None, **kw):
        seen[model] = (checkpoint, dtype)
        return _Eng()

    monkeypatch.setattr(engine_pkg, "build_engine", fake_build)
    build = service.engine_factory(s)
    build(s.nl2sql_model)
    build(s.explain_model)
    build("mistral")
    assert seen == {s.nl2sql_model: ("/models/nsql.gguf", "q4_0"), s.explain_model: ("/models/llama-blob", "q4_0"),
                    "mistral": (None, "q4_0")}
    # health: the weight kind and the file's tensor count per type
    p = tmp_path / "h.gguf"
    gc.build_checkpoint(p, "tiny-nsql", output="Q6_K")
    eng = build_engine("tiny-nsql", device="cpu", checkpoint=str(p), dtype="q4_0", max_slots=2, max_model_len=128)
    h = client_mod._weights_health(eng)
    assert h == {"weight_kind": "q4_0", "checkpoint_format": "gguf v3",
                 "gguf_tensor_types": {"Q4_0": 15, "F32": 5, "Q6_K": 1}}
    rnd = build_engine("tiny-nsql", device="cpu", dtype="q4_0", max_slots=2, max_model_len=128)
    assert client_mod._weights_health(rnd) == {"weight_kind": "q4_0"} and not rnd.runner.w.layers[0].norms_folded
    assert rnd.runner.w.lm_head.requested == "q4_0" and not rnd.runner.spec_supported()


def test_safetensors_directory_path_unchanged(tmp_path):
    """A directory still goes to the safetensors loader (which needs its config.json); a non-GGUF file does too."""
    with pytest.raises(FileNotFoundError):
        build_engine("tiny-nsql", device="cpu", checkpoint=str(tmp_path), max_slots=2, max_model_len=128)
    assert not G.is_gguf(str(tmp_path)) and not G.is_gguf(str(tmp_path / "missing"))
