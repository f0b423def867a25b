"""Regex-constrained decoding on the CPU: the regex -> byte DFA compiler (engine/guided.py), the tokenizers' byte
table, the host twin of the mask kernel (ops.reference.dfa_mask), the engine path (tiny model, ByteTokenizer) and the
service switch (Pipeline.nl2sql with sql_guided)."""
import itertools
import json
import random
import re

import numpy as np
import pytest
import torch

from llm_based_apache_spark_optimization_amd import prompts
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.guided import DEAD, MAX_TABLE, compile_regex
from llm_based_apache_spark_optimization_amd.models.tokenizer import ByteTokenizer, HFTokenizer, token_bytes
from llm_based_apache_spark_optimization_amd.ops import reference as ref

BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"

# (pattern, strings it was written to accept): together they cover every supported construct
PATTERNS = [
    (r"abc", [b"abc"]),
    (r"a|bc|", [b"a", b"bc", b""]),
    (r"(ab)*c+d?", [b"c", b"ababccd"]),
    (r"[a-c]{2,4}", [b"ab", b"abca"]),
    (r"x{2}", [b"xx"]),
    (r"x{2,}y", [b"xxy", b"xxxxxy"]),
    (r"a{0}b", [b"b"]),
    (r"(a?){3}b", [b"b", b"aaab"]),
    (r"\d{3}-\w+\s", [b"123-ab_9 ", b"000-x\n"]),
    (r"\t\n\r", [b"\t\n\r"]),
    (r"\(\)\.\*\\", [b"().*\\"]),
    (r"a.b", [b"a.b", b"axb"]),
    (r"[^a-c\n]x*", [b"dxx", b"\xffx"]),
    (r"[\d\-_]+", [b"1-2_3"]),
    (r"[]a]+", [b"]a]"]),
    (r"[a\]b-]+", [b"a]-b"]),
    (r"(a|b)*abb", [b"abb", b"babababb"]),
    ("(é|ü)+z", ["éüz".encode()]),
    ("naïve", ["naïve".encode()]),
    (r"(?i)[^s]t", [b"AT", b"xt"]),
    (r"(?i)ab[c-e]+", [b"ABCDE", b"abE"]),
    (BOUNDED, [b"SELECT abc from temp_view;", b"wItH c FROM TEMP_VIEW;"]),
    (prompts.SQL_STATEMENT_REGEX, [b"SELECT * FROM temp_view;", b"with\nx as (select 1) select 2;"]),
]


@pytest.mark.parametrize("pattern,accepts", PATTERNS, ids=[p for p, _ in PATTERNS])
def test_compiler_matches_re_fullmatch(pattern, accepts):
    dfa = compile_regex(pattern)
    rx = re.compile(pattern.encode("utf-8"))
    assert dfa.n_states * dfa.n_classes <= MAX_TABLE and dfa.trans.dtype == np.uint16
    for s in accepts:
        assert rx.fullmatch(s) and dfa.fullmatch(s), s
    rng = random.Random(pattern)
    alphabet = sorted(set(pattern.encode("utf-8")) | set(b"".join(accepts)) | set(b"abx1 \n"))
    pool = list(accepts)
    for _ in range(400):
        if rng.random() < 0.5:  # a mutation of an accepted string: near misses
            s = bytearray(rng.choice(pool))
            for _ in range(rng.randint(0, 2)):
                k = rng.randint(0, len(s))
                if s and rng.random() < 0.5:
                    del s[min(k, len(s) - 1)]
                else:
                    s.insert(k, rng.choice(alphabet))
            s = bytes(s)
        else:
            s = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 8)))
        assert dfa.fullmatch(s) == (rx.fullmatch(s) is not None), (pattern, s)


@pytest.mark.parametrize("pattern,alphabet", [(r"(ab)*c+d?", b"abcd"), (r"a{2,3}b|ba", b"ab"), (r"[ab]c*a", b"abc")])
def test_liveness_against_brute_force(pattern, alphabet):
    """After every prefix, a byte leads to a state other than DEAD exactly when some completion matches (all strings up
    to length 6 enumerated)."""
    rx = re.compile(pattern.encode())
    dfa = compile_regex(pattern)
    words = [bytes(w) for n in range(7) for w in itertools.product(alphabet, repeat=n)]
    matches = {w for w in words if rx.fullmatch(w)}
    viable = {m[:k] for m in matches for k in range(len(m) + 1)}  # prefixes with a matching completion (<= 6 bytes)
    # every pattern here completes within 2 bytes from any live prefix, so prefixes up to 3 bytes plus one byte are exact
    for w in (w for w in words if len(w) <= 3):
        st = dfa.walk(dfa.start, w)
        assert (st != DEAD) == (w in viable), w
        if st != DEAD:
            for byte in range(256):
                nxt = dfa.walk(st, bytes([byte]))
                assert (nxt != DEAD) == (w + bytes([byte]) in viable), (w, byte)
            assert dfa.accepts(st) == (w in matches)


@pytest.mark.parametrize("pattern", [r"a(?=b)", r"a(?!b)", r"(?<=a)b", r"(a)\1", r"a*?", r"a+?", r"a++", r"(?:a)",
                                     r"a(?i)b", r"^a", r"a$", r"\bword", r"\D", r"(a", r"a)", r"[a", r"a{2,1}", r"*a",
                                     r"a**", r"[é]", "\\"])
def test_unsupported_syntax_raises(pattern):
    with pytest.raises(ValueError, match="position"):
        compile_regex(pattern)


def test_table_size_rule():
    with pytest.raises(ValueError, match="pattern too large"):
        compile_regex(r"(abcdefghijklmnopqrstuvwxyz0123456789){40}")  # 1441 states x 37 classes
    with pytest.raises(ValueError, match="pattern too large"):
        compile_regex(r".*a.{15}")  # 2^16 subset states
    at_limit = compile_regex(r"(abcdefghijklmnopqrstuvwxyz01234){33}")  # 1024 states x 32 classes
    assert at_limit.n_states * at_limit.n_classes == MAX_TABLE
    small = compile_regex(r"[a-z]{1,200}[0-9]{1,200}")  # many states, three classes: fits
    assert small.n_states * small.n_classes <= MAX_TABLE and small.fullmatch(b"a" * 200 + b"7")
    assert compile_regex(r"abc") is compile_regex(r"abc")  # cached by pattern string


# ------------------------------------------------------------------------------------------- token byte table
def test_token_bytes_byte_tokenizer():
    tok = ByteTokenizer(512, bos_id=1, eos_ids=(2,), offset=3, specials=("<|eot_id|>",))
    off, blob = token_bytes(tok, 520)
    assert off.dtype == np.int32 and blob.dtype == np.uint8 and off.shape == (521,) and off[-1] == blob.shape[0] == 256
    for i in range(520):
        b = blob[off[i]:off[i + 1]].tobytes()
        assert b == (bytes([i - 3]) if 3 <= i < 259 else b""), i  # BOS, EOS, specials, padding: zero bytes


def test_token_bytes_byte_level_tokenizer_json(tmp_path):
    pytest.importorskip("tokenizers")
    from llm_based_apache_spark_optimization_amd.models.tokenizer import _gpt2_unicode_to_byte

    b2u = {b: u for u, b in _gpt2_unicode_to_byte().items()}
    enc = lambda bs: "".join(b2u[b] for b in bs)  # noqa: E731
    pieces = [bytes([b]) for b in range(256)] + [b" select", b"from", "é".encode(), b" \n"]
    vocab = {enc(p): i for i, p in enumerate(pieces)}
    cfg = {"version": "1.0", "truncation": None, "padding": None,
           "added_tokens": [{"id": len(pieces), "content": "<|end|>", "single_word": False, "lstrip": False,
                             "rstrip": False, "normalized": False, "special": True}],
           "normalizer": None,
           "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
           "post_processor": None,
           "decoder": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
           "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": None,
                     "end_of_word_suffix": None, "fuse_unk": False, "byte_fallback": False, "vocab": vocab,
                     "merges": []}}
    (tmp_path / "tokenizer.json").write_text(json.dumps(cfg))
    tok = HFTokenizer(str(tmp_path), bos_id=len(pieces), eos_ids=(len(pieces),))
    off, blob = token_bytes(tok)
    assert off.shape == (len(pieces) + 2,)
    for i, p in enumerate(pieces):
        assert blob[off[i]:off[i + 1]].tobytes() == p, i
    assert off[len(pieces) + 1] == off[len(pieces)]  # the added special: zero bytes
    assert blob[off[258]:off[259]].tobytes() == "é".encode()


def test_token_bytes_sentencepiece_style_tokenizer_json(tmp_path):
    pytest.importorskip("tokenizers")
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "<0x0A>": 3, "<0xC3>": 4, "▁select": 5, "from": 6, "▁": 7}
    cfg = {"version": "1.0", "truncation": None, "padding": None,
           "added_tokens": [{"id": i, "content": c, "single_word": False, "lstrip": False, "rstrip": False,
                             "normalized": False, "special": True} for i, c in enumerate(("<unk>", "<s>", "</s>"))],
           "normalizer": None, "pre_tokenizer": None, "post_processor": None, "decoder": None,
           "model": {"type": "BPE", "dropout": None, "unk_token": "<unk>", "continuing_subword_prefix": None,
                     "end_of_word_suffix": None, "fuse_unk": True, "byte_fallback": True, "vocab": vocab, "merges": []}}
    (tmp_path / "tokenizer.json").write_text(json.dumps(cfg))
    off, blob = token_bytes(HFTokenizer(str(tmp_path), bos_id=1, eos_ids=(2,)))
    got = [blob[off[i]:off[i + 1]].tobytes() for i in range(8)]
    assert got == [b"", b"", b"", b"\n", b"\xc3", b" select", b"from", b" "]


# ------------------------------------------------------------------------------------------- reference mask
def _tables(dfas, slots):
    """Device-layout tables of ``dfas`` (None = an unconstrained row) for ``slots`` rows."""
    cls = torch.zeros(slots, 256, dtype=torch.uint8)
    trans = torch.full((slots, MAX_TABLE), -1, dtype=torch.int16)
    accept = torch.zeros(slots, MAX_TABLE, dtype=torch.uint8)
    dim = torch.zeros(slots, 2, dtype=torch.int32)
    on = torch.zeros(slots, dtype=torch.int32)
    for r, d in enumerate(dfas):
        if d is None:
            continue
        sc = d.n_states * d.n_classes
        cls[r] = torch.from_numpy(d.cls)
        trans[r, :sc] = torch.from_numpy(d.trans.view("int16"))
        accept[r, : d.n_states] = torch.from_numpy(d.accept)
        dim[r] = torch.tensor([d.n_states, d.n_classes], dtype=torch.int32)
        on[r] = 1
    return cls, trans, accept, dim, on


def test_ref_dfa_mask_against_python_loop():
    rng = random.Random(5)
    dfa = compile_regex(r"(ab|c)+(d?;)?")
    words = [b"", b"a", b"b", b"c", b"d", b";", b"ab", b"abc", b"cab", b"d;", b"cd;", b"ba", b"c" * 32, b"c" * 33,
             b"abd", b"cc;", b"x", b"", b";;"]
    words += [bytes(rng.choice(b"abcd;") for _ in range(rng.randint(1, 5))) for _ in range(60)]
    V = len(words)
    eos = [0, 17]  # two zero-byte ids
    lens = [len(w) for w in words]
    off = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)
    blob = torch.tensor(list(b"".join(words)), dtype=torch.uint8)
    cls, trans, accept, dim, on = _tables([dfa, dfa, None, dfa], 4)
    mid = dfa.walk(dfa.start, b"ab")      # accepting: EOS allowed
    g_state = torch.tensor([[dfa.start, dfa.start], [mid, mid], [0, 0], [dfa.start, dfa.start]], dtype=torch.int32)
    g_base = torch.zeros(4, dtype=torch.int32)
    gen_len = torch.zeros(4, dtype=torch.int32)
    finished = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    logits = torch.randn(4, V)
    want = logits.clone()
    for b, st in ((0, dfa.start), (1, mid)):
        for t, w in enumerate(words):
            ok = 1 <= len(w) <= 32 and dfa.walk(st, w) != DEAD
            if t in eos:
                ok = dfa.accepts(st)
            if not ok:
                want[b, t] = float("-inf")
    ref.dfa_mask(logits, off, blob, cls, trans, accept, dim, on, g_state, g_base, gen_len,
                 torch.zeros(4, dtype=torch.int32), finished, torch.tensor(eos, dtype=torch.int32))
    assert torch.equal(logits, want)  # rows 2 (g_on = 0) and 3 (finished) untouched
    assert (logits[0, eos] == float("-inf")).all() and torch.isfinite(logits[1, eos]).all()
    # lazy advance: the committed token's bytes move the state into the other slot
    t_cd = words.index(b"cd;")
    gen_len[0] = 1
    logits = torch.zeros(4, V)
    ref.dfa_mask(logits, off, blob, cls, trans, accept, dim, on, g_state, g_base, gen_len,
                 torch.tensor([t_cd, 0, 0, 0], dtype=torch.int32), finished, torch.tensor(eos, dtype=torch.int32))
    assert int(g_state[0, 1]) == dfa.walk(dfa.start, b"cd;") and int(g_state[0, 0]) == dfa.start
    assert torch.isfinite(logits[0]).nonzero().flatten().tolist() == eos  # after the ';' only EOS remains


# ------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def engines():
    kw = dict(device="cpu", max_slots=4, max_model_len=512)
    return build_engine("tiny-nsql", guided=True, **kw), build_engine("tiny-nsql", **kw)


PROMPT = [1] + list(range(40, 70))


@pytest.mark.parametrize("extra", [dict(), dict(temperature=0.8, seed=11), dict(repeat_penalty=1.3)],
                         ids=["greedy", "sampled", "repeat_penalty"])
def test_engine_output_full_matches(engines, extra):
    eng, _ = engines
    res = eng.generate([PROMPT], SamplingParams(max_tokens=64, regex=BOUNDED, **extra))[0]
    assert res.done_reason == "stop" and res.token_ids[-1] in eng.runner.eos_list
    assert re.fullmatch(BOUNDED, res.text), res.text
    assert eng.stats["guided_requests"] >= 1 and eng.stats["guided_steps"] >= len(res.token_ids) - 1


def test_unconstrained_request_in_a_guided_batch_is_bit_equal(engines):
    eng, plain = engines
    sp = SamplingParams(max_tokens=40)
    a = eng.add_request(PROMPT, SamplingParams(max_tokens=64, regex=BOUNDED))
    b = eng.add_request(PROMPT[:20], sp)
    eng.run_until_done([a, b])
    c = plain.add_request(PROMPT, SamplingParams(max_tokens=27))  # the same batch shape on the plain engine
    d = plain.add_request(PROMPT[:20], sp)
    plain.run_until_done([c, d])
    assert b.output_ids == d.output_ids and len(b.output_ids) > 1
    assert re.fullmatch(BOUNDED, eng.result(a).text)
    assert "guided_steps" not in plain.stats and not plain.runner.guided


def test_preempted_constrained_request_resumes_its_dfa_state():
    """Three constrained requests whose outputs outgrow a 8-block arena: the youngest is preempted, re-admitted with
    the DFA state its generated bytes reached, and produces the tokens of its solo run."""
    pattern = r"[a-d ]{140,150};"
    prompts_ = [[1] + list(range(3 + k, 40 + k)) for k in range(3)]
    eng = build_engine("tiny-nsql", device="cpu", max_slots=3, max_model_len=512, num_kv_blocks=9, guided=True)
    sp = SamplingParams(max_tokens=200, regex=pattern)
    solo = [eng.generate([p], sp)[0].token_ids for p in prompts_]
    reqs = [eng.add_request(p, sp) for p in prompts_]
    eng.run_until_done(reqs)
    assert eng.stats["preempted"] >= 1 and any(q.preemptions for q in reqs)
    assert [q.output_ids for q in reqs] == solo
    for q in reqs:
        assert re.fullmatch(pattern, eng.result(q).text) and q.output_ids[-1] in eng.runner.eos_list


def test_constrained_request_never_speculates():
    eng = build_engine("tiny-nsql", device="cpu", max_slots=4, max_model_len=512, guided=True, spec_tokens=3)
    assert eng.runner.spec_supported()
    res = eng.generate([PROMPT], SamplingParams(max_tokens=64, regex=BOUNDED))[0]
    assert re.fullmatch(BOUNDED, res.text) and eng.stats["spec_steps"] == 0
    eng.generate([PROMPT], SamplingParams(max_tokens=16))
    assert eng.stats["spec_steps"] > 0  # the same engine does speculate for an unconstrained request


def test_rejected_requests(engines):
    eng, plain = engines
    with pytest.raises(ValueError, match="guided"):
        plain.add_request(PROMPT, SamplingParams(regex=BOUNDED))
    with pytest.raises(ValueError, match="ignore_eos"):
        eng.add_request(PROMPT, SamplingParams(regex=BOUNDED, ignore_eos=True))
    with pytest.raises(ValueError, match="position"):
        eng.add_request(PROMPT, SamplingParams(regex=r"a(?=b)"))
    assert not eng.has_work() and not plain.has_work()
    assert SamplingParams.from_ollama_options({"regex": BOUNDED}).regex == BOUNDED
    assert SamplingParams.from_ollama_options({}).regex is None


# ------------------------------------------------------------------------------------------- service
def test_pipeline_nl2sql_sql_guided(engines):
    from llm_based_apache_spark_optimization_amd.client import EngineService, FakeBackend
    from llm_based_apache_spark_optimization_amd.serving.pipeline import Pipeline

    s = Settings()
    s.engine, s.guided, s.sql_guided = "fake", True, True
    fake = FakeBackend()
    pipe = Pipeline(fake, None, None, s)
    res = pipe.nl2sql("a (int)", "all rows")
    assert fake.calls[-1]["options"] == {"regex": prompts.SQL_STATEMENT_REGEX}
    assert fake.calls[-1]["system"] == prompts.nl2sql_system("a (int)")  # the prompt is untouched
    assert compile_regex(prompts.SQL_STATEMENT_REGEX).fullmatch(res.response.encode())
    pipe.nl2sql("a (int)", "all rows", {"regex": BOUNDED, "top_k": 5})
    assert fake.calls[-1]["options"] == {"regex": BOUNDED, "top_k": 5}  # the caller's pattern is left alone
    pipe.explain("boom")
    assert not (fake.calls[-1]["options"] or {}).get("regex")  # /explain_error is never constrained
    s.sql_guided = False
    Pipeline(fake, None, None, s).nl2sql("a (int)", "all rows")
    assert fake.calls[-1]["options"] is None
    s.engine, s.guided, s.sql_guided = "hip", False, True
    with pytest.raises(ValueError, match="guided"):
        Pipeline(fake, None, None, s)
    # through a real (CPU) engine: the option reaches the sampler and the answer is one statement
    s.engine, s.guided, s.sql_guided, s.nl2sql_model = "fake", True, True, "tiny-nsql"
    svc = EngineService(lambda model: engines[0], defaults={"num_predict": 64})
    try:
        out = Pipeline(svc, None, None, s).nl2sql("a (int)", "all rows", {"regex": BOUNDED})
        assert re.fullmatch(BOUNDED, out.response) and out.done_reason == "stop"
        out = Pipeline(svc, None, None, s).nl2sql("a (int)", "all rows", {"num_predict": 48})
        assert re.match(r"(?i)(select|with)\s[^;`]*;?$", out.response), out.response
        if out.done_reason == "stop":
            assert re.fullmatch(prompts.SQL_STATEMENT_REGEX, out.response)
    finally:
        for lp in svc._loops.values():
            lp.close()


def test_http_rejects_bad_constraints_with_400(engines, tmp_path):
    from fastapi.testclient import TestClient

    from llm_based_apache_spark_optimization_amd.client import EngineService
    from llm_based_apache_spark_optimization_amd.serving.fastapi_app import create_app
    from llm_based_apache_spark_optimization_amd.serving.service import make_context

    s = Settings()
    s.engine, s.input_dir, s.output_dir = "fake", str(tmp_path), str(tmp_path)
    s.history_dsn = "sqlite:///" + str(tmp_path / "h.db")
    svc = EngineService(lambda model: engines[0] if model == "guided" else engines[1], defaults={"num_predict": 32})
    try:
        c = TestClient(create_app(make_context(s, backend=svc)))
        r = c.post("/api/generate", json={"model": "plain", "prompt": "hi", "options": {"regex": "a+"}})
        assert r.status_code == 400 and "guided" in r.json()["detail"]
        r = c.post("/api/generate", json={"model": "guided", "prompt": "hi", "options": {"regex": "a(?=b)"}})
        assert r.status_code == 400 and "position 1" in r.json()["detail"]
        r = c.post("/api/generate", json={"model": "guided", "prompt": "hi", "options": {"regex": "(ab){1,3};"}})
        assert r.status_code == 200 and re.fullmatch("(ab){1,3};", r.json()["response"])
        assert c.get("/health").json()["engines"]["guided"]["guided_requests"] >= 1
        assert "lsa_guided_steps_total" in c.get("/metrics").text
    finally:
        for lp in svc._loops.values():
            lp.close()
