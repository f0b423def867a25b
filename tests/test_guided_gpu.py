"""Regex-constrained decoding on the GPU: the mask kernel (csrc/kernels/guided.hip) against its host twin
(ops.reference.dfa_mask) -- exact: allowed logits bit-unchanged, the others -inf, both state slots equal -- and the
engine path with captured graphs."""
import itertools
import random
import re

import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.engine.guided import DEAD, MAX_TABLE, compile_regex
from llm_based_apache_spark_optimization_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BOUNDED = r"(?i)(select|with) [a-c]{1,6} from temp_view;"
ALPHA = b"abcdefghijklmnopqrstuvwxyz01234"
TINY = r"(ab|c)+(d?;)?"
LIMIT = r"(abcdefghijklmnopqrstuvwxyz01234){33}"  # 1024 states x 32 classes = the table-size limit
EOS = [5, 40]  # id 5 has zero bytes, id 40 has bytes: an EOS id is ruled by accept[cur] alone


def _vocab(V):
    """Synthetic token table: lengths 0, 1, 2, 7, 32 and 33, tokens that die on their last byte, for both DFAs."""
    tail = ALPHA[3:] + ALPHA[:3]  # what follows "...abc" in LIMIT
    words = [b"", b"a", b"ab", b"c", b"abc", b"", b"abababc", b"c" * 32, b"c" * 33, b"abx", b"cc;x", b"d;", b";",
             b"cd;", b"d", b"de", tail[:7], (tail + tail)[:32], (tail + tail)[:33], b"defghiX", b"dx", b"x", b"ab;",
             b"abd", b"cab", b"k"]
    rng = random.Random(V)
    while len(words) < V:
        k = rng.random()
        if k < 0.05:
            words.append(b"")
        elif k < 0.5:
            words.append(bytes(rng.choice(b"abcd;x") for _ in range(rng.randint(1, 6))))
        else:  # runs of the LIMIT cycle from a random phase, sometimes broken at the end
            p, n = rng.randrange(31), rng.randint(1, 12)
            w = (ALPHA * 2)[p:p + n]
            words.append(w + b"#" if rng.random() < 0.2 else w)
    lens = [len(w) for w in words]
    off = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)
    blob = torch.tensor(list(b"".join(words)), dtype=torch.uint8)
    return words, off, blob


def _tables(dfas, slots):
    cls = torch.zeros(slots, 256, dtype=torch.uint8)
    trans = torch.full((slots, MAX_TABLE), -1, dtype=torch.int16)
    accept = torch.zeros(slots, MAX_TABLE, dtype=torch.uint8)
    dim = torch.zeros(slots, 2, dtype=torch.int32)
    for r, d in enumerate(dfas):
        sc = d.n_states * d.n_classes
        cls[r] = torch.from_numpy(d.cls)
        trans[r, :sc] = torch.from_numpy(d.trans.view("int16"))
        accept[r, : d.n_states] = torch.from_numpy(d.accept)
        dim[r] = torch.tensor([d.n_states, d.n_classes], dtype=torch.int32)
    return cls, trans, accept, dim


@pytest.fixture(scope="module")
def dfas():
    tiny, limit = compile_regex(TINY), compile_regex(LIMIT)
    assert limit.n_states * limit.n_classes == MAX_TABLE
    return tiny, limit


@pytest.mark.parametrize("V", [5000, 2048])  # three chunks with a partial last one; exactly one chunk
def test_dfa_mask_kernel_matches_reference(gpu, dfas, V):
    tiny, limit = dfas
    words, off, blob = _vocab(V)
    tok = {w: i for i, w in reversed(list(enumerate(words)))}  # first id of each word
    mid = limit.walk(limit.start, ALPHA * 5 + b"abc")
    assert mid != DEAD and not limit.accepts(mid)
    # rows: tiny DFA in its start state | limit DFA in a mid state | g_on = 0 | finished
    host = dict(zip(("cls", "trans", "accept", "dim"), _tables([tiny, limit, tiny, tiny], 4)))
    host.update(on=torch.tensor([1, 1, 0, 1], dtype=torch.int32), base=torch.zeros(4, dtype=torch.int32),
                state=torch.tensor([[tiny.start] * 2, [mid] * 2, [0, 0], [tiny.start] * 2], dtype=torch.int32),
                off=off, blob=blob, eos=torch.tensor(EOS, dtype=torch.int32))
    dev = {k: v.to(gpu) for k, v in host.items()}
    finished = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    gen = torch.Generator().manual_seed(V)

    def launch(gen_len, input_ids):
        logits = torch.randn(4, V, generator=gen)
        gl, ii = torch.tensor(gen_len, dtype=torch.int32), torch.tensor(input_ids, dtype=torch.int32)
        want = logits.clone()
        ref.dfa_mask(want, host["off"], host["blob"], host["cls"], host["trans"], host["accept"], host["dim"],
                     host["on"], host["state"], host["base"], gl, ii, finished, host["eos"])
        outs = []
        for _ in range(2):  # the second launch repeats the first bit for bit (the state slots are already advanced)
            got = logits.to(gpu)
            ops.dfa_mask(got, dev["off"], dev["blob"], dev["cls"], dev["trans"], dev["accept"], dev["dim"], dev["on"],
                         dev["state"], dev["base"], gl.to(gpu), ii.to(gpu), finished.to(gpu), dev["eos"])
            outs.append(got.cpu())
        assert torch.equal(outs[0], want) and torch.equal(outs[1], want)  # allowed: bit-unchanged; others: -inf
        assert torch.equal(dev["state"].cpu(), host["state"])
        assert torch.equal(want[2:], logits[2:])  # g_on = 0 and finished rows: untouched
        return want

    # launch 1: n = 0 = g_base, both rows read the state the admission wrote
    out = launch([0, 0, 0, 0], [0, 0, 0, 0])
    live0 = {t for t in range(V) if torch.isfinite(out[0, t])}
    assert live0 == {t for t, w in enumerate(words) if t not in EOS and 1 <= len(w) <= 32
                     and tiny.walk(tiny.start, w) != DEAD}
    assert tok[b"c" * 32] in live0 and tok[b"c" * 33] not in live0 and tok[b"abx"] not in live0
    live1 = {t for t in range(V) if torch.isfinite(out[1, t])}
    tail = ALPHA[3:] + ALPHA[:3]
    assert {tok[b"d"], tok[b"de"], tok[tail[:7]], tok[(tail + tail)[:32]]} <= live1
    assert not {tok[(tail + tail)[:33]], tok[b"defghiX"], tok[b"dx"], tok[b""], *EOS} & live1
    # launch 2: the commit wrote "ab" / a 7-byte token; the kernel advances into slot 1.  Row 0 is now accepting
    out = launch([1, 1, 0, 0], [tok[b"ab"], tok[tail[:7]], 0, 0])
    s0, s1 = tiny.walk(tiny.start, b"ab"), limit.walk(mid, tail[:7])
    assert host["state"][0].tolist() == [tiny.start, s0] and host["state"][1].tolist() == [mid, s1]
    assert tiny.accepts(s0) and torch.isfinite(out[0, EOS]).all() and torch.isinf(out[1, EOS]).all()
    # launch 3: gen_len held still -- the same state recomputed from the same slot
    launch([1, 1, 0, 0], [tok[b"ab"], tok[tail[:7]], 0, 0])
    assert host["state"][0].tolist() == [tiny.start, s0] and host["state"][1].tolist() == [mid, s1]
    # launch 4: slot parity flips back to 0
    out = launch([2, 2, 0, 0], [tok[b"c"], tok[b"k"], 0, 0])  # "k" follows "...abc" + "defghij"
    s0b = tiny.walk(s0, b"c")
    assert host["state"][0].tolist() == [s0b, s0] and int(host["state"][1, 0]) == limit.walk(s1, b"k")
    # launch 5: "d;" ends the statement: nothing but EOS stays
    out = launch([3, 3, 0, 0], [tok[b"d;"], tok[b"x"], 0, 0])
    assert torch.isfinite(out[0]).nonzero().flatten().tolist() == EOS
    assert int(host["state"][1, 1]) == DEAD  # a token from outside the mask: the row may only stop
    assert torch.isfinite(out[1]).nonzero().flatten().tolist() == EOS


def test_dfa_mask_kernel_row_map(gpu, dfas):
    """The prefill tail's launch: logits rows map to table rows (slots) through ``rows``."""
    tiny, limit = dfas
    V = 2500
    words, off, blob = _vocab(V)
    cls, trans, accept, dim = _tables([tiny, limit, tiny, limit], 4)
    on = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    mid = limit.walk(limit.start, b"abc")
    state = torch.tensor([[tiny.start] * 2, [0, 0], [tiny.walk(0, b"c")] * 2, [mid] * 2], dtype=torch.int32)
    base = torch.zeros(4, dtype=torch.int32)
    rows = torch.tensor([3, 1, 2], dtype=torch.int32)
    z = torch.zeros(3, dtype=torch.int32)
    logits = torch.randn(3, V, generator=torch.Generator().manual_seed(1))
    want = logits.clone()
    ref.dfa_mask(want, off, blob, cls, trans, accept, dim, on, state.clone(), base, z, z, z,
                 torch.tensor(EOS, dtype=torch.int32), rows=rows)
    got = logits.to(gpu)
    st = state.to(gpu)
    ops.dfa_mask(got, off.to(gpu), blob.to(gpu), cls.to(gpu), trans.to(gpu), accept.to(gpu), dim.to(gpu), on.to(gpu),
                 st, base.to(gpu), z.to(gpu), z.to(gpu), z.to(gpu), torch.tensor(EOS, dtype=torch.int32, device=gpu),
                 rows=rows.to(gpu))
    assert torch.equal(got.cpu(), want) and torch.equal(st.cpu(), state)
    assert torch.equal(want[1], logits[1]) and torch.isinf(want[0]).any() and torch.isinf(want[2]).any()


# ------------------------------------------------------------------------------------------- engine
PROMPT = [1] + list(range(40, 70))


@pytest.fixture(scope="module")
def engines(gpu):
    kw = dict(device=str(gpu), max_slots=4, max_model_len=512)
    return build_engine("tiny-nsql", guided=True, **kw), build_engine("tiny-nsql", **kw)


def test_engine_graphs_and_full_match(engines):
    eng, plain = engines
    free = SamplingParams(max_tokens=24)
    a = eng.generate([PROMPT], free)[0].token_ids
    assert a == plain.generate([PROMPT], free)[0].token_ids  # unconstrained on the guided engine: the plain tokens
    plain_keys = set(plain.runner.graphs)
    assert plain_keys and all(len(k) == 3 for k in plain_keys)  # guided off: the graph keys are what they were
    assert set(eng.runner.graphs) == plain_keys                 # ... and no guided variant without a constrained row
    for extra in (dict(), dict(temperature=0.8, seed=11)):
        sp = SamplingParams(max_tokens=64, regex=BOUNDED, **extra)
        r1, r2 = eng.generate([PROMPT], sp)[0], eng.generate([PROMPT], sp)[0]
        assert re.fullmatch(BOUNDED, r1.text), r1.text
        assert r1.done_reason == "stop" and r1.token_ids == r2.token_ids
    assert any(len(k) == 4 and k[3] is True for k in eng.runner.graphs)
    assert set(plain.runner.graphs) == plain_keys and eng.stats["guided_steps"] > 0


def test_engine_mixed_batch(engines):
    """A constrained and an unconstrained request in one decode batch: the guided graph masks only the first."""
    eng, plain = engines
    sp = SamplingParams(max_tokens=40)
    a = eng.add_request(PROMPT, SamplingParams(max_tokens=64, regex=BOUNDED))
    b = eng.add_request(PROMPT[:20], sp)
    eng.run_until_done([a, b])
    c = plain.add_request(PROMPT, SamplingParams(max_tokens=27))
    d = plain.add_request(PROMPT[:20], sp)
    plain.run_until_done([c, d])
    assert b.output_ids == d.output_ids and len(b.output_ids) > 1
    assert re.fullmatch(BOUNDED, eng.result(a).text)
