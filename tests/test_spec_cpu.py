"""Prompt-lookup speculative decoding on the CPU: the drafter and commit references against hand-written rules, and the
engine's verify steps (greedy, batch 1) against its plain steps -- the tokens must be identical, whatever is drafted."""
import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.config import Settings
from llm_based_apache_spark_optimization_amd.engine import SamplingParams, build_engine
from llm_based_apache_spark_optimization_amd.ops import reference as ref

SYSTEM = "Table name is temp_view. The structure of the table is:\nName (string)\nAge (int)"
PROMPT = "How many rows are there?"
K = 3

I32 = dict(dtype=torch.int32)

# hand-written contexts (token lists): name -> (context, what it exercises)
CONTEXTS = {
    "no_match": [1, 2, 3, 4, 5, 6],
    "match_n1": [7, 1, 2, 9, 3, 4, 2],                   # the last token 2 occurs once before; its left neighbours differ
    "long_beats_recent": [5, 6, 7, 8, 1, 9, 7, 2, 3, 5, 6, 7],  # ...5 6 7 at the start (m = 3) vs the later lone 7 (m = 1)
    "constant": [4] * 12,                                # every j matches: `full` must pick one with k real tokens
    "off_the_end": [3, 1, 2, 7, 7, 7, 1, 2, 1, 2],       # tie at m = 2: the full (older) match beats the recent one
    "tail_only": [6, 1, 2, 3, 4, 1, 2],                  # one match, with a full continuation
    "runs_off": [3, 5, 3],                               # the only candidate j = 0 has one token after it: -1 padding
    "short": [2, 2],                                     # L < n_max
}


def brute_draft(ctx, k, n_max=3, n_min=1):
    L = len(ctx)
    best = None
    for j in range(0, L - 1):
        m = 0
        while m < n_max and j - m >= 0 and ctx[j - m] == ctx[L - 1 - m]:
            m += 1
        if m >= n_min and m >= 1:
            key = (m, j + 1 + k <= L, j)
            best = key if best is None or key > best else best
    if best is None:
        return [-1] * k
    j = best[2]
    return [ctx[j + 1 + i] if j + 1 + i < L else -1 for i in range(k)]


def draft_inputs(ctx, n_prompt, device="cpu", max_len=None, max_new=None):
    """ctx split into a prompt of n_prompt tokens and generated tokens, as the runner holds them."""
    L = len(ctx)
    max_len = max_len or L + 4
    max_new = max_new or L + 4
    pt = torch.zeros(1, max_len, **I32)
    pt[0, :n_prompt] = torch.tensor(ctx[:n_prompt], **I32)
    ot = torch.zeros(1, max_new, **I32)
    ot[0, :L - n_prompt] = torch.tensor(ctx[n_prompt:], **I32)
    t = lambda v: torch.tensor([v], **I32).to(device)  # noqa: E731
    return (pt.to(device), t(n_prompt), ot.to(device), t(L - n_prompt), t(ctx[-1]), t(L - 1))


def run_draft(ctx, n_prompt, k=K, n_max=3, n_min=1, forced=None, device="cpu"):
    ins = draft_inputs(ctx, n_prompt, device)
    ids = torch.full((k + 1,), -7, **I32).to(device)
    pos = torch.full((k + 1,), -7, **I32).to(device)
    dr = torch.full((k,), -7, **I32).to(device)
    ops.spec_draft(*ins, k, ids, pos, dr, n_max=n_max, n_min=n_min, forced=forced)
    return ids.tolist(), pos.tolist(), dr.tolist()


@pytest.mark.parametrize("name", sorted(CONTEXTS))
@pytest.mark.parametrize("split", ["all_prompt", "mixed"])
def test_spec_draft_matches_brute_force(name, split):
    ctx = CONTEXTS[name]
    n_prompt = len(ctx) if split == "all_prompt" else max(1, len(ctx) // 2)
    ids, pos, dr = run_draft(ctx, n_prompt)
    want = brute_draft(ctx, K)
    assert dr == want
    assert ids == [ctx[-1]] + [max(d, 0) for d in want]          # spec_ids[0] is the row's input token
    assert pos == [len(ctx) - 1 + t for t in range(K + 1)]       # spec_pos continues from the row's position


def test_spec_draft_rule_cases():
    assert brute_draft(CONTEXTS["no_match"], K) == [-1, -1, -1]
    assert brute_draft(CONTEXTS["match_n1"], K) == [9, 3, 4]
    assert brute_draft(CONTEXTS["long_beats_recent"], K) == [8, 1, 9]
    assert brute_draft(CONTEXTS["constant"], K) == [4, 4, 4]      # not [4, -1, -1] from the most recent match
    assert brute_draft(CONTEXTS["off_the_end"], K) == [7, 7, 7]  # not [1, 2, -1]
    assert brute_draft(CONTEXTS["runs_off"], K) == [5, 3, -1]
    assert brute_draft(CONTEXTS["short"], K) == [2, -1, -1]
    # n_min = 2 rejects the n = 1 match
    assert run_draft(CONTEXTS["match_n1"], 3, n_min=2)[2] == [-1, -1, -1]
    assert run_draft(CONTEXTS["match_n1"], 3, n_min=2)[2] == brute_draft(CONTEXTS["match_n1"], K, n_min=2)


def test_spec_draft_random_against_brute_force():
    g = torch.Generator().manual_seed(3)
    for L in (2, 3, 17, 300):
        for k in (1, 3, 7):
            ctx = torch.randint(0, 6, (L,), generator=g).tolist()
            assert run_draft(ctx, max(1, L // 3), k=k)[2] == brute_draft(ctx, k)


def test_spec_draft_forced():
    ctx = CONTEXTS["constant"]
    one = torch.tensor([[11, 12, 13]], **I32)
    ids, pos, dr = run_draft(ctx, 5, forced=one)
    assert dr == [11, 12, 13] and ids == [4, 11, 12, 13] and pos == [11, 12, 13, 14]
    table = torch.arange(30, **I32).view(10, 3)      # row min(gen_len, 9): gen_len = 12 - 5 = 7
    assert run_draft(ctx, 5, forced=table)[2] == [21, 22, 23]
    assert run_draft(ctx, 1, forced=table)[2] == [27, 28, 29]   # gen_len 11 -> the last row


# ------------------------------------------------------------------------------------------------ spec_commit
def commit_state(max_new=16, gen=2, pos=9, limit=16, eos_on=1, finished=0):
    return dict(out_tokens=torch.zeros(1, max_new, **I32), gen_len=torch.tensor([gen], **I32),
                input_ids=torch.tensor([5], **I32), positions=torch.tensor([pos], **I32),
                finished=torch.tensor([finished], **I32), eos=torch.tensor([99], **I32),
                limit=torch.tensor([limit], **I32), eos_on=torch.tensor([eos_on], **I32))


def planted_logits(toks, V=128):
    g = torch.Generator().manual_seed(len(toks))
    lg = torch.randn(len(toks), V, generator=g)
    for i, t in enumerate(toks):
        lg[i, t] = 50.0
    return lg


def run_commit(toks, draft, device="cpu", V=128, **kw):
    st = {k: v.to(device) for k, v in commit_state(**kw).items()}
    stats = torch.zeros(3, dtype=torch.int64, device=device)
    ops.spec_commit(planted_logits(toks, V).to(device), torch.tensor(draft, **I32).to(device), stats,
                    st["out_tokens"], st["gen_len"], st["input_ids"], st["positions"], st["finished"], st["eos"],
                    st["limit"], st["eos_on"])
    return {k: v.cpu() for k, v in st.items()}, stats.tolist()


COMMIT_CASES = {
    # name: (argmax of the T rows, drafts, state overrides, tokens committed, finished, stats)
    "a0": ([10, 11, 12, 13], [7, 11, 12], {}, [10], 0, [1, 3, 0]),
    "ak": ([10, 11, 12, 13], [10, 11, 12], {}, [10, 11, 12, 13], 0, [1, 3, 3]),
    "mid_mismatch": ([10, 11, 12, 13], [10, 8, 12], {}, [10, 11], 0, [1, 3, 1]),
    "eos_inside": ([10, 99, 12, 13], [10, 99, 12], {}, [10, 99], 1, [1, 3, 1]),
    "eos_ignored": ([10, 99, 12, 13], [10, 99, 12], dict(eos_on=0), [10, 99, 12, 13], 0, [1, 3, 3]),
    "limit_inside": ([10, 11, 12, 13], [10, 11, 12], dict(limit=4), [10, 11], 1, [1, 3, 1]),
    "finished": ([10, 11, 12, 13], [10, 11, 12], dict(finished=1), [], 1, [0, 0, 0]),
    "minus_one": ([10, 0, 12, 13], [10, -1, 12], {}, [10, 0], 0, [1, 2, 1]),  # draft -1 ran as token 0: never accepted
}


@pytest.mark.parametrize("name", sorted(COMMIT_CASES))
def test_spec_commit_reference(name):
    toks, draft, kw, want, fin, stats = COMMIT_CASES[name]
    st, got_stats = run_commit(toks, draft, **kw)
    n = len(want)
    assert int(st["gen_len"]) == 2 + n
    assert st["out_tokens"][0, 2:2 + n].tolist() == want and int(st["out_tokens"][0, 2 + n]) == 0
    assert int(st["finished"]) == fin
    assert int(st["input_ids"]) == (want[-1] if want else 5)
    # the position advances once per committed token, except for a finishing one
    assert int(st["positions"]) == 9 + n - (1 if (fin and n) else 0)
    assert got_stats == stats


# ------------------------------------------------------------------------------------------------ engine
def make(model="tiny-nsql", **kw):
    return build_engine(model, device="cpu", max_slots=2, max_model_len=512, seed=0, **kw)


def gen(eng, n=96, prompt=PROMPT, **opts):
    sp = SamplingParams(max_tokens=n, ignore_eos=True, **opts)
    return eng.generate([prompt], sp, system=SYSTEM)[0].token_ids


@pytest.fixture(scope="module")
def plain():
    eng = make()
    toks = gen(eng)
    assert eng.stats["spec_steps"] == 0 and eng.stats["decode_steps"] == 95
    return eng, toks


def forced_table(plain_toks, kind, V):
    """[len, k] drafts indexed by the tokens generated so far: the step at g drafts tokens g, g + 1, ..."""
    n = len(plain_toks)
    right = lambda i: plain_toks[i] if i < n else 0  # noqa: E731
    wrong = lambda i: (right(i) + 1) % V             # noqa: E731
    rows = []
    for g in range(n + 1):
        if kind == "right":
            rows.append([right(g + i) for i in range(K)])
        elif kind == "wrong":
            rows.append([wrong(g + i) for i in range(K)])
        else:  # the first one right, the rest wrong
            rows.append([right(g)] + [wrong(g + i) for i in range(1, K)])
    return torch.tensor(rows, **I32)


def test_engine_spec_equals_plain_and_accepts(plain):
    _, toks = plain
    eng = make(spec_tokens=K)
    assert gen(eng) == toks
    st = eng.stats
    # recorded for this configuration: 52 verify steps, 43 accepted drafts (n = 3..1, k = 3)
    assert st["spec_accepted"] >= 1 and 0 < st["spec_steps"] < 95
    assert st["spec_steps"] + st["spec_accepted"] == 95  # every token after the prefill's is a step's first or accepted
    assert st["generated_tokens"] == 96 and st["decode_steps"] >= st["spec_steps"]


@pytest.mark.parametrize("kind,per_step", [("right", K), ("wrong", 0), ("first", 1)])
def test_engine_forced_drafts(plain, kind, per_step):
    peng, toks = plain
    eng = make(spec_tokens=K)
    eng.runner.set_spec_forced(forced_table(toks, kind, eng.runner.V))
    assert gen(eng) == toks
    st = eng.stats
    steps = -(-95 // (per_step + 1))
    assert st["spec_steps"] == steps
    # a = per_step at every step until the length limit truncates the last one
    assert st["spec_accepted"] == 95 - steps
    assert st["spec_drafted"] == K * steps
    if kind == "wrong":  # KV after a run that wrote 3 rejected rows per step: the committed context is untouched
        ctx = len(eng.encode(eng.render(PROMPT, SYSTEM, False))) + 95
        for e in (peng, eng):  # both engines are idle: their requests ran in the same blocks from a fresh arena
            assert e.sched.num_running == 0
        blocks = list(range(1, 1 + -(-ctx // 64)))
        a = eng.runner.kv[:, :, blocks].transpose(2, 3).reshape(eng.runner.L, 2, eng.runner.Hkv, -1, 128)[:, :, :, :ctx]
        b = peng.runner.kv[:, :, blocks].transpose(2, 3).reshape(peng.runner.L, 2, peng.runner.Hkv, -1, 128)[:, :, :, :ctx]
        assert torch.equal(a, b)


def test_engine_gating(plain):
    _, toks = plain
    # spec_tokens = 0
    eng = make()
    assert gen(eng, 24) == toks[:24] and eng.stats["spec_steps"] == 0
    eng = make(spec_tokens=K)
    # temperature > 0 / repetition penalty: the sampler path
    gen(eng, 12, temperature=0.8, seed=1)
    gen(eng, 12, repeat_penalty=1.1)
    assert eng.stats["spec_steps"] == 0
    # the request opts out ("speculate": false)
    sp = SamplingParams.from_ollama_options({"num_predict": 12, "speculate": False, "ignore_eos": True})
    assert sp.speculate is False and SamplingParams.from_ollama_options({}).speculate is True
    assert eng.generate([PROMPT], sp, system=SYSTEM)[0].token_ids == toks[:12]
    assert eng.stats["spec_steps"] == 0
    # two running requests
    res = eng.generate([PROMPT, PROMPT], SamplingParams(max_tokens=12, ignore_eos=True), system=SYSTEM)
    assert [r.token_ids for r in res] == [toks[:12]] * 2 and eng.stats["spec_steps"] == 0
    # ... and the same engine speculates again once a request runs alone
    assert gen(eng, 24) == toks[:24] and eng.stats["spec_steps"] > 0
    # fp8 KV cache
    e8 = make(spec_tokens=K, kv_dtype="fp8")
    assert not e8.runner.spec_supported()
    gen(e8, 12)
    assert e8.stats["spec_steps"] == 0


def test_engine_gating_window():
    """A request whose window leaves fewer than T spare positions beyond the run takes plain steps."""
    eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=128, seed=0, spec_tokens=K)
    ref_eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=128, seed=0)
    ids = eng.encode(eng.render(PROMPT, SYSTEM, False))
    ids = ids[:1] + ids[-(128 - 4):]  # 125 tokens: 3 positions left
    sp = SamplingParams(max_tokens=3, ignore_eos=True)
    a = eng.generate([ids], sp)[0].token_ids
    assert a == ref_eng.generate([ids], sp)[0].token_ids and len(a) == 3
    assert eng.stats["spec_steps"] == 0 and eng.stats["decode_steps"] == 2


def test_spec_tokens_clamped():
    eng = make("tiny-llama3", spec_tokens=9)  # G = 3: T * G <= 16 -> T <= 5
    r = eng.runner
    assert r.H // r.Hkv == 3 and r.spec_k() == 4 and r.spec_supported()
    base = gen(make("tiny-llama3"), 48)
    assert gen(eng, 48) == base and eng.stats["spec_steps"] > 0
    assert make(spec_tokens=9).runner.spec_k() == 7  # G = 1: T <= 8


def test_preempted_request_resumes_speculating():
    """Two requests in an arena too small for both: the younger is preempted, re-admitted alone after the older
    finishes (its generated tokens folded into the prompt the drafter searches), and still decodes its plain tokens."""
    prompts = [[1] + list(range(3 + k, 40 + k)) for k in range(2)]
    sp = SamplingParams(max_tokens=150, ignore_eos=True)
    solo_eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, num_kv_blocks=6)
    solo = [solo_eng.generate([p], sp)[0].token_ids for p in prompts]
    eng = build_engine("tiny-nsql", device="cpu", max_slots=2, max_model_len=512, num_kv_blocks=6, spec_tokens=K)
    eng.run_ahead = 16
    reqs = [eng.add_request(p, sp) for p in prompts]
    eng.run_until_done(reqs)
    assert [q.output_ids for q in reqs] == solo
    assert eng.stats["preempted"] >= 1 and any(q.preemptions for q in reqs)
    assert eng.stats["spec_steps"] > 0
    assert eng.sched.free_blocks == 5 and eng.sched.num_running == 0


def test_acceptance_guard_drops_request(plain):
    _, toks = plain
    eng = make(spec_tokens=K)
    eng.runner.set_spec_forced(forced_table(toks, "wrong", eng.runner.V))
    eng.runner.spec_min_accept = 0.5
    eng.run_ahead = 8
    assert gen(eng) == toks
    # 16 verify steps at zero acceptance, then plain steps for the rest of the request
    assert 16 <= eng.stats["spec_steps"] < 24 and eng.stats["spec_accepted"] == 0


def test_settings_and_stats_surface(monkeypatch):
    assert Settings().spec_tokens == 0
    monkeypatch.setenv("LSA_SPEC_TOKENS", "3")
    assert Settings().spec_tokens == 3
    eng = make()
    assert {"spec_steps", "spec_drafted", "spec_accepted"} <= set(eng.stats)
    assert eng.runner.spec_tokens == 0 and eng.runner.spec_min_accept >= 0.0
    assert ops.verify_split_plan(8, 2048) == ops.decode_split_plan(1, 8, 2048)
    ws = ops.verify_workspace(4, 24, 8, 17, "cpu")
    assert ws[0].numel() == 4 * 24 * 17 * 128 and ws[2].numel() >= 8
    assert ref.spec_draft is not None and ref.spec_commit is not None and ref.attn_verify is not None
