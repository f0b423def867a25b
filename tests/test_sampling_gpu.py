"""sampling.hip pinned to its exact host twin (ops.reference device_uniform / sample_pick_set): for a given seed and
draw counter the twin says which token the device must commit, so the keyed counter RNG, the seed packing, the
on-device draw counter, the candidate merge, the tie order, the top-k clamp, the nucleus rule, the renormalisation
and the inverse-CDF pick are each compared with something exact, as are the stop rules of commit_token."""
import pytest
import torch

from llm_based_apache_spark_optimization_amd import ops
from llm_based_apache_spark_optimization_amd.ops import reference as ref

from test_sampling_cpu import FAMILIES, M, family_case, pick_sets

pytestmark = pytest.mark.gpu

NAMES = ("out_tokens", "gen_len", "input_ids", "positions", "finished")


def new_state(B, max_new, gen_len=None, positions=None, finished=None):
    """CPU decode state (out_tokens, gen_len, input_ids, positions, finished), int32."""
    i32 = lambda x, d: torch.as_tensor(d if x is None else x, dtype=torch.int32).expand(B).clone()  # noqa: E731
    return [torch.full((B, max_new), -1, dtype=torch.int32), i32(gen_len, 0), i32(None, 0),
            i32(positions, torch.arange(B) + 10), i32(finished, 0)]


def to_dev(ts, dev):
    return [None if t is None else t.to(dev).clone() for t in ts]


def assert_state_equal(dev_state, cpu_state, what=""):
    for name, a, b in zip(NAMES, dev_state, cpu_state):
        assert torch.equal(a.cpu(), b), f"{what}{name}: device {a.cpu().tolist()} != reference {b.tolist()}"


def seed_for_u(lo, hi, gen_len=0, start=0):
    """A packed seed (offset 0) whose draw ``gen_len`` has lo <= u < hi, found by scanning keys on the host twin."""
    for key in range(start, start + 200000):
        if lo <= ref.device_uniform(ref.pack_seed(key, 0), gen_len) < hi:
            return ref.pack_seed(key, 0)
    raise AssertionError("no seed found")


def check_draws(gpu, logits, temp, topk, topp, seeds, gen0, min_decided=None, max_new=16):
    """One launch over CPU inputs; every committed token must lie in the twin's set and equal it where decided.
    Returns the device tokens."""
    B = logits.shape[0]
    sets = pick_sets(logits, temp, topk, topp, seeds, gen0)
    st = new_state(B, max_new, gen_len=gen0)
    dst = to_dev(st, gpu)
    eos = torch.tensor([-1], dtype=torch.int32)
    ops.sample_commit(logits.to(gpu).clone(), None, None, temp.to(gpu), topk.to(gpu), topp.to(gpu), seeds.to(gpu),
                      *dst, eos.to(gpu))
    torch.cuda.synchronize()
    toks = dst[0].cpu()[torch.arange(B), gen0.long()]
    decided = sum(len(s) == 1 for s in sets)
    wrong = [(b, int(toks[b]), sorted(sets[b])) for b in range(B) if int(toks[b]) not in sets[b]]
    print(f"decided {decided}/{B}, mismatches {wrong}")
    assert not wrong, f"(row, device token, twin set): {wrong}"
    if min_decided is not None:
        assert decided >= min_decided * B
    ref.commit(toks, *st, eos)
    assert_state_equal(dst, st)
    return toks


# ------------------------------------------------------------------------------------------------ predicted draws
@pytest.mark.parametrize("fi", range(len(FAMILIES)))
def test_predicted_draws(gpu, fi):
    check_draws(gpu, *family_case(fi, V=5000, B=64), min_decided=0.95)


@pytest.mark.parametrize("fi,V,B", [(0, 1000, 64), (0, 2049, 64), (0, 128256, 4), (0, 50, 64), (1, 50, 64)])
def test_predicted_draws_vocab_sizes(gpu, fi, V, B):
    """One padded chunk (1000), a second chunk of one token (2049), 4032 candidates padded to 4096 (128256), and
    fewer than 64 candidates (50; family 1 has top_k = 0, so the zero padding keys reach the softmax lanes)."""
    check_draws(gpu, *family_case(fi, V=V, B=B), min_decided=0.95 if B >= 64 else None)


# ------------------------------------------------------------------------------------------------ candidate merge
def _merge_rows():
    """Four planted rows at V = 3 * 2048 + 100 (four chunks, the last partial); near-flat planted values, so every
    one of the 64 candidates owns a visible slice of [0, 1)."""
    V = 3 * 2048 + 100
    g = torch.Generator().manual_seed(77)
    base = lambda: torch.randn(V, generator=g) * 0.3  # noqa: E731  (|x| < 2: far below the planted values)
    planted = lambda n: 6.0 - 0.02 * torch.randperm(n, generator=g).float()  # noqa: E731  distinct, 4.7 .. 6
    rows = []
    # (a) the whole top-64 inside chunk 1
    r = base()
    r[2048 + torch.randperm(2048, generator=g)[:64]] = planted(64)
    rows.append(r)
    # (b) exactly one of the top-64 in each of chunks 0, 2 and 3, the other 61 in chunk 1
    r = base()
    pos = torch.cat([torch.tensor([5, 4096 + 700, 6144 + 99]), 2048 + torch.randperm(2048, generator=g)[:61]])
    r[pos] = planted(64)
    rows.append(r)
    # (c) ranks 0 and 1 tie across the 4095 | 4096 chunk boundary, ranks 63 and 64 tie across 2047 | 2048
    r = base()
    r[4096 + 1 + torch.randperm(2000, generator=g)[:61]] = planted(61)
    r[4095] = r[4096] = 7.5
    r[2047] = r[2048] = 4.5
    rows.append(r)
    # (d) the largest value at index V - 1, the rest of the top-64 spread over all chunks
    r = base()
    r[torch.randperm(V - 1, generator=g)[:63]] = planted(63)
    r[V - 1] = 7.0
    rows.append(r)
    return rows


def test_candidate_merge(gpu):
    rows = _merge_rows()
    per = 16
    logits = torch.stack([r for r in rows for _ in range(per)])
    B = logits.shape[0]
    # u planted by seed search: a stratified sweep per row, its last two draws on the last candidate (1 / 64 wide)
    windows = [((j + 0.3) / (per - 2), (j + 0.7) / (per - 2)) for j in range(per - 2)] + [(0.992, 0.996), (0.998, 1.0)]
    seeds = torch.tensor([seed_for_u(*windows[b % per], start=1000 * b) for b in range(B)], dtype=torch.int64)
    temp, topk, topp = torch.ones(B), torch.zeros(B, dtype=torch.int32), torch.ones(B)
    gen0 = torch.zeros(B, dtype=torch.int32)
    # what the plants are meant to produce, on the twin
    c = [ref.sample_candidates(r, 0)[1].tolist() for r in rows]
    assert all(2048 <= i < 4096 for i in c[0])
    assert [[i // 2048 for i in c[1]].count(ch) for ch in range(4)] == [1, 61, 1, 1]
    assert c[2][:2] == [4095, 4096] and c[2][63] == 2047 and 2048 not in c[2]
    assert c[3][0] == logits.shape[1] - 1 and len({i // 2048 for i in c[3]}) == 4
    toks = check_draws(gpu, logits, temp, topk, topp, seeds, gen0, min_decided=0.95)
    toks = toks.view(len(rows), per)
    assert int(toks[2, -1]) == 2047 and 2048 not in toks[2].tolist()   # the 64th / 65th tie keeps the lower index
    assert 4095 in toks[2].tolist() and 4096 in toks[2].tolist()       # both tied leaders drawn, each in its slot
    assert int(toks[3, 0]) == logits.shape[1] - 1                      # u near 0 picks the best: index V - 1


# (key, counter offset, j): device_uniform(pack_seed(key, offset), 0) == j / 64 exactly (found by scanning the twin)
EXACT_U = [(0, 286707, 34), (0, 306713, 62), (1, 141367, 63), (0, 586614, 8), (1, 1473566, 0)]


def test_planted_u_on_a_cumulative_boundary(gpu):
    """64 equal logits at T = 1: every probability is 1/64 and every prefix sum j/64, exact in f32 and f64 alike.
    With u == j/64 exactly, "the first index whose cumulative mass EXCEEDS u" is candidate j (cum_j = (j + 1)/64),
    not j - 1 (cum = u); u == 0 picks candidate 0.  The offsets also reach far into the 24-bit counter field."""
    V, B = 2049, len(EXACT_U)
    g = torch.Generator().manual_seed(3)
    cand = torch.cat([torch.randperm(2048, generator=g)[:63], torch.tensor([2048])]).sort().values
    logits = torch.full((B, V), -20.0)
    logits[:, cand] = 3.0
    for key, off, j in EXACT_U:
        assert ref.device_uniform(ref.pack_seed(key, off), 0) == j / 64
    seeds = torch.tensor([ref.pack_seed(key, off) for key, off, _ in EXACT_U], dtype=torch.int64)
    want = [ref.sample_pick(logits[b], 1.0, 0, 1.0, j / 64) for b, (_, _, j) in enumerate(EXACT_U)]
    assert want == [int(cand[j]) for _, _, j in EXACT_U]
    st = new_state(B, 2)
    dst = to_dev(st, gpu)
    ops.sample_commit(logits.to(gpu), None, None, torch.ones(B, device=gpu),
                      torch.zeros(B, dtype=torch.int32, device=gpu), torch.ones(B, device=gpu), seeds.to(gpu), *dst,
                      torch.tensor([-1], dtype=torch.int32, device=gpu))
    assert dst[0][:, 0].tolist() == want


# ---------------------------------------------------------------------------------------------------- mixed batch
def test_mixed_batch(gpu):
    """Greedy, sampled, finished and penalised rows in one launch, top_k / top_p per row."""
    V, B, W = 5000, 32, 64
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, V, generator=g) * 2
    hist = torch.randint(0, V, (B, W), generator=g, dtype=torch.int32)
    pos = torch.tensor([(37 * b) % 200 for b in range(B)], dtype=torch.int32)
    temp = torch.tensor([0.0 if b % 4 == 0 else (0.6 + 0.1 * (b % 5)) for b in range(B)])
    temp[13] = 1e-6  # a sampled row that is the argmax in effect (every other candidate underflows to 0)
    topk = torch.tensor([(0, 1, 5, 40, 64, 100, 13)[b % 7] for b in range(B)], dtype=torch.int32)
    topp = torch.tensor([(1.0, 0.9, 0.5, 0.95, 0.0)[b % 5] for b in range(B)])
    pen = torch.tensor([(1.0, 1.1, 1.0, 1.5, 0.8, 1.0)[b % 6] for b in range(B)])
    last_n = torch.tensor([(64, 8, 64, 1, 33)[b % 5] for b in range(B)], dtype=torch.int32)
    fin = torch.tensor([1 if b % 8 in (3, 4) else 0 for b in range(B)], dtype=torch.int32)
    gen0 = torch.tensor([b % 3 for b in range(B)], dtype=torch.int32)
    seeds = torch.tensor([ref.pack_seed(b * 7919 + 17, b % 2) for b in range(B)], dtype=torch.int64)
    # the penalty must matter: each penalised row's best logit sits on one of its recent tokens
    for b in range(B):
        if float(pen[b]) != 1.0:
            logits[b, int(hist[b, int(pos[b]) % W])] = logits[b].max() + 0.05
    st = new_state(B, 8, gen_len=gen0, positions=pos, finished=fin)
    st[2] = torch.arange(B, dtype=torch.int32) + 100  # input_ids a finished row must keep
    dst, dh = to_dev(st, gpu), hist.to(gpu).clone()
    eos = torch.tensor([-1], dtype=torch.int32)
    ops.sample_commit(logits.to(gpu).clone(), dh, pen.to(gpu), temp.to(gpu), topk.to(gpu), topp.to(gpu),
                      seeds.to(gpu), *dst, eos.to(gpu), last_n=last_n.to(gpu))
    torch.cuda.synchronize()
    out = dst[0].cpu()
    toks = torch.zeros(B, dtype=torch.long)
    kinds = set()
    for b in range(B):
        if int(fin[b]):
            continue
        row = logits[b].clone()
        if float(pen[b]) != 1.0:
            row = ref.repeat_penalty(row, hist[b], float(pen[b]), int(pos[b]), int(last_n[b]))
        tok = int(out[b, int(gen0[b])])
        if float(temp[b]) <= 0:
            want = {int(row.argmax())}
        else:
            want = ref.sample_pick_set(row, float(temp[b]), int(topk[b]), float(topp[b]),
                                       ref.device_uniform(int(seeds[b]), int(gen0[b])), M)
        assert tok in want, (b, tok, sorted(want))
        kinds.add((float(temp[b]) > 0, float(pen[b]) != 1.0))
        toks[b] = tok
    assert len(kinds) == 4  # greedy / sampled x penalised / not all occurred among the live rows
    hc = hist.clone()
    ref.commit(toks, *st, eos, hist=hc)
    assert_state_equal(dst, st)
    assert torch.equal(dh.cpu(), hc)
    for b in torch.nonzero(fin).flatten().tolist():  # a finished row: five state entries and the ring untouched
        assert torch.equal(out[b], torch.full((8,), -1, dtype=torch.int32))
        assert [int(dst[i][b]) for i in (1, 2, 3, 4)] == [int(gen0[b]), 100 + b, int(pos[b]), 1]
        assert torch.equal(dh[b].cpu(), hist[b])


# ----------------------------------------------------------------------------------- multi-step state, graph replay
class Steps:
    """Eight launches over B = 12 rows, V = 2049, ring W = 64, max_new = 12, with planted dominant logits (gap >= 35
    at T = 1 and top_p = 0.9: only the planted token is kept, so the draw is decided whatever u is)."""
    V, B, W, MAX_NEW, N = 2049, 12, 64, 12, 8
    EOS = [7, 1500, 2040]
    R_LIMIT, R_EOS, R_NOEOS = 4, 5, 6  # limit 5 < max_new; EOS id drawn at step 3; the same draw with eos_on = 0

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        B, V = self.B, self.V
        self.logits = [torch.randn(B, V, generator=g) * 2 for _ in range(self.N)]
        for lg in self.logits:
            lg[self.R_NOEOS] = lg[self.R_EOS]
        for r in (self.R_EOS, self.R_NOEOS):
            self.logits[2][r, self.EOS[1]] = self.logits[2][r].max() + 35.0
        self.temp = torch.tensor([1.0, 0.8, 0.7, 1.3, 1.0, 1.0, 1.0, 0.0, 0.9, 1.0, 0.8, 1.2])
        self.topk = torch.tensor([40, 0, 64, 10, 40, 40, 40, 1, 5, 100, 40, 2], dtype=torch.int32)
        self.topp = torch.tensor([0.9, 1.0, 0.95, 0.5, 0.9, 0.9, 0.9, 1.0, 0.9, 1.0, 0.9, 0.9])
        self.pen = torch.tensor([1.0, 1.1, 1.0, 1.3, 1.0, 1.0, 1.0, 1.2, 1.0, 1.0, 0.9, 1.0])
        self.last_n = torch.tensor([64, 64, 16, 64, 64, 64, 64, 5, 64, 64, 64, 64], dtype=torch.int32)
        self.seeds = torch.tensor([ref.pack_seed(b * 7919 + 17, 3 * (b % 2)) for b in range(B)], dtype=torch.int64)
        self.seeds[self.R_NOEOS] = self.seeds[self.R_EOS]
        self.limit = torch.full((B,), self.MAX_NEW, dtype=torch.int32)
        self.limit[self.R_LIMIT] = 5
        self.limit[9] = 100  # above max_new: max_new rules
        self.eos_on = torch.ones(B, dtype=torch.int32)
        self.eos_on[self.R_NOEOS] = 0
        self.eos = torch.tensor(self.EOS, dtype=torch.int32)
        self.hist0 = torch.randint(0, V, (B, self.W), generator=g, dtype=torch.int32)
        # positions straddling W - 1 -> W (the ring slot (p + 1) % W wraps within the eight steps)
        self.pos0 = torch.tensor([60, 61, 62, 63, 64, 59, 59, 58, 0, 5, 126, 127], dtype=torch.int32)
        self.gen0 = torch.tensor([0, 1, 0, 2, 0, 0, 0, 0, 0, 5, 0, 3], dtype=torch.int32)

    def state(self):
        return new_state(self.B, self.MAX_NEW, gen_len=self.gen0, positions=self.pos0), self.hist0.clone()

    def params(self, dev):
        return [t.to(dev) for t in (self.temp, self.topk, self.topp, self.seeds)]

    def launch(self, logits_dev, dst, dh, dev_params, dev_extra, workspace=None):
        pen, eos, limit, eos_on, last_n = dev_extra
        ops.sample_commit(logits_dev, dh, pen, *dev_params, *dst, eos, limit, eos_on, workspace=workspace,
                          last_n=last_n)

    def extra(self, dev):
        return [t.to(dev) for t in (self.pen, self.eos, self.limit, self.eos_on, self.last_n)]

    def twin_sets(self, step, st, hist):
        """Admissible tokens of each live row from the mirror state before the launch."""
        sets = {}
        for b in range(self.B):
            if int(st[4][b]):
                continue
            row = self.logits[step][b].clone()
            if float(self.pen[b]) != 1.0:
                row = ref.repeat_penalty(row, hist[b], float(self.pen[b]), int(st[3][b]), int(self.last_n[b]))
            if float(self.temp[b]) <= 0:
                sets[b] = {int(row.argmax())}
            else:
                sets[b] = ref.sample_pick_set(row, float(self.temp[b]), int(self.topk[b]), float(self.topp[b]),
                                              ref.device_uniform(int(self.seeds[b]), int(st[1][b])), M)
        return sets


@pytest.fixture(scope="module")
def steps():
    return Steps()


def test_multi_step_state(gpu, steps):
    s = steps
    st, hist = s.state()
    dst, dh = to_dev(st, gpu), hist.to(gpu).clone()
    params, extra = s.params(gpu), s.extra(gpu)
    for step in range(s.N):
        sets = s.twin_sets(step, st, hist)
        gen_before = st[1].clone()
        s.launch(s.logits[step].to(gpu).clone(), dst, dh, params, extra)
        torch.cuda.synchronize()
        out = dst[0].cpu()
        toks = torch.zeros(s.B, dtype=torch.long)
        for b, want in sets.items():
            toks[b] = int(out[b, int(gen_before[b])])
            assert int(toks[b]) in want, (step, b, int(toks[b]), sorted(want))
        # an undecided draw follows the device's element of the set, so the mirror stays comparable
        ref.commit(toks, *st, s.eos, s.limit, s.eos_on, hist=hist)
        assert_state_equal(dst, st, what=f"step {step}: ")
        assert torch.equal(dh.cpu(), hist), f"step {step}: hist"
        if step == 2:  # the planted EOS draw: finishes the row that heeds EOS, not its twin row with eos_on = 0
            assert int(toks[s.R_EOS]) == s.EOS[1] == int(toks[s.R_NOEOS])
            assert int(st[4][s.R_EOS]) == 1 and int(st[1][s.R_EOS]) == 3 and int(st[4][s.R_NOEOS]) == 0
    assert int(st[1][s.R_EOS]) == 3 and int(st[3][s.R_EOS]) == int(s.pos0[s.R_EOS]) + 2  # left alone for 5 launches
    assert int(st[4][s.R_LIMIT]) == 1 and int(st[1][s.R_LIMIT]) == 5                       # per-row limit < max_new
    assert int(st[4][s.R_NOEOS]) == 0 and int(st[1][s.R_NOEOS]) == s.N
    assert int(st[4][9]) == 1 and int(st[1][9]) == s.MAX_NEW and int(st[4][0]) == 0         # max_new caps limit 100


def test_captured_graph_replays_the_eager_draws(gpu, steps):
    """One launch captured once, replayed six times with new logits in its static buffer, is bitwise the eager run:
    the draw counter (gen_len) is read on the device at replay time, not frozen at capture."""
    s, n = steps, 6
    params, extra = s.params(gpu), s.extra(gpu)
    nch, nch2 = (s.V + 4095) // 4096, (s.V + 2047) // 2048
    ws = (torch.empty(s.B * nch, device=gpu, dtype=torch.int64),
          torch.empty(s.B * nch2 * 64, device=gpu, dtype=torch.int64))

    st, hist = s.state()
    est, eh = to_dev(st, gpu), hist.to(gpu).clone()
    for step in range(n):
        s.launch(s.logits[step].to(gpu).clone(), est, eh, params, extra, workspace=ws)
    torch.cuda.synchronize()

    gst, gh = to_dev(st, gpu), hist.to(gpu).clone()
    static_logits = torch.zeros(s.B, s.V, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # recorded, not executed: the state is still the start state
            s.launch(static_logits, gst, gh, params, extra, workspace=ws)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for step in range(n):
        static_logits.copy_(s.logits[step])
        graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, gst, est):
        assert torch.equal(a, b), name
    assert torch.equal(gh, eh)
    assert int((est[1].cpu() - s.gen0).max()) == n  # rows that ran all six steps drew at six different counters


# ------------------------------------------------------------------------------------------ greedy partial reduce
@pytest.mark.parametrize("V", [1, 4096, 4097, 128256])
def test_argmax_partial_reduce(gpu, V):
    ninf = float("-inf")
    g = torch.Generator().manual_seed(V)
    rows = []
    for at in sorted({0, 4095, 4096, V - 1}):  # the maximum at each place the row has
        if at < V:
            r = torch.randn(V, generator=g)
            r[at] = 50.0
            rows.append(r)
    rows.append(torch.full((V,), 1.25))                      # whole-row tie -> index 0
    if V > 4096:                                             # tie across the 4096-chunk boundary -> 4095
        r = torch.randn(V, generator=g)
        r[4095] = r[4096] = 40.0
        rows.append(r)
    for at in sorted({0, min(4095, V - 1), V - 1}):          # all -inf except one entry
        r = torch.full((V,), ninf)
        r[at] = -3.0
        rows.append(r)
    rows.append(torch.full((V,), ninf))                      # all -inf: torch and the kernel both give 0
    logits = torch.stack(rows)
    B = logits.shape[0]
    eos = torch.tensor([0, V - 1, 4095], dtype=torch.int32)
    limit = torch.tensor([(4, 1, 9, 2)[b % 4] for b in range(B)], dtype=torch.int32)   # 9 > max_new = 4
    eos_on = torch.tensor([(1, 1, 0)[b % 3] for b in range(B)], dtype=torch.int32)
    st = new_state(B, 4, gen_len=torch.tensor([b % 2 for b in range(B)]))
    dst = to_dev(st, gpu)
    ops.argmax_commit(logits.to(gpu), *dst, eos.to(gpu), limit.to(gpu), eos_on.to(gpu))
    torch.cuda.synchronize()
    want = logits.argmax(-1)
    got = dst[2].cpu().long()
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert int(want[-1]) == 0
    ref.argmax_commit(logits, *st, eos, limit, eos_on)
    assert_state_equal(dst, st)
    assert 0 < int(st[4].sum()) < B or V == 1  # both finished and running rows occurred


# ------------------------------------------------------------------------------------------------------ size limit
def test_largest_vocab_commits_the_twin_token(gpu):
    """V = 262144, the documented maximum: 8192 candidates, 64 KiB of dynamic LDS in the merge kernel."""
    V = 262144
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(1, V, generator=g) * 2
    logits[0, V - 1] = logits.max() + 0.5  # the last chunk's last lane takes part
    temp, topk, topp = torch.tensor([0.8]), torch.tensor([40], dtype=torch.int32), torch.tensor([0.9])
    seeds = torch.tensor([ref.pack_seed(17, 2)], dtype=torch.int64)
    gen0 = torch.tensor([1], dtype=torch.int32)
    assert len(pick_sets(logits, temp, topk, topp, seeds, gen0)[0]) == 1  # a decided draw
    check_draws(gpu, logits, temp, topk, topp, seeds, gen0, min_decided=1.0)


def test_oversize_vocab_rejected_before_any_launch(gpu):
    """Regression: V = 262145 used to run the penalty, argmax and top-k kernels (rewriting the logits) before the
    size check refused the launch.  It must raise with the state, the ring and the logits untouched."""
    V, W = 262145, 64
    logits = torch.randn(1, V)
    hist = torch.full((1, W), 5, dtype=torch.int32)
    logits[0, 5] = 3.0
    st = new_state(1, 4, gen_len=torch.tensor([1]))
    dst, dh, dl = to_dev(st, gpu), hist.to(gpu).clone(), logits.to(gpu).clone()
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=gpu)  # noqa: E731
    with pytest.raises(RuntimeError):
        ops.sample_commit(dl, dh, one(1.5, torch.float32), one(0.8, torch.float32), one(40, torch.int32),
                          one(0.9, torch.float32), one(17, torch.int64), *dst, one(-1, torch.int32))
    torch.cuda.synchronize()
    assert_state_equal(dst, st)
    assert torch.equal(dh.cpu(), hist)
    assert torch.equal(dl.cpu(), logits)
