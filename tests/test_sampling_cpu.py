"""The exact host twin of sampling.hip's sampled draw (ops.reference device_uniform / sample_candidates /
sample_pick / sample_pick_set), checked on its own: the RNG against an independent splitmix64, the pick against
``sample_probs``, the edge conventions, and the share of draws the twin cannot decide within its f32 margin.
tests/test_sampling_gpu.py pins the kernels to this twin and shares the input families defined here."""
import pytest
import torch

from llm_based_apache_spark_optimization_amd.ops import reference as ref

M = ref.SAMPLE_MARGIN

# (logit scale, temperature, top_k, top_p); the first is Ollama's default option set
FAMILIES = [(2.0, 0.8, 40, 0.9), (4.0, 1.0, 0, 1.0), (1.0, 0.7, 64, 0.95), (3.0, 1.5, 10, 0.5), (2.0, 0.05, 40, 0.9),
            (1.0, 5.0, 100, 1.0)]


def family_case(fi: int, V: int = 5000, B: int = 64):
    """Inputs of family ``fi``: B distinct random rows, per-row parameter tensors (f32 / int32 as the kernel reads
    them), seeds ``pack_seed(b * 7919 + 17, off)`` with ``off > 0`` on every third row, and mixed start ``gen_len``."""
    scale, T, K, P = FAMILIES[fi]
    g = torch.Generator().manual_seed(1000 + 17 * fi + V)
    logits = torch.randn(B, V, generator=g) * scale
    temp = torch.full((B,), T)
    topk = torch.full((B,), K, dtype=torch.int32)
    topp = torch.full((B,), P)
    offs = [(5 * b + 1) if b % 3 == 0 else 0 for b in range(B)]
    seeds = torch.tensor([ref.pack_seed(b * 7919 + 17, offs[b]) for b in range(B)], dtype=torch.int64)
    gen0 = torch.tensor([(3 * b) % 7 for b in range(B)], dtype=torch.int32)
    return logits, temp, topk, topp, seeds, gen0


def pick_sets(logits, temp, topk, topp, seeds, gen_len):
    """Per row: the twin's set of admissible tokens for the draw the device makes at ``gen_len``."""
    return [ref.sample_pick_set(logits[b], float(temp[b]), int(topk[b]), float(topp[b]),
                                ref.device_uniform(int(seeds[b]), int(gen_len[b])), M)
            for b in range(logits.shape[0])]


# ------------------------------------------------------------------------------------------------ device_uniform
_G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


class SplitMix64:
    """The textbook generator (state += golden; output = finalizer(state)), written independently of the twin."""

    def __init__(self, state):
        self.s = state & _M64

    def next(self):
        self.s = (self.s + _G) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)


def test_device_uniform_is_a_keyed_splitmix64_stream():
    """lsa_key_mix(key) is the first splitmix64 output of state ``key``; draw c is the top 24 bits of output c + 1
    of the splitmix64 stream whose state is that scrambled key."""
    assert SplitMix64(0).next() == 0xE220A8397B1DCDAF  # published first output of seed 0
    for key in (0, 1, 17, 7919 * 5 + 17, (1 << 40) - 1):
        stream = SplitMix64(SplitMix64(key).next())
        for c in range(6):
            assert ref.device_uniform(ref.pack_seed(key, 0), c) == (stream.next() >> 40) / 2 ** 24
    # only the low 40 bits are the key; the high 24 are the counter offset
    assert ref.device_uniform((3 << 40) | 5, 2) == ref.device_uniform(5, 5)
    # a negative int64 word (bit 63 of the offset field set) is read as unsigned, as the kernel does
    assert ref.device_uniform(-1, 0) == ref.device_uniform((1 << 64) - 1, 0)


def test_device_uniform_range_grid_and_mean():
    us = [ref.device_uniform(ref.pack_seed(k, 0), g) for k in range(200) for g in range(50)]
    assert all(0.0 <= u < 1.0 for u in us)
    assert all(float(u * 2 ** 24).is_integer() for u in us)
    mean = sum(us) / len(us)
    print(f"device_uniform mean over 200 keys x 50 draws: {mean:.4f}")
    assert abs(mean - 0.5) < 0.02


def test_device_uniform_resume_continuity():
    for k in (0, 3, 7919 + 17, (1 << 40) - 1):
        for off in (1, 2, 63, 4096, (1 << 23) - 1):
            for g in (0, 1, 9):
                assert ref.device_uniform(ref.pack_seed(k, off), g) == ref.device_uniform(ref.pack_seed(k, 0), g + off)


def test_device_uniform_neighbouring_keys_and_counters_do_not_collide():
    for k in range(50):
        for g in range(20):
            assert ref.device_uniform(ref.pack_seed(k, 0), g + 1) != ref.device_uniform(ref.pack_seed(k + 1, 0), g)


# ---------------------------------------------------------------------------------------------------- sample_pick
@pytest.mark.parametrize("T,K,P", [(0.8, 40, 0.9), (1.0, 0, 1.0), (1.5, 10, 0.5), (0.3, 64, 0.95)])
def test_sample_pick_reproduces_sample_probs(T, K, P):
    """Sweeping u over a fine grid, the picks have ``sample_probs``'s distribution to within the grid step (each
    token's interval has two ends, each placed to within one step) and never leave its support."""
    torch.manual_seed(11)
    row = torch.randn(300) * 2
    idx, p = ref.sample_probs(row, T, K, P)
    want = torch.zeros(300, dtype=torch.float64)
    want[idx] = p.double()
    N = 2048
    counts = torch.zeros(300, dtype=torch.float64)
    for j in range(N):
        counts[ref.sample_pick(row, T, K, P, (j + 0.5) / N)] += 1
    assert set(torch.nonzero(counts).flatten().tolist()) <= set(idx[p > 0].tolist())
    assert float((counts / N - want).abs().max()) <= 2.0 / N + 1e-6


U_SWEEP = [0.0, 2.0 ** -24, 0.1, 0.37, 0.5, 0.9, 0.999, 1 - 2.0 ** -24, 1.0, 1.5]  # >= 1: the fallback branch


def test_sample_pick_top_p_zero_keeps_only_the_best():
    torch.manual_seed(12)
    row = torch.randn(500)
    for tp in (0.0, -1.0):
        assert {ref.sample_pick(row, 1.0, 40, tp, u) for u in U_SWEEP} == {int(row.argmax())}


def test_sample_pick_top_k_out_of_range_means_64():
    torch.manual_seed(13)
    row = torch.randn(500) * 0.5  # flat enough that the 64th candidate has visible mass
    for k in (0, -1, 65, 1000):
        vals, idx = ref.sample_candidates(row, k)
        assert idx.numel() == 64 and torch.equal(idx, ref.sample_candidates(row, 64)[1])
        for u in U_SWEEP:
            assert ref.sample_pick(row, 1.0, k, 1.0, u) == ref.sample_pick(row, 1.0, 64, 1.0, u)
    i64 = ref.sample_candidates(row, 64)[1]
    assert ref.sample_pick(row, 1.0, 0, 1.0, 1 - 2.0 ** -24) == int(i64[63])  # the 64th is reachable ...
    assert ref.sample_pick(row, 1.0, 63, 1.0, 1 - 2.0 ** -24) == int(i64[62])  # ... and only with k = 64
    assert ref.sample_candidates(torch.randn(50), 0)[1].numel() == 50          # a short row has fewer


def test_sample_pick_tie_at_kth_place_keeps_lower_index():
    row = torch.full((40,), -5.0)
    row[2], row[7], row[9], row[5] = 10.0, 9.0, 8.0, 8.0
    assert ref.sample_candidates(row, 3)[1].tolist() == [2, 7, 5]
    assert ref.sample_candidates(row, 4)[1].tolist() == [2, 7, 5, 9]
    picks = {ref.sample_pick(row, 1.0, 3, 1.0, (j + 0.5) / 512) for j in range(512)} | \
            {ref.sample_pick(row, 1.0, 3, 1.0, u) for u in U_SWEEP}
    assert picks == {2, 7, 5}
    assert ref.sample_pick(row, 1.0, 3, 1.0, 1.5) == 5  # fallback: the last kept candidate


def test_sample_pick_tiny_temperature_is_argmax():
    torch.manual_seed(14)
    row = torch.randn(2000) * 3
    assert {ref.sample_pick(row, 1e-6, 40, 0.9, u) for u in U_SWEEP} == {int(row.argmax())}
    assert {ref.sample_pick(row, 1e-6, 0, 1.0, u) for u in U_SWEEP[:-2]} == {int(row.argmax())}


@pytest.mark.parametrize("j", [1, 2, 3])
def test_sample_pick_never_picks_minus_inf(j):
    row = torch.full((300,), float("-inf"))
    finite = [257, 3, 100][:j]
    for n, t in enumerate(finite):
        row[t] = 1.0 - 0.5 * n
    for K, P in ((0, 1.0), (40, 0.9), (2, 1.0), (64, 1.0 + M)):
        for u in U_SWEEP + [(i + 0.5) / 64 for i in range(64)]:
            assert ref.sample_pick(row, 1.0, K, P, u) in finite
        assert ref.sample_pick_set(row, 1.0, K, P, 1 - 2.0 ** -24, M) <= set(finite)
    assert ref.sample_pick(row, 1.0, 0, 1.0, 1.5) == finite[-1]  # fallback stops at the last finite candidate


# -------------------------------------------------------------------------------------------------- decided share
@pytest.mark.parametrize("fi", range(len(FAMILIES)))
def test_decided_share_of_gpu_families(fi):
    """The reference alone: at most 5% of a family's draws may be left undecided by the margin, so the GPU test
    (which must match every decided draw exactly) cannot hide behind its slack."""
    logits, temp, topk, topp, seeds, gen0 = family_case(fi)
    sets = pick_sets(logits, temp, topk, topp, seeds, gen0)
    undecided = sum(len(s) > 1 for s in sets) / len(sets)
    print(f"family {FAMILIES[fi]}: undecided share {undecided:.4f}")
    assert undecided <= 0.05
