"""The drain model (tools/drain_model.py) walks a lane's hit words the way the tile kernel's drain loop does, under several policies.
Whatever the policy, a lane consumes exactly its own bits, each once, from the top of a word and word after word — that is what keeps
the kernel's sums bit-identical — and a word advance in front of either pair never needs more iterations than one advance per iteration."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import drain_model as dm  # noqa: E402


def _expected(words):
    return [(w, b) for w, v in enumerate(words) for b in range(32) if (int(v) >> (31 - b)) & 1]


def _random_lanes():
    rng = np.random.default_rng(7)
    lanes = [[0], [0, 0, 0, 0], [1 << 31], [1], [0xFFFFFFFF], [0, 0, 0, 1 << 31], [1 << 31, 0, 0, 0], [0, 1, 0, 1, 0, 1],
             [1, 1 << 31, 1 << 15, 1 << 7] * 3, [0xFFFFFFFF] * 12, []]
    for nW in (1, 2, 3, 9, 12):
        for mean_bits in (0.3, 1.0, 3.0, 8.0):
            for _ in range(12):
                counts = np.minimum(rng.poisson(mean_bits, nW), 32)
                lanes.append([int(sum(1 << int(b) for b in rng.choice(32, int(c), replace=False))) for c in counts])
    return lanes


LANES = _random_lanes()


@pytest.mark.parametrize("policy", dm.POLICIES)
def test_every_policy_consumes_each_bit_once_and_in_order(policy):
    for words in LANES:
        iters, seq = dm.walk(words, policy)
        assert seq == _expected(words), (policy, words)
        nbits = len(seq)
        per = 3 if policy == "pop3" else 2
        assert iters >= -(-nbits // per)                         # no more than `per` bits per iteration
        assert iters <= nbits + len(words)                       # and the walk ends


def test_advance_in_front_of_either_pair_never_takes_more_iterations():
    for words in LANES:
        today, either, idle2 = (dm.walk(words, p)[0] for p in ("today", "either", "idle2"))
        assert either <= idle2 <= today, words


def test_iteration_counts_of_hand_walked_lanes():
    top = 1 << 31
    # one bit, two empty words, one bit: today 4 iterations (bit | advance | advance | advance + bit), either 2 (bit + advance |
    # advance + advance + bit: the last word is reached in front of the second pair of the second iteration)
    assert dm.walk([top, 0, 0, top], "today")[0] == 4
    assert dm.walk([top, 0, 0, top], "either")[0] == 2
    # three bits, three bits: today leaves a dead slot per word (2 + 2), either pairs across the boundary (3)
    assert dm.walk([7 << 29, 7 << 29], "today")[0] == 4
    assert dm.walk([7 << 29, 7 << 29], "either")[0] == 3
    assert dm.walk([7 << 29, 7 << 29], "pop3")[0] == 2
    # an all-empty lane still walks its words: one advance per iteration today, two now; the last word costs no iteration of its own
    assert dm.walk([0] * 9, "today")[0] == 7 and dm.walk([0] * 9, "either")[0] == 3
    assert dm.walk([0], "today")[0] == 0 and dm.walk([top], "either")[0] == 1


def test_words_rebuilt_from_positions_hold_every_pair_inside_the_cutoff():
    """The geometry half of the model on a small liquid-like box: every pair within the cut-off is a set bit of exactly one lane of its
    owner, a lane's bits are the even or the odd slots, and the model's ordering either <= today holds for whole passes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import lattice_positions
    n, L, rc = 2700, 15.0, 2.5
    pos = lattice_positions(n, L, seed=3, jitter=0.3)
    t = dm.Tiles(pos, [L] * 3, rc)
    assert t.n.tolist() == [6, 6, 6]
    p = t.p
    for (x0, ty, tz) in [(0, 0, 0), (2, 3, 5), (4, 5, 2)]:
        own = np.concatenate([t.cell(x0, ty, tz), t.cell(x0 + 1, ty, tz)])
        passes = t.passes(x0, ty, tz)
        assert len(passes) == -(-len(own) // 32)
        d = p[own][:, None, :] - p[None, :, :]
        d -= np.round(d / L) * L
        inside = ((d ** 2).sum(-1) < rc * rc).sum(1)             # (the owner itself included: it is a candidate, and a hit)
        for k, lanes in enumerate(passes):
            bits = np.array([[bin(int(v)).count("1") for v in l] for l in lanes]).sum(1)
            per_owner = bits[:32] + bits[32:]
            m = min(32, len(own) - 32 * k)
            assert np.all(per_owner[:m] >= inside[32 * k:32 * k + m])          # the prefilter is a superset ...
            assert np.all(per_owner[:m] <= inside[32 * k:32 * k + m] + 6)      # ... by a thin shell
            assert np.all(per_owner[m:] == 0)
            assert max(dm.walk(l, "either")[0] for l in lanes) <= max(dm.walk(l, "today")[0] for l in lanes)


def test_model_on_the_melted_liquid_reproduces_the_priced_ratios():
    """tests/golden/lj_melt_21952.npy (rho* = 0.8, T = 1, 12^3 cells): the ratios DESIGN 5.2 quotes, on a sample small enough for a test."""
    path = os.path.join(ROOT, "tests", "golden", "lj_melt_21952.npy")
    pos = np.load(path)
    assert pos.shape == (21952, 3) and pos.dtype == np.float32
    t = dm.Tiles(pos, [(21952 / 0.8) ** (1 / 3)] * 3)
    assert t.n.tolist() == [12, 12, 12]
    it, hits, npass = dm.model(t, 120)
    assert 18.0 < hits < 24.0                                    # ~27 per lane with an owner, ~25 owners of 32
    assert 0.82 < it["either"] / it["today"] < 0.90              # 0.860 on 800 pairs
    assert 0.74 < it["pop3"] / it["today"] < 0.82                # 0.767; measured on the GPU: 14.5 / 18.9 = 0.77
    assert it["either"] < it["idle2"] < it["today"]
