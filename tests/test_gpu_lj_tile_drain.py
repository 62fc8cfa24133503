"""The tile kernels' drain (uammd_amd/csrc/lj_tile.hip, tile_words) with a word advance in front of either pair of an iteration.

The change moves no pair to another lane and keeps every lane's order of evaluation, so nothing may move: every case compares the
forces WORD FOR WORD with forces recorded from the parent commit (tests/golden/lj_tile_drain_parent.npz, which names the commit; written
by tools/record_lj_tile_drain_golden.py), and with the exact kernel (the reference's summation order) at the bar of tests/test_gpu_lj_tile.py.
Shapes: 6 x 6 x 6 cells — interior and face tiles, 27 bricks — at liquid density, periodic and open, through the brick kernel and the
one-wave kernel; dilute boxes whose hit words hold no bit or one (chains of empty words, second advances in consecutive iterations);
an odd number of cells along x; a wave that fills all kMaxW hit words (the look-ahead's clamp) in a brick that does not fall back; bricks
that do; a pair with a second pass of owners; pairs with one owner."""
import os

import numpy as np
import pytest
import torch

import lj_tile_drain_cases as dc
from test_gpu_lj import _check_force

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lj_tile_drain_parent.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert len(str(g["parent_commit"])) == 40
    return g


@pytest.fixture(scope="module")
def exact(hip):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = dc.run(hip, torch, dc.case(name), dc.EXACT)[:3]
        return cache[name]
    return get


def _same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name,algo", dc.RUNS, ids=[dc.key(n, a) for n, a in dc.RUNS])
def test_drain_forces_are_the_parents_bits_and_agree_with_the_exact_kernel(hip, golden, exact, name, algo):
    c = dc.case(name)
    k = dc.key(name, algo)
    assert str(golden[k + "/pos_sha1"]) == dc.digest(c["pos"]), "the configuration is not the one the forces were recorded on"
    f, e, v, st, cd = dc.run(hip, torch, c, algo, stats=True)
    assert cd == ([5, 6, 6] if name == "odd-x" else [6, 6, 6])
    # ---- the paths the case is there for ----
    if algo == dc.BRICK:
        assert st["bricks"] == 27
        if name == "fallback":
            assert st["fallback_bricks"] == 27
        elif name in ("kmaxw", "liquid", "liquid-ev", "liquid-open", "owners40", "single-owner"):
            assert st["fallback_bricks"] == 0
    if name in ("kmaxw", "owners40", "single-owner"):
        p = c["pos"][:, :3].astype(np.float64)
        cell = np.floor((p + 7.5) / dc.RC).astype(int)
        counts = np.zeros((6, 6, 6), int)
        np.add.at(counts, tuple(cell.T), 1)
        words, cands = dc.wave_words(counts, periodic=c["periodic"][0] == 1)
        assert max(cands.values()) <= dc.BRICK_CAP
        if name == "kmaxw":
            assert np.array_equal(counts, dc.kmaxw_counts())
            assert words[1, 1, 1, 0, 0] == dc.KMAXW == max(words.values())
        if name == "owners40":
            assert counts[2, 2, 2] + counts[3, 2, 2] == 40
        if name == "single-owner":
            assert (counts[2, 2, 2], counts[3, 2, 2], counts[4, 3, 3], counts[5, 3, 3]) == (1, 0, 0, 1)
    # ---- the parent's bits ----
    assert np.all(f[:, 3] == 0)
    nd = int((f[:, :3].view(np.uint32) != golden[k + "/f"].view(np.uint32)).sum())
    print(f"[{k}] N {len(f)}; words differing from the parent's ({str(golden['parent_commit'])[:7]}): {nd} / {f[:, :3].size}")
    assert nd == 0
    # ---- the exact kernel ----
    xf, xe, xv = exact(name)
    _check_force(f, xf, k + " vs exact", reordered=True)
    if e is not None:
        assert _same_words(e, golden[k + "/e"]) and _same_words(v, golden[k + "/v"])
        assert np.abs(e - xe).max() <= 1e-5 * np.abs(xe).max()
        assert np.abs(v - xv).max() <= 1e-5 * np.abs(xv).max()
