#!/usr/bin/env python
"""Price a drain policy of the LJ tile kernel (uammd_amd/csrc/lj_tile.hip, tile_words) on the CPU before it is built.

The traversal is bound by vector-instruction issue, and the drain loop runs, per pass of 32 owners, as many iterations as
its BUSIEST lane needs.  This script rebuilds, for sampled x-pairs of a configuration, exactly what a wave of the brick kernel drains —
the candidate order (three runs = the planes dz = -1, 0, 1; in each the rows dy = -1, 0, 1 of the four cells x0 - 1 .. x0 + 2), the
words of 64 slots (a run's last word is partial), the hit bits of the half-precision distance test with the kernel's margin, and the
split of an owner's candidates between its two lanes (bit j from the top of lane h's word = slot 2 j + h) — and walks the loop lane by
lane under each policy:

  today    one word advance at the top of an iteration, then the two highest bits of THAT word (the kernel until the two-advance drain)
  pop3     the same with three bits per iteration (built and measured once, DESIGN 9: 87 instructions per iteration)
  either   a word advance allowed in front of EITHER pair (the kernel now)
  idle2    a second advance only when the first did not fire

It prints iterations per pass (mean over passes of the maximum over the 64 lanes), the ratio to `today`, and the ratio of issued drain
instructions when an iteration of the policy costs X more vector instructions than today's BASE: ratio * (BASE + X) / BASE.
The absolute count comes out ~10 % above the GPU's measured one (the order of particles inside a cell differs); the RATIOS are what the
model is for: pop3 / today is 0.77 here against 14.5 / 18.9 = 0.77 measured.

usage: python tools/drain_model.py [positions.npy] [--box L] [--pairs 800] [--x 6] [--base 57]
(positions: N x 3 or N x 4 float32; default the melted liquid tests/golden/lj_melt_21952.npy, rho* = 0.8, T = 1)"""
import argparse
import os

import numpy as np

POLICIES = ("today", "pop3", "either", "idle2")
MARGIN = 9.5e-3          # tile_margin (units of the largest cell edge, squared)


def walk(words, policy):
    """One lane's drain.  words: its 32-bit hit words in order.  Returns (iterations, [(word index, bit from the top), ...] in the order
    the bits are consumed).  An iteration counts while the lane took a bit in it or still has words left behind it: what keeps the
    kernel's loop running (`ballot(live) | more`)."""
    nW = len(words)
    if nW == 0:
        return 0, []
    npop = 3 if policy == "pop3" else 2
    wi, cw = 0, int(words[0])
    seq, iters = [], 0
    while True:
        took = False
        fired = False
        for k in range(npop):
            may = k == 0 or policy == "either" or (policy == "idle2" and not fired)
            if may and cw == 0 and wi < nW - 1:
                wi += 1
                cw = int(words[wi])
                fired = fired or k == 0
            if cw:
                b = 32 - cw.bit_length()
                cw &= ~(0x80000000 >> b)
                seq.append((wi, b))
                took = True
        if not (took or wi < nW - 1):
            return iters, seq
        iters += 1


def rtz_half(x):
    """float32 -> the half-precision value rounded toward zero (v_cvt_pkrtz), as float32"""
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


class Tiles:
    def __init__(self, pos, L, rc=2.5, cells=None):
        self.L = np.broadcast_to(np.asarray(L, np.float64), (3,)).copy()
        self.n = np.array(cells if cells is not None else np.floor(self.L / rc), int)
        self.edge = self.L / self.n
        self.rc = rc
        p = np.asarray(pos, np.float64)[:, :3]
        self.p = p - np.floor(p / self.L + 0.5) * self.L            # in [-L/2, L/2)
        c = np.minimum(((self.p + self.L / 2) / self.edge).astype(int), self.n - 1)
        flat = c[:, 0] + self.n[0] * (c[:, 1] + self.n[1] * c[:, 2])
        self.order = np.argsort(flat, kind="stable")
        self.start = np.searchsorted(flat[self.order], np.arange(self.n.prod() + 1))

    def cell(self, x, y, z):
        x, y, z = x % self.n[0], y % self.n[1], z % self.n[2]
        f = x + self.n[0] * (y + self.n[1] * z)
        return self.order[self.start[f]:self.start[f + 1]]

    def passes(self, x0, ty, tz):
        """the hit words of every pass of 32 owners of the pair (x0, x0 + 1; ty; tz): a list of uint32 arrays [64 lanes][nW]"""
        own = np.concatenate([self.cell(x0, ty, tz), self.cell(x0 + 1, ty, tz)]) if x0 + 1 < self.n[0] else self.cell(x0, ty, tz)
        if len(own) == 0:
            return []
        runs = [np.concatenate([self.cell(x0 - 1 + dx, ty + dy, tz + dz) for dy in (-1, 0, 1) for dx in range(4)]) for dz in (-1, 0, 1)]
        centre = np.array([(x0 + 1) * self.edge[0], (ty + 0.5) * self.edge[1], (tz + 0.5) * self.edge[2]]) - self.L / 2
        s = 1.0 / self.edge.max()

        def scaled(idx):
            d = (self.p[idx] - centre) * s
            Ls = self.L * s
            return rtz_half((d - np.floor(d / Ls + 0.5) * Ls).astype(np.float32))
        a = scaled(own)
        thr = np.float32(self.rc * self.rc * s * s + MARGIN)
        words = []                                                   # per word: bool [owners][64 slots]
        for r in runs:
            if len(r) == 0:
                continue
            b = scaled(r)
            hit = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) < thr
            for k in range(0, len(r), 64):
                h = np.zeros((len(own), 64), bool)
                h[:, :min(64, len(r) - k)] = hit[:, k:k + 64]
                words.append(h)
        w = np.stack(words, 1)                                       # [owners][nW][64]
        wt = (1 << np.arange(31, -1, -1, dtype=np.uint64))
        out = []
        for o0 in range(0, len(own), 32):
            lanes = np.zeros((64, w.shape[1]), np.uint32)
            blk = w[o0:o0 + 32]
            for h in (0, 1):
                lanes[32 * h:32 * h + len(blk)] = (blk[:, :, h::2] * wt).sum(-1).astype(np.uint32)
            out.append(lanes)
        return out


def model(tiles, npairs, seed=1):
    rng = np.random.default_rng(seed)
    npx = (tiles.n[0] + 1) // 2
    allp = [(2 * px, y, z) for z in range(tiles.n[2]) for y in range(tiles.n[1]) for px in range(npx)]
    pick = rng.permutation(len(allp))[:npairs]
    tot, hits, npass = {p: 0 for p in POLICIES}, 0, 0
    for i in pick:
        for lanes in tiles.passes(*allp[i]):
            npass += 1
            hits += sum(bin(int(v)).count("1") for v in lanes.ravel())
            for pol in POLICIES:
                tot[pol] += max(walk(l, pol)[0] for l in lanes)
    return {p: tot[p] / max(npass, 1) for p in POLICIES}, hits / max(64 * npass, 1), npass


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("positions", nargs="?", default=os.path.join(root, "tests", "golden", "lj_melt_21952.npy"))
    ap.add_argument("--box", type=float, nargs="+", default=None, help="box edge(s); default: rho* = 0.8 for the file's particle count")
    ap.add_argument("--rc", type=float, default=2.5)
    ap.add_argument("--cells", type=int, nargs=3, default=None, help="default: floor(L / rc) per direction")
    ap.add_argument("--pairs", type=int, default=800, help="x-pairs sampled")
    ap.add_argument("--x", type=float, default=6.0, help="extra vector instructions per iteration of `either` and `idle2`")
    ap.add_argument("--base", type=float, default=57.0, help="vector instructions per iteration today")
    ap.add_argument("--pop3", type=float, default=87.0, help="vector instructions per iteration of pop3")
    a = ap.parse_args()
    pos = np.load(a.positions)
    L = a.box if a.box else [(len(pos) / 0.8) ** (1.0 / 3.0)]
    L = L * 3 if len(L) == 1 else L
    t = Tiles(pos, L, a.rc, a.cells)
    it, hpl, npass = model(t, a.pairs)
    print(f"{len(pos)} particles, box {[round(v, 3) for v in L]}, cells {t.n.tolist()}, {npass} passes, {hpl:.1f} hits per lane (ideal {hpl / 2:.1f} iterations)")
    print(f"{'policy':<8}{'iterations / pass':>20}{'relative':>10}{'instructions':>14}")
    for p in POLICIES:
        cost = a.pop3 if p == "pop3" else a.base + (0.0 if p == "today" else a.x)
        print(f"{p:<8}{it[p]:>20.2f}{it[p] / it['today']:>10.3f}{it[p] * cost / (it['today'] * a.base):>14.3f}")
