"""Restatement of MC_NVT::Anderson (Integrator/MonteCarlo/NVT/Anderson.cu) for the parity tests, written from its description.

Positions move in numpy float32 exactly as the kernels move them (shift by the origin, unshift, displacement, particle pick, the cell of
the shifted new position as utils/Grid.cuh:50-71); the cell contents come from the oracle's cell list on the shifted positions; the
Saru draws from the oracle's integer stream with f = float32(int32(u >> 1)) * 2^-31.  The energy difference and the Metropolis test
are float64.  u(a, b) is the LJ PAIR energy of the type-pair table (0 at r2 == 0 and past the cut-off), so
dH = sum_j u(new, j) - sum_j u(old, j) is the change of the potential energy.

Every try is also classified: it is UNDECIDED when a float32 evaluation of the same rule could decide differently.  With
S = sum_j (|u(old, j)| + |u(new, j)|), a try is undecided if
    dH > 0 and |ln Z + beta dH| < 16 * 2^-24 * beta * S + 1e-6,   or
    dH <= 0 and |dH| < 16 * 2^-24 * S,   or
    some pair has |r2 / rc2 - 1| < 1e-6 (the unshifted potential jumps by 0.016 epsilon there),   or
    the shifted new position lies within 1e-5 cell edges of a cell face.
A run without undecided tries has its decisions determined, and parity with it is bit equality of positions and counters.  The parity
fixtures below were chosen (system seed searched) so that the restatement alone reports zero undecided tries;
tests/test_mc_cpu.py asserts that on the CPU.
"""
import functools
import math

import numpy as np

from util import lattice_positions

F = np.float32
TWO_M31 = F(1.0 / 2147483648.0)
OFFSET3D = [(g & 1, (g >> 1) & 1, (g >> 2) & 1) for g in range(8)]   # Anderson.cuh:93-100


def lj_table(pairs, ntypes):
    """LJFunctor::processPairParameters (Potential.cuh:66-82) in float32; pairs: {(ti, tj): (cutOff, sigma, epsilon, shift)}."""
    tab = np.zeros((ntypes * ntypes, 4), F)
    for (ti, tj), (rc, sigma, eps, shift) in pairs.items():
        rc, sigma, eps = F(rc), F(sigma), F(eps)
        c2, s2 = rc * rc, sigma * sigma
        sh = F(0)
        if shift:
            i2 = s2 / c2
            i6 = i2 * i2 * i2
            sh = eps * F(4) * i6 * (i6 - F(1))
        row = np.array([c2, s2, eps / s2, sh], F)
        tab[ti + ntypes * tj] = row
        tab[tj + ntypes * ti] = row
    return tab


def create_grid(L, rc):
    cd = [int(F(l) / F(rc)) for l in L]
    cd = [c - 1 if c % 2 else c for c in cd]
    if L[2] == 0:
        cd[2] = 1
    return cd


def saru_f(o32, seed, step, icell, n):
    u = o32.saru_u32((seed & 0xFFFFFFFF, step & 0xFFFFFFFF, icell), n)
    return (u >> np.uint32(1)).astype(np.int32).astype(F) * TWO_M31


def host_draws(rng, Lx, is2D):
    """Anderson::updateOrigin and performStep's shuffle from a System::rng() mirror (next() and uniform() only)."""
    maxd = float(F(0.5 * float(F(Lx))))
    u = [rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0)]
    origin = np.array([F(x * maxd) for x in u], F)
    if is2D:
        origin[2] = 0
    n = 4 if is2D else 8
    order = list(range(8))
    for i in range(n - 1):
        j = i + rng.next() % (n - i)
        order[i], order[j] = order[j], order[i]
    return origin, order[:n]


class Grid:
    """utils/Grid.cuh:21-71 and Box.cuh:16-58 in float32."""

    def __init__(self, L, periodic, cellDim):
        self.L = np.asarray(L, F)
        self.per = [bool(p) and l != 0 for p, l in zip(periodic, self.L)]
        self.cd = [int(c) for c in cellDim]
        self.cellSize = np.array([self.L[k] / F(self.cd[k]) for k in range(3)], F)
        with np.errstate(divide="ignore"):
            self.inv = np.array([F(1) / self.cellSize[k] for k in range(3)], F)
            if self.L[2] == 0:
                self.inv[2] = 0
            self.minv = np.array([F(-1) / self.L[k] if self.per[k] else F(0) for k in range(3)], F)

    def cell_fraction(self, r):
        """(p + L/2) / cellSize per axis in float32, p the minimum image of r; the cell is its truncation."""
        out = np.zeros(3, F)
        for k in range(3):
            p = F(r[k])
            if self.per[k]:
                fl = F(math.floor(float(F(float(r[k]) * float(self.minv[k]) + 0.5))))   # floor(fma(r, -1/L, 0.5))
                p = p + fl * self.L[k]
            out[k] = (p + F(0.5) * self.L[k]) * self.inv[k]
        return out

    def get_cell(self, r):
        fr = self.cell_fraction(r)
        c = [int(fr[k]) for k in range(3)]
        return tuple(0 if c[k] == self.cd[k] else c[k] for k in range(3)), fr


def pair_energy(ri, rj, L, per, tab, ntypes):
    """u(ri, rj[:]) in float64: (energies, r2 / rc2)."""
    d = rj[:, :3].astype(np.float64) - ri[:3].astype(np.float64)
    for k in range(3):
        if per[k]:
            Lk = float(L[k])
            d[:, k] += np.floor(d[:, k] * (-1.0 / Lk) + 0.5) * Lk
    r2 = (d * d).sum(1)
    if ntypes == 1:
        p = np.broadcast_to(tab[0].astype(np.float64), (len(rj), 4))
    else:
        ti = np.full(len(rj), int(ri[3]))
        tj = rj[:, 3].astype(np.int64)
        lo, hi = np.minimum(ti, tj), np.maximum(ti, tj)
        idx = np.where((lo >= ntypes) | (hi >= ntypes), 0, lo + ntypes * hi)
        p = tab[idx].astype(np.float64)
    c2, s2, eds2, sh = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        i2 = s2 / r2
        i6 = i2 * i2 * i2
        u = eds2 * s2 * 4.0 * i6 * (i6 - 1.0) - sh
    inside = (r2 != 0.0) & (r2 < c2)
    return np.where(inside, u, 0.0), r2 / c2


def mc_step(o32, pos, L, periodic, cellDim, origin, order, tries, beta, jump, step, seed, tab, ntypes):
    """One forwardTime without the tuning.  Returns (pos, tried[ncells], accepted[ncells], info)."""
    pos = np.ascontiguousarray(pos, F)
    origin = np.asarray(origin, F)
    grid = Grid(L, periodic, cellDim)
    cd = grid.cd
    is2D = cd[2] == 1
    ncells = cd[0] * cd[1] * cd[2]
    shifted = pos.copy()
    shifted[:, :3] = pos[:, :3] + origin
    cl = o32.celllist_build(shifted, np.asarray(L, F), [int(p) for p in grid.per], cd)
    assert cl["error"] == 0
    sp = cl["sortPos"].astype(F).copy()
    sp[:, :3] = sp[:, :3] + (F(-1) * origin)
    start = cl["cellStart"].astype(np.int64) - int(cl["validCell"])
    empty = cl["cellStart"].astype(np.int64) < int(cl["validCell"])
    end = cl["cellEnd"].astype(np.int64)
    tried, accepted = np.zeros(ncells, np.uint32), np.zeros(ncells, np.uint32)
    info = dict(undecided=0, tries=0, out_of_cell=0, visits=np.zeros(ncells, np.int64),
                max_in_cell=int(np.where(empty, 0, end - start).max()), max_neighbourhood=0)
    jump, beta = F(jump), float(F(beta))
    for g in order:
        off = OFFSET3D[g]
        for cz in ([0] if is2D else range(off[2], cd[2], 2)):
            for cy in range(off[1], cd[1], 2):
                for cx in range(off[0], cd[0], 2):
                    icell = cx + cd[0] * (cy + cd[1] * cz)
                    info["visits"][icell] += 1
                    if empty[icell]:
                        continue
                    first, nin = int(start[icell]), int(end[icell] - start[icell])
                    rows = []
                    for k in range(9 if is2D else 27):
                        n = [cx + k % 3 - 1, cy + (k // 3) % 3 - 1, cz if is2D else cz + k // 9 - 1]
                        ok = True
                        for a in range(3):
                            if grid.per[a]:
                                n[a] %= cd[a]
                            elif not 0 <= n[a] < cd[a]:
                                ok = False
                        j = n[0] + cd[0] * (n[1] + cd[1] * n[2])
                        if ok and not empty[j]:
                            rows.extend(range(int(start[j]), int(end[j])))
                    rows = np.array(rows, np.int64)
                    info["max_neighbourhood"] = max(info["max_neighbourhood"], len(rows))
                    f = saru_f(o32, seed, step, icell, 5 * tries)
                    q = 0
                    for _ in range(tries):
                        tried[icell] += 1
                        info["tries"] += 1
                        pick = min(int(f[q] * F(nin)), nin - 1)
                        i = first + pick
                        old = sp[i].copy()
                        d = [jump * (F(2) * f[q + 1] - F(1)), jump * (F(2) * f[q + 2] - F(1)), jump * (F(2) * f[q + 3] - F(1))]
                        q += 4
                        new = old.copy()
                        new[0], new[1] = old[0] + d[0], old[1] + d[1]
                        if not is2D:
                            new[2] = old[2] + d[2]
                        cell, fr = grid.get_cell(new[:3] + origin)
                        near_face = any(abs(float(fr[a]) - round(float(fr[a]))) < 1e-5 for a in range(2 if is2D else 3))
                        if near_face:
                            info["undecided"] += 1
                        if cell != (cx, cy, cz):
                            info["out_of_cell"] += 1
                            continue
                        uo, xo = pair_energy(old, sp[rows], grid.L, grid.per, tab, ntypes)
                        others = sp[rows].copy()
                        others[rows == i] = new
                        un, xn = pair_energy(new, others, grid.L, grid.per, tab, ntypes)
                        dH = float(un.sum() - uo.sum())
                        S = float(np.abs(un).sum() + np.abs(uo).sum())
                        Z = float(f[q])
                        q += 1
                        lnZ = math.log(Z) if Z > 0 else -math.inf
                        if dH > 0:
                            accept = lnZ + beta * dH <= 0
                            und = abs(lnZ + beta * dH) < 16 * 2.0 ** -24 * beta * S + 1e-6
                        else:
                            accept = True
                            und = abs(dH) < 16 * 2.0 ** -24 * S
                        und = und or bool((np.abs(xo - 1.0) < 1e-6).any() or (np.abs(xn - 1.0) < 1e-6).any())
                        if und and not near_face:
                            info["undecided"] += 1
                        if accept:
                            sp[i] = new
                            accepted[icell] += 1
    out = pos.copy()
    out[cl["index"]] = sp
    return out, tried, accepted, info


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
RC = 2.5


def _packed(n_pack, edge, n_bg, L, seed):
    """n_pack particles on a lattice inside a cube of `edge` around the centre plus a sparse jittered background."""
    rng = np.random.default_rng(seed)
    m = int(math.ceil(n_pack ** (1 / 3)))
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)[:n_pack]
    p = (g + 0.5) / m * edge - edge / 2 + rng.uniform(-0.02, 0.02, (n_pack, 3))
    bg = lattice_positions(n_bg, L, seed=seed + 1, jitter=0.2)
    pos = np.zeros((n_pack + n_bg, 4), F)
    pos[:n_pack, :3] = p
    pos[n_pack:] = bg
    return pos


def _flat(n, L, seed):
    rng = np.random.default_rng(seed)
    m = int(math.ceil(math.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    sel = np.sort(rng.permutation(len(g))[:n])
    pos = np.zeros((n, 4), F)
    pos[:, :2] = (g[sel] + 0.5) / m * L - L / 2 + rng.uniform(-0.1, 0.1, (n, 2))
    return pos


ONE = {(0, 0): (RC, 1.0, 1.0, False)}
ONE_SHIFTED = {(0, 0): (RC, 1.0, 1.0, True)}
TWO = {(0, 0): (RC, 1.0, 1.0, False), (0, 1): (2.0, 0.9, 0.7, True), (1, 1): (2.2, 0.8, 1.3, False)}

# name -> (positions, L, pairs, ntypes, system seed).  Common: T = 1.5, jump 0.15, 10 tries per cell, 3 steps, Saru seed 1234.
FIXTURES = {
    "cube6": (lambda: lattice_positions(1500, 15.0, seed=11, jitter=0.1), (15.0, 15.0, 15.0), ONE, 1, 301),
    "cube6_shifted": (lambda: lattice_positions(1500, 15.0, seed=11, jitter=0.1), (15.0, 15.0, 15.0), ONE_SHIFTED, 1, 301),
    "cube6_two_types": (lambda: lattice_positions(1500, 15.0, seed=11, jitter=0.1, ntypes=2), (15.0, 15.0, 15.0), TWO, 2, 101),
    "cube4": (lambda: lattice_positions(500, 10.0, seed=12, jitter=0.1), (10.0, 10.0, 10.0), ONE, 1, 102),
    "brick": (lambda: lattice_positions(1500, (15.5, 10.2, 20.3), seed=13, jitter=0.1), (15.5, 10.2, 20.3), ONE, 1, 303),
    "flat": (lambda: _flat(250, 20.0, 14), (20.0, 20.0, 0.0), ONE, 1, 204),
    "dilute": (lambda: lattice_positions(40, 15.0, seed=15, jitter=0.3), (15.0, 15.0, 15.0), ONE, 1, 105),
    "packed": (lambda: _packed(120, 2.0, 200, 15.0, 16), (15.0, 15.0, 15.0), ONE, 1, 206),
}
TEMPERATURE, JUMP, TRIES, STEPS, SARU_SEED = 1.5, 0.15, 10, 3, 1234


class Fixture:
    def __init__(self, name):
        make, L, pairs, ntypes, sysseed = FIXTURES[name]
        self.name, self.pos, self.L, self.pairs, self.ntypes, self.sysseed = name, make(), L, pairs, ntypes, sysseed
        self.table = lj_table(pairs, ntypes)
        self.rc = max(p[0] for p in pairs.values())
        self.cellDim = create_grid(L, self.rc)
        self.is2D = L[2] == 0
        self.periodic = [True, True, not self.is2D]


@functools.lru_cache(maxsize=None)
def reference_run(name, sysseed=None):
    """The restatement's trajectory of a fixture: one (pos, tried, accepted, info, origin, order) per step, counters never reset.
    Computed once per process and shared; the arrays are read-only."""
    import oracle
    from uammd_amd.md import Xorshift128plus
    o32 = oracle.get("f32")
    fx = Fixture(name)
    rng = Xorshift128plus()
    rng.set_seed(fx.sysseed if sysseed is None else sysseed)
    pos = fx.pos
    beta = F(1.0 / float(F(TEMPERATURE)))
    T, A = 0, 0
    out = []
    for step in range(1, STEPS + 1):
        origin, order = host_draws(rng, fx.L[0], fx.is2D)
        pos, t, a, info = mc_step(o32, pos, fx.L, fx.periodic, fx.cellDim, origin, order, TRIES, beta, JUMP, step, SARU_SEED, fx.table,
                                  fx.ntypes)
        T, A = T + t, A + a
        for arr in (pos, T, A):
            arr.setflags(write=False)
        out.append((pos, T, A, info, origin, order))
    return out
