"""Configurations for the tile kernel's drain (tests/test_gpu_lj_tile_drain.py and tools/record_lj_tile_drain_golden.py build them from
here, so the recorded forces and the test see the same bytes).  All are 6 x 6 x 6 cells of edge 2.5 or a little off that: the smallest
boxes that have interior and face tiles, more than one brick, and every path of the drain's word walk."""
import functools
import hashlib

import numpy as np

from util import lattice_positions

RC = 2.5
KMAXW, BRICK_CAP = 12, 1024          # lj_tile.hip: hit words one wave holds per pass, candidate slots of a brick
BRICK, SOLO, EXACT = 8, 10, 9        # uammd_celllist_transverse_lj algorithms: four waves per brick, one wave per x-pair, the reference's order


def _scatter(n, L, seed, dmin=0.9):
    """n uniform random points, none closer than dmin to another (minimum image)"""
    rng = np.random.default_rng(seed)
    L = np.broadcast_to(np.asarray(L, np.float64), (3,))
    pts = np.zeros((0, 3))
    while len(pts) < n:
        c = rng.uniform(-L / 2, L / 2, 3)
        d = pts - c
        d -= np.round(d / L) * L
        if len(pts) == 0 or (d * d).sum(1).min() >= dmin * dmin:
            pts = np.concatenate([pts, c[None]])
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = pts
    return pos


def _by_cell(counts, seed, dmin=0.7, edge=RC):
    """counts[x, y, z] particles placed uniformly inside cell (x, y, z), 0.05 off its faces, none closer than dmin to another"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    L = np.array(counts.shape) * edge
    pts = np.zeros((0, 3))
    for z in range(counts.shape[2]):
        for y in range(counts.shape[1]):
            for x in range(counts.shape[0]):
                k = 0
                while k < counts[x, y, z]:
                    c = (np.array([x, y, z]) + rng.uniform(0.02, 0.98, 3)) * edge - L / 2
                    d = pts - c
                    if len(pts) == 0 or (d * d).sum(1).min() >= dmin * dmin:
                        pts = np.concatenate([pts, c[None]])
                        k += 1
    pos = np.zeros((len(pts), 4), np.float32)
    pos[:, :3] = pts[rng.permutation(len(pts))]
    return pos


def kmaxw_counts():
    """One wave of brick (1, 1, 1) — cells 2..3 along each direction, wave (wy, wz) = (0, 0): rows y = 1..3 of the planes z = 1..3,
    cells x = 1..4 — gets three uneven runs of 193, 200 and 230 candidates = 4 + 4 + 4 = kMaxW words, its pair holds exactly 32 owners,
    the rest of the box one particle per cell: the brick stages 623 + 28 candidates and does not fall back."""
    c = np.ones((6, 6, 6), int)
    c[1:5, 1:4, 1:4] = 16
    c[1, 1, 1] += 1                   # 193
    c[1, 1:3, 2] += 4                 # 200
    c[1:5, 1:4, 3] = 19
    c[1, 1, 3] += 2                   # 230
    return c


def wave_words(counts, periodic):
    """words per wave of the brick kernel (sum over the wave's three runs of ceil(run length / 64)) and candidates per brick, from cell
    counts: {(bx, by, bz, wy, wz): nW}, {(bx, by, bz): C}"""
    n = counts.shape

    def cnt(x, y, z):
        if not periodic and not (0 <= x < n[0] and 0 <= y < n[1] and 0 <= z < n[2]):
            return 0
        return int(counts[x % n[0], y % n[1], z % n[2]])
    words, cands = {}, {}
    for bz in range((n[2] + 1) // 2):
        for by in range((n[1] + 1) // 2):
            for bx in range((n[0] + 1) // 2):
                x0, y0, z0 = 2 * bx, 2 * by, 2 * bz
                cands[bx, by, bz] = sum(cnt(x0 - 1 + i, y0 - 1 + j, z0 - 1 + k) for i in range(4) for j in range(4) for k in range(4))
                for wz in (0, 1):
                    for wy in (0, 1):
                        runs = [sum(cnt(x0 - 1 + i, y0 - 1 + wy + j, z0 - 1 + wz + p) for i in range(4) for j in range(3)) for p in range(3)]
                        words[bx, by, bz, wy, wz] = sum((r + 63) // 64 for r in runs)
    return words, cands


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(pos, L, periodic, fev): positions N x 4 float32, box, periodicity, (force, energy, virial) wanted"""
    per, fev, L = (1, 1, 1), (True, False, False), 15.0
    if name in ("liquid", "liquid-ev"):                  # periodic liquid, rho* = 0.8: face tiles with the minimum image and interior tiles
        pos = lattice_positions(2700, L, seed=21, jitter=0.12)
        fev = (True, True, True) if name == "liquid-ev" else fev
    elif name == "liquid-open":
        pos, per = lattice_positions(2700, L, seed=21, jitter=0.12), (0, 0, 0)
    elif name == "rho0.05":                              # most words hold no bit or one: chains of empty words, second advances in a row
        pos = _scatter(168, L, seed=22)
    elif name == "rho0.2":
        pos = _scatter(675, L, seed=23)
    elif name == "odd-x":                                # 5 x 6 x 6 cells: the last x-pair is a single cell
        L = (12.5, 15.0, 15.0)
        pos = lattice_positions(2250, L, seed=24, jitter=0.12)
    elif name == "kmaxw":
        pos, per = _by_cell(kmaxw_counts(), seed=25), (0, 0, 0)
    elif name == "fallback":                             # rho* = 1.5: every brick's 64 cells hold ~1500 candidates > kBrickCap
        pos = lattice_positions(5062, L, seed=26, jitter=0.05)
    elif name == "owners40":                             # one x-pair with 40 owners (a second pass of 8), sparse around it
        c = np.full((6, 6, 6), 2)
        c[2:4, 2, 2] = 20
        pos, per = _by_cell(c, seed=27), (0, 0, 0)
    elif name == "single-owner":                         # waves whose pair holds one particle, in the first or in the second cell
        c = np.full((6, 6, 6), 8)
        c[2, 2, 2], c[3, 2, 2] = 1, 0
        c[4, 3, 3], c[5, 3, 3] = 0, 1
        pos = _by_cell(c, seed=28)
    else:
        raise KeyError(name)
    pos.setflags(write=False)
    return dict(pos=pos, L=L, periodic=per, fev=fev)


# (case, algorithm): both kernels on the liquid boxes and wherever the one-wave kernel walks other words than the brick kernel
RUNS = [("liquid", BRICK), ("liquid", SOLO), ("liquid-ev", BRICK), ("liquid-open", BRICK), ("liquid-open", SOLO), ("rho0.05", BRICK),
        ("rho0.05", SOLO), ("rho0.2", BRICK), ("odd-x", BRICK), ("odd-x", SOLO), ("kmaxw", BRICK), ("fallback", BRICK), ("owners40", BRICK),
        ("owners40", SOLO), ("single-owner", BRICK), ("single-owner", SOLO)]


def key(name, algo):
    return f"{name}/{'brick' if algo == BRICK else 'solo'}"


def digest(pos):
    return hashlib.sha1(np.ascontiguousarray(pos).tobytes()).hexdigest()


def run(hip, torch, c, algo, stats=False):
    """-> (force N x 4, energy or None, virial or None, tile stats or None, cell counts) of one traversal with `algo`"""
    pos = c["pos"]
    n = len(pos)
    box = hip.Box(c["L"], c["periodic"])
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(RC, 1.0, 1.0, False))
    cl = hip.CellList()
    cd, ubox = hip.CellList.create_update_grid(box, RC)
    cl.update_grid(torch.from_numpy(pos.copy()).cuda(), ubox, cd)
    f = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    e = torch.zeros(n, dtype=torch.float32, device="cuda") if c["fev"][1] else None
    v = torch.zeros(n, dtype=torch.float32, device="cuda") if c["fev"][2] else None
    if stats:
        cl.tile_stats(True)
    cl.transverse_lj(pot.device_table(), 1, box, f, e, v, None, algo)
    torch.cuda.synchronize()
    st = cl.tile_stats(False) if stats else None
    return f.cpu().numpy(), None if e is None else e.cpu().numpy(), None if v is None else v.cpu().numpy(), st, list(cd)
