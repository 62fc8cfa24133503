"""The counting build's stable placement (k_rank_scatter2) ranks every member of a cell inside an LDS window of the provisional
slots around its workgroup: the workgroup's own KBLOCK slots and HALO more on either side; a cell that runs on past the window is
followed in global memory.  It finds a cell's ends from the head bit k_members sets in a cell's first slot, and writes sortHash itself
from the position it has gathered.  Every case builds one input twice, on a default CellList (counting build: the key spaces used here, at most 2^15
keys, are below 8 N + 4096) and on one forced to the rocPRIM radix build, and compares index, hash (sortHash), sortPos, cellStart
and cellEnd word for word.  cellStart / cellEnd are compared in canonical form (tests/util.py): the entries of EMPTY cells are not
part of the contract, the radix build never writes them.

Sizes are the smallest at which the placement takes another path: around one workgroup, around the window's edges, cells that
straddle an edge by less and by more than the halo, a cell longer than any window, a cell that is the whole list."""
import numpy as np
import pytest
import torch

from util import canon_cell_tables, lattice_positions

pytestmark = pytest.mark.gpu

KBLOCK = 256  # kBlock of uammd_amd/csrc/celllist.hip: slots per workgroup of k_rank_scatter2
HALO = 32     # kRankHalo: slots beside them that the window also holds
RC = 2.5


def _grid(hip, ncell):
    L = RC * ncell + 0.5
    box = hip.Box(L)
    cd, ubox = hip.CellList.create_update_grid(box, RC)
    assert list(cd) == [ncell] * 3
    return L, box, cd, ubox


def _pos4(xyz):
    pos = np.zeros((len(xyz), 4), np.float32)
    pos[:, :3] = xyz
    return pos


def _uniform(n, L, seed):
    return _pos4(np.random.default_rng(seed).uniform(-L / 2, L / 2, (n, 3)))


def _in_cell(rng, cell, n, L, ncell):
    """n points well inside cell (cx, cy, cz) of the ncell^3 grid over [-L/2, L/2)^3"""
    side = L / ncell
    return (np.asarray(cell) + rng.uniform(0.05, 0.95, (n, 3))) * side - L / 2


def _same(a, b, tag="", epoch=True):
    if epoch:
        assert a["validCell"] == b["validCell"], tag
    for k in ("index", "hash"):
        assert np.array_equal(a[k], b[k]), (tag, k)
    assert np.array_equal(a["sortPos"].view(np.uint32), b["sortPos"].view(np.uint32)), (tag, "sortPos")
    sa, ea = canon_cell_tables(a)
    sb, eb = canon_cell_tables(b)
    assert np.array_equal(sa, sb), (tag, "cellStart")
    assert np.array_equal(ea, eb), (tag, "cellEnd")


def _build_pair(hip, pos, ubox, cd):
    cl, ref = hip.CellList(), hip.CellList()
    ref.set_option("force_radix", 1)
    d_pos = torch.from_numpy(pos).cuda()
    cl.update_grid(d_pos, ubox, cd)
    ref.update_grid(d_pos, ubox, cd)
    a, b = cl.to_host(), ref.to_host()
    _same(a, b)
    assert np.array_equal(np.sort(a["index"]), np.arange(len(pos)))
    return a, cl, ref, d_pos


def _cell_range(lst, cell):
    cd = lst["cellDim"]
    c = cell[0] + cd[0] * (cell[1] + cd[1] * cell[2])
    return int(lst["cellStart"][c]) - lst["validCell"], int(lst["cellEnd"][c])


@pytest.mark.parametrize("n", [1, 63, KBLOCK - 1, KBLOCK, KBLOCK + 1, KBLOCK + HALO - 1, KBLOCK + HALO, KBLOCK + HALO + 1,
                               3 * KBLOCK + 17])
def test_sizes_around_a_workgroup(hip, n):
    L, _, cd, ubox = _grid(hip, 6)
    _build_pair(hip, _uniform(n, L, seed=n), ubox, cd)


@pytest.mark.parametrize("before,inside", [(KBLOCK - 5, 11), (KBLOCK - 50, 100), (KBLOCK - HALO, 2 * HALO), (KBLOCK - HALO - 1, 2 * HALO + 2),
                                           (KBLOCK - 4, 4), (KBLOCK, 7)],
                         ids=["within_halo", "past_halo_both_sides", "exactly_the_halo", "one_past_the_halo", "ends_on_the_edge",
                              "starts_on_the_edge"])
def test_cell_across_a_window_edge(hip, before, inside):
    """N = 2 KBLOCK.  Morton keys 0, 1, 2 are the cells (0,0,0), (1,0,0), (0,1,0): `before` particles in the first put the `inside`
    particles of the second on the slots [before, before + inside), across or against the edge between the two workgroups."""
    L, _, cd, ubox = _grid(hip, 6)
    n = 2 * KBLOCK
    rng = np.random.default_rng(before)
    xyz = np.concatenate([_in_cell(rng, (0, 0, 0), before, L, 6), _in_cell(rng, (1, 0, 0), inside, L, 6),
                          _in_cell(rng, (0, 1, 0), n - before - inside, L, 6)])
    a, *_ = _build_pair(hip, _pos4(xyz[rng.permutation(n)]), ubox, cd)
    assert _cell_range(a, (0, 0, 0)) == (0, before)
    assert _cell_range(a, (1, 0, 0)) == (before, before + inside)
    assert _cell_range(a, (0, 1, 0)) == (before + inside, n)


@pytest.mark.parametrize("n", [4096, 1500])
def test_cell_longer_than_a_window(hip, n):
    """1500 particles in one cell of a 4^3 grid (every one of its threads leaves the window on one side or both), the rest uniform; with
    N = 1500 that cell is the whole list."""
    L, _, cd, ubox = _grid(hip, 4)
    rng = np.random.default_rng(n)
    xyz = np.concatenate([_in_cell(rng, (1, 2, 1), 1500, L, 4), rng.uniform(-L / 2, L / 2, (n - 1500, 3))])
    a, *_ = _build_pair(hip, _pos4(xyz[rng.permutation(n)]), ubox, cd)
    s, e = _cell_range(a, (1, 2, 1))
    assert e - s >= 1500
    if n == 1500:
        assert (s, e) == (0, n)
        assert np.array_equal(a["index"], np.arange(n))  # stable: one cell, ascending particle index


@pytest.fixture(scope="module")
def liquid(hip):
    """20 000 uniform particles in 20^3 cells, in random memory order, and the order a sort by cell gives them"""
    L, _, cd, ubox = _grid(hip, 20)
    pos = _uniform(20000, L, seed=5)
    a, *_ = _build_pair(hip, pos, ubox, cd)
    return pos, a["index"].copy(), ubox, cd


@pytest.mark.parametrize("order", ["random", "sorted", "sorted_10pc_swapped"])
def test_order_of_the_input(hip, liquid, order):
    """random: every key spans many workgroups of the hash kernel, the provisional ranks are fully scrambled; sorted: they are already
    the stable ones; in between: what a simulation has some hundred steps after a sort."""
    pos, by_cell, ubox, cd = liquid
    n = len(pos)
    if order != "random":
        pos = pos[by_cell]
    if order == "sorted_10pc_swapped":
        rng = np.random.default_rng(11)
        rows = rng.choice(n, n // 10, replace=False)
        pos = pos.copy()
        pos[rows] = pos[rng.permutation(rows)]
    a, *_ = _build_pair(hip, np.ascontiguousarray(pos), ubox, cd)
    if order == "sorted":
        assert np.array_equal(a["index"], np.arange(n))


def test_empty_cells_and_particles_outside_the_box(hip):
    """N = 500 in 12^3 cells: most cells are empty.  Some particles are stored one box length outside the primary box: the per-cell
    "outside" flags (not part of to_host) switch the LJ traversal of those cells to the minimum-image arithmetic, so the forces on both
    lists, and against the same particles folded back into the box, show a flag that was lost.  A lost flag misplaces a neighbour by a
    box length, an error of the order of the force itself.  The coordinates are multiples of 2^-10 and L = 30.5, so moving a particle
    by a box length and folding it back are exact in float32 and the separations are the same numbers either way: 1e-5 of the largest
    force (some float32 roundings, the bound of smoke()) is left for the two forms of the traversal's arithmetic."""
    L, box, cd, ubox = _grid(hip, 12)
    assert L == 30.5
    n = 500
    pos = np.round(lattice_positions(n, L, seed=3, jitter=1.2) * 1024) / np.float32(1024)  # (no pair closer than 1.4: forces of order one)
    pos = np.clip(pos, -L / 2, L / 2 - 1 / 1024).astype(np.float32)
    folded = pos.copy()
    pos[:40, 0] += np.float32(L)
    pos[40:60, 1] -= np.float32(L)
    pos[60:70, 2] += np.float32(L)
    a, cl, ref, d_pos = _build_pair(hip, pos, ubox, cd)
    assert (canon_cell_tables(a)[0] < 0).sum() >= 12 ** 3 - n
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(RC, 1.0, 1.0, False))
    forces = []
    for lst in (cl, ref):
        f = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        lst.transverse_lj(pot.device_table(), 1, box, f)
        forces.append(f.cpu().numpy())
    assert np.array_equal(forces[0], forces[1])  # the same list, the same tables, the same kernel
    inbox = hip.CellList()
    inbox.update_grid(torch.from_numpy(folded).cuda(), ubox, cd)
    f = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    inbox.transverse_lj(pot.device_table(), 1, box, f)
    fin = f.cpu().numpy()
    scale = np.abs(fin[:, :3]).max()
    assert scale > 0
    assert np.abs(forces[0][:, :3] - fin[:, :3]).max() <= 1e-5 * scale


def test_one_handle_many_builds(hip):
    """Five builds on one handle, N = 5000, 1200, 5000, another grid, 5000 again, each against a fresh radix handle: the trailing blocks
    of the placement hand the key counters back zeroed for the next build."""
    cl = hip.CellList()
    grids = {k: _grid(hip, k) for k in (8, 5)}
    for it, (n, ncell) in enumerate([(5000, 8), (1200, 8), (5000, 8), (5000, 5), (5000, 8)]):
        L, _, cd, ubox = grids[ncell]
        d_pos = torch.from_numpy(_uniform(n, L, seed=100 + it)).cuda()
        cl.update_grid(d_pos, ubox, cd)
        ref = hip.CellList()
        ref.set_option("force_radix", 1)
        ref.update_grid(d_pos, ubox, cd)
        # (VALID_CELL counts the builds of a handle at one N, tests/test_gpu_celllist.py: the tables are compared relative to it)
        _same(cl.to_host(), ref.to_host(), tag=it, epoch=False)
