"""Hydro::ICM_Compressible between two walls on the GPU (uammd_amd/csrc/icm_compressible.hip, the WALLS instantiations and
k_icmc_ghost_fill) through the Python layer on the C ABI, against the NumPy restatement tests/icm_compressible_walls_ref.py.

PARITY BOUND (the one of tests/test_gpu_icm_compressible.py).  For every compared field, the GPU's maximum error against the FLOAT64
restatement, relative to the field's maximum, may be at most 4 x the same error of the FLOAT32 restatement on the same inputs."""
import os
import subprocess

import numpy as np
import pytest
import torch

import icm_compressible_ref as ref
import icm_compressible_walls_ref as wref
from test_gpu_icm_compressible import PAR, Fixed, _bound, _compare_fluid, _hip, _set, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one layer touches both walls; two layers; rows longer than a wave with odd sizes; a cube.  (No constructor rule refuses any of them.)
GRIDS = [(5, 7, 1), (5, 7, 2), (70, 9, 5), (16, 16, 16)]


class Walls:
    """what the Python layer takes: velocities(t) -> ((bx, by), (tx, ty))"""

    def __init__(self, velocities):
        self.velocities = velocities


def _make(cells, velocities, h=1.0, N=0, par=PAR, rule=None):
    """the integrator and the two restatements (float64, float32) of one configuration between walls"""
    hip = _hip()
    L = [c * h for c in cells]
    pd = hip.ParticleData(N)
    p = hip.Hydro.ICM_Compressible.Parameters(shearViscosity=par["shear"], bulkViscosity=par["bulk"], speedOfSound=par["c"], dt=par["dt"],
                                              boxSize=L, cellDim=cells, seed=1234, walls=Walls(velocities))
    icm = hip.Hydro.ICM_Compressible(pd, p)
    refs = [wref.WallFluid(cells, L, par["shear"], par["bulk"], par["c"], par["dt"], rule or wref.MovingWalls(velocities, ty), 0.0, ty)
            for ty in (np.float64, np.float32)]
    return pd, icm, refs


def _smooth(f, drho=0.05, dv=0.05):
    """smooth, periodic in x and y, nothing special at the walls"""
    x, y, z = [2 * np.pi * c.astype(np.float64) / l for c, l in zip(f.centers(), f.L.astype(np.float64))]
    rho = 1 + drho * np.sin(x + 0.3) * np.cos(y - 0.2) * np.cos(0.5 * z + 0.1)
    v = [dv * np.sin(y + 0.5) * np.cos(0.5 * z + 0.2), dv * np.cos(x + 0.4) * np.sin(0.5 * z + 0.4), dv * np.sin(x - 0.1) * np.cos(y + 0.2) * np.cos(0.5 * z - 0.4)]
    assert np.abs(v[2][0]).max() > 0.3 * dv and np.abs(v[2][-1]).max() > 0.3 * dv      # v_z next to both walls: every ghost read carries weight
    return rho, v


def _run(icm, refs, steps):
    for _ in range(steps):
        icm.forwardTime()
        for f in refs:
            f.forward(np.zeros((0, 3)))


@pytest.mark.parametrize("cells", GRIDS, ids=lambda c: "x".join(map(str, c)))
def test_fluid_parity_between_moving_walls(cells):
    pd, icm, refs = _make(cells, lambda t: ((0.04, -0.03), (-0.02, 0.05)))
    _set(icm, refs, *_smooth(refs[0]))
    _run(icm, refs, 10)
    _compare_fluid(f"{cells} between walls after 10 steps", icm, refs)
    col = icm.getCurrentVelocity().cpu().numpy()                                # the collocated export: v_z of layer 0 averages with the ghost
    stag = icm.getCurrentVelocity(collocated=False).cpu().numpy()
    ghost = icm.getBottomGhostCells()[1].cpu().numpy()
    below = np.concatenate([ghost[2][None], stag[2][:-1]], 0)
    assert np.array_equal(col[2], np.float32(0.5) * (stag[2] + below))
    assert np.array_equal(col[0], np.float32(0.5) * (stag[0] + ref.shift(stag[0], 0, -1)))


def test_oscillating_bottom_wall():
    """omega dt = 0.1: a fill that used the time of another sub-stage would move the wall's velocity by 3 % of its amplitude"""
    omega = 0.1 / PAR["dt"]
    pd, icm, refs = _make((8, 8, 12), lambda t: ((0.05 * np.cos(omega * t), 0.05 * np.sin(omega * t)), (0.0, 0.0)))
    _set(icm, refs, *_smooth(refs[0], dv=0.01))
    _run(icm, refs, 20)
    _compare_fluid("oscillating bottom wall, 20 steps on (8, 8, 12)", icm, refs)


def test_a_sine_on_the_couette_profile_decays():
    from test_icm_compressible_walls_cpu import COUETTE as C, couette, couette_growth
    f32, profile, mode = couette(np.float32, C["amplitude"])
    hip = _hip()
    pd = hip.ParticleData(0)
    p = hip.Hydro.ICM_Compressible.Parameters(shearViscosity=C["shear"], bulkViscosity=C["bulk"], speedOfSound=C["c"], dt=C["dt"],
                                              boxSize=list(C["L"]), cellDim=list(C["cells"]), seed=1,
                                              walls=Walls(lambda t: ((C["U"], 0.0), (0.0, 0.0))))
    icm = hip.Hydro.ICM_Compressible(pd, p)
    icm.setFluid(*[torch.from_numpy(np.ascontiguousarray(a)) for a in (f32.rho, *f32.v)])
    steps = 200
    for _ in range(steps):
        icm.forwardTime()
        f32.step_fluid()
    rho, g, v = _state(icm)
    assert not v[1].any() and not v[2].any() and (rho == np.float32(C["rho0"])).all()          # nothing but v_x moves
    analytic = profile + C["amplitude"] * couette_growth() ** steps * mode
    _bound(f"sine between the walls after {steps} steps, v_x against profile + A G^n mode", v[0], analytic, f32.v[0])


def test_the_periodic_path_is_unchanged_by_the_mode_field():
    """20 steps at T > 0 with 64 particles under forces, on the C ABI: a handle made from a struct that says nothing about walls (zero),
    driven by uammd_icmc_fluid_and_corrector, and one with the mode written as "none", driven through the pieces of the step, give the same
    bits.  (tests/test_gpu_icm_compressible.py holds the link to what the periodic solver computed before.)  The particles sit 4 cells
    apart, so no two windows share a cell and the order of the spreading's atomic adds cannot show."""
    import ctypes as C
    from uammd_amd import _lib
    from uammd_amd.md import _ptr
    lib = _lib.load()
    cells, N, steps = (16, 16, 16), 64, 20
    rng = np.random.default_rng(12)
    i = np.arange(N)
    p4 = np.zeros((N, 4), np.float32)
    p4[:, :3] = np.stack([i % 4, (i // 4) % 4, i // 16], 1) * 4.0 - 6.0 + rng.uniform(-0.3, 0.3, (N, 3))
    F4 = np.zeros((N, 4), np.float32)
    F4[:, :3] = rng.normal(0, 1, (N, 3))
    f64 = ref.Fluid(cells, [16.0] * 3, PAR["shear"], PAR["bulk"], PAR["c"], PAR["dt"])
    fields = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (lambda r, v: (r, *v))(*_smooth(f64))]
    out = []
    for pieces in (False, True):
        p = _lib.ICMCompressibleParameters()
        p.boxSize[:] = [16.0] * 3
        p.cells[:] = cells
        p.shearViscosity, p.bulkViscosity, p.speedOfSound, p.dt = PAR["shear"], PAR["bulk"], PAR["c"], PAR["dt"]
        p.temperature, p.hydrodynamicRadius, p.seed = 0.01, -1.0, 4711
        if pieces:
            p.walls = p.WALLS_NONE
        h, cd = C.c_void_p(), (C.c_int * 3)()
        _lib.check(lib.uammd_icmc_create(C.byref(p), C.byref(h), C.byref(cd)))
        try:
            _lib.check(lib.uammd_icmc_set_fluid(h, *[_ptr(a) for a in fields], None))
            pos, force = torch.from_numpy(p4).cuda(), torch.from_numpy(F4).cuda()
            for _ in range(steps):
                _lib.check(lib.uammd_icmc_predictor(h, _ptr(pos), N, None))
                if not pieces:
                    _lib.check(lib.uammd_icmc_fluid_and_corrector(h, _ptr(pos), _ptr(force), N, None))
                    continue
                _lib.check(lib.uammd_icmc_fluid_begin(h, _ptr(pos), _ptr(force), N, None))
                for s in range(3):
                    _lib.check(lib.uammd_icmc_substage(h, s, None))
                    _lib.check(lib.uammd_icmc_ghost_fill(h, None))
                    _lib.check(lib.uammd_icmc_substage_velocity(h, None))
                    _lib.check(lib.uammd_icmc_ghost_fill(h, None))
                _lib.check(lib.uammd_icmc_fluid_end(h, _ptr(pos), N, None))
            rho = torch.empty(cells[::-1], dtype=torch.float32, device="cuda")
            v, g = torch.empty((3,) + cells[::-1], dtype=torch.float32, device="cuda"), torch.empty((3,) + cells[::-1], dtype=torch.float32, device="cuda")
            pv, pg = (C.c_void_p * 3)(*[v[c].data_ptr() for c in range(3)]), (C.c_void_p * 3)(*[g[c].data_ptr() for c in range(3)])
            _lib.check(lib.uammd_icmc_get_fluid(h, _ptr(rho), C.byref(pv), C.byref(pg), None))
            torch.cuda.synchronize()
            out.append([a.cpu().numpy() for a in (rho, v, g, pos)])
        finally:
            lib.uammd_icmc_destroy(h)
    for a, b in zip(*out):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(out[0][3] - p4).max() > 1e-4 and np.abs(out[0][3][:, :3] - p4[:, :3]).max() < 0.5      # they moved, and stayed apart


def _wall_particles(cells, n=64, seed=6):
    """n positions in a box of unit cells: a quarter within 1e-3 h of a wall plane (z = -+ L_z / 2), a quarter within 1.5 h of one, so that
    their windows cross it, the rest anywhere, some outside the primary box"""
    rng = np.random.default_rng(seed)
    L = np.array(cells, np.float64)
    pos = rng.uniform(-0.6, 0.6, (n, 3)) * L
    k = n // 4
    side = np.where(np.arange(k) % 2 == 0, -0.5, 0.5) * L[2]
    pos[:k, 2] = side + rng.uniform(-1e-3, 1e-3, k)
    pos[k:2 * k, 2] = side + rng.uniform(-1.5, 1.5, k)
    p4 = np.zeros((n, 4), np.float32)
    p4[:, :3] = pos
    p4[:, 3] = np.arange(n) % 3
    return p4


def test_full_steps_with_particles_between_walls():
    """the windows wrap periodically through the walls, as the reference's do"""
    cells, steps = (12, 10, 8), 10
    p4 = _wall_particles(cells)
    pd, icm, refs = _make(cells, lambda t: ((0.04, -0.03), (-0.02, 0.05)), N=len(p4))
    pd.setPos(p4)
    _set(icm, refs, *_smooth(refs[0]))
    F = np.random.default_rng(9).normal(0, 1, (len(p4), 3)).astype(np.float32)
    fixed = Fixed(pd, F)
    icm.addInteractor(fixed)
    q = [p4[:, :3].astype(np.float64), p4[:, :3].copy()]
    for _ in range(steps):
        icm.forwardTime()
        q = [f.forward(p, lambda qh: F.astype(f.dtype)) for f, p in zip(refs, q)]
    _compare_fluid(f"{len(p4)} particles between walls, {steps} steps", icm, refs)
    got = pd.getPos("read").cpu().numpy()
    _bound("positions", got[:, :3], q[0], q[1])
    dt = PAR["dt"]
    assert np.allclose(fixed.times[:4], [0.5 * dt, dt / 3, 2 * dt / 3, dt], rtol=1e-6) and len(fixed.times) == 4 * steps


def test_the_bottom_ghost_plane_is_the_rule_applied_to_layer_zero():
    ub, ut = (0.04, -0.03), (-0.02, 0.05)
    pd, icm, refs = _make((5, 7, 3), lambda t: (ub, ut))
    _set(icm, refs, *_smooth(refs[0]))
    for when in ("after setFluid", "after 3 steps"):
        torch.cuda.synchronize()
        rho, v, g = [a.cpu().numpy() for a in icm.getBottomGhostCells()]
        r0 = icm.getCurrentDensity().cpu().numpy()[0]
        v0 = icm.getCurrentVelocity(collocated=False).cpu().numpy()[:, 0]
        g0 = icm.getMomentum().cpu().numpy()[:, 0]
        u = np.array([ub[0], ub[1], 0.0], np.float32)
        two = np.float32(2)
        assert np.array_equal(rho, r0), when
        for c in range(3):
            assert np.array_equal(v[c], two * u[c] - v0[c]), (when, c)
            assert np.array_equal(g[c], two * u[c] * r0 - g0[c]), (when, c)
        assert np.abs(v[2]).max() > 0
        for _ in range(3):
            icm.forwardTime()


def test_validation_through_the_python_layer():
    hip = _hip()
    pd = hip.ParticleData(0)
    good = dict(shearViscosity=1.0, bulkViscosity=1.0, speedOfSound=4.0, dt=0.05, boxSize=[8.0, 8.0, 8.0], cellDim=[8, 8, 8])
    with pytest.raises(ValueError, match="never draws"):
        hip.Hydro.ICM_Compressible(pd, hip.Hydro.ICM_Compressible.Parameters(temperature=0.1, walls=Walls(lambda t: ((0, 0), (0, 0))), **good))
    with pytest.raises(ValueError, match="velocities"):
        hip.Hydro.ICM_Compressible(pd, hip.Hydro.ICM_Compressible.Parameters(walls=object(), **good))
    periodic = hip.Hydro.ICM_Compressible(pd, hip.Hydro.ICM_Compressible.Parameters(**good))
    with pytest.raises(Exception, match="no walls"):
        periodic.getBottomGhostCells()


def test_icmc_walls_program_matches_the_python_layer():
    """tests/cxx/icmc_walls.cpp (built by examples/Makefile): a class derived from MovingWalls in plain C++ against the Python layer on the
    same input — the same library calls on the same numbers."""
    import math
    hip = _hip()
    exe = os.path.join(ROOT, "examples", "_build", "icmc_walls")
    assert os.path.exists(exe), f"{exe} is not built (examples/Makefile)"
    steps, dt = 20, 0.05
    r = subprocess.run([exe, str(steps)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    print(r.stdout.strip())
    lines = {l.split()[1]: l.split() for l in r.stdout.splitlines() if l.startswith("icmcw ")}
    assert np.allclose([float(x) for x in lines["times"][2:6]], [0.5 * dt, dt / 3, 2 * dt / 3, dt], rtol=1e-6, atol=0)
    assert int(lines["ghost"][2]) == 11 * 8 and int(lines["ghost"][4]) == 1

    def velocities(t):                                         # the program's walls hear the time as a float
        t = float(np.float32(t))
        return (np.float32(0.04 * math.cos(2.0 * t)), 0.0), (-0.01, 0.02)
    N = 64
    i = np.arange(N)
    pos = np.stack([(i % 4) * 1.1 - 1.9, ((i // 4) % 4) * 1.7 - 2.3, (i // 16) * 1.3 - 2.1, i % 3], 1).astype(np.float32)
    F = np.stack([(i % 7 - 3) / 4.0, (i % 5 - 2) / 3.0, (i % 3 - 1) / 2.0], 1).astype(np.float32)
    pd = hip.ParticleData(N)
    pd.setPos(pos)
    par = hip.Hydro.ICM_Compressible.Parameters(
        shearViscosity=1.3, bulkViscosity=0.7, speedOfSound=4.0, dt=dt, boxSize=[9.0, 6.0, 5.0], cellDim=[9, 6, 5], seed=77,
        initialDensity=lambda r: 1 + 0.05 * math.sin(2 * math.pi * r[0] / 9), initialVelocityX=lambda r: 0.05 * math.sin(2 * math.pi * r[1] / 6),
        initialVelocityZ=lambda r: 0.02 * math.cos(2 * math.pi * r[0] / 9), walls=Walls(velocities))
    icm = hip.Hydro.ICM_Compressible(pd, par)
    icm.addInteractor(Fixed(pd, F))
    for _ in range(steps):
        icm.forwardTime()
    rho, g, v = _state(icm)
    q = pd.getPos("read").cpu().numpy().astype(np.float64)
    w = (np.arange(rho.size) % 17 + 1).astype(np.float64)
    wq = (i % 17 + 1).astype(np.float64)
    d = lines["density"]
    got = [float(d[2])] + [float(x) for x in d[4:7]] + [float(x) for x in d[8:11]] + [float(x) for x in d[12:15]]
    mine = [(w * rho.ravel()).sum()] + [(w * c.ravel()).sum() for c in v] + [(w * c.ravel()).sum() for c in g] + [(wq * q[:, c]).sum() for c in range(3)]
    scale = ([np.abs(w * rho.ravel()).sum()] + [np.abs(w * c.ravel()).sum() for c in v] + [np.abs(w * c.ravel()).sum() for c in g]
             + [np.abs(wq[:, None] * q[:, :3]).sum()] * 3)
    for name, a, b, s in zip("rho vx vy vz gx gy gz qx qy qz".split(), got, mine, scale):
        print(f"{name}: program {a:.9g}, python layer {b:.9g}")
        assert abs(a - b) <= 2e-6 * s, name


def test_user_written_walls():
    """tests/cxx/icmc_walls_user.hip (built by examples/Makefile), 20 steps on (9, 6, 5): (a) the walltest rule as a user class gives
    the bits of MovingWalls — the program's exit status; (b) a free-slip rule against the restatement with the same callable."""
    import tempfile
    exe = os.path.join(ROOT, "examples", "_build", "icmc_walls_user")
    assert os.path.exists(exe), f"{exe} is not built (examples/Makefile)"
    cells, steps, nc = (9, 6, 5), 20, 270
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fields.bin")
        r = subprocess.run([exe, str(steps), out], capture_output=True, text=True, timeout=120)
        print(r.stdout.strip())
        assert r.returncode == 0 and "icmcu same 1 values 1890" in r.stdout, (r.stdout + r.stderr)[-2000:]
        assert float(r.stdout.split("max|v_x|")[1].split()[0]) > 1e-3
        a = np.fromfile(out, np.float32).reshape(11, cells[2], cells[1], cells[0])
    par = dict(shear=1.3, bulk=0.7, c=4.0, dt=0.05)
    refs = [wref.WallFluid(cells, [9.0, 6.0, 5.0], par["shear"], par["bulk"], par["c"], par["dt"], wref.FreeSlipWalls(), 0.0, ty)
            for ty in (np.float64, np.float32)]
    for f in refs:
        f.set(rho=a[0], v=list(a[1:4]))
        for _ in range(steps):
            f.step_fluid()
    assert np.abs(a[3][0]).max() > 1e-3 and np.abs(a[3][-1]).max() > 1e-3                 # v_z next to both walls
    _bound("free slip rho", a[4], refs[0].rho, refs[1].rho)
    _bound("free slip v", a[5:8], np.array(refs[0].v), np.array(refs[1].v))
    _bound("free slip g", a[8:11], np.array(refs[0].g), np.array(refs[1].g))


def test_reference_walltest_against_the_python_layer(tmp_path):
    """The reference's test/Hydro/ICM_Compressible/walltest.cu, built from where it lies (examples/Makefile), on its data.main.wall with
    16^3 cells in a box of 16^3, no relaxation, 50 steps, and the wallAmplitude line the program requires but the reference's file omits.
    The last block of vel.dat — the collocated v_x against z at (n.x / 2, n.y / 2) after 50 steps — and the Python layer on the same
    parameters, each against the float64 restatement under the bound."""
    exe = os.path.join(ROOT, "examples", "_build", "ref_test_walltest")
    if not os.path.exists(exe):
        pytest.skip("ref_test_walltest was not built (no reference tree where `make -C examples` ran)")
    dt, n, steps, freq, amp = 0.005, 16, 50, 1e-3, 1.0
    par = dict(shear=12.868, bulk=10.0, c=0.015625, dt=dt)
    (tmp_path / "data.main.wall").write_text(
        f"dt  {dt}\nboxSize  {n} {n} {n}\ncellDim  {n} {n} {n}\nbulkViscosity 10\nspeedOfSound  0.015625\nshearViscosity 12.868\n"
        f"temperature 0\ninitialDensity 1.0\n\nwallFreq {freq}\nwallAmplitude {amp}\n\nrelaxTime 0\nsimulationTime {steps * dt}\nprintTime      {10 * dt}\n")
    r = subprocess.run([exe, "data.main.wall"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    blocks = (tmp_path / "vel.dat").read_text().split("#")[1:]
    assert len(blocks) == 6
    last = np.array([[float(x) for x in l.split()] for l in blocks[-1].strip().splitlines()])
    assert last.shape == (n, 2) and np.allclose(last[:, 0], np.arange(n) + 0.5)

    def velocities(t):                                        # ICMWalls holds bottomWallvx = 0 until it hears its first time: the ghosts of
        if t == 0:                                            # the initial fluid are filled with the wall at rest (walltest.cu:24, :73-76)
            return (0.0, 0.0), (0.0, 0.0)
        return (amp * np.cos(2 * np.pi * freq * t), 0.0), (0.0, 0.0)
    pd, icm, refs = _make((n, n, n), velocities, par=par)
    _run(icm, refs, steps)
    col = [0.5 * (f.v[0] + ref.shift(f.v[0], 0, -1))[:, n // 2, n // 2] for f in refs]
    mine = icm.getCurrentVelocity().cpu().numpy()[0][:, n // 2, n // 2]
    assert np.abs(col[0]).max() > 0.1 * amp and np.abs(col[0][n // 2]) > 1e-6 * amp       # the wall's motion has reached the middle
    _bound("walltest.cu, v_x(z) after 50 steps", last[:, 1], col[0], col[1])
    _bound("the Python layer, v_x(z) after 50 steps", mine, col[0], col[1])
