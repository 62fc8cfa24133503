"""float64 NumPy restatement of the DPD pair force (Interactor/Potential/DPD.cuh:121-152) and of the VerletNVE step
(Integrator/VerletNVE.cu:64-85,160-188), written from the formulas; a test helper like bonded_ref.py.

    rij = pbc(ri - rj), vij = vi - vj, r = |rij|; nothing if r == 0 or r >= rc
    wr = 1 - r/rc
    F_i += (A wr / r  -  g wr^2 (rij . vij) / r^2  +  xi sigma sqrt(g) wr / r) rij,   sigma = sqrt(2 kT) / sqrt(dt)
    xi = Saru(min(i,j) + N max(i,j), seed, step).gf(0, 1).x   (key in 32-bit unsigned arithmetic, seed and step truncated to 32 bits)

The Gaussian of a pair comes from the oracle's Saru (oracle.saru_gf, pinned on tests/golden/saru_u32.npz by the oracle's own tests), or
from any callable `xi(keys) -> array` (the thermostat reference uses NumPy's generator there: only the statistics matter).
"""
import numpy as np


def min_image(d, L, periodic=(True, True, True)):
    d = np.array(d, dtype=np.float64)
    L = np.broadcast_to(np.asarray(L, np.float64), (3,))
    for k in range(3):
        if periodic[k]:
            d[..., k] -= np.floor(d[..., k] / L[k] + 0.5) * L[k]
    return d


def pairs(pos, L, periodic, rc):
    """(i, j, rij) with i < j (positions in the arrays' order), 0 < |rij| < rc, rij = pbc(ri - rj)."""
    pos = np.asarray(pos, np.float64)[:, :3]
    n = len(pos)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    try:
        from scipy.spatial import cKDTree
    except ImportError:   # (the chunked all-pairs search below does for every size, slowly)
        cKDTree = None
    if cKDTree is not None and all(periodic) and n >= 1000:
        w = pos - np.floor(pos / L3) * L3
        w = np.where(w >= L3, 0.0, w)
        ij = cKDTree(w, boxsize=L3).query_pairs(rc, output_type="ndarray")
        I, J = ij[:, 0], ij[:, 1]
    else:
        Is, Js = [], []
        for a in range(0, n, 256):
            d = min_image(pos[a:a + 256, None, :] - pos[None, :, :], L3, periodic)
            r2 = (d * d).sum(-1)
            ii, jj = np.nonzero(r2 < rc * rc)
            ii += a
            keep = ii < jj
            Is.append(ii[keep])
            Js.append(jj[keep])
        I, J = np.concatenate(Is), np.concatenate(Js)
    rij = min_image(pos[I] - pos[J], L3, periodic)
    r = np.sqrt((rij * rij).sum(-1))
    keep = (r > 0) & (r < rc)
    return I[keep], J[keep], rij[keep]


def pair_keys(ki, kj, nkey):
    """min + N max in 32-bit unsigned arithmetic (what the compiled reference's overflowing int product gives)."""
    lo = np.minimum(ki, kj).astype(np.uint64)
    hi = np.maximum(ki, kj).astype(np.uint64)
    return ((lo + np.uint64(nkey) * hi) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def saru_xi(keys, seed, step):
    """Saru(key, seed, step).gf(0, 1).x for every key, from the oracle."""
    import oracle
    o = oracle.get("f32")
    s, t = int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF
    return np.array([o.saru_gf((int(k), s, t), 0.0, 1.0, 1)[0] for k in keys], np.float64)


def dpd_forces(pos, vel, L, periodic, rc, A, gamma, kT, dt, seed=0, step=0, keys=None, nkey=None, xi=None):
    """Forces on the particles of pos / vel (n x 3).  keys: the particles' indices in the ParticleData (default arange), nkey: its size."""
    pos = np.asarray(pos, np.float64)[:, :3]
    vel = np.asarray(vel, np.float64)[:, :3]
    n = len(pos)
    keys = np.arange(n) if keys is None else np.asarray(keys)
    nkey = n if nkey is None else nkey
    I, J, rij = pairs(pos, L, periodic, rc)
    r = np.sqrt((rij * rij).sum(-1))
    wr = 1.0 - r / rc
    vij = vel[I] - vel[J]
    Fc = A * wr / r
    Fd = -gamma * wr * wr * (rij * vij).sum(-1) / (r * r)
    Fr = 0.0
    if kT > 0 and gamma > 0:
        sigma = np.sqrt(2.0 * kT) / np.sqrt(dt)
        k = pair_keys(keys[I], keys[J], nkey)
        z = saru_xi(k, seed, step) if xi is None else xi(k)
        Fr = z * sigma * np.sqrt(gamma) * wr / r
    fij = (Fc + Fd + Fr)[:, None] * rij
    F = np.zeros((n, 3))
    np.add.at(F, I, fij)
    np.add.at(F, J, -fij)
    return F


def nve_half(pos, vel, force, mass, dt, step, is2D=False):
    """VerletNVE_ns::integrateGPU<step> (VerletNVE.cu:64-85) in float64; returns new (pos, vel)."""
    vel = np.asarray(vel, np.float64) + np.asarray(force, np.float64)[:, :3] / np.asarray(mass, np.float64).reshape(-1, 1) * dt * 0.5
    if is2D:
        vel[:, 2] = 0.0
    pos = np.array(pos, np.float64)
    if step == 1:
        pos[:, :3] += vel * dt
    return pos, vel


def lj_forces_energy(pos, L, rc, shift=True):
    """Truncated (and shifted) Lennard-Jones, sigma = epsilon = 1: forces and the total potential energy, all pairs, float64."""
    pos = np.asarray(pos, np.float64)[:, :3]
    d = min_image(pos[:, None, :] - pos[None, :, :], L)
    r2 = (d * d).sum(-1)
    np.fill_diagonal(r2, np.inf)
    inside = r2 < rc * rc
    ir2 = np.where(inside, 1.0 / r2, 0.0)
    ir6 = ir2 ** 3
    fmod = (48.0 * ir6 - 24.0) * ir6 * ir2          # |f| / r, f_i = fmod * (ri - rj)
    F = (fmod[:, :, None] * d).sum(1)
    eshift = 4.0 * (rc ** -12 - rc ** -6) if shift else 0.0
    U = 0.5 * np.where(inside, 4.0 * ir6 * (ir6 - 1.0) - eshift, 0.0).sum()
    return F, U


def nve_run_lj(pos, vel, L, rc, dt, steps, mass=1.0):
    """Velocity Verlet as VerletNVE::forwardTime sequences it; returns the total energy after every step (and before the first)."""
    pos = np.array(pos, np.float64)[:, :3]
    vel = np.array(vel, np.float64)
    m = np.full(len(pos), mass, np.float64)
    F, U = lj_forces_energy(pos, L, rc)
    E = [U + 0.5 * (m[:, None] * vel * vel).sum()]
    for _ in range(steps):
        pos, vel = nve_half(pos, vel, F, m, dt, 1)
        F, U = lj_forces_energy(pos, L, rc)
        _, vel = nve_half(pos, vel, F, m, dt, 2)
        E.append(U + 0.5 * (m[:, None] * vel * vel).sum())
    return np.array(E)


def dpd_run(n, steps, rho=3.0, rc=1.0, A=25.0, gamma=4.5, kT=1.0, dt=0.01, seed=1):
    """The DPD scheme (VerletNVE + the pair force above) from uniform random positions at rest; NumPy's Gaussian stream stands in for
    Saru.  Returns the kinetic temperature sum v^2 / (3 n) after every step."""
    rng = np.random.default_rng(seed)
    L = (n / rho) ** (1.0 / 3.0)
    pos = rng.uniform(-L / 2, L / 2, (n, 3))
    vel = np.zeros((n, 3))
    m = np.ones(n)
    xi = lambda k: rng.standard_normal(len(k))
    per = (True, True, True)
    F = dpd_forces(pos, vel, L, per, rc, A, gamma, kT, dt, xi=xi)
    T = []
    for _ in range(steps):
        pos, vel = nve_half(pos, vel, F, m, dt, 1)
        F = dpd_forces(pos, vel, L, per, rc, A, gamma, kT, dt, xi=xi)
        _, vel = nve_half(pos, vel, F, m, dt, 2)
        T.append((vel * vel).sum() / (3.0 * n))
    return np.array(T)


def block_average(x, blocks=20):
    """(mean, standard error of the block means)."""
    x = np.asarray(x, np.float64)
    per = len(x) // blocks
    b = x[len(x) - per * blocks:].reshape(blocks, per).mean(1)
    return float(b.mean()), float(b.std(ddof=1) / np.sqrt(blocks))
