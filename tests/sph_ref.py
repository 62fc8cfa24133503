"""NumPy restatement of the SPH interactor (Interactor/SPH.cuh), written from the formulas; a test helper like dpd_ref.py.  With h the
support, m the mass (1 without masses), rij = pbc(rj - ri), r = |rij|, vij = vj - vi and j over every particle (i itself included):

    W(rij, h): q = r / h;      0 if q >= 2;  ((2 - q)^3 - [q <= 1] 4 (1 - q)^3) / (4 pi h^3)
    G(rij, h): q = r (1 / h);  0 if q >= 2;  c (3 r - 4 h) rij if q <= 1, else c (2 h - r)^2 rij;  c = -3 / (4 pi h^6)
    rho_i = sum_j m_j W;  P_i = K (rho_i - rho0);  Pi_ij = -nu (vij . rij) / (r^2 + 0.001 h^2)
    F_i = sum_j m_i m_j (P_i / rho_i^2 + P_j / rho_j^2 + Pi_ij) G

G is the reference's formula as written, not the derivative of W.  Every operation runs in `dtype` (float64 or float32) and the sums of a
particle run in ascending-j order.  The two branches of G differ by a finite jump at q = 1, so that a float and a double evaluation may
legitimately choose differently there: sph_sums also returns the UNDECIDED particles, those in a pair with |r / h - 1| < window.
"""
import numpy as np

WINDOW = 4e-6   # the float rounding of r / h is about 2e-7: a factor 20


def min_image(d, L, periodic=(True, True, True)):
    """d - floor(d / L + 1/2) L in the periodic directions, in d's own dtype"""
    d = np.array(d)
    L = np.broadcast_to(np.asarray(L, d.dtype), (3,))
    for k in range(3):
        if periodic[k]:
            d[..., k] -= np.floor(d[..., k] / L[k] + d.dtype.type(0.5)) * L[k]
    return d


def W(rij, h, dtype=np.float64):
    T = np.dtype(dtype).type
    rij = np.asarray(rij, dtype).reshape(-1, 3)
    h = T(h)
    r = np.sqrt((rij * rij).sum(-1, dtype=dtype))
    q = r / h
    w = (T(2) - q) ** 3 - np.where(q <= T(1), T(4) * (T(1) - q) ** 3, T(0))
    return np.where(q >= T(2), T(0), w * (T(1) / (T(4) * T(np.pi) * h * h * h))).astype(dtype)


def G(rij, h, dtype=np.float64):
    T = np.dtype(dtype).type
    rij = np.asarray(rij, dtype).reshape(-1, 3)
    h = T(h)
    r = np.sqrt((rij * rij).sum(-1, dtype=dtype))
    q = r * (T(1) / h)
    c = T(-3) / (T(4) * T(np.pi) * h ** 6)
    g = np.where(q <= T(1), c * (T(3) * r - T(4) * h), c * (T(2) * h - r) ** 2)
    g = np.where(q >= T(2), T(0), g)
    return (g[:, None] * rij).astype(dtype)


def neighbours(pos, L, periodic, rc):
    """(I, J) of every ordered pair with |pbc(rj - ri)| < rc in float64, the self pairs included, sorted by (I, J)"""
    pos = np.asarray(pos, np.float64)[:, :3]
    n = len(pos)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    try:
        from scipy.spatial import cKDTree
    except ImportError:   # (the chunked all-pairs search below does for every size, slowly)
        cKDTree = None
    if cKDTree is not None and all(periodic) and n >= 1000 and rc < 0.5 * L3.min():
        w = pos - np.floor(pos / L3) * L3
        w = np.where(w >= L3, 0.0, w)
        ij = cKDTree(w, boxsize=L3).query_pairs(rc, output_type="ndarray")
        I = np.concatenate([ij[:, 0], ij[:, 1], np.arange(n)])
        J = np.concatenate([ij[:, 1], ij[:, 0], np.arange(n)])
    else:
        Is, Js = [], []
        for a in range(0, n, 256):
            d = min_image(pos[None, :, :] - pos[a:a + 256, None, :], L3, periodic)
            ii, jj = np.nonzero((d * d).sum(-1) < rc * rc)
            Is.append(ii + a)
            Js.append(jj)
        I, J = np.concatenate(Is), np.concatenate(Js)
    order = np.lexsort((J, I))
    return I[order], J[order]


def sph_sums(pos, vel, mass, L, periodic, h, K, rho0, nu, dtype=np.float64, window=WINDOW):
    """density, pressure, force (n x 3) in `dtype`, and the sorted indices of the undecided particles"""
    T = np.dtype(dtype).type
    n = len(pos)
    pos = np.asarray(np.asarray(pos)[:, :3], dtype)
    vel = np.asarray(vel, dtype)
    m = np.ones(n, dtype) if mass is None else np.asarray(mass, dtype).reshape(n)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    I, J = neighbours(pos, L3, periodic, 2.0 * float(h) * (1 + 1e-6))   # (a margin: the exact q >= 2 test is W's and G's own)
    rij = min_image(pos[J] - pos[I], L3.astype(dtype), periodic)
    r2 = (rij * rij).sum(-1, dtype=dtype)
    rho = np.zeros(n, dtype)
    np.add.at(rho, I, m[J] * W(rij, h, dtype))      # unbuffered and in the order of I: ascending j for every i
    P = T(K) * (rho - T(rho0))
    Pr = P / (rho * rho)
    vij = vel[J] - vel[I]
    vis = T(-nu) * ((vij * rij).sum(-1, dtype=dtype) / (r2 + T(0.001) * T(h) * T(h)))
    s = m[I] * m[J] * (Pr[I] + Pr[J] + vis)
    F = np.zeros((n, 3), dtype)
    np.add.at(F, I, s[:, None] * G(rij, h, dtype))
    r64 = np.sqrt((min_image(pos[J].astype(np.float64) - pos[I].astype(np.float64), L3, periodic) ** 2).sum(-1))
    near = np.abs(r64 / float(h) - 1.0) < window
    undecided = np.unique(np.concatenate([I[near], J[near]]))
    return rho, P.astype(dtype), F, undecided


def nve_step(pos, vel, mass, dt, forces):
    """One VerletNVE::forwardTime after its first (VerletNVE.cu:133-188) in float64: half kick and drift with the forces of the current
    state, new forces, half kick.  forces(pos, vel) -> (n x 3).  Returns the new (pos, vel)."""
    pos = np.array(pos, np.float64)
    vel = np.array(vel, np.float64)
    m = np.ones(len(pos)) if mass is None else np.asarray(mass, np.float64).reshape(-1)
    vel = vel + forces(pos, vel) / m[:, None] * dt * 0.5
    pos[:, :3] += vel * dt
    vel = vel + forces(pos, vel) / m[:, None] * dt * 0.5
    return pos, vel


def random_fluid(n, L, seed, vel_scale=1.0):
    """n uniform random positions in the box (float32, w = 0) and Gaussian velocities: the fixtures of the parity tests"""
    rng = np.random.default_rng(seed)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * L3 * 0.999
    vel = (vel_scale * rng.normal(0.0, 1.0, (n, 3))).astype(np.float32)
    return pos, vel


def random_masses(n, seed):
    return np.random.default_rng(seed + 1000).uniform(0.5, 1.5, n).astype(np.float32)


# The GPU parity fixtures (tests/test_gpu_sph.py): name -> (n, L, periodic, seed, masses, parameter overrides).  tests/test_sph_cpu.py
# asserts on the CPU that none of them has an undecided particle, so the GPU parity tests exclude nobody.
PARAMS = dict(h=1.0, K=100.0, rho0=0.4, nu=50.0)
FIXTURES = {
    "cubic": (3000, 10.0, (True, True, True), 21, False, {}),
    "cubic_masses": (3000, 10.0, (True, True, True), 32, True, {}),   # (seed 22 puts a pair within 4e-6 of r = h)
    "anisotropic_open_z": (3000, (12.5, 10.0, 8.0), (True, True, False), 23, False, {}),
    "anisotropic_open_z_masses": (3000, (12.5, 10.0, 8.0), (True, True, False), 24, True, {}),
    "K0": (3000, 10.0, (True, True, True), 25, False, dict(K=0.0)),
    "nu0": (3000, 10.0, (True, True, True), 26, False, dict(nu=0.0)),
    "at_rest": (3000, 10.0, (True, True, True), 27, False, dict(vel_scale=0.0)),
    "small_box": (450, 5.0, (True, True, True), 28, True, {}),    # L < 3 x 2h: the list's cell list has fewer than three cells a side
}


def fixture(name):
    """(pos, vel, mass or None, L, periodic, parameters) of a parity fixture"""
    n, L, per, seed, masses, over = FIXTURES[name]
    over = dict(over)
    pos, vel = random_fluid(n, L, seed, over.pop("vel_scale", 1.0))
    return pos, vel, (random_masses(n, seed) if masses else None), L, per, {**PARAMS, **over}
