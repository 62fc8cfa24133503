"""float64 NumPy restatement of the bonded kinds (reference: src/Interactor/BondedForces.cuh, AngularBondedForces.cuh,
TorsionalBondedForces.cuh) and of BondProcessor / buildBondList (BondedForces.cu:35-137).  Torsional uses the intended member mapping
(-fj, fm+fj-fk, fn+fk-fm, -fn).  Used by tests/test_bonded_cpu.py and tests/test_gpu_bonded.py."""
import numpy as np

KIND_MEMBERS = {"harmonic": 2, "fene": 2, "angular": 3, "torsional": 4, "fourier": 4}


def rows_restated(ids, members):
    """BondProcessor::registerBond + buildBondList: rows in ascending particle id (std::set), entries the bonds of the row in
    registration order; negative ids register nothing."""
    ids = np.asarray(ids).reshape(-1, members)
    isIn = {}
    for b, bond in enumerate(ids):
        for i in bond:
            if i >= 0:
                isIn.setdefault(int(i), []).append(b)
    rowId = sorted(isIn)
    rowStart = [0]
    entry = []
    for p in rowId:
        entry += isIn[p]
        rowStart.append(len(entry))
    return np.asarray(rowId, np.int64), np.asarray(rowStart, np.int64), np.asarray(entry, np.int64)


def _pbc(r, L, periodic):
    r = np.array(r, np.float64)
    for d in range(3):
        if periodic[d] and L[d] != 0 and np.isfinite(L[d]):
            r[..., d] -= np.floor(r[..., d] / L[d] + 0.5) * L[d]
    return r


def bond_terms(kind, P, info, L, periodic=(True, True, True)):
    """P[nb, m, 3] member positions, info[nb, 2] in the FILE order ("k p0").  Returns F[nb, m, 3], E[nb, m], V[nb, m]: what member m of
    each bond adds to itself."""
    P = np.asarray(P, np.float64)
    nb = P.shape[0]
    k, p0 = np.asarray(info, np.float64)[:, 0], np.asarray(info, np.float64)[:, 1]
    m = KIND_MEMBERS[kind]
    F = np.zeros((nb, m, 3))
    E = np.zeros((nb, m))
    V = np.zeros((nb, m))
    pb = lambda r: _pbc(r, L, periodic)  # noqa: E731
    if kind in ("harmonic", "fene"):
        r01 = pb(P[:, 1] - P[:, 0])           # from member 0 to member 1
        r2 = np.einsum("ij,ij->i", r01, r01)
        with np.errstate(all="ignore"):
            if kind == "harmonic":
                r = np.sqrt(r2)
                f = -k * (1 - p0 / r)
                e = 0.25 * k * (r - p0) ** 2
            else:
                r02 = p0 * p0
                f = -r02 * k / (r02 - r2)
                e = -0.25 * k * r02 * np.log(1 - r2 / r02)
        ok = r2 != 0
        # member 0: rij = r0 - r1 (the swap in Harmonic::compute), member 1: rij = r1 - r0
        F[:, 1] = np.where(ok[:, None], f[:, None] * r01, 0)
        F[:, 0] = -F[:, 1]
        E[:, 0] = E[:, 1] = np.where(ok, e, 0)
        v = np.where(ok, f * r2, 0)
        V[:, 0] = V[:, 1] = v
        return F, E, V
    if kind == "angular":
        ang0, ks = p0, k
        rij = pb(P[:, 1] - P[:, 0])
        rjk = pb(P[:, 2] - P[:, 1])
        rij2 = np.einsum("ij,ij->i", rij, rij)
        rjk2 = np.einsum("ij,ij->i", rjk, rjk)
        a2 = 1 / np.sqrt(rij2 * rjk2)
        c = np.clip(np.einsum("ij,ij->i", rij, rjk) * a2, -1, 1)
        theta = np.arccos(c)
        with np.errstate(all="ignore"):
            s = np.sin(0.5 * theta)
            ampli = np.where(ang0 == 0, -2 * ks, -2 * ks * (s - np.sin(ang0 * 0.5)) / s)
        zero = (ang0 != 0) & (theta == 0)
        ampli = np.where(zero, 0, ampli)
        a11 = (ampli * c / rij2)[:, None]
        a12 = (ampli * a2)[:, None]
        a22 = (ampli * c / rjk2)[:, None]
        F[:, 0] = a12 * rjk - a11 * rij
        F[:, 1] = -((-a11 - a12) * rij + (a12 + a22) * rjk)
        F[:, 2] = -(a12 * rij - a22 * rjk)
        return F, E, V
    r12 = pb(P[:, 1] - P[:, 0])
    r23 = pb(P[:, 2] - P[:, 1])
    r34 = pb(P[:, 3] - P[:, 2])
    if kind == "torsional":
        phi0, kk = p0, k
        n1 = np.cross(r12, r23)
        n2 = np.cross(r23, r34)
        q1 = np.einsum("ij,ij->i", n1, n1)
        q2 = np.einsum("ij,ij->i", n2, n2)
        inv1, inv2 = 1 / np.sqrt(q1), 1 / np.sqrt(q2)
        c = np.einsum("ij,ij->i", n1, n2) * inv1 * inv2
        with np.errstate(all="ignore"):
            phi = np.arccos(c)
            Fmod = np.where((c * c <= 1) & (phi * phi > 0), -kk * (phi - phi0) / np.sin(phi), 0.0)
        u1, u2 = n1 * inv1[:, None], n2 * inv2[:, None]
        v1 = (u2 - c[:, None] * u1) * inv1[:, None]
        v2 = (u1 - c[:, None] * u2) * inv2[:, None]
        fj = Fmod[:, None] * np.cross(v1, r23)
        fk = Fmod[:, None] * np.cross(v2, r34)
        fm = Fmod[:, None] * np.cross(v1, r12)
        fn = Fmod[:, None] * np.cross(v2, r23)
        F[:, 0], F[:, 1], F[:, 2], F[:, 3] = -fj, fm + fj - fk, fn + fk - fm, -fn
        return F, E, V
    # FourierLAMMPS
    phi0, kdih = p0, k
    v123 = np.cross(r12, r23)
    v234 = np.cross(r23, r34)
    q1 = np.einsum("ij,ij->i", v123, v123)
    q2 = np.einsum("ij,ij->i", v234, v234)
    inv1, inv2 = 1 / np.sqrt(q1), 1 / np.sqrt(q2)
    c = np.clip(np.einsum("ij,ij->i", v123, v234) * inv1 * inv2, -1, 1)
    ru23 = r23 / np.linalg.norm(r23, axis=1)[:, None]
    u1 = r12 / np.linalg.norm(r12, axis=1)[:, None]
    u2 = ru23 - np.einsum("ij,ij->i", u1, ru23)[:, None] * u1
    sgn = np.where(np.einsum("ij,ij->i", r34, np.cross(u1, u2)) < 0, -1.0, 1.0)
    phi = sgn * np.arccos(c)
    e = 0.25 * kdih * (1 + np.cos(phi - phi0))
    pref = -kdih * np.sin(phi - phi0) / np.sin(phi)
    w1 = (v234 * inv2[:, None] - c[:, None] * v123 * inv1[:, None]) * inv1[:, None]
    w2 = (v123 * inv1[:, None] - c[:, None] * v234 * inv2[:, None]) * inv2[:, None]
    r13 = pb(P[:, 2] - P[:, 0])
    r24 = pb(P[:, 3] - P[:, 1])
    pr = pref[:, None]
    F[:, 0] = pr * np.cross(w1, r23)
    c34, c13 = np.cross(w2, r34), np.cross(w1, r13)
    F[:, 1] = pr * (c34 - c13)
    c12, c24 = np.cross(w1, r12), np.cross(w2, r24)
    F[:, 2] = pr * (c12 - c24)
    F[:, 3] = pr * np.cross(w2, r23)
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)  # noqa: E731
    V[:, 0] = dot(F[:, 0], r23)
    V[:, 1] = dot(pr * c34, r34) - dot(pr * c13, r13)
    V[:, 2] = dot(pr * c12, r12) - dot(pr * c24, r24)
    V[:, 3] = dot(F[:, 3], r23)
    for j in range(4):
        E[:, j] = e
    degenerate = (q1 < 1e-15) | (q2 < 1e-15) | (np.abs(phi) < 1e-10) | (np.pi - np.abs(phi) < 1e-10)
    F[degenerate] = 0
    V[degenerate] = 0
    E[(q1 < 1e-15) | (q2 < 1e-15)] = 0
    return F, E, V


def per_particle(kind, pos, ids, info, L, periodic=(True, True, True), fixedPoints=None):
    """Sum of bond_terms onto the particles (by index in pos): force[N, 3], energy[N], virial[N]."""
    pos = np.asarray(pos, np.float64)[:, :3]
    ids = np.asarray(ids).reshape(len(info), -1)
    m = ids.shape[1]
    P = np.zeros(ids.shape + (3,))
    for j in range(m):
        neg = ids[:, j] < 0
        P[~neg, j] = pos[ids[~neg, j]]
        if neg.any():
            P[neg, j] = np.asarray(fixedPoints, np.float64)[-ids[neg, j] - 1, :3]
    F, E, V = bond_terms(kind, P, info, L, periodic)
    N = pos.shape[0]
    f, e, v = np.zeros((N, 3)), np.zeros(N), np.zeros(N)
    for j in range(m):
        ok = ids[:, j] >= 0
        np.add.at(f, ids[ok, j], F[ok, j])
        np.add.at(e, ids[ok, j], E[ok, j])
        np.add.at(v, ids[ok, j], V[ok, j])
    return f, e, v
