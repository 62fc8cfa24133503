"""NumPy restatement of the Chebyshev transforms and of the batched boundary value problem solver, for the tests.

Everything takes a `real` dtype: np.float64 is the reference the tests compare against; np.float32 runs the same sums in single
precision (direct sums, left to right), which is how the bars of the single-precision GPU tests are measured.

Layout of a field: array of shape (nz, ny, nx), element (i, j, k) at [k, j, i]; plane k lies at cos(pi k / (nz - 1)).
"""
import numpy as np


def _cplx(real):
    return np.complex128 if real == np.float64 else np.complex64


# ---------------------------------------------------------------------------------------------------------------- transforms
def cos_table(nz, real=np.float64):
    n = nz - 1
    return np.cos(np.pi * np.arange(2 * n) / n).astype(real)


def _cos_sum(x, nz, weights, scale, real):
    """out[k] = scale[k] * sum_j weights[j] x[j] cos(pi j k / n), summed over j left to right in `real` precision."""
    n = nz - 1
    tab = cos_table(nz, real)
    x = x.astype(_cplx(real)).reshape(nz, -1)
    k = np.arange(nz)
    acc = np.zeros_like(x)
    for j in range(nz):
        acc = acc + (real(weights[j]) * x[j])[None, :] * tab[(j * k) % (2 * n)][:, None]
    return (acc * scale.astype(real)[:, None]).astype(_cplx(real))


def chebyshev_forward(f, real=np.float64):
    """c_k = pm_k / (2 n) [f_0 + (-1)^k f_n + 2 sum_{0 < j < n} f_j cos(pi j k / n)] along axis 0."""
    nz, n = f.shape[0], f.shape[0] - 1
    w = np.full(nz, 2.0)
    w[[0, n]] = 1.0
    pm = np.full(nz, 2.0)
    pm[[0, n]] = 1.0
    return _cos_sum(f, nz, w, pm / (2 * n), real).reshape(f.shape)


def chebyshev_inverse(c, real=np.float64):
    """f_j = sum_k c_k cos(pi j k / n) along axis 0."""
    nz = c.shape[0]
    return _cos_sum(c, nz, np.ones(nz), np.ones(nz), real).reshape(c.shape)


def _plane_dft(x, sign, real):
    """Unnormalised 2-D DFT over the last two axes with e^{sign i ...}; np.fft in double, direct sums in single precision."""
    if real == np.float64:
        return np.fft.fft2(x) if sign < 0 else np.fft.ifft2(x) * (x.shape[-1] * x.shape[-2])
    out = x.astype(np.complex64)
    for axis in (-1, -2):
        m = out.shape[axis]
        idx = np.arange(m)
        w = np.exp(sign * 2j * np.pi * ((idx[:, None] * idx[None, :]) % m) / m).astype(np.complex64)
        moved = np.moveaxis(out, axis, -1)
        acc = np.zeros_like(moved)
        for q in range(m):
            acc = acc + moved[..., q:q + 1] * w[q][None, :]
        out = np.moveaxis(acc, -1, axis)
    return out


def fourier_chebyshev_forward(f, real=np.float64):
    nz, ny, nx = f.shape
    planes = _plane_dft(f.astype(_cplx(real)), -1, real) * real(1.0 / (nx * ny))
    return chebyshev_forward(planes.astype(_cplx(real)), real)


def fourier_chebyshev_inverse(c, real=np.float64):
    return _plane_dft(chebyshev_inverse(c, real), +1, real).astype(_cplx(real))


# ---------------------------------------------------------------------------------------------------------------- BVP
def first_integral_matrix(nz):
    """d = J a: the Chebyshev coefficients d_1 ... d_{nz - 1} of the integral of sum a_i T_i (row 0, the constant, stays empty)."""
    J = np.zeros((nz, nz))
    J[1, 0] = 1.0
    if nz > 2:
        J[1, 2] = -0.5
    for j in range(2, nz):
        J[j, j - 1] = 1.0 / (2 * j)
        if j + 1 < nz:
            J[j, j + 1] = -1.0 / (2 * j)
    return J


def tables(k, H, nz, tfi, tsi, bfi, bsi):
    """The per-system tables in float64, each of shape (rows, nsys): dense linear algebra, one system at a time."""
    k, tfi, tsi, bfi, bsi = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (k, tfi, tsi, bfi, bsi)]
    nsys = k.shape[0]
    J = first_integral_matrix(nz)
    T = J @ J
    ones, alt = np.ones(nz), (-1.0) ** np.arange(nz)
    out = {name: np.zeros((rows, nsys)) for name, rows in (("beta", nz), ("diagonal_p2", nz), ("diagonal_m2", nz), ("cinvA", 2 * nz), ("m22", 4),
                                                            ("kH2", 1))}
    cache = {}
    for s in range(nsys):
        key = (k[s], tfi[s], tsi[s], bfi[s], bsi[s])
        if key not in cache:
            kH2 = k[s] ** 2 * H ** 2
            A = np.eye(nz) - kH2 * T
            Cm = np.vstack([tfi[s] * (J.T @ ones) + tsi[s] * (T.T @ ones), bfi[s] * (J.T @ alt) + bsi[s] * (T.T @ alt)])
            D = np.array([[tsi[s], tfi[s] + tsi[s]], [bsi[s], bfi[s] - bsi[s]]])
            CinvA = np.linalg.solve(A.T, Cm.T).T
            M = -kH2 * CinvA[:, :2] - D
            beta = np.zeros(nz)
            for i in range(nz):
                beta[i] = A[i, i] if i < 2 else A[i, i] - A[i, i - 2] * A[i - 2, i] / beta[i - 2]
            p2 = np.array([A[i, i + 2] if i + 2 < nz else 0.0 for i in range(nz)])
            m2 = np.array([A[i, i - 2] if i >= 2 else 0.0 for i in range(nz)])
            cache[key] = (beta, p2, m2, CinvA.reshape(-1), M.reshape(-1), np.array([kH2]))
        for name, v in zip(("beta", "diagonal_p2", "diagonal_m2", "cinvA", "m22", "kH2"), cache[key]):
            out[name][:, s] = v
    return out


def solve(tab, H, fn, alpha, beta, real=np.float64):
    """fn: (nrhs, nz, nsys) complex, alpha / beta: (nrhs, nsys).  The tables are cast to `real`, then every step runs in it.
    Returns (cn, an)."""
    cplx = _cplx(real)
    t = {name: v.astype(real) for name, v in tab.items()}
    nz = t["beta"].shape[0]
    fn, alpha, beta = fn.astype(cplx), alpha.astype(cplx), beta.astype(cplx)
    r0 = np.zeros_like(alpha)
    r1 = np.zeros_like(alpha)
    for i in range(nz):
        r0 = r0 + fn[:, i] * t["cinvA"][i]
        r1 = r1 + fn[:, i] * t["cinvA"][nz + i]
    r0, r1 = r0 - alpha, r1 - beta
    m = t["m22"]
    det = m[0] * m[3] - m[1] * m[2]
    c0 = (r0 * m[3] - r1 * m[1]) / det
    d0 = (r1 * m[0] - r0 * m[2]) / det
    an = np.zeros_like(fn)
    an[:, 0] = fn[:, 0] + c0 * t["kH2"][0]
    an[:, 1] = fn[:, 1] + d0 * t["kH2"][0]
    for i in range(2, nz):
        an[:, i] = fn[:, i] - an[:, i - 2] * t["diagonal_m2"][i] / t["beta"][i - 2]
    for i in range(nz - 1, -1, -1):
        v = an[:, i]
        if i + 2 < nz:
            v = v - an[:, i + 2] * t["diagonal_p2"][i]
        an[:, i] = v / t["beta"][i]
    zero = np.zeros_like(c0)

    def a(i):
        return an[:, i] if i < nz else zero

    def d(i):
        if i == 0:
            return d0
        if i >= nz:
            return zero
        if i == 1:
            return a(0) - a(2) * real(0.5)
        return (a(i - 1) - a(i + 1)) * (real(0.5) / real(i))

    H2 = real(H * H)
    cn = np.zeros_like(fn)
    cn[:, 0] = c0 * H2
    cn[:, 1] = (d0 - d(2) * real(0.5)) * H2
    for i in range(2, nz):
        cn[:, i] = ((d(i - 1) - d(i + 1)) * (real(0.5) / real(i))) * H2
    return cn.astype(cplx), an.astype(cplx)


# ---------------------------------------------------------------------------------------------------------------- test problems
def boundary_factors(k, H):
    """The factors of the reference's unit test: a Robin pair for k != 0, Dirichlet at k = 0."""
    k = np.atleast_1d(np.asarray(k, dtype=np.float64))
    nonzero = k != 0
    return (np.where(nonzero, H, 0.0), np.where(nonzero, k * H * H, 1.0), np.where(nonzero, H, 0.0), np.where(nonzero, -k * H * H, 1.0))


def nodes(nz, H):
    return H * np.cos(np.pi * np.arange(nz) / (nz - 1))


def manufactured(z, kind="smooth"):
    """(y, y', y'') at z."""
    if kind == "quadratic":
        return z * z + z, 2 * z + 1, 2 + 0 * z
    e = np.exp(-z * z)
    return e + 0.3 * np.sin(2 * z), -2 * z * e + 0.6 * np.cos(2 * z), (4 * z * z - 2) * e - 1.2 * np.sin(2 * z)


def manufactured_problem(k, H, nz, kind="smooth"):
    """fn (nz, nsys), alpha, beta (nsys) and the samples of y (nz) for the wave numbers k with boundary_factors(k, H)."""
    k = np.atleast_1d(np.asarray(k, dtype=np.float64))
    z = nodes(nz, H)
    y, yp, ypp = manufactured(z, kind)
    f = ypp[:, None] - (k ** 2)[None, :] * y[:, None]
    fn = chebyshev_forward(f.astype(np.complex128))
    tfi, tsi, bfi, bsi = boundary_factors(k, H)
    alpha = tfi * yp[0] / H + tsi * y[0] / H ** 2
    beta = bfi * yp[-1] / H + bsi * y[-1] / H ** 2
    return fn, alpha.astype(np.complex128), beta.astype(np.complex128), y
