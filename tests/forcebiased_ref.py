"""NumPy restatement of MC::ForceBiased (uammd_amd/csrc/forcebiased.hip), for the CPU and GPU tests.

  normals(o32, seed, step, n)        the draws of the proposal: Saru(seed, step, i), first pair -> x, y; first of the second pair -> z
  propose(X, FX, h, beta, xi)        float32, in the kernel's order: X + (F h + amp xi), amp = float32(sqrt(2 h / beta)); .w from X
  sums(X, Y, FX, FY, energy, h)      float64 terms from the float32 inputs: sum e, sum |Y - X - h F(X)|^2, sum |X - Y - h F(Y)|^2,
                                     and the sums of the absolute values of the terms (the error bound of the GPU test scales with them)
  decide(EX, S, h, beta, Z)          float64: E_Y (FLT_MAX when not finite), T_XY, T_YX, the exponent and Z < exp(exponent)
  Optimize                           forcebiased_ns::Optimize in the reference's types
  Driver                             forwardTime() over any force_energy(pos) callable, recording the trials of every call
U is the sum of the per-particle energies (not half of it): DESIGN.md section 19.
"""
import math

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def normals(o32, seed, step, n):
    xi = np.zeros((n, 4), F)
    for i in range(n):
        g = o32.saru_gf((seed, step, i), 0.0, 1.0, 2)
        xi[i, 0], xi[i, 1], xi[i, 2] = g[0], g[1], g[2]
    return xi


def noise_amplitude(h, beta):
    with np.errstate(divide="ignore"):
        return F(np.sqrt(np.float64(2.0) * np.float64(F(h)) / np.float64(F(beta))))


def propose(X, FX, h, beta, xi):
    X, FX, xi = np.asarray(X, F), np.asarray(FX, F), np.asarray(xi, F)
    h, amp = F(h), noise_amplitude(h, beta)
    Y = X.copy()
    Y[:, :3] = X[:, :3] + (FX[:, :3] * h + amp * xi[:, :3])
    assert Y.dtype == np.float32
    return Y


def exp_or_inf(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def sums(X, Y, FX, FY, energy, h):
    """(S[3], A[3]): the three sums and the sums of the absolute values of their terms, all float64."""
    X, Y, FX, FY = (np.asarray(a, F).astype(np.float64)[:, :3] for a in (X, Y, FX, FY))
    e = np.asarray(energy, F).astype(np.float64)
    h = np.float64(F(h))
    with np.errstate(all="ignore"):
        t1 = (((Y - X) - h * FX) ** 2).sum(axis=1)
        t2 = (((X - Y) - h * FY) ** 2).sum(axis=1)
        S = np.array([e.sum(), t1.sum(), t2.sum()])
        A = np.array([np.abs(e).sum(), t1.sum(), t2.sum()])
    return S, A


def clamp_energy(e):
    """An energy that is not finite, or past the range of float32, becomes FLT_MAX."""
    e = float(e)
    return e if abs(e) <= FLT_MAX else FLT_MAX


def decide(EX, S, h, beta, Z):
    h, beta = float(F(h)), float(F(beta))
    with np.errstate(all="ignore"):
        EY = clamp_energy(S[0])
        TXY, TYX = float(np.float64(S[1]) / (4.0 * h)), float(np.float64(S[2]) / (4.0 * h))
        exponent = float(np.float64(-beta) * ((np.float64(EY) - np.float64(EX)) + (np.float64(TYX) - np.float64(TXY))))
    accepted = (not math.isnan(exponent)) and Z < exp_or_inf(exponent)
    return dict(EX=EX, EY=EY, TXY=TXY, TYX=TYX, exponent=exponent, accepted=accepted, current=EY if accepted else EX)


class Optimize:
    """forcebiased_ns::Optimize: a control every 1000 tries; x 1.02 above the target while the step is below 2, x 0.9 below it while the
    step is above 1e-8; float arithmetic; the ratio is published at each control."""

    def __init__(self, target, step):
        self.target, self.step, self.ratio = F(target), F(step), F(0)
        self.naccept = self.ntry = 0

    def register(self, accepted):
        self.naccept += int(bool(accepted))
        self.ntry += 1
        if self.ntry % 1000 == 0:
            ratio = F(self.naccept) / F(self.ntry)
            if ratio > self.target and self.step < F(2):
                self.step = F(self.step * F(1.02))
            elif ratio < self.target and self.step > F(1e-8):
                self.step = F(self.step * F(0.9))
            self.naccept = self.ntry = 0
            self.ratio = ratio


class Driver:
    """MC::ForceBiased over force_energy(pos4) -> (force4, energy[N]); xi(step, n) supplies the normals of a trial (real4 rows) and
    uniform() the Z of a trial."""

    def __init__(self, pos, force_energy, beta, stepSize, acceptanceRatio, xi, uniform, maxTrials=1000000):
        self.fe, self.beta, self.xi, self.uniform, self.maxTrials = force_energy, F(beta), xi, uniform, maxTrials
        self.opt = Optimize(acceptanceRatio, stepSize)
        self.X = np.asarray(pos, F).copy()
        self.FX, e = force_energy(self.X)
        self.FX = np.asarray(self.FX, F)
        self.EX = clamp_energy(np.asarray(e, F).astype(np.float64).sum())
        self.step = 0
        self.trials = []          # trials of every forwardTime()
        self.last = None

    def try_new_step(self):
        self.step += 1
        h = self.opt.step
        Y = propose(self.X, self.FX, h, self.beta, self.xi(self.step, len(self.X)))
        FY, e = self.fe(Y)
        FY = np.asarray(FY, F)
        S, _ = sums(self.X, Y, self.FX, FY, e, h)
        self.last = d = decide(self.EX, S, h, self.beta, float(F(self.uniform())))
        if d["accepted"]:
            self.X, self.FX, self.EX = Y, FY, d["EY"]
        self.opt.register(d["accepted"])
        return d["accepted"]

    def forward_time(self):
        n = 0
        while True:
            n += 1
            if self.try_new_step():
                self.trials.append(n)
                return
            if n >= self.maxTrials:
                raise RuntimeError("maxTrials")


def weighted_mean_and_error(u_start, trials, nbatch=20):
    """The trial-weighted mean of u_start (the energy each call STARTED from, weight = the trials that call took) and its standard error
    from nbatch consecutive batches of calls."""
    u, w = np.asarray(u_start, np.float64), np.asarray(trials, np.float64)
    mean = (u * w).sum() / w.sum()
    b = [(ub * wb).sum() / wb.sum() for ub, wb in zip(np.array_split(u, nbatch), np.array_split(w, nbatch))]
    return mean, float(np.std(b, ddof=1) / np.sqrt(nbatch))


def trap(k=1.0):
    """force = -k x, energy = k |x|^2 / 2 per particle, in float32."""
    def fe(pos):
        pos = np.asarray(pos, F)
        f = np.zeros_like(pos)
        f[:, :3] = -F(k) * pos[:, :3]
        return f, (F(0.5) * F(k)) * (pos[:, :3] * pos[:, :3]).sum(axis=1, dtype=F)
    return fe
