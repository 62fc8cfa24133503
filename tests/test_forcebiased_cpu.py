"""CPU tests of MC::ForceBiased: the exported symbols and the refusals that are decided on the host, the header and
the example under plain g++ (the C++ constructor's refusals need a ParticleData, which allocates on the device: they run in
tests/test_gpu_forcebiased.py), forcebiased_ns::Optimize of the header against the restatement's rule step for step, the host draws of the
Python class, and the restatement tests/forcebiased_ref.py itself on the harmonic trap, where <U> is known exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forcebiased_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include", "uammd"), "-I", os.path.join(ROOT, "include")]
GXX = ["g++", "-std=c++14", "-x", "c++", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + INC
REF_PROGRAM = "/root/reference/test/MC/ForceBiased/ForceBiased.cu"
F = np.float32


def test_symbols_and_host_side_refusals(hip):
    """Everything below is decided before the library touches the device: it runs without a GPU."""
    from uammd_amd._lib import UammdHipError, check
    lib = hip.load()
    for name in ("create", "destroy", "begin", "propose", "decide", "result", "stored"):
        assert hasattr(lib, "uammd_mc_forcebiased_" + name)
    h = C.c_void_p()
    check(lib.uammd_mc_forcebiased_create(C.byref(h)))
    p = C.c_void_p(4096)   # never dereferenced: every call below is refused first
    acc, out = C.c_int(), (C.c_double * 6)()
    calls = {
        "create null": lambda: lib.uammd_mc_forcebiased_create(None),
        "begin null handle": lambda: lib.uammd_mc_forcebiased_begin(None, p, p, p, 8, None),
        "begin null pos": lambda: lib.uammd_mc_forcebiased_begin(h, None, p, p, 8, None),
        "begin null force": lambda: lib.uammd_mc_forcebiased_begin(h, p, None, p, 8, None),
        "begin null energy": lambda: lib.uammd_mc_forcebiased_begin(h, p, p, None, 8, None),
        "begin N = 0": lambda: lib.uammd_mc_forcebiased_begin(h, p, p, p, 0, None),
        "begin N < 0": lambda: lib.uammd_mc_forcebiased_begin(h, p, p, p, -3, None),
        "propose null pos": lambda: lib.uammd_mc_forcebiased_propose(h, None, 8, 0.1, 1.0, 1, 1, None, None),
        "propose N = 0": lambda: lib.uammd_mc_forcebiased_propose(h, p, 0, 0.1, 1.0, 1, 1, None, None),
        "propose before begin": lambda: lib.uammd_mc_forcebiased_propose(h, p, 8, 0.1, 1.0, 1, 1, None, None),
        "decide null force": lambda: lib.uammd_mc_forcebiased_decide(h, p, None, p, 8, 0.1, 1.0, 0.5, None),
        "decide N = 0": lambda: lib.uammd_mc_forcebiased_decide(h, p, p, p, 0, 0.1, 1.0, 0.5, None),
        "decide before begin": lambda: lib.uammd_mc_forcebiased_decide(h, p, p, p, 8, 0.1, 1.0, 0.5, None),
        "result null": lambda: lib.uammd_mc_forcebiased_result(h, None, out, None),
        "result before begin": lambda: lib.uammd_mc_forcebiased_result(h, C.byref(acc), out, None),
        "stored null": lambda: lib.uammd_mc_forcebiased_stored(h, None, p, None),
        "stored before begin": lambda: lib.uammd_mc_forcebiased_stored(h, p, p, None),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert b"uammd_mc_forcebiased" in lib.uammd_hip_last_error(), what
        with pytest.raises(UammdHipError):
            check(call())
    check(lib.uammd_mc_forcebiased_destroy(h))


def test_step_size_and_beta_are_refused(hip):
    """stepSize <= 0 (or NaN) and beta < 0 are refused with a message of their own, before the size is looked at."""
    from uammd_amd._lib import check
    lib = hip.load()
    h = C.c_void_p()
    check(lib.uammd_mc_forcebiased_create(C.byref(h)))
    p = C.c_void_p(4096)   # never dereferenced
    for step, beta, msg in ((0.0, 1.0, b"stepSize must be positive"), (-0.1, 1.0, b"stepSize must be positive"),
                            (float("nan"), 1.0, b"stepSize must be positive"), (0.1, -1e-3, b"beta must not be negative"),
                            (0.1, float("nan"), b"beta must not be negative")):
        assert lib.uammd_mc_forcebiased_propose(h, p, 8, step, beta, 1, 1, None, None) != 0
        assert msg in lib.uammd_hip_last_error() and b"propose" in lib.uammd_hip_last_error()
        assert lib.uammd_mc_forcebiased_decide(h, p, p, p, 8, step, beta, 0.5, None) != 0
        assert msg in lib.uammd_hip_last_error() and b"decide" in lib.uammd_hip_last_error()
    check(lib.uammd_mc_forcebiased_destroy(h))


def test_python_class_exists_and_refuses(hip):
    import uammd_amd
    assert uammd_amd.MC.ForceBiased is hip.MC.ForceBiased and "MC" in uammd_amd.__all__
    P = hip.MC.ForceBiased.Parameters
    assert (P().beta, P().stepSize, P().acceptanceRatio, P().maxTrials) == (-1.0, 0.1, 0.5, 1000000)
    pd = hip.ParticleData(8, device="cpu")
    for kw in (dict(), dict(beta=-0.5), dict(beta=1.0, stepSize=0.0), dict(beta=1.0, stepSize=-1.0), dict(beta=1.0, acceptanceRatio=0.0),
               dict(beta=1.0, maxTrials=0)):
        with pytest.raises(RuntimeError, match="Invalid parameter"):
            hip.MC.ForceBiased(pd, P(**kw))
    with pytest.raises(RuntimeError, match="group other than"):
        hip.MC.ForceBiased(hip.ParticleGroup(pd, [0, 1, 2]), P(beta=1.0))
    hip.MC.ForceBiased(hip.ParticleGroup(pd), P(beta=1.0))     # the group of all particles is the other constructor


def test_python_host_draws_follow_the_system_generator(hip):
    """seed = next32() at construction (ForceBiased.cuh:178), nothing else; a refused construction draws nothing."""
    from uammd_amd.md import Xorshift128plus
    pd = hip.ParticleData(8, device="cpu", seed=0xC0FFEE)
    r = Xorshift128plus()
    r.set_seed(0xC0FFEE)
    with pytest.raises(RuntimeError):
        hip.MC.ForceBiased(pd, hip.MC.ForceBiased.Parameters(beta=-1.0))
    assert pd.rng.s == r.s
    mala = hip.MC.ForceBiased(pd, hip.MC.ForceBiased.Parameters(beta=2.0, stepSize=0.3))
    assert mala.seed == r.next32() and pd.rng.s == r.s
    assert mala.getCurrentStepSize() == float(F(0.3)) and mala.getCurrentAcceptanceRatio() == 0.0
    assert mala.getLastNumberOfTrials() == 0 and mala.getTotalNumberOfTrials() == 0 and mala.getCurrentEnergy() == 0.0


def test_header_and_example_pass_plain_gxx(tmp_path):
    for src in (os.path.join(ROOT, "examples", "forcebiased.cpp"), os.path.join(ROOT, "tests", "cxx", "forcebiased_host.cpp")):
        r = subprocess.run(GXX + [src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    dp = tmp_path / "dp.cpp"
    dp.write_text('#include "Integrator/MonteCarlo/ForceBiased.cuh"\nint main() { return 0; }\n')
    r = subprocess.run(GXX + ["-DDOUBLE_PRECISION", str(dp)], capture_output=True, text=True)
    assert r.returncode != 0 and "single-precision backend only" in r.stderr and "ForceBiased.cuh" in r.stderr, r.stderr[-2000:]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory, hip):
    """tests/cxx/forcebiased_host.cpp built with plain g++ against the library (no device code, no GPU needed to run it)."""
    hip.load()
    exe = str(tmp_path_factory.mktemp("forcebiased") / "forcebiased_host")
    libdir = os.path.join(ROOT, "uammd_amd", "lib")
    cmd = ["g++", "-std=c++14", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + INC + [
        os.path.join(ROOT, "tests", "cxx", "forcebiased_host.cpp"), "-o", exe, "-L" + libdir, "-luammd_hip", "-L/opt/rocm/lib", "-lamdhip64",
        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _scripts():
    """3000 tries each (three controls), together crossing both bounds: the step may pass 2 by one growth and then stays; it may fall
    under 1e-8 by one shrink and then stays; a ratio exactly on the target changes nothing."""
    rng = np.random.default_rng(5)
    blocks = lambda *p: "".join("".join("1" if x else "0" for x in rng.random(1000) < q) for q in p)
    return [(0.5, 1.99, "1" * 1000 + "1" * 1000 + "0" * 1000),            # grows past 2, is held there, shrinks
            (0.5, 1.05e-8, "0" * 1000 + "0" * 1000 + "1" * 1000),         # shrinks under 1e-8, is held there, grows
            (0.5, 0.3, ("10" * 500) + blocks(0.7, 0.2)),                  # exactly on target: unchanged; then up; then down
            (0.9, 1.0, blocks(0.95, 0.85, 0.9)),                          # the reference's default target
            (0.25, 1.97, blocks(0.3, 0.3, 0.1))]


@pytest.mark.parametrize("case", range(5))
def test_optimize_of_the_header_follows_the_rule(host_program, case, hip):
    target, step, script = _scripts()[case]
    assert len(script) == 3000
    r = subprocess.run([host_program, "optimize", repr(target), repr(step)], input=script + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [tuple(float.fromhex(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == 3000
    want, py = ref.Optimize(target, step), hip.MC.Optimize(target, step)
    changes = 0
    for k, c in enumerate(script):
        before = want.step
        want.register(c == "1")
        (py.registerAccept if c == "1" else py.registerReject)()
        changes += want.step != before
        assert got[k] == (float(want.step), float(want.ratio)), (k, got[k], want.step, want.ratio)
        assert (float(py.getStepSize()), float(py.getCurrentAcceptanceRatio())) == got[k], k
    assert changes == (2, 2, 2, 3, 2)[case]
    if case == 0:
        assert got[999][0] > 2.0 and got[1999][0] == got[999][0] and got[2999][0] < got[1999][0]
    if case == 1:
        assert got[999][0] < 1e-8 and got[1999][0] == got[999][0] and got[2999][0] > got[1999][0]
    if case == 2:
        assert got[999] == (float(F(0.3)), 0.5)


@pytest.mark.skipif(not os.path.isfile(REF_PROGRAM), reason="the reference tree is not on this machine")
def test_reference_test_program_compiles(tmp_path):
    """test/MC/ForceBiased/ForceBiased.cu of the reference (BD, VerletNVT and MC::ForceBiased over PairForces with LJ and with a
    potential of its own), read from where it lies with the one-token substitutions of tests/test_reference_programs_compile.py."""
    from test_reference_programs_compile import _source
    src, _ = _source("../test/MC/ForceBiased/ForceBiased.cu", tmp_path, ".hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-fsyntax-only", "-std=c++17", "-w", "-I", os.path.dirname(REF_PROGRAM)] + INC + [src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_restatement_pieces():
    """The proposal is float32 in the stated order, .w is kept, the sums are float64, the decision follows its corner rules."""
    rng = np.random.default_rng(1)
    X, FX, xi = (rng.normal(0, 1, (5, 4)).astype(F) for _ in range(3))
    Y = ref.propose(X, FX, 0.3, 2.0, xi)
    amp = F(np.sqrt(2.0 * float(F(0.3)) / 2.0))
    for i in range(5):
        for c in range(3):
            assert Y[i, c] == F(X[i, c] + F(F(FX[i, c] * F(0.3)) + F(amp * xi[i, c])))
        assert Y[i, 3] == X[i, 3]
    FY, e = rng.normal(0, 1, (5, 4)).astype(F), rng.normal(0, 1, 5).astype(F)
    S, A = ref.sums(X, Y, FX, FY, e, 0.3)
    h = float(F(0.3))
    want = sum(sum((float(Y[i, c]) - float(X[i, c]) - h * float(FX[i, c])) ** 2 for c in range(3)) for i in range(5))
    assert abs(S[1] - want) <= 1e-14 * want and S[0] == pytest.approx(float(e.astype(np.float64).sum()), abs=1e-15) and A[0] >= abs(S[0])
    d = ref.decide(1.0, S, 0.3, 2.0, 0.0)
    assert d["exponent"] == -2.0 * ((d["EY"] - 1.0) + (d["TYX"] - d["TXY"])) and d["TXY"] == S[1] / (4 * h)
    assert ref.decide(1.0, [np.nan, 1, 1], 0.3, 2.0, 0.0)["EY"] == ref.FLT_MAX and not ref.decide(1.0, [np.nan, 1, 1], 0.3, 2.0, 0.0)["accepted"]
    assert not ref.decide(1.0, [np.inf, 1, 1], 0.3, 2.0, 0.0)["accepted"]
    assert not ref.decide(1.0, [1.0, 1, np.inf], 0.3, 2.0, 0.0)["accepted"]
    assert not ref.decide(1.0, [1.0, np.inf, np.inf], 0.3, 2.0, 0.0)["accepted"]        # a NaN exponent rejects
    assert ref.decide(ref.FLT_MAX, [5.0, 1, 2], 0.3, 2.0, 1 - 2.0 ** -24)["accepted"]   # E_X = FLT_MAX accepts any finite Y
    assert ref.decide(1.0, [0.5, 1, 1], 0.3, 2.0, 1 - 2.0 ** -24)["accepted"]           # a positive exponent accepts every Z < 1


def test_restatement_samples_the_harmonic_trap():
    """N = 64 particles in U = k |x|^2 / 2, k = 1, beta = 2: <U> = 3 N / (2 beta) = 48 exactly.  10 000 calls from h0 = 0.3, the first
    fifth dropped.  The trial-weighted mean (the state a call starts from, weighted by the trials the call took) must be within 3 of its
    own 20-batch standard errors of 48; the unweighted mean over the states after each call is biased upwards and is
    only printed.  Measured: weighted 48.128, unweighted 49.378, se_ref 0.0892 (the GPU test and DESIGN.md section 19 quote this se_ref)."""
    N, k, beta, h0, calls = 64, 1.0, 2.0, 0.3, 10000
    rng = np.random.default_rng(2024)
    pos = np.zeros((N, 4), F)
    pos[:, :3] = rng.normal(0, np.sqrt(1 / (beta * k)), (N, 3))
    xi = lambda step, n: rng.normal(0, 1, (n, 4)).astype(F)
    drv = ref.Driver(pos, ref.trap(k), beta, h0, 0.5, xi, rng.random)
    u_start, u_after = [], []
    for _ in range(calls):
        u_start.append(drv.EX)
        drv.forward_time()
        u_after.append(drv.EX)
    drop = calls // 5
    mean, se = ref.weighted_mean_and_error(u_start[drop:], drv.trials[drop:])
    print(f"trap: weighted <U> {mean:.4f}  unweighted <U> {np.mean(u_after[drop:]):.4f}  se_ref {se:.4f}  trials {sum(drv.trials)}  "
          f"step {drv.opt.step:.4f}  ratio {drv.opt.ratio:.3f}")
    assert abs(mean - 48.0) <= 3 * se, (mean, se)
