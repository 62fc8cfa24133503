"""MC_NVT::Anderson from C++ (include/uammd/Integrator/MonteCarlo/NVT/Anderson.cuh) on the GPU: the program of tests/cxx against the
Python class, and the reference's own two Monte Carlo programs where they were built (examples/Makefile builds them from the reference
tree when it is present)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mc_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "examples", "_build")


def _fnv1a(words):
    h = 1469598103934665603
    for c in words.tobytes():
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", ["cube6", "cube6_shifted"])
def test_mc_builtin_matches_the_python_class(hip, name, tmp_path):
    """The same system seed gives the same trajectory from either front end: position words and acceptance ratio are equal exactly."""
    exe = os.path.join(BUILD, "mc_builtin")
    assert os.path.exists(exe), "examples/_build/mc_builtin is missing: build() makes it"
    fx = mc_ref.Fixture(name)
    steps, sysseed = 3, 0xA11CE
    fx.pos.astype(np.float32).tofile(tmp_path / "pos.bin")
    shift = int(fx.pairs[(0, 0)][3])
    r = subprocess.run([exe, str(tmp_path / "pos.bin"), str(len(fx.pos)), repr(fx.L[0]), str(steps), str(sysseed), str(mc_ref.SARU_SEED),
                        str(shift)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-1500:])
    assert r.returncode == 0
    m = re.search(r"mc N (\d+) steps (\d+) hash ([0-9a-f]{16}) ratio (\S+) jump (\S+)", r.stdout)
    assert m and int(m.group(1)) == len(fx.pos)
    pd = hip.ParticleData(len(fx.pos), seed=sysseed)
    pd.setPos(fx.pos.copy())
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, bool(shift)))
    mc = hip.MC_NVT.Anderson(pd, pot, hip.MC_NVT.Anderson.Parameters(box=hip.Box(fx.L), temperature=1.5, triesPerCell=10, initialJumpSize=0.15,
                                                                      tuneSteps=steps, seed=mc_ref.SARU_SEED))
    for _ in range(steps):
        mc.forwardTime()
    words = pd.getPos().cpu().numpy().view(np.uint32)
    assert not np.array_equal(words, fx.pos.view(np.uint32))
    assert int(m.group(3), 16) == _fnv1a(words)
    assert float(m.group(4)) == float("%.9g" % mc.getCurrentAcceptanceRatio()) and 0 < float(m.group(4)) < 1
    assert float(m.group(5)) == float("%.9g" % mc.getCurrentStepSize())


@pytest.mark.parametrize("name", ["cube6", "cube6_shifted"])
def test_mc_user_functor_matches_the_builtin(name, tmp_path):
    """Potential::Radial<UserLJ> through device/Anderson.hip.hpp: the same positions, ratio and step size as the built-in potential."""
    fx = mc_ref.Fixture(name)
    fx.pos.astype(np.float32).tofile(tmp_path / "pos.bin")
    lines = []
    for prog in ("mc_builtin", "mc_user"):
        exe = os.path.join(BUILD, prog)
        assert os.path.exists(exe), "examples/_build/%s is missing: build() makes it" % prog
        r = subprocess.run([exe, str(tmp_path / "pos.bin"), str(len(fx.pos)), repr(fx.L[0]), "3", "12345", str(mc_ref.SARU_SEED),
                            str(int(fx.pairs[(0, 0)][3]))], capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr[-1500:])
        assert r.returncode == 0
        lines.append([l for l in r.stdout.splitlines() if l.startswith("mc N")][-1])
    assert lines[0] == lines[1]


def _rows(path):
    return [[float(x) for x in line.split()] for line in open(path) if line.strip()]


def test_reference_example_program(tmp_path):
    """examples/integration_schemes/others/MCNVT.cu compiled from where it lies: 2^11 particles in a box of 12, 40 steps printing every
    20, T = 2, 10 tries per cell, jump 0.1, target 0.8."""
    exe = os.path.join(BUILD, "ref_MCNVT")
    if not os.path.exists(exe):
        pytest.skip("ref_MCNVT was not built (no reference tree where `make -C examples` ran)")
    r = subprocess.run([exe, "11", "12", "40", "20", "2", "10", "0.1", "0", "0.8"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    rows = _rows(tmp_path / "energy.dat")       # sumEnergy (always 0), acceptance ratio, step size at j = 1 and 21
    assert len(rows) == 2 and all(len(x) == 3 and np.isfinite(x).all() for x in rows)
    frames = open(tmp_path / "pos.dat").read().split("#\n")[1:]
    assert len(frames) == 2 and all(len(f.strip().splitlines()) == 2048 for f in frames)
    assert np.isfinite(np.array([[float(v) for v in line.split()[:3]] for line in frames[-1].strip().splitlines()])).all()


def test_reference_acceptance_program(tmp_path):
    """test/MC/ShortRange/MonteCarlo.cu compiled from where it lies, on a small data.main written here: N = 4096, rho = 0.6, T = 2,
    test.bash's sampling parameters with a shorter run.  Every energy row is finite with U / N < 0."""
    exe = os.path.join(BUILD, "ref_test_MonteCarlo")
    if not os.path.exists(exe):
        pytest.skip("ref_test_MonteCarlo was not built (no reference tree where `make -C examples` ran)")
    n, rho = 4096, 0.6
    L = (n / rho) ** (1.0 / 3.0)
    (tmp_path / "data.main").write_text(
        f"boxSize {L} {L} {L}\nnumberSteps 100\nprintSteps 10\nrelaxSteps 50\nnumberParticles {n}\nsigma 1\nepsilon 1\ntemperature 2\n"
        "outfile pos.dat\nenergyOutfile energy.dat\nshiftLJ 0\ncutOff 2.5\ntriesPerCell 40\ninitialJumpSize 0.1\ntuneSteps 20\n"
        "desiredAcceptanceRatio 0.8\n")
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    rows = _rows(tmp_path / "energy.dat")
    assert len(rows) == 10
    for u, k in rows:
        assert np.isfinite(u) and u < 0 and k == 3.0
