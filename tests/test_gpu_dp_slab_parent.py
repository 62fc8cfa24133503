"""The doubly periodic solvers give the bits they gave before their shared code moved into csrc/dp_slab.hpp.

tests/golden/dp_slab_parent.npz was recorded on an MI355X by tools/record_dp_slab_golden.py from the commit before the move.  Everything
compared here is on the default path (owner-computes spread, the gather's fixed butterfly, the unchanged transforms), which is
reproducible to the bit; every entry is compared with np.array_equal, large grids through the SHA-256 of their bytes.

  DPStokes   Mdot in full, SHA-256 of fluid_cheb(): the cases below; "A10" is shape A with w = 10, a footprint of 100 columns, so the
             gather's second column per lane runs (w = 6 only ever runs the first)
  DPPoisson  field_potential, force and energy in full, SHA-256 of grid_near, grid_all and mismatch: support 12, 144 columns, three per lane
"""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_dppoisson as dpp  # noqa: E402
import test_gpu_dpstokes as dps  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "dp_slab_parent.npz")
STOKES = [("A", 65, "slit"), ("B", 300, "slit"), ("C", 65, "bottom"), ("B", 1, "none"), ("A10", 65, "slit")]
POISSON = [("A", "metal_top"), ("B", "dielectric"), ("C", "uniform")]
REALS = ["double", "float"]


def _digest(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def stokes_entries(shape, n, mode, real):
    """name -> array of one DPStokes case, in the handle's own precision"""
    import torch
    solver = dps.product(shape, mode, real)
    pos, force = dps.particles(shape, n)
    out = solver.Mdot(dps.upload(pos, real), dps.upload(force, real))
    torch.cuda.synchronize()
    key = f"dpstokes_{shape}_{n}_{mode}_{real}_"
    fluid = solver.fluid_cheb()
    return {key + "mdot": out.cpu().numpy(), key + "fluid_cheb_sha256": _digest(np.stack([fluid.real, fluid.imag], axis=-1))}


def poisson_entries(shape, wall, real):
    """name -> array of one DPPoisson case, in the handle's own precision"""
    import torch
    slab = dpp.product(shape, wall, real)
    slab.set_option("keep_stages", 1)
    pos, q = dpp.particles(shape)
    p, c = dpp.upload(pos, q, real)
    force = torch.zeros((len(q), 4), dtype=p.dtype, device="cuda")
    energy = torch.zeros((len(q),), dtype=p.dtype, device="cuda")
    fp = slab.field_potential_arrays(p, c, force, energy)
    torch.cuda.synchronize()
    key = f"dppoisson_{shape}_{wall}_{real}_"
    out = {key + "field_potential": fp.cpu().numpy(), key + "force": force.cpu().numpy(), key + "energy": energy.cpu().numpy()}
    for name in ("grid_near", "grid_all", "mismatch"):
        out[key + name + "_sha256"] = _digest(slab.get_stage(name).cpu().numpy())
    return out


def record(path):
    """What tools/record_dp_slab_golden.py writes."""
    out = {}
    for real in REALS:
        for case in STOKES:
            out.update(stokes_entries(*case, real))
        for case in POISSON:
            out.update(poisson_entries(*case, real))
    np.savez(path, **out)
    return out


def _same(got):
    assert os.path.exists(GOLDEN)
    with np.load(GOLDEN) as want:
        for name, a in got.items():
            assert name in want.files, name
            assert a.dtype == want[name].dtype and np.array_equal(a, want[name]), f"{name} differs from the parent's"


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,n,mode", STOKES)
def test_dpstokes_same_bits_as_the_parent(shape, n, mode, real):
    _same(stokes_entries(shape, n, mode, real))


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,wall", POISSON)
def test_dppoisson_same_bits_as_the_parent(shape, wall, real):
    _same(poisson_entries(shape, wall, real))


def test_every_golden_entry_is_compared():
    names = set()
    for real in REALS:
        for shape, n, mode in STOKES:
            names |= {f"dpstokes_{shape}_{n}_{mode}_{real}_{k}" for k in ("mdot", "fluid_cheb_sha256")}
        for shape, wall in POISSON:
            names |= {f"dppoisson_{shape}_{wall}_{real}_{k}"
                      for k in ("field_potential", "force", "energy", "grid_near_sha256", "grid_all_sha256", "mismatch_sha256")}
    with np.load(GOLDEN) as want:
        assert set(want.files) == names
