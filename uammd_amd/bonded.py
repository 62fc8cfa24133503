"""Bonded interactions: BondedForces / AngularBondedForces / TorsionalBondedForces with the built-in kinds.

Mirror of the reference's Interactor/BondedForces.{cuh,cu}, AngularBondedForces.cuh and TorsionalBondedForces.cuh; every sum runs in
libuammd_hip.so (uammd_bonded_*, uammd_amd/csrc/bonded.hip).  A bond set comes from a bond file in the reference's format or from
arrays:

    nbonds
    i j [k [l]] BONDINFO          (BONDINFO = the two numbers "k p0" of the kind, as each BondType::readBond reads them)
    ...
    nFixedPoints                  (2-member kinds only, optional)
    i x y z BONDINFO

The rows follow the particles through ParticleData.sortParticles (pd.connectReorder).  Torsional uses the intended member mapping, not
the reference's shifted one.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, f3, i3
from .md import Box, Interactor, _ptr, current_stream


class _Kind:
    kind = -1
    members = 2
    swap = True   # the bond line gives "k p0"; BondInfo holds {p0, k} (readBond reads into the fields in that order)

    def __init__(self, box=None):
        self.box = box if box is not None else Box(0.0)   # Harmonic(Box box = Box()): no minimum image


class _Harmonic(_Kind):
    """BondedType::Harmonic (BondedForces.cuh:83-117): BondInfo {k, r0}."""
    kind, members, swap = 0, 2, False


class _FENE(_Kind):
    """BondedType::FENE (BondedForces.cuh:140-166): BondInfo {r0, k}; the file gives k then r0."""
    kind, members = 1, 2


class _Angular(_Kind):
    """BondedType::Angular (AngularBondedForces.cuh:50-138): BondInfo {ang0, k}; force only."""
    kind, members = 2, 3


class _Torsional(_Kind):
    """BondedType::Torsional (TorsionalBondedForces.cuh:43-117): BondInfo {phi0, k}; force only."""
    kind, members = 3, 4


class _FourierLAMMPS(_Kind):
    """BondedType::FourierLAMMPS (TorsionalBondedForces.cuh:119-217): BondInfo {phi0, kdih}; force, energy and virial."""
    kind, members = 4, 4


class BondedType:
    Harmonic = _Harmonic
    FENE = _FENE
    Angular = _Angular
    Torsional = _Torsional
    FourierLAMMPS = _FourierLAMMPS


def read_bond_file(fileName, members):
    """BondedForces::readBonds (BondedForces.cu:139-185): returns (ids int32[nbonds, members] with fixed points as -(j+1),
    info float32[nbonds, 2] as the file gives it ("k p0"), fixedPoints float32[nfixed, 4]).  A missing file raises RuntimeError, a file
    that ends before its count OSError (std::ios_base::failure)."""
    try:
        with open(fileName) as f:
            tok = f.read().split()
    except OSError:
        raise RuntimeError(f"[BondedForces] File {fileName} cannot be opened.") from None
    pos = [0]

    def nxt(conv, what):
        if pos[0] >= len(tok):
            raise OSError(f"[BondedForces] ERROR! Bond file ended too soon! ({what})")
        v = conv(tok[pos[0]])
        pos[0] += 1
        return v

    def opt_int():   # `in >> n` at the end of the stream leaves n as it was (0)
        return nxt(int, "") if pos[0] < len(tok) else 0

    nbonds = opt_int()
    ids, info = [], []
    for b in range(nbonds):
        ids.append([nxt(int, f"expected {nbonds} lines, found {b}") for _ in range(members)])
        info.append([nxt(float, "bond info"), nxt(float, "bond info")])
    fixed = []
    if members == 2:
        nfp = opt_int()
        for b in range(nfp):
            i = nxt(int, f"expected {nfp} lines, found {b}")
            p = [nxt(float, "fixed point position") for _ in range(3)]
            ids.append([i, -(b + 1)])
            info.append([nxt(float, "bond info"), nxt(float, "bond info")])
            fixed.append(p + [0.0])
    return (np.asarray(ids, np.int32).reshape(-1, members), np.asarray(info, np.float32).reshape(-1, 2),
            np.asarray(fixed, np.float32).reshape(-1, 4))


def build_rows(ids, members):
    """The host-only CSR build (uammd_bonded_build_rows): (rowId, rowStart, entryBond)."""
    lib = _lib.load()
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    nb = ids.size // members
    nr, ne = C.c_int(), C.c_int()
    cap = max(1, ids.size)
    rid, rs, eb = np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
    check(lib.uammd_bonded_build_rows(members, nb, ids.ctypes.data_as(C.c_void_p), C.byref(nr), C.byref(ne), rid.ctypes.data_as(C.c_void_p),
                                      rs.ctypes.data_as(C.c_void_p), eb.ctypes.data_as(C.c_void_p)))
    return rid[:nr.value].copy(), rs[:nr.value + 1].copy(), eb[:ne.value].copy()


class BondedForces(Interactor):
    """BondedForces<BondType, particlesPerBond> (BondedForces.cuh:170-212).

    BondedForces(pd, BondedForces.Parameters(file=...), bondType) reads a bond file; BondedForces(pd, bondType=..., ids=, info=,
    fixedPoints=) takes arrays: ids int[nbonds, members] (a negative id -(j+1) names fixedPoints[j]), info float[nbonds, 2] in the file's
    order ("k p0")."""

    class Parameters:
        def __init__(self, file=""):
            self.file = file

    particlesPerBond = None   # set by the aliases below

    def __init__(self, pd, par=None, bondType=None, ids=None, info=None, fixedPoints=None):
        self.lib = _lib.load()
        self.pd = pd
        self.bondType = bondType if bondType is not None else BondedType.Harmonic()
        m = self.bondType.members
        if self.particlesPerBond is not None and m != self.particlesPerBond:
            raise ValueError(f"{type(self).__name__} takes bonds of {self.particlesPerBond} particles, {type(self.bondType).__name__} has {m}")
        if par is not None and par.file:
            ids, info, fixedPoints = read_bond_file(par.file, m)
        ids = np.ascontiguousarray(np.asarray(ids if ids is not None else np.zeros((0, m)), np.int32).reshape(-1, m))
        info = np.asarray(info if info is not None else np.zeros((0, 2)), np.float32).reshape(-1, 2)
        fixedPoints = np.ascontiguousarray(np.asarray(fixedPoints if fixedPoints is not None else np.zeros((0, 4)), np.float32).reshape(-1, 4))
        if info.shape[0] != ids.shape[0]:
            raise ValueError("one BondInfo per bond")
        self.nbonds = ids.shape[0]
        structInfo = np.ascontiguousarray(info[:, ::-1] if self.bondType.swap else info, np.float32)
        h = C.c_void_p()
        check(self.lib.uammd_bonded_create(C.byref(h)))
        self.h = h
        box = self.bondType.box
        check(self.lib.uammd_bonded_upload(self.h, self.bondType.kind, self.nbonds, ids.ctypes.data_as(C.c_void_p),
                                           structInfo.ctypes.data_as(C.c_void_p), fixedPoints.shape[0], fixedPoints.ctypes.data_as(C.c_void_p),
                                           f3(box.boxSize), i3([int(p) for p in box.periodic])))
        self._refresh()
        pd.connectReorder(self._refresh)

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            torch.cuda.synchronize()
            self.lib.uammd_bonded_destroy(h)
            self.h = None

    def _refresh(self):
        pd = self.pd
        id2index = torch.empty_like(pd.id)
        id2index[pd.id.long()] = torch.arange(pd.N, dtype=torch.int32, device=pd.id.device)   # ParticleData::getIdOrderedIndices
        self._id2index = id2index
        check(self.lib.uammd_bonded_refresh(self.h, _ptr(id2index), pd.N, current_stream()))

    def shape(self):
        """(rows, entries, rows on the lane-per-row shape, rows on the wave-per-row shape)."""
        r, e, lr, wr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.lib.uammd_bonded_get_shape(self.h, C.byref(r), C.byref(e), C.byref(lr), C.byref(wr)))
        return r.value, e.value, lr.value, wr.value

    def sum(self, force=True, energy=False, virial=False):
        pd = self.pd
        f = pd.getForce("readwrite") if force else None
        e = pd.getEnergy("readwrite") if energy else None
        v = pd.getVirial("readwrite") if virial else None
        check(self.lib.uammd_bonded_sum(self.h, _ptr(pd.getPos("read")), _ptr(f), _ptr(e), _ptr(v), current_stream()))


class AngularBondedForces(BondedForces):
    """AngularBondedForces<BondType> = BondedForces<BondType, 3> (AngularBondedForces.cuh:146)."""
    particlesPerBond = 3


class TorsionalBondedForces(BondedForces):
    """TorsionalBondedForces<BondType> = BondedForces<BondType, 4> (TorsionalBondedForces.cuh:225)."""
    particlesPerBond = 4


def set_tunable(name, value):
    """uammd_hip_set_tunable: "bonded_baseline" (0 / 1), "bonded_wave_threshold" (entries)."""
    check(_lib.load().uammd_hip_set_tunable(name.encode(), int(value)))
