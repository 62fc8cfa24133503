"""Smoothed particle hydrodynamics: the SPH interactor.

Mirror of the reference's Interactor/SPH.cuh, with the sequencing of the C++ class in include/uammd/Interactor/SPH.cuh; the density and the
force sums run in libuammd_hip.so (uammd_sph_sum_verletlist, uammd_amd/csrc/sph.hip) over a VerletList with cut-off 2 * support.

    sph = SPH(pd, box, support=2.4, viscosity=10.0, gasStiffness=60.0, restDensity=0.3)
    verlet = VerletNVE(pd, dt=0.01, initVelocities=False)
    verlet.addInteractor(sph)
    verlet.forwardTime()

The kernel "gradient" is the reference's formula as written and the force carries m_i m_j.
"""
import logging

import numpy as np
import torch

from ._lib import check, f3, i3, load
from .md import Interactor, ParticleGroup, VerletList, _ptr, current_stream

_log = logging.getLogger("uammd_amd")


class SPH(Interactor):
    """SPH (Interactor/SPH.cuh:42-75, SPH.cu)."""

    NeighbourList = VerletList

    def __init__(self, pd, box, support=1.0, viscosity=50.0, gasStiffness=100.0, restDensity=0.4, nl=None):
        if isinstance(pd, ParticleGroup):
            pg, pd = pd, pd.getParticleData()
            if pg.getNumberParticles() != pd.getNumParticles():   # SPH.cu:50-52
                _log.critical("[SPH] Not compatible with groups yet!.")
                raise RuntimeError("[CRITICAL] [SPH] Not compatible with groups yet!.")
        self.lib = load()
        self.pd, self.box = pd, box
        self.support, self.viscosity = float(support), float(viscosity)
        self.gasStiffness, self.restDensity = float(gasStiffness), float(restDensity)
        self.nl = nl
        self._density = self._pressure = None

    def updateBox(self, box):
        self.box = box

    def sum(self, force=True, energy=False, virial=False):
        """SPH::sum (SPH.cu:178-215).  The Computables are ignored as there: the force is always added, nothing else is produced."""
        pd = self.pd
        if self.nl is None:
            self.nl = VerletList(pd)
        rcut = float(np.float32(2.0) * np.float32(self.support))   # Kernel::getCutOff
        self.nl.update(self.box, rcut)
        if self._density is None or self._density.shape[0] != pd.N:
            self._density = torch.empty(pd.N, dtype=torch.float32, device=pd.device)
            self._pressure = torch.empty(pd.N, dtype=torch.float32, device=pd.device)
        mass = pd.getMass("read") if pd.isAllocated("mass") else None
        check(self.lib.uammd_sph_sum_verletlist(self.nl.h, _ptr(pd.getVel("read")), _ptr(mass), f3(self.box.boxSize),
                                                i3([int(p) for p in self.box.periodic]), self.support, self.viscosity, self.gasStiffness,
                                                self.restDensity, _ptr(pd.getForce("readwrite")), _ptr(self._density), _ptr(self._pressure),
                                                current_stream()))

    def density(self):
        """rho of the last sum, in particle order (the order ParticleData had at that sum)."""
        return self._density

    def pressure(self):
        """P = gasStiffness (rho - restDensity) of the last sum, in particle order."""
        return self._pressure
