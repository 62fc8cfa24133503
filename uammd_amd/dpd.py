"""Dissipative particle dynamics and constant-energy MD: Potential.DPD and VerletNVE.

Mirror of the reference's Interactor/Potential/DPD.cuh and Integrator/VerletNVE.{cuh,cu}, with the step sequencing of the C++ classes in
include/uammd (Interactor/Potential/DPD.cuh, Integrator/VerletNVE.cuh); every force sum and every half step runs in libuammd_hip.so
(uammd_dpd_transverse_celllist / _nbody in uammd_amd/csrc/dpd.hip, uammd_verletnve in integrators.hip).

    dpd = Potential.DPD(cutOff=1.0, dt=0.01, gamma=4.5, temperature=1.0, A=25.0)
    verlet = VerletNVE(pd, dt=0.01, initVelocities=False)
    verlet.addInteractor(PairForces(pd, box, dpd))
    verlet.forwardTime()

PairForces<Potential::DPD> sums what DPD.cuh's ForceTransverser::compute plainly means, although the reference's PairForces never reaches it
(DESIGN.md section 12).
"""
import logging
import math

import numpy as np
import torch

from ._lib import check, f3, i3
from .md import CellList, Integrator, ParticleGroup, Potential, _ptr, current_stream

_log = logging.getLogger("uammd_amd")


class DPD:
    """Potential::DPD = DPD_impl<DefaultDissipation> (DPD.cuh:40-181): a constant gamma."""

    def __init__(self, cutOff=1.0, dt=0.0, gamma=1.0, temperature=0.0, A=1.0):
        self.rcut, self.dt, self.gamma, self.temperature, self.A = float(cutOff), float(dt), float(gamma), float(temperature), float(A)
        self.step = 0
        self.seed = None
        self._update_sigma()

    def _update_sigma(self):   # DPD.cuh:69: sigma = sqrt(2 kT) / sqrt(dt), in double, stored as real
        self.sigma = float(np.float32(math.sqrt(2.0 * self.temperature) / math.sqrt(self.dt))) if self.dt > 0 else float("inf")

    def getCutOff(self):
        return self.rcut

    def updateTemperature(self, T):   # DPD.cuh:82-85
        self.temperature = float(T)
        self._update_sigma()

    def updateTimeStep(self, dt):     # DPD.cuh:87-90
        self.dt = float(dt)
        self._update_sigma()

    def next_force_arguments(self, pd):
        """DPD.cuh:161-170: the seed is drawn once from the System's generator, the step advances once per transverser request."""
        if self.seed is None:
            self.seed = pd.rng.next()
        self.step += 1
        return self.seed, self.step

    def sum_pair_forces(self, pf, force, energy, virial):
        """PairForces<Potential::DPD, CellList>::sum (PairForces.cu:43-78 with DPD.cuh:121-152)."""
        pd, box = pf.pd, pf.box
        if energy or virial:   # DPD.cuh:171-180
            _log.critical("[DPD] No way of measuring energy in DPD")
        seed, step = self.next_force_arguments(pd)
        if not force:
            return
        rc = np.float32(self.rcut)
        L = box.boxSize
        per = i3([int(p) for p in box.periodic])
        useNL = not (L[0] <= 3 * rc and L[1] <= 3 * rc and L[2] <= 3 * rc)
        f = pd.getForce("readwrite")
        vel = pd.getVel("read")
        gidx = pf.pg.getIndexIterator() if pf.pg is not None else None
        args = (float(rc), self.A, self.gamma, self.sigma, seed, step, pd.N, _ptr(f), _ptr(gidx), current_stream())
        if useNL:
            if gidx is not None:   # the list is built on the members' positions (pg->getPropertyIterator(pos))
                if pf.nl is None:
                    pf.nl = CellList()
                pf.nl.force_next_update = True
                pf.nl.update(box, rc, pf.pg.getPropertyIterator(pd.getPos("read")).contiguous())
            else:
                if pf.nl is None:
                    pf.nl = CellList(pd)
                pf.nl.update(box, rc)
            if type(pf.nl) is not CellList:
                raise NotImplementedError("PairForces<Potential::DPD> runs on the CellList (a VerletList needs the C++ hipcc path)")
            check(pf.lib.uammd_dpd_transverse_celllist(pf.nl.h, _ptr(vel), f3(L), per, *args))
        else:
            n = pf.pg.getNumberParticles() if gidx is not None else pd.N
            check(pf.lib.uammd_dpd_transverse_nbody(_ptr(pd.getPos("read")), _ptr(vel), n, f3(L), per, *args))


class VerletNVE(Integrator):
    """VerletNVE (Integrator/VerletNVE.cuh:30-75, VerletNVE.cu)."""

    def __init__(self, pd, dt=0.0, energy=0.0, is2D=False, initVelocities=True, mass=-1.0):
        self.pg = None
        if isinstance(pd, ParticleGroup):
            self.pg, pd = (pd if not pd.allParticles else None), pd.getParticleData()
        super().__init__(pd)
        self.dt, self.energy, self.is2D, self.initVelocities = float(dt), float(energy), bool(is2D), bool(initVelocities)
        self.defaultMass = float(mass)
        if not pd.isAllocated("mass") and self.defaultMass < 0:   # VerletNVE.cu:51-55
            self.defaultMass = 1.0
        self.updatables = []

    def addInteractor(self, it):     # Integrator.cuh:96-107: an interactor is an updatable too
        super().addInteractor(it)
        self.addUpdatable(it)

    def addUpdatable(self, u):
        if not any(u is v for v in self.updatables):
            self.updatables.append(u)

    def _index(self):
        return self.pg.getIndexIterator() if self.pg is not None else None

    def _n(self):
        return self.pg.getNumberParticles() if self.pg is not None else self.pd.N

    def _reset_forces(self):         # VerletNVE.cu:152-158: the members' forces only
        f = self.pd.getForce("write")
        if self.pg is not None:
            check(self.lib.uammd_fill_zero_indexed(_ptr(f), _ptr(self._index()), self._n(), 16, current_stream()))
        else:
            f.zero_()

    def _sum_forces(self):
        for it in self.interactors:
            it.sum(force=True, energy=False, virial=False)

    def _integrate(self, step):      # VerletNVE.cu:133-150; the mass array wins whenever it is allocated (:76)
        pd = self.pd
        mass = pd.getMass("read") if pd.isAllocated("mass") else None
        check(self.lib.uammd_verletnve(step, _ptr(pd.getPos("readwrite")), _ptr(pd.getVel("readwrite")), _ptr(pd.getForce("read")),
                                       _ptr(mass), self.defaultMass, _ptr(self._index()), self._n(), self.dt, int(self.is2D),
                                       current_stream()))

    def _initialize_velocities(self):   # VerletNVE.cu:88-131
        pd, n = self.pd, self._n()
        idx = self._index()
        e = pd.getEnergy("write")
        if idx is None:
            e.zero_()
        else:
            e[idx.long()] = 0.0
        for it in self.interactors:
            it.sum(force=False, energy=True, virial=False)
        e = pd.getEnergy("read")
        members = np.arange(pd.N) if idx is None else idx.cpu().numpy()
        U = float(np.float32(e.cpu().numpy()[members].sum(dtype=np.float32))) / n
        K = self.energy - U
        if K < 0:
            _log.error("[VerletNVE] Cannot fix requested energy per particle. Requested E = U + K = %g, but U=%g", self.energy, U)
            raise RuntimeError("[VerletNVE] Cannot fix energy")
        mass = pd.getMass("read").cpu().numpy() if pd.isAllocated("mass") else None
        vel = pd.getVel("write")
        v = vel.cpu().numpy()
        for i in members:
            d = np.array(pd.rng.gaussian3(0.0, 1.0), dtype=np.float32)
            d = d / np.float32(math.sqrt(float(np.dot(d, d))))
            m = float(mass[i]) if mass is not None else self.defaultMass
            v[i] = np.float32(math.sqrt(2.0 * K / m)) * d
        vel.copy_(torch.from_numpy(v).to(vel.device))

    def forwardTime(self):           # VerletNVE.cu:160-188
        self.steps += 1
        if self.steps == 1:
            if self.initVelocities:
                self._initialize_velocities()
            self._reset_forces()
            for u in self.updatables:
                u.updateTimeStep(self.dt)
            self._sum_forces()
        self._integrate(1)
        self._reset_forces()
        for u in self.updatables:
            u.updateSimulationTime(self.steps * self.dt)
        self._sum_forces()
        self._integrate(2)

    def sumEnergy(self):             # VerletNVE.cu:203-224: defaultMass wins here whenever it is positive; returns 0
        pd = self.pd
        mass = None if self.defaultMass > 0 else pd.getMass("read")
        check(self.lib.uammd_sum_kinetic_energy(_ptr(pd.getVel("read")), _ptr(pd.getEnergy("readwrite")), _ptr(mass), self.defaultMass,
                                                _ptr(self._index()), self._n(), current_stream()))
        return 0.0


Potential.DPD = DPD
