"""Host-side mirror of the reference's Hydro namespace (Integrator/Hydro/ICM.cuh, ICM_Compressible.cuh): class names, parameters, error
behaviour.  Every call goes through the C ABI (uammd_icm_*, uammd_icmc_*); no CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import ICMCompressibleParameters, ICMParameters, check
from .md import Integrator, _ptr, current_stream


class ICM(Integrator):
    """Hydro::ICM(pd, par) — ICM.cuh:123-231: inertial coupling of the particles to an incompressible fluctuating fluid."""

    class Parameters:
        def __init__(self, temperature=0.0, viscosity=-1.0, density=-1.0, hydrodynamicRadius=-1.0, dt=0.0, box=None, cells=(-1, -1, -1),
                     sumThermalDrift=False, removeTotalMomentum=True, seed=0):
            self.temperature, self.viscosity, self.density, self.hydrodynamicRadius = temperature, viscosity, density, hydrodynamicRadius
            self.dt, self.box, self.cells = dt, box, list(cells)
            self.sumThermalDrift, self.removeTotalMomentum, self.seed = sumThermalDrift, removeTotalMomentum, seed

    def __init__(self, pd, par):
        super().__init__(pd)
        p = ICMParameters()
        for k in range(3):
            p.boxSize[k] = float(par.box.boxSize[k])
            p.cells[k] = int(par.cells[k])
        p.temperature, p.viscosity, p.density, p.hydrodynamicRadius, p.dt = (float(par.temperature), float(par.viscosity),
                                                                             float(par.density), float(par.hydrodynamicRadius), float(par.dt))
        p.sumThermalDrift, p.removeTotalMomentum = int(bool(par.sumThermalDrift)), int(bool(par.removeTotalMomentum))
        p.seed = int(par.seed if par.seed else pd.rng.next32()) & 0xFFFFFFFF       # seed = sys->rng().next32(), ICM.cu:831
        h, cells, rh = C.c_void_p(), (C.c_int * 3)(), C.c_float(0)
        try:
            check(self.lib.uammd_icm_create(C.byref(p), C.byref(h), C.byref(cells), C.byref(rh)))
        except _lib.UammdHipError as e:
            if "ICM]" in str(e):          # System::CRITICAL in the reference (ICM.cu:833-839, :869-872)
                raise RuntimeError(str(e)) from e
            raise
        self.h, self.cells, self.hydrodynamicRadius = h, [int(c) for c in cells], float(rh.value)
        self.par, self.box = par, par.box

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_icm_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def getHydrodynamicRadius(self):
        return self.hydrodynamicRadius

    def getSelfMobility(self):       # ICM.cuh:164-168
        rh = self.hydrodynamicRadius
        return 1.0 / (6 * math.pi * self.par.viscosity * rh) * (1 - 2.837297 * rh / float(self.box.boxSize[0]))

    def getNumberFluidCells(self):
        return list(self.cells)

    def getFluidVelocities(self, collocated=True):
        """Cell-centred fluid velocities real3[nz, ny, nx] (ICM::getFluidVelocities); collocated=False: the staggered field."""
        nx, ny, nz = self.cells
        out = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.pd.device)
        check(self.lib.uammd_icm_get_fluid_velocity(self.h, _ptr(out), int(collocated), current_stream()))
        return out

    def setFluidVelocities(self, v):
        check(self.lib.uammd_icm_set_fluid_velocity(self.h, _ptr(v.contiguous()), current_stream()))

    def set_noise(self, random):
        self._noise = random
        check(self.lib.uammd_icm_set_noise(self.h, _ptr(random) if random is not None else None))

    def forwardTime(self):
        pd, par = self.pd, self.par
        self.steps += 1
        if self.steps == 1:
            for it in self.interactors:
                it.updateTemperature(par.temperature)
                it.updateTimeStep(par.dt)
                it.updateBox(self.box)
                it.updateSimulationTime(0)
            for it in self.interactors:      # ICM.cu:1201-1203 (these forces are overwritten before they are used)
                it.sum(force=True)
        check(self.lib.uammd_icm_predictor(self.h, _ptr(pd.getPos("readwrite")), pd.N, current_stream()))
        for it in self.interactors:
            it.updateSimulationTime((self.steps - 0.5) * par.dt)
        force = None
        if self.interactors:                 # spreadParticleForces, :1040-1066: forces at q^{n+1/2}
            pd.getForce("write").zero_()
            for it in self.interactors:
                it.sum(force=True)
            force = _ptr(pd.getForce("read"))
        check(self.lib.uammd_icm_fluid_and_corrector(self.h, _ptr(pd.getPos("readwrite")), force, pd.N, current_stream()))
        pd.getForce("write").zero_()         # correctorStep resets the forces (:1176-1181)
        for it in self.interactors:
            it.updateSimulationTime(self.steps * par.dt)


class ICM_Compressible(Integrator):
    """Hydro::ICM_Compressible(pd, par) — ICM_Compressible.cuh:183-452: inertial coupling of the particles to a fluctuating compressible
    fluid (density and momentum on a staggered grid, explicit RK3), triply periodic or between two walls in z.  pd may hold no
    particles: a fluid-only run."""

    class Parameters:
        """The reference's Parameters (:193-208).  The initial fields are callables of a position (x, y, z), evaluated on the host at
        (cell / n + 0.5) * L as the reference does (:170-179, :385-403; also for the face-centred velocities), or arrays [nz, ny, nx].
        walls: None (triply periodic), or an object with velocities(t) -> ((bx, by), (tx, ty)), the in-plane velocities of the bottom and
        the top wall at time t (the library's built-in rule, uammd_hip.h).  If it has updateSimulationTime(t) it hears the four times of
        a step like any updatable; velocities(t) is asked at the three sub-step times, each before the ghost fills of that sub-stage, and
        at t = 0 on construction."""

        def __init__(self, shearViscosity=-1.0, bulkViscosity=-1.0, speedOfSound=-1.0, temperature=0.0, dt=-1.0, boxSize=None,
                     cellDim=(-1, -1, -1), hydrodynamicRadius=-1.0, seed=0, initialDensity=None, initialVelocityX=None,
                     initialVelocityY=None, initialVelocityZ=None, walls=None):
            self.shearViscosity, self.bulkViscosity, self.speedOfSound = shearViscosity, bulkViscosity, speedOfSound
            self.temperature, self.dt, self.boxSize, self.cellDim = temperature, dt, boxSize, list(cellDim)
            self.hydrodynamicRadius, self.seed, self.walls = hydrodynamicRadius, seed, walls
            self.initialDensity, self.initialVelocityX = initialDensity, initialVelocityX
            self.initialVelocityY, self.initialVelocityZ = initialVelocityY, initialVelocityZ

    def __init__(self, pd, par):
        super().__init__(pd)
        if par.walls is not None and not callable(getattr(par.walls, "velocities", None)):
            raise ValueError("[ICM_Compressible] walls must have velocities(t) -> ((bx, by), (tx, ty))")
        if par.boxSize is None:
            raise ValueError("[ICM_Compressible] Invalid box size")
        L = np.broadcast_to(np.asarray(getattr(par.boxSize, "boxSize", par.boxSize), dtype=np.float64), (3,))
        p = ICMCompressibleParameters()
        for k in range(3):
            p.boxSize[k] = float(L[k])
            p.cells[k] = int(par.cellDim[k])
        p.shearViscosity, p.bulkViscosity, p.speedOfSound = float(par.shearViscosity), float(par.bulkViscosity), float(par.speedOfSound)
        p.temperature, p.dt, p.hydrodynamicRadius = float(par.temperature), float(par.dt), float(par.hydrodynamicRadius)
        p.walls = p.WALLS_NONE if par.walls is None else p.WALLS_BUILTIN
        h, cells = C.c_void_p(), (C.c_int * 3)()
        try:
            check(self.lib.uammd_icmc_validate(C.byref(p)))    # checkInputValidity comes first: a refused set draws nothing from the generator
            p.seed = int(par.seed if par.seed else pd.rng.next32()) & 0xFFFFFFFF      # :219
            check(self.lib.uammd_icmc_create(C.byref(p), C.byref(h), C.byref(cells)))
        except _lib.UammdHipError as e:
            if "ICM_Compressible]" in str(e) or "not supported" in str(e):       # std::runtime_error in the reference (:293-311)
                raise ValueError(str(e)) from e
            raise
        self.h, self.cells, self.seed = h, [int(c) for c in cells], int(p.seed)
        self.par, self.boxSize, self.updatables, self._noise = par, [float(x) for x in L], [], None
        self.walls = par.walls
        if self.walls is not None:                 # the reference's walls object is an updatable (ICM_Compressible.cuh:226)
            if hasattr(self.walls, "updateSimulationTime"):
                self.updatables.append(self.walls)
            self._set_wall_velocities(0.0)
        self._initialize_fluid(par)
        if self.walls is not None:                 # setUpGhostCells (:418-422)
            check(self.lib.uammd_icmc_ghost_fill(self.h, current_stream()))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_icmc_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _initialize_fluid(self, par):
        given = [par.initialDensity, par.initialVelocityX, par.initialVelocityY, par.initialVelocityZ]
        if all(g is None for g in given):
            return
        nx, ny, nz = self.cells
        fields, pos = [], None
        for g in given:
            if g is None:
                fields.append(None)
                continue
            if callable(g):
                if pos is None:
                    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
                    to32 = lambda c, n, L: ((c.astype(np.float32) / np.float32(n) + np.float32(0.5)) * np.float32(L)).ravel()
                    pos = np.stack([to32(x, nx, self.boxSize[0]), to32(y, ny, self.boxSize[1]), to32(z, nz, self.boxSize[2])], 1)
                a = np.array([g(tuple(float(c) for c in r)) for r in pos], dtype=np.float32)
            else:
                a = np.ascontiguousarray(g, dtype=np.float32)
                if a.size != nx * ny * nz:
                    raise ValueError(f"[ICM_Compressible] an initial field of {a.size} values for {nx} x {ny} x {nz} cells")
            fields.append(torch.from_numpy(a.reshape(nz, ny, nx)).to(self.pd.device))
        self.setFluid(*fields)

    def addUpdatable(self, u):
        self.updatables.append(u)

    def setFluid(self, density=None, vx=None, vy=None, vz=None):
        """Replaces the given fields [nz, ny, nx] (None keeps one) and derives the momentum from density and velocity."""
        t = [None if a is None else a.to(device=self.pd.device, dtype=torch.float32).contiguous() for a in (density, vx, vy, vz)]
        if any(a is not None and a.numel() != self.cells[0] * self.cells[1] * self.cells[2] for a in t):
            raise ValueError("[ICM_Compressible] a fluid field of the wrong size")
        check(self.lib.uammd_icmc_set_fluid(self.h, *[_ptr(a) for a in t], current_stream()))

    def getGridSize(self):
        return list(self.cells)

    def _field(self, n=1):
        nx, ny, nz = self.cells
        return torch.empty((n, nz, ny, nx), dtype=torch.float32, device=self.pd.device)

    def getCurrentDensity(self):
        out = self._field()[0]
        check(self.lib.uammd_icmc_get_fluid(self.h, _ptr(out), None, None, current_stream()))
        return out

    def getCurrentVelocity(self, collocated=True):
        """[3, nz, ny, nx]: the velocity averaged to the cell centres (the reference's getCurrentVelocity), or the staggered field."""
        out = self._field(3)
        if collocated:
            check(self.lib.uammd_icmc_get_collocated_velocity(self.h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), current_stream()))
        else:
            v = (C.c_void_p * 3)(*[out[c].data_ptr() for c in range(3)])
            check(self.lib.uammd_icmc_get_fluid(self.h, None, C.byref(v), None, current_stream()))
        return out

    def getMomentum(self):
        out = self._field(3)
        g = (C.c_void_p * 3)(*[out[c].data_ptr() for c in range(3)])
        check(self.lib.uammd_icmc_get_fluid(self.h, None, None, C.byref(g), current_stream()))
        return out

    def get_noise(self, step):
        """The stochastic stress the integrator draws at `step`: [6, nz, ny, nx, 2] = (W_A, W_B) of xx, yy, zz, xy, xz, yz."""
        nx, ny, nz = self.cells
        out = torch.empty((6, nz, ny, nx, 2), dtype=torch.float32, device=self.pd.device)
        check(self.lib.uammd_icmc_get_noise(self.h, int(step), _ptr(out), current_stream()))
        return out

    def set_noise(self, noise):
        """Test hook: the following steps use these numbers ([6, nz, ny, nx, 2]) instead of drawing; None draws again."""
        if noise is not None:
            noise = noise.to(device=self.pd.device, dtype=torch.float32).contiguous()
            if noise.numel() != 12 * self.cells[0] * self.cells[1] * self.cells[2]:
                raise ValueError("[ICM_Compressible] the noise holds 12 numbers per cell")
        check(self.lib.uammd_icmc_set_noise(self.h, _ptr(noise), current_stream()))

    def _update_time(self, t):
        for u in self.updatables + self.interactors:
            u.updateSimulationTime(t)

    def forwardTime(self):
        pd, dt = self.pd, self.par.dt
        N = pd.N
        pos = _ptr(pd.getPos("readwrite")) if N > 0 else None
        check(self.lib.uammd_icmc_predictor(self.h, pos, N, current_stream()))
        self._update_time((self.steps + 0.5) * dt)         # computeCurrentFluidForcing, ICM_Compressible.cu:176-185
        force = None
        if N > 0:
            pd.getForce("write").zero_()                    # updateParticleForces, :153-161
            for it in self.interactors:
                it.sum(force=True)
            if self.interactors:
                force = _ptr(pd.getForce("read"))
        thirds = (1.0 / 3.0, 2.0 / 3.0, 1.0)
        if self.walls is None:
            check(self.lib.uammd_icmc_fluid_and_corrector(self.h, pos, force, N, current_stream()))
            for third in thirds:                            # callRungeKuttaSubStep, :88-90 (the host calls only order the callbacks)
                self._update_time((self.steps + third) * dt)
        else:                                               # the same step in pieces: each sub-stage's fills see the walls at its time
            st = current_stream()
            check(self.lib.uammd_icmc_fluid_begin(self.h, pos, force, N, st))
            for s, third in enumerate(thirds):              # callRungeKuttaSubStep, :83-93
                check(self.lib.uammd_icmc_substage(self.h, s, st))
                t = (self.steps + third) * dt
                self._update_time(t)
                self._set_wall_velocities(t)
                check(self.lib.uammd_icmc_ghost_fill(self.h, st))
                check(self.lib.uammd_icmc_substage_velocity(self.h, st))
                check(self.lib.uammd_icmc_ghost_fill(self.h, st))
            check(self.lib.uammd_icmc_fluid_end(self.h, pos, N, st))
        self.steps += 1

    def _set_wall_velocities(self, t):
        bottom, top = self.walls.velocities(t)
        b, u = (C.c_float * 2)(float(bottom[0]), float(bottom[1])), (C.c_float * 2)(float(top[0]), float(top[1]))
        check(self.lib.uammd_icmc_set_wall_velocities(self.h, C.byref(b), C.byref(u)))

    def getBottomGhostCells(self):
        """With walls: the bottom ghost plane as (density [ny, nx], velocity [3, ny, nx], momentum [3, ny, nx])."""
        nx, ny, nz = self.cells
        rho = torch.empty((ny, nx), dtype=torch.float32, device=self.pd.device)
        v, g = torch.empty((3, ny, nx), dtype=torch.float32, device=self.pd.device), torch.empty((3, ny, nx), dtype=torch.float32, device=self.pd.device)
        pv, pg = (C.c_void_p * 3)(*[v[c].data_ptr() for c in range(3)]), (C.c_void_p * 3)(*[g[c].data_ptr() for c in range(3)])
        check(self.lib.uammd_icmc_get_bottom_ghost(self.h, _ptr(rho), C.byref(pv), C.byref(pg), current_stream()))
        return rho, v, g


class Hydro:
    ICM = ICM
    ICM_Compressible = ICM_Compressible
