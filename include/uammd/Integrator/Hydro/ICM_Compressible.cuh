// Hydro::ICM_Compressible — same include path, class names and Parameters as the reference's src/Integrator/Hydro/ICM_Compressible.cuh.
// The compressible Inertial Coupling Method: particles advected by a fluctuating compressible fluid (density and momentum on a staggered
// grid, explicit three-stage Runge-Kutta), triply periodic.  The solver is uammd_icmc_* of libuammd_hip; this header is
// host code only and compiles with a plain C++ compiler.
//
//   using ICM = Hydro::ICM_Compressible;
//   ICM::Parameters par;
//   par.shearViscosity = 1.0; par.bulkViscosity = 1.0; par.speedOfSound = 16; par.temperature = 0; par.dt = 0.1;
//   par.boxSize = make_real3(32, 32, 32);
//   par.cellDim = make_int3(32, 32, 32);     // or par.hydrodynamicRadius = 1 (cells = int(L / (0.91 a))): exactly one of the two
//   par.initialVelocityX = [](real3 r) { return 0.01 * sin(2 * M_PI * r.y / 32); };      // optional, as initialDensity / VelocityY / Z
//   auto icm = std::make_shared<ICM>(pd, par);
//   icm->addInteractor(...); icm->forwardTime();
//
// Not here: walls (a Walls class whose isEnabled() is true is refused at compile time — its boundary conditions are device code of the
// user's), other equations of state or windows, and a double-precision build.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "ICM_Compressible.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../../uammd.h"
#include <functional>
#include <memory>
#include <stdexcept>
#include <vector>

namespace uammd {
namespace Hydro {
namespace icm_compressible {

// The equation of state pi = c^2 rho (the solver's only one: the member is what the constructor passes on)
struct DensityToPressure {
  real isothermalSpeedOfSound = 1.0;
  real operator()(real density) const { return isothermalSpeedOfSound * isothermalSpeedOfSound * density; }
};

// No walls: periodic in the three directions.  (A ParameterUpdatable as in the reference: it hears the sub-step times.)
class DefaultWalls : public ParameterUpdatable {
public:
  static constexpr bool isEnabled() { return false; }
};

// three device arrays of one size
struct DataXYZ {
  uninitialized_cached_vector<real> m_x, m_y, m_z;
  DataXYZ() : DataXYZ(0) {}
  DataXYZ(int size) { resize(size); }
  void resize(int newSize) { m_x.resize(newSize); m_y.resize(newSize); m_z.resize(newSize); }
  void fillWithZero() const {
    if (!size()) return;
    detail::check(uammd_fill_zero(x(), sizeof(real) * size(), nullptr));
    detail::check(uammd_fill_zero(y(), sizeof(real) * size(), nullptr));
    detail::check(uammd_fill_zero(z(), sizeof(real) * size(), nullptr));
  }
  using Iterator = real *;
  Iterator x() const { return const_cast<real *>(m_x.data().get()); }
  Iterator y() const { return const_cast<real *>(m_y.data().get()); }
  Iterator z() const { return const_cast<real *>(m_z.data().get()); }
  void swap(DataXYZ &o) { m_x.swap(o.m_x); m_y.swap(o.m_y); m_z.swap(o.m_z); }
  void clear() { m_x.clear(); m_y.clear(); m_z.clear(); }
  size_t size() const { return m_x.size(); }
};

// (cell / n + 0.5) L: where the reference evaluates the initial fields (ICM_Compressible.cuh:176-179)
inline real3 cell2CenterPos(int3 cell, int3 n, real3 L) {
  return make_real3((real(cell.x) / real(n.x) + real(0.5)) * L.x, (real(cell.y) / real(n.y) + real(0.5)) * L.y,
                    (real(cell.z) / real(n.z) + real(0.5)) * L.z);
}
}  // namespace icm_compressible

template <class Walls> class ICM_Compressible_impl : public Integrator {
  static_assert(!Walls::isEnabled(), "Hydro::ICM_Compressible: walls are not supported, the solver is triply periodic "
                                     "(use icm_compressible::DefaultWalls or a Walls class whose isEnabled() is false)");
public:
  using DataXYZ = icm_compressible::DataXYZ;
  using DensityToPressure = icm_compressible::DensityToPressure;

  struct Parameters {
    real shearViscosity = -1;
    real bulkViscosity = -1;
    real speedOfSound = -1;  // for the equation of state
    real temperature = 0;
    real dt = -1;
    real3 boxSize = make_real3(0, 0, 0);
    int3 cellDim = make_int3(-1, -1, -1);  // exactly one of cellDim and hydrodynamicRadius (the reference leaves this member uninitialised)
    real hydrodynamicRadius = -1;
    uint seed = 0;  // 0 takes a value from the System's generator
    std::function<real(real3)> initialDensity;
    std::function<real(real3)> initialVelocityX;
    std::function<real(real3)> initialVelocityY;
    std::function<real(real3)> initialVelocityZ;
    std::shared_ptr<Walls> walls;
  };

  ICM_Compressible_impl(std::shared_ptr<ParticleData> pd, Parameters par) : Integrator(pd, "ICM::Compressible"), dt(par.dt) {
    densityToPressure = std::make_shared<DensityToPressure>();
    densityToPressure->isothermalSpeedOfSound = par.speedOfSound;
    uammd_icmc_parameters p{};
    p.boxSize[0] = par.boxSize.x; p.boxSize[1] = par.boxSize.y; p.boxSize[2] = par.boxSize.z;
    p.cells[0] = par.cellDim.x; p.cells[1] = par.cellDim.y; p.cells[2] = par.cellDim.z;
    p.shearViscosity = par.shearViscosity; p.bulkViscosity = par.bulkViscosity; p.speedOfSound = par.speedOfSound;
    p.temperature = par.temperature; p.dt = par.dt; p.hydrodynamicRadius = par.hydrodynamicRadius;
    // checkInputValidity comes first in the reference (:293-311), so a refused parameter set draws nothing from the generator
    if (uammd_icmc_validate(&p) != 0) throw std::runtime_error(uammd_hip_last_error());
    p.seed = seed = (par.seed == 0) ? sys->rng().next32() : par.seed;
    int cd[3] = {0, 0, 0};
    if (uammd_icmc_create(&p, &h, cd) != 0) throw std::runtime_error(uammd_hip_last_error());
    cells = make_int3(cd[0], cd[1], cd[2]);
    boxSize = par.boxSize;
    walls = par.walls ? par.walls : std::make_shared<Walls>();
    this->addUpdatable(walls);
    initializeFluid(par);
    System::log<System::MESSAGE>("[ICM_Compressible] dt: %g, shear viscosity: %g, bulk viscosity: %g, isothermal speed of sound: %g, temperature: %g",
                                 (double)par.dt, (double)par.shearViscosity, (double)par.bulkViscosity, (double)par.speedOfSound, (double)par.temperature);
    System::log<System::MESSAGE>("[ICM_Compressible] Box size: %g %g %g, fluid cells: %d %d %d, seed: %u", (double)par.boxSize.x,
                                 (double)par.boxSize.y, (double)par.boxSize.z, cells.x, cells.y, cells.z, seed);
  }
  ICM_Compressible_impl(const ICM_Compressible_impl &) = delete;
  ~ICM_Compressible_impl() { uammd_icmc_destroy(h); }

  void forwardTime() override {
    const int N = groupSize();
    Interactor::Computables c; c.force = true;
    if (N > 0) {  // q^{n+1/2} = q^n + dt/2 J^n v^n
      auto pos = pd->getPos(access::gpu, access::readwrite);
      detail::check(uammd_icmc_predictor(h, (float *)pos.raw(), N, nullptr));
    }
    for (auto &u : updatables) u->updateSimulationTime((steps + 0.5) * dt);
    if (pd->getNumParticles() > 0) {
      auto force = pd->getForce(access::gpu, access::write);
      detail::check(uammd_fill_zero(force.raw(), sizeof(real4) * force.size(), nullptr));
    }
    for (auto &f : interactors) f->sum(c, 0);
    if (N > 0) {  // the forcing at q^{n+1/2}, the fluid to n + 1, q^{n+1} = q^n + dt/2 J^{n+1/2} (v^n + v^{n+1})
      auto pos = pd->getPos(access::gpu, access::readwrite);
      auto force = pd->getForce(access::gpu, access::read);
      detail::check(uammd_icmc_fluid_and_corrector(h, (float *)pos.raw(), interactors.empty() ? nullptr : (const float *)force.raw(), N, nullptr));
    } else {
      detail::check(uammd_icmc_fluid_and_corrector(h, nullptr, nullptr, 0, nullptr));
    }
    // the times the updatables hear after each Runge-Kutta sub-stage (ICM_Compressible.cu:51-68, :88-90)
    const real subStepTime[3] = {real(1.0 / 3.0), real(2.0 / 3.0), real(1)};
    for (int s = 0; s < 3; ++s)
      for (auto &u : updatables) u->updateSimulationTime((steps + subStepTime[s]) * dt);
    steps++;
  }

  // the number of fluid cells per direction (without ghost cells: there are none)
  int3 getGridSize() const { return cells; }

  // the fluid density, n.x n.y n.z values, cell (i, j, k) at i + (j + k n.y) n.x, in device memory
  uninitialized_cached_vector<real> getCurrentDensity() const {
    uninitialized_cached_vector<real> density(numberCells());
    detail::check(uammd_icmc_get_fluid(h, (float *)density.data().get(), nullptr, nullptr, nullptr));
    return density;
  }

  // the fluid velocity interpolated to the cell centres, in device memory.  The first n.x n.y n.z entries of each component are the cells;
  // size() is the reference's ((n.x + 2)(n.y + 2)(n.z + 2), its ghost grid), the tail is zero.
  DataXYZ getCurrentVelocity() const {
    DataXYZ v((cells.x + 2) * (cells.y + 2) * (cells.z + 2));
    v.fillWithZero();
    detail::check(uammd_icmc_get_collocated_velocity(h, v.x(), v.y(), v.z(), nullptr));
    return v;
  }

  // What the reference returns here is the first plane of its ghost grid: (n.x + 2)(n.y + 2) staggered velocities below the bottom of the
  // box, entry (i + 1) + (j + 1)(n.x + 2) for cell (i, j).  Without walls that plane is the periodic image of the top one, z = n.z - 1.
  DataXYZ getCurrentBottomGhostCellVelocity() const {
    const size_t nc = numberCells();
    DataXYZ v((int)nc);
    float *src[3] = {v.x(), v.y(), v.z()};
    detail::check(uammd_icmc_get_fluid(h, nullptr, src, nullptr, nullptr));
    const int gx = cells.x + 2, gy = cells.y + 2;
    DataXYZ plane(gx * gy);
    float *dst[3] = {plane.x(), plane.y(), plane.z()};
    std::vector<real> top((size_t)cells.x * cells.y), out((size_t)gx * gy);
    for (int c = 0; c < 3; ++c) {
      detail::hipCheck(hipMemcpy(top.data(), src[c] + (size_t)(cells.z - 1) * cells.x * cells.y, sizeof(real) * top.size(), hipMemcpyDeviceToHost), "hipMemcpy");
      for (int j = 0; j < gy; ++j)
        for (int i = 0; i < gx; ++i)
          out[i + (size_t)j * gx] = top[(i - 1 + cells.x) % cells.x + (size_t)((j - 1 + cells.y) % cells.y) * cells.x];
      detail::hipCheck(hipMemcpy(dst[c], out.data(), sizeof(real) * out.size(), hipMemcpyHostToDevice), "hipMemcpy");
    }
    return plane;
  }

  // the staggered fields as the solver keeps them (no reference counterpart): component a of cell i lies at r_i + h_a / 2
  DataXYZ getCurrentStaggeredVelocity() const { return staggered(false); }
  DataXYZ getCurrentMomentum() const { return staggered(true); }

private:
  uammd_icmc *h = nullptr;
  int3 cells = make_int3(0, 0, 0);
  real3 boxSize;
  std::shared_ptr<Walls> walls;
  std::shared_ptr<DensityToPressure> densityToPressure;
  int steps = 0;
  real dt;
  uint seed = 1234;

  size_t numberCells() const { return (size_t)cells.x * cells.y * cells.z; }

  DataXYZ staggered(bool momentum) const {
    DataXYZ v((int)numberCells());
    float *p[3] = {v.x(), v.y(), v.z()};
    detail::check(uammd_icmc_get_fluid(h, nullptr, momentum ? nullptr : p, momentum ? p : nullptr, nullptr));
    return v;
  }

  // initializeFluid (:374-414): rho = 1, v = 0 unless a function is given; the functions run on the host at (cell / n + 0.5) L
  void initializeFluid(const Parameters &par) {
    const std::function<real(real3)> *fn[4] = {&par.initialDensity, &par.initialVelocityX, &par.initialVelocityY, &par.initialVelocityZ};
    if (!*fn[0] && !*fn[1] && !*fn[2] && !*fn[3]) return;
    const size_t nc = numberCells();
    detail::DeviceArray<real> d[4];
    std::vector<real> host(nc);
    for (int k = 0; k < 4; ++k) {
      if (!*fn[k]) continue;
      for (int z = 0; z < cells.z; ++z)
        for (int y = 0; y < cells.y; ++y)
          for (int x = 0; x < cells.x; ++x)
            host[x + (size_t)cells.x * (y + (size_t)cells.y * z)] = (*fn[k])(icm_compressible::cell2CenterPos(make_int3(x, y, z), cells, boxSize));
      d[k].resize(nc);
      detail::hipCheck(hipMemcpy(d[k].d, host.data(), sizeof(real) * nc, hipMemcpyHostToDevice), "hipMemcpy");
    }
    detail::check(uammd_icmc_set_fluid(h, d[0].d, d[1].d, d[2].d, d[3].d, nullptr));
    detail::hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
};

using ICM_Compressible = ICM_Compressible_impl<icm_compressible::DefaultWalls>;
}  // namespace Hydro
}  // namespace uammd
