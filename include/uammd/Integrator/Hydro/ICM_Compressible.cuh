// Hydro::ICM_Compressible — same include path, class names and Parameters as the reference's src/Integrator/Hydro/ICM_Compressible.cuh.
// The compressible Inertial Coupling Method: particles advected by a fluctuating compressible fluid (density and momentum on a staggered
// grid, explicit three-stage Runge-Kutta), triply periodic or between two walls in z.  The solver is uammd_icmc_* of libuammd_hip; this header is
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
// Walls in z: ICM_Compressible_impl<Walls> with icm_compressible::MovingWalls or a class derived from it (a bottom and a top wall, each
// moving in its plane; override updateSimulationTime and call setVelocities there — an oscillating wall is five lines):
//
//   struct Oscillating : Hydro::icm_compressible::MovingWalls {
//     void updateSimulationTime(real t) override { setVelocities(make_real2(0.1 * cos(0.5 * t), 0), make_real2(0, 0)); }
//   };
//   using ICM = Hydro::ICM_Compressible_impl<Oscillating>;  par.walls = std::make_shared<Oscillating>();
//
// The ghost planes are filled by the library's built-in rule (uammd_hip.h: v_ghost = 2 u_wall - v_adj, ...), at the reference's places in
// the step and with the velocities the walls object holds then.  temperature > 0 is refused with walls.
//
// User-written walls (hipcc translation units only; device/ICM_Compressible.hip.hpp): any other Walls class whose isEnabled() is true,
// with the reference's members
//   __device__ void applyBoundaryConditionZBottom(FluidPointers fluid, int3 ghostCell, int3 n) const;      and ...ZTop(...)
// works as in the reference: the rule is called for every (i, j) of the ghost grid with ghostCell.z = 0 and n.z + 1, and the reference's
// index arithmetic x + (y + z (n.y + 2)) (n.x + 2) is valid for z in {0, 1} (bottom) and {n.z, n.z + 1} (top).  A rule may read the
// adjacent interior plane and write the ghost plane; WRITES TO THE INTERIOR PLANE ARE DROPPED.  The walls object is passed to the
// kernel by value.  Under a plain C++ compiler such a class is refused at compile time.
//
// Not here: other equations of state or windows, and a double-precision build.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "ICM_Compressible.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../../uammd.h"
#include <functional>
#include <memory>
#include <stdexcept>
#include <type_traits>
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

// Walls at the bottom and the top of the box, each moving in its plane with a velocity (u_x, u_y); host code.  The integrator reads
// the velocities before every ghost fill, so a derived class changes them in updateSimulationTime, which it hears with the four times of a
// step: (n + 1/2) dt, then (n + 1/3) dt, (n + 2/3) dt, (n + 1) dt, each of the last three before the fills of its Runge-Kutta sub-stage.
class MovingWalls : public ParameterUpdatable {
  real2 bottom = make_real2(0, 0), top = make_real2(0, 0);
public:
  MovingWalls() {}
  MovingWalls(real2 bottom, real2 top) : bottom(bottom), top(top) {}
  static constexpr bool isEnabled() { return true; }
  void setVelocities(real2 newBottom, real2 newTop) { bottom = newBottom; top = newTop; }
  real2 getBottomVelocity() const { return bottom; }
  real2 getTopVelocity() const { return top; }
};

// What a user's wall rule receives (the reference's FluidPointers, ICM_Compressible/utils.cuh): with this port the pointers address the
// packed wall planes of the library (uammd_hip.h), offset so that the reference's ghost-grid index lands in them
struct FluidPointers {
  real *density = nullptr, *velocityX = nullptr, *velocityY = nullptr, *velocityZ = nullptr;
  real *momentumX = nullptr, *momentumY = nullptr, *momentumZ = nullptr;
};

namespace walls_detail {
// Walls::isEnabled() as a constant, where it is one (the reference's own classes spell it as a non-static member: known = false)
template <class W, class = void> struct StaticEnabled : std::false_type { static constexpr bool known = false; };
template <class W>
struct StaticEnabled<W, decltype(void(std::integral_constant<bool, W::isEnabled()>{}))> : std::integral_constant<bool, W::isEnabled()> {
  static constexpr bool known = true;
};
}  // namespace walls_detail

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
}  // namespace Hydro
}  // namespace uammd
#if defined(__HIPCC__)
#include "../../device/ICM_Compressible.hip.hpp"
#endif
namespace uammd {
namespace Hydro {

template <class Walls> class ICM_Compressible_impl : public Integrator {
  static constexpr bool hasWalls = std::is_base_of<icm_compressible::MovingWalls, Walls>::value;  // the library's built-in rule
  using StaticEnabled = icm_compressible::walls_detail::StaticEnabled<Walls>;
#if defined(__HIPCC__)
  static constexpr bool userWalls = !hasWalls && !(StaticEnabled::known && !StaticEnabled::value);  // a rule of the user's, device code
#else
  static constexpr bool userWalls = false;
  static_assert(hasWalls || (StaticEnabled::known && !StaticEnabled::value),
                "Hydro::ICM_Compressible: walls are not supported, the solver is triply periodic "
                "(use icm_compressible::DefaultWalls or a Walls class whose isEnabled() is false)");
#endif
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
    walls = par.walls ? par.walls : std::make_shared<Walls>();
    wallMode = hasWalls ? UAMMD_ICMC_WALLS_BUILTIN
                        : (userWalls && enabledNow(walls.get(), std::integral_constant<bool, StaticEnabled::known>{}) ? UAMMD_ICMC_WALLS_EXTERNAL
                                                                                                                      : UAMMD_ICMC_WALLS_NONE);
    p.walls = wallMode;
    // checkInputValidity comes first in the reference (:293-311), so a refused parameter set draws nothing from the generator
    if (uammd_icmc_validate(&p) != 0) throw std::runtime_error(uammd_hip_last_error());
    p.seed = seed = (par.seed == 0) ? sys->rng().next32() : par.seed;
    int cd[3] = {0, 0, 0};
    if (uammd_icmc_create(&p, &h, cd) != 0) throw std::runtime_error(uammd_hip_last_error());
    cells = make_int3(cd[0], cd[1], cd[2]);
    boxSize = par.boxSize;
    this->addUpdatable(walls);
    if (wallMode == UAMMD_ICMC_WALLS_EXTERNAL) {  // initializeFluid and setUpGhostCells (:411-421) with the walls as they are now
      initializeFluid(par);
      fillGhostCells();
      detail::check(uammd_icmc_velocity_to_momentum(h, nullptr));
      fillGhostCells();
    } else {
      sendWallVelocities(walls.get());
      initializeFluid(par);
      fillGhostCells();
    }
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
    // the times the updatables hear after each Runge-Kutta sub-stage (ICM_Compressible.cu:51-68, :88-90)
    const real subStepTime[3] = {real(1.0 / 3.0), real(2.0 / 3.0), real(1)};
    if (wallMode != UAMMD_ICMC_WALLS_NONE) {
      forwardFluidWithWalls(N, subStepTime);
      steps++;
      return;
    }
    if (N > 0) {  // the forcing at q^{n+1/2}, the fluid to n + 1, q^{n+1} = q^n + dt/2 J^{n+1/2} (v^n + v^{n+1})
      auto pos = pd->getPos(access::gpu, access::readwrite);
      auto force = pd->getForce(access::gpu, access::read);
      detail::check(uammd_icmc_fluid_and_corrector(h, (float *)pos.raw(), interactors.empty() ? nullptr : (const float *)force.raw(), N, nullptr));
    } else {
      detail::check(uammd_icmc_fluid_and_corrector(h, nullptr, nullptr, 0, nullptr));
    }
    for (int s = 0; s < 3; ++s)
      for (auto &u : updatables) u->updateSimulationTime((steps + subStepTime[s]) * dt);
    steps++;
  }

  // the number of fluid cells per direction (without ghost cells; with walls the library keeps two ghost planes in z, which are not counted)
  int3 getGridSize() const { return cells; }

  // the fluid density, n.x n.y n.z values, cell (i, j, k) at i + (j + k n.y) n.x, in device memory
  uninitialized_cached_vector<real> getCurrentDensity() const {
    uninitialized_cached_vector<real> density(numberCells());
    detail::check(uammd_icmc_get_fluid(h, (float *)density.data().get(), nullptr, nullptr, nullptr));
    finished();
    return density;
  }

  // the fluid velocity interpolated to the cell centres, in device memory.  The first n.x n.y n.z entries of each component are the cells;
  // size() is the reference's ((n.x + 2)(n.y + 2)(n.z + 2), its ghost grid), the tail is zero.
  DataXYZ getCurrentVelocity() const {
    DataXYZ v((cells.x + 2) * (cells.y + 2) * (cells.z + 2));
    v.fillWithZero();
    detail::check(uammd_icmc_get_collocated_velocity(h, v.x(), v.y(), v.z(), nullptr));
    finished();
    return v;
  }

  // What the reference returns here is the first plane of its ghost grid: (n.x + 2)(n.y + 2) staggered velocities below the bottom of the
  // box, entry (i + 1) + (j + 1)(n.x + 2) for cell (i, j).  Without walls that plane is the periodic image of the top one, z = n.z - 1.
  // With walls it is the real ghost plane, as the wall rule wrote it (x and y ghost columns: periodic images, which is what the rule gives
  // there).
  DataXYZ getCurrentBottomGhostCellVelocity() const {
    if (wallMode != UAMMD_ICMC_WALLS_NONE) return bottomGhostPlane();
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
  int wallMode = UAMMD_ICMC_WALLS_NONE;
  std::shared_ptr<DensityToPressure> densityToPressure;
  int steps = 0;
  real dt;
  uint seed = 1234;

  // The reference's programs read what the getters return from the host through raw pointers (thrust::copy on DataXYZ::x(), walltest.cu:
  // 140-145), with nothing that waits for the device in between: the getters return finished arrays.
  static void finished() { detail::hipCheck(hipStreamSynchronize(nullptr), "hipStreamSynchronize"); }

  size_t numberCells() const { return (size_t)cells.x * cells.y * cells.z; }

  void sendWallVelocities(const icm_compressible::MovingWalls *w) {
    const real2 b = w->getBottomVelocity(), t = w->getTopVelocity();
    const float fb[2] = {(float)b.x, (float)b.y}, ft[2] = {(float)t.x, (float)t.y};
    detail::check(uammd_icmc_set_wall_velocities(h, fb, ft));
  }
  void sendWallVelocities(const void *) {}  // no walls

  template <class W> static bool enabledNow(W *, std::true_type) { return StaticEnabled::value; }
  template <class W> static bool enabledNow(W *w, std::false_type) { return w->isEnabled(); }

  // fillGhostCells (ICM_Compressible.cu:97-102): the built-in rule with the velocities the walls hold now, or the user's rule on the
  // packed planes
  void fillGhostCells() {
    if (wallMode == UAMMD_ICMC_WALLS_BUILTIN) {
      sendWallVelocities(walls.get());
      detail::check(uammd_icmc_ghost_fill(h, nullptr));
    } else if (wallMode == UAMMD_ICMC_WALLS_EXTERNAL) {
      userFill(std::integral_constant<bool, userWalls>{});
    }
  }
  void userFill(std::false_type) {}
  void userFill(std::true_type) {
#if defined(__HIPCC__)
    float *planes = nullptr;
    detail::check(uammd_icmc_wall_planes_get(h, &planes, nullptr));
    icm_compressible::callUserWallFill(planes, *walls, cells);
    detail::check(uammd_icmc_wall_planes_put(h, nullptr));
#endif
  }

  // callRungeKuttaSubStep (ICM_Compressible.cu:70-95) through the pieces of the library's step: momentum and density, the sub-step time,
  // ghost fill, velocity, ghost fill.  The particle arrays are held only around the two pieces that use them: the updatables that run
  // in between may ask for them, as they may in the reference.
  void forwardFluidWithWalls(int N, const real *subStepTime) {
    if (N > 0) {
      auto pos = pd->getPos(access::gpu, access::readwrite);
      auto force = pd->getForce(access::gpu, access::read);
      detail::check(uammd_icmc_fluid_begin(h, (const float *)pos.raw(), interactors.empty() ? nullptr : (const float *)force.raw(), N, nullptr));
    } else {
      detail::check(uammd_icmc_fluid_begin(h, nullptr, nullptr, 0, nullptr));
    }
    for (int s = 0; s < 3; ++s) {
      detail::check(uammd_icmc_substage(h, s, nullptr));
      for (auto &u : updatables) u->updateSimulationTime((steps + subStepTime[s]) * dt);
      fillGhostCells();
      detail::check(uammd_icmc_substage_velocity(h, nullptr));
      fillGhostCells();
    }
    if (N > 0) {
      auto pos = pd->getPos(access::gpu, access::readwrite);
      detail::check(uammd_icmc_fluid_end(h, (float *)pos.raw(), N, nullptr));
    } else {
      detail::check(uammd_icmc_fluid_end(h, nullptr, 0, nullptr));
    }
  }

  DataXYZ bottomGhostPlane() const {
    const size_t nxy = (size_t)cells.x * cells.y;
    DataXYZ v((int)nxy);
    float *src[3] = {v.x(), v.y(), v.z()};
    detail::check(uammd_icmc_get_bottom_ghost(h, nullptr, src, nullptr, nullptr));
    const int gx = cells.x + 2, gy = cells.y + 2;
    DataXYZ plane(gx * gy);
    float *dst[3] = {plane.x(), plane.y(), plane.z()};
    std::vector<real> in(nxy), out((size_t)gx * gy);
    for (int c = 0; c < 3; ++c) {
      detail::hipCheck(hipMemcpy(in.data(), src[c], sizeof(real) * nxy, hipMemcpyDeviceToHost), "hipMemcpy");
      for (int j = 0; j < gy; ++j)
        for (int i = 0; i < gx; ++i)
          out[i + (size_t)j * gx] = in[(i - 1 + cells.x) % cells.x + (size_t)((j - 1 + cells.y) % cells.y) * cells.x];
      detail::hipCheck(hipMemcpy(dst[c], out.data(), sizeof(real) * out.size(), hipMemcpyHostToDevice), "hipMemcpy");
    }
    return plane;
  }

  DataXYZ staggered(bool momentum) const {
    DataXYZ v((int)numberCells());
    float *p[3] = {v.x(), v.y(), v.z()};
    detail::check(uammd_icmc_get_fluid(h, nullptr, momentum ? nullptr : p, momentum ? p : nullptr, nullptr));
    finished();
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
