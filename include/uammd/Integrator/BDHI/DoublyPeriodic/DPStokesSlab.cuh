// Integrator/BDHI/DoublyPeriodic/DPStokesSlab.cuh — the doubly periodic Stokes mobility and its integrator: particles in a fluid that is
// periodic in x and y and open, bounded by a no-slip wall at z = -H/2, or confined in a slit, z in [-H/2, H/2].  Same include path, names
// and parameters as the reference's header; plain C++14 over the C ABI (uammd_dpstokes_*, csrc/dpstokes.hip), both
// precisions: -DDOUBLE_PRECISION routes to the _f64 calls.  Torques (the dipole kernel: w_d, beta_d, alpha_d) are not implemented:
// Mdot with a non-null torque pointer throws.
#pragma once
#include "../../../uammd.h"
#include <cmath>
#include <stdexcept>
#include <utility>
namespace uammd {
namespace DPStokesSlab_ns {
template <class T> using cached_vector = uninitialized_cached_vector<T>;   // StokesSlab/utils.cuh
enum class WallMode { bottom, slit, none };                                 // StokesSlab/utils.cuh

namespace detail {
template <class T> struct StrideOf;   // positions and forces are rows of 3 or 4 reals
template <> struct StrideOf<real3> { static constexpr int value = 3; };
template <> struct StrideOf<real4> { static constexpr int value = 4; };
template <class Ptr> struct Pointee;
template <class T> struct Pointee<T *> { using type = typename std::remove_cv<T>::type; };
template <class Ptr> constexpr int strideOf() { return StrideOf<typename Pointee<Ptr>::type>::value; }
inline int modeIndex(WallMode m) { return m == WallMode::none ? 0 : (m == WallMode::bottom ? 1 : 2); }
#if defined(DOUBLE_PRECISION)
constexpr int doublePrecision = 1;
#else
constexpr int doublePrecision = 0;
#endif
inline void throwLast() {
  const std::string msg = uammd_hip_last_error();
  if (msg.find("not implemented") != std::string::npos) throw std::runtime_error("Operation not implemented: " + msg);
  throw std::runtime_error(msg.find("[DPStokes]") == 0 ? "[DPStokes] Invalid argument: " + msg : msg);   // initialization.cu:12-26
}
}  // namespace detail

class DPStokes {
public:
  using WallMode = DPStokesSlab_ns::WallMode;
  struct Parameters {   // DPStokesSlab.cuh:149-174
    int nx, ny;
    int nz = -1;        // -1: pi H / min(hx, hy)
    real viscosity;
    real Lx, Ly;
    real H;             // the slab is z in [-H/2, H/2]
    real w;             // support of the window in cells
    real w_d;           // (torque kernel: accepted, not read)
    real3 beta = {-1.0, -1.0, -1.0};    // width of the window per axis; y and z default to x
    real3 beta_d = {-1.0, -1.0, -1.0};  // (torque kernel: accepted, not read)
    real alpha = -1;    // half support of the window in cells, typically w / 2
    real alpha_d = -1;  // (torque kernel: accepted, not read)
    WallMode mode = WallMode::none;
  };
  static uammd_dpstokes_parameters toC(const Parameters &par) {
    uammd_dpstokes_parameters p{};
    p.nx = par.nx; p.ny = par.ny; p.nz = par.nz;
    p.viscosity = par.viscosity; p.Lx = par.Lx; p.Ly = par.Ly; p.H = par.H;
    p.w = par.w; p.beta[0] = par.beta.x; p.beta[1] = par.beta.y; p.beta[2] = par.beta.z; p.alpha = par.alpha;
    p.mode = detail::modeIndex(par.mode);
    return p;
  }

  DPStokes(Parameters par) {
    const uammd_dpstokes_parameters p = toC(par);
    if (uammd_dpstokes_create(&p, detail::doublePrecision, &h, &info) != 0) detail::throwLast();
  }
  DPStokes(const DPStokes &) = delete;
  ~DPStokes() { if (owned) uammd_dpstokes_destroy(h); }

  // the velocities M F of particles at pos (real3* or real4*) under forces (real3* or real4*), device pointers
  template <class PosIterator, class ForceIterator>
  cached_vector<real3> Mdot(PosIterator pos, ForceIterator forces, int numberParticles, hipStream_t st = 0) {
    return Mdot(pos, forces, (real4 *)nullptr, numberParticles, st).first;
  }
  template <class PosIterator, class ForceIterator, class TorqueIterator>
  std::pair<cached_vector<real3>, cached_vector<real3>> Mdot(PosIterator pos, ForceIterator forces, TorqueIterator torques, int numberParticles,
                                                            hipStream_t st) {
    if (torques) throw std::runtime_error("[DPStokes] Torques are not implemented (the dipole kernel is out of scope)");
    cached_vector<real3> mf(numberParticles);
    run(pos, detail::strideOf<PosIterator>(), forces, detail::strideOf<ForceIterator>(), numberParticles, mf.data().get(), st);
    return {std::move(mf), cached_vector<real3>()};
  }
  // the plane average of u (direction 0) or v (1) at the nz planes, plane 0 at the top
  template <class PosIterator, class ForceIterator>
  std::vector<double> computeAverageVelocity(PosIterator pos, ForceIterator forces, int numberParticles, int direction = 0, hipStream_t st = 0) {
    if (direction != 0 && direction != 1) throw std::runtime_error("[DPStokesSlab] Can only average in direction X (0) or Y (1)");
    std::vector<double> out(info.cells[2], 0.0);
#if defined(DOUBLE_PRECISION)
    const int e = uammd_dpstokes_average_velocity_f64(h, (const double *)&*pos, detail::strideOf<PosIterator>(), (const double *)&*forces,
                                                      detail::strideOf<ForceIterator>(), numberParticles, direction, out.data(), (void *)st);
#else
    const int e = uammd_dpstokes_average_velocity(h, (const float *)&*pos, detail::strideOf<PosIterator>(), (const float *)&*forces,
                                                  detail::strideOf<ForceIterator>(), numberParticles, direction, out.data(), (void *)st);
#endif
    if (e) detail::throwLast();
    return out;
  }
  int3 getCells() const { return make_int3(info.cells[0], info.cells[1], info.cells[2]); }
  int getSupport() const { return info.support; }
  int getNumberOutside() {
    int n = 0;
    uammd::detail::check(uammd_dpstokes_outside_count(h, &n));
    return n;
  }
  void setOption(const char *name, int value) { uammd::detail::check(uammd_dpstokes_set_option(h, name, value)); }

private:
  friend class DPStokesIntegrator;
  DPStokes(uammd_dpstokes *borrowed, const Parameters &par) : h(borrowed), owned(false) {   // the integrator's solver
    const uammd_dpstokes_parameters p = toC(par);
    if (uammd_dpstokes_create(&p, detail::doublePrecision, nullptr, &info) != 0) detail::throwLast();
  }
  uammd_dpstokes *h = nullptr;
  bool owned = true;
  uammd_dpstokes_info info{};
  template <class P, class F> void run(P pos, int ps, F forces, int fs, int n, real3 *mf, hipStream_t st) {
#if defined(DOUBLE_PRECISION)
    const int e = uammd_dpstokes_mdot_f64(h, (const double *)&*pos, ps, (const double *)&*forces, fs, nullptr, n, (double *)mf, (void *)st);
#else
    const int e = uammd_dpstokes_mdot(h, (const float *)&*pos, ps, (const float *)&*forces, fs, nullptr, n, (float *)mf, (void *)st);
#endif
    if (e) detail::throwLast();
  }
};

// Brownian dynamics with the DPStokes mobility: pos += dt M F + dt sqrt(2 T / dt) M^(1/2) W + T dt div M, the fluctuations by Lanczos, the
// drift by random finite differences (DPStokesSlab.cuh:424-583)
class DPStokesIntegrator : public Integrator {
public:
  template <class T> using cached_vector = DPStokesSlab_ns::cached_vector<T>;
  struct Parameters : DPStokes::Parameters {   // DPStokesSlab.cuh:499-505
    real temperature = 0;
    bool useLeimkuhler = false;   // average the noise with the previous step's; Euler-Maruyama otherwise
    real dt;
    real tolerance = 1e-7;        // of the Lanczos iteration
    real deltaRFD = -1;           // the random-finite-difference step; <= 0: the reference's 1e-6, which single precision cannot resolve:
                                  // there temperature > 0 needs a value here
  };

  DPStokesIntegrator(shared_ptr<ParticleData> pd, Parameters par) : Integrator(pd, "DPStokes"), par(par) {
    uammd_dpstokes_integrator_parameters ip{};
    ip.temperature = par.temperature; ip.dt = par.dt; ip.tolerance = par.tolerance; ip.deltaRFD = par.deltaRFD;
    ip.useLeimkuhler = par.useLeimkuhler ? 1 : 0;
    ip.seed = pd->getSystem()->rng().next32();      // DPStokesSlab.cuh:520-521
    ip.seedRFD = pd->getSystem()->rng().next32();
    const uammd_dpstokes_parameters p = DPStokes::toC(par);
    if (uammd_dpstokes_integrator_create(&p, &ip, detail::doublePrecision, &h) != 0) detail::throwLast();
    dpstokes.reset(new DPStokes(uammd_dpstokes_integrator_solver(h), par));
    sys->log<System::MESSAGE>("[DPStokes] dt %g", (double)par.dt);
    sys->log<System::MESSAGE>("[DPStokes] temperature: %g", (double)par.temperature);
    sys->log<System::MESSAGE>("[DPStokes] tolerance: %g", (double)par.tolerance);
  }
  DPStokesIntegrator(const DPStokesIntegrator &) = delete;
  ~DPStokesIntegrator() {
    dpstokes.reset();
    uammd_dpstokes_integrator_destroy(h);
  }

  void forwardTime() override {
    if (steps == 0) setUpInteractors();
    resetGroupForces(0);
    for (auto &i : interactors) {
      i->updateSimulationTime(par.dt * steps);
      Interactor::Computables comp;
      comp.force = true;
      i->sum(comp, 0);
    }
    if (pd->isTorqueAllocated()) {
      sys->log<System::EXCEPTION>("[DPStokes] Torques are not yet implemented");
      throw std::runtime_error("Operation not implemented");
    }
    const int N = pd->getNumParticles();
    auto pos = pd->getPos(access::gpu, access::readwrite);
    auto force = pd->getForce(access::gpu, access::read);
#if defined(DOUBLE_PRECISION)
    const int e = uammd_dpstokes_integrator_step_f64(h, (double *)pos.raw(), 4, (const double *)force.raw(), 4, N, nullptr);
#else
    const int e = uammd_dpstokes_integrator_step(h, (float *)pos.raw(), 4, (const float *)force.raw(), 4, N, nullptr);
#endif
    if (e) detail::throwLast();
    steps++;
  }
  shared_ptr<DPStokes> getSolver() { return dpstokes; }

private:
  Parameters par;
  uammd_dpstokes_integrator *h = nullptr;
  shared_ptr<DPStokes> dpstokes;
  int steps = 0;
  void setUpInteractors() {   // DPStokesSlab.cuh:569-578
    Box box(make_real3(par.Lx, par.Ly, par.H));
    box.setPeriodicity(1, 1, 0);
    for (auto &i : interactors) {
      i->updateBox(box);
      i->updateTimeStep(par.dt);
      i->updateTemperature(par.temperature);
      i->updateViscosity(par.viscosity);
    }
  }
};
}  // namespace DPStokesSlab_ns
}  // namespace uammd
