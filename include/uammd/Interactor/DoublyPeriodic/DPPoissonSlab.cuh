// Interactor/DoublyPeriodic/DPPoissonSlab.cuh — doubly periodic electrostatics in a slab: charges of Gaussian width gw between two walls
// at z = +-H/2, periodic in x and y, each wall a dielectric jump or (infinite permittivity) a metal.  Same include path and class as the
// reference's src/Interactor/DoublyPeriodic/DPPoissonSlab.cuh; plain C++14 over the C ABI (uammd_dppoisson_*, csrc/dppoisson.hip,
// DESIGN.md 17), both precisions: -DDOUBLE_PRECISION routes to the _f64 calls.  The triply periodic quadrupole test of the reference
// includes this path too and overloads getL on Parameters (test/Potentials/Poisson/common/quadrupole_test_base.cuh:4,45-50).
#pragma once
#include "../../uammd.h"
#include <array>
#include <cmath>
// (not used here: the reference's header of this name brings them in, and its example examples/interaction_modules/DoublyPeriodicPoisson.cu
// calls std::setprecision and opens a std::ofstream without including <iomanip> itself — it does not compile without them)
#include <fstream>
#include <iomanip>
#include <numeric>
#include <complex>
#include <stdexcept>
namespace uammd {
namespace DPPoissonSlab_ns {
struct Permitivity { real top = 1, bottom = 1, inside = 1; };
// Surface charge density of each wall — or, where the wall is metallic, its potential (PoissonSlab/utils.cuh:20-26)
class SurfaceValueDispatch {
public:
  virtual ~SurfaceValueDispatch() = default;
  virtual real top(real x, real y) { return 0; }
  virtual real bottom(real x, real y) { return 0; }
};
}  // namespace DPPoissonSlab_ns

class DPPoissonSlab : public Interactor {
public:
  using Permitivity = DPPoissonSlab_ns::Permitivity;
  using SurfaceValueDispatch = DPPoissonSlab_ns::SurfaceValueDispatch;
  struct Parameters {   // DPPoissonSlab.cuh:21-38
    real upsampling = 1.2;
    real2 Lxy = real2();
    int Nxy = -1;
    real H = 0;
    Permitivity permitivity;
    real tolerance = 1e-4;
    real gw = -1;
    int support = 12;   // at most 16 nodes per axis here (the gather keeps ceil(support^2 / 64) <= 4 columns per lane); the reference has no limit
    real numberStandardDeviations = 4;
    real split = -1;
    std::shared_ptr<SurfaceValueDispatch> surfaceValues = std::make_shared<SurfaceValueDispatch>();
    bool printK0Mode = false;  // accepted and not read: the k = 0 column is kept on every call, getK0Mode() always works
  };
  using complex4 = std::array<std::complex<real>, 4>;  // (Ex, Ey, Ez, phi) of one Chebyshev coefficient

  DPPoissonSlab(shared_ptr<ParticleGroup> pg, Parameters par) : Interactor(pg, "IBM::DPPoissonSlab") {
    uammd_dppoisson_parameters p{};
    p.Lxy[0] = par.Lxy.x; p.Lxy[1] = par.Lxy.y;
    p.H = par.H; p.gw = par.gw; p.split = par.split; p.Nxy = par.Nxy;
    p.permitivity[0] = par.permitivity.top; p.permitivity[1] = par.permitivity.bottom; p.permitivity[2] = par.permitivity.inside;
    p.tolerance = par.tolerance; p.upsampling = par.upsampling; p.support = par.support;
    p.numberStandardDeviations = par.numberStandardDeviations;
#if defined(DOUBLE_PRECISION)
    const int doublePrecision = 1;
#else
    const int doublePrecision = 0;
#endif
    if (uammd_dppoisson_create(&p, doublePrecision, &h, &info) != 0) {
      const std::string msg = uammd_hip_last_error();
      // initialization.cu:15-57, FarField.cuh:43-51, NearField.cuh:79-88 throw std::invalid_argument; initialization.cu:78-83 a runtime_error
      if (msg.find("Bottom metallic wall") != std::string::npos) throw std::runtime_error(msg);
      if (msg.find("Missing input") == 0 || msg.find("Invalid input") == 0 || msg.find("Invalid splitting") == 0 ||
          msg.find("[DPPoissonSlab]") == 0)
        throw std::invalid_argument(msg);
      throw std::runtime_error(msg);
    }
    setUpSurfaceValues(par);
  }
  DPPoissonSlab(shared_ptr<ParticleData> pd, Parameters par) : DPPoissonSlab(std::make_shared<ParticleGroup>(pd, "All"), par) {}
  DPPoissonSlab(const DPPoissonSlab &) = delete;
  ~DPPoissonSlab() { uammd_dppoisson_destroy(h); }

  // far field, then near field: both always add q E to the forces and q phi to the energies (DPPoissonSlab.cuh:47-55)
  void sum(Computables comp, hipStream_t st = 0) override {
    if (comp.virial) throw std::runtime_error("[Poisson] not implemented");
    run(nullptr, st);
  }
  // (Ex, Ey, Ez, phi) at the particles; like the reference's call it also adds to the forces and the energies
  std::vector<real4> computeFieldPotentialAtParticles() {
    const int N = numberParticles();
    detail::DeviceArray<real4> fp(N);
    if (N > 0) detail::check(uammd_fill_zero(fp.d, sizeof(real4) * (size_t)N, nullptr));
    run(fp.d, nullptr);
    std::vector<real4> out(N);
    if (N > 0) detail::hipCheck(hipMemcpy(out.data(), fp.d, sizeof(real4) * (size_t)N, hipMemcpyDeviceToHost), "hipMemcpy");
    return out;
  }
  // deprecated in the reference (DPPoissonSlab.cuh:57-72): the same with w zeroed
  std::vector<real4> computeFieldAtParticles() {
    auto out = computeFieldPotentialAtParticles();
    for (auto &v : out) v.w = 0;
    return out;
  }
  // a uniform value per wall: x the top wall's, y the bottom wall's (the other modes of the surface values keep theirs)
  void setSurfaceValuesZeroModeFourier(std::complex<real> top, std::complex<real> bottom) {
    detail::check(uammd_dppoisson_set_surface_zero_mode(h, top.real(), bottom.real()));
  }
  // the corrected k = 0 column of the last call, one entry per Chebyshev coefficient
  std::vector<complex4> getK0Mode() {
    std::vector<double> raw(8 * (size_t)info.cells[2]);
    detail::check(uammd_dppoisson_get_k0_mode(h, raw.data()));
    std::vector<complex4> out(info.cells[2]);
    for (int i = 0; i < info.cells[2]; ++i)
      for (int c = 0; c < 4; ++c) out[i][c] = std::complex<real>((real)raw[8 * i + 2 * c], (real)raw[8 * i + 2 * c + 1]);
    return out;
  }
  int3 getCells() const { return make_int3(info.cells[0], info.cells[1], info.cells[2]); }
  real getExtraHeight() const { return info.He; }
  real getNearFieldCutOff() const { return info.nearFieldCutOff; }
  int getNumberOutside() {
    int n = 0;
    detail::check(uammd_dppoisson_outside_count(h, &n));
    return n;
  }
  void setOption(const char *name, int value) { detail::check(uammd_dppoisson_set_option(h, name, value)); }

private:
  uammd_dppoisson *h = nullptr;
  uammd_dppoisson_info info{};
  detail::DeviceArray<real4> posRows, forceRows;  // the rows of a proper subgroup, gathered
  detail::DeviceArray<real> chargeRows, energyRows;
  int numberParticles() const { return subgroup ? subgroup->getNumberParticles() : pd->getNumParticles(); }

  void run(real4 *fieldPotential, hipStream_t st) {
    const int N = numberParticles();
    if (N == 0) return;
    auto pos = pd->getPos(access::gpu, access::read);
    auto charge = pd->getCharge(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::readwrite);
    auto energy = pd->getEnergy(access::gpu, access::readwrite);
    ParticleGroup *g = subgroup.get();
    real4 *f = const_cast<real4 *>(detail::groupRows((const real4 *)force.raw(), g, forceRows, st));
    real *e = const_cast<real *>(detail::groupRows((const real *)energy.raw(), g, energyRows, st));
    const real4 *posNow = detail::groupRows((const real4 *)pos.raw(), g, posRows, st);
    const real *chargeNow = detail::groupRows((const real *)charge.raw(), g, chargeRows, st);
#if defined(DOUBLE_PRECISION)
    if (fieldPotential) detail::check(uammd_dppoisson_field_potential_f64(h, (const double *)posNow, chargeNow, N, (double *)fieldPotential, (double *)f, e, (void *)st));
    else detail::check(uammd_dppoisson_sum_f64(h, (const double *)posNow, chargeNow, N, (double *)f, e, 0, (void *)st));
#else
    if (fieldPotential) detail::check(uammd_dppoisson_field_potential(h, (const float *)posNow, chargeNow, N, (float *)fieldPotential, (float *)f, e, (void *)st));
    else detail::check(uammd_dppoisson_sum(h, (const float *)posNow, chargeNow, N, (float *)f, e, 0, (void *)st));
#endif
    detail::scatterRows((const real4 *)f, force.raw(), g, st);
    detail::scatterRows((const real *)e, energy.raw(), g, st);
  }

  // FarField::setUpSurfaceValues (FarField.cuh:257-290): the walls sampled at the nodes, and the electroneutrality warning
  void setUpSurfaceValues(const Parameters &par) {
    const int nx = info.cells[0], ny = info.cells[1];
    std::vector<double> top((size_t)nx * ny), bottom((size_t)nx * ny);
    double wallTotal = 0;
    bool any = false;
    if (par.surfaceValues) {
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          const real x = (i / real(nx) - real(0.5)) * par.Lxy.x, y = (j / real(ny) - real(0.5)) * par.Lxy.y;
          const double t = par.surfaceValues->top(x, y), b = par.surfaceValues->bottom(x, y);
          top[i + (size_t)nx * j] = t;
          bottom[i + (size_t)nx * j] = b;
          wallTotal += t + b;
          any = any || t != 0 || b != 0;
        }
    }
    double qtot = 0;
    {
      auto charge = pd->getCharge(access::cpu, access::read);
      for (int i = 0; i < pd->getNumParticles(); ++i) qtot += charge.raw()[i];
    }
    if (qtot + wallTotal != 0) {
      sys->log<System::WARNING>("[DPPoissonSlab] The system is not electroneutral (found %g total charge)", qtot + wallTotal);
      sys->log<System::WARNING>("[DPPoissonSlab] To ensure electroneutrality half an opposite charge will be placed on each wall. This is an "
                                "assumption of the algorithm and cannot be avoided.");
    }
    if (any) detail::check(uammd_dppoisson_set_surface_values(h, top.data(), bottom.data()));
  }
};
}  // namespace uammd
