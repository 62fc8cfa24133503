// DPPoissonSlab the way a user builds it from a plain C++14 translation unit (g++, the C ABI), with real = float and, with
// -DDOUBLE_PRECISION, real = double (Interactor/DoublyPeriodic/DPPoissonSlab.cuh).
//   dppoisson_builtin host   the host-only part: every refusal of the constructor's parameter checks with its message, and the grid,
//                            extra height, cut-off and table size of two configurations, through uammd_dppoisson_create with no handle
//                            asked for.  Needs no GPU; the CPU test builds this mode with the address and undefined-behaviour sanitizers.
//   dppoisson_builtin        the above, then on the GPU: 64 charges between two metallic walls.  The field with wall potentials
//                            (V_t, V_b) minus the field with (0, 0) is (0, 0, -(V_t - V_b) / H) at every particle, to the quadrature
//                            deficit of the truncated window, 1.7e-6 (the k = 0 correction is linear and exact on the grid); force = q E; a virial request throws; the deprecated field call zeroes w.
// Exit status 0 when every check holds; one line per check.
#include "Interactor/DoublyPeriodic/DPPoissonSlab.cuh"
#include "uammd.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

static int failures = 0;
static void check(bool ok, const char *what) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++failures;
}

static uammd_dppoisson_parameters base() {
  uammd_dppoisson_parameters p{};
  p.Lxy[0] = 8; p.Lxy[1] = 7; p.H = 4; p.gw = 0.2; p.split = 1.2; p.Nxy = -1;
  p.permitivity[0] = p.permitivity[1] = p.permitivity[2] = 1;
  p.tolerance = 1e-3; p.upsampling = 1.2; p.support = 12; p.numberStandardDeviations = 4;
  return p;
}
static bool refused(uammd_dppoisson_parameters p, const char *message) {
  uammd_dppoisson_info info{};
  const int e = uammd_dppoisson_create(&p, sizeof(uammd::real) == sizeof(double), nullptr, &info);
  const std::string msg = e ? uammd_hip_last_error() : "";
  return e != 0 && msg.find(message) != std::string::npos;
}

static void hostChecks() {
  const double inf = std::numeric_limits<double>::infinity();
  { auto p = base(); p.split = -1; check(refused(p, "Missing input parameters"), "neither split nor Nxy"); }
  { auto p = base(); p.Nxy = 20; check(refused(p, "Invalid input parameters"), "both split and Nxy"); }
  { auto p = base(); p.split = 0.1; check(refused(p, "Invalid splitting parameter"), "split below the range"); }
  { auto p = base(); p.split = 5; check(refused(p, "Invalid splitting parameter"), "split above the range"); }
  { auto p = base(); p.permitivity[1] = inf; check(refused(p, "Bottom metallic wall not implemented"), "only the bottom wall metallic"); }
  { auto p = base(); p.Lxy[0] = 2; check(refused(p, "[DPPoissonSlab] Incompatible parameters: Extra height"), "He above the smallest box length"); }
  { auto p = base(); p.H = 2.4; p.split = 1.3; check(refused(p, "[DPPoissonSlab] Incompatible parameters: Close range"), "near cut-off above H"); }
  {
    auto p = base();
    p.Lxy[0] = p.Lxy[1] = 50; p.H = 5; p.gw = 0.163299; p.split = 1.70103; p.tolerance = 1e-4;
    uammd_dppoisson_info i{};
    const int e = uammd_dppoisson_create(&p, 1, nullptr, &i);
    check(e == 0 && i.cells[0] == 180 && i.cells[1] == 180 && i.cells[2] == 85 && std::fabs(i.He - 1.681) < 1e-3 && i.nTable == 65536,
          "configuration of the quadrupole test: 180 x 180 x 85, He 1.681");
  }
  {
    auto p = base();
    p.Lxy[0] = p.Lxy[1] = 100; p.H = 10; p.gw = 0.2; p.split = 0.75; p.tolerance = 1e-7;
    uammd_dppoisson_info i{};
    const int e = uammd_dppoisson_create(&p, 1, nullptr, &i);
    check(e == 0 && i.cells[0] == 176 && i.cells[1] == 176 && i.cells[2] == 85 && std::fabs(i.nearFieldCutOff - 6.536) < 1e-3 && i.nTable == (1 << 20),
          "configuration of the three-charge test: 176 x 176 x 85, cut-off 6.536");
  }
}

int main(int argc, char *argv[]) {
  using namespace uammd;
  hostChecks();
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return failures ? 1 : 0;
  const int N = 64;
  const real H = 4, Vt = 0.7, Vb = -0.2;
  auto sys = std::make_shared<System>();
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto charge = pd->getCharge(access::cpu, access::write);
    double total = 0;
    for (int i = 0; i < N; ++i) {  // a fixed, irregular arrangement
      pos[i] = make_real4(real(-4 + 8 * std::fmod(i * 0.618033988749895, 1.0)), real(-3.5 + 7 * std::fmod(i * 0.414213562373095, 1.0)),
                          real(-2 + 4 * std::fmod(0.37 + i * 0.732050807568877, 1.0)), 0);
      charge[i] = real(((i * 37) % 11 - 5) * 0.2);
      total += charge[i];
    }
    charge[0] -= real(total);
  }
  struct Walls : public DPPoissonSlab::SurfaceValueDispatch {
    real t, b;
    Walls(real t, real b) : t(t), b(b) {}
    real top(real, real) override { return t; }
    real bottom(real, real) override { return b; }
  };
  DPPoissonSlab::Parameters par;
  par.Lxy = make_real2(8, 7);
  par.H = H;
  par.gw = 0.2;
  par.split = 1.2;
  par.tolerance = 1e-3;
  par.permitivity.top = par.permitivity.bottom = std::numeric_limits<real>::infinity();
  par.permitivity.inside = 1.7;
  auto zeroForces = [&]() {
    auto force = pd->getForce(access::cpu, access::write);
    auto energy = pd->getEnergy(access::cpu, access::write);
    for (int i = 0; i < N; ++i) { force[i] = make_real4(0, 0, 0, 3); energy[i] = 0; }
  };
  par.surfaceValues = std::make_shared<Walls>(0, 0);
  std::vector<real4> grounded, biased;
  {
    DPPoissonSlab slab(pd, par);
    zeroForces();
    grounded = slab.computeFieldPotentialAtParticles();
    check(slab.getNumberOutside() == 0, "no particle outside the slab");
    bool threw = false;
    try { slab.sum(Interactor::Computables{true, true, true, false}, 0); } catch (const std::runtime_error &) { threw = true; }
    check(threw, "a virial request throws");
  }
  par.surfaceValues = std::make_shared<Walls>(Vt, Vb);
  {
    DPPoissonSlab slab(pd, par);
    zeroForces();
    biased = slab.computeFieldPotentialAtParticles();
    double worst = 0, scale = 0, wrongW = 0;
    {
      auto force = pd->getForce(access::cpu, access::read);
      auto charge = pd->getCharge(access::cpu, access::read);
      for (int i = 0; i < N; ++i) {
        const real4 f = force[i];
        worst = std::fmax(worst, std::fabs(f.x - charge[i] * biased[i].x) + std::fabs(f.y - charge[i] * biased[i].y) + std::fabs(f.z - charge[i] * biased[i].z));
        scale = std::fmax(scale, std::fabs(f.z));
        wrongW += std::fabs(f.w - 3);
      }
    }
    check(worst <= 1e-5 * scale && wrongW == 0, "force = q E, force.w untouched");
    zeroForces();
    auto old = slab.computeFieldAtParticles();
    double w = 0;
    for (auto &v : old) w += std::fabs(v.w);
    check(w == 0 && std::fabs(old[5].z - biased[5].z) <= 1e-5 * std::fabs(biased[5].z), "the deprecated field call zeroes w");
    check((int)slab.getK0Mode().size() == slab.getCells().z, "the k = 0 column has one entry per plane");
  }
  {
    const double expect = -(Vt - Vb) / H;
    const double tol = sizeof(real) == sizeof(double) ? 4e-7 : 2e-4;  // double: twice the window's deficit (x 10 below); float: the two runs' own rounding, fields of order one
    double worst = 0;
    for (int i = 0; i < N; ++i)
      worst = std::fmax(worst, std::fmax(std::fabs((biased[i].z - grounded[i].z) - expect),
                                         std::fmax(std::fabs(biased[i].x - grounded[i].x), std::fabs(biased[i].y - grounded[i].y))));
    std::printf("wall potentials: largest deviation from (0, 0, %.6f): %.3e\n", expect, worst);
    check(worst <= tol * std::fabs(expect) * 10, "the wall potentials add the field (0, 0, -(Vt - Vb) / H)");
  }
  sys->finish();
  return failures ? 1 : 0;
}
