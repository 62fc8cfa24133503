// Hydro::ICM_Compressible_impl<Walls> between two walls from a plain C++14 translation unit (g++, the C ABI): a class derived from
// icm_compressible::MovingWalls with an oscillating bottom wall and a steady top wall, a 9 x 6 x 5 grid of unit cells with initial
// fields given as functions, 64 particles under a constant force each.  Argument: steps (default 20).  Prints, for tests/test_gpu_icm_compressible_walls.py to
// compare with the Python layer on the same input:
//   "icmcw times <the four updateSimulationTime values the walls heard in the first step>"
//   "icmcw ghost <size> rule <0|1>"       the bottom ghost plane in the (n.x + 2)(n.y + 2) layout equals 2 u - v of layer 0, exactly
//   "icmcw density <sum w rho> velocity <sum w v_x> <sum w v_y> <sum w v_z> (staggered) momentum <sum w g_x> <..> <..> positions <sum w q_x> <..> <..>"
// with w = (index % 17) + 1, the index running over cells or particles.
#include "Integrator/Hydro/ICM_Compressible.cuh"
#include "uammd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace uammd;

struct Oscillating : public Hydro::icm_compressible::MovingWalls {
  std::vector<double> times;
  Oscillating() : MovingWalls(make_real2(0.04, 0), make_real2(-0.01, 0.02)) {}
  void updateSimulationTime(real t) override {
    times.push_back(t);
    setVelocities(make_real2(real(0.04 * std::cos(2.0 * (double)t)), 0), make_real2(-0.01, 0.02));
  }
};

struct ConstantForce : public Interactor {
  ConstantForce(std::shared_ptr<ParticleData> pd) : Interactor(pd, "ConstantForce") {}
  void sum(Computables comp, hipStream_t st = 0) override {
    if (!comp.force) return;
    auto force = pd->getForce(access::cpu, access::readwrite);
    for (int i = 0; i < pd->getNumParticles(); ++i) {
      force[i].x += real((i % 7 - 3) / 4.0);
      force[i].y += real((i % 5 - 2) / 3.0);
      force[i].z += real((i % 3 - 1) / 2.0);
    }
  }
};

static std::vector<real> toHost(const real *d, size_t n) {
  std::vector<real> h(n);
  if (hipMemcpy(h.data(), d, sizeof(real) * n, hipMemcpyDeviceToHost) != hipSuccess) std::exit(3);
  return h;
}
static double weighted(const std::vector<real> &v, size_t n) {
  double s = 0;
  for (size_t i = 0; i < n; ++i) s += (double)(i % 17 + 1) * (double)v[i];
  return s;
}

int main(int argc, char *argv[]) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 20;
  auto sys = std::make_shared<System>();
  const int N = 64;
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    for (int i = 0; i < N; ++i) pos[i] = make_real4(real((i % 4) * 1.1 - 1.9), real(((i / 4) % 4) * 1.7 - 2.3), real((i / 16) * 1.3 - 2.1), real(i % 3));
  }
  using ICM = Hydro::ICM_Compressible_impl<Oscillating>;
  ICM::Parameters par;
  par.shearViscosity = 1.3;
  par.bulkViscosity = 0.7;
  par.speedOfSound = 4;
  par.dt = 0.05;
  par.boxSize = make_real3(9, 6, 5);
  par.cellDim = make_int3(9, 6, 5);
  par.seed = 77;
  par.initialDensity = [](real3 r) { return real(1 + 0.05 * std::sin(2 * M_PI * (double)r.x / 9)); };
  par.initialVelocityX = [](real3 r) { return real(0.05 * std::sin(2 * M_PI * (double)r.y / 6)); };
  par.initialVelocityZ = [](real3 r) { return real(0.02 * std::cos(2 * M_PI * (double)r.x / 9)); };
  bool refused = false;
  try {
    ICM::Parameters bad = par;
    bad.temperature = 0.1;  // noise with walls
    ICM wrong(pd, bad);
  } catch (const std::runtime_error &e) {
    refused = std::string(e.what()).find("never draws") != std::string::npos;
  }
  if (!refused) { std::printf("icmcw: temperature > 0 with walls was not refused\n"); return 2; }
  par.walls = std::make_shared<Oscillating>();
  auto icm = std::make_shared<ICM>(pd, par);
  icm->addInteractor(std::make_shared<ConstantForce>(pd));
  for (int s = 0; s < steps; ++s) icm->forwardTime();
  const std::vector<double> &times = par.walls->times;
  if (times.size() != (size_t)4 * steps) { std::printf("icmcw: %zu times recorded\n", times.size()); return 2; }
  std::printf("icmcw times %.9g %.9g %.9g %.9g\n", times[0], times[1], times[2], times[3]);
  const int3 n = icm->getGridSize();
  const size_t nc = (size_t)n.x * n.y * n.z;
  auto density = icm->getCurrentDensity();
  auto stag = icm->getCurrentStaggeredVelocity();
  auto mom = icm->getCurrentMomentum();
  auto ghost = icm->getCurrentBottomGhostCellVelocity();
  const std::vector<real> rho = toHost(density.data().get(), density.size());
  std::vector<real> v[3] = {toHost(stag.x(), nc), toHost(stag.y(), nc), toHost(stag.z(), nc)};
  std::vector<real> g[3] = {toHost(mom.x(), nc), toHost(mom.y(), nc), toHost(mom.z(), nc)};
  std::vector<real> gh[3] = {toHost(ghost.x(), ghost.size()), toHost(ghost.y(), ghost.size()), toHost(ghost.z(), ghost.size())};
  const real2 ub = par.walls->getBottomVelocity();
  const real u[3] = {ub.x, ub.y, 0};
  bool rule = ghost.size() == (size_t)(n.x + 2) * (n.y + 2);
  for (int c = 0; c < 3 && rule; ++c)
    for (int j = 0; j < n.y + 2; ++j)
      for (int i = 0; i < n.x + 2; ++i) {
        const real adj = v[c][(i - 1 + n.x) % n.x + (size_t)n.x * ((j - 1 + n.y) % n.y)];
        rule = rule && gh[c][i + (size_t)j * (n.x + 2)] == real(2) * u[c] - adj;
      }
  std::printf("icmcw ghost %zu rule %d\n", (size_t)ghost.size(), (int)rule);
  double q[3] = {0, 0, 0};
  {
    auto pos = pd->getPos(access::cpu, access::read);
    for (int i = 0; i < N; ++i) {
      const real4 p = pos[i];
      q[0] += (i % 17 + 1) * (double)p.x; q[1] += (i % 17 + 1) * (double)p.y; q[2] += (i % 17 + 1) * (double)p.z;
    }
  }
  std::printf("icmcw density %.9g velocity %.9g %.9g %.9g momentum %.9g %.9g %.9g positions %.9g %.9g %.9g\n", weighted(rho, nc), weighted(v[0], nc),
              weighted(v[1], nc), weighted(v[2], nc), weighted(g[0], nc), weighted(g[1], nc), weighted(g[2], nc), q[0], q[1], q[2]);
  return 0;
}
