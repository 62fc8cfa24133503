// Hydro::ICM_Compressible the way a user builds it from a plain C++14 translation unit (g++, the C ABI): a 5 x 7 x 6 grid of unit cells
// with initial fields given as functions, 64 particles under a constant force each, and an updatable that records the times it hears.
// Argument: steps (default 5).  Prints, for tests/test_icm_compressible_cxx.py to compare with the Python layer on the same input:
//   "icmc times <the four updateSimulationTime values of the first step>"
//   "icmc grid <nx> <ny> <nz> densitySize <n> velocitySize <n> tailZero <0|1> ghostPlane <0|1>"
//   "icmc density <sum w rho>  velocity <sum w v_x> <sum w v_y> <sum w v_z> (collocated)  momentum <sum w g_x> <..> <..>  positions <sum w q_x> <..> <..>"
// with w = (index % 17) + 1, the index running over cells or particles.
#include "Integrator/Hydro/ICM_Compressible.cuh"
#include "uammd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace uammd;

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

struct Recorder : public ParameterUpdatable {
  std::vector<double> times;
  void updateSimulationTime(real t) override { times.push_back(t); }
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
  const int steps = argc > 1 ? std::atoi(argv[1]) : 5;
  const int N = 64;
  auto sys = std::make_shared<System>();
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    for (int i = 0; i < N; ++i) pos[i] = make_real4(real((i % 4) * 1.1 - 1.9), real(((i / 4) % 4) * 1.7 - 2.3), real((i / 16) * 1.3 - 2.1), real(i % 3));
  }
  using ICM = Hydro::ICM_Compressible;
  ICM::Parameters par;
  par.shearViscosity = 1.3;
  par.bulkViscosity = 0.7;
  par.speedOfSound = 4;
  par.dt = 0.05;
  par.boxSize = make_real3(5, 7, 6);
  par.cellDim = make_int3(5, 7, 6);
  par.seed = 77;
  par.initialDensity = [](real3 r) { return real(1 + 0.05 * std::sin(2 * M_PI * (double)r.x / 5)); };
  par.initialVelocityX = [](real3 r) { return real(0.05 * std::sin(2 * M_PI * (double)r.y / 7)); };
  par.initialVelocityZ = [](real3 r) { return real(0.02 * std::cos(2 * M_PI * (double)r.x / 5)); };
  bool refused = false;
  try {
    ICM::Parameters bad = par;
    bad.hydrodynamicRadius = 1;  // both given
    ICM wrong(pd, bad);
  } catch (const std::runtime_error &e) {
    refused = std::string(e.what()).find("either an hydrodynamic radius") != std::string::npos;
  }
  if (!refused) { std::printf("icmc: cellDim and hydrodynamicRadius together were not refused\n"); return 2; }
  auto icm = std::make_shared<ICM>(pd, par);
  icm->addInteractor(std::make_shared<ConstantForce>(pd));
  auto rec = std::make_shared<Recorder>();
  icm->addUpdatable(rec);
  for (int s = 0; s < steps; ++s) icm->forwardTime();
  if (rec->times.size() != (size_t)4 * steps) { std::printf("icmc: %zu times recorded\n", rec->times.size()); return 2; }
  std::printf("icmc times %.9g %.9g %.9g %.9g\n", rec->times[0], rec->times[1], rec->times[2], rec->times[3]);
  const int3 n = icm->getGridSize();
  const size_t nc = (size_t)n.x * n.y * n.z;
  auto density = icm->getCurrentDensity();
  auto vel = icm->getCurrentVelocity();
  auto stag = icm->getCurrentStaggeredVelocity();
  auto mom = icm->getCurrentMomentum();
  auto ghost = icm->getCurrentBottomGhostCellVelocity();
  const std::vector<real> rho = toHost(density.data().get(), density.size());
  std::vector<real> v[3] = {toHost(vel.x(), vel.size()), toHost(vel.y(), vel.size()), toHost(vel.z(), vel.size())};
  std::vector<real> g[3] = {toHost(mom.x(), nc), toHost(mom.y(), nc), toHost(mom.z(), nc)};
  bool tailZero = true;
  for (int c = 0; c < 3; ++c)
    for (size_t i = nc; i < v[c].size(); ++i) tailZero = tailZero && v[c][i] == 0;
  // the ghost plane is the periodic image of the top plane of the staggered field
  const std::vector<real> sz = toHost(stag.z(), nc), gz = toHost(ghost.z(), ghost.size());
  bool ghostPlane = ghost.size() == (size_t)(n.x + 2) * (n.y + 2);
  for (int j = 0; j < n.y && ghostPlane; ++j)
    for (int i = 0; i < n.x; ++i) ghostPlane = ghostPlane && gz[(i + 1) + (size_t)(j + 1) * (n.x + 2)] == sz[i + (size_t)n.x * (j + (size_t)n.y * (n.z - 1))];
  ghostPlane = ghostPlane && gz[0] == sz[(n.x - 1) + (size_t)n.x * ((n.y - 1) + (size_t)n.y * (n.z - 1))];
  std::printf("icmc grid %d %d %d densitySize %zu velocitySize %zu tailZero %d ghostPlane %d\n", n.x, n.y, n.z, (size_t)density.size(),
              (size_t)vel.size(), (int)tailZero, (int)ghostPlane);
  double q[3] = {0, 0, 0};
  {
    auto pos = pd->getPos(access::cpu, access::read);
    for (int i = 0; i < N; ++i) {
      const real4 p = pos[i];
      if (p.w != real(i % 3)) { std::printf("icmc: pos.w of particle %d changed\n", i); return 2; }
      q[0] += (i % 17 + 1) * (double)p.x; q[1] += (i % 17 + 1) * (double)p.y; q[2] += (i % 17 + 1) * (double)p.z;
    }
  }
  std::printf("icmc density %.9g velocity %.9g %.9g %.9g momentum %.9g %.9g %.9g positions %.9g %.9g %.9g\n", weighted(rho, nc), weighted(v[0], nc),
              weighted(v[1], nc), weighted(v[2], nc), weighted(g[0], nc), weighted(g[1], nc), weighted(g[2], nc), q[0], q[1], q[2]);
  return 0;
}
