// DPStokesSlab_ns::DPStokes in a slit: the self mobility of one particle against its height, parallel and perpendicular to the walls, in
// units of the open-boundary value 1 / (6 pi eta a).  Both vanish at the walls, the perpendicular one faster; at mid height of a wide slit
// they approach 1.  The last lines run DPStokesIntegrator at zero temperature: one step moves the particle by dt M F.
#include "uammd.cuh"
#include "Integrator/BDHI/DoublyPeriodic/DPStokesSlab.cuh"
#include <cstdio>
using namespace uammd;
using DPStokesSlab_ns::DPStokes;
using DPStokesSlab_ns::DPStokesIntegrator;
using DPStokesSlab_ns::cached_vector;

struct Pull : public Interactor {
  using Interactor::Interactor;
  void sum(Computables, hipStream_t) override {
    auto f = pd->getForce(access::cpu, access::write);
    f[0] = make_real4(1, 1, 1, 0);
  }
};

// the window of a force-only particle of hydrodynamic radius a with w = 6 (DPStokesSlab.cuh, "recommended parameters")
template <class Parameters> static Parameters slit(real Lxy, real H, real viscosity, real a) {
  const real h = a / 1.554;
  Parameters par;
  par.nx = par.ny = int(Lxy / h + 0.5);
  par.nz = int(M_PI * H / (2 * h));
  par.w = 6;
  par.beta.x = 1.714 * par.w;
  par.alpha = par.w * 0.5;
  par.mode = DPStokes::WallMode::slit;
  par.viscosity = viscosity;
  par.Lx = par.Ly = Lxy;
  par.H = H;
  return par;
}

int main(int argc, char *argv[]) {
  auto sys = std::make_shared<System>(argc, argv);
  const real a = 1, Lxy = 32, H = 16, viscosity = 1 / (6 * M_PI);
  auto par = slit<DPStokes::Parameters>(Lxy, H, viscosity, a);
  DPStokes solver(par);
  cached_vector<real3> pos(1), force(1);
  int bad = 0;
  double previous = 0;
  std::printf("# height above the bottom wall / a, parallel and perpendicular self mobility x 6 pi eta a\n");
  const int points = 9;
  for (int i = 0; i <= points; ++i) {
    const real z = -0.5 * H + (0.5 * H) * i / points;   // from the bottom wall to mid height
    pos[0] = {0, 0, z};
    force[0] = {1, 0, 0};
    const real3 parallel = solver.Mdot(pos.data().get(), force.data().get(), 1)[0];
    force[0] = {0, 0, 1};
    const real3 perpendicular = solver.Mdot(pos.data().get(), force.data().get(), 1)[0];
    std::printf("%8.4f %10.6f %10.6f\n", double(z + 0.5 * H), double(parallel.x), double(perpendicular.z));
    if (i == 0) bad += std::abs(parallel.x) > 1e-10 || std::abs(perpendicular.z) > 1e-10;   // a particle on a wall spreads nothing
    else bad += !(parallel.x > previous) || !(perpendicular.z > 0) || !(perpendicular.z < parallel.x);
    previous = parallel.x;
  }
  bad += !(previous > 0.5 && previous < 1.0);
  {  // the integrator at zero temperature against the solver
    auto pd = std::make_shared<ParticleData>(1, sys);
    { auto p = pd->getPos(access::cpu, access::write); p[0] = make_real4(0, 0, 1, 0); }
    auto pari = slit<DPStokesIntegrator::Parameters>(Lxy, H, viscosity, a);
    pari.temperature = 0;
    pari.dt = 0.5;
    DPStokesIntegrator integrator(pd, pari);
    integrator.addInteractor(std::make_shared<Pull>(pd, "pull"));
    integrator.forwardTime();
    real4 after;
    { auto p = pd->getPos(access::cpu, access::read); after = p[0]; }
    pos[0] = {0, 0, 1};
    force[0] = {1, 1, 1};
    const real3 mf = solver.Mdot(pos.data().get(), force.data().get(), 1)[0];
    std::printf("one step of dt = %g: moved by (%g, %g, %g), dt M F = (%g, %g, %g)\n", double(pari.dt), double(after.x), double(after.y),
                double(after.z - 1), double(mf.x * pari.dt), double(mf.y * pari.dt), double(mf.z * pari.dt));
    bad += std::abs(after.x - mf.x * pari.dt) > 1e-5 || std::abs(after.y - mf.y * pari.dt) > 1e-5 || std::abs(after.z - 1 - mf.z * pari.dt) > 1e-5;
  }
  sys->finish();
  return bad;
}
