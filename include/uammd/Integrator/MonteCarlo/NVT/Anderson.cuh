// Same include path as the reference's src/Integrator/MonteCarlo/NVT/Anderson.cuh: Anderson's checkerboard Monte Carlo NVT
// (Anderson.cuh:47-119, Anderson.cu) for Potential::LJ on the C ABI — host code only, usable from plain g++ (C++14).
//
//   using NVT = MC_NVT::Anderson<Potential::LJ>;
//   NVT::Parameters par;
//   par.box = box; par.temperature = 1.5; par.triesPerCell = 10; par.initialJumpSize = 0.1;
//   auto mc = std::make_shared<NVT>(pd, pot, par);
//   mc->forwardTime();  mc->sumEnergy();  mc->getCurrentAcceptanceRatio();
//
// The host draws — the origin of the checkerboard and the order of the subgrids — come from System::rng() in the reference's order; the
// step itself runs in the library (uammd_mc_anderson_step, uammd_hip.h), on the default stream and without a host synchronisation; only a
// tune step reads the counters back.  The Metropolis rule uses the whole pair energy, an invalid
// grid throws, and every cell of a subgrid is visited exactly once.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "Anderson.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../../../uammd.h"

#include <array>

namespace uammd {
namespace MC_NVT {

namespace Anderson_ns {
inline int3 createGridDimensions(Box box, real cutOff) {  // Anderson.cu:52-65
  int3 cellDim = make_int3((int)(box.boxSize.x / cutOff), (int)(box.boxSize.y / cutOff), (int)(box.boxSize.z / cutOff));
  if (cellDim.x % 2 != 0) cellDim.x -= 1;  // an even number of cells
  if (cellDim.y % 2 != 0) cellDim.y -= 1;
  if (cellDim.z % 2 != 0) cellDim.z -= 1;
  if (box.boxSize.z == 0) cellDim.z = 1;
  return cellDim;
}
inline bool checkGridValidity(int3 cellDim) { return !(cellDim.x < 3 || cellDim.y < 3 || cellDim.z == 2); }  // Anderson.cu:67-73

// The host side of the integrator, shared by Anderson<Potential::LJ> below and the generic Anderson<Pot> of device/Anderson.hip.hpp:
// parameters, grid, the draws from System::rng() in the reference's order and the jump-size tuning.  The derived class owns the device
// state and runs the step between beginStep() / drawSubgridOrder() and tune().
class HostSide : public Integrator {
public:
  struct Parameters {  // Anderson.cuh:49-60
    Box box;
    real temperature = -1;
    int triesPerCell = 10;
    real initialJumpSize = 1.0;
    real acceptanceRatio = 0.5;
    int tuneSteps = 10;
    int seed = 0;  // 0: drawn from the system generator
  };
  real getCurrentStepSize() { return jumpSize; }
  real getCurrentAcceptanceRatio() { return currentAcceptanceRatio; }

protected:
  Parameters par;
  bool is2D = false;
  int steps = 0;
  int seed = 0;
  Box box;
  int3 cellDim;
  real3 cellSize;
  real3 currentOrigin;
  real maxOriginDisplacement = 0;
  real jumpSize;
  real currentAcceptanceRatio = 0;

  HostSide(shared_ptr<ParticleData> pd, Parameters in_par, real rcut)  // Anderson.cu:77-105
      : Integrator(pd, "MonteCarlo::Anderson"), par(in_par), jumpSize(in_par.initialJumpSize) {
    System::log<System::MESSAGE>("[MC_NVT::Anderson] Created");
    System::log<System::MESSAGE>("[MC_NVT::Anderson] Temperature: %e", (double)par.temperature);
    if (par.temperature < real(0.0)) {
      System::log<System::ERROR>("[MC_NVT::Anderson] Please specify a temperature!");
      throw std::invalid_argument("Negative temperature detected");
    }
    if (par.box.boxSize.z == real(0.0)) is2D = true;
    setGrid(par.box, rcut);
    System::log<System::MESSAGE>("[MC_NVT::Anderson] Box size: %e %e %e", (double)box.boxSize.x, (double)box.boxSize.y, (double)box.boxSize.z);
    System::log<System::MESSAGE>("[MC_NVT::Anderson] Grid dimensions: %d %d %d", cellDim.x, cellDim.y, cellDim.z);
    seed = par.seed;
    if (par.seed == 0) seed = sys->rng().next32();
  }
  void setGrid(Box newBox, real rcut) {  // Anderson.cu:107-119; the invalid grid is thrown (the reference builds the exception and drops it)
    for (auto &u : updatables) u->updateBox(par.box);
    const int3 cd = createGridDimensions(newBox, rcut);
    if (!checkGridValidity(cd)) {
      System::log<System::ERROR>("[MC_NVT::Anderson] I cannot work with such a large cut off (%e) in this box (%e)!", (double)rcut,
                                 (double)newBox.boxSize.x);
      throw std::invalid_argument("Cut off is too large");
    }
    box = newBox;
    cellDim = cd;
    cellSize = make_real3(box.boxSize.x / real(cd.x), box.boxSize.y / real(cd.y), box.boxSize.z / real(cd.z));
    maxOriginDisplacement = 0.5 * box.boxSize.x;
  }
  int numberSubGrids() const { return is2D ? 4 : 8; }
  void beginStep() {  // Anderson.cu:155-164,177-185: the origin's product in double, then the cast
    System::log<System::DEBUG>("[MC_NVT::Anderson] Performing Monte Carlo Parallel step: %d", steps);
    if (steps == 0)
      for (auto &u : updatables) u->updateTemperature(par.temperature);
    steps++;
    const ::double3 u = sys->rng().uniform3(-1.0, 1.0);
    currentOrigin = make_real3((real)(u.x * maxOriginDisplacement), (real)(u.y * maxOriginDisplacement), (real)(u.z * maxOriginDisplacement));
    if (is2D) currentOrigin.z = 0;
    System::log<System::DEBUG1>("[MC_NVT::Anderson] Current origin: %e %e %e", (double)currentOrigin.x, (double)currentOrigin.y,
                                (double)currentOrigin.z);
  }
  std::array<int, 8> drawSubgridOrder() {  // Anderson.cu:219-225; entry g is the offset (g & 1, g >> 1 & 1, g >> 2 & 1)
    std::array<int, 8> shuffled = {0, 1, 2, 3, 4, 5, 6, 7};
    for (int i = 0; i < numberSubGrids() - 1; ++i) {
      const int j = i + (sys->rng().next() % (numberSubGrids() - i));
      std::swap(shuffled[i], shuffled[j]);
    }
    return shuffled;
  }
  bool isTuneStep() const { return steps % par.tuneSteps == 0 && steps > 1; }
  void tune(unsigned tried, unsigned accepted) {  // Anderson.cu:126-153
    currentAcceptanceRatio = real(accepted) / tried;
    const real3 maxJump = cellSize;
    const real minJumpSize = cellSize.x / 100000;
    if (currentAcceptanceRatio < par.acceptanceRatio) {
      jumpSize *= 0.9;
      if (jumpSize <= minJumpSize) jumpSize = minJumpSize;
    } else if (currentAcceptanceRatio > par.acceptanceRatio) {
      jumpSize *= 1.02;
      jumpSize = std::min({jumpSize, maxJump.x, maxJump.y});
      if (!is2D) jumpSize = std::min(jumpSize, maxJump.z);
    }
    System::log<System::DEBUG>("[MC_NVT::Anderson] Current acceptance ratio: %e", (double)currentAcceptanceRatio);
    System::log<System::DEBUG>("[MC_NVT::Anderson] Current step size: %e, %e*cellSize", (double)jumpSize, (double)(jumpSize / cellSize.x));
  }
};
}  // namespace Anderson_ns

template <class Pot> class Anderson;

template <> class Anderson<Potential::LJ> : public Anderson_ns::HostSide {
public:
  Anderson(shared_ptr<ParticleData> pd, shared_ptr<Potential::LJ> pot, Parameters in_par)
      : Anderson_ns::HostSide(pd, in_par, pot->getCutOff()), pot(pot) {
    detail::check(uammd_mc_anderson_create(&handle));
  }
  ~Anderson() { uammd_mc_anderson_destroy(handle); }
  Anderson(const Anderson &) = delete;

  void updateSimulationBox(Box newBox) {  // Anderson.cu:107-124
    setGrid(newBox, pot->getCutOff());
    unsigned long long tried = 0, accepted = 0;
    detail::check(uammd_mc_anderson_counters(handle, &tried, &accepted, 1, nullptr));
  }

  void forwardTime() override {  // Anderson.cu:155-175
    beginStep();
    const std::array<int, 8> shuffled = drawSubgridOrder();
    const real beta = 1.0 / par.temperature;
    float L[3], o[3] = {currentOrigin.x, currentOrigin.y, currentOrigin.z};
    int per[3];
    box.toArrays(L, per);
    const int cd[3] = {cellDim.x, cellDim.y, cellDim.z};
    {
      auto pos = pd->getPos(access::gpu, access::readwrite);
      detail::check(uammd_mc_anderson_step(handle, (float *)pos.raw(), pd->getNumParticles(), L, per, cd, o, shuffled.data(), numberSubGrids(),
                                           par.triesPerCell, beta, jumpSize, (unsigned)steps, (unsigned)seed, pot->deviceTable(),
                                           pot->getNumberTypes(), nullptr));
    }
    if (isTuneStep()) {
      unsigned long long tried = 0, accepted = 0;
      detail::check(uammd_mc_anderson_counters(handle, &tried, &accepted, 1, nullptr));
      tune((unsigned)tried, (unsigned)accepted);
    }
  }

  real sumEnergy() override {  // Anderson.cu:377-400
    currentOrigin = real3();
    float L[3];
    int per[3];
    box.toArrays(L, per);
    const int cd[3] = {cellDim.x, cellDim.y, cellDim.z};
    auto pos = pd->getPos(access::gpu, access::read);
    auto energy = pd->getEnergy(access::gpu, access::write);
    detail::check(uammd_mc_anderson_energy(handle, (const float *)pos.raw(), pd->getNumParticles(), L, per, cd, pot->deviceTable(),
                                           pot->getNumberTypes(), energy.raw(), nullptr));
    return 0;
  }

private:
  shared_ptr<Potential::LJ> pot;
  uammd_mc_anderson *handle = nullptr;
};

}  // namespace MC_NVT
}  // namespace uammd
