// Same include path as the reference's src/Interactor/BondedForces.cuh: BondedForces<BondType, particlesPerBond>, ComputeType and the
// built-in 2-member kinds BondedType::Harmonic and BondedType::FENE (plus fixed-point bonds).  Angular / Torsional / FourierLAMMPS are
// in AngularBondedForces.cuh and TorsionalBondedForces.cuh.
//
// A BUILT-IN kind runs in libuammd_hip (uammd_bonded_*, C ABI): plain g++ -std=c++14 is enough.  A USER kind — a struct with
//     __device__ ComputeType compute(int bond_index, int ids[N], real3 pos[N], Interactor::Computables comp, BondInfo bi);
//     static BondInfo readBond(std::istream &in);
// is device code: the template lives in device/BondedForces.hip.hpp and needs hipcc (as it needs nvcc in the reference).
// bond_index and ids[] are current indices, as in the reference.  A BondType that is ParameterUpdatable hears every update.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "BondedForces.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../uammd.h"

#include <array>
#include <fstream>
#include <istream>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace uammd {
struct ComputeType {  // BondedForces.cuh:46-50
  real3 force;
  real virial;
  real energy;
};

namespace BondedType {
struct Harmonic {  // BondedForces.cuh:83-117 (the arithmetic: uammd_amd/csrc/bonded.hip)
  Box box;
  Harmonic(Box box = Box()) : box(box) {}
  struct BondInfo { real k, r0; };
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.k >> bi.r0;
    return bi;
  }
};
class FENE {  // BondedForces.cuh:140-166
public:
  Box box;
  FENE(Box box = Box()) : box(box) {}
  struct BondInfo { real r0, k; };
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.k >> bi.r0;
    return bi;
  }
};
}  // namespace BondedType

namespace BondedForces_ns {
// which built-in kind a BondType is (uammd_hip.h UAMMD_BOND_*), -1 for a user kind
template <class T> struct builtin_kind : std::integral_constant<int, -1> {};
template <> struct builtin_kind<BondedType::Harmonic> : std::integral_constant<int, UAMMD_BOND_HARMONIC> {};
template <> struct builtin_kind<BondedType::FENE> : std::integral_constant<int, UAMMD_BOND_FENE> {};

// what a bond file holds (BondedForces.cu:77-185): ids per bond (a fixed point as -(j+1), registered after the particle bonds), the
// BondInfo per bond and the fixed points
template <class BondInfo, int N> struct BondSet {
  std::vector<std::array<int, N>> ids;
  std::vector<BondInfo> info;
  std::vector<real4> fixedPoints;
};

template <class BondType, int N> BondSet<typename BondType::BondInfo, N> readBondFile(const std::string &fileName) {
  BondSet<typename BondType::BondInfo, N> set;
  std::ifstream in(fileName);
  if (!in) throw std::runtime_error("[BondedForces] File " + fileName + " cannot be opened.");
  int nbonds = 0;
  in >> nbonds;
  for (int b = 0; b < nbonds; ++b) {
    std::array<int, N> ids;
    for (int i = 0; i < N; ++i)
      if (!(in >> ids[i])) {
        System::log<System::EXCEPTION>("[BondedForces] ERROR! Bond file ended too soon! Expected %d lines, found %d", nbonds, b);
        throw std::ios_base::failure("File unreadable");
      }
    set.ids.push_back(ids);
    set.info.push_back(BondType::readBond(in));
  }
  if (N == 2) {  // fixed-point bonds: a particle tied to a point in space (BondedForces.cu:160-178)
    int nbondsFP = 0;
    in >> nbondsFP;
    for (int b = 0; b < nbondsFP; ++b) {
      std::array<int, N> ids;
      if (!(in >> ids[0])) {
        System::log<System::EXCEPTION>("[BondedForces] ERROR! Bond file ended too soon! Expected %d lines, found %d", nbondsFP, b);
        throw std::ios_base::failure("File unreadable");
      }
      ids[N - 1] = -(b + 1);
      real3 p;
      in >> p;
      set.fixedPoints.push_back(make_real4(p.x, p.y, p.z, 0));
      set.ids.push_back(ids);
      set.info.push_back(BondType::readBond(in));
    }
  }
  System::log<System::MESSAGE>("[BondedForces] Detected: %d bonds", (int)set.ids.size());
  return set;
}

template <class F> std::enable_if_t<std::is_base_of<ParameterUpdatable, F>::value, ParameterUpdatable *> updatable(F *f) { return f; }
template <class F> std::enable_if_t<!std::is_base_of<ParameterUpdatable, F>::value, ParameterUpdatable *> updatable(F *) { return nullptr; }

// the built-in kinds: the library's CSR kernels
template <class BondType, int N> class LibraryBackend {
  uammd_bonded *h = nullptr;
public:
  LibraryBackend(const BondSet<typename BondType::BondInfo, N> &set, const BondType &bt) {
    static_assert(sizeof(typename BondType::BondInfo) == 2 * sizeof(float), "a built-in BondInfo is two floats");
    detail::check(uammd_bonded_create(&h));
    std::vector<int> ids;
    for (auto &b : set.ids) ids.insert(ids.end(), b.begin(), b.end());
    const float L[3] = {bt.box.boxSize.x, bt.box.boxSize.y, bt.box.boxSize.z};
    const int per[3] = {bt.box.minusInvBoxSize.x != 0, bt.box.minusInvBoxSize.y != 0, bt.box.minusInvBoxSize.z != 0};
    detail::check(uammd_bonded_upload(h, builtin_kind<BondType>::value, (int)set.ids.size(), ids.data(),
                                      reinterpret_cast<const float *>(set.info.data()), (int)set.fixedPoints.size(),
                                      reinterpret_cast<const float *>(set.fixedPoints.data()), L, per));
  }
  ~LibraryBackend() {
    if (h) { (void)hipDeviceSynchronize(); uammd_bonded_destroy(h); }
  }
  LibraryBackend(const LibraryBackend &) = delete;
  LibraryBackend &operator=(const LibraryBackend &) = delete;
  void refresh(const int *d_id2index, int numberParticles, hipStream_t st) { detail::check(uammd_bonded_refresh(h, d_id2index, numberParticles, st)); }
  void sum(BondType &, const real4 *pos, real4 *force, real *energy, real *virial, hipStream_t st) {
    detail::check(uammd_bonded_sum(h, reinterpret_cast<const float *>(pos), reinterpret_cast<float *>(force), energy, virial, st));
  }
};
template <class BondType, int N> class DeviceBackend;  // a user kind: device/BondedForces.hip.hpp (hipcc)
}  // namespace BondedForces_ns

template <class BondType, int particlesPerBond> class BondedForces : public Interactor {
public:
  struct Parameters {
    std::string file;  // the bond file
  };
private:
  static constexpr bool builtin = BondedForces_ns::builtin_kind<BondType>::value >= 0;
  using Backend = std::conditional_t<builtin, BondedForces_ns::LibraryBackend<BondType, particlesPerBond>,
                                     BondedForces_ns::DeviceBackend<BondType, particlesPerBond>>;
  std::shared_ptr<BondType> bondCompute;
  std::unique_ptr<Backend> backend;
  int nbonds = 0;
  bool needsRefresh = true;
  connection reorderConnection;
  ParameterUpdatable *delegate() { return BondedForces_ns::updatable(bondCompute.get()); }
public:
  explicit BondedForces(shared_ptr<ParticleData> pd, Parameters par, std::shared_ptr<BondType> bondForce = std::make_shared<BondType>())
      : Interactor(pd, "BondedForces"), bondCompute(bondForce) {
    System::log<System::MESSAGE>("[BondedForces] Initialized");
    auto set = BondedForces_ns::readBondFile<BondType, particlesPerBond>(par.file);
    nbonds = (int)set.ids.size();
    backend.reset(new Backend(set, *bondCompute));
    reorderConnection = pd->getReorderSignal()->connect([this]() { needsRefresh = true; });  // rows follow ParticleData::sortParticles
  }
  ~BondedForces() override { reorderConnection.disconnect(); }
  void sum(Computables comp, hipStream_t st = 0) override {
    if (nbonds == 0) return;
    if (needsRefresh) {
      backend->refresh(pd->getIdOrderedIndices(access::gpu), pd->getNumParticles(), st);
      needsRefresh = false;
    }
    auto pos = pd->getPos(access::gpu, access::read);
    auto force = comp.force ? pd->getForce(access::gpu, access::readwrite) : property_ptr<real4>();
    auto energy = comp.energy ? pd->getEnergy(access::gpu, access::readwrite) : property_ptr<real>();
    auto virial = comp.virial ? pd->getVirial(access::gpu, access::readwrite) : property_ptr<real>();
    backend->sum(*bondCompute, pos.raw(), force.raw(), energy.raw(), virial.raw(), st);
  }
  void updateTimeStep(real v) override { if (auto *d = delegate()) d->updateTimeStep(v); }
  void updateSimulationTime(real v) override { if (auto *d = delegate()) d->updateSimulationTime(v); }
  void updateBox(Box v) override { if (auto *d = delegate()) d->updateBox(v); }
  void updateTemperature(real v) override { if (auto *d = delegate()) d->updateTemperature(v); }
  void updateViscosity(real v) override { if (auto *d = delegate()) d->updateViscosity(v); }
};
}  // namespace uammd

#if defined(__HIPCC__)
#include "../device/BondedForces.hip.hpp"
#endif
