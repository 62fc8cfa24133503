// Same include path as the reference's src/Interactor/AngularBondedForces.cuh: 3-member bonds i---j---k (j the central particle),
// BondedType::Angular on the library's kernels (the arithmetic: uammd_amd/csrc/bonded.hip), AngularBondedForces<B> = BondedForces<B, 3>.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "AngularBondedForces.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "BondedForces.cuh"

namespace uammd {
namespace BondedType {
struct Angular {  // AngularBondedForces.cuh:50-138: force only (no energy, no virial)
  Box box;
  Angular(real3 lbox) : box(Box(lbox)) {}
  struct BondInfo { real ang0, k; };
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.k >> bi.ang0;
    return bi;
  }
};
}  // namespace BondedType
namespace BondedForces_ns {
template <> struct builtin_kind<BondedType::Angular> : std::integral_constant<int, UAMMD_BOND_ANGULAR> {};
}
namespace AngularBondedForces_ns {
using AngularBond = BondedType::Angular;
}
template <class BondType> using AngularBondedForces = BondedForces<BondType, 3>;
}  // namespace uammd
