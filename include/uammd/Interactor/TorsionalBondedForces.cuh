// Same include path as the reference's src/Interactor/TorsionalBondedForces.cuh: 4-member bonds i---j---k---l, BondedType::Torsional and
// BondedType::FourierLAMMPS on the library's kernels (the arithmetic: uammd_amd/csrc/bonded.hip), TorsionalBondedForces<B> =
// BondedForces<B, 4>.  Torsional gives members 0..3 the forces -fj, fm+fj-fk, fn+fk-fm, -fn; the reference's chain of comparisons is
// shifted by one (it ends at ids[4]) and its bonds do not conserve momentum.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "TorsionalBondedForces.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "BondedForces.cuh"

namespace uammd {
namespace BondedType {
struct Torsional {  // TorsionalBondedForces.cuh:43-117: force only
  Box box;
  Torsional(real3 lbox) : box(Box(lbox)) {}
  struct BondInfo { real phi0, k; };
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.k >> bi.phi0;
    return bi;
  }
};
struct FourierLAMMPS {  // TorsionalBondedForces.cuh:119-217: U = kdih (1 + cos(phi - phi0)), force, energy and virial
  Box box;
  FourierLAMMPS(Box box) : box(box) {}
  struct BondInfo { real phi0, kdih; };
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.kdih >> bi.phi0;
    return bi;
  }
};
}  // namespace BondedType
namespace BondedForces_ns {
template <> struct builtin_kind<BondedType::Torsional> : std::integral_constant<int, UAMMD_BOND_TORSIONAL> {};
template <> struct builtin_kind<BondedType::FourierLAMMPS> : std::integral_constant<int, UAMMD_BOND_FOURIER_LAMMPS> {};
}
namespace TorsionalBondedForces_ns {
using TorsionalBond = BondedType::Torsional;
}
template <class BondType> using TorsionalBondedForces = BondedForces<BondType, 4>;
}  // namespace uammd
