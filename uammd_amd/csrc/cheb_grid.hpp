// Indexing of a doubly periodic grid that is regular in x and y and Chebyshev in z (misc/ChevyshevUtils.cuh:72-175 in the reference),
// and the two windows the doubly periodic solvers spread and gather with, under the footprint rule of the reference's immersed boundary
// kernels (misc/IBM.cu:10-31).  DESIGN.md 17, 18.
//   node (i, j) lies at ((i / nx - 1/2) Lx, (j / ny - 1/2) Ly): the reference's "cell centre" of this grid is the cell's corner
//   plane k lies at (span / 2) cos(pi k / (nz - 1)), k = 0 at the top; the heights come from a table computed once on the host
// A window covers `support` consecutive nodes per periodic axis, starting at leftmost(), and every plane within reach_z() of the particle.
// ChebGeometry is everything that does not depend on the window; a grid type adds its parameters, weight_x, weight_y, weight_z(z, zk) and
// reach_z(), which is all the shared kernels of dp_slab.hpp ask of it.
#pragma once
#include "device_common.hpp"

namespace uammd_hip {

UH_HD float exp_(float a) { return expf(a); }
UH_HD double exp_(double a) { return exp(a); }
UH_HD float acos_(float a) { return acosf(a); }
UH_HD double acos_(double a) { return acos(a); }
UH_HD float abs_(float a) { return fabsf(a); }
UH_HD double abs_(double a) { return fabs(a); }

template <class U> struct ChebGeometry {
  int nx, ny, nz, support;
  U Lx, Ly, span, hx, hy, invhx, invhy;  // span: the height the planes cover, top plane at span / 2
  U rmax;                                // the planes a window is looked for in lie within rmax of the particle
  const U *zplane;                       // [nz] plane heights (device)
  const U *qw;                           // [nz] quadrature weights hx hy (span / 2) clencurt(k, nz - 1) (device)

  UH_D static U fold(U x, U L) { return x - floor_(x / L + U(0.5)) * L; }
  // the cell of a folded coordinate, clamped: no input can produce an index outside [0, n)
  UH_D static int cell(U xin, U L, U invh, int n) {
    int c = (int)((xin + U(0.5) * L) * invh);
    if (c == n) c = 0;
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
  }
  UH_D static U node_distance(U xin, int node, U L, U h) { return fold(xin - (U(-0.5) * L + h * U(node)), L); }
  // first node of the window of a folded coordinate (may be negative: nodes wrap)
  UH_D int leftmost(U xin, U L, U h, U invh, int n) const {
    const int c = cell(xin, L, invh, n);
    int P = support / 2;
    if (abs_(node_distance(xin, c - P, L, h)) > U(support) * h / U(2.0)) P -= 1;
    return c - P;
  }
  UH_D int leftmost_x(U xin) const { return leftmost(xin, Lx, hx, invhx, nx); }
  UH_D int leftmost_y(U yin) const { return leftmost(yin, Ly, hy, invhy, ny); }
  UH_D static int wrap(int c, int n) { return c < 0 ? c + n : (c >= n ? c - n : c); }
  // planes [lo, hi] that can lie within rmax of z: the reference's range (PoissonSlab/spreadInterp.cuh:42-50, StokesSlab/spreadInterp.cuh:102-110)
  // widened by one plane on each side and clamped; the window's own cut decides inside it
  UH_D void plane_range(U z, int &lo, int &hi) const {
    const U bound = span * U(0.5);
    const U zt = fmin(z + rmax, bound), zb = fmax(z - rmax, -bound);
    const U a = fmin(fmax(zt / bound, U(-1)), U(1)), b = fmin(fmax(zb / bound, U(-1)), U(1));
    lo = (int)(U(nz - 1) * (acos_(a) / U(M_PI))) - 1;
    hi = (int)(U(nz - 1) * (acos_(b) / U(M_PI))) + 1;
    lo = lo < 0 ? 0 : (lo > nz - 1 ? nz - 1 : lo);
    hi = hi < 0 ? 0 : (hi > nz - 1 ? nz - 1 : hi);
  }
};

// The truncated Gaussian of the doubly periodic Poisson solver (PoissonSlab/spreadInterp.cuh:22-67): prefactor exp(tau r^2) for
// |r| <= rcut = 1.000001 rmax, else 0, the same on every axis.  DESIGN.md 17.
template <class U> struct ChebGrid : ChebGeometry<U> {
  U prefactor, tau, rcut;

  UH_D U phi(U r) const { return abs_(r) > rcut ? U(0) : prefactor * exp_(tau * r * r); }
  UH_D U weight_x(U xin, int node) const { return phi(this->node_distance(xin, node, this->Lx, this->hx)); }
  UH_D U weight_y(U yin, int node) const { return phi(this->node_distance(yin, node, this->Ly, this->hy)); }
  UH_D U weight_z(U z, U zk) const { return phi(z - zk); }
  UH_D U reach_z() const { return rcut; }
};

// The window of the doubly periodic Stokes solver (StokesSlab/spreadInterp.cuh:70-135): the "exponential of a semicircle" of Barnett and
// Magland per axis, phi(r) = bm(r / a) / a with a = (hx, hy, min(hx, hy)), zero beyond |r| = alpha a; in z the particle's image in the
// nearer wall is subtracted.  The slab is the whole grid: the walls lie at +-span / 2.  DESIGN.md 18.
template <class U> struct ChebGridBM : ChebGeometry<U> {
  U alpha, az, betax, betay, betaz, invnormx, invnormy, invnormz;
  U reachz;  // 1.000001 alpha az: no plane farther than this from a particle takes anything from it

  UH_D static U bm(U r, U a, U alpha, U beta, U invnorm) {  // IBM_kernels.cuh:83-112
    const U z = (r / a) / alpha;
    const U dz2 = U(1) - z * z;
    if (dz2 < U(0)) return U(0);
    return (exp_(beta * (sqrt_(dz2) - U(1))) * invnorm) / a;
  }
  UH_D U weight_x(U xin, int node) const { return bm(this->node_distance(xin, node, this->Lx, this->hx), this->hx, alpha, betax, invnormx); }
  UH_D U weight_y(U yin, int node) const { return bm(this->node_distance(yin, node, this->Ly, this->hy), this->hy, alpha, betay, invnormy); }
  UH_D U weight_z(U z, U zk) const {
    const U H = this->span;
    const U r = z - zk;
    const U top = H - U(2.0) * z + r, bot = -H - U(2.0) * z + r;
    const U rimg = fmin(abs_(top), abs_(bot));
    return bm(r, az, alpha, betaz, invnormz) - bm(rimg, az, alpha, betaz, invnormz);
  }
  UH_D U reach_z() const { return reachz; }
};

}  // namespace uammd_hip
