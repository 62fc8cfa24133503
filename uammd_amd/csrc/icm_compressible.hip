// Hydro::ICM_Compressible — compressible Inertial Coupling Method: particles advected by a fluctuating COMPRESSIBLE Navier-Stokes fluid
// (density and momentum) on a staggered grid, explicit three-stage Runge-Kutta, no FFT.  Triply periodic
// (ICM_Compressible_impl<DefaultWalls>) or between two walls in z (the Walls section below), single precision.
//
// Reference behaviour (Integrator/Hydro/ICM_Compressible.cu forwardTime :246-257):
//   predictor  q^{n+1/2} = q^n + dt/2 J(q^n) v^n                                                                  :216-227
//   forcing    f = S(q^{n+1/2}) F(q^{n+1/2}), component a on the grid shifted by -h_a/2, three-point Peskin       spreadInterp.cuh:37-57
//   noise      six pairs (W_A, W_B) per cell from Saru(seed, step, cell)                                          Fluctuations.cuh:129-166
//   fluid      three sub-stages U^c = A U^a + B (U^b + dU(U^b)), U^a always the fluid at n                        FluidSolver.cuh:141-200
//                d rho = -dt div g
//                d g   = -dt [div(g (x) v) + grad pi - eta lap v - (xi + eta/3) grad div v] + div Z + dt f,  pi = c^2 rho
//              every operator in the staggered form of SpatialDiscretization.cuh (the Laplacian and grad div as written there: sums of
//              differences over h_b, divided by h_a); after a sub-stage v_a = g_a / (1/2 (rho_i + rho_{i+a}))      :370-385
//   corrector  q^{n+1} = q^n + dt/2 J(q^{n+1/2}) (v^n + v^{n+1})                                                   :231-244
//
// Layout.  The reference keeps an (n+2)^3 ghost layer that it refills with two launches twice per sub-stage and turns momentum into
// velocity in a third pass.  Here a time level is seven planes of n^3 floats {rho, g_x, g_y, g_z, v_x, v_y, v_z}, x fastest, no ghosts:
// the periodic wrap is in the index.  Three levels rotate: the fluid at n, and two scratch levels for the sub-stages.
// A sub-stage is two launches: k_icmc_substage writes rho^c and g^c (thread per cell, direct global loads), k_icmc_velocity divides by
// the face densities, which need rho^c of the +a neighbours.
// The library is compiled with -ffp-contract=off, so the pressure difference pi(i+a) - pi(i) is never contracted into an FMA
// (SpatialDiscretization.cuh:316-366): a uniform fluid at rest stays bitwise at rest.
//
// Walls (GhostCells.cuh, ICM_Compressible.cu:70-102).  With walls in z a field is n.x n.y (n.z + 2) floats: plane 0 and plane n.z + 1 are the
// ghost planes below the bottom and above the top wall, rows still n.x floats, so the interior is one contiguous block of n^3 floats at
// offset n.x n.y.  The kernels are the periodic ones instantiated on WALLS: the z entries of the index object are z, z + 1, z + 2 without a
// wrap, x and y keep their selects.  k_icmc_ghost_fill writes both ghost planes from the adjacent interior layers; the host calls it
// where the reference calls fillGhostCells: after the momentum and density update (the velocity kernel reads the ghost density for the top
// face) and again after the velocity kernel.  The particle windows do not see the walls: they wrap periodically (misc/IBM.cu:41-59).
#include "celllist.hpp"
#include "stagger.hpp"

#include <cmath>
#include <new>
#include <utility>
#include <vector>

namespace uammd_hip {

struct ICMCState {
  uammd_icmc_parameters par{};
  GridT<float> grid{};
  size_t nc = 0;      // interior cells
  size_t fs = 0;      // floats per field: nc, with walls nc + 2 nxy
  size_t off = 0;     // the first interior cell of a field: 0, with walls nxy
  float wallU[4] = {0, 0, 0, 0};  // bottom u_x, u_y, top u_x, u_y of the next ghost fill
  int stage = -1;     // the pieces of a step: -1 idle, s = 0..2 the next sub-stage, 3 the corrector
  float *target = nullptr;        // the level the last sub-stage wrote (ghost fill, velocity)
  const float *forcingNow = nullptr;
  const float2 *noiseNow = nullptr;
  DeviceBuffer level[3], forcing, noise, posOld, planes;  // planes: the packed wall planes of the external mode
  float *cur = nullptr, *tmp1 = nullptr, *tmp2 = nullptr;
  bool injected = false;  // uammd_icmc_set_noise: the noise buffer holds the caller's numbers
  unsigned int step = 0;
};

struct ICMCCoef {
  float A, B, noiseB;      // U^c = A U^a + B (U^b + dU); W = W_A + noiseB W_B
  float dt, eta, bulk, c;  // bulk = xi + eta / 3
  // RungeKutta3::incrementScalar (FluidSolver.cuh:126-130) with A = 1 - B spelled out: U^a + B ((U^b + dU) - U^a), and U^b + dU alone
  // in the first sub-stage (A = 0, B = 1).  Written A U^a + B (...) with the rounded 1/3 and 2/3, a third of all float densities do not
  // survive the last sub-stage of a fluid at rest (1/3 rho + 2/3 rho != rho); this form returns U^a exactly whenever U^b + dU == U^a.
  UH_D float combine(float ua, float x) const { return A == 0.0f ? x : ua + B * (x - ua); }
};

// fillStochasticTensorD (Fluctuations.cuh:129-166); W[e * ncells + cell] = {W_A, W_B}, e = xx, yy, zz, xy, xz, yz
__global__ void __launch_bounds__(256) k_icmc_noise(float2 *__restrict__ W, int ncells, uint seed, uint step, float dt, float eta, float xi,
                                                    float T, float dV) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ncells) return;
  const float pc = sqrtf((dt * 2.0f * eta * T) / dV);
  const float pt = sqrtf((dt * xi * T) / (3.0f * dV)) - (1.0f / 3.0f) * sqrtf((dt * 2.0f * eta * T) / dV);
  Saru rng(seed, step, (uint)i);
  const float sq2 = 1.4142135623730950488016887f;
  const float2 wxx = rng.gf(0.0f, sq2), wyy = rng.gf(0.0f, sq2), wzz = rng.gf(0.0f, sq2);
  const float2 wxy = rng.gf(0.0f, 1.0f), wxz = rng.gf(0.0f, 1.0f), wyz = rng.gf(0.0f, 1.0f);
  const float2 tr = make_float2(wxx.x + wyy.x + wzz.x, wxx.y + wyy.y + wzz.y);
  const size_t n = (size_t)ncells;
  W[i] = make_float2(pc * wxx.x + pt * tr.x, pc * wxx.y + pt * tr.y);
  W[n + i] = make_float2(pc * wyy.x + pt * tr.x, pc * wyy.y + pt * tr.y);
  W[2 * n + i] = make_float2(pc * wzz.x + pt * tr.x, pc * wzz.y + pt * tr.y);
  W[3 * n + i] = make_float2(pc * wxy.x, pc * wxy.y);
  W[4 * n + i] = make_float2(pc * wxz.x, pc * wxz.y);
  W[5 * n + i] = make_float2(pc * wyz.x, pc * wyz.y);
}

// the cell and its neighbours at -1, 0, +1 along each axis: wrapped, or with WALLS the planes z, z + 1, z + 2 of a field that carries its
// two ghost planes (interior layer z is plane z + 1)
template <bool WALLS>
struct ICMCNbr {
  int xs[3], ys[3], zs[3], nx, ny;
  UH_D ICMCNbr(int3 n, int x, int y, int z) : nx(n.x), ny(n.y) {
    xs[0] = x == 0 ? n.x - 1 : x - 1; xs[1] = x; xs[2] = x + 1 == n.x ? 0 : x + 1;
    ys[0] = y == 0 ? n.y - 1 : y - 1; ys[1] = y; ys[2] = y + 1 == n.y ? 0 : y + 1;
    if (WALLS) { zs[0] = z; zs[1] = z + 1; zs[2] = z + 2; }
    else { zs[0] = z == 0 ? n.z - 1 : z - 1; zs[1] = z; zs[2] = z + 1 == n.z ? 0 : z + 1; }
  }
  UH_D size_t operator()(int a, int b, int c) const { return (size_t)xs[a + 1] + (size_t)nx * ((size_t)ys[b + 1] + (size_t)ny * (size_t)zs[c + 1]); }
};

// floats per field and the index of interior cell ic in it
template <bool WALLS> UH_D size_t icmc_field_size(int3 n, size_t nc) { return WALLS ? nc + 2 * (size_t)n.x * (size_t)n.y : nc; }
template <bool WALLS> UH_D auto icmc_centre(int3 n, int ic) {
  if constexpr (WALLS) return (size_t)ic + (size_t)n.x * (size_t)n.y;
  else return ic;
}

// a time level: rho at 0, g_a at (1 + a) nc, v_a at (4 + a) nc; nc the floats per field
struct ICMCLevel {
  const float *p;
  size_t nc;
  UH_D const float *rho() const { return p; }
  UH_D const float *g(int a) const { return p + (size_t)(1 + a) * nc; }
  UH_D const float *v(int a) const { return p + (size_t)(4 + a) * nc; }
};

// rho^c of the cell: combine(rho^a, rho^b - dt div g^b)                                              FluidSolver.cuh:59-66, :156-162
template <class NBR>
UH_D float icmc_density(const NBR &I, const ICMCLevel &a, const ICMCLevel &b, real3f ih, const ICMCCoef &k) {
  float div = 0.0f;
  div += ih.x * (b.g(0)[I(0, 0, 0)] - b.g(0)[I(-1, 0, 0)]);
  div += ih.y * (b.g(1)[I(0, 0, 0)] - b.g(1)[I(0, -1, 0)]);
  div += ih.z * (b.g(2)[I(0, 0, 0)] - b.g(2)[I(0, 0, -1)]);
  const float inc = -div * k.dt;
  return k.combine(a.rho()[I(0, 0, 0)], b.rho()[I(0, 0, 0)] + inc);
}

// Z^{ab} = 1/2 (g_b(c) + g_b(c + a)) 1/2 (v_a(c) + v_a(c + b)) at cell c = owner + (ox, oy, oz)     SpatialDiscretization.cuh:113-128
template <int AL, int BE, class NBR>
UH_D float icmc_kinetic(const NBR &I, const ICMCLevel &b, int ox, int oy, int oz) {
  const int ax = AL == 0, ay = AL == 1, az = AL == 2, bx = BE == 0, by = BE == 1, bz = BE == 2;
  const float vA = b.v(AL)[I(ox, oy, oz)];
  const float gB = b.g(BE)[I(ox, oy, oz)];
  const float gBp = b.g(BE)[I(ox + ax, oy + ay, oz + az)];
  const float gCorner = 0.5f * (gB + gBp);
  const float vAp = b.v(AL)[I(ox + bx, oy + by, oz + bz)];
  const float vCorner = 0.5f * (vA + vAp);
  return gCorner * vCorner;
}

// the momentum increment of component AL                                                             FluidSolver.cuh:75-106, :163-179
template <int AL, bool NOISE, class NBR>
UH_D float icmc_momentum_increment(const NBR &I, const ICMCLevel &b, real3f h, real3f ih, const ICMCCoef &k, const float2 *__restrict__ W,
                                   const float *__restrict__ forcing, size_t nc) {
  const int ax = AL == 0, ay = AL == 1, az = AL == 2;
  const float iha = AL == 0 ? ih.x : (AL == 1 ? ih.y : ih.z), ha = AL == 0 ? h.x : (AL == 1 ? h.y : h.z);
  // div(g (x) v), :138-149, :274-289
  float kin = 0.0f;
  kin += ih.x * (icmc_kinetic<AL, 0>(I, b, 0, 0, 0) - icmc_kinetic<AL, 0>(I, b, -1, 0, 0));
  kin += ih.y * (icmc_kinetic<AL, 1>(I, b, 0, 0, 0) - icmc_kinetic<AL, 1>(I, b, 0, -1, 0));
  kin += ih.z * (icmc_kinetic<AL, 2>(I, b, 0, 0, 0) - icmc_kinetic<AL, 2>(I, b, 0, 0, -1));
  // grad pi, :329-367 (no FMA: the file is built with -ffp-contract=off)
  const float c2 = k.c * k.c;
  const float gradPi = iha * (c2 * b.rho()[I(ax, ay, az)] - c2 * b.rho()[I(0, 0, 0)]);
  // lap v, :156-164, :235-252, :257-267
  const float *vA = b.v(AL);
  const float v0 = vA[I(0, 0, 0)];
  const float lx = (vA[I(1, 0, 0)] - 2.0f * v0 + vA[I(-1, 0, 0)]) / h.x;
  const float ly = (vA[I(0, 1, 0)] - 2.0f * v0 + vA[I(0, -1, 0)]) / h.y;
  const float lz = (vA[I(0, 0, 1)] - 2.0f * v0 + vA[I(0, 0, -1)]) / h.z;
  const float lap = (lx + ly + lz) / ha;
  // grad div v, :170-184, :204-231
  const float dx = b.v(0)[I(ax, ay, az)] - b.v(0)[I(ax - 1, ay, az)] - b.v(0)[I(0, 0, 0)] + b.v(0)[I(-1, 0, 0)];
  const float dy = b.v(1)[I(ax, ay, az)] - b.v(1)[I(ax, ay - 1, az)] - b.v(1)[I(0, 0, 0)] + b.v(1)[I(0, -1, 0)];
  const float dz = b.v(2)[I(ax, ay, az)] - b.v(2)[I(ax, ay, az - 1)] - b.v(2)[I(0, 0, 0)] + b.v(2)[I(0, 0, -1)];
  const float gd = (dx / h.x + dy / h.y + dz / h.z) / ha;
  const float stress = -gradPi + k.eta * lap + k.bulk * gd;
  float m = 0.0f;
  m += kin;
  m -= stress;
  const float det = -k.dt * m;
  float fl = 0.0f;
  if (NOISE) {  // Fluctuations.cuh:80-113: sum_b (Z^{ab}(i) - Z^{ab}(i - b)) / h_b, Z = W_A + noiseB W_B
    constexpr int ex = AL == 0 ? 0 : (AL == 1 ? 3 : 4), ey = AL == 0 ? 3 : (AL == 1 ? 1 : 5), ez = AL == 0 ? 4 : (AL == 1 ? 5 : 2);
    auto z = [&](int e, size_t cell) { const float2 w = W[(size_t)e * nc + cell]; return 1.0f * w.x + k.noiseB * w.y; };
    const size_t c0 = I(0, 0, 0);
    fl += ih.x * (z(ex, c0) - z(ex, I(-1, 0, 0)));
    fl += ih.y * (z(ey, c0) - z(ey, I(0, -1, 0)));
    fl += ih.z * (z(ez, c0) - z(ez, I(0, 0, -1)));
  }
  const float f = forcing ? forcing[(size_t)AL * nc + I(0, 0, 0)] : 0.0f;
  return det + fl + k.dt * f;
}

// rungeKuttaSubStepD (FluidSolver.cuh:141-200): rho^c and g^c into out, which never aliases a or b
template <bool NOISE, bool WALLS>
__global__ void __launch_bounds__(256) k_icmc_substage(const float *__restrict__ pa, const float *__restrict__ pb, float *__restrict__ out,
                                                       int3 n, real3f h, real3f ih, ICMCCoef k, const float2 *__restrict__ W,
                                                       const float *__restrict__ forcing) {
  const int ic = blockIdx.x * 256 + threadIdx.x;
  const size_t nc = (size_t)n.x * n.y * n.z;
  if ((size_t)ic >= nc) return;
  const int x = ic % n.x, y = (ic / n.x) % n.y, z = ic / (n.x * n.y);
  const ICMCNbr<WALLS> I(n, x, y, z);
  const size_t fs = icmc_field_size<WALLS>(n, nc);
  const auto c0 = icmc_centre<WALLS>(n, ic);
  const ICMCLevel a{pa, fs}, b{pb, fs};
  const float rhoC = icmc_density(I, a, b, ih, k);
  float gC[3];
  gC[0] = k.combine(a.g(0)[c0], b.g(0)[c0] + icmc_momentum_increment<0, NOISE>(I, b, h, ih, k, W, forcing, fs));
  gC[1] = k.combine(a.g(1)[c0], b.g(1)[c0] + icmc_momentum_increment<1, NOISE>(I, b, h, ih, k, W, forcing, fs));
  gC[2] = k.combine(a.g(2)[c0], b.g(2)[c0] + icmc_momentum_increment<2, NOISE>(I, b, h, ih, k, W, forcing, fs));
  out[c0] = rhoC;
  out[fs + c0] = gC[0]; out[2 * fs + c0] = gC[1]; out[3 * fs + c0] = gC[2];
}

// momentumToVelocityD (SpatialDiscretization.cuh:370-385) and velocityToMomentumD (:394-409) on one level, in place
template <bool TO_VELOCITY, bool WALLS>
__global__ void __launch_bounds__(256) k_icmc_velocity(float *__restrict__ p, int3 n) {
  const int ic = blockIdx.x * 256 + threadIdx.x;
  const size_t nc = (size_t)n.x * n.y * n.z;
  if ((size_t)ic >= nc) return;
  const int x = ic % n.x, y = (ic / n.x) % n.y, z = ic / (n.x * n.y);
  const ICMCNbr<WALLS> I(n, x, y, z);
  const size_t fs = icmc_field_size<WALLS>(n, nc);
  const auto c0 = icmc_centre<WALLS>(n, ic);
  const float r0 = p[c0];
  const float d[3] = {0.5f * (r0 + p[I(1, 0, 0)]), 0.5f * (r0 + p[I(0, 1, 0)]), 0.5f * (r0 + p[I(0, 0, 1)])};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (TO_VELOCITY) p[(size_t)(4 + c) * fs + c0] = p[(size_t)(1 + c) * fs + c0] / d[c];
    else p[(size_t)(1 + c) * fs + c0] = p[(size_t)(4 + c) * fs + c0] * d[c];
  }
}

// computeCollocatedVelocityD (:419-444); with WALLS the bottom layer's v_z average reads the bottom ghost plane, as the reference's does
template <bool WALLS>
__global__ void __launch_bounds__(256) k_icmc_collocate(const float *__restrict__ p, int3 n, float *__restrict__ ox, float *__restrict__ oy,
                                                        float *__restrict__ oz) {
  const int ic = blockIdx.x * 256 + threadIdx.x;
  const size_t nc = (size_t)n.x * n.y * n.z;
  if ((size_t)ic >= nc) return;
  const int x = ic % n.x, y = (ic / n.x) % n.y, z = ic / (n.x * n.y);
  const ICMCNbr<WALLS> I(n, x, y, z);
  const auto c0 = icmc_centre<WALLS>(n, ic);
  const ICMCLevel l{p, icmc_field_size<WALLS>(n, nc)};
  ox[ic] = 0.5f * (l.v(0)[c0] + l.v(0)[I(-1, 0, 0)]);
  oy[ic] = 0.5f * (l.v(1)[c0] + l.v(1)[I(0, -1, 0)]);
  oz[ic] = 0.5f * (l.v(2)[c0] + l.v(2)[I(0, 0, -1)]);
}

// spreadParticleForces (spreadInterp.cuh:37-57): one wave per particle, 81 atomics into the three forcing planes.  A node outside the grid
// (the cell of a position that is not finite) is skipped: nothing is read or written out of bounds.  With WALLS f points at the first
// interior cell of a field with ghost planes; the window wraps periodically all the same (misc/IBM.cu:41-59).
template <bool WALLS>
__global__ void __launch_bounds__(256) k_icmc_spread(const float4 *__restrict__ pos, const float4 *__restrict__ force, float *__restrict__ f,
                                                     size_t nc, int N, GridT<float> grid, float invh) {
  const int lane = threadIdx.x & 63;
  const int id = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= N) return;
  const float4 p = pos[id], F = force[id];
  for (int l = lane; l < 81; l += 64) {
    const StagNode s = stag_node(grid, grid.cellDim.x, invh, real3f{p.x, p.y, p.z}, l);
    const int c = l / 27;
    if (s.node < nc) unsafeAtomicAdd(&f[(size_t)c * icmc_field_size<WALLS>(grid.cellDim, nc) + s.node], s.w * (c == 0 ? F.x : (c == 1 ? F.y : F.z)));
  }
}

// out = base + dt/2 J(eval) (va [+ vb]): one wave per particle, the 81 (component, node) pairs of the shifted three-point windows
// (interpolateFluidVelocities, spreadInterp.cuh:59-79; MidStepEulerFunctor, ICM_Compressible.cu:190-198).  keep: q^n saved (predictor).
// With WALLS va and vb point at the first interior cell of v_x in a level with ghost planes.
template <bool WALLS>
__global__ void __launch_bounds__(256) k_icmc_advect(float4 *__restrict__ pos, float4 *__restrict__ posOld, bool predictor,
                                                     const float *__restrict__ va, const float *__restrict__ vb, size_t nc, int N,
                                                     GridT<float> grid, float invh, float dt) {
  const int lane = threadIdx.x & 63;
  const int id = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= N) return;
  const float4 p = pos[id];
  const float dV = grid.cellSize.x * grid.cellSize.y * grid.cellSize.z;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int l = lane; l < 81; l += 64) {
    const StagNode s = stag_node(grid, grid.cellDim.x, invh, real3f{p.x, p.y, p.z}, l);
    const int c = l / 27;
    if (s.node >= nc) continue;  // the cell of a position that is not finite
    const size_t fs = icmc_field_size<WALLS>(grid.cellDim, nc);
    float u = va[(size_t)c * fs + s.node];
    if (vb) u += vb[(size_t)c * fs + s.node];
    const float v = s.w * u * dV;
    acc[0] += c == 0 ? v : 0.0f; acc[1] += c == 1 ? v : 0.0f; acc[2] += c == 2 ? v : 0.0f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc[0] += __shfl_xor(acc[0], o, 64); acc[1] += __shfl_xor(acc[1], o, 64); acc[2] += __shfl_xor(acc[2], o, 64);
  }
  if (lane != 0) return;
  const float pref = 0.5f * dt;
  if (predictor) {
    posOld[id] = p;
    pos[id] = make_float4(p.x + pref * acc[0], p.y + pref * acc[1], p.z + pref * acc[2], p.w);
  } else {
    const float4 po = posOld[id];
    pos[id] = make_float4(po.x + pref * acc[0], po.y + pref * acc[1], po.z + pref * acc[2], po.w);
  }
}

// The built-in wall rule, both walls in one launch, a thread per (i, j) column: with "adj" the interior layer next to the wall and
// u = (u_x, u_y, 0) the wall's velocity,  rho_ghost = rho_adj,  v_ghost = 2 u - v_adj,  g_ghost = 2 u rho_adj - g_adj
// (test/Hydro/ICM_Compressible/walltest.cu:38-71, for both tangential components and both walls).  u = {bottom x, y, top x, y}.
__global__ void __launch_bounds__(256) k_icmc_ghost_fill(float *__restrict__ p, int3 n, float4 u) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  const size_t nxy = (size_t)n.x * (size_t)n.y;
  if ((size_t)id >= nxy) return;
  const size_t fs = nxy * ((size_t)n.z + 2);
  const size_t ghost[2] = {(size_t)id, ((size_t)n.z + 1) * nxy + id}, adj[2] = {nxy + id, (size_t)n.z * nxy + id};
  const float uw[2][3] = {{u.x, u.y, 0.0f}, {u.z, u.w, 0.0f}};
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const float rho = p[adj[w]];
    p[ghost[w]] = rho;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[(size_t)(4 + c) * fs + ghost[w]] = 2.0f * uw[w][c] - p[(size_t)(4 + c) * fs + adj[w]];
      p[(size_t)(1 + c) * fs + ghost[w]] = 2.0f * uw[w][c] * rho - p[(size_t)(1 + c) * fs + adj[w]];
    }
  }
}

// The four planes a user's wall rule touches, in the reference's ghost-grid strides: per field 4 planes of (n.x + 2)(n.y + 2) floats,
// {bottom ghost, bottom adjacent layer, top adjacent layer, top ghost}, the x / y ghost columns periodic images.  The ghost planes are
// handed out holding their periodic images in z, as the reference's are when its wall rule runs (updateGhostCellsD, GhostCells.cuh:73-82).
__global__ void __launch_bounds__(256) k_icmc_pack_wall_planes(const float *__restrict__ p, float *__restrict__ out, int3 n) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  const int gx = n.x + 2, gy = n.y + 2;
  if (id >= gx * gy) return;
  const int i = id % gx, j = id / gx;
  const int x = i == 0 ? n.x - 1 : (i == gx - 1 ? 0 : i - 1), y = j == 0 ? n.y - 1 : (j == gy - 1 ? 0 : j - 1);
  const size_t nxy = (size_t)n.x * (size_t)n.y, fs = nxy * ((size_t)n.z + 2), P = (size_t)gx * gy;
  const size_t col = (size_t)x + (size_t)n.x * (size_t)y;
  const size_t src[4] = {(size_t)n.z * nxy + col, nxy + col, (size_t)n.z * nxy + col, nxy + col};
#pragma unroll
  for (int f = 0; f < 7; ++f)
#pragma unroll
    for (int k = 0; k < 4; ++k) out[((size_t)f * 4 + k) * P + id] = p[(size_t)f * fs + src[k]];
}

// the ghost planes back into the level (interior columns); what a rule wrote into the adjacent planes is dropped
__global__ void __launch_bounds__(256) k_icmc_unpack_wall_planes(float *__restrict__ p, const float *__restrict__ in, int3 n) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  const size_t nxy = (size_t)n.x * (size_t)n.y;
  if ((size_t)id >= nxy) return;
  const int gx = n.x + 2, gy = n.y + 2;
  const size_t fs = nxy * ((size_t)n.z + 2), P = (size_t)gx * gy;
  const size_t g = (size_t)(id % n.x + 1) + (size_t)gx * (size_t)(id / n.x + 1);
#pragma unroll
  for (int f = 0; f < 7; ++f) {
    p[(size_t)f * fs + id] = in[((size_t)f * 4 + 0) * P + g];
    p[(size_t)f * fs + ((size_t)n.z + 1) * nxy + id] = in[((size_t)f * 4 + 3) * P + g];
  }
}

static inline dim3 icmc_blocks(size_t nc) { return dim3((unsigned)((nc + 255) / 256)); }

static inline bool icmc_walls(const ICMCState *f) { return f->par.walls != UAMMD_ICMC_WALLS_NONE; }

static void icmc_launch_ghost_fill(ICMCState *f, float *level, hipStream_t st) {
  const int3 n = f->grid.cellDim;
  hipLaunchKernelGGL(k_icmc_ghost_fill, icmc_blocks((size_t)n.x * n.y), dim3(256), 0, st, level, n,
                     make_float4(f->wallU[0], f->wallU[1], f->wallU[2], f->wallU[3]));
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

// checkInputValidity, ICM_Compressible.cuh:293-311
int uammd_icmc_validate(const uammd_icmc_parameters *par) {
  if (!par) { set_last_error("uammd_icmc_validate: null argument"); return -1; }
  if (par->shearViscosity <= 0) { set_last_error("[ICM_Compressible] Invalid shear viscosity"); return -2; }
  if (par->bulkViscosity < 0) { set_last_error("[ICM_Compressible] Invalid bulk viscosity"); return -2; }
  if (par->temperature < 0) { set_last_error("[ICM_Compressible] Invalid temperature"); return -2; }
  if (par->dt < 0) { set_last_error("[ICM_Compressible] Invalid dt"); return -2; }
  if (par->speedOfSound <= 0) { set_last_error("[ICM_Compressible] Invalid speed of sound"); return -2; }
  if (par->boxSize[0] <= 0) { set_last_error("[ICM_Compressible] Invalid box size"); return -2; }
  if ((par->cells[0] <= 0 && par->hydrodynamicRadius <= 0) || (par->cells[0] > 0 && par->hydrodynamicRadius > 0)) {
    set_last_error("[ICM_Compressible] I need either an hydrodynamic radius or a number of cells");
    return -2;
  }
  if (!(par->boxSize[1] > 0) || !(par->boxSize[2] > 0)) { set_last_error("[ICM_Compressible] Invalid box size"); return -2; }
  if (par->walls != UAMMD_ICMC_WALLS_NONE) {
    if (par->walls != UAMMD_ICMC_WALLS_BUILTIN && par->walls != UAMMD_ICMC_WALLS_EXTERNAL) { set_last_error("[ICM_Compressible] Invalid wall mode %d", par->walls); return -2; }
    if (par->temperature > 0) {
      set_last_error("[ICM_Compressible] walls with temperature > 0 are not supported: the reference reads a stochastic stress in the "
                     "bottom ghost plane that it never draws, and no rule for the noise at a wall is pinned");
      return -2;
    }
    if (par->cells[0] > 0 && par->cells[2] < 1) { set_last_error("[ICM_Compressible] walls need at least one layer of cells in z"); return -2; }
  }
  return 0;
}

int uammd_icmc_create(const uammd_icmc_parameters *par, uammd_icmc **out, int cells[3]) {
  if (!par || !out) { set_last_error("uammd_icmc_create: null argument"); return -1; }
  if (int e = uammd_icmc_validate(par)) return e;
  int cd[3] = {par->cells[0], par->cells[1], par->cells[2]};
  if (par->hydrodynamicRadius > 0) {  // :221-223, 0.91 is the three-point Peskin kernel's
    const float hgrid = (float)(0.91 * (double)par->hydrodynamicRadius);
    for (int a = 0; a < 3; ++a) cd[a] = (int)(par->boxSize[a] / hgrid);
  }
  if (cd[0] < 1 || cd[1] < 1 || cd[2] < 1 || (double)cd[0] * cd[1] * cd[2] > 2.0e8) {
    set_last_error("uammd_icmc_create: a grid of %d x %d x %d cells is not supported", cd[0], cd[1], cd[2]);
    return -2;
  }
  ICMCState *f = new (std::nothrow) ICMCState();
  if (!f) { set_last_error("uammd_icmc_create: out of host memory"); return -3; }
  f->par = *par;
  const int per[3] = {1, 1, 1};
  f->grid = make_grid(make_box<float>(par->boxSize, per), make_int3(cd[0], cd[1], cd[2]));
  f->nc = (size_t)cd[0] * cd[1] * cd[2];
  f->off = icmc_walls(f) ? (size_t)cd[0] * cd[1] : 0;
  f->fs = f->nc + 2 * f->off;
  const size_t bytes = sizeof(float) * 7 * f->fs;
  int e = 0;
  for (int l = 0; l < 3 && !e; ++l) e = f->level[l].reserve(bytes);
  if (!e) e = f->forcing.reserve(sizeof(float) * 3 * f->fs);
  if (!e) e = f->noise.reserve(sizeof(float) * 12 * f->nc);
  if (!e && par->walls == UAMMD_ICMC_WALLS_EXTERNAL) e = f->planes.reserve(sizeof(float) * 28 * (size_t)(cd[0] + 2) * (cd[1] + 2));
  if (e) { delete f; return e; }
  f->cur = (float *)f->level[0].ptr; f->tmp1 = (float *)f->level[1].ptr; f->tmp2 = (float *)f->level[2].ptr;
  // the default fluid: rho = 1, v = 0 (:376-377); with walls at rest these are also the ghost planes of the built-in rule.  The scratch
  // levels start at zero so that the first fill after a sub-stage reads defined velocities (it only needs the density).
  std::vector<float> one(f->fs, 1.0f);
  if (hipMemset(f->cur, 0, bytes) != hipSuccess || hipMemcpy(f->cur, one.data(), sizeof(float) * f->fs, hipMemcpyHostToDevice) != hipSuccess ||
      (icmc_walls(f) && (hipMemset(f->tmp1, 0, bytes) != hipSuccess || hipMemset(f->tmp2, 0, bytes) != hipSuccess)) ||
      hipMemset(f->noise.ptr, 0, sizeof(float) * 12 * f->nc) != hipSuccess) {
    set_last_error("uammd_icmc_create: initialising the fluid failed");
    delete f;
    return -4;
  }
  if (cells) for (int a = 0; a < 3; ++a) cells[a] = cd[a];
  *out = reinterpret_cast<uammd_icmc *>(f);
  return 0;
}

int uammd_icmc_destroy(uammd_icmc *h) {
  delete reinterpret_cast<ICMCState *>(h);
  return 0;
}

int uammd_icmc_set_fluid(uammd_icmc *h, const float *d_density, const float *d_vx, const float *d_vy, const float *d_vz, void *stream) {
  if (!h) { set_last_error("uammd_icmc_set_fluid: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  hipStream_t st = (hipStream_t)stream;
  const size_t b = sizeof(float) * f->nc;
  const float *src[4] = {d_density, d_vx, d_vy, d_vz};
  const int plane[4] = {0, 4, 5, 6};
  for (int i = 0; i < 4; ++i)
    if (src[i]) UH_CHECK(hipMemcpyAsync(f->cur + plane[i] * f->fs + f->off, src[i], b, hipMemcpyDeviceToDevice, st));
  if (f->par.walls == UAMMD_ICMC_WALLS_EXTERNAL) return 0;  // the caller: its fill, uammd_icmc_velocity_to_momentum, its fill
  if (icmc_walls(f)) {  // initializeFluid (:411-413): fill, velocity to momentum (the top face reads the ghost density), fill
    icmc_launch_ghost_fill(f, f->cur, st);
    hipLaunchKernelGGL((k_icmc_velocity<false, true>), icmc_blocks(f->nc), dim3(256), 0, st, f->cur, f->grid.cellDim);
    icmc_launch_ghost_fill(f, f->cur, st);
  } else {
    hipLaunchKernelGGL((k_icmc_velocity<false, false>), icmc_blocks(f->nc), dim3(256), 0, st, f->cur, f->grid.cellDim);
  }
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_icmc_get_fluid(uammd_icmc *h, float *d_density, float *const d_v[3], float *const d_g[3], void *stream) {
  if (!h) { set_last_error("uammd_icmc_get_fluid: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  hipStream_t st = (hipStream_t)stream;
  const size_t b = sizeof(float) * f->nc;
  const float *cur = f->cur + f->off;  // the interior is contiguous
  if (d_density) UH_CHECK(hipMemcpyAsync(d_density, cur, b, hipMemcpyDeviceToDevice, st));
  for (int c = 0; c < 3; ++c) {
    if (d_g && d_g[c]) UH_CHECK(hipMemcpyAsync(d_g[c], cur + (1 + c) * f->fs, b, hipMemcpyDeviceToDevice, st));
    if (d_v && d_v[c]) UH_CHECK(hipMemcpyAsync(d_v[c], cur + (4 + c) * f->fs, b, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

int uammd_icmc_get_bottom_ghost(uammd_icmc *h, float *d_density, float *const d_v[3], float *const d_g[3], void *stream) {
  if (!h) { set_last_error("uammd_icmc_get_bottom_ghost: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (!icmc_walls(f)) { set_last_error("uammd_icmc_get_bottom_ghost: this fluid has no walls, so no ghost plane"); return -2; }
  hipStream_t st = (hipStream_t)stream;
  const size_t b = sizeof(float) * f->off;
  if (d_density) UH_CHECK(hipMemcpyAsync(d_density, f->cur, b, hipMemcpyDeviceToDevice, st));
  for (int c = 0; c < 3; ++c) {
    if (d_g && d_g[c]) UH_CHECK(hipMemcpyAsync(d_g[c], f->cur + (1 + c) * f->fs, b, hipMemcpyDeviceToDevice, st));
    if (d_v && d_v[c]) UH_CHECK(hipMemcpyAsync(d_v[c], f->cur + (4 + c) * f->fs, b, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

int uammd_icmc_get_collocated_velocity(uammd_icmc *h, float *d_vx, float *d_vy, float *d_vz, void *stream) {
  if (!h || !d_vx || !d_vy || !d_vz) { set_last_error("uammd_icmc_get_collocated_velocity: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (icmc_walls(f))
    hipLaunchKernelGGL(k_icmc_collocate<true>, icmc_blocks(f->nc), dim3(256), 0, (hipStream_t)stream, (const float *)f->cur, f->grid.cellDim,
                       d_vx, d_vy, d_vz);
  else
    hipLaunchKernelGGL(k_icmc_collocate<false>, icmc_blocks(f->nc), dim3(256), 0, (hipStream_t)stream, (const float *)f->cur, f->grid.cellDim,
                       d_vx, d_vy, d_vz);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_icmc_get_noise(uammd_icmc *h, unsigned int step, float *d_out, void *stream) {
  if (!h || !d_out) { set_last_error("uammd_icmc_get_noise: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  const uammd_icmc_parameters &p = f->par;
  hipLaunchKernelGGL(k_icmc_noise, icmc_blocks(f->nc), dim3(256), 0, (hipStream_t)stream, (float2 *)d_out, (int)f->nc, p.seed, step, p.dt,
                     p.shearViscosity, p.bulkViscosity, p.temperature, f->grid.cellSize.x * f->grid.cellSize.y * f->grid.cellSize.z);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_icmc_set_noise(uammd_icmc *h, const float *d_noise, void *stream) {
  if (!h) { set_last_error("uammd_icmc_set_noise: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  f->injected = d_noise != nullptr;
  if (d_noise) UH_CHECK(hipMemcpyAsync(f->noise.ptr, d_noise, sizeof(float) * 12 * f->nc, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// forwardPositionsToHalfStep (:216-227): q^n is kept, d_pos becomes q^{n+1/2}
int uammd_icmc_predictor(uammd_icmc *h, float *d_pos, int N, void *stream) {
  if (!h || (N > 0 && !d_pos)) { set_last_error("uammd_icmc_predictor: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (N <= 0) return 0;
  if (int e = f->posOld.reserve(sizeof(float4) * (size_t)N)) return e;
  const float *v = f->cur + 4 * f->fs + f->off;
  if (icmc_walls(f))
    hipLaunchKernelGGL(k_icmc_advect<true>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (float4 *)d_pos, (float4 *)f->posOld.ptr, true,
                       v, (const float *)nullptr, f->nc, N, f->grid, 1.0f / f->grid.cellSize.x, f->par.dt);
  else
    hipLaunchKernelGGL(k_icmc_advect<false>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (float4 *)d_pos, (float4 *)f->posOld.ptr, true,
                       v, (const float *)nullptr, f->nc, N, f->grid, 1.0f / f->grid.cellSize.x, f->par.dt);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_icmc_set_wall_velocities(uammd_icmc *h, const float bottom[2], const float top[2]) {
  if (!h || !bottom || !top) { set_last_error("uammd_icmc_set_wall_velocities: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (f->par.walls != UAMMD_ICMC_WALLS_BUILTIN) { set_last_error("uammd_icmc_set_wall_velocities: this fluid has no built-in walls"); return -2; }
  f->wallU[0] = bottom[0]; f->wallU[1] = bottom[1]; f->wallU[2] = top[0]; f->wallU[3] = top[1];
  return 0;
}

// spreadCurrentParticleForcesToFluid (:176-185) and computeStochasticTensor (:124-142): the forcing and the noise of this step
int uammd_icmc_fluid_begin(uammd_icmc *h, const float *d_pos, const float *d_force, int N, void *stream) {
  if (!h || (N > 0 && !d_pos)) { set_last_error("uammd_icmc_fluid_begin: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (N > 0 && f->posOld.cap < sizeof(float4) * (size_t)N) {
    set_last_error("uammd_icmc_fluid_begin: uammd_icmc_predictor has not run for these %d particles", N);
    return -1;
  }
  f->stage = -1;  // a step that failed half way is abandoned: the fluid at n is untouched until uammd_icmc_fluid_end
  f->target = nullptr;
  hipStream_t st = (hipStream_t)stream;
  const uammd_icmc_parameters &p = f->par;
  const size_t nc = f->nc;
  const float invh = 1.0f / f->grid.cellSize.x;
  f->forcingNow = nullptr;
  if (d_force && N > 0) {
    UH_CHECK(hipMemsetAsync(f->forcing.ptr, 0, sizeof(float) * 3 * f->fs, st));
    if (icmc_walls(f))
      hipLaunchKernelGGL(k_icmc_spread<true>, dim3((N + 3) / 4), dim3(256), 0, st, (const float4 *)d_pos, (const float4 *)d_force,
                         (float *)f->forcing.ptr + f->off, nc, N, f->grid, invh);
    else
      hipLaunchKernelGGL(k_icmc_spread<false>, dim3((N + 3) / 4), dim3(256), 0, st, (const float4 *)d_pos, (const float4 *)d_force,
                         (float *)f->forcing.ptr, nc, N, f->grid, invh);
    f->forcingNow = (const float *)f->forcing.ptr;
  }
  f->noiseNow = nullptr;
  if (p.temperature > 0) {
    if (!f->injected)
      hipLaunchKernelGGL(k_icmc_noise, icmc_blocks(nc), dim3(256), 0, st, (float2 *)f->noise.ptr, (int)nc, p.seed, f->step, p.dt,
                         p.shearViscosity, p.bulkViscosity, p.temperature, f->grid.cellSize.x * f->grid.cellSize.y * f->grid.cellSize.z);
    f->noiseNow = (const float2 *)f->noise.ptr;
  }
  UH_CHECK(hipGetLastError());
  f->stage = 0;
  return 0;
}

// rungeKuttaSubStepD of sub-stage s = 0, 1, 2, in this order: density and momentum into the next scratch level
int uammd_icmc_substage(uammd_icmc *h, int s, void *stream) {
  if (!h) { set_last_error("uammd_icmc_substage: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (s < 0 || s > 2 || s != f->stage) { set_last_error("uammd_icmc_substage: sub-stage %d where %d is due", s, f->stage); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const uammd_icmc_parameters &p = f->par;
  const int3 n = f->grid.cellDim;
  // RungeKutta3 (FluidSolver.cuh:108-131) and the noise combinations (Fluctuations.cuh:28-35)
  const float sqrt3 = (float)sqrt(3.0);
  const float A[3] = {0.0f, 3.0f / 4.0f, 1.0f / 3.0f}, B[3] = {1.0f, 0.25f, 2.0f / 3.0f}, nB[3] = {-sqrt3, sqrt3, 0.0f};
  const float *tb[3] = {f->cur, f->tmp1, f->tmp2};
  float *tc[3] = {f->tmp1, f->tmp2, f->tmp1};
  const real3f ih = f->grid.invCellSize;
  const ICMCCoef k{A[s], B[s], nB[s], p.dt, p.shearViscosity, p.bulkViscosity + p.shearViscosity / 3.0f, p.speedOfSound};
  const dim3 g = icmc_blocks(f->nc), b(256);
  const float2 *W = f->noiseNow;
  const float *forcing = f->forcingNow;
  if (icmc_walls(f)) {  // uammd_icmc_validate admits walls at temperature 0 only
    if (W) { set_last_error("uammd_icmc_substage: noise with walls"); return -1; }
    hipLaunchKernelGGL((k_icmc_substage<false, true>), g, b, 0, st, (const float *)f->cur, tb[s], tc[s], n, f->grid.cellSize, ih, k, W, forcing);
  } else if (W) {
    hipLaunchKernelGGL((k_icmc_substage<true, false>), g, b, 0, st, (const float *)f->cur, tb[s], tc[s], n, f->grid.cellSize, ih, k, W, forcing);
  } else {
    hipLaunchKernelGGL((k_icmc_substage<false, false>), g, b, 0, st, (const float *)f->cur, tb[s], tc[s], n, f->grid.cellSize, ih, k, W, forcing);
  }
  UH_CHECK(hipGetLastError());
  f->target = tc[s];
  f->stage = s + 1;
  return 0;
}

// fillGhostCells (:97-102) with the built-in rule and the wall velocities set last: on the level of the sub-stage under way, between
// steps on the fluid itself.  Without walls there are no ghost planes: nothing to do.
int uammd_icmc_ghost_fill(uammd_icmc *h, void *stream) {
  if (!h) { set_last_error("uammd_icmc_ghost_fill: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (!icmc_walls(f)) return 0;
  if (f->par.walls == UAMMD_ICMC_WALLS_EXTERNAL) {
    set_last_error("uammd_icmc_ghost_fill: external walls are filled by the caller (uammd_icmc_wall_planes_get / _put)");
    return -2;
  }
  icmc_launch_ghost_fill(f, f->stage > 0 ? f->target : f->cur, (hipStream_t)stream);
  UH_CHECK(hipGetLastError());
  return 0;
}

// External walls: the packed planes of the level a ghost fill would act on (k_icmc_pack_wall_planes for the layout), and back.
int uammd_icmc_wall_planes_get(uammd_icmc *h, float **d_planes, void *stream) {
  if (!h || !d_planes) { set_last_error("uammd_icmc_wall_planes_get: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (f->par.walls != UAMMD_ICMC_WALLS_EXTERNAL) { set_last_error("uammd_icmc_wall_planes_get: this fluid has no external walls"); return -2; }
  const int3 n = f->grid.cellDim;
  hipLaunchKernelGGL(k_icmc_pack_wall_planes, icmc_blocks((size_t)(n.x + 2) * (n.y + 2)), dim3(256), 0, (hipStream_t)stream,
                     (const float *)(f->stage > 0 ? f->target : f->cur), (float *)f->planes.ptr, n);
  UH_CHECK(hipGetLastError());
  *d_planes = (float *)f->planes.ptr;
  return 0;
}

int uammd_icmc_wall_planes_put(uammd_icmc *h, void *stream) {
  if (!h) { set_last_error("uammd_icmc_wall_planes_put: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (f->par.walls != UAMMD_ICMC_WALLS_EXTERNAL) { set_last_error("uammd_icmc_wall_planes_put: this fluid has no external walls"); return -2; }
  const int3 n = f->grid.cellDim;
  hipLaunchKernelGGL(k_icmc_unpack_wall_planes, icmc_blocks((size_t)n.x * n.y), dim3(256), 0, (hipStream_t)stream,
                     f->stage > 0 ? f->target : f->cur, (const float *)f->planes.ptr, n);
  UH_CHECK(hipGetLastError());
  return 0;
}

// velocityToMomentumD on the fluid itself: for external walls, between the caller's two fills after uammd_icmc_set_fluid
int uammd_icmc_velocity_to_momentum(uammd_icmc *h, void *stream) {
  if (!h) { set_last_error("uammd_icmc_velocity_to_momentum: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (icmc_walls(f)) hipLaunchKernelGGL((k_icmc_velocity<false, true>), icmc_blocks(f->nc), dim3(256), 0, (hipStream_t)stream, f->cur, f->grid.cellDim);
  else hipLaunchKernelGGL((k_icmc_velocity<false, false>), icmc_blocks(f->nc), dim3(256), 0, (hipStream_t)stream, f->cur, f->grid.cellDim);
  UH_CHECK(hipGetLastError());
  return 0;
}

// momentumToVelocityD on the level the last sub-stage wrote
int uammd_icmc_substage_velocity(uammd_icmc *h, void *stream) {
  if (!h) { set_last_error("uammd_icmc_substage_velocity: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (f->stage < 1) { set_last_error("uammd_icmc_substage_velocity: no sub-stage has run"); return -1; }
  const dim3 g = icmc_blocks(f->nc), b(256);
  if (icmc_walls(f)) hipLaunchKernelGGL((k_icmc_velocity<true, true>), g, b, 0, (hipStream_t)stream, f->target, f->grid.cellDim);
  else hipLaunchKernelGGL((k_icmc_velocity<true, false>), g, b, 0, (hipStream_t)stream, f->target, f->grid.cellDim);
  UH_CHECK(hipGetLastError());
  return 0;
}

// the fluid of the third sub-stage becomes the fluid at n + 1, forwardPositionsToNextStep (:231-244).  Counts the step.
int uammd_icmc_fluid_end(uammd_icmc *h, float *d_pos, int N, void *stream) {
  if (!h || (N > 0 && !d_pos)) { set_last_error("uammd_icmc_fluid_end: null argument"); return -1; }
  ICMCState *f = reinterpret_cast<ICMCState *>(h);
  if (f->stage != 3) { set_last_error("uammd_icmc_fluid_end: %d of the three sub-stages have run", f->stage < 0 ? 0 : f->stage); return -1; }
  hipStream_t st = (hipStream_t)stream;
  std::swap(f->cur, f->tmp1);  // tmp1 now holds the fluid at n: the corrector needs v^n
  f->stage = -1;
  f->target = nullptr;
  if (N > 0) {
    const float *vn = f->tmp1 + 4 * f->fs + f->off, *vnew = f->cur + 4 * f->fs + f->off;
    const float invh = 1.0f / f->grid.cellSize.x;
    if (icmc_walls(f))
      hipLaunchKernelGGL(k_icmc_advect<true>, dim3((N + 3) / 4), dim3(256), 0, st, (float4 *)d_pos, (float4 *)f->posOld.ptr, false, vn, vnew,
                         f->nc, N, f->grid, invh, f->par.dt);
    else
      hipLaunchKernelGGL(k_icmc_advect<false>, dim3((N + 3) / 4), dim3(256), 0, st, (float4 *)d_pos, (float4 *)f->posOld.ptr, false, vn, vnew,
                         f->nc, N, f->grid, invh, f->par.dt);
  }
  f->step++;
  UH_CHECK(hipGetLastError());
  return 0;
}

// spreadCurrentParticleForcesToFluid + forwardFluidDensityAndVelocityToNextStep + forwardPositionsToNextStep (:246-257).
// d_pos holds q^{n+1/2}, d_force real4[N] the forces there (NULL: none).  Counts the step.  The composition of the pieces above; with
// walls the wall velocities stay what they are through the step.
int uammd_icmc_fluid_and_corrector(uammd_icmc *h, float *d_pos, const float *d_force, int N, void *stream) {
  if (!h || (N > 0 && !d_pos)) { set_last_error("uammd_icmc_fluid_and_corrector: null argument"); return -1; }
  if (N > 0 && reinterpret_cast<ICMCState *>(h)->posOld.cap < sizeof(float4) * (size_t)N) {
    set_last_error("uammd_icmc_fluid_and_corrector: uammd_icmc_predictor has not run for these %d particles", N);
    return -1;
  }
  if (reinterpret_cast<ICMCState *>(h)->par.walls == UAMMD_ICMC_WALLS_EXTERNAL) {
    set_last_error("uammd_icmc_fluid_and_corrector: with external walls the caller issues the pieces, its own fills between them");
    return -2;
  }
  if (int e = uammd_icmc_fluid_begin(h, d_pos, d_force, N, stream)) return e;
  for (int s = 0; s < 3; ++s) {
    if (int e = uammd_icmc_substage(h, s, stream)) return e;
    if (int e = uammd_icmc_ghost_fill(h, stream)) return e;
    if (int e = uammd_icmc_substage_velocity(h, stream)) return e;
    if (int e = uammd_icmc_ghost_fill(h, stream)) return e;
  }
  return uammd_icmc_fluid_end(h, d_pos, N, stream);
}

}  // extern "C"
