/* libuammd_hip — C-ABI of the MI355X (gfx950) implementation of UAMMD's data-parallel hot path.
 *
 * UAMMD is a header-only C++/CUDA template library: there is no reference FFI.  The entry points
 * below are what a C ABI for its two hot paths binds — one per reference call site that crosses
 * host->device — each citing the reference interface it replaces (paths relative to
 * /root/reference/src).  The UAMMD-shaped C++14 headers in include/uammd/ call these.
 *
 * Conventions
 *   - every pointer argument named d_* is a DEVICE pointer (HBM), everything else is host memory;
 *   - `real4` arrays are plain float[4*N] (x,y,z,w; w = particle type for positions), `real3`
 *     arrays are float[3*N], matching UAMMD's default `real=float` build (global/defines.h:33-44);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     with respect to the host unless stated;
 *   - return value: 0 = ok, non-zero = error; uammd_hip_last_error() returns the message
 *     (thread local).  The C++ headers turn non-zero into the exceptions UAMMD throws
 *     (utils/debugTools.h:20-64).
 */
#ifndef UAMMD_HIP_H
#define UAMMD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAMMD_HIP_ABI_VERSION 1

int uammd_hip_abi_version(void);
const char *uammd_hip_last_error(void);
/* number of visible devices / select one (System::System --device N, System/System.h:128-139) */
int uammd_hip_device_count(int *count);
int uammd_hip_set_device(int device);

/* ------------------------------------------------------------------------------------------------
 * Path A — neighbour search.  Replaces CellList / CellListBase / ParticleSorter:
 *   Interactor/NeighbourList/CellList.cuh:100-126,149-182        (createUpdateGrid, update, transverseList)
 *   Interactor/NeighbourList/CellList/CellListBase.cuh:124-172   (update, getCellList, CellListData)
 *   utils/ParticleSorter.cuh:156-164,178-187,243-274,303-321     (hash, stable radix sort, reorder)
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_celllist uammd_celllist; /* opaque; owns index/hash/sortPos/cellStart/cellEnd */

/* POD view of the list handed to kernels — field-for-field CellListBase::CellListData
 * (CellListBase.cuh:145-160) plus the sorted Morton keys. */
typedef struct {
  const unsigned int *d_cellStart; /* first sorted index of the cell + VALID_CELL; < VALID_CELL = empty */
  const int *d_cellEnd;            /* one past the last sorted index of the cell */
  const float *d_sortPos;          /* real4[N], positions in sorted (Morton cell) order */
  const int *d_groupIndex;         /* sorted index -> index in the input array */
  const unsigned int *d_sortHash;  /* Morton key of each sorted particle */
  int cellDim[3];
  float boxSize[3];
  int periodic[3];
  unsigned int VALID_CELL;
  int numberParticles;
} uammd_celllist_data;

int uammd_celllist_create(uammd_celllist **out);
int uammd_celllist_destroy(uammd_celllist *h);

/* Host logic of CellList::createUpdateGrid (CellList.cuh:100-126): cellDim = int3(L/cutOff) by C
 * truncation in float, any dimension with <= 3 cells collapses to 1, an infinite dimension becomes
 * 64*cutOff and non periodic. */
int uammd_celllist_create_grid(const float L[3], const int periodic[3], const float cutOff[3], int cellDim_out[3],
                               float L_out[3], int periodic_out[3]);

/* CellListBase::update(pos, N, grid, st): hash -> stable sort on [0,maxbit) -> reorder -> cell
 * tables.  d_pos is real4[N]. */
int uammd_celllist_update(uammd_celllist *h, const float *d_pos, int numberParticles, const float L[3],
                          const int periodic[3], const int cellDim[3], void *stream);
int uammd_celllist_get(uammd_celllist *h, uammd_celllist_data *out);
/* NaN positions or particles outside a non-periodic box: the reference raises a device flag (CellListBase.cuh:82-85) and, in
 * UAMMD_DEBUG builds only, synchronises and throws overflow_error("CellList encountered NaN positions") inside every update
 * (:258-264); its release builds carry on silently.  Here the build kernels raise a flag in host-mapped memory and the NEXT
 * uammd_celllist_update / _get on the handle fails with that message (no per-step synchronisation).
 * uammd_celllist_check_errors synchronises `stream` and reports at once; option "strict_errors" = 1 makes every update do so
 * (the reference's debug behaviour); option "report_errors" = 0 gives the reference's release behaviour. */
int uammd_celllist_check_errors(uammd_celllist *h, void *stream);
/* Measurement hook (no reference counterpart): while enabled, every LJ traversal of this list that runs as ONE kernel (the TILE
 * kernels) is launched through hipExtLaunchKernel with a start / stop event pair attached to its own dispatch, and
 * uammd_lj_profile_read returns the summed kernel time (ms) and the number of launches since the enable.  bench.py derives
 * roofline.achieved from it: every launch of the timed region, no events between kernels. */
/* Slab decomposition (new design, the reference is single GPU): the positions a rank sends to its two z neighbours —
 * d_outUp[k] = pos[idxUp[k]] + (0, 0, dzUp), d_outDown[k] = pos[idxDown[k]] + (0, 0, dzDown) — in one launch. */
int uammd_halo_pack(const float *d_pos, const int *d_idxUp, int nUp, const int *d_idxDown, int nDown, float dzUp, float dzDown,
                    float *d_outUp, float *d_outDown, void *stream);
/* The decomposed step with GronbechJensen's first half step (Integrator/VerletNVT/GronbechJensen.cu:86-116) folded into the two
 * kernels that read the positions anyway, instead of a launch of its own before the exchange:
 *   uammd_halo_pack_gj1: the half step of every LISTED row (noise keyed by d_keys[row], the global particle id; force zeroed), then
 *     uammd_halo_pack of the new positions.  The up and down lists must be disjoint (a slab wider than two reaches): a row in both
 *     would take the half step twice.
 *   uammd_celllist_update_gj1: uammd_celllist_update over rows [0, numberParticles) = owned + ghosts, the half step applied, as the
 *     rows are loaded, to the owned rows [0, numberOwned) with d_skip[row] == 0 (d_skip: one byte per owned row, the listed rows —
 *     uammd_slab_refresh_lj writes it; NULL: nobody is skipped).  The list is built from the new positions; forces of the
 *     integrated rows are zeroed.  Bit-identical to uammd_verletnvt_gj_keyed(1, ...) followed by the plain calls. */
int uammd_halo_pack_gj1(float *d_pos, float *d_vel, float *d_force, const float *d_mass, float defaultMass, const int *d_keys,
                        const int *d_idxUp, int nUp, const int *d_idxDown, int nDown, float dzUp, float dzDown, float *d_outUp,
                        float *d_outDown, float dt, float friction, int is2D, float noiseAmplitude, unsigned int stepNum, unsigned int seed,
                        void *stream);
int uammd_celllist_update_gj1(uammd_celllist *h, float *d_pos, int numberParticles, const float L[3], const int periodic[3],
                              const int cellDim[3], float *d_vel, float *d_force, const float *d_mass, float defaultMass,
                              const int *d_keys, const unsigned char *d_skip, int numberOwned, float dt, float friction, int is2D,
                              float noiseAmplitude, unsigned int stepNum, unsigned int seed, void *stream);
/* The bookkeeping of a membership refresh of the slab decomposition (uammd_amd/csrc/slab.hip):
 *   uammd_slab_select: ASCENDING indices of the rows with z >= zUp (d_idxUp) and with z < zDown (d_idxDown), their numbers in
 *     d_counts[0..1] (device memory; the caller reads them to size its messages); d_workspace: uammd_slab_select_workspace(n) bytes;
 *   uammd_slab_pack_rows: the listed rows as 8 floats {x, y, z + dz, w, vx, vy, vz, id} for the neighbour above / below;
 *   uammd_slab_unpack_rows: arrivals (8-float rows, those from below first) into the holes the leavers make, arrivals in excess
 *     appended at row n, and when fewer arrive than leave the staying rows of the tail moved into the open holes: afterwards the
 *     first n - nUp - nDown + nArrive rows are the owned particles.  d_holes: nUp + nDown ints of scratch;
 *   uammd_slab_max_displacement: atomicMax of |pos - ref| over the rows into *d_max (a float the caller zeroes). */
int uammd_slab_select_workspace(int n, size_t *bytes);
int uammd_slab_select(const float *d_pos, int n, float zUp, float zDown, int *d_idxUp, int *d_idxDown, int *d_counts, void *d_workspace,
                      void *stream);
int uammd_slab_pack_rows(const float *d_pos, const float *d_vel, const int *d_ids, const int *d_idxUp, int nUp, const int *d_idxDown,
                         int nDown, float dzUp, float dzDown, float *d_outUp, float *d_outDown, void *stream);
int uammd_slab_unpack_rows(float *d_pos, float *d_vel, int *d_ids, int n, const int *d_idxUp, int nUp, const int *d_idxDown, int nDown,
                           const float *d_arrivals, int nArrive, int *d_holes, void *stream);
int uammd_slab_max_displacement(const float *d_pos, const float *d_ref, int n, float *d_max, void *stream);
/* two segments of `count` floats in one launch: dst0 += src0, dst1 += src1 (the halo planes of the spread grid folded into the owned
 * planes, FCM slab decomposition) and dst0 = src0, dst1 = src1 (the planes received before the gather); a segment's dst and src
 * must not overlap */
int uammd_slab_add2(float *d_dst0, const float *d_src0, float *d_dst1, const float *d_src1, size_t count, void *stream);
int uammd_slab_copy2(float *d_dst0, const float *d_src0, float *d_dst1, const float *d_src1, size_t count, void *stream);
/* Measurement hook (no reference counterpart): counters of the tile traversal (AUTO / TILE) of this list.  The call first copies the
 * counters accumulated so far into out (nullable; zeros when the hook was off) — out[0] = workgroups (2 x 2 x 2-cell bricks) that took
 * the in-kernel dense-brick fallback, out[1] = bricks launched, out[2..3] reserved, out[4..15] = phase times of diagnostic builds
 * (-DUAMMD_TILE_TIMELINE, tools/variants_tile.sh; zeros otherwise) —, then zeroes them and turns the hook on (enable != 0) or off.
 * tests/test_gpu_bench_state.py asserts with it that the melted state bench.py times runs on the main path. */
int uammd_lj_tile_stats(uammd_celllist *h, int enable, unsigned int out[16], void *stream);
int uammd_lj_profile_enable(uammd_celllist *h, int enable);
int uammd_lj_profile_read(uammd_celllist *h, double *total_ms, long long *launches);
/* options: "force_radix" = 1 makes the build use the stable radix sort path (test hook); "num_owned" = n marks the
 * particles with input index >= n as ghosts of a domain decomposition: they are neighbours of the others but the LJ
 * traversal computes nothing for them (n < 0 turns it off) */
int uammd_celllist_set_option(uammd_celllist *h, const char *name, int value);
/* library-wide tunables (measurement switches; an unknown name or a bad value is an error):
 *   "bonded_baseline" = 1        uammd_bonded_sum runs the reference-shaped kernel (thread per particle, AoS entries, id2index looked up
 *                                on every step, BondedForces.cu:191-246); 0 (default) the CSR kernels
 *   "bonded_wave_threshold" = T  rows with more than T entries take the wave-per-row shape (default 32)
 *   "mc_baseline" = 1            uammd_mc_anderson_step runs the reference-shaped kernel (thread per cell, Anderson.cu:302-349); 0 (default)
 *                                the wave-per-cell kernel with the neighbourhood staged in LDS
 *   "mc_stage_capacity" = R      rows of LDS a wave of that kernel stages (default 512, 0..960) */
int uammd_hip_set_tunable(const char *name, int value);

/* ParticleSorter::updateOrderWithCustomHash + applyCurrentOrder building blocks
 * (ParticleSorter.cuh:118-135,178-187): stable sort of (key,value) on key bits [0,end_bit) and a
 * gather out[i] = in[index[i]] for 4/8/12/16/24/32-byte elements.  Used by ParticleData::sortParticles. */
int uammd_sort_pairs(unsigned int *d_keys, int *d_values, int n, int end_bit, void *stream);
int uammd_gather(const void *d_in, const int *d_index, void *d_out, int n, int elem_bytes, void *stream);
/* the inverse: out[index[i]] = in[i] (distinct indices).  What assigning through pg->getPropertyIterator(prop) does in the reference
 * (ParticleData/ParticleGroup.cuh:473-496): the modules that solve on the gathered rows of a proper subgroup write positions back with it. */
int uammd_scatter(const void *d_in, const int *d_index, void *d_out, int n, int elem_bytes, void *stream);
/* out[i] = (float) in[i]: the single-precision image of a DOUBLE_PRECISION ParticleData's positions, whose cell list orders
 * ParticleData::sortParticles (ParticleData.cuh:492-522: a memory-locality order) */
int uammd_convert_f64_to_f32(const double *d_in, float *d_out, size_t count, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path A — traversal with the Lennard-Jones Transverser.  Replaces
 *   CellList::transverseList<Radial<LJFunctor>::Transverser>      Interactor/NeighbourList/CellList.cuh:165-182
 *   NeighbourList_ns::transverseWithNeighbourContainer            Interactor/NeighbourList/common.cuh:10-34
 *   Radial<LJFunctor>::Transverser::compute/set                   Interactor/Potential/RadialPotential.cuh:107-127
 *   NBody::transverse (small-box fallback, PairForces.cu:49-53)   Interactor/NBodyBase.cuh:46-159
 * ---------------------------------------------------------------------------------------------- */
/* LJFunctor::PairParameters (Potential/Potential.cuh:31-35) */
typedef struct { float cutOff2, sigma2, epsilonDivSigma2, shift; } uammd_lj_pair_parameters;
/* LJFunctor::processPairParameters (Potential/Potential.cuh:66-82), host */
int uammd_lj_process_pair_parameters(float cutOff, float sigma, float epsilon, int shift, uammd_lj_pair_parameters *out);
/* A list caches what it needs of the table (largest cut-off; whether sigma = epsilon = 1) keyed by the table's device address.  After
 * rewriting a table in place — or uploading a new one into memory a previous table occupied — call this before the next traversal: every
 * list reads its table again (one small device-to-host copy).  Potential::LJ::setPotParameters between steps (legal in the reference,
 * Potential.cuh:60-82) goes through here in both host layers. */
int uammd_lj_table_changed(void);

/* flags for `algo` */
#define UAMMD_LJ_ALGO_AUTO 0    /* the kernel measured fastest for the grid: TILE where the grid allows it (forces to rounding level, the
                                   north star's stated tolerance), else EXACT */
#define UAMMD_LJ_ALGO_TILE 8    /* wave per pair of x-adjacent cells, 32 x 32 distance tiles on the matrix pipe (f32 MFMA), hits re-evaluated
                                   with the reference's arithmetic: same pairs, sums in another order (rounding-level differences) */
#define UAMMD_LJ_ALGO_TILE1 10  /* TILE with one wave per pair of cells and a private 4 x 3 x 3-cell halo (TILE = a workgroup of four waves per
                                   2 x 2 x 2 brick of cells sharing one staged halo); same results as TILE up to summation order */
#define UAMMD_LJ_ALGO_EXACT 9   /* the fastest kernel that keeps the reference's summation order, bit-identical to GENERAL
                                   (RING_HALF where the grid allows it, else RING, else GENERAL) */
#define UAMMD_LJ_ALGO_GENERAL 1 /* thread-per-particle walk of the 27 cells (any grid) */
#define UAMMD_LJ_ALGO_RING 6    /* GENERAL with a ring FIFO: a drain takes a few pairs from every lane (bit-identical to GENERAL) */
#define UAMMD_LJ_ALGO_RING_HALF 7 /* RING + half-precision superset prefilter, two candidates per load (bit-identical to GENERAL) */

/* d_paramTable: ntypes*ntypes PairParameters indexed [ti + ntypes*tj] (ParameterHandler.cuh:17-37);
 * d_force real4[·], d_energy/d_virial real[·] are nullable and ACCUMULATED into at the particle's
 * index in the input array (Transverser::set does +=); d_globalIndex (group->global, nullable). */
int uammd_lj_transverse_celllist(uammd_celllist *h, const uammd_lj_pair_parameters *d_paramTable, int ntypes,
                                 const float boxL[3], const int boxPeriodic[3], float *d_force, float *d_energy,
                                 float *d_virial, const int *d_globalIndex, int algo, void *stream);
int uammd_lj_transverse_nbody(const float *d_pos, int numberParticles, const uammd_lj_pair_parameters *d_paramTable,
                              int ntypes, const float boxL[3], const int boxPeriodic[3], float *d_force,
                              float *d_energy, float *d_virial, const int *d_globalIndex, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Potential::DPD (Interactor/Potential/DPD.cuh): PairForces<Potential::DPD> on the cell list and on all pairs
 *
 * Replaces DPD_impl::ForceTransverser::compute / getInfo / set (DPD.cuh:121-158) run by CellList::transverseList
 * (PairForces.cu:55-68) and by NBody (PairForces.cu:49-53).  Per pair within the cut-off, in float:
 *   rij = pbc(ri - rj), vij = vi - vj, wr = 1 - r/cutOff
 *   F_i += (A wr / r  -  gamma wr^2 (rij . vij) / r^2  +  xi sigma sqrt(gamma) wr / r) rij
 *   xi = Saru(min(i,j) + numberParticlesKey max(i,j), seed, step).gf(0, 1).x      (key in unsigned arithmetic, seed and step
 *                                                                                   truncated to 32 bits as Saru's constructor does)
 * i, j are the particles' indices in d_vel / d_force (what getInfo receives); with d_globalIndex (group -> global, nullable) the list's
 * or the loop's member t is particle d_globalIndex[t].  sigma = sqrt(2 kT) / sqrt(dt) is the caller's (DPD.cuh:69); numberParticlesKey
 * is pd->getNumParticles() (DPD.cuh:167).  d_vel is real3[.] in input order; d_force real4[.] is ACCUMULATED at the particle's index
 * (set does +=, DPD.cuh:156-158).  Every particle sums its own pairs in a fixed order: no atomics, the same bits run to run.
 * Energy and virial are not defined for DPD (DPD.cuh:171-180).
 * The list variant gathers {velocity, index} into list order once per call, into scratch memory the handle owns (allocated on the
 * first call of a size); it needs a list whose cells are at least cutOff wide (uammd_celllist_create_grid with that cut-off). */
int uammd_dpd_transverse_celllist(uammd_celllist *h, const float *d_vel, const float boxL[3], const int boxPeriodic[3], float cutOff,
                                  float A, float gamma, float sigma, unsigned long long seed, unsigned long long step,
                                  int numberParticlesKey, float *d_force, const int *d_globalIndex, void *stream);
/* d_pos is the UN-gathered real4 array: member t reads d_pos[d_globalIndex[t]] (NBody over the group's iterators) */
int uammd_dpd_transverse_nbody(const float *d_pos, const float *d_vel, int numberParticles, const float boxL[3], const int boxPeriodic[3],
                               float cutOff, float A, float gamma, float sigma, unsigned long long seed, unsigned long long step,
                               int numberParticlesKey, float *d_force, const int *d_globalIndex, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path A — Verlet list.  Replaces
 *   VerletListBase::{update,needsRebuild,getVerletList,setCutOffMultiplier,forceNextUpdate,getNumberOfStepsSinceLastUpdate}
 *                                                               Interactor/NeighbourList/VerletList/VerletListBase.cuh:73-199
 *   BasicNeighbourListBase::{update,getBasicNeighbourList}      Interactor/NeighbourList/BasicList/BasicListBase.cuh:76-215
 *   fillBasicNeighbourList (K7), checkMaximumDrift (K8)         BasicListBase.cuh:41-75, VerletListBase.cuh:55-69
 *   VerletList::transverseList<Radial<LJFunctor>::Transverser>  Interactor/NeighbourList/VerletList.cuh:138-155
 * The list is built on the cell list of the STORED positions with cut-off multiplier*cutOff (1.08), capacity 32 per
 * particle growing by 32; entry k of sorted particle i is d_neighbourList[k*particleStride + i]; the particle itself is
 * one of its neighbours (r2 = 0 <= cutOff2, as in the reference).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_verletlist uammd_verletlist;
/* BasicNeighbourListBase::BasicNeighbourListData (BasicListBase.cuh:144-152), with VerletListBase's current sortPos */
typedef struct {
  const int *d_neighbourList;
  const int *d_numberNeighbours;
  const float *d_sortPos;   /* real4[N]: CURRENT positions in the order of the last build */
  const int *d_groupIndex;  /* sorted index -> index in the input array */
  int particleStride;       /* = numberParticles */
  int maxNeighboursPerParticle;
  int numberParticles;
} uammd_verletlist_data;
int uammd_verletlist_create(uammd_verletlist **out);
int uammd_verletlist_destroy(uammd_verletlist *h);
/* VerletListBase::update(pos, N, box, cutOff, st): rebuilds if forced / box, cutOff or N changed / some particle drifted
 * >= (multiplier*cutOff - cutOff)/2 from its stored position (one 4-byte read-back, as in the reference), then refreshes
 * sortPos.  *rebuilt (nullable) tells whether the list was rebuilt. */
int uammd_verletlist_update(uammd_verletlist *h, const float *d_pos, int numberParticles, const float L[3],
                            const int periodic[3], float cutOff, void *stream, int *rebuilt);
int uammd_verletlist_force_next_update(uammd_verletlist *h);
int uammd_verletlist_set_cutoff_multiplier(uammd_verletlist *h, float newMultiplier);
int uammd_verletlist_get_steps_since_last_update(uammd_verletlist *h, int *steps);
int uammd_verletlist_get(uammd_verletlist *h, uammd_verletlist_data *out);
int uammd_lj_transverse_verletlist(uammd_verletlist *h, const uammd_lj_pair_parameters *d_paramTable, int ntypes,
                                   const float boxL[3], const int boxPeriodic[3], float *d_force, float *d_energy,
                                   float *d_virial, const int *d_globalIndex, void *stream);

/* ------------------------------------------------------------------------------------------------
 * SPH (Interactor/SPH.cuh): the density and the force sums of smoothed particle hydrodynamics over an UPDATED Verlet list
 *
 * Replaces SPH::sum (SPH.cu:178-215): DensityTransverser, the Density2Pressure transform and ForceTransverser, with the M4 cubic spline
 * of SPH/Kernel.cuh.  In float, with h = support, m = d_mass or 1, rij = pbc(rj - ri), r = |rij|, vij = vj - vi and j over the list
 * entries of i (i itself included: the self term counts in the density):
 *   W: q = r / h;      0 if q >= 2;  ((2 - q)^3 - [q <= 1] 4 (1 - q)^3) / (4 pi h^3)
 *   G: q = r (1 / h);  0 if q >= 2;  c (3 r - 4 h) rij if q <= 1, else c (2 h - r)^2 rij;  c = -3 / (4 pi h^6)   (as the reference writes it)
 *   rho_i = sum_j m_j W;  P_i = gasStiffness (rho_i - restDensity)
 *   F_i += sum_j m_i m_j (P_i / rho_i^2 + P_j / rho_j^2 - viscosity (vij . rij) / (r^2 + 0.001 h^2)) G
 * The list must have been updated (uammd_verletlist_update) with a cut-off of at least 2 support on the positions of this state; -3
 * otherwise.  d_vel real3[N] and d_mass real[N] (nullable) are in the order of the positions the list was updated with; d_force real4[N]
 * is ACCUMULATED at the particle's index, .w untouched; d_density / d_pressure real[N] (nullable) receive rho and P in the same order.
 * Two launches, one lane per particle, no atomics: the same bits run to run.  Scratch rows ({velocity, P / rho^2} and mass in list
 * order) belong to the handle and are allocated on the first call of a size.  No energy or virial is defined.  -1 on null arguments or
 * support <= 0; an empty list returns 0. */
int uammd_sph_sum_verletlist(uammd_verletlist *h, const float *d_vel /*real3[N]*/, const float *d_mass /*nullable*/,
                             const float boxL[3], const int boxPeriodic[3], float support, float viscosity,
                             float gasStiffness, float restDensity, float *d_force /*real4[N], accumulated*/,
                             float *d_density /*nullable out, particle order*/, float *d_pressure /*nullable out*/,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Monte Carlo NVT on a checkerboard (Integrator/MonteCarlo/NVT/Anderson.cuh, Anderson.cu) with Potential::LJ
 *
 * Replaces one MC_NVT::Anderson<LJ>::forwardTime minus its host draws, which stay with the caller so that every front end takes them
 * from its System::rng() in the reference's order: origin = float(uniform3(-1, 1) * 0.5 L.x) (z = 0 in 2D), then the Fisher-Yates order
 * of the 8 (4 in 2D) subgrids, entry g standing for the offset (g & 1, g >> 1 & 1, g >> 2 & 1).  The handle owns the cell list, the
 * sorted unshifted positions and two counters per cell.  One step, all on `stream`, no host synchronisation:
 *   list of d_pos + origin on cellDim (as given: no <= 3-cells collapse);  sortPos = list.sortPos + (-origin);
 *   per subgrid in subgridOrder, per non-empty cell of it with Saru(seed, step, icell), triesPerCell times:
 *     tried[icell]++;  i = min(int(f() * nincell), nincell - 1);  new = old + jumpSize * (2 f() - 1) per axis (three draws; z kept in 2D);
 *     getCell(new + origin) != cell: next try without another draw;  dH = sum_j u(new, j) - sum_j u(old, j) over the 27 (9) cells with
 *     u the LJ pair energy of the table (0 at r2 == 0, the moved particle standing for itself);  accept if f() <= min(1, exp(-beta dH)):
 *     sortPos[i] = new, accepted[icell]++
 *   d_pos[groupIndex[k]] = sortPos[k]     (a particle that did not move ends at (p + o) - o in float)
 * u is the whole pair energy, 2 x the per-particle half that the traversals accumulate.  Positions move by plain
 * float multiply and add (no contraction).  No atomics: each kernel is deterministic (the same state gives the same bits run to run).  The
 * two kernels sum dH in different orders, so a try within rounding of its threshold can be decided differently by one and the other.  cellDim: every extent
 * even, x and y >= 4, z == 1 (2D) or >= 4; numberSubgrids 4 for z == 1, else 8; -1 otherwise and on null arguments.  Cells past the edge
 * of a non-periodic axis are skipped.  Tunables (uammd_hip_set_tunable): "mc_baseline" = 1 runs the reference-shaped kernel (thread per
 * cell, global memory) instead of the wave-per-cell kernel with the neighbourhood staged in LDS; "mc_stage_capacity" = rows of LDS per
 * wave (default 512, at most 960): a cell whose neighbourhood holds more is walked in global memory by the same wave.
 *
 * uammd_mc_anderson_counters: the sums of tried and accepted over the cells since the last reset (synchronises the stream); reset != 0
 * zeroes them behind the read.  uammd_mc_anderson_cell_counters: the per-cell values into host arrays of cellDim.x * y * z (tests).
 * uammd_mc_anderson_energy (Anderson::sumEnergy, Anderson.cu:377-400): rebuilds the list on d_pos with origin 0 and writes the
 * per-particle LJ energy (half of every pair, as uammd_lj_transverse_celllist) into d_energy[N], zeroed first. */
typedef struct uammd_mc_anderson uammd_mc_anderson;
int uammd_mc_anderson_create(uammd_mc_anderson **out);
int uammd_mc_anderson_destroy(uammd_mc_anderson *h);
int uammd_mc_anderson_step(uammd_mc_anderson *h, float *d_pos /*real4[N], updated*/, int numberParticles, const float boxL[3],
                           const int boxPeriodic[3], const int cellDim[3], const float origin[3], const int *subgridOrder /*host*/,
                           int numberSubgrids /*8 or 4*/, int triesPerCell, float beta, float jumpSize, unsigned int step,
                           unsigned int seed, const uammd_lj_pair_parameters *d_paramTable, int ntypes, void *stream);
int uammd_mc_anderson_counters(uammd_mc_anderson *h, unsigned long long *tried, unsigned long long *accepted, int reset, void *stream);
int uammd_mc_anderson_cell_counters(uammd_mc_anderson *h, unsigned int *tried /*host, ncells*/, unsigned int *accepted, void *stream);
int uammd_mc_anderson_energy(uammd_mc_anderson *h, const float *d_pos, int numberParticles, const float boxL[3],
                             const int boxPeriodic[3], const int cellDim[3], const uammd_lj_pair_parameters *d_paramTable, int ntypes,
                             float *d_energy, void *stream);

/* Force biased Monte Carlo (Integrator/MonteCarlo/ForceBiased.cuh): the Metropolized Euler-Maruyama scheme (MALA), the integrator's own
 * part of a trial; forces and per-particle energies come from the caller's interactors.  Single precision arrays,
 * every sum and the acceptance exponent in double.  The handle owns the stored configuration X, F(X) (real4[N]) and E_X, the per-block
 * partial sums and the result record (device, mirrored in pinned host memory).
 *
 * uammd_mc_forcebiased_begin: adopts d_pos, d_force as X, F(X) and E_X = sum_i d_energy[i] (the reference's firstStep after its
 *   interactors ran).  An energy that is not finite, or past FLT_MAX, becomes FLT_MAX (here and in decide).
 * uammd_mc_forcebiased_propose: one kernel reading the STORED arrays (a rejected trial needs no restore before the next proposal): per
 *   particle i, rng = Saru(seed, step, i), xi.xy = rng.gf(0, 1), xi.z = rng.gf(0, 1).x; in float, without contraction,
 *     d_pos[i].c = X[i].c + (F[i].c * stepSize + amp * xi.c),  amp = (float)sqrt(2.0 * stepSize / beta),  d_pos[i].w = X[i].w
 *   d_noise, when not null, receives (xi.x, xi.y, xi.z, 0) per particle (test hook).
 * uammd_mc_forcebiased_decide: after the caller has zeroed force and energy and run its interactors on Y = d_pos.  With h = stepSize:
 *     E_Y = sum energy[i],  T_XY = sum |Y - X - h F(X)|^2 / (4 h),  T_YX = sum |X - Y - h F(Y)|^2 / (4 h)   (terms and sums in double)
 *     exponent = -beta ((E_Y - E_X) + (T_YX - T_XY)),  accepted = Z < exp(exponent)   (a NaN exponent rejects)
 *   accepted: stored <- (d_pos, d_force), E_X <- E_Y;  rejected: (d_pos, d_force) <- stored.  Two kernels, no atomics, no synchronisation:
 *   the same inputs give the same bits on every run.
 * uammd_mc_forcebiased_result: the one host synchronisation of a trial: the decision of the last decide (1 after begin) and
 *   out = {E_X before, E_Y, T_XY, T_YX, exponent, current energy}.
 * uammd_mc_forcebiased_stored: copies the stored X, F(X) into device arrays (test hook).
 * Null arguments, numberParticles <= 0 or other than what begin adopted, stepSize <= 0 and beta < 0 return -1 with a message, decided on
 * the host before anything touches the device. */
typedef struct uammd_mc_forcebiased uammd_mc_forcebiased;
int uammd_mc_forcebiased_create(uammd_mc_forcebiased **out);
int uammd_mc_forcebiased_destroy(uammd_mc_forcebiased *h);
int uammd_mc_forcebiased_begin(uammd_mc_forcebiased *h, const float *d_pos /*real4[N]*/, const float *d_force /*real4[N]*/,
                               const float *d_energy /*real[N]*/, int numberParticles, void *stream);
int uammd_mc_forcebiased_propose(uammd_mc_forcebiased *h, float *d_pos /*real4[N], written*/, int numberParticles, float stepSize, float beta,
                                 unsigned int step, unsigned int seed, float *d_noise /*nullable, real4[N]*/, void *stream);
int uammd_mc_forcebiased_decide(uammd_mc_forcebiased *h, float *d_pos, float *d_force, const float *d_energy, int numberParticles,
                                float stepSize, float beta, double Z, void *stream);
int uammd_mc_forcebiased_result(uammd_mc_forcebiased *h, int *accepted, double out[6], void *stream);
int uammd_mc_forcebiased_stored(uammd_mc_forcebiased *h, float *d_pos_out, float *d_force_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Integrator kernels.  Replace
 *   VerletNVT::GronbechJensen_ns::integrateGPU<step>   Integrator/VerletNVT/GronbechJensen.cu:28-62
 *   VerletNVT::Basic_ns::integrateGPU<step>            Integrator/VerletNVT/Basic.cu:86-114
 *   VerletNVT::Basic_ns::initialVelocities             Integrator/VerletNVT/Basic.cu:12-29
 *   BD::EulerMaruyama_ns::integrateGPU                 Integrator/BrownianDynamics.cu:119-144
 *   BDHI::FCM_ns::integrateEulerMaruyamaD              Integrator/BDHI/BDHI_FCM.cu:67-92
 * d_vel is real3[N]; d_mass nullable (defaultMass > 0 wins); d_index = ParticleGroup index iterator
 * (nullable = identity).
 * ---------------------------------------------------------------------------------------------- */
int uammd_verletnvt_gj(int step, float *d_pos, float *d_vel, float *d_force, const float *d_mass, float defaultMass,
                       const int *d_index, int numberParticles, float dt, float friction, int is2D,
                       float noiseAmplitude, unsigned int stepNum, unsigned int seed, void *stream);
/* The same step with the thermostat's random stream of thread t keyed by d_noiseKey[t] instead of t (nullable: then exactly
 * uammd_verletnvt_gj).  New design for the domain-decomposed drivers (the reference is single GPU): the key is the particle's GLOBAL id,
 * so a particle draws the same kicks whichever rank and row holds it — the trajectory of an N-rank run does not depend on the
 * decomposition or on the order migration leaves the rows in, and slabs are not correlated through equal row numbers. */
int uammd_verletnvt_gj_keyed(int step, float *d_pos, float *d_vel, float *d_force, const float *d_mass, float defaultMass,
                             const int *d_index, const int *d_noiseKey, int numberParticles, float dt, float friction, int is2D,
                             float noiseAmplitude, unsigned int stepNum, unsigned int seed, void *stream);
/* One whole VerletNVT::GronbechJensen::forwardTime (Integrator/VerletNVT/GronbechJensen.cu:88-115) whose only interactor is
 * PairForces<Potential::LJ, CellList> on every particle (Interactor/PairForces.cu:43-78), fused into five launches: the first half step
 * rides in the cell list's hash kernel, the second in the traversal's store.  Bit-identical to the sequence
 *   uammd_verletnvt_gj(1) -> uammd_celllist_update(updateL, updatePeriodic, cellDim) -> uammd_lj_transverse_celllist(algo) -> uammd_verletnvt_gj(2)
 * which is also what runs where the list does not take the aggregated counting build or the tile kernel.  d_force holds f(t) on entry
 * (the integrator's first step computes it the plain way) and f(t + dt) on return; updateL / updatePeriodic / cellDim as
 * uammd_celllist_create_grid returns them for (boxL, boxPeriodic, cut-off). */
int uammd_verletnvt_gj_lj_step(uammd_celllist *h, float *d_pos, float *d_vel, float *d_force, const float *d_mass, float defaultMass,
                               int numberParticles, const float boxL[3], const int boxPeriodic[3], const float updateL[3],
                               const int updatePeriodic[3], const int cellDim[3], const uammd_lj_pair_parameters *d_paramTable,
                               int ntypes, float dt, float friction, int is2D, float noiseAmplitude, unsigned int stepNum,
                               unsigned int seed, int algo, void *stream);

/* The second half of that fusion alone, for lists with ghosts (the domain-decomposed drivers exchange the halo between the first half
 * step and the list build, so only the traversal's store can carry a half step): PairForces<Potential::LJ, CellList>::sum on the owned
 * rows (option num_owned of the list) with GronbechJensen's second half step (GronbechJensen.cu:28-62) applied to them in the store.
 * d_force must be zero on the owned rows on entry.  Same bits as uammd_lj_transverse_celllist -> uammd_verletnvt_gj(2) on the owned rows. */
int uammd_lj_transverse_celllist_gj2(uammd_celllist *h, const uammd_lj_pair_parameters *d_paramTable, int ntypes, const float boxL[3],
                                     const int boxPeriodic[3], float *d_force, float *d_vel, const float *d_mass, float defaultMass,
                                     float dt, int is2D, int algo, void *stream);

int uammd_verletnvt_basic(int step, float *d_pos, float *d_vel, float *d_force, const float *d_mass,
                          float defaultMass, const int *d_index, int numberParticles, float dt, float friction,
                          int is2D, float noiseAmplitude, unsigned int stepNum, unsigned int seed, void *stream);
/* VerletNVE_ns::integrateGPU<step> (Integrator/VerletNVE.cu:64-85): vel += force / m * dt / 2, vel.z = 0 if is2D, and in step 1
 * pos += vel * dt.  m = d_mass[i] whenever d_mass is given, else defaultMass (:76).  The forces are read only: zeroing them between the
 * two halves is the caller's (VerletNVE::resetForces, :152-158).  d_index (group -> global, nullable). */
int uammd_verletnve(int step, float *d_pos, float *d_vel, const float *d_force, const float *d_mass, float defaultMass,
                    const int *d_index, int numberParticles, float dt, int is2D, void *stream);
int uammd_verletnvt_initial_velocities(float *d_vel, const int *d_index, float velAmplitude, int is2D,
                                       int numberParticles, unsigned int seed, void *stream);
/* VerletNVT::Basic::sumKineticEnergy (VerletNVT/Basic.cu:173-207): energy[i] += 0.5 m |v|^2 (Integrator::sumEnergy) */
int uammd_sum_kinetic_energy(const float *d_vel, float *d_energy, const float *d_mass, float defaultMass,
                             const int *d_index, int numberParticles, void *stream);
int uammd_bd_euler_maruyama(float *d_pos, const int *d_index, const float *d_force, const float K[9],
                            float selfMobility, const float *d_radius, float dt, int is2D, float temperature,
                            int numberParticles, unsigned int stepNum, unsigned int seed, void *stream);
int uammd_fcm_euler_maruyama(float *d_pos, const int *d_index, const float *d_linearVelocity, int numberParticles,
                             float dt, void *stream);
/* The other schemes of Integrator/BrownianDynamics.cuh:121-183 / .cu:160-387 — BD::MidPoint (two calls per step: substep 0 after the
 * first force evaluation, 1 after the second; d_aux real4[N] keeps the step's starting positions), BD::AdamsBashforth (d_aux real4[N] = the
 * previous step's forces in group order) and BD::Leimkuhler (d_originalIndex = ParticleData::getIdOrderedIndices, nullable = identity).
 * Arguments as uammd_bd_euler_maruyama.  MidPoint and AdamsBashforth key their noise by the GROUP index, as the reference does. */
#define UAMMD_BD_MIDPOINT 1
#define UAMMD_BD_ADAMS_BASHFORTH 2
#define UAMMD_BD_LEIMKUHLER 3
int uammd_bd_scheme_step(int scheme, int substep, float *d_pos, float *d_aux, const int *d_index, const int *d_originalIndex, const float *d_force,
                         const float K[9], float selfMobility, const float *d_radius, float dt, int is2D, float temperature, int numberParticles,
                         unsigned int stepNum, unsigned int seed, void *stream);
/* ... and the four schemes with real = double (d_pos, d_aux, d_force double4[N], d_radius double[N]; UAMMD_BD_EULER_MARUYAMA is the scheme of
 * uammd_bd_euler_maruyama).  The draws are float Gaussians, as in the reference's double build (Saru::gf). */
#define UAMMD_BD_EULER_MARUYAMA 0
int uammd_bd_scheme_step_f64(int scheme, int substep, double *d_pos, double *d_aux, const int *d_index, const int *d_originalIndex,
                             const double *d_force, const double K[9], double selfMobility, const double *d_radius, double dt, int is2D,
                             double temperature, int numberParticles, unsigned int stepNum, unsigned int seed, void *stream);
/* BDHI::EulerMaruyama_ns::integrateGPUD (Integrator/BDHI/BDHI_EulerMaruyama.cu:82-113): pos += dt (K pos + MF) + sqrt2Tdt BdW;
 * d_MF, d_BdW real3[N] (d_BdW nullable), K row-major 3x3 (nullable) */
int uammd_bdhi_euler_maruyama(float *d_pos, const int *d_index, const float *d_MF, const float *d_BdW, const float K[9],
                              int numberParticles, float sqrt2Tdt, float dt, int is2D, void *stream);
int uammd_fill_zero(void *d_ptr, size_t bytes, void *stream);
/* thrust::fill(pg->getPropertyIterator(prop), ..., T()) — zero element index[i] (elem_bytes each, a multiple of 4) for i < n */
int uammd_fill_zero_indexed(void *d_ptr, const int *d_index, int n, int elem_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path B — Immersed Boundary spreading / interpolation on a regular grid.  Replaces
 *   IBM<Kernel,Grid,LinearIndex3D>::spread / gather     misc/IBM.cuh:99-203
 *   IBM_ns::particles2GridD / grid2ParticlesDTPP        misc/IBM.cu:83-147, :164-235
 * A user-defined window functor cannot cross a C ABI; the windows UAMMD ships are selected by `kind`
 * (a user-defined window is device code: it is compiled by hipcc with the user's
 * translation unit, as in the reference; include/uammd/device/Transverser.hip.hpp is that path for Transversers).
 * ---------------------------------------------------------------------------------------------- */
#define UAMMD_IBM_KERNEL_GAUSSIAN 0 /* prefactor*exp(tau r^2), 0 for r >= rmax   misc/IBM_kernels.cuh:28-40, BDHI/FCM/FCM_kernels.cuh:22-58 */
#define UAMMD_IBM_KERNEL_PESKIN3 1  /* Peskin::threePoint                          misc/IBM_kernels.cuh:115-137 */
#define UAMMD_IBM_KERNEL_PESKIN4 2  /* Peskin::fourPoint                           misc/IBM_kernels.cuh:140-160 */
#define UAMMD_IBM_KERNEL_CONSTANT 3 /* phi = 1 (test/misc/ibm/test_ibm_regular.cu:11-14) */
#define UAMMD_IBM_KERNEL_BARNETT_MAGLAND 4 /* exp(beta(sqrt(1-(r/(a alpha))^2)-1))/(a norm); prefactor=1/norm, tau=beta, rmax=alpha,
                                             invh[0]=a (a LENGTH, not an inverse)  misc/IBM_kernels.cuh:82-112, FCM_kernels.cuh:82-155 */
#define UAMMD_IBM_KERNEL_SIXPOINT 5 /* GaussianFlexible::sixPoint, support 6, invh = 1/h        misc/IBM_kernels.cuh:162-236 */
#define UAMMD_IBM_KERNEL_GAUSS2D 6         /* BDHI2D_ns::Gaussian: prefactor*exp(tau r^2) in x and y, 1 in z   Integrator/Hydro/BDHI_quasi2D.cuh:112-132 */
#define UAMMD_IBM_KERNEL_GAUSS2D_DRIFT_X 7 /* GaussianThermalDrift<0>: the same times r along x                  BDHI_quasi2D.cuh:134-153 */
#define UAMMD_IBM_KERNEL_GAUSS2D_DRIFT_Y 8 /* GaussianThermalDrift<1> */
typedef struct {
  int kind;
  int support[3];
  float prefactor, tau, rmax; /* Gaussian */
  float invh[3];              /* Peskin: 1/h per axis */
} uammd_ibm_kernel;

/* FCM_ns::Kernels::Gaussian(h, tolerance) (BDHI/FCM/FCM_kernels.cuh:22-58), host: fills `out` and returns the
 * effective hydrodynamic radius a = h*u(tol)*sqrt(pi) in *a_eff. */
int uammd_fcm_gaussian_kernel(float h, float tolerance, uammd_ibm_kernel *out, float *a_eff);
/* IBM_kernels::BarnettMagland(alpha, beta) (misc/IBM_kernels.cuh:82-112), host: alpha = half support in length
 * units of `lengthUnit`, norm by the reference's 20000-interval Simpson rule.  `support` = nodes per axis (the
 * reference leaves it to the caller's getSupport).  lengthUnit = 1 is the plain window; the FCM wrapper
 * FCM_ns::Kernels::BarnettMagland(h, tol) is (alpha = w/2, beta = 3.6 w, support = w, lengthUnit = h),
 * BDHI/FCM/FCM_kernels.cuh:82-155. */
int uammd_ibm_barnett_magland_kernel(float alpha, float beta, int support, float lengthUnit, uammd_ibm_kernel *out);
/* Kernel::adviseGridSize (FCM_kernels.cuh:47-50), host */
float uammd_fcm_advise_grid_size(float hydrodynamicRadius, float tolerance);

/* d_pos: float[posStride*N] (xyz first; posStride 3 or 4).  d_quantity / d_out: float[ncomp*N].  d_grid:
 * float[ncomp * nxStride*ny*nz], components interleaved, node index i + nxStride*(j + ny*k)
 * (LinearIndex3D(nxStride, ny, nz)).  spread ADDS into the grid, gather ADDS into d_out (as the reference).
 * ncomp is 1 or 3.  A grid with cellDim[2] == 1 is treated as 2D (IBM.cuh:182-194). */
int uammd_ibm_spread(const float *d_pos, int posStride, const float *d_quantity, int ncomp, int numberParticles,
                     const float L[3], const int periodic[3], const int cellDim[3], int nxStride,
                     const uammd_ibm_kernel *kernel, float *d_grid, void *stream);
int uammd_ibm_gather(const float *d_pos, int posStride, float *d_out, int ncomp, int numberParticles,
                     const float L[3], const int periodic[3], const int cellDim[3], int nxStride,
                     const uammd_ibm_kernel *kernel, const float *d_grid, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path B — Force Coupling Method (triply periodic Stokes).  Replaces
 *   FCM_impl<Gaussian,GaussianTorque>  ctor / computeHydrodynamicDisplacements / getSelfMobility
 *                                       Integrator/BDHI/FCM/FCM_impl.cuh:56-129, :652-693
 *   spreadForces, forwardTransform, convolveFourier, addBrownianNoise, inverseTransform, interpolateVelocity
 *                                       FCM_impl.cuh:245-262, :293-304, :399-411, :514-581
 *   BDHI::FCM::computeMF                Integrator/BDHI/BDHI_FCM.cuh:131-142
 * The solver owns its grids (3 planar padded real grids transformed in place by rocFFT).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_fcm uammd_fcm;
typedef struct {
  float boxSize[3];
  int cells[3];
  float viscosity;
  unsigned int seed;        /* FCM_impl::Parameters::seed (0 is NOT replaced here: the C++ header draws it) */
  uammd_ibm_kernel kernel;  /* spreading window (uammd_fcm_gaussian_kernel) */
  float hydrodynamicRadius; /* reported by getHydrodynamicRadius / used by getSelfMobility */
} uammd_fcm_parameters;
int uammd_fcm_create(const uammd_fcm_parameters *par, uammd_fcm **out);
int uammd_fcm_destroy(uammd_fcm *h);
/* FCM_impl::computeHydrodynamicDisplacements(pos, force, torque=nullptr, N, T, prefactor, st):
 * d_linearVelocity real3[N] is OVERWRITTEN with M F + prefactor*sqrt(2 T) M^{1/2} dW.  d_force may be NULL
 * (noise only).  Every call with temperature > 0 advances the noise stream (the reference's static seed2). */
int uammd_fcm_displacements(uammd_fcm *h, const float *d_pos, const float *d_force, int numberParticles,
                            float temperature, float prefactor, float *d_linearVelocity, void *stream);
/* BDHI::FCMIntegrator::forwardTime without torques (Integrator/BDHI/BDHI_FCM.cu:94-119 -> computeHydrodynamicDisplacements, then
 * integrateEulerMaruyamaD :67-92): the same velocities as uammd_fcm_displacements, then pos[i].xyz += v_i dt IN PLACE (the fma of
 * uammd_fcm_euler_maruyama: identical positions) by a kernel that also bins the positions it writes, so that the next call can
 * start at the tile scan.  d_linearVelocity real3[N] receives v; it may be NULL (a buffer of the handle is used).
 * flags: UAMMD_FCM_STEP_POSITIONS_KEPT = d_pos holds exactly what the previous uammd_fcm_step_euler_maruyama call on this handle left
 * there (same array, size and stream; nobody asked for write access in between: ParticleData::getPosWriteRequestedSignal is how the
 * host layers know) -> that call's binning is used instead of a binning pass.  Without the flag nothing is assumed.
 * option "bin_ahead" = 0 switches the binning ahead off. */
#define UAMMD_FCM_STEP_POSITIONS_KEPT 1
int uammd_fcm_step_euler_maruyama(uammd_fcm *h, float *d_pos, const float *d_force, int numberParticles, float temperature,
                                  float prefactor, float dt, float *d_linearVelocity, int flags, void *stream);
/* Hasimoto-corrected self mobility, FCM_impl::getSelfMobility (FCM_impl.cuh:102-119), host */
double uammd_fcm_self_mobility(double hydrodynamicRadius, double viscosity, double Lx);
/* noise call counter (the reference's process-global `static uint seed2`, FCM_impl.cuh:517; per handle here) */
int uammd_fcm_get_seed2(uammd_fcm *h, unsigned int *seed2);
int uammd_fcm_set_seed2(uammd_fcm *h, unsigned int seed2);
/* test hooks: run the pipeline up to the Fourier-space kernel (stage = 1; stage = 0 is the full solve) and copy the
 * Fourier grid out as complex3[nz*ny*(nx/2+1)] = {x.re,x.im,y.re,y.im,z.re,z.im} (the reference's layout) */
int uammd_fcm_displacements_staged(uammd_fcm *h, const float *d_pos, const float *d_force, int numberParticles,
                                   float temperature, float prefactor, float *d_linearVelocity, int stage,
                                   void *stream);
int uammd_fcm_export_fourier(uammd_fcm *h, float *d_out6, void *stream);
/* test hook: the solver's own batched 3-D real FFT (the LDS pipeline that serves axis lengths 2^a 3^b 5^c 7^d 11^e, x even in [16, 512],
 * y in [2, 256], z in [2, 512]) and nothing else, in place on d_grid in the solver's layout: three planar components, each nz * ny rows
 * of 2 * (nx / 2 + 1) floats = nx / 2 + 1 complex.  Needs no handle and builds no rocFFT plans; returns an error (and touches nothing)
 * for any other grid.  Both directions are unnormalised.
 *   UAMMD_FCM_FFT_FORWARD_XY   the x and y passes: the R2C over (y, x) of every plane
 *   UAMMD_FCM_FFT_FORWARD_XYZ  ... then the forward z pass of the fused z kernel, without its operator and its inverse: the 3-D R2C
 *   UAMMD_FCM_FFT_INVERSE_ZYX  the inverse z pass of the fused z kernel alone, the inverse y pass and the C2R rows: the 3-D C2R, into
 *                              `target`: the planar real grids in place, or d_inter as the gather's float4 grid [nz][ny][nx] = (x, y, z, 0)
 *                              or its packed form of three floats per node
 * info (may be null): [0] = UAMMD_FCM_FFT_PATH_* of the forward x / y passes (-1 for the inverse), [1] = nodes per workgroup of the z pass
 * (0 when it did not run) */
#define UAMMD_FCM_FFT_FORWARD_XY 0
#define UAMMD_FCM_FFT_FORWARD_XYZ 1
#define UAMMD_FCM_FFT_INVERSE_ZYX 2
#define UAMMD_FCM_FFT_TARGET_PLANAR 0
#define UAMMD_FCM_FFT_TARGET_FLOAT4 1
#define UAMMD_FCM_FFT_TARGET_PACKED 2
#define UAMMD_FCM_FFT_PATH_ROWS_LINES 0  /* row kernel + y lines */
#define UAMMD_FCM_FFT_PATH_PLANE_P2 1    /* a whole plane per workgroup, power-of-two instantiation */
#define UAMMD_FCM_FFT_PATH_PLANE_DENSE 2 /* ... mixed radix, two planes per compute unit */
#define UAMMD_FCM_FFT_PATH_PLANE_LARGE 3 /* ... mixed radix, one plane per compute unit */
int uammd_fcm_fft_probe(const int cells[3], int mode, int target, float *d_grid, float *d_inter, int *info, void *stream);
/* "atomic_spread" = 1 forces the one-wave-per-particle atomic spread/gather instead of the tile-owned kernels;
 * "tile_gather" = 1 selects the LDS-staged gather (supports <= 6; slower than the default at 24 particles per tile) */
int uammd_fcm_set_option(uammd_fcm *h, const char *name, int value);
/* diagnostics, host-side bookkeeping only: how the last solve on this handle got its stencils (out[0]) and what the update of the last
 * uammd_fcm_step_euler_maruyama did for the next solve (out[1]; UAMMD_FCM_UPDATE_NO_STEP when the last call was a plain solve) */
#define UAMMD_FCM_PREP_NONE 0            /* no solve yet, or the atomic spread: nothing is prepared */
#define UAMMD_FCM_PREP_SORTED_FRESH 1    /* k_fcm_bin_count -> k_fcm_tile_scan -> k_fcm_prepare */
#define UAMMD_FCM_PREP_SORTED_CLAIMED 2  /* ... from the binning that the previous step's k_fcm_update_bin left */
#define UAMMD_FCM_PREP_SLOTS_CLAIMED 3   /* the slot layout that the previous step's k_fcm_step_prep left */
#define UAMMD_FCM_PREP_SLOTS_SELF 4      /* the slot layout prepared on the spot from the entry order of an earlier solve */
#define UAMMD_FCM_UPDATE_NO_STEP 0
#define UAMMD_FCM_UPDATE_STEP_PREP 1     /* k_fcm_step_prep: the next solve's slot layout */
#define UAMMD_FCM_UPDATE_BIN 2           /* k_fcm_update_bin that also bins the positions it writes */
#define UAMMD_FCM_UPDATE_PLAIN 3         /* k_fcm_update_bin without binning */
int uammd_fcm_last_preparation(uammd_fcm *h, int out[2]);
/* test hook: the two ends of a solve on their own, through the solve's own launch code.  Grids are the solver's three planar real
 * grids, [3][nz][ny][2 * (nx / 2 + 1)] floats.  To the handle's bookkeeping either stage is a completed solve (the noise counter stays).
 *   UAMMD_FCM_PROBE_SPREAD  prepares the stencils as a solve of (d_pos, d_force) would — UAMMD_FCM_PROBE_POSITIONS_KEPT as the flag of
 *                           uammd_fcm_step_euler_maruyama —, runs the spread the handle would launch, stops in front of the forward FFT
 *                           and copies the grids to d_grid.  UAMMD_FCM_PROBE_NAN_FILL: the grids hold quiet NaNs before a tile-owned
 *                           spread, which has no memset and must write every node (the atomic spread keeps its memset).
 *   UAMMD_FCM_PROBE_GATHER  prepares the stencils of d_pos without forces and runs the gather that the handle's options select on the
 *                           caller's d_grid (interleaved by k_fcm_interleave where the gather reads a float4 grid) into
 *                           d_linearVelocity real3[N].  UAMMD_FCM_PROBE_PACKED: the caller supplies d_inter instead, [nz][ny][nx] nodes
 *                           of three floats as UAMMD_FCM_FFT_TARGET_PACKED writes them, and the packed k_fcm_gather_inter reads it (in
 *                           a solve: grids above 128 MB).  UAMMD_FCM_PROBE_ACCUMULATE: the output is added to, this call only.
 * info[UAMMD_FCM_PROBE_INFO_LEN] (may be null) says what ran:
 *   spread  [0] stage, [1] UAMMD_FCM_PREP_*, [2] 1 tile-owned / 0 atomic, [3] waves per tile W, [4] slot layout, [5] compile-time edge E,
 *           [6] speculative first round, [7..9] tile edge per axis, [10] list entries per chunk, [11] slot capacity, [12] lanes per
 *           particle and [13] UAMMD_FCM_PREP_KERNEL_* of the preparation kernel this call launched, noted at its launch
 *   gather  [0] stage, [1] UAMMD_FCM_PREP_*, [2] UAMMD_FCM_GATHER_*, [3] R (inter) or S (half), [4] particles per wave P, [5] SZMAX,
 *           [6] packed, [7] accumulate, [12], [13] as above */
#define UAMMD_FCM_PROBE_SPREAD 1
#define UAMMD_FCM_PROBE_GATHER 2
#define UAMMD_FCM_PROBE_POSITIONS_KEPT 1
#define UAMMD_FCM_PROBE_NAN_FILL 2
#define UAMMD_FCM_PROBE_PACKED 4
#define UAMMD_FCM_PROBE_ACCUMULATE 8
/* (not a flag) the length of info */
#define UAMMD_FCM_PROBE_INFO_LEN 16
#define UAMMD_FCM_PREP_KERNEL_NONE 0      /* the atomic spread, or a slot layout claimed from the previous step */
#define UAMMD_FCM_PREP_KERNEL_PREPARE 1   /* k_fcm_prepare */
#define UAMMD_FCM_PREP_KERNEL_STEP_PREP 2 /* k_fcm_step_prep without the update */
#define UAMMD_FCM_GATHER_ATOMIC 0 /* k_fcm_ibm */
#define UAMMD_FCM_GATHER_TILE 1   /* k_fcm_gather_tile */
#define UAMMD_FCM_GATHER_PREP 2   /* k_fcm_gather_prep */
#define UAMMD_FCM_GATHER_INTER 3  /* k_fcm_gather_inter<R, P, packed> */
#define UAMMD_FCM_GATHER_COL 4    /* k_fcm_gather_col<P, SZMAX> */
#define UAMMD_FCM_GATHER_HALF 5   /* k_fcm_gather_half<S, SZMAX> */
int uammd_fcm_probe(uammd_fcm *h, int stage, const float *d_pos, const float *d_force, int numberParticles, int flags, float *d_grid,
                    float *d_inter, float *d_linearVelocity, int *info, void *stream);

/* Torques and rotation (FCM_impl.cuh:306-358, :590-649; FCM_kernels.cuh:60-80; BDHI_FCM.cu:67-92).  The torque window is
 * GaussianTorque(width = a/(6 sqrt(pi))^(1/3), h, tolerance); torques are spread with it, half their curl is added to the
 * Fourier forces, and the angular velocity is half the curl of the Fourier velocity interpolated with the same window.
 * d_dir: orientation quaternions real4 (n, vx, vy, vz), nullable. */
int uammd_fcm_torque_gaussian_kernel(float hydrodynamicRadius, float h, float tolerance, uammd_ibm_kernel *out);
int uammd_fcm_set_torque_kernel(uammd_fcm *h, const uammd_ibm_kernel *kernelTorque);
int uammd_fcm_displacements_torque(uammd_fcm *h, const float *d_pos, const float *d_force, const float *d_torque,
                                   int numberParticles, float temperature, float prefactor, float *d_linearVelocity,
                                   float *d_angularVelocity, void *stream);
int uammd_fcm_euler_maruyama_dir(float *d_pos, float *d_dir, const int *d_index, const float *d_linearVelocity,
                                 const float *d_angularVelocity, int numberParticles, float dt, void *stream);

/* ------------------------------------------------------------------------------------------------
 * BDHI::Cholesky — dense open-boundary RPY mobility with an explicit Cholesky factor (the other half of
 * test/BDHI/Lanczos_Cholesky).  Replaces Integrator/BDHI/BDHI_Cholesky.cu:
 *   setup_step (fillMobilityRPYD :34-80, :158-178)   computeMF (symv, :196-233)   computeBdW (potrf + trmv, :235-262)
 * d_index: group index iterator (nullable = all particles); d_radius nullable when hydrodynamicRadius > 0.
 * rocSOLVER / rocBLAS are loaded on first use (not load-time dependencies of this library).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_bdhi_cholesky uammd_bdhi_cholesky;
int uammd_bdhi_cholesky_create(int numberParticles, float viscosity, float hydrodynamicRadius, uammd_bdhi_cholesky **out);
int uammd_bdhi_cholesky_destroy(uammd_bdhi_cholesky *h);
int uammd_bdhi_cholesky_setup_step(uammd_bdhi_cholesky *h, const float *d_pos, const int *d_index, const float *d_radius, void *stream);
/* d_force real4[N]; d_MF real3[N] (overwritten).  Rebuilds M first if computeBdW consumed it, like the reference. */
int uammd_bdhi_cholesky_mf(uammd_bdhi_cholesky *h, const float *d_pos, const float *d_force, const int *d_index, const float *d_radius,
                           float *d_MF, void *stream);
/* d_BdW real3[N]: N(0,1) draws on entry (the reference's cuRAND stream is unpinned third party), B dW on exit. */
int uammd_bdhi_cholesky_bdw(uammd_bdhi_cholesky *h, const float *d_pos, const int *d_index, const float *d_radius, float *d_BdW,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * BDHI::True2D / BDHI::Quasi2D — hydrodynamics of particles confined to a plane.  Replaces
 *   BDHI2D<HydroKernel>::BDHI2D / forwardTime      Integrator/Hydro/BDHI_quasi2D.cuh:155-257, .cu:18-205
 *   spreadThermalDrift / spreadParticleForces / forceFourier2Vel / fourierBrownianNoise / interpolateVelocities /
 *   updateParticlePositions                         .cu:234-541
 * cells[0] <= 0: grid from h = 0.8 a (the tolerance parameter is ignored by the reference, .cu:143-145).
 * ---------------------------------------------------------------------------------------------- */
#define UAMMD_BDHI2D_TRUE2D 0  /* BDHI2D_ns::True2D:  f_k = 0, g_k = 1/k^4                       BDHI_quasi2D.cuh:83-93 */
#define UAMMD_BDHI2D_QUASI2D 1 /* BDHI2D_ns::Quasi2D: 3D Stokes integrated over z, thermal drift  BDHI_quasi2D.cuh:95-110 */
typedef struct uammd_bdhi2d uammd_bdhi2d;
typedef struct {
  float boxSize[2];
  float hydrodynamicRadius, viscosity, temperature, dt;
  int cells[2];
  unsigned int seed; /* the reference draws it from System::rng().next32() */
  int kernel;        /* UAMMD_BDHI2D_* */
} uammd_bdhi2d_parameters;
/* Errors (-2) carry the reference's messages ("Invalid box", "Invalid hydrodynamic radius"). */
int uammd_bdhi2d_create(const uammd_bdhi2d_parameters *par, uammd_bdhi2d **out, int cells[2], int *support);
int uammd_bdhi2d_destroy(uammd_bdhi2d *h);
/* One step's particle velocities (through interpolateVelocities): d_pos real4[N]; d_force real4[N] or NULL when no
 * Interactor is attached (then only the thermal terms act); d_vel real2[N], overwritten. */
int uammd_bdhi2d_velocities(uammd_bdhi2d *h, const float *d_pos, const float *d_force, int numberParticles, float *d_vel,
                            void *stream);
/* pos += make_real4(vel * dt) */
int uammd_bdhi2d_update_positions(float *d_pos, const float *d_vel, int numberParticles, float dt, void *stream);
int uammd_bdhi2d_get_counter(uammd_bdhi2d *h, unsigned int *counter); /* number of stochastic steps taken (Saru seed) */

/* ------------------------------------------------------------------------------------------------
 * BDHI::FIB — Fluctuating Immersed Boundary on a staggered grid.  Replaces
 *   FIB::FIB / forwardTime / forwardMidpoint     Integrator/BDHI/FIB/FIB.cuh:131-236, FIB.cu:87-135, :965-1000, :1058-1079
 *   addRandomAdvection, spreadParticleForces, solveStokesFourier, midPointStep     FIB.cu:274-391, :528-597, :667-724, :726-823
 * As in the reference both Scheme values run the simple midpoint scheme (FIB.cu:1072-1079) and the RFD thermal drift
 * is disabled (:400).  Exactly one of hydrodynamicRadius > 0 / cells[0] > 0 must be given (the other negative).
 * ---------------------------------------------------------------------------------------------- */
#define UAMMD_FIB_MIDPOINT 0
#define UAMMD_FIB_IMPROVED_MIDPOINT 1
typedef struct uammd_fib uammd_fib;
typedef struct {
  float boxSize[3];
  float temperature, viscosity, hydrodynamicRadius, dt;
  int cells[3];
  int scheme;        /* UAMMD_FIB_*; both run forwardMidpoint, as in the reference */
  unsigned int seed; /* the reference seeds cuRAND from System::rng(); here Saru(cell, seed, step) */
} uammd_fib_parameters;
int uammd_fib_create(const uammd_fib_parameters *par, uammd_fib **out, int cells[3], float *hydrodynamicRadius);
int uammd_fib_destroy(uammd_fib *h);
/* One step after the Interactors have filled d_force (real4[N]; NULL = no forces): d_pos real4[N] is advanced in place. */
int uammd_fib_forward(uammd_fib *h, float *d_pos, const float *d_force, int numberParticles, void *stream);
/* Test hook: take the 6*ncells fluid random numbers (slot-major: XX, YY, ZZ, XY, XZ, YZ) from this device array. */
int uammd_fib_set_noise(uammd_fib *h, const float *d_random);
float uammd_fib_self_mobility(float hydrodynamicRadius, float viscosity, float L); /* FIB::getSelfMobility, FIB.cuh:152-163 */

/* ------------------------------------------------------------------------------------------------
 * Hydro::ICM — Inertial Coupling Method, zero excess mass.  Replaces
 *   ICM::ICM / forwardTime                         Integrator/Hydro/ICM.cuh:123-231, ICM.cu:825-888, :1191-1224
 *   midPointStep, updateCellVelocityUnperturbed, spreadParticleForces, addThermalDrift, solveStokesFourier
 *                                                  ICM.cu:413-500, :793-822, :86-159, :161-275, :349-411
 * The fluid velocity persists in the handle between steps.  Exactly one of hydrodynamicRadius > 0 / cells[0] > 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_icm uammd_icm;
typedef struct {
  float boxSize[3];
  float temperature, viscosity, density, hydrodynamicRadius, dt;
  int cells[3];
  int sumThermalDrift;     /* default 0 in the reference */
  int removeTotalMomentum; /* default 1 in the reference */
  unsigned int seed;
} uammd_icm_parameters;
int uammd_icm_create(const uammd_icm_parameters *par, uammd_icm **out, int cells[3], float *hydrodynamicRadius);
int uammd_icm_destroy(uammd_icm *h);
/* One step = predictor (d_pos real4[N]: q^n -> q^{n+1/2}), the caller's Interactors at q^{n+1/2}, then the fluid update and the
 * corrector (d_pos -> q^{n+1}); d_force real4[N] or NULL when no Interactor is attached. */
int uammd_icm_predictor(uammd_icm *h, float *d_pos, int numberParticles, void *stream);
int uammd_icm_fluid_and_corrector(uammd_icm *h, float *d_pos, const float *d_force, int numberParticles, void *stream);
/* real3[nz][ny][nx]: the face-centred field, or (collocated = 1) ICM::getFluidVelocities (ICM.cuh:96-119, :176-199) */
int uammd_icm_get_fluid_velocity(uammd_icm *h, float *d_out, int collocated, void *stream);
int uammd_icm_set_fluid_velocity(uammd_icm *h, const float *d_in, void *stream);
int uammd_icm_set_noise(uammd_icm *h, const float *d_random); /* test hook: 6*ncells fluid random numbers, slot-major */

/* ------------------------------------------------------------------------------------------------
 * Hydro::ICM_Compressible — compressible Inertial Coupling Method, triply periodic or between two walls in z.  Replaces
 *   ICM_Compressible_impl<Walls> / forwardTime            Integrator/Hydro/ICM_Compressible.cuh:183-452, ICM_Compressible.cu:246-257
 *   updateGhostCellsWallsD with the built-in wall rule    ICM_Compressible/GhostCells.cuh:84-112
 *   rungeKuttaSubStepD, momentumToVelocityD, fillStochasticTensorD, spreadParticleForces, interpolateFluidVelocities
 *                                                         ICM_Compressible/{FluidSolver,SpatialDiscretization,Fluctuations,spreadInterp}.cuh
 * Density, momentum and velocity persist in the handle between steps: n^3 floats each, x fastest, no ghost cells, momentum and
 * velocity on the faces (component a of cell i at r_i + h_a/2); with walls each field also carries its two ghost planes, which no
 * getter but uammd_icmc_get_bottom_ghost returns.  Exactly one of hydrodynamicRadius > 0 / cells[0] > 0; the
 * reference's parameter checks fail with its messages.  seed is used as given (the callers draw one when theirs is 0).
 * Precondition: CUBIC cells (boxSize[a] / cells[a] the same on the three axes).  As in the reference, the window's scale is 1 / h_x on
 * every axis and the Laplacian and grad div are sums of differences over h_b divided by h_a; other cells are accepted and run, but
 * what they compute is not the continuum operator.
 * Rounding: the Runge-Kutta combination A U^a + B (U^b + dU) is evaluated as U^a + B ((U^b + dU) - U^a), so that an unchanged state
 * is returned exactly; results differ from the reference's literal form at the level of an ulp per sub-stage.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_icmc uammd_icmc;
typedef struct {
  float boxSize[3];
  int cells[3];
  float shearViscosity, bulkViscosity, speedOfSound, temperature, dt, hydrodynamicRadius;
  unsigned int seed;
  int walls; /* UAMMD_ICMC_WALLS_*: a zero-initialised struct has no walls */
} uammd_icmc_parameters;
/* Walls in z (ICM_Compressible_impl<Walls>, GhostCells.cuh; DESIGN.md §15 "Walls").  NONE: triply periodic.  BUILTIN: a wall at the
 * bottom and one at the top of the box, each moving in its plane with a velocity (u_x, u_y) the caller sets; every field then carries
 * two ghost planes that uammd_icmc_ghost_fill writes from the adjacent interior layer:
 *   rho_ghost = rho_adj,  v_ghost = 2 u_wall - v_adj,  g_ghost = 2 u_wall rho_adj - g_adj,  u_wall = (u_x, u_y, 0)
 * (the rule of the reference's test/Hydro/ICM_Compressible/walltest.cu, for both tangential components and both walls).  The particle
 * windows do not see the walls: they wrap periodically, as the reference's do.  temperature > 0 is refused with walls. */
enum { UAMMD_ICMC_WALLS_NONE = 0, UAMMD_ICMC_WALLS_BUILTIN = 1, UAMMD_ICMC_WALLS_EXTERNAL = 2 };
/* EXTERNAL: the same layout, but the ghost planes are written by a kernel of the caller's.  Where BUILTIN calls uammd_icmc_ghost_fill the
 * caller calls uammd_icmc_wall_planes_get, runs its kernel on the packed planes, and calls uammd_icmc_wall_planes_put.  The planes: per
 * field (rho, g_x, g_y, g_z, v_x, v_y, v_z, in this order) four planes of P = (cells[0] + 2)(cells[1] + 2) floats — bottom ghost, bottom
 * adjacent layer, top adjacent layer, top ghost — entry (i + 1) + (j + 1)(cells[0] + 2) for column (i, j), the border columns periodic
 * images; field f, plane k at d_planes + (4 f + k) P.  The ghost planes arrive holding their periodic images in z.  _put copies the two
 * ghost planes of every field back; writes to the adjacent planes are dropped.  uammd_icmc_set_fluid only copies the fields then: the
 * caller fills, calls uammd_icmc_velocity_to_momentum and fills again.  uammd_icmc_ghost_fill and uammd_icmc_fluid_and_corrector fail. */
int uammd_icmc_wall_planes_get(uammd_icmc *h, float **d_planes, void *stream);
int uammd_icmc_wall_planes_put(uammd_icmc *h, void *stream);
int uammd_icmc_velocity_to_momentum(uammd_icmc *h, void *stream);
/* the parameter checks alone (host code, no GPU): 0, or -2 with the reference's message in uammd_hip_last_error() */
int uammd_icmc_validate(const uammd_icmc_parameters *par);
int uammd_icmc_create(const uammd_icmc_parameters *par, uammd_icmc **out, int cells[3]); /* validates; the fluid starts at rho = 1, v = 0 */
int uammd_icmc_destroy(uammd_icmc *h);
/* n^3 floats each (NULL: that field keeps its values); the momentum is derived: g_a = v_a (rho_i + rho_{i+a}) / 2 */
int uammd_icmc_set_fluid(uammd_icmc *h, const float *d_density, const float *d_vx, const float *d_vy, const float *d_vz, void *stream);
/* the staggered fields; null pointers (the arrays or their entries) are skipped */
int uammd_icmc_get_fluid(uammd_icmc *h, float *d_density, float *const d_v[3], float *const d_g[3], void *stream);
/* the velocity averaged to the cell centres (computeCollocatedVelocityD, SpatialDiscretization.cuh:419-444) */
int uammd_icmc_get_collocated_velocity(uammd_icmc *h, float *d_vx, float *d_vy, float *d_vz, void *stream);
/* One step = predictor (d_pos real4[N]: q^n -> q^{n+1/2}, q^n kept in the handle), the caller's Interactors at q^{n+1/2}, then the
 * forcing, the noise, the three Runge-Kutta sub-stages and the corrector (d_pos -> q^{n+1}); d_force real4[N] or NULL.  N = 0: fluid only.
 * The second call counts the step (the noise of step s is Saru(seed, s, cell), s from 0). */
int uammd_icmc_predictor(uammd_icmc *h, float *d_pos, int numberParticles, void *stream);
int uammd_icmc_fluid_and_corrector(uammd_icmc *h, float *d_pos, const float *d_force, int numberParticles, void *stream);
/* The second call in pieces, so that a host can send the sub-step times and set the wall velocities before each ghost fill
 * (callRungeKuttaSubStep, ICM_Compressible.cu:70-95):
 *   fluid_begin (forcing and noise);  for s = 0, 1, 2: substage(s), ghost_fill, substage_velocity, ghost_fill;  fluid_end (corrector).
 * uammd_icmc_fluid_and_corrector is this composition with the wall velocities held fixed.  ghost_fill uses the velocities set last
 * (bottom and top, {u_x, u_y} each; zero after create); it acts on the level of the sub-stage under way, and on the fluid itself between
 * steps.  Without walls ghost_fill does nothing and set_wall_velocities fails. */
int uammd_icmc_set_wall_velocities(uammd_icmc *h, const float bottom[2], const float top[2]);
int uammd_icmc_fluid_begin(uammd_icmc *h, const float *d_pos, const float *d_force, int numberParticles, void *stream);
int uammd_icmc_substage(uammd_icmc *h, int s, void *stream);
int uammd_icmc_ghost_fill(uammd_icmc *h, void *stream);
int uammd_icmc_substage_velocity(uammd_icmc *h, void *stream);
int uammd_icmc_fluid_end(uammd_icmc *h, float *d_pos, int numberParticles, void *stream);
/* the bottom ghost plane (walls only): cells[0] * cells[1] floats per field, column (i, j) at i + j cells[0]; null pointers are skipped */
int uammd_icmc_get_bottom_ghost(uammd_icmc *h, float *d_density, float *const d_v[3], float *const d_g[3], void *stream);
/* Test hooks: the stochastic stress as float2 W[6][ncells] = {W_A, W_B} of the entries xx, yy, zz, xy, xz, yz (12 ncells floats).
 * get: the numbers the handle draws at `step`.  set: the following steps use a copy of d_noise instead of drawing (NULL: draw again). */
int uammd_icmc_get_noise(uammd_icmc *h, unsigned int step, float *d_out, void *stream);
int uammd_icmc_set_noise(uammd_icmc *h, const float *d_noise, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Triply periodic electrostatics (another consumer of the spread / FFT / gather engine).  Replaces
 *   Poisson::Poisson / sum / computeFieldPotentialAtParticles    Interactor/SpectralEwaldPoisson.cuh:83-136, .cu:71-160
 *   farField (spread q, R2C, chargeFourier2FieldAndPotential, 4 x C2R, gather + UnZip2Real4)   .cu:332-360, :410-559
 *   nearFieldForce / nearFieldEnergy / nearFieldFieldPotential over a CellList                 .cu:222-329, :362-408
 * split <= 0 disables the Ewald splitting (far field only).  As in the reference, Parameters::cells and ::support are
 * not consulted (the grid comes from upsampling or the tolerance heuristic).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_poisson uammd_poisson;
typedef struct {
  float boxSize[3];
  float epsilon;    /* permittivity */
  float tolerance;
  float gw;         /* Gaussian source width */
  float split;      /* Ewald splitting parameter, <= 0: no splitting */
  float upsampling; /* > 0: h = 1/upsampling */
} uammd_poisson_parameters;
typedef struct {
  int cells[3];
  int support;
  float nearFieldCutOff;
  int nTable;
  float h;
} uammd_poisson_info;
/* Errors (-2) carry the reference's messages: kernel support too large (.cu:95-102), near field cut off too large (:111-116). */
int uammd_poisson_create(const uammd_poisson_parameters *par, uammd_poisson **out, uammd_poisson_info *info);
int uammd_poisson_destroy(uammd_poisson *h);
/* "atomic_spread" = 1: spread the charges with global atomics instead of the tile-owned LDS kernel (test hook) */
int uammd_poisson_set_option(uammd_poisson *h, const char *name, int value);
/* Poisson::sum.  d_pos real4[N], d_charge real[N] (pd->getCharge).  The far field ADDS q E to d_force (real4[N]) and q phi
 * to d_energy (real[N]) whenever the pointer is non-null — the reference's interpolateFields adds both regardless of the
 * Computables (.cu:561-579), so a faithful caller passes both; nearForce / nearEnergy select the near-field passes
 * (comp.force / comp.energy). */
int uammd_poisson_sum(uammd_poisson *h, const float *d_pos, const float *d_charge, int numberParticles, float *d_force,
                      float *d_energy, int nearForce, int nearEnergy, void *stream);
/* Poisson::computeFieldPotentialAtParticles: d_fieldPotential real4[N] (Ex, Ey, Ez, phi) is ADDED to (the reference
 * zero-fills it first).  d_force / d_energy (nullable) receive the far-field side effect the reference's call has. */
int uammd_poisson_field_potential(uammd_poisson *h, const float *d_pos, const float *d_charge, int numberParticles,
                                  float *d_fieldPotential, float *d_force, float *d_energy, void *stream);
/* test hook: one stage of the far field alone, through the host functions and launches uammd_poisson_sum uses (the grids are
 * [nz][ny][2*(nx/2+1)], the layout of the in-place transforms):
 *   UAMMD_POISSON_PROBE_SPREAD    cell list, pack, spread of the charges ("atomic_spread" is honoured); d_out: the charge grid, float
 *   UAMMD_POISSON_PROBE_CONVOLVE  d_in: a charge grid; forward transform, Fourier-space kernel, the four inverse transforms and the
 *                                 interleave; d_out: the float4 grid (Ex, Ey, Ez, phi).  Needs no particles.
 *   UAMMD_POISSON_PROBE_GATHER    d_in: a float4 grid; cell list, pack, gather: (E, phi) is ADDED to d_out (real4[N]), q E to d_force
 *                                 (real4[N], nullable) and q phi to d_energy (real[N], nullable), as uammd_poisson_field_potential does
 * d_force and d_energy are consulted by the gather only.  info (may be null) reports what ran: [0..2] = tile dimensions of the
 * tile-owned spread, [3] = its waves per workgroup (0: the atomic spread ran), [4] = the compile-time support of its instantiation
 * (0: the generic body), [5] = UAMMD_POISSON_GATHER_*; entries of a stage that did not run are -1. */
#define UAMMD_POISSON_PROBE_SPREAD 0
#define UAMMD_POISSON_PROBE_CONVOLVE 1
#define UAMMD_POISSON_PROBE_GATHER 2
#define UAMMD_POISSON_GATHER_COL1 1 /* one stencil column per lane */
#define UAMMD_POISSON_GATHER_COL2 2 /* two columns per lane */
#define UAMMD_POISSON_GATHER_FLAT 3 /* node by node */
int uammd_poisson_probe(uammd_poisson *h, int stage, const float *d_pos, const float *d_charge, int numberParticles, const float *d_in,
                        float *d_out, float *d_force, float *d_energy, int *info, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path B on several GPUs — z-slab decomposition of the FCM grid (the reference is single GPU, so these
 * have no reference counterpart: they are the per-rank compute stages of uammd_fcm_displacements, cut where the
 * exchanges happen.  The exchanges themselves are RCCL calls of the host layer, uammd_amd/parallel_fcm.py).
 * Rank layouts (float2 = one complex):
 *   real window  float  [nzLocal + 2*halo][3][ny][2*(nx/2+1)]   owned planes are [halo, halo + nzLocal)
 *   xy spectrum  float2 [nzLocal][3][ny][nx/2+1]                 = the owned planes after the in-place 2-D R2C
 *   z buffer     float2 [nz][3][nyLocal][nx/2+1]                 rows y0 .. y0 + nyLocal of the Fourier grid
 * Sequence per step: slab_spread -> (halo planes ADDED into the neighbours) -> slab_forward_xy -> (all-to-all) ->
 * slab_fft_z(0) -> slab_kspace -> slab_fft_z(1) -> (all-to-all) -> slab_inverse_xy -> (halo planes COPIED from the
 * neighbours) -> slab_gather.  Positions are in the window frame: z relative to the centre of the owned slab.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_fcm_slab uammd_fcm_slab;
int uammd_fcm_slab_create(const uammd_fcm_parameters *par, int nzLocal, int z0, int halo, int nyLocal, int y0,
                          uammd_fcm_slab **out);
int uammd_fcm_slab_destroy(uammd_fcm_slab *h);
int uammd_fcm_slab_set_option(uammd_fcm_slab *h, const char *name, int value);
int uammd_fcm_slab_spread(uammd_fcm_slab *h, const float *d_posLocal, const float *d_force, int numberParticles,
                          float *d_grid, void *stream);
int uammd_fcm_slab_gather(uammd_fcm_slab *h, const float *d_posLocal, int numberParticles, const float *d_grid,
                          float *d_linearVelocity, void *stream);
int uammd_fcm_slab_forward_xy(uammd_fcm_slab *h, float *d_grid, void *stream);
/* device side of the all-to-all transposes (uammd_comm_alltoall moves block p of the send buffer to rank p): pack the owned planes'
 * spectrum [zl][c][y][kx] into [p][zl][c][yl][kx]; what arrives is the z buffer as it stands; on the way back unpack
 * [src][zl][c][yl][kx] into the spectrum of the window.  Buffers: 3 nzLocal ny (nx/2+1) float2 each. */
int uammd_fcm_slab_transpose_pack(uammd_fcm_slab *h, const float *d_grid, float *d_send, void *stream);
int uammd_fcm_slab_transpose_unpack(uammd_fcm_slab *h, const float *d_recv, float *d_grid, void *stream);
/* the same with the halo fold on the way: d_fromDown / d_fromUp (`planes` planes each, laid out like the window) are added to the first /
 * last `planes` owned planes as the x pass loads them (one launch less than adding them first).  Returns 1 when the solver's own FFT
 * does not serve this grid: add the planes and call uammd_fcm_slab_forward_xy */
int uammd_fcm_slab_forward_xy_fold(uammd_fcm_slab *h, float *d_grid, const float *d_fromDown, const float *d_fromUp, int planes, void *stream); /* in place on the owned planes */
int uammd_fcm_slab_inverse_xy(uammd_fcm_slab *h, float *d_grid, void *stream);
/* the inverse writing the owned planes of a float4 window d_inter[z][y][x] = (vx, vy, vz, 0) (returns 1 and does nothing when the grid
 * does not take the library's own FFT), and the gather that reads that window once the caller has exchanged its halo planes */
int uammd_fcm_slab_inverse_xy_inter(uammd_fcm_slab *h, float *d_grid, float *d_inter, void *stream);
/* world size 1 (the rank is its own neighbour through the periodic z faces): the same, and the first / last `wrapPlanes` owned planes are
 * also stored into the halo planes above / below the owned block — the window is ready for the gather without a halo exchange */
int uammd_fcm_slab_inverse_xy_inter_wrap(uammd_fcm_slab *h, float *d_grid, float *d_inter, int wrapPlanes, void *stream);
int uammd_fcm_slab_gather_inter(uammd_fcm_slab *h, const float *d_posLocal, int N, const float *d_inter, float *d_vel, void *stream);
int uammd_fcm_slab_fft_z(uammd_fcm_slab *h, float *d_cplxZ, int inverse, void *stream);
/* the three calls above (forward z, operator, inverse z) in one pass over d_cplxZ when nz is a power of two; returns 1 (and does
 * nothing) when the grid does not allow it */
int uammd_fcm_slab_z_fused(uammd_fcm_slab *h, float *d_cplxZ, int haveForce, float temperature, float prefactor, unsigned int seed2,
                           void *stream);
int uammd_fcm_slab_kspace(uammd_fcm_slab *h, float *d_cplxZ, int haveForce, float temperature, float prefactor,
                          unsigned int seed2, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path B, spectral Ewald variant — Positively Split Ewald RPY (BDHI::PSE).  Replaces
 *   pse_ns::NearField  ctor / Mdot / computeStochasticDisplacements / setShearStrain
 *                                              Integrator/BDHI/PSE/NearField.cuh:29-99, :239-285
 *   RPYPSE_near::FandG + TabulatedFunction     Integrator/BDHI/PSE/RPY_PSE.cuh:45-128, misc/TabulatedFunction.cuh:63-157
 *   pse_ns::FarField   ctor / computeHydrodynamicDisplacements / setShearStrain
 *                                              Integrator/BDHI/PSE/FarField.cuh:25-41, :85-308, :318-342, :569-654
 * Seeds: the reference draws `seed` from System::rng() in each constructor (near first, then far) and a fresh `seed2`
 * from the same generator at every stochastic call; they are explicit here (the C++/Python layers draw them).
 * The far field is a uammd_fcm handle in PSE mode (same spread / rocFFT / gather machinery, other greens function).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_pse_near uammd_pse_near;
/* errors with the reference's text "[BDHI::PSE] Cut off is too large, try increasing psi" when rcut > L/2 */
int uammd_pse_near_create(const float boxSize[3], float viscosity, float hydrodynamicRadius, float tolerance, float psi,
                          float shearStrain, unsigned int seed, uammd_pse_near **out, float *rcut_out,
                          int *nPointsTable_out);
int uammd_pse_near_destroy(uammd_pse_near *h);
int uammd_pse_near_set_shear_strain(uammd_pse_near *h, float shearStrain);
/* "exact_order" (default 0): 1 = thread-per-particle product in the reference's summation order (NearField.cuh:154-185 over
 * NeighbourList/common.cuh:10-34), bit for bit; 0 = eight lanes per particle, same pairs and per-pair arithmetic, another order.
 * "lazy_list" (default 0): 1 = the near-field cell list is rebuilt only after uammd_pse_near_positions_changed() (the host layers wire
 * it to ParticleData's position write signal) or when the position array / N of a call changes — CellList::update's needsRebuild
 * (NeighbourList/CellList.cuh:134-136,192-204); 0 = every mdot / stochastic / dot call rebuilds.
 * "pair_list" (default 1; takes effect with "lazy_list"): the pairs inside the cut-off are evaluated once per list build into 24-byte
 * records (F, (G - F) / r^2, r_ij, j) and the ~8 products of a step stream them; 0 = every product scans the 27 cells. */
int uammd_pse_near_set_option(uammd_pse_near *h, const char *name, int value);
int uammd_pse_near_positions_changed(uammd_pse_near *h);
/* The list update of the calls below (cl->update, NearField.cuh:231-237) ahead of them, nothing waited for; with "lazy_list" and
 * "pair_list" also the launch of the pair records' build.  Optional: a caller that queues other work between this and the first
 * product (BDHI::PSE::computeMF's far field, BDHI_PSE.cuh:92-120) hides the build's one host read behind it. */
int uammd_pse_near_prepare(uammd_pse_near *h, const float *d_pos, int numberParticles, void *stream);
/* diagnostics: pair records in use (0 while the products scan the cells) and allocated */
int uammd_pse_near_pair_records(uammd_pse_near *h, long long *records, long long *capacity);
/* Option "list_skin_percent" (40; with "lazy_list" and "pair_list", no shear): the particle order of a list build and every particle's
 * candidates within rc + skin (skin = percent / 100 x rc) are KEPT over the following steps; a step then refreshes the sorted positions
 * and makes its pair records from the candidates alone — exact while nobody has moved more than skin / 2 since the build, which is
 * measured on the device every step and read with the records' counters (a broken bound repeats the build from scratch, and the solve
 * that streamed the records).  Same pairs as a build per step, summed in another order.  0 = a list build per step.
 * uammd_pse_near_list_stats: {builds from scratch, record builds from a kept list, repeated builds, 1 while the mechanism is on}. */
int uammd_pse_near_list_stats(uammd_pse_near *h, long long out[4]);
/* diagnostics: the product kernel the handle launched last — 0 none yet, 1 the thread-per-particle walk ("exact_order"), 2 eight lanes per
 * particle scanning the cells, 3 pair records, 4 a wave per cell ("near_kernel" 0), 5 pair records fused with the Lanczos recurrence,
 * 6 the same with the uammd_pse_near_set_mdot_rider product riding along (a solve whose first product carried the rider reports 6 until
 * the handle's next product outside it).  Host-side bookkeeping: tests assert from it which path a set of options really took. */
int uammd_pse_near_last_product(uammd_pse_near *h, int *kind);
/* One-shot: the NEXT uammd_pse_near_stochastic on the handle also performs uammd_pse_near_mdot(h, pos, d_force, N, d_MF) with its own
 * positions — BDHI_PSE.cuh:92-126 calls the two back to back on the same list.  Where the solve streams pair records its first product
 * applies them to F as a second right-hand side (the records are read once for both vectors); otherwise (T = 0, scanning products) the
 * plain product runs before the call returns.  d_force NULL disarms. */
int uammd_pse_near_set_mdot_rider(uammd_pse_near *h, const float *d_force, float *d_MF);
/* d_MF real3[N] += M_near F (d_force real4[N]; NULL = nothing to do) */
int uammd_pse_near_mdot(uammd_pse_near *h, const float *d_pos, const float *d_force, int numberParticles, float *d_MF,
                        void *stream);
/* d_BdW real3[N] = prefactor sqrt(2 T) M_near^(1/2) dW by Lanczos (OVERWRITES d_BdW, as the reference); no-op at T == 0 */
int uammd_pse_near_stochastic(uammd_pse_near *h, const float *d_pos, int numberParticles, float temperature,
                              float prefactor, unsigned int seed2, float *d_BdW, void *stream, int *iterations);
/* test hooks: the Saru noise vector, and the raw product d_Mv3 = M_near d_v3 (what the Lanczos callback computes) */
int uammd_pse_near_noise(uammd_pse_near *h, int numberParticles, float variance, unsigned int seed2, float *d_out3,
                         void *stream);
int uammd_pse_near_dot(uammd_pse_near *h, const float *d_pos, const float *d_v3, int numberParticles, float *d_Mv3,
                       void *stream);
/* FarField::initializeGrid: grid cells BEFORE nextFFTWiseSize3D (utils/Grid.cuh:142-213, host logic of the caller) */
int uammd_pse_far_raw_cells(const float boxSize[3], float psi, float tolerance, int cells_out[3]);
int uammd_pse_far_create(const float boxSize[3], const int cells[3], float viscosity, float hydrodynamicRadius,
                         float tolerance, float psi, float shearStrain, unsigned int seed, uammd_fcm **out,
                         int *support_out, float *eta_out);
int uammd_pse_far_set_shear_strain(uammd_fcm *h, float shearStrain);
/* d_MF real3[N] += M_far F + prefactor sqrt(2T) M_far^(1/2) dW   (IBM::gather adds; d_force NULL = noise only) */
int uammd_pse_far_displacements(uammd_fcm *h, const float *d_pos, const float *d_force, int numberParticles,
                                float temperature, float prefactor, unsigned int seed2, float *d_MF, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Lanczos sqrt(M) v.  Replaces lanczos::Solver (misc/LanczosAlgorithm.cuh:32-83,
 * misc/LanczosAlgorithm/LanczosAlgorithm.cu:27-262) and the MatrixDot functor (LanczosAlgorithm/MatrixDot.h:7-25):
 * the matrix is a host callback that ENQUEUES d_Mv = M d_v (n floats, device pointers) on `stream` and returns 0.
 * uammd_lanczos_run returns 0 and the iteration count, or an error whose message is the reference's exception text
 * ("[Lanczos] Could not converge", "[Lanczos] Unknown error (found NaN in result guess) at iteration i").
 * The adaptive convergence-check schedule (starts at 3) is kept per handle, as per Solver instance.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_lanczos uammd_lanczos;
typedef int (*uammd_matvec_fn)(void *ctx, const float *d_v, float *d_Mv, int n, void *stream);
int uammd_lanczos_create(uammd_lanczos **out);
int uammd_lanczos_destroy(uammd_lanczos *h);
int uammd_lanczos_run(uammd_lanczos *h, uammd_matvec_fn dot, void *ctx, float *d_Bv, const float *d_v,
                      float tolerance, int n, void *stream, int *iterations);
/* Solver::runIterations (LanczosAlgorithm.cuh:49-67, LanczosAlgorithm.cu:183-200): exactly numberIterations Lanczos steps without a
 * convergence test; d_Bv = the estimate after the last step, *residual = |Bz_m - Bz_(m-1)| / |Bz_(m-1)| between the last two estimates. */
int uammd_lanczos_run_iterations(uammd_lanczos *h, uammd_matvec_fn dot, void *ctx, float *d_Bv, const float *d_v, int numberIterations, int n,
                                 void *stream, float *residual);
int uammd_lanczos_set_iteration_hard_limit(uammd_lanczos *h, int limit);
/* "defer_checks" (default 1): the reference checks convergence at every iteration from an adaptive first step on
 * (LanczosAlgorithm.cu:218-232); here the checks of the iterations before the one the PREVIOUS run stopped at are evaluated together
 * at that iteration — one host round trip and one pass over the Krylov basis instead of one per iteration; the run still stops at
 * the first iteration whose error passes, with that iteration's estimate (the reference's result and iteration count).  The checks are
 * evaluated in the reference's order: a tridiagonal block that cannot be diagonalised fails the run (-20) only if no EARLIER check
 * ends it.  Side effect to know about: a run that would have stopped at iteration k has by then called `dot` for the iterations up to
 * the previous run's stopping point (at most 7 more calls than the reference makes) — a callback that counts its calls sees them.
 * 0 = every check as its iteration completes, the reference's call count exactly. */
int uammd_lanczos_set_option(uammd_lanczos *h, const char *name, int value);
/* Vectors sharded over several ranks (Lanczos row): `n` is then the LOCAL length, the matvec callback computes the
 * local rows of M v, and every dot product / norm of the recurrence is completed by `reduce`, which must sum d_values[0..count)
 * in place over all ranks on `stream` (RCCL all-reduce of 1 float, 3 per iteration + 2 per convergence check).  ownsFirstElement:
 * non-zero on the rank that holds global element 0.  reduce == NULL restores the single-rank behaviour. */
typedef int (*uammd_allreduce_fn)(void *ctx, float *d_values, int count, void *stream);
int uammd_lanczos_set_allreduce(uammd_lanczos *h, uammd_allreduce_fn reduce, void *ctx, int ownsFirstElement);
/* {check_convergence_steps, lastRunRequiredSteps}: the adaptive schedule a run leaves behind (LanczosAlgorithm.cu:175, :245-251); a caller
 * that repeats a run restores it first */
int uammd_lanczos_get_schedule(uammd_lanczos *h, int state[2]);
int uammd_lanczos_set_schedule(uammd_lanczos *h, const int state[2]);
/* fn(ctx, stream) is called ONCE during the next uammd_lanczos_run: after the host has answered the run's first convergence check and
 * before it waits for the outcome (or when the run ends, if it never waited).  What fn queues on the stream runs behind the check's
 * kernels while the host is busy with the check: the one wait of a run is no longer a drained stream.  One-shot. */
typedef int (*uammd_interleave_fn)(void *ctx, void *stream);
int uammd_lanczos_set_interleave(uammd_lanczos *h, uammd_interleave_fn fn, void *ctx);
/* one stage earlier: called after the first check's scalars are on their way to the host and BEFORE the kernels that wait for the host's
 * answer; what fn queues runs while the host solves the check's small eigenproblems.  One-shot; called before the callback above. */
int uammd_lanczos_set_interleave_early(uammd_lanczos *h, uammd_interleave_fn fn, void *ctx);
/* the same for the solve inside the next uammd_pse_near_stochastic (BDHI::PSE queues its far field there); fn must not call into the
 * near-field handle.  One-shot. */
int uammd_pse_near_set_interleave(uammd_pse_near *h, uammd_interleave_fn fn, void *ctx);
int uammd_pse_near_set_interleave_early(uammd_pse_near *h, uammd_interleave_fn fn, void *ctx);
/* uammd_pse_far_displacements queued in two halves on the same stream with the same arguments (1: binning, spreading, forward x / y
 * transforms; 2: z transforms + operator + noise, inverse transforms, gather) — for the two callbacks above */
int uammd_pse_far_displacements_half(uammd_fcm *h, const float *d_pos, const float *d_force, int numberParticles, float temperature,
                                     float prefactor, unsigned int seed2, float *d_MF, int half, void *stream);
int uammd_lanczos_get_last_run_required_steps(uammd_lanczos *h, int *steps);

/* BDHI::Lanczos (open boundaries, dense RPY mobility, matrix free).  Replaces
 *   Lanczos_ns::NbodyMatrixFreeMobilityDot + NBody::transverse   Integrator/BDHI/BDHI_Lanczos.cu:56-118, Interactor/NBodyBase.cuh:46-159
 *   RotnePragerYamakawa                                           Integrator/BDHI/BDHI.cuh:27-96
 *   Lanczos::computeMF / computeBdW                               BDHI_Lanczos.cu:120-188
 * d_Mv real3[N] is OVERWRITTEN.  The reference draws the noise of computeBdW with cuRAND (parity unpinned):
 * the caller supplies 3N standard normal numbers. */
int uammd_rpy_nbody_mdot(const float *d_pos, const float *d_v, int vstride, const float *d_radius, float hydrodynamicRadius,
                         float viscosity, int numberParticles, float *d_Mv, void *stream);
int uammd_rpy_lanczos_bdw(uammd_lanczos *solver, const float *d_pos, const float *d_radius, float hydrodynamicRadius,
                          float viscosity, int numberParticles, const float *d_noise, float tolerance, float *d_BdW,
                          void *stream, int *iterations);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU (new design: the reference is single GPU).  One process per GPU, RCCL over xGMI, loaded on first use.
 * Set-up: rank 0 calls uammd_comm_unique_id and hands the 128 bytes to the other processes by any means (MPI, a file, a TCP
 * store: outside this library); every process then calls uammd_comm_init on ITS device.  All calls are asynchronous on `stream`
 * except uammd_comm_exchange_counts and uammd_comm_exchange_counts_device (the latter takes the two sizes from device memory and
 * returns {toUp, toDown, fromDown, fromUp} with one synchronisation).  The ranks form a periodic ring along z: "up" = rank + 1, "down" = rank - 1.
 *   path A  uammd_halo_pack -> uammd_comm_halo_exchange (4 floats per row), receive straight into the tail of the position array
 *   path B  uammd_fcm_slab_* + uammd_comm_halo_exchange (grid planes) + uammd_comm_alltoall (FFT transposes)
 *   Lanczos uammd_lanczos_set_allreduce with a callback that calls uammd_comm_allreduce_sum
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_comm uammd_comm;
int uammd_comm_unique_id(char id[128]);
/* the version of the librccl this library loaded (ncclGetVersion's integer: major * 10000 + minor * 100 + patch) */
int uammd_comm_rccl_version(int *version);
int uammd_comm_init(uammd_comm **out, int rank, int world, const char id[128]);
int uammd_comm_destroy(uammd_comm *h);
int uammd_comm_rank(const uammd_comm *h);
int uammd_comm_world(const uammd_comm *h);
int uammd_comm_halo_exchange(uammd_comm *h, const float *d_sendUp, int nUp, const float *d_sendDown, int nDown, float *d_recvFromDown,
                             int nFromDown, float *d_recvFromUp, int nFromUp, int floatsPerRow, void *stream);
int uammd_comm_exchange_counts(uammd_comm *h, const int toUpDown[2], int fromDownUp[2], void *stream);
int uammd_comm_exchange_counts_device(uammd_comm *h, const int *d_toUpDown, int all4[4], void *stream);
/* The membership refresh of a slab step in ONE call — the sequence above as uammd_amd/parallel.py (DistributedLJ) and
 * include/uammd/Distributed.h run it: displacement since the last refresh (when refRows == n; d_ref / d_maxDisplacement nullable),
 * leavers selected, the sizes to and from the two neighbours (host read 1), migration rows packed, exchanged (8 floats per row) and
 * dropped into the holes, forces of the owned rows zeroed, halo members selected with `reach` = rc + 3 skin, their sizes (host read 2),
 * positions packed with the frame shift and received straight into rows [n, n + ghosts) of d_pos, d_ref <- d_pos.
 * d_idx: int[4][capRows] (leavers up / down, halo up / down: rows 2 and 3 are the cached membership lists of the steps until the next
 * refresh); d_rows, d_arrivals: float[capRows][8]; d_send: float[capRows][4]; d_counts: int[4]; d_holes: int[capRows];
 * d_selectWorkspace: uammd_slab_select_workspace(capRows) bytes.  comm == NULL: a world of one in process.
 * d_listedMask (nullable, capRows bytes): 1 for the owned rows that are in a halo list, 0 for the others.
 * out = {owned rows, owned + ghosts, halo up, halo down, ghosts from below, from above, left up, left down, arrived from below, above}. */
int uammd_slab_refresh_lj(uammd_comm *comm, float *d_pos, float *d_vel, int *d_ids, float *d_force, int n, int capRows, float width, float reach,
                          int *d_idx, int *d_holes, int *d_counts, void *d_selectWorkspace, float *d_rows, float *d_arrivals, float *d_send,
                          float *d_ref, int refRows, float *d_maxDisplacement, unsigned char *d_listedMask, int out[10], void *stream);
int uammd_comm_alltoall(uammd_comm *h, const void *d_send, void *d_recv, size_t bytesPerPeer, void *stream);
int uammd_comm_allreduce_sum(uammd_comm *h, float *d_buf, int n, void *stream);

/* ------------------------------------------------------------------------------------------------
 * DOUBLE_PRECISION build of path B (global/defines.h:9-11,33-44 makes `real` a build switch; every accuracy assertion the
 * reference ships is compiled with it: test/CMakeLists.txt:9, test/BDHI/FCM/Makefile:9).  The `_f64` entry points below are
 * that build of the layout-generic kernels: IBM spread / gather, FCM_impl (deterministic part), PSE near / far field and
 * lanczos::Solver with real = double, so that the reference's own known answers run on the GPU at their own tolerances:
 *   test/BDHI/FCM/fcm_test.cu:85-144 (Hasimoto, 1e-8)        test/misc/ibm/test_ibm_regular.cu:113-136,240-274 (1e-10)
 *   test/misc/lanczos/test_lanczos.cu:236-269 (1e-7)          test/BDHI/PSE/pse_test.cu:64-117
 * Positions / forces are real4 = double[4], velocities real3 = double[3].  The tuned hot path (tile-owned MFMA spreading,
 * the in-LDS FFT, the pair prefilter) is single precision by construction: UAMMD's default `real`, and what bench.py measures.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int kind;        /* UAMMD_IBM_KERNEL_GAUSSIAN, _PESKIN3, _PESKIN4 or _CONSTANT */
  int support[3];
  double prefactor, tau, rmax;
  double invh[3];
} uammd_ibm_kernel_f64;
typedef struct {
  double boxSize[3];
  int cells[3];
  double viscosity;
  uammd_ibm_kernel_f64 kernel;
} uammd_fcm_parameters_f64;
typedef struct uammd_fcm_f64 uammd_fcm_f64;
typedef struct uammd_pse_near_f64 uammd_pse_near_f64;
typedef struct uammd_lanczos_f64 uammd_lanczos_f64;
int uammd_fcm_gaussian_kernel_f64(double h, double tolerance, uammd_ibm_kernel_f64 *out, double *a_eff);
double uammd_fcm_advise_grid_size_f64(double hydrodynamicRadius, double tolerance);
int uammd_ibm_spread_f64(const double *d_pos, int posStride, const double *d_quantity, int ncomp, int numberParticles,
                         const double boxSize[3], const int periodic[3], const int cellDim[3], int nxStride,
                         const uammd_ibm_kernel_f64 *kernel, double *d_grid, void *stream);
int uammd_ibm_gather_f64(const double *d_pos, int posStride, double *d_out, int ncomp, int numberParticles, const double boxSize[3],
                         const int periodic[3], const int cellDim[3], int nxStride, const uammd_ibm_kernel_f64 *kernel,
                         const double *d_grid, void *stream);
int uammd_fcm_create_f64(const uammd_fcm_parameters_f64 *par, uammd_fcm_f64 **out);
int uammd_fcm_destroy_f64(uammd_fcm_f64 *h);
/* d_velocity real3[N] = M F (overwritten; a PSE far-field handle ADDS, as FarField.cuh:563-566) */
int uammd_fcm_displacements_f64(uammd_fcm_f64 *h, const double *d_pos, const double *d_force, int numberParticles,
                                double *d_velocity, void *stream);
/* the same with the thermal term: d_velocity = M F + prefactor sqrt(2 T M) dW, Fourier noise keyed Saru(node, seed1, seed2)
 * (FCM_impl.cuh:437-542, FarField.cuh:235-308,471-501); d_force may be NULL (noise only) */
int uammd_fcm_displacements_thermal_f64(uammd_fcm_f64 *h, const double *d_pos, const double *d_force, int numberParticles, double temperature,
                                        double prefactor, unsigned int seed1, unsigned int seed2, double *d_velocity, void *stream);
/* BDHI::EulerMaruyama_ns::integrateGPUD with real = double (see uammd_bdhi_euler_maruyama) */
int uammd_bdhi_euler_maruyama_f64(double *d_pos, const int *d_index, const double *d_MF, const double *d_BdW, const double K[9], int numberParticles,
                                  double sqrt2Tdt, double dt, int is2D, void *stream);
/* BDHI::True2D / BDHI::Quasi2D with real = double (see uammd_bdhi2d_create: Integrator/Hydro/BDHI_quasi2D.cuh:155-257, .cu:61-88, :179-541;
 * the reference's test/BDHI/quasi2D/quasi2d_test.cu is compiled with -DDOUBLE_PRECISION).  d_pos / d_force real4[N] of doubles, d_vel real2[N]. */
typedef struct uammd_bdhi2d_f64 uammd_bdhi2d_f64;
typedef struct {
  double boxSize[2];
  double hydrodynamicRadius, viscosity, temperature, dt;
  int cells[2];
  unsigned int seed;
  int kernel; /* UAMMD_BDHI2D_* */
} uammd_bdhi2d_parameters_f64;
int uammd_bdhi2d_create_f64(const uammd_bdhi2d_parameters_f64 *par, uammd_bdhi2d_f64 **out, int cells[2], int *support);
int uammd_bdhi2d_destroy_f64(uammd_bdhi2d_f64 *h);
int uammd_bdhi2d_velocities_f64(uammd_bdhi2d_f64 *h, const double *d_pos, const double *d_force, int numberParticles, double *d_vel, void *stream);
int uammd_bdhi2d_update_positions_f64(double *d_pos, const double *d_vel, int numberParticles, double dt, void *stream);
/* Poisson with real = double (see uammd_poisson_create: Interactor/SpectralEwaldPoisson.cuh:83-136; the reference's
 * test/Potentials/Poisson/TriplyPeriodic tests are compiled with -DDOUBLE_PRECISION, the quadrupole at tolerance 1e-14 / support 41).  Near
 * field over all pairs with the minimum image.  d_pos / d_force / d_fieldPotential real4[N] of doubles, d_charge / d_energy real[N]. */
typedef struct uammd_poisson_f64 uammd_poisson_f64;
typedef struct {
  double boxSize[3];
  double epsilon, tolerance, gw, split, upsampling;
} uammd_poisson_parameters_f64;
typedef struct {
  int cells[3];
  int support;
  double nearFieldCutOff;
  int nTable;
  double h;
} uammd_poisson_info_f64;
int uammd_poisson_create_f64(const uammd_poisson_parameters_f64 *par, uammd_poisson_f64 **out, uammd_poisson_info_f64 *info);
int uammd_poisson_destroy_f64(uammd_poisson_f64 *h);
int uammd_poisson_sum_f64(uammd_poisson_f64 *h, const double *d_pos, const double *d_charge, int numberParticles, double *d_force, double *d_energy,
                          int nearForce, int nearEnergy, void *stream);
int uammd_poisson_field_potential_f64(uammd_poisson_f64 *h, const double *d_pos, const double *d_charge, int numberParticles, double *d_fieldPotential,
                                      double *d_force, double *d_energy, void *stream);
int uammd_pse_far_raw_cells_f64(const double boxSize[3], double psi, double tolerance, int cells_out[3]);
int uammd_pse_far_create_f64(const double boxSize[3], const int cells[3], double viscosity, double hydrodynamicRadius,
                             double tolerance, double psi, double shearStrain, uammd_fcm_f64 **out, int *support_out,
                             double *eta_out);
int uammd_pse_near_create_f64(const double boxSize[3], double viscosity, double hydrodynamicRadius, double tolerance, double psi,
                              uammd_pse_near_f64 **out, double *rcut_out, int *nPointsTable_out);
int uammd_pse_near_destroy_f64(uammd_pse_near_f64 *h);
/* d_MF real3[N] += M_near v, v = d_v with stride 4 (real4 forces) or 3 */
int uammd_pse_near_mdot_f64(uammd_pse_near_f64 *h, const double *d_pos, const double *d_v, int vstride, int numberParticles,
                            double *d_MF, void *stream);
typedef int (*uammd_matvec_fn_f64)(void *ctx, const double *d_v, double *d_Mv, int n, void *stream);
int uammd_lanczos_create_f64(uammd_lanczos_f64 **out);
/* NearField::computeStochasticDisplacements (NearField.cuh:255-284): d_BdW real3[N] = prefactor sqrt(2 T) sqrt(M_near) dW (overwritten),
 * noise keyed Saru(particle, seed1, seed2); `solver` is the caller's handle (its check schedule adapts from call to call) */
int uammd_pse_near_stochastic_f64(uammd_pse_near_f64 *h, uammd_lanczos_f64 *solver, const double *d_pos, int numberParticles, double temperature,
                                  double prefactor, unsigned int seed1, unsigned int seed2, double tolerance, double *d_BdW, void *stream,
                                  int *iterations);
int uammd_lanczos_destroy_f64(uammd_lanczos_f64 *h);
int uammd_lanczos_run_f64(uammd_lanczos_f64 *h, uammd_matvec_fn_f64 dot, void *ctx, double *d_Bv, const double *d_v,
                          double tolerance, int n, void *stream, int *iterations);
/* Solver::runIterations with real = double (see uammd_lanczos_run_iterations) */
int uammd_lanczos_run_iterations_f64(uammd_lanczos_f64 *h, uammd_matvec_fn_f64 dot, void *ctx, double *d_Bv, const double *d_v,
                                     int numberIterations, int n, void *stream, double *residual);
int uammd_lanczos_set_iteration_hard_limit_f64(uammd_lanczos_f64 *h, int limit);
int uammd_lanczos_get_last_run_required_steps_f64(uammd_lanczos_f64 *h, int *steps);
/* BDHI::Lanczos and BDHI::Cholesky with real = double (see uammd_rpy_nbody_mdot, uammd_rpy_lanczos_bdw, uammd_bdhi_cholesky_*: Integrator/BDHI/
 * BDHI_Lanczos.cu:56-188, BDHI_Cholesky.cu:34-262).  The reference's acceptance test of the two (test/BDHI/Lanczos_Cholesky) is compiled with
 * -DDOUBLE_PRECISION (its Makefile:3) and its bar of 1e-7 is for that build.  rocSOLVER dpotrf, rocBLAS dsymv / dtrmv. */
int uammd_rpy_nbody_mdot_f64(const double *d_pos, const double *d_v, int vstride, const double *d_radius, double hydrodynamicRadius, double viscosity,
                             int numberParticles, double *d_Mv, void *stream);
int uammd_rpy_lanczos_bdw_f64(uammd_lanczos_f64 *solver, const double *d_pos, const double *d_radius, double hydrodynamicRadius, double viscosity,
                              int numberParticles, const double *d_noise, double tolerance, double *d_BdW, void *stream, int *iterations);
typedef struct uammd_bdhi_cholesky_f64 uammd_bdhi_cholesky_f64;
int uammd_bdhi_cholesky_create_f64(int numberParticles, double viscosity, double hydrodynamicRadius, uammd_bdhi_cholesky_f64 **out);
int uammd_bdhi_cholesky_destroy_f64(uammd_bdhi_cholesky_f64 *h);
int uammd_bdhi_cholesky_setup_step_f64(uammd_bdhi_cholesky_f64 *h, const double *d_pos, const int *d_index, const double *d_radius, void *stream);
int uammd_bdhi_cholesky_mf_f64(uammd_bdhi_cholesky_f64 *h, const double *d_pos, const double *d_force, const int *d_index, const double *d_radius,
                               double *d_MF, void *stream);
int uammd_bdhi_cholesky_bdw_f64(uammd_bdhi_cholesky_f64 *h, const double *d_pos, const int *d_index, const double *d_radius, double *d_BdW,
                                void *stream);

/* ------------------------------------------------------------------------------------------------
 * Path A in double (uammd_amd/csrc/md_f64.hip): the cell list, the Lennard-Jones traversal and the Verlet integrators with
 * real = double.  The same reference interfaces as the single-precision blocks above:
 *   CellList::createUpdateGrid / CellListBase::update / getCellList   Interactor/NeighbourList/CellList.cuh:100-126,149-182,
 *                                                                     CellList/CellListBase.cuh:68-94,124-172,210-230
 *   ParticleSorter hash, stable sort, reorder                         utils/ParticleSorter.cuh:102-111,178-187,303-321
 *   transverseWithNeighbourContainer + Radial<LJFunctor>              Interactor/NeighbourList/common.cuh:10-34,
 *                                                                     Potential/RadialPotential.cuh:107-127, Potential.cuh:37-82
 *   NBody::transverse (boxes of at most 3 cut-offs)                   Interactor/NBodyBase.cuh:46-159, PairForces.cu:43-68
 *   VerletNVT GronbechJensen / Basic, initialVelocities, energy       Integrator/VerletNVT/GronbechJensen.cu:28-62, Basic.cu:12-29,86-114,173-207
 *   VerletNVE                                                         Integrator/VerletNVE.cu:64-85
 * Positions / forces are real4 = double[4N], velocities real3 = double[3N].  Every particle sums its pairs in the reference's neighbour
 * order (the 27 cells in common.cuh order, members in sorted order).  The Verlet list, the bonded kinds and DPD follow at the end of
 * this block (verletlist_f64.hip, bonded_f64.hip, dpd_f64.hip).  The UAMMD-shaped C++ headers do not route here yet: they refuse
 * -DDOUBLE_PRECISION as before.  Single precision only: SPH, the MC modules, the tile and ring traversals, the fused MD step, the slab
 * drivers, num_owned ghosts and the profiling hooks.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_celllist_f64 uammd_celllist_f64; /* opaque; owns index/hash/sortPos/cellStart/cellEnd */
/* uammd_celllist_data field for field, with double positions and box */
typedef struct {
  const unsigned int *d_cellStart;
  const int *d_cellEnd;
  const double *d_sortPos; /* real4[N] */
  const int *d_groupIndex;
  const unsigned int *d_sortHash;
  int cellDim[3];
  double boxSize[3];
  int periodic[3];
  unsigned int VALID_CELL;
  int numberParticles;
} uammd_celllist_data_f64;
int uammd_celllist_create_f64(uammd_celllist_f64 **out);
int uammd_celllist_destroy_f64(uammd_celllist_f64 *h);
/* uammd_celllist_create_grid with the division and the truncation in double (host only) */
int uammd_celllist_create_grid_f64(const double L[3], const int periodic[3], const double cutOff[3], int cellDim_out[3], double L_out[3],
                                   int periodic_out[3]);
/* hash (Morton key of the position's cell) -> stable sort of (key, index) on the key's bits -> gather of the rows -> cell tables.
 * d_pos is real4[N] in double; numberParticles = 0 is a no-op.  A NaN position or a particle outside a non-periodic box has no cell: it is
 * left out of the tables (it sorts behind every cell) and raises the list's host-mapped flag; the next update / get / traversal on the
 * handle fails with the reference's message, uammd_celllist_check_errors_f64 synchronises `stream` and reports at once. */
int uammd_celllist_update_f64(uammd_celllist_f64 *h, const double *d_pos, int numberParticles, const double L[3], const int periodic[3],
                              const int cellDim[3], void *stream);
int uammd_celllist_get_f64(uammd_celllist_f64 *h, uammd_celllist_data_f64 *out);
int uammd_celllist_check_errors_f64(uammd_celllist_f64 *h, void *stream);

/* LJFunctor::PairParameters and processPairParameters (Potential/Potential.cuh:31-35,66-82) in double, host */
typedef struct { double cutOff2, sigma2, epsilonDivSigma2, shift; } uammd_lj_pair_parameters_f64;
int uammd_lj_process_pair_parameters_f64(double cutOff, double sigma, double epsilon, int shift, uammd_lj_pair_parameters_f64 *out);
/* `algo` of uammd_lj_transverse_celllist_f64: UAMMD_LJ_ALGO_AUTO, UAMMD_LJ_ALGO_GENERAL or */
#define UAMMD_LJ_ALGO_SCAN32 11 /* GENERAL's pair evaluation fed by a distance scan over a single-precision image of the sorted positions
                                   (a strict superset of the pairs inside the cut-off; the evaluation applies the exact test in double):
                                   the same bits as GENERAL.  Grids the image does not cover (another box than the list's, a periodic
                                   direction with fewer than 5 cells) run GENERAL */
/* Arguments as uammd_lj_transverse_celllist.  With ntypes > 1 the kernels read the table's largest cut-off themselves: a table may be
 * rewritten in place between calls without telling the library. */
int uammd_lj_transverse_celllist_f64(uammd_celllist_f64 *h, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes,
                                     const double boxL[3], const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial,
                                     const int *d_globalIndex, int algo, void *stream);
int uammd_lj_transverse_nbody_f64(const double *d_pos, int numberParticles, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes,
                                  const double boxL[3], const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial,
                                  const int *d_globalIndex, void *stream);

/* The integrators of the single-precision block with double for every float.  The thermostat's Gaussians are Saru's single-precision
 * Box-Muller pair promoted to double, as in the reference's double build (third_party/saruprng.cuh:115-128; uammd_bd_scheme_step_f64). */
int uammd_verletnvt_gj_f64(int step, double *d_pos, double *d_vel, double *d_force, const double *d_mass, double defaultMass,
                           const int *d_index, int numberParticles, double dt, double friction, int is2D, double noiseAmplitude,
                           unsigned int stepNum, unsigned int seed, void *stream);
int uammd_verletnvt_basic_f64(int step, double *d_pos, double *d_vel, double *d_force, const double *d_mass, double defaultMass,
                              const int *d_index, int numberParticles, double dt, double friction, int is2D, double noiseAmplitude,
                              unsigned int stepNum, unsigned int seed, void *stream);
int uammd_verletnve_f64(int step, double *d_pos, double *d_vel, const double *d_force, const double *d_mass, double defaultMass,
                        const int *d_index, int numberParticles, double dt, int is2D, void *stream);
int uammd_verletnvt_initial_velocities_f64(double *d_vel, const int *d_index, double velAmplitude, int is2D, int numberParticles,
                                           unsigned int seed, void *stream);
int uammd_sum_kinetic_energy_f64(const double *d_vel, double *d_energy, const double *d_mass, double defaultMass, const int *d_index,
                                 int numberParticles, void *stream);

/* The Verlet list in double (verletlist_f64.hip): the single-precision block argument for argument with double for every float.  The
 * list is built on an internal uammd_celllist_f64 of the STORED positions with radius multiplier * cutOff (1.08); the test is
 * r2 <= (multiplier * cutOff)^2 in double and the particle itself is one of its neighbours; neighbours come in the reference's order;
 * entry k of sorted particle i is d_neighbourList[k * particleStride + i]; capacity 32 per particle, growing by 32 (the fill counts every
 * neighbour and stores only below the capacity it was launched with); the list is rebuilt when forced, when box, cutOff or N changed, when
 * the threshold (multiplier * cutOff - cutOff) / 2 is <= 1e-6 or when a particle drifted that far (one 4-byte read-back); sortPos is
 * refreshed on every update.  N = 0 is a no-op; a null handle, a non-positive cut-off or a multiplier < 1 return -1 before anything is
 * launched; a NaN position comes back as the cell list's error code. */
typedef struct uammd_verletlist_f64 uammd_verletlist_f64;
typedef struct {
  const int *d_neighbourList;
  const int *d_numberNeighbours;
  const double *d_sortPos;  /* real4[N]: CURRENT positions in the order of the last build */
  const int *d_groupIndex;  /* sorted index -> index in the input array */
  int particleStride;       /* = numberParticles */
  int maxNeighboursPerParticle;
  int numberParticles;
} uammd_verletlist_data_f64;
int uammd_verletlist_create_f64(uammd_verletlist_f64 **out);
int uammd_verletlist_destroy_f64(uammd_verletlist_f64 *h);
int uammd_verletlist_update_f64(uammd_verletlist_f64 *h, const double *d_pos, int numberParticles, const double L[3], const int periodic[3],
                                double cutOff, void *stream, int *rebuilt);
int uammd_verletlist_force_next_update_f64(uammd_verletlist_f64 *h);
int uammd_verletlist_set_cutoff_multiplier_f64(uammd_verletlist_f64 *h, double newMultiplier);
int uammd_verletlist_get_steps_since_last_update_f64(uammd_verletlist_f64 *h, int *steps);
int uammd_verletlist_get_f64(uammd_verletlist_f64 *h, uammd_verletlist_data_f64 *out);
/* every listed pair through the full minimum image and the pair evaluation of uammd_lj_transverse_celllist_f64, in list order */
int uammd_lj_transverse_verletlist_f64(uammd_verletlist_f64 *h, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes,
                                       const double boxL[3], const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial,
                                       const int *d_globalIndex, void *stream);

/* Bonded forces in double (bonded_f64.hip): the "Bonded interactions" block below with double for every float.  The same kinds, BondInfo
 * order, CSR layout and two shapes (uammd_bonded_build_rows and the "bonded_wave_threshold" tunable are shared); 1.0 / sqrt(r2), acos,
 * sin, cos and log in double.  refresh returns -1 when numberParticles is below the largest id + 1 of the uploaded set (checked on the
 * host: the sum would read out of range); sum before an upload and a refresh returns -1; a failed upload leaves the handle as it was. */
typedef struct uammd_bonded_f64 uammd_bonded_f64;
int uammd_bonded_create_f64(uammd_bonded_f64 **out);
int uammd_bonded_destroy_f64(uammd_bonded_f64 *h);
int uammd_bonded_upload_f64(uammd_bonded_f64 *h, int kind, int nbonds, const int *ids, const double *info, int nfixed,
                            const double *fixedPoints, const double L[3], const int periodic[3]);
int uammd_bonded_refresh_f64(uammd_bonded_f64 *h, const int *d_id2index, int numberParticles, void *stream);
int uammd_bonded_sum_f64(uammd_bonded_f64 *h, const double *d_pos, double *d_force, double *d_energy, double *d_virial, void *stream);
int uammd_bonded_get_shape_f64(uammd_bonded_f64 *h, int *rows, int *entries, int *laneRows, int *waveRows);

/* Potential::DPD in double (dpd_f64.hip): formula, key and truncations as documented at uammd_dpd_transverse_celllist, in double; xi is
 * Saru's single-precision Box-Muller x promoted to double (as the thermostats above); r2 == 0 and 1/r <= 1/cutOff reject exactly.
 * d_vel is real3[.] = double[3N] in input order.  The list variant gathers {velocity, key} into 32-byte rows in scratch memory the list
 * handle owns and needs a list whose cells are at least cutOff wide. */
int uammd_dpd_transverse_celllist_f64(uammd_celllist_f64 *h, const double *d_vel, const double boxL[3], const int boxPeriodic[3],
                                      double cutOff, double A, double gamma, double sigma, unsigned long long seed, unsigned long long step,
                                      int numberParticlesKey, double *d_force, const int *d_globalIndex, void *stream);
int uammd_dpd_transverse_nbody_f64(const double *d_pos, const double *d_vel, int numberParticles, const double boxL[3],
                                   const int boxPeriodic[3], double cutOff, double A, double gamma, double sigma, unsigned long long seed,
                                   unsigned long long step, int numberParticlesKey, double *d_force, const int *d_globalIndex, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Bonded interactions.  Replaces BondedForces<BondType, particlesPerBond> (Interactor/BondedForces.{cuh,cu}),
 * AngularBondedForces.cuh and TorsionalBondedForces.cuh for the built-in kinds.  Every particle with bonds sums, in registration
 * order, each bond it is a member of and adds the result to its own force / energy / virial: no atomics, the same bits on every run.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_bonded uammd_bonded; /* opaque; owns the CSR rows of one bond set */
/* kinds and their BondInfo, two floats in the reference's struct order (the bond file gives the same two numbers as "k p0"):
 *   0 Harmonic {k, r0}      1 FENE {r0, k}      (2 members; fixed points allowed)
 *   2 Angular {ang0, k}     (3 members)
 *   3 Torsional {phi0, k}   4 FourierLAMMPS {phi0, kdih}   (4 members) */
#define UAMMD_BOND_HARMONIC 0
#define UAMMD_BOND_FENE 1
#define UAMMD_BOND_ANGULAR 2
#define UAMMD_BOND_TORSIONAL 3
#define UAMMD_BOND_FOURIER_LAMMPS 4
int uammd_bonded_create(uammd_bonded **out);
int uammd_bonded_destroy(uammd_bonded *h);
/* Host logic only (no GPU): BondProcessor + buildBondList (BondedForces.cu:35-74,109-137).  ids[nbonds * particlesPerBond] are
 * particle ids, negative = a fixed point (registers nothing).  Rows are the particles with bonds in ascending id; row r is
 * rowId[r] and its entries are entryBond[rowStart[r] .. rowStart[r+1]), the bonds it belongs to in registration order.  Sizes:
 * rowId, rowStart - 1 and entryBond at most nbonds * particlesPerBond; any output may be NULL (the counts alone). */
int uammd_bonded_build_rows(int particlesPerBond, int nbonds, const int *ids, int *nrows, int *nentries, int *rowId, int *rowStart,
                            int *entryBond);
/* Upload one bond set (host arrays): ids[nbonds * members] (a negative id -(j+1) names fixedPoints[j], real4[nfixed], 2-member kinds
 * only), info[2 * nbonds] (BondInfo per bond, struct order above) and the box the kind applies the minimum image in.  The rows are
 * laid out here and split between the two traversal shapes by their length.  Synchronous. */
int uammd_bonded_upload(uammd_bonded *h, int kind, int nbonds, const int *ids, const float *info, int nfixed, const float *fixedPoints,
                        const float L[3], const int periodic[3]);
/* After an upload and after every ParticleData reorder: d_id2index[numberParticles] (ParticleData::getIdOrderedIndices) maps the
 * stored ids to current indices; the handle keeps its own copy. */
int uammd_bonded_refresh(uammd_bonded *h, const int *d_id2index, int numberParticles, void *stream);
/* Interactor::sum: force real4[N] += , energy[N] += , virial[N] += , each NULL when not requested (Interactor::Computables). */
int uammd_bonded_sum(uammd_bonded *h, const float *d_pos, float *d_force, float *d_energy, float *d_virial, void *stream);
/* the CSR as laid out: rows, entries and how many rows each shape takes under the current "bonded_wave_threshold" */
int uammd_bonded_get_shape(uammd_bonded *h, int *rows, int *entries, int *laneRows, int *waveRows);

/* ------------------------------------------------------------------------------------------------
 * Fast Chebyshev and Fourier-Chebyshev transforms (chebyshev.hip).  Replaces
 *   chebyshevTransform3DCufft / inverseChebyshevTransform3DCufft / fourierChebyshevTransform3DCufft /
 *   inverseFourierChebyshevTransform3DCufft            misc/Chebyshev/FastChebyshevTransform.cuh:147-260
 * A field holds nx ny nz complex values, element (i, j, k) at i + nx (j + ny k); plane k lies at cos(pi k / (nz - 1)).  With n = nz - 1:
 *   forward  c_k = pm_k / (2 n) [f_0 + (-1)^k f_n + 2 sum_{j = 1}^{n - 1} f_j cos(pi j k / n)],  pm_k = 1 for k = 0 and k = n, else 2
 *   inverse  f_j = sum_k c_k cos(pi j k / n)
 * The Fourier-Chebyshev calls add a 2-D complex transform over (i, j) in every plane: forward divided by nx ny, inverse not.
 * Out of place: d_in == d_out, a null pointer and nz < 2 are errors with a message.  The handle keeps the cosine table and the plans.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_fct uammd_fct;
#define UAMMD_FCT_FORWARD 1
#define UAMMD_FCT_INVERSE (-1)
int uammd_fct_create(int nx, int ny, int nz, int double_precision, uammd_fct **out);
int uammd_fct_destroy(uammd_fct *h);
int uammd_fct_chebyshev(uammd_fct *h, const float *d_in, float *d_out, int direction, void *stream);
int uammd_fct_chebyshev_f64(uammd_fct *h, const double *d_in, double *d_out, int direction, void *stream);
int uammd_fct_fourier_chebyshev(uammd_fct *h, const float *d_in, float *d_out, int direction, void *stream);
int uammd_fct_fourier_chebyshev_f64(uammd_fct *h, const double *d_in, double *d_out, int direction, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Batched boundary value problem solver (bvp.hip, bvp_host.hpp).  Replaces
 *   BVP::BatchedBVPHandlerReal / BatchedBVPGPUSolverReal::solve       misc/BoundaryValueProblem/BVPSolver.cuh:161-290
 * y'' - k^2 y = f on [-H, H] in Chebyshev space, one system per wave number, with
 *   tfi y'(H) / H + tsi y(H) / H^2 = alpha,   bfi y'(-H) / H + bsi y(-H) / H^2 = beta.
 * create: k, tfi, tsi, bfi, bsi are HOST doubles [nsys]; the tables are computed in double precision and kept on the device in the
 * precision asked for.  nz < 4, a non-finite k or factor and a singular 2 x 2 boundary system refuse the whole batch (the message names
 * the system).
 * solve: complex arrays (re, im interleaved).  Element i of system s of right-hand side r sits at r nsys nz + s sysStride + i coefStride,
 * with (sysStride, coefStride) = (1, nsys) - the solvers' layout - or (nz, 1); d_alpha / d_beta hold nrhs nsys values.  d_fn is not
 * modified; d_an receives the coefficients of y'', d_cn those of y.  A system's result depends on neither its place in the batch nor
 * the batch's size.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_bvp uammd_bvp;
int uammd_bvp_create(int nsys, int nz, double H, const double *k, const double *tfi, const double *tsi, const double *bfi,
                     const double *bsi, int double_precision, uammd_bvp **out);
int uammd_bvp_destroy(uammd_bvp *h);
int uammd_bvp_solve(uammd_bvp *h, const float *d_fn, const float *d_alpha, const float *d_beta, float *d_an, float *d_cn, int nrhs,
                    long long sysStride, long long coefStride, void *stream);
int uammd_bvp_solve_f64(uammd_bvp *h, const double *d_fn, const double *d_alpha, const double *d_beta, double *d_an, double *d_cn, int nrhs,
                        long long sysStride, long long coefStride, void *stream);
/* The device tables, for kernels of the caller's own (include/uammd/device/BVP.hip.hpp lays Tables<U> over them): rows of nsys
 * values, element s of row i at s + nsys i - beta[nz], diagonal_p2[nz], diagonal_m2[nz], C A^-1 [2 nz], 2 x 2 matrix [4], k^2 H^2 [1]. */
typedef struct {
  const void *d_tables; /* float or double, as the handle was created */
  int nsys, nz, double_precision;
} uammd_bvp_tables;
int uammd_bvp_device_tables(uammd_bvp *h, uammd_bvp_tables *out);

/* ------------------------------------------------------------------------------------------------
 * Doubly periodic electrostatics in a slab (dppoisson.hip).  Replaces
 *   DPPoissonSlab                          Interactor/DoublyPeriodic/DPPoissonSlab.cuh, PoissonSlab/...
 * Charges of Gaussian width gw between two walls at z = +-H/2, periodic in x and y.  permitivity = (top, bottom, inside); an infinite
 * wall permittivity is a metallic wall, whose surface value is a potential instead of a charge density.  Exactly one of split and Nxy
 * is positive.  create refuses what the reference's constructor refuses, with its message, before anything touches the device; with
 * out == NULL it only fills info (host only: no device is needed).
 * A particle with |z| > H/2 is left out of every stage, receives nothing and is counted (uammd_dppoisson_outside_count).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_dppoisson uammd_dppoisson;
typedef struct {
  double Lxy[2], H, gw, split;
  int Nxy;
  double permitivity[3]; /* top, bottom, inside */
  double tolerance, upsampling;
  int support;
  double numberStandardDeviations;
} uammd_dppoisson_parameters;
typedef struct {
  int cells[3];
  double He, gt, h;
  int support, supportZ; /* nodes per periodic axis; the reference's bound on the planes a window reaches (spreadInterp.cuh:33-35) */
  double nearFieldCutOff;
  int nTable;
  double kmax, split;
} uammd_dppoisson_info;
int uammd_dppoisson_create(const uammd_dppoisson_parameters *par, int double_precision, uammd_dppoisson **out, uammd_dppoisson_info *info);
int uammd_dppoisson_destroy(uammd_dppoisson *h);
/* "simple_spread": a lane per particle with atomic adds instead of the owner-computes spread (cross-check); "keep_stages": keep the
 * spread grid for uammd_dppoisson_get_stage; "skip_near_field": far field only (timing); "time_stages": record device events between
 * the stage launches for uammd_dppoisson_stage_times.  The window takes at most 16 nodes per axis (support <= 16; the reference has no
 * such limit): the gather keeps ceil(support^2 / 64) <= 4 columns per lane in registers; a larger support is refused by create. */
int uammd_dppoisson_set_option(uammd_dppoisson *h, const char *name, int value);
/* HOST arrays of nx ny samples at x = (i / nx - 1/2) Lx, y = (j / ny - 1/2) Ly, element (i, j) at i + nx j; NULL means zeros */
int uammd_dppoisson_set_surface_values(uammd_dppoisson *h, const double *top, const double *bottom);
/* setSurfaceValuesZeroModeFourier: a uniform wall value per wall (the other modes keep their values) */
int uammd_dppoisson_set_surface_zero_mode(uammd_dppoisson *h, double top, double bottom);
/* Interactor::sum: far field, then near field; force real4[N] += q E (w untouched), energy[N] += q phi, always both.  virial != 0 is
 * refused ("not implemented").  N = 0 launches nothing. */
int uammd_dppoisson_sum(uammd_dppoisson *h, const float *d_pos, const float *d_charge, int numberParticles, float *d_force, float *d_energy,
                        int virial, void *stream);
int uammd_dppoisson_sum_f64(uammd_dppoisson *h, const double *d_pos, const double *d_charge, int numberParticles, double *d_force, double *d_energy,
                            int virial, void *stream);
/* computeFieldPotentialAtParticles: d_fieldPotential real4[N] += (Ex, Ey, Ez, phi); like the reference's call it adds to force and energy too */
int uammd_dppoisson_field_potential(uammd_dppoisson *h, const float *d_pos, const float *d_charge, int numberParticles, float *d_fieldPotential,
                                    float *d_force, float *d_energy, void *stream);
int uammd_dppoisson_field_potential_f64(uammd_dppoisson *h, const double *d_pos, const double *d_charge, int numberParticles,
                                        double *d_fieldPotential, double *d_force, double *d_energy, void *stream);
/* the corrected k = 0 column of the last call: nz x (Ex, Ey, Ez, phi) complex as 8 nz HOST doubles (synchronises) */
int uammd_dppoisson_get_k0_mode(uammd_dppoisson *h, double *out);
int uammd_dppoisson_outside_count(uammd_dppoisson *h, int *count); /* synchronises */
/* test hook, into DEVICE memory in the handle's precision: "grid_near", "grid_all" (nx ny nz reals; option keep_stages) and "mismatch"
 * (4 nx ny + 2 complex: mP0, mPH, mE0, mEH, component c of wave number s = i + nx j at c nx ny + s, then the k = 0 line A0, B0) */
int uammd_dppoisson_get_stage(uammd_dppoisson *h, const char *name, void *d_out);
/* Milliseconds per stage of the last run (option time_stages; synchronises), ms[13]: classify, spread, forward transform, solve (both
 * systems, both at the walls, the mismatch: one kernel), correction, z pass of d phi / dz, z pass of phi, assemble, inverse transform of
 * (Ex, Ey), of (Ez, phi), gather, cell list + pack, near field; 0 for a stage that did not run */
int uammd_dppoisson_stage_times(uammd_dppoisson *h, double *ms);

/* ------------------------------------------------------------------------------------------------
 * Doubly periodic Stokes mobility and its integrator (dpstokes.hip).  Replaces
 *   DPStokesSlab_ns::DPStokes, DPStokesIntegrator      Integrator/BDHI/DoublyPeriodic/DPStokesSlab.cuh, StokesSlab/...
 * Particles in a fluid that is periodic in x and y and open (mode 0), bounded by a no-slip wall at z = -H/2 (1) or by walls at both
 * z = +-H/2 (2).  The window is the Barnett-Magland one: w nodes per axis, width beta (beta[1], beta[2] < 0 take beta[0]), alpha the
 * half support in cells.  nz < 0 takes pi H / min(hx, hy).  create refuses what the reference's constructor refuses, with its message,
 * and nz < 4, a support above 16 nodes and a window without w, alpha, beta[0], before anything touches the device; with out == NULL it
 * only fills info (host only: no device is needed).
 * Positions and forces are rows of posStride / forceStride (3 or 4) reals; velocities are rows of 3.  A particle with |z| > H/2 or a
 * non-finite coordinate is left out of every stage, receives zero and is counted (uammd_dpstokes_outside_count).  Torques are not
 * implemented: a non-null d_torque is refused.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uammd_dpstokes uammd_dpstokes;
typedef struct uammd_dpstokes_integrator uammd_dpstokes_integrator;
typedef struct {
  int nx, ny, nz;
  double viscosity, Lx, Ly, H;
  double w, beta[3], alpha;
  int mode; /* 0 none, 1 bottom, 2 slit */
} uammd_dpstokes_parameters;
typedef struct {
  int cells[3], support;
  double hx, hy, rmax, beta[3];
} uammd_dpstokes_info;
typedef struct {
  double temperature, dt, tolerance; /* tolerance: of the Lanczos iteration */
  double deltaRFD;                   /* <= 0: the reference's 1e-6 (double precision only: single precision refuses temperature > 0 without it) */
  int useLeimkuhler;
  unsigned int seed, seedRFD;
} uammd_dpstokes_integrator_parameters;
int uammd_dpstokes_create(const uammd_dpstokes_parameters *par, int double_precision, uammd_dpstokes **out, uammd_dpstokes_info *info);
int uammd_dpstokes_destroy(uammd_dpstokes *h);
/* "simple_spread": a lane per particle with atomic adds instead of the owner-computes spread (cross-check); "time_stages": record device
 * events between the stage launches for uammd_dpstokes_stage_times */
int uammd_dpstokes_set_option(uammd_dpstokes *h, const char *name, int value);
/* DPStokes::Mdot: d_mf real3[N] = M F (overwritten) */
int uammd_dpstokes_mdot(uammd_dpstokes *h, const float *d_pos, int posStride, const float *d_force, int forceStride, const float *d_torque,
                        int numberParticles, float *d_mf, void *stream);
int uammd_dpstokes_mdot_f64(uammd_dpstokes *h, const double *d_pos, int posStride, const double *d_force, int forceStride, const double *d_torque,
                            int numberParticles, double *d_mf, void *stream);
/* computeAverageVelocity: the plane average of u (direction 0) or v (1) at the nz planes, HOST doubles, plane 0 at the top (synchronises) */
int uammd_dpstokes_average_velocity(uammd_dpstokes *h, const float *d_pos, int posStride, const float *d_force, int forceStride,
                                    int numberParticles, int direction, double *averageVelocity, void *stream);
int uammd_dpstokes_average_velocity_f64(uammd_dpstokes *h, const double *d_pos, int posStride, const double *d_force, int forceStride,
                                        int numberParticles, int direction, double *averageVelocity, void *stream);
/* the corrected Chebyshev-space (u, v, w, p) of the last call into DEVICE memory in the handle's precision: 4 nz nx ny complex,
 * coefficient m of wave number s = i + nx j of component c at (c nz + m) nx ny + s; normalised like the library's forward transform, so
 * the k = 0 column of a velocity is its plane average (synchronises) */
int uammd_dpstokes_fluid_cheb(uammd_dpstokes *h, float *d_out);
int uammd_dpstokes_fluid_cheb_f64(uammd_dpstokes *h, double *d_out);
int uammd_dpstokes_outside_count(uammd_dpstokes *h, int *count); /* synchronises */
/* Milliseconds per stage of the last run (option time_stages; synchronises), ms[13]: classify, spread, forward transform of (fx, fy), of
 * fz, pressure solve, velocity solves, correction constants, correction at the planes, its z passes, zero mode + assemble, inverse
 * transform of (u, v), of (w, p), gather; 0 for a stage that did not run */
int uammd_dpstokes_stage_times(uammd_dpstokes *h, double *ms);
/* DPStokesIntegrator: a solver of its own plus the Lanczos handle.  step is forwardTime after the interactors have summed their forces:
 * pos += dt M F [+ dt sqrt(2 T / dt) M^(1/2) W (averaged with the previous step's under useLeimkuhler) + the thermal drift].
 * thermal_drift: d_drift real3[N] = (T dt / delta) [M(q + delta W / 2) W - M(q - delta W / 2) W] for the caller's W (real3[N]);
 * fluctuations: d_out real3[N] = M^(1/2) W for the caller's W.  _solver: the integrator's solver (owned by the integrator). */
int uammd_dpstokes_integrator_create(const uammd_dpstokes_parameters *par, const uammd_dpstokes_integrator_parameters *ipar, int double_precision,
                                     uammd_dpstokes_integrator **out);
int uammd_dpstokes_integrator_destroy(uammd_dpstokes_integrator *h);
uammd_dpstokes *uammd_dpstokes_integrator_solver(uammd_dpstokes_integrator *h);
int uammd_dpstokes_integrator_step(uammd_dpstokes_integrator *h, float *d_pos, int posStride, const float *d_force, int forceStride,
                                   int numberParticles, void *stream);
int uammd_dpstokes_integrator_step_f64(uammd_dpstokes_integrator *h, double *d_pos, int posStride, const double *d_force, int forceStride,
                                       int numberParticles, void *stream);
/* test hook: what the last step added up, real3[N] into DEVICE memory in the handle's precision (synchronises): which = 0 M F,
 * 1 the fluctuations, 2 the thermal drift, 3 the fluctuations of the step before (useLeimkuhler) */
int uammd_dpstokes_integrator_last(uammd_dpstokes_integrator *h, int which, int numberParticles, void *d_out);
int uammd_dpstokes_integrator_thermal_drift(uammd_dpstokes_integrator *h, const float *d_pos, int posStride, const float *d_w, int numberParticles,
                                            float *d_drift, void *stream);
int uammd_dpstokes_integrator_thermal_drift_f64(uammd_dpstokes_integrator *h, const double *d_pos, int posStride, const double *d_w,
                                                int numberParticles, double *d_drift, void *stream);
int uammd_dpstokes_integrator_fluctuations(uammd_dpstokes_integrator *h, const float *d_pos, int posStride, const float *d_w, int numberParticles,
                                           float *d_out, void *stream);
int uammd_dpstokes_integrator_fluctuations_f64(uammd_dpstokes_integrator *h, const double *d_pos, int posStride, const double *d_w,
                                               int numberParticles, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
