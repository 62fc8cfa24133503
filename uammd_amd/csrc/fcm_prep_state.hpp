// How a solve of the FCM handle (fcm.hip) gets its stencils, decided on the host: plain C++14, no HIP header; device pointers and
// streams are opaque `const void *`.  fcm.hip asks before every solve and after the solve of every uammd_fcm_step_euler_maruyama, and
// executes the plan it is given: reserves, waits, memsets and launches are all there.  tests/cxx/fcm_prep_state.cpp drives this type
// against a model of the device side, exhaustively, under the sanitizers.
//
// A solve takes one of four preparations (FcmPreparation):
//   sorted fresh      k_fcm_bin_count -> k_fcm_tile_scan -> k_fcm_prepare
//   sorted claimed    k_fcm_tile_scan -> k_fcm_prepare on the binning that the previous step's k_fcm_update_bin left pending
//   slots claimed     nothing: the previous step's k_fcm_step_prep left the slot layout pending
//   slots self        k_fcm_step_prep without the update, from the entry order that an earlier solve of the same N particles left
// and the update of a step does one of three things for the next solve (FcmUpdate).
//
// Device state this type keeps track of:
//   tileCount           the compact layout's tile populations.  k_fcm_bin_count and a binning k_fcm_update_bin count ON TOP of them;
//                       k_fcm_tile_scan consumes them and leaves zeros.
//   slotCount[2]        the slot layout's counters, two parities.  k_fcm_step_prep counts ON TOP of one; the spread of the slot-layout
//                       solve that reads it zeroes the other for the update kernel that follows.
//   the entry order     origin[0 .. orderN).w is a permutation of the particles, left by a sorted solve of orderN particles and kept by
//                       every slot-layout solve since.
#pragma once
#include <cstdlib>

namespace uammd_hip {

enum FcmPreparation { kFcmPrepNone = 0, kFcmPrepSortedFresh = 1, kFcmPrepSortedClaimed = 2, kFcmPrepSlotsClaimed = 3, kFcmPrepSlotsSelf = 4 };
enum FcmUpdate { kFcmUpdateNoStep = 0, kFcmUpdateStepPrep = 1, kFcmUpdateBin = 2, kFcmUpdatePlain = 3 };

// what the rules read from outside, per call
struct FcmPrepInputs {
  const void *pos;
  int N;
  const void *stream;
  bool positionsKept;  // the caller vouches: pos is what the previous step left (solves; ignored by afterStepSolve)
  bool haveForce;      // (no force: no spread, which would have zeroed the other parity's counters)
  bool tiles;          // the tile-owned kernels run: the grid allows them and option "atomic_spread" is off
  bool overflowReport;   // slotFlagHost[0]: a spread met an overflow list long enough to cost time
  bool scrambledReport;  // slotFlagHost[1] above its threshold: the entries' order no longer follows the tiles
  bool slotFits;         // the slot records of N particles stay under 1 GiB and N < 2^21 (a record holds entry and particle in 21 bits each)
  int slotCap;           // records per tile for this N
  bool slotBuffersHold;  // the slot buffers are large enough for N and slotCap
};

// the slot layout's preparation kernel, as part of either plan
struct FcmStepPrepPlan {
  bool growSlots = false;     // wait for the stream, then reserve the slot buffers for (N, slotCap)
  bool zeroSlotCounts = false;  // memset both parities first
  int parity = 0;             // count into this parity
  bool clearScrambled = false;  // the scrambled report was read and acted on: reset slotFlagHost[1]
};

struct FcmSolvePlan : FcmStepPrepPlan {   // (the base: only with kFcmPrepSlotsSelf, except clearScrambled; parity: of either slot preparation)
  FcmPreparation prep = kFcmPrepNone;
  bool growCompact = false;      // wait for the stream, then reserve the compact buffers for N
  const void *waitFor = nullptr;  // wait for this stream first: the handle's buffers are ordered by the stream of the last sorted solve
  bool haveWait = false;
  bool zeroTileCount = false;    // memset tileCount before the binning
  bool zeroSlotNext = false;     // memset parity ^ 1 after the preparation
  bool slots() const { return prep == kFcmPrepSlotsClaimed || prep == kFcmPrepSlotsSelf; }
};

struct FcmUpdatePlan : FcmStepPrepPlan {  // (the base: only with kFcmUpdateStepPrep)
  FcmUpdate update = kFcmUpdatePlain;
  bool zeroTileCount = false;    // kFcmUpdateBin: memset tileCount first
};

class FcmPrepState {
 public:
  // options (uammd_fcm_set_option)
  bool slots = true;         // "slots" (handle creation starts it from FcmSwitches::slots: A/B runs of programs that set no options)
  bool binAhead = true;      // "bin_ahead": the step's update kernel also prepares the next solve
  // "slot_refresh": after so many slot-layout preparations in a row the next one is refused, so that a sorted solve renews the entries'
  // order (it keeps the gather's windows local).  In a run of vouching steps the refusal meets the update: it bins instead, the solve
  // after it finds slotSteps back at 0 and prepares the slot layout on the spot, and the binning is dropped unused: the run repeats
  // slots claimed ... slots claimed / binning, slots self / step-prep, and takes no sorted solve.  That is the logic this type was
  // given to keep, and what tests/golden/fcm_preparation_trace.json records; it is not what the option was meant to do.
  int slotRefresh = 128;
  bool tileGather = false;   // "tile_gather": k_fcm_gather_tile walks compact tile ranges, so every solve is sorted

  // what the type takes a counter array to hold: zeros, the counts of what is pending and nothing else, or anything
  enum Counters { kZero, kHoldsPending, kGarbage };
  Counters tileCountHolds() const { return tileCount; }
  Counters slotCountHolds(int parity) const { return slotCount[parity]; }
  bool somethingPending() const { return pending.what != kNothing; }

  int compactCapacity() const { return compactCap; }
  int slotCapacity() const { return slotCap; }
  FcmPreparation lastPreparation() const { return lastPrep; }
  FcmUpdate lastUpdate() const { return lastUpd; }
  bool lastSolveReadSlots() const { return lastSolveSlots; }
  int lastSlotParity() const { return slotParity; }

  // ---- buffer events ----
  void compactBuffersReallocated(int N) {
    drop();
    tileCount = kGarbage;
    orderN = 0;
    compactCap = N;
  }
  void slotBuffersReallocated(int cap) {   // (or the records per tile changed: the counters' meaning with them)
    if (pending.what == kSlotPrep) drop();
    slotCount[0] = slotCount[1] = kGarbage;
    slotCap = cap;
  }

  // fcm.hip could not execute a plan (a reserve or a launch failed, and the call returns the error): the plan was recorded as taken, so
  // nothing recorded holds any more.  The next solve reserves again and sorts from scratch.
  void planNotExecuted() {
    drop();
    tileCount = slotCount[0] = slotCount[1] = kGarbage;
    orderN = 0;
    compactCap = 0;
    lastSolveSlots = false;
    halfPending = false;
    lastPrep = kFcmPrepNone;
    lastUpd = kFcmUpdateNoStep;
  }

  // ---- before a solve ----
  FcmSolvePlan beforeSolve(const FcmPrepInputs &c) {
    FcmSolvePlan p;
    halfPending = false;   // (a first half whose second never came is forgotten by the next solve)
    lastUpd = kFcmUpdateNoStep;
    if (!c.tiles) {        // the atomic spread prepares nothing and uses nothing
      drop();
      lastSolveSlots = false;
      return finish(p);
    }
    // 1. the previous step's update prepared exactly this solve (used whatever its order: it is correct, and the next update looks at the order)
    if (pending.what == kSlotPrep && !tileGather && claims(c)) {
      p.prep = kFcmPrepSlotsClaimed;
      pending.what = kNothing;
    } else {
      if (pending.what == kSlotPrep) drop();
      p.clearScrambled = c.scrambledReport;
      // 2. nobody prepared it, but the entries are in the order of an earlier solve of these N particles on this stream
      if (!c.scrambledReport && slots && !tileGather && orderN == c.N && haveStream && stream == c.stream && planStepPrep(c, false, &p)) {
        p.prep = kFcmPrepSlotsSelf;
        pending.what = kNothing;
      }
    }
    if (p.slots()) {
      p.parity = slotParity;
      p.zeroSlotNext = !c.haveForce;
      slotCount[slotParity] = kGarbage;   // read by this solve
      slotCount[slotParity ^ 1] = kZero;  // by its spread, or by the memset
      lastSolveSlots = true;
      return finish(p);
    }
    // 3. the sorted layout
    slotSteps = 0;   // (the entries' order is fresh)
    if (compactCap < c.N) {
      p.growCompact = true;
      compactBuffersReallocated(c.N);
    }
    if (haveStream && stream != c.stream) {  // (the zeroed counters too are ordered by that stream only)
      p.haveWait = true;
      p.waitFor = stream;
      drop();
      tileCount = kGarbage;
    }
    const bool claim = pending.what == kBinning && claims(c);
    if (!claim) drop();
    pending.what = kNothing;
    stream = c.stream;
    haveStream = true;
    p.zeroTileCount = tileCount == kGarbage;
    tileCount = kZero;   // (k_fcm_tile_scan hands the counters back zeroed)
    orderN = c.N;        // (origin[slot].w = the particle of compact slot `slot`: the entry order of the slot layout)
    lastSolveSlots = false;
    p.prep = claim ? kFcmPrepSortedClaimed : kFcmPrepSortedFresh;
    return finish(p);
  }

  // ---- a solve queued in two halves (uammd_pse_far_displacements_half): the second reads what the first prepared ----
  void firstHalfQueued(int N) {
    halfPending = true;
    halfN = N;
  }
  bool takeSecondHalf(int N) {
    if (!halfPending || halfN != N) return false;
    halfPending = false;
    return true;
  }

  // ---- after the solve of uammd_fcm_step_euler_maruyama: what the update kernel does for the next solve ----
  FcmUpdatePlan afterStepSolve(const FcmPrepInputs &c) {
    FcmUpdatePlan u;
    const bool ahead = c.tiles && binAhead && compactCap >= c.N;
    if (ahead && slots && planStepPrep(c, true, &u)) u.update = kFcmUpdateStepPrep;
    else if (ahead) {
      u.update = kFcmUpdateBin;
      u.zeroTileCount = tileCount != kZero;
      tileCount = kHoldsPending;
      pending = Pending{kBinning, c.pos, c.N, c.stream};
    }
    lastUpd = u.update;
    return u;
  }

 private:
  enum What { kNothing, kBinning, kSlotPrep };
  // what the previous step's update left for the next solve: one thing at most, made from this array, of this many particles, on this stream
  struct Pending { What what; const void *pos; int N; const void *stream; };
  Pending pending{kNothing, nullptr, 0, nullptr};
  Counters tileCount = kGarbage;
  Counters slotCount[2] = {kGarbage, kGarbage};
  int slotParity = 0;           // the parity that the pending, or the last used, slot preparation counted into
  bool lastSolveSlots = false;  // the solve that has just run read the slot layout
  int slotSteps = 0;            // slot-layout preparations since the last sorted solve
  int orderN = 0;
  const void *stream = nullptr;  // of the last sorted solve
  bool haveStream = false;
  int compactCap = 0, slotCap = 0;
  bool halfPending = false;
  int halfN = 0;
  FcmPreparation lastPrep = kFcmPrepNone;
  FcmUpdate lastUpd = kFcmUpdateNoStep;

  bool claims(const FcmPrepInputs &c) const {
    return c.positionsKept && pending.pos == c.pos && pending.N == c.N && pending.stream == c.stream;
  }
  FcmSolvePlan finish(const FcmSolvePlan &p) {
    lastPrep = p.prep;
    return p;
  }

  // Forgets what is pending.  The counters that it counted into still hold its counts, so they are no longer zero; this is the only
  // place that says so.  Round 6 had this rule written out at each site that dropped something, and one site lacked it: a slot-layout
  // solve dropped an unclaimed binning and left tileCount marked as zeroed.  The next sorted solve ranked its particles on top of the
  // stale counts and k_fcm_prepare wrote its rows past the arrays (a memory fault when the host ran ahead of the device), or the next
  // update binned on top of them and a sorted solve then claimed the sum (wrong stencil rows).
  void drop() {
    if (pending.what == kBinning) tileCount = kGarbage;
    if (pending.what == kSlotPrep) slotCount[slotParity] = kGarbage;
    pending.what = kNothing;
  }

  // The slot layout's preparation (k_fcm_step_prep), by the step's update or on the spot for a solve.  False: the slot layout is not to
  // be used for the next solve.
  bool planStepPrep(const FcmPrepInputs &c, bool update, FcmStepPrepPlan *p) {
    if (c.overflowReport) {   // this system is too clustered for fixed capacities
      slots = false;
      return false;
    }
    if (slotSteps >= slotRefresh) {
      slotSteps = 0;
      return false;
    }
    if (update && c.scrambledReport) {  // (the update then bins for the compact layout, so that the next solve sorts)
      p->clearScrambled = true;
      return false;
    }
    if (!c.slotFits) return false;
    if (!c.slotBuffersHold || slotCap != c.slotCap) {
      p->growSlots = true;
      slotBuffersReallocated(c.slotCap);
    }
    // (the other parity only right after a slot-layout solve, whose spread has just zeroed it)
    if (lastSolveSlots && slotCount[slotParity ^ 1] == kZero) p->parity = slotParity ^ 1;
    else {
      p->zeroSlotCounts = true;
      slotCount[0] = slotCount[1] = kZero;
      p->parity = 0;
    }
    drop();   // (a binning that the previous update left and this solve did not get to claim)
    slotParity = p->parity;
    slotCount[slotParity] = kHoldsPending;
    pending = Pending{kSlotPrep, c.pos, c.N, c.stream};
    slotSteps++;
    return true;
  }
};

}  // namespace uammd_hip
