// Drives the FCM handle's host-side decisions (uammd_amd/csrc/fcm_prep_state.hpp) against a model of the device side.  Plain C++, no
// device: tests/test_fcm_prep_state_cpu.py builds it with the address and undefined-behaviour sanitizers.
//   fcm_prep_state replay            plays the call list on stdin (one call per line, see replay()) and prints the (preparation, update)
//                                    pair after every solve or step, as uammd_fcm_last_preparation reports them
//   fcm_prep_state enumerate DEPTH   every sequence of up to DEPTH letters of the alphabet below, slot_refresh = 2
//   fcm_prep_state random SEQS LEN   SEQS random sequences of LEN letters, fixed seed
// The driver does what fcm.hip does with a plan, on the model instead of the device, and checks after every call:
//   I1  no kernel counts on top of counters that the model does not hold as zero
//   I2  a claimed binning or slot preparation was made from this array version, this N and this stream
//   I3  k_fcm_step_prep only walks an entry order that is a permutation of exactly N particles
//   I4  with `slots` and `bin_ahead` off every update is without binning, and every solve is sorted fresh from the second one after the
//       options went off: the first may still claim what the last update with them on left pending, as the logic before this type let
//       it (in the golden trace the solve after `slots` goes off still claims the slot layout).  The issue states I4 without this.
//       (A solve with `atomic_spread` on prepares nothing, whatever the options.)
//   I5  after the overflow report was seen the slot layout is never chosen again
//   I6  the second half of a solve is accepted only directly after its own first half, with the same N
//   I7  what the type takes the counters to hold is true of the model: zeros are zeros, and the counts of what is pending are there,
//       in one array at most, exactly while something is pending
// and that whatever is launched finds buffers that hold it, also after a call that failed in a reserve (letter "fail": the driver then
// does what fcm.hip does, tells the state that its plan was not executed, and returns).
#include "../../uammd_amd/csrc/fcm_prep_state.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

using namespace uammd_hip;

namespace {

constexpr int kTiles = 64;   // 32^3 in tiles of edge 8
char streamTags[2];

struct Made {   // what a binning or a slot preparation was made from
  int array, version, N;
  const void *stream;
  bool operator==(const Made &o) const { return array == o.array && version == o.version && N == o.N && stream == o.stream; }
};
enum Holds { kZero, kCounts, kGarbage };
struct Counter { Holds holds = kGarbage; Made of{-1, -1, -1, nullptr}; };

struct Device {   // the handle's device arrays, as far as the decisions depend on them
  Counter tileCount, slotCount[2];
  int orderN = -1;         // the entries are a permutation of this many particles (-1: of none)
  int compactCap = 0;      // particles the compact arrays hold
  long recCap = 0;         // slot records
  int ovfCap = 0, slotCap = 0;
  bool haveCounts = false;
};

struct Caller {   // the program that uses the handle
  int array = 0, nIndex = 0, streamIndex = 0;
  int version[2] = {0, 0};
  bool mayVouch[2] = {false, false};   // the last writer of the array was a step on this handle
  bool overflow = false, scrambled = false;
};

struct World {
  FcmPrepState state;
  Device dev;
  Caller who;
  bool overflowSeen = false;
  bool tiles = true;         // option "atomic_spread" is off
  bool failReserve = false;  // the next reserve that a plan asks for fails, and the call with it
  bool halfOpen = false;   // a first half was queued and no solve came since
  int halfN = 0;
  int callsWithBothOff = 0;
};

int kN[2] = {3000, 4000};   // the caller's two sizes (replay: kN[0] is the call's own)
std::string history;   // the letters applied so far, for the failure message

[[noreturn]] void fail(const char *what) {
  std::printf("FAILED %s after: %s\n", what, history.c_str());
  std::exit(1);
}
void require(bool ok, const char *what) { if (!ok) fail(what); }

FcmPrepInputs inputs(const World &w, int array, int N, const void *stream, bool kept, bool force) {
  FcmPrepInputs c{};
  static const char arrays[2] = {0, 0};
  c.pos = &arrays[array];
  c.N = N;
  c.stream = stream;
  c.positionsKept = kept;
  c.haveForce = force;
  c.tiles = w.tiles;
  c.overflowReport = w.who.overflow;
  c.scrambledReport = w.who.scrambled;
  c.slotCap = std::max(32, ((int)(3.0 * ((double)N / kTiles)) + 16 + 7) & ~7);
  c.slotFits = true;
  c.slotBuffersHold = w.dev.recCap >= (long)kTiles * c.slotCap + N && w.dev.ovfCap >= N && w.dev.haveCounts;
  return c;
}

// a reserve failed: what it was to grow is gone (DeviceBuffer::reserve frees first), the call returns the error
void reserveFailed(World &w, bool compact) {
  Device &d = w.dev;
  w.failReserve = false;
  if (compact) {
    d.compactCap = 0;
    d.tileCount = Counter{};
    d.orderN = -1;
  } else {
    d.recCap = 0;
    d.ovfCap = 0;
    d.haveCounts = false;
    d.slotCount[0] = d.slotCount[1] = Counter{};
  }
  w.state.planNotExecuted();
}

// k_fcm_step_prep as planned: counts on top of `parity`.  False: the call failed.
bool stepPrep(World &w, const FcmStepPrepPlan &p, const FcmPrepInputs &c, const Made &of) {
  Device &d = w.dev;
  if (p.growSlots && w.failReserve) { reserveFailed(w, false); return false; }
  if (p.growSlots) {   // a reallocation: everything in the slot buffers is garbage
    d.recCap = std::max(d.recCap, (long)kTiles * c.slotCap + c.N);
    d.ovfCap = std::max(d.ovfCap, c.N);
    d.haveCounts = true;
    d.slotCap = c.slotCap;
    d.slotCount[0] = d.slotCount[1] = Counter{};
  }
  require(d.recCap >= (long)kTiles * c.slotCap + c.N && d.ovfCap >= c.N && d.haveCounts && d.slotCap == c.slotCap, "k_fcm_step_prep: buffers too small");
  if (p.zeroSlotCounts) d.slotCount[0].holds = d.slotCount[1].holds = kZero;
  require(d.slotCount[p.parity].holds == kZero, "I1 (k_fcm_step_prep counts on top of counters that are not zero)");
  require(d.orderN == c.N, "I3 (k_fcm_step_prep walks entries that are no permutation of N particles)");
  require(!w.overflowSeen, "I5 (the slot layout after the overflow report was seen)");
  d.slotCount[p.parity] = Counter{kCounts, of};
  return true;
}

// False: the call failed.
bool solve(World &w, bool kept, bool force, bool firstHalf) {
  Caller &who = w.who;
  Device &d = w.dev;
  const int N = kN[who.nIndex];
  const void *stream = &streamTags[who.streamIndex];
  const Made now{who.array, who.version[who.array], N, stream};
  const FcmPrepInputs c = inputs(w, who.array, N, stream, kept, force);
  const bool bothOff = !w.state.slots && !w.state.binAhead;
  const bool slotsWereOn = w.state.slots;
  const FcmSolvePlan p = w.state.beforeSolve(c);
  if (c.overflowReport && slotsWereOn && !w.state.slots) w.overflowSeen = true;
  if (p.clearScrambled) who.scrambled = false;
  w.halfOpen = false;
  require((p.prep != kFcmPrepNone) == w.tiles, "a solve prepares something exactly when the tile kernels run");
  if (!w.tiles) {   // (the atomic spread reads none of the handle's arrays)
    w.callsWithBothOff = bothOff ? w.callsWithBothOff + 1 : 0;
  } else if (p.slots()) {
    require(!w.overflowSeen, "I5 (the slot layout after the overflow report was seen)");
    if (p.prep == kFcmPrepSlotsSelf && !stepPrep(w, p, c, now)) return false;
    require(d.slotCount[p.parity].holds == kCounts && d.slotCount[p.parity].of == now, "I2 (a slot preparation of other particles)");
    require(d.orderN == N, "I3 (the slot layout over entries that are no permutation of N particles)");
    require(force || p.zeroSlotNext, "no spread and no memset for the other parity");
    d.slotCount[p.parity ^ 1].holds = kZero;   // by the spread, or by the memset
    d.slotCount[p.parity].holds = kGarbage;    // read; still holds the counts
  } else {
    if (p.growCompact && w.failReserve) { reserveFailed(w, true); return false; }
    if (p.growCompact) {   // a reallocation: everything is garbage
      d.compactCap = std::max(d.compactCap, N);
      d.tileCount = Counter{};
      d.orderN = -1;
    }
    require(d.compactCap >= N, "a sorted solve: buffers too small");
    if (p.zeroTileCount) d.tileCount.holds = kZero;
    if (p.prep == kFcmPrepSortedFresh) {
      require(d.tileCount.holds == kZero, "I1 (k_fcm_bin_count counts on top of counters that are not zero)");
      d.tileCount = Counter{kCounts, now};
    }
    require(d.tileCount.holds == kCounts && d.tileCount.of == now, "I2 (a binning of other particles)");
    d.tileCount.holds = kZero;   // k_fcm_tile_scan
    d.orderN = N;                // k_fcm_prepare writes the entries anew
    for (Counter &s : d.slotCount)
      if (s.holds == kCounts) s.holds = kGarbage;   // (a preparation that points into the entries it replaced)
  }
  if (w.tiles) {
    if (bothOff && w.callsWithBothOff > 0) require(p.prep == kFcmPrepSortedFresh, "I4 (slots and bin_ahead off: a solve that is not sorted fresh)");
    w.callsWithBothOff = bothOff ? w.callsWithBothOff + 1 : 0;
  }
  if (firstHalf) {
    w.state.firstHalfQueued(N);
    w.halfOpen = true;
    w.halfN = N;
  }
  return true;
}

void step(World &w, bool vouch, bool force) {
  Caller &who = w.who;
  Device &d = w.dev;
  if (!solve(w, vouch && who.mayVouch[who.array], force, false)) return;
  const int N = kN[who.nIndex];
  const void *stream = &streamTags[who.streamIndex];
  const FcmPrepInputs c = inputs(w, who.array, N, stream, false, force);
  const bool bothOff = !w.state.slots && !w.state.binAhead;
  const bool slotsWereOn = w.state.slots;
  const FcmUpdatePlan u = w.state.afterStepSolve(c);
  if (c.overflowReport && slotsWereOn && !w.state.slots) w.overflowSeen = true;
  if (u.clearScrambled) who.scrambled = false;
  const Made next{who.array, who.version[who.array] + 1, N, stream};
  // (a call that fails before its kernel leaves the particles where they were: whoever could vouch for the array still can)
  if (u.update == kFcmUpdateStepPrep && !stepPrep(w, u, c, next)) return;
  who.version[who.array]++;   // the update kernel moves the particles, and prepares for what it wrote
  who.mayVouch[who.array] = true;
  if (u.update == kFcmUpdateBin) {
    require(d.compactCap >= N && d.orderN == N, "k_fcm_update_bin: no entries of these particles to walk");
    if (u.zeroTileCount) d.tileCount.holds = kZero;
    require(d.tileCount.holds == kZero, "I1 (k_fcm_update_bin counts on top of counters that are not zero)");
    d.tileCount = Counter{kCounts, next};
  } else require(u.update == kFcmUpdateStepPrep || u.update == kFcmUpdatePlain, "an update that is none of the three");
  if (bothOff) require(u.update == kFcmUpdatePlain, "I4 (slots and bin_ahead off: an update that bins)");
}

void checkKnowledge(const World &w) {
  const FcmPrepState &s = w.state;
  const Device &d = w.dev;
  const FcmPrepState::Counters believed[3] = {s.tileCountHolds(), s.slotCountHolds(0), s.slotCountHolds(1)};
  const Counter *const held[3] = {&d.tileCount, &d.slotCount[0], &d.slotCount[1]};
  int pending = 0;
  for (int k = 0; k < 3; ++k) {
    if (believed[k] == FcmPrepState::kZero) require(held[k]->holds == kZero, "I7 (counters taken for zero that are not)");
    if (believed[k] == FcmPrepState::kHoldsPending) {
      require(held[k]->holds == kCounts, "I7 (counters taken for a pending preparation's that are not)");
      ++pending;
    }
  }
  require(pending == (s.somethingPending() ? 1 : 0), "I7 (counters of a pending preparation without one, or one without counters)");
}

void checkHalves(const World &w) {
  for (int N : kN) {
    FcmPrepState probe = w.state;
    require(probe.takeSecondHalf(N) == (w.halfOpen && w.halfN == N), "I6 (the second half of a solve)");
  }
}

enum Letter { kStepVouch, kStep, kStepNoForceVouch, kSolve, kSolveNoForce, kBothHalves, kFirstHalf, kMove, kOtherArray, kOtherN, kOtherStream,
              kToggleSlots, kToggleBinAhead, kScrambled, kOverflow, kToggleTiles, kFailReserve, kLetters };
const char *const kNames[kLetters] = {"step+", "step", "step0+", "solve", "solve0", "halves", "half", "move", "array", "N", "stream", "slots", "bin_ahead",
                                      "scrambled", "overflow", "atomic_spread", "fail"};

long calls = 0;

void apply(World &w, int letter) {
  Caller &who = w.who;
  ++calls;
  switch (letter) {
    case kStepVouch: step(w, true, true); break;
    case kStep: step(w, false, true); break;
    case kStepNoForceVouch: step(w, true, false); break;
    case kSolve: solve(w, false, true, false); break;
    case kSolveNoForce: solve(w, false, false, false); break;
    case kBothHalves:
      if (!solve(w, false, true, true)) break;
      checkHalves(w);
      require(w.state.takeSecondHalf(kN[who.nIndex]), "I6 (the second half directly after its first)");
      w.halfOpen = false;
      break;
    case kFirstHalf: solve(w, false, true, true); break;
    case kMove: who.version[who.array]++; who.mayVouch[who.array] = false; break;
    case kOtherArray: who.array ^= 1; break;
    case kOtherN: who.nIndex ^= 1; break;
    case kOtherStream: who.streamIndex ^= 1; break;
    case kToggleSlots: w.state.slots = !w.state.slots; break;
    case kToggleBinAhead: w.state.binAhead = !w.state.binAhead; break;
    case kScrambled: who.scrambled = true; break;
    case kOverflow: who.overflow = true; break;   // (nobody resets this report)
    case kToggleTiles: w.tiles = !w.tiles; break;
    case kFailReserve: w.failReserve = true; break;
  }
  checkHalves(w);
  checkKnowledge(w);
}

World fresh(int refresh) {
  World w;
  w.state.slots = true;   // (whatever the environment says)
  w.state.slotRefresh = refresh;
  return w;
}

long sequences = 0;
void enumerate(const World &w, int depth) {
  for (int letter = 0; letter < kLetters; ++letter) {
    const size_t mark = history.size();
    history += kNames[letter];
    history += ' ';
    World next = w;
    apply(next, letter);
    ++sequences;
    if (depth > 1) enumerate(next, depth - 1);
    history.resize(mark);
  }
}

// one call per line:  step ARRAY N KEPT FORCE STREAM | solve ARRAY N FORCE | move ARRAY | option NAME VALUE   (ARRAY: A or B)
int replay() {
  World w = fresh(128);
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    char op[32], a[32];
    int n = 0, x = 0, y = 0, z = 0;
    const int got = std::sscanf(line, "%31s %31s %d %d %d %d", op, a, &n, &x, &y, &z);
    if (got < 2) continue;
    history += line;
    Caller &who = w.who;
    if (!std::strcmp(op, "option")) {
      if (!std::strcmp(a, "slots")) w.state.slots = n != 0;
      else if (!std::strcmp(a, "bin_ahead")) w.state.binAhead = n != 0;
      else if (!std::strcmp(a, "slot_refresh")) w.state.slotRefresh = n;
      else { std::printf("unknown option %s\n", a); return 2; }
      continue;
    }
    who.array = a[0] == 'B';
    if (!std::strcmp(op, "move")) { who.version[who.array]++; who.mayVouch[who.array] = false; continue; }
    kN[0] = n;
    who.nIndex = 0;
    if (!std::strcmp(op, "step")) {
      who.streamIndex = z;
      const bool honest = who.mayVouch[who.array];
      if (x && !honest) { std::printf("the script vouches for an array that was touched\n"); return 2; }
      step(w, x != 0, y != 0);
    } else if (!std::strcmp(op, "solve")) {
      who.streamIndex = 0;
      solve(w, false, x != 0, false);
    } else { std::printf("unknown call %s\n", op); return 2; }
    checkHalves(w);
    checkKnowledge(w);
    std::printf("%d %d\n", (int)w.state.lastPreparation(), (int)w.state.lastUpdate());
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "replay") return replay();
  if (mode == "enumerate" && argc == 3) {
    enumerate(fresh(2), std::atoi(argv[2]));
    std::printf("enumerated %ld sequences, %ld calls: invariants hold\n", sequences, calls);
    return 0;
  }
  if (mode == "random" && argc == 4) {
    const long seqs = std::atol(argv[2]);
    const int len = std::atoi(argv[3]);
    std::uint64_t s = 0x9E3779B97F4A7C15ull;
    for (long q = 0; q < seqs; ++q) {
      World w = fresh(2 + (int)(q % 3));
      history.clear();
      for (int i = 0; i < len; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int letter = (int)((s >> 33) % kLetters);
        history += kNames[letter];
        history += ' ';
        apply(w, letter);
      }
    }
    std::printf("random: %ld sequences of %d letters, %ld calls: invariants hold\n", seqs, len, calls);
    return 0;
  }
  std::fprintf(stderr, "usage: %s replay | enumerate DEPTH | random SEQUENCES LENGTH\n", argv[0]);
  return 2;
}
