// kh_lattice_plan.h - the host sizing of the lattice kernels (csrc/kh_lattice.hip): plain C++, no HIP, so that the arithmetic
// that decides which form of a kernel runs is tested on the CPU (tests/test_lattice_plan_host.py) and reported by
// kh_lattice_last_plan.
//
//   PlanPrep   the dataflow preparation (PrepKernelDF): workgroups that share a CU, slots of the state-time window, states whose
//              counters stay in LDS (a larger lattice counts in device memory), bytes of dynamic LDS
//   PlanSweep  the dataflow sweeps (ForwardBackwardDFKernel): workgroups that share a CU, arcs of a 64-state block staged per
//              wave, slots of the value window (a lattice of more states than that uses half of them as tags), dynamic LDS
//
// The level preparation (PrepKernel) has no plan: its three work arrays are static LDS of kLevelPrepLdsStates states.
#ifndef KH_LATTICE_PLAN_H_
#define KH_LATTICE_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace kh_latplan {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;         // of a CU
constexpr int kMaxPerCu = 4;                  // (more than four resident workgroups per CU: the window gets too small)
constexpr int kPrepStaticBytes = 21 * 1024;   // PrepKernelDF: the sort's staging area + the static words
constexpr int kPrepWinLarge = 4096, kPrepWinSmall = 1024;   // state-time window: one 8-byte word per slot
constexpr int kStageLarge = 384, kStageSmall = 192;
constexpr int kWinMin = 512, kWinMax = 16384;
constexpr int kLevelPrepLdsStates = 5120;     // PrepKernel: 60 KB of LDS for the three work arrays

// static LDS the sweep reserves for a staging area of `stage` arcs per wave (a double, an int and a float per arc) + the words
constexpr int SweepStageBytes(int stage) { return stage * 16 * kWaves + 256; }

// "a window slot is rewritten by the wave that wrote it": the state `slots` further on belongs to the same wave
constexpr bool SameWaveRewrites(int slots) { return slots >= 64 && (slots / 64) % kWaves == 0; }

inline int PerCu(int n_lats, int cus) {
  cus = std::max(1, cus);
  return std::max(1, std::min(kMaxPerCu, (n_lats + cus - 1) / cus));
}

struct PrepPlan {
  int per_cu, win, lds_states;
  size_t dyn_bytes;
};

inline PrepPlan PlanPrep(int n_lats, int max_ns, int cus) {
  PrepPlan p;
  p.per_cu = PerCu(n_lats, cus);
  const int budget = kLdsBytes / p.per_cu - kPrepStaticBytes;
  p.win = p.per_cu <= 2 ? kPrepWinLarge : kPrepWinSmall;
  p.lds_states = std::max(0, std::min(std::max(1, max_ns), (budget - p.win * 8) / 4));
  p.dyn_bytes = static_cast<size_t>(p.win) * 8 + static_cast<size_t>(p.lds_states) * 4;
  return p;
}

// KH_LATTICE_WIN: taken only for a power of two in [kWinMin, kWinMax]
constexpr bool ValidWinOverride(int v) { return v >= kWinMin && v <= kWinMax && (v & (v - 1)) == 0; }

struct SweepPlan {
  int per_cu, stage, win;
  size_t dyn_bytes;
};

// win_override: 0 = none
inline SweepPlan PlanSweep(int n_lats, int max_ns, int cus, int win_override) {
  SweepPlan p;
  p.per_cu = PerCu(n_lats, cus);
  p.stage = p.per_cu > 2 ? kStageSmall : kStageLarge;
  const int stage_bytes = SweepStageBytes(p.stage);
  int win = kWinMin;
  while (win < kWinMax && win < max_ns && (2 * win) * 8 + stage_bytes <= kLdsBytes / p.per_cu) win *= 2;
  if (ValidWinOverride(win_override)) win = win_override;
  p.win = win;
  p.dyn_bytes = static_cast<size_t>(win) * sizeof(double);
  return p;
}

// kh_lattice_last_plan: the words of the record
enum {
  kRecCus = 0, kRecPrepDataflow, kRecPrepPerCu, kRecPrepWin, kRecPrepLdsStates, kRecPrepOffLds,
  kRecSweepDataflow, kRecSweepPerCu, kRecSweepStage, kRecSweepWin, kRecTagged, kRecReserved, kRecWords
};
static_assert(kRecWords == 12, "kh_lattice_last_plan fills int32_t[12]");

}  // namespace kh_latplan

#endif  // KH_LATTICE_PLAN_H_
