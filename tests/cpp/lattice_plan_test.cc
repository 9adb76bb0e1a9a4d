// The host sizing of the lattice kernels (csrc/kh_lattice_plan.h) in a stand-alone program: the workgroups per CU, windows,
// LDS-resident states and staging sizes at every edge of the batch size, the window rule, the KH_LATTICE_WIN override, the
// LDS budget of a CU and the "same wave rewrites the slot" condition.  Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <cstdlib>

#include "../../old-kaldi-git_amd/csrc/kh_lattice_plan.h"

using namespace kh_latplan;

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond);          \
      failures++;                                                             \
    }                                                                         \
  } while (0)
#define EXPECT_EQ(a, b)                                                                                   \
  do {                                                                                                    \
    const long long a_ = static_cast<long long>(a), b_ = static_cast<long long>(b);                       \
    if (a_ != b_) {                                                                                       \
      std::printf("%s:%d: failed: %s = %lld, %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_);           \
      failures++;                                                                                         \
    }                                                                                                     \
  } while (0)

struct Row { int n_lats, per_cu, prep_win, lds_cap, stage, win_cap; };

// cus = 256: the values the kernels were measured and sized with
static const Row kRows[] = {
    {1, 1, 4096, 27392, 384, 16384},   {256, 1, 4096, 27392, 384, 16384}, {257, 2, 4096, 6912, 384, 4096},
    {512, 2, 4096, 6912, 384, 4096},   {513, 3, 1024, 6229, 192, 4096},   {768, 3, 1024, 6229, 192, 4096},
    {769, 4, 1024, 2816, 192, 2048},   {5000, 4, 1024, 2816, 192, 2048},
};

static int NextPow2(int v) {
  int p = 1;
  while (p < v) p *= 2;
  return p;
}

static void TestTable() {
  const int kMaxNs[] = {1, 2, 511, 512, 513, 1024, 1025, 2048, 2049, 2816, 2817, 4096, 4097, 5000, 6229, 6230, 6912, 6913,
                        8192, 8193, 16384, 16385, 27392, 27393, 200000, 1000000};
  for (const Row &r : kRows) {
    for (int max_ns : kMaxNs) {
      const PrepPlan p = PlanPrep(r.n_lats, max_ns, 256);
      EXPECT_EQ(p.per_cu, r.per_cu);
      EXPECT_EQ(p.win, r.prep_win);
      EXPECT_EQ(p.lds_states, max_ns < r.lds_cap ? max_ns : r.lds_cap);
      EXPECT_EQ(p.dyn_bytes, static_cast<size_t>(p.win) * 8 + static_cast<size_t>(p.lds_states) * 4);
      const SweepPlan s = PlanSweep(r.n_lats, max_ns, 256, 0);
      EXPECT_EQ(s.per_cu, r.per_cu);
      EXPECT_EQ(s.stage, r.stage);
      int want = NextPow2(max_ns);   // the smallest power of two >= max_ns, at least 512, at most the cap
      if (want < 512) want = 512;
      if (want > r.win_cap) want = r.win_cap;
      EXPECT_EQ(s.win, want);
      EXPECT_EQ(s.dyn_bytes, static_cast<size_t>(s.win) * 8);
    }
  }
  // a lattice is tagged exactly when it has more states than the window: the largest direct lattice per row
  EXPECT_EQ(PlanSweep(1, 16384, 256, 0).win, 16384);
  EXPECT_EQ(PlanSweep(1, 16385, 256, 0).win, 16384);
  EXPECT_EQ(PlanSweep(1000, 2048, 256, 0).win, 2048);
  EXPECT_EQ(PlanSweep(1000, 2049, 256, 0).win, 2048);
  // other CU counts move the edges with them
  EXPECT_EQ(PlanPrep(304, 100, 304).per_cu, 1);
  EXPECT_EQ(PlanPrep(305, 100, 304).per_cu, 2);
  EXPECT_EQ(PlanPrep(4, 100, 1).per_cu, 4);
  EXPECT_EQ(PlanPrep(3, 100, 1).per_cu, 3);
  EXPECT_EQ(PlanPrep(1, 100, 0).per_cu, 1);   // (a device that reports no CU count)
  EXPECT_EQ(kLevelPrepLdsStates, 5120);
  EXPECT(3 * kLevelPrepLdsStates * 4 <= 64 * 1024);   // PrepKernel's three static arrays stay within a workgroup's 64 KB
}

static void TestOverride() {
  for (int v = -4; v <= 40000; v++) {
    const bool pow2 = v > 0 && (v & (v - 1)) == 0;
    const bool valid = pow2 && v >= 512 && v <= 16384;
    EXPECT_EQ(ValidWinOverride(v), valid);
    for (int n_lats : {1, 1000}) {
      const SweepPlan base = PlanSweep(n_lats, 3000, 256, 0), s = PlanSweep(n_lats, 3000, 256, v);
      EXPECT_EQ(s.win, valid ? v : base.win);
      EXPECT_EQ(s.dyn_bytes, static_cast<size_t>(s.win) * 8);
      EXPECT_EQ(s.stage, base.stage);
      EXPECT_EQ(s.per_cu, base.per_cu);
    }
  }
  for (int v : {512, 1024, 2048, 4096, 8192, 16384}) EXPECT(ValidWinOverride(v));
  for (int v : {0, 256, 511, 513, 768, 16383, 16385, 32768}) EXPECT(!ValidWinOverride(v));
}

// per_cu workgroups with their dynamic + reserved static LDS fit a CU; every window keeps "the same wave rewrites the slot"
static void TestBudgetAndWaves() {
  for (int cus : {1, 64, 256, 304})
    for (int n_lats = 1; n_lats <= 2000; n_lats++)
      for (int max_ns : {1, 512, 513, 5000, 1000000}) {
        const PrepPlan p = PlanPrep(n_lats, max_ns, cus);
        EXPECT(p.per_cu >= 1 && p.per_cu <= kMaxPerCu);
        EXPECT(static_cast<size_t>(p.per_cu) * (p.dyn_bytes + kPrepStaticBytes) <= static_cast<size_t>(kLdsBytes));
        EXPECT(p.lds_states >= 1 && p.lds_states <= max_ns);
        EXPECT((p.win & (p.win - 1)) == 0);
        EXPECT((p.win / 64) % 4 == 0);
        EXPECT(SameWaveRewrites(p.win));
        const SweepPlan s = PlanSweep(n_lats, max_ns, cus, 0);
        EXPECT_EQ(s.per_cu, p.per_cu);
        EXPECT(static_cast<size_t>(s.per_cu) * (s.dyn_bytes + SweepStageBytes(s.stage)) <= static_cast<size_t>(kLdsBytes));
        EXPECT(s.win >= kWinMin && s.win <= kWinMax && (s.win & (s.win - 1)) == 0);
        EXPECT((s.win / 64) % 4 == 0);
        EXPECT(((s.win / 2) / 64) % 4 == 0);   // the tagged form keeps win / 2 value slots
        EXPECT(SameWaveRewrites(s.win / 2));
        EXPECT(s.stage == kStageLarge || s.stage == kStageSmall);
      }
  for (int v = kWinMin; v <= kWinMax; v *= 2) EXPECT(((v / 2) / 64) % 4 == 0 && SameWaveRewrites(v / 2));
  EXPECT(!SameWaveRewrites(128) && !SameWaveRewrites(0) && !SameWaveRewrites(320));
  EXPECT_EQ(SweepStageBytes(384), 24832);
  EXPECT_EQ(SweepStageBytes(192), 12544);
  EXPECT_EQ(kPrepStaticBytes, 21 * 1024);
}

int main() {
  TestTable();
  TestOverride();
  TestBudgetAndWaves();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
