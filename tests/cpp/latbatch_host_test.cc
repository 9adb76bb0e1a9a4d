// latbatch_host_test.cc — the host-only helpers of csrc/kh_latbatch_host.h, alone: the incoming-arc lists, the refusals of
// a batch that is not top-sorted (with the texts the entry points report) and the chunk plan.  Built with plain g++ under
// -fsanitize=address,undefined by tests/test_latbatch_host.py; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../old-kaldi-git_amd/csrc/kh_latbatch_host.h"

namespace {

int g_failed = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                  \
    }                                                              \
  } while (0)

template <typename T>
bool Same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

struct Batch {
  std::vector<int32_t> lat_state_offsets{0}, start, next;
  std::vector<int64_t> arc_offsets{0};
  // a lattice given as its states' lists of destinations
  void Add(const std::vector<std::vector<int32_t>> &states, int32_t start_state = 0) {
    for (const auto &arcs : states) {
      next.insert(next.end(), arcs.begin(), arcs.end());
      arc_offsets.push_back(static_cast<int64_t>(next.size()));
    }
    lat_state_offsets.push_back(lat_state_offsets.back() + static_cast<int32_t>(states.size()));
    start.push_back(start_state);
  }
  int n_lats() const { return static_cast<int>(start.size()); }
};

bool Build(const Batch &b, bool with_start, kh::Incoming *in, std::string *err, std::vector<int64_t> *filled = nullptr) {
  return kh::BuildIncoming("kh_entry", b.n_lats(), b.lat_state_offsets.data(), with_start ? b.start.data() : nullptr,
                           b.arc_offsets.data(), b.next.data(), in, err, kh::NoLatHook(), kh::NoStateHook(), kh::NoArcHook(),
                           kh::NoLatHook(), [&](int l, int64_t k, int64_t j) {
                             if (filled) (*filled)[k] = j * 100 + l;
                           });
}

void TestIncoming() {
  kh::Incoming in;
  std::string err;
  Batch b;
  // arcs 0: 0->2, 1: 0->2 (parallel), 2: 0->3, 3: 1->2
  b.Add({{2, 2, 3}, {2}, {}, {}});
  // a second lattice: arcs 0: 0->1, 1: 0->2, 2: 1->2; then one state without arcs
  b.Add({{1, 2}, {2}, {}});
  b.Add({{}});
  std::vector<int64_t> filled(7, -1);
  CHECK(Build(b, true, &in, &err, &filled));
  CHECK(err.empty());
  CHECK(Same<int64_t>(in.in_off, {0, 0, 0, 3, 4, 4, 5, 7, 7}));
  CHECK(Same<int32_t>(in.in_src, {0, 0, 1, 0, 0, 0, 1}));     // state-relative; state 2's list in (source, position) order
  CHECK(Same<int32_t>(in.in_arc, {0, 1, 3, 2, 0, 1, 2}));     // relative to the lattice's first arc
  CHECK(Same<int64_t>(filled, {0, 100, 300, 200, 401, 501, 601}));   // (k, batch arc j, lattice l) of every arc, once

  Batch one;
  one.Add({{}});
  CHECK(Build(one, true, &in, &err));
  CHECK(Same<int64_t>(in.in_off, {0, 0}) && in.in_src.empty() && in.in_arc.empty());

  Batch none;                                                  // A == 0 over several lattices
  none.Add({{}, {}});
  none.Add({{}});
  CHECK(Build(none, false, &in, &err));
  CHECK(Same<int64_t>(in.in_off, {0, 0, 0, 0}) && in.in_src.empty() && in.in_arc.empty());
}

void Refused(const Batch &b, bool with_start, const std::string &text) {
  kh::Incoming in;
  std::string err;
  CHECK(!Build(b, with_start, &in, &err));
  if (err != text) {
    std::printf("refusal: got  \"%s\"\n         want \"%s\"\n", err.c_str(), text.c_str());
    g_failed++;
  }
}

void TestRefusals() {
  const std::string tail = ": input lattice must be topologically sorted";
  Batch ok;
  ok.Add({{1}, {}});
  {
    Batch b = ok;                                              // a self-loop, in the second lattice
    b.Add({{1}, {1}, {}});
    Refused(b, true, "kh_entry: lattice 1: arc 1 (state 1 -> 1 of 3)" + tail);
  }
  {
    Batch b;                                                   // an arc to a lower state
    b.Add({{1, 0}, {2}, {}});
    Refused(b, false, "kh_entry: lattice 0: arc 1 (state 0 -> 0 of 3)" + tail);
  }
  {
    Batch b;                                                   // an arc to ns
    b.Add({{1}, {3}, {}});
    Refused(b, false, "kh_entry: lattice 0: arc 1 (state 1 -> 3 of 3)" + tail);
  }
  {
    Batch b;
    b.Add({{1}, {2}, {}}, -1);
    Refused(b, true, "kh_entry: lattice 0: start state -1 of 3 states");
    kh::Incoming in;
    std::string err;
    CHECK(Build(b, false, &in, &err));                         // (an entry point without start states does not look)
  }
  {
    Batch b = ok;
    b.Add({{1}, {2}, {}}, 3);
    Refused(b, true, "kh_entry: lattice 1: start state 3 of 3 states");
  }
  {
    std::string err;                                           // the single-arc form, as kh_latrescore.hip uses it
    CHECK(kh::ForwardArc("kh_entry", 2, 5, 1, 2, 3, &err) && err.empty());
    CHECK(!kh::ForwardArc("kh_entry", 2, 5, 1, 1, 3, &err));
    CHECK(err == "kh_entry: lattice 2: arc 5 (state 1 -> 1 of 3)" + tail);
  }
  {
    // hooks run in the walk's order and the first refusal wins: the state hook of state 0 comes before the bad arc of state 0
    Batch b;
    b.Add({{0}, {}});
    kh::Incoming in;
    std::string err;
    const bool r = kh::BuildIncoming("kh_entry", 1, b.lat_state_offsets.data(), nullptr, b.arc_offsets.data(), b.next.data(), &in,
                                     &err, kh::NoLatHook(),
                                     [&](int l, int32_t, int32_t s) { return kh::Refuse(&err, "state hook %d %d", l, s); });
    CHECK(!r && err == "state hook 0 0");
  }
}

void TestPlanChunks() {
  const size_t huge = ~static_cast<size_t>(0) / 2;
  {
    const kh::ChunkPlan p = kh::PlanChunks({5, 7, 5, 7, 1}, huge);   // ties keep the input order
    CHECK(Same<int32_t>(p.order, {1, 3, 0, 2, 4}));
    CHECK(p.ranges.size() == 1 && p.ranges[0].begin == 0 && p.ranges[0].end == 5);
  }
  {
    const kh::ChunkPlan p = kh::PlanChunks({3, 10, 3}, 6);           // the item above the limit runs alone
    CHECK(Same<int32_t>(p.order, {1, 0, 2}));
    CHECK(p.ranges.size() == 2 && p.ranges[0].begin == 0 && p.ranges[0].end == 1 && p.ranges[1].begin == 1 && p.ranges[1].end == 3);
  }
  {
    const kh::ChunkPlan fit = kh::PlanChunks({4, 6}, 10), tight = kh::PlanChunks({4, 6}, 9);
    CHECK(fit.ranges.size() == 1 && fit.ranges[0].end == 2);
    CHECK(tight.ranges.size() == 2 && tight.ranges[0].end == 1 && tight.ranges[1].begin == 1 && tight.ranges[1].end == 2);
  }
  {
    const std::vector<size_t> ones(65536, 1);
    const kh::ChunkPlan p = kh::PlanChunks(ones, huge);
    CHECK(p.ranges.size() == 2 && p.ranges[0].begin == 0 && p.ranges[0].end == 65535 && p.ranges[1].begin == 65535 &&
          p.ranges[1].end == 65536);
    std::vector<int> seen(ones.size(), 0);
    for (const kh::ChunkRange &c : p.ranges)
      for (size_t i = c.begin; i < c.end; i++) seen[p.order[i]]++;
    bool once = true;
    for (int n : seen) once = once && n == 1;
    CHECK(once);
  }
  {
    const std::vector<size_t> sizes{9, 1, 8}, keys{1, 2, 3};         // keys decide the order, sizes the filling
    const kh::ChunkPlan p = kh::PlanChunks(sizes, 9, 65535, &keys);
    CHECK(Same<int32_t>(p.order, {2, 1, 0}));
    CHECK(p.ranges.size() == 2 && p.ranges[0].end == 2 && p.ranges[1].end == 3);
  }
  CHECK(kh::PlanChunks({}, 1).ranges.empty());
}

}  // namespace

int main() {
  TestIncoming();
  TestRefusals();
  TestPlanChunks();
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
