// tree_plan_test.cc - the host plan of kh_tree_acc_stats (csrc/kh_tree_plan.h) on its edge cases, as a program of its own:
// built with plain g++, with and without -fsanitize=address,undefined, by tests/test_tree_plan_host.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../old-kaldi-git_amd/csrc/kh_tree_plan.h"

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

using kh_tree::Plan;

// what every plan must satisfy: the runs partition the used frames, ascending within a run; the items cover every event
// with a frame once per column block, in falling run length
static void Invariants(const std::vector<int32_t> &fe, int E, int D, const Plan &p) {
  const int T = static_cast<int>(fe.size());
  CHECK(static_cast<int>(p.event_offsets.size()) == E + 1 && p.event_offsets[0] == 0);
  int used = 0, events_used = 0, longest = 0;
  std::vector<int> seen(T, 0);
  for (int e = 0; e < E; e++) {
    const int b = p.event_offsets[e], n = p.event_offsets[e + 1] - b;
    CHECK(n >= 0);
    used += n;
    events_used += n > 0;
    if (n > longest) longest = n;
    for (int i = 0; i < n; i++) {
      const int t = p.sorted_row[b + i];
      CHECK(t >= 0 && t < T && fe[t] == e && !seen[t]);
      CHECK(i == 0 || p.sorted_row[b + i - 1] < t);
      seen[t] = 1;
    }
  }
  int want_used = 0;
  for (int t = 0; t < T; t++) want_used += fe[t] >= 0;
  CHECK(used == want_used && p.used == used && static_cast<int>(p.sorted_row.size()) == used);
  CHECK(p.events_used == events_used && p.longest == longest);
  const int blocks = kh_tree::ColumnBlocks(D);
  CHECK(p.work_event.size() == static_cast<size_t>(events_used) * blocks && p.work_block.size() == p.work_event.size());
  for (size_t w = 0; w < p.work_event.size(); w++) {
    const int e = p.work_event[w];
    CHECK(e >= 0 && e < E && p.event_offsets[e + 1] > p.event_offsets[e]);
    CHECK(p.work_block[w] == static_cast<int>(w % blocks));
    if (w % blocks) CHECK(p.work_event[w - 1] == e);
    if (w >= static_cast<size_t>(blocks)) {
      const int q = p.work_event[w - blocks];
      const int nq = p.event_offsets[q + 1] - p.event_offsets[q], ne = p.event_offsets[e + 1] - p.event_offsets[e];
      if (w % blocks == 0) CHECK(nq > ne || (nq == ne && q < e));
    }
  }
}

static Plan Run(const std::vector<int32_t> &fe, int E, int D) {
  std::string err;
  CHECK(kh_tree::Check(static_cast<int>(fe.size()), fe.data(), E, &err));
  Plan p;
  kh_tree::Build(static_cast<int>(fe.size()), fe.data(), E, D, &p);
  Invariants(fe, E, D, p);
  return p;
}

int main() {
  {  // empty input, with and without events
    Plan p = Run({}, 0, 40);
    CHECK(p.used == 0 && p.work_event.empty() && p.longest == 0);
    p = Run({}, 5, 40);
    CHECK(p.used == 0 && p.work_event.empty() && p.event_offsets.size() == 6);
    std::string err;
    CHECK(kh_tree::Check(0, nullptr, 0, &err));
  }
  {  // all frames -1
    Plan p = Run(std::vector<int32_t>(100, -1), 3, 65);
    CHECK(p.used == 0 && p.events_used == 0 && p.work_event.empty());
    p = Run(std::vector<int32_t>(7, -1), 0, 1);
    CHECK(p.used == 0 && p.work_event.empty());
  }
  {  // one event holding everything
    Plan p = Run(std::vector<int32_t>(1000, 2), 4, 130);
    CHECK(p.used == 1000 && p.events_used == 1 && p.longest == 1000 && p.work_event.size() == 3);
    for (int i = 0; i < 1000; i++) CHECK(p.sorted_row[i] == i);
    CHECK(p.work_event[0] == 2 && p.work_block[2] == 2);
  }
  {  // E events of one frame each, met backwards
    const int E = 500;
    std::vector<int32_t> fe(E);
    for (int t = 0; t < E; t++) fe[t] = E - 1 - t;
    Plan p = Run(fe, E, 64);
    CHECK(p.used == E && p.events_used == E && p.longest == 1 && p.work_event.size() == static_cast<size_t>(E));
    for (int e = 0; e < E; e++) CHECK(p.sorted_row[e] == E - 1 - e && p.work_event[e] == e);   // ties: by rising event
  }
  {  // interleaved runs of different lengths with unused frames: longest first, stable within an event
    std::vector<int32_t> fe;
    for (int t = 0; t < 600; t++) fe.push_back(t % 7 == 0 ? -1 : (t % 3 == 0 ? 1 : (t % 5 == 0 ? 3 : 0)));
    Plan p = Run(fe, 5, 512);
    CHECK(p.events_used == 3 && p.work_event.size() == 24 && p.work_event[0] == 0 && p.work_event[8] == 1 && p.work_event[16] == 3);
  }
  {  // refusals name the frame
    std::string err;
    const std::vector<int32_t> high = {0, 1, 2}, low = {0, -2};
    CHECK(!kh_tree::Check(3, high.data(), 2, &err) && err == "frame 2 names event 2, the call has 2 events (-1: frame not used)");
    CHECK(!kh_tree::Check(2, low.data(), 2, &err) && err == "frame 1 names event -2, the call has 2 events (-1: frame not used)");
    CHECK(!kh_tree::Check(1, high.data(), 0, &err) && err == "frame 0 names event 0, the call has 0 events (-1: frame not used)");
  }
  std::printf("ok\n");
  return 0;
}
