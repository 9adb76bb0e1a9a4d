// gselect_plan_test.cc - the host side of kh_gmm_gselect and kh_gmm_preselect_posteriors (csrc/kh_gselect_plan.h) on its edge
// cases, as a program of its own: built with plain g++, with and without -fsanitize=address,undefined, by
// tests/test_gselect_plan_host.py.  With an argument it prints the refusal of that case (the Python test holds the texts);
// without one it runs the checks and prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../old-kaldi-git_amd/csrc/kh_gselect_plan.h"

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

using kh_gselect::CheckLists;

struct Case {
  const char *name;
  std::vector<int64_t> off;
  std::vector<int32_t> gauss;
  std::vector<float> weight;   // empty: no weights
  int num_gauss, max_len;
  bool refuse_twice;
};

static std::string Run(const Case &c) {
  std::string err;
  const int T = static_cast<int>(c.off.size()) - 1;
  const bool ok = CheckLists(T, c.off.data(), c.gauss.data(), c.num_gauss, c.max_len, c.weight.empty() ? nullptr : c.weight.data(),
                             c.refuse_twice, "sel_offsets", &err);
  CHECK(ok == err.empty());
  return err;
}

int main(int argc, char **argv) {
  const std::vector<Case> refusals = {
      {"first", {1, 2}, {0, 0}, {}, 4, 4, true},
      {"backwards", {0, 2, 1, 3}, {0, 1, 2}, {}, 4, 4, true},
      {"negative", {0, 1, 3}, {0, 1, -1}, {}, 4, 4, true},
      {"range", {0, 1, 3}, {0, 1, 4}, {}, 4, 4, true},
      {"empty", {0, 1, 1, 2}, {0, 1}, {}, 4, 4, true},
      {"twice", {0, 2, 5}, {0, 1, 2, 3, 2}, {}, 4, 4, true},
      {"long", {0, 1, 4}, {0, 0, 1, 0}, {}, 4, 2, false},
  };
  if (argc > 1) {
    for (const Case &c : refusals)
      if (!std::strcmp(argv[1], c.name)) {
        std::printf("%s\n", Run(c).c_str());
        return 0;
      }
    return 2;
  }
  for (const Case &c : refusals) CHECK(!Run(c).empty());
  // no frame; one frame; the same Gaussian in two frames; twice allowed for a preselection
  CHECK(Run({"", {0}, {}, {}, 4, 4, true}).empty());
  CHECK(Run({"", {0, 4}, {3, 2, 1, 0}, {}, 4, 4, true}).empty());
  CHECK(Run({"", {0, 2, 4}, {1, 2, 2, 1}, {}, 4, 4, true}).empty());
  CHECK(Run({"", {0, 2, 5}, {0, 1, 2, 3, 2}, {}, 4, 4, false}).empty());
  // a frame of weight 0 (and -0) is not looked at: empty, out of range, twice
  CHECK(Run({"", {0, 1, 1, 2}, {0, 1}, {1.f, 0.f, 2.f}, 4, 4, true}).empty());
  CHECK(Run({"", {0, 1, 3, 4}, {0, 9, 9, 1}, {1.f, -0.f, -1.f}, 4, 4, true}).empty());
  CHECK(!Run({"", {0, 1, 3, 4}, {0, 9, 9, 1}, {1.f, 1e-30f, -1.f}, 4, 4, true}).empty());
  // the used frames, in order
  {
    const float w[5] = {1.f, 0.f, -2.f, -0.f, 0.5f};
    CHECK((kh_gselect::UsedFrames(5, w) == std::vector<int32_t>{0, 2, 4}));
    CHECK((kh_gselect::UsedFrames(3, nullptr) == std::vector<int32_t>{0, 1, 2}));
    CHECK(kh_gselect::UsedFrames(0, nullptr).empty());
  }
  // the row chunks: at least one row, at most T, the limit's whole rows between
  CHECK(kh_gselect::ChunkRows(100, 10, 0) == 1);
  CHECK(kh_gselect::ChunkRows(100, 10, 39) == 1);
  CHECK(kh_gselect::ChunkRows(100, 10, 40) == 1);
  CHECK(kh_gselect::ChunkRows(100, 10, 119) == 2);
  CHECK(kh_gselect::ChunkRows(100, 10, 120) == 3);
  CHECK(kh_gselect::ChunkRows(100, 10, size_t(1) << 40) == 100);
  CHECK(kh_gselect::ChunkRows(0, 10, size_t(1) << 40) == 1);
  CHECK(kh_gselect::ChunkRows(2147483647, 4096, ~size_t(0)) == 2147483647);
  std::printf("ok\n");
  return 0;
}
