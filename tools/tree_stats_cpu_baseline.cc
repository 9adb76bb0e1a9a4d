// tree_stats_cpu_baseline.cc - one host thread doing what acc-tree-stats' inner loop does, for tools/tree_stats_rate.py to time
// next to the library's route (kh_tree_acc_stats, csrc/kh_tree.hip) and for tests/test_tree_stats_cpu_baseline.py to hold
// against tests/tree_stats_restatement.py.  Our own statement of the accumulation: frame after frame, the frame's event - a
// sorted vector of (key, value) pairs - is built and looked up in a std::map of events, inserted with zero statistics when
// it is new, and the row is added: the count by one, the first-order row by double(x[d]), the second-order row by the
// float-rounded product x[d] * x[d] widened to double.  Build with -ffp-contract=off.
//
//   tree_stats_cpu_baseline <input> <output>      prints "ms <accumulate>" on standard output
// input  (little endian): int32 T D E P; float feats[T*D]; int32 frame_event[T] (-1: frame not used); int32 event_offsets[E+1]
//        into int32 pairs[2*P] (key, value, key, value ...): event e is pairs[2*event_offsets[e] ... 2*event_offsets[e+1])
// output: int64 n; per event in map order: int32 n_pairs; int32 pairs[2*n_pairs]; double count; double stats[2*D]
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace {

template <typename T> std::vector<T> Read(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "tree_stats_cpu_baseline: short input\n");
    exit(2);
  }
  return v;
}
template <typename T> void Write(FILE *f, const T *p, size_t n) {
  if (n && fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "tree_stats_cpu_baseline: short write\n");
    exit(2);
  }
}
double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

typedef std::vector<std::pair<int32_t, int32_t> > Event;
struct Stats {
  double count = 0.0;
  std::vector<double> sums;   // [2][D]
};

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: tree_stats_cpu_baseline <input> <output>\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const std::vector<int32_t> h = Read<int32_t>(f, 4);
  const int T = h[0], D = h[1], E = h[2], P = h[3];
  if (T < 0 || D <= 0 || D > 4096 || E < 0 || P < 0) {
    fprintf(stderr, "tree_stats_cpu_baseline: bad header\n");
    return 2;
  }
  const std::vector<float> feats = Read<float>(f, static_cast<size_t>(T) * D);
  const std::vector<int32_t> frame_event = Read<int32_t>(f, T);
  const std::vector<int32_t> offsets = Read<int32_t>(f, static_cast<size_t>(E) + 1);
  const std::vector<int32_t> pairs = Read<int32_t>(f, 2 * static_cast<size_t>(P));
  fclose(f);
  // every index before it is used
  bool ok = offsets[0] == 0 && offsets[E] == P;
  for (int e = 0; ok && e < E; e++) ok = offsets[e + 1] >= offsets[e];
  for (int t = 0; ok && t < T; t++) ok = frame_event[t] >= -1 && frame_event[t] < E;
  if (!ok) {
    fprintf(stderr, "tree_stats_cpu_baseline: inconsistent offsets\n");
    return 2;
  }

  const double t0 = Now();
  std::map<Event, Stats> stats;
  Event event;
  for (int t = 0; t < T; t++) {
    const int e = frame_event[t];
    if (e < 0) continue;
    event.clear();
    for (int i = offsets[e]; i < offsets[e + 1]; i++) event.push_back(std::make_pair(pairs[2 * i], pairs[2 * i + 1]));
    std::map<Event, Stats>::iterator it = stats.find(event);
    if (it == stats.end()) {
      it = stats.insert(std::make_pair(event, Stats())).first;
      it->second.sums.assign(2 * static_cast<size_t>(D), 0.0);
    }
    const float *x = &feats[static_cast<size_t>(t) * D];
    double *s1 = it->second.sums.data(), *s2 = s1 + D;
    it->second.count += 1.0;
    for (int d = 0; d < D; d++) s1[d] += x[d];
    for (int d = 0; d < D; d++) s2[d] += x[d] * x[d];       // float operands: the product is rounded to float
  }
  const double t1 = Now();

  FILE *o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  const int64_t n = static_cast<int64_t>(stats.size());
  Write(o, &n, 1);
  for (std::map<Event, Stats>::const_iterator it = stats.begin(); it != stats.end(); ++it) {
    const int32_t np = static_cast<int32_t>(it->first.size());
    Write(o, &np, 1);
    for (size_t i = 0; i < it->first.size(); i++) {
      Write(o, &it->first[i].first, 1);
      Write(o, &it->first[i].second, 1);
    }
    Write(o, &it->second.count, 1);
    Write(o, it->second.sums.data(), it->second.sums.size());
  }
  if (fclose(o) != 0) { perror(argv[2]); return 1; }
  printf("ms %.3f\n", t1 - t0);
  return 0;
}
