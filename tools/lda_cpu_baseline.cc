// lda_cpu_baseline.cc - one host thread doing what the library's LDA statistics route does (kh_rand_prune_at then
// kh_lda_acc_stats, csrc/kh_lda.hip), for tools/lda_rate.py to time next to the device route and for
// tests/test_lda_cpu_baseline.py to hold against tests/lda_restatement.py.  Our own statement of the accumulation: one
// entry after another in frame order; RandPrune of the weight with the C library's rand(); for a weight that is not zero the
// row widened to double, the count, the class's first-order row  first[c][d] += w x[d],  and the packed rank-one update of
// the second-order matrix, row by row of its lower triangle:  second[r (r + 1) / 2 + c] += x[c] * (w x[r]).  Build with
// -ffp-contract=off: the double sums are then a product and an addition each.
//
//   lda_cpu_baseline <input> <output>      prints "ms <prune> <accumulate>" on standard output
// input  (little endian): int32 T D C E seed (seed < 0: the generator is left unseeded); float rand_prune; float feats[T*D];
//        int64 frame_entry_offsets[T+1]; int32 entry_pdf[E]; float entry_weight[E] (unpruned)
// output: float pruned[E]; int64 items; double zero[C] first[C*D] second[D(D+1)/2]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

template <typename T> std::vector<T> Read(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "lda_cpu_baseline: short input\n");
    exit(2);
  }
  return v;
}
template <typename T> void Write(FILE *f, const std::vector<T> &v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    fprintf(stderr, "lda_cpu_baseline: short write\n");
    exit(2);
  }
}
double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// RandPrune; the quotient is a double division
float RandPrune(float post, float thresh) {
  if (post == 0.0 || std::fabs(post) >= thresh) return post;
  const float u = static_cast<float>((rand() + 1.0) / (RAND_MAX + 2.0));
  return static_cast<float>((post >= 0 ? 1.0 : -1.0) * (u <= std::fabs(static_cast<double>(post)) / thresh ? thresh : 0.0));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: lda_cpu_baseline <input> <output>\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const std::vector<int32_t> h = Read<int32_t>(f, 5);
  const int T = h[0], D = h[1], C = h[2], E = h[3], seed = h[4];
  const float thresh = Read<float>(f, 1)[0];
  if (T < 0 || D <= 0 || D > 4096 || C <= 0 || E < 0 || !(thresh >= 0.f)) {
    fprintf(stderr, "lda_cpu_baseline: bad header\n");
    return 2;
  }
  const std::vector<float> feats = Read<float>(f, static_cast<size_t>(T) * D);
  const std::vector<int64_t> feo = Read<int64_t>(f, T + 1);
  const std::vector<int32_t> entry_pdf = Read<int32_t>(f, E);
  std::vector<float> weight = Read<float>(f, E);
  fclose(f);
  // every index before it is used
  bool ok = feo[0] == 0 && feo[T] == E;
  for (int t = 0; ok && t < T; t++) ok = feo[t + 1] >= feo[t];
  for (int e = 0; ok && e < E; e++) ok = entry_pdf[e] >= 0 && entry_pdf[e] < C;
  if (!ok) {
    fprintf(stderr, "lda_cpu_baseline: inconsistent offsets\n");
    return 2;
  }
  if (seed >= 0) srand(static_cast<unsigned>(seed));

  // ---- RandPrune in entry order
  const double t0 = Now();
  for (float &w : weight) w = RandPrune(w, thresh);
  // ---- the accumulation, entry by entry in frame order
  const double t1 = Now();
  const size_t Q = static_cast<size_t>(D) * (D + 1) / 2;
  std::vector<double> zero(C, 0.0), first(static_cast<size_t>(C) * D, 0.0), second(Q, 0.0), x(D);
  int64_t items = 0;
  for (int t = 0; t < T; t++) {
    for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
      if (weight[e] == 0.0) continue;
      const double w = weight[e];
      for (int d = 0; d < D; d++) x[d] = feats[static_cast<size_t>(t) * D + d];
      zero[entry_pdf[e]] += w;
      double *row = &first[static_cast<size_t>(entry_pdf[e]) * D];
      for (int d = 0; d < D; d++) row[d] += w * x[d];
      double *ap = second.data();
      for (int r = 0; r < D; r++) {
        const double temp = w * x[r];
        for (int c = 0; c <= r; c++) ap[c] += x[c] * temp;
        ap += r + 1;
      }
      items++;
    }
  }
  const double t2 = Now();
  FILE *o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  Write(o, weight);
  Write(o, std::vector<int64_t>{items});
  Write(o, zero);
  Write(o, first);
  Write(o, second);
  if (fclose(o) != 0) { perror(argv[2]); return 1; }
  printf("ms %.3f %.3f\n", t1 - t0, t2 - t1);
  return 0;
}
