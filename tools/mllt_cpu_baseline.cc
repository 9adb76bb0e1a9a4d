// mllt_cpu_baseline.cc - one host thread doing what the library's MLLT statistics route does after the posteriors
// (kh_rand_prune then kh_mllt_acc_stats, csrc/kh_mllt.hip), for tools/mllt_rate.py to time next to the device route and for
// tests/test_mllt_cpu_baseline.py to hold against tests/mllt_restatement.py.  Written as the reference writes it, one entry
// after another in frame order and one Gaussian after another (transform/mllt.cc:131-160): RandPrune of the posterior with the
// C library's rand(); the float mean = means_invvars / inv_vars, the float offset mean - data, widened; the packed outer
// product of the offset (exact in double); then, for every row j, G_j += double(float(inv_var[j] * posterior)) * tmp; beta
// adds each entry's double sum of its surviving posteriors.  Build with -ffp-contract=off: the double sums are then a product
// and an addition each.
//
//   mllt_cpu_baseline <input> <output>      prints "ms <prune> <accumulate>" on standard output
// input  (little endian): int32 T D num_pdfs M E seed (seed < 0: the generator is left unseeded); float rand_prune;
//        float feats[T*D] means_invvars[M*D] inv_vars[M*D]; int32 pdf_offsets[num_pdfs+1]; int64 frame_entry_offsets[T+1];
//        int32 entry_pdf[E]; float post[NP] (NP = the sum of the entries' pdf sizes: the posteriors, times the weight, unpruned)
// output: int64 NP; float pruned[NP]; int64 items; double beta; double G[D * D(D+1)/2] (row j the packed G_j)
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
    fprintf(stderr, "mllt_cpu_baseline: short input\n");
    exit(2);
  }
  return v;
}
template <typename T> void Write(FILE *f, const std::vector<T> &v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    fprintf(stderr, "mllt_cpu_baseline: short write\n");
    exit(2);
  }
}
double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// base/kaldi-math.h:169-175; the quotient is a double division (::fabs(double))
float RandPrune(float post, float thresh) {
  if (post == 0.0 || std::fabs(post) >= thresh) return post;
  const float u = static_cast<float>((rand() + 1.0) / (RAND_MAX + 2.0));
  return static_cast<float>((post >= 0 ? 1.0 : -1.0) * (u <= std::fabs(static_cast<double>(post)) / thresh ? thresh : 0.0));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mllt_cpu_baseline <input> <output>\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const std::vector<int32_t> h = Read<int32_t>(f, 6);
  const int T = h[0], D = h[1], num_pdfs = h[2], M = h[3], E = h[4], seed = h[5];
  const float thresh = Read<float>(f, 1)[0];
  if (T < 0 || D <= 0 || D > 1024 || num_pdfs <= 0 || M <= 0 || E < 0 || !(thresh >= 0.f)) {
    fprintf(stderr, "mllt_cpu_baseline: bad header\n");
    return 2;
  }
  const std::vector<float> feats = Read<float>(f, static_cast<size_t>(T) * D), mi = Read<float>(f, static_cast<size_t>(M) * D),
                           iv = Read<float>(f, static_cast<size_t>(M) * D);
  const std::vector<int32_t> pdf_off = Read<int32_t>(f, num_pdfs + 1);
  const std::vector<int64_t> feo = Read<int64_t>(f, T + 1);
  const std::vector<int32_t> entry_pdf = Read<int32_t>(f, E);
  // every index before it is used
  bool ok = pdf_off[0] == 0 && pdf_off[num_pdfs] == M && feo[0] == 0 && feo[T] == E;
  for (int j = 0; ok && j < num_pdfs; j++) ok = pdf_off[j + 1] > pdf_off[j];
  for (int t = 0; ok && t < T; t++) ok = feo[t + 1] >= feo[t];
  for (int e = 0; ok && e < E; e++) ok = entry_pdf[e] >= 0 && entry_pdf[e] < num_pdfs;
  if (!ok) {
    fprintf(stderr, "mllt_cpu_baseline: inconsistent offsets\n");
    return 2;
  }
  std::vector<int64_t> goff(E + 1, 0);
  for (int e = 0; e < E; e++) goff[e + 1] = goff[e] + pdf_off[entry_pdf[e] + 1] - pdf_off[entry_pdf[e]];
  std::vector<float> post = Read<float>(f, goff[E]);
  fclose(f);
  if (seed >= 0) srand(static_cast<unsigned>(seed));

  // ---- RandPrune in entry order then Gaussian order
  const double t0 = Now();
  for (float &p : post) p = RandPrune(p, thresh);
  // ---- AccumulateFromPosteriors per entry, in frame order
  const double t1 = Now();
  const int Q = D * (D + 1) / 2;
  std::vector<double> G(static_cast<size_t>(D) * Q, 0.0), tmp(Q), offset_dbl(D);
  double beta = 0.0;
  int64_t items = 0;
  for (int t = 0; t < T; t++) {
    const float *x = &feats[static_cast<size_t>(t) * D];
    for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
      const int m0 = pdf_off[entry_pdf[e]], n = pdf_off[entry_pdf[e] + 1] - m0;
      double this_beta = 0.0;
      for (int g = 0; g < n; g++) {
        const float posterior = post[goff[e] + g];
        if (posterior == 0.0) continue;
        const float *mir = &mi[static_cast<size_t>(m0 + g) * D], *ivr = &iv[static_cast<size_t>(m0 + g) * D];
        for (int d = 0; d < D; d++) {
          const float mean = mir[d] / ivr[d];
          offset_dbl[d] = static_cast<float>(mean - x[d]);
        }
        for (int a = 0, q = 0; a < D; a++)
          for (int b = 0; b <= a; b++, q++) tmp[q] = offset_dbl[a] * offset_dbl[b];
        for (int j = 0; j < D; j++) {
          const double alpha = static_cast<float>(ivr[j] * posterior);
          double *row = &G[static_cast<size_t>(j) * Q];
          for (int q = 0; q < Q; q++) row[q] += alpha * tmp[q];
        }
        this_beta += posterior;
        items++;
      }
      beta += this_beta;
    }
  }
  const double t2 = Now();
  FILE *o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  Write(o, std::vector<int64_t>{goff[E]});
  Write(o, post);
  Write(o, std::vector<int64_t>{items});
  Write(o, std::vector<double>{beta});
  Write(o, G);
  if (fclose(o) != 0) { perror(argv[2]); return 1; }
  printf("ms %.3f %.3f\n", t1 - t0, t2 - t1);
  return 0;
}
