// gmm_acc_cpu_baseline.cc - one host thread doing what the library's GMM statistics route does (kh_gmm_acc_component_posteriors then
// kh_gmm_acc_stats, csrc/kh_gmmacc.hip), for tools/gmm_acc_rate.py to time next to the device route and
// for tests/test_gmm_acc_cpu_baseline.py to hold against tests/gmm_acc_restatement.py.  Written as the reference writes it, one
// entry after another in frame order: ComponentPosteriors and Scale(weight) (gmm/diag-gmm.cc:601-615,
// gmm/mle-diag-gmm.cc:198-200), then AccumulateFromPosteriors (:171-189) in double - occupancy_.AddVec, AddVecVec on the means,
// ApplyPow(2.0), AddVecVec on the variances - and total_log_like_ / total_frames_ (gmm/mle-am-diag-gmm.cc:76-77).
// expf / logf are the host libm's.  Build with -ffp-contract=off: the double sums are then a product and an addition each.
//
//   gmm_acc_cpu_baseline <input> <output>      prints "ms <posteriors> <accumulate>" on standard output
// input  (little endian): int32 T D D2 num_pdfs M E flags; float feats[T*D] feats2[T*D2] gconsts[M] means_invvars[M*D]
//        inv_vars[M*D]; int32 pdf_offsets[num_pdfs+1]; int64 frame_entry_offsets[T+1]; int32 entry_pdf[E]; float entry_weight[E]
//        (feats2: the features the statistics are taken from; flags: m 1 | v 2 | w 4, augmented by the caller)
// output: int64 n_post; float post[n_post] like[E]; double occ[M] mean_acc[M*D2] var_acc[M*D2] total_like total_frames
//        (an accumulator the flags exclude is written as zeros)
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
    fprintf(stderr, "gmm_acc_cpu_baseline: short input\n");
    exit(2);
  }
  return v;
}
template <typename T> void Write(FILE *f, const std::vector<T> &v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    fprintf(stderr, "gmm_acc_cpu_baseline: short write\n");
    exit(2);
  }
}
double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: gmm_acc_cpu_baseline <input> <output>\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const std::vector<int32_t> h = Read<int32_t>(f, 7);
  const int T = h[0], D = h[1], D2 = h[2], num_pdfs = h[3], M = h[4], E = h[5], flags = h[6];
  if (T < 0 || D <= 0 || D2 <= 0 || num_pdfs <= 0 || M <= 0 || E < 0 || (flags & ~7) || !(flags & 4) || ((flags & 2) && !(flags & 1))) {
    fprintf(stderr, "gmm_acc_cpu_baseline: bad header\n");
    return 2;
  }
  const std::vector<float> feats = Read<float>(f, static_cast<size_t>(T) * D), feats2 = Read<float>(f, static_cast<size_t>(T) * D2),
                           gconsts = Read<float>(f, M), mi = Read<float>(f, static_cast<size_t>(M) * D),
                           iv = Read<float>(f, static_cast<size_t>(M) * D);
  const std::vector<int32_t> pdf_off = Read<int32_t>(f, num_pdfs + 1);
  const std::vector<int64_t> feo = Read<int64_t>(f, T + 1);
  const std::vector<int32_t> entry_pdf = Read<int32_t>(f, E);
  const std::vector<float> entry_w = Read<float>(f, E);
  fclose(f);
  // every index before it is used
  bool ok = pdf_off[0] == 0 && pdf_off[num_pdfs] == M && feo[0] == 0 && feo[T] == E;
  for (int j = 0; ok && j < num_pdfs; j++) ok = pdf_off[j + 1] > pdf_off[j];
  for (int t = 0; ok && t < T; t++) ok = feo[t + 1] >= feo[t];
  for (int e = 0; ok && e < E; e++) ok = entry_pdf[e] >= 0 && entry_pdf[e] < num_pdfs;
  if (!ok) {
    fprintf(stderr, "gmm_acc_cpu_baseline: inconsistent offsets\n");
    return 2;
  }
  const bool means = flags & 1, vars = flags & 2;

  // ---- ComponentPosteriors and Scale(weight) per entry
  const double t0 = Now();
  std::vector<int64_t> goff(E + 1, 0);
  for (int e = 0; e < E; e++) goff[e + 1] = goff[e] + pdf_off[entry_pdf[e] + 1] - pdf_off[entry_pdf[e]];
  std::vector<float> post(goff[E]), like(E);
  for (int t = 0; t < T; t++) {
    const float *x = &feats[static_cast<size_t>(t) * D];
    for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
      const int m0 = pdf_off[entry_pdf[e]], n = pdf_off[entry_pdf[e] + 1] - m0;
      float *p = &post[goff[e]];
      float mx = -HUGE_VALF;
      for (int g = 0; g < n; g++) {
        const float *mir = &mi[static_cast<size_t>(m0 + g) * D], *ivr = &iv[static_cast<size_t>(m0 + g) * D];
        float a1 = 0.f, a2 = 0.f;
        for (int d = 0; d < D; d++) {
          a1 = fmaf(x[d], mir[d], a1);
          a2 = fmaf(x[d] * x[d], ivr[d], a2);
        }
        p[g] = (gconsts[m0 + g] + a1) + (-0.5f * a2);
        if (p[g] > mx) mx = p[g];
      }
      float sum = 0.f;
      for (int g = 0; g < n; g++) sum += (p[g] = expf(p[g] - mx));
      const float inv = static_cast<float>(1.0 / sum);
      for (int g = 0; g < n; g++) p[g] = (p[g] * inv) * entry_w[e];
      like[e] = mx + logf(sum);
    }
  }
  // ---- AccumulateFromPosteriors per entry, in frame order
  const double t1 = Now();
  std::vector<double> occ(M, 0.0), mean_acc(static_cast<size_t>(M) * D2, 0.0), var_acc(static_cast<size_t>(M) * D2, 0.0), data_d(D2);
  double total_like = 0.0, total_frames = 0.0;
  for (int t = 0; t < T; t++) {
    const float *x2 = &feats2[static_cast<size_t>(t) * D2];
    for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
      const int m0 = pdf_off[entry_pdf[e]], n = pdf_off[entry_pdf[e] + 1] - m0;
      const float *p = &post[goff[e]];
      for (int g = 0; g < n; g++) occ[m0 + g] += static_cast<double>(p[g]);
      if (means) {
        for (int d = 0; d < D2; d++) data_d[d] = x2[d];
        for (int g = 0; g < n; g++) {
          const double pg = p[g];
          double *row = &mean_acc[static_cast<size_t>(m0 + g) * D2];
          for (int d = 0; d < D2; d++) row[d] += pg * data_d[d];
        }
        if (vars) {
          for (int d = 0; d < D2; d++) data_d[d] = data_d[d] * data_d[d];
          for (int g = 0; g < n; g++) {
            const double pg = p[g];
            double *row = &var_acc[static_cast<size_t>(m0 + g) * D2];
            for (int d = 0; d < D2; d++) row[d] += pg * data_d[d];
          }
        }
      }
      total_like += static_cast<double>(like[e] * entry_w[e]);
      total_frames += static_cast<double>(entry_w[e]);
    }
  }
  const double t2 = Now();
  FILE *o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  Write(o, std::vector<int64_t>{goff[E]});
  Write(o, post);
  Write(o, like);
  Write(o, occ);
  Write(o, mean_acc);
  Write(o, var_acc);
  Write(o, std::vector<double>{total_like, total_frames});
  if (fclose(o) != 0) { perror(argv[2]); return 1; }
  printf("ms %.3f %.3f\n", t1 - t0, t2 - t1);
  return 0;
}
