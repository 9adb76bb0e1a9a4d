// gmm_rescore_cpu_baseline.cc — what gmm-rescore-lattice does per lattice, on ONE host thread, as the yardstick of
// tools/gmm_rescore_rate.py: state times, the list of (state, arc, transition-id) per frame, a walk over the frames in
// ascending order that adds -loglike to the owning weight in place, and a cache of one log-likelihood per (frame, pdf) filled
// on first use (a diagonal-covariance mixture: per Gaussian gconst + <mean/var, x> - 1/2 <1/var, x^2>, then log-sum-exp).
// Written for this repository; the batch arrives as the arrays of api.compact_lattice_rescore_raw behind int64 counts.
//   gmm_rescore_cpu_baseline in.bin out.bin [repeat]   -> prints the milliseconds of its best pass
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T>
static bool ReadArray(FILE *f, std::vector<T> *v) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n < 0) return false;
  v->resize(static_cast<size_t>(n));
  return n == 0 || fread(v->data(), sizeof(T), static_cast<size_t>(n), f) == static_cast<size_t>(n);
}

struct Owner { int32_t kind; int64_t index; int32_t tid; };   // kind 0: arc, 1: final weight

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: gmm_rescore_cpu_baseline in.bin out.bin [repeat]\n"); return 2; }
  const int repeat = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<int32_t> soff, next, strings, rows, tid2pdf, pdf_off, dims;
  std::vector<int64_t> aoff, aso, fso;
  std::vector<float> arc_a0, fin_g, fin_a0, feats, gconsts, mean_invvar, inv_var;
  const bool ok = ReadArray(f, &soff) && ReadArray(f, &aoff) && ReadArray(f, &next) && ReadArray(f, &arc_a0) && ReadArray(f, &aso) &&
                  ReadArray(f, &fin_g) && ReadArray(f, &fin_a0) && ReadArray(f, &fso) && ReadArray(f, &strings) && ReadArray(f, &rows) &&
                  ReadArray(f, &tid2pdf) && ReadArray(f, &dims) && ReadArray(f, &feats) && ReadArray(f, &gconsts) &&
                  ReadArray(f, &mean_invvar) && ReadArray(f, &inv_var) && ReadArray(f, &pdf_off);
  fclose(f);
  if (!ok || dims.size() != 1 || soff.empty()) { fprintf(stderr, "bad input file\n"); return 2; }
  const int D = dims[0], n_lats = static_cast<int>(soff.size()) - 1, n_pdfs = static_cast<int>(pdf_off.size()) - 1;
  std::vector<float> arc_a, fin_a, x2(D);
  double best_ms = 1e300;
  for (int pass = 0; pass < repeat; pass++) {
    arc_a = arc_a0;
    fin_a = fin_a0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> times;
    std::vector<std::vector<Owner> > at;
    std::vector<float> cache;
    std::vector<int32_t> cached_at;
    for (int l = 0; l < n_lats; l++) {
      const int32_t s0 = soff[l], ns = soff[l + 1] - s0;
      if (ns == 0) continue;
      times.assign(ns, -1);
      times[0] = 0;
      int32_t utt_len = -1;
      for (int32_t s = 0; s < ns; s++) {
        for (int64_t j = aoff[s0 + s]; j < aoff[s0 + s + 1]; j++)
          if (times[next[j]] == -1) times[next[j]] = times[s] + static_cast<int32_t>(aso[j + 1] - aso[j]);
        if (!(fin_g[s0 + s] == INFINITY && fin_a[s0 + s] == INFINITY))
          utt_len = std::max(utt_len, times[s] + static_cast<int32_t>(fso[s0 + s + 1] - fso[s0 + s]));
      }
      if (utt_len <= 0 || rows[l + 1] - rows[l] < utt_len) continue;
      at.assign(utt_len, std::vector<Owner>());
      for (int32_t s = 0; s < ns; s++) {
        const int32_t t = times[s];
        if (t < 0 || t >= utt_len) continue;
        for (int64_t j = aoff[s0 + s]; j < aoff[s0 + s + 1]; j++)
          for (int64_t k = aso[j]; k < aso[j + 1] && t + (k - aso[j]) < utt_len; k++) at[t + (k - aso[j])].push_back(Owner{0, j, strings[k]});
        for (int64_t k = fso[s0 + s]; k < fso[s0 + s + 1] && t + (k - fso[s0 + s]) < utt_len; k++)
          at[t + (k - fso[s0 + s])].push_back(Owner{1, s0 + s, strings[k]});
      }
      cache.assign(n_pdfs, 0.f);
      cached_at.assign(n_pdfs, -1);
      for (int32_t t = 0; t < utt_len; t++) {
        const float *x = feats.data() + static_cast<size_t>(rows[l] + t) * D;
        bool squared = false;
        for (const Owner &o : at[t]) {
          const int32_t pdf = tid2pdf[o.tid];
          if (cached_at[pdf] != t) {
            if (!squared) { for (int d = 0; d < D; d++) x2[d] = x[d] * x[d]; squared = true; }
            float mx = -INFINITY;
            const int32_t g0 = pdf_off[pdf], g1 = pdf_off[pdf + 1];
            std::vector<float> ll(g1 - g0);
            for (int32_t g = g0; g < g1; g++) {
              const float *mi = mean_invvar.data() + static_cast<size_t>(g) * D, *iv = inv_var.data() + static_cast<size_t>(g) * D;
              float a = 0.f, b = 0.f;
              for (int d = 0; d < D; d++) { a += mi[d] * x[d]; b += iv[d] * x2[d]; }
              ll[g - g0] = gconsts[g] + a - 0.5f * b;
              mx = std::max(mx, ll[g - g0]);
            }
            double sum = 0.0;
            for (float v : ll) sum += std::exp(static_cast<double>(v - mx));
            cache[pdf] = mx + static_cast<float>(std::log(sum));
            cached_at[pdf] = t;
          }
          float &w = o.kind == 0 ? arc_a[o.index] : fin_a[o.index];
          w = -cache[pdf] + w;
        }
      }
    }
    best_ms = std::min(best_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  f = fopen(argv[2], "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  fwrite(arc_a.data(), sizeof(float), arc_a.size(), f);
  fwrite(fin_a.data(), sizeof(float), fin_a.size(), f);
  fclose(f);
  printf("%.6f\n", best_ms);
  return 0;
}
