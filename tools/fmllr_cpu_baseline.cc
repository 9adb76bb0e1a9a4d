// fmllr_cpu_baseline.cc - one host thread doing what the library's four fMLLR stages do (csrc/kh_fmllr.hip), for
// tools/fmllr_rate.py to time next to the device route and for tests/test_fmllr_cpu_baseline.py to hold against
// tests/fmllr_restatement.py.  A1 and A2 are written as the reference writes them (one entry after another, the single-frame
// statistics committed when the data changes: transform/fmllr-diag-gmm.cc:30-43, :542-596), B adds every merged frame's
// scaled scatter into the D packed matrices in frame order (:562-596), C is the library's own host source
// (csrc/kh_fmllr_update.h).  expf / logf are the host libm's.
//
//   fmllr_cpu_baseline <input> <output>      prints "ms <A1> <A2> <B> <C>" on standard output
// input  (little endian): int32 T D num_pdfs M n_utts n_spk E type num_iters; float min_count;
//        float feats[T*D] gconsts[M] means_invvars[M*D] inv_vars[M*D]; int32 pdf_offsets[num_pdfs+1] utt_row_offsets[n_utts+1]
//        spk_utt_offsets[n_spk+1]; int64 frame_entry_offsets[T+1]; int32 entry_pdf[E]; float entry_weight[E]
// output: int64 n_post; float post[n_post] like[E]; int32 R; int32 run_row[R] spk_run_offsets[n_spk+1]; float a[R*D] b[R*D];
//        double count[R] beta[n_spk] K[n_spk*D*(D+1)] G[n_spk*D*P]; float W[n_spk*D*(D+1)] impr[n_spk] count[n_spk]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../old-kaldi-git_amd/csrc/kh_fmllr_update.h"

namespace {

template <typename T> std::vector<T> Read(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "fmllr_cpu_baseline: short input\n");
    exit(2);
  }
  return v;
}
template <typename T> void Write(FILE *f, const std::vector<T> &v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    fprintf(stderr, "fmllr_cpu_baseline: short write\n");
    exit(2);
  }
}
double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: fmllr_cpu_baseline <input> <output>\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const std::vector<int32_t> h = Read<int32_t>(f, 9);
  const int T = h[0], D = h[1], num_pdfs = h[2], M = h[3], n_utts = h[4], n_spk = h[5], E = h[6], type = h[7], num_iters = h[8];
  const float min_count = Read<float>(f, 1)[0];
  if (T < 0 || D <= 0 || num_pdfs <= 0 || M <= 0 || n_utts < 0 || n_spk < 0 || E < 0 || type < 0 || type > 3) {
    fprintf(stderr, "fmllr_cpu_baseline: bad header\n");
    return 2;
  }
  const std::vector<float> feats = Read<float>(f, static_cast<size_t>(T) * D), gconsts = Read<float>(f, M),
                           mi = Read<float>(f, static_cast<size_t>(M) * D), iv = Read<float>(f, static_cast<size_t>(M) * D);
  const std::vector<int32_t> pdf_off = Read<int32_t>(f, num_pdfs + 1), utt_off = Read<int32_t>(f, n_utts + 1),
                             spk_off = Read<int32_t>(f, n_spk + 1);
  const std::vector<int64_t> feo = Read<int64_t>(f, T + 1);
  const std::vector<int32_t> entry_pdf = Read<int32_t>(f, E);
  const std::vector<float> entry_w = Read<float>(f, E);
  fclose(f);
  // every index before it is used
  bool ok = pdf_off[0] == 0 && pdf_off[num_pdfs] == M && feo[0] == 0 && feo[T] == E && utt_off[0] == 0 && utt_off[n_utts] == T &&
            spk_off[0] == 0 && spk_off[n_spk] == n_utts;
  for (int j = 0; ok && j < num_pdfs; j++) ok = pdf_off[j + 1] > pdf_off[j];
  for (int t = 0; ok && t < T; t++) ok = feo[t + 1] >= feo[t];
  for (int u = 0; ok && u < n_utts; u++) ok = utt_off[u + 1] >= utt_off[u];
  for (int s = 0; ok && s < n_spk; s++) ok = spk_off[s + 1] >= spk_off[s];
  for (int e = 0; ok && e < E; e++) ok = entry_pdf[e] >= 0 && entry_pdf[e] < num_pdfs;
  if (!ok) {
    fprintf(stderr, "fmllr_cpu_baseline: inconsistent offsets\n");
    return 2;
  }
  const int D1 = D + 1, P = D1 * (D + 2) / 2;

  // ---- A1: ComponentPosteriors and Scale(weight) per entry
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
  // ---- A2: AccumulateFromPosteriors with the single-frame statistics
  const double t1 = Now();
  std::vector<int32_t> run_row, spk_run(n_spk + 1, 0);
  std::vector<float> a, b;
  std::vector<double> count;
  for (int s = 0; s < n_spk; s++) {
    spk_run[s] = static_cast<int32_t>(run_row.size());
    int cur = -1;
    for (int t = utt_off[spk_off[s]]; t < utt_off[spk_off[s + 1]]; t++) {
      for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
        bool changed = cur < 0;   // DataHasChanged, once per entry as the reference calls it
        for (int d = 0; !changed && d < D; d++) changed = feats[static_cast<size_t>(t) * D + d] != feats[static_cast<size_t>(cur) * D + d];
        if (changed) {
          run_row.push_back(t);
          a.resize(a.size() + D, 0.f);
          b.resize(b.size() + D, 0.f);
          count.push_back(0.0);
          cur = t;
        }
        const int m0 = pdf_off[entry_pdf[e]], n = pdf_off[entry_pdf[e] + 1] - m0;
        const float *p = &post[goff[e]];
        float *ar = &a[a.size() - D], *br = &b[b.size() - D];
        double psum = 0.0;
        for (int g = 0; g < n; g++) {
          psum += p[g];
          for (int d = 0; d < D; d++) {
            ar[d] = fmaf(p[g], mi[static_cast<size_t>(m0 + g) * D + d], ar[d]);
            br[d] = fmaf(p[g], iv[static_cast<size_t>(m0 + g) * D + d], br[d]);
          }
        }
        count.back() += static_cast<double>(static_cast<float>(psum));
      }
    }
  }
  spk_run[n_spk] = static_cast<int32_t>(run_row.size());
  const int R = static_cast<int>(run_row.size());
  // ---- B: CommitSingleFrameStats per merged frame
  const double t2 = Now();
  std::vector<double> beta(n_spk, 0.0), K(static_cast<size_t>(n_spk) * D * D1, 0.0), G(static_cast<size_t>(n_spk) * D * P, 0.0);
  std::vector<double> xp(D1), scatter(P);
  for (int s = 0; s < n_spk; s++) {
    double *Ks = &K[static_cast<size_t>(s) * D * D1], *Gs = &G[static_cast<size_t>(s) * D * P];
    for (int r = spk_run[s]; r < spk_run[s + 1]; r++) {
      if (count[r] == 0.0) continue;
      for (int d = 0; d < D; d++) xp[d] = feats[static_cast<size_t>(run_row[r]) * D + d];
      xp[D] = 1.0;
      beta[s] += count[r];
      for (int i = 0; i < D; i++) {
        const double ai = a[static_cast<size_t>(r) * D + i];
        for (int j = 0; j < D1; j++) Ks[i * D1 + j] += ai * xp[j];
      }
      for (int rr = 0, k = 0; rr < D1; rr++)
        for (int c = 0; c <= rr; c++) scatter[k++] = xp[rr] * xp[c];
      for (int i = 0; i < D; i++) {
        const double bi = b[static_cast<size_t>(r) * D + i];
        double *Gi = Gs + static_cast<size_t>(i) * P;
        for (int k = 0; k < P; k++) Gi[k] += bi * scatter[k];
      }
    }
  }
  // ---- C
  const double t3 = Now();
  static const char *kTypes[4] = {"full", "diag", "offset", "none"};
  std::vector<float> W(static_cast<size_t>(n_spk) * D * D1), impr(n_spk), cnt(n_spk);
  for (int s = 0; s < n_spk; s++) {
    kh_fmllr::SpkStats st{D, beta[s], &K[static_cast<size_t>(s) * D * D1], &G[static_cast<size_t>(s) * D * P]};
    std::string err;
    if (kh_fmllr::UpdateSpeaker(st, kTypes[type], min_count, num_iters, &W[static_cast<size_t>(s) * D * D1], &impr[s], &cnt[s], &err) !=
        kh_fmllr::kOk) {
      fprintf(stderr, "fmllr_cpu_baseline: speaker %d: %s\n", s, err.c_str());
      return 3;
    }
  }
  const double t4 = Now();
  FILE *o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  Write(o, std::vector<int64_t>{goff[E]});
  Write(o, post);
  Write(o, like);
  Write(o, std::vector<int32_t>{R});
  Write(o, run_row);
  Write(o, spk_run);
  Write(o, a);
  Write(o, b);
  Write(o, count);
  Write(o, beta);
  Write(o, K);
  Write(o, G);
  Write(o, W);
  Write(o, impr);
  Write(o, cnt);
  if (fclose(o) != 0) { perror(argv[2]); return 1; }
  printf("ms %.3f %.3f %.3f %.3f\n", t1 - t0, t2 - t1, t3 - t2, t4 - t3);
  return 0;
}
