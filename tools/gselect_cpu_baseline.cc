// gselect_cpu_baseline.cc - a plain one-thread C++ statement of what csrc/kh_gselect.hip and the accumulation behind it
// compute, for tools/gselect_rate.py (the CPU time next to the device's, on the same frames) and tests/test_gselect_baseline.py
// (bit for bit against tests/gselect_restatement.py in library mode).  Not the reference's text: the order is stated directly.
//
//   scores      per Gaussian two fmaf chains over d in order, ll = (g + a1) + (-0.5f * a2)
//   selection   the n largest under (score descending, index descending), scores compared as floats; with a preselection over
//               the listed Gaussians, position p carrying list[p] as its index, n = min(n, list size)
//   frame_like  tot = LogAdd(tot, score) over the selected, best first, from -inf; float LogAdd, exp / log1p as the float of
//               the double function
//   posteriors  over each frame's SELECTED list in list order: float max, e = fl32(exp((double)(f - max))), the float sum in
//               order, (e * fl32(1.0 / sum)) * 1.0f, like = max + fl32(log((double)sum))
//   statistics  frame by frame, Gaussian by Gaussian in list order, in double: occ += p, mean += p x, var += p (x x)
//
// usage: gselect_cpu_baseline in.bin out.bin [repeats]
//   in.bin   int32 T, D, G, n, has_pre; float feats [T x D], gconsts [G], means_invvars [G x D], inv_vars [G x D];
//            with has_pre: int64 offsets [T + 1], int32 items [offsets[T]]
//   out.bin  int32 sel [T x n_out] (padded with -1), count [T]; float frame_like [T]; float post (the selected lists' posteriors,
//            concatenated), post_like [T]; double occ [G], mean [G x D], var [G x D]
// stdout: one JSON line with the milliseconds of the three stages (the best of `repeats` passes).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <utility>
#include <vector>

static const float kMinLogDiffFloat = std::log(std::numeric_limits<float>::epsilon());

static float LogAdd(float x, float y) {
  float diff;
  if (x < y) {
    diff = x - y;
    x = y;
  } else {
    diff = y - x;
  }
  if (diff >= kMinLogDiffFloat) {
    const float e = static_cast<float>(std::exp(static_cast<double>(diff)));
    return x + static_cast<float>(std::log1p(static_cast<double>(e)));
  }
  return x;
}

static float Score(const float *x, int D, const float *g, const float *mi, const float *iv, int idx) {
  const float *mir = mi + static_cast<size_t>(idx) * D, *ivr = iv + static_cast<size_t>(idx) * D;
  float a1 = 0.f, a2 = 0.f;
  for (int d = 0; d < D; d++) {
    const float v = x[d];
    a1 = std::fmaf(v, mir[d], a1);
    a2 = std::fmaf(v * v, ivr[d], a2);
  }
  return (g[idx] + a1) + (-0.5f * a2);
}

template <typename T>
static void ReadAll(std::FILE *f, std::vector<T> *v, size_t n) {
  v->resize(n);
  if (n && std::fread(v->data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "gselect_cpu_baseline: short input\n");
    std::exit(2);
  }
}
template <typename T>
static void WriteAll(std::FILE *f, const std::vector<T> &v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    std::fprintf(stderr, "gselect_cpu_baseline: short output\n");
    std::exit(2);
  }
}

static double Ms(std::chrono::steady_clock::time_point a) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: gselect_cpu_baseline in.bin out.bin [repeats]\n");
    return 1;
  }
  const int repeats = argc > 3 ? std::max(1, std::atoi(argv[3])) : 1;
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  std::vector<int32_t> head;
  ReadAll(in, &head, 5);
  const int T = head[0], D = head[1], G = head[2], n = head[3], has_pre = head[4];
  if (T < 0 || D < 1 || G < 1 || n < 1) { std::fprintf(stderr, "gselect_cpu_baseline: bad header\n"); return 2; }
  std::vector<float> feats, g, mi, iv;
  ReadAll(in, &feats, static_cast<size_t>(T) * D);
  ReadAll(in, &g, G);
  ReadAll(in, &mi, static_cast<size_t>(G) * D);
  ReadAll(in, &iv, static_cast<size_t>(G) * D);
  std::vector<int64_t> off;
  std::vector<int32_t> items;
  if (has_pre) {
    ReadAll(in, &off, static_cast<size_t>(T) + 1);
    ReadAll(in, &items, static_cast<size_t>(off[T]));
    for (int t = 0; t < T; t++)
      if (off[t + 1] <= off[t] || off[t + 1] - off[t] > G) { std::fprintf(stderr, "gselect_cpu_baseline: bad list at frame %d\n", t); return 2; }
    for (int32_t i : items)
      if (i < 0 || i >= G) { std::fprintf(stderr, "gselect_cpu_baseline: bad index %d\n", i); return 2; }
  }
  std::fclose(in);
  const int n_out = std::min(n, G);
  std::vector<int32_t> sel(static_cast<size_t>(T) * n_out, -1), count(T, 0);
  std::vector<float> like(T, 0.f), post, post_like(T, 0.f);
  std::vector<double> occ(G), mean(static_cast<size_t>(G) * D), var(static_cast<size_t>(G) * D);
  double best[3] = {1e300, 1e300, 1e300};
  for (int rep = 0; rep < repeats; rep++) {
    // selection
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<float, int32_t>> pairs;
    for (int t = 0; t < T; t++) {
      const float *x = feats.data() + static_cast<size_t>(t) * D;
      const int len = has_pre ? static_cast<int>(off[t + 1] - off[t]) : G;
      pairs.resize(len);
      for (int p = 0; p < len; p++) {
        const int idx = has_pre ? items[off[t] + p] : p;
        pairs[p] = std::make_pair(Score(x, D, g.data(), mi.data(), iv.data(), idx), idx);
      }
      const int c = std::min(n, len);
      std::partial_sort(pairs.begin(), pairs.begin() + c, pairs.end(), std::greater<std::pair<float, int32_t>>());
      float tot = -std::numeric_limits<float>::infinity();
      for (int j = 0; j < c; j++) {
        sel[static_cast<size_t>(t) * n_out + j] = pairs[j].second;
        tot = LogAdd(tot, pairs[j].first);
      }
      for (int j = c; j < n_out; j++) sel[static_cast<size_t>(t) * n_out + j] = -1;
      count[t] = c;
      like[t] = tot;
    }
    best[0] = std::min(best[0], Ms(t0));
    // posteriors over the selected lists
    t0 = std::chrono::steady_clock::now();
    post.clear();
    std::vector<float> f;
    for (int t = 0; t < T; t++) {
      const float *x = feats.data() + static_cast<size_t>(t) * D;
      const int c = count[t];
      f.resize(c);
      float mx = -std::numeric_limits<float>::infinity();
      for (int j = 0; j < c; j++) {
        f[j] = Score(x, D, g.data(), mi.data(), iv.data(), sel[static_cast<size_t>(t) * n_out + j]);
        mx = std::max(mx, f[j]);
      }
      float sum = 0.f;
      for (int j = 0; j < c; j++) {
        f[j] = static_cast<float>(std::exp(static_cast<double>(f[j] - mx)));
        sum += f[j];
      }
      const float inv = static_cast<float>(1.0 / static_cast<double>(sum));
      for (int j = 0; j < c; j++) post.push_back((f[j] * inv) * 1.0f);
      post_like[t] = mx + static_cast<float>(std::log(static_cast<double>(sum)));
    }
    best[1] = std::min(best[1], Ms(t0));
    // statistics
    t0 = std::chrono::steady_clock::now();
    std::fill(occ.begin(), occ.end(), 0.0);
    std::fill(mean.begin(), mean.end(), 0.0);
    std::fill(var.begin(), var.end(), 0.0);
    size_t at = 0;
    for (int t = 0; t < T; t++) {
      const float *x = feats.data() + static_cast<size_t>(t) * D;
      for (int j = 0; j < count[t]; j++, at++) {
        const int gi = sel[static_cast<size_t>(t) * n_out + j];
        const double p = static_cast<double>(post[at]);
        occ[gi] += p;
        double *m = mean.data() + static_cast<size_t>(gi) * D, *v = var.data() + static_cast<size_t>(gi) * D;
        for (int d = 0; d < D; d++) {
          const double xd = static_cast<double>(x[d]);
          m[d] += p * xd;
          v[d] += p * (xd * xd);
        }
      }
    }
    best[2] = std::min(best[2], Ms(t0));
  }
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  WriteAll(out, sel);
  WriteAll(out, count);
  WriteAll(out, like);
  WriteAll(out, post);
  WriteAll(out, post_like);
  WriteAll(out, occ);
  WriteAll(out, mean);
  WriteAll(out, var);
  std::fclose(out);
  std::printf("{\"frames\": %d, \"dim\": %d, \"gauss\": %d, \"n\": %d, \"repeats\": %d, \"select_ms\": %.3f, \"posteriors_ms\": %.3f, "
              "\"accumulate_ms\": %.3f}\n", T, D, G, n, repeats, best[0], best[1], best[2]);
  return 0;
}
