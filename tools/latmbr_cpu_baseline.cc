// latmbr_cpu_baseline.cc - minimum Bayes risk decoding of lattices (the computation of lat/sausages.cc's MinimumBayesRisk)
// on ONE host thread: the baseline tools/lattice_mbr_rate.py times next to kh_compact_lattice_mbr, and a second
// implementation tests/test_latmbr_cpu_baseline.py compares with the Python restatement bit for bit.  Written without a
// look at the kernel: sequential loops over q, a std::map per bin, nothing shared with csrc/kh_latmbr.hip.
//
//   latmbr_cpu_baseline IN OUT     (g++ -O2 -std=c++14 -ffp-contract=off)
//
// IN, little-endian, flat: int64 { n_lats, n_points, do_mbr, n_states S, n_arcs A, n_hyp_words H }, then
//   int32 state_offsets[n_lats + 1], int64 arc_offsets[S + 1], int32 label[A], int32 nextstate[A], float graph[A],
//   float acoustic[A], int32 state_times[S], double scales[4 n_points], float penalties[n_points],
//   int64 hyp_offsets[n_lats n_points + 1], int32 hyp_words[H]
// (lattices as api.compact_lattice_mbr_prepare leaves them: top-sorted, the last state the only final one, weight One).
// OUT: per (lattice, point) in order: int32 { n_words, n_bins, n_stats, iterations }, double L, int32 words[n_words],
//   float one_best_times[2 n_words], float one_best_confidences[n_words], int32 bin_sizes[n_bins], float bin_times[2 n_bins],
//   int32 stat_words[n_stats], float stat_post[n_stats].
// Exit status 2: arguments or input refused (a message on stderr).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

struct Reader {
  std::vector<char> buf;
  size_t at = 0;
  bool ok = true;
  template <typename T>
  std::vector<T> Take(int64_t n) {
    std::vector<T> v;
    if (n < 0 || at + sizeof(T) * static_cast<size_t>(n) > buf.size()) {
      ok = false;
      return v;
    }
    v.resize(n);
    if (n) std::memcpy(v.data(), buf.data() + at, sizeof(T) * n);
    at += sizeof(T) * n;
    return v;
  }
};

template <typename T>
void Put(std::vector<char> *out, const T *p, size_t n) {
  const char *c = reinterpret_cast<const char *>(p);
  out->insert(out->end(), c, c + sizeof(T) * n);
}

struct InArc {     // an arc as its destination sees it
  int32_t src, word;
  float loglike;
  double post;     // exp(alpha(src) + loglike - alpha(dst))
};

double LogAdd(double x, double y) {
  static const double min_log_diff = std::log(DBL_EPSILON);
  double diff;
  if (x < y) {
    diff = x - y;
    x = y;
  } else {
    diff = y - x;
  }
  if (diff >= min_log_diff) return x + std::log1p(std::exp(diff));
  return x;
}

inline double Loss(int32_t a, int32_t b) { return a == b ? 0.0 : 1.0; }

struct Decoder {
  int32_t N = 0;                                   // states, 0-based here
  std::vector<std::vector<InArc>> in;              // per destination, in (source state, arc position) order
  std::vector<int32_t> times;
  std::vector<int32_t> R;                          // hypothesis with epsilons between the words
  double L = 0.0;
  int32_t iterations = 0;
  std::vector<std::vector<std::pair<int32_t, float>>> bins;
  std::vector<std::pair<float, float>> bin_times, best_times;
  std::vector<float> best_conf;

  // one arc's row: value[q] and choice[q] (1 match/substitute, 2 insert the arc's word, 3 skip r_q)
  void ArcRow(const std::vector<double> &from, int32_t word, std::vector<double> *value, std::vector<char> *choice) const {
    const double delta = static_cast<double>(1.0e-05f);
    const int Q = static_cast<int>(R.size());
    (*value)[0] = from[0] + Loss(word, 0) + delta;
    for (int q = 1; q <= Q; q++) {
      const int32_t r_q = R[q - 1];
      const double diag = from[q - 1] + Loss(word, r_q), ins = from[q] + Loss(word, 0) + delta, del = (*value)[q - 1] + Loss(0, r_q);
      if (diag <= ins) {
        if (diag <= del) { (*choice)[q] = 1; (*value)[q] = diag; } else { (*choice)[q] = 3; (*value)[q] = del; }
      } else {
        if (ins <= del) { (*choice)[q] = 2; (*value)[q] = ins; } else { (*choice)[q] = 3; (*value)[q] = del; }
      }
    }
  }

  void Accumulate() {
    const int Q = static_cast<int>(R.size());
    std::vector<std::vector<double>> fwd(N, std::vector<double>(Q + 1, 0.0)), bwd(N, std::vector<double>(Q + 1, 0.0));
    std::vector<double> value(Q + 1, 0.0), mass(Q + 1, 0.0), t_begin(Q + 1, 0.0), t_end(Q + 1, 0.0);
    std::vector<char> choice(Q + 1, 0);
    std::vector<std::map<int32_t, double>> gamma(Q + 1);
    auto add = [](std::map<int32_t, double> *m, int32_t w, double d) {
      if (d == 0) return;
      auto r = m->insert(std::make_pair(w, d));
      if (!r.second) r.first->second += d;
    };
    for (int q = 1; q <= Q; q++) fwd[0][q] = fwd[0][q - 1] + Loss(0, R[q - 1]);
    for (int32_t n = 1; n < N; n++) {
      for (const InArc &arc : in[n]) {
        ArcRow(fwd[arc.src], arc.word, &value, &choice);
        for (int q = 0; q <= Q; q++) fwd[n][q] += arc.post * value[q];
      }
    }
    L = fwd[N - 1][Q];
    bwd[N - 1][Q] = 1.0;
    for (int32_t n = N - 1; n >= 1; n--) {
      for (const InArc &arc : in[n]) {
        ArcRow(fwd[arc.src], arc.word, &value, &choice);
        std::fill(mass.begin(), mass.end(), 0.0);
        for (int q = Q; q >= 1; q--) {
          mass[q] += arc.post * bwd[n][q];
          if (choice[q] == 1) {
            bwd[arc.src][q - 1] += mass[q];
            add(&gamma[q], arc.word, mass[q]);
            t_begin[q] += times[arc.src] * mass[q];
            t_end[q] += times[n] * mass[q];
          } else if (choice[q] == 2) {
            bwd[arc.src][q] += mass[q];
          } else {
            mass[q - 1] += mass[q];
            add(&gamma[q], 0, mass[q]);
            t_begin[q] += times[n] * mass[q];
            t_end[q] += times[n] * mass[q];
          }
        }
        mass[0] += arc.post * bwd[n][0];
        bwd[arc.src][0] += mass[0];
      }
    }
    std::fill(mass.begin(), mass.end(), 0.0);
    for (int q = Q; q >= 1; q--) {
      mass[q] += bwd[0][q];
      mass[q - 1] += mass[q];
      add(&gamma[q], 0, mass[q]);
      t_begin[q] += times[0] * mass[q];
      t_end[q] += times[0] * mass[q];
    }
    bins.assign(Q, std::vector<std::pair<int32_t, float>>());
    bin_times.assign(Q, std::make_pair(0.f, 0.f));
    for (int q = 1; q <= Q; q++) {
      for (const auto &e : gamma[q]) bins[q - 1].push_back(std::make_pair(e.first, static_cast<float>(e.second)));
      std::sort(bins[q - 1].begin(), bins[q - 1].end(), [](const std::pair<int32_t, float> &a, const std::pair<int32_t, float> &b) {
        if (a.second > b.second) return true;
        if (a.second < b.second) return false;
        return a.first > b.first;
      });
      bin_times[q - 1].first = static_cast<float>(t_begin[q]);
      bin_times[q - 1].second = static_cast<float>(t_end[q]);
      if (q > 1 && bin_times[q - 2].second > bin_times[q - 1].first) {
        const double avg = 0.5 * (bin_times[q - 2].second + bin_times[q - 1].first);
        bin_times[q - 2].second = bin_times[q - 1].first = static_cast<float>(avg);
      }
    }
  }

  bool Decode(bool do_mbr, std::string *why) {
    for (size_t counter = 0;; counter++) {
      std::vector<int32_t> spaced(1, 0);
      for (int32_t w : R) {
        if (w != 0) {
          spaced.push_back(w);
          spaced.push_back(0);
        }
      }
      R.swap(spaced);
      Accumulate();
      iterations++;
      double change = 0.0;
      best_times.clear();
      best_conf.clear();
      for (size_t q = 0; q < R.size(); q++) {
        if (do_mbr) {
          if (bins[q].empty()) {
            *why = "a bin without statistics";
            return false;
          }
          double old_gamma = 0, new_gamma = bins[q][0].second;
          const int32_t rq = R[q], rhat = bins[q][0].first;
          for (const auto &e : bins[q])
            if (e.first == rq) old_gamma = e.second;
          change += (old_gamma - new_gamma);
          R[q] = rhat;
        }
        if (R[q] != 0) {
          best_times.push_back(bin_times[q]);
          float confidence = 0.0;
          for (const auto &e : bins[q])
            if (e.first == R[q]) confidence = e.second;
          best_conf.push_back(confidence);
        }
      }
      if (change == 0) break;
      if (counter > 100) break;
    }
    R.erase(std::remove(R.begin(), R.end(), 0), R.end());
    return true;
  }
};

int Fail(const std::string &msg) {
  std::fprintf(stderr, "latmbr_cpu_baseline: %s\n", msg.c_str());
  return 2;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return Fail("usage: latmbr_cpu_baseline IN OUT");
  Reader in;
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return Fail(std::string("cannot open ") + argv[1]);
    char chunk[1 << 16];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) in.buf.insert(in.buf.end(), chunk, chunk + n);
    std::fclose(f);
  }
  const std::vector<int64_t> head = in.Take<int64_t>(6);
  if (!in.ok) return Fail("short header");
  const int64_t n_lats = head[0], P = head[1], S = head[3], A = head[4], H = head[5];
  const bool do_mbr = head[2] != 0;
  if (n_lats < 1 || P < 1 || S < n_lats || A < 0 || H < 0 || n_lats > (1 << 24) || P > (1 << 16)) return Fail("header out of range");
  const std::vector<int32_t> soff = in.Take<int32_t>(n_lats + 1);
  const std::vector<int64_t> aoff = in.Take<int64_t>(S + 1);
  const std::vector<int32_t> label = in.Take<int32_t>(A), next = in.Take<int32_t>(A);
  const std::vector<float> graph = in.Take<float>(A), acoustic = in.Take<float>(A);
  const std::vector<int32_t> times = in.Take<int32_t>(S);
  const std::vector<double> scales = in.Take<double>(4 * P);
  const std::vector<float> pens = in.Take<float>(P);
  const std::vector<int64_t> hoff = in.Take<int64_t>(n_lats * P + 1);
  const std::vector<int32_t> hw = in.Take<int32_t>(H);
  if (!in.ok || in.at != in.buf.size()) return Fail("input size does not match its header");
  if (soff[0] != 0 || soff[n_lats] != S || aoff[0] != 0 || aoff[S] != A || hoff[0] != 0 || hoff[n_lats * P] != H)
    return Fail("offsets do not match the header");
  for (int64_t s = 0; s < S; s++)
    if (aoff[s + 1] < aoff[s]) return Fail("arc_offsets descend");
  for (int64_t o = 0; o < n_lats * P; o++)
    if (hoff[o + 1] < hoff[o]) return Fail("hyp_offsets descend");
  const float finf = std::numeric_limits<float>::infinity();
  std::vector<char> out;
  for (int64_t l = 0; l < n_lats; l++) {
    const int32_t s0 = soff[l], ns = soff[l + 1] - s0;
    if (ns < 1) return Fail("a lattice without states");
    for (int32_t s = 0; s < ns; s++)
      for (int64_t j = aoff[s0 + s]; j < aoff[s0 + s + 1]; j++)
        if (next[j] <= s || next[j] >= ns) return Fail("lattice " + std::to_string(l) + ": arc " + std::to_string(j - aoff[s0]) + " is not forward");
    if (aoff[s0 + ns] != aoff[s0 + ns - 1]) return Fail("lattice " + std::to_string(l) + ": the last state has arcs");
    for (int64_t p = 0; p < P; p++) {
      Decoder d;
      d.N = ns;
      d.in.assign(ns, std::vector<InArc>());
      d.times.assign(times.begin() + s0, times.begin() + s0 + ns);
      for (int32_t s = 0; s < ns; s++) {
        for (int64_t j = aoff[s0 + s]; j < aoff[s0 + s + 1]; j++) {
          float g2, a2;
          if (graph[j] == finf) {
            g2 = a2 = finf;
          } else {
            g2 = static_cast<float>(scales[4 * p] * static_cast<double>(graph[j]) + scales[4 * p + 1] * static_cast<double>(acoustic[j]));
            a2 = static_cast<float>(scales[4 * p + 2] * static_cast<double>(graph[j]) + scales[4 * p + 3] * static_cast<double>(acoustic[j]));
          }
          if (label[j] != 0) g2 = g2 + pens[p];
          const float loglike = -(g2 + a2);
          if (std::isnan(loglike) || loglike == finf) return Fail("lattice " + std::to_string(l) + ": arc weight NaN or -inf");
          d.in[next[j]].push_back(InArc{s, label[j], loglike, 0.0});
        }
      }
      std::vector<double> alpha(ns, 0.0);
      for (int32_t n = 1; n < ns; n++) {
        double a = -std::numeric_limits<double>::infinity();
        for (const InArc &arc : d.in[n]) a = LogAdd(a, alpha[arc.src] + arc.loglike);
        if (a == -std::numeric_limits<double>::infinity()) return Fail("lattice " + std::to_string(l) + ": state " + std::to_string(n) + ": alpha = -inf");
        alpha[n] = a;
        for (InArc &arc : d.in[n]) arc.post = std::exp(alpha[arc.src] + arc.loglike - a);
      }
      const int64_t o = l * P + p;
      d.R.assign(hw.begin() + hoff[o], hw.begin() + hoff[o + 1]);
      std::string why;
      if (!d.Decode(do_mbr, &why)) return Fail("lattice " + std::to_string(l) + ": " + why);
      std::vector<int32_t> sizes, sw;
      std::vector<float> sp, bt, obt;
      for (const auto &b : d.bins) {
        sizes.push_back(static_cast<int32_t>(b.size()));
        for (const auto &e : b) {
          sw.push_back(e.first);
          sp.push_back(e.second);
        }
      }
      for (const auto &t : d.bin_times) {
        bt.push_back(t.first);
        bt.push_back(t.second);
      }
      for (const auto &t : d.best_times) {
        obt.push_back(t.first);
        obt.push_back(t.second);
      }
      const int32_t counts[4] = {static_cast<int32_t>(d.R.size()), static_cast<int32_t>(sizes.size()), static_cast<int32_t>(sw.size()), d.iterations};
      Put(&out, counts, 4);
      Put(&out, &d.L, 1);
      Put(&out, d.R.data(), d.R.size());
      Put(&out, obt.data(), obt.size());
      Put(&out, d.best_conf.data(), d.best_conf.size());
      Put(&out, sizes.data(), sizes.size());
      Put(&out, bt.data(), bt.size());
      Put(&out, sw.data(), sw.size());
      Put(&out, sp.data(), sp.size());
    }
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return Fail(std::string("cannot write ") + argv[2]);
  const bool wrote = out.empty() || std::fwrite(out.data(), 1, out.size(), f) == out.size();
  if (std::fclose(f) != 0 || !wrote) return Fail("write failed");
  return 0;
}
