// align_cpu_baseline.cc — forced alignment on one host thread by the rule of kh_align_compiled (include/kaldi_hip.h): the
// baseline tools/align_rate.py times the device call against, and an independent second implementation of the rule (it shares
// no code with csrc/kh_align.hip: arcs are walked forward in their CSR order, the cutoff is found with nth_element).
//   g++ -O2 -std=c++14 tools/align_cpu_baseline.cc -o align_cpu_baseline;   align_cpu_baseline DUMP [REPEAT]
// DUMP: the plain dump of tests/align_cases.py (write_dump); floats travel as the decimal value of their bits.  Prints per
// utterance "status cost_bits best_state path_len" and the path's arcs "ilabel olabel graph_bits acoustic_bits"; with REPEAT
// the search runs that many times and the milliseconds per pass go to standard error.
//
// FasterDecoder (decoder/faster-decoder.cc) with max_active = INT_MAX: GetCutoff :151-213 on float-rounded costs,
// ProcessEmitting :224-303 accepted against the frame's FINAL next_weight_cutoff, ProcessNonemitting :306-346 in rounds that
// each read the round before, equal costs to the lowest arc position, equal final totals to the lowest state; the path from
// per-(frame, state) backpointers, its floats as GetBestPath :117-126 forms them.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

const double kInf = std::numeric_limits<double>::infinity();
enum { kDone = 0, kNoFinal = 1, kNeedsRoom = 2, kBound = 4 };

struct Arc { int src, dst, il, ol; float w; };
struct Utt {
  int S = 0, start = 0, T = 0, row0 = 0, room = 0, n_eps = 0;
  std::vector<Arc> arcs;
  std::vector<float> fin;
};
struct Result {
  int status = kDone, best = -1, len = 0;
  double cost = kInf;
  std::vector<int> path;
  std::vector<float> ac;
};

long long ReadInt(FILE *f) {
  long long v;
  if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short dump\n"); exit(2); }
  return v;
}
float Bits(long long b) { const uint32_t u = static_cast<uint32_t>(b); float x; memcpy(&x, &u, 4); return x; }

bool Closure(const Utt &U, std::vector<double> *cur, double cutoff, int *bprow) {
  if (U.n_eps == 0) return true;
  std::vector<double> nxt;
  std::vector<int> got(U.S);
  for (int round = 0; round <= U.S; round++) {
    nxt = *cur;
    std::fill(got.begin(), got.end(), -1);
    for (size_t a = 0; a < U.arcs.size(); a++) {
      const Arc &A = U.arcs[a];
      if (A.il != 0) continue;
      const double cs = (*cur)[A.src];
      if (!(cs < kInf) || cs > cutoff) continue;
      const double nc = cs + static_cast<double>(A.w);
      if (nc > cutoff) continue;
      if (nc < nxt[A.dst]) { nxt[A.dst] = nc; got[A.dst] = static_cast<int>(a); }
    }
    bool changed = false;
    for (int d = 0; d < U.S; d++)
      if (got[d] >= 0) { bprow[d] = got[d]; changed = true; }
    cur->swap(nxt);
    if (!changed) return true;
  }
  return false;
}

Result Align(const Utt &U, const float *ll, int cols, const std::vector<int> &tid2pdf, float beam, int min_active, float beam_delta) {
  Result R;
  std::vector<double> cur(U.S, kInf), nxt(U.S);
  std::vector<int> bp(static_cast<size_t>(U.T + 1) * U.S, -1);
  std::vector<float> tmp;
  cur[U.start] = 0.0;
  bool ok = Closure(U, &cur, static_cast<double>(std::numeric_limits<float>::max()), bp.data());
  for (int f = 0; f < U.T && ok; f++) {
    double best = kInf;
    tmp.clear();
    for (int s = 0; s < U.S; s++)
      if (cur[s] < kInf) { tmp.push_back(static_cast<float>(cur[s])); best = std::min(best, cur[s]); }
    const double beam_cutoff = best + static_cast<double>(beam);
    double weight_cutoff = beam_cutoff;
    float adaptive_beam = beam;
    if (min_active > 0) {
      double min_active_cutoff = kInf;
      if (tmp.size() > static_cast<size_t>(min_active)) {
        std::nth_element(tmp.begin(), tmp.begin() + min_active, tmp.end());
        min_active_cutoff = tmp[min_active];
      }
      if (min_active_cutoff > beam_cutoff) {
        adaptive_beam = static_cast<float>(min_active_cutoff - best + static_cast<double>(beam_delta));
        weight_cutoff = min_active_cutoff;
      }
    }
    const float *row = ll + static_cast<size_t>(U.row0 + f) * cols;
    int *bprow = bp.data() + static_cast<size_t>(f + 1) * U.S;
    std::fill(nxt.begin(), nxt.end(), kInf);
    for (size_t a = 0; a < U.arcs.size(); a++) {
      const Arc &A = U.arcs[a];
      if (A.il == 0 || !(cur[A.src] < weight_cutoff)) continue;
      const float ac = -row[tid2pdf[A.il]];
      const double nw = (cur[A.src] + static_cast<double>(A.w)) + static_cast<double>(ac);
      if (nw < nxt[A.dst]) { nxt[A.dst] = nw; bprow[A.dst] = static_cast<int>(a); }
    }
    double gmin = kInf;
    for (int s = 0; s < U.S; s++) gmin = std::min(gmin, nxt[s]);
    const double next_cutoff = gmin + static_cast<double>(adaptive_beam);
    for (int s = 0; s < U.S; s++)
      if (!(nxt[s] < next_cutoff)) { nxt[s] = kInf; bprow[s] = -1; }
    cur.swap(nxt);
    ok = Closure(U, &cur, next_cutoff, bprow);
  }
  if (!ok) { R.status = kBound; return R; }
  for (int s = 0; s < U.S; s++) {
    if (cur[s] < kInf && U.fin[s] != std::numeric_limits<float>::infinity()) {
      const double tc = cur[s] + static_cast<double>(U.fin[s]);
      if (tc < R.cost) { R.cost = tc; R.best = s; }
    }
  }
  if (R.best < 0) { R.status = kNoFinal; return R; }
  int state = R.best, frame = U.T;
  const long long max_steps = static_cast<long long>(U.T + 1) * U.S;
  bool at_start = false;
  for (long long step = 0; step <= max_steps; step++) {
    const int a = bp[static_cast<size_t>(frame) * U.S + state];
    if (a < 0) { at_start = frame == 0 && state == U.start; break; }
    R.path.push_back(a);
    if (U.arcs[a].il != 0 && --frame < 0) break;
    state = U.arcs[a].src;
  }
  if (!at_start) { R.status = kBound; R.path.clear(); return R; }
  std::reverse(R.path.begin(), R.path.end());
  R.len = static_cast<int>(R.path.size());
  if (R.len > U.room) { R.status = kNeedsRoom; return R; }
  double c = 0.0;
  int fr = 0;
  for (int a : R.path) {
    const Arc &A = U.arcs[a];
    double nc = c + static_cast<double>(A.w);
    if (A.il != 0) {
      const float ac = -ll[static_cast<size_t>(U.row0 + fr) * cols + tid2pdf[A.il]];
      nc += static_cast<double>(ac);
      fr++;
    }
    const float tot = static_cast<float>(nc - c);
    R.ac.push_back(tot - A.w);
    c = nc;
  }
  return R;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2 || argc > 3) { fprintf(stderr, "usage: align_cpu_baseline DUMP [REPEAT]\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int repeat = argc == 3 ? atoi(argv[2]) : 0;
  const int n = static_cast<int>(ReadInt(f));
  const float beam = Bits(ReadInt(f));
  const int min_active = static_cast<int>(ReadInt(f));
  const float beam_delta = Bits(ReadInt(f));
  const int n_tid = static_cast<int>(ReadInt(f)), rows = static_cast<int>(ReadInt(f)), cols = static_cast<int>(ReadInt(f));
  std::vector<int> tid2pdf(n_tid);
  for (auto &x : tid2pdf) x = static_cast<int>(ReadInt(f));
  std::vector<Utt> utts(n);
  for (Utt &U : utts) {
    U.S = static_cast<int>(ReadInt(f));
    const int A = static_cast<int>(ReadInt(f));
    U.start = static_cast<int>(ReadInt(f));
    U.T = static_cast<int>(ReadInt(f));
    U.row0 = static_cast<int>(ReadInt(f));
    U.room = static_cast<int>(ReadInt(f));
    U.arcs.resize(A);
    for (Arc &a : U.arcs) {
      a.src = static_cast<int>(ReadInt(f)); a.dst = static_cast<int>(ReadInt(f)); a.il = static_cast<int>(ReadInt(f));
      a.ol = static_cast<int>(ReadInt(f)); a.w = Bits(ReadInt(f));
      if (a.src < 0 || a.src >= U.S || a.dst < 0 || a.dst >= U.S || a.il < 0 || a.il >= n_tid ||
          (a.il != 0 && (tid2pdf[a.il] < 0 || tid2pdf[a.il] >= cols))) { fprintf(stderr, "bad arc\n"); return 2; }
      U.n_eps += a.il == 0;
    }
    U.fin.resize(U.S);
    for (float &x : U.fin) x = Bits(ReadInt(f));
    if (U.start < 0 || U.start >= U.S || U.row0 < 0 || U.row0 + U.T > rows) { fprintf(stderr, "bad utterance\n"); return 2; }
  }
  std::vector<float> ll(static_cast<size_t>(rows) * cols);
  for (float &x : ll) x = Bits(ReadInt(f));
  fclose(f);
  std::vector<Result> res(n);
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < std::max(repeat, 1); r++)
    for (int u = 0; u < n; u++) res[u] = Align(utts[u], ll.data(), cols, tid2pdf, beam, min_active, beam_delta);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (repeat > 0) fprintf(stderr, "ms_per_pass %.6f\n", ms / repeat);
  for (int u = 0; u < n; u++) {
    const Result &R = res[u];
    const bool have = R.status == kDone || R.status == kNeedsRoom;
    const double c = have ? R.cost : kInf;
    uint64_t cb;
    memcpy(&cb, &c, 8);
    printf("%d %llu %d %d\n", R.status, static_cast<unsigned long long>(cb), have ? R.best : -1, have ? R.len : 0);
    if (R.status != kDone) continue;
    for (int i = 0; i < R.len; i++) {
      const Arc &A = utts[u].arcs[R.path[i]];
      uint32_t gb, ab;
      memcpy(&gb, &A.w, 4);
      memcpy(&ab, &R.ac[i], 4);
      printf("%d %d %u %u\n", A.il, A.ol, gb, ab);
    }
  }
  return 0;
}
