// latalign_cpu_baseline.cc - the rule of kh_compact_lattice_align_words (include/kaldi_hip.h) on ONE host thread: the baseline
// tools/lattice_align_rate.py times next to the device call, and a second implementation that tests/test_lattice_align_words.py
// compares with the Python restatement bit for bit.  It follows the reference's own shape (lat/word-align-lattice.cc): the
// machine over tuples with its epsilon arcs and LIFO queue, then the epsilon closure of every output state - not the pair
// tables of csrc/kh_latalign.hip.
//
//   latalign_cpu_baseline IN OUT [REPEAT]
// IN: the C call's input arrays, each as an int64 count and the data, in the order tools/lattice_align_rate.py pack() writes.
// OUT: per lattice int32 status, n_tuples, n_states, n_arcs, n_string_words, then final graph / acoustic costs, arc source,
// destination, label, graph, acoustic, string length, strings.  Prints the milliseconds of the best of REPEAT passes.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace {

typedef std::vector<int32_t> Ints;
const float kInf = std::numeric_limits<float>::infinity();
enum { kNoPhone = 0, kBegin, kEnd, kSingleton, kInternal, kNonWord };
enum { kOk = 0, kError, kEmpty, kTooMany, kFatal };

struct Input {
  Ints soff, start, label, next, astr, fstr, tid_phone, tid_final, tid_self, ptype, scalars, max_states;
  std::vector<int64_t> aoff, asoff, fsoff;
  std::vector<float> g, a, fg, fa;
};

struct Weight {
  float g, a;
};

// Compare of fstext/lattice-weight.h:295-308; where it is 0 the smaller acoustic cost
bool Better(Weight x, Weight y) {
  const float f1 = x.g + x.a, f2 = y.g + y.a;
  if (f1 < f2) return true;
  if (f1 > f2) return false;
  if (x.g < y.g) return true;
  if (x.g > y.g) return false;
  return x.a < y.a;
}

struct Arc {
  int32_t label;
  Weight w;
  Ints string;
  int32_t dst;
};

struct Tuple {
  int32_t in;
  Ints tids, words;
  bool operator<(const Tuple &o) const { return std::tie(in, tids, words) < std::tie(o.in, o.tids, o.words); }
};

struct MArc {   // an arc of the machine
  bool eps;
  int32_t label;
  Weight w;
  int32_t n_string;   // the first n_string pending ids of the source tuple
  int32_t dst;
};

struct OutLat {
  int32_t status = kOk, n_tuples = 0;
  std::vector<float> fg, fa, g, a;
  Ints src, dst, label, len, strings;
};

struct Aligner {
  const Input &in;
  int32_t n = 0, sf = -1, start = 0, sil = 0, partial = 0, max_states = 0;
  bool reorder = false, error = false, fatal = false, too_many = false;
  std::vector<std::vector<Arc>> arcs;
  std::map<Tuple, int32_t> map;
  std::vector<Tuple> tuples;
  std::vector<std::vector<MArc>> out;
  std::vector<char> is_final;
  std::vector<int32_t> queue;
  std::string message;

  explicit Aligner(const Input &i) : in(i) {}
  int32_t Phone(int32_t t) const { return in.tid_phone[t]; }
  bool Final(int32_t t) const { return in.tid_final[t] != 0; }
  bool Self(int32_t t) const { return in.tid_self[t] != 0; }
  int32_t Type(int32_t p) const { return in.ptype[p]; }

  int32_t StateFor(const Tuple &t) {                              // GetStateForTuple :159-170
    auto it = map.find(t);
    if (it != map.end()) return it->second;
    const int32_t s = static_cast<int32_t>(tuples.size());
    map[t] = s;
    tuples.push_back(t);
    out.emplace_back();
    is_final.push_back(0);
    queue.push_back(s);
    return s;
  }

  // OutputArc :59-69: the label, the ids consumed and the words dropped
  bool OutputArc(const Ints &t, const Ints &w, int32_t *label, int32_t *consume, int32_t *wdrop) {
    if (t.empty()) return false;
    const int32_t len = static_cast<int32_t>(t.size()), phone = Phone(t[0]), type = Type(phone);
    int32_t i;
    if (type == kBegin && !w.empty()) {                           // :443-528
      for (i = 0; i < len && !Final(t[i]); i++) {}
      if (i == len) return false;
      i++;
      if (reorder) for (; i < len && Self(t[i]); i++) {}
      if (i == len) return false;
      if (Phone(t[i - 1]) != phone) error = true;
      for (; i < len; i++) {
        const int32_t tp = Type(Phone(t[i]));
        if (tp == kEnd) break;
        if (tp != kInternal) error = true;
      }
      if (i == len) return false;
      const int32_t final_phone = Phone(t[i]);
      for (; i < len; i++) {
        if (Phone(t[i]) != final_phone) error = true;
        if (Final(t[i])) break;
      }
      if (i == len) return false;
      i++;
      if (reorder) while (i < len && Self(t[i])) i++;
      if (i == len) return false;
      if (Phone(t[i - 1]) != final_phone) error = true;
      *label = w[0]; *consume = i; *wdrop = 1;
      return true;
    }
    if (type == kNonWord) {                                       // :346-389
      for (i = 1; i < len; i++) {
        if (Phone(t[i]) != phone) error = true;
        if (Final(t[i])) break;
      }
      if (i == len) return false;
      i++;
      if (reorder) while (i < len && Self(t[i])) i++;
      if (i == len) return false;
      *label = sil; *consume = i; *wdrop = 0;
      return true;
    }
    if (type == kSingleton && !w.empty()) {                       // :392-438
      for (i = 1; i < len; i++) if (Final(t[i])) break;
      if (i == len) return false;
      i++;
      if (reorder) while (i < len && Self(t[i])) i++;
      if (i == len) return false;
      if (Phone(t[i - 1]) != phone) error = true;
      *label = w[0]; *consume = i; *wdrop = 1;
      return true;
    }
    return false;
  }

  void Force(const Ints &t, const Ints &w, int32_t *label, int32_t *consume, int32_t *wdrop) {   // :554-635
    const int32_t len = static_cast<int32_t>(t.size());
    *consume = len;
    if (!w.empty() && len > 0) {
      const int32_t first = Phone(t[0]), last = Phone(t[len - 1]);
      bool plausible = false;                                     // :532-551
      if ((Type(first) == kSingleton && first == last) || (Type(first) == kBegin && Type(last) == kEnd)) {
        int32_t k = len - 1;
        if (reorder) while (k > 0 && Self(t[k])) k--;
        plausible = Final(t[k]);
      }
      if (!plausible) error = true;
      *label = w[0]; *wdrop = 1;
    } else if (!w.empty()) {
      error = true;
      *label = 0; *wdrop = static_cast<int32_t>(w.size());
    } else {
      *wdrop = 0;
      const int32_t first = Phone(t[0]);
      if (Type(first) == kNonWord) {
        if (first != Phone(t[len - 1])) {
          fatal = true;
        } else {
          int32_t k = len - 1;
          if (reorder) while (Self(t[k]) && k > 0) k--;
          if (!Final(t[k])) error = true;
        }
        *label = sil;
      } else {
        error = true;
        *label = partial;
      }
    }
  }

  void Process() {                                                // :201-250
    const int32_t s = queue.back();
    queue.pop_back();
    const Tuple T = tuples[s];
    int32_t label, consume, wdrop;
    bool arc = OutputArc(T.tids, T.words, &label, &consume, &wdrop);
    if (!arc && T.in == sf) {
      if (T.tids.empty() && T.words.empty()) {
        is_final[s] = 1;
      } else {
        Force(T.tids, T.words, &label, &consume, &wdrop);
        arc = true;
      }
    }
    if (arc) {
      Tuple D{T.in, Ints(T.tids.begin() + consume, T.tids.end()), Ints(T.words.begin() + wdrop, T.words.end())};
      const int32_t d = StateFor(D);
      out[s].push_back(MArc{false, label, Weight{0.f, 0.f}, consume, d});
      return;
    }
    for (const Arc &x : arcs[T.in]) {                             // Advance :40-48
      Tuple D{x.dst, T.tids, T.words};
      D.tids.insert(D.tids.end(), x.string.begin(), x.string.end());
      if (x.label != 0) D.words.push_back(x.label);
      const int32_t d = StateFor(D);
      out[s].push_back(MArc{true, 0, x.w, 0, d});
    }
  }

  // false: the lattice is refused (message)
  bool Run(int l, OutLat *O) {
    const int32_t s0 = in.soff[l], N = in.soff[l + 1] - s0;
    start = in.start[l];
    if (N == 0 || start < 0) {
      O->status = kEmpty;
      return true;
    }
    reorder = in.scalars[0] != 0;
    const int32_t sil_in = in.scalars[1], partial_in = in.scalars[2];
    max_states = in.max_states[l];
    const int64_t a0 = in.aoff[s0];
    arcs.assign(N, std::vector<Arc>());
    std::vector<int32_t> finals;
    int32_t highest = 0;
    for (int32_t s = 0; s < N; s++) {
      for (int64_t a = in.aoff[s0 + s]; a < in.aoff[s0 + s + 1]; a++) {
        if (in.next[a] <= s || in.next[a] >= N) {
          message = "lattice " + std::to_string(l) + ": arc " + std::to_string(a - a0) + " is not forward";
          return false;
        }
        arcs[s].push_back(Arc{in.label[a], Weight{in.g[a], in.a[a]}, Ints(in.astr.begin() + in.asoff[a], in.astr.begin() + in.asoff[a + 1]),
                              in.next[a]});
        highest = std::max(highest, in.label[a]);
      }
      if (!(in.fg[s0 + s] == kInf && in.fa[s0 + s] == kInf)) finals.push_back(s);
    }
    n = N;
    sf = -1;
    if (finals.size() == 1) {                                     // CreateSuperFinal
      const int32_t f = finals[0];
      if (in.fg[s0 + f] == 0.f && in.fa[s0 + f] == 0.f && in.fsoff[s0 + f] == in.fsoff[s0 + f + 1] && arcs[f].empty()) sf = f;
    }
    if (sf < 0) {
      sf = N;
      n = N + 1;
      arcs.emplace_back();
      for (int32_t f : finals)
        arcs[f].push_back(Arc{0, Weight{in.fg[s0 + f], in.fa[s0 + f]},
                              Ints(in.fstr.begin() + in.fsoff[s0 + f], in.fstr.begin() + in.fsoff[s0 + f + 1]), N});
    }
    std::vector<int32_t> tm(n, -1);
    tm[start] = 0;
    for (int32_t s = 0; s < n; s++) {
      if (tm[s] < 0) continue;
      for (const Arc &x : arcs[s]) {
        const int32_t t = tm[s] + static_cast<int32_t>(x.string.size());
        if (tm[x.dst] >= 0 && tm[x.dst] != t) {
          message = "lattice " + std::to_string(l) + ": state " + std::to_string(x.dst) + " is reached after " +
                    std::to_string(tm[x.dst]) + " and after " + std::to_string(t) + " transition-ids";
          return false;
        }
        tm[x.dst] = t;
      }
    }
    const int32_t unused = 1 + highest;                           // :275-282
    sil = sil_in == 0 ? unused : sil_in;
    partial = partial_in == 0 ? unused : partial_in;
    StateFor(Tuple{start, Ints(), Ints()});
    while (!queue.empty()) {                                      // :314-323
      if (max_states > 0 && static_cast<int32_t>(tuples.size()) > max_states) {
        too_many = true;
        break;
      }
      Process();
    }
    O->n_tuples = static_cast<int32_t>(tuples.size());
    if (too_many) {
      O->n_tuples = max_states + 1;   // the contract's count for this status; tuples.size() depends on the queue order
      O->status = kTooMany;
      return true;
    }
    if (fatal) {
      O->status = kFatal;
      return true;
    }
    O->status = error ? kError : kOk;
    // the epsilon closure of every output state, tuples in ascending input state
    const int32_t nT = O->n_tuples;
    std::vector<char> is_out(nT, 0);
    is_out[0] = 1;
    for (const auto &v : out) for (const MArc &x : v) if (!x.eps) is_out[x.dst] = 1;
    std::vector<int32_t> by_in(nT), states;
    for (int32_t t = 0; t < nT; t++) by_in[t] = t;
    std::stable_sort(by_in.begin(), by_in.end(), [&](int32_t x, int32_t y) { return tuples[x].in < tuples[y].in; });
    for (int32_t t = 0; t < nT; t++) if (is_out[t]) states.push_back(t);
    auto key_less = [&](int32_t x, int32_t y) {
      if (x == 0 || y == 0) return x == 0 && y != 0;
      const Tuple &X = tuples[x], &Y = tuples[y];
      const int32_t tx = tm[X.in] - static_cast<int32_t>(X.tids.size()), ty = tm[Y.in] - static_cast<int32_t>(Y.tids.size());
      if (tx != ty) return tx < ty;
      if (X.in != Y.in) return X.in < Y.in;
      if (X.words.size() != Y.words.size()) return X.words.size() > Y.words.size();
      if (X.words != Y.words) return X.words < Y.words;
      return X.tids < Y.tids;
    };
    std::sort(states.begin(), states.end(), key_less);
    const int32_t m = static_cast<int32_t>(states.size());
    std::vector<int32_t> num(nT, -1);
    for (int32_t i = 0; i < m; i++) num[states[i]] = i;
    struct OArc { int32_t dst, label; Weight w; int32_t tuple, len; };
    std::vector<std::vector<OArc>> oarcs(m);
    std::vector<Weight> fin(m, Weight{kInf, kInf});
    std::vector<Weight> d(nT);
    std::vector<int32_t> seen(nT, -1);
    for (int32_t i = 0; i < m; i++) {
      const int32_t S = states[i];
      seen[S] = i;
      d[S] = Weight{0.f, 0.f};
      for (int32_t T : by_in) {
        if (seen[T] != i) continue;
        if (is_final[T] && Better(d[T], fin[i])) fin[i] = d[T];
        for (const MArc &x : out[T]) {
          if (x.eps) {
            const Weight c{d[T].g + x.w.g, d[T].a + x.w.a};
            if (seen[x.dst] != i || Better(c, d[x.dst])) d[x.dst] = c;
            seen[x.dst] = i;
          } else {
            oarcs[i].push_back(OArc{num[x.dst], x.label, d[T], T, x.n_string});
          }
        }
      }
    }
    std::vector<char> keep(m, 0);
    for (int32_t i = m - 1; i >= 0; i--) {
      keep[i] = !(fin[i].g == kInf && fin[i].a == kInf);
      for (const OArc &x : oarcs[i]) keep[i] = keep[i] || keep[x.dst];
    }
    if (!keep[0]) return true;
    std::vector<int32_t> renum(m, -1);
    int32_t k = 0;
    for (int32_t i = 0; i < m; i++) if (keep[i]) renum[i] = k++;
    auto better_arc = [&](const OArc &x, const OArc &y) {          // fstext/lattice-weight.h:562-576
      if (Better(x.w, y.w)) return true;
      if (Better(y.w, x.w)) return false;
      if (x.len != y.len) return x.len < y.len;
      const Ints &p = tuples[x.tuple].tids, &q = tuples[y.tuple].tids;
      for (int32_t j = 0; j < x.len; j++) if (p[j] != q[j]) return p[j] > q[j];
      return false;
    };
    for (int32_t i = 0; i < m; i++) {
      if (!keep[i]) continue;
      O->fg.push_back(fin[i].g);
      O->fa.push_back(fin[i].a);
      std::vector<OArc> &v = oarcs[i];
      v.erase(std::remove_if(v.begin(), v.end(), [&](const OArc &x) { return !keep[x.dst]; }), v.end());
      std::stable_sort(v.begin(), v.end(), [&](const OArc &x, const OArc &y) {
        if (x.dst != y.dst) return x.dst < y.dst;
        if (x.label != y.label) return x.label < y.label;
        return better_arc(x, y);
      });
      for (size_t j = 0; j < v.size(); j++) {
        if (j > 0 && v[j].dst == v[j - 1].dst && v[j].label == v[j - 1].label) continue;
        const OArc &x = v[j];
        int32_t label = x.label;
        if ((sil_in == 0 && label == sil) || (partial_in == 0 && label == partial)) label = 0;
        O->src.push_back(renum[i]);
        O->dst.push_back(renum[x.dst]);
        O->label.push_back(label);
        O->g.push_back(x.w.g);
        O->a.push_back(x.w.a);
        O->len.push_back(x.len);
        const Ints &p = tuples[x.tuple].tids;
        O->strings.insert(O->strings.end(), p.begin(), p.begin() + x.len);
      }
    }
    return true;
  }
};

template <typename T>
bool ReadArray(FILE *f, std::vector<T> *v) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (1ll << 32)) return false;
  v->resize(static_cast<size_t>(n));
  return n == 0 || fread(v->data(), sizeof(T), static_cast<size_t>(n), f) == static_cast<size_t>(n);
}

template <typename T>
void WriteArray(FILE *f, const std::vector<T> &v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

bool ReadInput(const char *path, Input *in, std::string *why) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    *why = std::string("cannot open ") + path;
    return false;
  }
  const bool ok = ReadArray(f, &in->soff) && ReadArray(f, &in->start) && ReadArray(f, &in->aoff) && ReadArray(f, &in->label) &&
                  ReadArray(f, &in->next) && ReadArray(f, &in->g) && ReadArray(f, &in->a) && ReadArray(f, &in->asoff) &&
                  ReadArray(f, &in->astr) && ReadArray(f, &in->fg) && ReadArray(f, &in->fa) && ReadArray(f, &in->fsoff) &&
                  ReadArray(f, &in->fstr) && ReadArray(f, &in->tid_phone) && ReadArray(f, &in->tid_final) &&
                  ReadArray(f, &in->tid_self) && ReadArray(f, &in->ptype) && ReadArray(f, &in->scalars) && ReadArray(f, &in->max_states);
  const bool at_end = ok && fgetc(f) == EOF;
  fclose(f);
  if (!ok || !at_end) {
    *why = "the input does not match its header";
    return false;
  }
  const size_t n = in->soff.empty() ? 0 : in->soff.size() - 1;
  const size_t S = n ? static_cast<size_t>(in->soff[n]) : 0;
  if (n == 0 || in->soff[0] != 0 || in->start.size() != n || in->max_states.size() != n || in->aoff.size() != S + 1 ||
      in->fg.size() != S || in->fa.size() != S || in->fsoff.size() != S + 1 || in->scalars.size() != 3 ||
      in->tid_final.size() != in->tid_phone.size() || in->tid_self.size() != in->tid_phone.size()) {
    *why = "the input's arrays do not fit each other";
    return false;
  }
  const size_t A = static_cast<size_t>(in->aoff[S]);
  if (in->aoff[0] != 0 || in->label.size() != A || in->next.size() != A || in->g.size() != A || in->a.size() != A ||
      in->asoff.size() != A + 1 || in->asoff[0] != 0 || static_cast<size_t>(in->asoff[A]) != in->astr.size() || in->fsoff[0] != 0 ||
      static_cast<size_t>(in->fsoff[S]) != in->fstr.size()) {
    *why = "the input's arrays do not fit each other";
    return false;
  }
  for (size_t s = 0; s < S; s++) if (in->aoff[s + 1] < in->aoff[s] || in->fsoff[s + 1] < in->fsoff[s]) { *why = "offsets descend"; return false; }
  for (size_t a = 0; a < A; a++) if (in->asoff[a + 1] < in->asoff[a]) { *why = "offsets descend"; return false; }
  const int32_t num_tids = static_cast<int32_t>(in->tid_phone.size()) - 1, n_types = static_cast<int32_t>(in->ptype.size());
  for (int32_t t = 1; t <= num_tids; t++) if (in->tid_phone[t] < 0 || in->tid_phone[t] >= n_types) { *why = "a phone outside the word-boundary table"; return false; }
  for (const Ints *v : {&in->astr, &in->fstr}) for (int32_t t : *v) if (t < 1 || t > num_tids) { *why = "a transition-id outside the model"; return false; }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: latalign_cpu_baseline IN OUT [REPEAT]\n");
    return 2;
  }
  Input in;
  std::string why;
  if (!ReadInput(argv[1], &in, &why)) {
    fprintf(stderr, "latalign_cpu_baseline: %s\n", why.c_str());
    return 1;
  }
  const int repeat = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
  const int n = static_cast<int>(in.soff.size()) - 1;
  std::vector<OutLat> outs;
  double best = 1e300;
  for (int r = 0; r < repeat; r++) {
    outs.assign(n, OutLat());
    const auto t0 = std::chrono::steady_clock::now();
    for (int l = 0; l < n; l++) {
      Aligner A(in);
      if (!A.Run(l, &outs[l])) {
        fprintf(stderr, "latalign_cpu_baseline: %s\n", A.message.c_str());
        return 1;
      }
    }
    best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  FILE *f = fopen(argv[2], "wb");
  if (!f) {
    fprintf(stderr, "latalign_cpu_baseline: cannot write %s\n", argv[2]);
    return 1;
  }
  for (const OutLat &O : outs) {
    const int32_t head[5] = {O.status, O.n_tuples, static_cast<int32_t>(O.fg.size()), static_cast<int32_t>(O.src.size()),
                             static_cast<int32_t>(O.strings.size())};
    fwrite(head, sizeof(int32_t), 5, f);
    WriteArray(f, O.fg); WriteArray(f, O.fa); WriteArray(f, O.src); WriteArray(f, O.dst); WriteArray(f, O.label);
    WriteArray(f, O.g); WriteArray(f, O.a); WriteArray(f, O.len); WriteArray(f, O.strings);
  }
  fclose(f);
  printf("%.6f\n", best);
  return 0;
}
