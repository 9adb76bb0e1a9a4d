// A plain single-thread C++ implementation of the oracle path of latbin/lattice-oracle.cc as the integer dynamic programme
// kh_compact_lattice_oracle computes (include/kaldi_hip.h), over the same CSR arrays and mask words, one (lattice, point)
// after the other: the baseline of tools/lattice_oracle_rate.py.  Not the code under test: it shares nothing with
// csrc/kh_latoracle.hip - push form over outgoing arcs with a back-pointer per cell, where the kernel pulls over
// incoming-arc lists and searches the stored rows again on the walk back.  Strict "<" updates in the order the candidates
// arrive (sources by ascending state, their arcs in order = ascending arc number, an arc's diagonal before its insertion,
// the deletion when the row is complete) keep the FIRST candidate that attains a cell's value, which is the library's tie
// rule, so every output can be compared.  No state_keep and no frame sums.  g++ -O2.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
constexpr int32_t kSent = 0x3fffffff;
enum : uint8_t { kNone = 0, kEps = 1, kDiag = 2, kIns = 3, kDel = 4 };

inline bool Bit(const uint64_t *m, int64_t i, int64_t W, int p) {
  return m == nullptr || ((m[i * W + (p >> 6)] >> (p & 63)) & 1) != 0;
}
}  // namespace

// Returns the number of (lattice, point) pairs with a path, or -1 for arguments it does not take (an arc to a state that is
// not higher-numbered, a start state out of range, path room below n_states - 1).
extern "C" int64_t latoracle_cpu(int n_lats, const int32_t *lat_off, const int32_t *lat_start, const int64_t *arc_off,
                                 const int32_t *label, const int32_t *next, const int32_t *is_final, const int64_t *ref_off,
                                 const int32_t *ref_words, int n_wild, const int32_t *wild, int n_points,
                                 const uint64_t *arc_keep, const uint64_t *final_keep, int32_t *errors, int32_t *counts,
                                 int32_t *path_len, int32_t *path_arcs, const int64_t *path_offsets, int32_t *path_final) {
  const int64_t W = (static_cast<int64_t>(n_points) + 63) / 64;
  auto word = [&](int32_t w) { return std::binary_search(wild, wild + n_wild, w) ? 0 : w; };
  std::vector<int32_t> r, D, bp_arc, lab;
  std::vector<uint8_t> bp_type;
  int64_t n_ok = 0;
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_off[l], ns = lat_off[l + 1] - s0, start = lat_start[l];
    const int64_t a0 = arc_off[s0], na = arc_off[s0 + ns] - a0;
    if (start < 0 || start >= ns) return -1;
    r.assign(1, 0);                                              // r[1..R]
    for (int64_t i = ref_off[l]; i < ref_off[l + 1]; i++)
      if (word(ref_words[i]) != 0) r.push_back(ref_words[i]);
    const int64_t R = static_cast<int64_t>(r.size()) - 1, RS = R + 1;
    lab.resize(na);
    for (int64_t a = 0; a < na; a++) lab[a] = word(label[a0 + a]);
    for (int p = 0; p < n_points; p++) {
      const int64_t o = static_cast<int64_t>(l) * n_points + p;
      if (path_offsets[o + 1] - path_offsets[o] < ns - 1) return -1;
      D.assign(static_cast<size_t>(ns) * RS, kSent);
      bp_arc.assign(static_cast<size_t>(ns) * RS, -1);
      bp_type.assign(static_cast<size_t>(ns) * RS, kNone);
      for (int64_t j = 0; j <= R; j++) D[start * RS + j] = static_cast<int32_t>(j);
      int32_t best = kSent, end = -1;
      for (int32_t s = start; s < ns; s++) {
        int32_t *row = &D[s * RS];
        if (s != start) {                                        // every arc into s has been seen: the deletions close the row
          for (int64_t j = 1; j <= R; j++)
            if (row[j - 1] + 1 < row[j]) {
              row[j] = row[j - 1] + 1;
              bp_type[s * RS + j] = kDel;
            }
        }
        if (row[R] < best && is_final[s0 + s] != 0 && Bit(final_keep, s0 + s, W, p)) {
          best = row[R];
          end = s;
        }
        if (row[0] >= kSent) continue;                           // not reachable over kept arcs (a row is, in all its cells or in none)
        for (int64_t a = arc_off[s0 + s] - a0; a < arc_off[s0 + s + 1] - a0; a++) {
          const int32_t e = next[a0 + a];
          if (e <= s || e >= ns) return -1;
          if (!Bit(arc_keep, a0 + a, W, p)) continue;
          int32_t *dst = &D[e * RS];
          int32_t *ba = &bp_arc[e * RS];
          uint8_t *bt = &bp_type[e * RS];
          const int32_t w = lab[a];
          if (w == 0) {
            for (int64_t j = 0; j <= R; j++)
              if (row[j] < dst[j]) { dst[j] = row[j]; ba[j] = static_cast<int32_t>(a); bt[j] = kEps; }
          } else {
            for (int64_t j = 0; j <= R; j++) {
              if (j >= 1) {
                const int32_t d = row[j - 1] + (w != r[j] ? 1 : 0);
                if (d < dst[j]) { dst[j] = d; ba[j] = static_cast<int32_t>(a); bt[j] = kDiag; }
              }
              if (row[j] + 1 < dst[j]) { dst[j] = row[j] + 1; ba[j] = static_cast<int32_t>(a); bt[j] = kIns; }
            }
          }
        }
      }
      counts[4 * o] = counts[4 * o + 1] = counts[4 * o + 2] = counts[4 * o + 3] = 0;
      if (best >= kSent) {
        errors[o] = -1;
        path_len[o] = -1;
        path_final[o] = -1;
        continue;
      }
      n_ok++;
      int32_t *out = path_arcs + path_offsets[o];
      int32_t len = 0, e = end;
      int64_t j = R;
      // the source state of an arc: the arcs are in CSR order, so the state whose range holds it
      auto source = [&](int32_t a) {
        return static_cast<int32_t>(std::upper_bound(arc_off + s0, arc_off + s0 + ns, a0 + a) - (arc_off + s0)) - 1;
      };
      while (e != start) {
        const uint8_t t = bp_type[e * RS + j];
        if (t == kDel) {
          counts[4 * o + 3]++;
          j--;
          continue;
        }
        const int32_t a = bp_arc[e * RS + j];
        out[len++] = a;
        if (t == kDiag) {
          counts[4 * o + (lab[a] == r[j] ? 0 : 1)]++;
          j--;
        } else if (t == kIns) {
          counts[4 * o + 2]++;
        }
        e = source(a);
      }
      counts[4 * o + 3] += static_cast<int32_t>(j);              // D[start][j > 0] is a deletion
      std::reverse(out, out + len);
      errors[o] = best;
      path_len[o] = len;
      path_final[o] = end;
    }
  }
  return n_ok;
}
