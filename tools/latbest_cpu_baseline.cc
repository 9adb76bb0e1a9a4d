// A plain single-thread C++ restatement of lattice-scale | lattice-add-penalty | CompactLatticeShortestPath
// (lat/lattice-functions.cc:1060-1125) for ONE score point over CSR arrays: the baseline of tools/bench_lattice_best_path.py
// - what each of the 36 CPU jobs of local/score.sh computes, minus their I/O.  Not the code under test: it shares
// nothing with csrc/kh_latbest.hip (push form over outgoing arcs, as the reference has it).  g++ -O2 -ffp-contract=off.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

static inline void Scale(float g, float a, const double *s, float *g2, float *a2) {
  if (g == std::numeric_limits<float>::infinity()) { *g2 = g; *a2 = g; return; }
  *g2 = static_cast<float>(s[0] * g + s[1] * a);
  *a2 = static_cast<float>(s[2] * g + s[3] * a);
}

extern "C" int64_t latbest_cpu(int n_lats, const int32_t *lat_off, const int64_t *arc_off, const int32_t *label, const int32_t *next,
                               const float *g, const float *a, const float *fg, const float *fa, const double *scale, float pen,
                               int32_t *path_len, float *tot_g, float *tot_a) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> cost;
  std::vector<int32_t> pred, states;
  std::vector<float> g2, a2;
  int64_t checksum = 0;
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_off[l], ns = lat_off[l + 1] - s0;
    const int64_t a0 = arc_off[s0], na = arc_off[s0 + ns] - a0;
    g2.resize(na); a2.resize(na);
    for (int64_t j = 0; j < na; j++) {      // the scaled, penalised lattice the search reads (the first two programs)
      Scale(g[a0 + j], a[a0 + j], scale, &g2[j], &a2[j]);
      if (label[a0 + j] != 0) g2[j] = g2[j] + pen;
    }
    cost.assign(ns + 1, inf);
    pred.assign(ns + 1, -1);
    cost[0] = 0;
    for (int32_t s = 0; s < ns; s++) {
      const double my = cost[s];
      for (int64_t j = arc_off[s0 + s] - a0; j < arc_off[s0 + s + 1] - a0; j++) {
        const double nc = my + (static_cast<double>(g2[j]) + static_cast<double>(a2[j]));
        const int32_t nx = next[a0 + j];
        if (nc < cost[nx]) { cost[nx] = nc; pred[nx] = s; }
      }
      float f1, f2;
      Scale(fg[s0 + s], fa[s0 + s], scale, &f1, &f2);
      const double tf = my + (static_cast<double>(f1) + static_cast<double>(f2));
      if (tf < cost[ns]) { cost[ns] = tf; pred[ns] = s; }
    }
    states.clear();
    int32_t cur = ns;
    bool ok = true;
    while (cur != 0) {
      const int32_t prev = pred[cur];
      if (prev < 0) { ok = false; break; }
      states.push_back(prev);
      cur = prev;
    }
    if (!ok) { path_len[l] = -1; continue; }
    float tg = 0.f, ta = 0.f;
    for (std::size_t i = states.size(); i-- > 0;) {
      const int32_t s = states[i];
      if (i > 0) {
        int64_t best = -1;
        for (int64_t j = arc_off[s0 + s] - a0; j < arc_off[s0 + s + 1] - a0; j++)
          if (next[a0 + j] == states[i - 1] &&
              (best < 0 || static_cast<double>(g2[j]) + static_cast<double>(a2[j]) < static_cast<double>(g2[best]) + static_cast<double>(a2[best])))
            best = j;
        tg = tg + g2[best]; ta = ta + a2[best];
        checksum += best;
      } else {
        float f1, f2;
        Scale(fg[s0 + s], fa[s0 + s], scale, &f1, &f2);
        tg = tg + f1; ta = ta + f2;
      }
    }
    path_len[l] = static_cast<int32_t>(states.size()) - 1;
    tot_g[l] = tg; tot_a[l] = ta;
  }
  return checksum;
}
