// kh_latbest.hip — CompactLatticeShortestPath (lat/lattice-functions.cc:1043-1126) for a batch of top-sorted
// CompactLattices and K "score points" at once.  A score point is what lattice-scale (latbin/lattice-scale.cc:76-82) and
// lattice-add-penalty (lat/lattice-functions.cc:1128-1149) do to a weight before lattice-best-path searches: a 2x2 matrix
// of doubles and a float word insertion penalty.  The scoring scripts run the same search 36 times over the same graph;
// here the points are the lanes of a wavefront.
//
// Shape: one wave per (lattice, group of 64 points), lane = point.  The arc records are wave-uniform (one load serves
// every point), the per-state rows cost[state][point] / pred[state][point] are contiguous across lanes, and every lane
// executes the reference's statements in the reference's order, so its tie rules hold without any extra care:
//   * the relaxation runs in "pull" form over the incoming arcs of a state kept in (source state, arc position) order.
//     That is the order in which :1067-1079 offers candidates to best_cost_and_pred[nextstate], and "replace only on
//     strictly smaller" (:1075) then leaves the lowest-numbered source state on a tie - one store per state instead of
//     a read-modify-write per arc;
//   * the arc between two consecutive path states is chosen by ARC cost alone, the first on a tie (:1107-1118).  It is
//     searched for again during the trace-back and not remembered from the relaxation: two parallel arcs whose costs
//     differ can round to the same my_cost + arc_cost, and then the relaxation kept the first while :1113 takes the cheaper.
// The lanes never exchange data, so there are no barriers and no cross-lane operations.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"
#include "kh_scorepoint.h"

namespace kh {
namespace {

constexpr int kLanes = 64;

struct BpLat {
  int64_t state_base;  // first state of the lattice in the batch's state arrays
  int64_t ws_row;      // first row of the lattice in the workspace (cost / pred), rows of n_points
  int64_t path_row;    // first row of the lattice in the path buffer, rows of n_points
  int64_t arc_base;    // first arc of the lattice in the caller's arc order (path arcs are reported relative to it)
  int32_t n_states;
  int32_t depth;       // arcs on the longest path of the lattice = rows it owns in the path buffer
  int32_t lat;         // index in the caller's batch
  int32_t pad;
};

__global__ __launch_bounds__(kLanes) void BestPathKernel(
    const BpLat *__restrict__ lats, const int64_t *__restrict__ in_off, const int32_t *__restrict__ in_src,
    const int32_t *__restrict__ in_arc, const int32_t *__restrict__ in_label, const float *__restrict__ in_g,
    const float *__restrict__ in_a, const float *__restrict__ fin_g, const float *__restrict__ fin_a,
    const double *__restrict__ scales, const float *__restrict__ penalties, int n_points, double *cost, int32_t *pred,
    int32_t *path, int32_t *out_len, int32_t *out_final, float *out_g, float *out_a, int32_t *err) {
  // (out_*: row blockIdx.x of this launch, n_points entries per lattice; the host scatters them to the caller's order)
  const BpLat L = lats[blockIdx.x];
  const int p = blockIdx.y * kLanes + threadIdx.x;
  if (p >= n_points) return;
  const Point pt = LoadPoint(scales, penalties, p);
  const int64_t P = n_points;
  double *c = cost + L.ws_row * P + p;
  int32_t *pr = pred + L.ws_row * P + p;
  const int64_t *io = in_off + L.state_base;
  const float *fg = fin_g + L.state_base, *fa = fin_a + L.state_base;
  const double inf = std::numeric_limits<double>::infinity();
  // :1060-1086
  double best_final = inf;
  int32_t pred_final = -1;
  for (int32_t s = 0; s < L.n_states; s++) {
    double best = s == 0 ? 0.0 : inf;   // :1063,:1066
    int32_t bp = -1;                     // kNoStateId :1064
    const int64_t k1 = io[s + 1];
    for (int64_t k = io[s]; k < k1; k++) {
      const int32_t src = in_src[k];
      float g2, a2;
      ArcWeight(in_g[k], in_a[k], in_label[k], pt, &g2, &a2);
      const double next_cost = c[src * P] + Cost(g2, a2);   // :1073-1074
      if (next_cost < best) {                               // :1075
        best = next_cost;
        bp = src;
      }
    }
    c[s * P] = best;
    pr[s * P] = bp;
    float g2, a2;
    ScaleWeight(fg[s], fa[s], pt, &g2, &a2);
    const double tot_final = best + Cost(g2, a2);           // :1080-1081
    if (tot_final < best_final) {                           // :1082
      best_final = tot_final;
      pred_final = s;
    }
  }
  const int64_t o = static_cast<int64_t>(blockIdx.x) * P + p;
  out_final[o] = pred_final;
  out_g[o] = 0.f;
  out_a[o] = 0.f;
  if (pred_final < 0) {   // :1091 "Failure in best-path algorithm for lattice (infinite costs?)"
    out_len[o] = -1;
    return;
  }
  // :1088-1098 and :1102-1121, walking backwards: the path row i holds the position in the incoming arrays of the arc
  // into the (i+1)-th state from the end
  int32_t *pth = path + L.path_row * P + p;
  int32_t n = 0;
  for (int32_t cur = pred_final; cur != 0;) {
    const int32_t prev = pr[cur * P];
    if (prev < 0) {       // :1091
      out_len[o] = -1;
      out_final[o] = -1;
      return;
    }
    int64_t best_k = -1;
    double best_cost = 0.0;
    const int64_t k1 = io[cur + 1];
    for (int64_t k = io[cur]; k < k1; k++) {
      if (in_src[k] != prev) continue;                       // :1111
      float g2, a2;
      ArcWeight(in_g[k], in_a[k], in_label[k], pt, &g2, &a2);
      const double ac = Cost(g2, a2);
      if (best_k < 0 || ac < best_cost) {                    // :1112-1113
        best_k = k;
        best_cost = ac;
      }
    }
    if (n >= L.depth || best_k < 0) {   // cannot happen on a validated lattice; never write past the lattice's rows
      atomicExch(err, 1);
      out_len[o] = -1;
      return;
    }
    pth[static_cast<int64_t>(n) * P] = static_cast<int32_t>(best_k);
    n++;
    cur = prev;
  }
  // GetLinearSymbolSequence's total (lattice-best-path.cc:98): One, Times every path arc's weight in path order, the final
  // weight last; LatticeWeight Times = float sums of the two values
  float tg = 0.f, ta = 0.f;
  for (int32_t i = n - 1; i >= 0; i--) {
    const int64_t k = pth[static_cast<int64_t>(i) * P];
    float g2, a2;
    ArcWeight(in_g[k], in_a[k], in_label[k], pt, &g2, &a2);
    tg = tg + g2;
    ta = ta + a2;
  }
  {
    float g2, a2;
    ScaleWeight(fg[pred_final], fa[pred_final], pt, &g2, &a2);
    tg = tg + g2;
    ta = ta + a2;
  }
  // into path order, as arc numbers of the caller (relative to the lattice's first arc)
  for (int32_t i = 0, j = n - 1; i <= j; i++, j--) {
    const int32_t ki = pth[static_cast<int64_t>(i) * P], kj = pth[static_cast<int64_t>(j) * P];
    pth[static_cast<int64_t>(i) * P] = in_arc[kj];
    pth[static_cast<int64_t>(j) * P] = in_arc[ki];
  }
  out_len[o] = n;
  out_g[o] = tg;
  out_a[o] = ta;
}

thread_local CallStats<5, 1> g_stats;   // counts: kernel launches of the last call

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" int kh_compact_lattice_best_paths_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_compact_lattice_best_paths_last_timings(float *ms5, int32_t *n_launches) {
  return GetTimings(g_stats, ms5, n_launches);
}

extern "C" int kh_compact_lattice_best_paths(int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets,
                                             const int32_t *arc_label, const int32_t *arc_nextstate, const float *arc_graph,
                                             const float *arc_acoustic, const float *final_graph, const float *final_acoustic,
                                             int n_points, const double *scales, const float *penalties, int32_t *path_len,
                                             int32_t *path_arcs, const int64_t *path_offsets, int32_t *path_final_state,
                                             float *tot_graph, float *tot_acoustic) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && arc_offsets && arc_label && arc_nextstate && arc_graph && arc_acoustic &&
               final_graph && final_acoustic && n_points > 0 && scales && penalties && path_len && path_arcs && path_offsets &&
               path_final_state && tot_graph && tot_acoustic);
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0);
  for (int l = 0; l < n_lats; l++) KH_CHECK_ARG(lat_state_offsets[l + 1] - lat_state_offsets[l] > 0);
  CallTimer T;
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  KH_CHECK_ARG(A >= 0 && A < (1ll << 31));   // (positions in the incoming arrays are kept as int32 in the path rows)
  const int64_t P = n_points;
  for (int64_t i = 0; i < static_cast<int64_t>(n_lats) * P; i++) KH_CHECK_ARG(path_offsets[i + 1] >= path_offsets[i]);

  // validation (:1046, :1056), the incoming lists, and per lattice the arcs on its longest path
  std::vector<BpLat> lats(n_lats);
  std::vector<int32_t> depth, in_label(A);
  std::vector<float> in_g(A), in_a(A);
  int32_t max_depth = 0;
  Incoming in;
  std::string err;
  if (!BuildIncoming(
          "kh_compact_lattice_best_paths", n_lats, lat_state_offsets, nullptr, arc_offsets, arc_nextstate, &in, &err,
          [&](int, int32_t, int32_t ns) {
            depth.assign(ns, 0);
            max_depth = 0;
            return true;
          },
          [&](int, int32_t, int32_t s) {
            max_depth = std::max(max_depth, depth[s]);
            return true;
          },
          [&](int, int32_t s, int64_t, int32_t nx) {
            depth[nx] = std::max(depth[nx], depth[s] + 1);
            return true;
          },
          [&](int l, int32_t s0, int32_t ns) {
            BpLat &L = lats[l];
            L.state_base = s0;
            L.arc_base = arc_offsets[s0];
            L.n_states = ns;
            L.depth = std::max(max_depth, 1);
            L.lat = l;
            L.pad = 0;
            return true;
          },
          [&](int, int64_t k, int64_t j) {
            in_label[k] = arc_label[j];
            in_g[k] = arc_graph[j];
            in_a[k] = arc_acoustic[j];
          })) {
    SetError("%s", err.c_str());
    return KH_EINVAL;
  }
  // the lattices in flight: longest first, as many as the workspace limit admits per launch (at least one)
  size_t limit = g_stats.workspace_limit;
  if (limit == 0 && (rc = DefaultWorkspaceLimit(static_cast<size_t>(A) * 20 + static_cast<size_t>(S) * 16, &limit)) != KH_OK)
    return rc;
  std::vector<size_t> ws_bytes(n_lats), n_states(n_lats);
  for (int l = 0; l < n_lats; l++) {
    ws_bytes[l] = (static_cast<size_t>(lats[l].n_states) * 12 + static_cast<size_t>(lats[l].depth) * 4) * static_cast<size_t>(P);
    n_states[l] = lats[l].n_states;
  }
  const ChunkPlan plan = PlanChunks(ws_bytes, limit, 65535, &n_states);
  struct Rows { int64_t ws, path; };
  std::vector<Rows> rows;
  std::vector<BpLat> sorted(n_lats);
  int64_t max_ws_rows = 0, max_path_rows = 0;
  size_t max_chunk_lats = 0;
  for (const ChunkRange &c : plan.ranges) {
    Rows r{0, 0};
    for (size_t i = c.begin; i < c.end; i++) {
      BpLat L = lats[plan.order[i]];
      L.ws_row = r.ws;
      L.path_row = r.path;
      r.ws += L.n_states;
      r.path += L.depth;
      sorted[i] = L;
    }
    max_ws_rows = std::max(max_ws_rows, r.ws);
    max_path_rows = std::max(max_path_rows, r.path);
    max_chunk_lats = std::max(max_chunk_lats, c.end - c.begin);
    rows.push_back(r);
  }
  T.HostDone();

  hipStream_t st = Stream();
  KH_HIP(T.Init());
  Dev<BpLat> d_lats;
  Dev<int64_t> d_in_off;
  Dev<int32_t> d_in_src, d_in_arc, d_in_label, d_pred, d_path, d_len, d_final, d_err;
  Dev<float> d_in_g, d_in_a, d_fin_g, d_fin_a, d_pen, d_tg, d_ta;
  Dev<double> d_scales, d_cost;
  const size_t LP = max_chunk_lats * P;   // per-path results of one launch, in launch order
  if (d_lats.Alloc(n_lats) || d_in_off.Alloc(S + 1) || d_in_src.Alloc(A) || d_in_arc.Alloc(A) || d_in_label.Alloc(A) ||
      d_in_g.Alloc(A) || d_in_a.Alloc(A) || d_fin_g.Alloc(S) || d_fin_a.Alloc(S) || d_scales.Alloc(4 * P) || d_pen.Alloc(P) ||
      d_len.Alloc(LP) || d_final.Alloc(LP) || d_tg.Alloc(LP) || d_ta.Alloc(LP) || d_err.Alloc(1) ||
      d_cost.Alloc(static_cast<size_t>(max_ws_rows) * P) || d_pred.Alloc(static_cast<size_t>(max_ws_rows) * P) ||
      d_path.Alloc(static_cast<size_t>(max_path_rows) * P)) {
    SetError("kh_compact_lattice_best_paths: out of device memory (workspace of %lld rows x %d points)",
             static_cast<long long>(max_ws_rows), n_points);
    return KH_ENOMEM;
  }
  KH_HIP(T.Mark(0, st));
  KH_HIP(Up(d_lats, sorted.data(), n_lats, st));
  KH_HIP(Up(d_in_off, in.in_off.data(), S + 1, st));
  KH_HIP(Up(d_in_src, in.in_src.data(), A, st));
  KH_HIP(Up(d_in_arc, in.in_arc.data(), A, st));
  KH_HIP(Up(d_in_label, in_label.data(), A, st));
  KH_HIP(Up(d_in_g, in_g.data(), A, st));
  KH_HIP(Up(d_in_a, in_a.data(), A, st));
  KH_HIP(Up(d_fin_g, final_graph, S, st));
  KH_HIP(Up(d_fin_a, final_acoustic, S, st));
  KH_HIP(Up(d_scales, scales, 4 * P, st));
  KH_HIP(Up(d_pen, penalties, P, st));
  KH_HIP(hipMemsetAsync(d_err.p, 0, sizeof(int32_t), st));
  KH_HIP(T.Mark(1, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.Add(&T.up, 0, 1));

  std::vector<int32_t> h_path(static_cast<size_t>(max_path_rows) * P), h_len(LP), h_final(LP);
  std::vector<float> h_tg(LP), h_ta(LP);
  const int groups = static_cast<int>((P + kLanes - 1) / kLanes);
  for (size_t ci = 0; ci < plan.ranges.size(); ci++) {
    const ChunkRange &c = plan.ranges[ci];
    KH_HIP(T.Mark(1, st));
    hipLaunchKernelGGL(BestPathKernel, dim3(c.end - c.begin, groups), dim3(kLanes), 0, st, d_lats.p + c.begin, d_in_off.p,
                       d_in_src.p, d_in_arc.p, d_in_label.p, d_in_g.p, d_in_a.p, d_fin_g.p, d_fin_a.p, d_scales.p, d_pen.p,
                       n_points, d_cost.p, d_pred.p, d_path.p, d_len.p, d_final.p, d_tg.p, d_ta.p, d_err.p);
    KH_LAUNCH_CHECK();
    KH_HIP(T.Mark(2, st));
    KH_HIP(hipMemcpyAsync(h_path.data(), d_path.p, sizeof(int32_t) * static_cast<size_t>(rows[ci].path) * P, hipMemcpyDeviceToHost, st));
    const size_t CP = (c.end - c.begin) * P;
    KH_HIP(hipMemcpyAsync(h_len.data(), d_len.p, sizeof(int32_t) * CP, hipMemcpyDeviceToHost, st));
    KH_HIP(hipMemcpyAsync(h_final.data(), d_final.p, sizeof(int32_t) * CP, hipMemcpyDeviceToHost, st));
    KH_HIP(hipMemcpyAsync(h_tg.data(), d_tg.p, sizeof(float) * CP, hipMemcpyDeviceToHost, st));
    KH_HIP(hipMemcpyAsync(h_ta.data(), d_ta.p, sizeof(float) * CP, hipMemcpyDeviceToHost, st));
    KH_HIP(T.Mark(3, st));
    KH_HIP(hipStreamSynchronize(st));
    KH_HIP(T.Add(&T.kernel, 1, 2));
    KH_HIP(T.Add(&T.down, 2, 3));
    for (size_t i = c.begin; i < c.end; i++) {
      const BpLat &L = sorted[i];
      for (int64_t p = 0; p < P; p++) {
        const int64_t o = static_cast<int64_t>(L.lat) * P + p, r = static_cast<int64_t>(i - c.begin) * P + p;
        const int32_t n = h_len[r];
        path_len[o] = n;
        path_final_state[o] = h_final[r];
        tot_graph[o] = h_tg[r];
        tot_acoustic[o] = h_ta[r];
        if (n <= 0) continue;
        if (n > path_offsets[o + 1] - path_offsets[o]) {
          SetError("kh_compact_lattice_best_paths: lattice %d, point %d: the path has %d arcs, path_offsets leaves room for %lld",
                   L.lat, static_cast<int>(p), n, static_cast<long long>(path_offsets[o + 1] - path_offsets[o]));
          return KH_EINVAL;
        }
        int32_t *dst = path_arcs + path_offsets[o];
        const int32_t *src = h_path.data() + L.path_row * P + p;
        for (int32_t k = 0; k < n; k++) dst[k] = src[static_cast<int64_t>(k) * P];
      }
    }
  }
  KH_HIP(T.Mark(2, st));
  int32_t h_err = 0;
  KH_HIP(hipMemcpyAsync(&h_err, d_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KH_HIP(T.Mark(3, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.Add(&T.down, 2, 3));
  if (h_err != 0) {
    SetError("kh_compact_lattice_best_paths: a path left the rows of its lattice (internal error)");
    return KH_ESTATE;
  }
  T.Finish(g_stats.ms);
  g_stats.counts[0] = static_cast<int32_t>(plan.ranges.size());
  return KH_OK;
}
