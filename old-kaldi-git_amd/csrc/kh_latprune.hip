// kh_latprune.hip — PruneLattice<CompactLattice> (lat/lattice-functions.cc:186-265) for a batch of top-sorted
// CompactLattices and K "score points" at once: what `lattice-scale | lattice-add-penalty | lattice-prune --beam=B` computes
// once per point of the scoring grid (egs/tedlium/s5/local/score_sclite.sh and its relatives).  The score point is the one
// of kh_latbest.hip; both take it from kh_scorepoint.h.
//
// Shape: one wave per (lattice, group of 64 points), lane = point.  The arc records are wave-uniform, the per-state row
// cost[state][point] is contiguous across lanes, and every lane executes the reference's statements in the reference's
// order - the sweeps only take minima, but the three comparisons (:242, :254, :256) are written as the reference writes
// them, in its association, because `p + (a + b)` and `(p + a) + b` differ by an ulp often enough to flip an arc.
//   sweep 1  forward costs :211-229 in "pull" form over the incoming arcs of a state kept in (source state, arc position)
//            order: the order in which :221 is offered its candidates, one store per state;
//   sweep 2  backward costs and the prune decisions :239-262 in reverse state order; the costs share the forward costs'
//            memory as in the reference (:238).  One __ballot turns a decision of 64 lanes into the 64-bit mask word of
//            the arc; the co-reachability masks of fst::Connect (:263) fall out of the same loop:
//            co[s] = final_keep[s] | OR over the arcs (keep[a] & co[next]);
//   sweep 3  reachability from the start state over the kept arcs, forward over the incoming lists; wave-uniform 64-bit
//            words, no ballots.
// Mask words are written by lane 0 with ordinary vector stores and read back by the whole wave (wavefront-scope
// release / acquire).  A second, data-parallel kernel then forms arc_keep = keep & reach[src] & co[dst] and
// state_keep = reach & co for the whole batch.
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
constexpr int kFinishThreads = 256;

struct PrLat {
  int64_t state_base;  // first state of the lattice in the batch's state arrays
  int64_t arc_base;    // first arc of the lattice in the caller's arc order
  int64_t ws_row;      // first row of the lattice in the cost workspace, rows of 64 x n_words doubles
  int32_t n_states;
  int32_t start;       // lat->Start() :201
  int32_t lat;         // index in the caller's batch
  int32_t pad;
};

// a mask word written by lane 0 and read by every lane of the same wave later in program order
__device__ __forceinline__ void PutWord(uint64_t *p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t GetWord(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__global__ __launch_bounds__(kLanes) void PruneKernel(
    const PrLat *__restrict__ lats, const int64_t *__restrict__ in_off, const int32_t *__restrict__ in_src,
    const int32_t *__restrict__ in_arc, const int32_t *__restrict__ in_label, const float *__restrict__ in_g,
    const float *__restrict__ in_a, const int64_t *__restrict__ arc_off, const int32_t *__restrict__ arc_label,
    const int32_t *__restrict__ arc_next, const float *__restrict__ arc_g, const float *__restrict__ arc_a,
    const float *__restrict__ fin_g, const float *__restrict__ fin_a, const double *__restrict__ scales,
    const float *__restrict__ penalties, const float *__restrict__ beams, int n_points, int n_words, double *cost,
    uint64_t *keep, uint64_t *co, uint64_t *reach, uint64_t *final_keep, double *best_final_cost) {
  const PrLat L = lats[blockIdx.x];
  const int w = blockIdx.y, lane = threadIdx.x;
  // the lanes past the last point repeat the last point in a column of their own and are masked out of every word
  const bool valid = w * kLanes + lane < n_points;
  const int p = valid ? w * kLanes + lane : n_points - 1;
  const uint64_t live = __ballot(valid);
  const Point pt = LoadPoint(scales, penalties, p);
  const int64_t PP = static_cast<int64_t>(n_words) * kLanes, W = n_words;
  double *c = cost + L.ws_row * PP + w * kLanes + lane;
  const int64_t *io = in_off + L.state_base, *ao = arc_off + L.state_base;
  const float *fg = fin_g + L.state_base, *fa = fin_a + L.state_base;
  uint64_t *keep_w = keep + L.arc_base * W + w;
  uint64_t *co_w = co + L.state_base * W + w, *reach_w = reach + L.state_base * W + w, *fk_w = final_keep + L.state_base * W + w;
  const double inf = std::numeric_limits<double>::infinity();

  // sweep 1, :204-229
  double best_final = inf;                                   // :208
  for (int32_t s = 0; s < L.n_states; s++) {
    double fwd = s == L.start ? 0.0 : inf;                   // :204-206
    const int64_t k1 = io[s + 1];
    for (int64_t k = io[s]; k < k1; k++) {
      float g2, a2;
      ArcWeight(in_g[k], in_a[k], in_label[k], pt, &g2, &a2);
      const double next_forward_cost = c[in_src[k] * PP] + Cost(g2, a2);   // :219-220
      if (fwd > next_forward_cost) fwd = next_forward_cost;               // :221-222
    }
    c[s * PP] = fwd;
    float g2, a2;
    ScaleWeight(fg[s], fa[s], pt, &g2, &a2);
    const double this_final_cost = fwd + Cost(g2, a2);       // :225-226
    if (this_final_cost < best_final) best_final = this_final_cost;       // :227-228
  }
  if (valid) best_final_cost[static_cast<int64_t>(L.lat) * n_points + p] = best_final;
  const double cutoff = best_final + static_cast<double>(beams[p]);       // :231

  // sweep 2, :239-262
  for (int32_t s = L.n_states - 1; s >= 0; s--) {
    const double this_forward_cost = c[s * PP];              // :240
    float g2, a2;
    ScaleWeight(fg[s], fa[s], pt, &g2, &a2);
    double this_backward_cost = Cost(g2, a2);                // :241
    bool is_final = !(g2 == INFINITY && a2 == INFINITY);     // Final(state) != Weight::Zero(), what Connect asks
    if (this_backward_cost + this_forward_cost > cutoff && this_backward_cost != inf) is_final = false;   // :242-244
    const uint64_t fk = __ballot(is_final) & live;
    uint64_t co_s = fk;
    const int64_t j1 = ao[s + 1];
    for (int64_t j = ao[s]; j < j1; j++) {
      const int32_t nx = arc_next[j];
      ArcWeight(arc_g[j], arc_a[j], arc_label[j], pt, &g2, &a2);
      const double arc_cost = Cost(g2, a2);                                // :251
      const double arc_backward_cost = arc_cost + c[nx * PP];              // :252
      const double this_fb_cost = this_forward_cost + arc_backward_cost;   // :253
      if (arc_backward_cost < this_backward_cost) this_backward_cost = arc_backward_cost;   // :254-255
      const uint64_t k = __ballot(!(this_fb_cost > cutoff)) & live;        // :256: the arcs that keep their nextstate
      co_s |= k & GetWord(co_w + nx * W);
      if (lane == 0) PutWord(keep_w + (j - L.arc_base) * W, k);
    }
    c[s * PP] = this_backward_cost;                          // :261
    if (lane == 0) {
      fk_w[s * W] = fk;
      PutWord(co_w + s * W, co_s);
    }
  }

  // sweep 3: the states fst::Connect (:263) finds accessible from the start state
  for (int32_t s = 0; s < L.n_states; s++) {
    uint64_t r = s == L.start ? live : 0;
    const int64_t k1 = io[s + 1];
    for (int64_t k = io[s]; k < k1; k++) r |= GetWord(keep_w + in_arc[k] * W) & GetWord(reach_w + in_src[k] * W);
    if (lane == 0) PutWord(reach_w + s * W, r);
  }
}

// Connect's result: a state survives when it is accessible and coaccessible, an arc when it kept its nextstate and both
// its ends survive.  One block per lattice, a thread per (state, mask word).
__global__ __launch_bounds__(kFinishThreads) void PruneFinishKernel(
    const PrLat *__restrict__ lats, const int64_t *__restrict__ arc_off, const int32_t *__restrict__ arc_next, int n_words,
    const uint64_t *__restrict__ co, const uint64_t *__restrict__ reach, uint64_t *arc_keep, uint64_t *state_keep) {
  const PrLat L = lats[blockIdx.x];
  const int64_t W = n_words, n = static_cast<int64_t>(L.n_states) * W;
  for (int64_t i = threadIdx.x; i < n; i += kFinishThreads) {
    const int64_t s = i / W, w = i % W;
    const uint64_t r = reach[(L.state_base + s) * W + w];
    state_keep[(L.state_base + s) * W + w] = r & co[(L.state_base + s) * W + w];
    const int64_t j1 = arc_off[L.state_base + s + 1];
    for (int64_t j = arc_off[L.state_base + s]; j < j1; j++)
      arc_keep[j * W + w] = arc_keep[j * W + w] & r & co[(L.state_base + arc_next[j]) * W + w];
  }
}

thread_local CallStats<5, 1> g_stats;   // counts: PruneKernel launches of the last call

// NaN and -inf make a min sweep depend on the order of its candidates
inline bool BadWeight(float x) { return std::isnan(x) || x == -std::numeric_limits<float>::infinity(); }

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" int kh_compact_lattice_prune_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_compact_lattice_prune_last_timings(float *ms5, int32_t *n_launches) {
  return GetTimings(g_stats, ms5, n_launches);
}

extern "C" int kh_compact_lattice_prune(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                                        const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                                        const float *arc_graph, const float *arc_acoustic, const float *final_graph,
                                        const float *final_acoustic, int n_points, const double *scales, const float *penalties,
                                        const float *beams, uint64_t *arc_keep, uint64_t *state_keep, uint64_t *final_keep,
                                        double *best_final_cost) {
  int rc = EnsureDevice();
  if (rc) return rc;
  if (n_points < 1) {
    SetError("kh_compact_lattice_prune: n_points = %d: at least one score point is needed", n_points);
    return KH_EINVAL;
  }
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && lat_start && arc_offsets && arc_label && arc_nextstate && arc_graph &&
               arc_acoustic && final_graph && final_acoustic && scales && penalties && beams && arc_keep && state_keep &&
               final_keep && best_final_cost);
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0);
  for (int l = 0; l < n_lats; l++) KH_CHECK_ARG(lat_state_offsets[l + 1] - lat_state_offsets[l] > 0);
  CallTimer T;
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  KH_CHECK_ARG(A >= 0 && A < (1ll << 31));   // (arc positions within a lattice are kept as int32 in the incoming lists)
  const int64_t P = n_points, W = (P + kLanes - 1) / kLanes;
  for (int p = 0; p < n_points; p++) {
    if (!(beams[p] > 0.0f)) {                // KALDI_ASSERT(beam > 0.0) :192
      SetError("kh_compact_lattice_prune: point %d: beam %g: beam > 0.0", p, static_cast<double>(beams[p]));
      return KH_EINVAL;
    }
  }

  // validation (:193, :218: every arc goes to a higher-numbered state of its own lattice; the weights) and the incoming
  // lists: a counting sort by destination, which keeps the arcs of one destination in (source state, arc position) order.
  // This walk and the planner below are BuildIncoming and PlanChunks of kh_latbatch_host.h written out: a call here prepares
  // 64 small lattices in 8 us, and through the shared walker's hooks it measured about 1 us slower
  // (profiles/latbatch_refactor_ab.json).  A change to either belongs in both.
  std::vector<int64_t> in_off(S + 1, 0);
  std::vector<PrLat> lats(n_lats);
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
    if (lat_start[l] < 0 || lat_start[l] >= ns) {
      SetError("kh_compact_lattice_prune: lattice %d: start state %d of %d states", l, lat_start[l], ns);
      return KH_EINVAL;
    }
    for (int32_t s = 0; s < ns; s++) {
      KH_CHECK_ARG(arc_offsets[s0 + s + 1] >= arc_offsets[s0 + s]);
      if (BadWeight(final_graph[s0 + s]) || BadWeight(final_acoustic[s0 + s])) {
        SetError("kh_compact_lattice_prune: lattice %d: state %d: final weight (%g, %g): NaN and -inf are not taken", l, s,
                 static_cast<double>(final_graph[s0 + s]), static_cast<double>(final_acoustic[s0 + s]));
        return KH_EINVAL;
      }
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        const int32_t nx = arc_nextstate[j];
        if (nx <= s || nx >= ns) {
          SetError("kh_compact_lattice_prune: lattice %d: arc %lld (state %d -> %d of %d): input lattice must be "
                   "topologically sorted", l, static_cast<long long>(j - arc_offsets[s0]), s, nx, ns);
          return KH_EINVAL;
        }
        if (BadWeight(arc_graph[j]) || BadWeight(arc_acoustic[j])) {
          SetError("kh_compact_lattice_prune: lattice %d: arc %lld (state %d -> %d): weight (%g, %g): NaN and -inf are not "
                   "taken", l, static_cast<long long>(j - arc_offsets[s0]), s, nx, static_cast<double>(arc_graph[j]),
                   static_cast<double>(arc_acoustic[j]));
          return KH_EINVAL;
        }
        in_off[s0 + nx + 1]++;
      }
    }
  }
  for (int64_t s = 0; s < S; s++) in_off[s + 1] += in_off[s];
  std::vector<int32_t> in_src(A), in_arc(A), in_label(A);
  std::vector<float> in_g(A), in_a(A);
  {
    std::vector<int64_t> fill(in_off.begin(), in_off.end() - 1);
    for (int l = 0; l < n_lats; l++) {
      const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
      const int64_t a0 = arc_offsets[s0];
      for (int32_t s = 0; s < ns; s++) {
        for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
          const int64_t k = fill[s0 + arc_nextstate[j]]++;
          in_src[k] = s;
          in_arc[k] = static_cast<int32_t>(j - a0);
          in_label[k] = arc_label[j];
          in_g[k] = arc_graph[j];
          in_a[k] = arc_acoustic[j];
        }
      }
      PrLat &L = lats[l];
      L.state_base = s0;
      L.arc_base = a0;
      L.ws_row = 0;
      L.n_states = ns;
      L.start = lat_start[l];
      L.lat = l;
      L.pad = 0;
    }
  }
  // the lattices in flight: longest first, as many as the workspace limit admits per launch (at least one)
  std::vector<int32_t> order(n_lats);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return lats[x].n_states > lats[y].n_states; });
  const size_t row_bytes = sizeof(double) * kLanes * static_cast<size_t>(W);
  size_t limit = g_stats.workspace_limit;
  if (limit == 0 && (rc = DefaultWorkspaceLimit(static_cast<size_t>(A) * (36 + 8 * W) + static_cast<size_t>(S) * (24 + 32 * W),
                                                &limit)) != KH_OK)
    return rc;
  struct Chunk { int32_t begin, end; int64_t ws_rows; };
  std::vector<Chunk> chunks;
  std::vector<PrLat> sorted(n_lats);
  int64_t max_ws_rows = 0;
  for (int32_t i = 0; i < n_lats;) {
    Chunk c{i, i, 0};
    size_t bytes = 0;
    while (c.end < n_lats && c.end - c.begin < 65535) {
      PrLat L = lats[order[c.end]];
      const size_t b = static_cast<size_t>(L.n_states) * row_bytes;
      if (c.end > c.begin && bytes + b > limit) break;
      bytes += b;
      L.ws_row = c.ws_rows;
      c.ws_rows += L.n_states;
      sorted[c.end++] = L;
    }
    max_ws_rows = std::max(max_ws_rows, c.ws_rows);
    chunks.push_back(c);
    i = c.end;
  }
  T.HostDone();

  hipStream_t st = Stream();
  KH_HIP(T.Init());
  Dev<PrLat> d_lats;
  Dev<int64_t> d_in_off, d_arc_off;
  Dev<int32_t> d_in_src, d_in_arc, d_in_label, d_label, d_next;
  Dev<float> d_in_g, d_in_a, d_g, d_a, d_fin_g, d_fin_a, d_pen, d_beam;
  Dev<double> d_scales, d_cost, d_best;
  Dev<uint64_t> d_keep, d_co, d_reach, d_fk, d_sk;
  const size_t AW = static_cast<size_t>(A) * W, SW = static_cast<size_t>(S) * W, LP = static_cast<size_t>(n_lats) * P;
  if (d_lats.Alloc(n_lats) || d_in_off.Alloc(S + 1) || d_arc_off.Alloc(S + 1) || d_in_src.Alloc(A) || d_in_arc.Alloc(A) ||
      d_in_label.Alloc(A) || d_label.Alloc(A) || d_next.Alloc(A) || d_in_g.Alloc(A) || d_in_a.Alloc(A) || d_g.Alloc(A) ||
      d_a.Alloc(A) || d_fin_g.Alloc(S) || d_fin_a.Alloc(S) || d_pen.Alloc(P) || d_beam.Alloc(P) || d_scales.Alloc(4 * P) ||
      d_best.Alloc(LP) || d_keep.Alloc(AW) || d_co.Alloc(SW) || d_reach.Alloc(SW) || d_fk.Alloc(SW) || d_sk.Alloc(SW) ||
      d_cost.Alloc(static_cast<size_t>(max_ws_rows) * kLanes * W)) {
    SetError("kh_compact_lattice_prune: out of device memory (workspace of %lld rows x %lld points)",
             static_cast<long long>(max_ws_rows), static_cast<long long>(kLanes * W));
    return KH_ENOMEM;
  }
  KH_HIP(T.Mark(0, st));
  KH_HIP(Up(d_lats, sorted.data(), n_lats, st));
  KH_HIP(Up(d_in_off, in_off.data(), S + 1, st));
  KH_HIP(Up(d_arc_off, arc_offsets, S + 1, st));
  KH_HIP(Up(d_in_src, in_src.data(), A, st));
  KH_HIP(Up(d_in_arc, in_arc.data(), A, st));
  KH_HIP(Up(d_in_label, in_label.data(), A, st));
  KH_HIP(Up(d_in_g, in_g.data(), A, st));
  KH_HIP(Up(d_in_a, in_a.data(), A, st));
  KH_HIP(Up(d_label, arc_label, A, st));
  KH_HIP(Up(d_next, arc_nextstate, A, st));
  KH_HIP(Up(d_g, arc_graph, A, st));
  KH_HIP(Up(d_a, arc_acoustic, A, st));
  KH_HIP(Up(d_fin_g, final_graph, S, st));
  KH_HIP(Up(d_fin_a, final_acoustic, S, st));
  KH_HIP(Up(d_scales, scales, 4 * P, st));
  KH_HIP(Up(d_pen, penalties, P, st));
  KH_HIP(Up(d_beam, beams, P, st));
  KH_HIP(T.Mark(1, st));
  for (const Chunk &c : chunks) {
    hipLaunchKernelGGL(PruneKernel, dim3(c.end - c.begin, static_cast<unsigned>(W)), dim3(kLanes), 0, st, d_lats.p + c.begin,
                       d_in_off.p, d_in_src.p, d_in_arc.p, d_in_label.p, d_in_g.p, d_in_a.p, d_arc_off.p, d_label.p, d_next.p,
                       d_g.p, d_a.p, d_fin_g.p, d_fin_a.p, d_scales.p, d_pen.p, d_beam.p, n_points, static_cast<int>(W),
                       d_cost.p, d_keep.p, d_co.p, d_reach.p, d_fk.p, d_best.p);
    KH_LAUNCH_CHECK();
    hipLaunchKernelGGL(PruneFinishKernel, dim3(c.end - c.begin), dim3(kFinishThreads), 0, st, d_lats.p + c.begin, d_arc_off.p,
                       d_next.p, static_cast<int>(W), d_co.p, d_reach.p, d_keep.p, d_sk.p);
    KH_LAUNCH_CHECK();
  }
  KH_HIP(T.Mark(2, st));
  if (A > 0) KH_HIP(hipMemcpyAsync(arc_keep, d_keep.p, sizeof(uint64_t) * AW, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(state_keep, d_sk.p, sizeof(uint64_t) * SW, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(final_keep, d_fk.p, sizeof(uint64_t) * SW, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(best_final_cost, d_best.p, sizeof(double) * LP, hipMemcpyDeviceToHost, st));
  KH_HIP(T.Mark(3, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.AddAll());
  T.Finish(g_stats.ms);
  g_stats.counts[0] = static_cast<int32_t>(chunks.size());
  return KH_OK;
}
