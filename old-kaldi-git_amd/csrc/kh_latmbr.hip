// kh_latmbr.hip — MinimumBayesRisk (lat/sausages.{h,cc}: the class behind lattice-mbr-decode and lattice-to-ctm-conf) for a
// batch of top-sorted CompactLattices and K score points at once.  The lattices arrive in the class's own form
// (PrepareLatticeAndInitStats :268-315): start state 0, the last state the single final state with weight One.
//
// What is computed where.  AccStats (:133-266) needs per arc the double exp(alpha(s_a) + p_a - alpha(n)) (:125, :185, :213) and
// per state the LogAdd of :105.  A device exp or log does not give glibc's bits, and the three-way choice b_arc (:174-180)
// turns a last-bit difference into a different sausage, so the transcendentals are taken on the HOST, once per (lattice,
// point) - they do not depend on the hypothesis R_: alpha(n) with the reference's double LogAdd (base/kaldi-math.h:178-195)
// in pre_[n] order, then w_a = exp(alpha(s_a) + p_a - alpha(n)) in that association.  The kernel receives w_a and does
// nothing but double +, *, comparisons and integer work, in the reference's order (-ffp-contract=off: no fused
// multiply-add), so its results are the reference's statements' bits; no tolerance is involved.
//
// The one deliberate difference: a state other than the start with alpha = -inf (no arc with a finite weight reaches it)
// makes :125 compute exp(NaN); such a lattice is refused.
//
// MbrAccStatsKernel: one AccStats() per launch, one wave per (lattice, point) still iterating, lane = q in 0..Q, chunks of
// 64, Q = |R_| after NormalizeEps.  Rows of alpha_dash and beta_dash, N x (Q + 1) doubles each, stay in a device workspace;
// column q of every row is read and written by lane q % 64 alone, except alpha_dash's column in front of a chunk (the a1
// term of lane 0), which is why a wavefront fence follows each state of the forward sweep.
//   forward (EditDistance :97-129): states in number order, a state's arcs in pre_[n] order = ascending (source state, arc
//   position), the incoming-list order of the sibling kernels.  a1 takes the source row shifted by one lane.  The a3 term
//   is a serial chain c(q) = min(min(a1, a2)(q), c(q-1) + l(0, r_q)); a prefix scan would re-associate the sums, so the
//   wave relaxes c = min(c, shfl_up(c) + l_q) until a ballot shows no lane changed: every step evaluates the reference's
//   own expression on a value that only decreases towards the sequential one, and double + is monotone, so the fixed
//   point is the sequential result (lane 0 of a chunk takes the last column of the chunk before, carried in a register).
//   backward (:162-226): b_arc is recomputed per arc as :168-181 does and kept in a row of int32 (lane-private); then from
//   the top chunk down beta_dash_arc(q) = carry + w_a * beta_dash(n, q), the carry coming from lane q + 1 where
//   b_arc[q + 1] == 3 - runs of 3 resolve one lane per step from their top, again until a ballot shows no change.  The two
//   updates one arc can make to beta_dash(s_a, q) are applied in the reference's order: case 1 of q + 1 (by shuffle), then
//   case 2 of q (or :214 for q = 0).  gamma, tau_b, tau_e are lane-private accumulators in memory, added arc after arc.
//   gamma is a dense V x (Q + 1) double matrix, V = the lattice's distinct arc labels plus 0, zero = absent (every addend
//   is >= 0, and AddToMap skips d == 0).
// The host loop (MbrDecode :27-69) normalizes R_, launches over the pairs still iterating, casts gamma to float, sorts with
// GammaCompare, updates R_, and stops a pair when delta_Q == 0 or counter > 100.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <limits>
#include <numeric>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"
#include "kh_scorepoint.h"

namespace kh {
namespace {

constexpr int kLanes = 64;

struct MbrJob {
  int64_t state_base;  // first state of the lattice in the batch's state arrays
  int64_t w_off;       // first w_a of the (lattice, point) pair: indexed by incoming-list position of the whole batch
  int64_t ws_off;      // first double of the pair's workspace: alpha_dash, beta_dash [N x (Q + 1)], b_arc [(Q + 1) int32]
  int64_t out_off;     // first double of the pair's results: gamma [V x (Q + 1)], tau_b, tau_e [Q + 1], L
  int64_t r_off;       // first word of the pair's normalized hypothesis
  int32_t n_states;
  int32_t Q;
  int32_t V;
  int32_t pad;
};

// :113-123 / :168-181 for one arc and the 64 positions from c0: returns alpha_dash_arc(q) and b_arc[q]; *carry is
// alpha_dash_arc(c0 - 1) on entry and alpha_dash_arc(c0 + 63) on return.
__device__ __forceinline__ double ArcChunk(const double *__restrict__ src, int c0, int lane, int Q, int32_t w_a, int32_t r_q,
                                           double delta, double *carry, int *b_arc) {
  const int q = c0 + lane;
  const bool active = q <= Q, dp = active && q >= 1;
  const double a = active ? src[q] : 0.0;
  double d = __shfl_up(a, 1);
  if (lane == 0) d = c0 > 0 ? src[c0 - 1] : 0.0;
  const double a1 = d + (w_a == r_q ? 0.0 : 1.0);            // alpha_dash(s_a, q-1) + l(w_a, r_q)
  const double a2 = a + (w_a == 0 ? 0.0 : 1.0) + delta;      // alpha_dash(s_a, q) + l(w_a, 0) + delta()
  const double l_q = r_q == 0 ? 0.0 : 1.0;                   // l(0, r_q)
  double c = dp ? (a1 <= a2 ? a1 : a2) : a2;                 // q == 0: :115-116
  for (;;) {
    double prev = __shfl_up(c, 1);
    if (lane == 0) prev = *carry;
    const double a3 = prev + l_q;
    const bool less = dp && a3 < c;
    if (less) c = a3;
    if (__ballot(less) == 0) break;
  }
  double prev = __shfl_up(c, 1);
  if (lane == 0) prev = *carry;
  const double a3 = prev + l_q;
  *b_arc = a1 <= a2 ? (a1 <= a3 ? 1 : 3) : (a2 <= a3 ? 2 : 3);   // :174-180
  *carry = __shfl(c, kLanes - 1);
  return c;
}

__global__ __launch_bounds__(kLanes) void MbrAccStatsKernel(
    const MbrJob *__restrict__ jobs, const int64_t *__restrict__ in_off, const int32_t *__restrict__ in_src,
    const int32_t *__restrict__ in_label, const int32_t *__restrict__ in_v, const double *__restrict__ w,
    const int32_t *__restrict__ state_times, const int32_t *__restrict__ rw, double *ws, double *out) {
  const MbrJob J = jobs[blockIdx.x];
  const int lane = threadIdx.x, Q = J.Q, N = J.n_states;
  const int64_t QS = static_cast<int64_t>(Q) + 1;
  double *ad = ws + J.ws_off, *bd = ad + N * QS;
  int32_t *barc = reinterpret_cast<int32_t *>(bd + N * QS);
  double *gm = out + J.out_off, *tb = gm + J.V * QS, *te = tb + QS, *L_out = te + QS;
  const int32_t *r = rw + J.r_off;                           // r(q) = r[q - 1]
  const int64_t *io = in_off + J.state_base;
  const int32_t *st = state_times + J.state_base;
  const double *wa = w + J.w_off;
  const double delta = static_cast<double>(1.0e-05f);        // sausages.h:132: a BaseFloat, promoted where it is used
  const int last_c0 = (Q / kLanes) * kLanes;

  // :98-100: alpha_dash(1, q) = alpha_dash(1, q-1) + l(0, r(q)) - sums of 0.0 and 1.0 from 0.0 are exact integers, so the
  // count of words up to q is that sum's value
  {
    int before = 0;
    for (int c0 = 0; c0 <= Q; c0 += kLanes) {
      const int q = c0 + lane;
      const bool active = q <= Q;
      const unsigned long long m = __ballot(active && q >= 1 && r[q - 1] != 0);
      if (active) ad[q] = static_cast<double>(before + __popcll(m & ((2ull << lane) - 1ull)));
      before += __popcll(m);
    }
  }
  WaveFence();
  for (int32_t s = 1; s < N; s++) {                          // :101, n = s + 1
    const int64_t k1 = io[s + 1];
    for (int64_t k = io[s]; k < k1; k++) {                   // :109
      const double *src = ad + in_src[k] * QS;
      const int32_t w_a = in_label[k];
      const double wk = wa[k];
      double carry = 0.0;
      for (int c0 = 0; c0 <= Q; c0 += kLanes) {              // :113
        const int q = c0 + lane;
        const bool active = q <= Q;
        const int32_t r_q = active && q >= 1 ? r[q - 1] : 0;
        int b;
        const double c = ArcChunk(src, c0, lane, Q, w_a, r_q, delta, &carry, &b);
        if (active) ad[s * QS + q] = ad[s * QS + q] + wk * c;   // :125
      }
    }
    WaveFence();
  }
  if (lane == 0) *L_out = ad[(N - 1) * QS + Q];               // :129

  if (lane == Q % kLanes) bd[(N - 1) * QS + Q] = 1.0;         // :162 (the lane that owns column Q)
  for (int32_t s = N - 1; s >= 1; s--) {                     // :163
    const double t_n = static_cast<double>(st[s]);
    const int64_t k1 = io[s + 1];
    for (int64_t k = io[s]; k < k1; k++) {                   // :164
      const int32_t s_a = in_src[k], w_a = in_label[k];
      const double *src = ad + s_a * QS;
      double *gw = gm + in_v[k] * QS;
      const double wk = wa[k], t_sa = static_cast<double>(st[s_a]);
      double carry = 0.0;
      for (int c0 = 0; c0 <= Q; c0 += kLanes) {              // :168-181
        const int q = c0 + lane;
        const bool active = q <= Q;
        const int32_t r_q = active && q >= 1 ? r[q - 1] : 0;
        int b;
        (void)ArcChunk(src, c0, lane, Q, w_a, r_q, delta, &carry, &b);
        if (active) barc[q] = q >= 1 ? b : 0;
      }
      int top_b = 0;
      double top_x = 0.0;
      for (int c0 = last_c0; c0 >= 0; c0 -= kLanes) {        // :183-214
        const int q = c0 + lane;
        const bool active = q <= Q;
        const int b = active ? barc[q] : 0;
        const double t = active ? wk * bd[s * QS + q] : 0.0; // :185, :213
        int b_up = __shfl_down(b, 1);
        if (lane == kLanes - 1) b_up = top_b;
        const bool chain = b_up == 3;                        // :199 of q + 1 has added beta_dash_arc(q + 1) first
        double x = t;
        for (;;) {
          double up = __shfl_down(x, 1);
          if (lane == kLanes - 1) up = top_x;
          const double nx = chain ? up + t : t;
          const bool changed = nx != x;
          x = nx;
          if (__ballot(changed) == 0) break;
        }
        double up = __shfl_down(x, 1);
        if (lane == kLanes - 1) up = top_x;
        if (active) {
          double cell = bd[s_a * QS + q];
          if (b_up == 1) cell = cell + up;                   // :188 of q + 1
          if (q == 0 || b == 2) cell = cell + x;             // :196, :214
          bd[s_a * QS + q] = cell;
          if (b == 1) {
            if (x != 0) gw[q] = gw[q] + x;                   // :190
            tb[q] = tb[q] + t_sa * x;                        // :192
            te[q] = te[q] + t_n * x;                         // :193
          } else if (b == 3) {
            if (x != 0) gm[q] = gm[q] + x;                   // :201
            tb[q] = tb[q] + t_n * x;                         // :206
            te[q] = te[q] + t_n * x;                         // :207
          }
        }
        top_b = __shfl(b, 0);
        top_x = __shfl(x, 0);
      }
    }
  }
  // :217-226
  {
    const double t_1 = static_cast<double>(st[0]);
    double top_x = 0.0;
    for (int c0 = last_c0; c0 >= 0; c0 -= kLanes) {
      const int q = c0 + lane;
      const bool active = q <= Q, chain = q < Q;
      const double t = active ? bd[q] : 0.0;                 // :219
      double x = t;
      for (;;) {
        double up = __shfl_down(x, 1);
        if (lane == kLanes - 1) up = top_x;
        const double nx = chain ? up + t : t;                // :220 of q + 1, then :219
        const bool changed = nx != x;
        x = nx;
        if (__ballot(changed) == 0) break;
      }
      if (active && q >= 1) {
        if (x != 0) gm[q] = gm[q] + x;                       // :221
        tb[q] = tb[q] + t_1 * x;                             // :224
        te[q] = te[q] + t_1 * x;                             // :225
      }
      top_x = __shfl(x, 0);
    }
  }
}

// base/kaldi-math.h:178-195
inline double LogAddDouble(double x, double y) {
  static const double kMinLogDiffDouble = std::log(DBL_EPSILON);   // base/kaldi-math.h:45
  double diff;
  if (x < y) {
    diff = x - y;
    x = y;
  } else {
    diff = y - x;
  }
  if (diff >= kMinLogDiffDouble) {
    double res;
    res = x + std::log1p(std::exp(diff));
    return res;
  } else {
    return x;
  }
}

struct Pair {                    // one MinimumBayesRisk object
  std::vector<int32_t> R;        // R_
  double L = 0.0;                // L_
  int32_t iterations = 0;
  bool active = true;
  std::vector<int32_t> bin_sizes, stat_words, one_best_words;
  std::vector<float> stat_post, times, one_best_times, one_best_conf;   // gamma_, times_, one_best_times_, one_best_confidences_
};

// sausages.h:196-206
struct GammaCompare {
  bool operator()(const std::pair<int32_t, float> &a, const std::pair<int32_t, float> &b) const {
    if (a.second > b.second) return true;
    else if (a.second < b.second) return false;
    else return a.first > b.first;
  }
};

thread_local CallStats<6, 3> g_stats;   // ms[5]: the host loop; counts: launches, rounds of the host loop, AccStats() calls over all pairs

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" int kh_compact_lattice_mbr_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_compact_lattice_mbr_last_timings(float *ms6, int32_t *counts3) {
  return GetTimings(g_stats, ms6, counts3);
}

extern "C" int kh_compact_lattice_mbr(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                                      const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                                      const float *arc_graph, const float *arc_acoustic, const float *final_graph,
                                      const float *final_acoustic, const int32_t *state_times, int n_points,
                                      const double *scales, const float *penalties, const int64_t *hyp_offsets,
                                      const int32_t *hyp_words, int do_mbr, int32_t *n_words, const int64_t *word_offsets,
                                      int32_t *words, float *one_best_times, float *one_best_confidences, double *bayes_risk,
                                      int32_t *iterations, int32_t *n_bins, const int64_t *bin_offsets, int32_t *bin_sizes,
                                      float *bin_times, int32_t *n_stats, const int64_t *stat_offsets, int32_t *stat_words,
                                      float *stat_post) {
  int rc = EnsureDevice();
  if (rc) return rc;
  if (n_points < 1) {
    SetError("kh_compact_lattice_mbr: n_points = %d: at least one point is needed", n_points);
    return KH_EINVAL;
  }
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && lat_start && arc_offsets && arc_label && arc_nextstate && arc_graph &&
               arc_acoustic && final_graph && final_acoustic && state_times && scales && penalties && hyp_offsets &&
               n_words && word_offsets && words && one_best_times && one_best_confidences && bayes_risk && iterations &&
               n_bins && bin_offsets && bin_sizes && bin_times && n_stats && stat_offsets && stat_words && stat_post);
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0 && hyp_offsets[0] == 0 && word_offsets[0] == 0 &&
               bin_offsets[0] == 0 && stat_offsets[0] == 0);
  for (int l = 0; l < n_lats; l++) KH_CHECK_ARG(lat_state_offsets[l + 1] - lat_state_offsets[l] > 0);
  CallTimer T;
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  KH_CHECK_ARG(A >= 0 && A < (1ll << 31));
  const int64_t P = n_points, LP = static_cast<int64_t>(n_lats) * P;
  for (int64_t o = 0; o < LP; o++) {
    if (hyp_offsets[o + 1] < hyp_offsets[o] || hyp_offsets[o + 1] - hyp_offsets[o] >= (1 << 24)) {
      SetError("kh_compact_lattice_mbr: lattice %d, point %d: hyp_offsets %lld, %lld: the offsets must ascend, by less than 2^24",
               static_cast<int>(o / P), static_cast<int>(o % P), static_cast<long long>(hyp_offsets[o]),
               static_cast<long long>(hyp_offsets[o + 1]));
      return KH_EINVAL;
    }
    KH_CHECK_ARG(word_offsets[o + 1] >= word_offsets[o] && bin_offsets[o + 1] >= bin_offsets[o] && stat_offsets[o + 1] >= stat_offsets[o]);
  }
  KH_CHECK_ARG(hyp_offsets[LP] == 0 || hyp_words);
  const float finf = std::numeric_limits<float>::infinity();
  const double dinf = std::numeric_limits<double>::infinity();

  // validation and the incoming lists, whose order is pre_[n]'s (:297-313); V: 0 and the lattice's distinct labels
  std::vector<int32_t> in_label(A), in_v(A);
  std::vector<int64_t> in_arc(A);                            // (arc numbers of the whole batch)
  std::vector<std::vector<int32_t>> vocab(n_lats);
  std::vector<int32_t> zero_at(n_lats);
  Incoming in;
  std::string err;
  if (!BuildIncoming(
          "kh_compact_lattice_mbr", n_lats, lat_state_offsets, nullptr, arc_offsets, arc_nextstate, &in, &err,
          [&](int l, int32_t, int32_t) {
            if (lat_start[l] == 0) return true;
            return Refuse(&err, "kh_compact_lattice_mbr: lattice %d: start state %d: a top-sorted lattice starts at state 0", l,
                          lat_start[l]);
          },
          [&](int l, int32_t s0, int32_t s) {
            const int32_t ns = lat_state_offsets[l + 1] - s0;
            const float fg = final_graph[s0 + s], fa = final_acoustic[s0 + s];
            const int64_t n_arcs = arc_offsets[s0 + s + 1] - arc_offsets[s0 + s];
            if (s == ns - 1 ? (fg == 0.f && fa == 0.f && n_arcs == 0) : (fg == finf && fa == finf)) return true;
            return Refuse(&err, "kh_compact_lattice_mbr: lattice %d: state %d of %d (final weight %g, %g, %lld arcs): the last state "
                          "must be the single final state, with weight One and no arcs (compact_lattice_mbr_prepare)", l, s, ns,
                          fg, fa, static_cast<long long>(n_arcs));
          },
          [&](int l, int32_t s, int64_t j, int32_t nx) {
            const float g = arc_graph[j], a = arc_acoustic[j];
            if (!(std::isnan(g) || std::isnan(a) || g == -finf || a == -finf)) return true;
            return Refuse(&err, "kh_compact_lattice_mbr: lattice %d: arc %lld (state %d -> %d): weight %g, %g: NaN and -inf are not "
                          "taken", l, static_cast<long long>(j - arc_offsets[lat_state_offsets[l]]), s, nx, g, a);
          },
          [&](int l, int32_t s0, int32_t ns) {
            std::vector<int32_t> &v = vocab[l];
            v.assign(arc_label + arc_offsets[s0], arc_label + arc_offsets[s0 + ns]);
            v.push_back(0);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            zero_at[l] = static_cast<int32_t>(std::lower_bound(v.begin(), v.end(), 0) - v.begin());
            return true;
          },
          [&](int l, int64_t k, int64_t j) {
            const std::vector<int32_t> &ascending = vocab[l];
            const int32_t at = static_cast<int32_t>(std::lower_bound(ascending.begin(), ascending.end(), arc_label[j]) - ascending.begin());
            const int32_t z = zero_at[l];
            in_arc[k] = j;
            in_label[k] = arc_label[j];
            in_v[k] = at == z ? 0 : (at < z ? at + 1 : at);
          })) {
    SetError("%s", err.c_str());
    return KH_EINVAL;
  }
  for (int l = 0; l < n_lats; l++)                           // 0 comes first: column 0 is epsilon's
    std::rotate(vocab[l].begin(), vocab[l].begin() + zero_at[l], vocab[l].begin() + zero_at[l] + 1);
  const std::vector<int64_t> &in_off = in.in_off;
  const std::vector<int32_t> &in_src = in.in_src;
  // per (lattice, point): loglike (:306-307), alpha (:102-107), w_a (:125)
  std::vector<double> w(static_cast<size_t>(A) * P), alpha;
  std::vector<float> ll(A);
  for (int64_t p = 0; p < P; p++) {
    const Point pt = LoadPoint(scales, penalties, static_cast<int>(p));
    for (int l = 0; l < n_lats; l++) {
      const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
      alpha.assign(ns, 0.0);
      for (int32_t s = 1; s < ns; s++) {
        double alpha_n = -dinf;                              // :102
        for (int64_t k = in_off[s0 + s]; k < in_off[s0 + s + 1]; k++) {
          const int64_t j = in_arc[k];
          float g2, a2;
          ArcWeight(arc_graph[j], arc_acoustic[j], in_label[k], pt, &g2, &a2);
          const float loglike = -(g2 + a2);                  // :306-307
          if (std::isnan(loglike) || loglike == finf) {
            SetError("kh_compact_lattice_mbr: lattice %d, point %d: arc %lld: the scaled weight %g, %g: NaN and -inf are not taken",
                     l, static_cast<int>(p), static_cast<long long>(j - arc_offsets[s0]), g2, a2);
            return KH_EINVAL;
          }
          ll[k] = loglike;
          alpha_n = LogAddDouble(alpha_n, alpha[in_src[k]] + loglike);   // :105
        }
        if (alpha_n == -dinf) {
          SetError("kh_compact_lattice_mbr: lattice %d, point %d: state %d: alpha = -inf (no arc with a finite weight reaches it; "
                   "the reference computes NaN here)", l, static_cast<int>(p), s);
          return KH_EINVAL;
        }
        alpha[s] = alpha_n;                                  // :107
        for (int64_t k = in_off[s0 + s]; k < in_off[s0 + s + 1]; k++)
          w[p * A + k] = std::exp(alpha[in_src[k]] + ll[k] - alpha_n);   // :125
      }
    }
  }
  std::vector<Pair> pairs(LP);
  for (int64_t o = 0; o < LP; o++) pairs[o].R.assign(hyp_words + hyp_offsets[o], hyp_words + hyp_offsets[o + 1]);   // :342 / :358
  size_t limit = g_stats.workspace_limit;
  if (limit == 0 && (rc = DefaultWorkspaceLimit(static_cast<size_t>(A) * (12 + 8 * P) + static_cast<size_t>(S) * 12 +
                                                    64 * static_cast<size_t>(LP), &limit)) != KH_OK)
    return rc;
  T.HostDone();

  hipStream_t st = Stream();
  KH_HIP(T.Init());
  Dev<int64_t> d_in_off;
  Dev<int32_t> d_in_src, d_in_label, d_in_v, d_times, d_r;
  Dev<double> d_w, d_ws, d_out;
  Dev<MbrJob> d_jobs;
  if (d_in_off.Alloc(S + 1) || d_in_src.Alloc(A) || d_in_label.Alloc(A) || d_in_v.Alloc(A) || d_times.Alloc(S) ||
      d_w.Alloc(static_cast<size_t>(A) * P) || d_jobs.Alloc(LP)) {
    SetError("kh_compact_lattice_mbr: out of device memory");
    return KH_ENOMEM;
  }
  KH_HIP(T.Mark(0, st));
  KH_HIP(Up(d_in_off, in_off.data(), S + 1, st));
  KH_HIP(Up(d_times, state_times, S, st));
  KH_HIP(Up(d_in_src, in_src.data(), A, st));
  KH_HIP(Up(d_in_label, in_label.data(), A, st));
  KH_HIP(Up(d_in_v, in_v.data(), A, st));
  KH_HIP(Up(d_w, w.data(), static_cast<size_t>(A) * P, st));
  KH_HIP(T.Mark(1, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.Add(&T.up, 0, 1));

  // MbrDecode :27-69 for every pair; the staging vectors are reused between the rounds
  std::vector<MbrJob> jobs;
  std::vector<int64_t> job_pair;
  std::vector<int32_t> rw;
  std::vector<double> h_out;
  std::vector<std::pair<int32_t, float>> bin;
  int32_t n_launches = 0, n_rounds = 0, n_acc = 0;
  float ms_loop = 0.f;
  for (size_t counter = 0;; counter++) {                     // :29
    jobs.clear();
    job_pair.clear();
    rw.clear();
    for (int64_t o = 0; o < LP; o++) {
      Pair &pr = pairs[o];
      if (!pr.active) continue;
      std::vector<int32_t> &R = pr.R;                        // NormalizeEps :82-91
      R.erase(std::remove(R.begin(), R.end(), 0), R.end());
      const size_t nw = R.size();
      R.resize(1 + 2 * nw);
      for (int64_t i = static_cast<int64_t>(nw) - 1; i >= 0; i--) {
        R[2 * i + 1] = R[i];
        R[2 * i + 2] = 0;
      }
      R[0] = 0;
      const int l = static_cast<int>(o / P);
      MbrJob J;
      J.state_base = lat_state_offsets[l];
      J.w_off = (o % P) * A;
      J.ws_off = J.out_off = 0;
      J.r_off = static_cast<int64_t>(rw.size());
      J.n_states = lat_state_offsets[l + 1] - lat_state_offsets[l];
      J.Q = static_cast<int32_t>(R.size());
      J.V = static_cast<int32_t>(vocab[l].size());
      J.pad = 0;
      rw.insert(rw.end(), R.begin(), R.end());
      jobs.push_back(J);
      job_pair.push_back(o);
    }
    if (jobs.empty()) break;
    n_rounds++;
    // the pairs in flight: largest first, as many per launch as the workspace limit admits (at least one)
    auto ws_cells = [](const MbrJob &J) { return 2 * static_cast<size_t>(J.n_states) * (J.Q + 1) + static_cast<size_t>(J.Q + 2) / 2; };
    auto out_cells = [](const MbrJob &J) { return (static_cast<size_t>(J.V) + 2) * (J.Q + 1) + 1; };
    std::vector<size_t> job_bytes(jobs.size());
    for (size_t i = 0; i < jobs.size(); i++) job_bytes[i] = (ws_cells(jobs[i]) + out_cells(jobs[i])) * sizeof(double);
    const ChunkPlan plan = PlanChunks(job_bytes, limit);
    std::vector<MbrJob> sorted(jobs.size());
    std::vector<int64_t> sorted_pair(jobs.size());
    struct Chunk { size_t begin, end, ws, out, out_base; };
    std::vector<Chunk> chunks;
    size_t max_ws = 0, max_out = 0, out_total = 0;
    for (const ChunkRange &r : plan.ranges) {
      Chunk c{r.begin, r.end, 0, 0, out_total};
      for (size_t i = r.begin; i < r.end; i++) {
        MbrJob J = jobs[plan.order[i]];
        J.ws_off = static_cast<int64_t>(c.ws);
        J.out_off = static_cast<int64_t>(c.out);
        c.ws += ws_cells(J);
        c.out += out_cells(J);
        sorted_pair[i] = job_pair[plan.order[i]];
        sorted[i] = J;
      }
      max_ws = std::max(max_ws, c.ws);
      max_out = std::max(max_out, c.out);
      out_total += c.out;
      chunks.push_back(c);
    }
    if (d_ws.Grow(max_ws) || d_out.Grow(max_out) || d_r.Grow(rw.size())) {
      SetError("kh_compact_lattice_mbr: out of device memory (workspace of %lld + %lld doubles)", static_cast<long long>(max_ws),
               static_cast<long long>(max_out));
      return KH_ENOMEM;
    }
    if (h_out.size() < out_total) h_out.resize(out_total);
    KH_HIP(T.Mark(0, st));
    KH_HIP(Up(d_jobs, sorted.data(), sorted.size(), st));
    KH_HIP(Up(d_r, rw.data(), rw.size(), st));
    KH_HIP(T.Mark(1, st));
    KH_HIP(hipStreamSynchronize(st));
    KH_HIP(T.Add(&T.up, 0, 1));
    for (const Chunk &c : chunks) {
      KH_HIP(T.Mark(1, st));
      KH_HIP(hipMemsetAsync(d_ws.p, 0, sizeof(double) * c.ws, st));
      KH_HIP(hipMemsetAsync(d_out.p, 0, sizeof(double) * c.out, st));
      hipLaunchKernelGGL(MbrAccStatsKernel, dim3(static_cast<unsigned>(c.end - c.begin)), dim3(kLanes), 0, st, d_jobs.p + c.begin,
                         d_in_off.p, d_in_src.p, d_in_label.p, d_in_v.p, d_w.p, d_times.p, d_r.p, d_ws.p, d_out.p);
      KH_LAUNCH_CHECK();
      KH_HIP(T.Mark(2, st));
      KH_HIP(hipMemcpyAsync(h_out.data() + c.out_base, d_out.p, sizeof(double) * c.out, hipMemcpyDeviceToHost, st));
      KH_HIP(T.Mark(3, st));
      KH_HIP(hipStreamSynchronize(st));
      KH_HIP(T.Add(&T.kernel, 1, 2));
      KH_HIP(T.Add(&T.down, 2, 3));
      n_launches++;
    }
    const auto t_loop0 = std::chrono::steady_clock::now();
    for (const Chunk &c : chunks) {
      for (size_t i = c.begin; i < c.end; i++) {
        const MbrJob &J = sorted[i];
        Pair &pr = pairs[sorted_pair[i]];
        const std::vector<int32_t> &voc = vocab[sorted_pair[i] / P];
        const int64_t QS = static_cast<int64_t>(J.Q) + 1, Q = J.Q;
        const double *gm = h_out.data() + c.out_base + J.out_off, *tau_b = gm + J.V * QS, *tau_e = tau_b + QS;
        pr.L = tau_e[QS];                                    // :159
        pr.iterations++;
        n_acc++;
        pr.bin_sizes.assign(Q, 0);                           // :237-246
        pr.stat_words.clear();
        pr.stat_post.clear();
        pr.times.assign(2 * Q, 0.f);                         // :250-265
        pr.one_best_words.clear();                           // :34-35
        pr.one_best_times.clear();
        pr.one_best_conf.clear();
        double delta_Q = 0.0;                                // :32
        for (int64_t q = 1; q <= Q; q++) {
          bin.clear();
          for (int32_t v = 0; v < J.V; v++)
            if (gm[v * QS + q] != 0) bin.emplace_back(voc[v], static_cast<float>(gm[v * QS + q]));   // :242
          std::sort(bin.begin(), bin.end(), GammaCompare()); // :245
          pr.bin_sizes[q - 1] = static_cast<int32_t>(bin.size());
          for (const auto &e : bin) {
            pr.stat_words.push_back(e.first);
            pr.stat_post.push_back(e.second);
          }
          float *times = pr.times.data();
          times[2 * (q - 1)] = static_cast<float>(tau_b[q]);           // :253
          times[2 * (q - 1) + 1] = static_cast<float>(tau_e[q]);       // :254
          if (q > 1 && times[2 * (q - 2) + 1] > times[2 * (q - 1)]) {  // :257
            const double avg = 0.5 * (times[2 * (q - 2) + 1] + times[2 * (q - 1)]);   // :262 (a BaseFloat sum)
            times[2 * (q - 2) + 1] = times[2 * (q - 1)] = static_cast<float>(avg);   // :263
          }
          if (do_mbr && bin.empty()) {
            SetError("kh_compact_lattice_mbr: lattice %d, point %d: bin %lld has no statistics (the reference reads past an empty vector here)",
                     static_cast<int>(sorted_pair[i] / P), static_cast<int>(sorted_pair[i] % P), static_cast<long long>(q - 1));
            return KH_EINVAL;
          }
          if (do_mbr) {                                      // :40-52
            double old_gamma = 0, new_gamma = bin[0].second; // :43
            const int32_t rq = pr.R[q - 1], rhat = bin[0].first;       // :44
            for (size_t j = 0; j < bin.size(); j++)
              if (bin[j].first == rq) old_gamma = bin[j].second;       // :45-46
            delta_Q += (old_gamma - new_gamma);              // :47
            pr.R[q - 1] = rhat;                              // :51
          }
        }
        // :53-59 read times_ after the averaging of the NEXT bin has been applied to this one, as the reference does
        // (AccStats has finished before the loop of :39 runs)
        size_t at = 0;
        for (int64_t q = 1; q <= Q; q++) {
          const int32_t n_here = pr.bin_sizes[q - 1];
          if (pr.R[q - 1] != 0) {                            // :53
            pr.one_best_times.push_back(pr.times[2 * (q - 1)]);        // :54
            pr.one_best_times.push_back(pr.times[2 * (q - 1) + 1]);
            float confidence = 0.0;                          // :55
            for (int32_t j = 0; j < n_here; j++)
              if (pr.stat_words[at + j] == pr.R[q - 1]) confidence = pr.stat_post[at + j];   // :56-57
            pr.one_best_conf.push_back(confidence);          // :58
          }
          at += n_here;
        }
        if (delta_Q == 0 || counter > 100) pr.active = false;   // :62-66
      }
    }
    ms_loop += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_loop0).count();
  }
  // the outputs, where they fit
  bool fits = true;
  int64_t bad = -1;
  for (int64_t o = 0; o < LP; o++) {
    Pair &pr = pairs[o];
    pr.R.erase(std::remove(pr.R.begin(), pr.R.end(), 0), pr.R.end());   // :68
    n_words[o] = static_cast<int32_t>(pr.R.size());
    n_bins[o] = static_cast<int32_t>(pr.bin_sizes.size());
    n_stats[o] = static_cast<int32_t>(pr.stat_words.size());
    bayes_risk[o] = pr.L;
    iterations[o] = pr.iterations;
    if (n_words[o] > word_offsets[o + 1] - word_offsets[o] || n_bins[o] > bin_offsets[o + 1] - bin_offsets[o] ||
        n_stats[o] > stat_offsets[o + 1] - stat_offsets[o]) {
      if (fits) bad = o;
      fits = false;
    }
  }
  if (fits) {
    for (int64_t o = 0; o < LP; o++) {
      const Pair &pr = pairs[o];
      std::copy(pr.R.begin(), pr.R.end(), words + word_offsets[o]);
      std::copy(pr.one_best_times.begin(), pr.one_best_times.end(), one_best_times + 2 * word_offsets[o]);
      std::copy(pr.one_best_conf.begin(), pr.one_best_conf.end(), one_best_confidences + word_offsets[o]);
      std::copy(pr.bin_sizes.begin(), pr.bin_sizes.end(), bin_sizes + bin_offsets[o]);
      std::copy(pr.times.begin(), pr.times.end(), bin_times + 2 * bin_offsets[o]);
      std::copy(pr.stat_words.begin(), pr.stat_words.end(), stat_words + stat_offsets[o]);
      std::copy(pr.stat_post.begin(), pr.stat_post.end(), stat_post + stat_offsets[o]);
    }
  }
  T.Finish(g_stats.ms);
  g_stats.ms[5] = ms_loop;
  g_stats.counts[0] = n_launches;
  g_stats.counts[1] = n_rounds;
  g_stats.counts[2] = n_acc;
  if (!fits) {
    SetError("kh_compact_lattice_mbr: lattice %d, point %d: %d words, %d bins, %d statistics do not fit the room of %lld, %lld, "
             "%lld the offsets leave (n_words, n_bins and n_stats hold what every pair needs)", static_cast<int>(bad / P),
             static_cast<int>(bad % P), n_words[bad], n_bins[bad], n_stats[bad],
             static_cast<long long>(word_offsets[bad + 1] - word_offsets[bad]),
             static_cast<long long>(bin_offsets[bad + 1] - bin_offsets[bad]),
             static_cast<long long>(stat_offsets[bad + 1] - stat_offsets[bad]));
    return KH_EINVAL;
  }
  return KH_OK;
}
