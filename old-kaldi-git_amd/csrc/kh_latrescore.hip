// kh_latrescore.hip — RescoreCompactLatticeInternal(NULL, 1.0, ...) (lat/lattice-functions.cc:1163-1290) with
// CompactLatticeStateTimes (:69-106) for a batch of top-sorted CompactLattices and a device matrix of per-(frame, pdf)
// log-likelihoods: gmm-rescore-lattice's inner call.  The rule - statuses, what the host decides and the order of the float
// sums - is in include/kaldi_hip.h at kh_rescore_compact_lattice.
//
// Shape.  The reference walks t ascending and updates the arc (or final weight) that owns the transition-id at t in place
// (:1256-1287), so the new acoustic cost of one item is  v = old; for k: v = fl32((-ll[t_src + k][pdf(s_k)]) + v)  and the
// items never meet: one work item per arc and per non-Zero final weight, the k loop strictly serial.
//   * RescoreShortKernel: one THREAD per item, for strings of 1 .. kShortLen transition-ids - what a determinized lattice
//     mostly holds next to its few long arcs, and all that a state-level lattice holds.  The item arrays (offsets, rows,
//     costs) are read and written contiguously across the lanes; the gather is one dword per (item, k).
//   * RescoreLongKernel: one WAVE per item, for longer strings: the lanes gather 64 consecutive frames of the string at a
//     time (64 independent loads in flight, consecutive rows of the matrix) and every lane then folds the 64 values in
//     string order from the lanes' registers, so the serial chain is adds alone and never waits on memory.
// Which items go where is decided per item on the host (len > kShortLen), which builds the list of long items while it
// computes the state times.  Both kernels add in the same order, so the cut-over changes no bit.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"

namespace kh {
namespace {

constexpr int kShortLen = 8;    // strings up to this length: one thread; longer: one wave
constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / KH_WAVE;

struct Items {
  const int64_t *arc_off;     // [A + 1] into strings
  const int64_t *final_off;   // [S + 1] into strings
  const int32_t *strings;
  const int32_t *arc_row;     // [A] row of the matrix of the item's first transition-id; -1: not rescored
  const int32_t *final_row;   // [S]
  float *arc_a;               // [A] in/out
  float *final_a;             // [S] in/out
  const int32_t *tid2pdf;     // [num_tids + 1]
  const float *ll;
  int64_t stride;
  int64_t n_arcs, n_items;    // items = arcs, then final weights
};

// -log_like + Value2() (:1270, :1283), one frame
__device__ __forceinline__ float Step(float log_like, float v) { return (-log_like) + v; }

__global__ __launch_bounds__(kThreads) void RescoreShortKernel(Items I) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < I.n_items;
       i += static_cast<int64_t>(gridDim.x) * kThreads) {
    const bool arc = i < I.n_arcs;
    const int64_t j = arc ? i : i - I.n_arcs;
    const int32_t row = arc ? I.arc_row[j] : I.final_row[j];
    if (row < 0) continue;
    const int64_t *off = arc ? I.arc_off : I.final_off;
    const int64_t b = off[j], len = off[j + 1] - b;
    if (len <= 0 || len > kShortLen) continue;
    float *val = arc ? I.arc_a : I.final_a;
    float v = val[j];
    const float *ll = I.ll + static_cast<int64_t>(row) * I.stride;
    for (int64_t k = 0; k < len; k++) v = Step(ll[k * I.stride + I.tid2pdf[I.strings[b + k]]], v);
    val[j] = v;
  }
}

__global__ __launch_bounds__(kThreads) void RescoreLongKernel(Items I, const int64_t *__restrict__ long_items, int64_t n_long) {
  const int lane = threadIdx.x & (KH_WAVE - 1);
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (w >= n_long) return;
  const int64_t i = long_items[w];
  const bool arc = i < I.n_arcs;
  const int64_t j = arc ? i : i - I.n_arcs;
  const int32_t row = arc ? I.arc_row[j] : I.final_row[j];
  const int64_t *off = arc ? I.arc_off : I.final_off;
  const int64_t b = off[j], len = off[j + 1] - b;
  float *val = arc ? I.arc_a : I.final_a;
  float v = val[j];
  const float *ll = I.ll + static_cast<int64_t>(row) * I.stride;
  for (int64_t base = 0; base < len; base += KH_WAVE) {
    const int64_t k = base + lane;
    float x = 0.f;
    if (k < len) x = ll[k * I.stride + I.tid2pdf[I.strings[b + k]]];
    const int n = static_cast<int>(len - base < KH_WAVE ? len - base : KH_WAVE);
    for (int q = 0; q < n; q++) v = Step(__shfl(x, q), v);   // every lane folds the same values in string order
  }
  if (lane == 0) val[j] = v;
}

thread_local CallStats<5, 3> g_stats;   // counts: launches, short items, long items

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" int kh_rescore_compact_lattice_last_timings(float *ms5, int32_t *counts3) {
  return GetTimings(g_stats, ms5, counts3);
}

extern "C" int kh_rescore_compact_lattice(
    int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start, const int64_t *arc_offsets,
    const int32_t *arc_nextstate, float *arc_acoustic, const int64_t *arc_string_offsets, const float *final_graph,
    float *final_acoustic, const int64_t *final_string_offsets, const int32_t *strings, int64_t n_strings,
    const float *loglikes, KhMatrixDim d_loglikes, const int32_t *ll_row_offsets, int num_tids, const int32_t *tid2pdf,
    int32_t *status, int32_t *utt_len) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && lat_start && arc_offsets && arc_nextstate && arc_acoustic &&
               arc_string_offsets && final_graph && final_acoustic && final_string_offsets && strings && n_strings >= 0 &&
               loglikes && ll_row_offsets && num_tids > 0 && tid2pdf && status && utt_len);
  KH_CHECK_ARG(d_loglikes.rows >= 0 && d_loglikes.cols > 0 && d_loglikes.stride >= d_loglikes.cols);
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0 && ll_row_offsets[0] >= 0);
  for (int l = 0; l < n_lats; l++)
    KH_CHECK_ARG(lat_state_offsets[l + 1] >= lat_state_offsets[l] && ll_row_offsets[l + 1] >= ll_row_offsets[l]);
  KH_CHECK_ARG(ll_row_offsets[n_lats] <= d_loglikes.rows);
  CallTimer T;
  const int64_t S = lat_state_offsets[n_lats];
  for (int64_t s = 0; s < S; s++)
    KH_CHECK_ARG(arc_offsets[s + 1] >= arc_offsets[s] && final_string_offsets[s + 1] >= final_string_offsets[s] &&
                 final_string_offsets[s] >= 0 && final_string_offsets[s + 1] <= n_strings);
  const int64_t A = arc_offsets[S];
  for (int64_t a = 0; a < A; a++)
    KH_CHECK_ARG(arc_string_offsets[a + 1] >= arc_string_offsets[a] && arc_string_offsets[a] >= 0 &&
                 arc_string_offsets[a + 1] <= n_strings);
  for (int t = 1; t <= num_tids; t++) {   // (TransitionIdToPdf; entry 0 is not a transition-id)
    if (tid2pdf[t] < 0 || tid2pdf[t] >= d_loglikes.cols) {
      SetError("kh_rescore_compact_lattice: tid2pdf[%d] = %d, the matrix has %d columns", t, tid2pdf[t], d_loglikes.cols);
      return KH_EINVAL;
    }
  }
  const float inf = INFINITY;
  std::vector<int32_t> times, arc_row(A, -1), final_row(S, -1);
  std::vector<int64_t> long_items;
  std::string err;
  int64_t n_short = 0;
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
    const int64_t a0 = arc_offsets[s0], a1 = arc_offsets[s0 + ns];
    utt_len[l] = 0;
    if (ns == 0 || lat_start[l] < 0) {    // :1169 "Rescoring empty lattice"
      status[l] = KH_RESCORE_EMPTY;
      continue;
    }
    // kTopSorted (:1173; the caller sorts as fst::TopSort does)
    for (int32_t s = 0; s < ns; s++) {
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        if (!ForwardArc("kh_rescore_compact_lattice", l, j - a0, s, arc_nextstate[j], ns, &err)) {
          SetError("%s", err.c_str());
          return KH_EINVAL;
        }
      }
    }
    // CompactLatticeStateTimes :72-105
    bool consistent = lat_start[l] == 0;   // :72
    times.assign(ns, -1);
    times[0] = 0;
    int32_t ul = -1;
    for (int32_t s = 0; s < ns && consistent; s++) {
      const int32_t cur = times[s];
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        const int64_t len = arc_string_offsets[j + 1] - arc_string_offsets[j];
        const int32_t want = static_cast<int32_t>(cur + len), nx = arc_nextstate[j];
        if (times[nx] == -1) times[nx] = want;
        else if (times[nx] != want) consistent = false;   // :87
      }
      const int64_t flen = final_string_offsets[s0 + s + 1] - final_string_offsets[s0 + s];
      if (!(final_graph[s0 + s] == inf && final_acoustic[s0 + s] == inf && flen == 0)) {   // != Zero :89
        const int32_t this_len = static_cast<int32_t>(cur + flen);
        ul = ul == -1 ? this_len : std::max(ul, this_len);   // :91-97
      }
    }
    for (int32_t s = 0; s < ns && consistent; s++)
      if (times[s] < 0) consistent = false;   // :1187
    if (!consistent) {
      status[l] = KH_RESCORE_INCONSISTENT_TIMES;
      continue;
    }
    if (ul == -1) ul = 0;   // :101-104 "Utterance does not have a final-state."
    utt_len[l] = ul;
    // :1186-1218: which items own a frame
    bool mismatch = false, bad_tid = false;
    for (int32_t s = 0; s < ns && !mismatch; s++) {
      const int32_t t = times[s];
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        const int64_t len = arc_string_offsets[j + 1] - arc_string_offsets[j];
        if (len == 0) continue;
        if (t < ul) {
          if (t + len > ul) mismatch = true;   // (the reference indexes time_to_state past its end here)
        } else if (t != ul) {
          mismatch = true;                     // :1200-1204
        }
      }
    }
    if (mismatch) {
      status[l] = KH_RESCORE_MISMATCH;
      continue;
    }
    const int32_t r0 = ll_row_offsets[l], rows = ll_row_offsets[l + 1] - r0;
    if (rows < ul) {   // :1221-1225
      status[l] = KH_RESCORE_FEATURES_TOO_SHORT;
      continue;
    }
    auto check_tids = [&](int64_t b, int64_t e) {
      for (int64_t k = b; k < e; k++)
        if (strings[k] < 1 || strings[k] > num_tids) bad_tid = true;
    };
    for (int32_t s = 0; s < ns; s++) {
      if (times[s] < ul)
        for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++)
          check_tids(arc_string_offsets[j], arc_string_offsets[j + 1]);
      check_tids(final_string_offsets[s0 + s], final_string_offsets[s0 + s + 1]);
    }
    if (bad_tid) {
      status[l] = KH_RESCORE_BAD_TID;
      continue;
    }
    status[l] = KH_RESCORE_OK;
    for (int32_t s = 0; s < ns; s++) {
      const int32_t t = times[s];
      if (t < ul) {
        for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
          const int64_t len = arc_string_offsets[j + 1] - arc_string_offsets[j];
          if (len == 0) continue;
          arc_row[j] = r0 + t;
          if (len > kShortLen) long_items.push_back(j); else n_short++;
        }
      }
      const int64_t flen = final_string_offsets[s0 + s + 1] - final_string_offsets[s0 + s];
      if (flen > 0) {   // (a final weight with a string is not Zero; t + flen <= utt_len by :90-96)
        final_row[s0 + s] = r0 + t;
        if (flen > kShortLen) long_items.push_back(A + s0 + s); else n_short++;
      }
    }
    (void)a1;
  }
  const int64_t n_long = static_cast<int64_t>(long_items.size());
  T.HostDone();
  T.Finish(g_stats.ms);
  g_stats.counts[0] = 0;
  g_stats.counts[1] = static_cast<int32_t>(std::min<int64_t>(n_short, INT32_MAX));
  g_stats.counts[2] = static_cast<int32_t>(std::min<int64_t>(n_long, INT32_MAX));
  if (n_short + n_long == 0) return KH_OK;   // nothing owns a frame: every cost keeps its bits

  hipStream_t st = Stream();
  KH_HIP(T.Init());
  Dev<int64_t> d_arc_off, d_final_off, d_long;
  Dev<int32_t> d_strings, d_arc_row, d_final_row, d_t2p;
  Dev<float> d_arc_a, d_final_a;
  if (d_arc_off.Alloc(A + 1) || d_final_off.Alloc(S + 1) || d_long.Alloc(n_long) || d_strings.Alloc(n_strings) ||
      d_arc_row.Alloc(A) || d_final_row.Alloc(S) || d_t2p.Alloc(num_tids + 1) || d_arc_a.Alloc(A) || d_final_a.Alloc(S)) {
    SetError("kh_rescore_compact_lattice: out of device memory (%lld arcs, %lld transition-ids)", static_cast<long long>(A),
             static_cast<long long>(n_strings));
    return KH_ENOMEM;
  }
  KH_HIP(T.Mark(0, st));
  KH_HIP(Up(d_arc_off, arc_string_offsets, A + 1, st));
  KH_HIP(Up(d_final_off, final_string_offsets, S + 1, st));
  KH_HIP(Up(d_long, long_items.data(), n_long, st));
  KH_HIP(Up(d_strings, strings, n_strings, st));
  KH_HIP(Up(d_arc_row, arc_row.data(), A, st));
  KH_HIP(Up(d_final_row, final_row.data(), S, st));
  KH_HIP(Up(d_t2p, tid2pdf, num_tids + 1, st));
  KH_HIP(Up<float>(d_arc_a, arc_acoustic, A, st));
  KH_HIP(Up<float>(d_final_a, final_acoustic, S, st));
  KH_HIP(T.Mark(1, st));
  Items I;
  I.arc_off = d_arc_off.p;
  I.final_off = d_final_off.p;
  I.strings = d_strings.p;
  I.arc_row = d_arc_row.p;
  I.final_row = d_final_row.p;
  I.arc_a = d_arc_a.p;
  I.final_a = d_final_a.p;
  I.tid2pdf = d_t2p.p;
  I.ll = loglikes;
  I.stride = d_loglikes.stride;
  I.n_arcs = A;
  I.n_items = A + S;
  int32_t launches = 0;
  if (n_short > 0) {
    const int64_t blocks = std::min<int64_t>(DivUp64(A + S, kThreads), static_cast<int64_t>(NumCUs()) * 8);
    hipLaunchKernelGGL(RescoreShortKernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, I);
    KH_LAUNCH_CHECK();
    launches++;
  }
  for (int64_t done = 0; done < n_long;) {   // (a grid of at most 2^20 blocks per launch)
    const int64_t n = std::min<int64_t>(n_long - done, (1ll << 20) * kWavesPerBlock);
    hipLaunchKernelGGL(RescoreLongKernel, dim3(static_cast<unsigned>(DivUp64(n, kWavesPerBlock))), dim3(kThreads), 0, st, I,
                       d_long.p + done, n);
    KH_LAUNCH_CHECK();
    launches++;
    done += n;
  }
  KH_HIP(T.Mark(2, st));
  if (A > 0) KH_HIP(hipMemcpyAsync(arc_acoustic, d_arc_a.p, sizeof(float) * A, hipMemcpyDeviceToHost, st));
  if (S > 0) KH_HIP(hipMemcpyAsync(final_acoustic, d_final_a.p, sizeof(float) * S, hipMemcpyDeviceToHost, st));
  KH_HIP(T.Mark(3, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.AddAll());
  T.Finish(g_stats.ms);
  g_stats.counts[0] = launches;
  return KH_OK;
}
