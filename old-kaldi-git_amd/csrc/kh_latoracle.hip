// kh_latoracle.hip — the oracle path of latbin/lattice-oracle.cc (:313-421) for a batch of top-sorted CompactLattices, one
// reference word sequence each, and K "mask points" at once: the path through the lattice with the smallest edit distance
// to the reference, its error counts, and as a by-product the numerator of CompactLatticeDepth
// (lat/lattice-functions.cc:574-602).  The points are the keep masks kh_compact_lattice_prune returns, so oracle WER and
// depth as a function of the pruning beam come out of one pass.
//
// The reference builds an edit-distance transducer (:93-129), composes twice (:343, :351) and runs fst::ShortestPath (:356).
// Only the words matter to that (ConvertLatticeToUnweightedAcceptor :80-91 removes the weights, projects onto the words and
// maps label 0 and the wildcards to epsilon; the transition-id chains ConvertLattice adds carry epsilon), so it is the
// integer dynamic programme over (lattice state e, reference position j), r[1..R] = the reference without wildcards (:333):
//   D[start][j] = j
//   D[e][j] = min( over the kept arcs s -> e with word w:  w eps: D[s][j];  else D[s][j-1] + (w != r[j]) ("diagonal", j >= 1)
//                  and D[s][j] + 1 ("insertion");   D[e][j-1] + 1 ("deletion", j >= 1) )
// int32, with kSent for the states in front of the start state or unreachable over kept arcs; the answer is min D[f][R]
// over the states whose final weight is kept, -1 when there is none (the reference's "Best-path failed" :359-361).
//
// What is the reference's and what is not: errors, num_words = R and with them the "Overall %WER" total are fixed by the
// problem.  WHICH of several equal-cost paths is taken - hence the split into insertions, deletions and substitutions that
// CountErrors (:131-164) reads off the path, and the oracle word sequence (:351-356, :381) - is decided in the reference by
// OpenFst's ShortestPath over the composed machine; that is not reproduced.  The rule here is fixed instead: the end state is
// the lowest-numbered state with a kept final weight that attains the minimum; walking back, the first candidate that attains
// the cell's value is taken, in the order: incoming kept arcs by ascending arc number, for an arc with a word its diagonal
// before its insertion, the deletion last.
//
// Shape: one wave per (lattice, point), lane = reference position, 0..R in chunks of 64.  States in number order, each
// state's value pulled over its incoming-arc list (a counting sort by destination: (source state, arc position) order =
// ascending arc number).  The diagonal is a one-lane shift of the source row (__shfl_up), lane 0 taking the last column of
// the chunk before from memory.  The deletion is D[e][j] = j + min over k <= j of (c[k] - k): a wave prefix-min in six
// shuffle steps plus a carry between chunks, not a loop over j.  The rows stay in a device workspace of
// n_states x (R + 1) x 4 bytes per (lattice, point) - the walk back needs all of them - and are not staged in LDS: a row is
// read once per outgoing arc by the lanes that wrote it, the one foreign column is the carry.  The walk back is the tail of
// the same kernel: the lanes test 64 incoming arcs of the cell at once and one __ballot picks the first.  The frame sum is a
// wave reduction at the head of it.
#include <algorithm>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"

namespace kh {
namespace {

constexpr int kLanes = 64;
constexpr int32_t kSent = 0x3fffffff;   // no addition made here can overflow it
constexpr int32_t kMaxRefWords = 1 << 24;   // a reference is shorter than this: positions, and positions + 64, stay far inside int32

struct OrLat {
  int64_t state_base;  // first state of the lattice in the batch's state arrays
  int64_t arc_base;    // first arc of the lattice in the caller's arc order
  int64_t ws_off;      // first int32 of the lattice's rows (point 0) in the workspace
  int64_t ref_base;    // first word of its reference (wildcards removed)
  int32_t n_states;
  int32_t n_arcs;
  int32_t start;
  int32_t R;           // words of the reference
  int32_t lat;         // index in the caller's batch
  int32_t pad;
};

__device__ __forceinline__ bool Bit(const uint64_t *m, int64_t i, int64_t W, int p) {
  return m == nullptr || ((m[i * W + (p >> 6)] >> (p & 63)) & 1) != 0;
}

__global__ __launch_bounds__(kLanes) void OracleKernel(
    const OrLat *__restrict__ lats, const int64_t *__restrict__ in_off, const int32_t *__restrict__ in_src,
    const int32_t *__restrict__ in_arc, const int32_t *__restrict__ in_label, const int32_t *__restrict__ refw,
    const int32_t *__restrict__ is_final, const uint64_t *__restrict__ arc_keep, const uint64_t *__restrict__ state_keep,
    const uint64_t *__restrict__ final_keep, const int32_t *__restrict__ arc_frames, const int32_t *__restrict__ final_frames,
    int n_points, int n_words, int32_t *ws, int32_t *errors, int32_t *counts, int32_t *path_len, int32_t *path_arcs,
    const int64_t *__restrict__ path_offsets, int32_t *path_final, int64_t *frame_sum) {
  const OrLat L = lats[blockIdx.x];
  const int p = blockIdx.y, lane = threadIdx.x;
  const int64_t W = n_words, o = static_cast<int64_t>(L.lat) * n_points + p;
  const int R = L.R;
  const int64_t RS = static_cast<int64_t>(R) + 1;
  int32_t *D = ws + L.ws_off + static_cast<int64_t>(p) * L.n_states * RS;
  const int32_t *rw = refw + L.ref_base;     // r[j] = rw[j - 1]
  const int64_t *io = in_off + L.state_base;

  // the numerator of CompactLatticeDepth (lat/lattice-functions.cc:593-600) over what the point keeps
  if (arc_frames != nullptr) {
    long long fs = 0;
    for (int32_t a = lane; a < L.n_arcs; a += kLanes)
      if (Bit(arc_keep, L.arc_base + a, W, p)) fs += arc_frames[L.arc_base + a];
    for (int32_t s = lane; s < L.n_states; s += kLanes)
      if (Bit(state_keep, L.state_base + s, W, p) && Bit(final_keep, L.state_base + s, W, p)) fs += final_frames[L.state_base + s];
    for (int x = 32; x >= 1; x >>= 1) fs += __shfl_xor(fs, x);
    if (lane == 0) frame_sum[o] = fs;
  }

  // the rows, in state order
  int32_t best = kSent, best_state = -1;
  for (int32_t s = 0; s < L.n_states; s++) {
    int32_t carry = kSent, vR = kSent;
    for (int c0 = 0; c0 <= R; c0 += kLanes) {
      const int j = c0 + lane;
      const bool active = j <= R;
      int32_t v = kSent;
      if (s == L.start) {
        v = j;
      } else if (s > L.start) {
        const int32_t rj = active && j >= 1 ? rw[j - 1] : 0;
        const int64_t k1 = io[s + 1];
        for (int64_t k = io[s]; k < k1; k++) {
          if (!Bit(arc_keep, L.arc_base + in_arc[k], W, p)) continue;
          const int32_t *src = D + in_src[k] * RS;
          const int32_t a = active ? src[j] : kSent;
          const int32_t w = in_label[k];
          int32_t cand = a;
          if (w != 0) {
            int32_t d = __shfl_up(a, 1);
            if (lane == 0) d = c0 > 0 ? src[c0 - 1] : kSent;
            cand = min(d + (w != rj ? 1 : 0), a + 1);
          }
          v = min(v, cand);
        }
      }
      if (!active) v = kSent;
      // the deletions: an inclusive prefix-min of v[k] - k over the chunk and the chunks before it
      int32_t t = v - j;
#pragma unroll
      for (int x = 1; x < kLanes; x <<= 1) {
        const int32_t u = __shfl_up(t, x);
        if (lane >= x) t = min(t, u);
      }
      t = min(t, carry);
      carry = __shfl(t, kLanes - 1);
      v = min(t + j, kSent);
      if (active) D[s * RS + j] = v;
      if (c0 + kLanes > R) vR = __shfl(v, R - c0);
    }
    WaveFence();
    if (vR < best && is_final[L.state_base + s] != 0 && Bit(final_keep, L.state_base + s, W, p)) {
      best = vR;
      best_state = s;
    }
  }

  // the walk back from (best_state, R)
  int32_t n_cor = 0, n_sub = 0, n_ins = 0, n_del = 0, len = 0;
  int32_t *out = path_arcs + path_offsets[o];
  const int64_t room = path_offsets[o + 1] - path_offsets[o];
  bool lost = false;
  if (best < kSent) {
    int32_t e = best_state, j = R;
    while (e != L.start) {
      const int32_t val = D[e * RS + j];
      const int64_t k1 = io[e + 1];
      bool found = false;
      for (int64_t k0 = io[e]; k0 < k1 && !found; k0 += kLanes) {
        const int64_t k = k0 + lane;
        int32_t type = 0, src = 0, arc = 0;     // 1 epsilon, 2 correct, 3 substitution, 4 insertion
        if (k < k1) {
          arc = in_arc[k];
          if (Bit(arc_keep, L.arc_base + arc, W, p)) {
            src = in_src[k];
            const int32_t w = in_label[k], a = D[src * RS + j];
            if (w == 0) {
              if (a == val) type = 1;
            } else {
              const int32_t sub = j >= 1 && w != rw[j - 1] ? 1 : 0;
              if (j >= 1 && D[src * RS + j - 1] + sub == val) type = 2 + sub;
              else if (a + 1 == val) type = 4;
            }
          }
        }
        const unsigned long long m = __ballot(type != 0);
        if (m != 0) {
          const int first = __ffsll(m) - 1;
          const int32_t ty = __shfl(type, first);
          const int32_t taken = __shfl(arc, first);
          if (lane == 0 && len < room) out[len] = taken;
          len++;
          e = __shfl(src, first);
          if (ty == 2) n_cor++;
          if (ty == 3) n_sub++;
          if (ty == 2 || ty == 3) j--;
          if (ty == 4) n_ins++;
          found = true;
        }
      }
      if (!found) {
        if (j == 0) {           // cannot happen on rows this kernel wrote
          lost = true;
          break;
        }
        n_del++;
        j--;
      }
    }
    if (!lost) n_del += j;      // D[start][j > 0] is a deletion
    WaveFence();
    for (int32_t i = lane; i < len / 2 && len <= room; i += kLanes) {
      const int32_t x = out[i], y = out[len - 1 - i];
      out[i] = y;
      out[len - 1 - i] = x;
    }
  }
  if (lane == 0) {
    const bool ok = best < kSent && !lost;
    errors[o] = ok ? best : (lost ? -2 : -1);
    counts[4 * o] = ok ? n_cor : 0;
    counts[4 * o + 1] = ok ? n_sub : 0;
    counts[4 * o + 2] = ok ? n_ins : 0;
    counts[4 * o + 3] = ok ? n_del : 0;
    path_len[o] = ok ? len : -1;
    path_final[o] = ok ? best_state : -1;
  }
}

thread_local CallStats<5, 1> g_stats;   // counts: OracleKernel launches of the last call

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" int kh_compact_lattice_oracle_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_compact_lattice_oracle_last_timings(float *ms5, int32_t *n_launches) {
  return GetTimings(g_stats, ms5, n_launches);
}

extern "C" int kh_compact_lattice_oracle(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                                         const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                                         const int32_t *is_final, const int64_t *ref_offsets, const int32_t *ref_words,
                                         int n_wildcards, const int32_t *wildcards, int n_points, const uint64_t *arc_keep,
                                         const uint64_t *state_keep, const uint64_t *final_keep, const int32_t *arc_frames,
                                         const int32_t *final_frames, int32_t *errors, int32_t *counts, int32_t *path_len,
                                         int32_t *path_arcs, const int64_t *path_offsets, int32_t *path_final_state,
                                         int64_t *arc_frame_sum) {
  int rc = EnsureDevice();
  if (rc) return rc;
  if (n_points < 1) {
    SetError("kh_compact_lattice_oracle: n_points = %d: at least one point is needed", n_points);
    return KH_EINVAL;
  }
  const bool masked = arc_keep != nullptr;
  KH_CHECK_ARG(masked == (state_keep != nullptr) && masked == (final_keep != nullptr));
  if (!masked && n_points != 1) {
    SetError("kh_compact_lattice_oracle: n_points = %d without keep masks: no masks means one point that keeps everything",
             n_points);
    return KH_EINVAL;
  }
  KH_CHECK_ARG(n_points <= 65535);           // (the launch grid's second dimension)
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && lat_start && arc_offsets && arc_label && arc_nextstate && is_final &&
               ref_offsets && errors && counts && path_len && path_arcs && path_offsets && path_final_state);
  KH_CHECK_ARG(n_wildcards >= 0 && (n_wildcards == 0 || wildcards));
  KH_CHECK_ARG((arc_frames != nullptr) == (final_frames != nullptr) && (arc_frames == nullptr || arc_frame_sum != nullptr));
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0 && ref_offsets[0] == 0 && path_offsets[0] == 0);
  for (int l = 0; l < n_lats; l++) KH_CHECK_ARG(lat_state_offsets[l + 1] - lat_state_offsets[l] > 0);
  for (int i = 1; i < n_wildcards; i++) KH_CHECK_ARG(wildcards[i] > wildcards[i - 1]);
  CallTimer T;
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  KH_CHECK_ARG(A >= 0 && A < (1ll << 31));   // (arc positions within a lattice are kept as int32 in the incoming lists)
  const int64_t P = n_points, W = (P + kLanes - 1) / kLanes;
  // MapWildCards lattice-oracle.cc:58-75: a wildcard is epsilon, on the lattice (:88) and in the reference (:333)
  auto word = [&](int32_t w) { return std::binary_search(wildcards, wildcards + n_wildcards, w) ? 0 : w; };

  // validation and the incoming lists (ascending arc number within a state's list)
  std::vector<OrLat> lats(n_lats);
  std::vector<int32_t> refw, in_label(A);
  Incoming in;
  std::string err;
  if (!BuildIncoming(
          "kh_compact_lattice_oracle", n_lats, lat_state_offsets, lat_start, arc_offsets, arc_nextstate, &in, &err,
          [&](int l, int32_t, int32_t) {
            if (ref_offsets[l + 1] < ref_offsets[l])
              return Refuse(&err, "kh_compact_lattice_oracle: lattice %d: ref_offsets %lld, %lld: the offsets must ascend", l,
                            static_cast<long long>(ref_offsets[l]), static_cast<long long>(ref_offsets[l + 1]));
            if (ref_offsets[l + 1] - ref_offsets[l] >= kMaxRefWords)
              return Refuse(&err, "kh_compact_lattice_oracle: lattice %d: a reference of %lld words: at most %d are taken", l,
                            static_cast<long long>(ref_offsets[l + 1] - ref_offsets[l]), kMaxRefWords - 1);
            KH_REFUSE_ARG(&err, ref_offsets[l + 1] == ref_offsets[l] || ref_words);
            return true;
          },
          NoStateHook(), NoArcHook(),
          [&](int l, int32_t s0, int32_t ns) {
            for (int64_t p = 0; p < P; p++) {
              const int64_t o = static_cast<int64_t>(l) * P + p, room = path_offsets[o + 1] - path_offsets[o];
              if (room < ns - 1)
                return Refuse(&err, "kh_compact_lattice_oracle: lattice %d, point %d: path_offsets leaves room for %lld arcs, a "
                              "path may have %d", l, static_cast<int>(p), static_cast<long long>(room), ns - 1);
            }
            OrLat &L = lats[l];
            L.state_base = s0;
            L.arc_base = arc_offsets[s0];
            L.ws_off = 0;
            L.ref_base = static_cast<int64_t>(refw.size());
            L.n_states = ns;
            L.n_arcs = static_cast<int32_t>(arc_offsets[s0 + ns] - arc_offsets[s0]);
            L.start = lat_start[l];
            L.lat = l;
            L.pad = 0;
            for (int64_t i = ref_offsets[l]; i < ref_offsets[l + 1]; i++)
              if (word(ref_words[i]) != 0) refw.push_back(ref_words[i]);
            L.R = static_cast<int32_t>(static_cast<int64_t>(refw.size()) - L.ref_base);
            return true;
          },
          [&](int, int64_t k, int64_t j) { in_label[k] = word(arc_label[j]); })) {
    SetError("%s", err.c_str());
    return KH_EINVAL;
  }
  // the lattices in flight: longest first, as many as the workspace limit admits per launch (at least one)
  auto cells = [&](const OrLat &L) { return static_cast<size_t>(L.n_states) * (static_cast<size_t>(L.R) + 1) * static_cast<size_t>(P); };
  const int64_t path_total = path_offsets[static_cast<int64_t>(n_lats) * P];
  size_t limit = g_stats.workspace_limit;
  if (limit == 0 &&
      (rc = DefaultWorkspaceLimit(static_cast<size_t>(A) * (16 + (masked ? 8 * W : 0)) + static_cast<size_t>(S) * (16 + (masked ? 16 * W : 0)) +
                                      sizeof(int32_t) * (refw.size() + static_cast<size_t>(path_total)) + 48 * static_cast<size_t>(n_lats) * P,
                                  &limit)) != KH_OK)
    return rc;
  std::vector<size_t> ws_bytes(n_lats);
  for (int l = 0; l < n_lats; l++) ws_bytes[l] = cells(lats[l]) * sizeof(int32_t);
  const ChunkPlan plan = PlanChunks(ws_bytes, limit);
  std::vector<OrLat> sorted(n_lats);
  size_t max_ws_cells = 0;
  for (const ChunkRange &c : plan.ranges) {
    size_t ws_cells = 0;
    for (size_t i = c.begin; i < c.end; i++) {
      sorted[i] = lats[plan.order[i]];
      sorted[i].ws_off = static_cast<int64_t>(ws_cells);
      ws_cells += cells(sorted[i]);
    }
    max_ws_cells = std::max(max_ws_cells, ws_cells);
  }
  T.HostDone();

  hipStream_t st = Stream();
  KH_HIP(T.Init());
  Dev<OrLat> d_lats;
  Dev<int64_t> d_in_off, d_poff, d_fsum;
  Dev<int32_t> d_in_src, d_in_arc, d_in_label, d_refw, d_isfin, d_aframes, d_fframes, d_ws, d_err, d_cnt, d_plen, d_parcs, d_pfin;
  Dev<uint64_t> d_ak, d_sk, d_fk;
  const size_t AW = static_cast<size_t>(A) * W, SW = static_cast<size_t>(S) * W, LP = static_cast<size_t>(n_lats) * P;
  const bool frames = arc_frames != nullptr;
  if (d_lats.Alloc(n_lats) || d_in_off.Alloc(S + 1) || d_poff.Alloc(LP + 1) || d_fsum.Alloc(LP) || d_in_src.Alloc(A) ||
      d_in_arc.Alloc(A) || d_in_label.Alloc(A) || d_refw.Alloc(refw.size()) || d_isfin.Alloc(S) ||
      d_aframes.Alloc(frames ? A : 0) || d_fframes.Alloc(frames ? S : 0) || d_err.Alloc(LP) || d_cnt.Alloc(4 * LP) ||
      d_plen.Alloc(LP) || d_parcs.Alloc(path_total) || d_pfin.Alloc(LP) || d_ak.Alloc(masked ? AW : 0) ||
      d_sk.Alloc(masked ? SW : 0) || d_fk.Alloc(masked ? SW : 0) || d_ws.Alloc(max_ws_cells)) {
    SetError("kh_compact_lattice_oracle: out of device memory (workspace of %lld cells of 4 bytes)",
             static_cast<long long>(max_ws_cells));
    return KH_ENOMEM;
  }
  KH_HIP(T.Mark(0, st));
  KH_HIP(Up(d_lats, sorted.data(), n_lats, st));
  KH_HIP(Up(d_in_off, in.in_off.data(), S + 1, st));
  KH_HIP(Up(d_poff, path_offsets, LP + 1, st));
  KH_HIP(Up(d_isfin, is_final, S, st));
  KH_HIP(Up(d_refw, refw.data(), refw.size(), st));
  KH_HIP(Up(d_in_src, in.in_src.data(), A, st));
  KH_HIP(Up(d_in_arc, in.in_arc.data(), A, st));
  KH_HIP(Up(d_in_label, in_label.data(), A, st));
  if (frames) KH_HIP(Up(d_aframes, arc_frames, A, st));
  if (masked) KH_HIP(Up(d_ak, arc_keep, AW, st));
  if (frames) KH_HIP(Up(d_fframes, final_frames, S, st));
  if (masked) {
    KH_HIP(Up(d_sk, state_keep, SW, st));
    KH_HIP(Up(d_fk, final_keep, SW, st));
  }
  KH_HIP(T.Mark(1, st));
  for (const ChunkRange &c : plan.ranges) {
    hipLaunchKernelGGL(OracleKernel, dim3(c.end - c.begin, static_cast<unsigned>(P)), dim3(kLanes), 0, st, d_lats.p + c.begin,
                       d_in_off.p, d_in_src.p, d_in_arc.p, d_in_label.p, d_refw.p, d_isfin.p, masked ? d_ak.p : nullptr,
                       masked ? d_sk.p : nullptr, masked ? d_fk.p : nullptr, frames ? d_aframes.p : nullptr,
                       frames ? d_fframes.p : nullptr, n_points, static_cast<int>(W), d_ws.p, d_err.p, d_cnt.p, d_plen.p,
                       d_parcs.p, d_poff.p, d_pfin.p, d_fsum.p);
    KH_LAUNCH_CHECK();
  }
  KH_HIP(T.Mark(2, st));
  KH_HIP(hipMemcpyAsync(errors, d_err.p, sizeof(int32_t) * LP, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(counts, d_cnt.p, sizeof(int32_t) * 4 * LP, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(path_len, d_plen.p, sizeof(int32_t) * LP, hipMemcpyDeviceToHost, st));
  KH_HIP(hipMemcpyAsync(path_final_state, d_pfin.p, sizeof(int32_t) * LP, hipMemcpyDeviceToHost, st));
  if (path_total > 0) KH_HIP(hipMemcpyAsync(path_arcs, d_parcs.p, sizeof(int32_t) * path_total, hipMemcpyDeviceToHost, st));
  if (frames) KH_HIP(hipMemcpyAsync(arc_frame_sum, d_fsum.p, sizeof(int64_t) * LP, hipMemcpyDeviceToHost, st));
  KH_HIP(T.Mark(3, st));
  KH_HIP(hipStreamSynchronize(st));
  KH_HIP(T.AddAll());
  T.Finish(g_stats.ms);
  g_stats.counts[0] = static_cast<int32_t>(plan.ranges.size());
  for (size_t i = 0; i < LP; i++) {
    if (errors[i] == -2) {
      SetError("kh_compact_lattice_oracle: lattice %d, point %d: the walk back lost the path (internal error)",
               static_cast<int>(i / P), static_cast<int>(i % P));
      return KH_EDEVICE;
    }
  }
  return KH_OK;
}
