// kh_latbatch_host.h — the host-only half of kh_latbatch.h: what every batched compact-lattice entry point does to its CSR
// input before anything is uploaded.  Plain C++ (no HIP), so a host compiler can test it alone (tests/cpp/latbatch_host_test.cc).
//   BuildIncoming  the walk that refuses a batch that is not top-sorted, and the incoming-arc lists of every state;
//   ForwardArc     that refusal for one arc, for the callers that walk a lattice themselves;
//   PlanChunks     which items share a launch under a workspace limit.
// A refusal is written to a std::string; the entry point hands it to SetError.
#ifndef KH_LATBATCH_HOST_H_
#define KH_LATBATCH_HOST_H_

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)   // helpers of the including file, not exports of the library
namespace kh {

inline bool Refuse(std::string *err, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline bool Refuse(std::string *err, const char *fmt, ...) {   // always false: `return Refuse(err, ...)`
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  *err = buf;
  return false;
}

// KH_CHECK_ARG (kh_common.h) for the walks below and their hooks: the same text, to the string
#define KH_REFUSE_ARG(err, cond)                                                                              \
  do {                                                                                                        \
    if (!(cond)) return kh::Refuse(err, "%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond);       \
  } while (0)

// Top-sorted: every arc goes to a higher-numbered state of its own lattice.  `arc` is the arc's number within lattice l.
inline bool ForwardArc(const char *entry, int l, int64_t arc, int32_t s, int32_t nx, int32_t ns, std::string *err) {
  if (nx > s && nx < ns) return true;
  return Refuse(err, "%s: lattice %d: arc %lld (state %d -> %d of %d): input lattice must be topologically sorted", entry, l,
                static_cast<long long>(arc), s, nx, ns);
}

// The incoming arcs of every state of the batch: those of state s0 + s are in_src / in_arc[in_off[s0 + s] .. in_off[s0 + s + 1]),
// in (source state, arc position) order, which is ascending arc number - the order in which the reference's forward sweeps
// offer a state its candidates, so "first on a tie" means the same here.  in_src is relative to the lattice's first state,
// in_arc to its first arc.
struct Incoming {
  std::vector<int64_t> in_off;
  std::vector<int32_t> in_src, in_arc;
};

struct NoLatHook { bool operator()(int, int32_t, int32_t) const { return true; } };
struct NoStateHook { bool operator()(int, int32_t, int32_t) const { return true; } };
struct NoArcHook { bool operator()(int, int32_t, int64_t, int32_t) const { return true; } };
struct NoFill { void operator()(int, int64_t, int64_t) const {} };

// One validating walk over the batch, then the counting sort by destination.  In the order of the walk, for lattice l of ns
// states from state s0:
//   lat_start (may be null)       "start state ... of ... states"
//   begin_lat(l, s0, ns)
//   for each state s:             arc_offsets ascend;  on_state(l, s0, s);
//     for each arc j -> nx:       ForwardArc;  on_arc(l, s, j, nx)   (j counts from the batch's first arc)
//   end_lat(l, s0, ns)
// A hook returns false after writing its own refusal to the string it captured; the first refusal ends the walk.
// fill(l, k, j) is then called once per arc, k its place in the incoming lists: the caller copies what it keeps per arc.
template <class BeginLat = NoLatHook, class OnState = NoStateHook, class OnArc = NoArcHook, class EndLat = NoLatHook,
          class Fill = NoFill>
bool BuildIncoming(const char *entry, int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                   const int64_t *arc_offsets, const int32_t *arc_nextstate, Incoming *in, std::string *err,
                   BeginLat begin_lat = BeginLat(), OnState on_state = OnState(), OnArc on_arc = OnArc(),
                   EndLat end_lat = EndLat(), Fill fill = Fill()) {
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  std::vector<int64_t> &in_off = in->in_off;
  in_off.assign(S + 1, 0);
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
    if (lat_start && (lat_start[l] < 0 || lat_start[l] >= ns))
      return Refuse(err, "%s: lattice %d: start state %d of %d states", entry, l, lat_start[l], ns);
    if (!begin_lat(l, s0, ns)) return false;
    const int64_t a0 = arc_offsets[s0];
    for (int32_t s = 0; s < ns; s++) {
      KH_REFUSE_ARG(err, arc_offsets[s0 + s + 1] >= arc_offsets[s0 + s]);
      if (!on_state(l, s0, s)) return false;
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        const int32_t nx = arc_nextstate[j];
        if (!ForwardArc(entry, l, j - a0, s, nx, ns, err)) return false;
        if (!on_arc(l, s, j, nx)) return false;
        in_off[s0 + nx + 1]++;
      }
    }
    if (!end_lat(l, s0, ns)) return false;
  }
  for (int64_t s = 0; s < S; s++) in_off[s + 1] += in_off[s];
  in->in_src.resize(A);
  in->in_arc.resize(A);
  std::vector<int64_t> next(in_off.begin(), in_off.end() - 1);
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_state_offsets[l], ns = lat_state_offsets[l + 1] - s0;
    const int64_t a0 = arc_offsets[s0];
    for (int32_t s = 0; s < ns; s++) {
      for (int64_t j = arc_offsets[s0 + s]; j < arc_offsets[s0 + s + 1]; j++) {
        const int64_t k = next[s0 + arc_nextstate[j]]++;
        in->in_src[k] = s;
        in->in_arc[k] = static_cast<int32_t>(j - a0);
        fill(l, k, j);
      }
    }
  }
  return true;
}

// The items in flight: largest first (a stable sort, so equal items keep the caller's order), and greedily as many per
// launch as fit the limit together - one always runs, and at most max_per_launch (a launch grid's first dimension).
// order[i] is the item at sorted position i; launch c takes the positions [ranges[c].begin, ranges[c].end).  keys, when
// given, decide the order instead of the sizes.
struct ChunkRange { size_t begin, end; };
struct ChunkPlan {
  std::vector<int32_t> order;
  std::vector<ChunkRange> ranges;
};

inline ChunkPlan PlanChunks(const std::vector<size_t> &sizes, size_t limit, size_t max_per_launch = 65535,
                            const std::vector<size_t> *keys = nullptr) {
  const std::vector<size_t> &key = keys ? *keys : sizes;
  ChunkPlan plan;
  plan.order.resize(sizes.size());
  std::iota(plan.order.begin(), plan.order.end(), 0);
  std::stable_sort(plan.order.begin(), plan.order.end(), [&](int32_t x, int32_t y) { return key[x] > key[y]; });
  for (size_t i = 0; i < sizes.size();) {
    ChunkRange c{i, i};
    size_t bytes = 0;
    while (c.end < sizes.size() && c.end - c.begin < max_per_launch) {
      const size_t b = sizes[plan.order[c.end]];
      if (c.end > c.begin && bytes + b > limit) break;
      bytes += b;
      c.end++;
    }
    plan.ranges.push_back(c);
    i = c.end;
  }
  return plan;
}

}  // namespace kh
#pragma GCC visibility pop

#endif  // KH_LATBATCH_HOST_H_
