// kh_align.hip — forced alignment of a batch of utterances against their own graphs: FasterDecoder
// (decoder/faster-decoder.{h,cc}) as AlignUtteranceWrapper drives it (decoder/decoder-wrappers.cc:423-505; the work of
// gmm-align-compiled and nnet-align-compiled), max_active = INT_MAX.  The contract - what is computed, the one deliberate
// difference from the reference (acceptance against the frame's FINAL cutoff) and the tie rule - is in include/kaldi_hip.h
// at kh_align_compiled.
//
// AlignKernel: one workgroup of 256 lanes per utterance, resident for all its frames.  The host turns every graph into two
// incoming-arc CSRs, one of the emitting arcs and one of the eps-input arcs, each ordered by (destination, arc position), so a
// lane owns destination states (d = lane, lane + 256, ...) and the minimum over a state's incoming arcs with a strict `<` is
// the lowest arc position among equals: deterministic, no atomics.  Token costs are doubles in two buffers of `states`
// entries - in LDS when the utterance has at most g_lds_states states, else in the call's workspace.  Per frame:
//   GetCutoff (:151-213)  count and best cost by a workgroup reduction; with min_active > 0 and more than min_active tokens,
//            the number of tokens whose FLOAT-rounded cost is <= best + beam decides whether the (min_active+1)-th smallest
//            float-rounded cost is needed at all (it is the cutoff only when it lies above best + beam, i.e. when at most
//            min_active tokens lie inside the beam); then it is found by 32 bisection steps over the order-preserving integer
//            image of the float, each one count reduction;
//   ProcessEmitting (:224-303)  per destination the best candidate (prev + float weight) + float ac_cost over the sources
//            with cost < weight_cutoff; the frame's final next_weight_cutoff is (minimum candidate) + adaptive_beam - adding
//            a constant is monotone, so this IS min over candidates of (new_weight + adaptive_beam); candidates not below it
//            are dropped;
//   ProcessNonemitting (:306-346)  relaxation rounds over the eps CSR, each round reading one cost buffer and writing the other
//            (so a round sees only the round before: the result does not depend on lane timing), accepted at <= cutoff, a
//            strictly better cost replaces; ends on a workgroup-wide "nothing changed", after states + 1 rounds at most.
// Backpointers are int32 arc positions, [frames + 1][states] in the workspace: the emitting arc into this frame, the eps arc
// within it, or -1.  At the end ReachedFinal / the best final token (:78-112) by a reduction, then ONE lane walks the
// backpointers (bounded), writes the path's arc positions in path order and recomputes the token costs forward along the
// path to form GetBestPath's two floats (:117-126).
//
// Every loop is bounded; a bound that is hit ends the utterance with KH_ALIGNC_BOUND (a negative eps cycle, or
// backpointers that do not lead to the start).  The walk's bound is (frames + 1) * states - no token is visited twice -
// because frames + arcs is not an upper bound when a cycle with eps arcs is taken on every frame.
//
// The body is __host__ __device__ and keeps nothing in registers across a barrier: KH_FOR_LANES / KH_END_LANES are "this
// lane, then __syncthreads()" on the device and "for every lane in turn" on the host, so a stand-alone host program steps
// the same code with any lane count up to 256 (tools/align_host_step.cc).
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"

namespace kh {
namespace align {

constexpr int kLanes = 256;
constexpr int kMaxLanes = 256;    // the reduction arrays' size: lanes on the host, waves on the device
constexpr int kHdr = 4;           // status, path length, best final state, -

struct Job {
  int64_t st_base;     // first entry of the utterance in e_off / n_off (states + 1 entries per utterance)
  int64_t fin_base;    // first state of the utterance in final
  int64_t arc_base;    // first arc of the utterance in the by-arc arrays
  int64_t bp_off;      // first int32 of its backpointers in the workspace
  int64_t cost_off;    // first double of its two cost buffers in the workspace; -1: LDS
  int64_t path_off;    // first entry of its path room
  int64_t row0;        // first row of the log-likelihood matrix
  int32_t S, A, T, start, room, n_eps, utt, slot;
};

// one 16-byte record per arc (one load each, and few pointers: the kernel's arguments live in scalar registers)
struct EArc { int32_t src, col, arc; float w; };   // an emitting arc in its destination's list: source, matrix column, position
struct NArc { int32_t src, arc; float w; int32_t pad; };
struct PArc { int32_t src, il, col; float w; };    // by arc position, for the walk

struct Ctx {
  const int32_t *e_off;     // emitting arcs by destination; offsets absolute, states and arc positions inside the utterance
  const EArc *e;
  const int32_t *n_off;     // eps-input arcs by destination
  const NArc *n;
  const float *fin;
  const PArc *arc;
  const float *ll;
  int64_t ll_stride;
  float beam, beam_delta;
  int32_t min_active;
  int32_t *bp;
  double *cost_ws;
  int32_t *hdr;        // kHdr per job of the launch
  double *hdr_cost;
  int32_t *path_arc;
  float *path_ac;
};

struct Shared {
  double red_d[kMaxLanes];
  int32_t red_i[kMaxLanes];
};

#if defined(__HIP_DEVICE_COMPILE__)
#define KH_FOR_LANES { const int lane = static_cast<int>(threadIdx.x);
#define KH_END_LANES } __syncthreads();
#define KH_SYNC() __syncthreads()
__device__ __forceinline__ double WaveMinD(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int32_t WaveSumI(int32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ bool PartLeader(int lane) { return (lane & 63) == 0; }
__device__ __forceinline__ int PartOf(int lane) { return lane >> 6; }
__device__ __forceinline__ int NumParts(int n_lanes) { return n_lanes >> 6; }
#else
#define KH_FOR_LANES for (int lane = 0; lane < n_lanes; lane++) {
#define KH_END_LANES }
#define KH_SYNC() do {} while (0)
inline double WaveMinD(double v) { return v; }
inline int32_t WaveSumI(int32_t v) { return v; }
inline bool PartLeader(int) { return true; }
inline int PartOf(int lane) { return lane; }
inline int NumParts(int n_lanes) { return n_lanes; }
#endif

__host__ __device__ inline double Inf() { return __builtin_huge_val(); }

// the order-preserving unsigned image of a float (no NaN reaches it)
__host__ __device__ inline uint32_t FloatKey(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float KeyFloat(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

__host__ __device__ inline double CombineMin(const Shared *sh, int parts) {
  double v = sh->red_d[0];
  for (int p = 1; p < parts; p++) v = sh->red_d[p] < v ? sh->red_d[p] : v;
  return v;
}
__host__ __device__ inline int32_t CombineSum(const Shared *sh, int parts) {
  int32_t v = 0;
  for (int p = 0; p < parts; p++) v += sh->red_i[p];
  return v;
}

// ProcessNonemitting on `cur` (the other buffer is scratch); on return `cur` holds the result.  false: the bound was hit.
__host__ __device__ inline bool Closure(const Job &J, const Ctx &X, double *&cur, double *&oth, double cutoff, int32_t *bprow,
                                        Shared *sh, int n_lanes) {
  if (J.n_eps == 0) return true;
  const int32_t S = J.S;
  const int32_t *n_off = X.n_off + J.st_base;
  const double inf = Inf();
  for (int32_t round = 0; round <= S; round++) {
    KH_FOR_LANES
      int32_t changed = 0;
      for (int32_t d = lane; d < S; d += n_lanes) {
        double best = cur[d];
        int32_t arc = -1;
        for (int32_t k = n_off[d]; k < n_off[d + 1]; k++) {
          const NArc r = X.n[k];
          const double cs = cur[r.src];
          if (cs < inf && !(cs > cutoff)) {                 // :316
            const double nc = cs + static_cast<double>(r.w);   // Token(arc, prev), faster-decoder.h:124-132
            if (!(nc > cutoff) && nc < best) {              // :326, :334
              best = nc;
              arc = r.arc;
            }
          }
        }
        oth[d] = best;
        if (arc >= 0) {
          bprow[d] = arc;
          changed++;
        }
      }
      changed = WaveSumI(changed);
      if (PartLeader(lane)) sh->red_i[PartOf(lane)] = changed;
    KH_END_LANES
    const int32_t any = CombineSum(sh, NumParts(n_lanes));
    KH_SYNC();
    double *t = cur; cur = oth; oth = t;
    if (any == 0) return true;
  }
  return false;
}

// number of tokens whose float-rounded cost is <= `bound` (by_key = false) or has a key <= `key`
__host__ __device__ inline int32_t CountTokens(const Job &J, const double *cur, bool by_key, uint32_t key, double bound, Shared *sh,
                                               int n_lanes) {
  const double inf = Inf();
  KH_FOR_LANES
    int32_t cnt = 0;
    for (int32_t d = lane; d < J.S; d += n_lanes) {
      const double c = cur[d];
      if (c < inf) {
        const float cf = static_cast<float>(c);
        if (by_key ? FloatKey(cf) <= key : static_cast<double>(cf) <= bound) cnt++;
      }
    }
    cnt = WaveSumI(cnt);
    if (PartLeader(lane)) sh->red_i[PartOf(lane)] = cnt;
  KH_END_LANES
  const int32_t n = CombineSum(sh, NumParts(n_lanes));
  KH_SYNC();
  return n;
}

// The whole search of one utterance by n_lanes lanes (256 on the device).  costA / costB: two buffers of J.S doubles.
__host__ __device__ inline void AlignBody(const Job &J, const Ctx &X, double *costA, double *costB, Shared *sh, int n_lanes) {
  const double inf = Inf();
  const int32_t S = J.S;
  const int parts = NumParts(n_lanes);
  int32_t *bp = X.bp + J.bp_off;
  const int32_t *e_off = X.e_off + J.st_base;
  const float *fin = X.fin + J.fin_base;
  const PArc *parc = X.arc + J.arc_base;
  int32_t *hdr = X.hdr + static_cast<int64_t>(kHdr) * J.slot;
  double *cur = costA, *oth = costB;
  int32_t status = KH_ALIGNC_DONE;

  // InitDecoding :36-45
  KH_FOR_LANES
    for (int32_t d = lane; d < S; d += n_lanes) {
      cur[d] = d == J.start ? 0.0 : inf;
      bp[d] = -1;
    }
  KH_END_LANES
  if (!Closure(J, X, cur, oth, static_cast<double>(std::numeric_limits<float>::max()), bp, sh, n_lanes)) status = KH_ALIGNC_BOUND;

  for (int32_t f = 0; f < J.T && status == KH_ALIGNC_DONE; f++) {
    // GetCutoff :151-213, max_active = INT_MAX
    KH_FOR_LANES
      double best = inf;
      int32_t cnt = 0;
      for (int32_t d = lane; d < S; d += n_lanes) {
        const double c = cur[d];
        if (c < inf) {
          cnt++;
          best = c < best ? c : best;
        }
      }
      best = WaveMinD(best);
      cnt = WaveSumI(cnt);
      if (PartLeader(lane)) {
        sh->red_d[PartOf(lane)] = best;
        sh->red_i[PartOf(lane)] = cnt;
      }
    KH_END_LANES
    const double best_cost = CombineMin(sh, parts);
    const int32_t count = CombineSum(sh, parts);
    KH_SYNC();
    const double beam_cutoff = best_cost + static_cast<double>(X.beam);
    double weight_cutoff = beam_cutoff;
    float adaptive_beam = X.beam;
    if (X.min_active > 0) {
      double min_active_cutoff = inf;
      if (count > X.min_active) {
        // tokens inside the beam after rounding to float (tmp_array_ is a vector<BaseFloat>): more than min_active of
        // them means tmp_array_[min_active] <= beam_cutoff, and the value itself is not used (:204-211)
        const int32_t n_in = CountTokens(J, cur, false, 0u, beam_cutoff, sh, n_lanes);
        if (n_in > X.min_active) {
          min_active_cutoff = beam_cutoff;
        } else {
          uint32_t lo = 0u, hi = 0xffffffffu;   // the smallest key with at least min_active + 1 keys at or below it
          for (int it = 0; it < 32; it++) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (CountTokens(J, cur, true, mid, 0.0, sh, n_lanes) >= X.min_active + 1) hi = mid;
            else lo = mid + 1u;
          }
          min_active_cutoff = static_cast<double>(KeyFloat(lo));
        }
      }
      if (min_active_cutoff > beam_cutoff) {
        adaptive_beam = static_cast<float>(min_active_cutoff - best_cost + static_cast<double>(X.beam_delta));
        weight_cutoff = min_active_cutoff;
      }
    }

    // ProcessEmitting :224-303: the best candidate of every destination, and the frame's minimum
    const float *llrow = X.ll + (J.row0 + f) * X.ll_stride;
    int32_t *bprow = bp + static_cast<int64_t>(f + 1) * S;
    KH_FOR_LANES
      double gmin = inf;
      for (int32_t d = lane; d < S; d += n_lanes) {
        double best = inf;
        int32_t arc = -1;
        for (int32_t k = e_off[d]; k < e_off[d + 1]; k++) {
          const EArc r = X.e[k];
          const double cs = cur[r.src];
          if (cs < weight_cutoff) {                                   // :268
            const float ac_cost = -llrow[r.col];                      // :276
            const double nw = (cs + static_cast<double>(r.w)) + static_cast<double>(ac_cost);   // :277 = Token(arc, ac_cost, prev)
            if (nw < best) {
              best = nw;
              arc = r.arc;
            }
          }
        }
        oth[d] = best;
        bprow[d] = arc;
        gmin = best < gmin ? best : gmin;
      }
      gmin = WaveMinD(gmin);
      if (PartLeader(lane)) sh->red_d[PartOf(lane)] = gmin;
    KH_END_LANES
    const double next_cutoff = CombineMin(sh, parts) + static_cast<double>(adaptive_beam);   // :252-253, :281-282 at the frame's end
    KH_SYNC();
    KH_FOR_LANES
      for (int32_t d = lane; d < S; d += n_lanes) {
        if (!(oth[d] < next_cutoff)) {                                // :278
          oth[d] = inf;
          bprow[d] = -1;
        }
      }
    KH_END_LANES
    { double *t = cur; cur = oth; oth = t; }
    if (!Closure(J, X, cur, oth, next_cutoff, bprow, sh, n_lanes)) status = KH_ALIGNC_BOUND;
  }

  // ReachedFinal :78-85 and the best final token :103-111; equal costs go to the lowest state
  KH_FOR_LANES
    double best = inf;
    int32_t bs = -1;
    for (int32_t d = lane; d < S; d += n_lanes) {
      const double c = cur[d];
      const float fw = fin[d];
      if (c < inf && fw != std::numeric_limits<float>::infinity()) {
        const double tc = c + static_cast<double>(fw);
        if (tc < best) {
          best = tc;
          bs = d;
        }
      }
    }
    sh->red_d[lane] = best;
    sh->red_i[lane] = bs;
  KH_END_LANES
  KH_FOR_LANES
    if (lane == 0) {
      double best = inf;
      int32_t bs = -1;
      for (int l = 0; l < n_lanes; l++) {
        const int32_t s = sh->red_i[l];
        if (s >= 0 && (sh->red_d[l] < best || (sh->red_d[l] == best && s < bs))) {
          best = sh->red_d[l];
          bs = s;
        }
      }
      int32_t len = 0;
      if (status == KH_ALIGNC_DONE && bs < 0) status = KH_ALIGNC_NO_FINAL;
      if (status == KH_ALIGNC_DONE) {
        // the walk: no (frame, state) is met twice, so (frames + 1) * states steps bound it
        const int64_t max_steps = (static_cast<int64_t>(J.T) + 1) * S;
        int32_t state = bs, frame = J.T;
        bool at_start = false;
        for (int64_t step = 0; step <= max_steps; step++) {
          const int32_t arc = bp[static_cast<int64_t>(frame) * S + state];
          if (arc < 0) {
            at_start = frame == 0 && state == J.start;
            break;
          }
          if (arc >= J.A) break;
          if (parc[arc].il != 0 && --frame < 0) break;
          state = parc[arc].src;
          len++;
        }
        if (!at_start) status = KH_ALIGNC_BOUND;
      }
      if (status == KH_ALIGNC_DONE && len > J.room) status = KH_ALIGNC_NEEDS_ROOM;
      if (status == KH_ALIGNC_DONE) {
        int32_t *path = X.path_arc + J.path_off;
        float *pac = X.path_ac + J.path_off;
        int32_t state = bs, frame = J.T;
        for (int32_t i = len - 1; i >= 0; i--) {
          const int32_t arc = bp[static_cast<int64_t>(frame) * S + state];
          path[i] = arc;
          if (parc[arc].il != 0) frame--;
          state = parc[arc].src;
        }
        // GetBestPath :117-126: the tokens' costs again, formed as they were formed
        double c = 0.0;
        int32_t fr = 0;
        for (int32_t i = 0; i < len; i++) {
          const int32_t arc = path[i];
          const PArc r = parc[arc];
          const float w = r.w;
          double nc = c + static_cast<double>(w);
          if (r.il != 0) {
            const float ac = -X.ll[(J.row0 + fr) * X.ll_stride + r.col];
            nc += static_cast<double>(ac);
            fr++;
          }
          const float tot_cost = static_cast<float>(nc - c);
          pac[i] = tot_cost - w;
          c = nc;
        }
      }
      hdr[0] = status;
      hdr[1] = len;
      hdr[2] = bs;
      hdr[3] = 0;
      X.hdr_cost[J.slot] = best;
    }
  KH_END_LANES
}

#if !defined(KH_ALIGN_BODY_ONLY)
__global__ __launch_bounds__(kLanes) void AlignKernel(const Job *__restrict__ jobs, Ctx X) {
  extern __shared__ double lds_cost[];
  __shared__ Shared sh;
  const Job J = jobs[blockIdx.x];
  double *a = J.cost_off < 0 ? lds_cost : X.cost_ws + J.cost_off;
  AlignBody(J, X, a, a + J.S, &sh, kLanes);
}
#endif

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct Prepared {
  std::vector<int32_t> e_off, n_off;
  std::vector<EArc> e;
  std::vector<NArc> n;
  std::vector<PArc> arc;
  std::vector<Job> jobs;                 // one per utterance that may be launched
  std::vector<int32_t> status;           // per utterance: KH_ALIGNC_BAD_INPUT, or KH_ALIGNC_DONE = to be run
};

// Validation and the two incoming-arc CSRs.  A graph with a bad arc gets KH_ALIGNC_BAD_INPUT and is not launched; offsets
// that do not describe a batch at all refuse the call.
inline int Prepare(int n_utts, const int32_t *state_offsets, const int64_t *arc_offsets, const int32_t *start,
                   const int32_t *ilabel, const float *weight, const int32_t *nextstate, const float *final_w, int n_tid,
                   const int32_t *tid2pdf, int ll_rows, int ll_cols, const int32_t *row_offsets, const int64_t *path_offsets,
                   Prepared *P, std::string *first_bad) {
  const char *me = "kh_align_compiled";
  if (state_offsets[0] != 0 || arc_offsets[0] != 0 || path_offsets[0] != 0 || row_offsets[0] < 0) {
    SetError("%s: state, arc and path offsets start at 0 and row offsets are not negative", me);
    return KH_EINVAL;
  }
  for (int u = 0; u < n_utts; u++) {
    if (state_offsets[u + 1] < state_offsets[u] || row_offsets[u + 1] < row_offsets[u] || row_offsets[u + 1] > ll_rows ||
        path_offsets[u + 1] < path_offsets[u] || path_offsets[u + 1] - path_offsets[u] > INT32_MAX) {
      SetError("%s: utterance %d: offsets decrease, or rows %d..%d lie outside the matrix of %d rows", me, u, row_offsets[u],
               row_offsets[u + 1], ll_rows);
      return KH_EINVAL;
    }
  }
  const int64_t n_states = state_offsets[n_utts];
  for (int64_t s = 0; s < n_states; s++) {
    if (arc_offsets[s + 1] < arc_offsets[s]) {
      SetError("%s: arc offsets decrease at state %lld", me, static_cast<long long>(s));
      return KH_EINVAL;
    }
  }
  const int64_t n_arcs = arc_offsets[n_states];
  if (n_arcs > INT32_MAX - 1) {
    SetError("%s: %lld arcs in one call", me, static_cast<long long>(n_arcs));
    return KH_EINVAL;
  }
  P->status.assign(n_utts, KH_ALIGNC_DONE);
  P->e_off.reserve(n_states + n_utts);
  P->n_off.reserve(n_states + n_utts);
  P->arc.resize(n_arcs);
  std::vector<int32_t> cnt_e, cnt_n;
  char buf[256];
  for (int u = 0; u < n_utts; u++) {
    const int64_t s0 = state_offsets[u];
    const int32_t S = state_offsets[u + 1] - state_offsets[u];
    const int64_t a0 = arc_offsets[s0], a1 = arc_offsets[s0 + S];
    bool bad = false;
    auto Bad = [&](const char *what, int64_t where, double v) {
      if (!bad && first_bad->empty()) {
        snprintf(buf, sizeof(buf), "%s: utterance %d: %s (at %lld: %g)", me, u, what, static_cast<long long>(where), v);
        *first_bad = buf;
      }
      bad = true;
    };
    if (S <= 0 || start[u] < 0 || start[u] >= S) Bad("no start state", start[u], S);
    if (a1 - a0 > INT32_MAX / 2) Bad("too many arcs", a1 - a0, 0);
    cnt_e.assign(S > 0 ? S + 1 : 1, 0);
    cnt_n.assign(S > 0 ? S + 1 : 1, 0);
    int32_t n_eps = 0;
    for (int32_t s = 0; s < S && !bad; s++) {
      const float fw = final_w[s0 + s];
      if (std::isnan(fw) || fw == -std::numeric_limits<float>::infinity()) Bad("a final weight is NaN or -inf", s, fw);
      for (int64_t a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; a++) {
        const int32_t il = ilabel[a], ns = nextstate[a];
        if (ns < 0 || ns >= S) { Bad("nextstate out of range", a - a0, ns); break; }
        if (il < 0 || il >= n_tid) { Bad("ilabel outside 0..n_tid-1", a - a0, il); break; }
        if (!std::isfinite(weight[a])) { Bad("an arc weight is not finite", a - a0, weight[a]); break; }
        int32_t col = -1;
        if (il != 0) {
          col = tid2pdf ? tid2pdf[il] : il - 1;
          if (col < 0 || col >= ll_cols) { Bad("the pdf of a transition-id lies outside the matrix's columns", a - a0, col); break; }
          cnt_e[ns + 1]++;
        } else {
          cnt_n[ns + 1]++;
          n_eps++;
        }
        P->arc[a] = PArc{s, il, col, weight[a]};
      }
    }
    if (bad) {
      P->status[u] = KH_ALIGNC_BAD_INPUT;
      continue;
    }
    Job J{};
    J.st_base = static_cast<int64_t>(P->e_off.size());
    J.fin_base = s0;
    J.arc_base = a0;
    J.S = S;
    J.A = static_cast<int32_t>(a1 - a0);
    J.T = row_offsets[u + 1] - row_offsets[u];
    J.row0 = row_offsets[u];
    J.start = start[u];
    J.room = static_cast<int32_t>(path_offsets[u + 1] - path_offsets[u]);
    J.path_off = path_offsets[u];
    J.n_eps = n_eps;
    J.utt = u;
    const int32_t e_base = static_cast<int32_t>(P->e.size()), n_base = static_cast<int32_t>(P->n.size());
    for (int32_t s = 0; s < S; s++) {
      cnt_e[s + 1] += cnt_e[s];
      cnt_n[s + 1] += cnt_n[s];
    }
    for (int32_t s = 0; s <= S; s++) {
      P->e_off.push_back(e_base + cnt_e[s]);
      P->n_off.push_back(n_base + cnt_n[s]);
    }
    P->e.resize(e_base + cnt_e[S]);
    P->n.resize(n_base + cnt_n[S]);
    // arcs in ascending position, so every destination's list is in ascending position
    for (int64_t a = a0; a < a1; a++) {
      const int32_t ns = nextstate[a], rel = static_cast<int32_t>(a - a0);
      const PArc &r = P->arc[a];
      if (r.il != 0) P->e[e_base + cnt_e[ns]++] = EArc{r.src, r.col, rel, r.w};
      else P->n[n_base + cnt_n[ns]++] = NArc{r.src, rel, r.w, 0};
    }
    P->jobs.push_back(J);
  }
  return KH_OK;
}

#if !defined(KH_ALIGN_BODY_ONLY)
static thread_local CallStats<5, 3> g_stats;   // counts: launches, utterances whose costs lay in the workspace, utterances launched
thread_local int32_t g_lds_states = 3584;       // 2 x 8 x 3584 = 56 KiB of the 64 KiB a workgroup may ask for
constexpr int32_t kMaxLdsStates = 3584;

inline size_t BpWords(const Job &J) { return (static_cast<size_t>(J.T) + 1) * static_cast<size_t>(J.S); }
inline size_t WorkspaceBytes(const Job &J, bool lds) {
  return sizeof(int32_t) * BpWords(J) + (lds ? 0 : 2 * sizeof(double) * static_cast<size_t>(J.S));
}
#endif

}  // namespace align
}  // namespace kh

#if !defined(KH_ALIGN_BODY_ONLY)
using namespace kh;
using namespace kh::align;

extern "C" int kh_align_compiled_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_align_compiled_set_lds_states(int max_states) {
  KH_CHECK_ARG(max_states >= 0 && max_states <= kMaxLdsStates);
  g_lds_states = max_states;
  return KH_OK;
}

extern "C" int kh_align_compiled_last_timings(float *ms5, int32_t *counts3) {
  return GetTimings(g_stats, ms5, counts3);
}

extern "C" int kh_align_compiled(int n_utts, const int32_t *state_offsets, const int64_t *arc_offsets, const int32_t *start,
                                 const int32_t *ilabel, const int32_t *olabel, const float *weight, const int32_t *nextstate,
                                 const float *final_w, int n_tid, const int32_t *tid2pdf, const float *loglikes, int ll_rows,
                                 int ll_cols, int ll_stride, const int32_t *utt_row_offsets, float beam, int min_active,
                                 float beam_delta, const int64_t *path_offsets, int32_t *status, double *total_cost,
                                 int32_t *best_state, int32_t *path_len, int32_t *path_ilabel, int32_t *path_olabel, float *path_graph,
                                 float *path_acoustic) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(n_utts > 0 && state_offsets && arc_offsets && start && ilabel && olabel && weight && nextstate && final_w &&
               n_tid > 0 && loglikes && ll_rows >= 0 && ll_cols > 0 && ll_stride >= ll_cols && utt_row_offsets && path_offsets &&
               status && total_cost && best_state && path_len && path_ilabel && path_olabel && path_graph && path_acoustic);
  KH_CHECK_ARG(beam > 0.f && min_active >= 0 && beam_delta >= 0.f && !std::isnan(beam) && !std::isnan(beam_delta));
  CallTimer T;
  Prepared P;
  std::string first_bad;
  if ((rc = Prepare(n_utts, state_offsets, arc_offsets, start, ilabel, weight, nextstate, final_w, n_tid, tid2pdf, ll_rows,
                    ll_cols, utt_row_offsets, path_offsets, &P, &first_bad)) != KH_OK)
    return rc;
  T.HostDone();
  for (int u = 0; u < n_utts; u++) {
    status[u] = P.status[u];
    total_cost[u] = std::numeric_limits<double>::infinity();
    path_len[u] = 0;
    best_state[u] = -1;
  }
  int32_t n_launches = 0, n_ws_cost = 0, n_run = 0;
  if (!P.jobs.empty()) {
    hipStream_t st = Stream();
    KH_HIP(T.Init());
    size_t limit = g_stats.workspace_limit;   // by default half of what is free now, before the fixed buffers
    if (limit == 0 && (rc = DefaultWorkspaceLimit(0, &limit)) != KH_OK) return rc;
    Dev<int32_t> d_e_off, d_n_off, d_path_arc, d_hdr;
    Dev<EArc> d_e;
    Dev<NArc> d_n;
    Dev<PArc> d_arc;
    Dev<float> d_fin, d_path_ac;
    Dev<double> d_hdr_cost;
    Dev<unsigned char> d_ws;
    Dev<Job> d_jobs;
    const size_t path_room = static_cast<size_t>(path_offsets[n_utts]);
    const std::vector<float> fin(final_w, final_w + state_offsets[n_utts]);
    KH_HIP(T.Mark(0, st));
    if (d_e_off.Upload(P.e_off, st) || d_e.Upload(P.e, st) || d_n_off.Upload(P.n_off, st) || d_n.Upload(P.n, st) ||
        d_arc.Upload(P.arc, st) || d_fin.Upload(fin, st) || d_path_arc.Alloc(path_room) || d_path_ac.Alloc(path_room)) {
      SetError("kh_align_compiled: out of device memory");
      return KH_ENOMEM;
    }
    KH_HIP(T.Mark(1, st));
    KH_HIP(hipStreamSynchronize(st));
    KH_HIP(T.Add(&T.up, 0, 1));
    // what can run at all; largest workspace first, as many per launch as the limit admits
    std::vector<int32_t> todo;
    for (size_t j = 0; j < P.jobs.size(); j++) {
      const Job &J = P.jobs[j];
      if (WorkspaceBytes(J, J.S <= g_lds_states) > limit || BpWords(J) > static_cast<size_t>(INT32_MAX) * 64) status[J.utt] = KH_ALIGNC_TOO_LARGE;
      else todo.push_back(static_cast<int32_t>(j));
    }
    std::stable_sort(todo.begin(), todo.end(), [&](int32_t x, int32_t y) {
      return WorkspaceBytes(P.jobs[x], P.jobs[x].S <= g_lds_states) > WorkspaceBytes(P.jobs[y], P.jobs[y].S <= g_lds_states);
    });
    std::vector<Job> batch;
    std::vector<int32_t> h_hdr, h_arc;
    std::vector<double> h_cost;
    std::vector<float> h_ac;
    for (size_t i = 0; i < todo.size();) {
      batch.clear();
      size_t bytes = 0, lds_bytes = 0;
      size_t e = i;
      while (e < todo.size() && e - i < 65535) {
        Job J = P.jobs[todo[e]];
        const bool lds = J.S <= g_lds_states;
        const size_t w = WorkspaceBytes(J, lds);
        if (e > i && bytes + w > limit) break;
        // doubles first (8-byte aligned: every share is a multiple of 4 bytes, so round up)
        bytes = (bytes + 7) & ~static_cast<size_t>(7);
        if (lds) {
          J.cost_off = -1;
          lds_bytes = std::max(lds_bytes, 2 * sizeof(double) * static_cast<size_t>(J.S));
        } else {
          J.cost_off = static_cast<int64_t>(bytes / sizeof(double));
          bytes += 2 * sizeof(double) * static_cast<size_t>(J.S);
          n_ws_cost++;
        }
        J.bp_off = static_cast<int64_t>(bytes / sizeof(int32_t));
        bytes += sizeof(int32_t) * BpWords(J);
        J.slot = static_cast<int32_t>(batch.size());
        batch.push_back(J);
        e++;
      }
      if (d_ws.Grow(bytes + 8) || d_jobs.Grow(batch.size()) || d_hdr.Grow(kHdr * batch.size()) || d_hdr_cost.Grow(batch.size())) {
        SetError("kh_align_compiled: out of device memory (workspace of %lld bytes)", static_cast<long long>(bytes));
        return KH_ENOMEM;
      }
      Ctx X{d_e_off.p, d_e.p, d_n_off.p, d_n.p, d_fin.p, d_arc.p, loglikes, static_cast<int64_t>(ll_stride), beam, beam_delta,
            min_active, reinterpret_cast<int32_t *>(d_ws.p), reinterpret_cast<double *>(d_ws.p), d_hdr.p, d_hdr_cost.p,
            d_path_arc.p, d_path_ac.p};
      KH_HIP(T.Mark(0, st));
      KH_HIP(Up(d_jobs, batch.data(), batch.size(), st));
      KH_HIP(T.Mark(1, st));
      hipLaunchKernelGGL(AlignKernel, dim3(static_cast<unsigned>(batch.size())), dim3(kLanes), lds_bytes, st, d_jobs.p, X);
      KH_LAUNCH_CHECK();
      KH_HIP(T.Mark(2, st));
      h_hdr.resize(kHdr * batch.size());
      h_cost.resize(batch.size());
      KH_HIP(hipMemcpyAsync(h_hdr.data(), d_hdr.p, sizeof(int32_t) * h_hdr.size(), hipMemcpyDeviceToHost, st));
      KH_HIP(hipMemcpyAsync(h_cost.data(), d_hdr_cost.p, sizeof(double) * h_cost.size(), hipMemcpyDeviceToHost, st));
      KH_HIP(hipStreamSynchronize(st));
      for (size_t k = 0; k < batch.size(); k++) {
        const Job &J = batch[k];
        const int32_t s = h_hdr[kHdr * k], len = h_hdr[kHdr * k + 1];
        if (s < KH_ALIGNC_DONE || s > KH_ALIGNC_BOUND || s == KH_ALIGNC_TOO_LARGE || len < 0 || (s == KH_ALIGNC_DONE && len > J.room) ||
            ((s == KH_ALIGNC_DONE || s == KH_ALIGNC_NEEDS_ROOM) && (h_hdr[kHdr * k + 2] < 0 || h_hdr[kHdr * k + 2] >= J.S))) {
          SetError("kh_align_compiled: utterance %d: the kernel left status %d and path length %d (room %d)", J.utt, s, len, J.room);
          return KH_EDEVICE;
        }
        status[J.utt] = s;
        if (s == KH_ALIGNC_DONE || s == KH_ALIGNC_NEEDS_ROOM) {
          path_len[J.utt] = len;
          total_cost[J.utt] = h_cost[k];
          best_state[J.utt] = h_hdr[kHdr * k + 2];
        }
        if (s == KH_ALIGNC_DONE && len > 0) {
          h_arc.resize(len);
          h_ac.resize(len);
          KH_HIP(hipMemcpyAsync(h_arc.data(), d_path_arc.p + J.path_off, sizeof(int32_t) * len, hipMemcpyDeviceToHost, st));
          KH_HIP(hipMemcpyAsync(h_ac.data(), d_path_ac.p + J.path_off, sizeof(float) * len, hipMemcpyDeviceToHost, st));
          KH_HIP(hipStreamSynchronize(st));
          for (int32_t p = 0; p < len; p++) {
            const int32_t arc = h_arc[p];
            if (arc < 0 || arc >= J.A) {
              SetError("kh_align_compiled: utterance %d: the kernel left arc %d of %d on the path", J.utt, arc, J.A);
              return KH_EDEVICE;
            }
            path_ilabel[J.path_off + p] = ilabel[J.arc_base + arc];
            path_olabel[J.path_off + p] = olabel[J.arc_base + arc];
            path_graph[J.path_off + p] = weight[J.arc_base + arc];
            path_acoustic[J.path_off + p] = h_ac[p];
          }
        }
      }
      KH_HIP(T.Mark(3, st));
      KH_HIP(hipStreamSynchronize(st));
      KH_HIP(T.AddAll());
      n_launches++;
      n_run += static_cast<int32_t>(batch.size());
      i = e;
    }
  }
  if (!first_bad.empty()) SetError("%s", first_bad.c_str());
  T.Finish(g_stats.ms);
  g_stats.counts[0] = n_launches;
  g_stats.counts[1] = n_ws_cost;
  g_stats.counts[2] = n_run;
  return KH_OK;
}
#endif  // KH_ALIGN_BODY_ONLY
