// kh_latalign.hip — WordAlignLattice (lat/word-align-lattice.{h,cc}, class LatticeWordAligner: the work of lattice-align-words)
// for a batch of top-sorted CompactLattices.  The contract - which result is computed, and the numbering that is this
// library's own rule - is in include/kaldi_hip.h at kh_compact_lattice_align_words.
//
// The reference builds a machine over tuples (input state, pending transition-ids, pending words) with one epsilon arc per
// input arc (Advance :40-48) and labelled arcs where a word, a silence or a one-phone word can be cut off the front of the
// pending transition-ids (OutputArc :59-69), then removes the epsilons with OpenFst's RmEpsilon.  Here the epsilon-free
// machine is built directly: the unit of work is a PAIR (S, T) - S an output state (the start tuple or the destination of a
// labelled arc), T a tuple reachable from S by Advance alone - with d(S, T), the Times of the input arcs' weights along the
// epsilon path, two float sums accumulated left to right.
//
// AlignKernel: one wave per lattice.  Tuples live in a per-lattice table keyed by (input state, pending lengths, a hash of
// the pending content; content compared on a hit), pending strings in a per-lattice arena; the destination of a labelled
// arc is a suffix of its source's pending strings and shares them.  Pairs live in a second table keyed (S, T) and are
// chained per input state of T.  The input is top-sorted and Advance goes to a higher-numbered input state, so the wave
// walks the input states in ascending order: when it reaches state s every d(S, T) with T on s is final (all its epsilon
// predecessors sit on lower states; where two epsilon paths meet, Plus keeps the better one BEFORE T is expanded, which is a
// topological shortest distance, not a label-correcting one, so no result depends on scheduling).  Per state, while pairs
// are chained there: up to 64 pairs are taken, one per lane;
//   A  (lanes in parallel) the word-boundary automaton of T, if T was not classified yet: the scans of OutputNormalWordArc /
//      OutputSilenceArc / OutputOnePhoneWordArc / OutputArcForce over (phone, IsFinal, IsSelfLoop) of the pending ids;
//   B  step j = 0, 1, ... of every lane: the destination tuple of T's labelled arc, or T advanced over the j-th input arc.
//      Lanes hash and look their candidate up in parallel; then the lanes take turns (a loop over the ballot, a wavefront
//      fence between turns) to insert what was not found - copying the pending strings into the arena - and to relax the
//      pair: a new root pair (T', T') with weight One on the same input state, or (S, T + arc) with d(S, T) x w(arc).
// One lane at a time changes the tables, so there are no atomics and no lane ever waits for another.  Every loop is bounded
// by a table's capacity: a table or arena that runs full ends the lattice with kNeedsRoom and the host runs it again with
// twice the room; nothing is written past a capacity.  Labelled arcs that stay on one input state chain root pairs onto
// the state being processed, which is why the per-state loop repeats until the chain is empty.
//
// The host then (Finish) reads tuples and pairs back: arcs and final weights per output state, the states that reach a
// final weight, the numbering key, the Plus merges of equal (label, destination), the sort.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "kh_common.h"
#include "kh_latbatch.h"

namespace kh {
namespace latalign {

constexpr int kLanes = 64;
// WordBoundaryInfo::PhoneType (word-align-lattice.h:136-146)
enum { kNoPhone = 0, kWordBeginPhone, kWordEndPhone, kWordBeginAndEndPhone, kWordInternalPhone, kNonWordPhone };
// t_kind
enum { kKindEps = 0, kKindOut = 1, kKindForce = 2, kKindFinal = 3 };
// hdr[0]; 0 = done
enum { kTooMany = 3, kNeedsRoom = 5 };
// tinfo[tid]: phone | final << 30 | self-loop << 29
constexpr int32_t kFinalBit = 1 << 30, kSelfBit = 1 << 29, kPhoneMask = (1 << 29) - 1;
constexpr int kHdr = 8;        // status, tuples, pairs, arena used, error, fatal
constexpr int kTupleCols = 11, kPairCols = 5;

struct AlignJob {
  int64_t ws_off;      // first int32 of the lattice's workspace
  int64_t hdr_off;     // first int32 of its header: the headers of a launch lie together in front of the workspaces
  int64_t state_base;  // first state of the lattice in arc_off
  int32_t n_states;    // after CreateSuperFinal
  int32_t start, sf;   // start state, the single final state
  int32_t C, HS, PC, PS, R;   // room: tuples, tuple slots (a power of two), pairs, pair slots, arena words
  int32_t max_states;
  int32_t sil, partial;       // labels inside the construction (:275-282)
  int32_t lat;
};

struct AlignCtx {
  const int32_t *arc_off;     // per state of the batch (+1): arcs of the batch, numbered from 0
  const int32_t *arc_label, *arc_next;
  const float *arc_g, *arc_a;
  const int32_t *str_off;     // per arc (+1)
  const int32_t *strings;
  const int32_t *tinfo, *ptype;
  int32_t reorder;
  int32_t *ws;
};

inline size_t WorkspaceWords(const AlignJob &J) {
  return static_cast<size_t>(J.n_states) + J.HS + J.PS + static_cast<size_t>(kTupleCols) * J.C +
         static_cast<size_t>(kPairCols) * J.PC + J.R;
}

// what the host reads back of a finished lattice: tuples, pairs and the used part of the arena lie in front
inline size_t ResultWords(const AlignJob &J, int32_t arena_used) {
  return static_cast<size_t>(kTupleCols) * J.C + static_cast<size_t>(kPairCols) * J.PC + static_cast<size_t>(arena_used);
}

struct View {   // the lattice's header and workspace, all int32: tuples, pairs, arena, then chain heads and slots
  int32_t *hdr, *head, *tslots, *pslots;
  int32_t *t_in, *t_toff, *t_tlen, *t_woff, *t_wlen, *t_hash, *t_kind, *t_consume, *t_wdrop, *t_label, *t_dest;
  int32_t *p_S, *p_T, *p_g, *p_a, *p_next;
  int32_t *arena;
  __host__ __device__ View(int32_t *h, int32_t *w, const AlignJob &J) {
    hdr = h;
    t_in = w; t_toff = t_in + J.C; t_tlen = t_toff + J.C; t_woff = t_tlen + J.C; t_wlen = t_woff + J.C;
    t_hash = t_wlen + J.C; t_kind = t_hash + J.C; t_consume = t_kind + J.C; t_wdrop = t_consume + J.C;
    t_label = t_wdrop + J.C; t_dest = t_label + J.C;
    p_S = t_dest + J.C; p_T = p_S + J.PC; p_g = p_T + J.PC; p_a = p_g + J.PC; p_next = p_a + J.PC;
    arena = p_next + J.PC;
    head = arena + J.R; tslots = head + J.n_states; pslots = tslots + J.HS;
  }
};

// a tuple that may not be in the table yet: pending ids = a ++ b, pending words = w (+ one more)
struct Cand {
  int32_t in, hash;
  const int32_t *a, *b, *w;
  int32_t la, lb, lw, extra;   // extra: the word appended behind w (0 = none)
  int32_t share_toff, share_woff;   // >= 0: the strings are a suffix of an existing tuple's (b and extra are empty)
};

__host__ __device__ inline float AsFloat(int32_t b) { float f; memcpy(&f, &b, 4); return f; }
__host__ __device__ inline int32_t AsBits(float f) { int32_t b; memcpy(&b, &f, 4); return b; }

// Compare of fstext/lattice-weight.h:295-308 decides; where it returns 0 and the acoustic costs still differ (the sums
// round alike), the smaller acoustic cost wins, so that Plus does not depend on the order of its arguments.
__host__ __device__ inline bool Better(float g1, float a1, float g2, float a2) {
  const float f1 = g1 + a1, f2 = g2 + a2;
  if (f1 < f2) return true;
  if (f1 > f2) return false;
  if (g1 < g2) return true;
  if (g1 > g2) return false;
  return a1 < a2;
}

__host__ __device__ inline int32_t HashCand(const Cand &c) {
  uint32_t h = 2166136261u ^ (static_cast<uint32_t>(c.in) * 0x9E3779B1u);
  for (int i = 0; i < c.la; i++) h = (h ^ static_cast<uint32_t>(c.a[i])) * 16777619u;
  for (int i = 0; i < c.lb; i++) h = (h ^ static_cast<uint32_t>(c.b[i])) * 16777619u;
  h = (h ^ 0x5bd1e995u) * 16777619u;
  for (int i = 0; i < c.lw; i++) h = (h ^ static_cast<uint32_t>(c.w[i])) * 16777619u;
  if (c.extra) h = (h ^ static_cast<uint32_t>(c.extra)) * 16777619u;
  return static_cast<int32_t>(h & 0x7fffffffu);
}

// the tuple's number, or -1 - slot of the first empty slot met, or INT32_MIN when the table holds no empty slot
__host__ __device__ inline int32_t FindTuple(const View &V, const AlignJob &J, const Cand &c) {
  const int32_t mask = J.HS - 1, lt = c.la + c.lb, lw = c.lw + (c.extra ? 1 : 0);
  int32_t slot = c.hash & mask;
  for (int32_t probe = 0; probe < J.HS; probe++, slot = (slot + 1) & mask) {
    const int32_t t = V.tslots[slot];
    if (t < 0) return -1 - slot;
    if (V.t_hash[t] != c.hash || V.t_in[t] != c.in || V.t_tlen[t] != lt || V.t_wlen[t] != lw) continue;
    const int32_t *pt = V.arena + V.t_toff[t], *pw = V.arena + V.t_woff[t];
    bool same = true;
    for (int i = 0; same && i < c.la; i++) same = pt[i] == c.a[i];
    for (int i = 0; same && i < c.lb; i++) same = pt[c.la + i] == c.b[i];
    for (int i = 0; same && i < c.lw; i++) same = pw[i] == c.w[i];
    if (same && c.extra) same = pw[c.lw] == c.extra;
    if (same) return t;
  }
  return std::numeric_limits<int32_t>::min();
}

// One lane at a time.  -1 with hdr[0] set when the lattice cannot go on.
__host__ __device__ inline int32_t InsertTuple(const View &V, const AlignJob &J, const Cand &c) {
  const int32_t f = FindTuple(V, J, c);
  if (f >= 0) return f;
  const int32_t lt = c.la + c.lb, lw = c.lw + (c.extra ? 1 : 0);
  const int32_t need = c.share_toff >= 0 ? 0 : lt + lw;
  const int32_t n = V.hdr[1], used = V.hdr[3];
  if (f == std::numeric_limits<int32_t>::min() || n >= J.C || need > J.R - used) {
    V.hdr[0] = kNeedsRoom;
    return -1;
  }
  int32_t toff = c.share_toff, woff = c.share_woff;
  if (toff < 0) {
    toff = used;
    woff = used + lt;
    int32_t *pt = V.arena + toff, *pw = V.arena + woff;
    for (int i = 0; i < c.la; i++) pt[i] = c.a[i];
    for (int i = 0; i < c.lb; i++) pt[c.la + i] = c.b[i];
    for (int i = 0; i < c.lw; i++) pw[i] = c.w[i];
    if (c.extra) pw[c.lw] = c.extra;
    V.hdr[3] = used + need;
  }
  V.t_in[n] = c.in; V.t_toff[n] = toff; V.t_tlen[n] = lt; V.t_woff[n] = woff; V.t_wlen[n] = lw; V.t_hash[n] = c.hash;
  V.tslots[-1 - f] = n;
  V.hdr[1] = n + 1;
  if (J.max_states > 0 && n + 1 > J.max_states) {   // :315: the tuple that pushes the count over
    V.hdr[0] = kTooMany;
    return -1;
  }
  return n;
}

// One lane at a time: d(S, T) = Plus(d(S, T), (g, a)); a new pair is chained onto T's input state.
__host__ __device__ inline void RelaxPair(const View &V, const AlignJob &J, int32_t S, int32_t T, float g, float a) {
  const int32_t mask = J.PS - 1;
  int32_t slot = static_cast<int32_t>((static_cast<uint32_t>(S) * 0x9E3779B1u) ^ (static_cast<uint32_t>(T) * 0x85EBCA6Bu)) & mask;
  for (int32_t probe = 0; probe < J.PS; probe++, slot = (slot + 1) & mask) {
    const int32_t p = V.pslots[slot];
    if (p < 0) {
      const int32_t n = V.hdr[2];
      if (n >= J.PC) break;
      V.p_S[n] = S; V.p_T[n] = T; V.p_g[n] = AsBits(g); V.p_a[n] = AsBits(a);
      const int32_t level = V.t_in[T];
      V.p_next[n] = V.head[level];
      V.head[level] = n;
      V.pslots[slot] = n;
      V.hdr[2] = n + 1;
      return;
    }
    if (V.p_S[p] == S && V.p_T[p] == T) {
      if (Better(g, a, AsFloat(V.p_g[p]), AsFloat(V.p_a[p]))) { V.p_g[p] = AsBits(g); V.p_a[p] = AsBits(a); }
      return;
    }
  }
  V.hdr[0] = kNeedsRoom;
}

// ProcessQueueElement's decision for one tuple (:201-250): OutputArc (:59-69; the three cases are disjoint by the type of
// the first pending phone), else on the final state ProcessFinal (:172-198) with OutputArcForce (:554-635), else epsilons.
// error = the conditions that set error_ (an OR, so the order of visits does not matter; :375-379 and :406-410 only warn);
// fatal = the KALDI_ERR of :595-603.
__host__ __device__ inline void Classify(const AlignCtx &X, const AlignJob &J, int32_t in, const int32_t *tids, int32_t len,
                                         const int32_t *words, int32_t wlen, int32_t *kind, int32_t *consume,
                                         int32_t *wdrop, int32_t *label, bool *error, bool *fatal) {
#define KH_PHONE(i) (X.tinfo[tids[i]] & kPhoneMask)
#define KH_FINAL(i) ((X.tinfo[tids[i]] & kFinalBit) != 0)
#define KH_SELF(i) ((X.tinfo[tids[i]] & kSelfBit) != 0)
  *kind = kKindEps; *consume = 0; *wdrop = 0; *label = 0;
  bool out = false;
  int32_t i = 0;
  if (len > 0) {
    const int32_t phone = KH_PHONE(0), type = X.ptype[phone];
    if (type == kWordBeginPhone && wlen > 0) {                     // OutputNormalWordArc :443-528
      do {
        for (i = 0; i < len && !KH_FINAL(i); i++) {}
        if (i == len) break;
        i++;
        if (X.reorder) for (; i < len && KH_SELF(i); i++) {}
        if (i == len) break;
        if (KH_PHONE(i - 1) != phone) *error = true;               // :464-469
        for (; i < len; i++) {
          const int32_t tp = X.ptype[KH_PHONE(i)];
          if (tp == kWordEndPhone) break;
          if (tp != kWordInternalPhone) *error = true;             // :478-483
        }
        if (i == len) break;
        const int32_t final_phone = KH_PHONE(i);
        for (; i < len; i++) {
          if (KH_PHONE(i) != final_phone) *error = true;           // :494-498
          if (KH_FINAL(i)) break;
        }
        if (i == len) break;
        i++;
        if (X.reorder) while (i < len && KH_SELF(i)) i++;
        if (i == len) break;
        if (KH_PHONE(i - 1) != final_phone) *error = true;         // :508-513
        out = true; *label = words[0]; *wdrop = 1;
      } while (false);
    } else if (type == kNonWordPhone) {                            // OutputSilenceArc :346-389
      do {
        for (i = 1; i < len; i++) {
          if (KH_PHONE(i) != phone) *error = true;                 // :361-365
          if (KH_FINAL(i)) break;
        }
        if (i == len) break;
        i++;
        if (X.reorder) while (i < len && KH_SELF(i)) i++;
        if (i == len) break;
        out = true; *label = J.sil;
      } while (false);
    } else if (type == kWordBeginAndEndPhone && wlen > 0) {        // OutputOnePhoneWordArc :392-438
      do {
        for (i = 1; i < len; i++) if (KH_FINAL(i)) break;
        if (i == len) break;
        i++;
        if (X.reorder) while (i < len && KH_SELF(i)) i++;
        if (i == len) break;
        if (KH_PHONE(i - 1) != phone) *error = true;               // :420-425
        out = true; *label = words[0]; *wdrop = 1;
      } while (false);
    }
  }
  if (out) {
    *kind = kKindOut;
    *consume = i;
    return;
  }
  if (in != J.sf) return;
  if (len == 0 && wlen == 0) {                                     // :177-181
    *kind = kKindFinal;
    return;
  }
  *kind = kKindForce;
  *consume = len;
  if (wlen > 0 && len > 0) {                                       // :559-573
    const int32_t first = KH_PHONE(0), last = KH_PHONE(len - 1);
    bool plausible = false;                                        // IsPlausibleWord :532-551
    if ((X.ptype[first] == kWordBeginAndEndPhone && first == last) ||
        (X.ptype[first] == kWordBeginPhone && X.ptype[last] == kWordEndPhone)) {
      int32_t k = len - 1;
      if (X.reorder) while (k > 0 && KH_SELF(k)) k--;
      plausible = KH_FINAL(k);
    }
    if (!plausible) *error = true;
    *label = words[0]; *wdrop = 1;
  } else if (wlen > 0) {                                           // :574-589: the word labels are discarded
    *error = true;
    *label = 0; *wdrop = wlen;
  } else {                                                         // :590-630
    const int32_t first = KH_PHONE(0);
    if (X.ptype[first] == kNonWordPhone) {
      if (first != KH_PHONE(len - 1)) {
        *fatal = true;                                             // :595-603
      } else {
        int32_t k = len - 1;
        if (X.reorder) while (KH_SELF(k) && k > 0) k--;
        if (!KH_FINAL(k)) *error = true;                           // :604-613
      }
      *label = J.sil;
    } else {
      *error = true;                                               // :621-624
      *label = J.partial;
    }
  }
#undef KH_PHONE
#undef KH_FINAL
#undef KH_SELF
}

// WaveFence(): the tables are written by one lane and read by the others of the same wave later in program order.  The
// device pass takes kh::WaveFence (kh_latbatch.h); on the host pass the stub below, declared in this inner namespace,
// hides that __device__ function for AlignBody, which a host program steps through with one lane.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ unsigned long long Ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int32_t FromLane(int32_t v, int l) { return __shfl(v, l); }
__device__ __forceinline__ int FirstBit(unsigned long long m) { return __ffsll(static_cast<long long>(m)) - 1; }
#else
inline void WaveFence() {}
inline unsigned long long Ballot(bool p) { return p ? 1ull : 0ull; }
inline int32_t FromLane(int32_t v, int) { return v; }
inline int FirstBit(unsigned long long m) { return m ? 0 : -1; }
#endif

// The whole construction of one lattice by n_lanes lanes in lock step (64 on the device; 1 when a host program steps
// through the same statements).
__host__ __device__ inline void AlignBody(const AlignJob &J, const AlignCtx &X, int lane, int n_lanes) {
  const View V(X.ws + J.hdr_off, X.ws + J.ws_off, J);
  volatile int32_t *hdr = V.hdr;
  volatile int32_t *head = V.head;
  const int32_t *aoff = X.arc_off + J.state_base;
  // -1 = empty / not yet known: chain heads and both slot tables (they lie together), every tuple's kind and destination
  const int32_t n_slots = J.n_states + J.HS + J.PS;
  for (int32_t i = lane; i < n_slots; i += n_lanes) V.head[i] = -1;
  for (int32_t i = lane; i < J.C; i += n_lanes) {
    V.t_kind[i] = -1;
    V.t_dest[i] = -1;
  }
  if (lane == 0) for (int i = 0; i < kHdr; i++) V.hdr[i] = 0;
  WaveFence();
  if (lane == 0) {
    Cand c{J.start, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0, -1, -1};
    c.hash = HashCand(c);
    const int32_t t = InsertTuple(V, J, c);                        // :309-312
    if (t >= 0) RelaxPair(V, J, t, t, 0.f, 0.f);
  }
  WaveFence();
  if (hdr[0] != 0) return;
  for (int32_t s = 0; s < J.n_states; s++) {
    for (int32_t round = 0; round <= J.PC; round++) {
      const int32_t h0 = head[s];
      if (h0 < 0) break;
      int32_t mine = h0;                                           // lane k takes the k-th pair of the chain
      for (int hop = 0; hop < lane && mine >= 0; hop++) mine = V.p_next[mine];
      const int32_t rest = FromLane(mine >= 0 ? V.p_next[mine] : -1, n_lanes - 1);
      WaveFence();
      if (lane == 0) head[s] = rest;
      WaveFence();
      int32_t S = -1, T = -1, kind = -1, steps = 0;
      float g = 0.f, a = 0.f;
      if (mine >= 0) {
        S = V.p_S[mine]; T = V.p_T[mine]; g = AsFloat(V.p_g[mine]); a = AsFloat(V.p_a[mine]);
        kind = V.t_kind[T];
        if (kind < 0) {
          int32_t consume, wdrop, label;
          bool error = false, fatal = false;
          Classify(X, J, s, V.arena + V.t_toff[T], V.t_tlen[T], V.arena + V.t_woff[T], V.t_wlen[T], &kind, &consume, &wdrop,
                   &label, &error, &fatal);
          V.t_consume[T] = consume; V.t_wdrop[T] = wdrop; V.t_label[T] = label; V.t_kind[T] = kind;
          if (error) hdr[4] = 1;
          if (fatal) hdr[5] = 1;
        }
        steps = kind == kKindEps ? aoff[s + 1] - aoff[s] : (kind == kKindFinal ? 0 : 1);
      }
      WaveFence();
      for (int32_t j = 0; Ballot(j < steps) != 0ull; j++) {
        const bool active = j < steps;
        Cand c{s, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0, -1, -1};
        int32_t found = -1, arc = -1;
        if (active) {
          const int32_t toff = V.t_toff[T], tlen = V.t_tlen[T], woff = V.t_woff[T], wlen = V.t_wlen[T];
          if (kind == kKindEps) {                                  // Advance :40-48
            arc = aoff[s] + j;
            c.in = X.arc_next[arc];
            c.a = V.arena + toff; c.la = tlen;
            c.b = X.strings + X.str_off[arc]; c.lb = X.str_off[arc + 1] - X.str_off[arc];
            c.w = V.arena + woff; c.lw = wlen;
            c.extra = X.arc_label[arc];
          } else {                                                 // what the labelled arc leaves pending
            const int32_t consume = V.t_consume[T], wdrop = V.t_wdrop[T];
            c.a = V.arena + toff + consume; c.la = tlen - consume;
            c.w = V.arena + woff + wdrop; c.lw = wlen - wdrop;
            c.share_toff = toff + consume; c.share_woff = woff + wdrop;
          }
          c.hash = HashCand(c);
          found = FindTuple(V, J, c);
        }
        unsigned long long turn = Ballot(active);
        while (turn != 0ull) {
          const int l = FirstBit(turn);
          turn &= turn - 1ull;
          if (lane == l && hdr[0] == 0) {
            const int32_t t = found >= 0 ? found : InsertTuple(V, J, c);
            if (t >= 0) {
              if (kind == kKindEps) {
                RelaxPair(V, J, S, t, g + X.arc_g[arc], a + X.arc_a[arc]);
              } else {
                V.t_dest[T] = t;
                RelaxPair(V, J, t, t, 0.f, 0.f);
              }
            }
          }
          WaveFence();
        }
        if (hdr[0] != 0) return;
      }
    }
    if (head[s] >= 0) {                                            // cannot happen with PC pairs; never spin
      if (lane == 0) hdr[0] = kNeedsRoom;
      WaveFence();
      return;
    }
  }
}

__global__ __launch_bounds__(kLanes) void AlignKernel(const AlignJob *__restrict__ jobs, AlignCtx X) {
  const AlignJob J = jobs[blockIdx.x];
  AlignBody(J, X, static_cast<int>(threadIdx.x), kLanes);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct Prepared {
  int n_lats = 0;
  std::vector<int32_t> soff;                  // per lattice (+1): states after CreateSuperFinal
  std::vector<int32_t> arc_off, arc_label, arc_next, str_off, strings, state_time, tinfo, ptype;
  std::vector<float> arc_g, arc_a;
  std::vector<AlignJob> jobs;                 // one per lattice with a start state
  std::vector<int32_t> job_of_lat;            // -1: empty lattice
  std::vector<int64_t> string_words;          // per lattice: transition-ids of the input
  int32_t reorder = 0, sil_in = 0, partial_in = 0;
};

struct OutLat {
  int32_t status = 0, n_tuples = 0;
  std::vector<float> final_g, final_a;
  std::vector<int32_t> arc_src, arc_dst, arc_label, arc_len, strings;
  std::vector<float> arc_g, arc_a;
};

inline int32_t Pow2AtLeast(int64_t x) {
  int32_t p = 16;
  while (p < x && p < (1 << 30)) p <<= 1;
  return p;
}

inline void SetRoom(AlignJob *J, int64_t C, int64_t PC, int64_t R) {
  if (J->max_states > 0) C = std::min<int64_t>(C, static_cast<int64_t>(J->max_states) + 1);
  const int64_t cap = (1ll << 28);
  J->C = static_cast<int32_t>(std::min(C, cap));
  J->PC = static_cast<int32_t>(std::min(PC, cap));
  J->R = static_cast<int32_t>(std::min(R, 4 * cap));
  J->HS = Pow2AtLeast(2ll * J->C);
  J->PS = Pow2AtLeast(2ll * J->PC);
}

// Validation, CreateSuperFinal (fstext/fstext-utils-inl.h), the labels of :275-282, state times.
int Prepare(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start, const int64_t *arc_offsets,
            const int32_t *arc_label, const int32_t *arc_nextstate, const float *arc_graph, const float *arc_acoustic,
            const int64_t *arc_string_offsets, const int32_t *arc_strings, const float *final_graph,
            const float *final_acoustic, const int64_t *final_string_offsets, const int32_t *final_strings, int num_tids,
            const int32_t *tid_phone, const int32_t *tid_is_final, const int32_t *tid_is_self_loop, int n_phone_types,
            const int32_t *phone_type, int reorder, int silence_label, int partial_word_label, const int32_t *max_states,
            Prepared *P) {
  const char *me = "kh_compact_lattice_align_words";
  const float inf = std::numeric_limits<float>::infinity();
  P->n_lats = n_lats;
  P->reorder = reorder ? 1 : 0;
  P->sil_in = silence_label;
  P->partial_in = partial_word_label;
  P->ptype.assign(phone_type, phone_type + n_phone_types);
  for (int p = 0; p < n_phone_types; p++) {
    if (phone_type[p] < kNoPhone || phone_type[p] > kNonWordPhone) {
      SetError("%s: phone %d: type %d is not one of WordBoundaryInfo::PhoneType", me, p, phone_type[p]);
      return KH_EINVAL;
    }
  }
  P->tinfo.assign(static_cast<size_t>(num_tids) + 1, 0);
  for (int t = 1; t <= num_tids; t++) {
    if (tid_phone[t] < 0 || tid_phone[t] >= n_phone_types) {       // TypeOfPhone :147-152
      SetError("%s: transition-id %d: phone %d was not specified in the word-boundary table of %d entries", me, t,
               tid_phone[t], n_phone_types);
      return KH_EINVAL;
    }
    P->tinfo[t] = tid_phone[t] | (tid_is_final[t] ? kFinalBit : 0) | (tid_is_self_loop[t] ? kSelfBit : 0);
  }
  const int64_t S = lat_state_offsets[n_lats], A = arc_offsets[S];
  KH_CHECK_ARG(A >= 0 && A < (1ll << 30) && arc_string_offsets[0] == 0 && final_string_offsets[0] == 0);
  KH_CHECK_ARG(arc_string_offsets[A] + final_string_offsets[S] < (1ll << 30));
  P->soff.assign(1, 0);
  P->arc_off.assign(1, 0);
  P->str_off.assign(1, 0);
  P->job_of_lat.assign(n_lats, -1);
  P->string_words.assign(n_lats, 0);
  auto check_string = [&](const int32_t *s, int64_t b, int64_t e, int l, const char *what, long long which) {
    if (e < b) {
      SetError("%s: lattice %d: %s %lld: string offsets descend", me, l, what, which);
      return false;
    }
    for (int64_t i = b; i < e; i++) {
      if (s[i] < 1 || s[i] > num_tids) {
        SetError("%s: lattice %d: %s %lld: transition-id %d of a model with %d", me, l, what, which, s[i], num_tids);
        return false;
      }
    }
    return true;
  };
  for (int l = 0; l < n_lats; l++) {
    const int32_t s0 = lat_state_offsets[l], N = lat_state_offsets[l + 1] - s0;
    if (N < 0 || lat_start[l] >= N) {
      SetError("%s: lattice %d: %d states, start state %d", me, l, N, lat_start[l]);
      return KH_EINVAL;
    }
    const int64_t a0 = arc_offsets[s0];
    for (int32_t s = 0; s < N; s++) {
      if (arc_offsets[s0 + s + 1] < arc_offsets[s0 + s] || arc_offsets[s0 + s + 1] > A) {
        SetError("%s: lattice %d: state %d: arc_offsets %lld, %lld of %lld arcs: the offsets must ascend", me, l, s,
                 static_cast<long long>(arc_offsets[s0 + s]), static_cast<long long>(arc_offsets[s0 + s + 1]), static_cast<long long>(A));
        return KH_EINVAL;
      }
    }
    const bool has_start = N > 0 && lat_start[l] >= 0;
    // CreateSuperFinal: a single final state with weight One, an empty string and no arcs is used as it is
    std::vector<int32_t> finals;
    int32_t highest = 0;
    for (int32_t s = 0; s < N && has_start; s++) {
      const float fg = final_graph[s0 + s], fa = final_acoustic[s0 + s];
      if (fg != fg || fa != fa || fg == -inf || fa == -inf) {
        SetError("%s: lattice %d: state %d: final weight %g, %g: NaN and -inf are not taken", me, l, s, fg, fa);
        return KH_EINVAL;
      }
      if (!(fg == inf && fa == inf)) finals.push_back(s);
      if (!check_string(final_strings, final_string_offsets[s0 + s], final_string_offsets[s0 + s + 1], l, "final state", s))
        return KH_EINVAL;
    }
    bool single = false;
    if (finals.size() == 1) {
      const int32_t f = finals[0];
      single = final_graph[s0 + f] == 0.f && final_acoustic[s0 + f] == 0.f &&
               final_string_offsets[s0 + f + 1] == final_string_offsets[s0 + f] && arc_offsets[s0 + f + 1] == arc_offsets[s0 + f];
    }
    const int32_t N2 = has_start ? (single ? N : N + 1) : 0, sf = has_start ? (single ? finals[0] : N) : -1;
    int64_t words = 0;
    for (int32_t s = 0; s < N && has_start; s++) {
      for (int64_t a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; a++) {
        const int32_t d = arc_nextstate[a];
        if (d <= s || d >= N) {
          SetError("%s: lattice %d: arc %lld (state %d -> %d of %d): the lattice must be top-sorted", me, l,
                   static_cast<long long>(a - a0), s, d, N);
          return KH_EINVAL;
        }
        const float g = arc_graph[a], ac = arc_acoustic[a];
        if (g != g || ac != ac || g == -inf || ac == -inf) {
          SetError("%s: lattice %d: arc %lld (state %d -> %d): weight %g, %g: NaN and -inf are not taken", me, l,
                   static_cast<long long>(a - a0), s, d, g, ac);
          return KH_EINVAL;
        }
        if (arc_label[a] < 0) {
          SetError("%s: lattice %d: arc %lld: label %d", me, l, static_cast<long long>(a - a0), arc_label[a]);
          return KH_EINVAL;
        }
        if (!check_string(arc_strings, arc_string_offsets[a], arc_string_offsets[a + 1], l, "arc", a - a0)) return KH_EINVAL;
        highest = std::max(highest, arc_label[a]);
        P->arc_label.push_back(arc_label[a]);
        P->arc_next.push_back(d);
        P->arc_g.push_back(g);
        P->arc_a.push_back(ac);
        P->strings.insert(P->strings.end(), arc_strings + arc_string_offsets[a], arc_strings + arc_string_offsets[a + 1]);
        P->str_off.push_back(static_cast<int32_t>(P->strings.size()));
        words += arc_string_offsets[a + 1] - arc_string_offsets[a];
      }
      if (!single && !(final_graph[s0 + s] == inf && final_acoustic[s0 + s] == inf)) {   // the arc to the new final state
        P->arc_label.push_back(0);
        P->arc_next.push_back(N);
        P->arc_g.push_back(final_graph[s0 + s]);
        P->arc_a.push_back(final_acoustic[s0 + s]);
        P->strings.insert(P->strings.end(), final_strings + final_string_offsets[s0 + s],
                          final_strings + final_string_offsets[s0 + s + 1]);
        P->str_off.push_back(static_cast<int32_t>(P->strings.size()));
        words += final_string_offsets[s0 + s + 1] - final_string_offsets[s0 + s];
      }
      P->arc_off.push_back(static_cast<int32_t>(P->arc_label.size()));
    }
    if (has_start && !single) P->arc_off.push_back(static_cast<int32_t>(P->arc_label.size()));
    P->string_words[l] = words;
    const int32_t base = P->soff.back();
    P->soff.push_back(base + N2);
    if (!has_start) continue;
    // state times: every path to a state reachable from the start consumes the same number of transition-ids
    P->state_time.resize(static_cast<size_t>(base) + N2, -1);
    int32_t *tm = P->state_time.data() + base;
    tm[lat_start[l]] = 0;
    for (int32_t s = 0; s < N2; s++) {
      if (tm[s] < 0) continue;
      for (int32_t a = P->arc_off[base + s]; a < P->arc_off[base + s + 1]; a++) {
        const int32_t d = P->arc_next[a], t = tm[s] + (P->str_off[a + 1] - P->str_off[a]);
        if (tm[d] >= 0 && tm[d] != t) {
          SetError("%s: lattice %d: state %d is reached after %d and after %d transition-ids: the state times are not "
                   "consistent", me, l, d, tm[d], t);
          return KH_EINVAL;
        }
        tm[d] = t;
      }
    }
    AlignJob J;
    memset(&J, 0, sizeof(J));
    J.state_base = base;
    J.n_states = N2;
    J.start = lat_start[l];
    J.sf = sf;
    J.max_states = max_states ? max_states[l] : 0;
    const int32_t unused = 1 + highest;                            // :275-282
    J.sil = silence_label == 0 ? unused : silence_label;
    J.partial = partial_word_label == 0 ? unused : partial_word_label;
    J.lat = l;
    const int64_t n_arcs = P->arc_off[base + N2] - P->arc_off[base];
    SetRoom(&J, 4 * (N2 + n_arcs) + 64, 8 * (N2 + n_arcs) + 128, 4 * words + 16 * (N2 + n_arcs) + 256);
    P->job_of_lat[l] = static_cast<int32_t>(P->jobs.size());
    P->jobs.push_back(J);
  }
  return KH_OK;
}

struct OutArc {
  int32_t dst, label, toff, len;
  float g, a;
};

// Compare of CompactLatticeWeight (fstext/lattice-weight.h:562-576) with Better() on the weights: is x better than y?
inline bool BetterArc(const OutArc &x, const OutArc &y, const int32_t *arena) {
  if (Better(x.g, x.a, y.g, y.a)) return true;
  if (Better(y.g, y.a, x.g, x.a)) return false;
  if (x.len != y.len) return x.len < y.len;
  for (int i = 0; i < x.len; i++) {
    if (arena[x.toff + i] != arena[y.toff + i]) return arena[x.toff + i] > arena[y.toff + i];
  }
  return false;
}

// From a finished lattice's tables to the numbered result.
void Finish(const Prepared &P, const AlignJob &J, const int32_t *hdr, const int32_t *ws, OutLat *O) {
  const View V(const_cast<int32_t *>(hdr), const_cast<int32_t *>(ws), J);
  const float inf = std::numeric_limits<float>::infinity();
  const int32_t n_tuples = V.hdr[1], n_pairs = V.hdr[2];
  O->n_tuples = n_tuples;
  O->status = V.hdr[5] ? KH_ALIGN_FATAL : (V.hdr[4] ? KH_ALIGN_ERROR : KH_ALIGN_OK);
  if (O->status == KH_ALIGN_FATAL) return;
  const int32_t *tm = P.state_time.data() + J.state_base;
  std::vector<int32_t> num(n_tuples, -1), states;                  // output states: the S of the pairs
  for (int32_t p = 0; p < n_pairs; p++) {
    if (num[V.p_S[p]] < 0) {
      num[V.p_S[p]] = 0;
      states.push_back(V.p_S[p]);
    }
  }
  auto key_less = [&](int32_t x, int32_t y) {
    if (x == 0 || y == 0) return x == 0 && y != 0;                 // the start tuple is tuple 0 and becomes state 0
    const int32_t tx = tm[V.t_in[x]] - V.t_tlen[x], ty = tm[V.t_in[y]] - V.t_tlen[y];
    if (tx != ty) return tx < ty;
    if (V.t_in[x] != V.t_in[y]) return V.t_in[x] < V.t_in[y];
    if (V.t_wlen[x] != V.t_wlen[y]) return V.t_wlen[x] > V.t_wlen[y];
    const int32_t *wx = V.arena + V.t_woff[x], *wy = V.arena + V.t_woff[y];
    if (!std::equal(wx, wx + V.t_wlen[x], wy)) return std::lexicographical_compare(wx, wx + V.t_wlen[x], wy, wy + V.t_wlen[y]);
    const int32_t *px = V.arena + V.t_toff[x], *py = V.arena + V.t_toff[y];
    return std::lexicographical_compare(px, px + V.t_tlen[x], py, py + V.t_tlen[y]);
  };
  std::sort(states.begin(), states.end(), key_less);
  const int32_t n = static_cast<int32_t>(states.size());
  for (int32_t i = 0; i < n; i++) num[states[i]] = i;
  std::vector<std::vector<OutArc>> arcs(n);
  std::vector<float> fg(n, inf), fa(n, inf);
  for (int32_t p = 0; p < n_pairs; p++) {
    const int32_t s = num[V.p_S[p]], T = V.p_T[p], kind = V.t_kind[T];
    const float g = AsFloat(V.p_g[p]), a = AsFloat(V.p_a[p]);
    if (kind == kKindFinal) {
      if (Better(g, a, fg[s], fa[s])) { fg[s] = g; fa[s] = a; }
    } else if (kind == kKindOut || kind == kKindForce) {
      arcs[s].push_back(OutArc{num[V.t_dest[T]], V.t_label[T], V.t_toff[T], V.t_consume[T], g, a});
    }
  }
  std::vector<char> keep(n, 0);                                    // the key is a topological order
  for (int32_t s = n - 1; s >= 0; s--) {
    keep[s] = !(fg[s] == inf && fa[s] == inf);
    for (const OutArc &x : arcs[s]) keep[s] = keep[s] || keep[x.dst];
  }
  if (n == 0 || !keep[0]) return;
  std::vector<int32_t> renum(n, -1);
  int32_t m = 0;
  for (int32_t s = 0; s < n; s++) if (keep[s]) renum[s] = m++;
  O->final_g.reserve(m);
  for (int32_t s = 0; s < n; s++) {
    if (!keep[s]) continue;
    O->final_g.push_back(fg[s]);
    O->final_a.push_back(fa[s]);
    std::vector<OutArc> &v = arcs[s];
    v.erase(std::remove_if(v.begin(), v.end(), [&](const OutArc &x) { return !keep[x.dst]; }), v.end());
    std::stable_sort(v.begin(), v.end(), [&](const OutArc &x, const OutArc &y) {
      if (x.dst != y.dst) return x.dst < y.dst;
      if (x.label != y.label) return x.label < y.label;
      return BetterArc(x, y, V.arena);
    });
    for (size_t i = 0; i < v.size(); i++) {
      if (i > 0 && v[i].dst == v[i - 1].dst && v[i].label == v[i - 1].label) continue;   // Plus: the better one came first
      const OutArc &x = v[i];
      int32_t label = x.label;                                     // RemoveEpsilonsFromLattice :292-300
      if ((P.sil_in == 0 && label == J.sil) || (P.partial_in == 0 && label == J.partial)) label = 0;
      O->arc_src.push_back(renum[s]);
      O->arc_dst.push_back(renum[x.dst]);
      O->arc_label.push_back(label);
      O->arc_g.push_back(x.g);
      O->arc_a.push_back(x.a);
      O->arc_len.push_back(x.len);
      O->strings.insert(O->strings.end(), V.arena + x.toff, V.arena + x.toff + x.len);
    }
  }
}

// ms[5]: the host's finishing pass; counts: launches, lattices run again with more room, tuples over all lattices
static thread_local CallStats<6, 3> g_stats;

}  // namespace latalign
}  // namespace kh

using namespace kh;
using namespace kh::latalign;

extern "C" int kh_compact_lattice_align_words_set_workspace_limit(size_t bytes) {
  g_stats.workspace_limit = bytes;
  return KH_OK;
}

extern "C" int kh_compact_lattice_align_words_last_timings(float *ms6, int32_t *counts3) {
  return GetTimings(g_stats, ms6, counts3);
}

extern "C" int kh_compact_lattice_align_words(
    int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start, const int64_t *arc_offsets,
    const int32_t *arc_label, const int32_t *arc_nextstate, const float *arc_graph, const float *arc_acoustic,
    const int64_t *arc_string_offsets, const int32_t *arc_strings, const float *final_graph, const float *final_acoustic,
    const int64_t *final_string_offsets, const int32_t *final_strings, int num_tids, const int32_t *tid_phone,
    const int32_t *tid_is_final, const int32_t *tid_is_self_loop, int n_phone_types, const int32_t *phone_type, int reorder,
    int silence_label, int partial_word_label, const int32_t *max_states, int32_t *status, int32_t *n_states,
    int32_t *n_arcs, int32_t *n_tuples, int64_t *n_string_words, const int64_t *out_state_offsets,
    const int64_t *out_arc_offsets, const int64_t *out_string_offsets, float *out_final_graph, float *out_final_acoustic,
    int32_t *out_arc_src, int32_t *out_arc_nextstate, int32_t *out_arc_label, float *out_arc_graph, float *out_arc_acoustic,
    int32_t *out_arc_string_len, int32_t *out_strings) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(n_lats > 0 && lat_state_offsets && lat_start && arc_offsets && arc_label && arc_nextstate && arc_graph &&
               arc_acoustic && arc_string_offsets && arc_strings && final_graph && final_acoustic && final_string_offsets &&
               final_strings && num_tids > 0 && tid_phone && tid_is_final && tid_is_self_loop && n_phone_types > 0 &&
               phone_type && status && n_states && n_arcs && n_tuples && n_string_words && out_state_offsets &&
               out_arc_offsets && out_string_offsets && out_final_graph && out_final_acoustic && out_arc_src &&
               out_arc_nextstate && out_arc_label && out_arc_graph && out_arc_acoustic && out_arc_string_len && out_strings);
  KH_CHECK_ARG(lat_state_offsets[0] == 0 && arc_offsets[0] == 0 && out_state_offsets[0] == 0 && out_arc_offsets[0] == 0 &&
               out_string_offsets[0] == 0 && silence_label >= 0 && partial_word_label >= 0);
  CallTimer T;
  Prepared P;
  if ((rc = Prepare(n_lats, lat_state_offsets, lat_start, arc_offsets, arc_label, arc_nextstate, arc_graph, arc_acoustic,
                    arc_string_offsets, arc_strings, final_graph, final_acoustic, final_string_offsets, final_strings,
                    num_tids, tid_phone, tid_is_final, tid_is_self_loop, n_phone_types, phone_type, reorder, silence_label,
                    partial_word_label, max_states, &P)) != KH_OK)
    return rc;
  T.HostDone();
  std::vector<OutLat> outs(n_lats);
  for (int l = 0; l < n_lats; l++) outs[l].status = P.job_of_lat[l] < 0 ? KH_ALIGN_EMPTY : KH_ALIGN_OK;
  double ms_finish = 0.0;
  int32_t n_launches = 0, n_again = 0;
  if (!P.jobs.empty()) {
    hipStream_t st = Stream();
    KH_HIP(T.Init());
    Dev<int32_t> d_arc_off, d_label, d_next, d_str_off, d_strings, d_tinfo, d_ptype, d_ws;
    Dev<float> d_g, d_a;
    Dev<AlignJob> d_jobs;
    KH_HIP(T.Mark(0, st));
    if (d_arc_off.Upload(P.arc_off, st) || d_label.Upload(P.arc_label, st) || d_next.Upload(P.arc_next, st) ||
        d_str_off.Upload(P.str_off, st) || d_strings.Upload(P.strings, st) || d_tinfo.Upload(P.tinfo, st) ||
        d_ptype.Upload(P.ptype, st) || d_g.Upload(P.arc_g, st) || d_a.Upload(P.arc_a, st)) {
      SetError("kh_compact_lattice_align_words: out of device memory");
      return KH_ENOMEM;
    }
    KH_HIP(T.Mark(1, st));
    KH_HIP(hipStreamSynchronize(st));
    KH_HIP(T.Add(&T.up, 0, 1));
    size_t limit = g_stats.workspace_limit;   // by default half of what is free: nothing else of this call is allocated later
    if (limit == 0 && (rc = DefaultWorkspaceLimit(0, &limit)) != KH_OK) return rc;
    std::vector<int32_t> todo(P.jobs.size());
    std::iota(todo.begin(), todo.end(), 0);
    std::vector<int32_t> h_ws;
    std::vector<AlignJob> batch;
    for (int attempt = 0; !todo.empty(); attempt++) {
      if (attempt > 24) {
        SetError("kh_compact_lattice_align_words: lattice %d still needs more room after %d attempts", P.jobs[todo[0]].lat, attempt);
        return KH_ENOMEM;
      }
      // largest first, as many per launch as the workspace limit admits (one always runs)
      std::stable_sort(todo.begin(), todo.end(), [&](int32_t x, int32_t y) { return WorkspaceWords(P.jobs[x]) > WorkspaceWords(P.jobs[y]); });
      std::vector<int32_t> again;
      for (size_t i = 0; i < todo.size();) {
        batch.clear();
        size_t words = 0;
        size_t e = i;
        while (e < todo.size() && e - i < 65535) {
          AlignJob &J = P.jobs[todo[e]];
          const size_t w = WorkspaceWords(J) + kHdr;
          if (e > i && (words + w) * sizeof(int32_t) > limit) break;
          J.ws_off = static_cast<int64_t>(words);        // behind the headers: shifted below
          words += w - kHdr;
          batch.push_back(J);
          e++;
        }
        const size_t hdr_words = static_cast<size_t>(kHdr) * batch.size();
        for (size_t k = 0; k < batch.size(); k++) {
          batch[k].hdr_off = static_cast<int64_t>(kHdr * k);
          batch[k].ws_off += static_cast<int64_t>(hdr_words);
        }
        words += hdr_words;
        if (d_ws.Grow(words) || d_jobs.Grow(batch.size())) {
          SetError("kh_compact_lattice_align_words: out of device memory (workspace of %lld words)", static_cast<long long>(words));
          return KH_ENOMEM;
        }
        if (h_ws.size() < words) h_ws.resize(words);
        AlignCtx X{d_arc_off.p, d_label.p, d_next.p, d_g.p, d_a.p, d_str_off.p, d_strings.p, d_tinfo.p, d_ptype.p, P.reorder, d_ws.p};
        KH_HIP(T.Mark(0, st));
        KH_HIP(Up(d_jobs, batch.data(), batch.size(), st));
        KH_HIP(T.Mark(1, st));
        hipLaunchKernelGGL(AlignKernel, dim3(static_cast<unsigned>(batch.size())), dim3(kLanes), 0, st, d_jobs.p, X);
        KH_LAUNCH_CHECK();
        KH_HIP(T.Mark(2, st));
        // the headers first; then of every finished lattice its tuples, pairs and the used part of its arena
        KH_HIP(hipMemcpyAsync(h_ws.data(), d_ws.p, sizeof(int32_t) * hdr_words, hipMemcpyDeviceToHost, st));
        KH_HIP(hipStreamSynchronize(st));
        for (size_t k = 0; k < batch.size(); k++) {
          const AlignJob &J = batch[k];
          const int32_t *h = h_ws.data() + J.hdr_off;
          if (h[0] != 0) continue;
          if (h[1] < 0 || h[1] > J.C || h[2] < 0 || h[2] > J.PC || h[3] < 0 || h[3] > J.R) {
            SetError("kh_compact_lattice_align_words: lattice %d: the kernel left counts %d, %d, %d beyond its room", J.lat, h[1], h[2], h[3]);
            return KH_EDEVICE;
          }
          KH_HIP(hipMemcpyAsync(h_ws.data() + J.ws_off, d_ws.p + J.ws_off, sizeof(int32_t) * ResultWords(J, h[3]), hipMemcpyDeviceToHost, st));
        }
        KH_HIP(T.Mark(3, st));
        KH_HIP(hipStreamSynchronize(st));
        KH_HIP(T.AddAll());
        n_launches++;
        const auto f0 = std::chrono::steady_clock::now();
        for (size_t k = 0; k < batch.size(); k++) {
          const AlignJob &J = batch[k];
          const int32_t *w = h_ws.data() + J.hdr_off;
          OutLat &O = outs[J.lat];
          if (w[0] == kNeedsRoom) {
            // twice the table that ran full; four times the arena, whose use grows with the square of the pending length
            AlignJob &Q = P.jobs[todo[i + k]];
            const bool tuples_full = w[1] >= Q.C, pairs_full = w[2] >= Q.PC;
            if (tuples_full || pairs_full) SetRoom(&Q, (tuples_full ? 2ll : 1ll) * Q.C, (pairs_full ? 2ll : 1ll) * Q.PC, Q.R);
            else SetRoom(&Q, Q.C, Q.PC, 4ll * Q.R);
            again.push_back(todo[i + k]);
            n_again++;
          } else if (w[0] == kTooMany) {
            O.status = KH_ALIGN_TOO_MANY_STATES;
            O.n_tuples = w[1];
          } else if (w[0] != 0) {
            SetError("kh_compact_lattice_align_words: lattice %d: the kernel left status %d", J.lat, w[0]);
            return KH_EDEVICE;
          } else {
            Finish(P, J, w, h_ws.data() + J.ws_off, &O);
          }
        }
        ms_finish += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count();
        i = e;
      }
      todo.swap(again);
    }
  }
  // counts always; the rest only when everything fits
  bool fits = true;
  int first_short = -1;
  int64_t tuples = 0;
  for (int l = 0; l < n_lats; l++) {
    const OutLat &O = outs[l];
    status[l] = O.status;
    n_states[l] = static_cast<int32_t>(O.final_g.size());
    n_arcs[l] = static_cast<int32_t>(O.arc_src.size());
    n_tuples[l] = O.n_tuples;
    n_string_words[l] = static_cast<int64_t>(O.strings.size());
    tuples += O.n_tuples;
    if (out_state_offsets[l + 1] - out_state_offsets[l] < n_states[l] || out_arc_offsets[l + 1] - out_arc_offsets[l] < n_arcs[l] ||
        out_string_offsets[l + 1] - out_string_offsets[l] < n_string_words[l]) {
      if (fits) first_short = l;
      fits = false;
    }
  }
  g_stats.ms[5] = static_cast<float>(ms_finish);
  g_stats.counts[0] = n_launches;
  g_stats.counts[1] = n_again;
  g_stats.counts[2] = static_cast<int32_t>(std::min<int64_t>(tuples, INT32_MAX));
  if (!fits) {
    T.Finish(g_stats.ms);
    SetError("kh_compact_lattice_align_words: lattice %d: %d states, %d arcs, %lld transition-ids do not fit the room of %lld, %lld, "
             "%lld", first_short, n_states[first_short], n_arcs[first_short], static_cast<long long>(n_string_words[first_short]),
             static_cast<long long>(out_state_offsets[first_short + 1] - out_state_offsets[first_short]),
             static_cast<long long>(out_arc_offsets[first_short + 1] - out_arc_offsets[first_short]),
             static_cast<long long>(out_string_offsets[first_short + 1] - out_string_offsets[first_short]));
    return KH_EINVAL;
  }
  for (int l = 0; l < n_lats; l++) {
    const OutLat &O = outs[l];
    std::copy(O.final_g.begin(), O.final_g.end(), out_final_graph + out_state_offsets[l]);
    std::copy(O.final_a.begin(), O.final_a.end(), out_final_acoustic + out_state_offsets[l]);
    const int64_t a0 = out_arc_offsets[l];
    std::copy(O.arc_src.begin(), O.arc_src.end(), out_arc_src + a0);
    std::copy(O.arc_dst.begin(), O.arc_dst.end(), out_arc_nextstate + a0);
    std::copy(O.arc_label.begin(), O.arc_label.end(), out_arc_label + a0);
    std::copy(O.arc_g.begin(), O.arc_g.end(), out_arc_graph + a0);
    std::copy(O.arc_a.begin(), O.arc_a.end(), out_arc_acoustic + a0);
    std::copy(O.arc_len.begin(), O.arc_len.end(), out_arc_string_len + a0);
    std::copy(O.strings.begin(), O.strings.end(), out_strings + out_string_offsets[l]);
  }
  T.Finish(g_stats.ms);
  return KH_OK;
}
