// kh_decoder_host.hip — the host side of the decoder (the kernels are in kh_decoder.hip, what the two share in
// kh_decoder_types.h): KhDecoder / KhOnlineDecoder, arena carving, lattice building and best paths on worker threads, the
// determinizer hook, the decoder's environment switches (DecoderEnv: the one place that reads them), the kh_fst_* /
// kh_decoder_* / kh_online_decoder_* C API and the serving control loop.  No kernel is defined here: every launch goes
// through a launcher of kh_decoder.hip, so an edit to this file recompiles in seconds and leaves the kernels' code - and
// the hash of kh_decoder.hip that locks the recorded memory traffic to them - alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kh_common.h"
#include "kh_decoder_types.h"

using namespace kh;
using namespace kh::dec;

struct KhDecoder {
  const KhFst *fst = nullptr;
  KhDecoderConfig cfg;
  int max_batch = 0, max_frames = 0;
  int tok_frame_cap = 0, link_frame_cap = 0, expected_tokens = 0;
  int win_tok = 0, win_link = 0;   // tokens / links per frame the compaction window is sized for (averages, not caps)
  int max_slots = 0;
  // slot arenas (one set per persistent workgroup)
  void *slab = nullptr;
  size_t slab_bytes = 0;
  int slab_slots = 0, slab_T = 0, slab_scale = 1;
  int lazy = 0, alloc_link_a = 1;         // Params::lazy_prune / keep_ac of the calls this decoder serves (kh_decoder_decode sets them)
  int slab_lazy = 0, slab_link_a = 1;     // ... and what the slab was carved for
  int exact = 1, slab_exact = 0;          // kh_decoder_set_reference_order (default since round 6: the reference's own order); whether the slab holds the exact-order temporaries
  int rec_order_ids = -1;            // what the second word of the arcs in `rec` holds: 0 output labels, 1 state ids (ArcPdfKernel), -1 not built
  std::vector<Utt> h_slots;
  Utt *d_slots = nullptr;
  std::vector<UttX> h_slotsx;      // exact reference order: the slots' temporaries (Utt::x points into d_slotsx)
  UttX *d_slotsx = nullptr;
  UttIn *d_in = nullptr;
  UttOut *d_out = nullptr;
  unsigned long long *d_used = nullptr;
  long long *d_phase = nullptr;
  int4 *rec = nullptr;             // BuildArcPdf: the state records with the pdf of every arc
  int *d_bad = nullptr;            // BuildArcPdf: {flag, transition-id, pdf} of a map entry outside the score matrix

  // lattice pool
  void *pool_slab = nullptr;
  size_t pool_bytes = 0;
  Pool pool;
  struct HostPool {
    std::vector<int32_t> t_frame, t_state, l_src, l_dst, l_il, l_ol;
    std::vector<float> l_g, l_a;
  };
  std::vector<HostPool> rounds;     // online snapshots: host copy of the device pool
  std::vector<int32_t> h_round;     // utterance -> entry of `rounds` holding its lattice; -1 = the pinned pool below
  // Offline decoding: the kernel exports finished lattices straight into pinned host memory
  // and the host builds them while the kernel is still running (kh_decoder_decode).
  void *hp_slab = nullptr;          // pinned: pool arrays
  size_t hp_bytes = 0;
  Pool hpool;                       // device-side pointers into hp_slab (+ used counters in device memory)
  struct PoolView {
    const int32_t *t_frame, *t_state, *l_src, *l_dst, *l_il, *l_ol;
    const float *l_g, *l_a;
  } hview;                          // host-side pointers into hp_slab
  UttOut *h_out_pinned = nullptr;   // [max_batch] pinned
  int32_t *h_done = nullptr;        // [max_batch] pinned completion list
  // bump allocators of the worker threads for the canonical lattices (chunks are kept across calls)
  struct Arena {
    std::vector<std::unique_ptr<char[]>> chunks;
    std::vector<size_t> sizes;
    size_t cur = 0, used = 0;
    void Reset() { cur = 0; used = 0; }
    void *Take(size_t bytes) {
      bytes = (bytes + 63) & ~static_cast<size_t>(63);
      while (cur < chunks.size() && used + bytes > sizes[cur]) { cur++; used = 0; }
      if (cur == chunks.size()) {
        const size_t sz = std::max<size_t>(bytes, 32u << 20);
        chunks.emplace_back(new char[sz]);
        sizes.push_back(sz);
        used = 0;
      }
      void *p = chunks[cur].get() + used;
      used += bytes;
      return p;
    }
  };
  std::vector<Arena> arenas;
  std::vector<UttOut> h_out;
  std::vector<int32_t> h_T;
  std::vector<int32_t> order;  // queue position -> utterance
  int n_utts = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_kernel_ms = 0.f;
  float last_host_tail_ms = 0.f;   // wall time the host threads needed after the stream was idle (summed over the launches)
  int slot_limit = std::numeric_limits<int>::max();  // slots that fit in memory (found by a failed allocation)
  // canonical lattices, built lazily per utterance
  // Array of a canonical lattice: its own vector, or (batch post-pass, kh_decoder_prepare) a
  // slice of the decoder's batch store.  One mmap + munmap per vector per utterance serialises
  // the host threads on the process's mm lock (0.7 s per 2620-utterance step before).
  template <class T>
  struct Buf {
    T *p = nullptr;
    size_t n = 0;
    bool bound = false;
    std::vector<T> own;
    void bind(T *ext, size_t count) { p = ext; n = count; bound = true; }
    void resize(size_t count) {
      if (bound && count == n) return;
      bound = false;
      own.resize(count);
      p = own.data();
      n = count;
    }
    void assign(size_t count, T v) {
      resize(count);
      for (size_t i = 0; i < count; i++) p[i] = v;
    }
    size_t size() const { return n; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
  };
  struct Lat {
    bool built = false;
    Buf<int32_t> state_frame, state_hclg;
    Buf<float> state_final;
    Buf<int32_t> arc_src, arc_dst, arc_il, arc_ol;
    Buf<float> arc_g, arc_a;
    // best path (GetBestPath), cached
    int bp_rc = 1;  // 1 = not computed yet
    std::vector<int32_t> bp_ali, bp_words;
    float bp_graph = 0.f, bp_acoustic = 0.f;
  };
  std::vector<Lat> lats;
  // determinization behind the decoder (kh_decoder_set_determinize): the CompactLattice of every utterance
  bool det_enable = false;
  void (*after_launch)(void *) = nullptr;   // kh_decoder_set_after_launch
  void *after_launch_arg = nullptr;
  double det_beam = 0.0;
  float det_delta = 0.0f;
  int64_t det_max_mem = 0;
  int det_phone = 0, det_word = 1, det_minimize = 0;
  std::vector<int32_t> det_tid_phone;
  std::vector<KhCompactLattice *> clats;
  void FreeClats() {
    for (KhCompactLattice *c : clats) if (c) kh_compact_lattice_free(c);
    clats.clear();
  }
  // batch store of kh_decoder_prepare (kept across calls: the pages stay mapped)
  std::vector<int32_t> st_i[6];   // state_frame, state_hclg, arc_src, arc_dst, arc_il, arc_ol
  std::vector<float> st_f[3];     // state_final, arc_g, arc_a
};

// LatticeFasterOnlineDecoder for num_streams concurrent utterances: stream i owns
// slot i of `base` for the whole utterance.
struct KhOnlineDecoder {
  KhDecoder *base = nullptr;
  int num_streams = 0, max_frames = 0;
  SlotState *d_states = nullptr;
  Job *d_jobs = nullptr;
  std::vector<int32_t> frames;       // NumFramesDecoded() per stream
  std::vector<char> inited, finalized;
  std::vector<long long> lat_key;    // what base->lats[stream] was built from (-1: nothing)
  // kh_online_decoder_set_pdf_map: the (map, columns) pair the decoder's arc records were last built for
  const int32_t *pinned_map = nullptr;
  int pinned_cols = 0;
  bool pinned = false;
  // persistent serving kernel (kh_online_decoder_serve_*)
  ServeCtl *serve_ctl = nullptr;          // pinned host memory, one 64-byte block per stream
  int32_t *serve_quit = nullptr;          // pinned
  hipStream_t serve_stream = nullptr;
  bool serve_launched = false;            // a kernel has been launched and not yet seen to have ended
  long long *d_serve_act = nullptr;       // device: wall clock of every stream's last activity (the grid's idle decision)
  long long serve_relaunches = 0;         // how often the kernel was launched again after it had left
  const float *serve_ll = nullptr;
  long long serve_rows = 0;
  int serve_stride = 0;
  const int32_t *serve_map = nullptr;
  std::vector<int32_t> serve_seq;         // last command sequence number issued per stream
};

namespace {

// KhDecodeStats::status / the codes the kernels leave in Shared::status
const char *StatusText(int code) {
  switch (code) {
    case 0: return "ok";
    case 6: return "the lattice did not fit the pool";
    case 7: return "the survivor lists are full";
    case 8: case 9: return "reference order: the list order could not be built";
    case 10: return "a frame's epsilon links are not a DAG - internal inconsistency";
    default: return "capacity: a token / link arena or a per-frame cap overflowed";
  }
}

// CPUs this process may use: the cgroup's cpu.max quota / period (v2; cpu.cfs_quota_us / cpu.cfs_period_us in v1), else
// the hardware concurrency.  A container with 256 visible cores and a 16-CPU quota runs 16 threads well and 160 badly.
int HostCpuQuota() {
  static const int quota = [] {
    int hw = static_cast<int>(std::thread::hardware_concurrency());
    if (hw <= 0) hw = 1;
    long long q = -1, per = -1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char buf[64] = {0};
      if (fscanf(f, "%63s %lld", buf, &per) == 2 && strcmp(buf, "max") != 0) q = atoll(buf);
      fclose(f);
    } else {
      if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &q) != 1) q = -1; fclose(g); }
      if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &per) != 1) per = -1; fclose(g); }
    }
    if (q > 0 && per > 0) hw = std::max(1, std::min<int>(hw, static_cast<int>((q + per - 1) / per)));
    return hw;
  }();
  return quota;
}

// The decoder's environment switches: one field per variable, filled by ReadDecoderEnv() - the only place of this file
// that reads the environment.  Every entry point of the C API that depends on one of them reads the whole set when it is
// called (tests and tools change the variables between calls within one process) and passes it down.
template <class T>
struct EnvOpt {   // a variable that replaces a COMPUTED default: whether it is set, and its value
  bool set = false;
  T v = T();
};
struct DecoderEnv {
  long long tokens_per_frame = 65536;          // KH_DECODER_TOKENS_PER_FRAME: per-frame token cap of a slot (a frame beyond it: decoded again, arenas x 2)
  EnvOpt<long long> links_per_frame;           // KH_DECODER_LINKS_PER_FRAME: per-frame link cap (default 4 x the token cap)
  EnvOpt<int> hash_tokens;                     // KH_DECODER_HASH_TOKENS: tokens of a frame the hash table is sized for (default from max_active)
  EnvOpt<long long> window_tokens_per_frame;   // KH_DECODER_WINDOW_TOKENS_PER_FRAME: average frame the compaction window is sized for, tokens
  EnvOpt<long long> window_links_per_frame;    // KH_DECODER_WINDOW_LINKS_PER_FRAME: ... links (default 4 x the tokens)
  long long stable_tokens_per_frame = 256;     // KH_DECODER_STABLE_TOKENS_PER_FRAME: lattice density behind the window the arenas are sized for
  EnvOpt<long long> pool_tokens_per_frame;     // KH_DECODER_POOL_TOKENS_PER_FRAME: lattice pool, states per frame (default 48, and 80 links; set: links = 3/2 x)
  EnvOpt<int> slots;                           // KH_DECODER_SLOTS: persistent workgroups = arena sets (default 2 per CU; >= 1)
  EnvOpt<double> arena_gb;                     // KH_DECODER_ARENA_GB: memory the lazy schedule's arenas may take (default: free memory less a reserve)
  int local_world_size = 1;                    // LOCAL_WORLD_SIZE (torchrun): ranks sharing the node's CPUs; > 1 divides the default host threads
  EnvOpt<int> host_threads;                    // KH_DECODER_HOST_THREADS: host threads for lattices / best paths (>= 1; default: the CPU quota, at most 64)
  bool no_host_overlap = false;                // KH_DECODER_NO_HOST_OVERLAP (presence): the host threads start only when the kernel has finished
  bool canonical_bestpath = false;             // KH_DECODER_CANONICAL_BESTPATH (presence): best path over the canonical lattice, not from the pool
  bool profile = false;                        // KH_DECODER_PROFILE (presence): per-phase cycle counters and host timings on stderr
  bool keep_ac = false;                        // KH_DECODER_KEEP_AC (non-zero): links store their acoustic cost instead of recomputing it at export
  bool prune_interval_schedule = false;        // KH_DECODER_PRUNE_SCHEDULE=interval|reference: prune every prune_interval frames (default: lazy, on demand)
  int order = -1;                              // KH_DECODER_ORDER=reference (1) | canonical (0): CHANGES THE SEARCH RESULT; anything else (-1) keeps the decoder's setting
  bool order_sort = false;                     // KH_DECODER_ORDER_SORT (non-zero): reference order by the radix sort in every frame (tests)
  bool no_mid_scan = false;                    // KH_DECODER_NO_MID_SCAN (non-zero): reference order, the scan through memory beyond the LDS tier (tests)
  int closure_cap = kClMaxLoad;                // KH_DECODER_CLOSURE_CAP: entries of the LDS epsilon-closure table (0 .. kClMaxLoad; 0 = general routine)
  bool no_lds_scores = false;                  // KH_DECODER_NO_LDS_SCORES (presence): the frame's score row is not staged in LDS
  int serve_lazy_span = 0;                     // KH_SERVE_LAZY_SPAN: lazy-schedule streams collect garbage every so many frames (0 = arenas only; see OnlineLazySpan)
  double serve_timeout_ms = 30000.0;           // KH_SERVE_TIMEOUT_MS: deadline of every wait for the serving kernel (>= 1)
  long long serve_idle_ticks = 200000000ll;    // KH_SERVE_IDLE_MS: idle time after which the serving grid leaves, in 100 MHz ticks (default 2 s; >= 1 tick)
  bool serve_share_cu = false;                 // KH_SERVE_SHARE_CU (non-zero): serving workgroups may share a CU (the round-5 launch)
};

DecoderEnv ReadDecoderEnv() {
  DecoderEnv v;
  auto nonzero = [](const char *name) { const char *e = getenv(name); return e != nullptr && atoi(e) != 0; };
  if (const char *e = getenv("KH_DECODER_TOKENS_PER_FRAME")) v.tokens_per_frame = atoll(e);
  if (const char *e = getenv("KH_DECODER_LINKS_PER_FRAME")) { v.links_per_frame.set = true; v.links_per_frame.v = atoll(e); }
  if (const char *e = getenv("KH_DECODER_HASH_TOKENS")) { v.hash_tokens.set = true; v.hash_tokens.v = atoi(e); }
  if (const char *e = getenv("KH_DECODER_WINDOW_TOKENS_PER_FRAME")) { v.window_tokens_per_frame.set = true; v.window_tokens_per_frame.v = atoll(e); }
  if (const char *e = getenv("KH_DECODER_WINDOW_LINKS_PER_FRAME")) { v.window_links_per_frame.set = true; v.window_links_per_frame.v = atoll(e); }
  if (const char *e = getenv("KH_DECODER_STABLE_TOKENS_PER_FRAME")) v.stable_tokens_per_frame = atoll(e);
  if (const char *e = getenv("KH_DECODER_POOL_TOKENS_PER_FRAME")) { v.pool_tokens_per_frame.set = true; v.pool_tokens_per_frame.v = atoll(e); }
  if (const char *e = getenv("KH_DECODER_SLOTS")) { v.slots.set = true; v.slots.v = std::max(1, atoi(e)); }
  if (const char *e = getenv("KH_DECODER_ARENA_GB")) { v.arena_gb.set = true; v.arena_gb.v = atof(e); }
  if (const char *e = getenv("LOCAL_WORLD_SIZE")) v.local_world_size = atoi(e);
  if (const char *e = getenv("KH_DECODER_HOST_THREADS")) { v.host_threads.set = true; v.host_threads.v = std::max(1, atoi(e)); }
  v.no_host_overlap = getenv("KH_DECODER_NO_HOST_OVERLAP") != nullptr;
  v.canonical_bestpath = getenv("KH_DECODER_CANONICAL_BESTPATH") != nullptr;
  v.profile = getenv("KH_DECODER_PROFILE") != nullptr;
  v.keep_ac = nonzero("KH_DECODER_KEEP_AC");
  if (const char *e = getenv("KH_DECODER_PRUNE_SCHEDULE")) v.prune_interval_schedule = strcmp(e, "interval") == 0 || strcmp(e, "reference") == 0;
  if (const char *e = getenv("KH_DECODER_ORDER")) v.order = strcmp(e, "reference") == 0 ? 1 : (strcmp(e, "canonical") == 0 ? 0 : -1);
  v.order_sort = nonzero("KH_DECODER_ORDER_SORT");
  v.no_mid_scan = nonzero("KH_DECODER_NO_MID_SCAN");
  if (const char *e = getenv("KH_DECODER_CLOSURE_CAP")) v.closure_cap = std::max(0, std::min(kClMaxLoad, atoi(e)));
  v.no_lds_scores = getenv("KH_DECODER_NO_LDS_SCORES") != nullptr;
  if (const char *e = getenv("KH_SERVE_LAZY_SPAN")) v.serve_lazy_span = std::max(0, atoi(e));
  if (const char *e = getenv("KH_SERVE_TIMEOUT_MS")) v.serve_timeout_ms = std::max(1.0, atof(e));
  if (const char *e = getenv("KH_SERVE_IDLE_MS")) v.serve_idle_ticks = std::max(1ll, static_cast<long long>(atof(e) * 1e5));
  v.serve_share_cu = nonzero("KH_SERVE_SHARE_CU");
  return v;
}

// The host-thread count `n` a call arrived at from the CPUs it may use, as the environment adjusts it: one process per GPU
// shares the container's CPUs with the node's other ranks (LOCAL_WORLD_SIZE is set by torchrun); KH_DECODER_HOST_THREADS
// overrides.
int EnvHostThreads(const DecoderEnv &env, int n) {
  if (env.local_world_size > 1) n = std::max(2, n / env.local_world_size);
  if (env.host_threads.set) n = env.host_threads.v;
  return n;
}

size_t Align(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

struct Carver {
  char *base;
  size_t off = 0;
  template <class T>
  GP(T) Take(size_t n) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += Align(n * sizeof(T));
    return (GP(T))p;
  }
};

// Token / link capacity of a slot's arenas.
struct ArenaCaps {
  long long tok = 0, link = 0;
};
// every arena array holds 4-byte elements addressed with a 32-bit byte offset (Arr<T>): < 2^30 slots
constexpr long long kMaxArenaSlots = (1ll << 30) - 1;

// The capacity the windowed schedule (PruneActiveTokens + compaction every prune_interval frames) needs:
// the compaction window at its average size + lattice density for the frames behind it.
ArenaCaps WindowedCaps(const DecoderEnv &env, int T, int tok_frame_cap, int link_frame_cap, int win_tok, int win_link, int prune_interval) {
  // window: 2 * max(prune_interval, 25) frames + one interval of new frames + frontier;
  // stable part: lattice density
  const long long win_frames = std::min<long long>((KH_COMPACT_EVERY + 1ll) * std::max(prune_interval, 25) + 1ll * KH_COMPACT_EVERY * prune_interval + 3, T + 2);
  const long long per_frame = env.stable_tokens_per_frame;
  const long long stable_tok = std::max<long long>(65536, per_frame * (T + 2));
  // the window holds win_frames frames of AVERAGE size (win_tok / win_link per frame) plus one
  // frame of the per-frame caps; an utterance that needs more reports an overflow and is
  // decoded again with larger arenas (kh_decoder_decode)
  ArenaCaps c;
  c.tok = std::min(kMaxArenaSlots, stable_tok + win_frames * win_tok + tok_frame_cap);
  c.link = std::min(kMaxArenaSlots, 3 * stable_tok + win_frames * win_link + link_frame_cap);
  return c;
}

// The capacity the lazy schedule would like: the whole utterance unpruned at the window's average frame size
// (links: twice the tokens - a frame materialises ~1.6 candidates per token it creates), never less than the
// windowed one.  EnsureSlots scales it down to the memory there is; a slot that fills up collects its garbage.
ArenaCaps LazyCaps(const ArenaCaps &floor, int T, int tok_frame_cap, int link_frame_cap, int win_tok) {
  ArenaCaps c;
  c.tok = std::min(kMaxArenaSlots, std::max(floor.tok, (T + 2ll) * win_tok + tok_frame_cap));
  c.link = std::min(kMaxArenaSlots, std::max(floor.link, 2 * (T + 2ll) * win_tok + 2ll * link_frame_cap));
  return c;
}

// Arena set of one slot, sized for utterances of up to T frames.
void CarveSlot(Carver &c, Utt &u, int T, int tok_frame_cap, int link_frame_cap, const ArenaCaps &caps, bool link_a,
               float hash_ratio, int expected_tokens, bool exact, UttX *xo = nullptr, int scale = 1) {
  u.T = T;
  u.tok_frame_cap = tok_frame_cap;
  u.link_frame_cap = link_frame_cap;
  u.window_cap = static_cast<int32_t>(caps.tok);
  u.tok_cap = static_cast<int32_t>(caps.tok);
  u.link_cap = static_cast<int32_t>(caps.link);
  const size_t nt = u.tok_cap, nl = u.link_cap;
  u.tok_state = c.Take<int32_t>(nt);
  u.tok_cost = c.Take<uint32_t>(nt);
  u.tok_extra = c.Take<float>(nt);
  u.tmp_remap = c.Take<int32_t>(nt);
  u.link_dst = c.Take<int32_t>(nl);
  u.link_src = c.Take<int32_t>(nl);
  u.link_arc = c.Take<int32_t>(nl);
  u.link_k = c.Take<float>(nl);
  u.link_a = c.Take<float>(link_a ? nl : 0);   // (offline decoding recomputes the acoustic costs at export: Params::keep_ac)
  u.frame_b = c.Take<int32_t>(T + 2);
  u.frame_e = c.Take<int32_t>(T + 2);
  u.feps_b = c.Take<int32_t>(T + 2);
  u.feps_e = c.Take<int32_t>(T + 2);
  u.femit_b = c.Take<int32_t>(T + 2);
  u.femit_e = c.Take<int32_t>(T + 2);
  u.cost_offset = c.Take<float>(T + 1);
  u.must_links = c.Take<uint8_t>(T + 2);
  u.must_toks = c.Take<uint8_t>(T + 2);
  u.tmp_slot = c.Take<int32_t>(tok_frame_cap);
  u.tmp_dirty = c.Take<int32_t>(tok_frame_cap);
  u.tmp_work0 = c.Take<int32_t>(tok_frame_cap);
  u.tmp_work1 = c.Take<int32_t>(tok_frame_cap);
  u.tmp_epslist = c.Take<int32_t>(tok_frame_cap);
  u.tmp_f0 = c.Take<float>(tok_frame_cap);
  u.tmp_acc0 = c.Take<uint32_t>(tok_frame_cap);
  u.tmp_acc1 = c.Take<uint32_t>(tok_frame_cap);
  // survivor lists of FinalBackward: ~4 x the lattice density the recipe's options give (17 states / 27 arcs per frame);
  // an utterance that needs more is decoded again with everything doubled (tok_frame_cap scales with the retry)
  u.surv_tok_cap = static_cast<int32_t>(std::min<long long>(caps.tok, 64ll * scale * (T + 2) + tok_frame_cap));
  u.surv_link_cap = static_cast<int32_t>(std::min<long long>(caps.link, 128ll * scale * (T + 2) + 2ll * tok_frame_cap));
  u.surv_tok = c.Take<int32_t>(2 * static_cast<size_t>(u.surv_tok_cap));
  u.surv_link = c.Take<int32_t>(2 * static_cast<size_t>(u.surv_link_cap));
  // hash_ratio x the tokens a frame is expected to hold (lattice-faster-decoder.cc:193-199
  // resizes to hash_ratio x the previous frame's count); never fewer entries than a
  // frame may hold.  A smaller table keeps more of it in L2.
  size_t hs = 1;
  while (hs < static_cast<size_t>(hash_ratio * expected_tokens) || hs <= static_cast<size_t>(tok_frame_cap)) hs <<= 1;
  u.hash_mask = static_cast<uint32_t>(hs - 1);
  u.hash = c.Take<unsigned long long>(hs);
  // exact reference order: per-frame temporaries (8 MB per slot at the default caps)
  {
    UttX x;
    const size_t tf = exact ? tok_frame_cap : 0, lf = exact ? link_frame_cap : 0;
    // the reference's table has at most hash_ratio x (tokens of a frame) buckets, 1000 to begin with (:37, :219-225)
    x.x_hcap = exact ? static_cast<int32_t>(std::max<double>(1000.0, static_cast<double>(hash_ratio) * tok_frame_cap) + 16) : 0;
    x.x_pos = c.Take<int32_t>(tf);
    x.x_m = c.Take<uint32_t>(tf);
    x.x_c = c.Take<int32_t>(tf);
    x.x_q = c.Take<uint32_t>(tf);
    x.x_bkt = c.Take<int32_t>(tf);
    x.x_epsidx = c.Take<int32_t>(tf);
    x.x_nl0 = c.Take<int32_t>(tf);
    x.x_nl1 = c.Take<int32_t>(tf);
    x.x_ncost = c.Take<float>(tf);
    x.x_ord = c.Take<int32_t>(lf);
    x.x_lw = c.Take<float>(lf);
    x.x_stack = c.Take<int32_t>(lf);
    x.x_bmin = c.Take<uint32_t>(static_cast<size_t>(x.x_hcap));
    x.x_key0 = c.Take<unsigned long long>(tf);
    x.x_key1 = c.Take<unsigned long long>(tf);
    x.x_val0 = c.Take<int32_t>(tf);
    x.x_val1 = c.Take<int32_t>(tf);
    x.x_h = c.Take<int32_t>(tf);
    x.x_inb = c.Take<int32_t>(tf);
    x.x_c0e = c.Take<uint32_t>(tf);
    x.x_csid = c.Take<int32_t>(lf);
    x.x_rec0 = Arr<const KhInt4>((GP(const KhInt4))nullptr);
    if (xo) *xo = x;
  }
  u.ll = (GP(const float))nullptr;
  u.ll_stride = 0;
  u.phase_cycles = (GP(long long))nullptr;
}

// canonical lattice of one utterance from the host copy of the pool (GetRawLattice
// :109-191 with use_final_probs = true after FinalizeDecoding)
int BuildLattice(KhDecoder *d, int ui) {
  KhDecoder::Lat &L = d->lats[ui];
  if (L.built) return KH_OK;
  const UttOut &o = d->h_out[ui];
  const KhDecodeStats &st = o.stats;
  if (st.status != 0) {
    SetError("utterance %d: decoder failed (code %d: %s)", ui, st.status, StatusText(st.status));
    return KH_ECAPACITY;
  }
  const int T = d->h_T[ui];
  const size_t n = o.n_tok, m = o.n_link;
  KhDecoder::PoolView hp;
  if (d->h_round[ui] < 0) {
    hp = d->hview;
  } else {
    const KhDecoder::HostPool &r = d->rounds[d->h_round[ui]];
    hp = KhDecoder::PoolView{r.t_frame.data(), r.t_state.data(), r.l_src.data(), r.l_dst.data(), r.l_il.data(),
                             r.l_ol.data(), r.l_g.data(), r.l_a.data()};
  }
  const int32_t *tf = hp.t_frame + o.tok_off, *ts = hp.t_state + o.tok_off;
  // (scratch vectors are per thread and only grow: no allocation per utterance)
  static thread_local std::vector<int32_t> ord, newidx, bucket;
  // canonical order (frame, HCLG state) with the start token first: lattice state 0 is the
  // start state (the reference gets that from TopSortTokens :839-914; ComputeBestPath and
  // the lattice writers rely on it), also when the start state has an epsilon arc to a
  // lower-numbered state.  Counting sort by frame (the kernel exports a frame's tokens together), then the
  // handful of tokens of a frame by state: two comparison sorts over the whole utterance were 2.5 ms of CPU per
  // utterance - as much as its determinization - on boxes whose CPU quota is what bounds the end-to-end step.
  const int32_t start = d->fst->start_state;
  int32_t max_f = 0;
  for (size_t k = 0; k < n; k++) {
    if (tf[k] < 0) { SetError("utterance %d: exported token %zu has frame %d", ui, k, tf[k]); return KH_ESTATE; }
    max_f = std::max(max_f, tf[k]);
  }
  bucket.assign(static_cast<size_t>(max_f) + 2, 0);
  for (size_t k = 0; k < n; k++) bucket[tf[k] + 1]++;
  for (int f = 0; f <= max_f; f++) bucket[f + 1] += bucket[f];
  ord.resize(n);
  {
    static thread_local std::vector<int32_t> fill;
    fill.assign(bucket.begin(), bucket.end() - 1);
    for (size_t k = 0; k < n; k++) ord[fill[tf[k]]++] = static_cast<int32_t>(k);
  }
  for (int f = 0; f <= max_f; f++) {
    int32_t *b = ord.data() + bucket[f], *e = ord.data() + bucket[f + 1];
    auto less = [&](int32_t x, int32_t y) {
      if (f == 0) {
        const bool xs = ts[x] != start, ys = ts[y] != start;
        if (xs != ys) return xs < ys;
      }
      return ts[x] < ts[y];
    };
    if (e - b <= 24) {
      for (int32_t *q = b + 1; q < e; q++) {
        const int32_t v = *q;
        int32_t *r = q;
        for (; r > b && less(v, r[-1]); r--) *r = r[-1];
        *r = v;
      }
    } else {
      std::sort(b, e, less);
    }
  }
  newidx.resize(n);
  for (size_t k = 0; k < n; k++) newidx[ord[k]] = static_cast<int32_t>(k);
  const float inf = std::numeric_limits<float>::infinity();
  L.state_frame.resize(n);
  L.state_hclg.resize(n);
  L.state_final.assign(n, inf);
  const bool have_final = st.reached_final != 0;
  for (size_t k = 0; k < n; k++) {
    const int32_t i = ord[k];
    L.state_frame[k] = tf[i];
    L.state_hclg[k] = ts[i];
    if (tf[i] == T) {  // :177-186
      if (have_final) {
        const float fc = d->fst->final_host[ts[i]];
        if (fc != inf) L.state_final[k] = fc;
      } else {
        L.state_final[k] = 0.0f;
      }
    }
  }
  // arcs in the order (src, ilabel, olabel, dst, graph cost, acoustic cost): counting sort by source state, then the few
  // arcs of a state among themselves
  struct A { int32_t src, il, ol, dst; float g, a; };
  static thread_local std::vector<A> arcs;
  static thread_local std::vector<int32_t> aoff;
  arcs.resize(m);
  const int32_t *ls = hp.l_src + o.link_off, *ld = hp.l_dst + o.link_off,
                *li = hp.l_il + o.link_off, *lo = hp.l_ol + o.link_off;
  const float *lg = hp.l_g + o.link_off, *la = hp.l_a + o.link_off;
  aoff.assign(n + 1, 0);
  for (size_t j = 0; j < m; j++) {
    if (ls[j] < 0 || static_cast<size_t>(ls[j]) >= n || ld[j] < 0 || static_cast<size_t>(ld[j]) >= n) {
      SetError("utterance %d: exported link %zu points outside the %zu tokens", ui, j, n);
      return KH_ESTATE;
    }
    aoff[newidx[ls[j]] + 1]++;
  }
  for (size_t k = 0; k < n; k++) aoff[k + 1] += aoff[k];
  {
    static thread_local std::vector<int32_t> fill;
    fill.assign(aoff.begin(), aoff.end() - 1);
    for (size_t j = 0; j < m; j++) {
      const int32_t sidx = newidx[ls[j]];
      arcs[fill[sidx]++] = A{sidx, li[j], lo[j], newidx[ld[j]], lg[j], la[j]};
    }
  }
  auto arc_less = [](const A &x, const A &y) {
    if (x.il != y.il) return x.il < y.il;
    if (x.ol != y.ol) return x.ol < y.ol;
    if (x.dst != y.dst) return x.dst < y.dst;
    if (x.g != y.g) return x.g < y.g;
    return x.a < y.a;
  };
  for (size_t k = 0; k < n; k++) {
    A *b = arcs.data() + aoff[k], *e = arcs.data() + aoff[k + 1];
    if (e - b <= 24) {
      for (A *q = b + 1; q < e; q++) {
        const A v = *q;
        A *r = q;
        for (; r > b && arc_less(v, r[-1]); r--) *r = r[-1];
        *r = v;
      }
    } else {
      std::sort(b, e, arc_less);
    }
  }
  L.arc_src.resize(m); L.arc_dst.resize(m); L.arc_il.resize(m);
  L.arc_ol.resize(m); L.arc_g.resize(m); L.arc_a.resize(m);
  for (size_t j = 0; j < m; j++) {
    L.arc_src[j] = arcs[j].src; L.arc_dst[j] = arcs[j].dst; L.arc_il[j] = arcs[j].il;
    L.arc_ol[j] = arcs[j].ol; L.arc_g[j] = arcs[j].g; L.arc_a[j] = arcs[j].a;
  }
  L.built = true;
  return KH_OK;
}

struct LatWeight { float v1, v2; };
// fstext/lattice-weight.h:297-312
inline int Compare(const LatWeight &w1, const LatWeight &w2) {
  const float f1 = w1.v1 + w1.v2, f2 = w2.v1 + w2.v2;
  if (f1 < f2) return 1;
  else if (f1 > f2) return -1;
  else if (w1.v1 < w2.v1) return 1;
  else if (w1.v1 > w2.v1) return -1;
  else return 0;
}

// Best path of utterance `utt` straight from the exported pool arrays, cached in the Lat: the result of ComputeBestPath
// below (same LatticeWeight arithmetic, same tie rule) without building the canonical lattice first - two counting sorts
// and one relaxation per link instead of the canonical sort of ~12 k states / ~20 k arcs and Bellman-Ford sweeps over all
// of them (2 ms of CPU per utterance, which a rank with two host threads does not have: DESIGN.md section 5).
// The raw lattice is layered: an emitting link goes from frame f to f + 1, an epsilon link stays inside its frame.  So the
// links are bucketed by (destination frame, emitting before epsilon) and relaxed frame by frame, the epsilon links of a
// frame to their fixed point.  Tie rule: ComputeBestPath prefers the smaller CANONICAL arc index among the arcs that reach
// a state with Compare-equal weights; canonical arcs are ordered by (source state's canonical index = (frame, start token
// first, HCLG state), ilabel, olabel, destination, graph cost, acoustic cost), which is compared on the keys here.
// Returns 1 if the pool's layout is not the one expected (the caller then takes the canonical route).
int ComputeBestPathLean(KhDecoder *d, int utt) {
  KhDecoder::Lat &L = d->lats[utt];
  const UttOut &o = d->h_out[utt];
  if (o.stats.status != 0) {
    SetError("utterance %d: decoder failed (code %d: %s)", utt, o.stats.status, StatusText(o.stats.status));
    return KH_ECAPACITY;
  }
  if (d->h_round[utt] >= 0) return 1;   // (online snapshots arrive built)
  const KhDecoder::PoolView hp = d->hview;
  const int T = d->h_T[utt];
  const int n = static_cast<int>(o.n_tok), m = static_cast<int>(o.n_link);
  if (n == 0) {
    SetError("GetBestPath: empty lattice for utterance %d", utt);
    return L.bp_rc = KH_ESTATE;
  }
  const int32_t *tf = hp.t_frame + o.tok_off, *ts = hp.t_state + o.tok_off;
  const int32_t *ls = hp.l_src + o.link_off, *ld = hp.l_dst + o.link_off, *li = hp.l_il + o.link_off, *lo = hp.l_ol + o.link_off;
  const float *lg = hp.l_g + o.link_off, *la = hp.l_a + o.link_off;
  const int32_t start = d->fst->start_state;
  const float inf = std::numeric_limits<float>::infinity();
  static thread_local std::vector<int32_t> cnt, ord, parent;
  static thread_local std::vector<LatWeight> dist;
  int max_f = 0;
  for (int k = 0; k < n; k++) {
    if (tf[k] < 0) return 1;
    max_f = std::max(max_f, tf[k]);
  }
  cnt.assign(2 * static_cast<size_t>(max_f) + 3, 0);
  for (int j = 0; j < m; j++) {
    if (ls[j] < 0 || ls[j] >= n || ld[j] < 0 || ld[j] >= n) return 1;
    const int fs = tf[ls[j]], fd = tf[ld[j]];
    if (fd != fs && fd != fs + 1) return 1;
    cnt[2 * fd + (fd == fs ? 1 : 0) + 1]++;
  }
  for (size_t b = 0; b + 1 < cnt.size(); b++) cnt[b + 1] += cnt[b];
  ord.resize(m);
  {
    static thread_local std::vector<int32_t> fill;
    fill.assign(cnt.begin(), cnt.end() - 1);
    for (int j = 0; j < m; j++) {
      const int fs = tf[ls[j]], fd = tf[ld[j]];
      ord[fill[2 * fd + (fd == fs ? 1 : 0)]++] = j;
    }
  }
  // canonical state 0: the first token of frame 0 in the order (start token first, HCLG state)
  int s0 = -1;
  for (int k = 0; k < n; k++) {
    if (tf[k] != 0) continue;
    if (s0 < 0) { s0 = k; continue; }
    const bool xs = ts[k] != start, ys = ts[s0] != start;
    if (xs != ys ? xs < ys : ts[k] < ts[s0]) s0 = k;
  }
  if (s0 < 0) return 1;
  dist.assign(n, LatWeight{inf, inf});
  parent.assign(n, -1);
  dist[s0] = LatWeight{0.f, 0.f};
  // is link j in front of link p in the canonical arc order?  (both end in the same state)
  auto before = [&](int j, int p) {
    const int a = ls[j], b = ls[p];
    if (a != b) {
      if (tf[a] != tf[b]) return tf[a] < tf[b];
      if (tf[a] == 0) {
        const bool xs = ts[a] != start, ys = ts[b] != start;
        if (xs != ys) return xs < ys;
      }
      if (ts[a] != ts[b]) return ts[a] < ts[b];
    }
    if (li[j] != li[p]) return li[j] < li[p];
    if (lo[j] != lo[p]) return lo[j] < lo[p];
    if (lg[j] != lg[p]) return lg[j] < lg[p];
    return la[j] < la[p];
  };
  auto relax = [&](int j) -> bool {
    const LatWeight sd = dist[ls[j]];
    if (sd.v1 == inf) return false;
    const LatWeight w{sd.v1 + lg[j], sd.v2 + la[j]};
    LatWeight &nd = dist[ld[j]];
    const int c = (nd.v1 == inf && nd.v2 == inf) ? 1 : Compare(w, nd);
    if (c == 1 || (c == 0 && parent[ld[j]] != j && (parent[ld[j]] < 0 || before(j, parent[ld[j]])))) {
      nd = w;
      parent[ld[j]] = j;
      return true;
    }
    return false;
  };
  for (int f = 0; f <= max_f; f++) {
    for (int q = cnt[2 * f]; q < cnt[2 * f + 1]; q++) (void)relax(ord[q]);   // emitting links into frame f
    const int eb = cnt[2 * f + 1], ee = cnt[2 * f + 2];
    for (int guard = 0; guard < ee - eb + 2; guard++) {                      // epsilon links inside frame f
      bool changed = false;
      for (int q = eb; q < ee; q++) changed |= relax(ord[q]);
      if (!changed) break;
    }
  }
  // the final state: best dist + final cost (:177-186 as BuildLattice), ties to the smaller canonical state
  const bool have_final = o.stats.reached_final != 0;
  LatWeight best{inf, inf};
  int best_state = -1;
  for (int k = 0; k < n; k++) {
    if (tf[k] != T || dist[k].v1 == inf) continue;
    float fc = 0.0f;
    if (have_final) {
      fc = d->fst->final_host[ts[k]];
      if (fc == inf) continue;
    }
    const LatWeight w{dist[k].v1 + fc, dist[k].v2 + 0.0f};
    bool take = best_state < 0;
    if (!take) {
      const int c = Compare(w, best);
      if (c == 1) take = true;
      else if (c == 0) {
        const bool xs = T == 0 && ts[k] != start, ys = T == 0 && ts[best_state] != start;
        take = xs != ys ? xs < ys : ts[k] < ts[best_state];
      }
    }
    if (take) { best = w; best_state = k; }
  }
  if (best_state < 0) {
    SetError("GetBestPath: no final state reachable for utterance %d", utt);
    return L.bp_rc = KH_ESTATE;
  }
  L.bp_ali.clear();
  L.bp_words.clear();
  for (int s = best_state; parent[s] >= 0; s = ls[parent[s]]) {
    const int j = parent[s];
    if (li[j] != 0) L.bp_ali.push_back(li[j]);
    if (lo[j] != 0) L.bp_words.push_back(lo[j]);
  }
  std::reverse(L.bp_ali.begin(), L.bp_ali.end());
  std::reverse(L.bp_words.begin(), L.bp_words.end());
  L.bp_graph = best.v1;
  L.bp_acoustic = best.v2;
  return L.bp_rc = KH_OK;
}

// Best path of utterance `utt`, cached in the Lat: from the pool (above) unless the canonical lattice exists already or
// KH_DECODER_CANONICAL_BESTPATH asks for the route over it (the cross-check of tests/test_gpu_decoder.py).
int ComputeBestPath(KhDecoder *d, const DecoderEnv &env, int utt) {
  {
    KhDecoder::Lat &L0 = d->lats[utt];
    if (L0.bp_rc == 1 && !L0.built && !env.canonical_bestpath) {
      const int rc = ComputeBestPathLean(d, utt);
      if (rc != 1) return rc;
    }
  }
  int rc = BuildLattice(d, utt);
  if (rc) return rc;
  KhDecoder::Lat &L = d->lats[utt];
  if (L.bp_rc != 1) {
    if (L.bp_rc != KH_OK) SetError("GetBestPath: no best path for utterance %d", utt);
    return L.bp_rc;
  }
  const int ns = static_cast<int>(L.state_frame.size()), na = static_cast<int>(L.arc_src.size());
  if (ns == 0) {
    SetError("GetBestPath: empty lattice for utterance %d", utt);
    return L.bp_rc = KH_ESTATE;
  }
  const float inf = std::numeric_limits<float>::infinity();
  static thread_local std::vector<LatWeight> dist;
  static thread_local std::vector<int32_t> parent;
  dist.assign(ns, LatWeight{inf, inf});
  parent.assign(ns, -1);
  dist[0] = LatWeight{0.f, 0.f};
  bool changed = true;
  for (int guard = 0; changed && guard < ns + 2; guard++) {
    changed = false;
    for (int j = 0; j < na; j++) {
      const LatWeight sd = dist[L.arc_src[j]];
      if (sd.v1 == inf) continue;
      const LatWeight w{sd.v1 + L.arc_g[j], sd.v2 + L.arc_a[j]};
      LatWeight &nd = dist[L.arc_dst[j]];
      const int c = (nd.v1 == inf && nd.v2 == inf) ? 1 : Compare(w, nd);
      if (c == 1 || (c == 0 && parent[L.arc_dst[j]] > j)) {
        nd = w;
        parent[L.arc_dst[j]] = j;
        changed = true;
      }
    }
  }
  LatWeight best{inf, inf};
  int best_state = -1;
  for (int s = 0; s < ns; s++) {
    if (L.state_final[s] == inf || dist[s].v1 == inf) continue;
    const LatWeight w{dist[s].v1 + L.state_final[s], dist[s].v2 + 0.0f};
    if (best_state < 0 || Compare(w, best) == 1) {
      best = w;
      best_state = s;
    }
  }
  if (best_state < 0) {
    SetError("GetBestPath: no final state reachable for utterance %d", utt);
    return L.bp_rc = KH_ESTATE;
  }
  std::vector<int32_t> path;
  for (int s = best_state; parent[s] >= 0; s = L.arc_src[parent[s]]) path.push_back(parent[s]);
  std::reverse(path.begin(), path.end());
  L.bp_ali.clear();
  L.bp_words.clear();
  for (int j : path) {
    if (L.arc_il[j] != 0) L.bp_ali.push_back(L.arc_il[j]);
    if (L.arc_ol[j] != 0) L.bp_words.push_back(L.arc_ol[j]);
  }
  L.bp_graph = best.v1;
  L.bp_acoustic = best.v2;
  return L.bp_rc = KH_OK;
}

// DeterminizeLatticePhonePrunedWrapper (decoder-wrappers.cc:264-274) on the utterance's raw lattice, cached.
int DeterminizeUtt(KhDecoder *d, int utt) {
  if (d->clats[utt]) return KH_OK;
  int rc = BuildLattice(d, utt);
  if (rc) return rc;
  const KhDecoder::Lat &L = d->lats[utt];
  KhCompactLattice *c = kh_determinize_lattice_phone_pruned(
      static_cast<int>(L.state_frame.size()), static_cast<int>(L.arc_src.size()), L.arc_src.data(), L.arc_dst.data(), L.arc_il.data(),
      L.arc_ol.data(), L.arc_g.data(), L.arc_a.data(), L.state_final.data(), d->det_phone ? d->det_tid_phone.data() : nullptr,
      static_cast<int>(d->det_tid_phone.size()), d->det_beam, d->det_delta, d->det_max_mem, d->det_phone, d->det_word, d->det_minimize);
  if (!c) return KH_EINVAL;
  d->clats[utt] = c;
  return KH_OK;
}

// Arena slab of the decoder: n_want slots sized for utterances of up to T_max frames
// (fewer if they do not fit in free memory); establishes the arena invariants.
int EnsureSlots(KhDecoder *d, const DecoderEnv &env, int n_want, int T_max, hipStream_t st, int *n_slots_out, int scale = 1) {
  int n_slots = n_want;
  const bool same_kind = d->slab_lazy == d->lazy && d->slab_link_a == d->alloc_link_a && d->slab_exact == d->exact;
  if (T_max <= d->slab_T && scale == d->slab_scale && same_kind) n_slots = std::min(n_slots, d->slot_limit);  // an earlier batch found that more do not fit
  const long long kCap = (1ll << 28);
  const int tfc = static_cast<int>(std::min<long long>(kCap, 1ll * d->tok_frame_cap * scale)),
            lfc = static_cast<int>(std::min<long long>(kCap, 1ll * d->link_frame_cap * scale)),
            wt = static_cast<int>(std::min<long long>(kCap, 1ll * d->win_tok * scale)),
            wl = static_cast<int>(std::min<long long>(kCap, 1ll * d->win_link * scale)),
            et = static_cast<int>(std::min<long long>(kCap, 1ll * d->expected_tokens * scale));
  if (n_slots > d->slab_slots || T_max > d->slab_T || scale != d->slab_scale || !same_kind) {
    PoolFree(d->slab);
    d->slab = nullptr;
    size_t slab_bytes = 0;
    // leave room for the lattice pool and the caller: all but 16 GB of what is free
    // (blocks cached by the library's own pool count as free: PoolMalloc returns
    // them to HIP when an allocation fails)
    size_t free_b = 0, total_b = 0;
    KH_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += PoolCachedBytes();
    const size_t budget = free_b > (16ull << 30) ? free_b - (16ull << 30) : free_b / 2;
    // the lazy schedule takes what memory it can use, not what it must have: it leaves 32 GB more to the caller
    size_t lazy_budget = budget > (64ull << 30) ? budget - (32ull << 30) : budget / 2;
    if (env.arena_gb.set) lazy_budget = std::min<size_t>(budget, static_cast<size_t>(env.arena_gb.v * (1ull << 30)));
    const int want_slots = n_slots;
    const ArenaCaps floor_caps = WindowedCaps(env, T_max, tfc, lfc, wt, wl, d->cfg.prune_interval);
    ArenaCaps caps = floor_caps;
    auto slot_bytes = [&](const ArenaCaps &c) {
      Carver sizer{nullptr};
      Utt tmp;
      CarveSlot(sizer, tmp, T_max, tfc, lfc, c, d->alloc_link_a != 0, d->cfg.hash_ratio, et, d->exact != 0, nullptr, scale);
      return sizer.off;
    };
    for (;; n_slots = (n_slots + 1) / 2) {
      caps = floor_caps;
      if (d->lazy) {
        const ArenaCaps want = LazyCaps(floor_caps, T_max, tfc, lfc, wt);
        const size_t b_floor = slot_bytes(floor_caps), b_want = slot_bytes(want), per_slot = lazy_budget / n_slots;
        if (b_want <= per_slot) {
          caps = want;
        } else if (per_slot > b_floor && b_want > b_floor) {
          // (the bytes of a slot are affine in its capacities up to alignment: interpolate, a little under)
          const double r = 0.999 * static_cast<double>(per_slot - b_floor) / static_cast<double>(b_want - b_floor);
          caps.tok = floor_caps.tok + static_cast<long long>(r * (want.tok - floor_caps.tok));
          caps.link = floor_caps.link + static_cast<long long>(r * (want.link - floor_caps.link));
        }
      }
      slab_bytes = slot_bytes(caps) * n_slots;
      if (slab_bytes <= budget || n_slots == 1) {
        d->slab = PoolMalloc(slab_bytes);
        if (d->slab || n_slots == 1) break;
      }
    }
    if (!d->slab) { d->slab_bytes = 0; d->slab_slots = 0; return KH_ENOMEM; }
    if (env.profile)
      fprintf(stderr, "[kh_decoder profile] arenas (scale %d, %s schedule): %d slots (wanted %d) x %.1f MB = %.1f GB (%lld tokens, %lld links per slot); device memory free %.1f GB of %.1f GB\n",
              scale, d->lazy ? "lazy" : "windowed", n_slots, want_slots, slab_bytes / 1e6 / n_slots, slab_bytes / 1e9, caps.tok, caps.link, free_b / 1e9, total_b / 1e9);
    d->slot_limit = n_slots < want_slots ? n_slots : std::numeric_limits<int>::max();
    Carver sizer{nullptr};
    sizer.off = slab_bytes;
    d->slab_bytes = sizer.off;
    d->slab_slots = n_slots;
    d->slab_T = T_max;
    d->slab_scale = scale;
    d->slab_lazy = d->lazy;
    d->slab_link_a = d->alloc_link_a;
    d->slab_exact = d->exact;
    d->h_slots.assign(n_slots, Utt());
    Carver carver{static_cast<char *>(d->slab)};
    d->h_slotsx.assign(n_slots, UttX());
    for (int i = 0; i < n_slots; i++)
      CarveSlot(carver, d->h_slots[i], T_max, tfc, lfc, caps, d->alloc_link_a != 0, d->cfg.hash_ratio, et, d->exact != 0, &d->h_slotsx[i], scale);
    for (int i = 0; i < n_slots; i++) d->h_slotsx[i].x_rec0 = Arr<const KhInt4>((GP(const KhInt4))d->fst->rec);
    // arena invariants for the first utterance of every slot (later ones are
    // restored by the kernel): token costs = +inf, hash empty, dirty flags zero
    for (int i = 0; i < n_slots; i++) {
      Utt &u = d->h_slots[i];
      LaunchFillU32(st, (uint32_t *)u.tok_cost.p, static_cast<size_t>(u.tok_cap), kEncInf);
      KH_HIP(hipMemsetAsync((void *)(unsigned long long *)u.hash.p, 0, sizeof(unsigned long long) * (static_cast<size_t>(u.hash_mask) + 1), st));
      KH_HIP(hipMemsetAsync((void *)(int32_t *)u.tmp_dirty.p, 0, sizeof(int32_t) * u.tok_frame_cap, st));
      const UttX &x = d->h_slotsx[i];
      if (x.x_hcap > 0) KH_HIP(hipMemsetAsync((void *)(uint32_t *)x.x_bmin.p, 0xFF, sizeof(uint32_t) * static_cast<size_t>(x.x_hcap), st));
    }
    PoolFree(d->d_slots);
    PoolFree(d->d_slotsx);
    d->d_slots = static_cast<Utt *>(PoolMalloc(sizeof(Utt) * n_slots));
    d->d_slotsx = static_cast<UttX *>(PoolMalloc(sizeof(UttX) * n_slots));
    if (!d->d_slots || !d->d_slotsx) return KH_ENOMEM;
    KH_HIP(hipMemcpyAsync(d->d_slotsx, d->h_slotsx.data(), sizeof(UttX) * n_slots, hipMemcpyHostToDevice, st));
  } else {
    // slots were left with dirty token costs by the previous call: refill
    for (int i = 0; i < n_slots; i++) {
      Utt &u = d->h_slots[i];
      LaunchFillU32(st, (uint32_t *)u.tok_cost.p, static_cast<size_t>(u.tok_cap), kEncInf);
    }
  }
  *n_slots_out = n_slots;
  return KH_OK;
}

// Validates, for every caller of the C-ABI (the Python wrapper checks its host copy of the map as well), that every
// transition-id ON AN ARC of the graph maps to a column of the score matrix (the C++ mirror and direct callers
// used to reach the gathers unchecked).
int BuildArcPdf(KhDecoder *d, Params *p, const int32_t *tid2pdf, int ll_stride, hipStream_t st) {
  const size_t bytes = sizeof(int4) * static_cast<size_t>(d->fst->num_units);
  if (d->rec == nullptr) {
    d->rec = static_cast<int4 *>(PoolMalloc(bytes));
    if (d->rec == nullptr) return KH_ENOMEM;
    KH_HIP(hipMemcpyAsync(d->rec, d->fst->rec, bytes, hipMemcpyDeviceToDevice, st));
  }
  if (d->d_bad == nullptr) {
    d->d_bad = static_cast<int *>(PoolMalloc(sizeof(int) * 4));
    if (d->d_bad == nullptr) return KH_ENOMEM;
  }
  KH_HIP(hipMemsetAsync(d->d_bad, 0, sizeof(int) * 4, st));
  LaunchArcPdf(NumCUs() * 8, st, (const int32_t *)d->fst->unit_ilabel,
                     static_cast<long long>(d->fst->num_units), tid2pdf, d->rec,
                     ll_stride > 0 ? ll_stride : std::numeric_limits<int>::max(),   // (a launch without score rows: InitDecoding / FinalizeDecoding jobs)
                     d->d_bad, (const int4 *)d->fst->rec, d->exact ? 1 : 0);
  KH_LAUNCH_CHECK();
  int bad[4] = {0, 0, 0, 0};
  KH_HIP(hipMemcpyAsync(bad, d->d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  KH_HIP(hipStreamSynchronize(st));
  if (bad[0] != 0) {
    SetError("the transition-id -> pdf map sends transition-id %d (on an arc of the graph) to pdf %d, outside the %d columns of the "
             "log-likelihood matrix", bad[1], bad[2], ll_stride);
    return KH_EINVAL;
  }
  d->rec_order_ids = d->exact ? 1 : 0;
  p->rec = (GP(const KhInt4))d->rec;
  return KH_OK;
}

// OFF by default (0).  With the span on, the serving stress harness saw what it never saw without it: two memory-access
// faults and one workgroup that never left its action in ~45 runs of the two serving legs (15 of 15 clean with the span off
// on the same box, 116 of 116 in round 5) - about one bad collection in several hundred thousand.  The collections
// themselves are the offline kernel's (PruneActiveTokens + full compaction), only far more frequent; the defect has not been
// found, so the switch stays an experiment: KH_SERVE_LAZY_SPAN=128 gives chunk latency max 113 -> 28 ms at 256 streams.
static int OnlineLazySpan(const DecoderEnv &env) { return env.serve_lazy_span; }

void FillParams(const KhDecoder *d, const DecoderEnv &env, Params *pp, int ll_stride, const int32_t *tid2pdf) {
  Params &p = *pp;
  (void)tid2pdf;
  p.rec = (GP(const KhInt4))d->rec;   // (BuildArcPdf allocates it on the first call and sets it again)
  p.n_arcs = (GP(const KhInt4))d->fst->n_arcs;
  p.unit_ilabel = (GP(const int32_t))d->fst->unit_ilabel;
  p.start = d->fst->start;
  p.num_units = static_cast<int32_t>(d->fst->num_units);
  p.num_eps = static_cast<int32_t>(d->fst->num_eps);
  p.start_has_eps = d->fst->start_has_eps;
  p.max_emit = d->fst->max_emit;
  p.lazy_span = 0;
  if (env.no_mid_scan) p.max_emit = 1 << 16;   // (tests: the scan through memory for every frame beyond the LDS tier)
  // the frame's score row fits in LDS (two workgroups per CU share 160 KB): stage it
  // the score row shares the workgroup's 64 KB of LDS with the static block (Shared)
  p.ll_cols = (sizeof(float) * static_cast<size_t>(ll_stride) + DecodeStaticLds() + 256 <= 78 * 1024) ? ll_stride : 0;
  p.keep_ac = 1;
  p.lazy_prune = 0;
  p.exact_order = 0;
  p.hash_ratio = d->cfg.hash_ratio;
  p.cl_max_load = env.closure_cap;
  if (env.no_lds_scores) p.ll_cols = 0;
  p.max_tid = d->fst->max_ilabel;
  p.beam = d->cfg.beam;
  p.lattice_beam = d->cfg.lattice_beam;
  p.beam_delta = d->cfg.beam_delta;
  p.prune_scale = d->cfg.prune_scale;
  p.max_active = d->cfg.max_active;
  p.min_active = d->cfg.min_active;
  p.prune_interval = d->cfg.prune_interval;
}

// The same pool in pinned HOST memory (offline decoding: the kernel writes finished lattices
// there and the host reads them while the kernel keeps running).
int EnsureHostPool(KhDecoder *d, long long pool_tok, long long pool_link) {
  Carver sizer{nullptr};
  sizer.Take<int32_t>(pool_tok); sizer.Take<int32_t>(pool_tok);
  for (int k = 0; k < 4; k++) sizer.Take<int32_t>(pool_link);
  sizer.Take<float>(pool_link); sizer.Take<float>(pool_link);
  if (sizer.off > d->hp_bytes) {
    if (d->hp_slab) (void)hipHostFree(d->hp_slab);
    d->hp_slab = nullptr;
    d->hp_bytes = 0;
    if (hipHostMalloc(&d->hp_slab, sizer.off, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      SetError("kh_decoder_decode: cannot pin %.1f GB of host memory for the lattice pool", sizer.off / 1e9);
      return KH_ENOMEM;
    }
    d->hp_bytes = sizer.off;
  }
  void *dev = nullptr;
  KH_HIP(hipHostGetDevicePointer(&dev, d->hp_slab, 0));
  Carver c{static_cast<char *>(dev)};
  d->hpool.t_frame = c.Take<int32_t>(pool_tok);
  d->hpool.t_state = c.Take<int32_t>(pool_tok);
  d->hpool.l_src = c.Take<int32_t>(pool_link);
  d->hpool.l_dst = c.Take<int32_t>(pool_link);
  d->hpool.l_il = c.Take<int32_t>(pool_link);
  d->hpool.l_ol = c.Take<int32_t>(pool_link);
  d->hpool.l_g = c.Take<float>(pool_link);
  d->hpool.l_a = c.Take<float>(pool_link);
  d->hpool.tok_cap = pool_tok;
  d->hpool.link_cap = pool_link;
  d->hpool.used = (GP(unsigned long long))d->d_used;
  Carver h{static_cast<char *>(d->hp_slab)};
  d->hview.t_frame = (const int32_t *)h.Take<int32_t>(pool_tok);
  d->hview.t_state = (const int32_t *)h.Take<int32_t>(pool_tok);
  d->hview.l_src = (const int32_t *)h.Take<int32_t>(pool_link);
  d->hview.l_dst = (const int32_t *)h.Take<int32_t>(pool_link);
  d->hview.l_il = (const int32_t *)h.Take<int32_t>(pool_link);
  d->hview.l_ol = (const int32_t *)h.Take<int32_t>(pool_link);
  d->hview.l_g = (const float *)h.Take<float>(pool_link);
  d->hview.l_a = (const float *)h.Take<float>(pool_link);
  return KH_OK;
}

// Lattice pool of pool_tok tokens / pool_link links (grown on demand).
int EnsurePool(KhDecoder *d, long long pool_tok, long long pool_link) {
    {
      Carver sizer{nullptr};
      sizer.Take<int32_t>(pool_tok); sizer.Take<int32_t>(pool_tok);
      for (int k = 0; k < 4; k++) sizer.Take<int32_t>(pool_link);
      sizer.Take<float>(pool_link); sizer.Take<float>(pool_link);
      if (sizer.off > d->pool_bytes) {
        PoolFree(d->pool_slab);
        d->pool_slab = PoolMalloc(sizer.off);
        if (!d->pool_slab) { d->pool_bytes = 0; return KH_ENOMEM; }
        d->pool_bytes = sizer.off;
      }
      Carver c{static_cast<char *>(d->pool_slab)};
      d->pool.t_frame = c.Take<int32_t>(pool_tok);
      d->pool.t_state = c.Take<int32_t>(pool_tok);
      d->pool.l_src = c.Take<int32_t>(pool_link);
      d->pool.l_dst = c.Take<int32_t>(pool_link);
      d->pool.l_il = c.Take<int32_t>(pool_link);
      d->pool.l_ol = c.Take<int32_t>(pool_link);
      d->pool.l_g = c.Take<float>(pool_link);
      d->pool.l_a = c.Take<float>(pool_link);
      d->pool.tok_cap = pool_tok;
      d->pool.link_cap = pool_link;
      d->pool.used = (GP(unsigned long long))d->d_used;
    }
  return KH_OK;
}

// One D2H per pool array (the lattices the reference would build on the host in
// GetRawLattice) into a new HostPool.
int FetchPool(KhDecoder *d, const unsigned long long *used, long long pool_tok, long long pool_link, hipStream_t st) {
    d->rounds.emplace_back();
    KhDecoder::HostPool &hp = d->rounds.back();
    const size_t ut = std::min<unsigned long long>(used[0], pool_tok), ul = std::min<unsigned long long>(used[1], pool_link);
    hp.t_frame.resize(ut); hp.t_state.resize(ut);
    hp.l_src.resize(ul); hp.l_dst.resize(ul); hp.l_il.resize(ul); hp.l_ol.resize(ul);
    hp.l_g.resize(ul); hp.l_a.resize(ul);
#define D2H(dst, src, n, type) if (n) KH_HIP(hipMemcpyAsync(dst.data(), src, sizeof(type) * (n), hipMemcpyDeviceToHost, st))
    D2H(hp.t_frame, (int32_t *)d->pool.t_frame, ut, int32_t);
    D2H(hp.t_state, (int32_t *)d->pool.t_state, ut, int32_t);
    D2H(hp.l_src, (int32_t *)d->pool.l_src, ul, int32_t);
    D2H(hp.l_dst, (int32_t *)d->pool.l_dst, ul, int32_t);
    D2H(hp.l_il, (int32_t *)d->pool.l_il, ul, int32_t);
    D2H(hp.l_ol, (int32_t *)d->pool.l_ol, ul, int32_t);
    D2H(hp.l_g, (float *)d->pool.l_g, ul, float);
    D2H(hp.l_a, (float *)d->pool.l_a, ul, float);
#undef D2H
    KH_HIP(hipStreamSynchronize(st));
  return KH_OK;
}

void PrintPhases(const std::vector<long long> &h_phase, int grid, int round, int np, float ms) {
  static const char *names[16] = {"cutoff", "emit_pass1", "emit_pass2", "eps_closure", "eps_links", "clear_hash",
                                  "prune", "compact", "finalize", "export", "", "", "", "", "", "other"};
  long long tot[NPH] = {0};
  long long all = 0;
  for (int i = 0; i < grid; i++)
    for (int k = 0; k < NPH; k++) {
      tot[k] += h_phase[NPH * i + k];
      if (k < 16) all += h_phase[NPH * i + k];
    }
  fprintf(stderr, "[kh_decoder profile] launch %d: %d utterances, kernel %.1f ms, %d slots; share of shader cycles:",
          round, np, ms, grid);
  all -= tot[10] + tot[11] + tot[12] + tot[13] + tot[14];
  all += tot[45];
  for (int k = 0; k < 16; k++)
    if (tot[k] && (k < 10 || k == 15)) fprintf(stderr, " %s=%.1f%%", names[k], 100.0 * tot[k] / all);
  if (tot[47]) fprintf(stderr, " [per frame: %.0f tokens, %.0f with epsilon arcs from the emitting pass, %.0f in all, %.0f epsilon link slots, %.0f tokens from the closure]",
                       double(tot[46]) / tot[47], double(tot[52]) / tot[47], double(tot[53]) / tot[47], double(tot[54]) / tot[47], double(tot[55]) / tot[47]);
  if (tot[45]) fprintf(stderr, " list_order=%.1f%% (ranks + buckets %.1f%%, queue order %.1f%%, replay %.1f%%, positions %.1f%% of it; %lld frames from LDS, %lld by the sort; "
                       "%lld of the %lld candidates under the running cutoff)", 100.0 * tot[45] / all,
                       100.0 * tot[48] / tot[45], 100.0 * tot[49] / tot[45], 100.0 * tot[50] / tot[45], 100.0 * tot[51] / tot[45], tot[56], tot[57], tot[58], tot[31]);
  if (tot[45]) fprintf(stderr, " [frames of <= 8160 / <= 16384 / more tokens: %lld / %lld / %lld; cycles per frame from LDS %.0f, by the sort %.0f; closure order by walks in %lld frames, by the queue in %lld; %lld frames with every intermediate in LDS]",
                       tot[61], tot[62], tot[63], tot[56] + tot[66] ? double(tot[59]) / (tot[56] + tot[66]) : 0.0, tot[57] ? double(tot[60]) / tot[57] : 0.0, tot[64], tot[65], tot[66]);
#ifdef KH_X_STAMPS
  if (tot[47]) {
    fprintf(stderr, "\n[kh_decoder profile] fine stamps, cycles per frame:");
    for (int k = 0; k < 64; k++) if (tot[96 + k]) fprintf(stderr, " %d:%.0f", k, double(tot[96 + k]) / tot[47]);
  }
#endif
  fprintf(stderr, "\n[kh_decoder profile] PruneActiveTokens calls %lld, frames pruned %lld (%.1f per call), tokens scanned "
          "per pruned frame %.0f, eps iterations per pruned frame %.2f, eps-closure rounds %lld\n",
          tot[12], tot[10], tot[12] ? double(tot[10]) / tot[12] : 0.0, tot[10] ? double(tot[11]) / tot[10] : 0.0,
          tot[10] ? double(tot[14]) / tot[10] : 0.0, tot[13]);
  fprintf(stderr, "[kh_decoder profile] prune by frame size: <=1024 tokens: %lld visits, %.1f%% of prune cycles (%.0f cycles each); "
          "larger: %lld visits, %.1f%% (%.0f cycles each)\n",
          tot[18], tot[6] ? 100.0 * tot[16] / tot[6] : 0.0, tot[18] ? double(tot[16]) / tot[18] : 0.0,
          tot[19], tot[6] ? 100.0 * tot[17] / tot[6] : 0.0, tot[19] ? double(tot[17]) / tot[19] : 0.0);
  fprintf(stderr, "[kh_decoder profile] PruneForwardLinks on frames > %d tokens, share of prune cycles: token init %.1f%%, "
          "emitting links %.1f%%, token + epsilon sweeps %.1f%%, excise + flags %.1f%%\n",
          NT, tot[6] ? 100.0 * tot[20] / tot[6] : 0.0, tot[6] ? 100.0 * tot[21] / tot[6] : 0.0,
          tot[6] ? 100.0 * tot[22] / tot[6] : 0.0, tot[6] ? 100.0 * tot[23] / tot[6] : 0.0);
  fprintf(stderr, "[kh_decoder profile] eps closure (thread 0), share of its cycles: list/flag/cost/state/offsets %.1f%%, arcs + wave combine %.1f%%, "
          "FindOrAdd + min + queue %.1f%%, round barrier %.1f%%; tokens processed per round %.1f; frames whose closure ran in LDS %lld, "
          "through the general routine %lld\n",
          tot[3] ? 100.0 * tot[27] / tot[3] : 0.0, tot[3] ? 100.0 * tot[28] / tot[3] : 0.0, tot[3] ? 100.0 * tot[29] / tot[3] : 0.0,
          tot[3] ? 100.0 * tot[30] / tot[3] : 0.0, tot[13] ? double(tot[33]) / tot[13] : 0.0, tot[38], tot[39]);
  fprintf(stderr, "[kh_decoder profile] emitting pass: %lld candidates materialised (%lld counted as accepted in the frames with more than 11000)\n", tot[31], tot[32]);
  fprintf(stderr, "[kh_decoder profile] compaction, share of its cycles: tokens %.1f%%, +inf fill and boundary links %.1f%%, links %.1f%%\n",
          tot[7] ? 100.0 * tot[24] / tot[7] : 0.0, tot[7] ? 100.0 * tot[25] / tot[7] : 0.0, tot[7] ? 100.0 * tot[26] / tot[7] : 0.0);
  fprintf(stderr, "[kh_decoder profile] final backward pass: %lld dense visits, %lld through the general routines, %lld hand-offs through memory; survivors %lld tokens, %lld links\n",
          tot[40], tot[41], tot[42], tot[43], tot[44]);
  fprintf(stderr, "[kh_decoder profile] link compaction: %lld single-chunk barriers, %lld group barriers, %lld slots scanned, %lld links moved\n",
          tot[34], tot[35], tot[36], tot[37]);
}

}  // namespace

extern "C" {

KhFst *kh_fst_create(int32_t num_states, int32_t start, const int64_t *arc_offsets,
                     const int32_t *ilabel, const int32_t *olabel, const float *weight,
                     const int32_t *nextstate, const float *final_cost) {
  if (EnsureDevice() != KH_OK) return nullptr;
  if (num_states <= 0 || start < 0 || start >= num_states || !arc_offsets || !ilabel || !olabel ||
      !weight || !nextstate || !final_cost) {
    SetError("kh_fst_create: bad arguments");
    return nullptr;
  }
  const int64_t na = arc_offsets[num_states];
  std::vector<uint8_t> has_eps(num_states, 0), eps_dst(num_states, 0);
  std::vector<int32_t> unit_of_state(num_states);
  int64_t units = 0, n_eps_total = 0;
  for (int32_t s = 0; s < num_states; s++) {
    unit_of_state[s] = static_cast<int32_t>(units);
    units += 1;
    for (int64_t a = arc_offsets[s]; a < arc_offsets[s + 1]; a++) {
      if (nextstate[a] < 0 || nextstate[a] >= num_states || ilabel[a] < 0) {
        SetError("kh_fst_create: arc %lld out of range", static_cast<long long>(a));
        return nullptr;
      }
      if (ilabel[a] == 0) {
        has_eps[s] = 1;
        eps_dst[nextstate[a]] = 1;
        n_eps_total++;
      } else {
        units++;
      }
    }
    // the kernels address the tables with 32-bit byte offsets (Arr<T>), 16 bytes per unit, and a
    // state id (= unit index) shares its word with two flag bits
    if (units >= (int64_t(1) << 28) || n_eps_total >= (int64_t(1) << 28)) {
      SetError("kh_fst_create: %lld states + emitting arcs exceed the 2^28 units a 32-bit byte offset reaches", static_cast<long long>(units));
      return nullptr;
    }
  }
  static_assert(kStateMask >= (1 << 28) - 1, "unit ids must fit the state field of an arc");
  std::vector<int4> rec(static_cast<size_t>(units)), n_arcs;
  std::vector<int32_t> unit_ilabel(static_cast<size_t>(units), 0);   // (every unit is written below)
  n_arcs.reserve(static_cast<size_t>(n_eps_total));
  int32_t max_il = 0, max_emit = 0;
  for (int32_t s = 0; s < num_states; s++) {
    const int32_t base = unit_of_state[s], eps_base = static_cast<int32_t>(n_arcs.size());
    int32_t ne = 0;
    for (int64_t a = arc_offsets[s]; a < arc_offsets[s + 1]; a++) {
      int wbits;
      memcpy(&wbits, &weight[a], 4);
      const int32_t ns = unit_of_state[nextstate[a]] | (has_eps[nextstate[a]] ? kHasEps : 0) | (eps_dst[nextstate[a]] ? kEpsDst : 0);
      if (ilabel[a] != 0) {
        ne++;
        rec[static_cast<size_t>(base) + ne] = make_int4(ilabel[a], olabel[a], wbits, ns);
        unit_ilabel[static_cast<size_t>(base) + ne] = ilabel[a];
        max_il = std::max(max_il, ilabel[a]);
      } else {
        n_arcs.push_back(make_int4(0, olabel[a], wbits, ns));
      }
    }
    int fbits;
    memcpy(&fbits, &final_cost[s], 4);
    rec[base] = make_int4(ne, eps_base, static_cast<int32_t>(n_arcs.size()) - eps_base, fbits);
    unit_ilabel[base] = -1 - s;
    max_emit = std::max(max_emit, ne);
  }
  KhFst *f = new KhFst();
  f->num_states = num_states;
  f->start = unit_of_state[start];
  f->start_state = start;
  f->num_arcs = na;
  f->num_units = units;
  f->num_emit = units - num_states;
  f->num_eps = static_cast<int64_t>(n_arcs.size());
  f->max_ilabel = max_il;
  f->max_emit = max_emit;
  f->final_host.assign(final_cost, final_cost + num_states);
  f->start_has_eps = has_eps[start];
  auto up = [&](void **dst, const void *src, size_t bytes) -> bool {
    *dst = PoolMalloc(bytes ? bytes : 16);
    if (!*dst) return false;
    if (bytes && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      SetError("kh_fst_create: upload failed");
      return false;
    }
    return true;
  };
  bool ok = up(reinterpret_cast<void **>(&f->rec), rec.data(), sizeof(int4) * rec.size()) &&
            up(reinterpret_cast<void **>(&f->unit_ilabel), unit_ilabel.data(), sizeof(int32_t) * unit_ilabel.size()) &&
            up(reinterpret_cast<void **>(&f->n_arcs), n_arcs.data(), sizeof(int4) * n_arcs.size());
  if (!ok) {
    kh_fst_destroy(f);
    return nullptr;
  }
  return f;
}

void kh_fst_destroy(KhFst *f) {
  if (!f) return;
  PoolFree(f->rec);
  PoolFree(f->unit_ilabel);
  PoolFree(f->n_arcs);
  delete f;
}

int64_t kh_fst_num_arcs(const KhFst *f) { return f ? f->num_arcs : 0; }

// The decode kernels gather tid2pdf[ilabel] and loglikes[t, pdf] unchecked: this validates,
// once per (graph, pdf map, model), what DecodableAmNnet / TransitionModel assert per call
// (decodable-am-nnet.h:76-78 "KALDI_ASSERT(transition_id ...)", transition-model.h:312).
// tid2pdf_host: HOST copy of the map, or NULL for the identity-minus-one map.
int kh_fst_check_pdf_map(const KhFst *f, const int32_t *tid2pdf_host, int n_tid2pdf, int num_cols) {
  KH_CHECK_ARG(f && num_cols > 0);
  if (!tid2pdf_host) {
    if (f->max_ilabel > num_cols) {
      SetError("kh_fst_check_pdf_map: largest ilabel %d of the graph exceeds the %d columns of the log-likelihood matrix",
               f->max_ilabel, num_cols);
      return KH_EINVAL;
    }
    return KH_OK;
  }
  if (f->max_ilabel >= n_tid2pdf) {
    SetError("kh_fst_check_pdf_map: largest ilabel %d of the graph is outside the transition-id -> pdf map (%d entries)",
             f->max_ilabel, n_tid2pdf);
    return KH_EINVAL;
  }
  for (int t = 1; t <= f->max_ilabel; t++)
    if (tid2pdf_host[t] < 0 || tid2pdf_host[t] >= num_cols) {
      SetError("kh_fst_check_pdf_map: transition-id %d maps to pdf %d, outside the %d columns of the log-likelihood matrix",
               t, tid2pdf_host[t], num_cols);
      return KH_EINVAL;
    }
  return KH_OK;
}

void kh_decoder_config_default(KhDecoderConfig *c) {
  c->beam = 16.0f;
  c->max_active = std::numeric_limits<int32_t>::max();
  c->min_active = 200;
  c->lattice_beam = 10.0f;
  c->prune_interval = 25;
  c->beam_delta = 0.5f;
  c->hash_ratio = 2.0f;
  c->prune_scale = 0.1f;
}

KhDecoder *kh_decoder_create(const KhFst *fst, const KhDecoderConfig *cfg, int max_batch,
                             int max_frames) {
  const DecoderEnv env = ReadDecoderEnv();
  if (EnsureDevice() != KH_OK) return nullptr;
  if (!fst || !cfg || max_batch <= 0 || max_frames <= 0) {
    SetError("kh_decoder_create: bad arguments");
    return nullptr;
  }
  // LatticeFasterDecoderConfig::Check() lattice-faster-decoder.h:89-94
  if (!(cfg->beam > 0.0 && cfg->max_active > 1 && cfg->lattice_beam > 0.0 && cfg->prune_interval > 0 &&
        cfg->beam_delta > 0.0 && cfg->hash_ratio >= 1.0 && cfg->prune_scale > 0.0 && cfg->prune_scale < 1.0)) {
    SetError("kh_decoder_create: LatticeFasterDecoderConfig::Check() failed");
    return nullptr;
  }
  KhDecoder *d = new KhDecoder();
  d->fst = fst;
  d->cfg = *cfg;
  d->max_batch = max_batch;
  d->max_frames = max_frames;
  // Per-frame caps (the temporaries of a frame): the reference has no limit; a frame that
  // exceeds them reports an overflow and its utterance is decoded again with doubled arenas.
  // max_active bounds the tokens that EXPAND, not the tokens they create: a language-model
  // state of an HCLG has hundreds of arcs, and frames of 40 k new tokens occur at
  // max-active 7000.
  const long long tf = env.tokens_per_frame;
  d->tok_frame_cap = static_cast<int>(tf);
  // tokens a frame is sized for in the hash (hash_ratio x this many entries): what a frame typically
  // holds - the reference resizes to hash_ratio x the previous frame's count (:219-225), which
  // max_active bounds before the closure adds to it - not the per-frame capacity; the table never
  // has fewer entries than that capacity (CarveSlot), so every token of a frame finds a slot
  d->expected_tokens = cfg->max_active == std::numeric_limits<int32_t>::max()
                           ? d->tok_frame_cap
                           : static_cast<int>(std::min<long long>(d->tok_frame_cap, cfg->max_active + cfg->max_active / 2));
  if (env.hash_tokens.set) d->expected_tokens = env.hash_tokens.v;
  long long lf = 4 * tf;
  if (env.links_per_frame.set) lf = env.links_per_frame.v;
  d->link_frame_cap = static_cast<int>(lf);
  // average frame the compaction window is sized for
  long long wt = cfg->max_active == std::numeric_limits<int32_t>::max()
                     ? tf : std::min<long long>(tf, std::max<long long>(4096, 2ll * cfg->max_active));
  if (env.window_tokens_per_frame.set) wt = env.window_tokens_per_frame.v;
  d->win_tok = static_cast<int>(wt);
  long long wl = std::min<long long>(lf, 4 * wt);
  if (env.window_links_per_frame.set) wl = env.window_links_per_frame.v;
  d->win_link = static_cast<int>(wl);
  d->max_slots = NumCUs() * KH_WG_PER_CU;  // persistent workgroups
  if (env.slots.set) d->max_slots = env.slots.v;
  return d;
}

int kh_decoder_set_determinize(KhDecoder *d, int enable, double beam, float delta, int64_t max_mem, const int32_t *tid_phone,
                               int n_tid, int phone_determinize, int word_determinize, int minimize) {
  KH_CHECK_ARG(d && (!enable || beam > 0.0) && (!enable || !phone_determinize || (tid_phone && n_tid > 0)));
  d->det_enable = enable != 0;
  d->det_beam = beam;
  d->det_delta = delta;
  d->det_max_mem = max_mem;
  d->det_phone = phone_determinize != 0;
  d->det_word = word_determinize != 0;
  d->det_minimize = minimize != 0;
  d->det_tid_phone.assign(tid_phone ? tid_phone : nullptr, tid_phone ? tid_phone + n_tid : nullptr);
  return KH_OK;
}

const KhCompactLattice *kh_decoder_get_compact_lattice(KhDecoder *d, int utt) {
  if (!d || utt < 0 || utt >= d->n_utts || !d->det_enable) {
    SetError("kh_decoder_get_compact_lattice: bad arguments (or kh_decoder_set_determinize was not called)");
    return nullptr;
  }
  if (DeterminizeUtt(d, utt) != KH_OK) return nullptr;
  return d->clats[utt];
}

int kh_decoder_compact_lattice_totals(KhDecoder *d, int64_t *totals) {
  KH_CHECK_ARG(d && totals && d->det_enable);
  totals[0] = totals[1] = totals[2] = totals[3] = 0;
  for (int u = 0; u < d->n_utts; u++) {
    if (d->h_out[u].stats.status != 0) continue;
    if (DeterminizeUtt(d, u) != KH_OK) return KH_EINVAL;
    int32_t ns, na, nl, nf, comp;
    kh_compact_lattice_sizes(d->clats[u], &ns, &na, &nl, &nf, &comp);
    totals[0] += ns; totals[1] += na; totals[2] += nl + nf; totals[3] += comp ? 0 : 1;
  }
  return KH_OK;
}

void kh_decoder_destroy(KhDecoder *d) {
  if (!d) return;
  d->FreeClats();
  PoolFree(d->slab);
  PoolFree(d->pool_slab);
  PoolFree(d->d_slots);
  PoolFree(d->d_slotsx);
  PoolFree(d->d_in);
  PoolFree(d->d_out);
  PoolFree(d->d_used);
  PoolFree(d->d_phase);
  PoolFree(d->rec);
  PoolFree(d->d_bad);
  if (d->hp_slab) (void)hipHostFree(d->hp_slab);
  if (d->h_out_pinned) (void)hipHostFree(d->h_out_pinned);
  if (d->h_done) (void)hipHostFree(d->h_done);
  delete d;
}

int kh_decoder_decode(KhDecoder *d, const float *loglikes, int ll_stride,
                      const int32_t *utt_off, int n_utts, const int32_t *tid2pdf) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(d && loglikes && utt_off && n_utts > 0 && n_utts <= d->max_batch && ll_stride > 0);
  hipStream_t st = Stream();
  const bool tprof = env.profile;
  auto tnow = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_enter = tnow();
  d->n_utts = n_utts;
  d->lats.assign(n_utts, KhDecoder::Lat());
  d->FreeClats();
  d->clats.assign(n_utts, nullptr);
  d->h_T.resize(n_utts);
  int T_max = 0;
  long long tot_frames = 0;
  for (int i = 0; i < n_utts; i++) {
    const int T = utt_off[i + 1] - utt_off[i];
    KH_CHECK_ARG(T > 0 && T <= d->max_frames);
    d->h_T[i] = T;
    T_max = std::max(T_max, T);
    tot_frames += T;
  }
  if (!d->d_in) {
    d->d_in = static_cast<UttIn *>(PoolMalloc(sizeof(UttIn) * d->max_batch));
    d->d_out = static_cast<UttOut *>(PoolMalloc(sizeof(UttOut) * d->max_batch));
    d->d_used = static_cast<unsigned long long *>(PoolMalloc(sizeof(unsigned long long) * 4));
    if (!d->d_in || !d->d_out || !d->d_used) return KH_ENOMEM;
    if (env.profile) {
      d->d_phase = static_cast<long long *>(PoolMalloc(sizeof(long long) * NPH * d->max_slots));
      if (!d->d_phase) return KH_ENOMEM;
    }
  }
  if (!d->h_out_pinned) {
    if (hipHostMalloc(reinterpret_cast<void **>(&d->h_out_pinned), sizeof(UttOut) * d->max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&d->h_done), sizeof(int32_t) * d->max_batch, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      SetError("kh_decoder_decode: cannot allocate pinned host memory");
      return KH_ENOMEM;
    }
  }
  // the graph's transition-ids and pdfs must lie inside the tables they index (the kernel
  // gathers tid2pdf[ilabel] and the score row unchecked)
  if (tid2pdf == nullptr && d->fst->max_ilabel > ll_stride) {
    SetError("kh_decoder_decode: the graph's largest ilabel %d exceeds the %d columns of the log-likelihood matrix",
             d->fst->max_ilabel, ll_stride);
    return KH_EINVAL;
  }
  // ---- queue order: longest first (greedy LPT over the persistent workgroups)
  d->order.resize(n_utts);
  for (int i = 0; i < n_utts; i++) d->order[i] = i;
  std::stable_sort(d->order.begin(), d->order.end(),
                   [&](int a, int b) { return d->h_T[a] > d->h_T[b]; });
  Params p;
  FillParams(d, env, &p, ll_stride, tid2pdf);
  // the whole score matrix stays in place until the lattices are exported: the acoustic costs of the links
  // are recomputed there instead of stored (KH_DECODER_KEEP_AC=1: stored, as the online decoder has to)
  p.keep_ac = env.keep_ac ? 1 : 0;
  // backward pruning on demand (Params::lazy_prune); KH_DECODER_PRUNE_SCHEDULE=interval: every prune_interval frames
  p.lazy_prune = env.prune_interval_schedule ? 0 : 1;
  d->lazy = p.lazy_prune;
  d->alloc_link_a = p.keep_ac;
  // the reference's own iteration order (kh_decoder_set_reference_order; KH_DECODER_ORDER=reference|canonical overrides)
  {
    const int ex = env.order >= 0 ? env.order : d->exact;
    d->exact = ex;
    p.exact_order = ex;
    // KH_DECODER_ORDER_SORT=1: list positions by the comparison-free radix sort of rounds 4 (OrderFrontierSort) in every
    // frame - the path frames beyond the LDS construction's capacity take; the tests run the suites through it
    if (ex && env.order_sort) p.exact_order = 2;
  }
  if ((rc = BuildArcPdf(d, &p, tid2pdf, ll_stride, Stream()))) return rc;
  if (!d->ev0) {
    KH_HIP(hipEventCreate(&d->ev0));
    KH_HIP(hipEventCreate(&d->ev1));
  }
  d->h_out.assign(n_utts, UttOut());
  d->h_round.assign(n_utts, 0);
  d->rounds.clear();
  d->last_kernel_ms = 0.f;
  d->last_host_tail_ms = 0.f;
  // lattice pool in pinned host memory: ~3 x the density the recipe's options give on the
  // structured workload (17 states / 27 arcs per frame); an utterance that does not fit reports
  // its exact size and is decoded again
  long long tok_per_frame = 48, link_per_frame = 80;
  if (env.pool_tokens_per_frame.set) {
    tok_per_frame = env.pool_tokens_per_frame.v;
    link_per_frame = tok_per_frame * 3 / 2;
  }
  std::vector<int> pending(d->order);
  int n_workers = static_cast<int>(std::thread::hardware_concurrency());
  // never more threads than the CPU time the container may use (cgroup quota: beyond it the kernel throttles the whole
  // group, and every thread stalls)
  n_workers = std::max(1, std::min(std::min(n_workers, std::min(64, HostCpuQuota())), n_utts));
  n_workers = EnvHostThreads(env, n_workers);
  if (static_cast<int>(d->arenas.size()) < n_workers) d->arenas.resize(n_workers);
  for (auto &a : d->arenas) a.Reset();
  // Two things are sized from estimates, and an utterance that outgrows either is decoded
  // again in a further launch while the finished ones are kept:
  //  * the lattice pool (status 6): the utterance reports its exact size, the next pool has it;
  //  * the slot arenas (status 1-4: tokens / links per frame, window): the next launch runs
  //    with arenas twice as large (the reference has no such limits).
  // An utterance that still overflows at 16 x the default arenas is left failed (its stats
  // carry the status; the getters return KH_ECAPACITY for it) - the caller counts it like the
  // reference counts a failed Decode() (num_fail, nnet-latgen-faster.cc:170).
  long long need_tok = 0, need_link = 0;
  int scale = 1;
  const int kMaxScale = 16;
  bool pool_exact = false;
  bool hook_called = false;   // kh_decoder_set_after_launch: once per call, after the last launch
  for (int round = 0; !pending.empty(); round++) {
    if (round > 8) {
      SetError("kh_decoder_decode: %d utterances still unfinished after %d launches", static_cast<int>(pending.size()), round);
      return KH_ECAPACITY;
    }
    const int np = static_cast<int>(pending.size());
    long long frames = 0;
    int T_round = 0;
    for (int ui : pending) { frames += d->h_T[ui]; T_round = std::max(T_round, d->h_T[ui]); }
    // ---- slot arenas
    int n_slots = 0;
    rc = EnsureSlots(d, env, std::min(np, d->max_slots), scale == 1 ? T_max : T_round, st, &n_slots, scale);
    if (rc) return rc;
    for (int i = 0; i < n_slots; i++) d->h_slots[i].ll_stride = ll_stride;
    KH_HIP(hipMemcpyAsync(d->d_slots, d->h_slots.data(), sizeof(Utt) * n_slots, hipMemcpyHostToDevice, st));
    const long long pool_tok = !pool_exact ? frames * tok_per_frame + 65536 : need_tok + 1024;
    const long long pool_link = !pool_exact ? frames * link_per_frame + 131072 : need_link + 1024;
    rc = EnsureHostPool(d, pool_tok, pool_link);
    if (rc) return rc;
    std::vector<UttIn> h_in(np);
    for (int q = 0; q < np; q++) {
      const int ui = pending[q];
      h_in[q].ll = (GP(const float))(loglikes + static_cast<size_t>(utt_off[ui]) * ll_stride);
      h_in[q].T = d->h_T[ui];
      h_in[q].pad = 0;
    }
    KH_HIP(hipMemcpyAsync(d->d_in, h_in.data(), sizeof(UttIn) * np, hipMemcpyHostToDevice, st));
    KH_HIP(hipMemsetAsync(d->d_used, 0, sizeof(unsigned long long) * 4, st));
    if (round > 0)
      for (int i = 0; i < n_slots; i++)
        LaunchFillU32(st, (uint32_t *)d->h_slots[i].tok_cost.p, static_cast<size_t>(d->h_slots[i].tok_cap), kEncInf);
    const int grid = std::min(np, n_slots);
    for (int q = 0; q < np; q++) d->h_done[q] = -1;
    void *d_out_dev = nullptr, *d_done_dev = nullptr;
    KH_HIP(hipHostGetDevicePointer(&d_out_dev, d->h_out_pinned, 0));
    KH_HIP(hipHostGetDevicePointer(&d_done_dev, d->h_done, 0));
    KH_HIP(hipEventRecord(d->ev0, st));
    LaunchDecode(p.lazy_prune != 0, p.exact_order != 0, grid, DynLdsBytes(p.ll_cols), st, d->d_slots, d->d_in,
                 static_cast<UttOut *>(d_out_dev), np, d->hpool, p, (GP(long long))d->d_phase, (GP(int32_t))d_done_dev,
                 (const UttX *)d->d_slotsx);
    KH_LAUNCH_CHECK();
    KH_HIP(hipEventRecord(d->ev1, st));
    // ---- host threads: canonical lattice + best path of every utterance as it completes
    // (GetRawLattice + GetBestPath, decoder-wrappers.cc:215-262), overlapped with the kernel
    std::atomic<int> next_done(0);
    std::atomic<bool> kernel_done(false);
    const int round_now = round;
    (void)round_now;
    auto worker = [&](int w) {
      for (;;) {
        const int i = next_done.fetch_add(1);
        if (i >= np) break;
        int q;
        for (;;) {
          q = __atomic_load_n(&d->h_done[i], __ATOMIC_ACQUIRE);
          if (q >= 0) break;
          if (kernel_done.load()) {
            q = __atomic_load_n(&d->h_done[i], __ATOMIC_ACQUIRE);
            break;
          }
          std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        if (q < 0) break;  // the kernel ended without this completion (launch failure)
        const UttOut qo = d->h_out_pinned[q];
        if (qo.stats.status != 0) continue;  // decoded again in a later launch, or left failed
        const int ui = pending[q];
        d->h_out[ui] = qo;
        d->h_round[ui] = -1;
        KhDecoder::Lat &L = d->lats[ui];
        KhDecoder::Arena &A = d->arenas[w];
        const size_t cn = qo.n_tok, cm = qo.n_link;
        L.state_frame.bind(static_cast<int32_t *>(A.Take(4 * cn)), cn); L.state_hclg.bind(static_cast<int32_t *>(A.Take(4 * cn)), cn);
        L.state_final.bind(static_cast<float *>(A.Take(4 * cn)), cn);
        L.arc_src.bind(static_cast<int32_t *>(A.Take(4 * cm)), cm); L.arc_dst.bind(static_cast<int32_t *>(A.Take(4 * cm)), cm);
        L.arc_il.bind(static_cast<int32_t *>(A.Take(4 * cm)), cm); L.arc_ol.bind(static_cast<int32_t *>(A.Take(4 * cm)), cm);
        L.arc_g.bind(static_cast<float *>(A.Take(4 * cm)), cm); L.arc_a.bind(static_cast<float *>(A.Take(4 * cm)), cm);
        (void)ComputeBestPath(d, env, ui);  // (an utterance without a best path reports it from its getter)
        if (d->det_enable) (void)DeterminizeUtt(d, ui);
      }
    };
    // (joined on every exit path; a D2H copy into pageable memory would block this thread until
    // the kernel has finished, so nothing of that kind is issued before the stream is idle)
    struct Workers {
      std::vector<std::thread> th;
      std::atomic<bool> *done;
      ~Workers() {
        done->store(true);
        for (auto &t : th) t.join();
      }
    } workers{{}, &kernel_done};
    const bool overlap = !env.no_host_overlap;
    const double t_launched = tnow();
    if (overlap)
      for (int w = 0; w < n_workers; w++) workers.th.emplace_back(worker, w);
    std::vector<UttOut> q_out(np);
    unsigned long long used[4] = {0, 0, 0, 0};
    // wait for the kernel without spinning on a core (hipStreamSynchronize busy-waits): the completion threads need the
    // CPUs - every one of them where the container's quota is 16 for one GPU, and all the more with eight ranks on a node
    hipError_t sync_err = hipSuccess;
    if (overlap) {
      while ((sync_err = hipEventQuery(d->ev1)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(200));
      if (sync_err == hipSuccess) sync_err = hipStreamSynchronize(st);
    } else {
      sync_err = hipStreamSynchronize(st);
    }
    const double t_synced = tnow();
    kernel_done.store(true);
    // the few words the host still wants from the device, while the stream is idle (the caller's turn below may queue a
    // whole forward pass on it: nothing of this call waits behind that)
    std::vector<long long> h_phase;
    if (sync_err == hipSuccess) {
      sync_err = hipMemcpyAsync(used, d->d_used, sizeof(used), hipMemcpyDeviceToHost, st);
      if (sync_err == hipSuccess && d->d_phase) {
        h_phase.resize(NPH * static_cast<size_t>(grid));
        sync_err = hipMemcpyAsync(h_phase.data(), d->d_phase, sizeof(long long) * NPH * grid, hipMemcpyDeviceToHost, st);
      }
      if (sync_err == hipSuccess) sync_err = hipStreamSynchronize(st);
    }
    for (int q = 0; q < np; q++) q_out[q] = d->h_out_pinned[q];
    // The caller's turn (kh_decoder_set_after_launch): the LAST decode kernel of this call has finished - no utterance is
    // waiting to be decoded again from the score matrix (an arena or pool overflow: the loop below), and with
    // Params::keep_ac == 0 the export inside the kernel was the last reader of the scores - while the completion threads
    // still build / determinize this batch's lattices.  Work the hook enqueues (the next batch's forward pass, into the
    // same score buffer if the caller likes) overlaps that host tail.
    if (sync_err == hipSuccess && d->after_launch != nullptr && !hook_called) {
      bool again = false;
      for (int q = 0; q < np && !again; q++) {
        const int s6 = q_out[q].stats.status;
        again = s6 == 6 || (s6 != 0 && scale < kMaxScale);
      }
      if (!again) {
        hook_called = true;
        d->after_launch(d->after_launch_arg);
      }
    }
    if (!overlap)
      for (int w = 0; w < n_workers; w++) workers.th.emplace_back(worker, w);
    for (auto &t : workers.th) t.join();
    workers.th.clear();
    d->last_host_tail_ms += static_cast<float>(tnow() - t_synced);
    if (tprof)
      fprintf(stderr, "[kh_decoder profile] host: %.1f ms before the launch returned, %.1f ms until the stream was idle, %.1f ms more for the host threads (%d)\n",
              t_launched - t_enter, t_synced - t_launched, tnow() - t_synced, n_workers);
    if (sync_err != hipSuccess) {
      SetError("kh_decoder_decode: %s", hipGetErrorString(sync_err));
      return KH_EDEVICE;
    }
    float ms = 0.f;
    KH_HIP(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    d->last_kernel_ms += ms;
#ifdef KH_BOUNDS_CHECK
    {
      int h[8];
      KH_HIP(ReadOob(h));
      fprintf(stderr, "[kh bounds check] violations=%d first: code=%d v=%d lo=%d hi=%d thread=%d\n", h[0], h[1], h[2], h[3], h[4], h[5]);
      KH_HIP(ClearOob());
    }
#endif
#ifdef KH_BARRIER_CHECK
    {
      int h[4];
      KH_HIP(ReadBarMisaligned(h));
      fprintf(stderr, "[kh barrier check] mismatches=%d first: n=%d neighbour=%d wave=%d\n", h[0], h[1], h[2], h[3]);
      KH_HIP(ClearBarMisaligned());
    }
#endif
    if (d->d_phase) PrintPhases(h_phase, grid, round, np, ms);
    std::vector<int> next;
    need_tok = need_link = 0;
    bool grow = false, pool_short = false;
    int n_failed = 0;
    static const char *what[] = {"", "token arena / tokens-per-frame cap", "link arena", "links-per-frame cap",
                                 "compaction window", "LDS token table", "lattice pool", "survivor lists",
                                 "closure replay (insertions do not match the closure's tokens: a defect, not a capacity)"};
    for (int q = 0; q < np; q++) {
      const int ui = pending[q];
      const KhDecodeStats &hs = q_out[q].stats;
      if (hs.status == 6) {  // lattice did not fit in the pool: exact size is known now
        next.push_back(ui);
        need_tok += q_out[q].n_tok;
        need_link += q_out[q].n_link;
        pool_short = true;
        continue;
      }
      if (hs.status != 0) {
        if (scale < kMaxScale) {
          next.push_back(ui);
          grow = true;
          if (env.profile)
            fprintf(stderr, "[kh_decoder profile] utterance %d overflowed the %s at frame %d (scale %d): decoded again with 2 x the arenas\n",
                    ui, what[std::min(std::max(hs.status, 0), 8)], hs.num_frames, scale);
          continue;
        }
        // give up on this utterance only
        n_failed++;
        SetError("kh_decoder_decode: utterance %d overflowed the %s at frame %d even with %d x the default arenas "
                 "(tokens/frame cap %d, links/frame cap %d); see KH_DECODER_TOKENS_PER_FRAME / "
                 "KH_DECODER_LINKS_PER_FRAME / KH_DECODER_STABLE_TOKENS_PER_FRAME",
                 ui, what[std::min(std::max(hs.status, 0), 8)], hs.num_frames, scale, d->tok_frame_cap, d->link_frame_cap);
      }
      if (hs.status != 0) {  // left failed: its counters and status are what the getters report
        d->h_out[ui] = q_out[q];
        d->h_round[ui] = -1;
      }
    }
    (void)used;
    // Another launch follows and will write its lattices over this one's in the pool: the canonical lattices of the
    // utterances that finished in this launch are built now (they are otherwise built on first access, from the pool).
    if (!next.empty()) {
      std::vector<int> keep;
      for (int q = 0; q < np; q++)
        if (q_out[q].stats.status == 0 && !d->lats[pending[q]].built) keep.push_back(pending[q]);
      std::atomic<int> nk(0);
      auto build = [&]() {
        for (;;) {
          const int i = nk.fetch_add(1);
          if (i >= static_cast<int>(keep.size())) break;
          (void)BuildLattice(d, keep[i]);   // (an error is reported again by the getter that asks for the lattice)
        }
      };
      std::vector<std::thread> th;
      for (int w = 1; w < std::min<int>(n_workers, static_cast<int>(keep.size())); w++) th.emplace_back(build);
      build();
      for (auto &t : th) t.join();
    }
    // the utterances that need larger arenas have no lattice size yet: estimate again
    pool_exact = pool_short && !grow;
    if (grow) scale *= 2;
    pending.swap(next);
  }
  if (d->slab_scale != 1) {  // enlarged arenas are not kept: the next batch starts from the defaults
    PoolFree(d->slab);
    d->slab = nullptr;
    d->slab_bytes = 0;
    d->slab_slots = 0;
    d->slab_T = 0;
    d->slab_scale = 1;
  }
  return KH_OK;
}

int kh_decoder_set_reference_order(KhDecoder *d, int enable) {
  KH_CHECK_ARG(d);
  d->exact = enable != 0;
  return KH_OK;
}

int kh_decoder_get_search_counters(const KhDecoder *d, int utt, int64_t *counters) {
  KH_CHECK_ARG(d && counters && utt >= -1 && utt < d->n_utts);
  counters[0] = 0;
  for (int u = std::max(utt, 0); u < (utt < 0 ? d->n_utts : utt + 1); u++) counters[0] += d->h_out[u].cand_mat;
  counters[1] = d->exact;
  return KH_OK;
}

int kh_decoder_set_after_launch(KhDecoder *d, void (*fn)(void *), void *arg) {
  KH_CHECK_ARG(d);
  d->after_launch = fn;
  d->after_launch_arg = arg;
  return KH_OK;
}

int kh_decoder_last_host_tail_ms(const KhDecoder *d, float *ms) {
  KH_CHECK_ARG(d && ms);
  *ms = d->last_host_tail_ms;
  return KH_OK;
}

int kh_decoder_last_kernel_ms(const KhDecoder *d, float *ms) {
  KH_CHECK_ARG(d && ms);
  *ms = d->last_kernel_ms;
  return KH_OK;
}

// Raw per-utterance counters of the last decode (no lattice export).
int kh_decoder_get_schedule_counters(const KhDecoder *d, int utt, int32_t *counters) {
  KH_CHECK_ARG(d && counters && utt >= 0 && utt < d->n_utts);
  for (int i = 0; i < 4; i++) counters[i] = d->h_out[utt].sched[i];
  return KH_OK;
}

int kh_decoder_get_counters(const KhDecoder *d, int utt, KhDecodeStats *stats) {
  KH_CHECK_ARG(d && stats && utt >= 0 && utt < d->n_utts);
  *stats = d->h_out[utt].stats;
  return KH_OK;
}

int kh_decoder_get_stats(const KhDecoder *dc, int utt, KhDecodeStats *stats) {
  KhDecoder *d = const_cast<KhDecoder *>(dc);
  KH_CHECK_ARG(d && stats && utt >= 0 && utt < d->n_utts);
  // the raw lattice's sizes are those of the export (the canonical lattice keeps every exported token and link)
  if (d->h_out[utt].stats.status != 0) {
    SetError("utterance %d: decoder failed (code %d: %s)", utt, d->h_out[utt].stats.status, StatusText(d->h_out[utt].stats.status));
    return KH_ECAPACITY;
  }
  *stats = d->h_out[utt].stats;
  stats->num_tokens = static_cast<int32_t>(d->h_out[utt].n_tok);
  stats->num_links = static_cast<int32_t>(d->h_out[utt].n_link);
  return KH_OK;
}

int kh_decoder_get_raw_lattice(const KhDecoder *dc, int utt, int32_t *state_frame,
                               int32_t *state_hclg, float *state_final, int32_t *arc_src,
                               int32_t *arc_dst, int32_t *arc_ilabel, int32_t *arc_olabel,
                               float *arc_graph, float *arc_acoustic) {
  KhDecoder *d = const_cast<KhDecoder *>(dc);
  KH_CHECK_ARG(d && utt >= 0 && utt < d->n_utts);
  int rc = BuildLattice(d, utt);
  if (rc) return rc;
  const KhDecoder::Lat &L = d->lats[utt];
  const size_t n = L.state_frame.size(), m = L.arc_src.size();
  if (state_frame) memcpy(state_frame, L.state_frame.data(), 4 * n);
  if (state_hclg) memcpy(state_hclg, L.state_hclg.data(), 4 * n);
  if (state_final) memcpy(state_final, L.state_final.data(), 4 * n);
  if (arc_src) memcpy(arc_src, L.arc_src.data(), 4 * m);
  if (arc_dst) memcpy(arc_dst, L.arc_dst.data(), 4 * m);
  if (arc_ilabel) memcpy(arc_ilabel, L.arc_il.data(), 4 * m);
  if (arc_olabel) memcpy(arc_olabel, L.arc_ol.data(), 4 * m);
  if (arc_graph) memcpy(arc_graph, L.arc_g.data(), 4 * m);
  if (arc_acoustic) memcpy(arc_acoustic, L.arc_a.data(), 4 * m);
  return KH_OK;
}

// GetBestPath :99-105 = fst::ShortestPath on the raw lattice +
// GetLinearSymbolSequence (decoder-wrappers.cc:232-246).  Host-side, as in the
// reference.  Tie rule (OpenFst leaves exact ties to its state numbering, which
// is arbitrary in the reference): strictly better LatticeWeight wins; on an exact
// tie the smaller canonical arc index, then the smaller final state index.
int kh_decoder_get_best_path(const KhDecoder *dc, int utt, int32_t *alignment, int cap_ali,
                             int32_t *n_ali, int32_t *words, int cap_words, int32_t *n_words,
                             float *graph_cost, float *acoustic_cost) {
  const DecoderEnv env = ReadDecoderEnv();
  KhDecoder *d = const_cast<KhDecoder *>(dc);
  KH_CHECK_ARG(d && utt >= 0 && utt < d->n_utts && n_ali && n_words && graph_cost && acoustic_cost);
  int rc = ComputeBestPath(d, env, utt);
  if (rc) return rc;
  const KhDecoder::Lat &L = d->lats[utt];
  const int a = static_cast<int>(L.bp_ali.size()), w = static_cast<int>(L.bp_words.size());
  *n_ali = a;
  *n_words = w;
  if ((alignment && a > cap_ali) || (words && w > cap_words)) {
    SetError("kh_decoder_get_best_path: buffers too small (alignment %d > %d or words %d > %d)", a, cap_ali, w, cap_words);
    return KH_EINVAL;
  }
  if (alignment) memcpy(alignment, L.bp_ali.data(), sizeof(int32_t) * std::min(a, std::max(cap_ali, 0)));
  if (words) memcpy(words, L.bp_words.data(), sizeof(int32_t) * std::min(w, std::max(cap_words, 0)));
  *n_ali = a;
  *n_words = w;
  *graph_cost = L.bp_graph;
  *acoustic_cost = L.bp_acoustic;
  return KH_OK;
}

// The same for utterances [first, first + n) in one call: alignments and word sequences row-concatenated
// (ali_off / words_off: n + 1 offsets), costs per utterance.  A caller that loops over a test set in C++
// calls kh_decoder_get_best_path per utterance; through a foreign-function interface the per-call cost
// (2620 utterances x 3 calls = 1 % of the benchmark's step) is what this saves.
int kh_decoder_get_best_paths(const KhDecoder *dc, int first, int n, int32_t *alignment, int64_t cap_ali, int64_t *ali_off,
                              int32_t *words, int64_t cap_words, int64_t *words_off, float *graph_cost, float *acoustic_cost) {
  const DecoderEnv env = ReadDecoderEnv();
  KhDecoder *d = const_cast<KhDecoder *>(dc);
  KH_CHECK_ARG(d && first >= 0 && n >= 0 && first + n <= d->n_utts && alignment && ali_off && words && words_off && graph_cost &&
               acoustic_cost);
  int64_t na = 0, nw = 0;
  for (int i = 0; i < n; i++) {
    const int rc = ComputeBestPath(d, env, first + i);
    if (rc) return rc;
    const KhDecoder::Lat &L = d->lats[first + i];
    const int64_t a = static_cast<int64_t>(L.bp_ali.size()), w = static_cast<int64_t>(L.bp_words.size());
    if (na + a > cap_ali || nw + w > cap_words) {
      SetError("kh_decoder_get_best_paths: buffers too small at utterance %d", first + i);
      return KH_EINVAL;
    }
    ali_off[i] = na;
    words_off[i] = nw;
    if (a) memcpy(alignment + na, L.bp_ali.data(), sizeof(int32_t) * a);
    if (w) memcpy(words + nw, L.bp_words.data(), sizeof(int32_t) * w);
    na += a;
    nw += w;
    graph_cost[i] = L.bp_graph;
    acoustic_cost[i] = L.bp_acoustic;
  }
  ali_off[n] = na;
  words_off[n] = nw;
  return KH_OK;
}

// kh_decoder_get_counters and kh_decoder_get_stats of utterances [first, first + n) (either array may be NULL)
int kh_decoder_get_stats_batch(const KhDecoder *dc, int first, int n, KhDecodeStats *counters, KhDecodeStats *stats) {
  KhDecoder *d = const_cast<KhDecoder *>(dc);
  KH_CHECK_ARG(d && first >= 0 && n >= 0 && first + n <= d->n_utts);
  for (int i = 0; i < n; i++) {
    int rc = KH_OK;
    if (counters && (rc = kh_decoder_get_counters(d, first + i, &counters[i]))) return rc;
    if (stats && (rc = kh_decoder_get_stats(d, first + i, &stats[i]))) return rc;
  }
  return KH_OK;
}

// Host post-pass of a batch in parallel: GetRawLattice + GetBestPath of every
// utterance (what DecodeUtteranceLatticeFaster does per utterance after Decode(),
// decoder-wrappers.cc:215-262), on num_threads host threads (<= 0: all cores).
int kh_decoder_prepare(KhDecoder *d, int num_threads) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(d);
  const int n = d->n_utts;
  if (n <= 0) return KH_OK;
  // (0: the CPUs the container may use - never the 256 visible cores of a box whose cgroup grants 16: beyond the quota the
  // kernel throttles the whole group, the thread that launches the next forward pass included - shared by the node's ranks)
  int nt = num_threads;
  if (nt <= 0) {
    nt = EnvHostThreads(env, std::min(64, HostCpuQuota()));
  }
  nt = std::max(1, std::min(std::min(nt, 128), n));
  // every lattice not built yet gets its slice of the batch store
  {
    size_t tot_n = 0, tot_m = 0;
    for (int ui = 0; ui < n; ui++)
      if (!d->lats[ui].built && d->h_out[ui].stats.status == 0) { tot_n += d->h_out[ui].n_tok; tot_m += d->h_out[ui].n_link; }
    for (int k = 0; k < 2; k++) if (d->st_i[k].size() < tot_n) d->st_i[k].resize(tot_n);
    for (int k = 2; k < 6; k++) if (d->st_i[k].size() < tot_m) d->st_i[k].resize(tot_m);
    if (d->st_f[0].size() < tot_n) d->st_f[0].resize(tot_n);
    for (int k = 1; k < 3; k++) if (d->st_f[k].size() < tot_m) d->st_f[k].resize(tot_m);
    size_t on = 0, om = 0;
    for (int ui = 0; ui < n; ui++) {
      KhDecoder::Lat &L = d->lats[ui];
      if (L.built || d->h_out[ui].stats.status != 0) continue;
      const size_t cn = d->h_out[ui].n_tok, cm = d->h_out[ui].n_link;
      L.state_frame.bind(d->st_i[0].data() + on, cn); L.state_hclg.bind(d->st_i[1].data() + on, cn);
      L.state_final.bind(d->st_f[0].data() + on, cn);
      L.arc_src.bind(d->st_i[2].data() + om, cm); L.arc_dst.bind(d->st_i[3].data() + om, cm);
      L.arc_il.bind(d->st_i[4].data() + om, cm); L.arc_ol.bind(d->st_i[5].data() + om, cm);
      L.arc_g.bind(d->st_f[1].data() + om, cm); L.arc_a.bind(d->st_f[2].data() + om, cm);
      on += cn;
      om += cm;
    }
  }
  std::atomic<int> next(0), first_rc(0);
  std::mutex mu;
  std::string first_err;
  auto work = [&]() {
    for (;;) {
      const int ui = next.fetch_add(1);
      if (ui >= n) break;
      if (d->h_out[ui].stats.status != 0) continue;  // an utterance that failed alone (capacity): its getters report it
      const int rc = ComputeBestPath(d, env, ui);
      if (rc != KH_OK) {
        std::lock_guard<std::mutex> l(mu);
        if (first_rc.load() == 0) { first_rc = rc; first_err = LastError(); }
      }
    }
  };
  std::vector<std::thread> th;
  for (int i = 1; i < nt; i++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  if (first_rc.load() != 0) {
    SetError("%s", first_err.c_str());
    return first_rc.load();
  }
  return KH_OK;
}


// ================================================================ online decoding
KhOnlineDecoder *kh_online_decoder_create(const KhFst *fst, const KhDecoderConfig *cfg, int num_streams,
                                          int max_frames) {
  const DecoderEnv env = ReadDecoderEnv();
  KhDecoder *b = kh_decoder_create(fst, cfg, num_streams, max_frames);
  if (!b) return nullptr;
  if (env.order >= 0) b->exact = env.order;   // (as kh_decoder_decode applies it)
  KhOnlineDecoder *o = new KhOnlineDecoder();
  o->base = b;
  o->num_streams = num_streams;
  o->max_frames = max_frames;
  hipStream_t st = Stream();
  int n_slots = 0;
  int rc = EnsureSlots(b, env, num_streams, max_frames, st, &n_slots);
  if (rc == KH_OK && n_slots < num_streams) {
    SetError("kh_online_decoder_create: only %d of %d streams fit in device memory", n_slots, num_streams);
    rc = KH_ENOMEM;
  }
  if (rc == KH_OK) {
    o->d_states = static_cast<SlotState *>(PoolMalloc(sizeof(SlotState) * num_streams));
    o->d_jobs = static_cast<Job *>(PoolMalloc(sizeof(Job) * num_streams));
    b->d_out = static_cast<UttOut *>(PoolMalloc(sizeof(UttOut) * num_streams));
    b->d_used = static_cast<unsigned long long *>(PoolMalloc(sizeof(unsigned long long) * 4));
    if (!o->d_states || !o->d_jobs || !b->d_out || !b->d_used) rc = KH_ENOMEM;
  }
  if (rc == KH_OK && hipMemsetAsync(o->d_states, 0, sizeof(SlotState) * num_streams, st) != hipSuccess) rc = KH_EDEVICE;
  if (rc == KH_OK && hipMemcpyAsync(b->d_slots, b->h_slots.data(), sizeof(Utt) * num_streams, hipMemcpyHostToDevice, st) != hipSuccess) rc = KH_EDEVICE;
  if (rc == KH_OK && hipStreamSynchronize(st) != hipSuccess) rc = KH_EDEVICE;
  if (rc != KH_OK) {
    kh_online_decoder_destroy(o);
    return nullptr;
  }
  b->n_utts = num_streams;
  b->lats.assign(num_streams, KhDecoder::Lat());
  b->h_out.assign(num_streams, UttOut());
  b->h_T.assign(num_streams, 0);
  b->h_round.assign(num_streams, 0);
  o->frames.assign(num_streams, 0);
  o->inited.assign(num_streams, 0);
  o->finalized.assign(num_streams, 0);
  o->lat_key.assign(num_streams, -1);
  return o;
}

void kh_online_decoder_destroy(KhOnlineDecoder *o) {
  if (!o) return;
  (void)kh_online_decoder_serve_stop(o);
  if (o->serve_ctl) (void)hipHostFree(o->serve_ctl);
  if (o->serve_quit) (void)hipHostFree(o->serve_quit);
  if (o->serve_stream) (void)hipStreamDestroy(o->serve_stream);
  if (o->d_serve_act) PoolFree(o->d_serve_act);
  PoolFree(o->d_states);
  PoolFree(o->d_jobs);
  kh_decoder_destroy(o->base);
  delete o;
}

static int LaunchJobs(KhOnlineDecoder *o, const DecoderEnv &env, const std::vector<Job> &jobs, int ll_stride, const int32_t *tid2pdf) {
  KhDecoder *b = o->base;
  hipStream_t st = Stream();
  Params p;
  FillParams(b, env, &p, ll_stride > 0 ? ll_stride : 1 << 30, tid2pdf);
  p.lazy_prune = b->lazy;   // kh_online_decoder_set_lazy_prune
  p.lazy_span = b->lazy ? OnlineLazySpan(env) : 0;
  if (ll_stride <= 0) p.ll_cols = 0;
  if (b->rec != nullptr && b->rec_order_ids == (b->exact ? 1 : 0) &&
      (ll_stride <= 0 || (o->pinned && tid2pdf == o->pinned_map && ll_stride == o->pinned_cols))) {
    // the records hold this map's pdfs already (kh_online_decoder_set_pdf_map) - or the jobs read no scores at all
    // (InitDecoding, FinalizeDecoding, export: only the graph's structure), and the records must not be rewritten under
    // a serving kernel that is using them
    p.rec = (GP(const KhInt4))b->rec;
  } else {
    const int rc = BuildArcPdf(b, &p, tid2pdf, ll_stride, st);
    if (rc) return rc;
    o->pinned = false;
  }
  KH_HIP(hipMemcpyAsync(o->d_jobs, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice, st));
  p.exact_order = b->exact ? 1 : 0;
  if (b->exact && env.order_sort) p.exact_order = 2;
  LaunchOnline(b->exact != 0, static_cast<unsigned>(jobs.size()), DynLdsBytes(p.ll_cols), st, b->d_slots, o->d_states, o->d_jobs,
               b->d_out, b->pool, p, b->exact ? (const UttX *)b->d_slotsx : (const UttX *)nullptr);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// a stream whose kernel status is not 0 -> the error the caller sees (KH_ECAPACITY: the message says which kind)
static int StreamFailed(const char *what, int stream, int code, int frame) {
  if (code == 10)
    SetError("%s: stream %d failed at frame %d (code 10: %s); the stream's utterance is lost, the other streams are not affected",
             what, stream, frame, StatusText(10));
  else
    SetError("%s: stream %d overflowed a decoder arena (code %d) at frame %d; see KH_DECODER_TOKENS_PER_FRAME / "
             "KH_DECODER_LINKS_PER_FRAME / KH_DECODER_STABLE_TOKENS_PER_FRAME", what, stream, code, frame);
  return KH_ECAPACITY;
}

// kernel status of the listed streams -> error
static int CheckStreams(KhOnlineDecoder *o, const int32_t *streams, int n, const char *what) {
  hipStream_t st = Stream();
  std::vector<SlotState> hs(o->num_streams);
  KH_HIP(hipMemcpyAsync(hs.data(), o->d_states, sizeof(SlotState) * o->num_streams, hipMemcpyDeviceToHost, st));
  KH_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; i++) {
    const SlotState &S = hs[streams[i]];
    if (!S.ok) return StreamFailed(what, streams[i], S.status, S.t);
    o->frames[streams[i]] = S.t;
  }
  return KH_OK;
}

static bool DistinctStreams(const KhOnlineDecoder *o, const int32_t *streams, int n) {
  std::vector<char> seen(o->num_streams, 0);
  for (int i = 0; i < n; i++) {
    if (streams[i] < 0 || streams[i] >= o->num_streams || seen[streams[i]]) return false;
    seen[streams[i]] = 1;
  }
  return true;
}

// InitDecoding (lattice-faster-online-decoder.cc:55-72) of the listed streams.
int kh_online_decoder_init_decoding(KhOnlineDecoder *o, const int32_t *streams, int n) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o && streams && n > 0 && n <= o->num_streams && DistinctStreams(o, streams, n));
  if (o->serve_launched) {
    SetError("%s: the serving kernel owns the streams (kh_online_decoder_serve_* / kh_online_decoder_serve_stop)", "kh_online_decoder_init_decoding");
    return KH_ESTATE;
  }
  std::vector<Job> jobs(n);
  for (int i = 0; i < n; i++) {
    jobs[i].slot = streams[i];
    jobs[i].op = kJobInit;
    jobs[i].ll = (GP(const float))nullptr;
    jobs[i].ll_stride = 0;
    jobs[i].n_frames = 0;
    o->inited[streams[i]] = 1;
    o->finalized[streams[i]] = 0;
    o->lat_key[streams[i]] = -1;
  }
  rc = LaunchJobs(o, env, jobs, 0, nullptr);
  if (rc) return rc;
  return CheckStreams(o, streams, n, "kh_online_decoder_init_decoding");
}

// AdvanceDecoding (:747-769): stream streams[i] decodes the next num_frames[i] frames,
// whose scaled log-likelihoods are the rows of loglikes[i] (device, row stride
// ll_stride, full rows allocated).
int kh_online_decoder_advance(KhOnlineDecoder *o, const int32_t *streams, int n, const float *const *loglikes,
                              int ll_stride, const int32_t *num_frames, const int32_t *tid2pdf) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o && streams && loglikes && num_frames && n > 0 && n <= o->num_streams && ll_stride > 0 &&
               DistinctStreams(o, streams, n));
  if (o->serve_launched) {
    SetError("kh_online_decoder_advance: the serving kernel owns the streams (kh_online_decoder_serve_publish / kh_online_decoder_serve_stop)");
    return KH_ESTATE;
  }
  std::vector<Job> jobs;
  for (int i = 0; i < n; i++) {
    const int sidx = streams[i];
    if (!o->inited[sidx] || o->finalized[sidx]) {
      SetError("kh_online_decoder_advance: stream %d: call InitDecoding() first, and not after FinalizeDecoding() "
               "(lattice-faster-online-decoder.cc:749-750)", sidx);
      return KH_ESTATE;
    }
    KH_CHECK_ARG(num_frames[i] >= 0 && o->frames[sidx] + num_frames[i] <= o->max_frames);
    if (num_frames[i] == 0) continue;
    KH_CHECK_ARG(loglikes[i] != nullptr);
    Job j;
    j.slot = sidx;
    j.op = kJobAdvance;
    // the kernel addresses the matrix by absolute frame
    j.ll = (GP(const float))(loglikes[i] - static_cast<ptrdiff_t>(o->frames[sidx]) * ll_stride);
    j.ll_stride = ll_stride;
    j.n_frames = num_frames[i];
    jobs.push_back(j);
    o->lat_key[sidx] = -1;
  }
  if (jobs.empty()) return KH_OK;
  rc = LaunchJobs(o, env, jobs, ll_stride, tid2pdf);
  if (rc) return rc;
  return CheckStreams(o, streams, n, "kh_online_decoder_advance");
}

int kh_online_decoder_set_pdf_map(KhOnlineDecoder *o, const int32_t *tid2pdf, int num_cols) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o && num_cols > 0);
  Params p;
  FillParams(o->base, env, &p, num_cols, tid2pdf);
  if ((rc = BuildArcPdf(o->base, &p, tid2pdf, num_cols, Stream()))) return rc;
  o->pinned_map = tid2pdf;
  o->pinned_cols = num_cols;
  o->pinned = true;
  return KH_OK;
}

int kh_online_decoder_num_frames_decoded(const KhOnlineDecoder *o, int stream, int32_t *num_frames) {
  KH_CHECK_ARG(o && num_frames && stream >= 0 && stream < o->num_streams);
  *num_frames = o->frames[stream];
  return KH_OK;
}

// FinalizeDecoding (:775-790) of the listed streams.
int kh_online_decoder_finalize(KhOnlineDecoder *o, const int32_t *streams, int n) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o && streams && n > 0 && n <= o->num_streams && DistinctStreams(o, streams, n));
  if (o->serve_launched) {
    SetError("%s: the serving kernel owns the streams (kh_online_decoder_serve_* / kh_online_decoder_serve_stop)", "kh_online_decoder_finalize");
    return KH_ESTATE;
  }
  std::vector<Job> jobs(n);
  for (int i = 0; i < n; i++) {
    const int sidx = streams[i];
    if (!o->inited[sidx] || o->finalized[sidx]) {
      SetError("kh_online_decoder_finalize: stream %d is not in a decoding run", sidx);
      return KH_ESTATE;
    }
    jobs[i].slot = sidx;
    jobs[i].op = kJobFinalize;
    jobs[i].ll = (GP(const float))nullptr;
    jobs[i].ll_stride = 0;
    jobs[i].n_frames = 0;
    o->finalized[sidx] = 1;
    o->lat_key[sidx] = -1;
  }
  rc = LaunchJobs(o, env, jobs, 0, nullptr);
  if (rc) return rc;
  return CheckStreams(o, streams, n, "kh_online_decoder_finalize");
}

// The offline kernel's LAZY pruning schedule for the streams (default off = the reference's: PruneActiveTokens every
// prune_interval frames): nothing is pruned while a stream advances unless its arenas run low, FinalizeDecoding prunes
// every frame once.  The final lattice, every best path and the endpointing quantities are those of the interval schedule
// (rule P, DESIGN.md section 2: the result does not depend on when the sweeps run); a raw lattice asked for BEFORE
// FinalizeDecoding is pruned as of the current frame instead of the last multiple of prune_interval.  The arenas are
// re-carved (every stream must be idle: before InitDecoding or after FinalizeDecoding + the last getter).
// The streams decode in the reference's own iteration order (kh_decoder_set_reference_order for the online decoder:
// LatticeFasterOnlineDecoder::ProcessEmitting, lattice-faster-online-decoder.cc:864-951, walks the same HashList against the
// same running next_cutoff).  Between utterances only, with the serving kernel stopped; a serving kernel started afterwards
// decodes in the same order (ServeKernel<true>).
int kh_online_decoder_set_reference_order(KhOnlineDecoder *o, int enable) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o);
  KhDecoder *b = o->base;
  if ((b->exact != 0) == (enable != 0)) return KH_OK;
  if (o->serve_launched) {
    SetError("kh_online_decoder_set_reference_order: stop the serving kernel first");
    return KH_ESTATE;
  }
  for (int s = 0; s < o->num_streams; s++)
    if (o->inited[s] && !o->finalized[s]) {
      SetError("kh_online_decoder_set_reference_order: stream %d is in a decoding run", s);
      return KH_ESTATE;
    }
  b->exact = enable != 0;
  o->pinned = false;   // (the decoder's arc records carry state ids in this mode: built again by the next launch)
  hipStream_t st = Stream();
  int n_slots = 0;
  rc = EnsureSlots(b, env, o->num_streams, o->max_frames, st, &n_slots);
  if (rc == KH_OK && n_slots < o->num_streams) {
    SetError("kh_online_decoder_set_reference_order: only %d of %d streams fit in device memory", n_slots, o->num_streams);
    rc = KH_ENOMEM;
  }
  if (rc) return rc;
  KH_HIP(hipMemsetAsync(o->d_states, 0, sizeof(SlotState) * o->num_streams, st));
  KH_HIP(hipMemcpyAsync(b->d_slots, b->h_slots.data(), sizeof(Utt) * o->num_streams, hipMemcpyHostToDevice, st));
  KH_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < o->num_streams; s++) {
    o->inited[s] = 0;
    o->finalized[s] = 0;
    o->frames[s] = 0;
    o->lat_key[s] = -1;
  }
  return KH_OK;
}

int kh_online_decoder_set_lazy_prune(KhOnlineDecoder *o, int enable) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o);
  KhDecoder *b = o->base;
  if ((b->lazy != 0) == (enable != 0)) return KH_OK;
  if (o->serve_launched) {
    SetError("kh_online_decoder_set_lazy_prune: stop the serving kernel first");
    return KH_ESTATE;
  }
  for (int s = 0; s < o->num_streams; s++)
    if (o->inited[s] && !o->finalized[s]) {
      SetError("kh_online_decoder_set_lazy_prune: stream %d is in a decoding run", s);
      return KH_ESTATE;
    }
  b->lazy = enable != 0;
  hipStream_t st = Stream();
  int n_slots = 0;
  rc = EnsureSlots(b, env, o->num_streams, o->max_frames, st, &n_slots);
  if (rc == KH_OK && n_slots < o->num_streams) {
    SetError("kh_online_decoder_set_lazy_prune: only %d of %d streams fit in device memory", n_slots, o->num_streams);
    rc = KH_ENOMEM;
  }
  if (rc) return rc;
  KH_HIP(hipMemsetAsync(o->d_states, 0, sizeof(SlotState) * o->num_streams, st));
  KH_HIP(hipMemcpyAsync(b->d_slots, b->h_slots.data(), sizeof(Utt) * o->num_streams, hipMemcpyHostToDevice, st));
  KH_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < o->num_streams; s++) { o->inited[s] = 0; o->finalized[s] = 0; o->frames[s] = 0; o->lat_key[s] = -1; }
  return KH_OK;
}

// ---- the persistent serving kernel (ServeKernel): start / stop, commands, progress
// No call below blocks for ever: every wait for the device has a deadline (KH_SERVE_TIMEOUT_MS, default 30 s) and reports
// KH_ETIMEOUT with the state of the streams' control blocks (what each workgroup was doing when it last spoke).
static double ServeTimeoutMs(const DecoderEnv &env) { return env.serve_timeout_ms; }
#ifdef KH_SERVE_MARKERS
static int32_t *g_wave_mark_host = nullptr;
#endif
static std::string ServeDump(const KhOnlineDecoder *o, const int32_t *streams, int n) {
  std::string out;
  char buf[256];
  int shown = 0;
  // two passes: the streams whose workgroup is still there or that have something pending first (what a time-out is about:
  // round 6 had a dump whose eight entries were all workgroups that had left), then the others
  int n_alive = 0, n_pending = 0;
  for (int s = 0; s < o->num_streams; s++) {
    const ServeCtl &c = o->serve_ctl[s];
    n_alive += __atomic_load_n(&c.alive, __ATOMIC_ACQUIRE) != 0 ? 1 : 0;
    n_pending += __atomic_load_n(&c.ack_seq, __ATOMIC_ACQUIRE) != o->serve_seq[s] ? 1 : 0;
  }
  snprintf(buf, sizeof buf, " %d of %d workgroups resident, %d streams with a command in flight;", n_alive, o->num_streams, n_pending);
  out += buf;
  for (int pass = 0; pass < 2; pass++)
  for (int i = 0; i < (streams ? n : o->num_streams) && shown < 8; i++) {
    const int s = streams ? streams[i] : i;
    const ServeCtl &c = o->serve_ctl[s];
    const int ack = __atomic_load_n(&c.ack_seq, __ATOMIC_ACQUIRE), dec = __atomic_load_n(&c.decoded, __ATOMIC_ACQUIRE);
    const bool pending = ack != o->serve_seq[s] || (!o->finalized[s] && __atomic_load_n(&c.avail, __ATOMIC_ACQUIRE) > dec);
    const bool hot = pending || __atomic_load_n(&c.alive, __ATOMIC_ACQUIRE) != 0;
    if (hot != (pass == 0)) continue;
    if (streams == nullptr && !pending && __atomic_load_n(&c.hb_phase, __ATOMIC_ACQUIRE) == 0) continue;
    snprintf(buf, sizeof buf, "%s stream %d: avail %d decoded %d cmd %d/%d ack %d alive %d phase %d (to frame %d) actions %d clock %u mark %d/%d", shown ? ";" : "",
             s, c.avail, dec, c.cmd_op, o->serve_seq[s], ack, c.alive, c.hb_phase, c.hb_arg, c.hb_actions, static_cast<unsigned>(c.hb_clock),
             static_cast<int>(static_cast<uint32_t>(c.pad1[0]) >> 24), c.pad1[0] & 0xffffff);
    out += buf;
#ifdef KH_SERVE_MARKERS
    if (pass == 0 && g_wave_mark_host != nullptr && s < 1024) {
      out += " waves";
      for (int w = 0; w < 16; w++) {
        const int32_t m = __atomic_load_n(&g_wave_mark_host[64 * s + w], __ATOMIC_ACQUIRE);
        snprintf(buf, sizeof buf, " %d/%d", static_cast<int>(static_cast<uint32_t>(m) >> 24), m & 0xffffff);
        out += buf;
      }
      out += " dbg";
      for (int w = 16; w < 52; w++) {
        snprintf(buf, sizeof buf, " %d", __atomic_load_n(&g_wave_mark_host[64 * s + w], __ATOMIC_ACQUIRE));
        out += buf;
      }
    }
#endif
    shown++;
  }
  snprintf(buf, sizeof buf, "%s quit %d, launched %d, relaunches %lld", shown ? ";" : "", o->serve_quit ? *o->serve_quit : -1,
           o->serve_launched ? 1 : 0, o->serve_relaunches);
  out += buf;
  return out;
}
// waits (bounded) for the serving kernel to have ended; KH_ETIMEOUT if it has not
static int ServeJoin(KhOnlineDecoder *o, const DecoderEnv &env, const char *what) {
  const auto t0 = std::chrono::steady_clock::now();
  const double limit = ServeTimeoutMs(env);
  for (;;) {
    const hipError_t q = hipStreamQuery(o->serve_stream);
    if (q == hipSuccess) break;
    (void)hipGetLastError();
    if (q != hipErrorNotReady) {
      o->serve_launched = false;
      SetError("%s: serving kernel: %s", what, hipGetErrorString(q));
      return KH_EDEVICE;
    }
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > limit) {
      SetError("%s: the serving kernel did not leave within %.0f ms [%s]", what, limit, ServeDump(o, nullptr, 0).c_str());
      return KH_ETIMEOUT;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
  o->serve_launched = false;
  return KH_OK;
}

static int ServeEnsureRunning(KhOnlineDecoder *o, const DecoderEnv &env) {
  if (!o->serve_ctl) {
    SetError("the serving kernel has not been started (kh_online_decoder_serve_start)");
    return KH_ESTATE;
  }
  if (o->serve_launched) {
    // running, and nobody has told it to leave: every stream has its workgroup (they leave only together)
    if (__atomic_load_n(o->serve_quit, __ATOMIC_ACQUIRE) == 0) {
      const hipError_t q = hipStreamQuery(o->serve_stream);
      if (q == hipErrorNotReady) return KH_OK;
      (void)hipGetLastError();
      if (q != hipSuccess) {
        o->serve_launched = false;
        SetError("serving kernel: %s", hipGetErrorString(q));
        return KH_EDEVICE;
      }
      o->serve_launched = false;   // (ended without being told to: cannot happen; launched again below)
    } else {
      // the grid has decided to leave (idle time): it is on its way out - launched again once it has gone
      const int rc = ServeJoin(o, env, "kh_online_decoder_serve");
      if (rc) return rc;
    }
    o->serve_relaunches++;
  }
  KhDecoder *b = o->base;
  hipStream_t st = Stream();
  Params p;
  FillParams(b, env, &p, o->serve_stride, o->serve_map);
  p.lazy_prune = b->lazy;
  p.lazy_span = b->lazy ? OnlineLazySpan(env) : 0;
  if (!(o->pinned && o->serve_map == o->pinned_map && o->serve_stride == o->pinned_cols && b->rec != nullptr &&
        b->rec_order_ids == (b->exact ? 1 : 0))) {
    const int rc = kh_online_decoder_set_pdf_map(o, o->serve_map, o->serve_stride);
    if (rc) return rc;
  }
  p.rec = (GP(const KhInt4))b->rec;
  KH_HIP(hipStreamSynchronize(st));   // whatever launch-per-job work is queued has written its SlotStates
  // no serving kernel is running here: what the PREVIOUS grid left in the residency fields (alive 0, phase 9 = "has left")
  // must not be read as the new grid's before its workgroups have started - kh_online_decoder_serve_poll would take the
  // freshly launched grid for one that lost a workgroup, tell it to quit and launch it a second time
  for (int s = 0; s < o->num_streams; s++) {
    __atomic_store_n(&o->serve_ctl[s].alive, 0, __ATOMIC_RELAXED);
    __atomic_store_n(&o->serve_ctl[s].hb_phase, 0, __ATOMIC_RELAXED);
  }
  __atomic_store_n(o->serve_quit, 0, __ATOMIC_RELEASE);
  void *ctl_dev = nullptr, *quit_dev = nullptr;
  KH_HIP(hipHostGetDevicePointer(&ctl_dev, o->serve_ctl, 0));
  KH_HIP(hipHostGetDevicePointer(&quit_dev, o->serve_quit, 0));
  const long long idle_ticks = env.serve_idle_ticks;   // (default: 2 s of the 100 MHz wall clock)
  p.exact_order = b->exact ? 1 : 0;
  // One resident workgroup per CU while the streams fit that way.  A CU takes two of these workgroups (64 VGPRs, 73 KB of
  // LDS each) and nothing tells the dispatcher to spread 256 of them over 256 CUs: when it doubled up on ONE CU (the CUs
  // it finds busy at launch time - a fill kernel, a forward pass - get none, others get two), those two streams ran at
  // half speed for the kernel's lifetime and, the host waiting for every stream per chunk, so did the service: round 5's
  // two regimes (350 k / 200 k frames/s, chunk p50 4.7 / 9 ms, chosen per launch).  LDS is the lever: a workgroup that
  // asks for more than half of the CU's 160 KB cannot get a neighbour.  KH_SERVE_SHARE_CU=1: the round-5 launch.
  size_t dyn_lds = DynLdsBytes(p.ll_cols);
  if (o->num_streams <= NumCUs() && !env.serve_share_cu) {
    size_t static_lds = 0;
    KH_HIP(ServeStaticLds(b->exact != 0, &static_lds));
    const size_t want_total = 88 * 1024;
    if (static_lds + dyn_lds < want_total) dyn_lds = want_total - static_lds;
    (void)SetServeDynLds(b->exact != 0, dyn_lds);
  }
#ifdef KH_SERVE_MARKERS
  {
    int32_t *mark = static_cast<int32_t *>(ctl_dev);
    KH_HIP(SetServeMark(mark));
    if (g_wave_mark_host == nullptr) {
      KH_HIP(hipHostMalloc(reinterpret_cast<void **>(&g_wave_mark_host), sizeof(int32_t) * 64 * 1024, hipHostMallocMapped));
      memset(g_wave_mark_host, 0, sizeof(int32_t) * 64 * 1024);
    }
    int32_t *wm_dev = nullptr;
    KH_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&wm_dev), g_wave_mark_host, 0));
    if (o->num_streams > 1024) wm_dev = nullptr;
    KH_HIP(SetWaveMark(wm_dev));
  }
#endif
  if (b->exact && env.order_sort) p.exact_order = 2;
  LaunchServe(b->exact != 0, static_cast<unsigned>(o->num_streams), dyn_lds, o->serve_stream, b->d_slots, o->d_states,
              static_cast<ServeCtl *>(ctl_dev), static_cast<int32_t *>(quit_dev), o->serve_ll, o->serve_rows, o->serve_stride, p,
              idle_ticks, o->d_serve_act, b->exact ? (const UttX *)b->d_slotsx : (const UttX *)nullptr);
  KH_LAUNCH_CHECK();
  o->serve_launched = true;
  return KH_OK;
}

int kh_online_decoder_serve_start(KhOnlineDecoder *o, const float *loglikes, int ll_stride, int64_t rows_per_stream,
                                  const int32_t *tid2pdf) {
  const DecoderEnv env = ReadDecoderEnv();
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(o && loglikes && ll_stride > 0 && rows_per_stream >= o->max_frames);
  if (o->num_streams > KH_WG_PER_CU * NumCUs()) {
    SetError("kh_online_decoder_serve_start: %d streams, but only %d workgroups can be resident at once", o->num_streams,
             KH_WG_PER_CU * NumCUs());
    return KH_EINVAL;
  }
  if ((rc = kh_online_decoder_serve_stop(o))) return rc;
  if (!o->serve_ctl) {
    KH_HIP(hipHostMalloc(reinterpret_cast<void **>(&o->serve_ctl), sizeof(ServeCtl) * o->num_streams, hipHostMallocMapped));
    KH_HIP(hipHostMalloc(reinterpret_cast<void **>(&o->serve_quit), 64, hipHostMallocMapped));
    KH_HIP(hipStreamCreateWithFlags(&o->serve_stream, hipStreamNonBlocking));
    o->d_serve_act = static_cast<long long *>(PoolMalloc(sizeof(long long) * o->num_streams));
    if (!o->d_serve_act) {
      SetError("kh_online_decoder_serve_start: out of device memory");
      return KH_ENOMEM;
    }
    KH_HIP(hipMemset(o->d_serve_act, 0, sizeof(long long) * o->num_streams));
    memset(o->serve_ctl, 0, sizeof(ServeCtl) * o->num_streams);
    o->serve_seq.assign(o->num_streams, 0);
  }
  for (int s = 0; s < o->num_streams; s++) {   // pick up where the launch-per-job calls left the streams
    o->serve_ctl[s].avail = o->frames[s];
    o->serve_ctl[s].decoded = o->frames[s];
    o->serve_ctl[s].ok = 1;
    // the arena's high-water mark as the LAST serving kernel reported it is stale once launch-per-job calls have decoded
    // on the stream in between (they raise SlotState::tok_hw, not this copy): 0 = the next InitDecoding is a plain kCmdInit,
    // the device clears [0, its own tok_hw) and reports the mark afresh (a host-side fill of the stale range
    // + kCmdInitCleared left finite costs behind)
    o->serve_ctl[s].hw = 0;
  }
  o->serve_ll = loglikes;
  o->serve_stride = ll_stride;
  o->serve_rows = rows_per_stream;
  o->serve_map = tid2pdf;
  return ServeEnsureRunning(o, env);
}

int kh_online_decoder_serve_stop(KhOnlineDecoder *o) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(o);
  if (!o->serve_ctl || !o->serve_launched) return KH_OK;
  __atomic_store_n(o->serve_quit, 1, __ATOMIC_RELEASE);
  const int rc = ServeJoin(o, env, "kh_online_decoder_serve_stop");
  if (rc) return rc;
  for (int s = 0; s < o->num_streams; s++) {
    o->frames[s] = __atomic_load_n(&o->serve_ctl[s].decoded, __ATOMIC_ACQUIRE);
    o->lat_key[s] = -1;
  }
  return KH_OK;
}

static int ServeCommand(KhOnlineDecoder *o, const DecoderEnv &env, const int32_t *streams, int n, int op_all, const int32_t *ops = nullptr) {
  for (int i = 0; i < n; i++) {
    ServeCtl &c = o->serve_ctl[streams[i]];
    const int op = ops ? ops[i] : op_all;
    if (op == kCmdInit || op == kCmdInitCleared) __atomic_store_n(&c.avail, 0, __ATOMIC_RELEASE);
    __atomic_store_n(&c.cmd_op, op, __ATOMIC_RELEASE);
    __atomic_store_n(&c.cmd_seq, ++o->serve_seq[streams[i]], __ATOMIC_RELEASE);
  }
  return ServeEnsureRunning(o, env);
}

// InitDecoding of the listed streams by the serving kernel (asynchronous: kh_online_decoder_serve_wait).
int kh_online_decoder_serve_init(KhOnlineDecoder *o, const int32_t *streams, int n) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(o && o->serve_ctl && streams && n > 0 && n <= o->num_streams && DistinctStreams(o, streams, n));
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    if (o->serve_seq[s] != __atomic_load_n(&o->serve_ctl[s].ack_seq, __ATOMIC_ACQUIRE)) {
      SetError("kh_online_decoder_serve_init: stream %d still has a command in flight", s);
      return KH_ESTATE;
    }
  }
  // The reset of a large token arena by a fill kernel over the whole chip instead of by the stream's one workgroup - only
  // for a stream whose utterance is finalized and acknowledged (its workgroup waits; nobody else touches the arena).
  std::vector<int32_t> ops(n, kCmdInit);
  bool filled = false;
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    const int hw = __atomic_load_n(&o->serve_ctl[s].hw, __ATOMIC_ACQUIRE);
    // (one workgroup per CU at most: the fill kernel needs room next to the resident workgroups)
    if (o->num_streams <= NumCUs() && o->inited[s] && o->finalized[s] && hw >= (1 << 18) && hw <= o->base->h_slots[s].tok_cap) {
      LaunchFillU32(Stream(), (uint32_t *)o->base->h_slots[s].tok_cost.p, static_cast<size_t>(hw), kEncInf);
      KH_LAUNCH_CHECK();
      ops[i] = kCmdInitCleared;
      filled = true;
    }
  }
  if (filled) KH_HIP(hipStreamSynchronize(Stream()));
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    o->inited[s] = 1;
    o->finalized[s] = 0;
    o->frames[s] = 0;
    o->lat_key[s] = -1;
  }
  return ServeCommand(o, env, streams, n, kCmdInit, ops.data());
}

// Scores of frames [0, avail[i]) of stream streams[i] are in its score buffer (the kernels that wrote them have completed):
// the stream decodes up to there.
int kh_online_decoder_serve_publish(KhOnlineDecoder *o, const int32_t *streams, int n, const int32_t *avail) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(o && o->serve_ctl && streams && avail && n > 0 && n <= o->num_streams);
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    KH_CHECK_ARG(s >= 0 && s < o->num_streams && avail[i] >= 0 && avail[i] <= o->max_frames);
    if (!o->inited[s] || o->finalized[s]) {
      SetError("kh_online_decoder_serve_publish: stream %d: call InitDecoding() first, and not after FinalizeDecoding()", s);
      return KH_ESTATE;
    }
    __atomic_store_n(&o->serve_ctl[s].avail, avail[i], __ATOMIC_RELEASE);
    o->lat_key[s] = -1;
  }
  return ServeEnsureRunning(o, env);
}

// FinalizeDecoding of the listed streams once their published frames are decoded (asynchronous).
int kh_online_decoder_serve_finalize(KhOnlineDecoder *o, const int32_t *streams, int n) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(o && o->serve_ctl && streams && n > 0 && n <= o->num_streams && DistinctStreams(o, streams, n));
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    if (!o->inited[s] || o->finalized[s]) {
      SetError("kh_online_decoder_serve_finalize: stream %d is not in a decoding run", s);
      return KH_ESTATE;
    }
    o->finalized[s] = 1;
    o->lat_key[s] = -1;
  }
  return ServeCommand(o, env, streams, n, kCmdFinalize);
}

// Progress of the listed streams: NumFramesDecoded() so far, and whether a command (InitDecoding / FinalizeDecoding) is
// still in flight.  Either output may be NULL.
static int ServePoll(KhOnlineDecoder *o, const DecoderEnv &env, const int32_t *streams, int n, int32_t *decoded, int32_t *in_flight) {
  KH_CHECK_ARG(o && o->serve_ctl && streams && n > 0);
  bool work = false, lost = false;
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    KH_CHECK_ARG(s >= 0 && s < o->num_streams);
    const ServeCtl &c = o->serve_ctl[s];
    const int ack = __atomic_load_n(&c.ack_seq, __ATOMIC_ACQUIRE);
    const int dec = __atomic_load_n(&c.decoded, __ATOMIC_ACQUIRE);
    if (!__atomic_load_n(&c.ok, __ATOMIC_ACQUIRE))
      return StreamFailed("serving kernel", s, __atomic_load_n(&c.pad1[1], __ATOMIC_ACQUIRE), dec);
    const bool pending = ack != o->serve_seq[s];
    // (between an InitDecoding command and its acknowledgement `decoded` still belongs to the previous utterance)
    o->frames[s] = (pending && (c.cmd_op == kCmdInit || c.cmd_op == kCmdInitCleared)) ? 0 : dec;
    if (decoded) decoded[i] = o->frames[s];
    if (in_flight) in_flight[i] = pending ? 1 : 0;
    const bool has_work = pending || (!o->finalized[s] && __atomic_load_n(&c.avail, __ATOMIC_ACQUIRE) > dec);
    work |= has_work;
    // a stream with work whose workgroup has left while the kernel is neither leaving nor gone: the protocol's invariant
    // (workgroups leave only together) is broken - stop the grid and start it again rather than wait for ever
    // (phase 9 is written by a workgroup of THIS launch only: ServeEnsureRunning resets the field before it launches)
    lost |= has_work && o->serve_launched && __atomic_load_n(&c.alive, __ATOMIC_ACQUIRE) == 0 && __atomic_load_n(o->serve_quit, __ATOMIC_ACQUIRE) == 0 &&
            __atomic_load_n(&c.hb_phase, __ATOMIC_ACQUIRE) == 9;
  }
  if (lost) {
    __atomic_store_n(o->serve_quit, 1, __ATOMIC_RELEASE);
    const int rc = ServeJoin(o, env, "kh_online_decoder_serve_poll");
    if (rc) return rc;
  }
  // a caller that only polls must still get its streams served after the grid has left by its idle time
  if (work && (!o->serve_launched || __atomic_load_n(o->serve_quit, __ATOMIC_ACQUIRE) != 0)) return ServeEnsureRunning(o, env);
  return KH_OK;
}
int kh_online_decoder_serve_poll(KhOnlineDecoder *o, const int32_t *streams, int n, int32_t *decoded, int32_t *in_flight) {
  return ServePoll(o, ReadDecoderEnv(), streams, n, decoded, in_flight);
}

// Blocks until the listed streams have decoded everything published to them and acknowledged their commands
// (timeout_ms <= 0: 60 s).  The getters of the online decoder may be used on them afterwards.
int kh_online_decoder_serve_wait(KhOnlineDecoder *o, const int32_t *streams, int n, int timeout_ms) {
  const DecoderEnv env = ReadDecoderEnv();
  KH_CHECK_ARG(o && o->serve_ctl && streams && n > 0);
  const auto t0 = std::chrono::steady_clock::now();
  const double limit = timeout_ms > 0 ? timeout_ms : ServeTimeoutMs(env);
  std::vector<int32_t> dec(n), fl(n);
  for (;;) {
    int rc = ServeEnsureRunning(o, env);
    if (rc) return rc;
    if ((rc = ServePoll(o, env, streams, n, dec.data(), fl.data()))) return rc;
    bool all = true;
    for (int i = 0; i < n && all; i++) {
      const ServeCtl &c = o->serve_ctl[streams[i]];
      all = !fl[i] && (o->finalized[streams[i]] || dec[i] >= __atomic_load_n(&c.avail, __ATOMIC_ACQUIRE));
    }
    if (all) return KH_OK;
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > limit) {
      SetError("kh_online_decoder_serve_wait: timed out after %.0f ms [%s]", limit, ServeDump(o, streams, n).c_str());
      return KH_ETIMEOUT;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// Snapshot of a stream's raw lattice into base->lats[stream] (GetRawLattice,
// lattice-faster-online-decoder.cc:143-233: before FinalizeDecoding the final costs are
// computed on the fly when use_final_probs is set, :160-165).
static int SnapshotLattice(KhOnlineDecoder *o, const DecoderEnv &env, int stream, int use_final_probs) {
  KhDecoder *b = o->base;
  KH_CHECK_ARG(stream >= 0 && stream < o->num_streams);
  if (!o->inited[stream]) {
    SetError("stream %d: InitDecoding() has not been called", stream);
    return KH_ESTATE;
  }
  if (o->finalized[stream] && !use_final_probs) {
    SetError("You cannot call FinalizeDecoding() and then call GetRawLattice() with use_final_probs == false "
             "(lattice-faster-online-decoder.cc:156-158)");
    return KH_ESTATE;
  }
  if (o->frames[stream] <= 0) {
    SetError("stream %d: no frames decoded yet (lattice-faster-online-decoder.cc:171)", stream);
    return KH_ESTATE;
  }
  const long long key = (static_cast<long long>(o->frames[stream]) << 2) | (use_final_probs ? 2 : 0) | (o->finalized[stream] ? 1 : 0);
  if (o->lat_key[stream] == key) return KH_OK;
  hipStream_t st = Stream();
  long long pool_tok = 65536 + 512ll * o->frames[stream], pool_link = 131072 + 1024ll * o->frames[stream];
  UttOut q;
  for (int attempt = 0;; attempt++) {
    int rc = EnsurePool(b, pool_tok, pool_link);
    if (rc) return rc;
    KH_HIP(hipMemsetAsync(b->d_used, 0, sizeof(unsigned long long) * 4, st));
    std::vector<Job> jobs(1);
    jobs[0].slot = stream;
    jobs[0].op = kJobExport;
    jobs[0].ll = (GP(const float))nullptr;
    jobs[0].ll_stride = 0;
    jobs[0].n_frames = 0;
    rc = LaunchJobs(o, env, jobs, 0, nullptr);
    if (rc) return rc;
    unsigned long long used[4] = {0, 0, 0, 0};
    KH_HIP(hipMemcpyAsync(&q, b->d_out, sizeof(UttOut), hipMemcpyDeviceToHost, st));
    KH_HIP(hipMemcpyAsync(used, b->d_used, sizeof(used), hipMemcpyDeviceToHost, st));
    KH_HIP(hipStreamSynchronize(st));
    if (q.stats.status == 6 && attempt == 0) {  // pool too small: the exact size is known now
      pool_tok = q.n_tok + 1024;
      pool_link = q.n_link + 1024;
      continue;
    }
    if (q.stats.status != 0) {
      SetError("stream %d: decoder failed (code %d: %s)", stream, q.stats.status, StatusText(q.stats.status));
      return KH_ECAPACITY;
    }
    b->rounds.clear();
    rc = FetchPool(b, used, pool_tok, pool_link, st);
    if (rc) return rc;
    break;
  }
  b->h_round[stream] = 0;
  b->h_T[stream] = o->frames[stream];
  KhDecoder::HostPool &hp = b->rounds[0];
  if (!o->finalized[stream]) {
    // ComputeFinalCosts :309 (:860-900) on the current last frame
    const float inf = std::numeric_limits<float>::infinity();
    bool any_final = false;
    float best = inf, best_final = inf;
    (void)best; (void)best_final;
    if (use_final_probs)
      for (int k = 0; k < q.n_tok; k++)
        if (hp.t_frame[q.tok_off + k] == o->frames[stream] && b->fst->final_host[hp.t_state[q.tok_off + k]] != inf) any_final = true;
    q.stats.reached_final = any_final ? 1 : 0;
  }
  b->h_out[stream] = q;
  b->lats[stream] = KhDecoder::Lat();
  int rc = BuildLattice(b, stream);
  b->rounds.clear();
  if (rc) return rc;
  o->lat_key[stream] = key;
  return KH_OK;
}

int kh_online_decoder_get_stats(KhOnlineDecoder *o, int stream, int use_final_probs, KhDecodeStats *stats) {
  KH_CHECK_ARG(o && stats);
  int rc = SnapshotLattice(o, ReadDecoderEnv(), stream, use_final_probs);
  if (rc) return rc;
  *stats = o->base->h_out[stream].stats;
  stats->num_tokens = static_cast<int32_t>(o->base->lats[stream].state_frame.size());
  stats->num_links = static_cast<int32_t>(o->base->lats[stream].arc_src.size());
  return KH_OK;
}

int kh_online_decoder_get_raw_lattice(KhOnlineDecoder *o, int stream, int use_final_probs, int32_t *state_frame,
                                      int32_t *state_hclg, float *state_final, int32_t *arc_src, int32_t *arc_dst,
                                      int32_t *arc_ilabel, int32_t *arc_olabel, float *arc_graph,
                                      float *arc_acoustic) {
  KH_CHECK_ARG(o);
  int rc = SnapshotLattice(o, ReadDecoderEnv(), stream, use_final_probs);
  if (rc) return rc;
  return kh_decoder_get_raw_lattice(o->base, stream, state_frame, state_hclg, state_final, arc_src, arc_dst,
                                    arc_ilabel, arc_olabel, arc_graph, arc_acoustic);
}

// GetBestPath (:107-108): the reference traces token backpointers (BestPathEnd /
// TraceBackBestPath); here it is the shortest path of the same raw lattice, which
// TestGetBestPath (:113) checks to be equivalent.
int kh_online_decoder_get_best_path(KhOnlineDecoder *o, int stream, int use_final_probs, int32_t *alignment,
                                    int cap_ali, int32_t *n_ali, int32_t *words, int cap_words, int32_t *n_words,
                                    float *graph_cost, float *acoustic_cost) {
  KH_CHECK_ARG(o);
  int rc = SnapshotLattice(o, ReadDecoderEnv(), stream, use_final_probs);
  if (rc) return rc;
  return kh_decoder_get_best_path(o->base, stream, alignment, cap_ali, n_ali, words, cap_words, n_words, graph_cost,
                                  acoustic_cost);
}

}  // extern "C"
