// kh_decoder_types.h — what the decoder's kernels (kh_decoder.hip) and its host code (kh_decoder_host.hip) must agree on:
// the device graph, the arena / parameter / job / control-block structs the kernels take, the constants the host sizes
// things from, and the host launchers kh_decoder.hip defines next to its kernels.  LDS layouts, scans and the search
// phases are private to kh_decoder.hip.  (Included by .hip files only: Arr<T> and GP() need hipcc.)
#ifndef KH_DECODER_TYPES_H_
#define KH_DECODER_TYPES_H_
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kh_common.h"

// ================================================================ device FST
// The graph as the kernel reads it: ONE table of 16-byte units in which a state is a RECORD
//   [header {#emitting arcs, first epsilon arc, #epsilon arcs, final cost}] [emitting arc] ... [emitting arc]
// and a state's id IS the unit index of its header (monotone in the caller's ids, so every smallest-
// state-id tie-break is unchanged).  Every read of this part moves a whole 128-byte line
// (profiles/r02_pmc_calibration.txt): with an offsets array + an arc table + a pdf table a token of a
// 2-arc HMM state cost three lines; its record is 48 bytes of one, next to the records of the states
// of the same HMM chain.  The epsilon arcs (3 % of the traffic) stay in their own table.
struct KhFst {
  int32_t num_states = 0, start = 0, start_state = 0;  // start: unit id; start_state: the caller's id
  int64_t num_arcs = 0, num_emit = 0, num_eps = 0, num_units = 0;
  int32_t max_emit = 0;            // the largest number of emitting arcs of one state
  int4 *rec = nullptr;             // [num_units] header {n_emit, eps_base, n_eps, final bits} | arc {ilabel, olabel, weight bits, nextstate unit | flags}
  int32_t *unit_ilabel = nullptr;  // [num_units] ilabel (> 0) of an arc unit (the decoder's copy of rec holds the pdf there); -1 - the caller's state id for a header
  int4 *n_arcs = nullptr;          // {0, olabel, weight bits, nextstate unit | flags}
  std::vector<float> final_host;       // host copy for lattice export, by the caller's state
  int start_has_eps = 0;
  int32_t max_ilabel = 0;
};

namespace kh {
namespace dec {

#ifndef KH_NT
#define KH_NT 1024
#endif
constexpr int NT = KH_NT;          // threads per workgroup (one utterance)
constexpr int NW = NT / 64;        // waves
#ifndef KH_NPH
#define KH_NPH 160
#endif
constexpr int NPH = KH_NPH;        // diagnostic counters per slot (96 on: the fine stamps of -DKH_X_STAMPS builds)
// Arc records carry, in bit 30 of the next state, whether that state has epsilon
// arcs: a token knows it at creation without touching the graph again.
constexpr int32_t kHasEps = 0x40000000, kStateMask = 0x1fffffff;
// bit 29: the state is the destination of some epsilon arc, i.e. the epsilon closure may look
// it up - only such tokens are entered in the global hash table (the emitting pass dedupes in LDS)
constexpr int32_t kEpsDst = 0x20000000;
constexpr uint32_t kEncInf = 0xFF800000u;  // Enc(+inf)
constexpr unsigned long long kEmpty = 0ull;

__host__ __device__ __forceinline__ uint32_t Enc(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float Dec(uint32_t e) {
  uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  return __builtin_bit_cast(float, u);
}

// Device pointers kept in structs are declared in address space 1 (global): a plain
// `T *` loaded from memory is a GENERIC pointer to hipcc, which then emits
// flat_load / flat_store (address-space check per access, counted on vmcnt AND
// lgkmcnt) and — MI355X guide, Guideline 16 — an sc1 flat_ access is not a
// dependable L1 bypass.  With the address space in the type every access below is
// a global_* instruction.
#define GP(T) __attribute__((address_space(1))) T *

// A global array addressed with a 32-BIT UNSIGNED BYTE OFFSET: a[i] is
// *(base + zext(uint32(i) * sizeof(T))), exactly the "SGPR base + 32-bit VGPR offset"
// form of global_load / global_store / global_atomic.  With plain pointers and int
// indices every access sign-extends and shifts to a 64-bit address in a VGPR pair of
// its own (464 of the kernel's 579 loads did), which is what pushed the sweeps over
// 64 VGPRs; here the six SoA arrays of a link sweep share ONE offset register.
// Precondition (checked on the host): count * sizeof(T) < 4 GiB.
template <class T>
struct Arr {
  GP(T) p;
  Arr() = default;
  __host__ __device__ Arr(GP(T) q) : p(q) {}
  template <class U>
  __host__ __device__ Arr(const Arr<U> &o) : p(o.p) {}
  __device__ __forceinline__ __attribute__((address_space(1))) T &operator[](int i) const {
    return *(GP(T))((__attribute__((address_space(1))) char *)p + static_cast<uint32_t>(i) * static_cast<uint32_t>(sizeof(T)));
  }
  __device__ __forceinline__ __attribute__((address_space(1))) T &operator[](uint32_t i) const {
    return *(GP(T))((__attribute__((address_space(1))) char *)p + i * static_cast<uint32_t>(sizeof(T)));
  }
  __host__ __device__ operator GP(T)() const { return p; }
};
// 16-byte arc record as a native vector (HIP's int4 is a class; it cannot be
// loaded through an address-space-qualified pointer)
typedef int KhInt4 __attribute__((ext_vector_type(4)));
// Four consecutive 4-byte elements of an SoA array with ONE 16-byte access per lane, at any 4-byte
// alignment: a coalesced dword-per-lane sweep streams at 3.3 TB/s on this part, the same sweep with 16
// bytes per lane at 5.6 TB/s (profiles/r02_pmc_calibration.txt: CalStreamDword / CalStreamDwordx4).
typedef int KhInt4U __attribute__((ext_vector_type(4), aligned(4)));
typedef float KhFloat4 __attribute__((ext_vector_type(4)));
typedef float KhFloat4U __attribute__((ext_vector_type(4), aligned(4)));
template <class T>
__device__ __forceinline__ KhInt4 Load4I(const Arr<T> &a, int i) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  return *(__attribute__((address_space(1))) const KhInt4U *)((__attribute__((address_space(1))) const char *)a.p + static_cast<uint32_t>(i) * 4u);
}
template <class T>
__device__ __forceinline__ KhFloat4 Load4F(const Arr<T> &a, int i) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  return *(__attribute__((address_space(1))) const KhFloat4U *)((__attribute__((address_space(1))) const char *)a.p + static_cast<uint32_t>(i) * 4u);
}
template <class T>
__device__ __forceinline__ void Store4I(const Arr<T> &a, int i, KhInt4 v) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  *(__attribute__((address_space(1))) KhInt4U *)((__attribute__((address_space(1))) char *)a.p + static_cast<uint32_t>(i) * 4u) = v;
}
// Non-temporal forms (the nt cache policy: the line is not kept in L2 for this access): for the arrays a frame writes once
// and nobody reads before the next pruning visit - far behind in the stream - and for that visit's reads.  What they no
// longer displace is the part of the arc table the next frames re-read (the active states of consecutive frames overlap).
template <class T>
__device__ __forceinline__ KhInt4 Load4I_NT(const Arr<T> &a, int i) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  return __builtin_nontemporal_load((__attribute__((address_space(1))) const KhInt4U *)((__attribute__((address_space(1))) const char *)a.p + static_cast<uint32_t>(i) * 4u));
}
template <class T>
__device__ __forceinline__ KhFloat4 Load4F_NT(const Arr<T> &a, int i) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  return __builtin_nontemporal_load((__attribute__((address_space(1))) const KhFloat4U *)((__attribute__((address_space(1))) const char *)a.p + static_cast<uint32_t>(i) * 4u));
}
template <class T>
__device__ __forceinline__ void Store4I_NT(const Arr<T> &a, int i, KhInt4 v) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  __builtin_nontemporal_store(v, (__attribute__((address_space(1))) KhInt4U *)((__attribute__((address_space(1))) char *)a.p + static_cast<uint32_t>(i) * 4u));
}
template <class T>
__device__ __forceinline__ void Store4F(const Arr<T> &a, int i, KhFloat4 v) {
  static_assert(sizeof(T) == 4, "4-byte elements");
  *(__attribute__((address_space(1))) KhFloat4U *)((__attribute__((address_space(1))) char *)a.p + static_cast<uint32_t>(i) * 4u) = v;
}

// Per-slot temporaries of the exact reference order (see "exact reference order" below).
struct UttX {
  // ---- exact reference order (Params::exact_order; carved only then).  [tok_frame_cap] unless noted.
  Arr<int32_t> x_pos;      // frontier token (i - frame begin) -> its position in the reference's HashList order
  Arr<uint32_t> x_m;       // by list position: Enc(min tot_cost + adaptive_beam) over the token's emitting arcs; after the scan the running next_cutoff BEFORE the token
  Arr<int32_t> x_c;        // by list position: # emitting arcs expanded; after the scan their exclusive prefix sum (ordinal of the token's first candidate)
  Arr<uint32_t> x_q;       // token of the frame under construction (i - nb) -> insertion key (order of HashList::Insert calls)
  Arr<int32_t> x_bkt;      // ... -> HashList bucket (caller's state id % hash size)
  Arr<int32_t> x_epsidx;   // ... -> index in tmp_epslist, or -1
  Arr<int32_t> x_nl0; Arr<int32_t> x_nl1;   // closure replay, by tmp_epslist index: the token's epsilon link slots [l0, l1) relative to the block
  Arr<float> x_ncost;      // closure replay: token cost as the replay proceeds
  Arr<int32_t> x_ord;      // [link_frame_cap] candidate ordinal of a materialised emitting candidate; then the closure replay's link destination codes
  Arr<float> x_lw;         // [link_frame_cap] closure replay: link weight
  Arr<int32_t> x_stack;    // [link_frame_cap] closure replay: the LIFO queue (:766-811)
  Arr<uint32_t> x_bmin;    // [x_hcap] HashList bucket -> smallest insertion key in it (all ones = empty: invariant between frames)
  Arr<unsigned long long> x_key0; Arr<unsigned long long> x_key1;   // radix sort keys, double buffered
  Arr<int32_t> x_val0; Arr<int32_t> x_val1;                         // radix sort payload
  Arr<int32_t> x_h; Arr<int32_t> x_inb;   // token of the frame under construction -> insertion rank of its bucket's first token; its rank inside the bucket
  Arr<uint32_t> x_c0e;     // entry of tmp_epslist made by the emitting pass -> the token's cost image before the epsilon closure
  Arr<int32_t> x_csid;     // [link_frame_cap] materialised candidate -> the caller's id of its destination state (what the reference hashes)
  Arr<const KhInt4> x_rec0;   // the graph's own records (KhFst::rec): in this mode the decoder's copy carries the caller's id of an
                              // arc's destination state where the output label was, and the export reads the label from here
  int32_t x_hcap;
};

// Per-utterance arenas and parameters (device-resident array of these).
//
// Tokens and links live in one append-only arena each, in frame order:
//   tokens: frame 0, frame 1, ...          links: eps(0), emit(0), eps(1), emit(1), ...
// Every prune_interval frames the tail of both arenas — the "window" = all frames
// since the compaction before the previous one — is compacted in place (sliding
// the survivors down).  Frames older than the window have been compacted twice
// (the second time >= prune_interval frames behind the frontier, i.e. already
// thinned to lattice density) and never move again.
struct Utt {
  // inputs
  GP(const float) ll;   // first row of this utterance's log-likelihood matrix
  int32_t ll_stride, T;
  // token arena
  int32_t tok_cap;
  Arr<int32_t> tok_state;    // HCLG state, -1 = pruned token
  Arr<uint32_t> tok_cost;    // Enc(tot_cost); free slots hold Enc(+inf)
  Arr<float> tok_extra;
  // link arena
  int32_t link_cap;
  Arr<int32_t> link_dst; Arr<int32_t> link_arc;   // dst: token index, -1 = excised; arc: index of the emitting arc, or -1 - index of the epsilon arc (labels are read from the arc at export)
  Arr<int32_t> link_src;     // owning token (links are also walked link-parallel)
  // link_k: the part of link_extra_cost (:309-311) that does not depend on extra_costs: for an emitting link the
  // candidate's tot_cost = (cost[src] + acoustic) + graph until the frame's first pruning visit, which turns it
  // into tot_cost - cost[dst] (cost[dst] is final by then); for an epsilon link that difference from its creation
  // on.  link_a: acoustic cost (emitting links only).  The graph cost of a link is its arc's weight (read at export).
  Arr<float> link_k; Arr<float> link_a;
  // per-frame bookkeeping
  Arr<int32_t> frame_b; Arr<int32_t> frame_e;      // [T+2] token range of frame f
  Arr<int32_t> feps_b; Arr<int32_t> feps_e;        // [T+2] link range of eps(f)
  Arr<int32_t> femit_b; Arr<int32_t> femit_e;      // [T+2] link range of emit(f)
  Arr<float> cost_offset;    // [T+1]
  Arr<uint8_t> must_links;   // [T+2] must_prune_forward_links
  Arr<uint8_t> must_toks;    // [T+2] must_prune_tokens
  // temporaries
  Arr<int32_t> tmp_slot;     // [tok_frame_cap] hash slot of frontier token (i - frontier begin)
  Arr<int32_t> tmp_dirty;    // [tok_frame_cap] 1 = queued in a nonemitting work list; all zero outside ProcessNonemitting
  Arr<int32_t> tmp_work0; Arr<int32_t> tmp_work1;  // [tok_frame_cap] nonemitting work lists (token indices), double buffered
  Arr<int32_t> tmp_epslist;  // [tok_frame_cap] the frontier's tokens whose state has epsilon arcs (each once, in creation order)
  Arr<float> tmp_f0;         // [tok_frame_cap] prune: extra_cost on entry (i - frame begin)
  Arr<uint32_t> tmp_acc0; Arr<uint32_t> tmp_acc1;  // [tok_frame_cap] prune: Enc(min link_extra_cost) over emitting / epsilon links
  Arr<int32_t> tmp_remap;    // [window_cap] compaction remap (i - window begin)
  int32_t tok_frame_cap, link_frame_cap, window_cap;
  // survivors of FinalizeDecoding (lazy schedule): {token index, frame} / {link slot, frame} pairs, what ExportSurvivors copies
  Arr<int32_t> surv_tok; Arr<int32_t> surv_link;
  int32_t surv_tok_cap, surv_link_cap;
  // hash
  Arr<unsigned long long> hash;
  uint32_t hash_mask;
  GP(long long) phase_cycles;  // [16] diagnostic (KH_DECODER_PROFILE=1), else nullptr
};

struct Params {
  Arr<const KhInt4> rec;      // the decoder's copy of KhFst::rec with the pdf in the first word of every arc unit
  Arr<const KhInt4> n_arcs;
  Arr<const int32_t> unit_ilabel;
  int32_t start, num_units, num_eps, start_has_eps;
  int32_t max_emit;           // largest emitting fan-out of a state (reference order: 16-bit arc counts in LDS when it fits)
  int32_t ll_cols;  // > 0: columns of the log-likelihood matrix, staged per frame in LDS
  int32_t keep_ac;  // 1: links store their acoustic cost (online decoding: a chunk's scores are gone when the lattice is
                    // exported); 0: it is recomputed at export from the score matrix, cost_offset[f] - loglike(f, pdf of the
                    // arc) - the same float expression - and the expansion writes one stream less per candidate
  int32_t max_tid;
  // 1 (offline batch decoding): the backward pruning between frames runs only when a slot's arenas are about to fill up
  // (a garbage collection), and FinalizeDecoding prunes every frame - most of them for the first and only time.  Under
  // the canonical rule P (exact fixed point, then excise) the final lattice does not depend on WHEN the intermediate
  // PruneActiveTokens calls run: an extra_cost computed against a frontier at frame t is a lower bound of the one
  // FinalizeDecoding computes (the frontier's own extra_costs, 0 at the time, only grow; float addition and min are
  // monotone), so a link excised early is excised at the end as well, and the final sweep recomputes every surviving
  // token's extra_cost from scratch.  0: PruneActiveTokens every prune_interval frames as :88-89 (online decoding, whose
  // mid-utterance getters expose that state).
  int32_t lazy_prune;
  // lazy schedule, online streams (round 6): a garbage collection also once this many frames have gone unpruned, not only
  // when the arenas run low - the collection of a 2000-frame backlog in the middle of an utterance was a 100 - 500 ms
  // stall of that stream's chunk (KH_SERVE_LAZY_SPAN frames; 0 = arenas only, the offline kernel's rule and the DEFAULT:
  // see OnlineLazySpan).  The lattice does not depend on when the collections run.
  int32_t lazy_span;
  // 1: the reference's iteration order is reproduced (HashList order, running next_cutoff, first-minimum tie, the LIFO
  // order of the epsilon closure's insertions) - see "exact reference order" below; the kernels are instantiated for it
  int32_t exact_order;
  // epsilon closure in LDS (ClosureLds): entries its table may take (<= kClMaxLoad; 0 = every frame takes the general
  // routine).  KH_DECODER_CLOSURE_CAP lowers it: the tests run whole suites through the general routine (0) and through
  // tables that fill up on the way (a handful of entries).
  int32_t cl_max_load;
  float hash_ratio;
  float beam, lattice_beam, beam_delta, prune_scale;
  int32_t max_active, min_active, prune_interval;
};

// slots of the LDS token table the emitting pass dedupes a frame's new tokens in (kh_decoder.hip: LdsKeys / LdsVals)
constexpr int kLdsSlots = 8192;
// dynamic LDS of the decode kernels: the score row or the table's values, whichever is larger
inline size_t DynLdsBytes(int ll_cols) { return std::max(sizeof(float) * static_cast<size_t>(ll_cols), sizeof(uint32_t) * static_cast<size_t>(kLdsSlots)); }
// most entries the LDS epsilon-closure table takes (Params::cl_max_load; kh_decoder.hip: ClosureLds)
constexpr int kClMaxLoad = 1300;

#ifndef KH_COMPACT_EVERY
#define KH_COMPACT_EVERY 2   // the window is compacted at every KH_COMPACT_EVERY-th call of PruneActiveTokens
#endif
#ifndef KH_WG_PER_CU
#define KH_WG_PER_CU 2   // two 1024-thread workgroups per CU (<= 64 VGPRs): more loads in flight
#endif

// Per-utterance inputs / outputs of the batch and the lattice pool the finished
// utterances are exported to (so that the slot's arenas can be reused).
struct UttIn {
  GP(const float) ll;
  int32_t T, pad;
};
struct UttOut {
  KhDecodeStats stats;
  long long tok_off, link_off;  // position in the pool
  int32_t n_tok, n_link;
  int32_t sched[4];             // Shared::sched of the utterance
  long long cand_mat;           // emitting candidates materialised (got a link slot)
};
struct Pool {
  GP(int32_t) t_frame; GP(int32_t) t_state;   // per exported token
  GP(int32_t) l_src; GP(int32_t) l_dst; GP(int32_t) l_il; GP(int32_t) l_ol;  // per exported link (utterance-relative)
  GP(float) l_g; GP(float) l_a;               // graph cost, acoustic cost - cost_offset[frame]
  long long tok_cap, link_cap;
  GP(unsigned long long) used;                // [0] tokens, [1] links, [2] utterance queue head
};

// Online decoding (OnlineKernel / ServeKernel): between launches the workgroup's LDS scalars live in SlotState.
struct SlotState {
  int32_t tok_end, link_end, front_b, status, max_tokens_frame, tok_hw, gc_tok, gc_link;
  int32_t t, fb, fe;          // Run
  int32_t ok, finalized, conv_upto;
  int32_t surv_nt, surv_nl;   // (lazy schedule) survivor lists of FinalizeDecoding
  uint32_t x_hsize;           // (reference order) HashList::hash_size_ of the stream's decoder (:219-225: it never shrinks)
  int32_t pad_;
  long long arcs_expanded, tokens_created;
  KhDecodeStats stats;        // valid once finalized
};
enum { kJobInit = 0, kJobAdvance = 1, kJobFinalize = 2, kJobExport = 3 };
struct Job {
  int32_t slot, op;
  GP(const float) ll;         // kJobAdvance: matrix addressed by ABSOLUTE frame (chunk pointer - t * stride)
  int32_t ll_stride, n_frames;
};

// Control block of a serving stream in pinned host memory (ServeKernel).
struct ServeCtl {
  int32_t avail, cmd_seq, cmd_op, pad0;     // host -> device
  int32_t ack_seq, decoded, ok, alive;      // device -> host
  // device -> host, diagnostics: what the stream's workgroup is doing (0 waiting, kActInit / kActAdvance / kActFinalize,
  // 9 = has left), the frame count it is advancing to, how many actions it has finished, the low word of the wall clock
  // (100 MHz) when it last started or finished one - what kh_online_decoder_serve_wait / _stop report when they time out
  int32_t hb_phase, hb_arg, hb_actions, hb_clock;
  int32_t hw;                               // device -> host: token slots of the stream's arena that hold something (InitDecoding resets them)
  int32_t pad1[3];                          // [0]: -DKH_SERVE_MARKERS progress word; [1]: device -> host, the kernel's status code behind ok == 0
};
static_assert(sizeof(ServeCtl) == 64, "one control block per 64-byte line");
// kCmdInitCleared: InitDecoding whose reset of the token arena the HOST has done (a fill kernel over the whole chip: the
// unpruned utterance of a lazy-schedule stream leaves ~70 MB to reset, 0.23 s for one workgroup - the 200 ms outliers of the
// round-4 chunk latencies were the first chunk of a slot's next utterance waiting for it)
enum { kCmdInit = 1, kCmdFinalize = 2, kCmdInitCleared = 3 };

// ---- host launchers, defined in kh_decoder.hip next to the kernels they launch.  Each is the plain launch (or attribute
// call) and nothing else: the caller keeps its KH_LAUNCH_CHECK() / KH_HIP().
void LaunchDecode(bool lazy, bool exact, int grid, size_t dyn_lds, hipStream_t st, const Utt *slots, const UttIn *in, UttOut *out,
                  int n_utts, const Pool &pool, const Params &p, GP(long long) phase_cycles, GP(int32_t) done_list, const UttX *slotsx);
void LaunchOnline(bool exact, unsigned grid, size_t dyn_lds, hipStream_t st, const Utt *slots, SlotState *states, const Job *jobs,
                  UttOut *out, const Pool &pool, const Params &p, const UttX *slotsx);
void LaunchServe(bool exact, unsigned grid, size_t dyn_lds, hipStream_t st, const Utt *slots, SlotState *states, ServeCtl *ctl,
                 int32_t *quit, const float *ll_base, long long ll_rows_per_stream, int ll_stride, const Params &p,
                 long long idle_ticks, long long *act_clock, const UttX *slotsx);
hipError_t ServeStaticLds(bool exact, size_t *bytes);    // static LDS of ServeKernel<exact> (hipFuncGetAttributes)
hipError_t SetServeDynLds(bool exact, size_t bytes);     // hipFuncAttributeMaxDynamicSharedMemorySize of ServeKernel<exact>
size_t DecodeStaticLds();                                // sizeof(Shared): the static LDS block of every decode kernel
void LaunchFillU32(hipStream_t st, uint32_t *p, size_t n, uint32_t v);
void LaunchArcPdf(int grid, hipStream_t st, const int32_t *unit_ilabel, long long n, const int32_t *tid2pdf, int4 *rec, int num_cols,
                  int *bad, const int4 *rec0, int order_ids);
// debug builds: the device symbols belong to kh_decoder.hip's code object, so the copies to / from them live there
#ifdef KH_BOUNDS_CHECK
hipError_t ReadOob(int h[8]);
hipError_t ClearOob();
#endif
#ifdef KH_BARRIER_CHECK
hipError_t ReadBarMisaligned(int h[4]);
hipError_t ClearBarMisaligned();
#endif
#ifdef KH_SERVE_MARKERS
hipError_t SetServeMark(int32_t *mark);
hipError_t SetWaveMark(int32_t *mark);
#endif

}  // namespace dec
}  // namespace kh

#endif  // KH_DECODER_TYPES_H_
