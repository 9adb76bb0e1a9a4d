// kh_tree.hip - the tree statistics of a batch of frames (acc-tree-stats).
//
// Replaces GaussClusterable::AddStats (tree/clusterable-classes.cc:137-142) under the frame loop of AccumulateTreeStats
// (hmm/tree-accu.cc:88-102), for frames whose event - the phonetic context and pdf-class the frame belongs to - the host has
// already worked out (api.tree_stats_frame_events).  Per frame t of event e, weight 1.0:
//     count[e] += 1,   stats[e][0][d] += double(x[d]),   stats[e][1][d] += double(fl32(x[d] * x[d])).
// Row 1 is AddVec2's alpha == 1.0 branch (matrix/kaldi-vector.cc:1044-1049): the product of two floats rounded to float, then
// widened; it is written __fmul_rn so that nothing can fuse it with the add.
//
// ORDER.  The reference's sums are fixed-order chains of double adds, so they are reproduced bit for bit: for every (event,
// column) ONE lane starts from the incoming value (add) or from zero and adds the event's frames in ascending frame order -
// which is utterance order, then time, as the reference meets them.  A chain is never cut into partial sums and no sum is
// shared between lanes: no atomics, no reduction, and a job gives the same bits however it is cut into calls that run on from
// one another with add.  The count is a whole number added on the host: exact below 2^53.
//
// TILING.  A work item is (event, block of 64 columns) and belongs to one wave, a workgroup of its own.  The wave walks the
// event's run of frame indices (kh_tree_plan.h: a stable counting sort by event) kTile rows at a time: ALL 64 lanes gather the
// tile's rows x the block's columns into LDS, element i of the tile (row i / width, column i % width, width = the block's
// columns) by lane i % 64 - so a 40-column row does not leave 24 lanes idle and the loads of a tile are in flight together -
// and lane d then adds column d of the tile's rows in order, in double.  The tile's frame indices are brought into LDS first,
// by one coalesced load, so that an element's load does not wait for a load of its own index; the gather makes kBatch = 8
// loads per lane, none of them behind a branch, before it stores any of them (32 at a time took 202 VGPRs: 2 waves per
// SIMD).  The LDS image is kTile rows at a pitch of 64 floats: lane d reads bank d, no conflict.
// Static LDS of TreeAccumulateKernel at every D: 32 x 64 x 4 + 32 x 4 = 8320 bytes.
//
// TAIL.  The chain of an event is serial by contract, so the longest event bounds the kernel: the plan launches the events
// by falling run length, the silence events first, and the short triphone events fill the machine beside them.
//
// TRANSFERS.  stats travels whole: all num_events rows go up under add and all come back, the events without a frame too, so
// a caller passes the events its frames touch (api.TreeStats compacts them), not a job's table.  Packing only the touched
// rows on the host was built and measured on the rate tool's set (26 279 of 40 005 events touched): the call went from 2.7
// to 4.5 ms from zero and from 3.2 to 5.7 ms running on - the host's gather, zero fill and scatter of 17 - 26 MB cost more
// than the 9 MB less that crossed the bus.
//
// Supported D: 1 ... 512 (kMaxD), KH_EINVAL above, before any launch.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmstats.h"
#include "kh_tree_plan.h"

using namespace kh;

namespace {

thread_local float g_ms[3] = {0.f, 0.f, 0.f};      // whole call; host plan (check, sort, work list); kernel (events)
thread_local int32_t g_counts[4] = {0, 0, 0, 0};   // frames used; events with a frame; work items (waves); longest run

constexpr int kTile = 32;            // rows staged in LDS per step
constexpr int kBatch = 8;            // loads per lane in flight while a tile is gathered
constexpr int kCols = kh_tree::kCols;
constexpr int kMaxD = 512;
static_assert(kCols == 64, "a lane per column of a work item");

// grid (work items); event_offsets [E + 1] into sorted_row; stats [E][2][D] holds the incoming sums (zeros without add)
__global__ void __launch_bounds__(64)
TreeAccumulateKernel(const float *__restrict__ feats, int feat_stride, int D, const int32_t *__restrict__ sorted_row,
                     const int32_t *__restrict__ event_offsets, const int32_t *__restrict__ work_event,
                     const int32_t *__restrict__ work_block, double *__restrict__ stats) {
  __shared__ float tile[kTile * kCols];
  __shared__ int32_t rows[kTile];
  const int lane = threadIdx.x;
  const int e = __builtin_amdgcn_readfirstlane(work_event[blockIdx.x]);
  const int c0 = __builtin_amdgcn_readfirstlane(work_block[blockIdx.x]) * kCols;
  const int width = D - c0 < kCols ? D - c0 : kCols;
  const int i0 = __builtin_amdgcn_readfirstlane(event_offsets[e]), i1 = __builtin_amdgcn_readfirstlane(event_offsets[e + 1]);
  const bool mine = lane < width;
  double *out = stats + static_cast<size_t>(e) * 2 * D + c0 + lane;
  double s1 = 0.0, s2 = 0.0;
  if (mine) {
    s1 = out[0];
    s2 = out[D];
  }
  // element i = 64 k + lane of a tile is (row i / width, column i % width); from k to k + 1 both move by these steps
  const int step_r = kCols / width, step_c = kCols - step_r * width;
  for (int t0 = i0; t0 < i1; t0 += kTile) {
    const int n = i1 - t0 < kTile ? i1 - t0 : kTile;
    __syncthreads();   // the previous tile has been added
    if (lane < n) rows[lane] = sorted_row[t0 + lane];   // the tile's frame indices: one coalesced load, not one per element
    __syncthreads();
    int r = lane / width, c = lane - r * width;
    // kBatch elements per lane at a time: the loads first, every one of them made - a row past the tile reads the tile's
    // last row instead, so no load hides behind a branch and all kBatch are in flight together - and then the stores
    for (int k = 0; k * kCols < n * width; k += kBatch) {
      float v[kBatch];
      int at[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int rr = r < n ? r : n - 1;
        v[u] = feats[static_cast<size_t>(rows[rr]) * feat_stride + c0 + c];
        at[u] = r < n ? r * kCols + c : -1;
        r += step_r;
        c += step_c;
        if (c >= width) {
          c -= width;
          r++;
        }
      }
#pragma unroll
      for (int u = 0; u < kBatch; u++)
        if (at[u] >= 0) tile[at[u]] = v[u];
    }
    __syncthreads();
    if (mine)
      for (int j = 0; j < n; j++) {
        const float x = tile[j * kCols + lane];
        s1 += static_cast<double>(x);
        s2 += static_cast<double>(__fmul_rn(x, x));
      }
  }
  if (mine) {
    out[0] = s1;
    out[D] = s2;
  }
}

}  // namespace

extern "C" {

int kh_tree_acc_stats(const float *feats, int T, int D, int feat_stride, const int32_t *frame_event, int num_events, int add,
                      double *count, double *stats) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_tree_acc_stats";
  KH_CHECK_ARG(T >= 0 && num_events >= 0);
  KH_CHECK_ARG(T == 0 || (feats && frame_event));
  KH_CHECK_ARG(num_events == 0 || (count && stats));
  if (D < 1 || D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  if (feat_stride < D) {
    SetError("%s: feat_stride %d is less than the feature dimension %d", fn, feat_stride, D);
    return KH_EINVAL;
  }
  std::string err;
  if (!kh_tree::Check(T, frame_event, num_events, &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  g_ms[1] = g_ms[2] = 0.f;
  g_counts[0] = g_counts[1] = g_counts[2] = g_counts[3] = 0;
  const size_t n_stats = static_cast<size_t>(num_events) * 2 * D;
  kh_tree::Plan plan;
  kh_tree::Build(T, frame_event, num_events, D, &plan);
  const size_t items = plan.work_event.size();
  if (items > static_cast<size_t>(INT32_MAX)) {
    SetError("%s: %zu work items (events with a frame x blocks of %d columns), at most 2^31 - 1", fn, items, kCols);
    return KH_EINVAL;
  }
  g_counts[0] = plan.used;
  g_counts[1] = plan.events_used;
  g_counts[2] = static_cast<int32_t>(items);
  g_counts[3] = plan.longest;
  // count[e]: the prior value (add) or zero, plus the frames of the run - written once the sums have come back
  auto add_counts = [&]() {
    for (int e = 0; e < num_events; e++)
      count[e] = (add ? count[e] : 0.0) + static_cast<double>(plan.event_offsets[e + 1] - plan.event_offsets[e]);
  };
  g_ms[1] = clk.Ms();
  if (items == 0) {     // T = 0, E = 0 or every frame -1: zeros, or unchanged under add
    if (!add) std::fill(stats, stats + n_stats, 0.0);
    add_counts();
    g_ms[0] = clk.Ms();
    return KH_OK;
  }
  Scratch sc;
  const int32_t *d_row = sc.Upload(plan.sorted_row.data(), plan.sorted_row.size());
  const int32_t *d_off = sc.Upload(plan.event_offsets.data(), plan.event_offsets.size());
  const int32_t *d_we = sc.Upload(plan.work_event.data(), items);
  const int32_t *d_wb = sc.Upload(plan.work_block.data(), items);
  double *d_stats = add ? sc.Upload(stats, n_stats) : sc.Get<double>(n_stats);
  if (!d_row || !d_off || !d_we || !d_wb || !d_stats) {
    SetError("%s: out of device memory (%d frames, %d events, %zu work items)", fn, plan.used, num_events, items);
    return KH_ENOMEM;
  }
  if (!add) KH_HIP(hipMemsetAsync(d_stats, 0, sizeof(double) * n_stats, Stream()));
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  ev.Begin();
  hipLaunchKernelGGL(TreeAccumulateKernel, dim3(static_cast<unsigned>(items)), dim3(64), 0, Stream(), feats, feat_stride, D, d_row, d_off,
                     d_we, d_wb, d_stats);
  ev.End();
  float ms = 0.f;
  const hipError_t e = ev.Collect(stats, d_stats, n_stats, &ms);
  if (e != hipSuccess) {
    SetError("%s: %s", fn, hipGetErrorString(e));
    return KH_EDEVICE;
  }
  add_counts();
  g_ms[2] = ms;
  g_ms[0] = clk.Ms();
  return KH_OK;
}

int kh_tree_max_dim(void) { return kMaxD; }
int kh_tree_tile(void) { return kTile; }

int kh_tree_last_timings(float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms && counts);
  for (int i = 0; i < 3; i++) ms[i] = g_ms[i];
  for (int i = 0; i < 4; i++) counts[i] = g_counts[i];
  return KH_OK;
}

}  // extern "C"
