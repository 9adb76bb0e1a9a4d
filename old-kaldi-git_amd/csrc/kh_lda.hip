// kh_lda.hip - the LDA statistics of a batch of frames (acc-lda).
//
// Replaces LdaEstimate::Accumulate (transform/lda-estimate.cc:45-55) under the loop of bin/acc-lda.cc:101-110, for (frame,
// pdf, weight) entries whose weights RandPrune has already been applied to (kh_rand_prune_at, kh_mllt.hip).  An item is an
// entry whose weight is not zero (-0.0 is zero, a NaN is an item: "if (weight != 0.0)").  Per item, w and x widened to double,
//     zero[c] += w,   first[c][d] += w x[d],   second[a, b] += (w x[a]) x[b]   for every packed pair a >= b,
// second [Q], Q = D (D + 1) / 2, packed as SpMatrix packs ((r, c), r >= c, at r (r + 1) / 2 + c).  w x[d] is the exact
// product of two widened floats (48 bits); the outer product of `second` rounds once, or not at all inside a fused multiply-add.
//
// SECOND ORDER.  Over the items of a slice it is the lower triangle of the weighted SYRK  X^T diag(w) X  on the fp64 matrix
// cores.  A workgroup is one (slice, pair of 64-column super tiles (R, C), R >= C): it stages kSub items at a time in LDS -
// the A image  double(w) * double(x[64 R + d])  and the B image  x[64 C + d],  both made while staging, rows and columns past
// D and items past the slice as zeros - and wave v owns row tile 4 R + v against the column tiles 4 C + j, j = 0 ... 3: one A
// fragment per four matrix-core operations.  In a diagonal super tile (R == C) wave v computes j <= v only, a tile that lies
// wholly past D is not computed, and a diagonal tile writes its lower half only.  Neither operand is stored in memory.  The LDS image does not depend on D; each feature
// row is read once per super-tile pair that needs its columns (ceil(D / 64) + 1 times in all), from the L2 / MALL mostly.
// v_mfma_f64_16x16x4_f64: A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15], one double per lane; C/D col = lane & 15,
// row = (lane >> 4) + 4 * reg (the operand layout of MlltAccumulateKernel, kh_mllt.hip).
//
// THE SUM TREE is fixed by the input alone.  The items are taken in entry order.  Within a segment (an utterance of the
// call) they are cut into slices of  slice_len = kChunk * max(1, ceil(n_seg / (kChunk * kMaxSlices)))  items, n_seg the
// segment's item count.  Every slice writes its partial [Q] to a workspace; LdaReduceKernel adds, per element, a segment's
// slices in slice order from zero, and the segments' sums in segment order onto (add ? what the buffer held : zero).  A
// segment without items adds nothing.  The workspace limit (kh_lda_set_workspace_limit; default 1 GiB) cuts the call into
// passes over runs of whole slices - one accumulation launch and one reduction launch per pass - and the reduction carries
// the running segment sum and the total from pass to pass in two [Q] buffers, so no sum depends on the limit.  A job gives
// the same bits however its utterances are grouped into calls: with `add` a later call runs on from the buffers.
//
// FIRST ORDER AND COUNTS.  The items are sorted by class (a stable counting sort: entry order within a class, hence segment
// order).  A class's run within one segment is cut into chunks of kChunk items; a chunk's partial is added item by item from
// zero, the chunks in chunk order onto the (segment, class) sum from zero, and those sums in segment order onto (add ? what
// the buffer held : zero).  LdaFirstKernel: one lane per (class, d), one wave per (class, 64 columns), walking the class's
// items; the host marks where a chunk and where a segment's run begins.  Plain vector fp64: a gather bound by memory.  A
// class with many items is a serial walk; the classes run side by side.  One launch per call, whatever the passes.
//
// Supported D: 1 ... 512 (kMaxD): a slice's partial is then 1.05 MB, at most kMaxSlices of them per segment; 40-dimensional
// features spliced +-4 with a 100-dimensional iVector are 460.  KH_EINVAL above, before any launch.
// Static LDS of LdaAccumulateKernel at every D: the A image kSub x kAs doubles and the B image kSub x kBs floats:
// 32 x 80 x 8 + 32 x 80 x 4 = 30720 bytes.  kAs = 80 doubles = 160 = 32 mod 64 banks: the two items of a half-wave's A
// fragment, 16 consecutive doubles each, fall on disjoint halves of the banks.  kBs = 80 = 16 mod 64: the four items of a B
// fragment, 16 consecutive floats each, fall on four disjoint runs of 16 banks.
// Accumulator registers per wave at every D: 4 column tiles x 4 doubles = 32 VGPRs (tests/test_lda_kernel_resources.py
// reads the totals from the compiler).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmacc_plan.h"
#include "kh_gmmstats.h"

using namespace kh;

namespace {

thread_local float g_ms[3] = {0.f, 0.f, 0.f};      // whole call; host plan (checks, item list, slices, sort); kernels (events)
thread_local int32_t g_counts[4] = {0, 0, 0, 0};   // items; slices; workgroups of the accumulate kernel; passes
thread_local size_t g_ws_limit = 0;                // kh_lda_set_workspace_limit
constexpr size_t kDefaultWorkspace = size_t(1) << 30;

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kChunk = 256;          // items per slice, times a whole number; items per chunk of the first-order walk
constexpr int kMaxSlices = 256;      // slices of one segment
constexpr int kSub = 32;             // items staged in LDS at a time
constexpr int kWaves = 4;
constexpr int kSuper = 64;           // columns of a super tile: kWaves row tiles, 4 column tiles
constexpr int kAs = 80;              // row pitch of the A image (doubles)
constexpr int kBs = 80;              // row pitch of the B image (floats)
constexpr int kMaxD = 512;
constexpr int kFirstWaves = 4;       // classes per workgroup of LdaFirstKernel
static_assert(kChunk % kSub == 0 && kSub % 4 == 0, "chunking");
static_assert(kSuper == 16 * kWaves && kSuper <= kAs && kSuper <= kBs, "images");

inline int64_t SliceLen(int64_t n) { return kChunk * std::max<int64_t>(1, DivUp64(n, static_cast<int64_t>(kChunk) * kMaxSlices)); }

// grid (slices of the pass, super-tile pairs); slice_begin / slice_end: item ranges; partial [slices of the pass][Q]
__global__ void __launch_bounds__(64 * kWaves)
LdaAccumulateKernel(const float *__restrict__ feats, int feat_stride, int D, const int32_t *__restrict__ item_row,
                    const float *__restrict__ item_w, const int32_t *__restrict__ slice_begin, const int32_t *__restrict__ slice_end,
                    double *__restrict__ partial) {
  __shared__ double as[kSub][kAs];
  __shared__ float bs[kSub][kBs];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Q = D * (D + 1) / 2;
  // blockIdx.y = R (R + 1) / 2 + C, R >= C
  int R = 0;
  while ((R + 1) * (R + 2) / 2 <= static_cast<int>(blockIdx.y)) R++;
  const int C = static_cast<int>(blockIdx.y) - R * (R + 1) / 2;
  const int i_begin = slice_begin[blockIdx.x], i_end = slice_end[blockIdx.x];
  // column tiles of this wave: the lower triangle in a diagonal super tile, and none that lies wholly past D
  const int in_d = (D - C * kSuper + 15) >> 4;
  const int lower = R == C ? wave + 1 : 4;
  const int n_col = R * kSuper + wave * 16 >= D ? 0 : (lower < in_d ? lower : in_d);
  f64x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int s0 = i_begin; s0 < i_end; s0 += kSub) {
    __syncthreads();   // the previous step's fragments have been read
    for (int i = t; i < kSub * kSuper; i += 64 * kWaves) {
      const int f = i >> 6, d = i & 63, it = s0 + f;
      double a = 0.0;                    // past the slice or past D: zeros
      float b = 0.f;
      if (it < i_end) {
        const float *x = feats + static_cast<size_t>(item_row[it]) * feat_stride;
        const int da = R * kSuper + d, db = C * kSuper + d;
        if (da < D) a = static_cast<double>(item_w[it]) * static_cast<double>(x[da]);   // exact
        if (db < D) b = x[db];
      }
      as[f][d] = a;
      bs[f][d] = b;
    }
    __syncthreads();
#pragma unroll 2
    for (int k0 = 0; k0 < kSub; k0 += 4) {
      const int f = k0 + (lane >> 4);
      const double av = as[f][wave * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j < n_col) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, static_cast<double>(bs[f][j * 16 + (lane & 15)]), acc[j], 0, 0, 0);
    }
  }
  double *dst = partial + static_cast<size_t>(blockIdx.x) * Q;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int b = C * kSuper + j * 16 + (lane & 15);
    if (j < n_col && b < D) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int a = R * kSuper + wave * 16 + (lane >> 4) + 4 * reg;
        if (a < D && b <= a) dst[static_cast<size_t>(a) * (a + 1) / 2 + b] = acc[j][reg];
      }
    }
  }
}

// Per element: the pass's slices in order.  slice_flag[s] != 0: slice s begins a segment (and is not the call's first
// slice): the running segment sum goes onto the total and starts again from zero.  first_pass: the segment sum starts at
// zero; last_pass: the last segment's sum goes onto the total.
__global__ void __launch_bounds__(256)
LdaReduceKernel(const double *__restrict__ partial, const uint8_t *__restrict__ slice_flag, int n_slices, int size, int first_pass,
                int last_pass, double *__restrict__ seg_sum, double *__restrict__ total) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= size) return;
  double tot = total[e], seg = first_pass ? 0.0 : seg_sum[e];
  for (int s = 0; s < n_slices; s++) {
    if (slice_flag[s]) {
      tot += seg;
      seg = 0.0;
    }
    seg += partial[static_cast<size_t>(s) * size + e];
  }
  if (last_pass) tot += seg;
  else seg_sum[e] = seg;
  total[e] = tot;
}

// One wave per (class, 64 columns), a lane per column.  sorted_*: the items by class, entry order within a class.
// sorted_flag bit 0: a chunk begins here; bit 1: a segment's run begins here (never set on a class's first item).
__global__ void __launch_bounds__(64 * kFirstWaves)
LdaFirstKernel(const float *__restrict__ feats, int feat_stride, int D, int num_classes, const int32_t *__restrict__ class_offsets,
               const int32_t *__restrict__ sorted_row, const float *__restrict__ sorted_w, const uint8_t *__restrict__ sorted_flag,
               double *__restrict__ zero, double *__restrict__ first) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kFirstWaves + static_cast<int>(threadIdx.x >> 6));
  const int d = blockIdx.y * 64 + lane;
  if (c >= num_classes || d >= D) return;
  const int i0 = class_offsets[c], i1 = class_offsets[c + 1];
  if (i0 == i1) return;                  // no item: the buffers keep what they hold
  double tot = first[static_cast<size_t>(c) * D + d], seg = 0.0, part = 0.0;
  double ztot = zero[c], zseg = 0.0, zpart = 0.0;
  for (int i = i0; i < i1; i++) {
    const int flag = sorted_flag[i];
    if (flag & 1) {
      seg += part;
      part = 0.0;
      zseg += zpart;
      zpart = 0.0;
    }
    if (flag & 2) {
      tot += seg;
      seg = 0.0;
      ztot += zseg;
      zseg = 0.0;
    }
    const double w = static_cast<double>(sorted_w[i]);
    part += w * static_cast<double>(feats[static_cast<size_t>(sorted_row[i]) * feat_stride + d]);   // the product is exact
    zpart += w;
  }
  seg += part;
  tot += seg;
  first[static_cast<size_t>(c) * D + d] = tot;
  if (d == 0) {
    zseg += zpart;
    ztot += zseg;
    zero[c] = ztot;
  }
}

}  // namespace

extern "C" {

int kh_lda_acc_stats(const float *feats, int T, int D, int feat_stride, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                     const float *entry_weight, int num_classes, const int64_t *segment_frame_offsets, int num_segments, int add,
                     double *zero, double *first, double *second) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_lda_acc_stats";
  KH_CHECK_ARG(frame_entry_offsets && zero && first && second && T >= 0 && D > 0 && num_classes > 0 && num_segments >= 0);
  KH_CHECK_ARG(segment_frame_offsets || num_segments == 0);
  if (D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  const int64_t *feo = frame_entry_offsets;
  if (feo[0] != 0) {
    SetError("%s: frame_entry_offsets[0] = %lld, not 0", fn, static_cast<long long>(feo[0]));
    return KH_EINVAL;
  }
  for (int t = 0; t < T; t++)
    if (feo[t + 1] < feo[t]) {
      SetError("%s: frame_entry_offsets runs backwards at frame %d", fn, t);
      return KH_EINVAL;
    }
  const int64_t E = feo[T];
  if (E >= (int64_t(1) << 31) - kChunk * 2) {
    SetError("%s: %lld entries, at most 2^31 - 1 - %d", fn, static_cast<long long>(E), kChunk * 2);
    return KH_EINVAL;
  }
  KH_CHECK_ARG(E == 0 || (feats && entry_pdf && entry_weight && feat_stride >= D));
  for (int64_t e = 0; e < E; e++)
    if (entry_pdf[e] < 0 || entry_pdf[e] >= num_classes) {
      SetError("%s: entry %lld names pdf %d, the accumulator has %d classes", fn, static_cast<long long>(e), entry_pdf[e], num_classes);
      return KH_EINVAL;
    }
  // the segments: NULL is one segment of all frames
  const int64_t whole[2] = {0, T};
  const int64_t *so = segment_frame_offsets ? segment_frame_offsets : whole;
  const int S = segment_frame_offsets ? num_segments : 1;
  if (so[0] != 0 || so[S] != T) {
    SetError("%s: segment_frame_offsets runs from %lld to %lld, not from 0 to %d", fn, static_cast<long long>(so[0]),
             static_cast<long long>(so[S]), T);
    return KH_EINVAL;
  }
  for (int s = 0; s < S; s++)
    if (so[s + 1] < so[s]) {
      SetError("%s: segment_frame_offsets runs backwards at segment %d", fn, s);
      return KH_EINVAL;
    }
  const int Q = D * (D + 1) / 2;
  const size_t CD = static_cast<size_t>(num_classes) * D;
  g_ms[1] = g_ms[2] = 0.f;
  g_counts[0] = g_counts[1] = g_counts[2] = g_counts[3] = 0;
  // the items in entry order, with their segments; the slices
  std::vector<int32_t> item_row, item_class, slice_begin, slice_end;
  std::vector<float> item_w;
  std::vector<int32_t> item_seg;
  std::vector<uint8_t> slice_flag;
  for (int s = 0; s < S; s++) {
    const int32_t b = static_cast<int32_t>(item_w.size());
    for (int64_t t = so[s]; t < so[s + 1]; t++)
      for (int64_t e = feo[t]; e < feo[t + 1]; e++)
        if (entry_weight[e] != 0.f) {    // "if (weight != 0.0)": -0.0 is no item, a NaN is one
          item_row.push_back(static_cast<int32_t>(t));
          item_class.push_back(entry_pdf[e]);
          item_w.push_back(entry_weight[e]);
          item_seg.push_back(s);
        }
    const int32_t e = static_cast<int32_t>(item_w.size());
    const int32_t len = static_cast<int32_t>(SliceLen(e - b));
    for (int32_t i = b; i < e; i += len) {
      slice_flag.push_back(i == b && !slice_begin.empty() ? 1 : 0);
      slice_begin.push_back(i);
      slice_end.push_back(e - i < len ? e : i + len);
    }
  }
  const int n = static_cast<int>(item_w.size());
  const int n_slices = static_cast<int>(slice_begin.size());
  if (n == 0) {
    if (!add) {
      std::fill(zero, zero + num_classes, 0.0);
      std::fill(first, first + CD, 0.0);
      std::fill(second, second + Q, 0.0);
    }
    g_ms[1] = g_ms[0] = clk.Ms();
    return KH_OK;
  }
  const size_t limit = g_ws_limit ? g_ws_limit : kDefaultWorkspace;
  const size_t slice_bytes = sizeof(double) * Q;
  if (limit < slice_bytes) {
    SetError("%s: the workspace limit of %zu bytes does not hold one slice's partial sums: %zu bytes needed", fn, limit, slice_bytes);
    return KH_ENOMEM;
  }
  const int per_pass = static_cast<int>(std::min<size_t>(limit / slice_bytes, static_cast<size_t>(n_slices)));
  const int n_passes = DivUp(n_slices, per_pass);
  // the items by class (stable), with the marks of the first-order walk
  std::vector<int32_t> class_offsets(static_cast<size_t>(num_classes) + 1, 0), sorted_row(n);
  std::vector<float> sorted_w(n);
  std::vector<uint8_t> sorted_flag(n);
  {
    for (int i = 0; i < n; i++) class_offsets[item_class[i] + 1]++;
    for (int c = 0; c < num_classes; c++) class_offsets[c + 1] += class_offsets[c];
    std::vector<int32_t> next(class_offsets.begin(), class_offsets.end() - 1), last_seg(num_classes, -1), run_pos(num_classes, 0);
    for (int i = 0; i < n; i++) {
      const int c = item_class[i], at = next[c]++;
      uint8_t flag = 0;
      if (at != class_offsets[c]) {
        if (item_seg[i] != last_seg[c]) {
          flag = 3;
          run_pos[c] = 0;
        } else if (run_pos[c] % kChunk == 0) {
          flag = 1;
        }
      }
      last_seg[c] = item_seg[i];
      run_pos[c]++;
      sorted_row[at] = item_row[i];
      sorted_w[at] = item_w[i];
      sorted_flag[at] = flag;
    }
  }
  const int ST = DivUp(D, kSuper), pairs = ST * (ST + 1) / 2;
  g_ms[1] = clk.Ms();
  Scratch sc;
  const int32_t *d_row = sc.Upload(item_row.data(), n);
  const float *d_w = sc.Upload(item_w.data(), n);
  const int32_t *d_sb = sc.Upload(slice_begin.data(), n_slices);
  const int32_t *d_se = sc.Upload(slice_end.data(), n_slices);
  const uint8_t *d_sf = sc.Upload(slice_flag.data(), n_slices);
  const int32_t *d_coff = sc.Upload(class_offsets.data(), class_offsets.size());
  const int32_t *d_srow = sc.Upload(sorted_row.data(), n);
  const float *d_sw = sc.Upload(sorted_w.data(), n);
  const uint8_t *d_sflag = sc.Upload(sorted_flag.data(), n);
  double *d_partial = sc.Get<double>(static_cast<size_t>(per_pass) * Q);
  double *d_seg = sc.Get<double>(Q);
  double *d_second = add ? sc.Upload(second, Q) : sc.Get<double>(Q);
  double *d_first = add ? sc.Upload(first, CD) : sc.Get<double>(CD);
  double *d_zero = add ? sc.Upload(zero, num_classes) : sc.Get<double>(num_classes);
  if (!d_row || !d_w || !d_sb || !d_se || !d_sf || !d_coff || !d_srow || !d_sw || !d_sflag || !d_partial || !d_seg || !d_second ||
      !d_first || !d_zero) {
    SetError("%s: out of device memory (%d items, %d slices, %d per pass)", fn, n, n_slices, per_pass);
    return KH_ENOMEM;
  }
  if (!add) {
    KH_HIP(hipMemsetAsync(d_second, 0, sizeof(double) * Q, Stream()));
    KH_HIP(hipMemsetAsync(d_first, 0, sizeof(double) * CD, Stream()));
    KH_HIP(hipMemsetAsync(d_zero, 0, sizeof(double) * num_classes, Stream()));
  }
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  ev.Begin();
  for (int p = 0; p < n_passes; p++) {
    const int s0 = p * per_pass, ns = std::min(per_pass, n_slices - s0);
    hipLaunchKernelGGL(LdaAccumulateKernel, dim3(ns, pairs), dim3(64 * kWaves), 0, Stream(), feats, feat_stride, D, d_row, d_w,
                       d_sb + s0, d_se + s0, d_partial);
    hipLaunchKernelGGL(LdaReduceKernel, dim3(DivUp(Q, 256)), dim3(256), 0, Stream(), d_partial, d_sf + s0, ns, Q, p == 0 ? 1 : 0,
                       p == n_passes - 1 ? 1 : 0, d_seg, d_second);
  }
  hipLaunchKernelGGL(LdaFirstKernel, dim3(DivUp(num_classes, kFirstWaves), DivUp(D, 64)), dim3(64 * kFirstWaves), 0, Stream(), feats,
                     feat_stride, D, num_classes, d_coff, d_srow, d_sw, d_sflag, d_zero, d_first);
  ev.End();
  float ms = 0.f;
  hipError_t e = ev.Collect(second, d_second, Q, &ms);
  if (e == hipSuccess) e = hipMemcpyAsync(first, d_first, sizeof(double) * CD, hipMemcpyDeviceToHost, Stream());
  if (e == hipSuccess) e = hipMemcpyAsync(zero, d_zero, sizeof(double) * num_classes, hipMemcpyDeviceToHost, Stream());
  if (e == hipSuccess) e = hipStreamSynchronize(Stream());
  if (e != hipSuccess) {
    SetError("%s: %s", fn, hipGetErrorString(e));
    return KH_EDEVICE;
  }
  g_ms[2] = ms;
  g_counts[0] = n;
  g_counts[1] = n_slices;
  g_counts[2] = static_cast<int32_t>(std::min<int64_t>(static_cast<int64_t>(n_slices) * pairs, INT32_MAX));
  g_counts[3] = n_passes;
  g_ms[0] = clk.Ms();
  return KH_OK;
}

int kh_lda_set_workspace_limit(size_t bytes) {
  g_ws_limit = bytes;
  return KH_OK;
}
int kh_lda_chunk(void) { return kChunk; }
int kh_lda_max_slices(void) { return kMaxSlices; }
int kh_lda_max_dim(void) { return kMaxD; }

int kh_lda_last_timings(float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms && counts);
  for (int i = 0; i < 3; i++) ms[i] = g_ms[i];
  for (int i = 0; i < 4; i++) counts[i] = g_counts[i];
  return KH_OK;
}

}  // extern "C"
