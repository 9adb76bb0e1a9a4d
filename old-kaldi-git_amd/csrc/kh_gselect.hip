// kh_gselect.hip - Gaussian selection and the posteriors over a selected list, for a batch of stacked frames and ONE DiagGmm
// (gmm-gselect, and the gselect branch of gmm-global-acc-stats up to the accumulation, which is kh_gmm_acc_stats unchanged).
//
// kh_gmm_gselect replaces DiagGmm::GaussianSelection(const MatrixBase&, ...) (gmm/diag-gmm.cc:801-871), its per-frame form
// (:765-799) and GaussianSelectionPreselect (:875-916).
//   Scores.  Without a preselection: kh_diag_gmm_loglikes' values bit for bit - that call, on row chunks into a workspace
//   (kh_gselect_set_workspace_limit bounds a chunk; no result depends on it).  With one: the same k-ordered fmaf chains over the
//   listed Gaussians, ll = (g + a1) + (-0.5f * a2).  This is the library's ONE order for both branches of
//   DiagGmm::LogLikelihoodsPreselect (:566-598): the reference takes BLAS's AddMatVec when the list is a contiguous range and
//   VecVec per Gaussian otherwise, so there a frame's scores depend on how the list happens to be laid out; here they do not.
//   (The reference's test for a contiguous range, :575, looks at the first and the last index only: a list ordered by score
//   with back + 1 - front == size is scored there as the range front ... front + size - 1, whatever it names.  The library
//   scores the Gaussians the list names; tests/gselect_restatement.py restates the reference's behaviour in reference mode.)
//   Selection.  The reference takes nth_element, keeps what is >= thresh, sorts the (score, index) pairs by std::greater and
//   takes the first n: the n largest under the total order (score descending, then index descending).  Scores compare as
//   floats (+0 == -0: the index decides); with a preselection the index of position p is preselect[p].  GselectKernel
//   implements that order directly, one wave per frame: the frame's scores in LDS; each lane keeps the best key of its own
//   column (positions lane, lane + 64, ...); a round is one wave arg-max over the 64 lane bests on the 64-bit key
//   (order-preserving image of the score, index); only the winning lane rescans its column.  n rounds; n <= kMaxN.
//   frame_like.  tot = LogAdd(tot, score_j) over the selected, best first, from -inf: the float LogAdd (base/kaldi-math.h:
//   198-215) with Exp and Log1p as the float of the double function (the convention kh_gmmstats.h states for <true>); every
//   lane carries the same chain.
//   A frame with a NaN score has no order (the reference's nth_element is undefined there): status[t] = 1, no selection
//   (sel_count 0, the row -1), frame_like NaN; the other frames are not touched by it.
//
// kh_gmm_preselect_posteriors replaces gmm-global-acc-stats.cc:117-131 up to the accumulation: per frame whose weight is not
// 0, LogLikelihoodsPreselect (the chains above), VectorBase::ApplySoftMax (matrix/kaldi-vector.cc:840-847) in LIST order,
// Scale(weight).  PreselectPosteriorsKernel, one wave per used frame, is ComponentPosteriorsKernel<true>'s arithmetic
// (kh_gmmstats.h) over a list: float max; e = fl32(exp((double)(f - max))); the float sum of e in list order;
// (e * fl32(1.0 / sum)) * w; like = max + fl32(log((double)sum)).  The posteriors go to one dense row of num_gauss floats per
// used frame (zero-filled by a memset on the stream before the kernel): the layout kh_gmm_acc_stats takes for a one-pdf
// model.  A Gaussian twice in a list is refused (kh_gselect_plan.h): the one deliberate difference from the reference.
//
// Both kernels exist in two sizes, chosen by the longest list (or num_gauss): up to kSmallCap positions with kSmallWaves
// waves per workgroup, up to kMaxGauss with kBigWaves.  Static LDS, the waves' score rows:
// 4 x 512 x 4 = 8192 bytes and 2 x 4096 x 4 = 32768 bytes.
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmstats.h"
#include "kh_gselect_plan.h"

using namespace kh;

namespace {

thread_local float g_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // gselect: whole call, score kernels, selection kernels; posteriors: whole call, kernel
thread_local int32_t g_counts[2] = {0, 0};                // gselect: row chunks; posteriors: used frames
thread_local size_t g_ws_limit = 0;                       // kh_gselect_set_workspace_limit

constexpr int kMaxGauss = 4096;
constexpr int kMaxN = 128;
constexpr int kMaxD = 96;            // kh_diag_gmm_loglikes' limit
constexpr int kSmallCap = 512, kSmallWaves = 4;
constexpr int kBigWaves = 2;
static_assert(kSmallWaves * kSmallCap * 4 == 8192 && kBigWaves * kMaxGauss * 4 == 32768, "the header's LDS figures");

// An unsigned image of a float score with the floats' order; +0 and -0 share one image; NaN: 0, below every score.
__device__ __forceinline__ uint32_t OrderKey(float f) {
  if (f != f) return 0u;
  if (f == 0.f) f = 0.f;
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// DiagGmm::LogLikelihoodsPreselect for one listed Gaussian: GmmLoglikesKernel's chains (kh_gmm.hip)
__device__ __forceinline__ float ScoreOne(const float *__restrict__ x, int D, const float *__restrict__ gconsts,
                                          const float *__restrict__ mi, const float *__restrict__ iv, int idx) {
  const float *mir = mi + static_cast<size_t>(idx) * D;
  const float *ivr = iv + static_cast<size_t>(idx) * D;
  float a1 = 0.f, a2 = 0.f;
  for (int d = 0; d < D; d++) {
    const float v = x[d];
    a1 = fmaf(v, mir[d], a1);
    a2 = fmaf(v * v, ivr[d], a2);   // data_sq.ApplyPow(2.0)
  }
  return (gconsts[idx] + a1) + (-0.5f * a2);
}

// LogAdd(float, float), base/kaldi-math.h:198-215; min_log_diff = kMinLogDiffFloat
__device__ __forceinline__ float LogAddF(float x, float y, float min_log_diff) {
  float diff;
  if (x < y) {
    diff = x - y;
    x = y;
  } else {
    diff = y - x;
  }
  if (diff >= min_log_diff) {
    const float e = static_cast<float>(exp(static_cast<double>(diff)));
    return x + static_cast<float>(log1p(static_cast<double>(e)));
  }
  return x;
}

template <int kO>
__device__ __forceinline__ void MaxStep(uint32_t *hi, uint32_t *lo) {
  const uint32_t ohi = static_cast<uint32_t>(kh_lane_xor_i<kO>(static_cast<int>(*hi)));
  const uint32_t olo = static_cast<uint32_t>(kh_lane_xor_i<kO>(static_cast<int>(*lo)));
  if (ohi > *hi || (ohi == *hi && olo > *lo)) {
    *hi = ohi;
    *lo = olo;
  }
}

// scores: the chunk's rows [t_begin, t_end) x G at pitch score_stride (no preselection), or unused (pre_off / pre_gauss given:
// the frame's list is pre_gauss[pre_off[t] .. pre_off[t + 1]), scored here).  sel [T x n_out], sel_count, frame_like, status:
// whole-call arrays indexed by t.
template <int kCap, int kWaves>
__global__ void __launch_bounds__(64 * kWaves)
GselectKernel(const float *__restrict__ scores, int score_stride, const float *__restrict__ feats, int feat_stride, int D,
              const float *__restrict__ gconsts, const float *__restrict__ mi, const float *__restrict__ iv,
              const int64_t *__restrict__ pre_off, const int32_t *__restrict__ pre_gauss, int t_begin, int t_end, int G, int n,
              int n_out, float min_log_diff, int32_t *__restrict__ sel, int32_t *__restrict__ sel_count,
              float *__restrict__ frame_like, int32_t *__restrict__ status) {
  __shared__ float rows[kWaves][kCap];
  const int lane = threadIdx.x & 63;
  float *sc = rows[threadIdx.x >> 6];
  for (int t0 = t_begin + blockIdx.x * kWaves + (threadIdx.x >> 6); t0 < t_end; t0 += gridDim.x * kWaves) {
    const int t = __builtin_amdgcn_readfirstlane(t0);
    int len = G;
    const int32_t *lst = nullptr;
    if (pre_off) {
      const long long b = pre_off[t];
      len = static_cast<int>(pre_off[t + 1] - b);
      lst = pre_gauss + b;
    }
    if (len > kCap) len = kCap;   // the host has refused it: never past the row
    int32_t *out = sel + static_cast<size_t>(t) * n_out;
    const float *x = feats + static_cast<size_t>(t) * feat_stride;
    const float *srow = scores + static_cast<size_t>(t - t_begin) * score_stride;
    // this lane's column: the scores to LDS, the best key
    uint32_t bu = 0u;
    int bidx = 0, bp = 0;
    float bf = 0.f;
    bool nan = false;
    for (int p = lane; p < len; p += 64) {
      const int idx = lst ? lst[p] : p;
      const float f = lst ? ScoreOne(x, D, gconsts, mi, iv, idx) : srow[p];
      sc[p] = f;
      nan |= f != f;
      const uint32_t u = OrderKey(f);
      if (u > bu || (u == bu && idx >= bidx)) {
        bu = u;
        bidx = idx;
        bp = p;
        bf = f;
      }
    }
    if (__ballot(nan)) {
      for (int r = lane; r < n_out; r += 64) out[r] = -1;
      if (lane == 0) {
        sel_count[t] = 0;
        frame_like[t] = __uint_as_float(0x7fc00000u);
        status[t] = 1;
      }
      continue;
    }
    int count = n < len ? n : len;
    if (count > n_out) count = n_out;   // never past the row of sel
    float tot = -INFINITY;
    int mine = -1;
    for (int r = 0; r < count; r++) {
      uint32_t hi = bu, lo = static_cast<uint32_t>(bidx);
      MaxStep<32>(&hi, &lo); MaxStep<16>(&hi, &lo); MaxStep<8>(&hi, &lo);
      MaxStep<4>(&hi, &lo); MaxStep<2>(&hi, &lo); MaxStep<1>(&hi, &lo);
      const unsigned long long who = __ballot(bu == hi && static_cast<uint32_t>(bidx) == lo);
      const int w = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(who)) - 1);   // the same Gaussian twice: the lower lane
      const float f = ReadLaneF(bf, w);
      tot = LogAddF(tot, f, min_log_diff);
      if (lane == (r & 63)) mine = static_cast<int>(lo);
      if ((r & 63) == 63 || r == count - 1) {
        const int r0 = r & ~63;
        if (r0 + lane <= r) out[r0 + lane] = mine;
      }
      if (lane == w) {   // taken: NaN in the row (no score of a frame that gets here is one); the column's next best
        sc[bp] = __uint_as_float(0x7fc00000u);
        bu = 0u;
        bidx = 0;
        bp = 0;
        bf = 0.f;
        for (int p = lane; p < len; p += 64) {
          const float g = sc[p];
          const uint32_t u = OrderKey(g);
          if (u == 0u) continue;
          const int idx = lst ? lst[p] : p;
          if (u > bu || (u == bu && idx >= bidx)) {
            bu = u;
            bidx = idx;
            bp = p;
            bf = g;
          }
        }
      }
    }
    for (int r = count + lane; r < n_out; r += 64) out[r] = -1;
    if (lane == 0) {
      sel_count[t] = count;
      frame_like[t] = tot;
      status[t] = 0;
    }
  }
}

// used [n_used]: the frames whose weight is not 0; used_weight [n_used]; post [n_used x G], zero on entry.
template <int kCap, int kWaves>
__global__ void __launch_bounds__(64 * kWaves)
PreselectPosteriorsKernel(const float *__restrict__ feats, int feat_stride, int D, const float *__restrict__ gconsts,
                          const float *__restrict__ mi, const float *__restrict__ iv, const int64_t *__restrict__ sel_off,
                          const int32_t *__restrict__ sel_gauss, const int32_t *__restrict__ used,
                          const float *__restrict__ used_weight, int n_used, int G, float *__restrict__ post,
                          float *__restrict__ frame_like) {
  __shared__ float rows[kWaves][kCap];
  const int lane = threadIdx.x & 63;
  float *sc = rows[threadIdx.x >> 6];
  for (int i0 = blockIdx.x * kWaves + (threadIdx.x >> 6); i0 < n_used; i0 += gridDim.x * kWaves) {
    const int i = __builtin_amdgcn_readfirstlane(i0);
    const int t = __builtin_amdgcn_readfirstlane(used[i]);
    const long long b = sel_off[t];
    int len = static_cast<int>(sel_off[t + 1] - b);
    if (len > kCap) len = kCap;   // the host has refused it
    const int32_t *lst = sel_gauss + b;
    const float *x = feats + static_cast<size_t>(t) * feat_stride;
    float mx = -INFINITY;
    for (int p = lane; p < len; p += 64) {
      const float f = ScoreOne(x, D, gconsts, mi, iv, lst[p]);
      sc[p] = f;
      mx = fmaxf(mx, f);
    }
    mx = kh_wave_max(mx);
    float sum = 0.f;   // the same value in every lane
    for (int p0 = 0; p0 < len; p0 += 64) {
      const int p = p0 + lane;
      float ev = 0.f;
      if (p < len) {
        ev = static_cast<float>(exp(static_cast<double>(sc[p] - mx)));
        sc[p] = ev;
      }
      const int cnt = len - p0 < 64 ? len - p0 : 64;
      for (int j = 0; j < cnt; j++) sum += ReadLaneF(ev, j);   // sum += (data_[i] = Exp(data_[i] - max)), in order
    }
    const float inv = static_cast<float>(1.0 / static_cast<double>(sum));   // this->Scale(1.0 / sum)
    const float w = used_weight[i];
    float *out = post + static_cast<size_t>(i) * G;
    for (int p = lane; p < len; p += 64) out[lst[p]] = (sc[p] * inv) * w;    // loglikes.Scale(weight)
    if (lane == 0) frame_like[t] = mx + static_cast<float>(log(static_cast<double>(sum)));
  }
}

// after ev.End(): the launches' error, the stream drained, *ms += Begin .. End
hipError_t Drain(KernelEvents *ev, float *ms) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(Stream());
  float t = 0.f;
  if (e == hipSuccess && hipEventElapsedTime(&t, ev->ev[0], ev->ev[1]) == hipSuccess) *ms += t;
  return e;
}

int CheckModel(const char *fn, int D, int feat_stride, int num_gauss) {
  if (D < 1 || D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  if (feat_stride < D) {
    SetError("%s: feat_stride %d is less than the feature dimension %d", fn, feat_stride, D);
    return KH_EINVAL;
  }
  if (num_gauss < 1 || num_gauss > kMaxGauss) {
    SetError("%s: %d Gaussians, supported 1 ... %d", fn, num_gauss, kMaxGauss);
    return KH_EINVAL;
  }
  return KH_OK;
}

int LongestList(int T, const int64_t *off, const float *frame_weight) {
  int64_t m = 0;
  for (int t = 0; t < T; t++)
    if (kh_gselect::Used(frame_weight, t)) m = std::max(m, off[t + 1] - off[t]);
  return static_cast<int>(m);
}

}  // namespace

extern "C" {

int kh_gmm_gselect(const float *feats, int T, int D, int feat_stride, const float *gconsts, const float *means_invvars,
                   const float *inv_vars, int num_gauss, int num_gselect, const int64_t *pre_offsets, const int32_t *pre_gauss,
                   int32_t *sel, int32_t *sel_count, float *frame_like, int32_t *status) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_gmm_gselect";
  KH_CHECK_ARG(T >= 0 && gconsts && means_invvars && inv_vars);
  KH_CHECK_ARG(T == 0 || (feats && sel && sel_count && frame_like && status));
  KH_CHECK_ARG(!pre_gauss || pre_offsets);
  if ((rc = CheckModel(fn, D, feat_stride, num_gauss))) return rc;
  if (num_gselect < 1 || num_gselect > kMaxN) {
    SetError("%s: num_gselect %d, supported 1 ... %d", fn, num_gselect, kMaxN);
    return KH_EINVAL;
  }
  if (pre_offsets) {
    std::string err;
    KH_CHECK_ARG(pre_gauss || pre_offsets[T] == 0 || T == 0);
    if (!kh_gselect::CheckLists(T, pre_offsets, pre_gauss, num_gauss, num_gauss, nullptr, false, "pre_offsets", &err)) {
      SetError("%s: %s", fn, err.c_str());
      return KH_EINVAL;
    }
  }
  g_ms[0] = g_ms[1] = g_ms[2] = 0.f;
  g_counts[0] = 0;
  if (T == 0) return KH_OK;
  const int n_out = std::min(num_gselect, num_gauss);
  const float min_log_diff = logf(FLT_EPSILON);   // kMinLogDiffFloat, base/kaldi-math.h:121
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  Scratch sc;
  auto launch = [&](const float *scores, const int64_t *d_off, const int32_t *d_gauss, int t0, int t1, int cap) {
    const int waves = cap <= kSmallCap ? kSmallWaves : kBigWaves;
    const unsigned blocks = static_cast<unsigned>(std::min<int64_t>(DivUp(t1 - t0, waves), static_cast<int64_t>(NumCUs()) * 16));
    if (cap <= kSmallCap)
      hipLaunchKernelGGL((GselectKernel<kSmallCap, kSmallWaves>), dim3(blocks), dim3(64 * kSmallWaves), 0, Stream(), scores, num_gauss,
                         feats, feat_stride, D, gconsts, means_invvars, inv_vars, d_off, d_gauss, t0, t1, num_gauss, num_gselect,
                         n_out, min_log_diff, sel, sel_count, frame_like, status);
    else
      hipLaunchKernelGGL((GselectKernel<kMaxGauss, kBigWaves>), dim3(blocks), dim3(64 * kBigWaves), 0, Stream(), scores, num_gauss,
                         feats, feat_stride, D, gconsts, means_invvars, inv_vars, d_off, d_gauss, t0, t1, num_gauss, num_gselect,
                         n_out, min_log_diff, sel, sel_count, frame_like, status);
  };
  if (pre_offsets) {
    const int64_t *d_off = sc.Upload(pre_offsets, static_cast<size_t>(T) + 1);
    const int32_t *d_gauss = sc.Upload(pre_gauss, static_cast<size_t>(pre_offsets[T]));
    if (!d_off || !d_gauss) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
    ev.Begin();
    launch(nullptr, d_off, d_gauss, 0, T, LongestList(T, pre_offsets, nullptr));
    ev.End();
    if (hipError_t e = Drain(&ev, &g_ms[2]); e != hipSuccess) {
      SetError("%s: %s", fn, hipGetErrorString(e));
      return KH_EDEVICE;
    }
    g_counts[0] = 1;
  } else {
    const int rows = kh_gselect::ChunkRows(T, num_gauss, g_ws_limit ? g_ws_limit : (size_t(1) << 28));
    float *ws = sc.Get<float>(static_cast<size_t>(rows) * num_gauss);
    if (!ws) { SetError("%s: out of device memory (%d rows x %d scores)", fn, rows, num_gauss); return KH_ENOMEM; }
    for (int t0 = 0; t0 < T; t0 += rows) {
      const int t1 = std::min(T, t0 + rows);
      ev.Begin();
      rc = kh_diag_gmm_loglikes(feats + static_cast<size_t>(t0) * feat_stride, KhMatrixDim{t1 - t0, D, feat_stride}, gconsts,
                                means_invvars, inv_vars, num_gauss, ws, num_gauss);
      if (rc) return rc;
      ev.End();
      hipError_t e = Drain(&ev, &g_ms[1]);
      if (e == hipSuccess) {
        ev.Begin();
        launch(ws, nullptr, nullptr, t0, t1, num_gauss);
        ev.End();
        e = Drain(&ev, &g_ms[2]);
      }
      if (e != hipSuccess) {
        SetError("%s: %s", fn, hipGetErrorString(e));
        return KH_EDEVICE;
      }
      g_counts[0]++;
    }
  }
  g_ms[0] = clk.Ms();
  return KH_OK;
}

int kh_gmm_preselect_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts, const float *means_invvars,
                                const float *inv_vars, int num_gauss, const int64_t *sel_offsets, const int32_t *sel_gauss,
                                const float *frame_weight, float *post, float *frame_like) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_gmm_preselect_posteriors";
  KH_CHECK_ARG(T >= 0 && gconsts && means_invvars && inv_vars && sel_offsets);
  KH_CHECK_ARG(T == 0 || (feats && frame_like));
  if ((rc = CheckModel(fn, D, feat_stride, num_gauss))) return rc;
  KH_CHECK_ARG(sel_gauss || T == 0 || sel_offsets[T] == 0);
  std::string err;
  if (!kh_gselect::CheckLists(T, sel_offsets, sel_gauss, num_gauss, num_gauss, frame_weight, true, "sel_offsets", &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  g_ms[3] = g_ms[4] = 0.f;
  g_counts[1] = 0;
  if (T == 0) return KH_OK;
  const std::vector<int32_t> used = kh_gselect::UsedFrames(T, frame_weight);
  const int n_used = static_cast<int>(used.size());
  KH_HIP(hipMemsetAsync(frame_like, 0, sizeof(float) * static_cast<size_t>(T), Stream()));
  if (n_used == 0) {
    KH_HIP(hipStreamSynchronize(Stream()));
    g_ms[3] = clk.Ms();
    return KH_OK;
  }
  KH_CHECK_ARG(post);
  std::vector<float> used_weight(n_used);
  for (int i = 0; i < n_used; i++) used_weight[i] = frame_weight ? frame_weight[used[i]] : 1.0f;
  Scratch sc;
  const int64_t *d_off = sc.Upload(sel_offsets, static_cast<size_t>(T) + 1);
  const int32_t *d_gauss = sc.Upload(sel_gauss, static_cast<size_t>(sel_offsets[T]));
  const int32_t *d_used = sc.Upload(used.data(), used.size());
  const float *d_w = sc.Upload(used_weight.data(), used_weight.size());
  if (!d_off || !d_gauss || !d_used || !d_w) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
  KH_HIP(hipMemsetAsync(post, 0, sizeof(float) * static_cast<size_t>(n_used) * num_gauss, Stream()));
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  const int cap = LongestList(T, sel_offsets, frame_weight);
  const int waves = cap <= kSmallCap ? kSmallWaves : kBigWaves;
  const unsigned blocks = static_cast<unsigned>(std::min<int64_t>(DivUp(n_used, waves), static_cast<int64_t>(NumCUs()) * 16));
  ev.Begin();
  if (cap <= kSmallCap)
    hipLaunchKernelGGL((PreselectPosteriorsKernel<kSmallCap, kSmallWaves>), dim3(blocks), dim3(64 * kSmallWaves), 0, Stream(), feats,
                       feat_stride, D, gconsts, means_invvars, inv_vars, d_off, d_gauss, d_used, d_w, n_used, num_gauss, post,
                       frame_like);
  else
    hipLaunchKernelGGL((PreselectPosteriorsKernel<kMaxGauss, kBigWaves>), dim3(blocks), dim3(64 * kBigWaves), 0, Stream(), feats,
                       feat_stride, D, gconsts, means_invvars, inv_vars, d_off, d_gauss, d_used, d_w, n_used, num_gauss, post,
                       frame_like);
  ev.End();
  if (hipError_t e = Drain(&ev, &g_ms[4]); e != hipSuccess) {
    SetError("%s: %s", fn, hipGetErrorString(e));
    return KH_EDEVICE;
  }
  g_counts[1] = n_used;
  g_ms[3] = clk.Ms();
  return KH_OK;
}

int kh_gselect_set_workspace_limit(size_t bytes) {
  g_ws_limit = bytes;
  return KH_OK;
}
int kh_gselect_max_gauss(void) { return kMaxGauss; }
int kh_gselect_max_n(void) { return kMaxN; }
int kh_gselect_max_dim(void) { return kMaxD; }
int kh_gselect_small_lists(void) { return kSmallCap; }

int kh_gselect_last_timings(float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms && counts);
  for (int i = 0; i < 5; i++) ms[i] = g_ms[i];
  for (int i = 0; i < 2; i++) counts[i] = g_counts[i];
  return KH_OK;
}

}  // extern "C"
