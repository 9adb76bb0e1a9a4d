// kh_gmmstats.h — what the GMM statistics routes share (kh_fmllr, kh_gmmacc, kh_mllt): the call clock, the device buffers
// of one call, the two events behind a "kernels" timing slot, and the component posteriors - one kernel in two
// instantiations and one host body behind the two entry points.  The entry-list check they share is kh_gmmacc::Check
// (kh_gmmacc_plan.h, plain C++, tested on the CPU).  Small functions, no framework: a new statistics route starts from these.
//
// ComponentPosteriorsKernel<kDoubleExpLog>, one wave per (frame, pdf) entry.  The per-Gaussian scores are kh_gmm.hip's
// k-ordered fmaf chains (ll = (g + a1) + (-0.5f * a2)), bit-identical to GmmLoglikesKernel.  Then in float: max;
// e = EXP(fl32(f - max)); the sum of e in Gaussian order; posterior = (e * fl32(1.0 / sum)) * weight; like = max + LOG(sum).
// Neither EXP / LOG is kh_gmm.hip's ExpTerm / LogOfSum: ApplySoftMax has no cutoff, so the exp2 form's argument rounding
// |f - max| * 2^-24 is not bounded, and the transcendental share of this kernel is one EXP per D fmaf pairs.
//   <false>  kh_gmm_component_posteriors (fMLLR's stage A1): EXP and LOG are libm's expf / logf (the device library's, 1 ulp
//            in float each).
//   <true>   kh_gmm_acc_component_posteriors (the gmm-acc-stats* routes): EXP and LOG are the float of the double function
//            (the device library's double exp / log, under 1 ulp in double, rounded to float) - which is how
//            DiagGmm::ComponentPosteriors' line-by-line restatement states them.  The statistics are written to a file as
//            floats and read by gmm-est: with 1-ulp posteriors a mean accumulator whose addends cancel moved by several float
//            ulps against the restatement; with these it does not.
#ifndef KH_GMMSTATS_H_
#define KH_GMMSTATS_H_

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmacc_plan.h"

#pragma GCC visibility push(hidden)   // helpers of the including file, not exports of the library
namespace kh {

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  float Ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Device buffers of one call, returned to the pool on every exit.  Not Dev<T> (kh_devbuf.h): a Scratch holds many buffers
// of any type, reports a failed allocation or upload as a null pointer (the caller tests them together and names what it
// asked for), and synchronises the stream before it frees, so a kernel still running never sees its buffers reused.
struct Scratch {
  std::vector<void *> ptrs;
  template <typename T> T *Get(size_t n) {
    void *p = PoolMalloc(sizeof(T) * std::max<size_t>(n, 1));
    if (p) ptrs.push_back(p);
    return static_cast<T *>(p);
  }
  template <typename T> T *Upload(const T *host, size_t n) {
    T *p = Get<T>(n);
    if (p && n && hipMemcpyAsync(p, host, sizeof(T) * n, hipMemcpyHostToDevice, Stream()) != hipSuccess) return nullptr;
    return p;
  }
  ~Scratch() {
    (void)hipStreamSynchronize(Stream());
    for (void *p : ptrs) PoolFree(p);
  }
};

// The two events around a call's kernels on the library stream.  Every operation hands back the HIP error; the caller
// makes its own SetError text and return code of it (a failed Init: kEventsFailed with the entry point's name and the error).
constexpr const char *kEventsFailed = "%s: hipEventCreate failed: %s";
struct KernelEvents {
  hipEvent_t ev[2] = {nullptr, nullptr};
  KernelEvents() = default;
  KernelEvents(const KernelEvents &) = delete;
  KernelEvents &operator=(const KernelEvents &) = delete;
  ~KernelEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t Init() {
    const hipError_t e = hipEventCreate(&ev[0]);
    return e != hipSuccess ? e : hipEventCreate(&ev[1]);
  }
  void Begin() { (void)hipEventRecord(ev[0], Stream()); }
  void End() { (void)hipEventRecord(ev[1], Stream()); }
  // After End(): the launches' error, dev[0 .. n) to host, the stream drained; then *ms += Begin .. End.
  template <typename T> hipError_t Collect(T *host, const T *dev, size_t n, float *ms) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, Stream());
    if (e == hipSuccess) e = hipStreamSynchronize(Stream());
    float t = 0.f;
    if (e == hipSuccess && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) *ms += t;
    return e;
  }
};

constexpr int kPostWaves = 4;

__device__ __forceinline__ float ReadLaneF(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// The arithmetic: the head of this file.  post is read back only by the lane that wrote the element.
template <bool kDoubleExpLog>
__global__ void __launch_bounds__(64 * kPostWaves)
ComponentPosteriorsKernel(const float *__restrict__ feats, int feat_stride, int D, const float *__restrict__ gconsts,
                          const float *__restrict__ mi, const float *__restrict__ iv, const int32_t *__restrict__ pdf_offsets,
                          const int32_t *__restrict__ entry_row, const int32_t *__restrict__ entry_pdf,
                          const float *__restrict__ entry_weight, const int64_t *__restrict__ entry_goff, long long E,
                          float *post, float *__restrict__ like) {
  const int lane = threadIdx.x & 63;
  for (long long e0 = static_cast<long long>(blockIdx.x) * kPostWaves + (threadIdx.x >> 6); e0 < E;
       e0 += static_cast<long long>(gridDim.x) * kPostWaves) {
    const int ei = __builtin_amdgcn_readfirstlane(static_cast<int>(e0));   // E < 2^31, checked by the host
    const int row = __builtin_amdgcn_readfirstlane(entry_row[ei]);
    const int pdf = __builtin_amdgcn_readfirstlane(entry_pdf[ei]);
    const int m0 = __builtin_amdgcn_readfirstlane(pdf_offsets[pdf]);
    const int n = __builtin_amdgcn_readfirstlane(pdf_offsets[pdf + 1]) - m0;
    const float *x = feats + static_cast<size_t>(row) * feat_stride;
    float *out = post + entry_goff[ei];
    float mx = -INFINITY;
    for (int g = lane; g < n; g += 64) {
      const float *mir = mi + static_cast<size_t>(m0 + g) * D;
      const float *ivr = iv + static_cast<size_t>(m0 + g) * D;
      float a1 = 0.f, a2 = 0.f;
      for (int d = 0; d < D; d++) {
        const float v = x[d];
        a1 = fmaf(v, mir[d], a1);
        a2 = fmaf(v * v, ivr[d], a2);   // data_sq.ApplyPow(2.0)
      }
      const float ll = (gconsts[m0 + g] + a1) + (-0.5f * a2);
      out[g] = ll;
      mx = fmaxf(mx, ll);
    }
    mx = kh_wave_max(mx);
    float sum = 0.f;   // the same value in every lane
    for (int g0 = 0; g0 < n; g0 += 64) {
      const int g = g0 + lane;
      float ev = 0.f;
      if (g < n) {
        if constexpr (kDoubleExpLog) ev = static_cast<float>(exp(static_cast<double>(out[g] - mx)));
        else ev = expf(out[g] - mx);
        out[g] = ev;
      }
      const int cnt = n - g0 < 64 ? n - g0 : 64;
      for (int j = 0; j < cnt; j++) sum += ReadLaneF(ev, j);   // sum += (data_[i] = Exp(data_[i] - max)), in order
    }
    const float inv = static_cast<float>(1.0 / static_cast<double>(sum));   // this->Scale(1.0 / sum)
    const float w = entry_weight[ei];
    for (int g = lane; g < n; g += 64) out[g] = (out[g] * inv) * w;          // posterior.Scale(weight)
    if (lane == 0) {
      if constexpr (kDoubleExpLog) like[ei] = mx + static_cast<float>(log(static_cast<double>(sum)));
      else like[ei] = mx + logf(sum);
    }
  }
}

// The body of kh_gmm_component_posteriors (<false>) and kh_gmm_acc_component_posteriors (<true>); fn names the entry point
// in messages, *call_ms is its slot of the caller's last_timings (0 when there is no entry, the call's time otherwise).
template <bool kDoubleExpLog>
int ComponentPosteriors(const char *fn, float *call_ms, const float *feats, int T, int D, int feat_stride, const float *gconsts,
                        const float *means_invvars, const float *inv_vars, const int32_t *pdf_offsets, int num_pdfs,
                        const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const float *entry_weight,
                        const int64_t *entry_gauss_offsets, float *gauss_post, float *entry_like) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(feats && gconsts && means_invvars && inv_vars && pdf_offsets && frame_entry_offsets && entry_gauss_offsets);
  KH_CHECK_ARG(T > 0 && D > 0 && feat_stride >= D && num_pdfs > 0);
  const int64_t E = frame_entry_offsets[T];
  KH_CHECK_ARG(E <= 0 || (entry_pdf && entry_weight && gauss_post && entry_like));
  std::string err;
  if (!kh_gmmacc::Check(T, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_gauss_offsets, &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  *call_ms = 0.f;
  if (E == 0) return KH_OK;
  std::vector<int32_t> entry_row(E);
  for (int t = 0; t < T; t++)
    for (int64_t e = frame_entry_offsets[t]; e < frame_entry_offsets[t + 1]; e++) entry_row[e] = t;
  Scratch sc;
  const int32_t *d_off = sc.Upload(pdf_offsets, num_pdfs + 1);
  const int32_t *d_row = sc.Upload(entry_row.data(), E);
  const int32_t *d_pdf = sc.Upload(entry_pdf, E);
  const float *d_w = sc.Upload(entry_weight, E);
  const int64_t *d_goff = sc.Upload(entry_gauss_offsets, E + 1);
  if (!d_off || !d_row || !d_pdf || !d_w || !d_goff) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
  const int blocks = static_cast<int>(std::min<int64_t>(DivUp64(E, kPostWaves), static_cast<int64_t>(NumCUs()) * 16));
  hipLaunchKernelGGL(ComponentPosteriorsKernel<kDoubleExpLog>, dim3(blocks), dim3(64 * kPostWaves), 0, Stream(), feats, feat_stride,
                     D, gconsts, means_invvars, inv_vars, d_off, d_row, d_pdf, d_w, d_goff, static_cast<long long>(E), gauss_post,
                     entry_like);
  KH_LAUNCH_CHECK();
  KH_HIP(hipStreamSynchronize(Stream()));   // the uploads' host arrays go out of scope
  *call_ms = clk.Ms();
  return KH_OK;
}

}  // namespace kh
#pragma GCC visibility pop

#endif  // KH_GMMSTATS_H_
