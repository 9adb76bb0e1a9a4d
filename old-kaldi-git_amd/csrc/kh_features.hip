// kh_features.hip — feature front-end on gfx950 (the step right
// before the hot path).  Replaces, for a waveform resident on the device:
//   Mfcc::ComputeInternal          feat/feature-mfcc.cc:119-184 (use_energy = false, dither = 0)
//     ExtractWindow / Preemphasize feat/feature-functions.cc:61-70,98-167 (snip_edges = true)
//     SplitRadixRealFft + ComputePowerSpectrum  matrix/srfft.cc, feature-functions.cc:186-207
//     MelBanks::Compute            feat/mel-computations.cc:219-246
//   ComputeDeltas                  feat/feature-functions.cc:244-267,361-372
//   AccCmvnStats                   transform/cmvn.cc:30-62
// The tables of the reference's constructors (window function, mel filter weights, DCT
// rows, lifter) are built by the caller exactly as the reference builds them and passed in.
// One workgroup per frame; the frame, its spectrum and the twiddle table live in LDS.  The
// transform is the DFT itself (each lane owns a frequency bin): 512 x 257 FMAs per frame is
// noise next to the acoustic model, and it needs no bit-reversal / butterfly stages.
#include <cmath>
#include <vector>

#include "kh_common.h"
#include "kh_devbuf.h"

using namespace kh;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPadded = 2048;

__global__ void __launch_bounds__(kThreads)
MfccKernel(const float *__restrict__ wave, int frame_shift, int frame_length, int padded, float preemph,
           int remove_dc, const float *__restrict__ window, const double *__restrict__ cos_t,
           const double *__restrict__ sin_t, int num_bins, const int32_t *__restrict__ mel_first,
           const int32_t *__restrict__ mel_off, const float *__restrict__ mel_w, int num_ceps,
           const float *__restrict__ dct, const float *__restrict__ lifter, float *__restrict__ out,
           int out_stride, int n_samples, KhMfccOptions opt) {
  __shared__ float win[kMaxPadded];
  __shared__ double fr[kMaxPadded], fi[kMaxPadded];   // the transform's work arrays (double: see below)
  __shared__ float power[kMaxPadded / 2 + 1];
  __shared__ float mel[256];
  __shared__ double red[kThreads / 64];
  __shared__ float log_energy_s;
  const int r = blockIdx.x;
  // ExtractWindow: copy (snip_edges: frame r starts at r * shift; else it is centred on
  // shift * (r + 0.5) and the signal extended by reflection, :107-135), dither, remove DC (Sum()
  // accumulates in double), raw log energy, pre-emphasis, window, zero pad
  const int begin = opt.snip_edges ? frame_shift * r : static_cast<int>(frame_shift * (r + 0.5)) - frame_length / 2;
  double part = 0.0;
  for (int i = threadIdx.x; i < padded; i += kThreads) {
    float v = 0.0f;
    if (i < frame_length) {
      int f = begin + i;
      if (f < 0) f = (-f) % n_samples;
      else if (f >= n_samples) f = n_samples - 1 - (f - n_samples) % n_samples;
      v = wave[f];
      if (opt.dither != 0.0f) {
        // Dither :51-54: RandGauss() * dither per sample of every window (independently for
        // overlapping frames, as there); counter-based generator instead of rand()
        uint64_t z = opt.dither_seed + 0x9e3779b97f4a7c15ull * (static_cast<uint64_t>(r) * frame_length + i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        const float u1 = (static_cast<float>(z >> 40) + 1.0f) * (1.0f / 16777216.0f);
        const float u2 = static_cast<float>((z >> 8) & 0xffffff) * (1.0f / 16777216.0f);
        v += sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795864769f * u2) * opt.dither;
      }
    }
    win[i] = v;
    part += v;
  }
  if (remove_dc) {
    part = kh_wave_sum_d(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    double sum = 0.0;
    for (int i = 0; i < kThreads / 64; i++) sum += red[i];
    const float c = -static_cast<float>(sum) / frame_length;
    for (int i = threadIdx.x; i < frame_length; i += kThreads) win[i] += c;
  }
  __syncthreads();
  auto log_energy_of = [&](int n) {   // Log(max(VecVec(w, w), FLT_MIN)) :151-155; float products, double sum
    double e = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) e += static_cast<double>(win[i] * win[i]);
    e = kh_wave_sum_d(e);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
      double sum = 0.0;
      for (int i = 0; i < kThreads / 64; i++) sum += red[i];
      const float ef = static_cast<float>(sum);
      log_energy_s = logf(ef > 1.17549435e-38f ? ef : 1.17549435e-38f);
    }
  };
  if (opt.use_energy && opt.raw_energy) log_energy_of(frame_length);
  // Preemphasize :61-67 reads the ORIGINAL neighbour (the loop runs from the end): two steps
  float pre[kMaxPadded / kThreads];
  int np = 0;
  for (int i = threadIdx.x; i < frame_length; i += kThreads, np++)
    pre[np] = preemph != 0.0f ? win[i] - preemph * win[i > 0 ? i - 1 : 0] : win[i];
  __syncthreads();
  np = 0;
  for (int i = threadIdx.x; i < frame_length; i += kThreads, np++) win[i] = pre[np] * window[i];
  __syncthreads();
  if (opt.use_energy && !opt.raw_energy) log_energy_of(padded);   // feature-mfcc.cc:140-142
  // X_k = sum_n x[n] e^{-2 pi i k n / N}; power spectrum (bins 0 .. N/2).  The transform runs in DOUBLE (radix-2
  // decimation in time in LDS, double twiddles): the reference runs a float split-radix FFT (matrix/srfft.cc) whose
  // rounding no other evaluation order reproduces, so this is the correctly rounded transform - the reference's own
  // cepstra differ from it by <= 8e-5 on the golden waveform (tests/test_feature_oracle.py attributes it), and a
  // float-accumulated DFT (N-term sums, rounds 1-2) was further from both.  As an FFT it also costs 9 butterfly rounds
  // instead of 512 multiply-adds per bin: 360 k frames in 6 ms instead of 17.7.
  int logn = 0;
  while ((1 << logn) < padded) logn++;
  for (int i = threadIdx.x; i < padded; i += kThreads) {
    const int j = static_cast<int>(__brev(static_cast<unsigned>(i)) >> (32 - logn));
    fr[j] = static_cast<double>(win[i]);
    fi[j] = 0.0;
  }
  __syncthreads();
  for (int sgm = 1; sgm <= logn; sgm++) {
    const int m = 1 << sgm, hm = m >> 1, tstep = padded >> sgm;
    for (int b = threadIdx.x; b < (padded >> 1); b += kThreads) {
      const int pos = b & (hm - 1), i0 = ((b >> (sgm - 1)) << sgm) + pos, i1 = i0 + hm;
      const double wr = cos_t[pos * tstep], wi = -sin_t[pos * tstep];       // e^{-2 pi i pos / m}
      const double xr = fr[i1], xi = fi[i1];
      const double tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
      const double ur = fr[i0], ui = fi[i0];
      fr[i0] = ur + tr; fi[i0] = ui + ti;
      fr[i1] = ur - tr; fi[i1] = ui - ti;
    }
    __syncthreads();
  }
  const int half = padded / 2;
  for (int k = threadIdx.x; k <= half; k += kThreads) {
    const float fre = static_cast<float>(fr[k]), fim = static_cast<float>(fi[k]);   // the reference's transform hands back floats
    power[k] = fre * fre + fim * fim;                                              // ComputePowerSpectrum feature-functions.cc:186-207
  }
  __syncthreads();
  // MelBanks::Compute, floor, log
  for (int b = threadIdx.x; b < num_bins; b += kThreads) {
    float e = 0.0f;
    const int f0 = mel_first[b], o0 = mel_off[b], o1 = mel_off[b + 1];
    for (int i = o0; i < o1; i++) e += mel_w[i] * power[f0 + (i - o0)];
    if (e < 1.17549435e-38f) e = 1.17549435e-38f;  // numeric_limits<float>::min()
    mel[b] = static_cast<float>(log(static_cast<double>(e)));   // = the host's correctly rounded logf (the device's logf is 1 ulp off on a
                                                                // part of the arguments, and the DCT + lifter amplify an ulp of log-energy ~30x)
  }
  __syncthreads();
  // this_mfcc = dct_matrix_ * mel_energies; MulElements(lifter_coeffs_)
  for (int c = threadIdx.x; c < num_ceps; c += kThreads) {
    float s = 0.0f;
    for (int b = 0; b < num_bins; b++) s += dct[c * num_bins + b] * mel[b];
    if (lifter != nullptr) s *= lifter[c];
    if (opt.use_energy && c == 0) {   // :167-171
      s = log_energy_s;
      if (opt.energy_floor > 0.0f && s < logf(opt.energy_floor)) s = logf(opt.energy_floor);
    }
    int col = c;
    if (opt.htk_compat) {             // :173-182: energy / C0 * sqrt(2) to the last column
      col = c == 0 ? num_ceps - 1 : c - 1;
      if (c == 0 && !opt.use_energy) s *= 1.41421356237309504880f;
    }
    out[static_cast<size_t>(r) * out_stride + col] = s;
  }
}

// DeltaFeatures::Process :244-267 for every (frame, order, dim): column on the lane
__global__ void DeltasKernel(const float *__restrict__ in, int rows, int cols, int in_stride, int order,
                             const float *__restrict__ scales, const int32_t *__restrict__ lens,
                             float *__restrict__ out, int out_stride) {
  for (int t = blockIdx.y; t < rows; t += gridDim.y)
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols * (order + 1); c += gridDim.x * blockDim.x) {
      const int i = c / cols, d = c - i * cols;
      int pos = 0;
      for (int j = 0; j < i; j++) pos += lens[j];
      const int max_offset = (lens[i] - 1) / 2;
      float acc = 0.0f;
      for (int j = -max_offset; j <= max_offset; j++) {
        int f = t + j;
        f = f < 0 ? 0 : (f >= rows ? rows - 1 : f);
        const float sc = scales[pos + j + max_offset];
        if (sc != 0.0f) acc += sc * in[static_cast<size_t>(f) * in_stride + d];
      }
      out[static_cast<size_t>(t) * out_stride + c] = acc;
    }
}

// AccCmvnStats: per column sum x and sum x*x (float products, double accumulation)
__global__ void __launch_bounds__(kThreads)
CmvnStatsKernel(const float *__restrict__ x, int rows, int cols, int stride, double *__restrict__ stats) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= cols) return;
  double s1 = 0.0, s2 = 0.0;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const float v = x[static_cast<size_t>(r) * stride + d];
    s1 += v;
    s2 += v * v;
  }
  atomicAdd(&stats[d], s1);
  atomicAdd(&stats[cols + 1 + d], s2);
}

}  // namespace

extern "C" {

int kh_mfcc_compute(const float *wave, int n_samples, int frame_shift, int frame_length, int padded,
                    float preemph_coeff, int remove_dc_offset, const float *window_host, int num_bins,
                    const int32_t *mel_first_host, const int32_t *mel_off_host, const float *mel_weights_host,
                    int num_ceps, const float *dct_host, const float *lifter_host, float *out, int out_stride,
                    int *num_frames) {
  KhMfccOptions opt;
  memset(&opt, 0, sizeof(opt));
  opt.snip_edges = 1;
  opt.raw_energy = 1;
  return kh_mfcc_compute_opts(wave, n_samples, frame_shift, frame_length, padded, preemph_coeff, remove_dc_offset, window_host,
                              num_bins, mel_first_host, mel_off_host, mel_weights_host, num_ceps, dct_host, lifter_host, &opt,
                              out, out_stride, num_frames);
}

int kh_mfcc_compute_opts(const float *wave, int n_samples, int frame_shift, int frame_length, int padded,
                         float preemph_coeff, int remove_dc_offset, const float *window_host, int num_bins,
                         const int32_t *mel_first_host, const int32_t *mel_off_host, const float *mel_weights_host,
                         int num_ceps, const float *dct_host, const float *lifter_host, const KhMfccOptions *options,
                         float *out, int out_stride, int *num_frames) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(options && n_samples >= 0 && options->dither >= 0.0f && options->energy_floor >= 0.0f);
  const KhMfccOptions opt = *options;
  KH_CHECK_ARG(wave && window_host && mel_first_host && mel_off_host && mel_weights_host && dct_host && num_frames &&
               frame_shift > 0 && frame_length > 0 && padded >= frame_length && padded <= kMaxPadded &&
               (padded & (padded - 1)) == 0 && num_bins >= 3 && num_bins <= 256 && num_ceps > 0 && num_ceps <= num_bins);
  // NumFrames feature-functions.cc:29-48
  const int rows = opt.snip_edges ? (n_samples < frame_length ? 0 : 1 + (n_samples - frame_length) / frame_shift)
                                  : static_cast<int>(n_samples * 1.0f / frame_shift + 0.5f);
  *num_frames = rows;
  if (rows == 0) return KH_OK;
  KH_CHECK_ARG(out && out_stride >= num_ceps);
  for (int b = 0; b < num_bins; b++)
    KH_CHECK_ARG(mel_first_host[b] >= 0 && mel_off_host[b + 1] >= mel_off_host[b] &&
                 mel_first_host[b] + (mel_off_host[b + 1] - mel_off_host[b]) <= padded / 2 + 1);
  std::vector<double> ct(padded), st_(padded);
  for (int i = 0; i < padded; i++) {
    const double a = 6.283185307179586476925286766559 * i / padded;
    ct[i] = cos(a);
    st_[i] = sin(a);
  }
  hipStream_t st = Stream();
  Dev<float> d_win, d_w, d_dct, d_lift;
  Dev<double> d_ct, d_st;
  Dev<int32_t> d_first, d_off;
  if ((rc = d_win.Upload(window_host, frame_length, st)) || (rc = d_ct.Upload(ct.data(), padded, st)) ||
      (rc = d_st.Upload(st_.data(), padded, st)) || (rc = d_w.Upload(mel_weights_host, mel_off_host[num_bins], st)) ||
      (rc = d_dct.Upload(dct_host, static_cast<size_t>(num_ceps) * num_bins, st)) ||
      (rc = d_first.Upload(mel_first_host, num_bins, st)) || (rc = d_off.Upload(mel_off_host, num_bins + 1, st)))
    return rc;
  if (lifter_host && (rc = d_lift.Upload(lifter_host, num_ceps, st))) return rc;
  hipLaunchKernelGGL(MfccKernel, dim3(rows), dim3(kThreads), 0, st, wave, frame_shift, frame_length, padded,
                     preemph_coeff, remove_dc_offset, d_win.p, d_ct.p, d_st.p, num_bins, d_first.p, d_off.p, d_w.p,
                     num_ceps, d_dct.p, lifter_host ? d_lift.p : nullptr, out, out_stride, n_samples, opt);
  KH_LAUNCH_CHECK();
  KH_HIP(hipStreamSynchronize(st));
  return KH_OK;
}

int kh_compute_deltas(const float *in, KhMatrixDim d_in, int order, const float *scales_host,
                      const int32_t *lens_host, float *out, int out_stride) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(in && out && scales_host && lens_host && order >= 0 && order < 1000 && d_in.rows > 0 && d_in.cols > 0 &&
               d_in.stride >= d_in.cols && out_stride >= d_in.cols * (order + 1));
  size_t n = 0;
  for (int i = 0; i <= order; i++) { KH_CHECK_ARG(lens_host[i] > 0 && (lens_host[i] & 1)); n += lens_host[i]; }
  hipStream_t st = Stream();
  Dev<float> d_sc;
  Dev<int32_t> d_len;
  if ((rc = d_sc.Upload(scales_host, n, st)) || (rc = d_len.Upload(lens_host, order + 1, st))) return rc;
  const int out_cols = d_in.cols * (order + 1);
  hipLaunchKernelGGL(DeltasKernel, dim3((out_cols + 63) / 64, std::min(d_in.rows, NumCUs() * 32)), dim3(64), 0, st, in,
                     d_in.rows, d_in.cols, d_in.stride, order, d_sc.p, d_len.p, out, out_stride);
  KH_LAUNCH_CHECK();
  KH_HIP(hipStreamSynchronize(st));
  return KH_OK;
}

int kh_acc_cmvn_stats(const float *feats, KhMatrixDim d, double *stats_host) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(feats && stats_host && d.rows >= 0 && d.cols > 0 && d.stride >= d.cols);
  if (d.rows == 0) return KH_OK;
  hipStream_t st = Stream();
  const size_t n = 2 * (static_cast<size_t>(d.cols) + 1);
  double *dev = static_cast<double *>(PoolMalloc(sizeof(double) * n));
  if (!dev) return KH_ENOMEM;
  hipError_t e = hipMemsetAsync(dev, 0, sizeof(double) * n, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(CmvnStatsKernel, dim3((d.cols + kThreads - 1) / kThreads, std::min(d.rows, 64)), dim3(kThreads), 0,
                       st, feats, d.rows, d.cols, d.stride, dev);
    e = hipGetLastError();
  }
  std::vector<double> h(n);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  PoolFree(dev);
  if (e != hipSuccess) {
    SetError("kh_acc_cmvn_stats: %s", hipGetErrorString(e));
    return KH_EDEVICE;
  }
  for (int c = 0; c < d.cols; c++) {
    stats_host[c] += h[c];
    stats_host[d.cols + 1 + c] += h[d.cols + 1 + c];
  }
  stats_host[d.cols] += static_cast<double>(d.rows);  // the count (weight 1 per frame)
  return KH_OK;
}

}  // extern "C"
