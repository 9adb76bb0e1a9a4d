// kh_mllt.hip - the MLLT (global semi-tied covariance) statistics of a batch of frames (gmm-acc-mllt).
//
// Replaces MlltAccs::AccumulateFromPosteriors (transform/mllt.cc:131-160) under AccumulateFromGmm (:162-170), for given
// Gaussian posteriors that RandPrune (base/kaldi-math.h:169-175) has already been applied to (kh_rand_prune below).  Per
// (entry, Gaussian) item i with a nonzero posterior p, the reference forms, in float,
//     mean[d] = means_invvars[g, d] / inv_vars[g, d],   o[d] = mean[d] - x[d],   w[j] = inv_vars[g, j] * p
// and adds, in double,  G_j[a, b] += w[j] * (o[a] * o[b])  for every j and every packed pair a >= b.
//
// Over a call this is one GEMM  Gout [D x Q] = W^T (D x n) times T (n x Q),  Q = D (D + 1) / 2 packed as SpMatrix does
// ((r, c), r >= c, at r (r + 1) / 2 + c),  W[i, j] = w_i[j],  T[i, q] = o_i[a(q)] o_i[b(q)].  Neither W nor T is stored: a
// workgroup stages kSub items at a time in LDS - each item's o row and w row, computed while staging - and a lane makes its
// T element from two floats of the o image, widened to double; the product of two widened floats is exact.
// The division is plain `/`: HIP compiles float division correctly rounded unless -fno-hip-fp32-correctly-rounded-divide-sqrt
// is given, and the library's flags (build.py: -fno-fast-math, -ffp-contract=off) do not give it; fp32 denormals are kept
// on gfx9.  tests/test_gpu_mllt.py holds the result to a bound that a 1-ulp o or w breaks by orders of magnitude.
// v_mfma_f64_16x16x4_f64: A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15], one double per lane; C/D col = lane & 15,
// row = (lane >> 4) + 4 * reg (the operand layout of FmllrAccumulateKernel, stage B of kh_fmllr.hip's header, and GmmAccumulateKernel).
//
// The host makes the item list - (row, Gaussian, posterior) with a nonzero posterior, in entry order then Gaussian order -
// and cuts it into slices of  slice_len = kChunk * max(1, ceil(n / (kChunk * kMaxSlices)))  items: a function of n and the
// two constants only, so equal inputs give equal bits and nothing a caller sets changes a sum.  A workgroup is one (slice,
// group of 16 column tiles of Q): its 4 waves own the column tiles w, w + 4, w + 8, w + 12 of the group, whose (a, b) are
// fixed for the launch and live in registers, and ALL ceil(D / 16) row tiles: the B fragment (two LDS reads, two
// conversions, one multiply) is shared by the row tiles.  The kernel is a template on the number of row tiles RT = 1 ... 4:
// a wave's accumulators are 4 column tiles x RT row tiles x 4 doubles = 32 RT VGPRs (128 at D = 64; 96 at D = 40).
// Every slice writes its partial [D x Q] to a workspace (at most kMaxSlices D Q doubles: 273 MB at D = 64, 67 MB at D = 40);
// a second kernel adds the slices in slice order.  No sum is shared between workgroups.
// Supported D: 1 ... 64 (the LDS images and the 8-bit (a, b) fields); KH_EINVAL above.
// Static LDS of MlltAccumulateKernel: the o image kSub x kOs floats and the w image kSub x kWs floats:
// 32 x 65 x 4 + 32 x 80 x 4 = 18560 bytes.  kOs = 65 is odd: the four items of a fragment fall on different banks for equal
// columns.  kWs = 80 = 16 mod 64: the four items of an A fragment, 16 consecutive columns each, fall on four disjoint runs
// of 16 banks.
//
// kh_rand_prune is RandPrune on a host array with the C library's rand() under a mutex, as the reference's Rand()
// (base/kaldi-math.cc:45-63) takes it.  kh_rand_prune_at first puts the generator where a job's draws stand - srand(seed),
// then `skip` draws discarded: a process that uses the GPU does not own the generator's state (the HIP runtime reseeds it
// when it initialises and draws from it at some first uses; seen on an MI355X), so a caller that wants the reference's
// sequence positions it at every call.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmacc_plan.h"
#include "kh_gmmstats.h"

using namespace kh;

namespace {

thread_local float g_ms[3] = {0.f, 0.f, 0.f};   // whole call; host plan (checks, download of the posteriors, item list); kernels (events)
thread_local int32_t g_counts[3] = {0, 0, 0};   // items; slices; workgroups of the accumulate kernel
std::mutex g_rand_mutex;

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kChunk = 256;          // items per slice, times a whole number (tests/mllt_cases.py restates the rule)
constexpr int kMaxSlices = 256;      // the workspace holds at most this many partial [D x Q]
constexpr int kSub = 32;             // items staged in LDS at a time
constexpr int kWaves = 4;
constexpr int kTilesPerWave = 4;     // 16-column tiles per wave
constexpr int kGroupTiles = kWaves * kTilesPerWave;   // column tiles of a workgroup
constexpr int kOs = 65;              // row pitch of the o image
constexpr int kWs = 80;              // row pitch of the w image
constexpr int kMaxD = 64;
constexpr int kMaxRT = kMaxD / 16;
static_assert(kChunk % kSub == 0 && kSub % 4 == 0, "chunking");
static_assert(kMaxD <= 64 && kMaxD < kOs && kMaxD <= kWs && kMaxD <= 256, "images");

inline int64_t SliceLen(int64_t n) { return kChunk * std::max<int64_t>(1, DivUp64(n, static_cast<int64_t>(kChunk) * kMaxSlices)); }

template <int RT>
__global__ void __launch_bounds__(64 * kWaves)
MlltAccumulateKernel(const float *__restrict__ feats, int feat_stride, int D, const float *__restrict__ mi,
                     const float *__restrict__ iv, const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_gauss,
                     const float *__restrict__ item_p, int n, int slice_len, double *__restrict__ partial) {
  __shared__ float os[kSub][kOs];
  __shared__ float ws[kSub][kWs];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Q = D * (D + 1) / 2, CT = (Q + 15) >> 4;
  const int i_begin = blockIdx.x * slice_len;                              // < n < 2^31
  const int i_end = n - i_begin < slice_len ? n : i_begin + slice_len;
  // this lane's column of each tile as (a, b) of o
  int ab[kTilesPerWave];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    const int v = (blockIdx.y * kGroupTiles + wave + kWaves * j) * 16 + (lane & 15);
    int a = 0, b = 0;
    if (v < Q) {
      a = static_cast<int>((sqrtf(8.f * static_cast<float>(v) + 1.f) - 1.f) * 0.5f);
      while (a * (a + 1) / 2 > v) a--;
      while ((a + 1) * (a + 2) / 2 <= v) a++;
      b = v - a * (a + 1) / 2;
    }
    ab[j] = a | (b << 8);
  }
  f64x4 acc[kTilesPerWave][RT];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[j][r] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int s0 = i_begin; s0 < i_end; s0 += kSub) {
    __syncthreads();   // the previous step's fragments have been read
    for (int i = t; i < kSub * 64; i += 64 * kWaves) {
      const int f = i >> 6, d = i & 63, it = s0 + f;
      float o = 0.f, w = 0.f;            // past the slice or past D: zeros
      if (it < i_end && d < D) {
        const size_t g = static_cast<size_t>(item_gauss[it]) * D + d;
        const float inv_var = iv[g];
        const float mean = mi[g] / inv_var;                                           // mean.AddVecDivVec(1.0, mean_invvar, inv_var, 0.0)
        o = mean - feats[static_cast<size_t>(item_row[it]) * feat_stride + d];        // mean.AddVec(-1.0, data)
        w = inv_var * item_p[it];                                                     // inv_var(j) * posterior
      }
      os[f][d] = o;
      ws[f][d] = w;
    }
    __syncthreads();
#pragma unroll 2
    for (int k0 = 0; k0 < kSub; k0 += 4) {
      const int f = k0 + (lane >> 4);
      double av[RT];
#pragma unroll
      for (int r = 0; r < RT; r++) av[r] = static_cast<double>(ws[f][r * 16 + (lane & 15)]);
#pragma unroll
      for (int j = 0; j < kTilesPerWave; j++) {
        if (static_cast<int>(blockIdx.y) * kGroupTiles + wave + kWaves * j < CT) {
          const double bv = static_cast<double>(os[f][ab[j] & 0xff]) * static_cast<double>(os[f][ab[j] >> 8]);
#pragma unroll
          for (int r = 0; r < RT; r++) acc[j][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv, acc[j][r], 0, 0, 0);
        }
      }
    }
  }
  double *dst = partial + static_cast<size_t>(blockIdx.x) * D * Q;
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    const int v = (blockIdx.y * kGroupTiles + wave + kWaves * j) * 16 + (lane & 15);
    if (v < Q) {
#pragma unroll
      for (int r = 0; r < RT; r++) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int row = r * 16 + (lane >> 4) + 4 * reg;
          if (row < D) dst[static_cast<size_t>(row) * Q + v] = acc[j][r][reg];
        }
      }
    }
  }
}

// out[e] = the slices' partial[.][e] added in slice order
__global__ void __launch_bounds__(256)
MlltReduceKernel(const double *__restrict__ partial, int n_slices, int size, double *__restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= size) return;
  double s = 0.0;
  for (int c = 0; c < n_slices; c++) s += partial[static_cast<size_t>(c) * size + e];
  out[e] = s;
}

template <int RT>
void LaunchAccumulate(dim3 grid, const float *feats, int feat_stride, int D, const float *mi, const float *iv, const int32_t *row,
                      const int32_t *gauss, const float *p, int n, int slice_len, double *partial) {
  hipLaunchKernelGGL(MlltAccumulateKernel<RT>, grid, dim3(64 * kWaves), 0, Stream(), feats, feat_stride, D, mi, iv, row, gauss, p, n,
                     slice_len, partial);
}

// RandPrune on post[0 .. n) in order, the caller holding g_rand_mutex; returns the number of draws taken.
int64_t RandPruneLocked(float *post, int64_t n, float thresh) {
  int64_t draws = 0;
  for (int64_t i = 0; i < n; i++) {
    const float p = post[i];
    if (p == 0.0 || std::abs(p) >= thresh) continue;
    const float u = static_cast<float>((rand() + 1.0) / (RAND_MAX + 2.0));             // RandUniform()
    const double q = std::fabs(static_cast<double>(p)) / static_cast<double>(thresh);   // ::fabs(double): see kaldi_hip.h
    post[i] = static_cast<float>((p >= 0 ? 1.0 : -1.0) * (static_cast<double>(u) <= q ? static_cast<double>(thresh) : 0.0));
    draws++;
  }
  return draws;
}

}  // namespace

extern "C" {

int kh_mllt_acc_stats(const float *feats, int T, int D, int feat_stride, const float *means_invvars, const float *inv_vars,
                      const int32_t *pdf_offsets, int num_pdfs, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                      const int64_t *entry_gauss_offsets, const float *gauss_post, double *G) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_mllt_acc_stats";
  KH_CHECK_ARG(pdf_offsets && frame_entry_offsets && G && T >= 0 && D > 0 && num_pdfs > 0);
  if (D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  const int64_t E = frame_entry_offsets[T];
  KH_CHECK_ARG(E <= 0 || (feats && means_invvars && inv_vars && entry_pdf && entry_gauss_offsets && gauss_post && feat_stride >= D));
  std::string err;
  if (!kh_gmmacc::Check(T, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_gauss_offsets, &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  const int Q = D * (D + 1) / 2, size = D * Q;
  std::fill(G, G + size, 0.0);
  g_ms[1] = g_ms[2] = 0.f;
  g_counts[0] = g_counts[1] = g_counts[2] = 0;
  if (E == 0) {
    g_ms[0] = clk.Ms();
    return KH_OK;
  }
  // the items: (row, Gaussian, posterior) with a nonzero posterior, in entry order then Gaussian order
  const int64_t NP = entry_gauss_offsets[E];
  std::vector<float> post(NP);
  if (NP) {
    KH_HIP(hipMemcpyAsync(post.data(), gauss_post, sizeof(float) * NP, hipMemcpyDeviceToHost, Stream()));
    KH_HIP(hipStreamSynchronize(Stream()));
  }
  std::vector<int32_t> item_row, item_gauss;
  std::vector<float> item_p;
  for (int t = 0; t < T; t++)
    for (int64_t e = frame_entry_offsets[t]; e < frame_entry_offsets[t + 1]; e++) {
      const int32_t g0 = pdf_offsets[entry_pdf[e]];
      const float *p = post.data() + entry_gauss_offsets[e];
      const int ng = static_cast<int>(entry_gauss_offsets[e + 1] - entry_gauss_offsets[e]);
      for (int i = 0; i < ng; i++)
        if (p[i] != 0.f) {               // "if (posterior == 0.0) continue;" - a NaN is an item, as there
          item_row.push_back(t);
          item_gauss.push_back(g0 + i);
          item_p.push_back(p[i]);
        }
    }
  const int64_t n64 = static_cast<int64_t>(item_p.size());
  if (n64 >= (int64_t(1) << 31) - kChunk * 2) {
    SetError("%s: %lld items, at most 2^31 - 1 - %d", fn, static_cast<long long>(n64), kChunk * 2);
    return KH_EINVAL;
  }
  const int n = static_cast<int>(n64);
  if (n == 0) {
    g_ms[1] = g_ms[0] = clk.Ms();
    return KH_OK;
  }
  const int slice_len = static_cast<int>(SliceLen(n));
  const int n_slices = DivUp(n, slice_len);
  const int CT = DivUp(Q, 16), GG = DivUp(CT, kGroupTiles), RT = DivUp(D, 16);
  g_ms[1] = clk.Ms();
  Scratch sc;
  const int32_t *d_row = sc.Upload(item_row.data(), n);
  const int32_t *d_gauss = sc.Upload(item_gauss.data(), n);
  const float *d_p = sc.Upload(item_p.data(), n);
  double *d_partial = sc.Get<double>(static_cast<size_t>(n_slices) * size);
  double *d_out = sc.Get<double>(size);
  if (!d_row || !d_gauss || !d_p || !d_partial || !d_out) {
    SetError("%s: out of device memory (%d items, %d slices)", fn, n, n_slices);
    return KH_ENOMEM;
  }
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  ev.Begin();
  const dim3 grid(n_slices, GG);
  switch (RT) {
    case 1: LaunchAccumulate<1>(grid, feats, feat_stride, D, means_invvars, inv_vars, d_row, d_gauss, d_p, n, slice_len, d_partial); break;
    case 2: LaunchAccumulate<2>(grid, feats, feat_stride, D, means_invvars, inv_vars, d_row, d_gauss, d_p, n, slice_len, d_partial); break;
    case 3: LaunchAccumulate<3>(grid, feats, feat_stride, D, means_invvars, inv_vars, d_row, d_gauss, d_p, n, slice_len, d_partial); break;
    default: LaunchAccumulate<kMaxRT>(grid, feats, feat_stride, D, means_invvars, inv_vars, d_row, d_gauss, d_p, n, slice_len, d_partial); break;
  }
  hipLaunchKernelGGL(MlltReduceKernel, dim3(DivUp(size, 256)), dim3(256), 0, Stream(), d_partial, n_slices, size, d_out);
  ev.End();
  float ms = 0.f;
  if (hipError_t e = ev.Collect(G, d_out, size, &ms); e != hipSuccess) {
    SetError("%s: %s", fn, hipGetErrorString(e));
    return KH_EDEVICE;
  }
  g_ms[2] = ms;
  g_counts[0] = n;
  g_counts[1] = n_slices;
  g_counts[2] = n_slices * GG;
  g_ms[0] = clk.Ms();
  return KH_OK;
}

int kh_rand_prune(float *post, int64_t n, float thresh, int reseed, unsigned seed) {
  KH_CHECK_ARG(n >= 0 && (post || n == 0));
  if (!(thresh >= 0.f)) {                // KALDI_ASSERT(prune_thresh >= 0.0)
    SetError("kh_rand_prune: prune threshold %g, must be >= 0", static_cast<double>(thresh));
    return KH_EINVAL;
  }
  std::lock_guard<std::mutex> lock(g_rand_mutex);
  if (reseed) srand(seed);
  RandPruneLocked(post, n, thresh);
  return KH_OK;
}

int kh_rand_prune_at(float *post, int64_t n, float thresh, unsigned seed, int64_t skip, int64_t *draws) {
  KH_CHECK_ARG(n >= 0 && (post || n == 0) && skip >= 0 && draws);
  if (!(thresh >= 0.f)) {
    SetError("kh_rand_prune_at: prune threshold %g, must be >= 0", static_cast<double>(thresh));
    return KH_EINVAL;
  }
  std::lock_guard<std::mutex> lock(g_rand_mutex);
  srand(seed);
  for (int64_t i = 0; i < skip; i++) (void)rand();
  *draws = RandPruneLocked(post, n, thresh);
  return KH_OK;
}

int kh_mllt_chunk(void) { return kChunk; }
int kh_mllt_max_slices(void) { return kMaxSlices; }
int kh_mllt_max_dim(void) { return kMaxD; }

int kh_mllt_last_timings(float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms && counts);
  for (int i = 0; i < 3; i++) ms[i] = g_ms[i];
  for (int i = 0; i < 3; i++) counts[i] = g_counts[i];
  return KH_OK;
}

}  // extern "C"
