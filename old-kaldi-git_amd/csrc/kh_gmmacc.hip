// kh_gmmacc.hip - the E-step of GMM training for a batch of frames (gmm-acc-stats-ali, gmm-acc-stats, gmm-acc-stats-twofeats).
//
// Replaces AccumDiagGmm::AccumulateFromPosteriors (gmm/mle-diag-gmm.cc:171-189) under AccumulateFromDiag (:191-204) under
// AccumAmDiagGmm::AccumulateForGmm / AccumulateForGmmTwofeats (gmm/mle-am-diag-gmm.cc:69-97), for given Gaussian posteriors
// (kh_gmm_component_posteriors' output: the posterior times the entry's weight).  Per Gaussian g of a pdf, in double, over
// the entries e that name the pdf:  occ[g] += p[e, g],  mean[g, d] += p[e, g] x[row(e), d],  var[g, d] += p[e, g] x[row(e), d]^2.
//
// Per pdf this is one GEMM  P^T (G x n)  times  S (n x C),  S_e = [1 | x | x o x],  C = 1 (flags w), 1 + D (mw), 1 + 2 D (mvw).
// S is never stored: a lane makes its element from one float of the x image in LDS (column D of the image holds 1), widened
// to double; x * x of a widened float is exact, and so is the product of two widened floats.
// v_mfma_f64_16x16x4_f64: A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15], one double per lane; C/D col = lane & 15,
// row = (lane >> 4) + 4 * reg (the operand layout of FmllrAccumulateKernel, stage B of kh_fmllr.hip's header).
// The host sorts the entries by pdf (stable: frame order within a pdf, csrc/kh_gmmacc_plan.h) and cuts each pdf's run into
// chunks of kChunk entries.  A workgroup is one (chunk, 16-Gaussian row tile): it stages kSub entries at a time - their x rows
// and the tile's 16 posteriors - in LDS; its 4 waves are the column groups: wave w owns the 16-column tiles w, w + 4, w + 8,
// w + 12 (the A operand is shared), so one work item = (pdf, chunk, row tile, column group).  Every chunk writes its partial
// sums [G x C] to a workspace; a second kernel adds a pdf's chunks in chunk order.  No atomics: the result depends only on the
// inputs, and the grouping of pdfs under the workspace limit changes no sum.
// Supported D: 1 ... 127 (16 column tiles = 256 columns >= 2 D + 1); KH_EINVAL above.
//
// The posteriors of this route, kh_gmm_acc_component_posteriors, one wave per entry: ComponentPosteriorsKernel<true> of
// kh_gmmstats.h, whose header states the arithmetic and why EXP and LOG are the float of the double function here.
// Static LDS of GmmAccumulateKernel: the x image kSub x kXs floats and the posterior image kSub x 16 floats:
// 32 x 144 x 4 + 32 x 16 x 4 = 20480 bytes.  kXs = 144 = 16 mod 64: the four entries of a fragment, 16 consecutive columns
// each, fall on four disjoint runs of 16 banks.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kh_common.h"
#include "kh_gmmacc_plan.h"
#include "kh_gmmstats.h"

using namespace kh;

namespace {

thread_local float g_ms[4] = {0.f, 0.f, 0.f, 0.f};   // acc_stats: whole call; host plan; the two kernels (device events); the posteriors' call
thread_local int32_t g_counts[3] = {0, 0, 0};      // groups; chunks; workgroups of the accumulate kernel
thread_local size_t g_ws_limit = 0;                // kh_gmm_acc_set_workspace_limit

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kChunk = 256;          // entries per chunk (tests/gmm_acc_cases.py: CHUNK)
constexpr int kSub = 32;             // entries staged in LDS at a time
constexpr int kAccWaves = 4;         // column groups of a workgroup
constexpr int kTilesPerWave = 4;     // 16-column tiles per wave: 16 accumulator doubles per lane
constexpr int kXs = 144;             // row pitch of the x image
constexpr int kMaxD = 127;
static_assert(kChunk % kSub == 0 && kSub % 4 == 0, "chunking");
static_assert(2 * kMaxD + 1 <= 16 * kAccWaves * kTilesPerWave && kMaxD + 1 <= kXs, "columns");

struct AccBlock {
  int64_t part_off;         // this chunk's partial sums [G x C] in the workspace
  int32_t e_begin, e_end;   // sorted entries
  int32_t G, rt;            // the pdf's Gaussians; this workgroup's row tile
};
struct AccPdf {
  int64_t part_off, out_off, size;   // first chunk's partial sums; the pdf's sums in the group's output; G x C
  int32_t n_chunks;
};

__global__ void __launch_bounds__(64 * kAccWaves)
GmmAccumulateKernel(const float *__restrict__ feats, int feat_stride, int D, int C, const int32_t *__restrict__ ent_row,
                    const int64_t *__restrict__ ent_goff, const float *__restrict__ post, const AccBlock *__restrict__ blocks,
                    double *__restrict__ partial) {
  __shared__ float xs[kSub][kXs];
  __shared__ float ps[kSub][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const AccBlock blk = blocks[blockIdx.x];
  const int CT = (C + 15) >> 4;
  // this lane's column of each tile as an index into the x image, and whether it is a square
  int src[kTilesPerWave];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    const int v = (wave + kAccWaves * j) * 16 + (lane & 15);
    int idx = D, sq = 0;               // column 0: the image's 1
    if (v >= 1 && v <= D) idx = v - 1;
    else if (v > D && v < C) { idx = v - 1 - D; sq = 1; }
    src[j] = idx | (sq << 8);
  }
  f64x4 acc[kTilesPerWave];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int g_mine = blk.rt * 16 + (lane & 15);
  for (int s0 = blk.e_begin; s0 < blk.e_end; s0 += kSub) {
    __syncthreads();   // the previous step's fragments have been read
    for (int f = wave; f < kSub; f += kAccWaves) {
      const int e = s0 + f;            // wave-uniform
      if (e < blk.e_end) {
        const float *x = feats + static_cast<size_t>(ent_row[e]) * feat_stride;
        for (int d = lane; d < D; d += 64) xs[f][d] = x[d];
        if (lane == 0) xs[f][D] = 1.f;
        if (lane < 16) ps[f][lane] = g_mine < blk.G ? post[ent_goff[e] + g_mine] : 0.f;
      } else {                         // past the chunk: zeros (an x of the image must be finite)
        for (int d = lane; d <= D; d += 64) xs[f][d] = 0.f;
        if (lane < 16) ps[f][lane] = 0.f;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int k0 = 0; k0 < kSub; k0 += 4) {
      const int f = k0 + (lane >> 4);
      const double av = static_cast<double>(ps[f][lane & 15]);
#pragma unroll
      for (int j = 0; j < kTilesPerWave; j++) {
        if (wave + kAccWaves * j < CT) {
          const double xv = static_cast<double>(xs[f][src[j] & 0xff]);
          const double bv = (src[j] >> 8) ? xv * xv : xv;
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
        }
      }
    }
  }
  double *dst = partial + blk.part_off;
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    const int v = (wave + kAccWaves * j) * 16 + (lane & 15);
    if (v < C) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int g = blk.rt * 16 + (lane >> 4) + 4 * reg;
        if (g < blk.G) dst[static_cast<size_t>(g) * C + v] = acc[j][reg];
      }
    }
  }
}

// out[pdf][e] = the pdf's chunks' partial[.][e] added in chunk order (0 for a pdf without chunks)
__global__ void __launch_bounds__(256)
GmmAccReduceKernel(const double *__restrict__ partial, const AccPdf *__restrict__ pdfs, int n_pdfs, double *__restrict__ out) {
  for (int p = blockIdx.x; p < n_pdfs; p += gridDim.x) {
    const AccPdf pd = pdfs[p];
    for (long long e = threadIdx.x; e < pd.size; e += 256) {
      double s = 0.0;
      for (int c = 0; c < pd.n_chunks; c++) s += partial[pd.part_off + static_cast<long long>(c) * pd.size + e];
      out[pd.out_off + e] = s;
    }
  }
}

}  // namespace

extern "C" {

int kh_gmm_acc_component_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts,
                                    const float *means_invvars, const float *inv_vars, const int32_t *pdf_offsets, int num_pdfs,
                                    const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const float *entry_weight,
                                    const int64_t *entry_gauss_offsets, float *gauss_post, float *entry_like) {
  return ComponentPosteriors<true>("kh_gmm_acc_component_posteriors", &g_ms[3], feats, T, D, feat_stride, gconsts, means_invvars,
                                   inv_vars, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_weight,
                                   entry_gauss_offsets, gauss_post, entry_like);
}

int kh_gmm_acc_stats(const float *feats, int T, int D, int feat_stride, const int32_t *pdf_offsets, int num_pdfs,
                     const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const int64_t *entry_gauss_offsets,
                     const float *gauss_post, int flags, double *occ, double *mean_acc, double *var_acc) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_gmm_acc_stats";
  KH_CHECK_ARG(pdf_offsets && frame_entry_offsets && occ && T >= 0 && D > 0 && num_pdfs > 0);
  KH_CHECK_ARG((flags & ~7) == 0 && (flags & 4) && (!(flags & 2) || (flags & 1)));   // AugmentGmmFlags: v needs m, m needs w
  const bool means = flags & 1, vars = flags & 2;
  KH_CHECK_ARG((!means || mean_acc) && (!vars || var_acc));
  if (D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  const int64_t E = frame_entry_offsets[T];
  KH_CHECK_ARG(E <= 0 || (feats && entry_pdf && entry_gauss_offsets && gauss_post && feat_stride >= D));
  std::string err;
  if (!kh_gmmacc::Check(T, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_gauss_offsets, &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  const int NG = pdf_offsets[num_pdfs];
  std::fill(occ, occ + NG, 0.0);
  if (means) std::fill(mean_acc, mean_acc + static_cast<size_t>(NG) * D, 0.0);
  if (vars) std::fill(var_acc, var_acc + static_cast<size_t>(NG) * D, 0.0);
  g_ms[1] = g_ms[2] = 0.f;
  g_counts[0] = g_counts[1] = g_counts[2] = 0;
  if (E == 0) {
    g_ms[0] = clk.Ms();
    return KH_OK;
  }
  const int C = 1 + (means ? D : 0) + (vars ? D : 0);
  kh_gmmacc::Plan plan;
  kh_gmmacc::Sort(T, num_pdfs, frame_entry_offsets, entry_pdf, &plan);
  std::vector<int64_t> sorted_goff(E);
  for (int64_t i = 0; i < E; i++) sorted_goff[i] = entry_gauss_offsets[plan.sorted_entry[i]];
  const size_t limit = g_ws_limit ? g_ws_limit : (size_t(1) << 30);
  const std::vector<kh_gmmacc::Group> groups = kh_gmmacc::Groups(plan, pdf_offsets, num_pdfs, C, kChunk, limit);
  g_ms[1] = clk.Ms();
  Scratch sc;
  const int32_t *d_row = sc.Upload(plan.sorted_row.data(), E);
  const int64_t *d_goff = sc.Upload(sorted_goff.data(), E);
  if (!d_row || !d_goff) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  float kernel_ms = 0.f;
  int64_t n_chunks = 0, n_blocks = 0;
  int rc2 = KH_OK;
  for (const kh_gmmacc::Group &gr : groups) {
    if (gr.n_chunks == 0) continue;   // no entry names a pdf of this group: the zeros stand
    std::vector<AccBlock> blocks;
    std::vector<AccPdf> pdfs;
    int64_t part = 0, out = 0;
    for (int p = gr.pdf_begin; p < gr.pdf_end; p++) {
      const int G = pdf_offsets[p + 1] - pdf_offsets[p];
      const int64_t e0 = plan.pdf_entry_offsets[p], e1 = plan.pdf_entry_offsets[p + 1];
      const int64_t size = static_cast<int64_t>(G) * C;
      pdfs.push_back(AccPdf{part, out, size, static_cast<int32_t>(kh_gmmacc::NumChunks(e1 - e0, kChunk))});
      for (int64_t e = e0; e < e1; e += kChunk) {
        for (int rt = 0; rt < DivUp(G, 16); rt++)
          blocks.push_back(AccBlock{part, static_cast<int32_t>(e), static_cast<int32_t>(std::min<int64_t>(e + kChunk, e1)), G, rt});
        part += size;
      }
      out += size;
    }
    n_chunks += gr.n_chunks;
    n_blocks += static_cast<int64_t>(blocks.size());
    Scratch gsc;   // this group's buffers go back to the pool before the next group asks
    const AccBlock *d_blocks = gsc.Upload(blocks.data(), blocks.size());
    const AccPdf *d_pdfs = gsc.Upload(pdfs.data(), pdfs.size());
    double *d_partial = gsc.Get<double>(part);
    double *d_out = gsc.Get<double>(out);
    if (!d_blocks || !d_pdfs || !d_partial || !d_out || blocks.size() >= (size_t(1) << 31)) {
      SetError("%s: out of device memory (pdfs %d .. %d, %zu workgroups)", fn, gr.pdf_begin, gr.pdf_end - 1, blocks.size());
      rc2 = KH_ENOMEM;
      break;
    }
    ev.Begin();
    hipLaunchKernelGGL(GmmAccumulateKernel, dim3(static_cast<unsigned>(blocks.size())), dim3(64 * kAccWaves), 0, Stream(), feats,
                       feat_stride, D, C, d_row, d_goff, gauss_post, d_blocks, d_partial);
    hipLaunchKernelGGL(GmmAccReduceKernel, dim3(static_cast<unsigned>(std::min<size_t>(pdfs.size(), 65536))), dim3(256), 0, Stream(),
                       d_partial, d_pdfs, static_cast<int>(pdfs.size()), d_out);
    ev.End();
    std::vector<double> h_out(out);
    if (hipError_t e = ev.Collect(h_out.data(), d_out, out, &kernel_ms); e != hipSuccess) {
      SetError("%s: %s", fn, hipGetErrorString(e));
      rc2 = KH_EDEVICE;
      break;
    }
    const double *src = h_out.data();
    for (int g = pdf_offsets[gr.pdf_begin]; g < pdf_offsets[gr.pdf_end]; g++, src += C) {
      occ[g] = src[0];
      if (means) std::copy(src + 1, src + 1 + D, mean_acc + static_cast<size_t>(g) * D);
      if (vars) std::copy(src + 1 + D, src + 1 + 2 * D, var_acc + static_cast<size_t>(g) * D);
    }
  }
  if (rc2 != KH_OK) return rc2;
  g_ms[2] = kernel_ms;
  g_counts[0] = static_cast<int32_t>(groups.size());
  g_counts[1] = static_cast<int32_t>(std::min<int64_t>(n_chunks, INT32_MAX));
  g_counts[2] = static_cast<int32_t>(std::min<int64_t>(n_blocks, INT32_MAX));
  g_ms[0] = clk.Ms();
  return KH_OK;
}

int kh_gmm_acc_set_workspace_limit(size_t bytes) {
  g_ws_limit = bytes;
  return KH_OK;
}
int kh_gmm_acc_max_dim(void) { return kMaxD; }
int kh_gmm_acc_chunk(void) { return kChunk; }

int kh_gmm_acc_last_timings(float *ms, int32_t *counts) {
  KH_CHECK_ARG(ms && counts);
  for (int i = 0; i < 4; i++) ms[i] = g_ms[i];
  for (int i = 0; i < 3; i++) counts[i] = g_counts[i];
  return KH_OK;
}

}  // extern "C"
