// kh_fmllr.hip - fMLLR estimation for batches of speakers (gmm-est-fmllr, gmm-est-fmllr-gpost, gmm-post-to-gpost).
//
// Replaces, stage by stage (each stage has explicit inputs and outputs, include/kaldi_hip.h):
//   A1 kh_gmm_component_posteriors  DiagGmm::ComponentPosteriors (gmm/diag-gmm.cc:601-615) with VectorBase::ApplySoftMax
//                                   (matrix/kaldi-vector.cc:840-847) and the posterior.Scale(weight) of
//                                   FmllrDiagGmmAccs::AccumulateForGmm (transform/fmllr-diag-gmm.cc:101-112), per entry
//   A2 kh_fmllr_frame_stats         AccumulateFromPosteriors (:30-43) with DataHasChanged / InitSingleFrameStats (:542-560)
//   B  kh_fmllr_accumulate          CommitSingleFrameStats (:562-596), update type "full", for all speakers
//   C  kh_fmllr_update              FmllrDiagGmmAccs::Update (:131-166), ComputeFmllrMatrixDiagGmmFull / FmllrInnerUpdate
//                                   (:193-273), ...Diagonal (:275-348), ...Offset (:350-378), FmllrAuxFuncDiagGmm (:481-508);
//                                   host C++ in double (csrc/kh_fmllr_update.h), threads over speakers, no device
//
// A1, one wave per (frame, pdf) entry: ComponentPosteriorsKernel<false> of kh_gmmstats.h, whose header states the arithmetic
// (EXP and LOG are the device library's expf / logf here).
//
// A2, one 64-lane workgroup per merged frame, lane = dimension: a[d] = fmaf(post, means_invvars[g][d], a[d]) and b[d] with
// inv_vars, over the merged frame's entries in order and each entry's Gaussians in order; count (double) adds each entry's
// fl32(double sum of its posteriors) (VectorBase::Sum, kaldi-vector.cc:680-684).
// Merged frames.  The reference keeps one frame's (x, a, b, count) and commits it when AccumulateFromPosteriors sees other
// data (:35-38); it is called once per entry, so frames without entries are never seen.  Hence: within a speaker, walking the
// frames THAT HAVE ENTRIES in order (across the speaker's utterance boundaries), a frame whose row equals the previous such
// frame's row joins its merged frame.  "Equals" is the reference's float != on every element (ApproxEqual with tol 0,
// kaldi-vector.cc:556-561): bit identity but for -0 == +0 and NaN != NaN.  The speaker's first frame always starts a merged
// frame (the reference compares it with zeros and skips InitSingleFrameStats when equal, which leaves the same state).  The
// entries of a merged frame are one contiguous range of the entry list.  A merged frame with count == 0 adds nothing (:566).
//
// B, the hot kernel: per speaker, in double,  K[i][j] = sum_t a_t[i] x+_t[j],  G_i[r][c] = sum_t b_t[i] x+_t[r] x+_t[c]
// (r >= c, packed as SpMatrix: r (r + 1) / 2 + c), x+ = [x, 1].  With P = (D + 1)(D + 2) / 2 this is one GEMM
// [b | a]^T (2D x frames) times S (frames x P), S_t[r, c] = x+_t[r] x+_t[c]: K's columns are S's last packed row (x+[D] = 1).
// S is never stored: a lane makes its element from two floats of x+ in LDS, and the double product of two floats is exact.
// v_mfma_f64_16x16x4_f64: A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15], one double per lane; C/D
// col = lane & 15, row = (lane >> 4) + 4 * reg.  A wave owns one 16-row tile and up to kTilesPerWave column tiles (the A
// operand is shared), a workgroup is 4 waves, blockIdx.y walks the (row tile, column group) items, blockIdx.x the chunks of
// at most kFrameChunk merged frames of one speaker.  Every chunk writes its partial sums to a workspace; a second kernel
// adds a speaker's chunks in chunk order.  No atomics: the result depends only on the inputs.  beta is summed on the host
// in merged-frame order, as the reference does.
// Supported D: 1 ... 63 (x+ has at most 64 elements: the LDS image and the 8-bit (r, c) fields); KH_EINVAL above.
// The plain v_fma_f64 form of this kernel was not built; on this part the two peak rates are equal, the MFMA form needs two
// LDS reads per 1024 multiply-adds where the vector form needs operands in registers per lane.
#include <algorithm>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "kh_common.h"
#include "kh_fmllr_update.h"
#include "kh_gmmstats.h"

using namespace kh;

namespace {

thread_local float g_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // A1, A2, B, C of this thread's last calls; B's kernels (events); B's groups
thread_local size_t g_ws_limit = 0;   // kh_fmllr_set_workspace_limit

// A2.
__global__ void __launch_bounds__(64)
FrameStatsKernel(int D, const float *__restrict__ mi, const float *__restrict__ iv, const int32_t *__restrict__ pdf_offsets,
                 const int64_t *__restrict__ run_entry_offsets, int n_runs, const int32_t *__restrict__ entry_pdf,
                 const int64_t *__restrict__ entry_goff, const float *__restrict__ post, float *__restrict__ a_out,
                 float *__restrict__ b_out, double *__restrict__ count_out) {
  for (int r = blockIdx.x; r < n_runs; r += gridDim.x) {
    const long long e0 = run_entry_offsets[r], e1 = run_entry_offsets[r + 1];
    for (int d = threadIdx.x; d < D; d += 64) {
      float a = 0.f, b = 0.f;
      for (long long e = e0; e < e1; e++) {
        const int m0 = pdf_offsets[entry_pdf[e]];
        const long long go = entry_goff[e];
        const int n = static_cast<int>(entry_goff[e + 1] - go);
        for (int g = 0; g < n; g++) {
          const float p = post[go + g];
          a = fmaf(p, mi[static_cast<size_t>(m0 + g) * D + d], a);   // stats.a.AddMatVec(1.0, means_invvars, kTrans, posterior, 1.0)
          b = fmaf(p, iv[static_cast<size_t>(m0 + g) * D + d], b);
        }
      }
      a_out[static_cast<size_t>(r) * D + d] = a;
      b_out[static_cast<size_t>(r) * D + d] = b;
    }
    if (threadIdx.x == 63) {
      double c = 0.0;
      for (long long e = e0; e < e1; e++) {
        double s = 0.0;
        for (long long g = entry_goff[e]; g < entry_goff[e + 1]; g++) s += post[g];
        c += static_cast<double>(static_cast<float>(s));   // stats.count += posterior.Sum()
      }
      count_out[r] = c;
    }
  }
}

// ---- B
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kFrameChunk = 256;     // merged frames per workgroup (tests/fmllr_cases.py: FRAME_CHUNK)
constexpr int kSub = 32;             // merged frames staged in LDS at a time
constexpr int kTilesPerWave = 8;     // 16-column tiles per wave: 32 accumulator doubles per lane
constexpr int kAccWaves = 4;
constexpr int kXs = 65;              // row pitch of the x+ image (odd: the four frames of a fragment fall on different banks)
constexpr int kMaxD = 63;
static_assert(kFrameChunk % kSub == 0 && kSub % 4 == 0, "chunking");

struct AccChunk { int32_t spk, run_begin, run_end; };

__global__ void __launch_bounds__(64 * kAccWaves)
FmllrAccumulateKernel(const float *__restrict__ feats, int feat_stride, int D, const int32_t *__restrict__ run_row,
                      const float *__restrict__ a_in, const float *__restrict__ b_in, const double *__restrict__ count,
                      const AccChunk *__restrict__ chunks, double *__restrict__ partial) {
  __shared__ float xs[kSub][kXs];
  __shared__ float ab[2][kSub][64];   // [0]: b (rows of the G tiles), [1]: a (rows of the K tiles)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int P = (D + 1) * (D + 2) / 2;
  const int RT = (D + 15) / 16, CT = (P + 15) / 16, GG = (CT + kTilesPerWave - 1) / kTilesPerWave;
  const int n_items = RT * GG + RT;   // (row tile, group of G column tiles) ..., then (row tile, the K columns)
  const int item = blockIdx.y * kAccWaves + wave;   // wave-uniform
  int kind = 0, rt = 0, ct0 = 0, n_tiles = 0;
  if (item < RT * GG) {
    rt = item / GG;
    ct0 = (item - rt * GG) * kTilesPerWave;
    n_tiles = CT - ct0 < kTilesPerWave ? CT - ct0 : kTilesPerWave;
  } else if (item < n_items) {
    kind = 1;
    rt = item - RT * GG;
    n_tiles = (D + 1 + 15) / 16;   // <= 4
  }
  // this lane's column of each tile as (r, c) of x+, and whether it exists
  int rc[kTilesPerWave];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    const int v = (ct0 + j) * 16 + (lane & 15);
    int r = 0, c = 0, ok = 0;
    if (j < n_tiles) {
      if (kind == 1) {
        if (v <= D) { r = D; c = v; ok = 1; }
      } else if (v < P) {
        r = static_cast<int>((sqrtf(8.f * static_cast<float>(v) + 1.f) - 1.f) * 0.5f);
        while (r * (r + 1) / 2 > v) r--;
        while ((r + 1) * (r + 2) / 2 <= v) r++;
        c = v - r * (r + 1) / 2;
        ok = 1;
      }
    }
    rc[j] = r | (c << 8) | (ok << 16);
  }
  f64x4 acc[kTilesPerWave];
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const AccChunk ch = chunks[blockIdx.x];
  const int arow = rt * 16 + (lane & 15);   // < 64
  for (int s0 = ch.run_begin; s0 < ch.run_end; s0 += kSub) {
    __syncthreads();   // the previous step's fragments have been read
    for (int i = t; i < kSub * 64; i += 64 * kAccWaves) {
      const int f = i >> 6, d = i & 63, r = s0 + f;
      float xv = 0.f, av = 0.f, bv = 0.f;
      if (r < ch.run_end) {
        // stats.count == 0.0: nothing is committed - the whole frame is zeros (its x too: 0 * inf would be NaN)
        if (count[r] != 0.0) {
          if (d < D) {
            xv = feats[static_cast<size_t>(run_row[r]) * feat_stride + d];
            av = a_in[static_cast<size_t>(r) * D + d];
            bv = b_in[static_cast<size_t>(r) * D + d];
          } else if (d == D) {
            xv = 1.f;
          }
        }
      }
      xs[f][d] = xv;
      ab[0][f][d] = bv;
      ab[1][f][d] = av;
    }
    __syncthreads();
    if (n_tiles > 0) {
#pragma unroll 2
      for (int k0 = 0; k0 < kSub; k0 += 4) {
        const int f = k0 + (lane >> 4);
        const double av = static_cast<double>(ab[kind][f][arow]);
#pragma unroll
        for (int j = 0; j < kTilesPerWave; j++) {
          if (j < n_tiles) {
            const double bv = static_cast<double>(xs[f][rc[j] & 0xff]) * static_cast<double>(xs[f][(rc[j] >> 8) & 0xff]);
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
    }
  }
  // partial[chunk] = G part [D][P], then K part [D][D + 1]
  const size_t S = static_cast<size_t>(D) * P + static_cast<size_t>(D) * (D + 1);
  double *dst = partial + S * blockIdx.x;
#pragma unroll
  for (int j = 0; j < kTilesPerWave; j++) {
    if (j < n_tiles && ((rc[j] >> 16) & 1)) {
      const int v = (ct0 + j) * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int i = rt * 16 + (lane >> 4) + 4 * reg;
        if (i < D) {
          if (kind == 0) dst[static_cast<size_t>(i) * P + v] = acc[j][reg];
          else dst[static_cast<size_t>(D) * P + static_cast<size_t>(i) * (D + 1) + v] = acc[j][reg];
        }
      }
    }
  }
}

// out[spk][e] = the speaker's chunks' partial[.][e] added in chunk order (0 for a speaker without chunks)
__global__ void __launch_bounds__(256)
FmllrReduceKernel(const double *__restrict__ partial, const int32_t *__restrict__ spk_chunk_offsets, int n_spk, long long S,
                  double *__restrict__ out) {
  for (int spk = blockIdx.y; spk < n_spk; spk += gridDim.y) {
    const int c0 = spk_chunk_offsets[spk], c1 = spk_chunk_offsets[spk + 1];
    for (long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; e < S; e += static_cast<long long>(gridDim.x) * 256) {
      double s = 0.0;
      for (int c = c0; c < c1; c++) s += partial[static_cast<size_t>(c) * S + e];
      out[static_cast<size_t>(spk) * S + e] = s;
    }
  }
}

// ---- shared host checks
bool CheckOffsets32(const char *fn, const char *what, const int32_t *o, int n, int64_t last) {
  if (o[0] != 0) { SetError("%s: %s[0] = %d, not 0", fn, what, o[0]); return false; }
  for (int i = 0; i < n; i++)
    if (o[i + 1] < o[i]) { SetError("%s: %s runs backwards at %d (%d .. %d)", fn, what, i, o[i], o[i + 1]); return false; }
  if (last >= 0 && o[n] != last) { SetError("%s: %s ends at %d, expected %lld", fn, what, o[n], static_cast<long long>(last)); return false; }
  return true;
}

}  // namespace

extern "C" {

int kh_gmm_component_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts,
                                const float *means_invvars, const float *inv_vars, const int32_t *pdf_offsets, int num_pdfs,
                                const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const float *entry_weight,
                                const int64_t *entry_gauss_offsets, float *gauss_post, float *entry_like) {
  return ComponentPosteriors<false>("kh_gmm_component_posteriors", &g_ms[0], feats, T, D, feat_stride, gconsts, means_invvars,
                                    inv_vars, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_weight,
                                    entry_gauss_offsets, gauss_post, entry_like);
}

int kh_fmllr_frame_stats(const float *feats, int T, int D, int feat_stride, const float *means_invvars, const float *inv_vars,
                         const int32_t *pdf_offsets, int num_pdfs, const int32_t *utt_row_offsets, int n_utts,
                         const int32_t *spk_utt_offsets, int n_spk, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                         const int64_t *entry_gauss_offsets, const float *gauss_post, int32_t *run_row, int32_t *spk_run_offsets,
                         float *a, float *b, double *count) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_fmllr_frame_stats";
  KH_CHECK_ARG(feats && means_invvars && inv_vars && pdf_offsets && utt_row_offsets && spk_utt_offsets && frame_entry_offsets &&
               entry_gauss_offsets && run_row && spk_run_offsets);
  KH_CHECK_ARG(T > 0 && D > 0 && feat_stride >= D && num_pdfs > 0 && n_utts > 0 && n_spk > 0);
  if (!CheckOffsets32(fn, "utt_row_offsets", utt_row_offsets, n_utts, T)) return KH_EINVAL;
  if (!CheckOffsets32(fn, "spk_utt_offsets", spk_utt_offsets, n_spk, n_utts)) return KH_EINVAL;
  const int64_t E = frame_entry_offsets[T];
  KH_CHECK_ARG(E <= 0 || (entry_pdf && gauss_post && a && b && count));
  std::string err;
  if (!kh_gmmacc::Check(T, pdf_offsets, num_pdfs, frame_entry_offsets, entry_pdf, entry_gauss_offsets, &err)) {
    SetError("%s: %s", fn, err.c_str());
    return KH_EINVAL;
  }
  // the merged frames: needs the rows on the host
  std::vector<float> h(static_cast<size_t>(T) * D);
  KH_HIP(hipMemcpy2DAsync(h.data(), sizeof(float) * D, feats, sizeof(float) * feat_stride, sizeof(float) * D, T, hipMemcpyDeviceToHost, Stream()));
  KH_HIP(hipStreamSynchronize(Stream()));
  std::vector<int64_t> run_entry;   // first entry of each merged frame, then E
  int n_runs = 0;
  for (int s = 0; s < n_spk; s++) {
    spk_run_offsets[s] = n_runs;
    int cur = -1;   // the row held by single_frame_stats_
    for (int t = utt_row_offsets[spk_utt_offsets[s]]; t < utt_row_offsets[spk_utt_offsets[s + 1]]; t++) {
      if (frame_entry_offsets[t + 1] == frame_entry_offsets[t]) continue;
      bool changed = cur < 0;
      if (!changed) {
        const float *x = &h[static_cast<size_t>(t) * D], *y = &h[static_cast<size_t>(cur) * D];
        for (int d = 0; d < D; d++)
          if (x[d] != y[d]) { changed = true; break; }
      }
      if (changed) {
        run_row[n_runs++] = t;
        run_entry.push_back(frame_entry_offsets[t]);
        cur = t;
      }
    }
  }
  spk_run_offsets[n_spk] = n_runs;
  run_entry.push_back(E);
  g_ms[1] = 0.f;
  if (n_runs == 0) return KH_OK;
  Scratch sc;
  const int32_t *d_off = sc.Upload(pdf_offsets, num_pdfs + 1);
  const int64_t *d_run = sc.Upload(run_entry.data(), run_entry.size());
  const int32_t *d_pdf = sc.Upload(entry_pdf, E);
  const int64_t *d_goff = sc.Upload(entry_gauss_offsets, E + 1);
  if (!d_off || !d_run || !d_pdf || !d_goff) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
  hipLaunchKernelGGL(FrameStatsKernel, dim3(std::min(n_runs, NumCUs() * 32)), dim3(64), 0, Stream(), D, means_invvars, inv_vars,
                     d_off, d_run, n_runs, d_pdf, d_goff, gauss_post, a, b, count);
  KH_LAUNCH_CHECK();
  KH_HIP(hipStreamSynchronize(Stream()));
  g_ms[1] = clk.Ms();
  return KH_OK;
}

int kh_fmllr_accumulate(const float *feats, int T, int D, int feat_stride, const int32_t *run_row, const int32_t *spk_run_offsets,
                        int n_spk, const float *a, const float *b, const double *count, double *beta, double *K, double *G) {
  Clock clk;
  int rc = EnsureDevice();
  if (rc) return rc;
  const char *fn = "kh_fmllr_accumulate";
  KH_CHECK_ARG(feats && spk_run_offsets && beta && K && G && T > 0 && D > 0 && feat_stride >= D && n_spk > 0);
  if (D > kMaxD) {
    SetError("%s: feature dimension %d, supported 1 ... %d", fn, D, kMaxD);
    return KH_EINVAL;
  }
  if (!CheckOffsets32(fn, "spk_run_offsets", spk_run_offsets, n_spk, -1)) return KH_EINVAL;
  const int n_runs = spk_run_offsets[n_spk];
  KH_CHECK_ARG(n_runs == 0 || (run_row && a && b && count));
  for (int r = 0; r < n_runs; r++)
    if (run_row[r] < 0 || run_row[r] >= T) { SetError("%s: merged frame %d names row %d of %d", fn, r, run_row[r], T); return KH_EINVAL; }
  const int P = (D + 1) * (D + 2) / 2;
  const size_t S = static_cast<size_t>(D) * P + static_cast<size_t>(D) * (D + 1);
  // beta_ += stats.count in merged-frame order (:572); a zero count adds nothing either way
  std::vector<double> h_count(n_runs);
  if (n_runs) {
    KH_HIP(hipMemcpyAsync(h_count.data(), count, sizeof(double) * n_runs, hipMemcpyDeviceToHost, Stream()));
    KH_HIP(hipStreamSynchronize(Stream()));
  }
  for (int s = 0; s < n_spk; s++) {
    double bsum = 0.0;
    for (int r = spk_run_offsets[s]; r < spk_run_offsets[s + 1]; r++) bsum += h_count[r];
    beta[s] = bsum;
  }
  // Speakers go in groups whose workspace (one partial per chunk, one sum per speaker, S doubles each) stays within the limit:
  // a per-utterance job of 10 000 utterances at D = 40 would otherwise ask for 6 GB at once.  A speaker is never split: one
  // speaker alone may exceed the limit (256 frames per 8 S bytes).  The grouping does not change any sum.
  const size_t limit = g_ws_limit ? g_ws_limit : (size_t(1) << 30);
  const size_t gs = static_cast<size_t>(D) * P, ks = static_cast<size_t>(D) * (D + 1);
  const int RT = DivUp(D, 16), CT = DivUp(P, 16), GG = DivUp(CT, kTilesPerWave);
  const int n_items = RT * GG + RT;
  Scratch sc;
  const int32_t *d_run_row = sc.Upload(run_row, n_runs);
  if (!d_run_row) { SetError("%s: out of device memory", fn); return KH_ENOMEM; }
  KernelEvents ev;
  if (hipError_t ee = ev.Init(); ee != hipSuccess) {
    SetError(kEventsFailed, fn, hipGetErrorString(ee));
    return KH_EDEVICE;
  }
  float kernel_ms = 0.f;
  int n_groups = 0;
  int rc2 = KH_OK;
  for (int s0 = 0; s0 < n_spk && rc2 == KH_OK;) {
    std::vector<AccChunk> chunks;
    std::vector<int32_t> spk_chunk(1, 0);
    int s1 = s0;
    while (s1 < n_spk) {
      const size_t nc = static_cast<size_t>(DivUp(spk_run_offsets[s1 + 1] - spk_run_offsets[s1], kFrameChunk));
      if (s1 > s0 && (chunks.size() + nc + (s1 - s0) + 1) * S * sizeof(double) > limit) break;
      for (int r = spk_run_offsets[s1]; r < spk_run_offsets[s1 + 1]; r += kFrameChunk)
        chunks.push_back(AccChunk{s1 - s0, r, std::min(r + kFrameChunk, spk_run_offsets[s1 + 1])});
      spk_chunk.push_back(static_cast<int32_t>(chunks.size()));
      s1++;
    }
    const int ng = s1 - s0;
    n_groups++;
    Scratch gsc;   // this group's buffers go back to the pool before the next group asks
    const AccChunk *d_chunks = gsc.Upload(chunks.data(), chunks.size());
    const int32_t *d_spk_chunk = gsc.Upload(spk_chunk.data(), spk_chunk.size());
    double *d_partial = gsc.Get<double>(S * chunks.size());
    double *d_out = gsc.Get<double>(S * ng);
    if (!d_chunks || !d_spk_chunk || !d_partial || !d_out) {
      SetError("%s: out of device memory (speakers %d .. %d, %zu chunks)", fn, s0, s1 - 1, chunks.size());
      rc2 = KH_ENOMEM;
      break;
    }
    ev.Begin();
    if (!chunks.empty())
      hipLaunchKernelGGL(FmllrAccumulateKernel, dim3(static_cast<unsigned>(chunks.size()), DivUp(n_items, kAccWaves)), dim3(64 * kAccWaves), 0,
                         Stream(), feats, feat_stride, D, d_run_row, a, b, count, d_chunks, d_partial);
    hipLaunchKernelGGL(FmllrReduceKernel, dim3(static_cast<unsigned>(std::min<size_t>(DivUp64(S, 256), 1024)), std::min(ng, 4096)), dim3(256), 0,
                       Stream(), d_partial, d_spk_chunk, ng, static_cast<long long>(S), d_out);
    ev.End();
    std::vector<double> h_out(S * ng);
    if (hipError_t e = ev.Collect(h_out.data(), d_out, S * ng, &kernel_ms); e != hipSuccess) {
      SetError("%s: %s", fn, hipGetErrorString(e));
      rc2 = KH_EDEVICE;
      break;
    }
    for (int s = 0; s < ng; s++) {
      std::copy(h_out.begin() + S * s, h_out.begin() + S * s + gs, G + gs * (s0 + s));
      std::copy(h_out.begin() + S * s + gs, h_out.begin() + S * (s + 1), K + ks * (s0 + s));
    }
    s0 = s1;
  }
  if (rc2 != KH_OK) return rc2;
  g_ms[4] = kernel_ms;
  g_ms[5] = static_cast<float>(n_groups);
  g_ms[2] = clk.Ms();
  return KH_OK;
}

int kh_fmllr_update(int n_spk, int D, const double *beta, const double *K, const double *G, const char *update_type, float min_count,
                    int num_iters, int num_threads, float *transforms, float *objf_impr, float *count) {
  Clock clk;
  KH_CHECK_ARG(n_spk > 0 && D > 0 && beta && K && G && update_type && transforms && objf_impr && count && num_iters >= 0);
  const std::string type(update_type);
  if (type != "full" && type != "diag" && type != "offset" && type != "none") {
    SetError("Unknown fMLLR update type %s, fmllr-update-type must be one of \"full\"|\"diag\"|\"offset\"|\"none\"", update_type);
    return KH_EINVAL;
  }
  const int D1 = D + 1, P = D1 * (D + 2) / 2;
  std::vector<int> status(n_spk, kh_fmllr::kOk);
  std::vector<std::string> errs(n_spk);
  auto one = [&](int s) {
    kh_fmllr::SpkStats st{D, beta[s], K + static_cast<size_t>(s) * D * D1, G + static_cast<size_t>(s) * D * P};
    status[s] = kh_fmllr::UpdateSpeaker(st, type, min_count, num_iters, transforms + static_cast<size_t>(s) * D * D1, &objf_impr[s],
                                        &count[s], &errs[s]);
  };
  int nt = num_threads > 0 ? num_threads : 16;
  nt = std::max(1, std::min(std::min(nt, 16), n_spk));
  if (nt == 1) {
    for (int s = 0; s < n_spk; s++) one(s);
  } else {
    std::vector<std::thread> th;
    for (int w = 0; w < nt; w++)
      th.emplace_back([&, w]() { for (int s = w; s < n_spk; s += nt) one(s); });
    for (auto &x : th) x.join();
  }
  g_ms[3] = clk.Ms();
  for (int s = 0; s < n_spk; s++)
    if (status[s] != kh_fmllr::kOk) {
      SetError("kh_fmllr_update: speaker %d: %s", s, errs[s].c_str());
      return KH_EINVAL;
    }
  return KH_OK;
}

int kh_fmllr_set_workspace_limit(size_t bytes) {
  g_ws_limit = bytes;
  return KH_OK;
}
int kh_fmllr_max_dim(void) { return kMaxD; }
int kh_fmllr_frame_chunk(void) { return kFrameChunk; }

int kh_fmllr_last_timings(float *ms) {
  KH_CHECK_ARG(ms);
  for (int i = 0; i < 6; i++) ms[i] = g_ms[i];
  return KH_OK;
}

}  // extern "C"
