// kh_gmm.hip — DiagGmm::LogLikelihoods over batched frames.
//
// Replaces DiagGmm::LogLikelihoods(const MatrixBase&, Matrix*)
// (gmm/diag-gmm.cc:546-562: two sgemm calls on [x | x^2]), ComputeGconsts
// (:114-152, host), and the per-(frame,pdf) scoring of
// DecodableAmDiagGmmUnmapped::LogLikelihoodZeroBased
// (gmm/decodable-am-diag-gmm.cc:28-71) + VectorBase::LogSumExp
// (matrix/kaldi-vector.cc:745-763) evaluated densely for every (frame, pdf).
//
// Kernel 1 (per-Gaussian log-likelihoods): frames on the lanes.  A wave owns 64
// frames whose features [x | x*x] live in registers; the Gaussian parameters
// (means_invvars / inv_vars rows, gconst) are wave-uniform, so they are fetched
// through the scalar cache and used as SGPR operands of the FMAs — no LDS
// traffic in the inner loop.  Each 64-frame x 64-Gaussian result tile is
// transposed through LDS so the T x M matrix is written in full coalesced rows.
// Numerics per element (bit-identical to the CPU oracle):
//   a1 = fmaf-chain_d(x_d, mi_d); a2 = fmaf-chain_d(x_d*x_d, iv_d);
//   ll = (g + a1) + (-0.5f * a2)
// Kernel 2: one thread per (frame, pdf): LogSumExp with the reference's float cutoff, kept set
// and double accumulation in Gaussian order.  The two transcendental steps are NOT libm's:
// exp(x) is the hardware exp2 of the float product x * log2(e), log(sum) is the hardware log2
// of the sum rounded to float, times ln 2 (ExpTerm / LogOfSum below).  Both units' accuracy is
// taken as 1 ulp: the figure the "CDNA3 Instruction Set Architecture" guide gives for V_EXP_F32
// and V_LOG_F32; gfx950 is assumed to match it.  Against the exact LogSumExp of the same float inputs the result is within
//   1/2 ulp_f32(|result|) + c(n),   n = #Gaussians of the pdf,
//   c(n) = 15.95 * 2^-24             rounding of the exp2 argument, |f - max| <= 15.95   9.5e-7
//        + 2^-21 + 15.95 * 1.4e-8    float f - max; log2(e) as a float                   6.9e-7
//        + 2^-23                     1 ulp of exp2                                       1.2e-7
//        + 2^-24                     the sum rounded to float                            0.6e-7
//        + ulp_f32(log2 n) * ln 2    1 ulp of log2                                  (n = 128: 3.3e-7)
//        + ulp_f32(ln n)             the product with ln 2 (as a float), rounded    (n = 128: 4.8e-7)
// = 2.6e-6 for a pdf of 128 Gaussians (tests/gmm_cases.py derives it and the suite holds the
// kernels to twice that); the project's requirement on frame log-likelihoods is 1e-4.
#include <cfloat>
#include <cmath>
#include <vector>

#include "kh_common.h"

using namespace kh;

namespace {

constexpr int kThreads = 256;
constexpr int kTileM = 64;

template <int DP>
__global__ void __launch_bounds__(kThreads)
GmmLoglikesKernel(const float *__restrict__ data, int T, int D, int data_stride,
                  const float *__restrict__ gconsts, const float *__restrict__ mi,
                  const float *__restrict__ iv, int M, float *__restrict__ out,
                  int out_stride, int m_per_block) {
  __shared__ float tile[kThreads / 64][kTileM][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = (blockIdx.x * (kThreads / 64) + wave) * 64;
  if (t0 >= T) return;  // wave-uniform
  const int t = t0 + lane;
  float x[DP], xx[DP];
#pragma unroll
  for (int d = 0; d < DP; d++) {
    float v = (d < D && t < T) ? data[static_cast<size_t>(t) * data_stride + d] : 0.f;
    x[d] = v;
    xx[d] = v * v;  // data_sq.ApplyPow(2.0)
  }
  const int m_begin = blockIdx.y * m_per_block;
  int m_end = m_begin + m_per_block;
  if (m_end > M) m_end = M;
  float(*tl)[65] = tile[wave];
  for (int mb = m_begin; mb < m_end; mb += kTileM) {
    const int nm = (m_end - mb) < kTileM ? (m_end - mb) : kTileM;
    for (int j = 0; j < nm; j++) {
      const int m = __builtin_amdgcn_readfirstlane(mb + j);
      const float *mir = mi + static_cast<size_t>(m) * D;
      const float *ivr = iv + static_cast<size_t>(m) * D;
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int d = 0; d < DP; d++) {
        if (d < D) {
          a1 = fmaf(x[d], mir[d], a1);
          a2 = fmaf(xx[d], ivr[d], a2);
        }
      }
      const float ll = (gconsts[m] + a1) + (-0.5f * a2);
      tl[j][lane] = ll;  // [gaussian][frame]
    }
    // wave-private tile: no block barrier needed, only LDS visibility in-wave
    __builtin_amdgcn_wave_barrier();
    for (int r = 0; r < 64; r++) {
      const int tr = t0 + r;
      if (tr >= T) break;
      if (lane < nm)
        out[static_cast<size_t>(tr) * out_stride + mb + lane] = tl[lane][r];
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// The two transcendental steps of LogSumExp (kaldi-vector.cc:755-761: "sum += Exp(f - max)",
// "max + Log(sum)") on the hardware's exp2 / log2 units: exp(x) = exp2(x * log2 e) and
// log(s) = log2(s) * ln 2.  The terms lie in (0, 1], the double sum in [1, #Gaussians of the pdf].
// The error against the exact LogSumExp is derived in this file's header: c(n) = 2.6e-6 for a pdf
// of 128 Gaussians beside the 1/2 ulp (2e-6 at |score| ~ 50) of the float result - north_star asks
// 1e-4 on frame log-likelihoods.  The libm versions
// (expf: ~15 VALU instructions, double log: ~150) made the fused kernel VALU-bound: 38 VALU
// instructions per MFMA instruction, matrix pipe 18 % busy.
__device__ __forceinline__ float ExpTerm(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ double LogOfSum(double sum) {
  return static_cast<double>(__builtin_amdgcn_logf(static_cast<float>(sum)) * 0.69314718055994530942f);
}

// VectorBase::LogSumExp(prune) kaldi-vector.cc:745-763 per (frame, pdf).
__global__ void __launch_bounds__(kThreads)
GmmPdfLseKernel(const float *__restrict__ ll, int T, int ll_stride,
                const int32_t *__restrict__ pdf_offsets, int num_pdfs, float prune,
                float min_log_diff, float *__restrict__ out, int out_stride) {
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const float *row = ll + static_cast<size_t>(t) * ll_stride;
    for (int j = blockIdx.x * kThreads + threadIdx.x; j < num_pdfs;
         j += gridDim.x * kThreads) {
      const int s = pdf_offsets[j], e = pdf_offsets[j + 1];
      float mx = -INFINITY;
      for (int m = s; m < e; m++) mx = fmaxf(mx, row[m]);
      float cutoff = mx + min_log_diff;
      if (prune > 0.0f && mx - prune > cutoff) cutoff = mx - prune;
      double sum = 0.0;
      for (int m = s; m < e; m++) {
        const float f = row[m];
        if (f >= cutoff) sum += static_cast<double>(ExpTerm(f - mx));
      }
      out[static_cast<size_t>(t) * out_stride + j] =
          static_cast<float>(static_cast<double>(mx) + LogOfSum(sum));
    }
  }
}

// Same, the row of per-Gaussian log-likelihoods staged in LDS first (read once, coalesced;
// above, every lane walks its own pdf's Gaussians with 20-byte strides).
constexpr int kLseLdsFloats = 12288;
__global__ void __launch_bounds__(kThreads)
GmmPdfLseRowKernel(const float *__restrict__ ll, int T, int ll_stride, int num_mix,
                   const int32_t *__restrict__ pdf_offsets, int num_pdfs, float prune,
                   float min_log_diff, float *__restrict__ out, int out_stride) {
  __shared__ float row[kLseLdsFloats];
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const float *src = ll + static_cast<size_t>(t) * ll_stride;
    for (int m = threadIdx.x; m < num_mix; m += kThreads) row[m] = src[m];
    __syncthreads();
    for (int j = threadIdx.x; j < num_pdfs; j += kThreads) {
      const int s = pdf_offsets[j], e = pdf_offsets[j + 1];
      float mx = -INFINITY;
      for (int m = s; m < e; m++) mx = fmaxf(mx, row[m]);
      float cutoff = mx + min_log_diff;
      if (prune > 0.0f && mx - prune > cutoff) cutoff = mx - prune;
      double sum = 0.0;
      for (int m = s; m < e; m++) {
        const float f = row[m];
        if (f >= cutoff) sum += static_cast<double>(ExpTerm(f - mx));
      }
      out[static_cast<size_t>(t) * out_stride + j] = static_cast<float>(static_cast<double>(mx) + LogOfSum(sum));
    }
    __syncthreads();
  }
}

template <int DP>
int LaunchLoglikes(const float *data, KhMatrixDim dd, const float *g,
                   const float *mi, const float *iv, int M, float *out,
                   int out_stride) {
  const int frame_blocks = DivUp(dd.rows, 64 * (kThreads / 64));
  // split the Gaussians over blockIdx.y until the chip is filled
  int my = 1;
  const int tiles_m = DivUp(M, kTileM);
  while (frame_blocks * my < NumCUs() * 4 && my < tiles_m) my *= 2;
  if (my > tiles_m) my = tiles_m;
  const int m_per_block = DivUp(tiles_m, my) * kTileM;
  my = DivUp(M, m_per_block);
  hipLaunchKernelGGL(GmmLoglikesKernel<DP>, dim3(frame_blocks, my), dim3(kThreads),
                     0, Stream(), data, dd.rows, dd.cols, dd.stride, g, mi, iv, M,
                     out, out_stride, m_per_block);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// Fused frame x pdf scores: the two products of DiagGmm::LogLikelihoods
// (diag-gmm.cc:546-562) on the matrix cores AND the per-pdf LogSumExp
// (kaldi-vector.cc:745-763) in one kernel, so that the T x #Gaussians matrix
// (7.2 GB for 200 k frames of cfg 2) never reaches HBM.
//
// A workgroup owns 64 frames, whose [x | x^2] MFMA operands stay in registers, and walks
// the Gaussians in tiles of <= 128 that hold WHOLE pdfs (tile list built on the host).
// Per tile: means_invvars / inv_vars / gconsts of the tile -> LDS ([k][gaussian] image,
// conflict-free ds_read_b32 fragments), two v_mfma_f32_32x32x2_f32 accumulations
// (k-ordered fmaf chains, as the unfused path), ll = (a1 + g) + (-0.5 a2) -> LDS
// [frame][gaussian], then one lane per (frame, pdf): max, cutoff, double sum of ExpTerm, LogOfSum.
// Same operations in the same order as kh_diag_gmm_loglikes + GmmPdfLseRowKernel: the
// results are bit-identical to the unfused path.
// Measured (200 k frames, cfg 2): 5.0 ms.  History: 6.2 ms = matrix cores 2.2 ms (their floor: 2 x 200k x
// 9000 x 40 MAC at the fp32 MFMA rate) + LogSumExp 2.7 ms + staging / barriers 1.4 ms, phases switched
// off one at a time; the LogSumExp phase was LDS latency (a dependent read per Gaussian, twice): chunks
// of 8 independent reads -> 5.4 ms; 8 waves per workgroup (4 per SIMD with the CU's second workgroup, so
// one workgroup's LogSumExp runs under the other's MFMAs) -> 5.2 ms; the tile list split over
// blockIdx.y so that the last round of workgroups is short -> 5.0 ms.
namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kFT = 64, kGT = 128, kGTP = kGT + 5, kOTP = kGT + 1;  // kGTP odd: the transposing tile stores spread over all banks
#ifndef KH_GMM_WAVES
#define KH_GMM_WAVES 8
#endif
constexpr int kGW = KH_GMM_WAVES, kGThreads = 64 * kGW, kGJ = 8 / kGW;  // waves per workgroup; 32-column MFMA tiles per wave (2 x 4 tiles of 32 x 32 cover 64 frames x 128 Gaussians)
static_assert(kGW == 4 || kGW == 8, "waves");

struct GmmTile { int32_t m_begin, m_end, pdf_begin, pdf_end; };

// (__launch_bounds__'s second argument is WAVES PER SIMD under hipcc, not workgroups per CU: with "2" the 40-dimensional
// instantiation took 166 registers and ONE 8-wave workgroup fitted a CU — nothing ran under a workgroup's LogSumExp
// phase; "4" = 128 registers = two workgroups, 77 KB of LDS each: 5.1 -> 3.9 ms together with the 16-byte loads.)
template <int KS>
__global__ void __launch_bounds__(kGThreads, 4)
GmmFusedPdfKernel(const float *__restrict__ data, int T, int D, int data_stride, const float *__restrict__ gconsts,
                  const float *__restrict__ mi, const float *__restrict__ iv, const int32_t *__restrict__ pdf_offsets,
                  const GmmTile *__restrict__ tiles, int n_tiles, float prune, float min_log_diff,
                  float *__restrict__ out, int out_stride) {
  __shared__ float Bmi[2 * KS][kGTP];
  __shared__ float Biv[2 * KS][kGTP];
  __shared__ float Bg[kGT];
  __shared__ int Po[2][kGT + 1];  // the tile's pdf boundaries, relative to its first Gaussian (double buffered: the
                                  // next tile's are stored while slow waves still read this tile's)
  __shared__ float Ot[kFT][kOTP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / (kGW / 2), wn = wave % (kGW / 2), kk = lane >> 5, l31 = lane & 31;
  const int t0 = blockIdx.x * kFT;
  // this wave's 32 frames as MFMA A operands: lane (l31, kk) holds x[frame l31][2 s + kk]
  float ax[KS], axx[KS];
  {
    const int fr = t0 + wm * 32 + l31;
#pragma unroll
    for (int s = 0; s < KS; s++) {
      const int k = 2 * s + kk;
      const float v = (fr < T && k < D) ? data[static_cast<size_t>(fr) * data_stride + k] : 0.f;
      ax[s] = v;
      axx[s] = v * v;  // data_sq.ApplyPow(2.0)
    }
  }
  // The tile's parameters travel global -> registers -> LDS, and the NEXT tile's are loaded
  // into the registers while this tile computes (the staging loop used to cost ~20 dependent
  // L2 round trips per tile: 21 us per tile against 2 us of MFMA work).
  // A tile's means_invvars / inv_vars rows are ONE contiguous run of nm x D floats: a lane fetches it as 16-byte pieces
  // (4-byte aligned: global_load_dwordx4 in unaligned-access mode) — 6 vector-memory instructions per wave and tile
  // instead of 20 dword loads.  (A vector-memory instruction costs the SIMD ~70 cycles of issue during which no MFMA
  // starts, tools/gemm_lab.hip: the 22 loads of a tile stood against its 40 MFMAs.)  Where a piece's four elements
  // land in the transposed LDS image [k][gaussian] does not depend on the tile: computed once.
  struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };
  constexpr int kF4 = (kGT * 2 * KS / 4 + kGThreads - 1) / kGThreads;   // 16-byte pieces per lane and array
  uint32_t dst[kF4][2];   // LDS word offsets of a piece's four elements, 16 bits each; 0xFFFF = beyond the tile
#pragma unroll
  for (int j = 0; j < kF4; j++) {
    uint32_t o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int flat = 4 * (t + kGThreads * j) + c;
      const int m = flat / D, k = flat - m * D;
      o[c] = m < kGT ? static_cast<uint32_t>(k * kGTP + m) : 0xFFFFu;
    }
    dst[j][0] = o[0] | (o[1] << 16);
    dst[j][1] = o[2] | (o[3] << 16);
  }
  {  // rows k >= D of the LDS images are never written: zero once
    float *zmi = &Bmi[0][0], *ziv = &Biv[0][0];
    for (int i = t; i < 2 * KS * kGTP; i += kGThreads) { zmi[i] = 0.f; ziv[i] = 0.f; }
    __syncthreads();
  }
  F4 rmi[kF4], riv[kF4];
  float rg = 0.f;
  int rp = 0;
  auto load_tile = [&](const GmmTile &tl) {
    const int nm = tl.m_end - tl.m_begin, nmD = nm * D;
    const float *pmi = mi + static_cast<size_t>(tl.m_begin) * D, *piv = iv + static_cast<size_t>(tl.m_begin) * D;
#pragma unroll
    for (int j = 0; j < kF4; j++) {
      const int f0 = 4 * (t + kGThreads * j);
      F4 a{0.f, 0.f, 0.f, 0.f}, b{0.f, 0.f, 0.f, 0.f};
      if (f0 + 4 <= nmD) {
        a = *reinterpret_cast<const F4 *>(pmi + f0);
        b = *reinterpret_cast<const F4 *>(piv + f0);
      } else if (f0 < nmD) {   // the run's last piece (one lane per tile): element by element, nothing read beyond it
        a.x = pmi[f0]; b.x = piv[f0];
        if (f0 + 1 < nmD) { a.y = pmi[f0 + 1]; b.y = piv[f0 + 1]; }
        if (f0 + 2 < nmD) { a.z = pmi[f0 + 2]; b.z = piv[f0 + 2]; }
      }
      rmi[j] = a;
      riv[j] = b;
    }
    rg = (t < kGT && t < nm) ? gconsts[tl.m_begin + t] : 0.f;
    rp = (t <= tl.pdf_end - tl.pdf_begin) ? pdf_offsets[tl.pdf_begin + t] - tl.m_begin : 0;
  };
  // blockIdx.y = which share of the tile list: the units of work are short enough that the last round of
  // workgroups does not leave most of the chip idle (3125 frame blocks on 512 slots = 6.1 rounds)
  const int ti_begin = static_cast<int>(static_cast<long long>(n_tiles) * blockIdx.y / gridDim.y);
  const int ti_end = static_cast<int>(static_cast<long long>(n_tiles) * (blockIdx.y + 1) / gridDim.y);
  if (ti_begin >= ti_end) return;
  GmmTile tl = tiles[ti_begin];
  load_tile(tl);
  for (int ti = ti_begin; ti < ti_end; ti++) {
    const int nm = tl.m_end - tl.m_begin;
    (void)nm;
    // ---- parameters of the tile -> LDS, transposed to [k][gaussian]; zero padding
    {
      float *bmi = &Bmi[0][0], *biv = &Biv[0][0];
#pragma unroll
      for (int j = 0; j < kF4; j++) {
        const uint32_t o0 = dst[j][0] & 0xFFFFu, o1 = dst[j][0] >> 16, o2 = dst[j][1] & 0xFFFFu, o3 = dst[j][1] >> 16;
        if (o0 != 0xFFFFu) { bmi[o0] = rmi[j].x; biv[o0] = riv[j].x; }
        if (o1 != 0xFFFFu) { bmi[o1] = rmi[j].y; biv[o1] = riv[j].y; }
        if (o2 != 0xFFFFu) { bmi[o2] = rmi[j].z; biv[o2] = riv[j].z; }
        if (o3 != 0xFFFFu) { bmi[o3] = rmi[j].w; biv[o3] = riv[j].w; }
      }
    }
    if (t < kGT) Bg[t] = rg;
    if (t <= kGT) Po[ti & 1][t] = rp;
    __syncthreads();  // (also: the previous tile's LogSumExp has finished reading Ot and Po)
    const GmmTile cur = tl;
    if (ti + 1 < ti_end) {
      tl = tiles[ti + 1];
      load_tile(tl);
    }
    f32x16 a1[kGJ], a2[kGJ];
#pragma unroll
    for (int j = 0; j < kGJ; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) { a1[j][r] = 0.f; a2[j][r] = 0.f; }
#pragma unroll
    for (int s = 0; s < KS; s++) {
      const int k = 2 * s + kk;
#pragma unroll
      for (int j = 0; j < kGJ; j++) {
        const int col = (wn * kGJ + j) * 32 + l31;
        a1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s], Bmi[k][col], a1[j], 0, 0, 0);
        a2[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(axx[s], Biv[k][col], a2[j], 0, 0, 0);
      }
    }
    // loglikes = gconsts + data * means_invvars^T; loglikes += -0.5 * data_sq * inv_vars^T
#pragma unroll
    for (int j = 0; j < kGJ; j++) {
      const int col = (wn * kGJ + j) * 32 + l31;
      const float g = Bg[col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
        Ot[row][col] = (a1[j][r] + g) + (-0.5f * a2[j][r]);
      }
    }
    __syncthreads();
    // ---- LogSumExp per (frame, pdf) of the tile: lane = frame, the waves share the pdfs - the
    // pdf's Gaussian range is wave-uniform (no divergence, no integer division), the 64 lanes
    // read 64 different rows of Ot (conflict-free: row pitch 129)
    const int np = cur.pdf_end - cur.pdf_begin;
    const bool row_ok = t0 + lane < T;
    float *orow = out + static_cast<size_t>(t0 + lane) * out_stride + cur.pdf_begin;
    // The pdf's scores in chunks of kLC registers: the LDS reads of a chunk are independent and go
    // out together (a loop "read, wait, fmax" per Gaussian was 10 dependent LDS round trips per pdf:
    // the LogSumExp phase was bound by that latency, 2.7 of the kernel's 6.2 ms; two pdfs per wave in
    // flight on top of that measured slower).  The ranges are wave-uniform; the maximum does not depend on the order, the
    // double sum keeps the Gaussian order.
    constexpr int kLC = 8;
    auto finish = [&](int sidx, int eidx, const float (&v0)[kLC]) -> float {
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < kLC; j++) mx = fmaxf(mx, sidx + j < eidx ? v0[j] : -INFINITY);
      for (int m0 = sidx + kLC; m0 < eidx; m0 += kLC) {
        float v[kLC];
#pragma unroll
        for (int j = 0; j < kLC; j++) v[j] = Ot[lane][min(m0 + j, kGT - 1)];
#pragma unroll
        for (int j = 0; j < kLC; j++) mx = fmaxf(mx, m0 + j < eidx ? v[j] : -INFINITY);
      }
      float cutoff = mx + min_log_diff;
      if (prune > 0.0f && mx - prune > cutoff) cutoff = mx - prune;
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < kLC; j++)
        if (sidx + j < eidx && v0[j] >= cutoff) sum += static_cast<double>(ExpTerm(v0[j] - mx));
      for (int m0 = sidx + kLC; m0 < eidx; m0 += kLC) {
        float v[kLC];
#pragma unroll
        for (int j = 0; j < kLC; j++) v[j] = Ot[lane][min(m0 + j, kGT - 1)];
#pragma unroll
        for (int j = 0; j < kLC; j++)
          if (m0 + j < eidx && v[j] >= cutoff) sum += static_cast<double>(ExpTerm(v[j] - mx));
      }
      return static_cast<float>(static_cast<double>(mx) + LogOfSum(sum));
    };
    for (int pj = wave; pj < np; pj += kGW) {
      const int sa = Po[ti & 1][pj], ea = Po[ti & 1][pj + 1];
      float va[kLC];
#pragma unroll
      for (int j = 0; j < kLC; j++) va[j] = Ot[lane][min(sa + j, kGT - 1)];
      const float ra = finish(sa, ea, va);
      if (row_ok) orow[pj] = ra;
    }
    // (the next tile's parameter load only touches Bmi / Biv / Bg: no barrier needed here)
  }
}

// Tile list: consecutive whole pdfs, <= kGT Gaussians per tile.  Returns false if a single
// pdf has more than kGT Gaussians (the caller then takes the unfused path).
bool BuildGmmTiles(const std::vector<int32_t> &off, std::vector<GmmTile> *tiles) {
  const int P = static_cast<int>(off.size()) - 1;
  int p = 0;
  while (p < P) {
    GmmTile tl{off[p], off[p], p, p};
    while (tl.pdf_end < P && off[tl.pdf_end + 1] - tl.m_begin <= kGT) {
      tl.pdf_end++;
      tl.m_end = off[tl.pdf_end];
    }
    if (tl.pdf_end == p) return false;
    tiles->push_back(tl);
    p = tl.pdf_end;
  }
  return true;
}

template <int KS>
int LaunchFused(const float *data, KhMatrixDim dd, const float *g, const float *mi, const float *iv,
                const int32_t *pdf_offsets, const GmmTile *d_tiles, int n_tiles, float prune, float min_log_diff,
                float *out, int out_stride) {
  const int blocks = DivUp(dd.rows, kFT);
  int split = DivUp(16 * 2 * NumCUs(), blocks);   // >= 16 rounds of the 2 x #CU resident workgroups
  if (const char *e = getenv("KH_GMM_SPLIT")) split = atoi(e);
  split = std::max(1, std::min(std::min(split, 8), n_tiles));
  hipLaunchKernelGGL(GmmFusedPdfKernel<KS>, dim3(blocks, split), dim3(kGThreads), 0, Stream(), data, dd.rows, dd.cols,
                     dd.stride, g, mi, iv, pdf_offsets, d_tiles, n_tiles, prune, min_log_diff, out, out_stride);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
}  // namespace

namespace {
// data_sq = data; data_sq.ApplyPow(2.0) (diag-gmm.cc:552-553), packed to a stride of 4 floats
__global__ void SquareKernel(float *__restrict__ y, int y_stride, const float *__restrict__ x, int x_stride, int rows, int cols) {
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x) {
      const float v = x[static_cast<size_t>(r) * x_stride + c];
      y[static_cast<size_t>(r) * y_stride + c] = v * v;
    }
}
}  // namespace

extern "C" {

// HOST: DiagGmm::ComputeGconsts gmm/diag-gmm.cc:114-152
int kh_gmm_compute_gconsts(const float *weights, const float *means_invvars,
                           const float *inv_vars, int num_mix, int dim,
                           float *gconsts) {
  KH_CHECK_ARG(weights && means_invvars && inv_vars && gconsts && num_mix > 0 && dim > 0);
  const double kLog2Pi = 1.8378770664093454835606594728112;
  const float offset = -0.5 * kLog2Pi * dim;
  int num_bad = 0;
  for (int mix = 0; mix < num_mix; mix++) {
    KH_CHECK_ARG(weights[mix] >= 0);  // KALDI_ASSERT :125
    float gc = logf(weights[mix]) + offset;
    for (int d = 0; d < dim; d++) {
      const float ivv = inv_vars[static_cast<size_t>(mix) * dim + d];
      const float miv = means_invvars[static_cast<size_t>(mix) * dim + d];
      gc += 0.5 * logf(ivv) - 0.5 * miv * miv / ivv;
    }
    if (std::isnan(gc)) {
      SetError("At component %d, not a number in gconst computation", mix);
      return KH_EINVAL;
    }
    if (std::isinf(gc)) {
      num_bad++;
      if (gc > 0) gc = -gc;
    }
    gconsts[mix] = gc;
  }
  return num_bad;
}

int kh_diag_gmm_loglikes(const float *data, KhMatrixDim dd, const float *gconsts,
                         const float *means_invvars, const float *inv_vars,
                         int num_mix, float *loglikes, int ll_stride) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(data && gconsts && means_invvars && inv_vars && loglikes);
  KH_CHECK_ARG(dd.rows > 0 && dd.cols > 0 && dd.stride >= dd.cols && num_mix > 0 &&
               ll_stride >= num_mix);  // KALDI_ASSERT(data.NumRows() != 0) :548
  const int D = dd.cols;
  // Large problems: the reference's own formulation (diag-gmm.cc:546-562) as two MFMA
  // GEMMs, loglikes = gconsts + data * means_invvars^T, then += -0.5 * data^2 * inv_vars^T
  // (same k-ordered accumulation as the register kernel below, ~3x its rate).
  if (static_cast<int64_t>(dd.rows) * num_mix >= (1 << 22) && !getenv("KH_GMM_NO_GEMM")) {
    const int sq_stride = (D + 3) & ~3;
    float *sq = static_cast<float *>(PoolMalloc(sizeof(float) * static_cast<size_t>(dd.rows) * sq_stride));
    if (!sq) return KH_ENOMEM;
    hipLaunchKernelGGL(SquareKernel, dim3(1, std::min(dd.rows, NumCUs() * 32)), dim3(64), 0, Stream(), sq, sq_stride, data,
                       dd.stride, dd.rows, D);
    const KhMatrixDim dsq{dd.rows, D, sq_stride}, dpar{num_mix, D, D}, dll{dd.rows, num_mix, ll_stride};
    rc = kh_affine(data, dd, means_invvars, dpar, gconsts, loglikes, dll);
    if (!rc) rc = kh_add_mat_mat(-0.5f, sq, dsq, 0, inv_vars, dpar, 1, 1.0f, loglikes, dll);
    hipError_t e = hipStreamSynchronize(Stream());
    PoolFree(sq);
    if (!rc && e != hipSuccess) { SetError("kh_diag_gmm_loglikes: %s", hipGetErrorString(e)); rc = KH_EDEVICE; }
    return rc;
  }
  if (D <= 16) return LaunchLoglikes<16>(data, dd, gconsts, means_invvars, inv_vars, num_mix, loglikes, ll_stride);
  if (D <= 32) return LaunchLoglikes<32>(data, dd, gconsts, means_invvars, inv_vars, num_mix, loglikes, ll_stride);
  if (D <= 40) return LaunchLoglikes<40>(data, dd, gconsts, means_invvars, inv_vars, num_mix, loglikes, ll_stride);
  if (D <= 64) return LaunchLoglikes<64>(data, dd, gconsts, means_invvars, inv_vars, num_mix, loglikes, ll_stride);
  if (D <= 96) return LaunchLoglikes<96>(data, dd, gconsts, means_invvars, inv_vars, num_mix, loglikes, ll_stride);
  SetError("kh_diag_gmm_loglikes: feature dimension %d > 96 not supported", D);
  return KH_EINVAL;
}

int kh_am_gmm_loglikes(const float *data, KhMatrixDim dd, const float *gconsts,
                       const float *means_invvars, const float *inv_vars,
                       const int32_t *pdf_offsets, int num_pdfs, int num_mix,
                       float log_sum_exp_prune, float *out, int out_stride) {
  int rc = EnsureDevice();
  if (rc) return rc;
  KH_CHECK_ARG(pdf_offsets && out && num_pdfs > 0 && out_stride >= num_pdfs);
  KH_CHECK_ARG(data && gconsts && means_invvars && inv_vars && dd.cols > 0 && dd.stride >= dd.cols && num_mix > 0);
  if (dd.rows <= 0) {  // DiagGmm::LogLikelihoods, diag-gmm.cc:548
    SetError("KALDI_ASSERT: data.NumRows() != 0");
    return KH_EINVAL;
  }
  const float min_log_diff_f = logf(FLT_EPSILON);  // kMinLogDiffFloat kaldi-math.h:121
  // The pdfs' Gaussian ranges: strictly increasing from 0 to num_mix (a DiagGmm has no empty mixture).  Both
  // paths below index with them unchecked - the fused kernel's boundary array holds kGT + 1 entries per tile.
  std::vector<int32_t> h_off(num_pdfs + 1);
  KH_HIP(hipMemcpyAsync(h_off.data(), pdf_offsets, sizeof(int32_t) * (num_pdfs + 1), hipMemcpyDeviceToHost, Stream()));
  KH_HIP(hipStreamSynchronize(Stream()));
  if (h_off[0] != 0) {
    SetError("kh_am_gmm_loglikes: pdf_offsets[0] = %d: pdf 0 does not start at Gaussian 0", h_off[0]);
    return KH_EINVAL;
  }
  for (int j = 0; j < num_pdfs; j++)
    if (h_off[j + 1] <= h_off[j]) {
      SetError("kh_am_gmm_loglikes: pdf %d is empty or runs backwards (pdf_offsets %d .. %d)", j, h_off[j], h_off[j + 1]);
      return KH_EINVAL;
    }
  if (h_off[num_pdfs] != num_mix) {
    SetError("kh_am_gmm_loglikes: pdf %d ends at Gaussian %d, the model has %d", num_pdfs - 1, h_off[num_pdfs], num_mix);
    return KH_EINVAL;
  }
  // Fused path (matrix cores + LogSumExp epilogue, nothing of T x #Gaussians in HBM) whenever
  // the problem is large enough for the tiles to fill the chip and every pdf fits a tile.
  if (dd.cols <= 40 && static_cast<int64_t>(dd.rows) * num_mix >= (1 << 22) && !getenv("KH_GMM_NO_FUSION") &&
      !getenv("KH_GMM_NO_GEMM")) {
    std::vector<GmmTile> tiles;
    if (BuildGmmTiles(h_off, &tiles)) {
      GmmTile *d_tiles = static_cast<GmmTile *>(PoolMalloc(sizeof(GmmTile) * tiles.size()));
      if (!d_tiles) return KH_ENOMEM;
      KH_HIP(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(GmmTile) * tiles.size(), hipMemcpyHostToDevice, Stream()));
      const int nt = static_cast<int>(tiles.size());
      if (dd.cols <= 16) rc = LaunchFused<8>(data, dd, gconsts, means_invvars, inv_vars, pdf_offsets, d_tiles, nt, log_sum_exp_prune, min_log_diff_f, out, out_stride);
      else rc = LaunchFused<20>(data, dd, gconsts, means_invvars, inv_vars, pdf_offsets, d_tiles, nt, log_sum_exp_prune, min_log_diff_f, out, out_stride);
      hipError_t e = hipStreamSynchronize(Stream());  // the tile list returns to the pool; the host copy goes out of scope
      PoolFree(d_tiles);
      if (!rc && e != hipSuccess) { SetError("kh_am_gmm_loglikes: %s", hipGetErrorString(e)); rc = KH_EDEVICE; }
      return rc;
    }
  }
  const int ll_stride = (num_mix + 3) & ~3;
  // Bound the scratch: process frames in slabs of at most ~1 GiB of T x M.
  const int64_t slab_rows = std::max<int64_t>(64, (int64_t(1) << 28) / ll_stride);
  const int T = dd.rows;
  float *scratch = static_cast<float *>(
      PoolMalloc(sizeof(float) * std::min<int64_t>(T, slab_rows) * ll_stride));
  if (!scratch) return KH_ENOMEM;
  const float min_log_diff = logf(FLT_EPSILON);  // kMinLogDiffFloat kaldi-math.h:121
  for (int64_t r0 = 0; r0 < T; r0 += slab_rows) {
    const int rows = static_cast<int>(std::min<int64_t>(slab_rows, T - r0));
    KhMatrixDim ds{rows, dd.cols, dd.stride};
    rc = kh_diag_gmm_loglikes(data + r0 * dd.stride, ds, gconsts, means_invvars,
                              inv_vars, num_mix, scratch, ll_stride);
    if (rc) break;
    int gx = DivUp(num_pdfs, kThreads);
    int gy = rows;
    const int cap = NumCUs() * 16 / gx;
    if (gy > cap) gy = cap > 0 ? cap : 1;
    if (num_mix <= kLseLdsFloats && num_mix >= 1024)
      hipLaunchKernelGGL(GmmPdfLseRowKernel, dim3(std::min(rows, NumCUs() * 12)), dim3(kThreads), 0, Stream(),
                         scratch, rows, ll_stride, num_mix, pdf_offsets, num_pdfs, log_sum_exp_prune, min_log_diff,
                         out + r0 * out_stride, out_stride);
    else
      hipLaunchKernelGGL(GmmPdfLseKernel, dim3(gx, gy), dim3(kThreads), 0, Stream(),
                         scratch, rows, ll_stride, pdf_offsets, num_pdfs,
                         log_sum_exp_prune, min_log_diff, out + r0 * out_stride,
                         out_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      SetError("GmmPdfLseKernel launch failed: %s", hipGetErrorString(e));
      rc = KH_EDEVICE;
      break;
    }
  }
  KH_HIP(hipStreamSynchronize(Stream()));  // scratch returns to the pool
  PoolFree(scratch);
  return rc;
}

}  // extern "C"
