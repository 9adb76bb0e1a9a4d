/* kaldi_hip.h — C-ABI of libkaldi_hip.so: the MI355X (gfx950) implementation of
 * Kaldi's acoustic-scoring + lattice-decoding hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no torch / C++
 * types.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference's src/).  Unless stated otherwise pointers
 * are DEVICE pointers, matrices are row-major float32 described by KhMatrixDim
 * (the reference's MatrixDim, cudamatrix/cu-matrixdim.h:49-53, stride in
 * elements), work is enqueued on the library's current HIP stream
 * (kh_set_stream) and — like the reference, whose CU_SAFE_CALL synchronises
 * after every call (cudamatrix/cu-common.h:37-44) — results are visible to the
 * host after kh_synchronize() or any kh_* call documented as synchronous.
 *
 * Error convention: functions return 0 on success and a negative KH_E* code on
 * failure; kh_last_error() returns the message.  The C++ host layer
 * (old-kaldi-git_amd/host/) turns a failure into std::runtime_error exactly as
 * KALDI_ERR does (base/kaldi-error.cc:143,179-182).  There is NO CPU fallback
 * in this library: if no gfx950 device is usable every compute call fails.
 */
#ifndef KALDI_HIP_H_
#define KALDI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_OK 0
#define KH_EINVAL (-1)  /* dimension / argument violation (KALDI_ASSERT) */
#define KH_EDEVICE (-2) /* HIP runtime failure (CU_SAFE_CALL) */
#define KH_ENOMEM (-3)
#define KH_ESTATE (-4)   /* call sequence violation */
#define KH_ECAPACITY (-5) /* a decoder arena overflowed; see message */
#define KH_ETIMEOUT (-6)  /* a wait for the device ran past its deadline (serving kernel); kh_last_error() holds the streams' state */

/* cudamatrix/cu-matrixdim.h:49-53 */
typedef struct KhMatrixDim {
  int32_t rows;
  int32_t cols;
  int32_t stride;
} KhMatrixDim;

/* ------------------------------------------------------------------ runtime
 * Replaces CuDevice (cudamatrix/cu-device.h:41-143, cu-device.cc). */
const char *kh_last_error(void);
/* cudaGetDeviceCount in SelectGpuId, cu-device.cc:93-192. */
int kh_device_count(void);
/* CuDevice::SelectGpuId with an explicit ordinal (needed for
 * one-process-per-GPU sharding).  ordinal < 0: keep the current device. */
int kh_select_gpu(int ordinal);
/* CuDevice::Enabled() cu-device.h:87 */
int kh_enabled(void);
/* CuDevice::DeviceGetName / GetFreeMemory cu-device.cc:391-397,195-225 */
int kh_device_name(char *buf, size_t len);
int kh_mem_info(size_t *free_bytes, size_t *total_bytes);
/* Use an externally owned hipStream_t (e.g. torch's current stream) for all
 * subsequent launches; NULL = the library's own stream. */
int kh_set_stream(void *hip_stream);
void *kh_get_stream(void);
int kh_synchronize(void);
/* CuDevice::Malloc / MallocPitch / Free cu-device.cc:530-555.  Served from a
 * caching pool (the reference allocates on every Resize).  Pitch is a multiple
 * of 256 bytes. */
void *kh_malloc(size_t bytes);
void *kh_malloc_pitch(size_t row_bytes, size_t num_rows, size_t *pitch_bytes);
int kh_free(void *ptr);
int kh_pool_release(void); /* return cached blocks to the driver */
/* cudaMemcpy2D H2D / D2H / D2D in CuMatrix::CopyFromMat / CopyToMat / Swap
 * cu-matrix.cc:112-147,197-231,283-307,387-412.  Synchronous. kind: 0 H2D,
 * 1 D2H, 2 D2D. Pitches and width in bytes. */
int kh_memcpy_2d(void *dst, size_t dst_pitch, const void *src, size_t src_pitch,
                 size_t width_bytes, size_t height, int kind);
int kh_memset(void *dst, int value, size_t bytes);

/* ------------------------------------------------------------------ a1
 * CuMatrixBase::AddMatMat cu-matrix.cc:947-982 (cublas_gemm
 * cublas-wrappers.h:28-33): C = alpha*op(A)*op(B) + beta*C, FP32 MFMA.
 * transX != 0 means kTrans.  dA/dB describe A/B as stored. */
int kh_add_mat_mat(float alpha, const float *A, KhMatrixDim dA, int transA,
                   const float *B, KhMatrixDim dB, int transB, float beta,
                   float *C, KhMatrixDim dC);
/* Fused affine layer: C = A * W^T + bias (row broadcast).  Equals
 * CopyRowsFromVec + AddMatMat(beta=1) (AffineComponent::Propagate
 * nnet2/nnet-component.cc:1221-1223) and AddMatMat(beta=0) + AddVecToRows
 * (FixedAffineComponent::Propagate :3340-3342). */
int kh_affine(const float *A, KhMatrixDim dA, const float *W, KhMatrixDim dW,
              const float *bias, float *C, KhMatrixDim dC);
/* AffineComponent::Propagate (nnet-component.cc:1219-1224) followed by PnormComponent::Propagate with p = 2
 * (:386-391, CuMatrixBase::GroupPnorm cu-matrix.cc:1037-1057) in one kernel: Y[r][c] = sqrt(sum_j x_j^2), x = row r of
 * A * W^T + bias, j over columns c*group_size .. (c+1)*group_size-1 in order; bit-identical to kh_affine followed by
 * kh_group_pnorm(power = 2).  dW.rows = dY.cols * group_size; kh_affine_pnorm_supported(group_size) says whether
 * the group size is one the kernel tiles (a divisor of 160); KH_EINVAL otherwise. */
int kh_affine_pnorm(const float *A, KhMatrixDim dA, const float *W, KhMatrixDim dW, const float *bias, float *Y,
                    KhMatrixDim dY, int group_size);
int kh_affine_pnorm_supported(int group_size);

/* ------------------------------------------------------------------ a2
 * cudaF_softmax_reduce / CuMatrixBase::ApplySoftMaxPerRow cu-matrix.cc:1251-1271.
 * d describes y; x has stride src_stride.
 * In place (y == x with src_stride == d.stride) is supported, as with the reference's kernel, for both functions, every
 * width and both element types: each kernel finishes a row's max and sum reductions before it stores to that row,
 * and the store pass reads an element in the thread that then writes that index.  y and x that overlap in any other
 * way are not. */
int kh_softmax_per_row(float *y, const float *x, KhMatrixDim d, int src_stride);
/* cudaF_log_softmax_reduce / ApplyLogSoftMaxPerRow cu-matrix.cc:1274-1295 */
int kh_log_softmax_per_row(float *y, const float *x, KhMatrixDim d,
                           int src_stride);

/* ------------------------------------------------------------------ a3
 * cudaF_copy_rows / CuMatrixBase::CopyRows cu-matrix.cc:1965-1990:
 * dst[i,:] = idx[i] < 0 ? 0 : src[idx[i],:].  indices is a DEVICE array of
 * dst_dim.rows int32. */
int kh_copy_rows(float *dst, KhMatrixDim dst_dim, const float *src,
                 int src_stride, const int32_t *indices);

/* ------------------------------------------------------------------ a4
 * cudaF_splice / cu::Splice cudamatrix/cu-math.cc:130-165:
 * y[r, k*D + c] = x[clamp(r + off[k], 0, R-1), c].  frame_offsets: DEVICE int32. */
int kh_splice(float *y, KhMatrixDim d_out, const float *x, KhMatrixDim d_in,
              const int32_t *frame_offsets, int n_offsets);

/* ------------------------------------------------------------------ a5
 * cudaF_group_pnorm / CuMatrixBase::GroupPnorm cu-matrix.cc:1147-1164.
 * d describes y (rows x cols); x has cols*group_size columns. */
int kh_group_pnorm(float *y, const float *x, KhMatrixDim d, int src_stride,
                   int group_size, float power);

/* ------------------------------------------------------------------ a6
 * NormalizeComponent::Propagate nnet2/nnet-component.cc:576-588 fused:
 * y = x / sqrt(max(mean(x^2), 2^-66)).  */
int kh_normalize(float *y, const float *x, KhMatrixDim d, int src_stride);
/* cudaF_add_diag_mat_mat via CuVectorBase::AddDiagMat2 cu-vector.cc:517-580
 * (kNoTrans): v[i] = beta*v[i] + alpha * sum_j M[i,j]^2 */
int kh_add_diag_mat2(float alpha, const float *M, KhMatrixDim d, float beta,
                     float *v);
/* cudaF_mul_rows_vec / MulRowsVec cu-matrix.cc:693-713 */
int kh_mul_rows_vec(float *M, KhMatrixDim d, const float *scale);
/* cudaF_mul_cols_vec / MulColsVec cu-matrix.cc:668 */
int kh_mul_cols_vec(float *M, KhMatrixDim d, const float *scale);

/* ------------------------------------------------------------------ a7 */
/* cudaF_copy_rows_from_vec / CopyRowsFromVec cu-matrix.cc:1673-1745 */
int kh_copy_rows_from_vec(float *M, KhMatrixDim d, const float *v);
/* cudaF_add_vec_to_rows / AddVecToRows cu-matrix.cc:916-939 */
int kh_add_vec_to_rows(float alpha, const float *v, float beta, float *M,
                       KhMatrixDim d);
/* cudaF_apply_floor :1845, _apply_log :600, _apply_exp, _apply_pow, _scale :579 */
int kh_apply_floor(float *M, KhMatrixDim d, float floor_val);
int kh_apply_log(float *M, KhMatrixDim d);
int kh_apply_exp(float *M, KhMatrixDim d);
int kh_apply_pow(float *M, KhMatrixDim d, float power);
int kh_scale(float *M, KhMatrixDim d, float alpha);
/* cudaF_sum_column_ranges / SumColumnRanges cu-matrix.cc:1994-2028; ranges:
 * DEVICE array of 2*d.cols int32 ([start,end) per output column). */
int kh_sum_column_ranges(float *y, KhMatrixDim d, const float *x,
                         KhMatrixDim d_src, const int32_t *ranges);
/* cudaF_matrix_lookup / CuMatrixBase::Lookup cu-matrix.cc:2327: out[k] =
 * M[pairs[2k], pairs[2k+1]]; pairs/out DEVICE arrays. */
int kh_matrix_lookup(const float *M, KhMatrixDim d, const int32_t *pairs, int n,
                     float *out);
/* DecodableAmNnet epilogue decodable-am-nnet.h:60-69 fused:
 * M = (log(max(M, 1e-20)) - log_priors[c]) * prob_scale */
int kh_log_prior_scale(float *M, KhMatrixDim d, const float *log_priors,
                       float prob_scale);

/* ------------------------------------------------------------------ a1-a7, <double>
 * The CuMatrix<double> / CuVector<double> instantiation (cu-matrix.cc:2415-2418, cu-vector.cc) of the primitives above:
 * same argument meaning, double elements (strides in elements).  AddMatMat runs on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64).  csrc/kh_double.hip; the cudaD_* launchers of include/cu_kernels_ansi_hip.h forward here. */
int kh_add_mat_mat_d(double alpha, const double *A, KhMatrixDim dA, int transA, const double *B, KhMatrixDim dB,
                     int transB, double beta, double *C, KhMatrixDim dC);
int kh_softmax_per_row_d(double *y, const double *x, KhMatrixDim d, int src_stride);
int kh_log_softmax_per_row_d(double *y, const double *x, KhMatrixDim d, int src_stride);
int kh_copy_rows_d(double *dst, KhMatrixDim dst_dim, const double *src, int src_stride, const int32_t *indices);
int kh_splice_d(double *y, KhMatrixDim d_out, const double *x, KhMatrixDim d_in, const int32_t *frame_offsets,
                int n_offsets);
int kh_group_pnorm_d(double *y, const double *x, KhMatrixDim d, int src_stride, int group_size, double power);
int kh_add_diag_mat2_d(double alpha, const double *M, KhMatrixDim d, double beta, double *v);
int kh_mul_rows_vec_d(double *M, KhMatrixDim d, const double *scale);
int kh_mul_cols_vec_d(double *M, KhMatrixDim d, const double *scale);
int kh_copy_rows_from_vec_d(double *M, KhMatrixDim d, const double *v);
int kh_add_vec_to_rows_d(double alpha, const double *v, double beta, double *M, KhMatrixDim d);
int kh_apply_floor_d(double *M, KhMatrixDim d, double floor_val);
int kh_apply_log_d(double *M, KhMatrixDim d);
int kh_apply_exp_d(double *M, KhMatrixDim d);
int kh_apply_pow_d(double *M, KhMatrixDim d, double power);
int kh_scale_d(double *M, KhMatrixDim d, double alpha);
int kh_sum_column_ranges_d(double *y, KhMatrixDim d, const double *x, KhMatrixDim d_src, const int32_t *ranges);
int kh_matrix_lookup_d(const double *M, KhMatrixDim d, const int32_t *pairs, int n, double *out);

/* ------------------------------------------------------------------ a8
 * nnet2 forward: Nnet + NnetComputer + DecodableAmNnet
 * (nnet2/nnet-nnet.h, nnet2/nnet-compute.cc:63-108,159-166,
 * nnet2/decodable-am-nnet.h:37-98, online-nnet2-decodable.cc:81-142). */
enum KhComponentType {
  KH_SPLICE = 1,
  KH_FIXED_AFFINE = 2,
  KH_AFFINE = 3,
  KH_PNORM = 4,
  KH_NORMALIZE = 5,
  KH_SOFTMAX = 6,
  KH_SUM_GROUP = 7,
  KH_FIXED_SCALE = 8,
  KH_FIXED_BIAS = 9
};
/* HOST-side description of one component; parameters are HOST pointers and are
 * copied to the device by kh_nnet_add_component. */
typedef struct KhComponentDesc {
  int32_t type;
  int32_t input_dim;
  int32_t output_dim;
  const float *linear;    /* [output_dim x input_dim] row-major */
  const float *bias;      /* [output_dim]; scales/bias for FixedScale/FixedBias */
  const int32_t *context; /* splice context */
  int32_t n_context;
  int32_t const_dim;
  float p;
  const int32_t *sizes; /* sum-group sizes */
  int32_t n_sizes;
} KhComponentDesc;

typedef struct KhNnet KhNnet;
KhNnet *kh_nnet_create(void);
void kh_nnet_destroy(KhNnet *nnet);
int kh_nnet_add_component(KhNnet *nnet, const KhComponentDesc *desc);
int kh_nnet_set_priors(KhNnet *nnet, const float *priors_host, int n);
int kh_nnet_num_components(const KhNnet *nnet);
int kh_nnet_input_dim(const KhNnet *nnet);
int kh_nnet_output_dim(const KhNnet *nnet);
int kh_nnet_left_context(const KhNnet *nnet);  /* Nnet::LeftContext nnet-nnet.cc:45 */
int kh_nnet_right_context(const KhNnet *nnet); /* Nnet::RightContext :55 */
/* NnetComputation over a BATCH of utterances stacked by rows.
 * feats: [utt_row_offsets[n_utts] x input_dim]; utterance u owns rows
 * [utt_row_offsets[u], utt_row_offsets[u+1]) (HOST array, n_utts+1).
 * pad_input != 0: each utterance is padded by edge-frame duplication
 * (nnet-compute.cc:75-89) so it yields as many output rows as input rows and
 * out uses the same row offsets; pad_input == 0: utterance u yields
 * T_u - left - right rows, packed in order (out_row_offsets_host, if non-NULL,
 * receives n_utts+1 offsets).
 * epilogue: 0 = raw network output (NnetComputation); 1 = DecodableAmNnet's
 * floor, log, minus log prior, times prob_scale (requires kh_nnet_set_priors). */
int kh_nnet_compute(KhNnet *nnet, const float *feats, int feat_stride,
                    const int32_t *utt_row_offsets_host, int n_utts,
                    int pad_input, int epilogue, float prob_scale, float *out,
                    int out_stride, int32_t *out_row_offsets_host);
/* The same call returning as soon as its work is QUEUED on the library's stream: `out` is valid for work queued on that
 * stream behind it (or after a synchronisation), the handle keeps the call's activation buffers until its next call or its
 * destruction.  What lets a caller prepare the consumer of the output while the forward pass runs
 * (kh_discriminative_lattice_computations_parts; a binary that reads the next archive entry while the GPU works). */
int kh_nnet_compute_async(KhNnet *nnet, const float *feats, int feat_stride,
                    const int32_t *utt_row_offsets_host, int n_utts,
                    int pad_input, int epilogue, float prob_scale, float *out,
                    int out_stride, int32_t *out_row_offsets_host);

/* ------------------------------------------------------------------ a9
 * DiagGmm (gmm/diag-gmm.h:83-135). */
/* DiagGmm::ComputeGconsts gmm/diag-gmm.cc:114-152 — HOST arrays (model-load
 * time, as in the reference).  Returns number of bad gconsts (>= 0). */
int kh_gmm_compute_gconsts(const float *weights, const float *means_invvars,
                           const float *inv_vars, int num_mix, int dim,
                           float *gconsts);
/* DiagGmm::LogLikelihoods(const MatrixBase&, Matrix*) diag-gmm.cc:546-562:
 * loglikes[T x num_mix]. */
int kh_diag_gmm_loglikes(const float *data, KhMatrixDim d_data,
                         const float *gconsts, const float *means_invvars,
                         const float *inv_vars, int num_mix, float *loglikes,
                         int ll_stride);
/* Frame x pdf matrix (gmm-compute-likes.cc:70-77; DecodableAmDiagGmmUnmapped::
 * LogLikelihoodZeroBased decodable-am-diag-gmm.cc:28-71 for every (t,pdf)):
 * out[t,j] = LogSumExp_{m in pdf j}(loglike[t,m], prune), LogSumExp as
 * matrix/kaldi-vector.cc:745-763.  All pdfs' Gaussians concatenated;
 * pdf_offsets: DEVICE int32 [num_pdfs+1], strictly increasing from 0 to
 * num_mix (a DiagGmm has no empty mixture).  Every call copies them to the
 * host, waits for the stream and checks that: KH_EINVAL with a message naming
 * the pdf otherwise, before any kernel runs.  The call returns after its
 * kernels have finished (it synchronises the stream again at its end).
 * No frames (d_data.rows == 0): KH_EINVAL, "KALDI_ASSERT: data.NumRows() != 0"
 * (diag-gmm.cc:548). */
int kh_am_gmm_loglikes(const float *data, KhMatrixDim d_data,
                       const float *gconsts, const float *means_invvars,
                       const float *inv_vars, const int32_t *pdf_offsets,
                       int num_pdfs, int num_mix, float log_sum_exp_prune,
                       float *out, int out_stride);

/* ------------------------------------------------------------------ a10-a14
 * LatticeFasterDecoder (decoder/lattice-faster-decoder.{h,cc}) over a
 * device-resident HCLG, decoding a batch of utterances per call. */
typedef struct KhFst KhFst;
/* fst::Fst<StdArc> as read by ReadFstKaldi (nnet-latgen-faster.cc:108):
 * HOST CSR arrays; arc_offsets has num_states+1 entries; final[s] = +inf for
 * non-final states (TropicalWeight::Zero()).  Limits (NULL + kh_last_error otherwise):
 * num_states + #arcs with ilabel != 0 < 2^28 and #arcs with ilabel == 0 < 2^28 (the
 * device tables are addressed with 32-bit byte offsets, 16 bytes per state / arc);
 * device memory: 20 bytes per state and per emitting arc, 16 per epsilon arc, and
 * 16 more per state and emitting arc in every decoder created on the graph. */
KhFst *kh_fst_create(int32_t num_states, int32_t start,
                     const int64_t *arc_offsets, const int32_t *ilabel,
                     const int32_t *olabel, const float *weight,
                     const int32_t *nextstate, const float *final_cost);
void kh_fst_destroy(KhFst *fst);
int64_t kh_fst_num_arcs(const KhFst *fst);
/* Validates once per (graph, pdf map, model) what the reference asserts on every
 * DecodableAmNnet::LogLikelihood call (nnet2/decodable-am-nnet.h:76-78) /
 * TransitionModel::TransitionIdToPdf (hmm/transition-model.h:312): every ilabel of the
 * graph has an entry in the HOST copy of tid2pdf (NULL: identity minus one) and maps to a
 * column < num_cols of the log-likelihood matrix.  The decode kernels gather unchecked. */
int kh_fst_check_pdf_map(const KhFst *fst, const int32_t *tid2pdf_host, int n_tid2pdf, int num_cols);

/* LatticeFasterDecoderConfig lattice-faster-decoder.h:40-95 (same defaults). */
typedef struct KhDecoderConfig {
  float beam;             /* 16.0 */
  int32_t max_active;     /* INT32_MAX */
  int32_t min_active;     /* 200 */
  float lattice_beam;     /* 10.0 */
  int32_t prune_interval; /* 25 */
  float beam_delta;       /* 0.5 */
  float hash_ratio;       /* 2.0 (sizes the device token table) */
  float prune_scale;      /* 0.1 */
} KhDecoderConfig;
void kh_decoder_config_default(KhDecoderConfig *cfg);

typedef struct KhDecoder KhDecoder;
/* max_batch: utterances decoded concurrently per kh_decoder_decode call
 * (one workgroup each).  max_frames: longest utterance.  max_tokens_per_frame /
 * arena sizes derive from max_active; see DESIGN.md "Decoder memory". */
KhDecoder *kh_decoder_create(const KhFst *fst, const KhDecoderConfig *cfg,
                             int max_batch, int max_frames);
void kh_decoder_destroy(KhDecoder *dec);
/* LatticeFasterDecoder::Decode (lattice-faster-decoder.cc:77-95) for a batch:
 * loglikes is what DecodableAmNnet::LogLikelihood / DecodableMatrixScaledMapped
 * (decoder/decodable-matrix.h:33-84) would return: row t of utterance u at
 * utt_row_offsets[u] + t, column tid2pdf[ilabel] (tid2pdf: DEVICE int32 LUT
 * indexed by transition-id, TransitionModel::TransitionIdToPdf
 * hmm/transition-model.h:312; NULL = identity minus one, ilabel-1).
 * Includes FinalizeDecoding.  Synchronous. */
int kh_decoder_decode(KhDecoder *dec, const float *loglikes, int ll_stride,
                      const int32_t *utt_row_offsets_host, int n_utts,
                      const int32_t *tid2pdf);
/* Per-utterance statistics of the last kh_decoder_decode call. */
typedef struct KhDecodeStats {
  int32_t num_frames;
  int32_t reached_final;      /* ReachedFinal() lattice-faster-decoder.h:143 */
  float final_relative_cost;  /* FinalRelativeCost() */
  float final_best_cost;
  int32_t num_tokens;         /* surviving tokens (lattice states) */
  int32_t num_links;          /* surviving forward links (lattice arcs) */
  int64_t arcs_expanded;      /* emitting+epsilon arcs visited (roofline unit) */
  int64_t tokens_created;
  int32_t status;             /* 0 ok; else the kernel's code: 1-5 a token / link arena or a per-frame cap overflowed, 6 the lattice
                               * did not fit the pool (retried with the exact size), 7 survivor lists full, 8-9 the reference order's
                               * list could not be built, 10 internal inconsistency (a frame's epsilon links are not a DAG: the
                               * backward pruning's fixed point did not stop) - the getters return KH_ECAPACITY with the text */
  int32_t max_tokens_frame;
} KhDecodeStats;
int kh_decoder_get_stats(const KhDecoder *dec, int utt, KhDecodeStats *stats);
/* Same counters without building the lattice (num_tokens / num_links are then the
 * arena slots in use).  Measurement aid, no reference counterpart. */
int kh_decoder_get_counters(const KhDecoder *dec, int utt, KhDecodeStats *stats);
/* How the pruning schedule of the last kh_decoder_decode call treated utterance `utt` (measurement / test aid,
 * no reference counterpart): counters[0] garbage collections (PruneActiveTokens + full compaction when the
 * slot's arenas filled up), [1] frames FinalizeDecoding visited with the frame's extra_costs in LDS, [2] frames
 * it visited through the general routines (more than 12288 tokens), [3] frames whose extra_costs went to the
 * next visit through memory.  All zero under KH_DECODER_PRUNE_SCHEDULE=interval (PruneActiveTokens every
 * prune_interval frames, lattice-faster-decoder.cc:88-89); the lattice is the same either way. */
int kh_decoder_get_schedule_counters(const KhDecoder *dec, int utt, int32_t *counters);
/* enable != 0 (THE DEFAULT since round 6): kh_decoder_decode reproduces the reference's own ITERATION ORDER, so that tokens and
 * forward links are the ones LatticeFasterDecoder itself creates: ProcessEmitting prunes against the running next_cutoff
 * (lattice-faster-decoder.cc:728-733) with the tokens in HashList order (util/hash-list-inl.h:118-147: buckets
 * state % hash_size in order of first occupation, insertion order inside a bucket; hash_size as :37, :219-225), the best
 * token of GetCutoff is the first minimum in that order (:599, :611), and the epsilon closure inserts in the order of its
 * LIFO queue (:766-811).  Each utterance is decoded as by a freshly constructed decoder (hash_size 1000 at its start).
 * enable == 0 (opt-in, "canonical"): the order-independent resolution of those three places (DESIGN.md "Decoder parity":
 * accept against the FINAL next_cutoff, ties to the smallest state id), which is what the reference computes whenever no
 * token lies between the final and the running cutoff - a cheaper kernel, NOT the reference's lattices in general.
 * The environment variable KH_DECODER_ORDER=reference|canonical overrides both. */
int kh_decoder_set_reference_order(KhDecoder *dec, int enable);
/* Search counters of utterance `utt` (-1: summed over the batch) in the last kh_decoder_decode call (measurement aid): counters[0] = emitting
 * candidates that were materialised (given a link slot: the rest of arcs_expanded were read and rejected),
 * counters[1] = 1 if the call ran in reference order. */
int kh_decoder_get_search_counters(const KhDecoder *dec, int utt, int64_t *counters);
/* Duration of the decode kernel of the last kh_decoder_decode call, from HIP
 * events recorded on the launch stream (measurement aid; the reference wraps
 * every CuMatrix op in a Timer, cu-device.cc:384-389). */
int kh_decoder_last_kernel_ms(const KhDecoder *dec, float *ms);
/* Wall time the host threads of the last kh_decoder_decode call (raw lattices, best paths, determinization when
 * kh_decoder_set_determinize is on) still needed after the decode kernel had finished: what the overlap with the
 * kernel did not hide (measurement aid). */
int kh_decoder_last_host_tail_ms(const KhDecoder *dec, float *ms);
/* fn(arg) is called by kh_decoder_decode on the calling thread, once per call, when the LAST decode kernel of the call has
 * finished — i.e. no utterance is waiting to be decoded again after an arena / lattice-pool overflow, and nothing on the
 * device will read the score matrix of this batch any more (offline decoding re-evaluates the acoustic cost of an exported
 * link from it inside the kernel) — and BEFORE the call waits for its completion threads (raw lattices, best paths,
 * determinization): the caller's turn while the host finishes the batch.  What a binary's main loop does there —
 * nnet-latgen-faster.cc:139-160 would compute the NEXT batch's log-likelihoods (kh_nnet_compute on the library's stream),
 * into the same score buffer if it likes.  The hook should return quickly (start the work, do not wait for it): the call's
 * host tail is measured from before it.  Nothing of kh_decoder_decode waits for work the hook enqueues.  (Until round 4
 * the hook fired right after the FIRST launch, which was wrong for a caller that reuses the score buffer when an utterance
 * had to be decoded again.)  fn = NULL: none (default). */
int kh_decoder_set_after_launch(KhDecoder *dec, void (*fn)(void *), void *arg);
/* GetRawLattice (lattice-faster-decoder.cc:109-191), use_final_probs = true,
 * in canonical form: states are the surviving tokens sorted by
 * (frame, hclg_state); arcs sorted by (src, ilabel, olabel, dst, graph, ac).
 * HOST output arrays sized from kh_decoder_get_stats (num_tokens/num_links):
 *   state_frame[num_tokens], state_hclg[num_tokens], state_final[num_tokens]
 *   (LatticeWeight(final,0) value1; +inf = not final),
 *   arc_src/arc_dst/arc_ilabel/arc_olabel[num_links], arc_graph/arc_acoustic
 *   (acoustic_cost - cost_offset[frame], :172). Any pointer may be NULL. */
int kh_decoder_get_raw_lattice(const KhDecoder *dec, int utt,
                               int32_t *state_frame, int32_t *state_hclg,
                               float *state_final, int32_t *arc_src,
                               int32_t *arc_dst, int32_t *arc_ilabel,
                               int32_t *arc_olabel, float *arc_graph,
                               float *arc_acoustic);
/* GetBestPath (lattice-faster-decoder.cc:99-105) + GetLinearSymbolSequence as
 * DecodeUtteranceLatticeFaster uses it (decoder-wrappers.cc:232-246):
 * alignment = ilabels != 0 along the best path, words = olabels != 0.
 * Returns lengths via *n_ali / *n_words (buffers of capacity cap_*), the total
 * weight as (graph, acoustic). */
int kh_decoder_get_best_path(const KhDecoder *dec, int utt, int32_t *alignment,
                             int cap_ali, int32_t *n_ali, int32_t *words,
                             int cap_words, int32_t *n_words,
                             float *graph_cost, float *acoustic_cost);
/* kh_decoder_get_best_path for utterances [first, first + n) in one call (the per-utterance loop of
 * nnet-latgen-faster.cc:163-186 on the library's side of a foreign-function interface): alignments and
 * word sequences row-concatenated, ali_off / words_off = n + 1 offsets into them, one cost pair per
 * utterance.  KH_EINVAL if a buffer is too small. */
int kh_decoder_get_best_paths(const KhDecoder *d, int first, int n, int32_t *alignment, int64_t cap_ali,
                              int64_t *ali_off, int32_t *words, int64_t cap_words, int64_t *words_off,
                              float *graph_cost, float *acoustic_cost);
/* kh_decoder_get_counters / kh_decoder_get_stats for utterances [first, first + n); either array may be NULL. */
int kh_decoder_get_stats_batch(const KhDecoder *d, int first, int n, KhDecodeStats *counters, KhDecodeStats *stats);
/* Host post-pass of the whole batch on num_threads host threads (<= 0: all
 * cores): GetBestPath of every utterance that has none yet, i.e. what
 * DecodeUtteranceLatticeFaster (decoder-wrappers.cc:215-262) does one utterance
 * at a time after Decode().  The per-utterance getters above then return the
 * cached results.  Optional: the getters compute on demand otherwise, and
 * kh_decoder_decode's own completion threads have normally done it already.
 * Since round 4 the best path (and kh_decoder_get_stats' lattice sizes) come
 * straight from the exported token / link arrays; the CANONICAL raw lattice of an
 * utterance is built on first access (kh_decoder_get_raw_lattice, determinization)
 * - the sort of every utterance's lattice was 2 ms of host CPU per utterance that a
 * rank with few host threads does not have. */
int kh_decoder_prepare(KhDecoder *dec, int num_threads);
/* DeterminizeLatticePhonePrunedWrapper behind the decoder, as DecodeUtteranceLatticeFaster runs it when
 * determinize_lattice is set (decoder/decoder-wrappers.cc:264-274; LatticeFasterDecoderConfig::det_opts,
 * lattice-faster-decoder.h:75-91).  With enable != 0 the host threads of kh_decoder_decode that build an utterance's
 * raw lattice as soon as the kernel has exported it also determinize it (beam = the lattice beam; delta, max_mem,
 * phone_determinize, word_determinize, minimize = DeterminizeLatticePhonePrunedOptions, tid_phone as
 * kh_determinize_lattice_phone_pruned takes it - copied), overlapped with the kernel that is still decoding the rest
 * of the batch.
 * kh_decoder_get_compact_lattice returns the utterance's CompactLattice (owned by the decoder, valid until the next
 * kh_decoder_decode / kh_decoder_destroy; read it with kh_compact_lattice_sizes / _get below), NULL on error. */
typedef struct KhCompactLattice KhCompactLattice;
int kh_decoder_set_determinize(KhDecoder *dec, int enable, double beam, float delta, int64_t max_mem, const int32_t *tid_phone,
                               int n_tid, int phone_determinize, int word_determinize, int minimize);
const KhCompactLattice *kh_decoder_get_compact_lattice(KhDecoder *dec, int utt);
/* totals[4] over the batch's CompactLattices: states, arcs, transition-ids on arcs and final weights, lattices whose
 * determinization stopped at max_mem (measurement aid: the size of what the binary would write). */
int kh_decoder_compact_lattice_totals(KhDecoder *dec, int64_t *totals);

/* ------------------------------------------------------------------ (f)1
 * LatticeFasterOnlineDecoder (decoder/lattice-faster-online-decoder.h:44-200) for
 * num_streams concurrent utterances, advanced a chunk of frames at a time (what
 * online2/ feeds from DecodableNnet2Online).  The search, its pruning schedule
 * (every prune_interval frames, :762-764) and therefore the lattice are those of
 * kh_decoder_decode on the concatenated chunks.  A stream is an index in
 * [0, num_streams); every call takes a list of DISTINCT streams and processes them
 * in one kernel launch (one workgroup per stream). */
typedef struct KhOnlineDecoder KhOnlineDecoder;
KhOnlineDecoder *kh_online_decoder_create(const KhFst *hclg, const KhDecoderConfig *config,
                                          int num_streams, int max_frames);
void kh_online_decoder_destroy(KhOnlineDecoder *dec);
/* InitDecoding() :160 (.cc:55-72). */
int kh_online_decoder_init_decoding(KhOnlineDecoder *dec, const int32_t *streams, int n);
/* AdvanceDecoding(decodable, max_num_frames) :166 (.cc:747-769): stream streams[i]
 * decodes the next num_frames[i] frames; loglikes[i] = device matrix of their
 * acoustic_scale * log-likelihoods (num_frames[i] rows of ll_stride floats, whole
 * rows allocated), the rows a Decodable would return for frames NumFramesDecoded()...;
 * tid2pdf as in kh_decoder_decode. */
int kh_online_decoder_advance(KhOnlineDecoder *dec, const int32_t *streams, int n,
                              const float *const *loglikes, int ll_stride,
                              const int32_t *num_frames, const int32_t *tid2pdf);
/* NumFramesDecoded() :194. */
int kh_online_decoder_num_frames_decoded(const KhOnlineDecoder *dec, int stream, int32_t *num_frames);
/* The offline kernel's lazy pruning schedule for the streams (default 0 = the reference's: PruneActiveTokens every
 * prune_interval frames, lattice-faster-online-decoder.cc:811-813): nothing is pruned while a stream advances unless its
 * arenas run low, FinalizeDecoding prunes every frame once.  The final lattice, every best path and the endpointing
 * quantities are unchanged; a raw lattice asked for BEFORE FinalizeDecoding is pruned as of the current frame, not as of
 * the last multiple of prune_interval.  Re-carves the arenas (as much memory as is free, less 48 GB): every stream must be idle.
 * Round 6, experimental: with KH_SERVE_LAZY_SPAN=n (default 0 = only when its arenas run low, the offline kernel's rule) a
 * stream also collects its garbage (PruneActiveTokens + compaction) once n frames have gone unpruned, so that no chunk of a
 * long utterance waits for the collection of a backlog of thousands of frames (chunk latency max 113 -> 28 ms at n = 128);
 * off by default: the serving stress harness saw rare GPU faults with it on (csrc/kh_decoder_host.hip OnlineLazySpan). */
int kh_online_decoder_set_lazy_prune(KhOnlineDecoder *dec, int enable);
/* kh_decoder_set_reference_order for the streams: LatticeFasterOnlineDecoder::ProcessEmitting (decoder/lattice-faster-online-
 * decoder.cc:864-951) walks the same HashList against the same running next_cutoff as the offline decoder, and with this set
 * the launch-per-job calls (kh_online_decoder_init_decoding / _advance / _finalize) and the persistent serving kernel
 * (kh_online_decoder_serve_*, started afterwards) reproduce it: chunked decoding, the offline kernel in reference order and
 * the line-by-line oracle (mode 0) give the same lattices bit for bit.  Between utterances only (KH_ESTATE while a stream is
 * in a decoding run or the serving kernel is running).  On by default (as kh_decoder_set_reference_order); KH_DECODER_ORDER=
 * reference|canonical in the environment overrides at creation. */
int kh_online_decoder_set_reference_order(KhOnlineDecoder *dec, int enable);
/* The same three calls without a kernel launch per chunk: a PERSISTENT serving kernel, one resident workgroup per stream
 * (num_streams <= 2 x the CU count), which waits on a control block in pinned host memory (online2-wav-nnet2-latgen-faster's
 * per-chunk loop :213-262 for many connections; a stream that is pruning - AdvanceDecoding prunes every prune_interval
 * frames, lattice-faster-online-decoder.cc:811-813 - no longer holds up the others, which a lockstep launch cannot avoid).
 * kh_online_decoder_serve_start: loglikes = the streams' score buffers (DEVICE, stream s owns rows
 * [s * rows_per_stream, (s + 1) * rows_per_stream), row t = frame t of its current utterance; rows_per_stream >= max_frames),
 * tid2pdf as kh_online_decoder_advance; the streams continue from where kh_online_decoder_* calls left them.
 * kh_online_decoder_serve_init / _finalize: InitDecoding / FinalizeDecoding requests (asynchronous; FinalizeDecoding
 * runs after the frames published so far).  kh_online_decoder_serve_publish: frames [0, avail[i]) of stream streams[i]
 * have their scores in the buffer - the kernels that wrote them must have COMPLETED - and the stream decodes up to
 * there.  kh_online_decoder_serve_poll: NumFramesDecoded() so far and whether a request is still in flight (either
 * may be NULL); kh_online_decoder_serve_wait: blocks until the listed streams have caught up (timeout_ms <= 0:
 * KH_SERVE_TIMEOUT_MS, default 30 s);
 * afterwards the getters (kh_online_decoder_get_best_path, _get_raw_lattice, _get_stats) may be used on them while the
 * kernel keeps serving the others.  kh_online_decoder_serve_stop: the kernel leaves (the grid also leaves by itself - as a
 * whole, never one stream's workgroup alone - once EVERY stream has been without work for 2 s, KH_SERVE_IDLE_MS, and is
 * launched again by the next request or poll that finds work: a device-wide synchronisation never waits longer than that);
 * the launch-per-job calls work again.  Results are those of the launch-per-job calls.
 * No call blocks for ever: every wait for the device has a deadline (the timeout argument of _serve_wait;
 * KH_SERVE_TIMEOUT_MS for _serve_stop and the relaunch), after which it returns KH_ETIMEOUT and kh_last_error() holds the
 * control blocks of the streams concerned - frames published / decoded, command and acknowledgement numbers, whether the
 * stream's workgroup is resident and what it was doing (InitDecoding / AdvanceDecoding to which frame / FinalizeDecoding)
 * when it last reported. */
int kh_online_decoder_serve_start(KhOnlineDecoder *dec, const float *loglikes, int ll_stride, int64_t rows_per_stream,
                                  const int32_t *tid2pdf);
int kh_online_decoder_serve_stop(KhOnlineDecoder *dec);
int kh_online_decoder_serve_init(KhOnlineDecoder *dec, const int32_t *streams, int n);
int kh_online_decoder_serve_publish(KhOnlineDecoder *dec, const int32_t *streams, int n, const int32_t *avail);
int kh_online_decoder_serve_finalize(KhOnlineDecoder *dec, const int32_t *streams, int n);
int kh_online_decoder_serve_poll(KhOnlineDecoder *dec, const int32_t *streams, int n, int32_t *decoded, int32_t *in_flight);
int kh_online_decoder_serve_wait(KhOnlineDecoder *dec, const int32_t *streams, int n, int timeout_ms);
/* Serving loops call kh_online_decoder_advance once per chunk with the same transition-id -> pdf map (DEVICE, or NULL) and
 * the same number of score columns: this builds the decoder's arc records for that pair ONCE (a pass over the whole graph
 * and a synchronisation otherwise repeated by every advance call) and validates the map as kh_online_decoder_advance
 * does.  Later advance calls with the same pointer and ll_stride == num_cols reuse the records; the caller must not change
 * the map's contents in between (any other pointer / stride rebuilds as before). */
int kh_online_decoder_set_pdf_map(KhOnlineDecoder *dec, const int32_t *tid2pdf, int num_cols);
/* FinalizeDecoding() :180 (.cc:775-790). */
int kh_online_decoder_finalize(KhOnlineDecoder *dec, const int32_t *streams, int n);
/* GetRawLattice(ofst, use_final_probs) :143 (.cc:143-233), GetBestPath :107 and the
 * counters, valid at any point after the first frame: before FinalizeDecoding the
 * lattice holds every token not yet pruned and, with use_final_probs, the final
 * costs computed on the fly (.cc:160-165).  use_final_probs == 0 after
 * FinalizeDecoding is an error as in the reference (.cc:156-158).  Layout as
 * kh_decoder_get_raw_lattice / kh_decoder_get_best_path (sizes via get_stats). */
int kh_online_decoder_get_stats(KhOnlineDecoder *dec, int stream, int use_final_probs, KhDecodeStats *stats);
int kh_online_decoder_get_raw_lattice(KhOnlineDecoder *dec, int stream, int use_final_probs,
                                      int32_t *state_frame, int32_t *state_hclg, float *state_final,
                                      int32_t *arc_src, int32_t *arc_dst, int32_t *arc_ilabel,
                                      int32_t *arc_olabel, float *arc_graph, float *arc_acoustic);
int kh_online_decoder_get_best_path(KhOnlineDecoder *dec, int stream, int use_final_probs,
                                    int32_t *alignment, int cap_ali, int32_t *n_ali, int32_t *words,
                                    int cap_words, int32_t *n_words, float *graph_cost,
                                    float *acoustic_cost);

/* ------------------------------------------------------------------ (f)3
 * Feature front-end, the step right before the path (feat/, transform/cmvn.cc).
 * kh_mfcc_compute = Mfcc::ComputeInternal (feat/feature-mfcc.cc:119-184) with
 * use_energy = false, dither = 0, snip_edges = true, for a waveform on the DEVICE.  The
 * tables are the ones the reference's constructors build (HOST arrays): window =
 * FeatureWindowFunction (feature-functions.cc:74-92, frame_length floats), mel_first /
 * mel_off / mel_weights = MelBanks::bins_ (mel-computations.cc:33-152: first FFT bin,
 * offsets into the concatenated weights), dct = the first num_ceps rows of
 * ComputeDctMatrix (matrix-functions.cc:592-608, num_ceps x num_bins), lifter =
 * ComputeLifterCoeffs (mel-computations.cc:248-254) or NULL.  padded = the power-of-two
 * FFT size (<= 2048).  *num_frames = NumFrames (feature-functions.cc:29-48); out must
 * hold that many rows of num_ceps floats. */
int kh_mfcc_compute(const float *wave, int n_samples, int frame_shift, int frame_length, int padded,
                    float preemph_coeff, int remove_dc_offset, const float *window_host, int num_bins,
                    const int32_t *mel_first_host, const int32_t *mel_off_host,
                    const float *mel_weights_host, int num_ceps, const float *dct_host,
                    const float *lifter_host, float *out, int out_stride, int *num_frames);
/* The same with the remaining MfccOptions / FrameExtractionOptions (feat/feature-mfcc.h:41-56,
 * feature-functions.h:77-96): snip_edges = 0: NumFrames = round(n / shift), frame r centred on
 * shift * (r + 0.5), the signal extended by reflection (ExtractWindow feature-functions.cc:107-135);
 * use_energy: C0 := log energy of the frame before pre-emphasis and windowing (raw_energy) or of
 * the windowed frame, floored at log(energy_floor) when energy_floor > 0 (feature-mfcc.cc:138-141,
 * :167-171); htk_compat: energy / C0 * sqrt(2) moved to the last column (:173-182); dither > 0:
 * Gaussian noise * dither added to every sample of every window (Dither :51-54) from a
 * counter-based generator seeded with dither_seed (the reference draws from rand(): same
 * distribution, not the same numbers).  kh_mfcc_compute = {snip_edges 1, raw_energy 1, rest 0}. */
typedef struct KhMfccOptions {
  int32_t snip_edges, use_energy, raw_energy, htk_compat;
  float energy_floor, dither;
  uint64_t dither_seed;
} KhMfccOptions;
int kh_mfcc_compute_opts(const float *wave, int n_samples, int frame_shift, int frame_length, int padded,
                         float preemph_coeff, int remove_dc_offset, const float *window_host, int num_bins,
                         const int32_t *mel_first_host, const int32_t *mel_off_host,
                         const float *mel_weights_host, int num_ceps, const float *dct_host,
                         const float *lifter_host, const KhMfccOptions *options, float *out, int out_stride,
                         int *num_frames);
/* ComputeDeltas (feat/feature-functions.cc:361-372): scales of DeltaFeatures
 * (:210-242) for orders 0..order back to back (HOST), their lengths in lens_host. */
int kh_compute_deltas(const float *in, KhMatrixDim d_in, int order, const float *scales_host,
                      const int32_t *lens_host, float *out, int out_stride);
/* AccCmvnStats (transform/cmvn.cc:49-62, no weights): adds the sums of feats (DEVICE) to
 * stats_host [2 x (cols + 1)] doubles (row 0: sum x and the count, row 1: sum x^2).
 * ApplyCmvn (:64-113) is kh_mul_cols_vec + kh_add_vec_to_rows with the offset / scale
 * vectors the caller derives from the stats as the reference does. */
int kh_acc_cmvn_stats(const float *feats, KhMatrixDim d, double *stats_host);

/* ------------------------------------------------------------------ (f)1, serving
 * The per-chunk loop of online2-wav-nnet2-latgen-faster (online2bin/online2-wav-nnet2-latgen-faster.cc:213-262) for many
 * concurrent streams in ONE call per step: the chunk's feature rows enter DecodableNnet2Online
 * (nnet2/online-nnet2-decodable.{h,cc}: NumFramesReady :75-89, ComputeForFrame :91-143 - the context-padded rows of every
 * advancing stream gathered into one matrix, one forward pass, the floor / log / -log prior / acoustic-scale epilogue) and
 * LatticeFasterOnlineDecoder::AdvanceDecoding consumes what became ready.  nnet (with priors set) and dec stay owned by
 * the caller and must outlive the object; results are read from dec (kh_online_decoder_get_*; kh_online_decoder_finalize at
 * the end of an utterance).  kh_online_nnet2_reset: a new utterance on the listed streams (InitDecoding).
 * kh_online_nnet2_step: stream streams[i] receives rows [src_rows[i], src_rows[i] + counts[i]) of the DEVICE matrix src
 * (counts[i] >= 0), finished[i] != 0 = InputFinished() after them; every listed stream then advances by the frames that
 * became ready (at most max_nnet_batch_size per call); frames_decoded (may be NULL) = NumFramesDecoded() afterwards.
 * tid2pdf as kh_online_decoder_advance (pin it with kh_online_decoder_set_pdf_map).  Synchronous. */
typedef struct KhOnlineNnet2 KhOnlineNnet2;
KhOnlineNnet2 *kh_online_nnet2_create(KhNnet *nnet, KhOnlineDecoder *dec, int num_streams, int max_frames, float acoustic_scale,
                                      int pad_input, int max_nnet_batch_size);
void kh_online_nnet2_destroy(KhOnlineNnet2 *h);
int kh_online_nnet2_reset(KhOnlineNnet2 *h, const int32_t *streams, int n);
int kh_online_nnet2_step(KhOnlineNnet2 *h, const int32_t *streams, int n, const float *src, int src_stride,
                         const int32_t *src_rows, const int32_t *counts, const int32_t *finished, const int32_t *tid2pdf,
                         int32_t *frames_decoded);
int kh_online_nnet2_num_frames_ready(const KhOnlineNnet2 *h, int stream, int32_t *ready);
/* Serving through the decoder's persistent kernel (kh_online_decoder_serve_*): after kh_online_nnet2_serve_start,
 * kh_online_nnet2_step returns as soon as the chunk's scores are in the streams' score buffers and published (its
 * frames_decoded = how far the decoder has got, which runs behind), kh_online_nnet2_reset requests InitDecoding,
 * kh_online_nnet2_serve_finalize requests FinalizeDecoding (after the frames submitted so far); _serve_poll / _serve_wait
 * as the decoder's calls.  The score buffers take num_streams x max_frames x output-dim floats of device memory.
 * kh_online_nnet2_serve_stop: back to one launch per step.  Same lattices either way. */
int kh_online_nnet2_serve_start(KhOnlineNnet2 *h, const int32_t *tid2pdf);
int kh_online_nnet2_serve_stop(KhOnlineNnet2 *h);
int kh_online_nnet2_serve_finalize(KhOnlineNnet2 *h, const int32_t *streams, int n);
int kh_online_nnet2_serve_poll(KhOnlineNnet2 *h, const int32_t *streams, int n, int32_t *decoded, int32_t *in_flight);
int kh_online_nnet2_serve_wait(KhOnlineNnet2 *h, const int32_t *streams, int n, int timeout_ms);

/* LatticeStateTimes (lat/lattice-functions.cc:36-67) for a batch of top-sorted lattices
 * (layout as kh_lattice_forward_backward): time of every state (-1: unreachable) and, per
 * lattice, the number of frames (max_times may be NULL).  KH_EINVAL if a lattice is not
 * top-sorted or its state times are inconsistent (the KALDI_ASSERTs of :38-39,:55,:61). */
int kh_lattice_state_times(int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets,
                           const int32_t *arc_ilabel, const int32_t *arc_nextstate, const float *state_final,
                           int32_t *state_times, int32_t *max_times);

/* ------------------------------------------------------------------ a15
 * Lattice forward-backward (lat/lattice-functions.cc:36-67,272-354) for a batch
 * of top-sorted lattices given as HOST CSR (state s owns arcs
 * [arc_offsets[s], arc_offsets[s+1])); lattices are concatenated, lattice l
 * owns states [lat_state_offsets[l], lat_state_offsets[l+1]) and its arcs'
 * nextstate values are lattice-local.  Arc weight = (graph, acoustic)
 * LatticeWeight (fstext/lattice-weight.h:47), final = value1+value2 sum
 * (+inf = Zero).  Outputs (HOST): per-arc posterior (float), per-lattice total
 * log-prob (double, tot_backward_prob) and acoustic_like_sum (double), per-state
 * time (LatticeStateTimes).  */
int kh_lattice_forward_backward(int n_lats, const int32_t *lat_state_offsets,
                                const int64_t *arc_offsets,
                                const int32_t *arc_ilabel,
                                const int32_t *arc_nextstate,
                                const float *arc_graph, const float *arc_acoustic,
                                const float *state_final, float *arc_post,
                                double *tot_like, double *acoustic_like_sum,
                                int32_t *state_times);

/* A batch of lattices KEPT ON THE DEVICE: the caller's arrays are uploaded and prepared (validation, LatticeStateTimes,
 * dependency levels, incoming-arc lists) once, and every computation on the batch — the numerator's and the denominator's
 * forward-backward, rescoring with a new score matrix, the forward-backward after it — runs from there
 * (lat/lattice-functions.cc:272-354, :1307-1358; nnet-compute-discriminative.cc:178-321 does exactly this sequence on one
 * lattice).  kh_lattice_batch_create takes the arguments of kh_lattice_forward_backward and returns NULL on an error
 * (kh_last_error).  kh_lattice_batch_forward_backward: outputs as kh_lattice_forward_backward, any may be NULL.
 * kh_lattice_batch_rescore: RescoreLattice with a DEVICE score matrix (lattice l uses rows ll_row_offsets[l]..., HOST
 * offsets; tid2pdf DEVICE or NULL = ilabel - 1); the acoustic costs change on the device, arc_acoustic_out (HOST, may be
 * NULL) receives them.  kh_lattice_last_timings: milliseconds the last lattice call of this thread spent in
 * { upload, device preparation, sweeps, download } (HIP events on the library's stream; measurement aid). */
typedef struct KhLatticeBatch KhLatticeBatch;
KhLatticeBatch *kh_lattice_batch_create(int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets,
                                        const int32_t *arc_ilabel, const int32_t *arc_nextstate, const float *arc_graph,
                                        const float *arc_acoustic, const float *state_final);
void kh_lattice_batch_destroy(KhLatticeBatch *batch);
int kh_lattice_batch_sizes(const KhLatticeBatch *batch, int32_t *n_lats, int32_t *total_states, int64_t *total_arcs);
int kh_lattice_batch_forward_backward(KhLatticeBatch *batch, float *arc_post, double *tot_like, double *acoustic_like_sum,
                                      int32_t *state_times);
/* ... with the arc posteriors left on the DEVICE (arc_post_dev: total_arcs floats in the batch's arc order; tot_like /
 * acoustic_like_sum HOST, may be NULL): no 4 bytes per arc over PCIe when the next consumer is a kernel. */
int kh_lattice_batch_forward_backward_dev(KhLatticeBatch *batch, float *arc_post_dev, double *tot_like, double *acoustic_like_sum);
int kh_lattice_batch_rescore(KhLatticeBatch *batch, const float *loglikes, int ll_stride, const int32_t *ll_row_offsets,
                             const int32_t *tid2pdf, float *arc_acoustic_out);
int kh_lattice_last_timings(float *ms4);
/* Which forms of the lattice kernels the last lattice call of this thread ran (the sizing: csrc/kh_lattice_plan.h), 12 words:
 * [0] CUs of the device; the preparation: [1] 1 = dataflow (PrepKernelDF), 0 = dependency levels (PrepKernel), [2] workgroups
 * planned per CU, [3] slots of the state-time window, [4] states whose counters stay in LDS ([2], [3]: 0 for the level
 * preparation), [5] lattices of more states than [4] (their counters are in device memory); the forward-backward sweep:
 * [6] 1 = dataflow, 0 = by level, -1 = the call ran none, [7] workgroups planned per CU, [8] arcs staged per wave, [9] slots
 * of the value window, [10] lattices of more states than [9] (tagged window) ([7]-[10]: 0 unless [6] = 1); [11] 0. */
int kh_lattice_last_plan(int32_t *out12);

/* ComputeLatticeAlphasAndBetas (lat/lattice-functions.cc:412-463) for a batch (same CSR
 * layout as above): alpha / beta per state (log-semiring, or the tropical one when
 * viterbi != 0: LogAddOrMax :395-410), tot[l] = 0.5 * (forward + backward total). */
int kh_lattice_alphas_betas(int n_lats, const int32_t *lat_state_offsets,
                            const int64_t *arc_offsets, const int32_t *arc_ilabel,
                            const int32_t *arc_nextstate, const float *arc_graph,
                            const float *arc_acoustic, const float *state_final,
                            int viterbi, double *alpha, double *beta, double *tot);

/* CompactLatticeShortestPath (lat/lattice-functions.cc:1043-1126) for a batch of top-sorted CompactLattices and n_points
 * "score points" in one call (csrc/kh_latbest.hip).  HOST CSR as kh_lattice_forward_backward (arc_label = the word of a
 * CompactLattice arc; final_graph / final_acoustic = the two values of the final weight, +inf / +inf = Zero; the strings
 * stay with the caller).  A score point is what lattice-scale and lattice-add-penalty do to a weight before
 * lattice-best-path searches: scales[4 p ...] = { lm_scale, acoustic2lm_scale, lm2acoustic_scale, acoustic_scale }
 * (latbin/lattice-scale.cc:76-82, doubles) and penalties[p] (float).  Per lattice and point, in the reference's order:
 *   (g, a) -> g' = (float)(s00 g + s01 a), a' = (float)(s10 g + s11 a), sums and products in double, Zero stays Zero
 *   (fstext/lattice-weight.h:233-241); g' = g' + penalty in float on arcs with a label != 0, never on final weights
 *   (lattice-functions.cc:1140-1143); cost = (double)g' + (double)a' (lattice-weight.h:799-801); the search of :1060-1086
 *   (a predecessor is replaced only by a strictly smaller cost: on a tie the lowest-numbered source state stays); between
 *   two consecutive path states the arc of smallest COST, the first on a tie (:1102-1121).
 * Outputs (HOST), entry l * n_points + p: path_len = arcs on the path, -1 = no path (:1091; the caller counts a failure);
 * the path's arcs as arc numbers relative to the lattice's first arc at path_arcs[path_offsets[l * n_points + p] ...]
 * (path_offsets: n_lats * n_points + 1 entries, the caller's room per path; n_states - 1 always suffices, KH_EINVAL if a
 * path does not fit); path_final_state = the state whose final weight ends the path; tot_graph / tot_acoustic = the float
 * sums GetLinearSymbolSequence forms (lattice-best-path.cc:98): from 0, every path arc's g' / a' in path order, the final
 * weight's last.  KH_EINVAL if a lattice is not top-sorted (an arc to a state that is not higher-numbered).
 * The workspace is (n_states x 12 + longest path x 4) bytes x n_points per lattice in flight; lattices are taken longest
 * first, as many per launch as half of the free device memory admits, or as
 * kh_compact_lattice_best_paths_set_workspace_limit(bytes) admits: a setting of the CALLING THREAD (0 = back to
 * automatic; one lattice always runs).  kh_compact_lattice_best_paths_last_timings: milliseconds the last call of this
 * thread spent in { host preparation (validation, incoming-arc lists), upload, kernels, download (HIP events; the host's
 * scatter and the allocations are not in these four), the whole call by the host's clock }, and its number of launches
 * (may be NULL). */
int kh_compact_lattice_best_paths(int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets,
                                  const int32_t *arc_label, const int32_t *arc_nextstate, const float *arc_graph,
                                  const float *arc_acoustic, const float *final_graph, const float *final_acoustic,
                                  int n_points, const double *scales, const float *penalties, int32_t *path_len,
                                  int32_t *path_arcs, const int64_t *path_offsets, int32_t *path_final_state,
                                  float *tot_graph, float *tot_acoustic);
int kh_compact_lattice_best_paths_set_workspace_limit(size_t bytes);
int kh_compact_lattice_best_paths_last_timings(float *ms5, int32_t *n_launches);

/* PruneLattice<CompactLattice> (lat/lattice-functions.cc:186-265) for a batch of top-sorted CompactLattices and n_points
 * score points in one call (csrc/kh_latprune.hip): what `lattice-scale | lattice-add-penalty | lattice-prune --beam=B`
 * (latbin/lattice-prune.cc:87) decides once per point of a scoring grid.  HOST CSR, scales and penalties as
 * kh_compact_lattice_best_paths; lat_start[l] = lat->Start() (:201) in the lattice's own numbering - the states in front of
 * it are unreachable, unlike the best-path search, which starts at state 0; beams[p] = the point's float beam.  Per
 * lattice and point, in the reference's order: the point applied to arc and final weights as kh_compact_lattice_best_paths
 * applies it (fstext/lattice-weight.h:233-241, lattice-functions.cc:1140-1143, cost = (double)g' + (double)a'); the
 * Viterbi forward sweep :211-229; cutoff = best_final_cost + (double)beam :231; the backward sweep :239-262 with its three
 * comparisons as written there (a final weight is cleared when backward + forward > cutoff and it is not +inf; an arc is
 * pruned when this_forward_cost + (arc_cost + backward_cost[next]) > cutoff, in that association; arc_backward_cost <
 * this_backward_cost); then fst::Connect :263, computed: a state survives when it is reachable from the start state over
 * unpruned arcs and reaches a state that kept its final weight, an arc when it is unpruned and both its ends survive.
 * Outputs (HOST) are bit masks over the points, W = ceil(n_points / 64) words per arc or state, bit p % 64 of word p / 64
 * for point p: arc_keep[a W + w] (the arc is in the pruned, connected lattice), state_keep[s W + w] (the state survives
 * Connect), final_keep[s W + w] (the state keeps its final weight), and best_final_cost[l n_points + p] (:208-229; +inf =
 * no final state is reachable: nothing is pruned and everything is disconnected).  The sweeps only take minima, which do
 * not depend on the order of the candidates as long as none is NaN or -inf, so the results equal the reference's bit for
 * bit; weights that are NaN or -inf are refused.  KH_EINVAL, with the arc, state or point named, for an arc to a state that
 * is not higher-numbered (:193, :218), lat_start out of range, beam <= 0 (:192), n_points < 1, a NaN or -inf weight.
 * The workspace is n_states x 8 bytes x 64 W per lattice in flight; lattices are taken longest first, as many per launch
 * as half of the free device memory admits, or as kh_compact_lattice_prune_set_workspace_limit(bytes) admits: a setting
 * of the CALLING THREAD (0 = back to automatic; one lattice always runs).  kh_compact_lattice_prune_last_timings:
 * milliseconds the last call of this thread spent in { host preparation (validation, incoming-arc lists), upload, kernels,
 * download (HIP events; the allocations are in none of the four), the whole call by the host's clock }, and its number of
 * launches of the sweep kernel (may be NULL). */
int kh_compact_lattice_prune(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                             const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                             const float *arc_graph, const float *arc_acoustic, const float *final_graph,
                             const float *final_acoustic, int n_points, const double *scales, const float *penalties,
                             const float *beams, uint64_t *arc_keep, uint64_t *state_keep, uint64_t *final_keep,
                             double *best_final_cost);
int kh_compact_lattice_prune_set_workspace_limit(size_t bytes);
int kh_compact_lattice_prune_last_timings(float *ms5, int32_t *n_launches);

/* The oracle path of latbin/lattice-oracle.cc:313-421 for a batch of top-sorted CompactLattices, one reference word
 * sequence each and n_points mask points in one call (csrc/kh_latoracle.hip), with the numerator of CompactLatticeDepth
 * (lat/lattice-functions.cc:574-602) as a by-product.  HOST CSR and lat_start as kh_compact_lattice_prune takes them;
 * is_final[s] != 0: the state has a final weight; ref_offsets[n_lats + 1], ref_words: the references; wildcards:
 * n_wildcards labels in ascending order.  Label 0 and the wildcards are epsilon on the lattice's arcs, and such words are
 * dropped from the reference (MapWildCards :58-75, :88, :333).  arc_keep, state_keep, final_keep: the masks of
 * kh_compact_lattice_prune in its layout (W = ceil(n_points / 64) words per arc or state), all three or none; NULL means
 * n_points = 1 and everything is kept.  Per lattice and point, over the kept arcs, with r[1..R] the reference:
 * D[start][j] = j; D[e][j] = min(over the arcs s -> e with word w: D[s][j] when w is epsilon, else D[s][j-1] + (w != r[j])
 * and D[s][j] + 1; D[e][j-1] + 1), int32; errors[l n_points + p] = min D[f][R] over the states whose final weight is kept,
 * or -1 when no such state is reachable (the reference's "Best-path failed" :359-361).  counts[4 (l n_points + p) + 0..3] =
 * correct, substitutions, insertions, deletions along one best path (CountErrors :131-164), path_len / path_arcs (arc
 * numbers relative to the lattice's first arc, written at path_offsets[l n_points + p]; room for n_states - 1 arcs always
 * suffices) / path_final_state as kh_compact_lattice_best_paths gives them, path_len = -1 for no path; the oracle word
 * sequence is the non-epsilon labels of those arcs in order.  errors, R = correct + substitutions + deletions and so the
 * "Overall %WER" total are fixed by the problem and equal the reference's.  WHICH of several equal-cost paths is reported -
 * the split into insertions, deletions and substitutions, and the word sequence - is in the reference the choice of
 * fst::ShortestPath over the composed machine (:351-356), which is not reproduced; the rule here is: the lowest-numbered
 * end state that attains the minimum, then, walking back, the first candidate that attains the cell's value among the
 * incoming kept arcs in ascending arc number (for an arc with a word its diagonal before its insertion) and the deletion
 * last.  arc_frames[a], final_frames[s] (both or neither; may be NULL): the lengths of the transition-id strings;
 * arc_frame_sum[l n_points + p] = their sum over the kept arcs and over the kept finals of surviving states
 * (lattice-functions.cc:593-600 on the pruned lattice).  KH_EINVAL, with the arc, state or point named, for an arc to a
 * state that is not higher-numbered, lat_start out of range, n_points < 1 (or > 1 without masks), ref_offsets that do not
 * ascend, a reference of 2^24 = 16777216 words or more (the limit of this call), path room below n_states - 1.  The workspace is n_states x (R + 1) x 4 bytes per lattice and point in flight;
 * lattices are taken longest first, as many per launch as half of the free device memory admits, or as
 * kh_compact_lattice_oracle_set_workspace_limit(bytes) admits: a setting of the CALLING THREAD (0 = back to automatic; one
 * lattice always runs).  kh_compact_lattice_oracle_last_timings: as kh_compact_lattice_prune_last_timings. */
int kh_compact_lattice_oracle(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                              const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                              const int32_t *is_final, const int64_t *ref_offsets, const int32_t *ref_words,
                              int n_wildcards, const int32_t *wildcards, int n_points, const uint64_t *arc_keep,
                              const uint64_t *state_keep, const uint64_t *final_keep, const int32_t *arc_frames,
                              const int32_t *final_frames, int32_t *errors, int32_t *counts, int32_t *path_len,
                              int32_t *path_arcs, const int64_t *path_offsets, int32_t *path_final_state,
                              int64_t *arc_frame_sum);
int kh_compact_lattice_oracle_set_workspace_limit(size_t bytes);
int kh_compact_lattice_oracle_last_timings(float *ms5, int32_t *n_launches);

/* MinimumBayesRisk (lat/sausages.{h,cc}), the class behind lattice-mbr-decode and lattice-to-ctm-conf, for a batch of
 * top-sorted CompactLattices and n_points score points in one call (csrc/kh_latmbr.hip).  HOST CSR, lat_start, scales and
 * penalties as kh_compact_lattice_prune takes them; the lattices are in the class's own form (PrepareLatticeAndInitStats
 * :268-315): lat_start = 0, the last state the single final state with weight One (0, 0) and no arcs, every other final
 * weight Zero (+inf, +inf); state_times[s] = CompactLatticeStateTimes.  hyp_words at hyp_offsets[l n_points + p]: the
 * initial R_ of the pair (the constructors' :342 / :358); do_mbr as the class's flag.  Per lattice and point, restating
 * sausages.cc:27-266 statement by statement: each weight scaled as kh_compact_lattice_best_paths documents, loglike =
 * -(g' + a') summed in float (:306-307), l() and delta() of sausages.h:110,132 (delta is the float 1.0e-05 promoted to
 * double).  The transcendentals are taken on the host with libm: alpha(n) by the double LogAdd of base/kaldi-math.h:178-195
 * in pre_[n] order and w_a = exp(alpha(s_a) + p_a - alpha(n)) per arc; the kernel (one AccStats() per launch, one wave per
 * pair still iterating) does only double +, *, comparisons and integer work in the reference's order, so the results are
 * the restatement's bits.  The one deliberate difference: a state other than the start with alpha = -inf, where :125
 * computes exp(NaN), is refused.
 * Outputs (HOST), entry o = l n_points + p: n_words[o] and words / one_best_confidences at word_offsets[o], one_best_times
 * (pairs) at 2 word_offsets[o]: R_ without epsilons (:68), one_best_confidences_, one_best_times_; bayes_risk[o] = L_
 * (double; GetBayesRisk narrows it to float); iterations[o] = AccStats() calls; the last iteration's bins: n_bins[o] and
 * bin_sizes / bin_times (pairs, after the averaging of :257-264) at bin_offsets[o] / 2 bin_offsets[o]; n_stats[o] and
 * gamma_ as stat_words / stat_post at stat_offsets[o], the bins one after the other, each sorted by GammaCompare.  The three
 * offset arrays (n_lats n_points + 1 entries) are the room the caller leaves; n_words, n_bins and n_stats are always
 * written, and KH_EINVAL is returned - nothing else written - when a pair does not fit, so a second call with the room they
 * name succeeds.  KH_EINVAL, with the state, arc or point named, also for an arc to a state that is not higher-numbered, a
 * start state other than 0, a last state that is not the single final state with weight One, a NaN or -inf weight (before
 * or after the point is applied), alpha = -inf as above, n_points < 1.
 * The workspace per pair in flight is 2 x n_states x (Q + 1) x 8 bytes (alpha_dash, beta_dash) + (Q + 1) x 4 (b_arc) +
 * (V + 2) x (Q + 1) x 8 (gamma, dense, V = the lattice's distinct arc labels plus 0; tau_b, tau_e), Q = 2 |R_| + 1 of the
 * current iteration; pairs are taken largest first, as many per launch as half of the free device memory admits, or as
 * kh_compact_lattice_mbr_set_workspace_limit(bytes) admits: a setting of the CALLING THREAD (0 = back to automatic; one
 * pair always runs).  kh_compact_lattice_mbr_last_timings: milliseconds the last call of this thread spent in { host
 * preparation (validation, incoming-arc lists, alpha and w_a), uploads, kernels with their memsets, downloads (HIP
 * events), the whole call by the host's clock, the host's part of MbrDecode (casting and sorting gamma, updating R_) },
 * and counts3 (may be NULL) = { kernel launches, rounds of the host loop = the largest iteration count, AccStats() calls
 * summed over the pairs }. */
int kh_compact_lattice_mbr(int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start,
                           const int64_t *arc_offsets, const int32_t *arc_label, const int32_t *arc_nextstate,
                           const float *arc_graph, const float *arc_acoustic, const float *final_graph,
                           const float *final_acoustic, const int32_t *state_times, int n_points, const double *scales,
                           const float *penalties, const int64_t *hyp_offsets, const int32_t *hyp_words, int do_mbr,
                           int32_t *n_words, const int64_t *word_offsets, int32_t *words, float *one_best_times,
                           float *one_best_confidences, double *bayes_risk, int32_t *iterations, int32_t *n_bins,
                           const int64_t *bin_offsets, int32_t *bin_sizes, float *bin_times, int32_t *n_stats,
                           const int64_t *stat_offsets, int32_t *stat_words, float *stat_post);
int kh_compact_lattice_mbr_set_workspace_limit(size_t bytes);
int kh_compact_lattice_mbr_last_timings(float *ms6, int32_t *counts3);

/* WordAlignLattice (lat/word-align-lattice.{h,cc}, class LatticeWordAligner; latbin/lattice-align-words.cc) for a batch of
 * top-sorted CompactLattices in one call (csrc/kh_latalign.hip).  HOST CSR as kh_compact_lattice_prune takes it (every arc
 * to a higher-numbered state; lat_start < 0 or no states = an empty lattice), with the transition-id strings: arc a's at
 * arc_strings[arc_string_offsets[a] .. [a + 1]), state s's final string at final_strings[final_string_offsets[s] .. [s + 1]).
 * tid_phone / tid_is_final / tid_is_self_loop: TransitionIdToPhone, IsFinal, IsSelfLoop as arrays of num_tids + 1 entries
 * indexed by transition-id; phone_type[p], n_phone_types entries: WordBoundaryInfo::phone_to_type (0 kNoPhone, 1 begin,
 * 2 end, 3 singleton, 4 internal, 5 nonword); reorder, silence_label, partial_word_label: its other members; max_states[l]
 * (NULL = all 0): WordAlignLattice's argument.
 *
 * THE RESULT.  The reference explores tuples (input state, pending transition-ids, pending words) of the input after
 * fst::CreateSuperFinal (fstext/fstext-utils-inl.h: a single final state with weight One, an empty string and no arcs is
 * used as it is; otherwise a new highest-numbered state becomes the only final state and every old final state gets a
 * label-0 arc to it that carries its whole final weight, string included), with 0 silence / partial-word labels replaced by
 * 1 + the highest label of the lattice (:275-282).  ProcessQueueElement (:201-250) either cuts a word, silence or one-phone
 * word off the front of the pending ids (OutputArc :59-69, a labelled arc) or emits one epsilon arc per input arc (Advance
 * :40-48, which carries the arc's weight) and, on the final state, ProcessFinal (:172-198) with OutputArcForce (:554-635);
 * RmEpsilon(connect) follows, whose state numbering and arc order are OpenFst's and are not reproduced.  What the problem
 * fixes is reproduced: every stored tuple has weight One, so tuple identity is (input state, pending ids, pending words).
 *   Output states: the start tuple (start, -, -) and every destination of a labelled arc, if a final weight is reachable.
 *   Arcs of an output state S: over every tuple T reachable from S by Advance alone (a tuple whose OutputArc succeeds takes
 *   no epsilon step, :214), d(S, T) = the Times of the input arcs' weights along the path, two float sums accumulated left
 *   to right from One; a T whose OutputArc succeeds gives the arc S -> T' with that label, string and weight d(S, T); a T on
 *   the final state with something pending gives the arc of OutputArcForce in the same way - the label-0, empty-string arc
 *   of :574-589 that discards word labels included, as an arc -; a T on the final state with nothing pending Plus-es
 *   d(S, T) into S's final weight.  Where two epsilon paths reach the same T (input that is not deterministic), d(S, T) is
 *   their Plus, taken before T is expanded (tuples in ascending input state).  Two arcs of S with the same destination and
 *   label (before the temporary labels are mapped back to 0) are merged by Plus of CompactLatticeWeight
 *   (fstext/lattice-weight.h:562-608: the better weight with its string; where Compare of two LatticeWeights is 0 and the
 *   acoustic costs still differ, the smaller acoustic cost is the better one here, so Plus does not depend on order).
 *   Times: every path to an input state reachable from the start must consume the same number of transition-ids, else
 *   KH_EINVAL with the state named (a deliberate difference: the reference goes on).  time(S) = time(input state) - number
 *   of pending ids.
 *   NUMBERING (this library's rule): the start state is state 0; the others ascend by the key (time(S), input state,
 *   descending number of pending words, pending words lexicographically, pending ids lexicographically) - a topological
 *   order, since a labelled arc consumes at least one id, except the discarding arc above, which stays on its input state
 *   and goes from k > 0 pending words to none.  A state's arcs ascend by (destination, label).
 *   status[l]: KH_ALIGN_OK; KH_ALIGN_ERROR = aligned, and one of the conditions that set error_ held at some tuple
 *   (:361-365, :420-425, :464-469, :478-483, :494-498, :508-513, :565-568, :578-582, :604-613, :621-624; :375-379 and
 *   :406-410 only warn) - an OR, so independent of the order of visits; KH_ALIGN_EMPTY = no start state;
 *   KH_ALIGN_TOO_MANY_STATES = max_states > 0 and the construction holds more than max_states distinct tuples (the lattices
 *   for which :315 fires), no lattice returned - the reference returns the fragment its LIFO order had reached;
 *   KH_ALIGN_FATAL = the KALDI_ERR of :595-603 at some tuple, whichever other condition held, no lattice returned (too
 *   many states is reported before it).  n_tuples[l] = distinct tuples explored; max_states + 1 for
 *   KH_ALIGN_TOO_MANY_STATES (the construction stops at the tuple that pushes the count over), 0 for KH_ALIGN_EMPTY.
 * Outputs (HOST): per lattice status, n_states, n_arcs, n_tuples, n_string_words - always written; the three out_*_offsets
 * arrays (n_lats + 1 entries) are the room the caller leaves, and KH_EINVAL is returned, nothing else written, when a
 * lattice does not fit, so a second call with the room they name succeeds.  Lattice l's states at out_state_offsets[l]:
 * final weights (+inf, +inf = not final; final strings are empty); its arcs at out_arc_offsets[l], sorted by source state:
 * source, destination, label, graph and acoustic cost, string length; the strings one after the other in arc order at
 * out_string_offsets[l].  A status without a lattice has 0 states.
 * The construction runs on the device, one wave per lattice; the sort and the merges on the host.  Workspace per lattice in
 * flight: tables for 4 (states + arcs) + 64 tuples and twice as many (S, T) pairs, an arena of 4 x the lattice's
 * transition-ids + 16 (states + arcs) words; a lattice whose tables run full is run again with twice the room.  Lattices are taken largest first, as
 * many per launch as half of the free device memory admits, or as kh_compact_lattice_align_words_set_workspace_limit(bytes)
 * admits: a setting of the CALLING THREAD (0 = back to automatic; one lattice always runs).
 * kh_compact_lattice_align_words_last_timings: milliseconds the last call of this thread spent in { host preparation,
 * uploads, kernels with their memsets, downloads (HIP events), the whole call by the host's clock, the host's sort and
 * merge }, and counts3 (may be NULL) = { kernel launches, lattices run again with more room, tuples over all lattices }. */
#define KH_ALIGN_OK 0
#define KH_ALIGN_ERROR 1
#define KH_ALIGN_EMPTY 2
#define KH_ALIGN_TOO_MANY_STATES 3
#define KH_ALIGN_FATAL 4
int kh_compact_lattice_align_words(
    int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start, const int64_t *arc_offsets,
    const int32_t *arc_label, const int32_t *arc_nextstate, const float *arc_graph, const float *arc_acoustic,
    const int64_t *arc_string_offsets, const int32_t *arc_strings, const float *final_graph, const float *final_acoustic,
    const int64_t *final_string_offsets, const int32_t *final_strings, int num_tids, const int32_t *tid_phone,
    const int32_t *tid_is_final, const int32_t *tid_is_self_loop, int n_phone_types, const int32_t *phone_type, int reorder,
    int silence_label, int partial_word_label, const int32_t *max_states, int32_t *status, int32_t *n_states,
    int32_t *n_arcs, int32_t *n_tuples, int64_t *n_string_words, const int64_t *out_state_offsets,
    const int64_t *out_arc_offsets, const int64_t *out_string_offsets, float *out_final_graph, float *out_final_acoustic,
    int32_t *out_arc_src, int32_t *out_arc_nextstate, int32_t *out_arc_label, float *out_arc_graph, float *out_arc_acoustic,
    int32_t *out_arc_string_len, int32_t *out_strings);
int kh_compact_lattice_align_words_set_workspace_limit(size_t bytes);
int kh_compact_lattice_align_words_last_timings(float *ms6, int32_t *counts3);

/* RescoreCompactLattice = RescoreCompactLatticeInternal(NULL, 1.0, ...) (lat/lattice-functions.cc:1163-1290; gmm-rescore-lattice,
 * gmmbin/gmm-rescore-lattice.cc) with CompactLatticeStateTimes (:69-106) for a batch of top-sorted CompactLattices in one
 * call (csrc/kh_latrescore.hip).  HOST CSR as kh_compact_lattice_align_words takes it (every arc to a higher-numbered state;
 * the caller renumbers as fst::TopSort does, :1173-1178), with ONE transition-id array: arc a's string at
 * strings[arc_string_offsets[a] .. [a + 1]), state s's final string at strings[final_string_offsets[s] .. [s + 1]), n_strings
 * entries in all.  loglikes: DEVICE matrix of LogLikelihood(frame, pdf), lattice l's frames in rows ll_row_offsets[l] ..
 * [l + 1]; tid2pdf: HOST, TransitionIdToPdf as num_tids + 1 entries indexed by transition-id (entry 0 unused), every value a
 * column of the matrix.  arc_acoustic / final_acoustic: HOST, updated in place.
 * status[l], utt_len[l] (HOST, always written), decided on the host before anything runs, the first that holds:
 *   KH_RESCORE_EMPTY               no states or lat_start < 0 (:1169 "Rescoring empty lattice");
 *   KH_RESCORE_INCONSISTENT_TIMES  lat_start != 0 (:72), two paths of different length into one state (the assertion at :87),
 *                                  or a state that no path reaches (time -1, :1187);
 *   KH_RESCORE_MISMATCH            a string that begins past utt_len (:1200-1204 "lattice/feature mismatch"), or one that
 *                                  begins before utt_len and ends past it, where the reference writes past time_to_state;
 *   KH_RESCORE_FEATURES_TOO_SHORT  fewer rows than utt_len (:1221-1225; the last frame the reference names is rows - 1);
 *   KH_RESCORE_BAD_TID             a transition-id outside 1 .. num_tids in a string that would be looked up (the reference
 *                                  indexes unchecked);
 *   KH_RESCORE_OK                  rescored.  A row range longer than utt_len is fine.
 * utt_len: :77-105 - the maximum of time + final string length over the final states when they disagree, 0 without a final
 * state; 0 for EMPTY and INCONSISTENT_TIMES.  A lattice with another status than OK keeps every bit (the reference has by
 * then updated the frames before the one it stops at, and its caller drops the lattice).
 * THE ARITHMETIC.  The reference walks t ascending and adds -LogLikelihood(t, tid) to the weight that owns (t, tid) in
 * place (:1270, :1283), so for an arc from a state of time t0 (or a non-Zero final weight there) with string s_0 .. s_{n-1}
 *   v = old;  for k = 0 .. n-1:  v = fl32((-loglikes[row0 + t0 + k][tid2pdf[s_k]]) + v)
 * strictly in that order; an empty string keeps its bits (a -0.0 too), and so does a string that begins at utt_len (:1196).
 * One device work item per arc and per final weight with a string: a thread for strings of up to 8 transition-ids, a wave
 * for longer ones (it gathers 64 frames at a time and folds them in string order) - the same sums either way.
 * kh_rescore_compact_lattice_last_timings: milliseconds the last call of this thread spent in { host preparation (times,
 * statuses, item lists), uploads, kernels, downloads (HIP events), the whole call by the host's clock }, and counts3 (may
 * be NULL) = { kernel launches, items of the thread mapping, items of the wave mapping }. */
#define KH_RESCORE_OK 0
#define KH_RESCORE_EMPTY 1
#define KH_RESCORE_INCONSISTENT_TIMES 2
#define KH_RESCORE_FEATURES_TOO_SHORT 3
#define KH_RESCORE_BAD_TID 4
#define KH_RESCORE_MISMATCH 5
int kh_rescore_compact_lattice(
    int n_lats, const int32_t *lat_state_offsets, const int32_t *lat_start, const int64_t *arc_offsets,
    const int32_t *arc_nextstate, float *arc_acoustic, const int64_t *arc_string_offsets, const float *final_graph,
    float *final_acoustic, const int64_t *final_string_offsets, const int32_t *strings, int64_t n_strings,
    const float *loglikes, KhMatrixDim d_loglikes, const int32_t *ll_row_offsets, int num_tids, const int32_t *tid2pdf,
    int32_t *status, int32_t *utt_len);
int kh_rescore_compact_lattice_last_timings(float *ms5, int32_t *counts3);

/* Forced alignment of a batch of utterances, each against its own graph: FasterDecoder (decoder/faster-decoder.{h,cc}) as
 * AlignUtteranceWrapper drives it (decoder/decoder-wrappers.cc:456-482; gmm-align-compiled, nnet-align-compiled), with
 * max_active = INT_MAX.  One call = one Decode() per utterance with the given beam; the retry with a second beam is the
 * caller's second call over the utterances that came back KH_ALIGNC_NO_FINAL.
 *   Graphs: concatenated in the CSR layout of kaldi_io.read_fst.  state_offsets (n_utts + 1): the first state of every
 *   utterance; arc_offsets (all states + 1, int64): the arcs of every state, numbered over the batch; start, nextstate:
 *   state numbers inside the utterance; final_w: +inf = not final.  tid2pdf: HOST table of n_tid entries indexed by
 *   transition-id (NULL = ilabel - 1); every ilabel is 0 or in 1..n_tid-1.
 *   loglikes: DEVICE matrix of ll_rows x ll_cols floats with ll_stride, as for kh_decoder_decode: row t of utterance u at
 *   utt_row_offsets[u] + t (host, n_utts + 1), column tid2pdf[ilabel]; ac_cost = -loglikes.
 * Reproduced with the reference's own arithmetic: token costs are doubles formed as (prev + float arc weight) + float
 * ac_cost (faster-decoder.h:115-132); GetCutoff (:151-213) with its min_active branch, which takes the (min_active+1)-th
 * smallest cost AFTER rounding each to float (tmp_array_ is a vector<BaseFloat>), gives +inf for cutoff and adaptive beam
 * at <= min_active tokens, and forms adaptive_beam = float(min_active_cutoff - best + beam_delta); ProcessNonemitting
 * (:306-346) accepts at <= cutoff and a strictly better cost replaces; the initial closure of InitDecoding (:36-45);
 * ReachedFinal and the best final token (:78-112).
 * THE ONE DELIBERATE DIFFERENCE: ProcessEmitting (:263-300) accepts a candidate against next_weight_cutoff while that value
 * still tightens as the HashList is walked, so which marginal tokens exist depends on the list's order.  This library
 * accepts against the frame's FINAL value, min over all candidates from propagating tokens of (new_weight + adaptive_beam),
 * which does not depend on any order.  Every token the reference has and this library lacks is at least adaptive_beam worse
 * than the frame's best; it can matter only through the min_active count of the next frame or by a comeback.  The list's
 * order is not reproduced.
 * TIES: the reference gives equal costs to the first arrival in list order; this library to the lowest arc position in the
 * utterance's CSR among the candidates of one pass (an emitting arc is only replaced by a STRICTLY better eps arc; the eps
 * closure runs in rounds, each round relaxing every state from the costs of the round before), and among final tokens of
 * equal total cost to the lowest state.  The path is read from per-(frame, state) backpointers; where the reference's token
 * keeps pointing at a predecessor token that was later replaced by a better one whose cost rounds to the same sum, the
 * library's path goes through the replacement.
 * Output per utterance u, path room path_offsets[u+1] - path_offsets[u] (n_utts + 1 entries, first 0):
 *   status[u]      KH_ALIGNC_DONE; KH_ALIGNC_NO_FINAL = no final state active on the last frame; KH_ALIGNC_NEEDS_ROOM =
 *                  path_len[u] arcs do not fit the room: call again with that much (nothing is retried on the device);
 *                  KH_ALIGNC_TOO_LARGE = the backpointers of this one utterance exceed the workspace limit; KH_ALIGNC_BOUND =
 *                  a loop bound was hit: the eps closure still changed after states + 1 rounds (a negative eps cycle) or
 *                  the backpointers did not lead to the start within (frames + 1) * states steps; KH_ALIGNC_BAD_INPUT = the
 *                  graph was refused on the host (no start state, nextstate or ilabel out of range, a pdf outside the
 *                  matrix's columns, a weight that is not finite): nothing of it is launched, kh_last_error() names the
 *                  first such finding, the other utterances run.
 *   total_cost[u]  the best token's cost_ plus its final weight, a double (DONE and NEEDS_ROOM; +inf otherwise)
 *   best_state[u]  the state of that token, whose final weight GetBestPath puts on the path's end (:139-141); -1 otherwise
 *   path_len[u], and at path_offsets[u] the path's arcs in path order: path_ilabel, path_olabel, path_graph = the arc's
 *                  weight, path_acoustic = float(cost - prev cost) - graph, as GetBestPath forms them (:117-126).
 * Offsets that do not describe a batch (decreasing, rows outside the matrix) refuse the call with KH_EINVAL, as do
 * beam <= 0, min_active < 0 and beam_delta < 0.
 * One workgroup per utterance; workspace per utterance in flight: (frames + 1) x states int32 backpointers, plus 2 x states
 * doubles when the utterance has more states than the LDS admits (3584; kh_align_compiled_set_lds_states(n) lowers that for
 * the calling thread, 0 = always the workspace - a test aid).  Utterances are taken largest first, as many per launch as half
 * of the free device memory, or kh_align_compiled_set_workspace_limit(bytes) (calling thread; 0 = automatic), admits.
 * kh_align_compiled_last_timings: milliseconds the last call of this thread spent in { host preparation, uploads, kernels,
 * downloads (HIP events), the whole call by the host's clock }; counts3 (may be NULL) = { kernel launches, utterances whose
 * costs lay in the workspace, utterances launched }. */
#define KH_ALIGNC_DONE 0
#define KH_ALIGNC_NO_FINAL 1
#define KH_ALIGNC_NEEDS_ROOM 2
#define KH_ALIGNC_TOO_LARGE 3
#define KH_ALIGNC_BOUND 4
#define KH_ALIGNC_BAD_INPUT 5
int kh_align_compiled(int n_utts, const int32_t *state_offsets, const int64_t *arc_offsets, const int32_t *start,
                      const int32_t *ilabel, const int32_t *olabel, const float *weight, const int32_t *nextstate,
                      const float *final_w, int n_tid, const int32_t *tid2pdf, const float *loglikes, int ll_rows,
                      int ll_cols, int ll_stride, const int32_t *utt_row_offsets, float beam, int min_active,
                      float beam_delta, const int64_t *path_offsets, int32_t *status, double *total_cost,
                      int32_t *best_state, int32_t *path_len, int32_t *path_ilabel, int32_t *path_olabel, float *path_graph,
                      float *path_acoustic);
int kh_align_compiled_set_workspace_limit(size_t bytes);
int kh_align_compiled_set_lds_states(int max_states);
int kh_align_compiled_last_timings(float *ms5, int32_t *counts3);

/* LatticeForwardBackwardMpeVariants (lat/lattice-functions.cc:740-919): criterion
 * "smbr" (is_mpfe = 0) or "mpfe".  tid2phone / tid2pdf = TransitionIdToPhone /
 * TransitionIdToPdf as arrays of num_tids + 1 entries indexed by transition-id;
 * silence_phones sorted; num_ali = the numerator alignments concatenated
 * (num_ali_offsets[n_lats + 1]; lattice l needs max_time(l) entries, :764).
 * arc_post[a] = posterior_smbr of arc a (0 on epsilon arcs); the Posterior is
 * post[state_times[src(a)]] += (ilabel, arc_post[a]) merged as MergePairVectorSumming
 * (:916-917).  tot_forward_score[l] = the expected frame accuracy (:919); state_times
 * (optional) = LatticeStateTimes of every state.  Fails with
 * KH_ESTATE when one of the reference's forward/backward checks fails (:808, :909). */
int kh_lattice_forward_backward_mpe(int n_lats, const int32_t *lat_state_offsets,
                                    const int64_t *arc_offsets, const int32_t *arc_ilabel,
                                    const int32_t *arc_nextstate, const float *arc_graph,
                                    const float *arc_acoustic, const float *state_final,
                                    const int32_t *tid2phone, const int32_t *tid2pdf, int num_tids,
                                    const int32_t *silence_phones, int n_sil, const int32_t *num_ali,
                                    const int32_t *num_ali_offsets, int is_mpfe, int one_silence_class,
                                    float *arc_post, double *tot_forward_score, int32_t *state_times);

/* RescoreLattice (lat/lattice-functions.cc:1307-1358) with a matrix decodable: every
 * arc with a transition-id gets -loglikes[t][tid2pdf ? tid2pdf[tid] : tid - 1] added to
 * its acoustic cost (host array, updated in place), t = LatticeStateTimes of its source
 * state.  loglikes: DEVICE matrix, lattice l uses rows ll_row_offsets[l]...  Top-sorted
 * input required (the reference sorts first). */
int kh_rescore_lattice(int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets,
                       const int32_t *arc_ilabel, const int32_t *arc_nextstate, float *arc_acoustic,
                       const float *loglikes, int ll_stride, const int32_t *ll_row_offsets,
                       const int32_t *tid2pdf);

/* NnetDiscriminativeUpdater::LatticeComputations (nnet2/nnet-compute-discriminative.cc:178-321) for a batch
 * of examples, everything between the network output and the derivative on the device: Lookup + pseudo
 * log-likelihoods log(max(post, 1e-20) / prior) * acoustic_scale written into the denominator lattices
 * (:196-277), LatticeForwardBackwardMmi (criterion 0) or LatticeForwardBackwardMpeVariants ("smbr" 1, "mpfe" 2)
 * (:324-343), the Posterior algebra of hmm/posterior.cc (MergePairVectorSumming, ScalePosterior,
 * ConvertPosteriorToPdfs, AlignmentToPosterior, MergePosteriors with cancellation and drop_frames,
 * ScalePosterior(eg.weight)) and CompObjfAndDeriv (:301-316).
 * Host arrays: the denominator lattices as one top-sorted CSR batch (as kh_lattice_forward_backward), the
 * numerator alignments concatenated (num_ali_offsets[n_lats + 1] = also the row ranges of the examples in the
 * matrices), eg_weights[n_lats], tid2pdf / tid2phone [num_tids + 1] (tid2phone may be NULL for MMI),
 * silence_phones sorted, priors[cols].  DEVICE matrices: posteriors = the network output [sum T x num_pdfs],
 * deriv of the same size (zeroed, then deriv(row, pdf) = w / posteriors(row, pdf) for every merged entry).
 * stats[5] = { tot_num_count, tot_num_objf (MMI), tot_den_objf, CompObjfAndDeriv's tot_objf, tot_weight }.
 * --boost is not supported.  KH_EINVAL where the reference asserts (:194 rows vs frames, :220 lattice length
 * vs alignment length, unsorted lattice); KH_ESTATE when a forward/backward agreement check fails. */
int kh_discriminative_lattice_computations(
    int n_lats, const int32_t *lat_state_offsets, const int64_t *arc_offsets, const int32_t *arc_ilabel,
    const int32_t *arc_nextstate, const float *arc_graph, const float *arc_acoustic, const float *state_final,
    const int32_t *num_ali, const int32_t *num_ali_offsets, const float *eg_weights, const int32_t *tid2pdf,
    const int32_t *tid2phone, int num_tids, const int32_t *silence_phones, int n_sil, int criterion,
    float acoustic_scale, int drop_frames, int one_silence_class, const float *priors, const float *posteriors,
    KhMatrixDim d_posteriors, float *deriv, KhMatrixDim d_deriv, double *stats);

/* The same call with the denominator lattices as they sit in the examples - one set of host arrays per lattice
 * (NnetDiscriminativeUpdater::Propagate gets its examples one by one, nnet2/nnet-compute-discriminative.cc:150-175):
 * n_states[l], arc_offsets[l][n_states[l] + 1] (starting at 0), and per arc arc_ilabel[l], arc_nextstate[l] (state
 * numbers within the lattice), arc_graph[l], arc_acoustic[l]; state_final[l][n_states[l]].  The library assembles the
 * batch in pinned memory with a few host threads and uploads / prepares it on a stream of its own, beside the forward
 * pass the caller has launched on the library's stream and not waited for; only the steps that read `posteriors` are
 * ordered behind it.  Everything else as kh_discriminative_lattice_computations. */
int kh_discriminative_lattice_computations_parts(
    int n_lats, const int32_t *n_states, const int64_t *const *arc_offsets, const int32_t *const *arc_ilabel,
    const int32_t *const *arc_nextstate, const float *const *arc_graph, const float *const *arc_acoustic,
    const float *const *state_final, const int32_t *num_ali, const int32_t *num_ali_offsets, const float *eg_weights,
    const int32_t *tid2pdf, const int32_t *tid2phone, int num_tids, const int32_t *silence_phones, int n_sil, int criterion,
    float acoustic_scale, int drop_frames, int one_silence_class, const float *priors, const float *posteriors,
    KhMatrixDim d_posteriors, float *deriv, KhMatrixDim d_deriv, double *stats);

/* ... and in two halves, so that the NEXT batch's forward pass runs beside this batch's lattice work (a trainer's loop:
 * forward(i) queued; begin(i); forward(i + 1) queued; end(i); begin(i + 1); ...).  _begin assembles, uploads and prepares
 * the batch and queues every device step of the call on a stream of the call's own - the steps that read `posteriors`
 * behind an event recorded on the library's stream at the moment of the call, i.e. behind the forward pass queued just
 * before it - and returns without waiting.  _end waits for them, fills stats[5] and destroys the call (also when it
 * returns an error).  posteriors / deriv must stay valid until _end; two calls may be in flight. */
typedef struct KhDiscCall KhDiscCall;
int kh_discriminative_lattice_computations_begin(
    int n_lats, const int32_t *n_states, const int64_t *const *arc_offsets, const int32_t *const *arc_ilabel,
    const int32_t *const *arc_nextstate, const float *const *arc_graph, const float *const *arc_acoustic,
    const float *const *state_final, const int32_t *num_ali, const int32_t *num_ali_offsets, const float *eg_weights,
    const int32_t *tid2pdf, const int32_t *tid2phone, int num_tids, const int32_t *silence_phones, int n_sil, int criterion,
    float acoustic_scale, int drop_frames, int one_silence_class, const float *priors, const float *posteriors,
    KhMatrixDim d_posteriors, float *deriv, KhMatrixDim d_deriv, KhDiscCall **call);
int kh_discriminative_lattice_computations_end(KhDiscCall *call, double *stats);

/* CuMatrix::CompObjfAndDeriv (cudamatrix/cu-matrix.cc:1198-1248): the supervision
 * labels (row, column, weight) as three host arrays, output / deriv DEVICE matrices of
 * equal size: *tot_objf = sum w log output(r, c), *tot_weight = sum w,
 * deriv(r, c) += w / output(r, c). */
int kh_comp_objf_and_deriv(int n, const int32_t *rows, const int32_t *cols, const float *weights,
                           const float *output, KhMatrixDim d_output, float *deriv, KhMatrixDim d_deriv,
                           float *tot_objf, float *tot_weight);

/* MergePairVectorSumming (util/stl-utils.h:303-322) applied to every frame of a batch at once: the
 * step between the arc posteriors and the Posterior lists of hmm/posterior.cc
 * (lattice-functions.cc:351-352, ConvertPosteriorToPdfs, MergePosteriors).  HOST arrays: entries
 * (row = frame < n_rows, key = transition-id / pdf-id, weight) -> sorted by (row, key), equal keys
 * summed in input order, exact zeros dropped; the outputs hold at most n entries. */
int kh_merge_pair_vector_summing(int64_t n, const int32_t *rows, const int32_t *keys, const float *weights,
                                 int32_t n_rows, int32_t *out_rows, int32_t *out_keys, float *out_weights,
                                 int64_t *n_out);

/* The device radix sort behind the (frame row, pdf) order of kh_discriminative_lattice_computations, by
 * itself: HOST arrays of n (key, payload) pairs -> the pairs in the STABLE order of
 *   (key & ((1 << lo_bits) - 1)) | (key & (((1 << hi_bits) - 1) << 32)),
 * i.e. of the low lo_bits bits of the key's low word and the low hi_bits bits of its high word; the other
 * key bits take no part in the order and are carried through unchanged.  0 <= n < 2^31 and
 * 0 <= lo_bits, hi_bits <= 31 (a field of 0 bits takes no part), anything else is KH_EINVAL; n == 0
 * succeeds and writes nothing.  Runs on the library's stream and returns when the outputs are written. */
int kh_sort_pairs64(int64_t n, const uint64_t *keys, const int32_t *vals, int lo_bits, int hi_bits,
                    uint64_t *keys_out, int32_t *vals_out);

/* ------------------------------------------------------------------ f2
 * DeterminizeLatticePhonePrunedWrapper (lat/determinize-lattice-pruned.cc:1497-1519, called by
 * DecodeUtteranceLatticeFaster, decoder/decoder-wrappers.cc:264-274): the raw state-level
 * lattice (arrays as kh_decoder_get_raw_lattice returns them: state 0 = start, arcs with
 * ilabel = transition-id, olabel = word, weight (graph, acoustic); state_final = +inf for
 * non-final states, else the final graph cost) -> a CompactLattice deterministic on words
 * (acceptor: ilabel = olabel = word; weight = (graph, acoustic) + transition-id string), pruned
 * to `beam` (LatticeFasterDecoderConfig::lattice_beam).  delta / max_mem:
 * DeterminizeLatticePhonePrunedOptions (determinize-lattice-pruned.h:145-162; defaults
 * kDelta = 2^-10, 50000000; max_mem <= 0: unlimited).  Host code (as in the reference).
 * Returns NULL on bad arguments.  `complete` = 0 when the determinization stopped at the
 * memory limit ("Determinization finished earlier than the beam", decoder-wrappers.cc:272). */
typedef struct KhCompactLattice KhCompactLattice;
KhCompactLattice *kh_determinize_lattice_pruned(int n_states, int n_arcs, const int32_t *arc_src, const int32_t *arc_dst,
                                                const int32_t *arc_ilabel, const int32_t *arc_olabel,
                                                const float *arc_graph, const float *arc_acoustic,
                                                const float *state_final, double beam, float delta, int64_t max_mem);
/* The same with every option of DeterminizeLatticePhonePrunedOptions (lat/determinize-lattice-pruned.h:145-175):
 * phone_determinize = the first pass on phone + word labels (:1386-1404), which needs what the reference asks its
 * TransitionModel per transition-id (:1335-1338): tid_phone[tid] = TransitionIdToPhone(tid) when
 * TransitionIdToHmmState(tid) == 0 && !IsSelfLoop(tid), else 0 (n_tid entries, index 0 unused); word_determinize = the
 * pass on words; minimize = PushCompactLatticeStrings + PushCompactLatticeWeights + MinimizeCompactLattice
 * (lat/push-lattice.cc, lat/minimize-lattice.cc).  The reference's defaults are (1, 1, 0);
 * kh_determinize_lattice_pruned is (0, 1, 0). */
KhCompactLattice *kh_determinize_lattice_phone_pruned(int n_states, int n_arcs, const int32_t *arc_src, const int32_t *arc_dst,
                                                      const int32_t *arc_ilabel, const int32_t *arc_olabel,
                                                      const float *arc_graph, const float *arc_acoustic,
                                                      const float *state_final, const int32_t *tid_phone, int n_tid,
                                                      double beam, float delta, int64_t max_mem, int phone_determinize,
                                                      int word_determinize, int minimize);
int kh_compact_lattice_sizes(const KhCompactLattice *clat, int32_t *n_states, int32_t *n_arcs,
                             int32_t *n_arc_string_labels, int32_t *n_final_string_labels, int32_t *complete);
/* arcs sorted by source state; arc_string_offsets has n_arcs + 1 entries, final_string_offsets
 * n_states + 1; final_graph / final_acoustic = +inf for non-final states.  NULL skips an array. */
int kh_compact_lattice_get(const KhCompactLattice *clat, int32_t *arc_src, int32_t *arc_dst, int32_t *arc_label,
                           float *arc_graph, float *arc_acoustic, int32_t *arc_string_offsets, int32_t *arc_strings,
                           float *final_graph, float *final_acoustic, int32_t *final_string_offsets,
                           int32_t *final_strings);
void kh_compact_lattice_free(KhCompactLattice *clat);

/* ------------------------------------------------------------------ f3
 * OnlineIvectorFeature (online2/online-ivector-feature.{h,cc}) in its deterministic mode: no
 * silence weighting, use_most_recent_ivector = false, a fresh OnlineIvectorExtractorAdaptationState
 * per utterance (no speaker CMVN stats).  The configuration is OnlineIvectorExtractionInfo
 * (online-ivector-feature.h:51-134) with its member models:
 *   lda_mat [feat_dim x lda_cols] (lda_cols = base_dim * (left + right + 1), + 1 for an offset
 *   column), global_cmvn_stats [2 x (base_dim + 1)] double (matrix of OnlineCmvn), diag UBM
 *   (gconsts, means_invvars, inv_vars as kh_diag_gmm_loglikes), IvectorExtractor: M
 *   [num_gauss][feat_dim][ivector_dim], Sigma_inv [num_gauss][feat_dim][feat_dim], prior_offset —
 * all HOST arrays, uploaded once; the derived U_i / Sigma_i^-1 M_i
 * (IvectorExtractor::ComputeDerivedVars, ivector/ivector-extractor.cc:186-217) are computed at
 * creation.  Returns NULL when OnlineIvectorExtractionInfo::Check (online-ivector-feature.cc:70-87)
 * would fail or a limit is exceeded (base_dim <= 64, num_gauss <= 2048, num_gselect <= 16,
 * ivector_dim, feat_dim <= 256). */
typedef struct KhIvectorConfig {
  int32_t base_dim, splice_left, splice_right, feat_dim, num_gauss, ivector_dim, lda_cols;
  int32_t cmn_window, speaker_frames, global_frames, normalize_mean, normalize_variance; /* OnlineCmvnOptions */
  int32_t ivector_period, num_gselect, num_cg_iters;
  float min_post, posterior_scale, max_count;
  double prior_offset;
  /* 1: use_most_recent_ivector + greedy_ivector_extractor (what --online=false sets,
   * online2-wav-nnet2-latgen-faster.cc: one estimate from all the frames of the utterance on every row);
   * 0: use_most_recent_ivector = false (row t: the estimate of frame (t / period) * period) */
  int32_t greedy_most_recent;
} KhIvectorConfig;
typedef struct KhIvectorExtractor KhIvectorExtractor;
KhIvectorExtractor *kh_ivector_extractor_create(const KhIvectorConfig *cfg, const float *lda_mat,
                                                const double *global_cmvn_stats, const float *ubm_gconsts,
                                                const float *ubm_means_invvars, const float *ubm_inv_vars,
                                                const double *M, const double *Sigma_inv);
void kh_ivector_extractor_destroy(KhIvectorExtractor *ext);
/* OnlineIvectorFeature::GetFrame for every frame of a batch of utterances
 * (online-ivector-feature.cc:286-299): feats = DEVICE base features, the utterances row-
 * concatenated, utterance u = rows [utt_row_offsets_host[u], utt_row_offsets_host[u + 1]);
 * ivectors = DEVICE [rows x ivector_dim]: row t holds the iVector estimated from frames
 * 0 .. (t / ivector_period) * ivector_period of its utterance, first dimension minus
 * PriorOffset. */
int kh_ivector_extract(const KhIvectorExtractor *ext, const float *feats, int feat_stride,
                       const int32_t *utt_row_offsets_host, int n_utts, float *ivectors, int ivector_stride);
/* The same with the speaker's OnlineIvectorExtractorAdaptationState (online-ivector-feature.h:138-176:
 * SetAdaptationState before the utterance, GetAdaptationState after it, :151-171): per utterance
 * kh_ivector_state_dim(ext) HOST doubles — CMVN speaker stats [2 x (base_dim + 1)], num_frames, the prior's
 * share of the quadratic diagonal, the linear term [ivector_dim], the per-Gaussian counts [num_gauss] (the
 * quadratic term is diag * I + sum_g count_g U_g).  state_in NULL: fresh speakers; state_out: the state
 * BEFORE LimitFrames (the caller applies it, as GetAdaptationState does, and chains the utterances of a
 * speaker through successive calls). */
int kh_ivector_state_dim(const KhIvectorExtractor *ext);
int kh_ivector_extract_adapt(const KhIvectorExtractor *ext, const float *feats, int feat_stride,
                             const int32_t *utt_row_offsets_host, int n_utts, const double *state_in_host,
                             double *state_out_host, float *ivectors, int ivector_stride);

/* OnlineIvectorFeature WITH FRAME WEIGHTS (online2/online-ivector-feature.h:299-362, .cc:155-254) for n utterances
 * side by side - the feature side of the decoder-traceback silence weighting (--ivector-silence-weighting.*,
 * online2-wav-nnet2-latgen-faster.cc:239-244).  create: the utterances' base features (DEVICE, row-concatenated),
 * the adaptation states they start from (layout of kh_ivector_extract_adapt, NULL = fresh) and the DEVICE matrix
 * [sum T x ivector_dim] whose rows the object fills as their estimation points are reached.  The per-frame inputs
 * that do not depend on the weights (lda_ features, pruned UBM posteriors) are computed here, once.
 *   update_frame_weights(stream, (frame, delta weight)...)  = UpdateFrameWeights() :155-170; num_frames_ready =
 *       NumFramesReady() of the stream at the time of the call (frames >= it are refused as the reference asserts)
 *   get_frames(streams, until_frame)  = what GetFrame(until_frame) triggers: UpdateStatsUntilFrameWeighted()
 *       :215-254 when weights were supplied, UpdateStatsUntilFrame() :191-213 otherwise, for all listed streams in
 *       one launch; rows [0, until_frame] of the streams' iVector matrix are valid afterwards
 *   get_stats(states_out [n x state_dim])  = the OnlineIvectorEstimationStats part of GetAdaptationState() :283-293
 *       (num_frames, quadratic diagonal share, linear term, per-Gaussian counts); the CMVN part of the state vectors
 *       is left untouched (it does not depend on the weights: kh_ivector_extract_adapt over the accepted frames).
 * use_most_recent_ivector / greedy_ivector_extractor are refused.  KH_ESTATE where the reference asserts
 * (a frame asked for beyond the most recent weight, a frame's weight leaving [0, 1]). */
typedef struct KhIvectorStreams KhIvectorStreams;
KhIvectorStreams *kh_ivector_streams_create(const KhIvectorExtractor *x, const float *feats, int feat_stride,
                                            const int32_t *utt_row_offsets, int n_utts, const double *state_in,
                                            float *ivectors, int ivector_stride);
void kh_ivector_streams_destroy(KhIvectorStreams *s);
int kh_ivector_streams_update_frame_weights(KhIvectorStreams *s, int stream, int n, const int32_t *frames,
                                            const float *delta_weights, int num_frames_ready);
int kh_ivector_streams_get_frames(KhIvectorStreams *s, int n, const int32_t *streams, const int32_t *until_frame);
int kh_ivector_streams_get_stats(const KhIvectorStreams *s, double *states_out);

/* ------------------------------------------------------------------ fMLLR estimation (csrc/kh_fmllr.hip)
 * gmm-est-fmllr / gmm-est-fmllr-gpost / gmm-post-to-gpost for a batch of speakers, in four stages with explicit inputs and
 * outputs.  A per-utterance run is one speaker per utterance.  Common layout: the frames of all utterances stacked by rows
 * (feats: DEVICE, T x D, row pitch feat_stride); utt_row_offsets[n_utts + 1] and spk_utt_offsets[n_spk + 1] HOST, a
 * speaker's utterances contiguous in spk2utt order; the (frame, pdf) entries in CSR form over frames, HOST:
 * frame_entry_offsets[T + 1], entry_pdf[], entry_weight[]; within a frame in ascending pdf order by convention (the
 * reference's order is an unordered_map's; the library takes the order given).  entry_gauss_offsets[E + 1] HOST: the running
 * sum of the entries' pdf sizes, built by the caller and checked here.  Model arrays (gconsts, means_invvars, inv_vars) DEVICE
 * as kh_diag_gmm_loglikes takes them, pdf_offsets[num_pdfs + 1] HOST.  Every index is checked on the host before a launch.
 *
 * A1  DiagGmm::ComponentPosteriors (gmm/diag-gmm.cc:601-615) with VectorBase::ApplySoftMax (matrix/kaldi-vector.cc:840-847)
 *     and the Scale(weight) of FmllrDiagGmmAccs::AccumulateForGmm (transform/fmllr-diag-gmm.cc:108-109), per entry:
 *     gauss_post (DEVICE, entry_gauss_offsets[E] floats) = softmax of the entry's per-Gaussian scores times its weight,
 *     entry_like (DEVICE, E floats) = max + log(sum), the value gmm-post-to-gpost sums (gmm-post-to-gpost.cc:118-121).
 *     Scores: kh_diag_gmm_loglikes's fmaf chains, bit for bit; then float max, fl32(f - max), expf, float sum in Gaussian
 *     order, times fl32(1.0 / sum), times the weight; expf and logf are the device math library's. */
int kh_gmm_component_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts,
                                const float *means_invvars, const float *inv_vars, const int32_t *pdf_offsets, int num_pdfs,
                                const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const float *entry_weight,
                                const int64_t *entry_gauss_offsets, float *gauss_post, float *entry_like);
/* A2  FmllrDiagGmmAccs::AccumulateFromPosteriors (fmllr-diag-gmm.cc:30-43) for given Gaussian posteriors (DEVICE) and a
 *     model's means_invvars / inv_vars - the model of A1, or another one with the same Gaussian counts (the two-model case of
 *     gmm-est-fmllr-gpost.cc:36-52); KH_EINVAL naming the pdf where a count differs.  Output per MERGED FRAME, restating
 *     DataHasChanged / InitSingleFrameStats / CommitSingleFrameStats (:542-596): within a speaker, over the frames that have
 *     entries and across its utterance boundaries, a frame whose row equals (float ==, every element) the previous such frame's
 *     row joins it; the entries are concatenated.  HOST outputs: run_row[] (the first row of each merged frame; room for T),
 *     spk_run_offsets[n_spk + 1].  DEVICE outputs, room for T merged frames: a, b [. x D] float (fmaf chains over the merged
 *     frame's entries in order, each entry's Gaussians in order), count [.] double (adds each entry's float posterior sum). */
int kh_fmllr_frame_stats(const float *feats, int T, int D, int feat_stride, const float *means_invvars, const float *inv_vars,
                         const int32_t *pdf_offsets, int num_pdfs, const int32_t *utt_row_offsets, int n_utts,
                         const int32_t *spk_utt_offsets, int n_spk, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                         const int64_t *entry_gauss_offsets, const float *gauss_post, int32_t *run_row, int32_t *spk_run_offsets,
                         float *a, float *b, double *count);
/* B   FmllrDiagGmmAccs::CommitSingleFrameStats (fmllr-diag-gmm.cc:562-596, update type "full") over every speaker's merged
 *     frames, in double: beta[n_spk], K[n_spk][D][D + 1], G[n_spk][D][(D + 1)(D + 2) / 2] (SpMatrix packing: (r, c), r >= c, at
 *     r (r + 1) / 2 + c), HOST outputs.  A merged frame whose count is 0 adds nothing (:566).  fp64 matrix-core GEMM with the
 *     scatter operand made on the fly; partial sums per chunk of kh_fmllr_frame_chunk merged frames, added in chunk order: the
 *     same input gives the same bits.  D = 1 ... kh_fmllr_max_dim (63); above: KH_EINVAL before any launch. */
int kh_fmllr_accumulate(const float *feats, int T, int D, int feat_stride, const int32_t *run_row, const int32_t *spk_run_offsets,
                        int n_spk, const float *a, const float *b, const double *count, double *beta, double *K, double *G);
/* C   FmllrDiagGmmAccs::Update (fmllr-diag-gmm.cc:131-166) from a unit transform, per speaker: ComputeFmllrMatrixDiagGmmFull
 *     with FmllrInnerUpdate (:193-273), ...Diagonal (:275-348), ...Offset (:350-378), "none", FmllrAuxFuncDiagGmm (:481-508);
 *     min_count and "objective function did not increase -> keep" included.  HOST code in double, needs no device;
 *     num_threads <= 16 threads over speakers (0 = 16).  transforms [n_spk][D][D + 1] float, objf_impr, count [n_spk] float.
 *     "diag" and "offset" read only the three elements per G_i that the reference would have accumulated for them. */
int kh_fmllr_update(int n_spk, int D, const double *beta, const double *K, const double *G, const char *update_type, float min_count,
                    int num_iters, int num_threads, float *transforms, float *objf_impr, float *count);
int kh_fmllr_max_dim(void);
int kh_fmllr_frame_chunk(void);
/* B takes the speakers in groups whose workspace (one partial sum per chunk and one sum per speaker, D P + D (D + 1) doubles
 * each) stays within this many bytes (calling thread; 0 = the default, 1 GiB); a speaker is never split.  No sum depends on it. */
int kh_fmllr_set_workspace_limit(size_t bytes);
/* ms[6]: milliseconds of the calling thread's last A1, A2, B and C calls (whole call, transfers and waits included), of B's
 * kernels alone (device events), and the number of speaker groups B took. */
int kh_fmllr_last_timings(float *ms);

/* ------------------------------------------------------------------ GMM training statistics (csrc/kh_gmmacc.hip)
 * The E-step of gmm-acc-stats-ali / gmm-acc-stats / gmm-acc-stats-twofeats for a batch of stacked frames: for given Gaussian
 * posteriors (kh_gmm_acc_component_posteriors below, stage A1 above, or any given ones) AccumDiagGmm::AccumulateFromPosteriors (gmm/mle-diag-gmm.cc:171-189) under
 * AccumulateFromDiag (:191-204) under AccumAmDiagGmm::AccumulateForGmm / AccumulateForGmmTwofeats
 * (gmm/mle-am-diag-gmm.cc:69-97).  Per Gaussian g of each pdf, in double, over the entries e that name the pdf:
 *     occ[g] += p[e, g],   mean_acc[g, d] += p[e, g] x[row(e), d],   var_acc[g, d] += p[e, g] x[row(e), d]^2,
 * p the float posterior (already times the entry's weight) and x the float feature row, both widened first.  feats (DEVICE,
 * T x D, row pitch feat_stride) are the features the STATISTICS are taken from: their D need not be the model's (the
 * two-feature route).  The entry list is A1's (HOST), gauss_post DEVICE.  flags: kGmmMeans 1 | kGmmVariances 2 | kGmmWeights 4
 * after AugmentGmmFlags (gmm/model-common.cc:52-61: v needs m, m needs w); an accumulator the flags exclude is not touched
 * and may be NULL.  HOST outputs occ [NG], mean_acc, var_acc [NG x D] (NG = pdf_offsets[num_pdfs]) are SET, not added to; a
 * pdf no entry names gets zeros; T = 0 or no entries: zeros.  Every index is checked on the host before a launch (KH_EINVAL
 * naming the pdf or entry).  The entries are sorted by pdf (stable: frame order within a pdf) and a pdf's run is cut into
 * chunks of kh_gmm_acc_chunk entries; per pdf an fp64 matrix-core GEMM P^T [1 | X | X o X] with the right operand made on the
 * fly, partial sums per chunk added in chunk order, no atomics: the same input gives the same bits.  The sum order is this
 * chunk tree's, not the reference's BLAS order.  D = 1 ... kh_gmm_acc_max_dim (127); above: KH_EINVAL before any launch.
 * total_log_like_ / total_frames_ (mle-am-diag-gmm.cc:76-77) are host sums over the posteriors call's entry_like, left to the caller. */
int kh_gmm_acc_stats(const float *feats, int T, int D, int feat_stride, const int32_t *pdf_offsets, int num_pdfs,
                     const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const int64_t *entry_gauss_offsets,
                     const float *gauss_post, int flags, double *occ, double *mean_acc, double *var_acc);
/* The Gaussian posteriors of this route: kh_gmm_component_posteriors' arguments, checks and arithmetic (stage A1 above), with
 * EXP and LOG as fl32 of the double function (the device library's double exp / log, under 1 ulp in double), which is how the
 * line-by-line restatement of DiagGmm::ComponentPosteriors states them, where A1 takes the device library's expf / logf (1 ulp in
 * float).  The checks are those of kh_gmm_acc_stats (csrc/kh_gmmacc_plan.h).  The statistics go to a file as floats: with 1-ulp
 * posteriors a mean accumulator whose addends cancel moves by several float ulps, with these it does not. */
int kh_gmm_acc_component_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts,
                                    const float *means_invvars, const float *inv_vars, const int32_t *pdf_offsets, int num_pdfs,
                                    const int64_t *frame_entry_offsets, const int32_t *entry_pdf, const float *entry_weight,
                                    const int64_t *entry_gauss_offsets, float *gauss_post, float *entry_like);
int kh_gmm_acc_chunk(void);
int kh_gmm_acc_max_dim(void);
/* The pdfs go in groups whose workspace ((chunks + 1) x Gaussians x columns doubles per pdf: a partial sum per chunk and the
 * sum) stays within this many bytes (calling thread; 0 = the default, 1 GiB); a pdf is never split.  No sum depends on it. */
int kh_gmm_acc_set_workspace_limit(size_t bytes);
/* ms[4]: milliseconds of the calling thread's last kh_gmm_acc_stats: the whole call, its host plan (checks, sort, groups), its
 * two kernels alone (device events); then of its last kh_gmm_acc_component_posteriors (whole call).  counts[3]: pdf groups,
 * chunks, workgroups of the accumulation kernel. */
int kh_gmm_acc_last_timings(float *ms, int32_t *counts);

/* ------------------------------------------------------------------ MLLT statistics (csrc/kh_mllt.hip)
 * gmm-acc-mllt for a batch of stacked frames: MlltAccs::AccumulateFromPosteriors (transform/mllt.cc:131-160) for every entry,
 * for given Gaussian posteriors that RandPrune has ALREADY been applied to (kh_gmm_acc_component_posteriors' output, brought
 * to the host, through kh_rand_prune, and back).  Per (entry, Gaussian) item i with a nonzero posterior p, in float,
 *     mean[d] = fl32(means_invvars[g, d] / inv_vars[g, d]),  o[d] = fl32(mean[d] - x[row, d]),  w[j] = fl32(inv_vars[g, j] * p)
 * (the division correctly rounded), and in double, for every j and every packed pair a >= b,
 *     G[j][a (a + 1) / 2 + b] += w[j] * (o[a] * o[b]),
 * o and w widened first, so that o[a] * o[b] is exact.  feats, means_invvars, inv_vars, gauss_post: DEVICE; the entry list is
 * kh_gmm_acc_stats' (HOST) and is checked in the same way before any launch (KH_EINVAL naming the pdf or entry).  HOST output
 * G [D][Q], Q = D (D + 1) / 2, row j the packed SpMatrix G_j, is SET, not added to; no item: zeros.  beta_ (the double sum
 * of the surviving posteriors) is the caller's.
 * The items are taken in entry order then Gaussian order and cut into slices of
 *     kh_mllt_chunk * max(1, ceil(n / (kh_mllt_chunk * kh_mllt_max_slices)))
 * items; per slice an fp64 matrix-core GEMM W^T T with both operands made on the fly, the slices' partial sums added in
 * slice order by a second kernel: the same input gives the same bits, and no setting changes a sum.  The sum order is this
 * tree's, not the reference's frame-by-frame one.  D = 1 ... kh_mllt_max_dim (64); above: KH_EINVAL before any launch. */
int kh_mllt_acc_stats(const float *feats, int T, int D, int feat_stride, const float *means_invvars, const float *inv_vars,
                      const int32_t *pdf_offsets, int num_pdfs, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                      const int64_t *entry_gauss_offsets, const float *gauss_post, double *G);
/* RandPrune (base/kaldi-math.h:169-175) on post[0 .. n) (HOST) in place and in order; host code, no device.  A value that is
 * 0 or whose magnitude is >= thresh stays; any other takes one draw u = float((rand() + 1.0) / (RAND_MAX + 2.0)) of the C
 * library's rand() (under a mutex, as the reference's Rand()) and becomes (post >= 0 ? 1.0 : -1.0) * (u <= q ? thresh : 0.0)
 * rounded to float - a negative value pruned away is -0.0, as there.  q: the reference writes fabs(post) / prune_thresh
 * inside namespace kaldi with only <cmath> included; unqualified fabs finds the C library's ::fabs(double), not the float
 * overload of std::fabs, so the quotient is the DOUBLE division double(|post|) / double(thresh) and u is widened for the
 * comparison.  That is what this function does.  reseed != 0: srand(seed) first (a process that never seeds draws the
 * sequence of srand(1)).  thresh < 0: KH_EINVAL; thresh == 0: nothing changes and nothing is drawn. */
int kh_rand_prune(float *post, int64_t n, float thresh, int reseed, unsigned seed);
/* The same after positioning the generator: srand(seed), `skip` draws discarded, then RandPrune; *draws: the draws taken
 * (one per value that is neither 0 nor >= thresh in magnitude).  A process that uses the GPU does not own the generator's
 * state - the HIP runtime reseeds the C library's generator when it initialises and draws from it at some first uses - so
 * "never seed and the sequence is the reference's" does not hold there.  A job pruned in several calls passes seed 1 (the
 * state of a process that never seeded) and the sum of the earlier calls' draws: the posteriors then meet the draws the
 * reference binary's would, call after call.  The cost is `skip` calls of rand(), some nanoseconds each. */
int kh_rand_prune_at(float *post, int64_t n, float thresh, unsigned seed, int64_t skip, int64_t *draws);
int kh_mllt_chunk(void);
int kh_mllt_max_slices(void);
int kh_mllt_max_dim(void);
/* ms[3]: milliseconds of the calling thread's last kh_mllt_acc_stats: the whole call, its host plan (checks, the posteriors'
 * download, the item list), its two kernels alone (device events).  counts[3]: items, slices, workgroups of the accumulation
 * kernel (slices x groups of 16 column tiles). */
int kh_mllt_last_timings(float *ms, int32_t *counts);

/* ------------------------------------------------------------------ LDA statistics (csrc/kh_lda.hip)
 * acc-lda for a batch of stacked frames: LdaEstimate::Accumulate (transform/lda-estimate.cc:45-55) for every (frame, pdf,
 * weight) entry whose weight is not zero (-0.0 is zero), the weights being those RandPrune has ALREADY been applied to
 * (kh_rand_prune_at).  feats (DEVICE, T x D, row pitch feat_stride); the entry list is HOST: frame_entry_offsets [T + 1],
 * entry_pdf [E], entry_weight [E].  segment_frame_offsets [num_segments + 1] (HOST): the utterances of the call, from 0 to T
 * (NULL: one segment).  Per item, w and x widened to double,
 *     zero[c] += w,   first[c][d] += w x[d],   second[a (a + 1) / 2 + b] += (w x[a]) x[b]   for a >= b,
 * HOST outputs zero [num_classes], first [num_classes x D], second [D (D + 1) / 2] packed as SpMatrix packs.  add == 0: the
 * outputs are SET; add != 0: the sums are added to what they hold.  T = 0 or no item: zeros, or unchanged under add.
 * The sum tree depends on the input alone.  The items are in entry order.  `second`: a segment's items are cut into slices of
 *     kh_lda_chunk * max(1, ceil(n_seg / (kh_lda_chunk * kh_lda_max_slices)))
 * items, per slice the lower triangle of an fp64 matrix-core X^T diag(w) X with both operands made on the fly; a segment's
 * sum is its slices' partial sums added in slice order from zero, and the segments' sums are added one after another in
 * segment order onto (add ? the buffer : zero).  `first`, `zero`: per (segment, class) the class's items in entry order in
 * chunks of kh_lda_chunk, the chunks' partial sums added in chunk order from zero, then the segments in order in the same
 * way.  No atomics: the same input gives the same bits, and a job gives the same bits however its segments are grouped into
 * calls that run on from one another with add.  D = 1 ... kh_lda_max_dim (512).  Before any launch, KH_EINVAL naming the
 * offender: D above the limit, a pdf outside 0 .. num_classes - 1, offsets that run backwards, segments that do not run from
 * 0 to T. */
int kh_lda_acc_stats(const float *feats, int T, int D, int feat_stride, const int64_t *frame_entry_offsets, const int32_t *entry_pdf,
                     const float *entry_weight, int num_classes, const int64_t *segment_frame_offsets, int num_segments, int add,
                     double *zero, double *first, double *second);
/* The slices' partial sums (D (D + 1) / 2 doubles each) go to a workspace of at most this many bytes (calling thread; 0 = the
 * default, 1 GiB): a call is cut into passes over runs of whole slices, one accumulation and one reduction launch per pass.
 * No sum depends on it.  A limit below one slice's partial sums: kh_lda_acc_stats returns KH_ENOMEM naming the bytes needed,
 * before any launch. */
int kh_lda_set_workspace_limit(size_t bytes);
int kh_lda_chunk(void);
int kh_lda_max_slices(void);
int kh_lda_max_dim(void);
/* ms[3]: milliseconds of the calling thread's last kh_lda_acc_stats: the whole call, its host plan (checks, item list, slices,
 * sort by class), its kernels alone (device events).  counts[4]: items, slices, workgroups of the accumulation kernel (slices
 * x pairs of 64-column super tiles), passes. */
int kh_lda_last_timings(float *ms, int32_t *counts);

/* ------------------------------------------------------------------ tree statistics (csrc/kh_tree.hip)
 * acc-tree-stats for a batch of stacked frames: GaussClusterable::AddStats(row, 1.0) (tree/clusterable-classes.cc:137-142)
 * for every frame whose event the caller has worked out (AccumulateTreeStats, hmm/tree-accu.cc:56-104).  feats (DEVICE, T x
 * D, row pitch feat_stride); frame_event (HOST, T entries): the frame's event 0 ... num_events - 1, or -1 for a frame that is
 * not used.  HOST outputs count [num_events] and stats [num_events x 2 x D] (an event's first-order row, then its
 * second-order row).  For every event e and column d, from the incoming value (add != 0) or from zero (add == 0: the
 * buffers are overwritten), over the frames with frame_event[t] == e in ascending t, x = feats[t][d]:
 *     stats[e][0][d] += (double)x,   stats[e][1][d] += (double)(float)(x * x)
 * - the product rounded to float and then widened, as AddVec2's alpha == 1.0 branch has it, never fused with the add - and
 * count[e] becomes its prior value (or zero) plus the number of those frames, which is exact below 2^53.  One chain of double
 * adds per (event, column), never cut into partial sums, no atomics: the result is bit-equal to the reference's loop, and a
 * job gives the same bits however it is cut into calls that run on from one another with add.  An event without a frame keeps
 * what it holds under add and is zero without.  COST: stats travels whole - all num_events rows go up under add and all come
 * back, events without a frame included (16 D bytes per event each way) - so give the call the events the frames touch, as
 * api.TreeStats does, not a job's whole table.  (Moving only the touched rows was built and measured: packing and unpacking
 * them on the host cost more than the bytes it saved at two thirds of the events touched.)  T = 0 and num_events = 0 are valid.  D = 1 ... kh_tree_max_dim (512).
 * Before any launch, KH_EINVAL naming the offender: D outside that range, feat_stride below D, a frame whose event lies
 * outside -1 ... num_events - 1. */
int kh_tree_acc_stats(const float *feats, int T, int D, int feat_stride, const int32_t *frame_event, int num_events, int add,
                      double *count, double *stats);
int kh_tree_max_dim(void);
/* Rows of an event's run staged per step (the tests' edge counts: runs of tile - 1, tile, tile + 1 frames). */
int kh_tree_tile(void);
/* ms[3]: milliseconds of the calling thread's last kh_tree_acc_stats: the whole call, its host plan (check, counting sort by
 * event, work list), its kernel alone (device events).  counts[4]: frames with an event, events with a frame, work items
 * (one wave per event with a frame and block of 64 columns), frames of the longest event. */
int kh_tree_last_timings(float *ms, int32_t *counts);

/* ------------------------------------------------------------------ Gaussian selection (csrc/kh_gselect.hip)
 * gmm-gselect and the gselect branch of gmm-global-acc-stats for a batch of stacked frames and ONE DiagGmm (gconsts [G],
 * means_invvars / inv_vars [G x D], DEVICE; feats DEVICE, T x D, row pitch feat_stride).
 *
 * kh_gmm_gselect: DiagGmm::GaussianSelection(const MatrixBase&, ...) (gmm/diag-gmm.cc:801-871), its per-frame form (:765-799)
 * and, with a preselection, GaussianSelectionPreselect (:875-916).  pre_offsets [T + 1] / pre_gauss (HOST, CSR; both NULL:
 * no preselection).  DEVICE outputs: sel [T x n_out] int32, n_out = min(num_gselect, num_gauss), a frame's Gaussians best
 * first, padded with -1; sel_count [T]; frame_like [T]; status [T].
 *   Scores: without a preselection kh_diag_gmm_loglikes' values bit for bit (that call, on row chunks into a workspace); with
 *   one the same k-ordered fmaf chains over the listed Gaussians, ll = (g + a1) + (-0.5f * a2).  This is the library's one
 *   order for both branches of DiagGmm::LogLikelihoodsPreselect (:566-598): the reference takes BLAS on a contiguous range of
 *   indices and VecVec per Gaussian otherwise.  (It decides "contiguous" from the first and last index alone, :575, so an
 *   unsorted list with back + 1 - front == size is scored there as that RANGE; the library scores the Gaussians listed.)
 *   Selection: the reference's nth_element, >= thresh, std::sort by std::greater<pair<float, int32>>, first n - that is, the
 *   n largest under the total order (score descending, then index descending), scores compared as floats (+0 == -0: the index
 *   decides); with a preselection position p carries preselect[p] as its index and n = min(num_gselect, list size) per frame.
 *   frame_like: tot = LogAdd(tot, score_j) over the selected, best first, from -inf - the float LogAdd (base/kaldi-math.h:
 *   198-215), Exp and Log1p being the float of the double function.
 *   A frame with a NaN score (the reference's nth_element is undefined there): status 1, sel_count 0, its row of sel -1,
 *   frame_like NaN; the call still returns KH_OK and the other frames have status 0.
 * Before any launch, KH_EINVAL naming the offender: num_gauss outside 1 ... kh_gselect_max_gauss (4096), num_gselect outside
 * 1 ... kh_gselect_max_n (128), D outside 1 ... kh_gselect_max_dim (96, kh_diag_gmm_loglikes'), feat_stride below D; of a
 * preselection: offsets not from 0 or running backwards, an index outside [0, num_gauss), an empty list, a list longer than
 * num_gauss (a Gaussian MAY be listed twice here, as in the reference).  T = 0 is valid. */
int kh_gmm_gselect(const float *feats, int T, int D, int feat_stride, const float *gconsts, const float *means_invvars,
                   const float *inv_vars, int num_gauss, int num_gselect, const int64_t *pre_offsets, const int32_t *pre_gauss,
                   int32_t *sel, int32_t *sel_count, float *frame_like, int32_t *status);
/* gmm-global-acc-stats.cc:117-131 up to the accumulation: per frame whose weight is not 0 (:119; frame_weight HOST [T], NULL:
 * every weight 1), DiagGmm::LogLikelihoodsPreselect over the frame's list (the chains above), VectorBase::ApplySoftMax
 * (matrix/kaldi-vector.cc:840-847) in LIST order, Scale(weight): float max; e = fl32(exp((double)(f - max))); the float sum of
 * e in list order; (e * fl32(1.0 / sum)) * w; like = max + fl32(log((double)sum)) - kh_gmm_acc_component_posteriors'
 * arithmetic.  The selection is HOST, CSR: sel_offsets [T + 1], sel_gauss.  DEVICE outputs: post, one dense zero-filled row
 * of num_gauss floats per used frame, contiguous, in frame order - what kh_gmm_acc_stats takes for a one-pdf model
 * (pdf_offsets = [0, num_gauss], one entry per used frame); frame_like [T], 0 for a frame that is not used.
 * Before any launch, KH_EINVAL naming the frame: offsets not from 0 or running backwards; on a used frame an index outside
 * [0, num_gauss), an empty list (the reference asserts gselect_size > 0), a Gaussian twice in the list.  The last is the one
 * deliberate difference from the reference, which would add both posteriors: gmm-gselect never writes a duplicate, and a dense
 * row holds one value per Gaussian. */
int kh_gmm_preselect_posteriors(const float *feats, int T, int D, int feat_stride, const float *gconsts, const float *means_invvars,
                                const float *inv_vars, int num_gauss, const int64_t *sel_offsets, const int32_t *sel_gauss,
                                const float *frame_weight, float *post, float *frame_like);
/* kh_gmm_gselect without a preselection scores at most this many bytes of T x num_gauss floats at a time (calling thread;
 * 0 = the default, 256 MiB; at least one row).  No result depends on it. */
int kh_gselect_set_workspace_limit(size_t bytes);
int kh_gselect_max_gauss(void);
int kh_gselect_max_n(void);
int kh_gselect_max_dim(void);
/* Lists (or num_gauss) up to this length take the kernels' small form, longer ones the large form (the tests' edge sizes). */
int kh_gselect_small_lists(void);
/* ms[5]: milliseconds of the calling thread's last kh_gmm_gselect - the whole call, its score kernels alone, its selection
 * kernels alone (device events) - and of its last kh_gmm_preselect_posteriors - the whole call, its kernel alone.  counts[2]:
 * row chunks of the gselect call; used frames of the posteriors call. */
int kh_gselect_last_timings(float *ms, int32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_HIP_H_ */
