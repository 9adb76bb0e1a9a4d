// kh_fmllr_update.h - the fMLLR update of one speaker in double: FmllrDiagGmmAccs::Update (transform/fmllr-diag-gmm.cc:131-166)
// from a unit transform, ComputeFmllrMatrixDiagGmmFull with FmllrInnerUpdate (:193-273), ...Diagonal (:275-348), ...Offset
// (:350-378), "none", FmllrAuxFuncDiagGmm (:481-508).  Plain C++ without any device call: kh_fmllr.hip (kh_fmllr_update) and
// tools/fmllr_cpu_baseline.cc compile this one source.  Statistics: beta, K [D][D + 1], G [D][(D + 1)(D + 2) / 2] packed lower
// triangles (SpMatrix).  SpMatrix::Invert / Matrix::Invert are Gauss-Jordan elimination with partial pivoting here (the
// reference calls LAPACK); a singular matrix is an error naming its place, as the reference's KALDI_ERR.
#ifndef KH_FMLLR_UPDATE_H_
#define KH_FMLLR_UPDATE_H_

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace kh_fmllr {

constexpr int kOk = 0, kInvalid = -1;   // KH_OK, KH_EINVAL of include/kaldi_hip.h

struct SpkStats {
  int D;
  double beta;
  const double *K;   // [D][D + 1]
  const double *G;   // [D][P] packed lower triangles
  int P() const { return (D + 1) * (D + 2) / 2; }
  double g(int i, int r, int c) const {
    if (r < c) std::swap(r, c);
    return G[static_cast<size_t>(i) * P() + r * (r + 1) / 2 + c];
  }
};

// In-place inverse of a row-major n x n matrix by Gauss-Jordan elimination with partial pivoting; log |det|.
inline bool Invert(std::vector<double> *Ap, int n, double *logdet) {
  std::vector<double> &A = *Ap;
  std::vector<int> piv(n);
  double ld = 0.0;
  for (int k = 0; k < n; k++) {
    int p = k;
    for (int i = k + 1; i < n; i++)
      if (std::fabs(A[i * n + k]) > std::fabs(A[p * n + k])) p = i;
    piv[k] = p;
    if (A[p * n + k] == 0.0 || !std::isfinite(A[p * n + k])) return false;
    if (p != k)
      for (int j = 0; j < n; j++) std::swap(A[k * n + j], A[p * n + j]);
    const double d = A[k * n + k];
    ld += std::log(std::fabs(d));
    const double inv = 1.0 / d;
    A[k * n + k] = 1.0;
    for (int j = 0; j < n; j++) A[k * n + j] *= inv;
    for (int i = 0; i < n; i++) {
      if (i == k) continue;
      const double f = A[i * n + k];
      if (f == 0.0) continue;
      A[i * n + k] = 0.0;
      for (int j = 0; j < n; j++) A[i * n + j] -= f * A[k * n + j];
    }
  }
  for (int k = n - 1; k >= 0; k--)
    if (piv[k] != k)
      for (int i = 0; i < n; i++) std::swap(A[i * n + k], A[i * n + piv[k]]);
  if (logdet) *logdet = ld;
  return true;
}

// FmllrAuxFuncDiagGmm(const MatrixBase<double> &, ...) :496-508; W is [D][D + 1].
inline bool AuxFunc(const std::vector<double> &W, const SpkStats &st, double *obj_out) {
  const int D = st.D, D1 = D + 1;
  std::vector<double> A(static_cast<size_t>(D) * D);
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) A[i * D + j] = W[i * D1 + j];
  double logdet;
  if (!Invert(&A, D, &logdet)) return false;
  double obj = st.beta * logdet;
  double tr = 0.0;
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D1; j++) tr += W[i * D1 + j] * st.K[i * D1 + j];   // TraceMatMat(xform, K_, kTrans)
  obj += tr;
  for (int d = 0; d < D; d++) {
    double q = 0.0;
    for (int r = 0; r < D1; r++) {
      double s = 0.0;
      for (int c = 0; c < D1; c++) s += st.g(d, r, c) * W[d * D1 + c];   // xform_row_g.AddSpVec(1.0, G_[d], xform.Row(d), 0.0)
      q += s * W[d * D1 + r];
    }
    obj -= 0.5 * q;
  }
  *obj_out = obj;
  return true;
}

inline bool ApproxEqualF(float a, float b, float tol = 0.001f) {   // base/kaldi-math.h ApproxEqual
  if (a == b) return true;
  const float diff = std::fabs(a - b);
  if (diff == HUGE_VALF || diff != diff) return false;
  return diff <= tol * (std::fabs(a) + std::fabs(b));
}

// ComputeFmllrMatrixDiagGmmFull :236-273 with FmllrInnerUpdate :193-234.  W: the float transform, in and out.
inline int UpdateFull(const SpkStats &st, int num_iters, std::vector<float> *Wf, float *impr, std::string *err) {
  const int D = st.D, D1 = D + 1;
  std::vector<std::vector<double>> inv_g(D);
  for (int d = 0; d < D; d++) {
    inv_g[d].resize(static_cast<size_t>(D1) * D1);
    for (int r = 0; r < D1; r++)
      for (int c = 0; c < D1; c++) inv_g[d][r * D1 + c] = st.g(d, r, c);
    if (!Invert(&inv_g[d], D1, nullptr)) {
      *err = "G_[" + std::to_string(d) + "] is singular (SpMatrix::Invert)";
      return kInvalid;
    }
  }
  std::vector<double> old_x(Wf->begin(), Wf->end()), new_x(Wf->begin(), Wf->end());
  double o;
  if (!AuxFunc(old_x, st, &o)) { *err = "the starting transform is singular"; return kInvalid; }
  const float old_objf = static_cast<float>(o);
  std::vector<double> cof(static_cast<size_t>(D) * D), row(D1), row_invg(D1);
  for (int iter = 0; iter < num_iters; iter++) {
    for (int d = 0; d < D; d++) {
      for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) cof[i * D + j] = new_x[j * D1 + i];   // CopyFromMat(..., kTrans)
      if (!Invert(&cof, D, nullptr)) { *err = "the transform became singular in FmllrInnerUpdate"; return kInvalid; }
      for (int j = 0; j < D; j++) row[j] = cof[d * D + j];
      row[D] = 0.0;
      const std::vector<double> &ig = inv_g[d];
      const double *k = st.K + static_cast<size_t>(d) * D1;
      double e1 = 0.0, e2 = 0.0;
      for (int r = 0; r < D1; r++) {
        double s = 0.0;
        for (int c = 0; c < D1; c++) s += ig[r * D1 + c] * row[c];
        row_invg[r] = s;
      }
      for (int r = 0; r < D1; r++) { e1 += row_invg[r] * row[r]; e2 += row_invg[r] * k[r]; }
      const double discr = std::sqrt(e2 * e2 + 4 * e1 * st.beta);
      const double alpha1 = (-e2 + discr) / (2 * e1), alpha2 = (-e2 - discr) / (2 * e1);
      const double auxf1 = st.beta * std::log(std::fabs(alpha1 * e1 + e2)) - 0.5 * alpha1 * alpha1 * e1;
      const double auxf2 = st.beta * std::log(std::fabs(alpha2 * e1 + e2)) - 0.5 * alpha2 * alpha2 * e1;
      const double alpha = (auxf1 > auxf2) ? alpha1 : alpha2;
      for (int r = 0; r < D1; r++) row[r] = alpha * row[r] + k[r];
      for (int r = 0; r < D1; r++) {
        double s = 0.0;
        for (int c = 0; c < D1; c++) s += ig[r * D1 + c] * row[c];
        new_x[d * D1 + r] = s;
      }
    }
  }
  if (!AuxFunc(new_x, st, &o)) { *err = "the estimated transform is singular"; return kInvalid; }
  const float new_objf = static_cast<float>(o), objf_improvement = new_objf - old_objf;
  if (objf_improvement < 0.0f && !ApproxEqualF(new_objf, old_objf)) {
    *impr = 0.0f;   // "No applying fMLLR transform change because objective function did not increase."
    return kOk;
  }
  for (size_t i = 0; i < new_x.size(); i++) (*Wf)[i] = static_cast<float>(new_x[i]);
  *impr = objf_improvement;
  return kOk;
}

// FmllrAuxFuncDiagGmm(const MatrixBase<float> &, ...) :481-494
inline bool AuxFuncF(const std::vector<float> &Wf, const SpkStats &st, float *obj) {
  std::vector<double> W(Wf.begin(), Wf.end());
  double o;
  if (!AuxFunc(W, st, &o)) return false;
  *obj = static_cast<float>(o);
  return true;
}

// ComputeFmllrMatrixDiagGmmDiagonal :275-348
inline int UpdateDiag(const SpkStats &st, std::vector<float> *Wf, float *impr, std::string *err) {
  const int D = st.D, D1 = D + 1;
  const double beta = st.beta;
  if (beta == 0.0) { *impr = 0.0f; return kOk; }
  float old_obj, new_obj;
  if (!AuxFuncF(*Wf, st, &old_obj)) { *err = "the starting transform is singular"; return kInvalid; }
  for (int i = 0; i < D; i++) {
    const double k_ii = st.K[i * D1 + i], k_id = st.K[i * D1 + D], g_iii = st.g(i, i, i), g_idd = st.g(i, D, D), g_idi = st.g(i, D, i);
    const double a = g_idi * g_idi / g_idd - g_iii, b = k_ii - g_idi * k_id / g_idd, c = beta;
    const double s = (-b - std::sqrt(b * b - 4 * a * c)) / (2 * a);
    if (!(s > 0.0)) { *err = "KALDI_ASSERT: s > 0.0 (diagonal update, row " + std::to_string(i) + ")"; return kInvalid; }
    const double o = (k_id - s * g_idi) / g_idd;
    (*Wf)[i * D1 + i] = static_cast<float>(s);
    (*Wf)[i * D1 + D] = static_cast<float>(o);
  }
  if (!AuxFuncF(*Wf, st, &new_obj)) { *err = "the estimated transform is singular"; return kInvalid; }
  *impr = new_obj - old_obj;
  return kOk;
}

// ComputeFmllrMatrixDiagGmmOffset :350-378
inline int UpdateOffset(const SpkStats &st, std::vector<float> *Wf, float *impr) {
  const int D = st.D, D1 = D + 1;
  float objf_impr = 0.0f;
  for (int i = 0; i < D; i++) {
    const double g_dd = st.g(i, D, D), g_id = st.g(i, i, D), k_id = st.K[i * D1 + D];
    float b_i = (*Wf)[i * D1 + D];
    const float before = static_cast<float>(-0.5 * b_i * b_i * g_dd - b_i * g_id + b_i * k_id);
    b_i = static_cast<float>((k_id - g_id) / g_dd);
    (*Wf)[i * D1 + D] = b_i;
    const float after = static_cast<float>(-0.5 * b_i * b_i * g_dd - b_i * g_id + b_i * k_id);
    objf_impr += after - before;
  }
  *impr = objf_impr;
  return kOk;
}


// Update :131-166 for one speaker: W [D][D + 1] float out (unit unless updated), *impr, *count.
inline int UpdateSpeaker(const SpkStats &st, const std::string &type, float min_count, int num_iters, float *W_out, float *impr_out,
                         float *count_out, std::string *err) {
  const int D = st.D, D1 = D + 1;
  std::vector<float> W(static_cast<size_t>(D) * D1, 0.f);
  for (int i = 0; i < D; i++) W[i * D1 + i] = 1.f;   // transform.SetUnit()
  float impr = 0.f;
  int status = kOk;
  if (st.beta > min_count) {   // :144
    if (type == "full") status = UpdateFull(st, num_iters, &W, &impr, err);
    else if (type == "diag") status = UpdateDiag(st, &W, &impr, err);
    else if (type == "offset") status = UpdateOffset(st, &W, &impr);
  }
  std::copy(W.begin(), W.end(), W_out);
  *impr_out = impr;
  *count_out = static_cast<float>(st.beta);
  return status;
}

}  // namespace kh_fmllr
#endif  // KH_FMLLR_UPDATE_H_
