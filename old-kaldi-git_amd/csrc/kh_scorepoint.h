// kh_scorepoint.h — the "score point" of the batched compact-lattice kernels: what lattice-scale (latbin/lattice-scale.cc:76-82)
// and lattice-add-penalty (lat/lattice-functions.cc:1128-1149) do to a weight before a lattice tool reads it: a 2x2 matrix of
// doubles and a float word insertion penalty.  One definition for the kernels (kh_latbest.hip, kh_latprune.hip) and for the
// host sweep of kh_latmbr.hip; host and device are compiled with -ffp-contract=off, so both give the reference's bits.
#ifndef KH_SCOREPOINT_H_
#define KH_SCOREPOINT_H_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace kh {

struct Point {
  double s00, s01, s10, s11;
  float pen;
};

// point p of the caller's arrays: scales holds 4 doubles per point (row-major), penalties one float
__host__ __device__ __forceinline__ Point LoadPoint(const double *scales, const float *penalties, int p) {
  Point pt;
  pt.s00 = scales[4 * p];
  pt.s01 = scales[4 * p + 1];
  pt.s10 = scales[4 * p + 2];
  pt.s11 = scales[4 * p + 3];
  pt.pen = penalties[p];
  return pt;
}

// ScaleTupleWeight fstext/lattice-weight.h:233-241: Zero stays Zero (:237-238); products and sums in double, the
// LatticeWeightTpl<float> constructor narrows.
__host__ __device__ __forceinline__ void ScaleWeight(float g, float a, const Point &pt, float *g2, float *a2) {
  if (g == INFINITY) {
    *g2 = INFINITY;
    *a2 = INFINITY;
  } else {
    *g2 = static_cast<float>(pt.s00 * static_cast<double>(g) + pt.s01 * static_cast<double>(a));
    *a2 = static_cast<float>(pt.s10 * static_cast<double>(g) + pt.s11 * static_cast<double>(a));
  }
}
// ... followed by AddWordInsPenToCompactLattice lat/lattice-functions.cc:1140-1143 (float sum, arcs with a word only)
__host__ __device__ __forceinline__ void ArcWeight(float g, float a, int32_t label, const Point &pt, float *g2, float *a2) {
  ScaleWeight(g, a, pt, g2, a2);
  if (label != 0) *g2 = *g2 + pt.pen;
}
// ConvertToCost fstext/lattice-weight.h:799-801
__host__ __device__ __forceinline__ double Cost(float g2, float a2) { return static_cast<double>(g2) + static_cast<double>(a2); }

}  // namespace kh

#endif  // KH_SCOREPOINT_H_
