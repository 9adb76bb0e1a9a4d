// kh_gselect_plan.h - the host side of kh_gmm_gselect and kh_gmm_preselect_posteriors (csrc/kh_gselect.hip): plain C++, no
// HIP, so that the checks and the row chunks are tested on the CPU (tests/test_gselect_plan_host.py).
//
//   CheckLists  a per-frame list of Gaussians in CSR form (offsets [T + 1], gauss []) against the model; the message names the
//               frame.  Both calls: offsets from 0 and never backwards, fewer than 2^31 items, every index in [0, num_gauss),
//               no list longer than max_len.  An empty list is refused on every frame that is used (the reference asserts
//               gselect_size > 0, gmm-global-acc-stats.cc:124; nth_element on an empty range in GaussianSelectionPreselect).
//               refuse_twice: a Gaussian twice in one frame's list is refused - kh_gmm_preselect_posteriors only, the one
//               deliberate difference from the reference (gmm-gselect never writes one; a dense posterior row holds one value
//               per Gaussian).  A frame whose weight is 0 is not used (gmm-global-acc-stats.cc:119): of its list only the
//               offsets are looked at.
//   UsedFrames  the frames whose weight is not 0 (all of them without weights), in order: row i of the posteriors is frame
//               used[i].
//   ChunkRows   rows of a T x num_gauss float score workspace within limit_bytes: at least 1, at most T.
#ifndef KH_GSELECT_PLAN_H_
#define KH_GSELECT_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace kh_gselect {

inline std::string Format(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c);
  return buf;
}

inline bool Used(const float *frame_weight, int t) { return !frame_weight || frame_weight[t] != 0.0f; }

// false with *err set; `what` names the offsets array in the messages ("pre_offsets", "sel_offsets")
inline bool CheckLists(int T, const int64_t *offsets, const int32_t *gauss, int num_gauss, int max_len, const float *frame_weight,
                       bool refuse_twice, const char *what, std::string *err) {
  if (offsets[0] != 0) { *err = std::string(what) + Format("[0] = %lld, not 0", offsets[0]); return false; }
  for (int t = 0; t < T; t++)
    if (offsets[t + 1] < offsets[t]) { *err = std::string(what) + Format(" runs backwards at frame %lld", t); return false; }
  if (offsets[T] >= (int64_t(1) << 31)) { *err = Format("%lld listed Gaussians, at most 2^31 - 1", offsets[T]); return false; }
  std::vector<int32_t> seen(refuse_twice ? num_gauss : 0, -1);   // the last frame that listed the Gaussian
  for (int t = 0; t < T; t++) {
    if (!Used(frame_weight, t)) continue;
    const int64_t b = offsets[t], e = offsets[t + 1];
    if (e == b) { *err = Format("frame %lld has an empty list", t); return false; }
    if (e - b > max_len) { *err = Format("frame %lld lists %lld Gaussians, at most %lld", t, e - b, max_len); return false; }
    for (int64_t i = b; i < e; i++) {
      const int32_t g = gauss[i];
      if (g < 0 || g >= num_gauss) { *err = Format("frame %lld lists Gaussian %lld, the model has %lld", t, g, num_gauss); return false; }
      if (refuse_twice) {
        if (seen[g] == t) { *err = Format("frame %lld lists Gaussian %lld twice", t, g); return false; }
        seen[g] = t;
      }
    }
  }
  return true;
}

inline std::vector<int32_t> UsedFrames(int T, const float *frame_weight) {
  std::vector<int32_t> used;
  for (int t = 0; t < T; t++)
    if (Used(frame_weight, t)) used.push_back(t);
  return used;
}

inline int ChunkRows(int T, int num_gauss, size_t limit_bytes) {
  const size_t row = sizeof(float) * static_cast<size_t>(num_gauss);
  const size_t rows = std::max<size_t>(limit_bytes / row, 1);
  return static_cast<int>(std::min<size_t>(rows, static_cast<size_t>(std::max(T, 1))));
}

}  // namespace kh_gselect
#endif  // KH_GSELECT_PLAN_H_
