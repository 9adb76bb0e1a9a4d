// kh_gmmacc_plan.h - the host plan of kh_gmm_acc_stats (csrc/kh_gmmacc.hip): plain C++, no HIP, so that the checks, the sort,
// the chunks and the groups are tested on the CPU (tests/test_gmmacc_plan_host.py).
//
//   Check    every offset and index of an entry list against the model; the message names the pdf or entry.  The one check of
//            every route that takes an entry list: the two posteriors calls (kh_gmmstats.h), kh_fmllr_frame_stats,
//            kh_gmm_acc_stats and kh_mllt_acc_stats.  Pdfs ascending within a frame is NOT required (the order is the caller's).
//   Sort     a stable counting sort of the entries by pdf: within a pdf the entries stay in entry (= frame) order
//   chunks   a pdf's run of n entries is cut into DivUp(n, chunk) chunks of at most `chunk` entries (a run of 0: no chunk)
//   Groups   consecutive pdfs whose workspace - (chunks + 1) * G * C doubles per pdf: one partial sum per chunk and the sum -
//            stays within the limit; a pdf is never split, so a pdf that alone exceeds the limit is a group of its own
#ifndef KH_GMMACC_PLAN_H_
#define KH_GMMACC_PLAN_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace kh_gmmacc {

struct Plan {
  std::vector<int32_t> sorted_entry;       // [E] entry indices, by pdf, stable
  std::vector<int32_t> sorted_row;         // [E] the frame of sorted_entry[i]
  std::vector<int64_t> pdf_entry_offsets;  // [num_pdfs + 1] into sorted_entry
};

struct Group { int32_t pdf_begin, pdf_end; int64_t n_chunks; };

inline int64_t NumChunks(int64_t n, int chunk) { return (n + chunk - 1) / chunk; }

inline std::string Format(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return buf;
}

// false with *err set when the entry list does not fit the model
inline bool Check(int T, const int32_t *pdf_offsets, int num_pdfs, const int64_t *feo, const int32_t *entry_pdf,
                  const int64_t *goff, std::string *err) {
  if (feo[0] != 0) { *err = Format("frame_entry_offsets[0] = %lld, not 0", feo[0]); return false; }
  for (int t = 0; t < T; t++)
    if (feo[t + 1] < feo[t]) { *err = Format("frame_entry_offsets runs backwards at frame %lld", t); return false; }
  const int64_t E = feo[T];
  if (E >= (int64_t(1) << 31)) { *err = Format("%lld entries, at most 2^31 - 1", E); return false; }
  if (pdf_offsets[0] != 0) { *err = Format("pdf_offsets[0] = %lld, not 0", pdf_offsets[0]); return false; }
  for (int j = 0; j < num_pdfs; j++)
    if (pdf_offsets[j + 1] <= pdf_offsets[j]) { *err = Format("pdf %lld is empty or runs backwards", j); return false; }
  if (E > 0 && goff[0] != 0) { *err = Format("entry_gauss_offsets[0] = %lld, not 0", goff[0]); return false; }
  for (int64_t e = 0; e < E; e++) {
    const int pdf = entry_pdf[e];
    if (pdf < 0 || pdf >= num_pdfs) { *err = Format("entry %lld names pdf %lld, the model has %lld", e, pdf, num_pdfs); return false; }
    const int64_t n = goff[e + 1] - goff[e];
    if (n != pdf_offsets[pdf + 1] - pdf_offsets[pdf]) {
      *err = Format("pdf %lld has %lld Gaussians in the model, entry %lld carries %lld posteriors", pdf,
                    pdf_offsets[pdf + 1] - pdf_offsets[pdf], e, n);
      return false;
    }
  }
  return true;
}

// the entries (already checked) by pdf
inline void Sort(int T, int num_pdfs, const int64_t *feo, const int32_t *entry_pdf, Plan *plan) {
  const int64_t E = feo[T];
  plan->pdf_entry_offsets.assign(static_cast<size_t>(num_pdfs) + 1, 0);
  for (int64_t e = 0; e < E; e++) plan->pdf_entry_offsets[entry_pdf[e] + 1]++;
  for (int j = 0; j < num_pdfs; j++) plan->pdf_entry_offsets[j + 1] += plan->pdf_entry_offsets[j];
  std::vector<int64_t> next(plan->pdf_entry_offsets.begin(), plan->pdf_entry_offsets.end() - 1);
  plan->sorted_entry.resize(E);
  plan->sorted_row.resize(E);
  for (int t = 0; t < T; t++)
    for (int64_t e = feo[t]; e < feo[t + 1]; e++) {
      const int64_t at = next[entry_pdf[e]]++;
      plan->sorted_entry[at] = static_cast<int32_t>(e);
      plan->sorted_row[at] = t;
    }
}

// workspace doubles of one pdf: a partial sum per chunk, and the sum
inline int64_t PdfDoubles(int64_t n_entries, int G, int C, int chunk) { return (NumChunks(n_entries, chunk) + 1) * G * C; }

inline std::vector<Group> Groups(const Plan &plan, const int32_t *pdf_offsets, int num_pdfs, int C, int chunk, size_t limit_bytes) {
  std::vector<Group> groups;
  for (int p0 = 0; p0 < num_pdfs;) {
    int p1 = p0;
    int64_t doubles = 0, chunks = 0;
    while (p1 < num_pdfs) {
      const int64_t n = plan.pdf_entry_offsets[p1 + 1] - plan.pdf_entry_offsets[p1];
      const int64_t d = PdfDoubles(n, pdf_offsets[p1 + 1] - pdf_offsets[p1], C, chunk);
      if (p1 > p0 && static_cast<uint64_t>(doubles + d) * sizeof(double) > limit_bytes) break;
      doubles += d;
      chunks += NumChunks(n, chunk);
      p1++;
    }
    groups.push_back(Group{p0, p1, chunks});
    p0 = p1;
  }
  return groups;
}

}  // namespace kh_gmmacc
#endif  // KH_GMMACC_PLAN_H_
