// The host plan of kh_gmm_acc_stats (csrc/kh_gmmacc_plan.h) in a stand-alone program: checks with their messages, the stable
// sort by pdf, the chunk counts, the groups under a workspace limit.  Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../old-kaldi-git_amd/csrc/kh_gmmacc_plan.h"

using namespace kh_gmmacc;

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond);          \
      failures++;                                                             \
    }                                                                         \
  } while (0)

struct Case {
  std::vector<int32_t> pdf_offsets;
  std::vector<int64_t> feo, goff;
  std::vector<int32_t> entry_pdf;
  int T() const { return static_cast<int>(feo.size()) - 1; }
  int NumPdfs() const { return static_cast<int>(pdf_offsets.size()) - 1; }
  void Finish() {   // goff from the pdfs
    goff.assign(1, 0);
    for (int32_t p : entry_pdf) goff.push_back(goff.back() + pdf_offsets[p + 1] - pdf_offsets[p]);
  }
  bool Check(std::string *err) const {
    return kh_gmmacc::Check(T(), pdf_offsets.data(), NumPdfs(), feo.data(), entry_pdf.data(), goff.data(), err);
  }
};

// pdfs of `sizes` Gaussians with `counts` entries each, dealt to frames round-robin over the pdfs that still have entries left,
// two or three entries per frame, every fifth frame empty: a pdf's entries are spread over the frames, never adjacent
static Case MakeCase(const std::vector<int> &sizes, const std::vector<int> &counts) {
  Case c;
  c.pdf_offsets.assign(1, 0);
  for (int s : sizes) c.pdf_offsets.push_back(c.pdf_offsets.back() + s);
  std::vector<int> left(counts);
  c.feo.assign(1, 0);
  size_t p = 0;
  long total = 0;
  for (int n : counts) total += n;
  for (int frame = 0; total > 0; frame++) {
    const int k = frame % 5 == 4 ? 0 : 2 + frame % 2;
    for (int i = 0; i < k && total > 0; i++) {
      while (left[p % sizes.size()] == 0) p++;
      c.entry_pdf.push_back(static_cast<int32_t>(p % sizes.size()));
      left[p % sizes.size()]--;
      total--;
      p++;
    }
    c.feo.push_back(static_cast<int64_t>(c.entry_pdf.size()));
  }
  c.feo.push_back(c.feo.back());   // a last frame without entries
  c.Finish();
  return c;
}

int main() {
  const int chunk = 256;
  // ---- chunk counts
  EXPECT(NumChunks(0, chunk) == 0 && NumChunks(1, chunk) == 1 && NumChunks(chunk - 1, chunk) == 1 && NumChunks(chunk, chunk) == 1);
  EXPECT(NumChunks(chunk + 1, chunk) == 2 && NumChunks(2 * chunk + 1, chunk) == 3);
  // ---- the sort: stable, frame order within a pdf
  const std::vector<int> sizes = {3, 1, 17, 2, 5, 40, 1};
  const std::vector<int> counts = {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 7};
  Case c = MakeCase(sizes, counts);
  std::string err;
  EXPECT(c.Check(&err));
  Plan plan;
  Sort(c.T(), c.NumPdfs(), c.feo.data(), c.entry_pdf.data(), &plan);
  const int64_t E = c.feo.back();
  EXPECT(static_cast<int64_t>(plan.sorted_entry.size()) == E && plan.pdf_entry_offsets.back() == E && plan.pdf_entry_offsets[0] == 0);
  std::vector<int> seen(E, 0);
  for (int p = 0; p < c.NumPdfs(); p++) {
    EXPECT(plan.pdf_entry_offsets[p + 1] - plan.pdf_entry_offsets[p] == counts[p]);
    for (int64_t i = plan.pdf_entry_offsets[p]; i < plan.pdf_entry_offsets[p + 1]; i++) {
      const int32_t e = plan.sorted_entry[i];
      EXPECT(c.entry_pdf[e] == p);
      seen[e]++;
      EXPECT(c.feo[plan.sorted_row[i]] <= e && e < c.feo[plan.sorted_row[i] + 1]);            // the entry's frame
      if (i > plan.pdf_entry_offsets[p]) {
        EXPECT(plan.sorted_entry[i - 1] < e);                                                  // entry order kept ...
        EXPECT(plan.sorted_row[i - 1] <= plan.sorted_row[i]);                                  // ... which is frame order
      }
    }
  }
  for (int64_t e = 0; e < E; e++) EXPECT(seen[e] == 1);
  // two entries of one pdf in one frame stay in the order given
  {
    Case d;
    d.pdf_offsets = {0, 2, 3};
    d.feo = {0, 3, 3, 5};
    d.entry_pdf = {1, 0, 1, 1, 0};
    d.Finish();
    EXPECT(d.Check(&err));
    Plan q;
    Sort(d.T(), d.NumPdfs(), d.feo.data(), d.entry_pdf.data(), &q);
    EXPECT((q.sorted_entry == std::vector<int32_t>{1, 4, 0, 2, 3}) && (q.sorted_row == std::vector<int32_t>{0, 2, 0, 0, 2}));
    EXPECT((q.pdf_entry_offsets == std::vector<int64_t>{0, 2, 5}));
  }
  // no frames at all
  {
    Case d;
    d.pdf_offsets = {0, 2};
    d.feo = {0};
    d.goff = {0};
    EXPECT(d.Check(&err));
    Plan q;
    Sort(0, 1, d.feo.data(), d.entry_pdf.data(), &q);
    EXPECT(q.sorted_entry.empty() && (q.pdf_entry_offsets == std::vector<int64_t>{0, 0}));
    const std::vector<Group> g = Groups(q, d.pdf_offsets.data(), 1, 5, chunk, 1 << 20);
    EXPECT(g.size() == 1 && g[0].n_chunks == 0);
  }
  // ---- groups
  const int C = 27;
  auto bytes_of = [&](int p) { return PdfDoubles(counts[p], sizes[p], C, chunk) * 8; };
  {
    const std::vector<Group> all = Groups(plan, c.pdf_offsets.data(), c.NumPdfs(), C, chunk, size_t(1) << 30);
    EXPECT(all.size() == 1 && all[0].pdf_begin == 0 && all[0].pdf_end == c.NumPdfs() && all[0].n_chunks == 0 + 1 + 1 + 1 + 2 + 3 + 1);
  }
  for (size_t limit : {size_t(1), size_t(3 * 16 * C * 8), size_t(20000), size_t(40 * C * 8 * 4), size_t(200000)}) {
    const std::vector<Group> gs = Groups(plan, c.pdf_offsets.data(), c.NumPdfs(), C, chunk, limit);
    int next = 0;
    for (const Group &g : gs) {
      EXPECT(g.pdf_begin == next && g.pdf_end > g.pdf_begin);          // consecutive, never empty, a pdf in one group only
      next = g.pdf_end;
      int64_t b = 0, ch = 0;
      for (int p = g.pdf_begin; p < g.pdf_end; p++) {
        b += bytes_of(p);
        ch += NumChunks(counts[p], chunk);
      }
      EXPECT(ch == g.n_chunks);
      EXPECT(static_cast<uint64_t>(b) <= limit || g.pdf_end - g.pdf_begin == 1);   // over the limit only alone
      if (g.pdf_end < c.NumPdfs())                                                  // and greedy: the next pdf did not fit
        EXPECT(static_cast<uint64_t>(b + bytes_of(g.pdf_end)) > limit);
    }
    EXPECT(next == c.NumPdfs());
    if (limit == 1) EXPECT(static_cast<int>(gs.size()) == c.NumPdfs());
  }
  {   // pdf 5 (40 Gaussians, 3 chunks: 4 x 40 x 27 x 8 = 34560 bytes) exceeds 20000 and goes alone
    const std::vector<Group> gs = Groups(plan, c.pdf_offsets.data(), c.NumPdfs(), C, chunk, 20000);
    bool alone = false;
    for (const Group &g : gs) alone = alone || (g.pdf_begin == 5 && g.pdf_end == 6);
    EXPECT(bytes_of(5) == 34560 && alone);
  }
  // ---- refusals and their messages
  auto refused = [&](Case bad, const char *want) {
    std::string e;
    const bool ok = bad.Check(&e);
    if (ok || e != want) {
      std::printf("expected refusal \"%s\", got %s \"%s\"\n", want, ok ? "acceptance" : "refusal", e.c_str());
      failures++;
    }
  };
  Case small;
  small.pdf_offsets = {0, 2, 3};
  small.feo = {0, 1, 3};
  small.entry_pdf = {0, 1, 0};
  small.Finish();
  EXPECT(small.Check(&err));
  { Case b = small; b.entry_pdf[1] = 2; refused(b, "entry 1 names pdf 2, the model has 2"); }
  { Case b = small; b.entry_pdf[2] = -1; refused(b, "entry 2 names pdf -1, the model has 2"); }
  { Case b = small; b.entry_pdf[0] = 1; refused(b, "pdf 1 has 1 Gaussians in the model, entry 0 carries 2 posteriors"); }
  { Case b = small; b.feo[0] = 1; refused(b, "frame_entry_offsets[0] = 1, not 0"); }
  { Case b = small; b.feo = {0, 4, 3}; refused(b, "frame_entry_offsets runs backwards at frame 1"); }
  { Case b = small; b.pdf_offsets = {0, 2, 2}; refused(b, "pdf 1 is empty or runs backwards"); }
  { Case b = small; b.pdf_offsets[0] = 1; refused(b, "pdf_offsets[0] = 1, not 0"); }
  { Case b = small; b.goff[0] = 1; refused(b, "entry_gauss_offsets[0] = 1, not 0"); }
  // no entries: entry_gauss_offsets[0] is not looked at
  {
    Case d;
    d.pdf_offsets = {0, 2, 3};
    d.feo = {0, 0, 0};
    d.goff = {7};
    EXPECT(d.Check(&err));
  }
  // a negative frame_entry_offsets[T] runs backwards somewhere; the entry arrays (null here) are not touched
  {
    const std::vector<int32_t> off = {0, 2, 3};
    const std::vector<int64_t> feo = {0, 0, -1};
    std::string e;
    EXPECT(!kh_gmmacc::Check(2, off.data(), 2, feo.data(), nullptr, nullptr, &e));
    EXPECT(e == "frame_entry_offsets runs backwards at frame 1");
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
