// align_host_step.cc — steps the __host__ __device__ body of csrc/kh_align.hip (AlignBody, with the library's own Prepare in
// front) on the host with a small lane count: no device, no library.  Reads the plain dump of tests/align_cases.py
// (write_dump) and prints what tools/align_cpu_baseline.cc prints.  Every buffer the body writes has guard words behind
// it, checked at the end; built with the host sanitizers this is the memory check of the kernel's index arithmetic.
//   hipcc -x hip --offload-arch=gfx950 -DKH_ALIGN_BODY_ONLY -O1 -g -Xarch_host -fsanitize=address,undefined
//         tools/align_host_step.cc -o align_host_step;   align_host_step DUMP LANES
#include <cstdio>
#include <cstdlib>

#ifndef KH_ALIGN_BODY_ONLY
#define KH_ALIGN_BODY_ONLY
#endif
#include "../old-kaldi-git_amd/csrc/kh_align.hip"

namespace kh {
void SetError(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace kh

using namespace kh::align;

static long long ReadInt(FILE *f) {
  long long v;
  if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short dump\n"); exit(2); }
  return v;
}
static float Bits(long long b) { const uint32_t u = static_cast<uint32_t>(b); float x; memcpy(&x, &u, 4); return x; }

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: align_host_step DUMP LANES\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  const int n_lanes = atoi(argv[2]);
  if (!f || n_lanes < 1 || n_lanes > kMaxLanes) { fprintf(stderr, "cannot read %s, or lanes outside 1..%d\n", argv[1], kMaxLanes); return 2; }
  const int n = static_cast<int>(ReadInt(f));
  const float beam = Bits(ReadInt(f));
  const int min_active = static_cast<int>(ReadInt(f));
  const float beam_delta = Bits(ReadInt(f));
  const int n_tid = static_cast<int>(ReadInt(f)), rows = static_cast<int>(ReadInt(f)), cols = static_cast<int>(ReadInt(f));
  std::vector<int32_t> tid2pdf(n_tid), soff{0}, start, il, ol, ns, roff{0};
  std::vector<int64_t> aoff{0}, poff{0};
  std::vector<float> w, fin;
  for (auto &x : tid2pdf) x = static_cast<int32_t>(ReadInt(f));
  for (int u = 0; u < n; u++) {
    const int S = static_cast<int>(ReadInt(f)), A = static_cast<int>(ReadInt(f));
    start.push_back(static_cast<int32_t>(ReadInt(f)));
    const int T = static_cast<int>(ReadInt(f));
    const int row0 = static_cast<int>(ReadInt(f));
    const int room = static_cast<int>(ReadInt(f));
    if (row0 != roff.back()) { fprintf(stderr, "rows are not consecutive\n"); return 2; }
    std::vector<int64_t> cnt(S + 1, 0);
    int last = 0;
    for (int a = 0; a < A; a++) {
      const int src = static_cast<int>(ReadInt(f));
      if (src < last || src >= S) { fprintf(stderr, "arcs are not sorted by state\n"); return 2; }
      last = src;
      cnt[src + 1]++;
      ns.push_back(static_cast<int32_t>(ReadInt(f)));
      il.push_back(static_cast<int32_t>(ReadInt(f)));
      ol.push_back(static_cast<int32_t>(ReadInt(f)));
      w.push_back(Bits(ReadInt(f)));
    }
    const int64_t a0 = aoff.back();
    for (int s = 0; s < S; s++) { cnt[s + 1] += cnt[s]; aoff.push_back(a0 + cnt[s + 1]); }
    for (int s = 0; s < S; s++) fin.push_back(Bits(ReadInt(f)));
    soff.push_back(soff.back() + S);
    roff.push_back(row0 + T);
    poff.push_back(poff.back() + room);
  }
  std::vector<float> ll(static_cast<size_t>(rows) * cols);
  for (auto &x : ll) x = Bits(ReadInt(f));
  fclose(f);

  Prepared P;
  std::string first_bad;
  if (Prepare(n, soff.data(), aoff.data(), start.data(), il.data(), w.data(), ns.data(), fin.data(), n_tid, tid2pdf.data(), rows,
              cols, roff.data(), poff.data(), &P, &first_bad) != KH_OK)
    return 3;
  if (!first_bad.empty()) fprintf(stderr, "%s\n", first_bad.c_str());
  constexpr int kGuard = 8;
  constexpr int32_t kMark = 0x5a5a5a5a;
  std::vector<int32_t> status(P.status);
  std::vector<std::vector<int32_t>> out_path(n);
  std::vector<std::vector<float>> out_ac(n);
  std::vector<double> out_cost(n, 0.0);
  std::vector<int32_t> out_best(n, -1), out_len(n, 0);
  int guard_errors = 0;
  for (const Job &J0 : P.jobs) {
    Job J = J0;
    // buffers of this utterance alone, each with guard words behind it
    std::vector<int32_t> bp((static_cast<size_t>(J.T) + 1) * J.S + kGuard, kMark), path(J.room + kGuard, kMark), hdr(kHdr + kGuard, kMark);
    std::vector<float> pac(J.room + kGuard);
    std::vector<double> cost(2 * static_cast<size_t>(J.S) + kGuard), hcost(1 + kGuard);
    const float fmark = Bits(kMark);
    const double dmark = -12345.678;
    for (int i = 0; i < kGuard; i++) { pac[J.room + i] = fmark; cost[2 * J.S + i] = dmark; hcost[1 + i] = dmark; }
    J.bp_off = 0; J.cost_off = 0; J.slot = 0;
    const int64_t path_off = J.path_off;
    J.path_off = 0;
    Ctx X{P.e_off.data(), P.e.data(), P.n_off.data(), P.n.data(), fin.data(), P.arc.data(), ll.data(), static_cast<int64_t>(cols),
          beam, beam_delta, min_active, bp.data(), cost.data(), hdr.data(), hcost.data(), path.data(), pac.data()};
    Shared sh;
    AlignBody(J, X, cost.data(), cost.data() + J.S, &sh, n_lanes);
    (void)path_off;
    for (int i = 0; i < kGuard; i++) {
      if (bp[bp.size() - kGuard + i] != kMark || path[J.room + i] != kMark || hdr[kHdr + i] != kMark || memcmp(&pac[J.room + i], &fmark, 4) != 0 ||
          cost[2 * J.S + i] != dmark || hcost[1 + i] != dmark)
        guard_errors++;
    }
    status[J.utt] = hdr[0];
    out_len[J.utt] = hdr[1];
    out_best[J.utt] = hdr[2];
    out_cost[J.utt] = hcost[0];
    if (hdr[0] == KH_ALIGNC_DONE) {
      out_path[J.utt].assign(path.begin(), path.begin() + hdr[1]);
      out_ac[J.utt].assign(pac.begin(), pac.begin() + hdr[1]);
    }
  }
  for (int u = 0; u < n; u++) {
    uint64_t cb;
    double c = (status[u] == KH_ALIGNC_DONE || status[u] == KH_ALIGNC_NEEDS_ROOM) ? out_cost[u] : std::numeric_limits<double>::infinity();
    memcpy(&cb, &c, 8);
    const bool have = status[u] == KH_ALIGNC_DONE || status[u] == KH_ALIGNC_NEEDS_ROOM;
    printf("%d %llu %d %d\n", status[u], static_cast<unsigned long long>(cb), have ? out_best[u] : -1, have ? out_len[u] : 0);
    if (status[u] == KH_ALIGNC_DONE) {
      const int64_t a0 = aoff[soff[u]];
      for (size_t i = 0; i < out_path[u].size(); i++) {
        const int64_t a = a0 + out_path[u][i];
        uint32_t gb, ab;
        memcpy(&gb, &w[a], 4);
        memcpy(&ab, &out_ac[u][i], 4);
        printf("%d %d %u %u\n", il[a], ol[a], gb, ab);
      }
    }
  }
  if (guard_errors) { fprintf(stderr, "%d guard words overwritten\n", guard_errors); return 4; }
  return 0;
}
