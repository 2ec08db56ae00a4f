// Host twin of rj_node.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_node.h run as plain loops, in the device's stage order, with std::sort / plain prefix sums where
// the device calls rocPRIM.  tests/test_node.py holds it equal to the plain-Python definition (tests/node_ref.py);
// tests/test_gpu_node.py holds the device equal to that definition too.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rj_node.h"

using namespace rj::node;
namespace cx = rj::crossings;

extern "C" {

// -> 0, 1 (flags, sizes, a malformed map, bad records) or 3 (more points than capacity: *counts holds the true counts),
// the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  origin may be null.
int node_twin(const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const Record* rec, uint64_t n_rec, uint32_t flags, uint64_t capacity,
              int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Counts* counts) {
  memset(counts, 0, sizeof(Counts));
  if (flags & ~kDropLast) return 1;
  if (np >= (1ull << 32) || nc > np || np - nc >= 0xFFFFFFFFull || (nc == 0 && np != 0)) return 1;
  if (n_rec >= (1ull << 31) || (nc == 0 && n_rec)) return 1;
  if (nc == 0) {
    if (out_row) out_row[0] = 0;
    return 0;
  }
  const uint64_t ne = np - nc, n = 2 * n_rec;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. the check
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, cx::check_row(c, row, nc, np));
  for (uint64_t i = 0; i < 2 * np; i++) meta.bad = std::max(meta.bad, cx::check_coordinate(xy[i]));
  if (flags & kDropLast)
    for (uint64_t c = 0; c < nc; c++) meta.bad = std::max(meta.bad, check_chain(c, row, np, xy));
  for (uint64_t r = 0; r < n_rec; r++) meta.bad = std::max(meta.bad, check_record(r, rec, ne, row, nc, xy));
  if (meta.bad) return 1;
  // 2. the candidates: every slot a call can have, the unused ones all ones
  std::vector<Cut> cand(n);
  if (n) memset(cand.data(), 0xFF, sizeof(Cut) * n);
  for (uint64_t r = 0; r < n_rec; r++) {
    const Record& R = rec[r];
    meta.counts.n_proper += R.kind == cx::kProper;
    meta.counts.n_equal += R.kind == cx::kEqual;
    if (!cuts(R.kind)) continue;
    meta.counts.n_used++;
    const uint64_t pe = R.eid[0] + cx::chain_of(R.eid[0], row, nc), pf = R.eid[1] + cx::chain_of(R.eid[1], row, nc);
    const Edge E{xy[2 * pe], xy[2 * pe + 1], xy[2 * pe + 2], xy[2 * pe + 3]}, F{xy[2 * pf], xy[2 * pf + 1], xy[2 * pf + 2], xy[2 * pf + 3]};
    for (int t = 0; t < 4; t++) {
      Cut cut;
      if (!candidate(t, R.eid[0], R.eid[1], E, F, pe, pf, &cut)) continue;
      if (meta.n_cand >= n) return 5;  // (more than two of four tests held: the header's bound is wrong)
      cand[meta.n_cand++] = cut;
    }
  }
  // 3. sorted; the kept cuts numbered
  std::sort(cand.begin(), cand.end(), [](const Cut& a, const Cut& b) { return cut_before(a, b); });
  std::vector<uint32_t> keep(n), kidx(n), first(ne, 0), cnt(ne + 1, 0), prefix(ne + 1);
  uint32_t sum = 0;
  for (uint64_t i = 0; i < n; i++) {
    keep[i] = cut_head(i, cand.data()) ? 1 : 0;
    kidx[i] = sum;
    sum += keep[i];
  }
  // 4. the cuts per edge, scanned
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t e = cand[i].edge;
    if (e == kNoEdge) continue;
    if (run_first(i, cand.data())) first[e] = kidx[i];
    if (run_last(i, n, cand.data())) cnt[e] = kidx[i] + keep[i];
  }
  sum = 0;
  for (uint64_t e = 0; e <= ne; e++) {
    const uint32_t k = e < ne ? cnt[e] - first[e] : 0;
    meta.counts.n_cut_edges += k != 0;
    meta.counts.n_max_cuts = std::max<uint64_t>(meta.counts.n_max_cuts, k);
    prefix[e] = sum;
    sum += k;
  }
  totals(np, nc, n ? (uint64_t) kidx[n - 1] + keep[n - 1] : 0, flags, capacity, &meta.counts, &meta.emit);
  *counts = meta.counts;
  if (np + meta.counts.n_cuts >= (1ull << 32)) return 1;
  if (!meta.emit) return 3;
  // 5. the two scatters
  for (uint64_t c = 0; c <= nc; c++) out_row[c] = (uint32_t) row_slot(c, row, prefix.data(), flags);
  for (uint64_t p = 0; p < np; p++) {
    const uint64_t c = point_chain(p, row, nc);
    const bool last = p + 1 == row[c + 1];
    if (last && (flags & kDropLast)) continue;
    const uint64_t slot = point_slot(p, c, prefix.data(), flags);
    out_xy[2 * slot] = xy[2 * p];
    out_xy[2 * slot + 1] = xy[2 * p + 1];
    if (origin && !last) origin[flags & kDropLast ? slot : slot - c] = (uint32_t) (p - c);
  }
  for (uint64_t i = 0; i < n; i++) {
    if (!keep[i]) continue;
    const Cut cut = cand[i];
    const uint64_t c = cx::chain_of(cut.edge, row, nc), slot = cut_slot(kidx[i], cut.edge, c, first.data(), prefix.data(), flags);
    out_xy[2 * slot] = xy[2 * (uint64_t) cut.src];
    out_xy[2 * slot + 1] = xy[2 * (uint64_t) cut.src + 1];
    if (origin) origin[flags & kDropLast ? slot : slot - c] = cut.edge;
  }
  return 0;
}

}  // extern "C"
