// Host twin of rj_snap.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_snap.h run as plain loops, in the device's stage order, with std::sort / plain prefix sums where
// the device calls rocPRIM.  tests/test_snap.py holds it equal to the plain-Python definition (tests/snap_ref.py);
// tests/test_gpu_snap.py holds the device equal to that definition too.  With SNAP_TWIN_MAIN it is a program of its own
// that runs a few maps through snap_twin (for a run under the host sanitizers).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rj_snap.h"

using namespace rj::snap;
namespace cx = rj::crossings;
namespace nd = rj::node;

extern "C" {

// -> 0, 1 (flags, sizes, a malformed map, bad records) or 3 (more points than capacity: *counts holds the true counts),
// the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  origin may be null.
int snap_twin(const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const Record* rec, uint64_t n_rec, uint32_t flags, uint64_t capacity,
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
    for (uint64_t c = 0; c < nc; c++) meta.bad = std::max(meta.bad, nd::check_chain(c, row, np, xy));
  for (uint64_t r = 0; r < n_rec; r++) meta.bad = std::max(meta.bad, nd::check_record(r, rec, ne, row, nc, xy));
  if (meta.bad) return 1;
  // 2. the candidates: every slot a call can have, the unused ones all ones
  std::vector<Cut> cand(n);
  if (n) memset((void*) cand.data(), 0xFF, sizeof(Cut) * n);
  for (uint64_t r = 0; r < n_rec; r++) {
    const Record& R = rec[r];
    meta.counts.n_proper += R.kind == cx::kProper;
    meta.counts.n_equal += R.kind == cx::kEqual;
    if (R.kind == cx::kEqual) continue;
    const uint64_t pe = R.eid[0] + cx::chain_of(R.eid[0], row, nc), pf = R.eid[1] + cx::chain_of(R.eid[1], row, nc);
    const Edge E{xy[2 * pe], xy[2 * pe + 1], xy[2 * pe + 2], xy[2 * pe + 3]}, F{xy[2 * pf], xy[2 * pf + 1], xy[2 * pf + 2], xy[2 * pf + 3]};
    Cut cut[2];
    int k;
    if (nd::cuts(R.kind)) {
      meta.counts.n_used++;
      k = touch_cuts(R.eid[0], R.eid[1], E, F, &cut[0], &cut[1]);
    } else {
      const Proper p = proper_point(E, F);
      uint32_t at_end;
      k = proper_cuts(R.eid[0], R.eid[1], E, F, p, &cut[0], &cut[1], &at_end);
      meta.counts.n_stale += p.stale;
      meta.counts.n_exact += p.exact;
      meta.counts.n_at_end += at_end;
    }
    for (int t = 0; t < k; t++) cand[meta.n_cand++] = cut[t];
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
    const uint32_t e = cut_edge(cand[i]);
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
  for (uint64_t c = 0; c <= nc; c++) out_row[c] = (uint32_t) nd::row_slot(c, row, prefix.data(), flags);
  for (uint64_t p = 0; p < np; p++) {
    const uint64_t c = nd::point_chain(p, row, nc);
    const bool last = p + 1 == row[c + 1];
    if (last && (flags & kDropLast)) continue;
    const uint64_t slot = nd::point_slot(p, c, prefix.data(), flags);
    out_xy[2 * slot] = xy[2 * p];
    out_xy[2 * slot + 1] = xy[2 * p + 1];
    if (origin && !last) origin[flags & kDropLast ? slot : slot - c] = (uint32_t) (p - c);
  }
  for (uint64_t i = 0; i < n; i++) {
    if (!keep[i]) continue;
    const Cut cut = cand[i];
    const uint32_t e = cut_edge(cut);
    const uint64_t c = cx::chain_of(e, row, nc), slot = nd::cut_slot(kidx[i], e, c, first.data(), prefix.data(), flags);
    out_xy[2 * slot] = cut.qx;
    out_xy[2 * slot + 1] = cut.qy;
    if (origin) origin[flags & kDropLast ? slot : slot - c] = e;
  }
  return 0;
}

// the rounded crossing point of two edges alone (the wide arithmetic): e[4], f[4] = ax, ay, bx, by;
// out[4] = stale, exact, qx, qy
void snap_point(const int64_t* e, const int64_t* f, int64_t* out) {
  const Proper p = proper_point(Edge{e[0], e[1], e[2], e[3]}, Edge{f[0], f[1], f[2], f[3]});
  out[0] = p.stale;
  out[1] = p.exact;
  out[2] = p.qx;
  out[3] = p.qy;
}

}  // extern "C"

#if defined(SNAP_TWIN_MAIN)
// all proper crossings of a small map by rj_crossings.h's relation, then one call; a few maps, the results summed
static uint64_t run(const std::vector<int64_t>& xy, const std::vector<uint32_t>& row, uint32_t flags) {
  const uint64_t np = xy.size() / 2, nc = row.size() - 1, ne = np - nc;
  std::vector<Record> rec;
  for (uint32_t e = 0; e < ne; e++)
    for (uint32_t f = e + 1; f < ne; f++) {
      const Edge E = cx::edge_of(e, row.data(), nc, xy.data()), F = cx::edge_of(f, row.data(), nc, xy.data());
      if (cx::is_zero(E) || cx::is_zero(F)) continue;
      const uint32_t k = cx::relate(E, F);
      if (k) rec.push_back(Record{{e, f}, k, 0});
    }
  Counts counts;
  int rc = snap_twin(xy.data(), np, row.data(), nc, rec.data(), rec.size(), flags, 0, nullptr, nullptr, nullptr, &counts);
  if (rc != 0 && rc != 3) return 1000000 + rc;
  std::vector<int64_t> out(2 * counts.n_points);
  std::vector<uint32_t> out_row(nc + 1), origin(counts.n_edges);
  rc = snap_twin(xy.data(), np, row.data(), nc, rec.data(), rec.size(), flags, counts.n_points, out.data(), out_row.data(), origin.data(), &counts);
  uint64_t sum = rc;
  for (int64_t v : out) sum += (uint64_t) v;
  for (uint32_t v : origin) sum += v;
  return sum + out_row[nc] + counts.n_cuts + counts.n_exact + counts.n_at_end;
}

int main() {
  const int64_t L = (int64_t) 1 << 46;
  uint64_t sum = run({0, 0, 4, 4, 0, 4, 4, 0}, {0, 2, 4}, 0);
  sum += run({0, 0, 3, 3, 0, 3, 3, 0}, {0, 2, 4}, 0);
  sum += run({-L, -L, L - 1, L - 2, -L, L - 1, L - 1, -L}, {0, 2, 4}, 0);
  sum += run({0, 0, 4, 0, 4, 4, 0, 4, 0, 0, 2, 2, 6, 2, 6, 6, 2, 6, 2, 2}, {0, 5, 10}, kDropLast);
  sum += run({0, 0, 8, 0, 2, 0, 2, 5, 5, -2, 6, 2, 3, -1, 4, 1}, {0, 2, 4, 6, 8}, 0);
  uint64_t state = 12345;
  for (int m = 0; m < 50; m++) {
    std::vector<int64_t> xy;
    std::vector<uint32_t> row{0};
    for (int c = 0; c < 30; c++) {
      for (int k = 0; k < 4; k++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        xy.push_back((int64_t) ((state >> 33) % 40) * (m % 2 ? (int64_t) 1 << 40 : 1) - (m % 2 ? 20 * ((int64_t) 1 << 40) : 0));
      }
      row.push_back((uint32_t) (xy.size() / 2));
    }
    sum += run(xy, row, 0);
  }
  printf("%llu\n", (unsigned long long) sum);
  return 0;
}
#endif
