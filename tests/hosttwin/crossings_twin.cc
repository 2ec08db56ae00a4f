// Host twin of rj_crossings.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_crossings.h run as plain loops, in the device's stage order, with std::stable_sort / plain prefix
// sums where the device calls rocPRIM.  tests/test_crossings.py holds it equal to the plain-Python definition
// (tests/crossings_ref.py); tests/test_gpu_crossings.py holds the device equal to both.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_crossings.h"

using namespace rj::crossings;

extern "C" {

struct Record {  // rj_crossing
  uint32_t eid[2], kind, pad;
};

// -> 0, 1 (flags, sizes, a malformed map, the guard) or 3 (more records than capacity: *counts holds the true counts),
// the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  shift 0: choose; budget, extent_factor, reg_factor 0: the defaults.
// stats[6]: the shift, the registrations, the longest run, the pair tests, the work items, 1 when the guard refused.
int crossings_twin(const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint32_t flags, uint64_t capacity, Record* out, Counts* counts,
                   int shift, uint64_t budget, uint64_t extent_factor, uint64_t reg_factor, uint64_t* stats) {
  memset(counts, 0, sizeof(Counts));
  if (stats) memset(stats, 0, 6 * sizeof(uint64_t));
  if (flags) return 1;
  if (np >= (1ull << 32) || nc > np || np - nc >= 0xFFFFFFFFull || (nc == 0 && np != 0)) return 1;
  if (shift && (shift < kMinShift || shift > kMaxShift)) return 1;
  if (nc == 0) return 0;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, check_row(c, row, nc, np));
  for (uint64_t i = 0; i < 2 * np; i++) meta.bad = std::max(meta.bad, check_coordinate(xy[i]));
  if (meta.bad) return 1;
  // A. the edges, the sums behind the choice of the shift
  const uint64_t ne = np - nc;
  meta.counts.n_edges = ne;
  std::vector<Edge> edges(ne);
  for (uint64_t e = 0; e < ne; e++) {
    const Edge E = edges[e] = edge_of(e, row, nc, xy);
    if (is_zero(E)) {
      meta.counts.n_zero_edges++;
      continue;
    }
    for (int k = 0; k < kShifts; k++) meta.regs[k] = clamp_add(meta.regs[k], reg_count(E, kMinShift + k));
    const uint64_t ext = extent_of(E);
    meta.extent_lo += ext & 0xFFFFFFFFull;
    meta.extent_hi += ext >> 32;
  }
  *counts = meta.counts;
  const uint64_t n_live = ne - meta.counts.n_zero_edges;
  if (n_live < 2) return 0;
  const int s = shift ? shift
                      : choose_shift(meta.extent_lo, meta.extent_hi, meta.regs, n_live, ne, extent_factor ? extent_factor : kExtentFactor,
                                     reg_factor ? reg_factor : kRegFactor);
  const uint64_t R = meta.regs[s - kMinShift];
  if (stats) stats[0] = (uint64_t) s, stats[1] = R;
  if (R >= kClamp) return 1;
  // B. the registrations, sorted by cell; runs and work items
  std::vector<uint64_t> cnt(ne + 1), off(ne + 1), key(R), skey(R), start(R), items;
  std::vector<uint32_t> eid(R), seid(R), order(R);
  for (uint64_t e = 0; e <= ne; e++) cnt[e] = e < ne && !is_zero(edges[e]) ? reg_count(edges[e], s) : 0;
  uint64_t sum = 0;
  for (uint64_t e = 0; e <= ne; e++) {
    off[e] = sum;
    sum += cnt[e];
  }
  for (uint64_t r = 0; r < R; r++) reg_at(r, off.data(), ne, edges.data(), s, &key[r], &eid[r]);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  for (uint64_t r = 0; r < R; r++) skey[r] = key[order[r]], seid[r] = eid[order[r]];
  uint64_t running = 0;
  for (uint64_t r = 0; r < R; r++) start[r] = running = std::max(running, run_head(r, skey.data()));
  for (uint64_t r = 0; r < R; r++) {
    uint64_t k;
    if (item_flag(r, R, skey.data(), start.data(), &k)) items.push_back(r);
    if (k) meta.pair_tests = clamp_add(meta.pair_tests, run_tests(k));
    meta.largest_run = std::max(meta.largest_run, k);
  }
  if (stats) stats[2] = meta.largest_run, stats[3] = meta.pair_tests, stats[4] = items.size();
  if (meta.pair_tests > (budget ? budget : kPairBudget)) {
    if (stats) stats[5] = 1;
    return 1;
  }
  // C. the pair pass; the hits sorted
  std::vector<std::pair<uint64_t, uint32_t>> hits;
  for (const uint64_t p : items)
    for (uint64_t j = p + 1; j < R && skey[j] == skey[p]; j++)
      for (uint64_t i = p; i < row_limit(p, j); i++) {
        const uint32_t kind = pair_kind(edges[seid[i]], edges[seid[j]], skey[p], s);
        if (kind == kNone) continue;
        hits.emplace_back(hit_key(seid[i], seid[j]), kind);
        (&meta.counts.n_proper)[kind - 1]++;
      }
  meta.counts.n_found = hits.size();
  *counts = meta.counts;
  if (hits.size() > capacity) return 3;
  std::sort(hits.begin(), hits.end());
  for (size_t r = 0; r < hits.size(); r++) out[r] = Record{{(uint32_t) (hits[r].first >> 32), (uint32_t) hits[r].first}, hits[r].second, 0};
  return 0;
}

}  // extern "C"
