// Host twin of rj_polygons.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_polygons.h run as plain loops, in the device's stage order, with std::sort / plain prefix sums where
// the device calls rocPRIM.  tests/test_polygons.py holds it equal to the plain-Python definition (tests/polygons_ref.py);
// tests/test_gpu_polygons.py holds the device equal to it where the input is too large for the Python loop.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

#include "rj_polygons.h"

using namespace rj::polygons;

extern "C" {

// -> 0, 1 (flags, a malformed input), 3 (a count exceeds its capacity: *counts holds the true counts) or 5 (round budget), the
// values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  stats: the chosen shift, the entries, the ceiling edges,
// the jumping rounds run, the longest bucket scanned for one hole.
int polygons_twin(const Ring* rings, uint64_t nr64, const uint32_t* row, const int64_t* xy, uint64_t np, uint32_t flags, uint64_t polygon_cap,
                  uint64_t member_cap, uint32_t* parent, Polygon* polygons_out, uint32_t* poly_first, uint32_t* poly_ring, Counts* counts,
                  uint64_t* stats) {
  memset(counts, 0, sizeof(Counts));
  if (stats) memset(stats, 0, 5 * sizeof(uint64_t));
  if (flags) return 1;
  if (nr64 > 0xFFFFFFFEull || np >= (1ull << 32) || (nr64 == 0 && np != 0)) return 1;
  const Out o{parent, polygons_out, poly_first, poly_ring, polygon_cap, member_cap};
  if (nr64 == 0) {
    if (o.poly_first) o.poly_first[0] = 0;
    return 0;
  }
  uint32_t bad = 0;
  for (uint64_t c = 0; c <= nr64; c++) bad = std::max(bad, check_row(c, row, nr64, np));
  for (uint64_t r = 0; r < nr64; r++) bad = std::max(bad, check_order(r, rings, nr64));
  for (uint64_t i = 0; i < 2 * np; i++) bad = std::max(bad, check_coordinate(xy[i]));
  if (bad) return 1;
  const uint32_t nr = (uint32_t) nr64;
  const size_t n1 = (size_t) nr64 + 1;
  const uint64_t cap = 2 * np;
  int rounds = 1;
  while ((1ull << (rounds - 1)) < nr64 && rounds < kMaxRounds) rounds++;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. tops and kinds; 2. the ring of every point slot
  std::vector<Top> top(nr);
  std::vector<uint32_t> kind(nr), has(nr), mark(np ? np : 1, 0), ring_at(np ? np : 1);
  for (uint32_t r = 0; r < nr; r++) {
    has[r] = ring_top(r, 0, 1, row, xy, &top[r]) ? 1 : 0;
    kind[r] = ring_kind(rings[r]);
    ring_mark(r, row, mark.data());
  }
  uint32_t running = 0;
  for (uint64_t i = 0; i < np; i++) ring_at[i] = running = std::max(running, mark[i]);
  // 3. the strip width; 4. the entries, sorted
  for (uint64_t i = 0; i < np; i++) meta.n_edges += edge_strips(i, ring_at.data(), rings, row, xy, meta.incid) ? 1 : 0;
  pick_shift(&meta);
  const int shift = (int) meta.shift;
  std::vector<uint64_t> off(np ? np : 1), keys(cap ? cap : 1, kNoKey);
  std::vector<uint32_t> vals(cap ? cap : 1, 0);
  uint64_t acc = 0;
  for (uint64_t i = 0; i < np; i++) {
    off[i] = acc;
    acc += entry_count(i, ring_at.data(), rings, row, xy, shift);
  }
  if (acc != meta.n_entries || acc > cap) return 5;  // (cannot happen)
  for (uint64_t i = 0; i < np; i++) entry_fill(i, ring_at.data(), rings, row, xy, shift, off.data(), keys.data(), vals.data(), cap);
  std::vector<std::pair<uint64_t, uint32_t>> entries(cap);
  for (uint64_t k = 0; k < cap; k++) entries[k] = {keys[k], vals[k]};
  std::stable_sort(entries.begin(), entries.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  for (uint64_t k = 0; k < cap; k++) {
    keys[k] = entries[k].first;
    vals[k] = entries[k].second;
  }
  // 5. the ring above every hole; 6. parents
  std::vector<Jump> jp[2] = {std::vector<Jump>(nr), std::vector<Jump>(nr)};
  uint64_t longest = 0;
  for (uint32_t r = 0; r < nr; r++) {
    uint32_t best = kNone;
    if (kind[r] == kKindHole && has[r]) {
      best = above_scan(r, 0, 1, top[r], rings, ring_at.data(), row, xy, keys.data(), vals.data(), meta.n_entries, shift);
      const uint64_t key = ((uint64_t) (uint32_t) rings[r].face << 32) | strip_of(top[r].x, shift);
      longest = std::max(longest, lower_bound(keys.data(), meta.n_entries, key + 1) - lower_bound(keys.data(), meta.n_entries, key));
      // what a lane group does: the entries dealt to three lanes, their winners reduced
      uint32_t folded = kNone;
      for (uint32_t lane = 0; lane < 3; lane++)
        folded = lower_slot(folded, above_scan(r, lane, 3, top[r], rings, ring_at.data(), row, xy, keys.data(), vals.data(), meta.n_entries, shift),
                            top[r].x, ring_at.data(), row, xy);
      if (folded != best) return 5;
    }
    jump_init(r, kind[r], best, ring_at.data(), jp[0].data(), jp[1].data());
  }
  for (int r = 0; r < rounds; r++) {
    if (!round_needed(meta.act, r)) {
      if (!meta.jump_done) meta.jump_done = (uint32_t) r;
      continue;
    }
    for (uint32_t i = 0; i < nr; i++) meta.act[r] += jump_round(i, jp[r & 1].data(), jp[(r + 1) & 1].data()) ? 1 : 0;
  }
  if (!meta.jump_done) {
    meta.jump_done = (uint32_t) rounds;
    if (meta.act[rounds - 1]) meta.unfinished = 1;
  }
  if (stats) {
    stats[0] = meta.shift;
    stats[1] = meta.n_entries;
    stats[2] = meta.n_edges;
    stats[3] = meta.jump_done;
    stats[4] = longest;
  }
  if (meta.unfinished) return 5;
  const Jump* J = jp[meta.jump_done & 1].data();
  // 7. polygons
  std::vector<uint64_t> skeys(nr);
  for (uint32_t r = 0; r < nr; r++) {
    int what = 0;
    skeys[r] = poly_key(r, kind.data(), J, o.parent, &what);
    meta.counts.n_holes += what == 1;
    meta.counts.n_orphans += what == 2;
    meta.counts.n_face0 += what == 3;
  }
  std::sort(skeys.begin(), skeys.end());
  std::vector<uint32_t> start(n1), pid(n1), first(n1, 0);
  std::vector<U128> area_at(n1), xbase(n1);
  for (size_t j = 0; j < n1; j++) member_mark(j, nr64, skeys.data(), rings, start.data(), area_at.data(), &meta);
  uint32_t pacc = 0;
  for (size_t j = 0; j < n1; j++) {
    pid[j] = pacc;
    pacc += start[j];
  }
  for (size_t j = 0; j < n1; j++) member_place(j, nr64, skeys.data(), start.data(), pid.data(), first.data(), o, &meta);
  U128 xacc{0, 0};
  for (size_t j = 0; j < n1; j++) {
    xbase[j] = xacc;
    xacc = rj::rings::add(xacc, area_at[j]);
  }
  for (uint64_t p = 0; p <= meta.counts.n_polygons; p++) poly_emit(p, skeys.data(), first.data(), xbase.data(), rings, o, &meta);
  *counts = meta.counts;
  return counts->n_polygons > polygon_cap || counts->n_members > member_cap ? 3 : 0;
}

}  // extern "C"
