// Host twin of rj_within.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_within.h and rj_nearest.h run as a brute force over ALL edges, through the device's own pipeline --
// every edge with its own quantised box goes through the prune (the reject against the box of the whole call's cells, then
// box_lb2 and admits against the bound of max_dist), the case split and within_filtered; a hit is counted and appended as
// a key while there is room; the counts are scanned; the keys are sorted over key_bits(n) bits only, stably; eid, record and
// distance are recomputed from the sorted keys.  Points and edges are taken in ascending or in descending order (the result
// must not depend on it), with or without the double filter, with or without the prune.  tests/test_within.py holds it equal
// to the plain-Python definition (tests/within_ref.py); tests/test_gpu_within.py holds the device equal to it.  With
// WITHIN_TWIN_MAIN it is a stand-alone program that reads cases with their answers from a file: what a host sanitizer run
// is made of.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rj_within.h"

using namespace rj::nearest;
using namespace rj::within;
using rj::Seg;

extern "C" {

// seg[ne][4] = (ax, ay, bx, by) in eid order; pts[n][2].  capacity 0: the counting call.  offsets[n + 1], rec, dist and
// evaluated (per point: the edges that were evaluated exactly) may be null; eid may be null in the counting call.
// counts[3] = n_pairs, n_points_hit, max_per_point.  -> 0; 1 for a bad max_dist, n or capacity (nothing written); 3 when the
// pairs do not fit (counts and offsets written, nothing else).
int within_twin(const int64_t* seg, uint64_t ne, const int64_t* pts, uint64_t n, int64_t max_dist, int reverse, int filter, int prune, uint64_t capacity,
                uint64_t* offsets, uint32_t* eid, Near* rec, double* dist, uint64_t* counts, uint64_t* evaluated) {
  if (max_dist < 0 || max_dist > kMaxDist || n >= kMaxPoints || capacity >= kMaxPoints || !counts || (capacity && !eid)) return 1;
  const uint64_t ub2 = ub2_of_max_dist(max_dist);
  const double m2 = approx_m2(max_dist);
  int32_t gx0 = 0x7FFFFFFF, gy0 = 0x7FFFFFFF, gx1 = -1, gy1 = -1;  // the box of the cells of all points: the "group"
  for (uint64_t i = 0; i < n; i++) {
    const int32_t qx = cell_of(pts[2 * i]), qy = cell_of(pts[2 * i + 1]);
    gx0 = qx < gx0 ? qx : gx0, gx1 = qx > gx1 ? qx : gx1, gy0 = qy < gy0 ? qy : gy0, gy1 = qy > gy1 ? qy : gy1;
  }
  // every edge's quantised box, and whether the reject against the group's box keeps it: neither depends on the point
  std::vector<int32_t> bx0(ne), by0(ne), bx1(ne), by1(ne);
  std::vector<char> near_group(ne);
  for (uint64_t e = 0; e < ne; e++) {
    const int64_t* s = seg + 4 * e;
    bx0[e] = cell_of(s[0] < s[2] ? s[0] : s[2]), bx1[e] = cell_of(s[0] < s[2] ? s[2] : s[0]);
    by0[e] = cell_of(s[1] < s[3] ? s[1] : s[3]), by1[e] = cell_of(s[1] < s[3] ? s[3] : s[1]);
    near_group[e] = n && admits(ub2, group_lb2(bx0[e], by0[e], bx1[e], by1[e], gx0, gy0, gx1, gy1));
  }
  std::vector<uint32_t> cnt(n + 1, 0);
  std::vector<uint64_t> keys(capacity);
  uint64_t appended = 0;
  for (uint64_t t = 0; t < n; t++) {
    const uint64_t i = reverse ? n - 1 - t : t;
    const int64_t px = pts[2 * i], py = pts[2 * i + 1];
    const int32_t qx = cell_of(px), qy = cell_of(py);
    uint64_t count = 0;
    for (uint64_t k = 0; k < ne; k++) {
      const uint64_t e = reverse ? ne - 1 - k : k;
      if (box_empty(bx0[e], bx1[e])) continue;  // (never: the box of an edge)
      if (prune && !near_group[e]) continue;
      if (prune && !admits(ub2, box_lb2(bx0[e], by0[e], bx1[e], by1[e], qx, qy))) continue;
      const Seg s = {seg[4 * e], seg[4 * e + 1], seg[4 * e + 2], seg[4 * e + 3]};
      count++;
      if (!within_filtered(candidate(s, (uint32_t) e, px, py), max_dist, m2, filter != 0)) continue;
      cnt[i]++;
      if (appended < capacity) keys[appended] = pair_key((uint32_t) i, (uint32_t) e);
      appended++;  // (a position at or behind the capacity is counted and not written)
    }
    if (evaluated) evaluated[i] = count;
  }
  // the scan and the totals
  std::vector<uint64_t> scanned(n + 1, 0);
  uint64_t hit = 0, longest = 0;
  for (uint64_t i = 0; i < n; i++) {
    scanned[i + 1] = scanned[i] + cnt[i];
    hit += cnt[i] != 0;
    longest = cnt[i] > longest ? cnt[i] : longest;
  }
  const uint64_t n_pairs = scanned[n];
  if (n_pairs != appended) return 5;
  counts[0] = n_pairs, counts[1] = hit, counts[2] = longest;
  if (offsets) memcpy(offsets, scanned.data(), (n + 1) * sizeof(uint64_t));
  if (!capacity) return 0;
  if (n_pairs > capacity) return 3;
  // the sort over the bits in use, and the outputs from the sorted keys
  const int bits = key_bits(n);
  const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
  keys.resize(n_pairs);
  std::stable_sort(keys.begin(), keys.end(), [mask](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });
  for (uint64_t k = 0; k < n_pairs; k++) {
    const uint32_t e = key_eid(keys[k]), p = key_point(keys[k]);
    eid[k] = e;
    if (!rec && !dist) continue;
    if (e >= ne || p >= n) return 5;  // (a mutated key: nothing to recompute from)
    const Cand c = candidate(Seg{seg[4 * (uint64_t) e], seg[4 * (uint64_t) e + 1], seg[4 * (uint64_t) e + 2], seg[4 * (uint64_t) e + 3]}, e, pts[2 * (uint64_t) p],
                             pts[2 * (uint64_t) p + 1]);
    if (rec) rec[k] = record_of(c);
    if (dist) dist[k] = dist_of(c);
  }
  return 0;
}

// the filter alone: 1 in, -1 out, 0 undecided
int within_in_or_out(double d2, double m2) { return in_or_out(d2, m2); }
int within_key_bits(uint64_t n) { return key_bits(n); }
uint64_t within_pair_key(uint32_t point, uint32_t eid) { return pair_key(point, eid); }
// the lower bound of the wave-uniform reject for the box of the edge s against the group's box g = {gx0, gy0, gx1, gy1} in cells
uint64_t within_group_lb2(const int64_t* s, const int32_t* g) {
  const int32_t x0 = cell_of(s[0] < s[2] ? s[0] : s[2]), x1 = cell_of(s[0] < s[2] ? s[2] : s[0]);
  const int32_t y0 = cell_of(s[1] < s[3] ? s[1] : s[3]), y1 = cell_of(s[1] < s[3] ? s[3] : s[1]);
  return group_lb2(x0, y0, x1, y1, g[0], g[1], g[2], g[3]);
}
// ... and the per-point lower bound of the same box
uint64_t within_point_lb2(const int64_t* s, int64_t px, int64_t py) {
  const int32_t x0 = cell_of(s[0] < s[2] ? s[0] : s[2]), x1 = cell_of(s[0] < s[2] ? s[2] : s[0]);
  const int32_t y0 = cell_of(s[1] < s[3] ? s[1] : s[3]), y1 = cell_of(s[1] < s[3] ? s[3] : s[1]);
  return box_lb2(x0, y0, x1, y1, cell_of(px), cell_of(py));
}

}  // extern "C"

#if defined(WITHIN_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_within.py writes, case after case:
//   ne n max_dist n_pairs | seg[ne][4] | pts[n][2] | offsets[n + 1] | n_pairs x (eid where num_lo num_hi den_lo den_hi)
// Every case runs in both orders, with and without the filter and the prune, at the exact capacity; then the counting call
// and, where there is a pair, the overflow at one less.
static unsigned long long word(FILE* f) {
  unsigned long long v = 0;
  if (fscanf(f, "%llu", &v) != 1) exit(2);
  return v;
}
static long long num(FILE* f) {
  long long v = 0;
  if (fscanf(f, "%lld", &v) != 1) exit(2);
  return v;
}
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  int failures = 0, cases = 0;
  long long first;
  while (fscanf(f, "%lld", &first) == 1) {
    const uint64_t ne = (uint64_t) first, n = word(f);
    const int64_t max_dist = num(f);
    const uint64_t n_pairs = word(f);
    std::vector<int64_t> seg(4 * ne), pts(2 * n);
    for (auto& v : seg) v = num(f);
    for (auto& v : pts) v = num(f);
    std::vector<uint64_t> want_off(n + 1);
    for (auto& v : want_off) v = word(f);
    std::vector<Near> want(n_pairs);
    for (auto& w : want) {
      w.eid = (uint32_t) word(f);
      w.where = (uint32_t) word(f);
      w.num_lo = word(f);
      w.num_hi = num(f);
      w.den_lo = word(f);
      w.den_hi = word(f);
    }
    bool ok = true;
    for (int variant = 0; variant < 8; variant++) {
      std::vector<uint64_t> off(n + 1);
      std::vector<uint32_t> eid(n_pairs + 1);
      std::vector<Near> rec(n_pairs + 1);
      std::vector<double> dist(n_pairs + 1);
      uint64_t counts[3] = {0, 0, 0};
      const int rc = within_twin(seg.data(), ne, pts.data(), n, max_dist, variant & 1, (variant >> 1) & 1, (variant >> 2) & 1, n_pairs + 1, off.data(), eid.data(),
                                 rec.data(), dist.data(), counts, nullptr);
      ok = ok && rc == 0 && counts[0] == n_pairs && off == want_off;
      for (uint64_t k = 0; ok && k < n_pairs; k++) {
        const Near &g = rec[k], &w = want[k];
        ok = eid[k] == w.eid && g.eid == w.eid && g.where == w.where && g.num_lo == w.num_lo && g.num_hi == w.num_hi && g.den_lo == w.den_lo &&
             g.den_hi == w.den_hi && dist[k] >= 0.0;
      }
      uint64_t counted[3] = {0, 0, 0};
      std::vector<uint64_t> off2(n + 1);
      ok = ok && within_twin(seg.data(), ne, pts.data(), n, max_dist, variant & 1, (variant >> 1) & 1, (variant >> 2) & 1, 0, off2.data(), nullptr, nullptr, nullptr,
                             counted, nullptr) == 0 && off2 == want_off && counted[0] == n_pairs;
      if (n_pairs > 1)
        ok = ok && within_twin(seg.data(), ne, pts.data(), n, max_dist, variant & 1, (variant >> 1) & 1, (variant >> 2) & 1, n_pairs - 1, off2.data(), eid.data(),
                               nullptr, nullptr, counted, nullptr) == 3 && counted[0] == n_pairs;
    }
    printf("case %d: %llu edges, %llu points, max_dist %lld, %llu pairs: %s\n", cases, (unsigned long long) ne, (unsigned long long) n, (long long) max_dist,
           (unsigned long long) n_pairs, ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
