// Host twin of rj_nearest.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_nearest.h run as a brute force over ALL edges -- every edge with its own quantised box goes through
// the prune (box_lb2, admits against the bound of the candidate held), the case split, the max_dist test and closer(),
// in ascending or in descending eid order, with or without the double filter.  tests/test_nearest.py holds it equal to the
// plain-Python definition (tests/nearest_ref.py); tests/test_gpu_nearest.py holds the device equal to it.  With
// NEAREST_TWIN_MAIN it is a stand-alone program that reads cases with their answers from a file: what a host sanitizer
// run is made of.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rj_nearest.h"

using namespace rj::nearest;
using rj::Seg;

extern "C" {

// seg[ne][4] = (ax, ay, bx, by) in eid order; pts[n][2].  reverse: the edges are taken from the last eid down (the result
// must not depend on it).  filter: closer() with its double filter.  prune 0: every edge is evaluated.  rec, dist and
// evaluated (per point: the edges that were evaluated exactly) may be null.  -> 0, or 1 for a max_dist above kMaxDist.
int nearest_twin(const int64_t* seg, uint64_t ne, const int64_t* pts, uint64_t n, int64_t max_dist, int reverse, int filter, int prune, uint32_t* eid,
                 Near* rec, double* dist, uint64_t* evaluated) {
  if (max_dist > kMaxDist) return 1;
  for (uint64_t i = 0; i < n; i++) {
    const int64_t px = pts[2 * i], py = pts[2 * i + 1];
    const int32_t qx = cell_of(px), qy = cell_of(py);
    Cand best = Cand{kMissEid, 0, 0, 0};
    double best_d2 = 0.0;
    uint64_t ub2 = ub2_of_max_dist(max_dist), count = 0;
    for (uint64_t k = 0; k < ne; k++) {
      const uint64_t e = reverse ? ne - 1 - k : k;
      const Seg s = {seg[4 * e], seg[4 * e + 1], seg[4 * e + 2], seg[4 * e + 3]};
      const int32_t x0 = cell_of(s.x1 < s.x2 ? s.x1 : s.x2), x1 = cell_of(s.x1 < s.x2 ? s.x2 : s.x1);
      const int32_t y0 = cell_of(s.y1 < s.y2 ? s.y1 : s.y2), y1 = cell_of(s.y1 < s.y2 ? s.y2 : s.y1);
      if (box_empty(x0, x1)) continue;  // (never: the box of an edge)
      if (prune && !admits(ub2, box_lb2(x0, y0, x1, y1, qx, qy))) continue;
      count++;
      const Cand c = candidate(s, (uint32_t) e, px, py);
      if (max_dist >= 0 && !within(c, max_dist)) continue;
      const double d2 = approx_d2(c);
      if (best.eid == kMissEid || closer(c, d2, best, best_d2, filter != 0)) {
        best = c;
        best_d2 = d2;
        const uint64_t u = ub2_of(c, d2);
        ub2 = u < ub2 ? u : ub2;
      }
    }
    const bool hit = best.eid != kMissEid;
    eid[i] = best.eid;
    if (rec) rec[i] = hit ? record_of(best) : record_miss();
    if (dist) dist[i] = hit ? dist_of(best) : dist_miss();
    if (evaluated) evaluated[i] = count;
  }
  return 0;
}

// N1 D2 against N2 D1 for N below 2^192 (three limbs, the lowest first) and D below 2^128 (two limbs): -1, 0, 1
int nearest_wide_cmp(const uint64_t* n1, const uint64_t* d2, const uint64_t* n2, const uint64_t* d1) {
  const W5 a = W5{{n1[0], n1[1], n1[2], 0, 0}}, b = W5{{n2[0], n2[1], n2[2], 0, 0}};
  const rj::u128 da = ((rj::u128) d2[1] << 64) | d2[0], db = ((rj::u128) d1[1] << 64) | d1[0];
  return w5_cmp(w5_mul3(a, da), w5_mul3(b, db));
}
// out[5] = a b for a, b below 2^128 (w5_mul); out[5] = n b for n below 2^192 (w5_mul3)
void nearest_wide_mul(const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const W5 r = w5_mul(((rj::u128) a[1] << 64) | a[0], ((rj::u128) b[1] << 64) | b[0]);
  memcpy(out, r.w, sizeof(r.w));
}
void nearest_wide_mul3(const uint64_t* n, const uint64_t* b, uint64_t* out) {
  const W5 r = w5_mul3(W5{{n[0], n[1], n[2], 0, 0}}, ((rj::u128) b[1] << 64) | b[0]);
  memcpy(out, r.w, sizeof(r.w));
}
// the lower bound of the prune for the point and the box of the edge, in the header's unit (d^2 >= 2^32 of it)
uint64_t nearest_box_lb2(const int64_t* s, int64_t px, int64_t py) {
  const int32_t x0 = cell_of(s[0] < s[2] ? s[0] : s[2]), x1 = cell_of(s[0] < s[2] ? s[2] : s[0]);
  const int32_t y0 = cell_of(s[1] < s[3] ? s[1] : s[3]), y1 = cell_of(s[1] < s[3] ? s[3] : s[1]);
  return box_lb2(x0, y0, x1, y1, cell_of(px), cell_of(py));
}
// the upper bound that the edge as a held candidate gives the prune (d^2 <= 2^32 of it)
uint64_t nearest_ub2(const int64_t* s, int64_t px, int64_t py) {
  const Cand c = candidate(Seg{s[0], s[1], s[2], s[3]}, 0, px, py);
  return ub2_of(c, approx_d2(c));
}
uint64_t nearest_ub2_of_max_dist(int64_t max_dist) { return ub2_of_max_dist(max_dist); }

}  // extern "C"

#if defined(NEAREST_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_nearest.py writes, case after case:
//   ne n max_dist | seg[ne][4] | pts[n][2] | n x (eid where num_lo num_hi den_lo den_hi)
// Every case runs in both edge orders, with and without the filter and the prune.
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
    std::vector<int64_t> seg(4 * ne), pts(2 * n);
    for (auto& v : seg) v = num(f);
    for (auto& v : pts) v = num(f);
    std::vector<Near> want(n);
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
      std::vector<uint32_t> eid(n);
      std::vector<Near> rec(n);
      std::vector<double> dist(n);
      ok = nearest_twin(seg.data(), ne, pts.data(), n, max_dist, variant & 1, (variant >> 1) & 1, (variant >> 2) & 1, eid.data(), rec.data(), dist.data(), nullptr) == 0 && ok;
      for (uint64_t i = 0; i < n; i++) {
        const Near &g = rec[i], &w = want[i];
        ok = ok && eid[i] == w.eid && g.eid == w.eid && g.where == w.where && g.num_lo == w.num_lo && g.num_hi == w.num_hi && g.den_lo == w.den_lo &&
             g.den_hi == w.den_hi && (w.eid == kMissEid) == (dist[i] == dist_miss());
      }
    }
    printf("case %d: %llu edges, %llu points, max_dist %lld: %s\n", cases, (unsigned long long) ne, (unsigned long long) n, (long long) max_dist, ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
