// Host twin of rj_knearest.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_knearest.h run as a brute force over ALL edges -- every edge with its own quantised box goes through
// the prune (box_lb2, admits against bound_of the list), the case split, the max_dist test and insert(); the row is written
// by order_step.  The edges are offered in any order the caller gives, with or without the double filter, and the list
// lies in a scratch of any stride that is NOT cleared between the points (as the device re-uses a wave's slab).
// tests/test_knearest.py holds it equal to the plain-Python definition (tests/knearest_ref.py); tests/test_gpu_knearest.py
// holds the device equal to it.  With KNEAREST_TWIN_MAIN it is a stand-alone program that reads cases with their answers
// from a file: what a host sanitizer run is made of.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rj_knearest.h"

using namespace rj::knearest;
using rj::Seg;

extern "C" {

// seg[ne][4] = (ax, ay, bx, by) in eid order; pts[n][2].  offer: null (ascending eids) or a permutation of [0, ne), the
// order the edges are offered in (the result must not depend on it).  filter: the double filter of closer() and of the
// passes over a list.  prune 0: every edge is evaluated.  stride >= 1: words between two words of a list.  Outputs as
// rj_knearest_query's: count[n], eid[n][k], rec[n][k], dist[n][k]; count, rec, dist and entered (per point: the
// candidates that entered the list) may be null.  -> 0, or 1 for a k outside [1, kMaxK] or a max_dist above kMaxDist.
int knearest_twin(const int64_t* seg, uint64_t ne, const int64_t* pts, uint64_t n, uint32_t k, int64_t max_dist, const uint32_t* offer, int filter,
                  int prune, uint64_t stride, uint32_t* count, uint32_t* eid, Near* rec, double* dist, uint64_t* entered) {
  if (k == 0 || k > kMaxK || max_dist > kMaxDist || stride == 0) return 1;
  std::vector<uint64_t> scratch(list_words(k) * stride, 0x7171717171717171ull);
  const List list{scratch.data(), stride};
  const uint64_t base = ub2_of_max_dist(max_dist);
  for (uint64_t i = 0; i < n; i++) {
    const int64_t px = pts[2 * i], py = pts[2 * i + 1];
    const int32_t qx = cell_of(px), qy = cell_of(py);
    Held H = held_none();
    uint64_t ub2 = base, took = 0;
    for (uint64_t t = 0; t < ne; t++) {
      const uint64_t e = offer ? offer[t] : t;
      const Seg s = {seg[4 * e], seg[4 * e + 1], seg[4 * e + 2], seg[4 * e + 3]};
      const int32_t x0 = cell_of(s.x1 < s.x2 ? s.x1 : s.x2), x1 = cell_of(s.x1 < s.x2 ? s.x2 : s.x1);
      const int32_t y0 = cell_of(s.y1 < s.y2 ? s.y1 : s.y2), y1 = cell_of(s.y1 < s.y2 ? s.y2 : s.y1);
      if (prune && !admits(ub2, box_lb2(x0, y0, x1, y1, qx, qy))) continue;
      const Cand c = candidate(s, (uint32_t) e, px, py);
      if (max_dist >= 0 && !within(c, max_dist)) continue;
      if (insert(list, H, k, c, approx_d2(c), filter != 0)) {
        ub2 = bound_of(H, k, base);
        took++;
      }
    }
    const uint64_t row = i * k;
    for (uint32_t j = 0; j < H.count; j++) {
      const Cand c = order_step(list, j, H.count, filter != 0);
      eid[row + j] = c.eid;
      if (rec) rec[row + j] = record_of(c);
      if (dist) dist[row + j] = dist_of(c);
    }
    for (uint32_t j = H.count; j < k; j++) {
      eid[row + j] = kMissEid;
      if (rec) rec[row + j] = record_miss();
      if (dist) dist[row + j] = dist_miss();
    }
    if (count) count[i] = H.count;
    if (entered) entered[i] = took;
  }
  return 0;
}

}  // extern "C"

#if defined(KNEAREST_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_knearest.py writes, case after case:
//   ne n k max_dist | seg[ne][4] | pts[n][2] | n x (count, then count x (eid where num_lo num_hi den_lo den_hi))
// Every case runs ascending and descending, with and without the filter and the prune, at the strides 1 and 64.
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
    const uint32_t k = (uint32_t) word(f);
    const int64_t max_dist = num(f);
    std::vector<int64_t> seg(4 * ne), pts(2 * n);
    for (auto& v : seg) v = num(f);
    for (auto& v : pts) v = num(f);
    std::vector<uint32_t> want_count(n);
    std::vector<Near> want(n * k, record_miss());
    for (uint64_t i = 0; i < n; i++) {
      want_count[i] = (uint32_t) word(f);
      for (uint32_t j = 0; j < want_count[i]; j++) {
        Near& w = want[i * k + j];
        w.eid = (uint32_t) word(f);
        w.where = (uint32_t) word(f);
        w.num_lo = word(f);
        w.num_hi = num(f);
        w.den_lo = word(f);
        w.den_hi = word(f);
      }
    }
    std::vector<uint32_t> down(ne);
    for (uint64_t e = 0; e < ne; e++) down[e] = (uint32_t) (ne - 1 - e);
    bool ok = true;
    for (int variant = 0; variant < 16; variant++) {
      std::vector<uint32_t> count(n), eid(n * k);
      std::vector<Near> rec(n * k);
      std::vector<double> dist(n * k);
      ok = knearest_twin(seg.data(), ne, pts.data(), n, k, max_dist, variant & 1 ? down.data() : nullptr, (variant >> 1) & 1, (variant >> 2) & 1,
                         variant & 8 ? 64 : 1, count.data(), eid.data(), rec.data(), dist.data(), nullptr) == 0 && ok;
      for (uint64_t i = 0; i < n; i++) {
        ok = ok && count[i] == want_count[i];
        for (uint32_t j = 0; j < k; j++) {
          const Near &g = rec[i * k + j], &w = want[i * k + j];
          ok = ok && eid[i * k + j] == w.eid && g.eid == w.eid && g.where == w.where && g.num_lo == w.num_lo && g.num_hi == w.num_hi &&
               g.den_lo == w.den_lo && g.den_hi == w.den_hi && (w.eid == kMissEid) == (dist[i * k + j] == dist_miss());
        }
      }
    }
    printf("case %d: %llu edges, %llu points, k %u, max_dist %lld: %s\n", cases, (unsigned long long) ne, (unsigned long long) n, k, (long long) max_dist,
           ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
