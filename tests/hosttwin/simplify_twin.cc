// Host twin of rj_simplify.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_simplify.h run as plain loops, in the device's stage order -- the check, the pins, the links, the
// rounds over a work list (or, with all_points, over every point), the slots and the scatter.
// tests/test_simplify.py holds it equal to the plain-Python definition (tests/simplify_ref.py);
// tests/test_gpu_simplify.py holds the device equal to both.  With SIMPLIFY_TWIN_MAIN it is a stand-alone program that
// thins a few built-in maps both ways and compares them: what a host sanitizer run is made of.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rj_simplify.h"

using namespace rj::simplify;
namespace cx = rj::crossings;

// what the last call looked at: the rounds it ran (the one that found nothing included) and the sizes of the work lists
// behind the first round, summed -- the device reports the same two numbers
static uint64_t last_rounds_run = 0, last_list_sum = 0;

extern "C" {

void simplify_twin_last(uint64_t* out) {
  out[0] = last_rounds_run;
  out[1] = last_list_sum;
}

// -> 0, 1 (flags, sizes, a malformed map) or 3 (more points than capacity: *counts holds the true counts), the values of
// RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  origin may be null.
int simplify_twin(const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint64_t tol_lo, uint64_t tol_hi, uint32_t flags, int all_points,
                  uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Counts* counts) {
  memset(counts, 0, sizeof(Counts));
  if (flags) return 1;
  if (np >= (1ull << 32) || nc > np || (nc == 0 && np != 0)) return 1;
  if (nc == 0) {
    if (out_row) out_row[0] = 0;
    return 0;
  }
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  const u128 tol = tolerance(tol_lo, tol_hi);
  // 1. the check
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, cx::check_row(c, row, nc, np));
  for (uint64_t i = 0; i < 2 * np; i++) meta.bad = std::max(meta.bad, cx::check_coordinate(xy[i]));
  if (meta.bad) return 1;
  // 2. the links and the pinned ends; the pins of the closed chains
  std::vector<uint8_t> flag(np);
  std::vector<uint32_t> prev(np), next(np), stamp(np, 0), list[2];
  std::vector<u128> stored(np, kNoWeight);
  for (uint64_t c = 0; c < nc; c++) {
    const uint64_t b = row[c], e = row[c + 1];
    for (uint64_t p = b; p < e; p++) {
      flag[p] = chain_end(p, b, e) ? kLive | kPinned : kLive;
      links_of(p, b, e, &prev[p], &next[p]);
    }
  }
  for (uint64_t c = 0; c < nc; c++) {
    const uint64_t b = row[c], e = row[c + 1];
    if (!is_closed(b, e, xy)) continue;
    meta.counts.n_closed++;
    Best m1 = no_best(), m2 = no_best();
    for (uint64_t q = b + 1; q + 1 < e; q++) {
      const Best v = far_of(b, q, xy);
      if (better(v, m1)) m1 = v;
    }
    if (!pins(m1)) continue;
    flag[m1.index] |= kPinned;
    meta.counts.n_pinned_extra++;
    for (uint64_t q = b + 1; q + 1 < e; q++) {
      const Best v = wide_of(b, m1.index, q, xy);
      if (better(v, m2)) m2 = v;
    }
    if (!pins(m2)) continue;
    flag[m2.index] |= kPinned;
    meta.counts.n_pinned_extra++;
  }
  // 3. the rounds: the first over every point, the later ones over the work list of the round before
  int cur = 0;
  bool first = true;
  last_rounds_run = last_list_sum = 0;
  for (uint32_t round = 1;; round++) {
    const bool whole = first || all_points;
    const uint64_t n = whole ? np : list[cur].size();
    if (n == 0) break;
    last_rounds_run++;
    if (!first && !all_points) last_list_sum += n;
    auto item = [&](uint64_t i) { return whole ? i : (uint64_t) list[cur][i]; };
    for (uint64_t i = 0; i < n; i++) stored[item(i)] = stored_weight(item(i), xy, flag.data(), prev.data(), next.data(), tol);
    std::vector<uint8_t> goes(n);
    for (uint64_t i = 0; i < n; i++) goes[i] = removes(item(i), stored.data(), prev.data(), next.data());
    std::vector<uint32_t>& out = list[1 - cur];
    out.clear();
    uint64_t removed = 0;
    auto add = [&](uint32_t q) {
      if (stamp[q] != round) {
        stamp[q] = round;
        out.push_back(q);
      }
    };
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t p = item(i);
      if (goes[i]) {
        const uint32_t u = prev[p], w = next[p];
        unlink(p, flag.data(), prev.data(), next.data());
        stored[p] = kNoWeight;
        removed++;
        if (needs_weight(u, flag.data())) add(u);
        if (needs_weight(w, flag.data())) add(w);
      } else if (stored[p] != kNoWeight) {
        add((uint32_t) p);
      }
    }
    first = false;
    cur = 1 - cur;
    if (!removed) break;
    meta.counts.n_rounds++;
    meta.counts.n_max_round = std::max(meta.counts.n_max_round, removed);
  }
  // 4. the slots, the counts, the scatter: all or nothing
  std::vector<uint32_t> slot(np);
  uint64_t total = 0;
  for (uint64_t p = 0; p < np; p++) {
    slot[p] = (uint32_t) total;
    total += is_live(p, flag.data());
  }
  totals(np, total, capacity, &meta.counts, &meta.emit);
  *counts = meta.counts;
  if (!meta.emit) return 3;
  for (uint64_t c = 0; c <= nc; c++) out_row[c] = (uint32_t) row_slot(c, row, nc, slot.data(), total);
  for (uint64_t p = 0; p < np; p++) {
    if (!is_live(p, flag.data())) continue;
    out_xy[2 * slot[p]] = xy[2 * p];
    out_xy[2 * slot[p] + 1] = xy[2 * p + 1];
    if (origin) origin[slot[p]] = (uint32_t) p;
  }
  return 0;
}

}  // extern "C"

#if defined(SIMPLIFY_TWIN_MAIN)
// a square with mid-side points, a long zigzag with collinear stretches, one-point chains between them: thinned over
// the work list and over all points at five tolerances, the two compared; then thinned again, which must remove nothing
int main() {
  std::vector<int64_t> xy;
  std::vector<uint32_t> row{0};
  auto chain = [&](std::vector<int64_t> pts) {
    xy.insert(xy.end(), pts.begin(), pts.end());
    row.push_back((uint32_t) (xy.size() / 2));
  };
  chain({0, 0, 5, 0, 10, 0, 10, 5, 10, 10, 5, 10, 0, 10, 0, 5, 0, 0});
  chain({7, 7});
  std::vector<int64_t> zig;
  for (int64_t i = 0; i < 3000; i++) {
    zig.push_back(3 * i);
    zig.push_back(i % 17 < 9 ? 2 * i : (i * i) % 23);
  }
  chain(zig);
  chain({-4, -4});
  chain({0, 0, 4, 0, 0, 0});
  const uint64_t np = xy.size() / 2, nc = row.size() - 1;
  int failures = 0;
  for (uint64_t tol : {0ull, 3ull, 40ull, 5000ull, ~0ull}) {
    std::vector<int64_t> a(2 * np), b(2 * np), c(2 * np);
    std::vector<uint32_t> ra(nc + 1), rb(nc + 1), rc(nc + 1), oa(np), ob(np);
    Counts ca, cb, cc;
    const int s1 = simplify_twin(xy.data(), np, row.data(), nc, tol, tol == ~0ull ? tol : 0, 0, 0, np, a.data(), ra.data(), oa.data(), &ca);
    const int s2 = simplify_twin(xy.data(), np, row.data(), nc, tol, tol == ~0ull ? tol : 0, 0, 1, np, b.data(), rb.data(), ob.data(), &cb);
    bool ok = s1 == 0 && s2 == 0 && !memcmp(&ca, &cb, sizeof(Counts)) && ra == rb && !memcmp(a.data(), b.data(), 16 * ca.n_points) &&
              !memcmp(oa.data(), ob.data(), 4 * ca.n_points);
    const int s3 = simplify_twin(a.data(), ca.n_points, ra.data(), nc, tol, tol == ~0ull ? tol : 0, 0, 0, np, c.data(), rc.data(), nullptr, &cc);
    ok = ok && s3 == 0 && cc.n_removed == 0 && cc.n_points == ca.n_points && ra == rc && !memcmp(a.data(), c.data(), 16 * ca.n_points);
    printf("tol %llu%s: %llu of %llu points in %llu rounds: %s\n", (unsigned long long) tol, tol == ~0ull ? " (and all the high bits)" : "",
           (unsigned long long) ca.n_points, (unsigned long long) np, (unsigned long long) ca.n_rounds, ok ? "ok" : "MISMATCH");
    failures += !ok;
  }
  return failures ? 1 : 0;
}
#endif
