// Host twin of rj_dissolve.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_dissolve.h run as plain loops, in the device's stage order -- the check, the classes and what is
// kept, the chain ends sorted and next, the two passes of pointer doubling, the class records, the totals, their scan and
// the scatter.  tests/test_dissolve.py holds it equal to the plain-Python definition (tests/dissolve_ref.py);
// tests/test_gpu_dissolve.py holds the device equal to both.  With DISSOLVE_TWIN_MAIN it is a stand-alone program that
// reads cases with their answers from a file of numbers and checks them: what a host sanitizer run is made of.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_dissolve.h"

using namespace rj::dissolve;
namespace rg = rj::rings;
namespace rm = rj::ringmap;

extern "C" {

// -> 0, 1 (flags, sizes, a malformed map, unmapped labels: *counts holds n_unmapped), 3 (a count above its capacity:
// *counts holds the true counts, nothing is written) or 5 (the doubling budget ran out), the values of RJ_OK,
// RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  table, classes, origin and chain_out may be null.
int dissolve_twin(const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc, const int32_t* table,
                  uint64_t n_labels, uint32_t flags, uint64_t class_cap, uint64_t chain_cap, uint64_t point_cap, ClassRec* classes, int32_t* out_left,
                  int32_t* out_right, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, uint32_t* chain_out, Counts* counts) {
  memset(counts, 0, sizeof(Counts));
  if (flags & ~kKeepEqual) return 1;
  if (table && n_labels == 0) return 1;
  if (nc >= (1ull << 31) || np >= (1ull << 32) || nc > np || 2 * (np - nc) >= (1ull << 32) || (nc == 0 && np != 0)) return 1;
  if (nc == 0) {
    if (out_row) out_row[0] = 0;
    return 0;
  }
  const Out o{classes, out_left, out_right, out_xy, out_row, origin, chain_out, classes ? class_cap : 0, chain_cap, point_cap};
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. the check, the classes, what is kept, the chain sums
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, rg::check_row(c, row, nc, np));
  std::vector<U128> S(nc);
  std::vector<int32_t> cl(nc), cr(nc);
  std::vector<uint32_t> state(nc);
  for (uint64_t c = 0; c < nc; c++) {
    i128 sum = 0;
    bool differs = false;
    uint32_t unmapped;
    chain_scan(c, 0, 1, xy, row, np, &meta.bad, &sum, &differs);
    const uint32_t st = chain_finish(c, left, right, table, n_labels, flags, sum, differs, cl.data(), cr.data(), S.data(), state.data(), &unmapped);
    meta.counts.n_dropped += st == kDropped;
    meta.counts.n_kept += st == kKept;
    meta.counts.n_skipped += st == kSkipped;
    meta.counts.n_unmapped += unmapped;
  }
  if (meta.bad) return 1;
  if (meta.counts.n_unmapped) {
    counts->n_unmapped = meta.counts.n_unmapped;
    return 1;
  }
  // 2. the chain ends by start point, next
  const uint64_t nh = 2 * nc, kept = 2 * meta.counts.n_kept;
  std::vector<uint32_t> seed(nh), pos(nh, kNone), next(nh);
  std::vector<Pt> start(nh);
  for (uint64_t h = 0; h < nh; h++) half_seed((uint32_t) h, state.data(), xy, row, seed.data(), start.data());
  std::vector<uint32_t> order(seed);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return half_before(a, b, start.data()); });
  for (uint64_t k = 0; k < kept; k++) half_pos(k, order.data(), pos.data());
  for (uint64_t h = 0; h < nh; h++)
    next[h] = state[h >> 1] == kKept ? next_of((uint32_t) h, kept, order.data(), pos.data(), start.data(), cl.data(), cr.data()) : kNone;
  // 3. the walks: two passes, the buffers swapped every round
  int rounds = 1;
  while ((1ull << (rounds - 1)) < nh && rounds < kMaxRounds) rounds++;
  std::vector<Walk> w0(nh), w1(nh);
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 0)
      for (uint64_t h = 0; h < nh; h++) walk_init((uint32_t) h, next.data(), row, w0.data(), w1.data());
    else {
      const std::vector<Walk> F((meta.done[0] & 1) ? w1 : w0);  // (the device reads and writes in place, every h its own entry)
      for (uint64_t h = 0; h < nh; h++) cut_init((uint32_t) h, F.data(), next.data(), row, w0.data(), w1.data());
    }
    for (int r = 0; r < rounds; r++) {
      if (!rm::round_needed(meta.act[pass], r)) {
        if (!meta.done[pass]) meta.done[pass] = (uint32_t) r;
        continue;
      }
      const Walk* in = (r & 1) ? w1.data() : w0.data();
      Walk* out = (r & 1) ? w0.data() : w1.data();
      for (uint64_t i = 0; i < nh; i++) meta.act[pass][r] += rm::walk_round((uint32_t) i, in, out) ? 1u : 0u;
    }
    if (!meta.done[pass]) {
      meta.done[pass] = (uint32_t) rounds;
      if (meta.act[pass][rounds - 1]) meta.unfinished = 1;
    }
  }
  if (meta.unfinished) return 5;
  const Walk* W = (meta.done[1] & 1) ? w1.data() : w0.data();
  // 4. the class records: the sides sorted by key, the unique keys, their sums
  std::vector<uint64_t> by_key(nh);
  std::iota(by_key.begin(), by_key.end(), 0);
  std::stable_sort(by_key.begin(), by_key.end(),
                   [&](uint64_t a, uint64_t b) { return side_key(a, state.data(), cl.data(), cr.data()) < side_key(b, state.data(), cl.data(), cr.data()); });
  std::vector<uint32_t> keys;
  std::vector<Side> sums;
  for (uint64_t i : by_key) {
    const uint32_t k = side_key(i, state.data(), cl.data(), cr.data());
    if (keys.empty() || keys.back() != k) {
      keys.push_back(k);
      sums.push_back(Side{U128{0, 0}, 0});
    }
    sums.back() = side_add(sums.back(), side_val(i, S.data()));
  }
  meta.n_keys = keys.size();
  // 5. the totals, their scan, the scatter: all or nothing
  std::vector<Slots> total(nh + 1), base(nh + 1);
  for (uint64_t h = 0; h <= nh; h++) meta.counts.n_closed += chain_total(h, nh, state.data(), W, next.data(), row, total.data()) ? 1 : 0;
  Slots run{0, 0};
  for (uint64_t h = 0; h <= nh; h++) {
    base[h] = run;
    run = Slots{run.halves + total[h].halves, run.points + total[h].points};
  }
  meta.counts.n_chains = base[nh].halves;
  meta.counts.n_points = base[nh].points;
  meta.counts.n_classes = rj::eliminate::count_faces(meta.n_keys, keys.data());
  *counts = meta.counts;
  if (!fits(meta.counts, o)) return 3;
  if (o.row) o.row[meta.counts.n_chains] = (uint32_t) meta.counts.n_points;
  if (o.classes)
    for (uint64_t k = 0; k < meta.counts.n_classes; k++) o.classes[k] = record_of(k, keys.data(), sums.data());
  for (uint64_t c = 0; c < nc; c++) chain_place(c, 0, 1, xy, row, state.data(), cl.data(), cr.data(), W, base.data(), o);
  return 0;
}

}  // extern "C"

#if defined(DISSOLVE_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_dissolve.py writes, case after case:
//   np nc n_labels (-1: no table) flags | xy[2 np] row[nc + 1] left[nc] right[nc] table[n_labels]
//   | status counts[8] | out_xy[2 n_points] out_row[n_chains + 1] out_left out_right origin [n_chains] chain_out[nc]
//   | n_classes x (label n_sides area2_lo area2_hi)       (the outputs only where status is 0)
// Every case runs as the sizing call, then with the exact capacities, with records, origin and chain_out.
static bool more(FILE* f, long long* v) { return fscanf(f, "%lld", v) == 1; }
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
  while (more(f, &first)) {
    const uint64_t np = (uint64_t) first, nc = word(f);
    const long long nl = num(f);
    const uint32_t flags = (uint32_t) word(f);
    std::vector<int64_t> xy(2 * np);
    std::vector<uint32_t> row(nc + 1);
    std::vector<int32_t> left(nc), right(nc), table(nl > 0 ? nl : 0);
    for (auto& v : xy) v = num(f);
    for (auto& v : row) v = (uint32_t) word(f);
    for (auto& v : left) v = (int32_t) num(f);
    for (auto& v : right) v = (int32_t) num(f);
    for (auto& v : table) v = (int32_t) num(f);
    const int want_status = (int) num(f);
    uint64_t want[8];
    for (auto& v : want) v = word(f);
    const int32_t* tab = nl >= 0 ? table.data() : nullptr;
    Counts c0, c1;
    const int s0 = dissolve_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, tab, (uint64_t) (nl > 0 ? nl : 0), flags, 0, 0, 0, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, &c0);
    bool ok = !memcmp(&c0, want, sizeof(want));
    if (want_status != 0) {
      ok = ok && s0 == want_status;
    } else {
      ok = ok && (s0 == 0 || s0 == 3);
      const uint64_t n = c0.n_chains, npts = c0.n_points, ncl = c0.n_classes;
      std::vector<int64_t> oxy(2 * npts), wxy(2 * npts);
      std::vector<uint32_t> orow(n + 1), wrow(n + 1), org(n), worg(n), cout_(nc), wcout(nc);
      std::vector<int32_t> ol(n), orr(n), wl(n), wr(n);
      std::vector<ClassRec> recs(ncl);
      for (auto& v : wxy) v = num(f);
      for (auto& v : wrow) v = (uint32_t) word(f);
      for (auto& v : wl) v = (int32_t) num(f);
      for (auto& v : wr) v = (int32_t) num(f);
      for (auto& v : worg) v = (uint32_t) word(f);
      for (auto& v : wcout) v = (uint32_t) word(f);
      const int s1 = dissolve_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, tab, (uint64_t) (nl > 0 ? nl : 0), flags, ncl, n, npts, recs.data(),
                                   ol.data(), orr.data(), oxy.data(), orow.data(), org.data(), cout_.data(), &c1);
      ok = ok && s1 == 0 && !memcmp(&c1, want, sizeof(want)) && oxy == wxy && orow == wrow && ol == wl && orr == wr && org == worg && cout_ == wcout;
      for (uint64_t k = 0; k < ncl; k++) {
        const int32_t label = (int32_t) num(f);
        const uint32_t sides = (uint32_t) word(f);
        const uint64_t lo = word(f);
        const int64_t hi = num(f);
        ok = ok && recs[k].label == label && recs[k].n_sides == sides && recs[k].area2_lo == lo && recs[k].area2_hi == hi;
      }
    }
    printf("case %d: %llu chains, %llu points -> %llu chains, %llu points: %s\n", cases, (unsigned long long) nc, (unsigned long long) np,
           (unsigned long long) c0.n_chains, (unsigned long long) c0.n_points, ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
