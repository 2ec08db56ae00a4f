// Host twin of rj_eliminate.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_eliminate.h run as plain loops, in the device's stage order -- the check and the chain sums, the
// sides sorted and summed by label, the directed pairs sorted and summed, the arg-max of every face, the pointers, the
// new labels, the keep flags and the scatter.  tests/test_eliminate.py holds it equal to the plain-Python definition
// (tests/eliminate_ref.py); tests/test_gpu_eliminate.py holds the device equal to both.  With ELIMINATE_TWIN_MAIN it is
// a stand-alone program that merges a few built-in maps and checks them: what a host sanitizer run is made of.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_eliminate.h"

using namespace rj::eliminate;
namespace rg = rj::rings;

extern "C" {

uint64_t eliminate_twin_isqrt(uint64_t lo, uint64_t hi) { return isqrt(((u128) hi << 64) | lo); }

// S[nc], L[nc] of a map that passes the check
void eliminate_twin_sums(const int64_t* xy, const uint32_t* row, uint64_t nc, U128* S, U128* L) {
  for (uint64_t c = 0; c < nc; c++) {
    U128 s{0, 0}, l{0, 0};
    for (uint64_t p = row[c]; p + 1 < row[c + 1]; p++) {
      s = rg::add(s, rg::limbs(edge_cross(xy[2 * p], xy[2 * p + 1], xy[2 * p + 2], xy[2 * p + 3])));
      l = rg::add(l, U128{edge_length(xy[2 * p], xy[2 * p + 1], xy[2 * p + 2], xy[2 * p + 3]), 0});
    }
    S[c] = s;
    L[c] = l;
  }
}

// -> 0, 1 (flags, sizes, a malformed map), 3 (a count above its capacity: *counts holds the true counts, nothing is
// written) or 5 (the jumping budget ran out), the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  faces and
// origin may be null; without kDrop out_xy, out_row and origin are not touched.
int eliminate_twin(const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc, uint64_t tol_lo,
                   uint64_t tol_hi, uint32_t flags, uint64_t face_cap, uint64_t chain_cap, uint64_t point_cap, Face* faces, int32_t* out_left,
                   int32_t* out_right, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Counts* counts) {
  memset(counts, 0, sizeof(Counts));
  if (flags & ~kDrop) return 1;
  const bool drop = (flags & kDrop) != 0;
  if (nc >= (1ull << 31) || np >= (1ull << 32) || nc > np || 2 * (np - nc) >= (1ull << 32) || (nc == 0 && np != 0)) return 1;
  if (nc == 0) {
    if (drop && out_row) out_row[0] = 0;
    return 0;
  }
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  const u128 tol = tolerance(tol_lo, tol_hi);
  // 1. the check, the chain sums
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, rg::check_row(c, row, nc, np));
  for (uint64_t i = 0; i < 2 * np; i++) meta.bad = std::max(meta.bad, rg::check_coordinate(xy[i]));
  if (meta.bad) return 1;
  std::vector<U128> S(nc), L(nc);
  eliminate_twin_sums(xy, row, nc, S.data(), L.data());
  // 2. the faces: the sides sorted by key, the unique keys, their sums
  const uint64_t ns = 2 * nc;
  std::vector<uint64_t> order(ns);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return side_key(a, left, right) < side_key(b, left, right); });
  std::vector<uint32_t> keys;
  std::vector<U128> area2;
  for (uint64_t i : order) {
    const uint32_t k = side_key(i, left, right);
    if (keys.empty() || keys.back() != k) {
      keys.push_back(k);
      area2.push_back(U128{0, 0});
    }
    area2.back() = rg::add(area2.back(), side_sum(i, S.data()));
  }
  meta.n_keys = keys.size();
  const uint64_t nf = meta.counts.n_faces = count_faces(meta.n_keys, keys.data());
  // 3. the directed pairs with their weights, ascending; the best of every face
  std::vector<uint64_t> dkey(ns);
  for (uint64_t i = 0; i < ns; i++) dkey[i] = directed_key(i, left, right, keys.data(), nf);
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return dkey[a] < dkey[b]; });
  std::vector<Cand> cand;
  for (uint64_t i : order) {
    if (dkey[i] == kNoPair) break;
    if (cand.empty() || cand.back().dir != dkey[i]) cand.push_back(cand_of(dkey[i], U128{0, 0}));
    const U128 w = rg::add(U128{cand.back().w_lo, cand.back().w_hi}, L[i >> 1]);
    cand.back() = cand_of(dkey[i], w);
  }
  meta.n_dir = cand.size();
  std::vector<uint32_t> best(nf, kNone), first(nf), ptr(nf), flag(nf);
  for (size_t i = 0; i < cand.size();) {
    Cand won = cand[i];
    size_t j = i + 1;
    for (; j < cand.size() && from_of(cand[j].dir) == from_of(cand[i].dir); j++) won = best_of(won, cand[j]);
    best[from_of(won.dir)] = to_of(won.dir);
    i = j;
  }
  // 4. the pointers
  for (uint32_t k = 0; k < nf; k++) first[k] = first_pointer(k, is_sliver(value(area2[k]), tol), best.data());
  for (uint32_t k = 0; k < nf; k++) {
    bool counted;
    ptr[k] = settle_mutual(k, first.data(), area2.data(), &counted);
    meta.counts.n_mutual += counted;
  }
  for (int r = 0; r < kMaxRounds; r++) {
    if (r > 0 && !meta.changed[r - 1]) break;
    for (uint32_t k = 0; k < nf; k++)
      if (jump(k, ptr.data())) meta.changed[r] = 1;
  }
  meta.unfinished = meta.changed[kMaxRounds - 1];
  for (uint32_t k = 0; k < nf; k++) {
    const i128 a = value(area2[k]);
    const uint32_t f = flag[k] = flags_of(k, is_sliver(a, tol), is_negative(a), best.data(), ptr.data());
    meta.counts.n_slivers += (f & kSliver) != 0;
    meta.counts.n_eliminated += (f & kEliminated) != 0;
    meta.counts.n_islands += (f & kIsland) != 0;
    meta.counts.n_negative += (f & kNegative) != 0;
  }
  if (meta.unfinished) return 5;
  // 5. the new labels, what stays, the output: all or nothing
  std::vector<int32_t> nl(nc), nr(nc);
  std::vector<uint32_t> keep(nc), slot(nc), offset(nc);
  uint64_t chains = 0, points = 0;
  for (uint64_t c = 0; c < nc; c++) {
    nl[c] = target_label(left[c], keys.data(), nf, ptr.data());
    nr[c] = target_label(right[c], keys.data(), nf, ptr.data());
    keep[c] = !drop || keeps(left[c], right[c], nl[c], nr[c]);
    slot[c] = (uint32_t) chains;
    offset[c] = (uint32_t) points;
    chains += keep[c];
    points += keep[c] ? row[c + 1] - row[c] : 0;
    meta.counts.n_dropped += !keep[c];
  }
  meta.counts.n_chains = chains;
  meta.counts.n_points = drop ? points : np;
  *counts = meta.counts;
  if (!fits(meta.counts, faces != nullptr, drop, face_cap, chain_cap, point_cap)) return 3;
  if (faces)
    for (uint32_t k = 0; k < nf; k++) faces[k] = record_of(k, keys.data(), area2.data(), flag[k], best.data(), ptr.data());
  for (uint64_t c = 0; c < nc; c++) {
    if (!keep[c]) continue;
    const uint64_t k = slot[c];
    out_left[k] = nl[c];
    out_right[k] = nr[c];
    if (!drop) continue;
    out_row[k] = offset[c];
    if (origin) origin[k] = (uint32_t) c;
    memcpy(out_xy + 2 * (uint64_t) offset[c], xy + 2 * (uint64_t) row[c], 16 * (size_t) (row[c + 1] - row[c]));
  }
  if (drop && out_row) out_row[chains] = (uint32_t) points;  // (every chain dropped fits the sizing call, whose arrays may be null)
  return 0;
}

}  // extern "C"

#if defined(ELIMINATE_TWIN_MAIN)
// a row of three slivers between two squares, a sliver hole, a dangle and a one-point chain: merged at five tolerances,
// with and without kDrop; the areas of the targets before and after agree, and a second call at the same tolerance on a
// map where the first call eliminated nothing eliminates nothing
static U128 total_area(const std::vector<Face>& f) {
  U128 t{0, 0};
  for (const Face& r : f) t = rg::add(t, U128{r.area2_lo, (uint64_t) r.area2_hi});
  return t;
}
int main() {
  std::vector<int64_t> xy;
  std::vector<uint32_t> row{0};
  std::vector<int32_t> left, right;
  auto chain = [&](std::vector<int64_t> pts, int32_t l, int32_t r) {
    xy.insert(xy.end(), pts.begin(), pts.end());
    row.push_back((uint32_t) (xy.size() / 2));
    left.push_back(l);
    right.push_back(r);
  };
  // faces 1 (a 100 x 100 square), 2, 3, 4 (1 x 100 strips to its right), 5 (a 50 x 100 block behind them)
  chain({100, 0, 0, 0, 0, 100, 100, 100}, 0, 1);
  for (int32_t k = 0; k < 4; k++) {
    const int64_t x = 100 + k;
    chain({x, 0, x, 100}, 1 + k, 2 + k);
    chain({x, 0, x + (k == 3 ? 50 : 1), 0}, 2 + k, 0);
    chain({x, 100, x + (k == 3 ? 50 : 1), 100}, 0, 2 + k);
  }
  chain({153, 0, 153, 100}, 5, 0);
  chain({10, 10, 10, 12, 12, 12, 12, 10, 10, 10}, 1, -7);  // a hole of face 1: clockwise, face -7 inside
  chain({50, 50, 60, 60, 70, 50}, 1, 1);                   // a dangle
  chain({500, 500}, 0, 0);
  const uint64_t np = xy.size() / 2, nc = row.size() - 1;
  int failures = 0;
  for (uint64_t tol : {0ull, 8ull, 200ull, 20000ull, ~0ull}) {
    for (uint32_t flags : {0u, kDrop}) {
      Counts c0, c1, c2;
      std::vector<Face> f0(2 * nc), f1(2 * nc);
      std::vector<int32_t> l1(nc), r1(nc), l2(nc), r2(nc);
      std::vector<int64_t> xy1(2 * np), xy2(2 * np);
      std::vector<uint32_t> row1(nc + 1), row2(nc + 1), org(nc);
      const uint64_t hi = tol == ~0ull ? tol : 0;
      const int s0 = eliminate_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, tol, hi, flags, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, &c0);
      const int s1 = eliminate_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, tol, hi, flags, c0.n_faces, c0.n_chains, c0.n_points, f0.data(),
                                    l1.data(), r1.data(), xy1.data(), row1.data(), org.data(), &c1);
      bool ok = s0 == 3 && s1 == 0 && !memcmp(&c0, &c1, sizeof(Counts)) && c1.n_faces == 6;
      f0.resize(c1.n_faces);
      const bool d = flags & kDrop;
      const int s2 = eliminate_twin(d ? xy1.data() : xy.data(), d ? c1.n_points : np, d ? row1.data() : row.data(), l1.data(), r1.data(), c1.n_chains, tol,
                                    hi, flags, 2 * nc, nc, np, f1.data(), l2.data(), r2.data(), xy2.data(), row2.data(), nullptr, &c2);
      f1.resize(c2.n_faces);
      const U128 a0 = total_area(f0), a1 = total_area(f1);
      ok = ok && s2 == 0 && a0.lo == a1.lo && a0.hi == a1.hi && c2.n_faces == c1.n_faces - c1.n_eliminated;
      printf("tol %llu%s flags %u: %llu faces, %llu slivers, %llu eliminated, %llu mutual, %llu dropped: %s\n", (unsigned long long) tol,
             tol == ~0ull ? " (and all the high bits)" : "", flags, (unsigned long long) c1.n_faces, (unsigned long long) c1.n_slivers,
             (unsigned long long) c1.n_eliminated, (unsigned long long) c1.n_mutual, (unsigned long long) c1.n_dropped, ok ? "ok" : "MISMATCH");
      failures += !ok;
    }
  }
  {  // a square between the faces 1 and 2, no face 0: its one chain goes, and the sizing call with null arrays fits
    const int64_t sq[] = {0, 0, 10, 0, 10, 10, 0, 10, 0, 0};
    const uint32_t sq_row[] = {0, 5};
    const int32_t sq_left[] = {1}, sq_right[] = {2};
    Counts c;
    const int s = eliminate_twin(sq, 5, sq_row, sq_left, sq_right, 1, 1000, 0, kDrop, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &c);
    const bool ok = s == 0 && c.n_chains == 0 && c.n_points == 0 && c.n_dropped == 1 && c.n_negative == 1 && c.n_eliminated == 1;
    printf("every chain dropped, null arrays: %s\n", ok ? "ok" : "MISMATCH");
    failures += !ok;
  }
  return failures ? 1 : 0;
}
#endif
