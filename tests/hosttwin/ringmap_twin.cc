// Host twin of rj_ringmap.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_ringmap.h run as plain loops, in the device's stage order, with std::sort / std::merge / plain prefix
// sums where the device calls rocPRIM.  tests/test_ringmap.py holds it equal to the plain-Python definition
// (tests/ringmap_ref.py); tests/test_gpu_ringmap.py holds the device equal to it where the input is too large for the
// Python loop.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_ringmap.h"

using namespace rj::ringmap;

extern "C" {

// -> 0, 1 (flags, stride, a malformed input), 3 (a count exceeds its capacity: *counts holds the true counts) or 5 (round
// budget), the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  stats: the rounds of the two doubling passes.
int ringmap_twin(const uint32_t* row, const int64_t* xy, uint64_t n, const void* face, uint64_t stride, uint64_t nr, uint32_t flags,
                 uint64_t chain_cap, uint64_t point_cap, int64_t* xy_out, uint32_t* row_out, int32_t* left_out, int32_t* right_out, Counts* counts,
                 uint64_t* stats) {
  memset(counts, 0, sizeof(Counts));
  if (stats) stats[0] = stats[1] = 0;
  if (flags & ~kDissolve) return 1;
  if (stride < 4 || stride % 4) return 1;
  if (nr > 0xFFFFFFFEull || n >= (1ull << 31) || (nr == 0 && n != 0)) return 1;
  const Out o{xy_out, row_out, left_out, right_out, chain_cap, point_cap};
  if (nr == 0) {
    if (o.row) o.row[0] = 0;
    return 0;
  }
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  for (uint64_t c = 0; c <= nr; c++) meta.bad = std::max(meta.bad, check_row(c, row, nr, n));
  for (uint64_t i = 0; i < 2 * n; i++) meta.bad = std::max(meta.bad, check_coordinate(xy[i]));
  if (n == 0) {
    if (meta.bad) return 1;
    if (o.row) o.row[0] = 0;
    return 0;
  }
  const bool bad = meta.bad != 0;
  const uint64_t n1 = n + 1, n2 = 2 * n, n21 = 2 * n + 1;
  int rounds = 1;
  while ((1ull << (rounds - 1)) < n2 && rounds < kMaxRounds) rounds++;
  // 1. the ring of every point slot; 2. canonical edges, the first sort
  std::vector<uint32_t> mark(n, 0), ring_at(n), dir(n), sv(n);
  std::vector<Seg> seg(n);
  if (!bad)
    for (uint64_t r = 0; r < nr; r++) ring_mark((uint32_t) r, row, mark.data());
  uint32_t running = 0;
  for (uint64_t i = 0; i < n; i++) ring_at[i] = running = std::max(running, mark[i]);
  for (uint64_t i = 0; i < n; i++) meta.counts.n_zero_edges += seg_of(i, bad, ring_at.data(), row, xy, seg.data(), dir.data()) == kZero && !bad;
  std::iota(sv.begin(), sv.end(), 0u);
  std::sort(sv.begin(), sv.end(), [&](uint32_t a, uint32_t b) { return seg_before(a, b, seg.data(), dir.data()); });
  // 3. unique edges, the kept ones numbered
  std::vector<uint32_t> head(n), gid(n), ghead(n), gconf(n, 0), keep(n1), eidx(n1);
  std::vector<int32_t> gleft(n, 0), gright(n, 0), eleft(n), eright(n);
  std::vector<Seg> E(n);
  for (uint64_t j = 0; j < n; j++) group_head(j, sv.data(), seg.data(), dir.data(), head.data());
  uint32_t acc = 0;
  for (uint64_t j = 0; j < n; j++) gid[j] = acc += head[j];
  for (uint64_t j = 0; j < n; j++)
    group_fill(j, sv.data(), dir.data(), head.data(), gid.data(), ring_at.data(), face, stride, ghead.data(), gleft.data(), gright.data(),
               gconf.data());
  meta.n_groups = gid[n - 1];
  for (uint64_t g = 0; g <= n; g++) {
    int what;
    group_keep(g, meta.n_groups, gleft.data(), gright.data(), gconf.data(), flags, keep.data(), &what);
    meta.counts.n_conflicts += what & 1;
    meta.counts.n_dissolved += (what >> 1) & 1;
  }
  acc = 0;
  for (uint64_t g = 0; g <= n; g++) {
    eidx[g] = acc;
    acc += keep[g];
  }
  for (uint64_t g = 0; g < meta.n_groups; g++)
    edge_emit(g, sv.data(), seg.data(), ghead.data(), gleft.data(), gright.data(), keep.data(), eidx.data(), E.data(), eleft.data(), eright.data());
  meta.counts.n_edges = eidx[n];
  const uint64_t ne = meta.counts.n_edges, nh = 2 * ne;
  // 4. half-edges by start point; 5. next
  std::vector<uint32_t> even(n), odd(n), S(n2), pos(n2), next(n2);
  for (uint64_t k = 0; k < n; k++) half_seed(k, ne, even.data(), odd.data());
  auto before = [&](uint32_t a, uint32_t b) { return half_before(a, b, E.data()); };
  std::sort(odd.begin(), odd.end(), before);
  if (!std::is_sorted(even.begin(), even.end(), before)) return 5;  // (cannot happen: lo is the first sort's first key)
  std::merge(even.begin(), even.end(), odd.begin(), odd.end(), S.begin(), before);
  for (uint64_t k = 0; k < nh; k++) half_pos(k, S.data(), pos.data());
  for (uint64_t h = 0; h < nh; h++) next[h] = next_of((uint32_t) h, nh, S.data(), pos.data(), E.data(), eleft.data(), eright.data());
  // 6. heads and leaders, then the closed walks opened and ranked
  std::vector<Walk> w[2] = {std::vector<Walk>(n2), std::vector<Walk>(n2)};
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 0)
      for (uint64_t h = 0; h < nh; h++) walk_init((uint32_t) h, next.data(), w[0].data(), w[1].data());
    else
      for (uint64_t h = 0; h < nh; h++) cut_init((uint32_t) h, w[meta.done[0] & 1].data(), next.data(), w[0].data(), w[1].data());
    for (int r = 0; r < rounds; r++) {
      if (!round_needed(meta.act[pass], r)) {
        if (!meta.done[pass]) meta.done[pass] = (uint32_t) r;
        continue;
      }
      for (uint64_t i = 0; i < nh; i++) meta.act[pass][r] += walk_round((uint32_t) i, w[r & 1].data(), w[(r + 1) & 1].data()) ? 1 : 0;
    }
    if (!meta.done[pass]) {
      meta.done[pass] = (uint32_t) rounds;
      if (meta.act[pass][rounds - 1]) meta.unfinished = 1;
    }
    if (stats) stats[pass] = meta.done[pass];
  }
  if (bad) return 1;
  if (meta.unfinished) return 5;
  const Walk* W = w[meta.done[1] & 1].data();
  // 7. chains
  std::vector<Slots> total(n21), base(n21);
  for (uint64_t h = 0; h <= n2; h++) meta.counts.n_closed += chain_total(h, nh, W, next.data(), total.data()) ? 1 : 0;
  Slots sum{0, 0};
  for (uint64_t h = 0; h <= n2; h++) {
    base[h] = sum;
    sum = Slots{sum.halves + total[h].halves, sum.points + total[h].points};
  }
  for (uint64_t h = 0; h <= nh; h++) chain_place(h, nh, W, base.data(), E.data(), eleft.data(), eright.data(), o, &meta);
  *counts = meta.counts;
  return counts->n_chains > chain_cap || counts->n_points > point_cap ? 3 : 0;
}

}  // extern "C"
