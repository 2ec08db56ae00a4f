// Host twin of rj_rings.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_rings.h run as plain loops, in the device's stage order, with std::sort / plain prefix sums where
// the device calls rocPRIM.  tests/test_rings.py holds it equal to the plain-Python definition (tests/rings_ref.py);
// tests/test_gpu_rings.py holds the device equal to it where the map is too large for the Python walk.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_rings.h"

using namespace rj::rings;

extern "C" {

// -> 0, 1 (unknown flags, a malformed map), 3 (a count exceeds its capacity: *counts holds the true counts) or 5 (round budget), the
// values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  stats[0] / stats[1]: the doubling / ranking rounds run.
int rings_twin(const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc64, uint32_t flags,
               uint64_t ring_cap, uint64_t half_cap, uint64_t point_cap, Ring* rings_out, uint32_t* ring_first, uint32_t* ring_half,
               uint32_t* ring_row, int64_t* ring_xy, Counts* counts, uint64_t* stats) {
  memset(counts, 0, sizeof(Counts));
  if (stats) stats[0] = stats[1] = 0;
  if (flags & ~(kSkipFace0 | kNoPoints)) return 1;
  Out o{rings_out, ring_first, ring_half, ring_row, ring_xy, ring_cap, half_cap, point_cap};
  if (flags & kNoPoints) {
    o.ring_row = nullptr;
    o.ring_xy = nullptr;
    o.point_cap = 0;
  }
  if (nc64 == 0) {
    if (o.ring_first) o.ring_first[0] = 0;
    if (o.ring_row) o.ring_row[0] = 0;
    return 0;
  }
  uint32_t bad = 0;
  for (uint64_t c = 0; c <= nc64; c++) bad = std::max(bad, check_row(c, row, nc64, np));
  for (uint64_t i = 0; i < 2 * np; i++) bad = std::max(bad, check_coordinate(xy[i]));
  if (bad) return 1;
  const uint32_t nc = (uint32_t) nc64, ni = 2 * nc;
  const size_t n1 = (size_t) ni + 1;
  int rounds = 1;
  while ((1ull << (rounds - 1)) < ni && rounds < kMaxRounds) rounds++;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. incidences, the one sort
  std::vector<Inc> inc(ni);
  for (uint32_t h = 0; h < ni; h++) meta.counts.n_skipped += incidence(h, xy, row, false, inc.data()) && !(h & 1) ? 1 : 0;
  std::vector<uint32_t> sv(ni);
  std::iota(sv.begin(), sv.end(), 0u);
  std::sort(sv.begin(), sv.end(), [&](uint32_t a, uint32_t b) { return inc_before(a, b, inc.data()); });
  // 2. junctions; 3. next
  std::vector<uint32_t> pos(ni), head(ni), begin(ni), next(ni);
  for (uint32_t j = 0; j < ni; j++) junction_head(j, sv.data(), inc.data(), pos.data(), head.data());
  uint32_t running = 0;
  for (uint32_t j = 0; j < ni; j++) begin[j] = running = std::max(running, head[j]);
  uint32_t* last_of = head.data();  // (head[] is dead behind its scan)
  for (uint32_t j = 0; j < ni; j++) junction_last(j, ni, sv.data(), inc.data(), begin.data(), last_of);
  std::vector<Link> lk[2] = {std::vector<Link>(ni), std::vector<Link>(ni)};
  for (uint32_t h = 0; h < ni; h++) next_of(h, sv.data(), inc.data(), pos.data(), begin.data(), last_of, next.data(), lk[0].data(), lk[1].data());
  auto finish = [&](uint32_t* done, const uint32_t* count) {
    if (!*done) {
      *done = (uint32_t) rounds;
      if (count[rounds - 1]) meta.unfinished = 1;
    }
  };
  for (int r = 0; r < rounds; r++) {
    if (!round_needed(meta.changed, r)) {
      if (!meta.cyc_done) meta.cyc_done = (uint32_t) r;
      continue;
    }
    for (uint32_t i = 0; i < ni; i++) meta.changed[r] += cyc_round(i, lk[r & 1].data(), lk[(r + 1) & 1].data()) ? 1 : 0;
  }
  finish(&meta.cyc_done, meta.changed);
  const Link* F = lk[meta.cyc_done & 1].data();
  // 4. ranking
  std::vector<Node> nd[2] = {std::vector<Node>(ni), std::vector<Node>(ni)};
  for (uint32_t h = 0; h < ni; h++) rank_init(h, F, next.data(), inc.data(), row, nd[0].data(), nd[1].data());
  for (int r = 0; r < rounds; r++) {
    if (!round_needed(meta.act, r)) {
      if (!meta.rank_done) meta.rank_done = (uint32_t) r;
      continue;
    }
    for (uint32_t i = 0; i < ni; i++) meta.act[r] += rank_round(i, nd[r & 1].data(), nd[(r + 1) & 1].data()) ? 1 : 0;
  }
  finish(&meta.rank_done, meta.act);
  const Node* N = nd[meta.rank_done & 1].data();
  if (stats) {
    stats[0] = meta.cyc_done;
    stats[1] = meta.rank_done;
  }
  if (meta.unfinished) return 5;
  // 5. the rings in their order, the two CSRs
  std::vector<uint64_t> skeys(ni);
  for (uint32_t h = 0; h < ni; h++) skeys[h] = ring_key(h, F, inc.data(), left, right, flags);
  std::sort(skeys.begin(), skeys.end());
  std::vector<uint32_t> ring_of(ni, kNone), mixed(n1, 0);
  std::vector<Slots> total(n1), base(n1);
  for (size_t r = 0; r < n1; r++) ring_slot((uint32_t) r, ni, skeys.data(), N, ring_of.data(), total.data(), &meta);
  Slots acc{0, 0};
  for (size_t r = 0; r < n1; r++) {
    base[r] = acc;
    acc = Slots{acc.halves + total[r].halves, acc.points + total[r].points};
  }
  // 6. half-chains and points to their slots; 7. areas and records
  std::vector<U128> cross_at(n1, U128{0, 0}), xbase(n1);
  for (uint32_t h = 0; h < ni; h++) {
    uint64_t slot = 0, pslot = 0;
    const uint32_t r = half_slots(h, F, inc.data(), N, ring_of.data(), base.data(), &slot, &pslot);
    if (r == kNone) continue;
    const U128 sum = half_points(h, 0, 1, xy, row, pslot, o.ring_xy, o.point_cap);
    half_store(h, r, slot, ni, sum, skeys.data(), left, right, cross_at.data(), mixed.data(), o.ring_half, o.half_cap);
  }
  U128 xacc{0, 0};
  for (size_t s = 0; s < n1; s++) {
    xbase[s] = xacc;
    xacc = add(xacc, cross_at[s]);
  }
  for (uint64_t r = 0; r <= meta.counts.n_rings; r++)
    meta.counts.n_mixed += ring_emit((uint32_t) r, skeys.data(), base.data(), xbase.data(), mixed.data(), o, &meta) ? 1 : 0;
  *counts = meta.counts;
  const bool over = counts->n_rings > ring_cap || counts->n_halves > half_cap || (!(flags & kNoPoints) && counts->n_points > point_cap);
  return over ? 3 : 0;
}

}  // extern "C"
