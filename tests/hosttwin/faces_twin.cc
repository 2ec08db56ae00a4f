// Host twin of rj_faces.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_faces.h (and those of rj_rings.h and rj_polygons.h that the device runs for it) as plain loops, in
// the device's stage order, with std::sort / plain prefix sums where the device calls rocPRIM.  tests/test_faces.py holds it
// equal to the plain-Python definition (tests/faces_ref.py); tests/test_gpu_faces.py holds the device equal to it where the
// map is too large for the Python loop.  With -DFACES_TWIN_MAIN it is a stand-alone program (host sanitizers).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

#include "rj_faces.h"

using namespace rj::faces;
namespace R = rj::rings;
namespace P = rj::polygons;

namespace {

struct Solo {  // the reduction of a group of one lane
  uint32_t operator()(uint32_t best) const { return best; }
};

// the ring stages without labels and without points -> false: a round budget ran out
bool label_free_rings(const int64_t* xy, const uint32_t* row, uint32_t nc, std::vector<Ring>& rings, std::vector<uint32_t>& ring_first,
                      std::vector<uint32_t>& ring_half, R::Meta& meta) {
  const uint32_t ni = 2 * nc;
  const size_t n1 = (size_t) ni + 1;
  int rounds = 1;
  while ((1ull << (rounds - 1)) < ni && rounds < R::kMaxRounds) rounds++;
  memset(&meta, 0, sizeof(meta));
  std::vector<R::Inc> inc(ni);
  for (uint32_t h = 0; h < ni; h++) meta.counts.n_skipped += R::incidence(h, xy, row, false, inc.data()) && !(h & 1) ? 1 : 0;
  std::vector<uint32_t> sv(ni);
  std::iota(sv.begin(), sv.end(), 0u);
  std::sort(sv.begin(), sv.end(), [&](uint32_t a, uint32_t b) { return R::inc_before(a, b, inc.data()); });
  std::vector<uint32_t> pos(ni), head(ni), begin(ni), next(ni);
  for (uint32_t j = 0; j < ni; j++) R::junction_head(j, sv.data(), inc.data(), pos.data(), head.data());
  uint32_t running = 0;
  for (uint32_t j = 0; j < ni; j++) begin[j] = running = std::max(running, head[j]);
  uint32_t* last_of = head.data();
  for (uint32_t j = 0; j < ni; j++) R::junction_last(j, ni, sv.data(), inc.data(), begin.data(), last_of);
  std::vector<R::Link> lk[2] = {std::vector<R::Link>(ni), std::vector<R::Link>(ni)};
  for (uint32_t h = 0; h < ni; h++) R::next_of(h, sv.data(), inc.data(), pos.data(), begin.data(), last_of, next.data(), lk[0].data(), lk[1].data());
  auto finish = [&](uint32_t* done, const uint32_t* count) {
    if (!*done) {
      *done = (uint32_t) rounds;
      if (count[rounds - 1]) meta.unfinished = 1;
    }
  };
  for (int r = 0; r < rounds; r++) {
    if (!R::round_needed(meta.changed, r)) {
      if (!meta.cyc_done) meta.cyc_done = (uint32_t) r;
      continue;
    }
    for (uint32_t i = 0; i < ni; i++) meta.changed[r] += R::cyc_round(i, lk[r & 1].data(), lk[(r + 1) & 1].data()) ? 1 : 0;
  }
  finish(&meta.cyc_done, meta.changed);
  const R::Link* F = lk[meta.cyc_done & 1].data();
  std::vector<R::Node> nd[2] = {std::vector<R::Node>(ni), std::vector<R::Node>(ni)};
  for (uint32_t h = 0; h < ni; h++) R::rank_init(h, F, next.data(), inc.data(), row, nd[0].data(), nd[1].data());
  for (int r = 0; r < rounds; r++) {
    if (!R::round_needed(meta.act, r)) {
      if (!meta.rank_done) meta.rank_done = (uint32_t) r;
      continue;
    }
    for (uint32_t i = 0; i < ni; i++) meta.act[r] += R::rank_round(i, nd[r & 1].data(), nd[(r + 1) & 1].data()) ? 1 : 0;
  }
  finish(&meta.rank_done, meta.act);
  const R::Node* N = nd[meta.rank_done & 1].data();
  if (meta.unfinished) return false;
  std::vector<uint64_t> skeys(ni);
  for (uint32_t h = 0; h < ni; h++) skeys[h] = R::ring_key(h, F, inc.data(), nullptr, nullptr, 0);
  std::sort(skeys.begin(), skeys.end());
  std::vector<uint32_t> ring_of(ni, R::kNone), mixed(n1, 0);
  std::vector<R::Slots> total(n1), base(n1);
  for (size_t r = 0; r < n1; r++) R::ring_slot((uint32_t) r, ni, skeys.data(), N, ring_of.data(), total.data(), &meta);
  R::Slots acc{0, 0};
  for (size_t r = 0; r < n1; r++) {
    base[r] = acc;
    acc = R::Slots{acc.halves + total[r].halves, acc.points + total[r].points};
  }
  rings.assign(ni, Ring{});
  ring_first.assign(n1, 0);
  ring_half.assign(ni, 0);
  const R::Out o{rings.data(), ring_first.data(), ring_half.data(), nullptr, nullptr, ni, ni, 0};
  std::vector<U128> cross_at(n1, U128{0, 0}), xbase(n1);
  for (uint32_t h = 0; h < ni; h++) {
    uint64_t slot = 0, pslot = 0;
    const uint32_t r = R::half_slots(h, F, inc.data(), N, ring_of.data(), base.data(), &slot, &pslot);
    if (r == R::kNone) continue;
    const U128 sum = R::half_points(h, 0, 1, xy, row, pslot, nullptr, 0);
    R::half_store(h, r, slot, ni, sum, skeys.data(), nullptr, nullptr, cross_at.data(), mixed.data(), o.ring_half, o.half_cap);
  }
  U128 xacc{0, 0};
  for (size_t s = 0; s < n1; s++) {
    xbase[s] = xacc;
    xacc = R::add(xacc, cross_at[s]);
  }
  for (uint64_t r = 0; r <= meta.counts.n_rings; r++) R::ring_emit((uint32_t) r, skeys.data(), base.data(), xbase.data(), mixed.data(), o, &meta);
  return true;
}

}  // namespace

extern "C" {

// -> 0, 1 (flags, a malformed map, one label array alone), 3 (faces given and n_faces > face_cap: *counts holds the true counts,
// left / right are complete) or 5 (round budget), the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW, RJ_E_INTERNAL.  faces_out
// may be null.  forced_shift: 0 or 15..47.  stats: the shift, the registrations, the ceiling edges, the ray tests, the cells
// visited, the jumping rounds run.  above_out (or null): per ring the ring above it, kNone without one or for a shell.
int faces_twin(const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc64, const int32_t* in_left, const int32_t* in_right, uint32_t flags,
               int forced_shift, uint64_t face_cap, int32_t* left, int32_t* right, Face* faces_out, Counts* counts, uint64_t* stats,
               uint32_t* above_out) {
  memset(counts, 0, sizeof(Counts));
  if (stats) memset(stats, 0, 6 * sizeof(uint64_t));
  if (flags || !in_left != !in_right) return 1;
  if (nc64 >= (1ull << 31) || np >= (1ull << 32) || nc64 > np || 2 * (np - nc64) >= (1ull << 32) || (nc64 == 0 && np != 0)) return 1;
  if (nc64 == 0) return 0;
  uint32_t bad = 0;
  for (uint64_t c = 0; c <= nc64; c++) bad = std::max(bad, R::check_row(c, row, nc64, np));
  for (uint64_t i = 0; i < 2 * np; i++) bad = std::max(bad, R::check_coordinate(xy[i]));
  if (bad) return 1;
  const uint32_t nc = (uint32_t) nc64, ni = 2 * nc;
  const size_t n1 = (size_t) ni + 1;
  int rounds = 1;
  while ((1ull << (rounds - 1)) < ni && rounds < kMaxRounds) rounds++;
  // 1. the rings
  std::vector<Ring> rings;
  std::vector<uint32_t> ring_first, ring_half;
  R::Meta rmeta;
  if (!label_free_rings(xy, row, nc, rings, ring_first, ring_half, rmeta)) return 5;
  const uint64_t nr = rmeta.counts.n_rings, n_halves = rmeta.counts.n_halves;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  P::Meta pmeta;
  memset(&pmeta, 0, sizeof(pmeta));
  // 2. tops and kinds
  std::vector<uint8_t> islast(np, 0);
  std::vector<Top> chain_top(nc);
  for (uint32_t c = 0; c < nc; c++) {
    P::ring_top(c, 0, 1, row, xy, &chain_top[c]);
    last_mark(c, row, islast.data());
  }
  std::vector<uint32_t> ring_of_half(ni, kNone), kind(ni, 0);
  std::vector<SegTop> seg(ni), segs(ni);
  memset(seg.data(), 0xFF, sizeof(SegTop) * ni);
  for (uint64_t s = 0; s < n_halves; s++) slot_seg(s, ring_first.data(), ring_half.data(), nr, chain_top.data(), ring_of_half.data(), seg.data());
  for (uint32_t s = 0; s < ni; s++) segs[s] = s ? seg_max(segs[s - 1], seg[s]) : seg[s];
  for (uint64_t r = 0; r < nr; r++) kind[r] = ring_kind(rings[r]);
  // 3. the grid
  for (uint64_t i = 0; i < np; i++) meta.n_ceil += edge_scan(i, islast.data(), xy, meta.regs, &meta.extent_lo, &meta.extent_hi) ? 1 : 0;
  pick_shift(&meta, forced_shift);
  const int shift = (int) meta.shift;
  const uint64_t cap = reg_cap(np - nc64);
  std::vector<uint64_t> off(np + 1);
  uint64_t acc = 0;
  for (uint64_t i = 0; i <= np; i++) {
    off[i] = acc;
    if (i < np) acc += reg_count_at(i, islast.data(), xy, shift);
  }
  if (acc != meta.n_regs || acc > cap) return 5;  // (cannot happen)
  std::vector<std::pair<uint64_t, uint32_t>> entries(meta.n_regs);
  for (uint64_t r = 0; r < meta.n_regs; r++) reg_at(r, off.data(), np, xy, shift, &entries[r].first, &entries[r].second);
  std::stable_sort(entries.begin(), entries.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  std::vector<uint64_t> keys(meta.n_regs + 1);
  std::vector<uint32_t> vals(meta.n_regs + 1);
  for (uint64_t r = 0; r < meta.n_regs; r++) {
    keys[r] = entries[r].first;
    vals[r] = entries[r].second;
  }
  // 4. the rays; 5. parents
  std::vector<Jump> jp[2] = {std::vector<Jump>(ni), std::vector<Jump>(ni)};
  for (uint64_t r = 0; r < nr; r++) {
    uint32_t best = kNone;
    if (kind[r] == P::kKindHole) {
      const Top p = segs[ring_first[r + 1] - 1].top;
      best = ray_walk(0, 1, p, keys.data(), vals.data(), meta.n_regs, xy, shift, Solo(), &meta.ray_tests, &meta.cells);
    }
    above_init((uint32_t) r, kind[r], best, row, nc64, xy, ring_of_half.data(), jp[0].data(), jp[1].data());
    if (above_out) above_out[r] = kind[r] == P::kKindHole && best != kNone ? jp[0][r].to : kNone;
  }
  for (int r = 0; r < rounds; r++) {
    if (!P::round_needed(pmeta.act, r)) {
      if (!pmeta.jump_done) pmeta.jump_done = (uint32_t) r;
      continue;
    }
    for (uint64_t i = 0; i < nr; i++) pmeta.act[r] += P::jump_round((uint32_t) i, jp[r & 1].data(), jp[(r + 1) & 1].data()) ? 1 : 0;
  }
  if (!pmeta.jump_done) {
    pmeta.jump_done = (uint32_t) rounds;
    if (pmeta.act[rounds - 1]) pmeta.unfinished = 1;
  }
  if (stats) {
    stats[0] = meta.shift;
    stats[1] = meta.n_regs;
    stats[2] = meta.n_ceil;
    stats[3] = meta.ray_tests;
    stats[4] = meta.cells;
    stats[5] = pmeta.jump_done;
  }
  if (pmeta.unfinished) return 5;
  const Jump* J = jp[pmeta.jump_done & 1].data();
  // 6. faces
  std::vector<uint64_t> skeys(ni, P::kNoKey);
  for (uint64_t r = 0; r < nr; r++) {
    int what = 0;
    skeys[r] = P::poly_key((uint32_t) r, kind.data(), J, nullptr, &what);
    meta.counts.n_holes += what == 1;
    meta.counts.n_outer += what == 2;
  }
  std::sort(skeys.begin(), skeys.end());
  std::vector<uint32_t> start(n1), pid(n1), first(n1, 0), face_of_ring(ni, 0);
  std::vector<U128> area_at(n1), xbase(n1);
  for (size_t j = 0; j < n1; j++) P::member_mark(j, ni, skeys.data(), rings.data(), start.data(), area_at.data(), &pmeta);
  uint32_t pacc = 0;
  for (size_t j = 0; j < n1; j++) {
    pid[j] = pacc;
    pacc += start[j];
  }
  const P::Out none{nullptr, nullptr, nullptr, nullptr, 0, 0};
  for (size_t j = 0; j < n1; j++) {
    P::member_place(j, ni, skeys.data(), start.data(), pid.data(), first.data(), none, &pmeta);
    if (j < ni) face_number(j, skeys.data(), start.data(), pid.data(), face_of_ring.data());
  }
  U128 xacc{0, 0};
  for (size_t j = 0; j < n1; j++) {
    xbase[j] = xacc;
    xacc = R::add(xacc, area_at[j]);
  }
  if (faces_out)
    for (uint64_t k = 0; k < pmeta.counts.n_polygons; k++)
      face_emit(k, skeys.data(), first.data(), xbase.data(), rings.data(), in_left, in_right, faces_out, face_cap);
  for (uint32_t h = 0; h < ni; h++) {
    const uint32_t what = half_face(h, ring_of_half.data(), J, face_of_ring.data(), rings.data(), in_left, in_right, left, right);
    meta.counts.n_dangling += what & 1;
    meta.counts.n_conflicts += what >> 1;
  }
  meta.counts.n_faces = pmeta.counts.n_polygons;
  meta.counts.n_rings = nr;
  meta.counts.n_skipped = rmeta.counts.n_skipped;
  *counts = meta.counts;
  return faces_out && counts->n_faces > face_cap ? 3 : 0;
}

}  // extern "C"

#ifdef FACES_TWIN_MAIN
// a square in a square, a dangle, an isolated segment and a one-point chain: face 1 between the squares (area2 200 - 32), face 2
// inside the inner one; the same answer at every shift
int main() {
  const int64_t xy[] = {0, 0, 10, 0, 10, 10, 0, 10, 0, 0,  // chain 0: the outer square, counter-clockwise
                        2, 2, 2, 6, 6, 6, 6, 2, 2, 2,      // chain 1: the inner square, clockwise
                        0, 0, 1, 1,                        // chain 2: a dangle from the outer square's first point into face 1
                        3, 3, 4, 4,                        // chain 3: an isolated segment inside the inner square
                        7, 7};                             // chain 4: one point
  const uint32_t row[] = {0, 5, 10, 12, 14, 15};
  int32_t left[5], right[5];
  Face faces[4];
  Counts c;
  uint64_t stats[6];
  for (int shift : {0, 15, 47}) {
    const int rc = faces_twin(xy, 15, row, 5, nullptr, nullptr, 0, shift, 4, left, right, faces, &c, stats, nullptr);
    const int32_t want_left[5] = {1, 1, 1, 2, 0}, want_right[5] = {0, 2, 1, 2, 0};
    bool ok = rc == 0 && c.n_faces == 2 && c.n_rings == 5 && c.n_holes == 2 && c.n_outer == 1 && c.n_skipped == 1 && c.n_dangling == 2;
    for (int k = 0; k < 5; k++) ok = ok && left[k] == want_left[k] && right[k] == want_right[k];
    ok = ok && faces[0].area2_lo == 200 - 32 && faces[0].n_holes == 1 && faces[1].area2_lo == 32 && faces[1].n_holes == 1;
    if (!ok) {
      printf("faces_twin: wrong answer at shift %d (rc %d, %llu faces)\n", shift, rc, (unsigned long long) c.n_faces);
      printf("  rings %llu holes %llu outer %llu skipped %llu dangling %llu\n", (unsigned long long) c.n_rings, (unsigned long long) c.n_holes,
             (unsigned long long) c.n_outer, (unsigned long long) c.n_skipped, (unsigned long long) c.n_dangling);
      for (int k = 0; k < 5; k++) printf("  chain %d: left %d right %d\n", k, left[k], right[k]);
      for (int k = 0; k < 2; k++) printf("  face %d: holes %u area2 %llu\n", k + 1, faces[k].n_holes, (unsigned long long) faces[k].area2_lo);
      return 1;
    }
  }
  printf("faces_twin ok\n");
  return 0;
}
#endif
