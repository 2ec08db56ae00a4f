// rj_snap.h -- cutting a chain map at its proper crossings too (rj_map_snap, include/rayjoin_amd.h; kernels in
// rj_snap.hip): rj_map_node (rj_node.h) plus one cut at the ROUNDED point of every kProper record.  rj_map_node leaves
// those records alone because their point is no integer; here the point is rounded to the nearest integer point, both
// edges are cut there, and the crossing becomes a shared vertex.  Moving a point can make new crossings (the edges bend by
// up to half a unit), so ONE call promises no planar map: a driver (ops.map_snap_rounds) repeats rj_map_crossings and this
// call until a check finds nothing -- snap rounding by iteration.  That the rounds end is measured, not
// proven: the call reports what it did and the check reports what is left.  Integers only, exact, and fully determined:
// no tuning choice below can change a result.
//
// INPUT   the map and the records exactly as rj_map_node takes them (rj_node.h INPUT), with the same checks and codes;
//         kDropLast means what node::kDropLast means.
// CUTS FROM kTouch AND kOverlap RECORDS   exactly rj_map_node's cut set (rj_node.h INSIDE, CUTS): four tests per record,
//         a cut exists only where the geometry holds, at most two of the four hold.
// CUTS FROM kProper RECORDS   for a record (e, f), e < f, with A, B the points of e and C, D the points of f, r = B - A,
//         s = D - C:  den = r x s, tn = (C - A) x s, un = (C - A) x r -- int128 cross products, all below 2^95 --, all three
//         negated when den < 0.  If den == 0 or not 0 < tn < den or not 0 < un < den the record is STALE: it does not fit
//         the geometry, cuts nothing and is counted in n_stale.  Otherwise the crossing point is A + r tn / den and
//             q = A + (rnd(r.x tn / den), rnd(r.y tn / den)),   rnd(v) = floor(v + 1/2):
//         halves go toward +infinity whatever the direction of the edge.  q is always computed from the lower-numbered
//         edge, so both edges get the same point.  q joins C(e) unless it equals A or B and joins C(f) unless it equals C
//         or D; each such drop counts once in n_at_end (the other edge is still cut there: the near miss becomes a shared
//         vertex).  n_exact: the records that are not stale whose point needed no rounding (both remainders 0).  q lies
//         in the closed boxes of both edges (the crossing point does, and a box's corners are integers): the output stays
//         in the coordinate range.  A record yields at most two cuts whatever its kind: a call has at most 2 n candidates.
// WIDTH   r.x tn reaches 2^142.  With |r.x| = h 2^24 + l (h < 2^23, l < 2^24):  h tn < 2^118 divided by den gives q1, r1;
//         r1 2^24 + l tn < 2^120 divided by den gives q2, R; the quotient is Q = q1 2^24 + q2 and the remainder R.  Both
//         partial quotients are below 2^26 (tn < den: q1 <= h, q2 < 2^24 + l), so each division is 26 steps of compare,
//         subtract and shift on unsigned 128-bit numbers (den << 25 < 2^120): no 128-bit division routine, no floating
//         point.  r.x >= 0: the rounded value is Q + (2 R >= den); r.x < 0: -Q - (2 R > den).
// ORDER   the major axis of an edge is x when |dx| >= |dy|, else y.  The cuts of an edge ascend by the pair
//         (|q.major - a.major|, |q.minor - a.minor|): a monotone function of the exact parameter along the edge both for
//         points on the segment and for rounded crossing points (rounding is monotone, and q stays in the edge's box, so
//         neither difference changes sign).  Equal pairs are equal points, which appear once.  For points on the
//         segment this is the order of rj_map_node.
// OUTPUT  the layout of rj_map_node (rj_node.h OUTPUT): out_xy, out_row[nc + 1], origin[k], all or nothing; chains, their
//         number and their order do not change.  Counts: node::Counts' eight fields with the same meaning (n_cuts: the
//         inserted points of all kinds; n_proper: all kProper records, stale ones included) and n_exact, n_at_end,
//         n_stale.  On records without a kProper kind the output arrays and the eight shared counts equal rj_map_node's
//         bit for bit.
//
// Every step is one function per element that rj_snap.hip / rj_cut_pipeline.h run as a grid-stride kernel and
// tests/hosttwin/snap_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   node::check_chain / node::check_record and the map check of rj_crossings.h   the input check, as rj_map_node's
//   touch_cuts    per record of kind kTouch / kOverlap: node's four tests, the cuts (edge, key, point) of those that hold
//   proper_cuts   per record of kind kProper: the stale test, the rounded point, the cuts that are not at an end
//   (one merge sort of the candidates by cut_before: (edge, major offset, minor offset); unused slots, all ones, go last)
//   cut_head      per sorted position: is it the first of its run of equal keys -- a kept cut
//   run_first / run_last   per sorted position: does its edge's run start / end here (first[e], last[e] as in rj_node.h)
//   node::point_chain / point_slot / row_slot / cut_slot / totals   the slots, unchanged
// No stage is serial in the number of cuts on one edge.
//
// Scratch per call: 144 bytes per record (2 candidates of 32 bytes, twice: unsorted and sorted; 2 flags and 2 numbers of
// 4 bytes), 12 bytes per edge (first, last - first, prefix) plus the sort's and the scans' temporary storage; allocated
// per call and freed.
#pragma once
#include <stdint.h>

#include "rj_node.h"

namespace rj {
namespace snap {

using crossings::Edge;
using node::Record;

typedef unsigned __int128 u128;

constexpr uint32_t kDropLast = node::kDropLast;  // RJ_SNAP_DROP_LAST
constexpr uint32_t kNoEdge = node::kNoEdge;      // an unused candidate slot

// a cut: the point, and the sort key (edge, major offset, minor offset) in two words -- both offsets are below 2^47
struct alignas(16) Cut {
  uint64_t hi;  // (edge << 32) | (major offset >> 15)
  uint64_t lo;  // ((major offset & 0x7FFF) << 47) | minor offset
  int64_t qx, qy;
};
struct Counts {  // rj_snap_counts
  uint64_t n_points, n_edges, n_cuts, n_cut_edges, n_max_cuts, n_used, n_proper, n_equal;  // as node::Counts
  uint64_t n_exact, n_at_end, n_stale;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;   // the input check's status (the codes of rj_node.h); not 0: nothing is read further
  uint32_t emit;  // 1: the output fits and is written
  uint64_t n_cand;
  Counts counts;
};

// ---- 1. candidates ---------------------------------------------------------------------------------------
RJ_RHD uint64_t abs_diff(int64_t a, int64_t b) { return (uint64_t) (a < b ? b - a : a - b); }
RJ_RHD uint32_t cut_edge(const Cut& c) { return (uint32_t) (c.hi >> 32); }
// the cut of edge number e (its points: E) at q: q on the segment or a rounded crossing point in E's closed box
RJ_RHD Cut cut_at(uint32_t e, const Edge& E, int64_t qx, int64_t qy) {
  const uint64_t dx = abs_diff(E.bx, E.ax), dy = abs_diff(E.by, E.ay), ox = abs_diff(qx, E.ax), oy = abs_diff(qy, E.ay);
  const uint64_t major = dx >= dy ? ox : oy, minor = dx >= dy ? oy : ox;
  return Cut{((uint64_t) e << 32) | (major >> 15), ((major & 0x7FFFull) << 47) | minor, qx, qy};
}
// a when take, else b, field by field (values, no addresses: on the device the cuts of a record stay in registers)
RJ_RHD Cut pick(bool take, const Cut& a, const Cut& b) { return Cut{take ? a.hi : b.hi, take ? a.lo : b.lo, take ? a.qx : b.qx, take ? a.qy : b.qy}; }
// a record of kind kTouch / kOverlap over the edges e < f: the four tests in rj_node.h's order (f.a inside e, f.b inside
// e, e.a inside f, e.b inside f) -> the number of tests that hold, at most 2 (rj_node.h CUTS); *c0, *c1: the cuts of
// the first and of the second that holds
RJ_RHD int touch_cuts(uint32_t e, uint32_t f, const Edge& E, const Edge& F, Cut* c0, Cut* c1) {
  const bool h0 = node::inside(E, F.ax, F.ay), h1 = node::inside(E, F.bx, F.by), h2 = node::inside(F, E.ax, E.ay), h3 = node::inside(F, E.bx, E.by);
  const Cut k0 = cut_at(e, E, F.ax, F.ay), k1 = cut_at(e, E, F.bx, F.by), k2 = cut_at(f, F, E.ax, E.ay), k3 = cut_at(f, F, E.bx, E.by);
  const Cut from2 = pick(h2, k2, k3), from1 = pick(h1, k1, from2);  // the first that holds among the tests 2.., 1..
  *c0 = pick(h0, k0, from1);
  *c1 = pick(h0, from1, pick(h1, from2, k3));
  const int n = (int) h0 + (int) h1 + (int) h2 + (int) h3;
  return n < 2 ? n : 2;
}
// floor(num / den) for a quotient below 2^26 and den < 2^95; *rem = the remainder
RJ_RHD uint64_t div_small(u128 num, u128 den, u128* rem) {
  uint64_t q = 0;
  for (int b = 25; b >= 0; b--) {
    const u128 d = den << b;
    if (num >= d) {
      num -= d;
      q |= 1ull << b;
    }
  }
  *rem = num;
  return q;
}
// rnd(d tn / den) for |d| < 2^47 and 0 < tn < den < 2^95; *exact = the remainder is 0
RJ_RHD int64_t rounded_part(int64_t d, u128 tn, u128 den, bool* exact) {
  const uint64_t m = (uint64_t) (d < 0 ? -d : d), h = m >> 24, l = m & 0xFFFFFFull;
  u128 r1, R;
  const uint64_t q1 = div_small((u128) h * tn, den, &r1);
  const uint64_t q2 = div_small((r1 << 24) + (u128) l * tn, den, &R);
  const int64_t Q = (int64_t) ((q1 << 24) + q2);
  *exact = R == 0;
  return d >= 0 ? Q + (2 * R >= den ? 1 : 0) : -Q - (2 * R > den ? 1 : 0);
}
struct Proper {
  bool stale, exact;
  int64_t qx, qy;
};
// the rounded crossing point of E and F, computed from E
RJ_RHD Proper proper_point(const Edge& E, const Edge& F) {
  const int64_t rx = E.bx - E.ax, ry = E.by - E.ay, sx = F.bx - F.ax, sy = F.by - F.ay, wx = F.ax - E.ax, wy = F.ay - E.ay;
  __int128 den = (__int128) rx * sy - (__int128) ry * sx, tn = (__int128) wx * sy - (__int128) wy * sx, un = (__int128) wx * ry - (__int128) wy * rx;
  if (den < 0) den = -den, tn = -tn, un = -un;
  Proper p{true, false, 0, 0};
  if (den == 0 || tn <= 0 || tn >= den || un <= 0 || un >= den) return p;
  bool ex, ey;
  p.qx = E.ax + rounded_part(rx, (u128) tn, (u128) den, &ex);
  p.qy = E.ay + rounded_part(ry, (u128) tn, (u128) den, &ey);
  p.stale = false;
  p.exact = ex && ey;
  return p;
}
// a record of kind kProper over the edges e < f with its point p -> the number of cuts (*c0, then *c1); *at_end: the
// edges (0..2) left uncut because the point is one of their ends
RJ_RHD int proper_cuts(uint32_t e, uint32_t f, const Edge& E, const Edge& F, const Proper& p, Cut* c0, Cut* c1, uint32_t* at_end) {
  const bool end_e = crossings::is_end(E, p.qx, p.qy), end_f = crossings::is_end(F, p.qx, p.qy);
  const Cut on_e = cut_at(e, E, p.qx, p.qy), on_f = cut_at(f, F, p.qx, p.qy);
  *c0 = pick(!end_e, on_e, on_f);
  *c1 = on_f;
  *at_end = p.stale ? 0 : (uint32_t) end_e + (uint32_t) end_f;
  return p.stale ? 0 : (int) !end_e + (int) !end_f;
}

// ---- 2. the sort, the kept cuts ----------------------------------------------------------------------------
RJ_RHD bool cut_before(const Cut& a, const Cut& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
// sorted position i of n: a cut that is the first of its run of equal (edge, offsets)
RJ_RHD bool cut_head(uint64_t i, const Cut* s) { return cut_edge(s[i]) != kNoEdge && (i == 0 || s[i - 1].hi != s[i].hi || s[i - 1].lo != s[i].lo); }
// does the run of one edge start / end at sorted position i (a cut) of n
RJ_RHD bool run_first(uint64_t i, const Cut* s) { return i == 0 || cut_edge(s[i - 1]) != cut_edge(s[i]); }
RJ_RHD bool run_last(uint64_t i, uint64_t n, const Cut* s) { return i + 1 == n || cut_edge(s[i + 1]) != cut_edge(s[i]); }

// ---- 3. slots: node::point_chain, point_slot, row_slot, cut_slot ---------------------------------------------
// the counts behind the scans (node::totals on the eight shared fields)
RJ_RHD void totals(uint64_t np, uint64_t nc, uint64_t n_cuts, uint32_t flags, uint64_t capacity, Counts* counts, uint32_t* emit) {
  node::Counts shared{};
  node::totals(np, nc, n_cuts, flags, capacity, &shared, emit);
  counts->n_cuts = shared.n_cuts;
  counts->n_edges = shared.n_edges;
  counts->n_points = shared.n_points;
}

}  // namespace snap

#if defined(__HIPCC__)
// what a call reports besides its counts
struct SnapReport : StageMs {};  // the check; the candidates; the sort and the kept cuts; the cuts per edge and their scan; the two scatters; all
// rj_map_snap behind its argument checks, on stream st: *result = the device's Meta (counts, the input check's status,
// whether the output was written).  Allocates and frees its scratch; synchronises the stream once, at the end.
hipError_t map_snap_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec, uint64_t n_rec,
                           uint32_t flags, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, snap::Meta* result,
                           SnapReport* report);
#endif

}  // namespace rj
