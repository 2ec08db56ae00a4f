// rj_window.h -- the edges of a map that meet each rectangle (rj_window_query, include/rayjoin_amd.h; the device work in
// rj_window.hip): the bounding-box select, sindex.query(box), the linework of a tile, "which chains does this extent
// touch".  The fifth query over the index of rj_build_lbvh and the second whose result is a CSR.  Integers only, exact, and
// fully determined.
//
// DEFINITION   A window is four int64 (x0, y0, x1, y1) in the scaled coordinates of the maps: the CLOSED rectangle
//         [x0, x1] x [y0, y1].  x0 > x1 or y0 > y1 is the empty window: it lists nothing and is no error.  A point (x0 == x1,
//         y0 == y1) and an axis-parallel segment are windows like any other.
//         Edge e = (A, B) belongs to window w iff the closed segment and the closed rectangle share a point, that is iff
//           (1) the bounding box of (A, B) overlaps w, closed on both sides, and
//           (2) the four corners C_k of w are not all strictly on one side of the line through A and B: with
//               s_k = sign((B - A) x (C_k - A)), the edge belongs unless all s_k > 0 or all s_k < 0.
//         (The rectangle is convex: the line misses it exactly when all corners lie strictly on one side; a line that meets
//         it does so in a stretch that (1) places on the segment, since both are intervals of the line whose projections on
//         both axes overlap.)  A == B gives s_k = 0, so (1) alone decides.  An end inside w settles the pair without a
//         product.  Per pair one byte of flags: bit 0 = A lies in w (closed), bit 1 = B does.  3: the edge lies wholly
//         inside; 0: it passes through, or touches, with both ends outside; 1, 2: it leaves through the border.
//
// CLAMP   Before anything else a window is normalised (normalise): the empty window stays empty; a window that lies wholly
// beside the domain that rj_upload_map accepts ([-2^46, 2^46 - 1] on both axes, rj_device.h) meets no edge and becomes
// empty; every coordinate of what is left is clamped to the domain.  Every map coordinate lies inside the domain, so
// the clamp removes only points that no edge has: it changes no result.  (A window beside the domain must become empty
// first: clamped, it would turn into a line ON the domain's border.)  Behind it every difference below fits 48 bits, every
// product 96.
//
// BOXES   The index's boxes are quantised, q(v) = (v + 2^46) >> 16 (nearest::cell_of, rj_device.h's quant); the window's
// corners are quantised the same way (QWin).  box_overlaps: the quantised closed intervals overlap -- floor is monotone, so
// real overlap implies it; what it keeps the exact test decides.  box_inside: the containment shortcut, see there.
// Padding boxes (nearest::box_empty) are excluded explicitly by both, as everywhere.
//
// ORDER   rj_within.h's: a pair is the 64-bit key (window number << 32) | eid (within::pair_key), appended in any order,
// sorted over within::key_bits(nw) bits; the per-window counts are scanned into the offsets.  The flags are never carried
// through the sort: they are recomputed from the sorted key (end_flags).
//
// SCRATCH of a call, allocated and freed by it: 12 bytes per window (the count and the scanned offset) + 8 bytes per pair
// of capacity (the unsorted keys) + 8 bytes per pair found (the sorted keys) + rocPRIM's temporaries of one scan over the
// windows and one radix sort over the pairs found.  The counting call takes the per-window part only.
//
// OUT OF SCOPE   the faces a window meets (a PIP of a corner as well), clipping the geometry, sharding across GPUs, the
// host CLIs, bench.py.
//
// One function per element that rj_window.hip runs on the device and tests/hosttwin/window_twin.cc as a brute force over
// all edges (a test-only twin, never a fallback):
//
//   normalise / quantise                 the clamp and the window in cells
//   box_meets / side / meets / end_flags the exact predicate and the flags
//   box_overlaps / box_inside            the prune and the containment shortcut
#pragma once
#include "rj_within.h"

namespace rj {
namespace window {

constexpr int64_t kDomainLo = -((int64_t) 1 << 46), kDomainHi = ((int64_t) 1 << 46) - 1;  // what rj_upload_map accepts
constexpr uint64_t kMaxWindows = within::kMaxPoints;  // nw and pair_capacity stay below it: both halves of a key are 32 bits
constexpr uint32_t kFlagA = 1, kFlagB = 2, kFlagsInside = 3;

struct Win {  // four int64 of the caller's array
  int64_t x0, y0, x1, y1;
};
struct QWin {  // the normalised window in cells
  int32_t x0, y0, x1, y1;
};
struct Counts {  // rj_window_counts
  uint64_t n_pairs, n_windows_hit, max_per_window;
};

// ---- 1. the clamp ----------------------------------------------------------------------------------------------------------
RJ_HD int64_t clamp_coord(int64_t v) { return v < kDomainLo ? kDomainLo : (v > kDomainHi ? kDomainHi : v); }
// false: the window lists nothing (empty, or wholly beside the domain); true: *w is the same window inside the domain
RJ_HD bool normalise(Win* w) {
  if (w->x0 > w->x1 || w->y0 > w->y1) return false;
  if (w->x1 < kDomainLo || w->x0 > kDomainHi || w->y1 < kDomainLo || w->y0 > kDomainHi) return false;
  w->x0 = clamp_coord(w->x0), w->y0 = clamp_coord(w->y0), w->x1 = clamp_coord(w->x1), w->y1 = clamp_coord(w->y1);
  return true;
}
RJ_HD QWin quantise(const Win& w) { return QWin{nearest::cell_of(w.x0), nearest::cell_of(w.y0), nearest::cell_of(w.x1), nearest::cell_of(w.y1)}; }

// ---- 2. the exact predicate (w normalised) ----------------------------------------------------------------------------------
RJ_HD bool point_in(int64_t x, int64_t y, const Win& w) { return x >= w.x0 && x <= w.x1 && y >= w.y0 && y <= w.y1; }
// bit 0: A lies in w, bit 1: B does
RJ_HD uint32_t end_flags(const Seg& s, const Win& w) { return (point_in(s.x1, s.y1, w) ? kFlagA : 0u) | (point_in(s.x2, s.y2, w) ? kFlagB : 0u); }
// (1): the bounding box of the segment overlaps the window, closed on both sides
RJ_HD bool box_meets(const Seg& s, const Win& w) {
  const int64_t lx = s.x1 < s.x2 ? s.x1 : s.x2, hx = s.x1 < s.x2 ? s.x2 : s.x1;
  const int64_t ly = s.y1 < s.y2 ? s.y1 : s.y2, hy = s.y1 < s.y2 ? s.y2 : s.y1;
  return hx >= w.x0 && lx <= w.x1 && hy >= w.y0 && ly <= w.y1;
}
// sign((B - A) x (C - A)): operands below 2^48, two products below 2^96
RJ_HD int side(const Seg& s, int64_t cx, int64_t cy) {
  const i128 v = (i128) (s.x2 - s.x1) * (cy - s.y1) - (i128) (s.y2 - s.y1) * (cx - s.x1);
  return (v > 0) - (v < 0);
}
// (2): the corners are not all strictly on one side of the line.  One corner at a time: two products alive at most.
RJ_HD bool line_meets(const Seg& s, const Win& w) {
  bool all_pos = true, all_neg = true;
  for (int k = 0; k < 4; k++) {
    const int sg = side(s, (k & 1) ? w.x1 : w.x0, (k & 2) ? w.y1 : w.y0);
    all_pos = all_pos && sg > 0;
    all_neg = all_neg && sg < 0;
  }
  return !(all_pos || all_neg);
}
// the edge belongs to the window; *flags: its byte (also where it does not belong: then 0)
RJ_HD bool meets(const Seg& s, const Win& w, uint32_t* flags) {
  *flags = end_flags(s, w);
  if (*flags) return true;  // an end inside settles the pair
  return box_meets(s, w) && line_meets(s, w);
}

// ---- 3. the boxes of the index ---------------------------------------------------------------------------------------------
// the box [bx0, bx1] x [by0, by1] (cells, closed) may hold a point of the window: the quantised closed intervals overlap
RJ_HD bool box_overlaps(int32_t bx0, int32_t by0, int32_t bx1, int32_t by1, const QWin& q) {
  return !nearest::box_empty(bx0, bx1) && bx0 <= q.x1 && bx1 >= q.x0 && by0 <= q.y1 && by1 >= q.y0;
}
// The containment shortcut: everything below the box lies in the window, flags 3, no test.  A coordinate v of a segment
// below the box has q(v) >= bx0 > q(x0).  Floor is monotone: v <= x0 would give q(v) <= q(x0), so v > x0; in the same way
// q(v) <= bx1 < q(x1) gives v < x1, and likewise on y.  Both ends of every such segment lie strictly inside w: flags 3, and
// the segment, a convex combination of them, lies inside with them.  STRICT on all four sides: a box that only reaches the
// window's own cell (bx0 == q(x0)) may hold coordinates on either side of x0 inside that cell.
RJ_HD bool box_inside(int32_t bx0, int32_t by0, int32_t bx1, int32_t by1, const QWin& q) {
  return !nearest::box_empty(bx0, bx1) && bx0 > q.x0 && bx1 < q.x1 && by0 > q.y0 && by1 < q.y1;
}

}  // namespace window

#if defined(__HIPCC__)
// what the device pipeline takes (rj_window.hip); filled by rj_window_query
struct WindowArgs {
  DeviceBvh bvh;
  const Seg* seg;      // the base map's segments in eid order: what the flags are recomputed from
  const int64_t* win;  // [nw][4]
  uint64_t nw;
  uint64_t capacity;   // pairs there is room for (0: the counting call)
  uint64_t* offsets;   // [nw + 1] or null
  uint32_t* eid;       // [capacity]
  uint8_t* flags;      // [capacity] or null
  uint32_t* fault;     // the handle's fault words as the device sees them
  unsigned long long* stats;  // null, or [16]: [0] nodes expanded, [1] leaf blocks loaded, [2] pairs tested exactly, [3] pairs handed out by containment, [4] pairs appended
  int stack_cap;       // the instrumented kernel only: a lower stack capacity (tests of the fault path)
  int start_level;     // 0: by rule (window_start_level); otherwise the level, clamped to [1, top]
  bool contained;      // the containment shortcut is on (off: every pair is tested exactly; the same result)
};
struct WindowResult {
  window::Counts counts;
  uint64_t appended;  // what the traversal appended (filling calls): equal to n_pairs, or the call is RJ_E_INTERNAL
  bool emitted;       // eid / flags were written (capacity > 0 and n_pairs <= capacity)
};
// THE START LEVEL: a work item of k_window is (window, group of 64 consecutive entries of level s), so a call has
// nw * ceil(nlvl[s] / 64) items.  s = top is one item per window: right for a million windows, one wave for one window over
// the whole map.  Every level down multiplies the items by up to 64, and the cheap rejects of a small window by as much.
// The rule goes down from the top while the call has fewer than 64 items per wave that the chip holds (`waves`): enough
// items to even out what one item takes.  Measured (profiles/window_fullsize.txt, 25.7 M edges, 4 levels, the filling call
// by level 1 / 2 / 3 / 4): one window 5.9 / 6.3 / 297 / 699 ms; 256 windows 6.3 / 7.3 / 7.4 / 7.2 ms (counting: 0.9 / 2.8 /
// 3.3 / 3.3); 2^20 tiles 2619 / 29.7 / 7.0 / 7.0 ms; 2^20 point windows 2623 / 28.3 / 2.1 / 1.9 ms.  The rule takes 5.9,
// 6.3, 7.0 and 1.9 ms there: no shape loses more than 5 % to its best level, on this map and on 7.1 M edges.
inline int window_start_level(const DeviceBvh& T, uint64_t nw, uint64_t waves) {
  int s = T.top;
  while (s > 1 && nw * ((T.nlvl[s] + 63) / 64) < 64 * waves) s--;
  return s;
}
// The whole call: marks ev[0] in front of the traversal, ev[1] behind it and ev[2] behind the outputs; one host sync behind
// the scan (the number of pairs sizes the sort) and one at the end.  Any grid gives the same result (blocks <= 0: by
// size).  The scratch is gone when it returns.
hipError_t window_device(hipStream_t st, const WindowArgs& a, bool stats, int blocks, int cus, StageEvents* ev, WindowResult* result);
#endif

}  // namespace rj
