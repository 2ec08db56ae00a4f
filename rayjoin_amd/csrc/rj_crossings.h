// rj_crossings.h -- the crossings inside ONE chain map (rj_map_crossings, include/rayjoin_amd.h; kernels in
// rj_crossings.hip): all pairs of edges that meet anywhere except in a shared end point.  A chain map without such a
// pair is a planar subdivision, which every other stage of the library assumes and none checks (the reference never
// validates a map either: Map::LoadFrom, src/map/map.h:162-233).  Integers only, exact, and fully determined: no tuning
// choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1]: a chain map with the contract of rj_map_rings (row_index starts at 0, ends at
//         np and ascends: a chain may have a single point; every coordinate in [-2^46, 2^46)).  Faces are not needed.
//         Edge e = p - c joins points p and p + 1 of chain c (the reference's numbering, map.h:200-203);
//         ne = np - nc < 2^32 - 1.  An edge whose two points are equal is skipped and counted in n_zero_edges.
// RELATION   for two distinct non-zero edges e < f let S be the intersection of their closed segments:
//         S empty                                                        none
//         one point, an end point of e AND an end point of f             none (consecutive edges of a chain, a junction)
//         one point, an end point of exactly one of them                 kTouch   2: a vertex inside another edge
//         one point, an end point of neither                             kProper  1
//         more than one point (collinear overlap), end-point sets differ kOverlap 3
//         the same two end points, in either direction                   kEqual   4 (a chain that folds back a -> b -> a)
//         decided from four orientation signs, each the sign of an int128 cross product of coordinate differences
//         (every difference below 2^47, every product below 2^94).  All four zero: the edges are collinear; with lo < hi
//         the end points of each in ascending (x, y), max(lo_e, lo_f) > min(hi_e, hi_f): empty; ==: a shared end point;
//         <: kOverlap, or kEqual when the end-point sets match.  Otherwise the first zero sign names the only point the
//         segments can share (orient(e.a, e.b, f.a) == 0 names f.a): it is in S iff it lies in the closed box of the
//         other segment, and it is a shared vertex iff it equals one of that segment's end points.  No zero sign: kProper
//         iff both pairs of signs differ.  No floating point, no division, no simulation of simplicity.
// RESULT  one record (eid[0] < eid[1], kind) per unordered pair with a kind other than none, every pair exactly once,
//         ascending by ((uint64) eid[0] << 32) | eid[1].
// CANDIDATES   a sparse uniform grid of the map's own: the cell of a coordinate is (v + 2^46) >> s, an integer shift and
//         monotone.  An edge is registered in every cell of its bounding box's cell range; the (cell, eid) pairs are
//         sorted by the 64-bit key cell = (cy << 32) | cx (so s >= 15) with one radix sort, and a run of equal keys is
//         one cell's list.  No dense table of cells: their number is unbounded.  A pair is tested only in its ANCHOR
//         cell (max of the two x-lows, max of the two y-lows): that cell lies in both ranges whenever the ranges overlap,
//         and segments that meet have overlapping ranges -- every reportable pair is tested exactly once, no sort-unique.
// CHOICE OF s   one pass sums max(|dx|, |dy|) over the non-zero edges and counts, for every s in 15..47, the
//         registrations.  The host takes the smallest s with 2^s >= kExtentFactor x the mean extent and
//         registrations(s) <= kRegFactor x ne + 1024 (s = 47 has one registration per edge: it always exists).  8 and 4:
//         DESIGN.md has what was measured.
// GUARD   the number of pair tests, the sum over the runs of k (k - 1) / 2, is known after the sort.  Above the budget
//         (kPairBudget) the pair pass is not launched: a few domain-long edges over millions of short ones would
//         occupy the device for minutes.
//
// Every step is one function per element that rj_crossings.hip runs as a grid-stride kernel and
// tests/hosttwin/crossings_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate   the input check; a map that fails is not read further
//   edge_of       per edge: its chain by a binary search of row_index, its two points
//   reg_count     per edge and shift: the cells of its bounding box (clamped: kClamp and above only says "too many")
//   extent_of     per edge: max(|dx|, |dy|)
//   choose_shift  the host's choice from the sums
//   reg_at        per registration r: its edge by a binary search of the scanned counts, its cell key
//   (one radix sort of the (cell, eid) pairs by cell)
//   run_head      per sorted position: its own position where a run starts, else 0 (inclusive max-scan: the run's start)
//   item_flag     per sorted position: does a work item start here -- a run, or the next kRowBlock rows of a long run;
//                 the last position of a run also gives the run's length
//   (the flagged positions selected: the list of work items)
//   row_limit / pair_kind   the pair pass: item p owns rows i in [p, p + kRowBlock) of its run, every row against the
//                 columns j > i of the run; pair_kind is the anchor-cell filter, then the relation
//   (one radix sort of the hits by (eid[0], eid[1]))
#pragma once
#include <stdint.h>

#include "rj_rings.h"

namespace rj {
namespace crossings {

constexpr uint32_t kNone = 0, kProper = 1, kTouch = 2, kOverlap = 3, kEqual = 4;  // RJ_CROSS_*
constexpr int64_t kHalfRange = (int64_t) 1 << 46;
constexpr int kMinShift = 15, kMaxShift = 47, kShifts = kMaxShift - kMinShift + 1;
constexpr uint64_t kRowBlock = 64;                 // rows of a run per work item: one per lane of a wave
constexpr uint64_t kPairBudget = 1ull << 36;       // pair tests above which the call refuses
constexpr uint64_t kClamp = 1ull << 37;            // sums that only have to say "above every threshold" stop here
constexpr uint64_t kExtentFactor = 8, kRegFactor = 4, kRegSlack = 1024;  // (measured: profiles/crossings_fullsize.txt)

struct alignas(16) Edge {
  int64_t ax, ay, bx, by;
};
struct Counts {  // rj_crossings_counts
  uint64_t n_found, n_proper, n_touch, n_overlap, n_equal, n_edges, n_zero_edges;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;            // the input check's status (kBad*); not 0: the map is not read further
  uint32_t _pad;
  uint64_t regs[kShifts];  // registrations at shift kMinShift + k; exact below kClamp
  uint64_t extent_lo, extent_hi;  // the sums of the low 32 bits and of the bits above them of every extent (each fits)
  uint64_t pair_tests;     // exact below kClamp
  uint64_t largest_run;    // the longest cell list
  uint64_t largest_at;     // ... and the smallest sorted position where one of that length starts
  uint64_t n_items;
  Counts counts;
};

RJ_RHD uint64_t clamp_add(uint64_t a, uint64_t b) { return a + b < kClamp ? a + b : kClamp; }  // (a, b <= kClamp)

// ---- 0. the input check ------------------------------------------------------------------------------
// The map check of rj_rings.h, one definition: the largest code met is the input's status, 0: fine.  c in [0, nc]; every
// coordinate.
using rings::check_coordinate;
using rings::check_row;
using rings::kBadCoordinate;
using rings::kBadEmptyChain;
using rings::kBadEnd;
using rings::kBadStart;

// ---- 1. edges ------------------------------------------------------------------------------------------
// the chain of edge e: the last c with row[c] - c <= e (chains of one point have no edge and share that number with
// the chain behind them)
RJ_RHD uint64_t chain_of(uint64_t e, const uint32_t* row, uint64_t nc) {
  uint64_t lo = 0, hi = nc;  // row[lo] - lo <= e < row[hi] - hi
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint64_t) row[mid] - mid <= e)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
RJ_RHD Edge edge_of(uint64_t e, const uint32_t* row, uint64_t nc, const int64_t* xy) {
  const uint64_t p = e + chain_of(e, row, nc);
  return Edge{xy[2 * p], xy[2 * p + 1], xy[2 * p + 2], xy[2 * p + 3]};
}
RJ_RHD bool is_zero(const Edge& e) { return e.ax == e.bx && e.ay == e.by; }

// ---- 2. the grid ---------------------------------------------------------------------------------------
RJ_RHD uint64_t cell_of(int64_t v, int s) { return (uint64_t) (v + kHalfRange) >> s; }
RJ_RHD int64_t lesser(int64_t a, int64_t b) { return a < b ? a : b; }
RJ_RHD int64_t greater(int64_t a, int64_t b) { return a < b ? b : a; }
struct Range {  // the cells of an edge's bounding box
  uint64_t x0, x1, y0, y1;
};
RJ_RHD Range range_of(const Edge& e, int s) {
  return Range{cell_of(lesser(e.ax, e.bx), s), cell_of(greater(e.ax, e.bx), s), cell_of(lesser(e.ay, e.by), s), cell_of(greater(e.ay, e.by), s)};
}
RJ_RHD uint64_t cell_key(uint64_t cx, uint64_t cy) { return (cy << 32) | cx; }
// the registrations of a non-zero edge at shift s: at most 2^32 cells a side, so the product is clamped in 128 bits
RJ_RHD uint64_t reg_count(const Edge& e, int s) {
  const Range r = range_of(e, s);
  const unsigned __int128 n = (unsigned __int128) (r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1);
  return n < kClamp ? (uint64_t) n : kClamp;
}
RJ_RHD uint64_t extent_of(const Edge& e) {
  const int64_t dx = e.ax < e.bx ? e.bx - e.ax : e.ax - e.bx, dy = e.ay < e.by ? e.by - e.ay : e.ay - e.by;
  return (uint64_t) greater(dx, dy);
}
// the smallest shift whose cells are kExtentFactor mean extents wide and whose registrations stay below the bound
// (n_live non-zero edges of ne; regs[] as Meta has them)
RJ_RHD int choose_shift(uint64_t extent_lo, uint64_t extent_hi, const uint64_t* regs, uint64_t n_live, uint64_t ne, uint64_t extent_factor,
                        uint64_t reg_factor) {
  const unsigned __int128 total = ((unsigned __int128) extent_hi << 32) + extent_lo;
  for (int s = kMinShift; s < kMaxShift; s++)
    if (((unsigned __int128) n_live << s) >= extent_factor * total && regs[s - kMinShift] <= reg_factor * ne + kRegSlack) return s;
  return kMaxShift;
}
// registration r: off[] = the exclusive scan of the edges' counts at the chosen shift (off[ne] = their sum), zero edges
// count 0.  The edge is the last e with off[e] <= r; its cells are numbered row by row.
RJ_RHD void reg_at(uint64_t r, const uint64_t* off, uint64_t ne, const Edge* edges, int s, uint64_t* key, uint32_t* eid) {
  uint64_t lo = 0, hi = ne;  // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  const Range g = range_of(edges[lo], s);
  const uint64_t k = r - off[lo], w = g.x1 - g.x0 + 1;
  *key = cell_key(g.x0 + k % w, g.y0 + k / w);
  *eid = (uint32_t) lo;
}

// ---- 3. runs and work items ---------------------------------------------------------------------------
// the inclusive max-scan of run_head over the sorted keys is start[]: where the run of position r begins
RJ_RHD uint64_t run_head(uint64_t r, const uint64_t* key) { return r > 0 && key[r] != key[r - 1] ? r : 0; }
// -> does a work item start at r; *run_len: the length of the run that ends at r (0: none ends here)
RJ_RHD bool item_flag(uint64_t r, uint64_t n, const uint64_t* key, const uint64_t* start, uint64_t* run_len) {
  const uint64_t at = r - start[r];
  *run_len = r + 1 == n || key[r + 1] != key[r] ? at + 1 : 0;
  return at % kRowBlock == 0;
}
// the pair tests of a run of k: k (k - 1) / 2, clamped
RJ_RHD uint64_t run_tests(uint64_t k) {
  const unsigned __int128 t = (unsigned __int128) k * (k - 1) / 2;
  return t < kClamp ? (uint64_t) t : kClamp;
}

// ---- 4. the relation -------------------------------------------------------------------------------------
RJ_RHD int orient(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t cx, int64_t cy) {
  const __int128 v = (__int128) (bx - ax) * (cy - ay) - (__int128) (by - ay) * (cx - ax);
  return v > 0 ? 1 : (v < 0 ? -1 : 0);
}
RJ_RHD bool lex_less(int64_t ax, int64_t ay, int64_t bx, int64_t by) { return ax != bx ? ax < bx : ay < by; }
// p on the line of s: is it on the closed segment; and is it one of its end points
RJ_RHD bool in_box(const Edge& s, int64_t px, int64_t py) {
  return lesser(s.ax, s.bx) <= px && px <= greater(s.ax, s.bx) && lesser(s.ay, s.by) <= py && py <= greater(s.ay, s.by);
}
RJ_RHD bool is_end(const Edge& s, int64_t px, int64_t py) { return (px == s.ax && py == s.ay) || (px == s.bx && py == s.by); }
RJ_RHD uint32_t on_line(const Edge& s, int64_t px, int64_t py) { return !in_box(s, px, py) || is_end(s, px, py) ? kNone : kTouch; }
// two non-zero edges
RJ_RHD uint32_t relate(const Edge& e, const Edge& f) {
  const int o1 = orient(e.ax, e.ay, e.bx, e.by, f.ax, f.ay), o2 = orient(e.ax, e.ay, e.bx, e.by, f.bx, f.by);
  const int o3 = orient(f.ax, f.ay, f.bx, f.by, e.ax, e.ay), o4 = orient(f.ax, f.ay, f.bx, f.by, e.bx, e.by);
  if (o1 == 0 && o2 == 0 && o3 == 0 && o4 == 0) {
    const bool ef = lex_less(e.ax, e.ay, e.bx, e.by), ff = lex_less(f.ax, f.ay, f.bx, f.by);
    const int64_t elx = ef ? e.ax : e.bx, ely = ef ? e.ay : e.by, ehx = ef ? e.bx : e.ax, ehy = ef ? e.by : e.ay;
    const int64_t flx = ff ? f.ax : f.bx, fly = ff ? f.ay : f.by, fhx = ff ? f.bx : f.ax, fhy = ff ? f.by : f.ay;
    const bool lo_e = lex_less(flx, fly, elx, ely), hi_e = lex_less(ehx, ehy, fhx, fhy);  // max of the lows, min of the highs
    const int64_t lx = lo_e ? elx : flx, ly = lo_e ? ely : fly, hx = hi_e ? ehx : fhx, hy = hi_e ? ehy : fhy;
    if (!lex_less(lx, ly, hx, hy)) return kNone;  // empty, or one shared end point
    return elx == flx && ely == fly && ehx == fhx && ehy == fhy ? kEqual : kOverlap;
  }
  if (o1 == 0) return on_line(e, f.ax, f.ay);
  if (o2 == 0) return on_line(e, f.bx, f.by);
  if (o3 == 0) return on_line(f, e.ax, e.ay);
  if (o4 == 0) return on_line(f, e.bx, e.by);
  return o1 != o2 && o3 != o4 ? kProper : kNone;
}

// ---- 5. the pair pass ---------------------------------------------------------------------------------------
// item p owns rows [p, p + kRowBlock) of its run; column j > p of the run meets the rows [p, row_limit(p, j))
RJ_RHD uint64_t row_limit(uint64_t p, uint64_t j) { return j < p + kRowBlock ? j : p + kRowBlock; }
// the pair of sorted positions i < j of one run (cell `key`): tested here only when this is its anchor cell
RJ_RHD uint32_t pair_kind(const Edge& a, const Edge& b, uint64_t key, int s) {
  const Range ra = range_of(a, s), rb = range_of(b, s);
  if (cell_key(ra.x0 < rb.x0 ? rb.x0 : ra.x0, ra.y0 < rb.y0 ? rb.y0 : ra.y0) != key) return kNone;
  return relate(a, b);
}
RJ_RHD uint64_t hit_key(uint32_t ea, uint32_t eb) { return ea < eb ? ((uint64_t) ea << 32) | eb : ((uint64_t) eb << 32) | ea; }

}  // namespace crossings

#if defined(__HIPCC__)
// what the entry point passes on: the forced shift (0: choose), the pair budget, the two factors
struct CrossingsTuning {
  int shift;
  uint64_t pair_budget, extent_factor, reg_factor;
};
// what a call reports besides its counts (tools and the guard's message)
struct CrossingsReport {
  int shift;
  uint64_t registrations, largest_run, largest_cell, pair_tests, n_items;
  bool over_budget;
  // edges and sums; registrations and their sort; runs and items; the pair pass; the sort of the hits; all.  StageMs'
  // entries, but not its first state: 0 until a call reaches the device (a map without chains included), -1 from there
  // on for what was not reached
  float ms[6];
};
// rj_map_crossings behind its argument checks, on stream st: *result = the device's Meta (counts, the input check's
// status).  Allocates and frees its scratch; synchronises the stream four times (the sums behind the grid's size; the
// pair tests; the number of hits; the end).
hipError_t map_crossings_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint64_t capacity, void* out,
                                const CrossingsTuning& tuning, crossings::Meta* result, CrossingsReport* report);
hipError_t warm_crossings_kernels(hipStream_t st);
#endif

}  // namespace rj
