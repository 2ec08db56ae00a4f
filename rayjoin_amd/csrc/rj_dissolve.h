// rj_dissolve.h -- merging the faces of a chain map by class and re-joining its chains (rj_map_dissolve,
// include/rayjoin_amd.h; kernels in rj_dissolve.hip): what GIS users know as Dissolve, and with RJ_DISS_KEEP_EQUAL and
// identity classes the re-joining of a map whose chains meet two by two.  A chain-level call: it never looks at an edge.
// Integers only, exact, and fully determined: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1], left[nc], right[nc]: a labelled chain map with the contract, the checks and the size
//         limits of rj_map_eliminate (rj_eliminate.h; a chain may have a single point).  Labels are any int32.  The point
//         arrays, input and output, are 16-byte aligned (device allocations are).
// CLASS   class(0) = 0.  Without a table class(f) = f.  With a table class_of[n_labels]: class(f) = class_of[f] for
//         0 < f < n_labels; a nonzero label outside that range is UNMAPPED: counted, and the call is refused with nothing
//         written.  A nonzero label may map to 0: that erases the face into the outside.
// KEPT    a chain whose points are all equal is SKIPPED.  Of the others a chain is KEPT unless class(left) ==
//         class(right) and kKeepEqual is not set (DROPPED): bridges and dangles go with the borders unless the flag
//         keeps them.
// HALF-CHAINS   h = 2 c walks chain c first -> last with classes (L, R) = (class(left), class(right)); h = 2 c + 1 walks
//         last -> first with classes (R, L).  h ^ 1 is the twin of h.  The start point of h is the chain's first point for
//         even h and its last point for odd h.  edges(h) = the chain's points - 1.
// PASSING A VERTEX   rj_ringmap.h's rule with chains for edges.  h arrives at the start point of h ^ 1.  When exactly two
//         kept half-chains start there (h ^ 1 and one other, g) and classes(g) == classes(h): next(h) = g.  Otherwise h
//         ends there (a junction, a dead end, a change of classes).  A closed chain alone at its vertex: the two are h ^ 1
//         and h, so next(h) = h.  Symmetric: next(h) = g <=> next(g ^ 1) = h ^ 1, so pred(g) = next(g ^ 1) ^ 1.
// WALKS   the maximal sequences under next: open, or closed (a cycle of one or more half-chains).  The twin walk of W:
//         its twins in reverse order; never W itself (next never turns round).  Leader: the first half-chain of an open
//         walk, the smallest of a closed one, which is read from there.  Of W and its twin the OUTPUT CHAIN is the one
//         with the smaller leader.
// OUTPUT  chains ascend by leader.  The points of a chain: every half-chain's points in its direction without its last
//         point, then the last point of the last half-chain; copied verbatim (repeated points inside an input chain stay),
//         a closed output chain repeats its first point.  out_left / out_right: the classes of the leader;
//         origin[k]: the leader's input chain; chain_out[c] = (k << 1) | reversed for a kept input chain c that output
//         chain k holds, kNone for a dropped or skipped one.  n_points = the edges of the kept chains + n_chains;
//         n_closed: the output chains that are closed walks; every output chain has at least 2 points: the contract of
//         rj_upload_map_dev.
// CLASS RECORDS   one per nonzero class value on a kept chain, ascending by (uint32_t) label (eliminate's numbering):
//         area2 = the sum of S(c) over the kept chains with class(left) = k minus the sum over class(right) = k, S =
//         eliminate::edge_cross summed per chain, an exact int128 (dropped chains have the class on both sides and cancel);
//         n_sides = the kept chain sides that carry the class.
//
// Every step is one function per element that rj_dissolve.hip runs as a kernel and tests/hosttwin/dissolve_twin.cc runs as
// a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate (rj_rings.h)   the input check: the largest code met is the status
//   chain_scan    per chain, lane l of w: the points l, l + w, ... -- their check, their edges' cross products, whether one
//                 differs from the first point (summed / ORed over the lanes: integer sums commute)
//   class_of / chain_finish   per chain: the classes of its sides, kept / dropped / skipped, S(c)
//   half_seed / half_start    per h: itself where kept (kNone sorts last), its start point
//   (merge sort of the half-chains by half_before: (start point, h); half_pos the inverse)
//   next_of       per h: next(h), from the two neighbours on each side of h ^ 1 in that order: no per-vertex loop, no
//                 degree cap
//   walk_init / ringmap::walk_round / cut_init   rj_ringmap.h's two-pass pointer doubling along pred; the state's cnt
//                 carries the EDGES walked (np < 2^32), so a half-chain knows its point offset in its output chain
//   side_key / side_val   per chain side: the sort key of its class on a kept chain (kZeroKey otherwise), +S, -S and 1
//   (sort by key, sum by key: the classes ascending with their areas and sides; class 0, if any, is the last key)
//   chain_total   per h: a kept leader gives 1 chain and its edges + 1 points (exclusive scan: chain number, first point)
//   chain_place   per chain, lane l of w: the points of its placed half-chain to their slots, consecutive lanes consecutive
//                 points, reversed for odd h; lane 0 the chain's chain_out and, for a leader, the row entry, the classes
//                 and the origin
//
// Scratch per call: per chain 28 bytes (S 16, the two classes 8, the state 4) and per half-chain (2 nc of them) 180 bytes
// (the start point 16; the seed, the order and its inverse 12; next 4; two walk states 32; the totals and their scan 32;
// the record sort's keys in and out 8 and values in and out 48, the unique keys 4 and the sums 24): 388 bytes per chain
// in all and NONE per point, plus rocPRIM's temporary storage.  Allocated per call and freed.
#pragma once
#include <stdint.h>

#include "rj_eliminate.h"
#include "rj_ringmap.h"

namespace rj {
namespace dissolve {

using rings::Slots;  // {halves, points}: here {chains, points}
using rings::U128;
using ringmap::Walk;
typedef __int128 i128;

constexpr uint32_t kKeepEqual = 1u;  // RJ_DISS_KEEP_EQUAL
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kZeroKey = eliminate::kZeroKey;
constexpr int kMaxRounds = 33;                                 // doubling steps: 2^32 half-chains at most
constexpr uint32_t kDropped = 0, kKept = 1, kSkipped = 2;      // the state of a chain

struct ClassRec {  // rj_diss_class (24 bytes)
  int32_t label;
  uint32_t n_sides;
  uint64_t area2_lo;
  int64_t area2_hi;
};
struct Counts {  // rj_dissolve_counts
  uint64_t n_kept, n_dropped, n_skipped, n_chains, n_points, n_closed, n_classes, n_unmapped;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t act[2][kMaxRounds];  // pass p, round r: walks that reached their head plus minima that changed
  uint32_t done[2];             // the first round that was not needed: the final state is in buffer done & 1
  uint32_t bad;                 // the input check's status (rings::kBad*); not 0: nothing further is read or written
  uint32_t unfinished;          // a round budget ran out (cannot happen)
  uint32_t emit;                // 1: every output fits its capacity and is written
  uint32_t pad;
  uint64_t n_keys;              // unique class keys (the classes, and kZeroKey where it occurs)
  Counts counts;
};
struct Pt {
  int64_t x, y;
};
struct Side {  // what a class sums over its sides
  U128 sum;
  uint64_t n;
};
// the caller's arrays (each may be null where the header says so) and their capacities (row: chain_cap + 1 entries)
struct Out {
  ClassRec* classes;
  int32_t *left, *right;
  int64_t* xy;
  uint32_t *row, *origin, *chain_out;
  uint64_t class_cap, chain_cap, point_cap;
};

RJ_RHD bool refused(const Meta& m) { return m.bad != 0 || m.counts.n_unmapped != 0; }

// ---- 1. the check, the classes, what is kept ---------------------------------------------------------------------
// lane `lane` of `width`: the points lane, lane + width, ... of chain c.  Reads nothing where row[] does not give a
// range inside the np points (the check of a malformed row says so elsewhere).
RJ_RHD void chain_scan(uint64_t c, uint32_t lane, uint32_t width, const int64_t* xy, const uint32_t* row, uint64_t np, uint32_t* bad, i128* sum,
                       bool* differs) {
  const uint64_t b = row[c], e = row[c + 1];
  if (!(b < e && e <= np)) return;
  const int64_t x0 = xy[2 * b], y0 = xy[2 * b + 1];
  for (uint64_t p = b + lane; p < e; p += width) {
    const int64_t px = xy[2 * p], py = xy[2 * p + 1];
    const uint32_t bx = rings::check_coordinate(px), by = rings::check_coordinate(py);
    *bad = *bad > bx ? *bad : bx;
    *bad = *bad > by ? *bad : by;
    *differs = *differs || px != x0 || py != y0;
    if (p + 1 < e) *sum += eliminate::edge_cross(px, py, xy[2 * p + 2], xy[2 * p + 3]);
  }
}
// -> the class of label f; *unmapped: f is a nonzero label outside the table
RJ_RHD int32_t class_of(int32_t f, const int32_t* table, uint64_t n_labels, bool* unmapped) {
  *unmapped = false;
  if (f == 0 || !table) return f;
  if (f > 0 && (uint64_t) f < n_labels) return table[f];
  *unmapped = true;
  return 0;
}
// once per chain, with what all its lanes found -> its state; *unmapped: how many of its two labels are
RJ_RHD uint32_t chain_finish(uint64_t c, const int32_t* left, const int32_t* right, const int32_t* table, uint64_t n_labels, uint32_t flags, i128 sum,
                             bool differs, int32_t* cl, int32_t* cr, U128* S, uint32_t* state, uint32_t* unmapped) {
  bool ul, ur;
  const int32_t l = class_of(left[c], table, n_labels, &ul), r = class_of(right[c], table, n_labels, &ur);
  const uint32_t s = !differs ? kSkipped : (l == r && !(flags & kKeepEqual) ? kDropped : kKept);
  cl[c] = l;
  cr[c] = r;
  S[c] = rings::limbs(sum);
  state[c] = s;
  *unmapped = (ul ? 1u : 0u) + (ur ? 1u : 0u);
  return s;
}

// ---- 2. chain ends by start point, next ---------------------------------------------------------------------------
RJ_RHD uint32_t edges_of(uint32_t h, const uint32_t* row) { return row[(h >> 1) + 1] - row[h >> 1] - 1; }
RJ_RHD int32_t left_of(uint32_t h, const int32_t* cl, const int32_t* cr) { return (h & 1) ? cr[h >> 1] : cl[h >> 1]; }
RJ_RHD int32_t right_of(uint32_t h, const int32_t* cl, const int32_t* cr) { return (h & 1) ? cl[h >> 1] : cr[h >> 1]; }
// h in [0, 2 nc): the half-chains that are not kept are fillers, which sort last and are never looked up
RJ_RHD void half_seed(uint32_t h, const uint32_t* state, const int64_t* xy, const uint32_t* row, uint32_t* seed, Pt* start) {
  const bool kept = state[h >> 1] == kKept;
  seed[h] = kept ? h : kNone;
  if (!kept) return;
  const uint64_t p = (h & 1) ? (uint64_t) row[(h >> 1) + 1] - 1 : row[h >> 1];
  start[h] = Pt{xy[2 * p], xy[2 * p + 1]};
}
// the order of the sort: (start point, h), fillers last.  A strict weak order; strict and total on the kept half-chains.
RJ_RHD bool half_before(uint32_t ha, uint32_t hb, const Pt* start) {
  if (hb == kNone) return ha != kNone;
  if (ha == kNone) return false;
  const Pt a = start[ha], b = start[hb];
  if (a.x != b.x) return a.x < b.x;
  if (a.y != b.y) return a.y < b.y;
  return ha < hb;
}
RJ_RHD void half_pos(uint64_t k, const uint32_t* order, uint32_t* pos) { pos[order[k]] = (uint32_t) k; }
RJ_RHD bool starts_at(uint32_t h, const Pt* start, Pt p) { return start[h].x == p.x && start[h].y == p.y; }
// order = the nh kept half-chains by (start point, h), pos its inverse; h kept.  Exactly two start where h ^ 1 does: one
// neighbour of h ^ 1 in the order starts there, and the position behind that neighbour (and the other neighbour) do not.
RJ_RHD uint32_t next_of(uint32_t h, uint64_t nh, const uint32_t* order, const uint32_t* pos, const Pt* start, const int32_t* cl, const int32_t* cr) {
  const uint64_t k = pos[h ^ 1];
  const Pt p = start[h ^ 1];
  const bool below = k > 0 && starts_at(order[k - 1], start, p), above = k + 1 < nh && starts_at(order[k + 1], start, p);
  if (below == above) return kNone;  // a dead end, or three and more
  uint32_t g;
  if (below) {
    if (k > 1 && starts_at(order[k - 2], start, p)) return kNone;
    g = order[k - 1];
  } else {
    if (k + 2 < nh && starts_at(order[k + 2], start, p)) return kNone;
    g = order[k + 1];
  }
  if (left_of(g, cl, cr) != left_of(h, cl, cr) || right_of(g, cl, cr) != right_of(h, cl, cr)) return kNone;
  return g;
}

// ---- 3. heads, leaders, offsets: rj_ringmap.h's pointer doubling with edges for steps -----------------------------------
// next[h] is kNone for a half-chain that is not kept: a walk of its own, which chain_total leaves out
RJ_RHD void walk_init(uint32_t h, const uint32_t* next, const uint32_t* row, Walk* a, Walk* b) {
  const uint32_t p = ringmap::pred_of(h, next);
  a[h] = b[h] = p == kNone ? Walk{h, 0, h, 1} : Walk{p, edges_of(p, row), p < h ? p : h, 0};
}
// F = the final states of the first pass: an open walk (done) keeps its head and its edges from there; a closed walk
// (never done, F.mn its smallest half-chain) is opened in front of that leader
RJ_RHD void cut_init(uint32_t h, const Walk* F, const uint32_t* next, const uint32_t* row, Walk* a, Walk* b) {
  const Walk f = F[h];
  Walk n;
  if (f.done)
    n = Walk{f.at, f.cnt, 0, 1};
  else if (f.mn == h)
    n = Walk{h, 0, 1, 1};
  else {
    const uint32_t p = ringmap::pred_of(h, next);
    n = Walk{p, edges_of(p, row), 1, 0};
  }
  a[h] = b[h] = n;
}

// ---- 4. class records -------------------------------------------------------------------------------------------
// chain side i = 2 c + s (s = 0 left, 1 right)
RJ_RHD uint32_t side_key(uint64_t i, const uint32_t* state, const int32_t* cl, const int32_t* cr) {
  return state[i >> 1] == kKept ? eliminate::key_of((i & 1) ? cr[i >> 1] : cl[i >> 1]) : kZeroKey;
}
RJ_RHD Side side_val(uint64_t i, const U128* S) { return Side{(i & 1) ? rings::sub(U128{0, 0}, S[i >> 1]) : S[i >> 1], 1}; }
RJ_RHD Side side_add(const Side& a, const Side& b) { return Side{rings::add(a.sum, b.sum), a.n + b.n}; }
RJ_RHD ClassRec record_of(uint64_t k, const uint32_t* keys, const Side* sums) {
  return ClassRec{eliminate::label_of(keys[k]), (uint32_t) sums[k].n, sums[k].sum.lo, (int64_t) sums[k].sum.hi};
}

// ---- 5. chains ------------------------------------------------------------------------------------------------------
// W = the final states of the second pass: W[h].at the leader of h's walk, W[h].cnt the edges in front of h in it,
// W[h].mn 1 on a closed walk.  h in [0, nh]: total[h]; entry nh closes the scan.  -> true for the leader of a closed chain
RJ_RHD bool chain_total(uint64_t h64, uint64_t nh, const uint32_t* state, const Walk* W, const uint32_t* next, const uint32_t* row, Slots* total) {
  if (h64 >= nh || state[h64 >> 1] != kKept || !ringmap::kept_leader((uint32_t) h64, W)) {
    total[h64] = Slots{0, 0};
    return false;
  }
  const uint32_t h = (uint32_t) h64;
  const bool closed = W[h].mn != 0;
  const uint32_t last = closed ? ringmap::pred_of(h, next) : h ^ 1;  // (open: h ^ 1 has as many edges behind its head as the walk in front of its last)
  total[h] = Slots{1, (uint64_t) W[last].cnt + edges_of(last, row) + 1};
  return closed;
}
// every output fits: classes only where records are asked for
RJ_RHD bool fits(const Counts& c, const Out& o) {
  return (!o.classes || c.n_classes <= o.class_cap) && c.n_chains <= o.chain_cap && c.n_points <= o.point_cap;
}
RJ_RHD void copy_point(const int64_t* src, int64_t* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<longlong2*>(dst) = *reinterpret_cast<const longlong2*>(src);  // (one 16-byte access)
#else
  dst[0] = src[0];
  dst[1] = src[1];
#endif
}
// base = the exclusive scan of total[].  lane `lane` of `width`, chain c of a call whose outputs fit: the points of the
// half-chain of c that lies in an output chain (of h and h ^ 1 exactly one has a kept leader)
RJ_RHD void chain_place(uint64_t c, uint32_t lane, uint32_t width, const int64_t* xy, const uint32_t* row, const uint32_t* state, const int32_t* cl,
                        const int32_t* cr, const Walk* W, const Slots* base, const Out& o) {
  if (state[c] != kKept) {
    if (lane == 0 && o.chain_out) o.chain_out[c] = kNone;
    return;
  }
  const uint32_t even = (uint32_t) (2 * c), h = ringmap::kept_leader(W[even].at, W) ? even : even + 1, a = W[h].at;
  const Slots at = base[a];
  const uint64_t n_pts = base[(uint64_t) a + 1].points - at.points, b = row[c], e = row[c + 1], ne = e - b - 1;
  const uint64_t off = at.points + W[h].cnt, count = ne + (W[h].cnt + ne + 1 == n_pts ? 1 : 0);  // (the last of its chain: its end point too)
  const bool back = h & 1;
  for (uint64_t k = lane; k < count; k += width) copy_point(xy + 2 * (back ? e - 1 - k : b + k), o.xy + 2 * (off + k));
  if (lane != 0) return;
  if (o.chain_out) o.chain_out[c] = (uint32_t) (at.halves << 1) | (back ? 1u : 0u);
  if (h == a) {
    o.row[at.halves] = (uint32_t) at.points;
    o.left[at.halves] = left_of(h, cl, cr);
    o.right[at.halves] = right_of(h, cl, cr);
    if (o.origin) o.origin[at.halves] = (uint32_t) c;
  }
}

}  // namespace dissolve

#if defined(__HIPCC__)
// what a call reports besides its counts
struct DissolveReport : StageMs {};  // check, classes and keep; ends sorted and next; walks; class records; totals and scatter; all
// rj_map_dissolve behind its argument checks, on stream st: *result = the device's Meta.  point_blocks: the grid of the
// point scatter (0: by size; any grid gives the same result).  Allocates and frees its scratch; synchronises the stream
// once, at the end.
hipError_t map_dissolve_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                               const int32_t* class_table, uint64_t n_labels, uint32_t flags, const dissolve::Out& out, int point_blocks,
                               dissolve::Meta* result, DissolveReport* report);
#endif

}  // namespace rj
