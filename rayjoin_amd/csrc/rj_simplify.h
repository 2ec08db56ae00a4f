// rj_simplify.h -- thinning the chains of a map by effective area (rj_map_simplify, include/rayjoin_amd.h; kernels in
// rj_simplify.hip): Visvalingam-Whyatt over the points of every chain, in rounds that remove many points at once.  A
// border that two faces share is one chain, so both polygons are thinned identically and no sliver or gap opens between
// neighbours; the ends of a chain stay, so junctions and the chain graph do not change.  Integers only, exact, and fully
// determined: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1]: a chain map with the contract of rj_map_crossings (rj_crossings.h; a chain may
//         have a single point).  tol: an unsigned 128-bit number, twice an area in scaled units^2 (the unit of
//         rj_overlay_face.area2).  flags must be 0.
// PINNED  points that are never removed: the first and the last point of every chain.  In a CLOSED chain (3 points or
//         more, the first equal to the last) with a its first point: m1, the interior point with the greatest squared
//         distance from a (below 2^95), ties to the lowest index, pinned only if that distance is > 0; and, if m1 is
//         pinned, m2, the interior point with the greatest |cross(m1 - a, q - a)|, ties to the lowest index, pinned only
//         if that value is > 0.  A ring never collapses below the triangle a, m1, m2; a ring a -> b -> a stays.
// WEIGHT  of a live unpinned point p whose live neighbours in its chain are u (before) and w (after):
//         W(p) = |cross(p - u, w - u)|, an int128 value (every difference below 2^47: below 2^95).  p is a CANDIDATE when
//         W(p) <= tol.  Its KEY is (W(p), (uint32) (p * 2654435761u)), p the input point index: the multiplier is odd, so
//         the second part never ties, and a run of equal weights (collinear points) does not lose one point per round as
//         it would under a tie-break by index.
// ROUND   every candidate whose key is smaller than the key of each of its two live neighbours that is also a candidate
//         is removed, all of a round at once.  Removed points are never adjacent; a point whose two neighbours both go
//         loses both links in the same round.  Rounds repeat until one has no candidate: a round with a candidate removes
//         the one with the least key, so the loop ends.
// OUTPUT  the live points in input order, out_row[nc + 1], origin[k] = the input point of output point k.  Chains, their
//         number and their order do not change.
// PROPERTIES   every unpinned output point has W > tol in the output; simplify(simplify(M, t), t) removes nothing; with
//         tol = 2^128 - 1 an open chain keeps 2 points (1 if it had 1) and a closed chain its pinned points; tol = 0
//         removes what the rounds remove of zero-weight points (collinear runs, spikes a -> b -> a').  NOT promised: that
//         the thinned map has no crossings -- rj_map_crossings tells.
//
// Every step is one function per element that rj_simplify.hip runs as a grid-stride kernel and
// tests/hosttwin/simplify_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate (rj_crossings.h)   the input check: the largest code met is the status; not 0: nothing
//                 further is read and nothing is written
//   is_closed     per chain
//   far_of / wide_of / better   the two pin reductions of a closed chain over its interior points: (value, index) pairs
//                 under `better` (greater value, then lower index), which is associative and commutative: any tree
//   chain_end / links_of   per point: is it an end of its chain (pinned); its first links, never across a chain boundary
//   weight / is_candidate / stored_weight   per point of the round's work: W, or kNoWeight for a point that is no candidate
//   key_less / removes   per candidate, from the stored weights and the links as they were when the round began
//   unlink        per removed point: its neighbours are linked to each other
//   (the next round's work: the candidates that stayed and the unpinned neighbours of the removed points -- only their
//    weights can have changed; a point that is no candidate and keeps its neighbours stays none)
//   (exclusive scan of the live flags: slot[p])
//   row_slot / totals   out_row[c] = slot[row[c]] (a chain's first point is live), the counts, whether the output fits
//
// Scratch per call: 38 bytes per point (the two links, the stored weight, one byte of flags, one of the round's
// decisions, the round stamp that keeps a point from entering a work list twice, two work lists that the scan's flags and
// slots reuse) plus the scan's temporary storage; allocated per call and freed.
#pragma once
#include <stdint.h>

#include "rj_crossings.h"

namespace rj {
namespace simplify {

typedef unsigned __int128 u128;

constexpr uint32_t kNone = 0xFFFFFFFFu;     // no point (np < 2^32)
constexpr u128 kNoWeight = ~(u128) 0;       // the stored weight of a point that is no candidate (a weight is below 2^95)
constexpr uint8_t kLive = 1, kPinned = 2;   // flags of a point
constexpr uint32_t kHashMul = 2654435761u;

struct Counts {  // rj_simplify_counts
  uint64_t n_points, n_removed, n_rounds, n_closed, n_pinned_extra, n_max_round;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;   // the input check's status (crossings::kBad*); not 0: nothing is read further
  uint32_t emit;  // 1: the output fits (n_points <= capacity) and is written
  uint64_t n_list[2];  // the sizes of the two work lists
  uint64_t removed;    // the points that the round removed
  Counts counts;
};

// ---- 1. closed chains and their pins -------------------------------------------------------------------
// the chain [b, e)
RJ_RHD bool is_closed(uint64_t b, uint64_t e, const int64_t* xy) {
  return e >= b + 3 && xy[2 * b] == xy[2 * e - 2] && xy[2 * b + 1] == xy[2 * e - 1];
}
struct Best {
  u128 value;
  uint32_t index;
};
RJ_RHD Best no_best() { return Best{0, kNone}; }
// the greater value, then the lower index: no_best() loses against every point
RJ_RHD bool better(const Best& a, const Best& b) { return a.value != b.value ? a.value > b.value : a.index < b.index; }
RJ_RHD __int128 cross(int64_t ox, int64_t oy, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (__int128) (ax - ox) * (by - oy) - (__int128) (ay - oy) * (bx - ox);
}
RJ_RHD u128 magnitude(__int128 v) { return v < 0 ? (u128) -v : (u128) v; }
// interior point q of a chain that starts at point a: its squared distance from a
RJ_RHD Best far_of(uint64_t a, uint64_t q, const int64_t* xy) {
  const __int128 dx = xy[2 * q] - xy[2 * a], dy = xy[2 * q + 1] - xy[2 * a + 1];
  return Best{(u128) (dx * dx + dy * dy), (uint32_t) q};
}
// ... and |cross(m1 - a, q - a)|
RJ_RHD Best wide_of(uint64_t a, uint64_t m1, uint64_t q, const int64_t* xy) {
  return Best{magnitude(cross(xy[2 * a], xy[2 * a + 1], xy[2 * m1], xy[2 * m1 + 1], xy[2 * q], xy[2 * q + 1])), (uint32_t) q};
}
// a reduction's result is pinned only where its value is not 0
RJ_RHD bool pins(const Best& best) { return best.index != kNone && best.value > 0; }

// ---- 2. links ---------------------------------------------------------------------------------------------
// point p of the chain [b, e)
RJ_RHD bool chain_first(uint64_t p, uint64_t b) { return p == b; }
RJ_RHD bool chain_last(uint64_t p, uint64_t e) { return p + 1 == e; }
RJ_RHD bool chain_end(uint64_t p, uint64_t b, uint64_t e) { return chain_first(p, b) || chain_last(p, e); }
RJ_RHD void links_of(uint64_t p, uint64_t b, uint64_t e, uint32_t* prev, uint32_t* next) {
  *prev = chain_first(p, b) ? kNone : (uint32_t) (p - 1);
  *next = chain_last(p, e) ? kNone : (uint32_t) (p + 1);
}

// ---- 3. weights and keys ------------------------------------------------------------------------------------
RJ_RHD u128 tolerance(uint64_t tol_lo, uint64_t tol_hi) { return ((u128) tol_hi << 64) | tol_lo; }
// p between its live neighbours u and w
RJ_RHD u128 weight(uint64_t u, uint64_t p, uint64_t w, const int64_t* xy) {
  return magnitude(cross(xy[2 * u], xy[2 * u + 1], xy[2 * p], xy[2 * p + 1], xy[2 * w], xy[2 * w + 1]));
}
RJ_RHD bool is_candidate(u128 weight, u128 tol) { return weight <= tol; }
// what the round keeps of point p: its weight where it is a candidate (live, not pinned: it has both neighbours)
RJ_RHD u128 stored_weight(uint64_t p, const int64_t* xy, const uint8_t* flag, const uint32_t* prev, const uint32_t* next, u128 tol) {
  if (flag[p] != kLive) return kNoWeight;
  const u128 w = weight(prev[p], p, next[p], xy);
  return is_candidate(w, tol) ? w : kNoWeight;
}
RJ_RHD uint32_t tie_of(uint64_t p) { return (uint32_t) p * kHashMul; }
RJ_RHD bool key_less(u128 wp, uint64_t p, u128 wq, uint64_t q) { return wp != wq ? wp < wq : tie_of(p) < tie_of(q); }
// candidate p against one neighbour q
RJ_RHD bool beats(uint64_t p, uint64_t q, const u128* stored) { return stored[q] == kNoWeight || key_less(stored[p], p, stored[q], q); }
// does the round remove p: the stored weights of the round, the links as they were when it began
RJ_RHD bool removes(uint64_t p, const u128* stored, const uint32_t* prev, const uint32_t* next) {
  return stored[p] != kNoWeight && beats(p, prev[p], stored) && beats(p, next[p], stored);
}
// removed points are never adjacent: nobody else writes these two links, and nobody reads them before the next round
RJ_RHD void unlink(uint64_t p, uint8_t* flag, uint32_t* prev, uint32_t* next) {
  const uint32_t u = prev[p], w = next[p];
  flag[p] = 0;
  next[u] = w;
  prev[w] = u;
}
// does the next round have to look at q, a neighbour of a removed point
RJ_RHD bool needs_weight(uint64_t q, const uint8_t* flag) { return flag[q] == kLive; }

// ---- 4. slots ---------------------------------------------------------------------------------------------
RJ_RHD uint32_t is_live(uint64_t p, const uint8_t* flag) { return flag[p] & kLive ? 1u : 0u; }
// slot[p]: the live points before p; total: all of them.  A chain's first point is live: its slot starts the chain.
RJ_RHD uint64_t row_slot(uint64_t c, const uint32_t* row, uint64_t nc, const uint32_t* slot, uint64_t total) {
  return c == nc ? total : slot[row[c]];
}
RJ_RHD void totals(uint64_t np, uint64_t total, uint64_t capacity, Counts* counts, uint32_t* emit) {
  counts->n_points = total;
  counts->n_removed = np - total;
  *emit = total <= capacity ? 1 : 0;
}

}  // namespace simplify

#if defined(__HIPCC__)
// what a call reports besides its counts
struct SimplifyReport : StageMs {  // the check; the links and the pins; the first round; the later rounds; the scan and the scatter; all
  static constexpr int kRounds = 10;
  uint64_t n_syncs;                 // host syncs of the call
  uint64_t list_sum, list_max;       // the work lists of the rounds behind the first: their sizes summed, the largest
  uint64_t round_list[kRounds];      // round k: the points it looked at (np in the first round) ...
  float round_ms[kRounds], late_ms;  // ... and the host's time from its first launch to its sync; the rounds from kRounds on, summed
  uint64_t late_list, late_rounds;
};
// rj_map_simplify behind its argument checks, on stream st: *result = the device's Meta with the host's round counts
// filled in.  all_points: every round looks at every point (tests).  Allocates and frees its scratch; synchronises the
// stream once per round and once at the end.
hipError_t map_simplify_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint64_t tol_lo, uint64_t tol_hi,
                               bool all_points, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, simplify::Meta* result,
                               SimplifyReport* report);
#endif

}  // namespace rj
