// rj_within.h -- every edge of a map within a distance of each point (rj_within_query, include/rayjoin_amd.h; the device
// work in rj_within.hip): what GIS users know as dwithin, "Select by distance" or "Generate Near Table (all)".  The
// fourth query over the index of rj_build_lbvh and the first whose result is a CSR: rj_nearest_query with max_dist says
// WHETHER something lies within the distance, this call says WHAT.  Integers only, exact, and fully determined.
//
// DEFINITION   Everything exact is rj_nearest.h's, unchanged: edge e belongs to point i iff
//         nearest::within(nearest::candidate(seg_e, e, P_i), max_dist), that is N <= max_dist^2 D, equality included,
//         for 0 <= max_dist <= 2^48.  A point on an interior vertex of a chain therefore lists both edges k and k + 1:
//         this is a pair list, not a nearest.  The list of a point ascends in eid; record and distance of a pair are
//         nearest::record_of and nearest::dist_of of that candidate.
//
// ORDER   The traversal finds the pairs in an order that depends on the tree, the grid and the order of the points; the
// result must not.  Every pair is therefore a 64-bit KEY, (point number << 32) | eid, appended to one array in any
// order and then sorted over the bits that are in use: ascending keys are ascending eids inside each point, and the
// boundaries between the points are the exclusive scan of the per-point counts, which the traversal writes beside the
// keys.  The 40-byte records are never carried through the sort: they are recomputed from the sorted keys.
//
// FILTER   max_dist is fixed, so for an interior foot the 256-bit compare of within() has a filter in double in front of
// it (in_or_out).  It has closer()'s property: it never decides a pair that the exact test would decide otherwise, so
// within_filtered(..., false) is the same function without it.
//
// PRUNING   The per-point prune is rj_nearest.h's box_lb2 / admits with the fixed bound ub2_of_max_dist(max_dist).  In
// front of it sits a wave-uniform reject against the box of the group's cells (group_lb2): a lower bound of every
// point's lower bound, so what it dismisses every lane would dismiss.  It is never the only test: on shuffled points the
// group's box is the whole map and it dismisses nothing.
//
// SCRATCH of a call, allocated and freed by it: 12 bytes per point (the count and the scanned offset) + 8 bytes per pair
// of capacity (the unsorted keys) + 8 bytes per pair found (the sorted keys) + rocPRIM's temporaries of one scan over
// the points and one radix sort over the pairs found.  The counting call takes the per-point part only.
//
// One function per element that rj_within.hip runs on the device and tests/hosttwin/within_twin.cc as a brute force over
// all edges (a test-only twin, never a fallback):
//
//   pair_key / key_point / key_eid / key_bits    the key and the bits the sort looks at
//   in_or_out / within_filtered                  the filter and the test behind it
//   group_gap / group_lb2                        the wave-uniform reject
#pragma once
#include "rj_nearest.h"
#if defined(__HIPCC__)
#include "rj_pipeline.h"
#endif

namespace rj {
namespace within {

constexpr uint64_t kMaxPoints = 1ull << 32;  // n and pair_capacity stay below it: both halves of a key are 32 bits

struct Counts {  // rj_within_counts
  uint64_t n_pairs, n_points_hit, max_per_point;
};

// ---- 1. the key ------------------------------------------------------------------------------------------------------------
RJ_HD uint64_t pair_key(uint32_t point, uint32_t eid) { return ((uint64_t) point << 32) | eid; }
RJ_HD uint32_t key_point(uint64_t key) { return (uint32_t) (key >> 32); }
RJ_HD uint32_t key_eid(uint64_t key) { return (uint32_t) key; }
// the low bits of a key that differ among n points: all 32 of the eid and those of the largest point number, n - 1
RJ_HD int key_bits(uint64_t n) {
  int b = 0;
  for (uint64_t v = n > 1 ? n - 1 : 0; v; v >>= 1) b++;
  return 32 + b;
}

// ---- 2. the filter ---------------------------------------------------------------------------------------------------------
// max_dist^2 in double: max_dist <= 2^48 converts exactly, the product rounds once: within 2^-53 relative.
RJ_HD double approx_m2(int64_t max_dist) { return (double) max_dist * (double) max_dist; }
// 1: certainly within, -1: certainly not, 0: the exact test decides.  d2 = approx_d2(c) is within e = 2^-50 relative of
// N / D (rj_nearest.h) and m2 within 2^-53 of max_dist^2.  d2 < m2 (1 - 4 e) gives N / D (1 - e) < max_dist^2 (1 + e / 8)
// (1 - 4 e), and the right side is below max_dist^2 (1 - e): N / D < max_dist^2.  d2 > m2 (1 + 4 e) gives N / D (1 + e) >
// max_dist^2 (1 - e / 8)(1 + 4 e) > max_dist^2 (1 + e): N / D > max_dist^2.  The rounding of the products m2 kIn and
// m2 kOut is 2^-53 each, far inside the 2 e to spare.  Equality, and m2 = 0 with d2 = 0, are left to the exact test;
// m2 = 0 with d2 > 0 is out, rightly: approx_d2 is 0 exactly when N is.
RJ_HD int in_or_out(double d2, double m2) {
  constexpr double kIn = 1.0 - 0x1p-48;
  constexpr double kOut = 1.0 + 0x1p-48;
  if (d2 < m2 * kIn) return 1;
  if (d2 > m2 * kOut) return -1;
  return 0;
}
// nearest::within, with the filter in front of the wide compare of an interior foot (an end is one 128-bit compare: no
// filter pays there).  m2 = approx_m2(max_dist).
RJ_HD bool within_filtered(const nearest::Cand& c, int64_t max_dist, double m2, bool filter) {
  if (filter && c.where == nearest::kInterior) {
    const int f = in_or_out(nearest::approx_d2(c), m2);
    if (f) return f > 0;
  }
  return nearest::within(c, max_dist);
}

// ---- 3. the wave-uniform reject --------------------------------------------------------------------------------------------
// nearest::gap for a query that is itself a range of cells [q0, q1]: the cells that certainly lie between it and [lo, hi]
RJ_HD uint32_t group_gap(int32_t lo, int32_t hi, int32_t q0, int32_t q1) {
  const int32_t below = lo - q1, above = q0 - hi;
  const int32_t g = below > above ? below : above;
  return g > 1 ? (uint32_t) (g - 1) : 0u;
}
// a lower bound of nearest::box_lb2(box, q) for every cell q inside the group's box [gx0, gx1] x [gy0, gy1]: per axis the
// gap to the nearest cell of the group is the smallest gap of any of its cells
RJ_HD uint64_t group_lb2(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t gx0, int32_t gy0, int32_t gx1, int32_t gy1) {
  const uint32_t gx = group_gap(x0, x1, gx0, gx1), gy = group_gap(y0, y1, gy0, gy1);
  return (uint64_t) gx * gx + (uint64_t) gy * gy;
}

}  // namespace within

#if defined(__HIPCC__)
// what the device pipeline takes (rj_within.hip); filled by rj_within_query
struct WithinArgs {
  DeviceBvh bvh;
  const Seg* seg;         // the base map's segments in eid order: what the outputs are recomputed from
  const int64_t* pts;     // [n][2]
  uint64_t n;
  const uint32_t* order;  // null, or a permutation of [0, n): the order the points are taken in (any order gives the same result)
  int64_t max_dist;       // in [0, 2^48]
  uint64_t capacity;      // pairs there is room for (0: the counting call)
  uint64_t* offsets;      // [n + 1] or null
  uint32_t* eid;          // [capacity]
  nearest::Near* rec;     // [capacity] or null
  double* dist;           // [capacity] or null
  uint32_t* fault;        // the handle's fault words as the device sees them
  unsigned long long* stats;  // null, or [16]: [0] .. [3] as k_nearest's, [4] pairs appended
  int stack_cap;          // the instrumented kernel only: a lower stack capacity (tests of the fault path)
};
struct WithinResult {
  within::Counts counts;
  uint64_t appended;  // what the traversal appended (filling calls): equal to n_pairs, or the call is RJ_E_INTERNAL
  bool emitted;       // eid / rec / dist were written (capacity > 0 and n_pairs <= capacity)
};
// The whole call behind the ordering of the points: marks ev[1] in front of the traversal, ev[2] behind it and ev[3] behind the
// outputs; one host sync behind the scan (the number of pairs sizes the sort) and one at the end.  Any grid gives the same
// result (blocks <= 0: by size).  The scratch is gone when it returns.
hipError_t within_device(hipStream_t st, const WithinArgs& a, bool stats, int blocks, int cus, StageEvents* ev, WithinResult* result);
#endif

}  // namespace rj
