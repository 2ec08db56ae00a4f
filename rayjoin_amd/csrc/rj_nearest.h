// rj_nearest.h -- the nearest edge of a map for every point (rj_nearest_query, include/rayjoin_amd.h; the traversal in
// rj_nearest.hip): what GIS users know as Near, sjoin_nearest or "join within a distance".  The third query over the
// index of rj_build_lbvh, beside "which edge lies above a point" (rj_pip_query) and "which edges cross" (rj_lsi_query).
// Integers only, exact, and fully determined: no tuning choice below can change a result.
//
// DEFINITION   Coordinates are the scaled int64 of the library, in [-2^46, 2^46).  For a point P and the edge (A, B)
//         with eid e:   l = |B - A|^2 < 2^95,   dot = (P - A) . (B - A), |dot| < 2^95.
//             dot <= 0        where = 1 (first end; also A == B)     d^2 = |P - A|^2          (an integer < 2^95)
//             dot >= l        where = 2 (second end)                 d^2 = |P - B|^2
//             0 < dot < l     where = 0 (interior)                   d^2 = c^2 / l,  c = (B - A) x (P - A), |c| < 2^95
//         So d^2 = N / D with N < 2^190 and D < 2^95 (D = 1 at an end).  The nearest edge is the one with the smallest
//         N / D; ties go to the SMALLER eid.  Ties are the common case: a point nearest to an interior vertex of a chain
//         ties between where = 2 of edge k and where = 1 of edge k + 1, and the answer is k.
// max_dist   negative: unlimited.  Otherwise an edge qualifies iff N <= max_dist^2 D, exactly, equality included;
//         max_dist <= 2^48 (kMaxDist: nothing in the domain is farther apart than 2^47.5).
// RECORD  where = 0: num = the SIGNED cross product c, den = l (d^2 = num^2 / den; the sign of num is the side of the edge
//         the point lies on: positive to the left of A -> B).  where = 1, 2: num = d^2, den = 1.  A miss: eid = kMissEid
//         and everything else 0.  Nothing is divided.
//
// COMPARING   N1 / D1 against N2 / D2 is N1 D2 against N2 D1: up to 285 bits.  W5 is a fixed-width unsigned integer of
// five 64-bit limbs with the three operations that this takes (w5_mul, w5_mul3, w5_cmp).  closer() first lets a filter
// in double settle the pairs it can separate (see approx_d2 for its error bound), and two end-point candidates compare
// their integers directly; only the rest pays for the wide product.  The filter never decides a pair that the wide
// compare would decide otherwise, so no result depends on it (closer(..., false) is the same function without it).
//
// PRUNING   The boxes of the index are quantised: cell_of(v) = (v + 2^46) >> 16.  For a point in cell (qx, qy) and a box
// [x0, x1] x [y0, y1] of cells let gx = max(x0 - qx, qx - x1, 0), gy likewise.  The point lies anywhere in its cell
// and the content anywhere in the cells of the box, so for gx >= 1 the true distance along x is at least
// (gx - 1) 2^16 + 1 -- one cell less than gx, because the two may sit at opposite ends of their cells -- and for
// gx = 0 at least 0.  With gap() = (g - 1)+ and box_lb2() = gap(x)^2 + gap(y)^2 (< 2^63: uint64_t):
//         d^2 (P, anything in the box) >= 2^32 box_lb2,   and > where box_lb2 > 0.
// ub2_of() gives an upper bound of a candidate's d^2 in the same unit, rounded up to an integer: d^2 <= 2^32 ub2.
// admits(ub2, lb2) = ub2 >= lb2 keeps a box; a dismissed box has lb2 >= ub2 + 1, so everything in it is strictly farther
// than the candidate held.  Equality keeps the box: an equally distant edge with a smaller eid may be inside -- at
// lb2 = ub2 = 0, a point on a vertex that several chains share, that is the rule and not the exception.
//
// Every step is one function per element that rj_nearest.hip runs in its traversal and tests/hosttwin/nearest_twin.cc
// runs as a brute force over all edges (a test-only twin, never a fallback):
//
//   cell_of / gap / box_lb2 / admits    the prune
//   candidate                           the case split: (edge, point) -> Cand
//   approx_d2 / closer                  the order of two candidates: the filter, the end-point shortcut, the wide compare
//   within                              the max_dist test
//   ub2_of / ub2_of_max_dist            the bound that a held candidate, or max_dist alone, gives the prune
//   record_of / dist_of                 the outputs
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "rj_predicates.h"

namespace rj {
namespace nearest {

constexpr uint32_t kMissEid = 0xFFFFFFFFu;          // RJ_MISS_EID
constexpr int64_t kMaxDist = (int64_t) 1 << 48;     // the largest max_dist
constexpr int kCellShift = 16;                      // kQuantShift
constexpr int64_t kHalfRange = (int64_t) 1 << 46;   // kCoordOffset
constexpr uint64_t kNoBound = ~0ull;                // ub2 of "no candidate, no max_dist": admits every box
constexpr uint32_t kInterior = 0, kFirstEnd = 1, kSecondEnd = 2;

struct Near {  // rj_near (40 bytes)
  uint32_t eid, where;
  uint64_t num_lo;
  int64_t num_hi;
  uint64_t den_lo, den_hi;
};
// a candidate: the edge, the case, and d^2 = num^2 / den (interior; num signed) or num / 1 (an end)
struct Cand {
  uint32_t eid, where;
  i128 num;
  u128 den;
};

// ---- 1. five limbs ---------------------------------------------------------------------------------------------------------
struct W5 {  // w[0] the lowest limb
  uint64_t w[5];
};
// a b, all 256 bits of it (w[4] = 0)
RJ_HD W5 w5_mul(u128 a, u128 b) {
  const uint64_t a0 = (uint64_t) a, a1 = (uint64_t) (a >> 64), b0 = (uint64_t) b, b1 = (uint64_t) (b >> 64);
  const u128 p00 = (u128) a0 * b0, p01 = (u128) a0 * b1, p10 = (u128) a1 * b0, p11 = (u128) a1 * b1;
  W5 r;
  r.w[0] = (uint64_t) p00;
  u128 t = (p00 >> 64) + (uint64_t) p01 + (uint64_t) p10;  // (three terms below 2^64: no wrap)
  r.w[1] = (uint64_t) t;
  t = (t >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t) p11;
  r.w[2] = (uint64_t) t;
  r.w[3] = (uint64_t) ((t >> 64) + (p11 >> 64));
  r.w[4] = 0;
  return r;
}
// a b for a < 2^192 (w[3] = w[4] = 0 are not looked at): all 320 bits
RJ_HD W5 w5_mul3(const W5& a, u128 b) {
  const uint64_t b0 = (uint64_t) b, b1 = (uint64_t) (b >> 64);
  const u128 p00 = (u128) a.w[0] * b0, p10 = (u128) a.w[1] * b0, p20 = (u128) a.w[2] * b0;
  const u128 p01 = (u128) a.w[0] * b1, p11 = (u128) a.w[1] * b1, p21 = (u128) a.w[2] * b1;
  W5 r;
  r.w[0] = (uint64_t) p00;
  u128 t = (p00 >> 64) + (uint64_t) p10 + (uint64_t) p01;
  r.w[1] = (uint64_t) t;
  t = (t >> 64) + (p10 >> 64) + (p01 >> 64) + (uint64_t) p20 + (uint64_t) p11;  // (five terms below 2^64)
  r.w[2] = (uint64_t) t;
  t = (t >> 64) + (p20 >> 64) + (p11 >> 64) + (uint64_t) p21;
  r.w[3] = (uint64_t) t;
  r.w[4] = (uint64_t) ((t >> 64) + (p21 >> 64));
  return r;
}
// -1, 0, 1: a below, equal to, above b
RJ_HD int limb_cmp(uint64_t a, uint64_t b, int lower) { return a < b ? -1 : (a > b ? 1 : lower); }
RJ_HD int w5_cmp(const W5& a, const W5& b) {  // (from the lowest limb: the highest difference has the last word)
  return limb_cmp(a.w[4], b.w[4], limb_cmp(a.w[3], b.w[3], limb_cmp(a.w[2], b.w[2], limb_cmp(a.w[1], b.w[1], limb_cmp(a.w[0], b.w[0], 0)))));
}

// ---- 2. the prune ----------------------------------------------------------------------------------------------------------
RJ_HD int32_t cell_of(int64_t v) { return (int32_t) ((v + kHalfRange) >> kCellShift); }
// cells that certainly lie between cell q and the cells [lo, hi] of a box that is not empty: one less than the difference of
// the cell numbers (cells are 31-bit, lo <= hi: every difference fits 32 bits)
RJ_HD uint32_t gap(int32_t lo, int32_t hi, int32_t q) {
  const int32_t below = lo - q, above = q - hi;
  const int32_t g = below > above ? below : above;
  return g > 1 ? (uint32_t) (g - 1) : 0u;
}
// the lower bound of the header: d^2 >= 2^32 box_lb2 for everything in the box, and > where it is not 0
RJ_HD uint64_t box_lb2(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t qx, int32_t qy) {
  const uint32_t gx = gap(x0, x1, qx), gy = gap(y0, y1, qy);
  return (uint64_t) gx * gx + (uint64_t) gy * gy;
}
// a box with this lower bound may hold something as near as, or nearer than, a candidate with this upper bound
RJ_HD bool admits(uint64_t ub2, uint64_t lb2) { return ub2 >= lb2; }
// padding slots and the nodes above them have the empty box {INT_MAX, INT_MAX, -1, -1}: never a candidate
RJ_HD bool box_empty(int32_t x0, int32_t x1) { return x1 < x0; }

// ---- 3. the case split -----------------------------------------------------------------------------------------------------
RJ_HD Cand candidate(const Seg& s, uint32_t eid, int64_t px, int64_t py) {
  const int64_t dx = s.x2 - s.x1, dy = s.y2 - s.y1;  // (every difference below 2^47 in magnitude)
  const int64_t ex = px - s.x1, ey = py - s.y1;
  const i128 dot = (i128) ex * dx + (i128) ey * dy;
  const i128 l = (i128) dx * dx + (i128) dy * dy;
  if (dot <= 0) return Cand{eid, kFirstEnd, (i128) ex * ex + (i128) ey * ey, 1};
  if (dot >= l) {
    const int64_t fx = px - s.x2, fy = py - s.y2;
    return Cand{eid, kSecondEnd, (i128) fx * fx + (i128) fy * fy, 1};
  }
  return Cand{eid, kInterior, (i128) dx * ey - (i128) dy * ex, (u128) l};
}
RJ_HD u128 magnitude(i128 v) { return v < 0 ? (u128) 0 - (u128) v : (u128) v; }
// N of the header in three limbs (w[3] = w[4] = 0)
RJ_HD W5 numerator(const Cand& c) {
  if (c.where != kInterior) return W5{{(uint64_t) c.num, (uint64_t) ((u128) c.num >> 64), 0, 0, 0}};
  const u128 m = magnitude(c.num);
  return w5_mul(m, m);  // (|c| < 2^95: below 2^190)
}

// ---- 4. the order of two candidates ----------------------------------------------------------------------------------------
// d^2 in double, within 2^-50 relative of N / D: an end is one conversion (2^-53); the interior is two conversions,
// one multiply and one divide -- (1 + e)^2 for the conversion of |c|, and one e each for the product, the conversion of l
// and the quotient: 5 e + O(e^2) < 2^-50 with e = 2^-53.  Nothing overflows or underflows (1 / 2^95 <= d^2 < 2^96 or 0),
// and the value is 0 exactly when d^2 is.
RJ_HD double approx_d2(const Cand& c) {
  if (c.where != kInterior) return i128_to_double(c.num);
  const double n = i128_to_double((i128) magnitude(c.num));
  return n * n / i128_to_double((i128) c.den);
}
// N_a D_b against N_b D_a: -1, 0, 1
RJ_HD int compare_exact(const Cand& a, const Cand& b) {
  if (a.where != kInterior && b.where != kInterior)  // (both denominators are 1: the integers themselves)
    return a.num < b.num ? -1 : (a.num > b.num ? 1 : 0);
  return w5_cmp(w5_mul3(numerator(a), b.den), w5_mul3(numerator(b), a.den));
}
// a is the better answer than b: nearer, or as near with the smaller eid.  da, db = approx_d2 of the two.  With the
// filter: a' <= a (1 + e) and b' >= b (1 - e) for e = 2^-50, so a' < b' (1 - 4 e) gives a (1 - e) < b (1 + e)(1 - 4 e),
// that is a < b (the product on the right is below 1 - e; the rounding of b' (1 - 4 e) itself is 2^-53, far inside the
// 2 e to spare).  What it cannot separate, equal distances among them, goes to compare_exact.
RJ_HD bool closer(const Cand& a, double da, const Cand& b, double db, bool filter) {
  constexpr double kKeep = 1.0 - 0x1p-48;
  if (filter && da < db * kKeep) return true;
  if (filter && db < da * kKeep) return false;
  const int c = compare_exact(a, b);
  return c < 0 || (c == 0 && a.eid < b.eid);
}
// N <= max_dist^2 D for max_dist in [0, kMaxDist] (max_dist^2 <= 2^96, times D below 2^191)
RJ_HD bool within(const Cand& c, int64_t max_dist) {
  const u128 m2 = (u128) (uint64_t) max_dist * (uint64_t) max_dist;
  if (c.where != kInterior) return (u128) c.num <= m2;
  return w5_cmp(numerator(c), w5_mul(m2, c.den)) <= 0;
}

// ---- 5. the bound a held candidate gives the prune -------------------------------------------------------------------------
// ub2 = an integer with d^2 <= 2^32 ub2, and 0 exactly when d^2 is 0 (a box that touches the point's cell must then still be
// admitted, and is: its lower bound is 0 too).  An end: the integer, rounded up.  The interior: approx_d2 is at most 2^-50
// below d^2, so 1 + 2^-40 times it lies above (and its own rounding cannot bring it back under); d^2 < 2^95 keeps the
// result in 64 bits.
RJ_HD uint64_t ub2_of(const Cand& c, double d2) {
  if (c.where != kInterior) return (uint64_t) (((u128) c.num + 0xFFFFFFFFu) >> 32);
  return d2 == 0.0 ? 0 : (uint64_t) (d2 * (1.0 + 0x1p-40) * 0x1p-32) + 1;
}
// the bound before the first candidate: no edge farther than max_dist qualifies
RJ_HD uint64_t ub2_of_max_dist(int64_t max_dist) {
  if (max_dist < 0) return kNoBound;
  const u128 u = ((u128) (uint64_t) max_dist * (uint64_t) max_dist + 0xFFFFFFFFu) >> 32;  // (<= 2^64)
  return u > (u128) kNoBound ? kNoBound : (uint64_t) u;
}

// ---- 6. the outputs --------------------------------------------------------------------------------------------------------
RJ_HD Near record_miss() { return Near{kMissEid, 0, 0, 0, 0, 0}; }
RJ_HD Near record_of(const Cand& c) {
  return Near{c.eid, c.where, (uint64_t) c.num, (int64_t) (c.num >> 64), (uint64_t) c.den, (uint64_t) (c.den >> 64)};
}
// sqrt(d^2) in double: separate conversions, one multiply, one divide, one square root (-ffp-contract=off), within 2^-50
// relative of the true distance -- the 5 e of approx_d2 are halved by the root, which adds its own: 3.5 e < 2^-50 / 2.
RJ_HD double dist_of(const Cand& c) { return sqrt(approx_d2(c)); }
RJ_HD double dist_miss() { return (double) INFINITY; }

}  // namespace nearest

#if defined(__HIPCC__)
}  // namespace rj
#include "rj_device.h"
namespace rj {
// what the traversal takes (rj_nearest.hip); filled by rj_nearest_query
struct NearestArgs {
  DeviceBvh bvh;
  const int64_t* pts;     // [n][2]
  uint64_t n;
  const uint32_t* order;  // null, or a permutation of [0, n): the order the points are taken in (any order gives the same result)
  int64_t max_dist;       // negative: unlimited
  uint32_t* eid;          // [n]
  nearest::Near* rec;     // [n] or null
  double* dist;           // [n] or null
  uint32_t* fault;        // the handle's fault words as the device sees them
  unsigned long long* stats;  // null, or [16]: [0] leaf blocks visited, summed over the points (the lanes that admit the block), [1] candidates evaluated exactly, [2] nodes expanded (per wave), [3] leaf blocks loaded (per wave)
  int stack_cap;          // the instrumented kernel only: a lower stack capacity (tests of the fault path)
};
// any grid gives the same result (blocks <= 0: by size).  Not synchronised.
hipError_t launch_nearest(hipStream_t st, const NearestArgs& a, bool stats, int blocks, int cus);
#endif

}  // namespace rj
