// rj_knearest.h -- the k nearest edges of a map for every point (rj_knearest_query, include/rayjoin_amd.h; the traversal
// in rj_knearest.hip): the closest-count field of Near and Generate Near Table, the candidate list of map matching.  The
// sixth query over the index of rj_build_lbvh.  Integers only, exact, and fully determined, on the functions of
// rj_nearest.h: no tuning choice below can change a result.
//
// DEFINITION   For a point P order ALL edges of the base map by (d^2, eid) ascending: d^2 = N / D exactly as in
//         rj_nearest.h (candidate), compared exactly (compare_exact / closer), equal distances to the SMALLER eid.  With
//         max_dist >= 0 only edges with N <= max_dist^2 D qualify (within).  The answer is the first
//         min(k, number of qualifying edges) entries of that order, in that order; 1 <= k <= kMaxK.  k = 1 is
//         rj_nearest_query.
//
// THE LIST   A point holds at most k candidates, UNORDERED, in `count` slots of a List: six 64-bit words per slot (the
// double approx_d2, then the candidate), word p of slot s at q[(6 s + p) stride].  On the device the list is a column of
// the wave's slab in global memory, stride = 64 lanes (slot-major: the lanes of a wave touch neighbouring addresses);
// the host twin uses stride 1.  Beside it, in registers (Held): the number held, and -- once the list is full -- of the
// WORST candidate held (the last of the held in the order above) its slot, its approx_d2 and the bound it gives.
//   insert     below k: the candidate takes the next slot.  At k: it enters iff it is closer() than the worst, overwrites
//              the worst's slot, and one pass over the k slots (worst_of) finds the new worst.
//   worst_of / first_of   one pass each over the doubles.  They settle what they can separate (filter_order: closer()'s
//              filter, the same margin); only what they cannot -- equal distances among them -- loads the two candidates
//              and takes compare_exact, then the eid (slot_before).  The filter never decides a pair that the exact compare
//              would decide otherwise, so no result depends on it (filter = false is the same function without it).
//   bound_of   the prune's bound: below k held, what max_dist alone gives (ub2_of_max_dist); at k, ub2_of the worst (never
//              above the former).  A box is dismissed only when its box_lb2 EXCEEDS that (admits of rj_nearest.h keeps
//              equality: an equally distant edge with a smaller eid may lie inside), so everything in it is strictly
//              farther than k edges already held.  The bound only ever falls.
//   order_step the final order, a selection: step j moves the first of the slots [j, count) out and the content of slot j
//              into its place.  At most k steps of at most k slots.
// The eids of a list are distinct -- no edge may be offered twice (rj_knearest.hip: DUPLICATES) -- so the order of any two
// held candidates is strict and the answer is one set in one order, whatever order the edges were offered in.
//
// Every step is one function per element that rj_knearest.hip runs in its traversal and tests/hosttwin/knearest_twin.cc
// runs as a brute force over all edges (a test-only twin, never a fallback).
#pragma once
#include "rj_nearest.h"

namespace rj {
namespace knearest {

using namespace nearest;

constexpr uint32_t kMaxK = 32;         // RJ_KNEAREST_MAX_K
constexpr uint32_t kSlotWords = 6;     // 64-bit words of a slot: approx_d2, eid | where << 32, num (2), den (2)

struct List {
  uint64_t* q;      // word 0 of slot 0
  uint64_t stride;  // words between two consecutive words of the list (64 on the device: the lanes of the wave lie between)
};
// words of a list of k slots at stride 1; a wave's slab is 64 of them
RJ_HD uint64_t list_words(uint32_t k) { return (uint64_t) k * kSlotWords; }

RJ_HD double bits_to_double(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, sizeof(d));
  return d;
}
RJ_HD uint64_t double_to_bits(double d) {
  uint64_t b;
  __builtin_memcpy(&b, &d, sizeof(b));
  return b;
}
RJ_HD double slot_d2(const List& L, uint32_t s) { return bits_to_double(L.q[(uint64_t) s * kSlotWords * L.stride]); }
RJ_HD Cand slot_cand(const List& L, uint32_t s) {
  const uint64_t* w = L.q + (uint64_t) s * kSlotWords * L.stride;
  const uint64_t ew = w[L.stride], n0 = w[2 * L.stride], n1 = w[3 * L.stride], d0 = w[4 * L.stride], d1 = w[5 * L.stride];
  return Cand{(uint32_t) ew, (uint32_t) (ew >> 32), (i128) (((u128) n1 << 64) | n0), ((u128) d1 << 64) | d0};
}
RJ_HD void slot_put(const List& L, uint32_t s, const Cand& c, double d2) {
  uint64_t* w = L.q + (uint64_t) s * kSlotWords * L.stride;
  w[0] = double_to_bits(d2);
  w[L.stride] = (uint64_t) c.eid | ((uint64_t) c.where << 32);
  w[2 * L.stride] = (uint64_t) c.num;
  w[3 * L.stride] = (uint64_t) ((u128) c.num >> 64);
  w[4 * L.stride] = (uint64_t) c.den;
  w[5 * L.stride] = (uint64_t) (c.den >> 64);
}

// what a point keeps beside its list
struct Held {
  uint32_t count;   // slots [0, count) are live: nothing else says so
  uint32_t slot;    // count == k: the slot of the worst,
  double worst_d2;  // ... its approx_d2 (the candidate itself stays in its slot: loaded when the doubles cannot tell)
  uint64_t ub2;     // ... and ub2_of it
};
RJ_HD Held held_none() { return Held{0, 0, 0.0, kNoBound}; }

// closer()'s filter alone: -1 the first is certainly nearer, 1 the second is, 0 the doubles cannot tell (rj_nearest.h:
// closer, the same margin and the same argument)
RJ_HD int filter_order(double da, double db) {
  constexpr double kKeep = 1.0 - 0x1p-48;
  return da < db * kKeep ? -1 : (db < da * kKeep ? 1 : 0);
}
// slot a comes before slot b in the order of the definition (da, db: their approx_d2)
RJ_HD bool slot_before(const List& L, uint32_t a, double da, uint32_t b, double db, bool filter) {
  const int f = filter ? filter_order(da, db) : 0;
  return f ? f < 0 : closer(slot_cand(L, a), da, slot_cand(L, b), db, false);
}

// The worst of the slots [0, count), count > 0: the one that none comes behind -- the farthest, the larger eid among
// equally distant ones -- with its approx_d2 and the bound it gives.
RJ_HD void worst_of(const List& L, uint32_t count, bool filter, Held& H) {
  uint32_t ws = 0;
  double dw = slot_d2(L, 0);
  for (uint32_t s = 1; s < count; s++) {
    const double ds = slot_d2(L, s);
    if (slot_before(L, ws, dw, s, ds, filter)) ws = s, dw = ds;
  }
  H.slot = ws, H.worst_d2 = dw, H.ub2 = ub2_of(slot_cand(L, ws), dw);
}

// The first of the slots [from, count), from < count, in the order of the definition: its slot.
RJ_HD uint32_t first_of(const List& L, uint32_t from, uint32_t count, bool filter) {
  uint32_t bs = from;
  double db = slot_d2(L, from);
  for (uint32_t s = from + 1; s < count; s++) {
    const double ds = slot_d2(L, s);
    if (slot_before(L, s, ds, bs, db, filter)) bs = s, db = ds;
  }
  return bs;
}

// A qualifying candidate (within() has passed) is offered to the list of at most k: true iff it entered.
RJ_HD bool insert(const List& L, Held& H, uint32_t k, const Cand& c, double d2, bool filter) {
  if (H.count < k) {
    slot_put(L, H.count, c, d2);
    H.count++;
    if (H.count == k) worst_of(L, k, filter, H);
    return true;
  }
  const int f = filter ? filter_order(d2, H.worst_d2) : 0;
  if (f > 0 || (f == 0 && !closer(c, d2, slot_cand(L, H.slot), H.worst_d2, false))) return false;
  slot_put(L, H.slot, c, d2);
  worst_of(L, k, filter, H);
  return true;
}

// The bound that the list gives the prune; base = ub2_of_max_dist(max_dist).
RJ_HD uint64_t bound_of(const Held& H, uint32_t k, uint64_t base) { return H.count < k || base < H.ub2 ? base : H.ub2; }

// Step j < count of the final order: -> the (j + 1)-th nearest of the list.  The slots below j are dead afterwards, the
// slots [j + 1, count) hold what is left.
RJ_HD Cand order_step(const List& L, uint32_t j, uint32_t count, bool filter) {
  const uint32_t s = first_of(L, j, count, filter);
  const Cand first = slot_cand(L, s);
  if (s != j) slot_put(L, s, slot_cand(L, j), slot_d2(L, j));
  return first;
}

}  // namespace knearest

#if defined(__HIPCC__)
// what the traversal takes (rj_knearest.hip); filled by rj_knearest_query
struct KNearestArgs {
  DeviceBvh bvh;
  const int64_t* pts;     // [n][2]
  uint64_t n;
  const uint32_t* order;  // null, or a permutation of [0, n): the order the points are taken in (any order gives the same result)
  uint32_t k;             // 1 .. kMaxK
  int64_t max_dist;       // negative: unlimited
  uint32_t* count;        // [n] or null
  uint32_t* eid;          // [n][k]
  nearest::Near* rec;     // [n][k] or null
  double* dist;           // [n][k] or null
  uint64_t* slab;         // knearest_slab_bytes(k, grid): the lists, one slab of 64 per wave of the grid
  uint32_t* fault;        // the handle's fault words as the device sees them
  unsigned long long* stats;  // null, or [16]: [0] .. [3] as NearestArgs::stats, [4] candidates that entered a list
  int stack_cap;          // the instrumented kernel only: a lower stack capacity (tests of the fault path)
};
// the grid of the traversal over n > 0 points (blocks <= 0: by size -- the blocks that are resident at once, the
// grid-stride loop takes the rest: the scratch goes by the grid) and the bytes of its slabs
dim3 knearest_grid(uint64_t n, int blocks, int cus);
uint64_t knearest_slab_bytes(uint32_t k, dim3 grid);
// any grid gives the same result.  Not synchronised.
hipError_t launch_knearest(hipStream_t st, const KNearestArgs& a, dim3 grid, bool stats);
#endif

}  // namespace rj
