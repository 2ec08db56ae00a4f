// rj_eliminate.h -- merging sliver faces into a neighbour (rj_map_eliminate, include/rayjoin_amd.h; kernels in
// rj_eliminate.hip): what GIS users know as Eliminate.  A face whose area is at most a tolerance joins the neighbour it
// shares the longest border with.  Integers only, exact, and fully determined: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1], left[nc], right[nc]: a labelled chain map with the contract, the checks and the size
//         limits of rj_map_rings (rj_rings.h; a chain may have a single point).  Labels are any int32.  tol: an unsigned
//         128-bit number, twice an area in scaled units^2 (the unit of rj_map_simplify's tol and of every area2).
// FACE    a label value other than 0 that occurs in left or right: a multi-part polygon with one label is ONE face (faces
//         from geometry: rj_map_faces first).  Faces are numbered by ascending (uint32_t) label, and every "smaller label"
//         below means that unsigned order.
// SUMS    of chain c over its edges p_i -> p_i+1:  S(c) = sum of cross(p_i, p_i+1), an int128 (a term is below 2^93, the
//         total below 2^125);  L(c) = sum of floor(sqrt(dx^2 + dy^2)), the exact integer square root of a value below
//         2^95 per edge, an unsigned 128-bit total (below 2^80).  No floating point result reaches an output: isqrt's
//         double estimate is corrected by integer compares.
// AREA    area2(f) = sum of S(c) over left[c] == f  -  sum of S(c) over right[c] == f: the rule of rj_overlay_faces, exact
//         for consistent labels; holes subtract themselves and no rings are needed.  f is a SLIVER when
//         0 <= area2(f) <= tol.  area2(f) < 0 is NEGATIVE (inconsistent labels): never a sliver, it may be a target.
// NEIGHBOURS   faces f != g, both not 0, are neighbours when some chain has {left, right} = {f, g};  w(f, g) = the sum of
//         L(c) over those chains.  A pair with w = 0 is still a pair.  Face 0 is never a neighbour, never a sliver, never a
//         target.  Chains with left == right contribute nothing.
// CHOICE  best(f) of a sliver = the neighbour g with the largest w(f, g); ties go to the smaller min(f, g), then to the
//         smaller max(f, g).  A sliver without a neighbour is an ISLAND and stays.  Every other face has no best (its
//         record holds its own label there).  The order on unordered pairs is strict, so the graph f -> best(f) can only
//         have cycles of length 2 (the Boruvka argument).
// MUTUAL  f and g with best(f) = g and best(g) = f: the one with the larger area2 stays as a root, a tie goes to the
//         smaller label; the other points at it.
// TARGET  target(f) = the root reached by following best: roots are the non-slivers, the islands and the winners of mutual
//         pairs.  Pointer jumping, at most kMaxRounds rounds.  target(0) = 0.  ONE CALL IS ONE ROUND: a merged group may
//         still be at most tol; the caller repeats the call.
// OUTPUT  out_left[c] = target(left[c]), out_right[c] = target(right[c]); record k of the k-th face: its label, target,
//         best, flags, its own area2.  Under kDrop a chain is dropped exactly when its input labels differ and its output
//         labels are equal (bridges and dangles that came with left == right stay); the kept chains are written in input
//         order with their points, origin[k] = the input chain of output chain k.  Chains are NOT re-joined at vertices
//         that drop to degree 2: that is rj_map_dissolve with RJ_DISS_KEEP_EQUAL (rj_dissolve.h).
//
// Every step is one function per element that rj_eliminate.hip runs as a kernel and tests/hosttwin/eliminate_twin.cc runs
// as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate (rj_rings.h)   the input check: the largest code met is the status
//   edge_cross / edge_length / isqrt   per edge: its two terms; summed per chain (any order: integer sums commute)
//   side_key / side_sum   per chain side i = 2 c + s (s = 0 left, 1 right): the sort key of its label, +S(c) or -S(c)
//   (sort by key, unique keys, sum by key: the labels ascending with their areas; label 0, if any, is the last key)
//   count_faces / face_index / label_of   the number of faces; the face of a label (a binary search)
//   is_sliver / is_negative   per face
//   directed_key   per chain side: (f << 32) | g for a chain that separates faces f (this side) and g, kNoPair otherwise
//   (sort by key, unique keys, sum of L(c) by key: every directed pair once, with w, ascending by f)
//   cand_of / better   per directed pair: what the arg-max of a face compares -- associative and commutative: any tree
//   first_pointer   per face: its best where it is a sliver with a neighbour, else itself
//   settle_mutual   per face, from the pointers as first_pointer left them: the winner of a mutual pair points at itself
//   jump          per face, in place: ptr[k] = ptr[ptr[k]] -- a read may see the old or the new value, both are ancestors
//   flags_of / record_of   per face
//   target_label / keeps   per chain
//   (under kDrop: exclusive scans of the keep flags and of the kept chains' points; the scatter)
//
// Scratch per call: per chain 56 bytes (the two sums, the two new labels, the keep flag, the points kept and their two
// scans) and per chain SIDE (2 nc of them) 164 bytes: the two sorts' keys in and out and their unique keys (12 + 24),
// the values in and out, which the second sort reuses, and the areas (48), the candidates in and out (64), the best, the
// two pointers and the flags of every face (16) -- 384 bytes per chain in all, plus rocPRIM's temporary storage.
// Allocated per call and freed.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rj_rings.h"

namespace rj {
namespace eliminate {

typedef unsigned __int128 u128;
typedef __int128 i128;
using rings::U128;

constexpr uint32_t kDrop = 1u;                                                    // RJ_ELIM_DROP
constexpr uint32_t kSliver = 1u, kEliminated = 2u, kIsland = 4u, kNegative = 8u;  // RJ_ELIM_SLIVER ... RJ_ELIM_NEGATIVE
constexpr uint32_t kNone = 0xFFFFFFFFu;  // no face (there are at most 2 nc < 2^32 - 1 faces)
constexpr uint32_t kZeroKey = 0xFFFFFFFFu;  // the sort key of label 0: behind every face
constexpr uint64_t kNoPair = ~0ull;         // the directed key of a chain side that separates nothing
constexpr int kMaxRounds = 33;              // jumping rounds: a path of 2^32 faces at most

struct Face {  // rj_elim_face (32 bytes)
  int32_t label, target, best;
  uint32_t flags;
  uint64_t area2_lo;
  int64_t area2_hi;
};
struct Counts {  // rj_eliminate_counts
  uint64_t n_faces, n_slivers, n_eliminated, n_islands, n_mutual, n_negative, n_chains, n_points, n_dropped;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;         // the input check's status (rings::kBad*); not 0: nothing further is written
  uint32_t unfinished;  // the jumping budget ran out (cannot happen: the pointers have no cycle behind settle_mutual)
  uint32_t emit;        // 1: every output fits its capacity and is written
  uint32_t changed[kMaxRounds];  // jumping: pointers that moved in round r
  uint64_t n_keys;      // unique label keys (the faces, and label 0 where it occurs)
  uint64_t n_dir;       // unique directed keys (the directed pairs, and kNoPair where a chain side separates nothing)
  uint64_t n_best;      // faces with a neighbour (and the run of kNoPair)
  Counts counts;
};
// what a face's arg-max compares: a directed pair (f, g) with its weight
struct alignas(16) Cand {
  uint64_t w_lo, w_hi;  // w(f, g)
  uint64_t pair;        // (min(f, g) << 32) | max(f, g)
  uint64_t dir;         // (f << 32) | g
};

RJ_RHD i128 value(U128 a) { return (i128) (((u128) a.hi << 64) | a.lo); }
RJ_RHD u128 tolerance(uint64_t tol_lo, uint64_t tol_hi) { return ((u128) tol_hi << 64) | tol_lo; }

// ---- 1. chain sums ------------------------------------------------------------------------------------------
// floor(sqrt(v)), v < 2^96: a double estimate (off by less than 1 at this size) corrected by integer compares of its
// square q, stepped by (r - 1)^2 = q - 2 r + 1 and (r + 1)^2 = q + 2 r + 1: one multiplication
RJ_RHD uint64_t isqrt(u128 v) {
  const double d = (double) (uint64_t) (v >> 64) * 18446744073709551616.0 + (double) (uint64_t) v;
  uint64_t r = (uint64_t) sqrt(d);
  u128 q = (u128) r * r;
  while (q > v) {
    q -= 2 * (u128) r - 1;
    r--;
  }
  while (q + 2 * (u128) r + 1 <= v) {
    q += 2 * (u128) r + 1;
    r++;
  }
  return r;
}
// the edge a -> b
RJ_RHD i128 edge_cross(int64_t ax, int64_t ay, int64_t bx, int64_t by) { return rings::cross(ax, ay, bx, by); }
RJ_RHD uint64_t edge_length(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  const i128 dx = bx - ax, dy = by - ay;  // (each below 2^47: the sum of the squares below 2^95)
  return isqrt((u128) (dx * dx + dy * dy));
}

// ---- 2. faces -----------------------------------------------------------------------------------------------
// ascending keys = ascending (uint32_t) label, with label 0 behind them all
RJ_RHD uint32_t key_of(int32_t label) { return (uint32_t) label - 1u; }
RJ_RHD int32_t label_of(uint32_t key) { return (int32_t) (key + 1u); }
// chain side i = 2 c + s
RJ_RHD int32_t side_label(uint64_t i, const int32_t* left, const int32_t* right) { return (i & 1) ? right[i >> 1] : left[i >> 1]; }
RJ_RHD uint32_t side_key(uint64_t i, const int32_t* left, const int32_t* right) { return key_of(side_label(i, left, right)); }
RJ_RHD U128 side_sum(uint64_t i, const U128* S) { return (i & 1) ? rings::sub(U128{0, 0}, S[i >> 1]) : S[i >> 1]; }
// keys[n_keys]: the unique keys, ascending
RJ_RHD uint64_t count_faces(uint64_t n_keys, const uint32_t* keys) { return n_keys - (n_keys && keys[n_keys - 1] == kZeroKey ? 1 : 0); }
// the face of a label that occurs in the map (label 0: kNone)
RJ_RHD uint32_t face_index(int32_t label, const uint32_t* keys, uint64_t nf) {
  if (label == 0) return kNone;
  const uint32_t key = key_of(label);
  uint64_t lo = 0, hi = nf;  // keys[lo] <= key < keys[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key)
      lo = mid;
    else
      hi = mid;
  }
  return (uint32_t) lo;
}
RJ_RHD bool is_negative(i128 area2) { return area2 < 0; }
RJ_RHD bool is_sliver(i128 area2, u128 tol) { return !is_negative(area2) && (u128) area2 <= tol; }

// ---- 3. pairs -----------------------------------------------------------------------------------------------
RJ_RHD bool separates(int32_t l, int32_t r) { return l != r && l != 0 && r != 0; }
// chain side i: (f << 32) | g, f the face on this side and g the face on the other
RJ_RHD uint64_t directed_key(uint64_t i, const int32_t* left, const int32_t* right, const uint32_t* keys, uint64_t nf) {
  const int32_t mine = side_label(i, left, right), other = side_label(i ^ 1, left, right);
  if (!separates(mine, other)) return kNoPair;
  return ((uint64_t) face_index(mine, keys, nf) << 32) | face_index(other, keys, nf);
}
RJ_RHD uint32_t from_of(uint64_t dir) { return (uint32_t) (dir >> 32); }
RJ_RHD uint32_t to_of(uint64_t dir) { return (uint32_t) dir; }
RJ_RHD Cand cand_of(uint64_t dir, U128 w) {
  const uint64_t f = from_of(dir), g = to_of(dir);
  return Cand{w.lo, w.hi, f < g ? (f << 32) | g : (g << 32) | f, dir};
}
// the larger weight, then the smaller min(f, g), then the smaller max(f, g): strict on the pairs of one face
RJ_RHD bool better(const Cand& a, const Cand& b) {
  if (a.w_hi != b.w_hi) return a.w_hi > b.w_hi;
  if (a.w_lo != b.w_lo) return a.w_lo > b.w_lo;
  return a.pair < b.pair;
}
RJ_RHD Cand best_of(const Cand& a, const Cand& b) { return better(b, a) ? b : a; }

// ---- 4. pointers ----------------------------------------------------------------------------------------------
// best[k]: the face that cand's arg-max named, kNone for a face without a neighbour
RJ_RHD uint32_t first_pointer(uint32_t k, bool sliver, const uint32_t* best) { return sliver && best[k] != kNone ? best[k] : k; }
// from the pointers as first_pointer left them: the winner of a mutual pair points at itself.  *counted: k is the
// smaller face of a mutual pair
RJ_RHD uint32_t settle_mutual(uint32_t k, const uint32_t* first, const U128* area2, bool* counted) {
  const uint32_t g = first[k];
  *counted = false;
  if (g == k || first[g] != k) return g;
  *counted = k < g;
  const i128 mine = value(area2[k]), other = value(area2[g]);
  const bool stays = mine != other ? mine > other : k < g;
  return stays ? k : g;
}
// in place; -> the pointer moved
RJ_RHD bool jump(uint32_t k, uint32_t* ptr) {
  const uint32_t p = ptr[k], q = ptr[p];
  if (q == p) return false;
  ptr[k] = q;
  return true;
}
RJ_RHD uint32_t flags_of(uint32_t k, bool sliver, bool negative, const uint32_t* best, const uint32_t* ptr) {
  return (sliver ? kSliver : 0u) | (ptr[k] != k ? kEliminated : 0u) | (sliver && best[k] == kNone ? kIsland : 0u) | (negative ? kNegative : 0u);
}
RJ_RHD Face record_of(uint32_t k, const uint32_t* keys, const U128* area2, uint32_t flags, const uint32_t* best, const uint32_t* ptr) {
  const bool chose = (flags & kSliver) && best[k] != kNone;
  return Face{label_of(keys[k]), label_of(keys[ptr[k]]), label_of(keys[chose ? best[k] : k]), flags, area2[k].lo, (int64_t) area2[k].hi};
}

// ---- 5. the new labels ------------------------------------------------------------------------------------------
RJ_RHD int32_t target_label(int32_t label, const uint32_t* keys, uint64_t nf, const uint32_t* ptr) {
  return label == 0 ? 0 : label_of(keys[ptr[face_index(label, keys, nf)]]);
}
// under kDrop: a chain goes exactly when its labels differed and no longer do
RJ_RHD bool keeps(int32_t l, int32_t r, int32_t out_l, int32_t out_r) { return !(l != r && out_l == out_r); }
// every output fits: faces only where records are asked for, points only under kDrop
RJ_RHD bool fits(const Counts& c, bool records, bool drop, uint64_t face_cap, uint64_t chain_cap, uint64_t point_cap) {
  return (!records || c.n_faces <= face_cap) && c.n_chains <= chain_cap && (!drop || c.n_points <= point_cap);
}

}  // namespace eliminate

#if defined(__HIPCC__)
// what a call reports besides its counts
struct EliminateReport : StageMs {};  // the check and the chain sums; the faces; the pairs and the choice; the pointers; the new labels and the scatter; all
// rj_map_eliminate behind its argument checks, on stream st: *result = the device's Meta.  point_blocks: the grid of the
// two passes over the points (0: by size; any grid gives the same result).  Allocates and frees its scratch;
// synchronises the stream once, at the end.
hipError_t map_eliminate_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                                uint64_t tol_lo, uint64_t tol_hi, uint32_t flags, uint64_t face_cap, uint64_t chain_cap, uint64_t point_cap,
                                eliminate::Face* faces, int32_t* out_left, int32_t* out_right, int64_t* out_xy, uint32_t* out_row, uint32_t* origin,
                                int point_blocks, eliminate::Meta* result, EliminateReport* report);
#endif

}  // namespace rj
