// rj_face_points.h -- per-face counts, sums and members of located points (rj_face_points, include/rayjoin_amd.h; kernels
// in rj_face_points.hip): the other half of a spatial join -- what GIS users know as Summarize Within, Points in Polygon
// count, or a spatial join with aggregation.  rj_pip_query answers "which face is this point in" with one int32 per point;
// this call turns that array into one row per face, numbered as rj_map_neighbours numbers its faces.  Integers only, exact,
// and fully determined: no tuning choice below can change a result.
//
// INPUT   label[n]: point i < n has label label[i] (what rj_pip_query wrote; any int32 is accepted), n < 2^32 (kMaxPoints:
//         point numbers and `first` are 32 bits, and the limb arithmetic below counts on it).  value (may be null) with
//         value_stride >= 1 in int64 elements: the value of point i is value[i * value_stride].  The scaled point array with
//         stride 2, and then that array + 1, give the sums of x and of y -- the mean centre of the points of every face.
//         Without values every sum is 0 and min / max hold the empty values.
// FACES   With a universe face_label[n_face_labels]: face k is face_label[k]; the array must ascend strictly by
//         eliminate::key_of (the nonzero labels in (uint32_t) order) and must not contain 0 -- exactly the label column of
//         rj_map_neighbours' records, so row k here is row k there.  One function per entry checks it (universe_bad); a
//         violation refuses the call.  A face without a point appears with n_points = 0.  Without a universe the faces are
//         the distinct nonzero labels among the points, in the same order.
// PER FACE   n_points; sum, a two's-complement int128, exact; min and max (INT64_MAX / INT64_MIN where the face has no point
//         or there are no values); first = the smallest point number in the face (kNoPoint = 0xFFFFFFFF where there is none).
// COUNTS  n_faces; n_members = the points whose label is a face; n_outside = the points with label 0; n_unmatched = the
//         points with a nonzero label that is not in the universe (0 without one); n_runs = the number of i with i == 0 or
//         label[i] != label[i - 1] -- the coherence of the point order, which is what decides the cost of the call.
//         n_members + n_outside + n_unmatched == n.
// MEMBERS under kMembers   offsets[n_faces + 1] and members[n_members]: the point numbers of face k lie at
//         [offsets[k], offsets[k + 1]), ascending; offsets[n_faces] = n_members.  So first(k) = members[offsets[k]] for a
//         face with a point.
//
// THE SUM WITHOUT A 128-BIT ATOMIC   A value v is split as v = h 2^32 + l with l = (uint32_t) v in [0, 2^32) and
// h = v >> 32 in [-2^31, 2^31) (arithmetic shift: the split is exact for every int64).  A face accumulates L = the sum of
// l in one unsigned 64-bit word and H = the sum of h in one signed 64-bit word.  Over n < 2^32 points
//     0 <= L <= (2^32 - 1)(2^32 - 1) < 2^64     and     |H| <= 2^31 (2^32 - 1) < 2^63,
// so neither word wraps, whatever the values are, and every partial sum of a wave run or of a lane has the same bounds.
// sum = H 2^32 + L, recombined in 128 bits when the record is written (sum_of).  5 x INT64_MAX + 3 x INT64_MIN in one face
// is L = 5 (2^32 - 1), H = 5 (2^31 - 1) - 3 2^31.
//
// ORDER   Every accumulator is an integer add, min or max: they commute and associate, so the result does not depend on the
// order in which the runs arrive, on the grid, or on where a wave or a block cuts the points.  No float atomics, no
// compare-and-swap loops.
//
// Every step is one function per element that rj_face_points.hip runs as a kernel and tests/hosttwin/face_points_twin.cc
// runs as a plain loop (a test-only twin, never a fallback):
//
//   universe_bad / universe_key   with a universe, per entry: the check; its sort key
//   is_head / head_key   without one, per point: the first of a run of equal labels; the key of its label
//   (the head keys compacted, radix-sorted, made unique: the keys of the faces ascending, and kZeroKey last where label 0
//   occurs.  Only the heads are sorted, never all n labels.  Their number is only known on the device, so WITHOUT a
//   universe the host reads it once, behind the compaction, to size the sort: one sync more than the one at the end.)
//   acc_empty     per face: the accumulators of a face without a point
//   part_of / part_add / seg_head   THE TABLE PASS, per point: what it contributes; how two neighbouring pieces of a run
//                 combine; where a run starts for the pass -- at a head, and at every multiple of kWave, where a wave starts.
//                 The device reduces the lanes of a run with a segmented scan over shuffles (no LDS round trip); the twin
//                 adds them one after the other.  The last lane of a run holds the run's Part.
//   run_apply     per run, by its last lane only: one binary search of the face (find_face), one set of adds / mins / maxes
//                 into the accumulators of the face.  -> kMember, kOutside or kUnmatched: the pass counts the points of the
//                 last two per lane and adds them once per block (label 0 takes most points of a typical query: one atomic
//                 per run on that single word would serialise the pass).
//   sum_of / face_record   per face: the record
//   (under kMembers an exclusive scan of n_points: the offsets)
//   member_key    under kMembers, per point: its face number, n_faces for a point that is no member
//   (a stable radix sort of (member_key, point number) over the low bits that hold n_faces: the members of every face
//   ascending, face after face; the points that are no member fall off the end)
//   fits          all or nothing
//
// Scratch per call, allocated and freed: per face (the universe's, or one per run head without a universe) 4 + 48 bytes
// (key, accumulators), under kMembers 8 more (the scanned offsets); without a universe 12 bytes per run head (the keys
// compacted, sorted, unique); under kMembers 12 bytes per point (the keys in and out, the sorted point numbers).  Plus
// rocPRIM's temporary storage.  Without kMembers and with a universe nothing is allocated per point: the pass reads
// 4 n bytes of labels and 8 n of values once and writes nothing per point.
#pragma once
#include <stdint.h>

#include "rj_eliminate.h"

namespace rj {
namespace face_points {

using rings::U128;
typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr uint32_t kMembers = 1u;  // RJ_FP_MEMBERS
constexpr uint32_t kZeroKey = eliminate::kZeroKey;
constexpr uint32_t kNone = 0xFFFFFFFFu;     // find_face: no such face
constexpr uint32_t kNoPoint = 0xFFFFFFFFu;  // `first` of a face without a point (n < 2^32: no point has this number)
constexpr uint64_t kMaxPoints = 1ull << 32;  // n stays below
constexpr uint32_t kWave = 64;               // the table pass cuts a run where a wave starts
constexpr int kMember = 0, kOutside = 1, kUnmatched = 2;  // run_apply
constexpr uint32_t kBadUniverse = 1;                      // Meta::bad

struct Face {  // rj_fp_face (48 bytes)
  int32_t label;
  uint32_t first;
  uint64_t n_points;
  uint64_t sum_lo;
  int64_t sum_hi;
  int64_t min, max;
};
struct Counts {  // rj_face_points_counts
  uint64_t n_faces, n_members, n_outside, n_unmatched, n_runs;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;   // kBadUniverse: nothing further is written
  uint32_t emit;  // 1: every output fits its capacity and is written
  uint64_t n_heads;  // without a universe: the run heads that the compaction found
  uint64_t n_keys;   // without a universe: their unique keys (the faces, and label 0 where it occurs)
  Counts counts;
};
// the accumulators of a face (48 bytes): the limbs L and H of the header, everything else as in the record
struct Acc {
  uint64_t n, lo;
  int64_t hi, min, max;
  uint32_t first, pad;
};
// what a piece of a run holds: points that follow each other and have one label
struct Part {
  uint32_t n, first;
  uint64_t lo;
  int64_t hi, min, max;
};

// ---- the adds, mins and maxes: atomics on the device, plain on the host ---------------------------------------------------
RJ_RHD void add_to(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long) v);
#else
  *p += v;
#endif
}
RJ_RHD void add_to(int64_t* p, int64_t v) { add_to(reinterpret_cast<uint64_t*>(p), (uint64_t) v); }  // (two's complement: the same add)
RJ_RHD void min_to(int64_t* p, int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(reinterpret_cast<long long*>(p), (long long) v);
#else
  if (v < *p) *p = v;
#endif
}
RJ_RHD void max_to(int64_t* p, int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(reinterpret_cast<long long*>(p), (long long) v);
#else
  if (v > *p) *p = v;
#endif
}
RJ_RHD void min_to(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}

// ---- 1. the universe ------------------------------------------------------------------------------------------------------
// entry k of a given universe: not 0, and behind its predecessor in key order
RJ_RHD bool universe_bad(uint64_t k, const int32_t* face_label) {
  if (face_label[k] == 0) return true;
  return k > 0 && eliminate::key_of(face_label[k - 1]) >= eliminate::key_of(face_label[k]);
}
RJ_RHD uint32_t universe_key(uint64_t k, const int32_t* face_label) { return eliminate::key_of(face_label[k]); }
// point i starts a run of equal labels
RJ_RHD bool is_head(uint64_t i, const int32_t* label) { return i == 0 || label[i] != label[i - 1]; }
RJ_RHD uint32_t head_key(uint64_t i, const int32_t* label) { return eliminate::key_of(label[i]); }
// keys[nf]: the keys of the faces, ascending.  -> the face of a label, kNone for label 0 and for a label that is no face
RJ_RHD uint32_t find_face(int32_t label, const uint32_t* keys, uint64_t nf) {
  if (label == 0 || nf == 0) return kNone;
  const uint32_t k = eliminate::face_index(label, keys, nf);  // (the last key that is not above the label's)
  return keys[k] == eliminate::key_of(label) ? k : kNone;
}

// ---- 2. the table pass ----------------------------------------------------------------------------------------------------
RJ_RHD Acc acc_empty() { return Acc{0, 0, 0, INT64_MAX, INT64_MIN, kNoPoint, 0}; }
// point i alone; value null: no values
RJ_RHD Part part_of(uint64_t i, const int64_t* value, uint64_t stride) {
  if (!value) return Part{1, (uint32_t) i, 0, 0, INT64_MAX, INT64_MIN};
  const int64_t v = value[i * stride];
  return Part{1, (uint32_t) i, (uint64_t) (uint32_t) v, v >> 32, v, v};
}
// a in front of b, both of one run
RJ_RHD Part part_add(const Part& a, const Part& b) {
  return Part{a.n + b.n, a.first < b.first ? a.first : b.first, a.lo + b.lo, a.hi + b.hi, a.min < b.min ? a.min : b.min, a.max > b.max ? a.max : b.max};
}
// where the pass starts a run: at a head, and where a wave starts
RJ_RHD bool seg_head(uint64_t i, const int32_t* label) { return i % kWave == 0 || is_head(i, label); }
// the run with Part p and this label: into its face, or nowhere.  -> kMember, kOutside, kUnmatched
RJ_RHD int run_apply(const Part& p, int32_t label, bool values, const uint32_t* keys, uint64_t nf, Acc* acc) {
  if (label == 0) return kOutside;
  const uint32_t k = find_face(label, keys, nf);
  if (k == kNone) return kUnmatched;
  Acc* a = acc + k;
  add_to(&a->n, (uint64_t) p.n);
  min_to(&a->first, p.first);
  if (values) {
    add_to(&a->lo, p.lo);
    add_to(&a->hi, p.hi);
    min_to(&a->min, p.min);
    max_to(&a->max, p.max);
  }
  return kMember;
}

// ---- 3. the records -------------------------------------------------------------------------------------------------------
// H 2^32 + L in 128 bits (|H| < 2^63: the shift stays far inside)
RJ_RHD U128 sum_of(const Acc& a) { return rings::limbs((i128) a.hi * ((i128) 1 << 32) + (i128) (u128) a.lo); }
RJ_RHD Face face_record(uint64_t k, const uint32_t* keys, const Acc* acc) {
  const Acc& a = acc[k];
  const U128 s = sum_of(a);
  return Face{eliminate::label_of(keys[k]), a.first, a.n, s.lo, (int64_t) s.hi, a.min, a.max};
}

// ---- 4. the members -------------------------------------------------------------------------------------------------------
RJ_RHD uint32_t member_key(uint64_t i, const int32_t* label, const uint32_t* keys, uint64_t nf) {
  const uint32_t k = find_face(label[i], keys, nf);
  return k == kNone ? (uint32_t) nf : k;
}
// the low bits that hold every key 0 .. nf: ceil(log2(nf + 1)), at least 1
RJ_RHD int key_bits(uint64_t nf) {
  int b = 1;
  while (b < 32 && (nf >> b) != 0) b++;
  return b;
}
// every output fits
RJ_RHD bool fits(const Counts& c, bool members, uint64_t face_cap, uint64_t member_cap) {
  return c.n_faces <= face_cap && (!members || c.n_members <= member_cap);
}

}  // namespace face_points

#if defined(__HIPCC__)
// what a call reports besides its counts
struct FacePointsReport : StageMs {};  // universe; table; records; members; (nothing); all
// rj_face_points behind its argument checks, on stream st: *result = the device's Meta.  table_blocks: the grid of the
// table pass (0: by size; any grid gives the same result).  Allocates and frees its scratch; synchronises the stream once,
// at the end, and without a universe once more, behind the compaction of the run heads: the host reads their number there
// and sizes the sort by it.
hipError_t face_points_device(hipStream_t st, const int32_t* label, uint64_t n, const int64_t* value, uint64_t value_stride, const int32_t* face_label,
                              uint64_t n_face_labels, uint32_t flags, uint64_t face_cap, uint64_t member_cap, face_points::Face* faces, uint64_t* offsets,
                              uint32_t* members, int table_blocks, face_points::Meta* result, FacePointsReport* report);
// label_dev[k] = faces_dev[k].label of rj_map_neighbours' records (a strided copy on the stream; not synchronised)
hipError_t neighbours_labels_device(hipStream_t st, const void* nb_faces, uint64_t n_faces, int32_t* label);
#endif

}  // namespace rj
