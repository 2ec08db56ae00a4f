// rj_overlay_ops.h -- the overlay OPERATIONS: which pieces the face table and the output map keep, and what names a face
// (rj_overlay_faces_op / rj_overlay_map_op, include/rayjoin_amd.h; kernels k_ovf_contrib_op in rj_overlay.hip and
// k_ovm_emit_op in rj_overlay_map.hip).  rj_overlay.h / rj_overlay_map.h hard-wire the intersection ("label != 0"); here
// that test is a selection predicate and a face key.
//
// A SIDE of a piece of a chain of map im has the ordered pair (f0, f1) = (face of map 0, face of map 1): the chain's
// left or right face and the piece's label (rj_overlay.h's label rule, unchanged: vertex faces and mid-point faces; the
// DONTKNOW of an edge's last record is never a label).
//   how  which pairs are faces of the result         by  what names a face
//     RJ_OV_INTERSECTION  f0 != 0 and f1 != 0          RJ_OV_BY_PAIR  (f0, f1)
//     RJ_OV_UNION         f0 != 0 or  f1 != 0          RJ_OV_BY_MAP0  (f0, 0): map 1's boundaries inside a face dissolve
//     RJ_OV_DIFFERENCE    f0 != 0 and f1 == 0          RJ_OV_BY_MAP1  (0, f1): map 0's boundaries dissolve
//     RJ_OV_SYMDIFF       (f0 != 0) != (f1 != 0)
//     RJ_OV_IDENTITY      f0 != 0
// A side's key is by(f0, f1) when the pair is selected and by(f0, f1) != (0, 0), else kNoKey ("no face").  A piece is
// KEPT WHEN ITS TWO SIDES' KEYS DIFFER, which subsumes "at least one side has a face": under BY_MAP0 a piece of map 1
// with the same map-0 face on both sides is dropped (the dissolve), under UNION / SYMDIFF a piece with label 0 is kept.
// Adjacent kept pieces of one chain are not merged HERE: a chain of map 0 that map 1 cuts leaves the emit pass cut under
// BY_MAP0 although both pieces then carry the same two faces; RJ_OVM_MERGE_PIECES joins them in a pass of its own over the
// staged pieces (pieces_join, rj_overlay_map.h).
// The face table: a kept piece adds +cross per point pair to its left key and -cross to its right key (a kNoKey side
// adds nothing); a row per key with a contribution, the row's face[] holding the key -- (f0, 0) is "f0 outside map 1"
// under BY_PAIR and "the selected part of f0" under BY_MAP0.
//
// (INTERSECTION, BY_PAIR) is rj_overlay.h / rj_overlay_map.h's rule on every map whose chains have different faces on
// their two sides (what a planar map's chains have); a chain with the SAME nonzero face on both sides is kept there
// (adding +v and -v to one row) and dropped here.
//
// The operation is wave-uniform: `Op` is computed once per kernel from the two kernel arguments, `selected` is a lookup
// in a 4-bit truth table and `by` two masks -- no branch on `how` / `by` per piece, none on loaded data.
//
// These functions are the source both the HIP kernels and the host twin (tests/hosttwin/overlay_ops_twin.cc) run.
#pragma once
#include "rj_overlay_map.h"

namespace rj {
namespace overlay {

// (the values of RJ_OV_* in include/rayjoin_amd.h)
constexpr uint32_t kHowIntersection = 0, kHowUnion = 1, kHowDifference = 2, kHowSymdiff = 3, kHowIdentity = 4, kHowCount = 5;
constexpr uint32_t kByPair = 0, kByMap0 = 1, kByMap1 = 2, kByCount = 3;

// bit ((f0 != 0) << 1 | (f1 != 0)) of the table: is the pair a face of the result
RJ_OHD uint32_t select_table(uint32_t how) {
  switch (how) {
    case kHowIntersection: return 0x8u;  // 11
    case kHowUnion: return 0xEu;         // 01, 10, 11
    case kHowDifference: return 0x4u;    // 10
    case kHowSymdiff: return 0x6u;       // 01, 10
    case kHowIdentity: return 0xCu;      // 10, 11
    default: return 0u;
  }
}

RJ_OHD bool selected(uint32_t how, int32_t f0, int32_t f1) {
  return (select_table(how) >> (((f0 != 0) << 1) | (f1 != 0))) & 1u;
}

struct Op {
  uint32_t table;  // select_table(how)
  uint32_t keep0, keep1;  // by: all ones for a face that is part of the name, 0 for one that dissolves
};

RJ_OHD Op make_op(uint32_t how, uint32_t by) {
  return Op{select_table(how), by == kByMap1 ? 0u : ~0u, by == kByMap0 ? 0u : ~0u};
}

// the key of the side of a piece of map im whose chain has face `mine` there and whose label is `label`
RJ_OHD uint64_t side_key(int im, int32_t mine, int32_t label, Op op) {
  const int32_t f0 = im ? label : mine, f1 = im ? mine : label;
  const bool sel = (op.table >> (((f0 != 0) << 1) | (f1 != 0))) & 1u;
  const uint32_t k0 = (uint32_t) f0 & op.keep0, k1 = (uint32_t) f1 & op.keep1;
  return sel && (k0 | k1) ? ((uint64_t) k0 << 32) | k1 : kNoKey;
}
RJ_OHD uint64_t side_key(int im, int32_t mine, int32_t label, uint32_t how, uint32_t by) {
  return side_key(im, mine, label, make_op(how, by));
}

RJ_OHD bool kept(int im, int32_t left, int32_t right, int32_t label, Op op) {
  return side_key(im, left, label, op) != side_key(im, right, label, op);
}

// contributions a sub-segment makes: none when its piece is dropped, else one per side with a face
RJ_OHD int sides(int im, int32_t left, int32_t right, int32_t label, Op op) {
  const uint64_t kl = side_key(im, left, label, op), kr = side_key(im, right, label, op);
  return kl == kr ? 0 : (kl != kNoKey) + (kr != kNoKey);
}

// calls f(key, value) for each side (left: +v, right: -v) of a sub-segment of a chain of map im
template <class F>
RJ_OHD void emit_sides(int im, int32_t left, int32_t right, int32_t label, __int128 v, Op op, F&& f) {
  const uint64_t kl = side_key(im, left, label, op), kr = side_key(im, right, label, op);
  if (kl == kr) return;
  if (kl != kNoKey) f(kl, v);
  if (kr != kNoKey) f(kr, -v);
}

// rj_overlay.h's edge_contributions under an operation: every sub-segment of edge e of map im, one f(key, value) call
// per side (the host twin's form; all sub-segments of a piece share the piece's label, so they are kept or dropped together)
template <class F>
RJ_OHD void edge_contributions(int im, uint64_t e, const int64_t* pts, const uint32_t* edge_chain, const uint32_t* edge_begin,
                               const int32_t* left, const int32_t* right, const Rec48* xs, uint64_t n, const int32_t* vertex_face,
                               Op op, F&& f) {
  const uint32_t c = edge_chain[e];
  const uint64_t lo = first_record_at(xs, 0, n, im, e), hi = first_record_at(xs, lo, n, im, e + 1);
  const int32_t l = left[c], r = right[c], tail = tail_label(xs, n, im, hi, c, edge_begin, vertex_face);
  if (lo == hi) {
    emit_sides(im, l, r, tail, whole_edge(pts, e, c), op, f);
    return;
  }
  emit_sides(im, l, r, head_label(e, c, vertex_face), head_part(pts, e, c, xs[lo]), op, f);
  for (uint64_t k = lo; k + 1 < hi; k++) emit_sides(im, l, r, xs[k].mid, middle_part(xs[k], xs[k + 1]), op, f);
  emit_sides(im, l, r, tail, tail_part(pts, e, c, xs[hi - 1]), op, f);
}

// rj_overlay_map.h's edge_emit under an operation: the same points in the same order with the same duplicate rule; a
// piece starts (start(label), then its points) when kept(label).  The early return for a chain without faces becomes one
// for left == right: the two keys are then equal under every operation and none of the chain's pieces is kept.
template <class S, class P>
RJ_OHD void edge_emit(int im, uint64_t e, uint32_t c, uint64_t lo, uint64_t hi, int32_t tail, const int64_t* pts,
                      const uint32_t* edge_begin, const int32_t* left, const int32_t* right, const Rec48* xs,
                      const int32_t* vertex_face, Op op, S&& start, P&& point) {
  const int32_t l = left[c], r = right[c];
  if (l == r) return;
  const uint64_t p = e + c;
  int64_t px = pts[2 * p], py = pts[2 * p + 1];  // the point emitted last (whether or not its piece is kept)
  int32_t label = lo < hi ? head_label(e, c, vertex_face) : tail;
  bool keep = kept(im, l, r, label, op);
  if (keep) {
    bool dup = false;
    if (edge_begin[c] == e) {
      start(label);
    } else if (lo > 0 && (uint64_t) xs[lo - 1].eid[im] == e - 1) {  // edge e - 1 (same chain) ends with a cut
      dup = xs[lo - 1].x_num == px && xs[lo - 1].y_num == py;
    } else {
      dup = pts[2 * p - 2] == px && pts[2 * p - 1] == py;
    }
    if (!dup) point(px, py);
  }
  for (uint64_t k = lo; k < hi; k++) {
    const int64_t cx = xs[k].x_num, cy = xs[k].y_num;
    if (keep && (cx != px || cy != py)) point(cx, cy);
    label = k + 1 < hi ? xs[k].mid : tail;
    keep = kept(im, l, r, label, op);
    if (keep) {
      start(label);
      point(cx, cy);
    }
    px = cx;
    py = cy;
  }
  if (keep && edge_begin[c + 1] == e + 1) {
    const int64_t lx = pts[2 * p + 2], ly = pts[2 * p + 3];
    if (lx != px || ly != py) point(lx, ly);
  }
}

// The scratch bounds of the intersection hold for every operation: max_contributions (rj_overlay.h) counts a value per
// piece and per wave boundary on both sides, max_pieces / max_points (rj_overlay_map.h) a piece per chain and per record
// and every vertex and cut point twice -- all of them count EVERY piece, kept or not.

}  // namespace overlay
}  // namespace rj
