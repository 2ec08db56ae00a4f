// rj_overlay.h -- the overlay's FACE TABLE: which face of map 0 overlaps which face of map 1, and twice the signed area
// of each overlap, exactly (rj_overlay_faces, include/rayjoin_amd.h; kernels in rj_overlay.hip).
//
// Semantics: the pieces of the output map that host/output_chain.h writes (CutChainsIntoPieces + OutputMapWriter::Add,
// the reference's WriteOutputChain, src/app/output_chain.h:42-205).  Every chain of map im is cut at its intersection
// records; a kept piece (other_face != 0) adds, for each consecutive pair a -> b of its points (head cut point, the
// chain's vertices inside it, tail cut point; scaled integers, the cut points being the records' x_num / y_num),
// cross(a, b) = a.x b.y - b.x a.y to the region (left face, other_face) and -cross(a, b) to (right face, other_face); a
// side whose face is 0 adds nothing.  Regions are oriented (face of map 0, face of map 1).  Since chains keep their face
// on the left, every sum is twice a positive area on maps in general position; where the maps share boundary (nested
// maps, shared vertices) the table inherits the output map's labels, exactly as the CDB file does.
//
// Exact: scaled coordinates lie in [-2^46, 2^46), so |cross| <= 2^93 and a sum of fewer than 2^28 sub-segments stays
// below 2^121 -- an int128 never overflows and the table is the same whatever the summation order.
//
// The label rule per EDGE (no walk along the chain): edge e of chain c runs from vertex p1(e) = e + c to e + c + 1; R =
// the records with eid[im] == e, in order along the edge (rj_overlay_edge_xsects' order):
//   * before the first cut on e:          vertex_face[p1(e)]          (the piece ends at that cut: its last vertex)
//   * between cut k and cut k + 1 on e:   R[k].mid_point_polygon_id
//   * after the last cut, or all of e without a cut: vertex_face[p1(e')] for the next edge e' > e of the chain that has
//     a cut, vertex_face[last vertex of c] when there is none -- the last vertex of the piece that sub-segment is in.
// The next cut edge is the record at upper_bound(eid[im] = e): the records are sorted by eid[im].
//
// These functions are the source both the HIP kernels and the host twin (tests/hosttwin/overlay_faces_twin.cc) run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RJ_OHD __host__ __device__ __forceinline__
#else
#define RJ_OHD inline
#endif

namespace rj {
namespace overlay {

struct Rec48 {  // == rj_xsect (include/rayjoin_amd.h), 48 bytes
  int64_t x_num, x_den, y_num, y_den;
  uint32_t eid[2];
  int32_t mid, pad;
};

// an int128 as two limbs (what the sort carries and the reduction adds): two's complement, value = hi * 2^64 + lo
struct Area2 {
  uint64_t lo;
  int64_t hi;
};

constexpr uint64_t kNoKey = ~0ull;  // unused slot: sorts behind every real key (face ids are nonnegative int32)

RJ_OHD Area2 to_limbs(__int128 v) { return Area2{(uint64_t) v, (int64_t) (v >> 64)}; }
RJ_OHD __int128 from_limbs(Area2 a) { return (__int128) (((unsigned __int128) (uint64_t) a.hi << 64) | a.lo); }
RJ_OHD Area2 add(Area2 a, Area2 b) {
  const uint64_t lo = a.lo + b.lo;
  return Area2{lo, (int64_t) ((uint64_t) a.hi + (uint64_t) b.hi + (lo < a.lo ? 1u : 0u))};
}

RJ_OHD __int128 cross(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (__int128) ax * by - (__int128) bx * ay;
}

// ((uint64)(uint32)f0 << 32) | (uint32)f1 of the region of a chain of map im with face `mine` and the other map's `other`
RJ_OHD uint64_t face_key(int im, int32_t mine, int32_t other) {
  const uint32_t f0 = (uint32_t) (im ? other : mine), f1 = (uint32_t) (im ? mine : other);
  return ((uint64_t) f0 << 32) | f1;
}

// sides of a sub-segment that make a contribution: none outside the other map, one per nonzero face of the chain
RJ_OHD int sides(int32_t label, int32_t left, int32_t right) {
  return label == 0 ? 0 : (left != 0) + (right != 0);
}

// calls f(key, value) for each side (left: +v, right: -v) of a sub-segment of a chain of map im
template <class F>
RJ_OHD void emit_sides(int im, int32_t left, int32_t right, int32_t label, __int128 v, F&& f) {
  if (label == 0) return;
  if (left != 0) f(face_key(im, left, label), v);
  if (right != 0) f(face_key(im, right, label), -v);
}

// first record in [b, e) whose eid[im] >= eid (records are sorted by eid[im])
RJ_OHD uint64_t first_record_at(const Rec48* xs, uint64_t b, uint64_t e, int im, uint64_t eid) {
  while (b < e) {
    const uint64_t m = b + (e - b) / 2;
    if ((uint64_t) xs[m].eid[im] < eid) b = m + 1;
    else e = m;
  }
  return b;
}

// label of the part of edge e (chain c) after its last cut, or of the whole edge without one; `hi` = the first record
// beyond edge e (upper_bound), edge_begin[c + 1] = one past the chain's last edge
RJ_OHD int32_t tail_label(const Rec48* xs, uint64_t n, int im, uint64_t hi, uint32_t c, const uint32_t* edge_begin,
                          const int32_t* vertex_face) {
  const uint32_t chain_end = edge_begin[c + 1];
  if (hi < n && xs[hi].eid[im] < chain_end) return vertex_face[(uint64_t) xs[hi].eid[im] + c];
  return vertex_face[(uint64_t) chain_end + c];  // the chain's last vertex: row_index[c + 1] - 1
}

// label of the part of edge e (chain c) before its first cut
RJ_OHD int32_t head_label(uint64_t e, uint32_t c, const int32_t* vertex_face) { return vertex_face[e + c]; }

// twice the signed area the sub-segments of edge e (chain c, records [lo, hi)) sweep, part by part
RJ_OHD __int128 whole_edge(const int64_t* pts, uint64_t e, uint32_t c) {
  const uint64_t p = e + c;
  return cross(pts[2 * p], pts[2 * p + 1], pts[2 * p + 2], pts[2 * p + 3]);
}
RJ_OHD __int128 head_part(const int64_t* pts, uint64_t e, uint32_t c, const Rec48& first) {
  const uint64_t p = e + c;
  return cross(pts[2 * p], pts[2 * p + 1], first.x_num, first.y_num);
}
RJ_OHD __int128 middle_part(const Rec48& a, const Rec48& b) { return cross(a.x_num, a.y_num, b.x_num, b.y_num); }
RJ_OHD __int128 tail_part(const int64_t* pts, uint64_t e, uint32_t c, const Rec48& last) {
  const uint64_t q = e + c + 1;
  return cross(last.x_num, last.y_num, pts[2 * q], pts[2 * q + 1]);
}

// Every sub-segment of edge e of map im, one f(key, value) call per side: the host twin's form (one contribution per
// sub-segment side; the kernel merges the sub-segments of a piece inside the wave first, rj_overlay.hip).
template <class F>
RJ_OHD void edge_contributions(int im, uint64_t e, const int64_t* pts, const uint32_t* edge_chain, const uint32_t* edge_begin,
                               const int32_t* left, const int32_t* right, const Rec48* xs, uint64_t n,
                               const int32_t* vertex_face, F&& f) {
  const uint32_t c = edge_chain[e];
  const uint64_t lo = first_record_at(xs, 0, n, im, e), hi = first_record_at(xs, lo, n, im, e + 1);
  const int32_t l = left[c], r = right[c], tail = tail_label(xs, n, im, hi, c, edge_begin, vertex_face);
  if (lo == hi) {
    emit_sides(im, l, r, tail, whole_edge(pts, e, c), f);
    return;
  }
  emit_sides(im, l, r, head_label(e, c, vertex_face), head_part(pts, e, c, xs[lo]), f);
  for (uint64_t k = lo; k + 1 < hi; k++) emit_sides(im, l, r, xs[k].mid, middle_part(xs[k], xs[k + 1]), f);
  emit_sides(im, l, r, tail, tail_part(pts, e, c, xs[hi - 1]), f);
}

// contributions of map im the kernel may store at most (rj_overlay.hip): per piece it emits one value, plus one per wave
// boundary -- pieces <= 2 n (a head piece and the pieces between cuts: one per record; a run that restarts at a cut
// edge: one per record) + nc (one restart per chain) + waves, two sides each
RJ_OHD uint64_t max_contributions(uint64_t ne, uint64_t nc, uint64_t n) { return 2 * (2 * n + nc + (ne + 63) / 64 + 1); }

}  // namespace overlay
}  // namespace rj
