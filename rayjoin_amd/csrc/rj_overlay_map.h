// rj_overlay_map.h -- the overlay's OUTPUT MAP as arrays (rj_overlay_map, include/rayjoin_amd.h; kernels in
// rj_overlay_map.hip): the pieces host/output_chain.h keeps, with their points in scaled integers.
//
// A piece of chain c of map im starts with the chain or at a cut (a record of the chain) and ends at the next cut or with
// the chain; it is kept when its label (the face of the other map it lies in, rj_overlay.h's rule) is nonzero and the
// chain has a face on at least one side.  Its points: head cut point, the chain's vertices inside it, tail cut point;
// consecutive equal points once.
//
// The rule per EDGE, in the order the points leave: edge e (chain c, records R[0..m) on it) emits
//   * its first vertex V(e): it belongs to the piece that covers the start of e (label: head_label with a cut on e,
//     tail_label without); the chain's first edge STARTS a piece with it;
//   * for every cut k: R[k]'s point as the end of the piece before it, then again as the START of the next piece
//     (label R[k].mid between two cuts of e, tail_label after the last);
//   * the chain's last vertex, when e is the chain's last edge.
// A point is dropped when it equals the point emitted just before it in the same piece.  That predecessor is on the same
// edge, or the last point of edge e - 1 (its last cut, else its first vertex): the rule stays local, and since equality
// is transitive, comparing with the emitted predecessor is comparing with the last point kept (std::unique).  The first
// point of a piece has no predecessor and is always written: a piece's row_index entry is the slot of that point.
//
// This function is the source both the HIP kernels and the host twin (tests/hosttwin/overlay_map_twin.cc) run.
#pragma once
#include "rj_overlay.h"

namespace rj {
namespace overlay {

// start(label) -- a kept piece starts: the next point() is its first; point(x, y) -- the next point of the open piece.
// lo, hi: the records of edge e (first_record_at e, e + 1); tail: tail_label(..., hi, c, ...).
template <class S, class P>
RJ_OHD void edge_emit(int im, uint64_t e, uint32_t c, uint64_t lo, uint64_t hi, int32_t tail, const int64_t* pts,
                      const uint32_t* edge_begin, const int32_t* left, const int32_t* right, const Rec48* xs,
                      const int32_t* vertex_face, S&& start, P&& point) {
  if (left[c] == 0 && right[c] == 0) return;  // no face on either side: none of the chain's pieces is kept
  const uint64_t p = e + c;
  int64_t px = pts[2 * p], py = pts[2 * p + 1];  // the point emitted last (whether or not its piece is kept)
  int32_t label = lo < hi ? head_label(e, c, vertex_face) : tail;
  if (label != 0) {
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
    if (label != 0 && (cx != px || cy != py)) point(cx, cy);
    label = k + 1 < hi ? xs[k].mid : tail;
    if (label != 0) {
      start(label);
      point(cx, cy);
    }
    px = cx;
    py = cy;
  }
  if (label != 0 && edge_begin[c + 1] == e + 1) {
    const int64_t lx = pts[2 * p + 2], ly = pts[2 * p + 3];
    if (lx != px || ly != py) point(lx, ly);
  }
}

// the two face keys of a kept piece (kNoKey: no face on that side)
RJ_OHD uint64_t side_key(int im, int32_t mine, int32_t label) { return mine != 0 ? face_key(im, mine, label) : kNoKey; }

// RJ_OVM_MERGE_PIECES, the join rule: chain b of the (unmerged) output map joins chain a, the chain before it, when
// both were cut from the same source chain (origin), have the same face on either side and b begins on the point a
// ends on (integer equality).  A rule on the arrays alone: whether a and b were neighbours on the source chain does not
// enter.  Side: a face id of the output map, or the face key it is the rank of (equal keys <=> equal ids).
// last_a / first_b: x, y of a's last and b's first point.
// This function is the source both k_ovm_join and the host twin (tests/hosttwin/overlay_merge_twin.cc) run.
template <class Side>
RJ_OHD bool pieces_join(uint32_t origin_a, Side left_a, Side right_a, const int64_t* last_a, uint32_t origin_b, Side left_b, Side right_b,
                        const int64_t* first_b) {
  return origin_a == origin_b && left_a == left_b && right_a == right_b && last_a[0] == first_b[0] && last_a[1] == first_b[1];
}

// what one map can emit at most: a piece per chain and per record, every vertex and every cut point twice
RJ_OHD uint64_t max_pieces(uint64_t nc, uint64_t n) { return nc + n; }
RJ_OHD uint64_t max_points(uint64_t np, uint64_t n) { return np + 2 * n; }

// index of key among the n ascending keys (it is one of them)
RJ_OHD uint64_t key_index(const uint64_t* keys, uint64_t n, uint64_t key) {
  uint64_t b = 0, e = n;
  while (b < e) {
    const uint64_t m = b + (e - b) / 2;
    if (keys[m] < key) b = m + 1;
    else e = m;
  }
  return b;
}

}  // namespace overlay
}  // namespace rj
