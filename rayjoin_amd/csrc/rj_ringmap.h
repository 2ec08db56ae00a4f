// rj_ringmap.h -- the chain map that a set of labelled rings bounds (rj_rings_map, include/rayjoin_amd.h; kernels in
// rj_ringmap.hip): the inverse of rj_map_rings.  Rings store every shared boundary twice, once per side; the map stores it
// once, with both faces, cut where boundaries meet, and with MAXIMAL chains: a chain ends only at a junction, a dead end
// or a change of labels.  Integers only, and fully determined for every input, overlapping rings included.
//
// INPUT   ring_row[n_rings + 1], the CSR into ring_xy[2 n_points] (the layout rj_map_rings writes).  Ring r is a closed
//         walk: point i is followed by i + 1, the last point by the first; a ring may have 0, 1 or 2 points.  face(r), a
//         32-bit label read through a byte stride (4: a plain int32 array, 32: the face field of rj_ring records in
//         place), lies on the LEFT of the walk, y up: shells counter-clockwise, holes clockwise.  Face 0 is "no face";
//         rings of face 0 are allowed (the boundaries of the outside that rj_map_rings returns).  n_points < 2^31 (every
//         half-edge has a 32-bit number), every coordinate in [-2^46, 2^46).
// DIRECTED EDGES   point slot i of ring r gives u -> v, v its successor in the ring.  u == v: the edge has zero length, it
//         is dropped and counted in n_zero_edges.  Otherwise lo < hi are its two points in ascending (x, y); the edge is
//         FORWARD when u == lo and then has face(r) on the left of lo -> hi, else BACKWARD with face(r) on the right.
// UNIQUE EDGES   one per distinct (lo, hi), ascending by (lo.x, lo.y, hi.x, hi.y).  left = the face of its forward
//         directed edge with the smallest point slot (0: it has none), right the same over its backward ones.  More than
//         one forward or more than one backward directed edge: counted in n_conflicts (overlapping input, no planar
//         subdivision; the result is still determined).  Under RJ_RMAP_DISSOLVE an edge with left == right (the boundary
//         between two parts of one polygon, a dangling edge) is left out and counted in n_dissolved.  The kept edges are
//         numbered e = 0 .. n_edges - 1 in that order.
// HALF-EDGES   h = 2 e walks lo -> hi with faces (left, right), h = 2 e + 1 walks hi -> lo with faces (right, left);
//         h ^ 1 is the twin of h.
// PASSING A VERTEX   h arrives at the start point of h ^ 1.  When exactly two kept half-edges start there (h ^ 1 and one
//         other, g) and faces(g) == faces(h): next(h) = g.  Otherwise h ends there (a junction, a dead end, a change of
//         labels).  Symmetric: next(h) = g <=> next(g ^ 1) = h ^ 1, so pred(g) = next(g ^ 1) ^ 1 needs no second table.
// WALKS AND CHAINS   the maximal sequences under next.  An open walk has a first half-edge without a predecessor; a
//         closed walk is a cycle (at least 3 edges).  The twin walk of W: its twins in reverse order; never W itself
//         (next never turns round).  Leader: the first half-edge of an open walk, the smallest of a closed one, which is
//         read from there.  Of W and its twin the CHAIN is the one with the smaller leader.  Its points: the start
//         points of its half-edges in order, then the end point of the last (a closed chain repeats its first point, like
//         a closed CDB chain); left / right: the faces of its leader; chains ascend by leader.
//         n_points = n_edges + n_chains, every chain has at least 2 points: the contract of rj_upload_map_dev.
//
// Every step is one function per element that rj_ringmap.hip runs as a grid-stride kernel and
// tests/hosttwin/ringmap_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate   the input check; its status word stays on the device, an input that fails is not read
//                 further (every slot then counts as a zero-length edge, and nothing follows from it)
//   ring_mark     per ring: its index at its first point slot (inclusive max-scan: the ring of every point slot)
//   seg_of        per point slot: its canonical edge (lo, hi) and its direction
//   (one merge sort of the slots by seg_before: (lo, hi, direction, slot), zero-length edges behind everything else)
//   group_head    per sorted position: does a unique edge start here (inclusive sum-scan: its number, plus one)
//   group_fill    per sorted position: left / right / conflict of its unique edge, and where the edge starts
//   group_keep    per unique edge: kept or dissolved (exclusive sum-scan: its number among the kept ones)
//   edge_emit     per unique edge: the kept edge's two points and faces at its number
//   half_seed     per k: the even half-edges in their order (ascending by start point already: lo is the sort's first
//                 key) and the odd ones unsorted; behind n_edges the filler kNone, which sorts last
//   (merge sort of the odd ones by half_before, then one merge with the even ones: all half-edges by (start point, h))
//   half_pos      per sorted position: the inverse permutation
//   next_of       per h: next(h), from the two neighbours on each side of h ^ 1 in that order (no per-vertex loop)
//   walk_init / walk_round   pointer doubling along pred: an open walk finds its first half-edge and the distance to it,
//                 a closed one its smallest half-edge (the window minimum of rj_rings.h's cyc_round).  A round counts the
//                 walks that reached their head and the minima that changed; a round that counted nothing ends it:
//                 while an open walk is on its way, the half-edge 2^r steps behind its head arrives in round r.
//   cut_init      the closed walks opened in front of their leaders; walk_round again ranks them (open walks rest)
//   chain_total   per h: a kept leader gives 1 chain and its edges + 1 points  (exclusive scan: chain number, first point)
//   chain_place   per h: its start point to its chain's slot (the last half-edge of a chain its end point too); a
//                 leader its chain's row entry and faces; the counts
//
// The leaders ascend with h, so the chains are numbered by a scan: no sort of the leaders.  The length of a walk with
// leader a: open, 1 + the distance of a ^ 1 to its own head (a ^ 1 is the last of the twin walk); closed, 1 + the
// distance of pred(a).
//
// Scratch per call, sized by the point slots n (the number of edges is known on the device only; e <= n, h < 2 n):
// 288 bytes per point slot (the ring of the slot and its mark 8; canonical edge 32, direction 4; sort input and output 8;
// group starts and numbers 8; per unique edge left, right, conflict, start 16, kept and its scan 8; per kept edge points 32
// and faces 8; even and odd half-edges and the odd ones sorted 12, merged 8, inverse 8, next 8; two walk states 64; chain
// totals and their scan 64), plus the sorts' and scans' temporary storage; allocated per call and freed.
#pragma once
#include <stdint.h>

#include "rj_rings.h"

namespace rj {
namespace ringmap {

using rings::Slots;  // {halves, points}: here {chains, points}

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kMaxRounds = 33;      // doubling steps: 2^32 half-edges at most
constexpr uint32_t kDissolve = 1u;  // RJ_RMAP_DISSOLVE
constexpr uint32_t kForward = 0, kBackward = 1, kZero = 2;
constexpr int64_t kHalfRange = (int64_t) 1 << 46;

struct alignas(16) Seg {  // a canonical edge: lo < hi by (x, y)
  int64_t lox, loy, hix, hiy;
};
struct alignas(16) Walk {  // the walk back from h along pred
  uint32_t at;             // how far it has come: a half-edge of h's walk; done: the walk's head
  uint32_t cnt;            // steps from h to `at`
  uint32_t mn;             // first pass: the smallest half-edge from h to `at`; second pass: 1 on a closed walk
  uint32_t done;
};
struct Counts {  // rj_rings_map_counts
  uint64_t n_chains, n_points, n_edges, n_closed, n_zero_edges, n_conflicts, n_dissolved;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t act[2][kMaxRounds];  // pass p, round r: walks that reached their head plus minima that changed
  uint32_t done[2];             // the first round that was not needed: the final state is in buffer done & 1
  uint32_t bad;                 // the input check's status (kBad*); not 0: the input is not read further
  uint32_t unfinished;          // a round budget ran out (cannot happen)
  uint64_t n_groups;            // the unique edges
  Counts counts;
};
// the caller's arrays and their capacities (row: chain_cap + 1 entries)
struct Out {
  int64_t* xy;
  uint32_t* row;
  int32_t *left, *right;
  uint64_t chain_cap, point_cap;
};

RJ_RHD int32_t face_at(const void* face, uint64_t stride, uint32_t r) {
  return *reinterpret_cast<const int32_t*>(static_cast<const char*>(face) + (uint64_t) r * stride);
}

// ---- 0. the input check ------------------------------------------------------------------------------
// The largest code met is the input's status, 0: fine.  c in [0, n_rings]; every coordinate.
constexpr uint32_t kBadStart = 4, kBadEnd = 3, kBadRow = 2, kBadCoordinate = 1;
RJ_RHD uint32_t check_row(uint64_t c, const uint32_t* row, uint64_t nr, uint64_t np) {
  const uint32_t b = row[c];
  if (c == 0 && b != 0) return kBadStart;
  if (c == nr) return (uint64_t) b != np ? kBadEnd : 0;
  return row[c + 1] < b ? kBadRow : 0;
}
RJ_RHD uint32_t check_coordinate(int64_t v) { return v < -kHalfRange || v >= kHalfRange ? kBadCoordinate : 0; }

// ---- 1. the ring of every point slot ---------------------------------------------------------------------
// mark[] zeroed before; the inclusive max-scan of mark[] is ring_at[] (a ring without points marks nothing)
RJ_RHD void ring_mark(uint32_t r, const uint32_t* row, uint32_t* mark) {
  if (row[(uint64_t) r + 1] > row[r]) mark[row[r]] = r;
}

// ---- 2. canonical edges and their order -------------------------------------------------------------------
// -> the direction of slot i (kZero: dropped; so is every slot of an input that failed its check, which is not read)
RJ_RHD uint32_t seg_of(uint64_t i, bool bad, const uint32_t* ring_at, const uint32_t* row, const int64_t* xy, Seg* seg, uint32_t* dir) {
  Seg s{0, 0, 0, 0};
  uint32_t d = kZero;
  if (!bad) {
    const uint32_t r = ring_at[i];
    const uint64_t j = i + 1 == row[(uint64_t) r + 1] ? row[r] : i + 1;
    const int64_t ux = xy[2 * i], uy = xy[2 * i + 1], vx = xy[2 * j], vy = xy[2 * j + 1];
    if (ux != vx || uy != vy) {
      const bool fwd = ux != vx ? ux < vx : uy < vy;
      s = fwd ? Seg{ux, uy, vx, vy} : Seg{vx, vy, ux, uy};
      d = fwd ? kForward : kBackward;
    }
  }
  seg[i] = s;
  dir[i] = d;
  return d;
}
RJ_RHD bool same_seg(const Seg& a, const Seg& b) { return a.lox == b.lox && a.loy == b.loy && a.hix == b.hix && a.hiy == b.hiy; }
// the order of the first sort: (lo, hi, direction, slot); zero-length edges behind everything else
RJ_RHD bool seg_before(uint32_t sa, uint32_t sb, const Seg* seg, const uint32_t* dir) {
  const uint32_t da = dir[sa], db = dir[sb];
  if ((da == kZero) != (db == kZero)) return db == kZero;
  if (da == kZero) return sa < sb;
  const Seg a = seg[sa], b = seg[sb];
  if (a.lox != b.lox) return a.lox < b.lox;
  if (a.loy != b.loy) return a.loy < b.loy;
  if (a.hix != b.hix) return a.hix < b.hix;
  if (a.hiy != b.hiy) return a.hiy < b.hiy;
  if (da != db) return da < db;
  return sa < sb;
}

// ---- 3. unique edges -----------------------------------------------------------------------------------------
// sorted position j holds slot sv[j].  head[j] = 1 where a unique edge starts (zero-length edges sort last: j - 1 is none
// of them); gid[] = the inclusive sum-scan of head[]: position j belongs to unique edge gid[j] - 1
RJ_RHD void group_head(uint64_t j, const uint32_t* sv, const Seg* seg, const uint32_t* dir, uint32_t* head) {
  const uint32_t s = sv[j];
  head[j] = dir[s] != kZero && (j == 0 || !same_seg(seg[s], seg[sv[j - 1]])) ? 1 : 0;
}
// gleft[], gright[], gconf[] zeroed before.  Inside a unique edge the forward slots come first, each kind by ascending
// slot: the first of each kind gives the face.  A slot behind one of its own kind is a conflict (every writer stores the
// same word).
RJ_RHD void group_fill(uint64_t j, const uint32_t* sv, const uint32_t* dir, const uint32_t* head, const uint32_t* gid, const uint32_t* ring_at,
                       const void* face, uint64_t stride, uint32_t* ghead, int32_t* gleft, int32_t* gright, uint32_t* gconf) {
  const uint32_t s = sv[j], d = dir[s];
  if (d == kZero) return;
  const uint32_t g = gid[j] - 1;
  const bool first = head[j] != 0;
  const uint32_t before = first ? kNone : dir[sv[j - 1]];
  if (first) ghead[g] = (uint32_t) j;
  if (d == kForward && first) gleft[g] = face_at(face, stride, ring_at[s]);
  if (d == kBackward && before != kBackward) gright[g] = face_at(face, stride, ring_at[s]);
  if (before == d) gconf[g] = 1;
}
// g in [0, n]: keep[g] (0 behind the unique edges; entry n closes the scan); *what: 1 a conflict, 2 dissolved, 3 both
RJ_RHD void group_keep(uint64_t g, uint64_t n_groups, const int32_t* gleft, const int32_t* gright, const uint32_t* gconf, uint32_t flags,
                       uint32_t* keep, int* what) {
  *what = 0;
  if (g >= n_groups) {
    keep[g] = 0;
    return;
  }
  const bool dissolved = (flags & kDissolve) && gleft[g] == gright[g];
  keep[g] = dissolved ? 0 : 1;
  *what = (gconf[g] ? 1 : 0) | (dissolved ? 2 : 0);
}
// eidx = the exclusive sum-scan of keep[]
RJ_RHD void edge_emit(uint64_t g, const uint32_t* sv, const Seg* seg, const uint32_t* ghead, const int32_t* gleft, const int32_t* gright,
                      const uint32_t* keep, const uint32_t* eidx, Seg* E, int32_t* eleft, int32_t* eright) {
  if (!keep[g]) return;
  const uint32_t e = eidx[g];
  E[e] = seg[sv[ghead[g]]];
  eleft[e] = gleft[g];
  eright[e] = gright[g];
}

// ---- 4. half-edges by start point ------------------------------------------------------------------------------
RJ_RHD void start_of(uint32_t h, const Seg* E, int64_t* x, int64_t* y) {
  const Seg s = E[h >> 1];
  *x = (h & 1) ? s.hix : s.lox;
  *y = (h & 1) ? s.hiy : s.loy;
}
RJ_RHD int32_t left_of(uint32_t h, const int32_t* eleft, const int32_t* eright) { return (h & 1) ? eright[h >> 1] : eleft[h >> 1]; }
RJ_RHD int32_t right_of(uint32_t h, const int32_t* eleft, const int32_t* eright) { return (h & 1) ? eleft[h >> 1] : eright[h >> 1]; }
// k in [0, n): the fillers behind the edges sort last and are never looked up
RJ_RHD void half_seed(uint64_t k, uint64_t n_edges, uint32_t* even, uint32_t* odd) {
  even[k] = k < n_edges ? (uint32_t) (2 * k) : kNone;
  odd[k] = k < n_edges ? (uint32_t) (2 * k + 1) : kNone;
}
// the order of the second sort and of the merge: (start point, h), fillers last.  A strict total order on the half-edges.
RJ_RHD bool half_before(uint32_t ha, uint32_t hb, const Seg* E) {
  if (hb == kNone) return ha != kNone;
  if (ha == kNone) return false;
  int64_t ax, ay, bx, by;
  start_of(ha, E, &ax, &ay);
  start_of(hb, E, &bx, &by);
  if (ax != bx) return ax < bx;
  if (ay != by) return ay < by;
  return ha < hb;
}
RJ_RHD void half_pos(uint64_t k, const uint32_t* S, uint32_t* pos) { pos[S[k]] = (uint32_t) k; }

// ---- 5. next ---------------------------------------------------------------------------------------------------
RJ_RHD bool starts_at(uint32_t h, const Seg* E, int64_t x, int64_t y) {
  int64_t hx, hy;
  start_of(h, E, &hx, &hy);
  return hx == x && hy == y;
}
// S = all nh half-edges by (start point, h), pos its inverse.  Exactly two start where h ^ 1 does: one neighbour of
// h ^ 1 in S starts there, and the position behind that neighbour (and the other neighbour) do not.
RJ_RHD uint32_t next_of(uint32_t h, uint64_t nh, const uint32_t* S, const uint32_t* pos, const Seg* E, const int32_t* eleft,
                        const int32_t* eright) {
  const uint64_t k = pos[h ^ 1];
  int64_t x, y;
  start_of(h ^ 1, E, &x, &y);
  const bool below = k > 0 && starts_at(S[k - 1], E, x, y), above = k + 1 < nh && starts_at(S[k + 1], E, x, y);
  if (below == above) return kNone;  // a dead end, or three and more
  uint32_t g;
  if (below) {
    if (k > 1 && starts_at(S[k - 2], E, x, y)) return kNone;
    g = S[k - 1];
  } else {
    if (k + 2 < nh && starts_at(S[k + 2], E, x, y)) return kNone;
    g = S[k + 1];
  }
  if (left_of(g, eleft, eright) != left_of(h, eleft, eright) || right_of(g, eleft, eright) != right_of(h, eleft, eright)) return kNone;
  return g;
}
RJ_RHD uint32_t pred_of(uint32_t h, const uint32_t* next) {
  const uint32_t n = next[h ^ 1];
  return n == kNone ? kNone : n ^ 1;
}

// ---- 6. heads, leaders, ranks: pointer doubling along pred -------------------------------------------------------
RJ_RHD void walk_init(uint32_t h, const uint32_t* next, Walk* a, Walk* b) {
  const uint32_t p = pred_of(h, next);
  a[h] = b[h] = p == kNone ? Walk{h, 0, h, 1} : Walk{p, 1, p < h ? p : h, 0};
}
// one round, in -> out; true when the walk from i reached its head or the minimum of its window changed.  A walk that
// ended in the round before still has its old state in `out` (written two rounds ago): copied once, then both hold it.
RJ_RHD bool walk_round(uint32_t i, const Walk* in, Walk* out) {
  const Walk a = in[i];
  if (a.done) {
    if (!out[i].done) out[i] = a;
    return false;
  }
  const Walk b = in[a.at];
  const Walk n{b.at, a.cnt + b.cnt, a.mn < b.mn ? a.mn : b.mn, b.done};
  out[i] = n;
  return n.done != 0 || n.mn != a.mn;
}
RJ_RHD bool round_needed(const uint32_t* count, int r) { return r == 0 || count[r - 1] != 0; }
// F = the final states of the first pass: an open walk (done) keeps its head and distance; a closed walk (never done, F.mn
// its smallest half-edge) is opened in front of that leader
RJ_RHD void cut_init(uint32_t h, const Walk* F, const uint32_t* next, Walk* a, Walk* b) {
  const Walk f = F[h];
  Walk n;
  if (f.done)
    n = Walk{f.at, f.cnt, 0, 1};
  else if (f.mn == h)
    n = Walk{h, 0, 1, 1};
  else
    n = Walk{pred_of(h, next), 1, 1, 0};
  a[h] = b[h] = n;
}

// ---- 7. chains ------------------------------------------------------------------------------------------------------
// W = the final states of the second pass: W[h].at the leader of h's walk, W[h].cnt the position of h in it, W[h].mn 1 on
// a closed walk
RJ_RHD bool kept_leader(uint32_t a, const Walk* W) { return W[a].at == a && a < W[a ^ 1].at; }
// h in [0, nh]: total[h]; entry nh closes the scan.  -> true for the leader of a closed chain (the caller counts them)
RJ_RHD bool chain_total(uint64_t h64, uint64_t nh, const Walk* W, const uint32_t* next, Slots* total) {
  if (h64 >= nh || !kept_leader((uint32_t) h64, W)) {
    total[h64] = Slots{0, 0};
    return false;
  }
  const uint32_t h = (uint32_t) h64;
  const bool closed = W[h].mn != 0;
  const uint32_t last = closed ? pred_of(h, next) : h ^ 1;  // (open: h ^ 1 is as far from its head as the walk is long)
  total[h] = Slots{1, (uint64_t) W[last].cnt + 2};
  return closed;
}
// base = the exclusive scan of total[].  h in [0, nh]; entry nh: the counts and the row's last entry
RJ_RHD void chain_place(uint64_t h64, uint64_t nh, const Walk* W, const Slots* base, const Seg* E, const int32_t* eleft, const int32_t* eright,
                        const Out& o, Meta* meta) {
  if (h64 == nh) {
    const Slots all = base[nh];
    meta->counts.n_chains = all.halves;
    meta->counts.n_points = all.points;
    if (!meta->bad && o.row && all.halves <= o.chain_cap) o.row[all.halves] = (uint32_t) all.points;  // (nothing for a rejected input)
    return;
  }
  const uint32_t h = (uint32_t) h64, a = W[h].at;
  if (!kept_leader(a, W)) return;
  const Slots at = base[a];
  const uint64_t n_pts = base[(uint64_t) a + 1].points - at.points, k = W[h].cnt, p = at.points + k;
  int64_t x, y;
  start_of(h, E, &x, &y);
  if (p < o.point_cap) {
    o.xy[2 * p] = x;
    o.xy[2 * p + 1] = y;
  }
  if (k + 2 == n_pts && p + 1 < o.point_cap) {  // the last half-edge of its chain
    start_of(h ^ 1, E, &x, &y);
    o.xy[2 * (p + 1)] = x;
    o.xy[2 * (p + 1) + 1] = y;
  }
  if (h == a && at.halves < o.chain_cap) {
    o.row[at.halves] = (uint32_t) at.points;
    o.left[at.halves] = left_of(h, eleft, eright);
    o.right[at.halves] = right_of(h, eleft, eright);
  }
}

}  // namespace ringmap

#if defined(__HIPCC__)
// rj_rings_map behind its argument checks, on stream st: *result = the device's Meta (counts, the input check's status, the
// round budget).  Allocates and frees its scratch; synchronises the stream once, at the end.
hipError_t rings_map_device(hipStream_t st, const uint32_t* ring_row, const int64_t* ring_xy, uint64_t n_points, const void* ring_face,
                            uint64_t face_stride, uint64_t n_rings, uint32_t flags, const ringmap::Out& out, ringmap::Meta* result);
#endif

}  // namespace rj
