// rj_node.h -- noding a chain map (rj_map_node, include/rayjoin_amd.h; kernels in rj_node.hip): every edge is cut at the
// vertices of the map that lie inside it, as the records of rj_map_crossings name them.  T-junctions and half-shared
// borders -- a vertex of one polygon on a border that its neighbour's ring runs straight past -- are what commonly makes
// a polygon layer fail the planar check (kTouch, kOverlap); every point that has to be inserted is already a vertex of
// the map, so the repair is exact in integers, and behind it overlapping edges are equal edges, which rj_rings_map
// stores once.  kProper crossings are counted and left alone (their point is no integer), kEqual needs no cut.
// Integers only, exact, and fully determined: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1]: a chain map with the contract of rj_map_crossings (rj_crossings.h).  Edge
//         e = p - c runs from a (point p) to b (point p + 1) of chain c; ne = np - nc.  rec[n]: the records that
//         rj_map_crossings wrote for this very map: eid[0] < eid[1] < ne, kind in 1..4, no zero-length edge named,
//         strictly ascending by ((uint64) eid[0] << 32) | eid[1]; n < 2^31.
// INSIDE  a point q lies inside e when e is not of zero length, orient(a, b, q) == 0 (an int128 cross product), q is in
//         e's closed box and q is neither a nor b.
// CUTS    C(e): the distinct points q such that some record (e, f) or (f, e) of kind kTouch or kOverlap exists, q is an
//         end point of f and q lies inside e.  The test is made for all four (end point, other edge) combinations of
//         every such record and a cut exists only where it holds: a record whose kind does not fit the geometry cannot
//         put a point off an edge.  At most two of the four hold (one point in common: an end point of one inside the
//         other, once; collinear: when both end points of f lie inside e, no end point of e lies in f): a call has at
//         most 2 n candidates, which sizes their array without a look at the device.
// OUTPUT  every chain keeps its points in order; after point p come the points of C(p - c), ascending by their distance
//         from a -- all lie on the segment, so this is |q.x - a.x|, or |q.y - a.y| on a vertical edge, below 2^47, and
//         equal distances on one edge are equal points, which appear once.  out_row[nc + 1]; chains, their number and
//         their order do not change.  origin[k]: the input edge that output edge k (= p' - c) is a part of.  Under
//         kDropLast every chain must have at least 2 points with the first equal to the last, and is written without
//         its last point: point slot k is then exactly output edge k.
//
// Every step is one function per element that rj_node.hip / rj_cut_pipeline.h run as a grid-stride kernel and
// tests/hosttwin/node_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate (rj_crossings.h) / check_chain / check_record   the input check: the largest code met
//                 is the status; not 0: nothing further is read and nothing is written
//   candidate     per record and t in 0..3: test t, and its cut (edge, source point, distance) where it holds
//   (one merge sort of the candidates by cut_before: (edge, distance, source point); unused slots, all ones, go last)
//   cut_head      per sorted position: is it the first of its run of equal (edge, distance) -- a kept cut
//   (exclusive scan of the flags: the number of a kept cut)
//   run_first / run_last   per sorted position: does its edge's run start / end here; first[e], last[e] = the numbers
//                 of the kept cuts of e (both 0 where there is none): no counter, no atomic
//   (exclusive scan over the edges of last[e] - first[e]: prefix[ne + 1])
//   point_chain / point_slot   per input point p: its chain (a binary search of row_index); its slot p + prefix[p - c]
//   row_slot      per c in [0, nc]: out_row[c] = row[c] + prefix[row[c] - c]
//   cut_slot      per kept cut: the slot of its edge's first point + 1 + its rank among the edge's cuts
//                 (all slots less c under kDropLast)
// No stage is serial in the number of cuts on one edge: an edge with thousands of T-junctions costs as many threads.
//
// Scratch per call: 80 bytes per record (2 candidates of 16 bytes, twice: unsorted and sorted; 2 flags and 2 numbers of
// 4 bytes), 12 bytes per edge (first, last - first, prefix) plus the sort's and the scans' temporary storage; allocated
// per call and freed.
#pragma once
#include <stdint.h>

#include "rj_crossings.h"

namespace rj {
namespace node {

using crossings::Edge;

constexpr uint32_t kDropLast = 1;  // RJ_NODE_DROP_LAST
constexpr uint32_t kNoEdge = 0xFFFFFFFFu;  // an unused candidate slot (ne < 2^32 - 1: no edge has this number)

struct Record {  // rj_crossing
  uint32_t eid[2], kind, pad;
};
struct alignas(16) Cut {
  uint64_t off;   // the distance from the edge's first point: in x, in y on a vertical edge
  uint32_t edge;  // the edge that is cut
  uint32_t src;   // the input point that cuts it
};
struct Counts {  // rj_node_counts
  uint64_t n_points, n_edges, n_cuts, n_cut_edges, n_max_cuts, n_used, n_proper, n_equal;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;   // the input check's status; not 0: nothing is read further
  uint32_t emit;  // 1: the output fits (n_points <= capacity and np + n_cuts < 2^32) and is written
  uint64_t n_cand;
  Counts counts;
};

// ---- 0. the input check ------------------------------------------------------------------------------
// codes above those of the map check (crossings::kBad*, 1..4); the largest met is the status
constexpr uint32_t kBadOpenChain = 5, kBadRecord = 6, kBadZeroEdge = 7, kBadOrder = 8;
// under kDropLast: chain c has two points or more, the first equal to the last (a row that the map check refuses may
// hold anything: nothing is read behind np)
RJ_RHD uint32_t check_chain(uint64_t c, const uint32_t* row, uint64_t np, const int64_t* xy) {
  const uint64_t b = row[c], e = row[c + 1];
  if (e > np || e < b + 2) return kBadOpenChain;
  return xy[2 * b] != xy[2 * e - 2] || xy[2 * b + 1] != xy[2 * e - 1] ? kBadOpenChain : 0;
}
RJ_RHD uint64_t record_key(const Record& r) { return ((uint64_t) r.eid[0] << 32) | r.eid[1]; }
// record r of n (an edge number below ne has its two points inside xy whatever the row holds)
RJ_RHD uint32_t check_record(uint64_t r, const Record* rec, uint64_t ne, const uint32_t* row, uint64_t nc, const int64_t* xy) {
  const Record& R = rec[r];
  if (R.eid[0] >= R.eid[1] || R.eid[1] >= ne || R.kind < crossings::kProper || R.kind > crossings::kEqual) return kBadRecord;
  if (r > 0 && record_key(rec[r - 1]) >= record_key(R)) return kBadOrder;
  return crossings::is_zero(crossings::edge_of(R.eid[0], row, nc, xy)) || crossings::is_zero(crossings::edge_of(R.eid[1], row, nc, xy)) ? kBadZeroEdge : 0;
}

// ---- 1. candidates ---------------------------------------------------------------------------------------
RJ_RHD bool cuts(uint32_t kind) { return kind == crossings::kTouch || kind == crossings::kOverlap; }
RJ_RHD bool inside(const Edge& e, int64_t qx, int64_t qy) {
  return !crossings::is_zero(e) && crossings::orient(e.ax, e.ay, e.bx, e.by, qx, qy) == 0 && crossings::in_box(e, qx, qy) &&
         !crossings::is_end(e, qx, qy);
}
// the distance of a point on e from e's first point
RJ_RHD uint64_t offset_on(const Edge& e, int64_t qx, int64_t qy) {
  const int64_t d = e.ax != e.bx ? qx - e.ax : qy - e.ay;
  return (uint64_t) (d < 0 ? -d : d);
}
// test t of a record of a cutting kind over the edges e < f, whose first points are pe and pf:
// 0: f.a inside e, 1: f.b inside e, 2: e.a inside f, 3: e.b inside f
RJ_RHD bool candidate(int t, uint32_t e, uint32_t f, const Edge& E, const Edge& F, uint64_t pe, uint64_t pf, Cut* cut) {
  const bool into_e = t < 2, second = t & 1;
  const Edge& host = into_e ? E : F;
  const Edge& from = into_e ? F : E;
  const int64_t qx = second ? from.bx : from.ax, qy = second ? from.by : from.ay;
  if (!inside(host, qx, qy)) return false;
  *cut = Cut{offset_on(host, qx, qy), into_e ? e : f, (uint32_t) ((into_e ? pf : pe) + (second ? 1 : 0))};
  return true;
}

// ---- 2. the sort, the kept cuts ----------------------------------------------------------------------------
RJ_RHD bool cut_before(const Cut& a, const Cut& b) {
  if (a.edge != b.edge) return a.edge < b.edge;
  if (a.off != b.off) return a.off < b.off;
  return a.src < b.src;
}
// sorted position i of n: a cut that is the first of its run of equal (edge, distance)
RJ_RHD bool cut_head(uint64_t i, const Cut* s) {
  return s[i].edge != kNoEdge && (i == 0 || s[i - 1].edge != s[i].edge || s[i - 1].off != s[i].off);
}
// does the run of one edge start / end at sorted position i (a cut) of n
RJ_RHD bool run_first(uint64_t i, const Cut* s) { return i == 0 || s[i - 1].edge != s[i].edge; }
RJ_RHD bool run_last(uint64_t i, uint64_t n, const Cut* s) { return i + 1 == n || s[i + 1].edge != s[i].edge; }

// ---- 3. slots --------------------------------------------------------------------------------------------
// the chain of point p: the last c with row[c] <= p (row ascends strictly)
RJ_RHD uint64_t point_chain(uint64_t p, const uint32_t* row, uint64_t nc) {
  uint64_t lo = 0, hi = nc;  // row[lo] <= p < row[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint64_t) row[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// prefix[e]: the cuts on the edges before e; p - c of a chain's last point is the first edge of the next chain (ne behind
// the last): exactly the cuts in front of that point
RJ_RHD uint64_t point_slot(uint64_t p, uint64_t c, const uint32_t* prefix, uint32_t flags) {
  return p + prefix[p - c] - (flags & kDropLast ? c : 0);
}
RJ_RHD uint64_t row_slot(uint64_t c, const uint32_t* row, const uint32_t* prefix, uint32_t flags) { return point_slot(row[c], c, prefix, flags); }
// kept cut number k of edge e of chain c; first[e]: the number of the edge's first kept cut
RJ_RHD uint64_t cut_slot(uint64_t k, uint32_t e, uint64_t c, const uint32_t* first, const uint32_t* prefix, uint32_t flags) {
  return point_slot((uint64_t) e + c, c, prefix, flags) + 1 + (k - first[e]);
}
// the counts behind the scans: n_cuts = the kept cuts
RJ_RHD void totals(uint64_t np, uint64_t nc, uint64_t n_cuts, uint32_t flags, uint64_t capacity, Counts* counts, uint32_t* emit) {
  counts->n_cuts = n_cuts;
  counts->n_edges = np - nc + n_cuts;
  counts->n_points = flags & kDropLast ? counts->n_edges : np + n_cuts;
  *emit = counts->n_points <= capacity && np + n_cuts < (1ull << 32) ? 1 : 0;
}

}  // namespace node

#if defined(__HIPCC__)
// what a call reports besides its counts
struct NodeReport : StageMs {};  // the check; the candidates; the sort and the kept cuts; the cuts per edge and their scan; the two scatters; all
// rj_map_node behind its argument checks, on stream st: *result = the device's Meta (counts, the input check's status,
// whether the output was written).  Allocates and frees its scratch; synchronises the stream once, at the end.
hipError_t map_node_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec, uint64_t n_rec,
                           uint32_t flags, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, node::Meta* result,
                           NodeReport* report);
#endif

}  // namespace rj
