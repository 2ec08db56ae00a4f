// rj_neighbours.h -- the face adjacency table of a chain map (rj_map_neighbours, include/rayjoin_amd.h; kernels in
// rj_neighbours.hip): which faces touch which, along how much border and at how many nodes -- what GIS users know as
// Polygon Neighbors, and the input of rook and queen contiguity weights.  A chain-level call with one pass over the
// points.  Integers only, exact, and fully determined: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1], left[nc], right[nc]: a labelled chain map with the contract, the checks and the size
//         limits of rj_map_eliminate (rj_eliminate.h; a chain may have a single point).  Labels are any int32.  Under
//         kVertex also nc < 2^30: the 4 nc incidences below are numbered in 32 bits.  The point array is 16-byte aligned
//         (device allocations are).
// FACES, S(c), L(c), area2(f)   exactly rj_eliminate.h's: a face is a label value other than 0 that occurs in left or
//         right, faces are numbered by ascending (uint32_t) label, S(c) is the sum of eliminate::edge_cross and L(c) the sum
//         of eliminate::edge_length (exact integer square roots) over the edges of chain c, area2(f) the sum of S(c) over
//         left[c] == f minus the sum over right[c] == f.  n_sides(f) = the chain sides that carry f (a chain with f on both
//         sides has two).
// EDGE NEIGHBOURS (rook)   eliminate's NEIGHBOURS: faces f != g, both not 0, are edge neighbours when some chain has
//         {left, right} = {f, g};  w(f, g) = the sum of L(c) over those chains, n_chains(f, g) their number.  A pair with
//         w = 0 is still a pair (a chain whose points are all equal gives one).  Chains with left == right contribute
//         nothing to any length.
// LENGTHS OF A FACE   perimeter(f) = the sum of L(c) over the chains with left != right and one side equal to f (the other
//         side may be 0);  outer(f) = the part of that sum whose other side is 0.  So perimeter(f) = outer(f) + the sum
//         of w(f, g) over g.
// NODES, VERTEX NEIGHBOURS (queen), under kVertex   A NODE IS A CHAIN END: a distinct point that is the first or the last
//         point of some chain (a chain of one point and a closed chain give their point once).  Points inside a chain are
//         never looked at, so the call is meant for noded maps whose shared vertices are chain ends -- what rj_rings_map,
//         rj_map_node, rj_map_snap and rj_map_dissolve produce.  A pseudo-node of degree 2 counts as a node: rj_map_dissolve
//         with RJ_DISS_KEEP_EQUAL (Join) first for canonical node counts.  F(P) = the set of nonzero labels on either
//         side of any chain that has P as an end point.  Faces f != g MEET AT P when both are in F(P);  n_nodes(f, g) = the
//         distinct nodes where they meet.  A pair with n_nodes > 0 and n_chains = 0 is a VERTEX-ONLY neighbour (the
//         diagonal cells of a checkerboard corner).  Without kVertex no node is looked at: every n_nodes and
//         n_vertex_nbrs is 0 and so are the counts n_vertex_pairs, n_nodes, n_node_pairs_raw and max_labels_at_node.
// OUTPUT  CSR over the faces.  Record k of the k-th face: its label, n_sides, n_edge_nbrs (neighbours with n_chains > 0),
//         n_vertex_nbrs (vertex-only neighbours), area2 (int128), perimeter and outer (unsigned 128-bit).
//         offsets[k] = where the entries of face k start, offsets[n_faces] = n_entries.  An entry: the neighbour's label and
//         face number, n_chains, n_nodes, w; the entries of a face ascend by the neighbour's (uint32_t) label, and every
//         pair appears in both directions with equal values.  Counts: n_faces, n_entries (directed), n_edge_pairs and
//         n_vertex_pairs (unordered), n_nodes, n_node_pairs_raw = the sum over nodes of m (m - 1) with m = |F(P)| (what the
//         call has to sort), max_labels_at_node = the largest m.
// LIMIT   n_node_pairs_raw < 2^32 (kMaxRawPairs): a call above it is refused with the count reported (the sum saturates
//         at 2^64 - 1).  A hub of 65 537 faces at one vertex is refused, one of 65 536 is just below.  Below the limit
//         the PRACTICAL limit is memory: 56 bytes of scratch per raw node pair, so the device's memory is full long before
//         2^32 pairs (240 GB), and the call then fails with the allocation's error, not with a refusal that names the
//         count.  The largest run so far sorted 2 nc + n_node_pairs_raw = 19.7 M keys (profiles/neighbours_fullsize.txt);
//         nothing above 2^32 keys in one rocPRIM call has been run.
//
// Every step is one function per element that rj_neighbours.hip runs as a kernel and tests/hosttwin/neighbours_twin.cc runs
// as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate (rj_rings.h)   the input check: the largest code met is the status
//   chain_sums    per chain, lane l of w: the points l, l + w, ... -- their check, their edges' cross products and lengths
//                 (summed over the lanes: integer sums commute)
//   eliminate::side_key / side_val / face_add   per chain side i = 2 c + s: the sort key of its label; +S or -S, 1, L where
//                 left != right, L where the other side is 0
//   (sort by key, sum by key: the labels ascending with area2, sides, perimeter and outer; label 0, if any, is the last key)
//   eliminate::directed_key / edge_val / pair_add   per chain side: (f << 32) | g with {L, 1, 0}, kNoPair where it separates nothing
//   end_point / inc_key / inc_before   under kVertex, per incidence j = 4 c + 2 e + s (e = 0 the first point of chain c, 1
//                 the last; s = 0 left, 1 right): its point, the key of its label; the order (point, key) -- label 0 is
//                 the last key of its point
//   (merge sort of the 4 nc incidences by inc_before)
//   inc_flags     per sorted position: HEAD the first of its point (a node), UNIQ the first of its (point, nonzero label)
//   (exclusive scan of {UNIQ, HEAD}: the slot u of a distinct (node, label) and the number of its node)
//   inc_place     per sorted position: face and node of slot u; the first slot of every node
//   labels_at / pair_count   per slot: m = |F(P)| of its node (a difference of two node starts), its m - 1 directed pairs
//   (saturating exclusive scan of the pair counts: where a slot writes; the total is n_node_pairs_raw -- the host reads it
//   here, in the one extra sync that kVertex costs, refuses a call at the limit and sizes the scratch of the pairs)
//   node_pairs    per slot: (f << 32) | g with {0, 0, 1} for every other slot g of its node -- a hub of hundreds of faces is
//                 a long run, and no loop is bounded by a degree cap
//   (one sort of the edge keys and the node keys together, one sum by key: every directed pair once, ascending by f, then g)
//   count_entries / is_edge / from_of   per directed pair: the face whose n_edge_nbrs or n_vertex_nbrs it adds to
//   face_offset   per face, and once for n_faces: the first directed pair not below (k << 32) -- a binary search
//   face_record / entry_of   per face, per directed pair
//
// The sorts move 4-byte side numbers, never the sums: side_val and pair_val are read where the sums by key need them.
//
// Scratch per call, allocated and freed: per chain 32 bytes (S, L); per chain SIDE (2 nc of them) 92 bytes -- the face
// sort's keys and side numbers in and out and the unique keys (20), the sums of every face (64), its two counters (8);
// per DIRECTED KEY 56 bytes -- keys in, out and unique (24), side numbers in and out (8), the sums (24).  Rook only there
// are 2 nc directed keys: 328 bytes per chain.  Under kVertex per chain side 28 bytes more (the edge keys until the node
// pairs are known 8, the end point 16, the node's first slot 4) and per INCIDENCE (4 nc) 48 bytes (the key and the order
// 8, the face and node of a slot 8, the flags and their scan 16, the pair count and its scan 16): 576 bytes per chain, and
// the 56 bytes of a directed key per RAW NODE PAIR.  Plus rocPRIM's temporary storage.
#pragma once
#include <stdint.h>

#include "rj_dissolve.h"
#include "rj_eliminate.h"

namespace rj {
namespace neighbours {

using dissolve::Pt;
using rings::U128;
typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr uint32_t kVertex = 1u;  // RJ_NB_VERTEX
constexpr uint32_t kZeroKey = eliminate::kZeroKey;
constexpr uint64_t kNoPair = eliminate::kNoPair;
constexpr uint64_t kMaxRawPairs = 1ull << 32;  // n_node_pairs_raw stays below
constexpr uint32_t kUniq = 1u, kHead = 2u;     // inc_flags
constexpr uint32_t kNoSide = 0xFFFFFFFFu;      // the chain side of a directed key that a node gave (there are 2 nc < 2^32 - 1 sides)

struct Face {  // rj_nb_face (64 bytes)
  int32_t label;
  uint32_t n_sides, n_edge_nbrs, n_vertex_nbrs;
  uint64_t area2_lo;
  int64_t area2_hi;
  uint64_t perimeter_lo, perimeter_hi, outer_lo, outer_hi;
};
struct Entry {  // rj_nb_entry (32 bytes)
  int32_t label;
  uint32_t face, n_chains, n_nodes;
  uint64_t w_lo, w_hi;
};
struct Counts {  // rj_neighbours_counts
  uint64_t n_faces, n_entries, n_edge_pairs, n_vertex_pairs, n_nodes, n_node_pairs_raw, max_labels_at_node;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t bad;         // the input check's status (rings::kBad*); not 0: nothing further is written
  uint32_t emit;        // 1: every output fits its capacity and is written
  uint32_t max_labels;  // the largest |F(P)|
  uint32_t pad;
  uint64_t n_keys;      // unique label keys (the faces, and label 0 where it occurs)
  uint64_t n_dir;       // unique directed keys (the directed pairs, and kNoPair where a chain side separates nothing)
  uint64_t n_slots;     // distinct (node, nonzero label)
  Counts counts;
};
struct FaceSum {  // what a face sums over its sides (64 bytes)
  U128 area2, perimeter, outer;
  uint64_t n, pad;
};
struct PairSum {  // what a directed pair sums (24 bytes)
  uint64_t w_lo, w_hi;
  uint32_t n_chains, n_nodes;
};
struct Flags {  // the scan over the sorted incidences: slots and nodes in front
  uint32_t uniq, head;
};

RJ_RHD bool refused(const Meta& m) { return m.bad != 0 || m.counts.n_node_pairs_raw >= kMaxRawPairs; }

// ---- 1. the check and the chain sums ---------------------------------------------------------------------------------
RJ_RHD Pt load_point(const int64_t* xy, uint64_t p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const longlong2 v = *reinterpret_cast<const longlong2*>(xy + 2 * p);  // (one 16-byte access: device point arrays are 16-byte aligned)
  return Pt{v.x, v.y};
#else
  return Pt{xy[2 * p], xy[2 * p + 1]};
#endif
}
// lane `lane` of `width`: the points lane, lane + width, ... of chain c with the edges that start there.  Reads nothing
// where row[] does not give a range inside the np points (the check of a malformed row says so elsewhere).
RJ_RHD void chain_sums(uint64_t c, uint32_t lane, uint32_t width, const int64_t* xy, const uint32_t* row, uint64_t np, uint32_t* bad, i128* S, u128* L) {
  const uint64_t b = row[c], e = row[c + 1];
  if (!(b < e && e <= np)) return;
  for (uint64_t p = b + lane; p < e; p += width) {
    const Pt a = load_point(xy, p);
    const uint32_t bx = rings::check_coordinate(a.x), by = rings::check_coordinate(a.y);
    *bad = *bad > bx ? *bad : bx;
    *bad = *bad > by ? *bad : by;
    if (p + 1 < e && !bx && !by) {
      const Pt q = load_point(xy, p + 1);
      if (rings::check_coordinate(q.x) || rings::check_coordinate(q.y)) continue;  // (refused by the lane of that point: no length of a wild edge)
      *S += eliminate::edge_cross(a.x, a.y, q.x, q.y);
      *L += eliminate::edge_length(a.x, a.y, q.x, q.y);
    }
  }
}
RJ_RHD U128 limbs(u128 v) { return U128{(uint64_t) v, (uint64_t) (v >> 64)}; }

// ---- 2. faces ---------------------------------------------------------------------------------------------------------
// chain side i = 2 c + s (s = 0 left, 1 right)
RJ_RHD FaceSum side_val(uint64_t i, const int32_t* left, const int32_t* right, const U128* S, const U128* L) {
  const int32_t mine = eliminate::side_label(i, left, right), other = eliminate::side_label(i ^ 1, left, right);
  const U128 zero{0, 0}, len = L[i >> 1];
  return FaceSum{eliminate::side_sum(i, S), mine != other ? len : zero, mine != other && other == 0 ? len : zero, 1, 0};
}
RJ_RHD FaceSum face_add(const FaceSum& a, const FaceSum& b) {
  return FaceSum{rings::add(a.area2, b.area2), rings::add(a.perimeter, b.perimeter), rings::add(a.outer, b.outer), a.n + b.n, 0};
}

// ---- 3. edge pairs ------------------------------------------------------------------------------------------------------
RJ_RHD PairSum edge_val(uint64_t i, const U128* L) { return PairSum{L[i >> 1].lo, L[i >> 1].hi, 1, 0}; }
// what a directed key adds: the key of chain side `side` its chain's length and one chain, the key of a node (kNoSide) one node
RJ_RHD PairSum pair_val(uint32_t side, const U128* L) { return side == kNoSide ? PairSum{0, 0, 0, 1} : edge_val(side, L); }
RJ_RHD PairSum pair_add(const PairSum& a, const PairSum& b) {
  const U128 w = rings::add(U128{a.w_lo, a.w_hi}, U128{b.w_lo, b.w_hi});
  return PairSum{w.lo, w.hi, a.n_chains + b.n_chains, a.n_nodes + b.n_nodes};
}

// ---- 4. nodes -------------------------------------------------------------------------------------------------------------
// chain end h = 2 c + e: the first point of chain c for e = 0, its last point for e = 1 (dissolve's half-chain start points)
RJ_RHD Pt end_point(uint64_t h, const int64_t* xy, const uint32_t* row) {
  const uint64_t p = (h & 1) ? (uint64_t) row[(h >> 1) + 1] - 1 : row[h >> 1];
  return Pt{xy[2 * p], xy[2 * p + 1]};
}
// incidence j = 2 h + s: the label on side s of the chain of end h
RJ_RHD uint32_t inc_key(uint64_t j, const int32_t* left, const int32_t* right) { return eliminate::side_key(((j >> 2) << 1) | (j & 1), left, right); }
// the order of the sort: (point, key, j) -- dissolve's order on points; label 0 has the last key.  Strict and total.
RJ_RHD bool inc_before(uint32_t ja, uint32_t jb, const Pt* pts, const uint32_t* key) {
  const Pt a = pts[ja >> 1], b = pts[jb >> 1];
  if (a.x != b.x) return a.x < b.x;
  if (a.y != b.y) return a.y < b.y;
  if (key[ja] != key[jb]) return key[ja] < key[jb];
  return ja < jb;
}
// sorted position k
RJ_RHD uint32_t inc_flags(uint64_t k, const uint32_t* order, const Pt* pts, const uint32_t* key) {
  const uint32_t j = order[k];
  bool head = k == 0, other_key = true;
  if (!head) {
    const uint32_t i = order[k - 1];
    head = pts[i >> 1].x != pts[j >> 1].x || pts[i >> 1].y != pts[j >> 1].y;
    other_key = key[i] != key[j];
  }
  return (head ? kHead : 0u) | (key[j] != kZeroKey && (head || other_key) ? kUniq : 0u);
}
RJ_RHD Flags flags_val(uint32_t f) { return Flags{(f & kUniq) ? 1u : 0u, (f & kHead) ? 1u : 0u}; }
RJ_RHD Flags flags_add(const Flags& a, const Flags& b) { return Flags{a.uniq + b.uniq, a.head + b.head}; }
// before = the exclusive scan of the flags at position k.  A head gives the first slot of its node (the node may have no
// slot: every label at it is 0), a uniq fills its slot: the face of its label and its node.
RJ_RHD void inc_place(uint64_t k, const uint32_t* order, const uint32_t* key, const Flags* mine, const Flags* before, const uint32_t* keys, uint64_t nf,
                      uint32_t* slot_face, uint32_t* slot_node, uint32_t* node_start) {
  const uint32_t u = before[k].uniq, node = before[k].head + mine[k].head - 1u;  // (position 0 is a head: never -1)
  if (mine[k].head) node_start[node] = u;
  if (mine[k].uniq) {
    slot_face[u] = eliminate::face_index(eliminate::label_of(key[order[k]]), keys, nf);
    slot_node[u] = node;
  }
}
// node_start has n_nodes + 1 entries, the last n_slots.  -> m = |F(P)| of the node of slot u
RJ_RHD uint32_t labels_at(uint64_t u, const uint32_t* slot_node, const uint32_t* node_start) {
  return node_start[slot_node[u] + 1] - node_start[slot_node[u]];
}
RJ_RHD uint64_t saturating_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
// slot u writes its m - 1 pairs from `at` on: every other face of its node, ascending
RJ_RHD void node_pairs(uint64_t u, const uint32_t* slot_face, const uint32_t* slot_node, const uint32_t* node_start, uint64_t at, uint64_t* key, uint32_t* side) {
  const uint64_t b = node_start[slot_node[u]], e = node_start[slot_node[u] + 1], f = slot_face[u];
  for (uint64_t v = b; v < e; v++) {
    if (v == u) continue;
    key[at] = (f << 32) | slot_face[v];
    side[at] = kNoSide;
    at++;
  }
}

// ---- 5. the table --------------------------------------------------------------------------------------------------------
// dir[n_dir]: the unique directed keys, ascending; kNoPair, if any, is the last
RJ_RHD uint64_t count_entries(uint64_t n_dir, const uint64_t* dir) { return n_dir - (n_dir && dir[n_dir - 1] == kNoPair ? 1 : 0); }
RJ_RHD bool is_edge(const PairSum& v) { return v.n_chains != 0; }
// where the entries of face k start: the first directed pair that is not below (k << 32); k = n_faces gives n_entries
RJ_RHD uint64_t face_offset(uint64_t k, const uint64_t* dir, uint64_t n_entries) {
  const uint64_t want = k << 32;
  uint64_t lo = 0, hi = n_entries;  // dir[lo - 1] < want <= dir[hi]
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (dir[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
RJ_RHD Face face_record(uint64_t k, const uint32_t* keys, const FaceSum* sums, const uint32_t* n_edge, const uint32_t* n_vertex) {
  const FaceSum& s = sums[k];
  return Face{eliminate::label_of(keys[k]), (uint32_t) s.n, n_edge[k], n_vertex[k], s.area2.lo, (int64_t) s.area2.hi, s.perimeter.lo, s.perimeter.hi,
              s.outer.lo, s.outer.hi};
}
RJ_RHD Entry entry_of(uint64_t i, const uint64_t* dir, const PairSum* sums, const uint32_t* keys) {
  const uint32_t g = eliminate::to_of(dir[i]);
  return Entry{eliminate::label_of(keys[g]), g, sums[i].n_chains, sums[i].n_nodes, sums[i].w_lo, sums[i].w_hi};
}
// every output fits (the offsets have face_cap + 1 entries, with or without records)
RJ_RHD bool fits(const Counts& c, uint64_t face_cap, uint64_t entry_cap) { return c.n_faces <= face_cap && c.n_entries <= entry_cap; }

}  // namespace neighbours

#if defined(__HIPCC__)
// what a call reports besides its counts
struct NeighboursReport : StageMs {};  // check and chain sums; faces; edge pairs; nodes; the table; all
// rj_map_neighbours behind its argument checks, on stream st: *result = the device's Meta.  point_blocks: the grid of the
// pass over the points (0: by size; any grid gives the same result).  Allocates and frees its scratch; synchronises the
// stream once, at the end, and under kVertex once more, behind the node stage: the host reads n_node_pairs_raw there,
// refuses a call at the limit and sizes the scratch of the node pairs.
hipError_t map_neighbours_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                                 uint32_t flags, uint64_t face_cap, uint64_t entry_cap, neighbours::Face* faces, uint64_t* offsets, neighbours::Entry* entries,
                                 int point_blocks, neighbours::Meta* result, NeighboursReport* report);
#endif

}  // namespace rj
