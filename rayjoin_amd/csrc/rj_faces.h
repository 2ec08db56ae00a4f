// rj_faces.h -- the faces of a chain map from its geometry alone (rj_map_faces, include/rayjoin_amd.h; kernels in
// rj_faces.hip): a face number on each side of every chain, computed, not copied; the face records with their exact
// areas; and, where the caller has labels, the check that they describe the same partition.  Integers only, and fully
// determined for every input: no tuning choice below can change a result.
//
// INPUT   xy[2 np], row_index[nc + 1]: a chain map as rj_map_rings takes it, without labels.  Chains meet only at their
//         end points; a chain may have a single point; nc < 2^31, np < 2^32, 2 (np - nc) < 2^32; every coordinate in
//         [-2^46, 2^46).  Optionally in_left[nc], in_right[nc]: the labels to check.
// HALF-CHAINS, INCIDENCES, JUNCTION ORDER, SUCCESSOR, RINGS, AREA2   all as rj_rings.h defines them, with no face
//         involved: the rings are the cycles of the successor permutation, each with its leader (its smallest h) and
//         twice its signed area (int128); they ascend by leader.  A chain whose points are all equal is SKIPPED
//         (n_skipped): in no ring, its left and right are 0.
// KINDS   shell: area2 > 0.  hole: every other ring -- the outside of a connected component, or an isolated tree
//         (area2 = 0).  TOP: a ring's largest (y, x).
// CEILING EDGES   a directed edge u -> v of a ring's walk with v.x < u.x: the ring's side lies below it.  Of the two
//         directions of a map edge exactly one is a ceiling, or neither (vertical and zero-length edges): the ceiling
//         edges are the non-vertical map edges, each read from its right end to its left end, and the ring of one is
//         the ring of the half-chain that walks it that way.
// ABOVE   hole H with top p.  Candidates: the ceiling edges of ALL rings with v.x <= p.x < u.x (half-open: the ray stands
//         at p.x + epsilon, it meets no vertex and no vertical edge) whose height at p.x is strictly above p.y.  The
//         winner: the smallest height, then the smaller slope, then the smaller directed-edge number 2 e + (h & 1), e the
//         map's edge number p - c (the same order as that of the edges' first points, which is what is compared).
//         All exact: polygons::candidate and polygons::lower.  above(H) = the winner's ring; tops rise strictly along
//         above.  Follow it until a shell is reached; a walk that ends with nothing above: H lies in face 0, the
//         unbounded face (n_outer).
// FACES   face k (1-based) is the k-th shell by ascending leader; a hole has the face of the shell its walk reaches
//         (n_holes counts these).  left[c] = the face of the ring of half-chain 2 c, right[c] that of 2 c + 1.
//         n_dangling = the chains that are not skipped and have left == right (bridges and dangles).  Record k - 1: the
//         shell's leader, n_holes, area2 = the shell's plus its holes' = twice the face's area, label (0 without labels).
// LABEL CHECK   label of face k = the given label of its shell's leader half-chain; face 0 has label 0.  n_conflicts =
//         the half-chains that are not skipped and whose given label differs from the label of their computed face.
// TIES    on a map without RJ_CROSS_OVERLAP / RJ_CROSS_EQUAL records no two candidates tie beyond the slope, and the
//         result equals rj_map_rings with one constant label followed by rj_rings_polygons' parent[].
//
// THE GRID   the composition buckets ceiling edges by x-strip alone: with one label a hole tests the whole height of the
//         map.  Here a sparse uniform grid over the ceiling edges, in the manner of rj_crossings.h: the cell of a
//         coordinate is (v + 2^46) >> s; an edge is registered in every cell of the box [v.x, u.x - 1] x [min y, max y];
//         the (cell, first point of the edge) pairs are sorted column-major by (cx << 32) | cy.  The ray from p starts
//         in the cell of p and takes the run of its key; it accepts the run's winner only when that height lies in the
//         cell's band, otherwise it goes to the next non-empty cell of the column (a lower_bound on the sorted keys).
//         Exact: an edge is registered in the cell that holds its height at p.x, so the lowest candidate of all is in
//         the run of its own band's cell, and no lower cell's run holds a candidate with a height in that lower band.
// THE FILLER   the slots are sized by their bound and sorted as a whole, since the count stays on the device; the unused
//         ones hold kNoKey = ~0.  At s = 15 that is also a real key: the cell of x, y in [2^46 - 2^15, 2^46).  Nothing
//         depends on telling the two apart: no key is larger, so the fillers sort behind every other key; the sort is
//         stable and the fillers stand behind the registrations before it, so they sort behind the corner cell's too;
//         and every search and every run is bounded by n_regs, not by the slots.  The run of the largest key ends at
//         n_regs (it has no key + 1 to search for).
// UNITS   a cell is at least 2^15 units wide (the floor of s), and the grid only separates what lies in different
//         cells: a map drawn in single units falls into one cell and every hole tests every ceiling edge -- the same
//         answer, at holes x edges.  Coordinates are expected scaled to the range.
// CHOICE OF s   on the device (the call waits for the device once, at its end): the smallest s in 15..47 with
//         2^s >= kExtentFactor x the mean extent max(|dx|, |dy|) of the ceiling edges and at most
//         kRegFactor E + kRegSlack registrations (E ceiling edges; s = 47 has one cell: it always exists).  A forced
//         shift replaces the extent rule and starts the search there; the registration bound still holds, so a
//         domain-wide edge only forces a coarser shift.
//
// Every step is one function per element that rj_faces.hip runs as a grid-stride kernel and tests/hosttwin/faces_twin.cc
// runs as a plain loop (a test-only twin, never a fallback):
//
//   (the ring stages of rj_rings.h, left and right null, without points: rings[], ring_first[], ring_half[])
//   last_mark     per chain: its last point starts no edge
//   chain top     per chain, by a lane group (polygons::ring_top over the chain's points: both half-chains have them)
//   slot_seg      per half-chain slot of the rings' CSR: its ring (a binary search of ring_first), ring_of_half, the
//                 chain's top (inclusive segmented max-scan: the last slot of a ring holds the ring's top)
//   ring_kind     per ring
//   edge_scan     per point: is its edge a ceiling; its extent; its registrations under every shift
//   pick_shift    once
//   reg_count / reg_at   per point its registrations under that shift (exclusive scan), then per registration its edge by
//                 a binary search of the scan and its cell key  (radix sort of the pairs)
//   ray_walk      per hole, by a lane group: the cells of its column upwards, run by run; polygons::lower reduces
//   polygons::jump_init / jump_round   pointer jumping over above
//   polygons::poly_key / member_mark / member_place   the members sorted by shell, the areas scanned
//   face_number / face_emit   per member start: the shell's face number; per face its record
//   half_face     per half-chain: its face to left / right; the dangling chains; the label check
//
// Scratch per call, allocated and freed: per chain 352 bytes of the ring stages plus 2 x (32 ring record + 4 + 4 the
// rings' CSR + 4 ring_of_half + 64 slot tops and their scan + 4 kind + 16 jump states + 16 member keys and their sorted
// form + 12 polygon starts + 32 areas and their scan + 4 face number) = 384, and 16 for the chain's top; per point 17
// (last mark 1, registration count and offset 16); per registration slot (4 (np - nc) + 1024 of them) 24 (key and point,
// with their sorted form); plus the sorts' and scans' temporary storage.
#pragma once
#include <stdint.h>

#include "rj_crossings.h"
#include "rj_polygons.h"
#include "rj_rings.h"

namespace rj {
namespace faces {

using polygons::Edge;
using polygons::Jump;
using polygons::Top;
using rings::Ring;
using rings::U128;

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kNoKey = ~0ull;  // the filler of the unused registration slots, and the largest key (THE FILLER above)
constexpr int kMinShift = 15, kMaxShift = 47, kShifts = kMaxShift - kMinShift + 1;
constexpr int kMaxRounds = 33;
constexpr int64_t kHalfRange = (int64_t) 1 << 46;
constexpr uint64_t kExtentFactor = 8, kRegFactor = 4, kRegSlack = 1024;
constexpr uint64_t kClamp = crossings::kClamp;

struct Face {  // rj_face (32 bytes)
  uint32_t leader, n_holes;
  int32_t label;
  uint32_t _pad;
  uint64_t area2_lo;
  int64_t area2_hi;
};
struct Counts {  // rj_faces_counts
  uint64_t n_faces, n_rings, n_holes, n_outer, n_skipped, n_dangling, n_conflicts;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage), next to the
// ring stages' rings::Meta and the member stages' polygons::Meta
struct Meta {
  uint32_t shift, _pad;
  uint64_t n_ceil;                 // E: the ceiling edges
  uint64_t n_regs;                 // their registrations under `shift`: at most reg_cap
  uint64_t regs[kShifts];          // ... under every shift, exact below kClamp
  uint64_t extent_lo, extent_hi;   // the sums of the low 32 bits and of the bits above them of every extent
  uint64_t ray_tests, cells;       // candidate tests made; cells that rays visited
  Counts counts;
};
// a half-chain slot of the rings' CSR under the segmented max-scan: the largest top of its ring so far
struct alignas(16) SegTop {
  Top top;
  uint32_t ring, _pad[3];
};

RJ_RHD uint64_t reg_cap(uint64_t ne) { return kRegFactor * ne + kRegSlack; }
RJ_RHD int32_t label_of(uint32_t h, const int32_t* in_left, const int32_t* in_right) { return (h & 1) ? in_right[h >> 1] : in_left[h >> 1]; }

// ---- 1. tops ---------------------------------------------------------------------------------------------
// islast[] zeroed before
RJ_RHD void last_mark(uint64_t c, const uint32_t* row, uint8_t* islast) { islast[row[c + 1] - 1] = 1; }
// the ring of half-chain slot s: the last r with ring_first[r] <= s (ring_first[0] = 0, s < ring_first[n_rings])
RJ_RHD uint32_t slot_ring(uint64_t s, const uint32_t* ring_first, uint64_t n_rings) {
  uint64_t lo = 0, hi = n_rings;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (ring_first[mid] <= s)
      lo = mid;
    else
      hi = mid;
  }
  return (uint32_t) lo;
}
// ring_of_half[] preset to kNone (the half-chains of skipped chains keep it)
RJ_RHD void slot_seg(uint64_t s, const uint32_t* ring_first, const uint32_t* ring_half, uint64_t n_rings, const Top* chain_top,
                     uint32_t* ring_of_half, SegTop* seg) {
  const uint32_t r = slot_ring(s, ring_first, n_rings), h = ring_half[s];
  ring_of_half[h] = r;
  seg[s] = SegTop{chain_top[h >> 1], r, {0, 0, 0}};
}
// the operator of the inclusive scan: slots of one ring are neighbours
RJ_RHD SegTop seg_max(const SegTop& a, const SegTop& b) {
  return a.ring == b.ring && polygons::top_before(b.top.x, b.top.y, a.top.x, a.top.y) ? a : b;
}
RJ_RHD uint32_t ring_kind(const Ring& g) {
  return g.area2_hi > 0 || (g.area2_hi == 0 && g.area2_lo != 0) ? polygons::kKindShell : polygons::kKindHole;
}

// ---- 2. the grid -----------------------------------------------------------------------------------------
RJ_RHD uint64_t cell_of(int64_t v, int s) { return (uint64_t) (v + kHalfRange) >> s; }
// the map edge that starts at point pt, read as a ceiling edge: u its end with the larger x
RJ_RHD Edge edge_up(uint64_t pt, const int64_t* xy) {
  const int64_t ax = xy[2 * pt], ay = xy[2 * pt + 1], bx = xy[2 * pt + 2], by = xy[2 * pt + 3];
  return ax > bx ? Edge{ax, ay, bx, by} : Edge{bx, by, ax, ay};
}
RJ_RHD bool ceiling_at(uint64_t pt, const uint8_t* islast, const int64_t* xy, Edge* e) {
  if (islast[pt]) return false;
  *e = edge_up(pt, xy);
  return e->vx < e->ux;
}
RJ_RHD uint64_t reg_count(const Edge& e, int s) {
  const uint64_t w = cell_of(e.ux - 1, s) - cell_of(e.vx, s) + 1;
  const uint64_t h = cell_of(e.uy < e.vy ? e.vy : e.uy, s) - cell_of(e.uy < e.vy ? e.uy : e.vy, s) + 1;
  const unsigned __int128 n = (unsigned __int128) w * h;
  return n < kClamp ? (uint64_t) n : kClamp;
}
RJ_RHD uint64_t clamp_add(uint64_t a, uint64_t b) { return a + b < kClamp ? a + b : kClamp; }  // (a, b <= kClamp)
// per point: -> is its edge a ceiling edge; then acc[k] += its registrations under shift kMinShift + k (clamped), ext += its extent
RJ_RHD bool edge_scan(uint64_t pt, const uint8_t* islast, const int64_t* xy, uint64_t* acc, uint64_t* ext_lo, uint64_t* ext_hi) {
  Edge e;
  if (!ceiling_at(pt, islast, xy, &e)) return false;
  for (int k = 0; k < kShifts; k++) acc[k] = clamp_add(acc[k], reg_count(e, kMinShift + k));
  const int64_t dx = e.ux - e.vx, dy = e.uy < e.vy ? e.vy - e.uy : e.uy - e.vy;
  const uint64_t ext = (uint64_t) (dx < dy ? dy : dx);
  *ext_lo += ext & 0xFFFFFFFFull;
  *ext_hi += ext >> 32;
  return true;
}
// once, behind the sums.  forced: 0, or the shift at which the search starts in place of the extent rule
RJ_RHD void pick_shift(Meta* meta, int forced) {
  const unsigned __int128 total = ((unsigned __int128) meta->extent_hi << 32) + meta->extent_lo;
  for (int s = forced ? forced : kMinShift; s <= kMaxShift; s++) {
    const bool wide = forced || ((unsigned __int128) meta->n_ceil << s) >= kExtentFactor * total;
    if ((wide && meta->regs[s - kMinShift] <= reg_cap(meta->n_ceil)) || s == kMaxShift) {
      meta->shift = (uint32_t) s;
      meta->n_regs = meta->regs[s - kMinShift];
      return;
    }
  }
}
RJ_RHD uint64_t reg_count_at(uint64_t pt, const uint8_t* islast, const int64_t* xy, int s) {
  Edge e;
  return ceiling_at(pt, islast, xy, &e) ? reg_count(e, s) : 0;
}
// registration r: off[] = the exclusive scan of the points' counts (np + 1 entries, off[np] their sum).  Its edge starts
// at the last pt with off[pt] <= r; the cells of the edge's box are numbered column by column.
RJ_RHD void reg_at(uint64_t r, const uint64_t* off, uint64_t np, const int64_t* xy, int s, uint64_t* key, uint32_t* val) {
  uint64_t lo = 0, hi = np;  // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  const Edge e = edge_up(lo, xy);
  const uint64_t x0 = cell_of(e.vx, s), y0 = cell_of(e.uy < e.vy ? e.uy : e.vy, s), y1 = cell_of(e.uy < e.vy ? e.vy : e.uy, s);
  const uint64_t k = r - off[lo], h = y1 - y0 + 1;
  *key = ((x0 + k / h) << 32) | (y0 + k % h);
  *val = (uint32_t) lo;
}

// ---- 3. the first ceiling edge above a top --------------------------------------------------------------------
// the winner of two winners (first points of edges; kNone: no candidate)
RJ_RHD uint32_t lower_pt(uint32_t sa, uint32_t sb, int64_t px, const int64_t* xy) {
  if (sa == kNone || sb == kNone) return sa == kNone ? sb : sa;
  return polygons::lower(edge_up(sa, xy), sa, edge_up(sb, xy), sb, px) ? sa : sb;
}
// lane `lane` of `width`: the winner among entries at + lane, at + lane + width, ... of the run of `key` that starts at `at`
RJ_RHD uint32_t run_scan(uint64_t at, uint64_t key, uint32_t lane, uint32_t width, const Top& p, const uint64_t* keys, const uint32_t* vals,
                         uint64_t n, const int64_t* xy) {
  uint32_t best = kNone;
  Edge be{0, 0, 0, 0};
  for (uint64_t k = at + lane; k < n && keys[k] == key; k += width) {
    const uint32_t pt = vals[k];
    const Edge e = edge_up(pt, xy);
    if (!polygons::candidate(e, p)) continue;
    if (best == kNone || polygons::lower(e, pt, be, best, p.x)) {
      best = pt;
      be = e;
    }
  }
  return best;
}
// does the height of candidate edge pt at px lie in the band of cell row cy
RJ_RHD bool in_band(uint32_t pt, int64_t px, int s, uint64_t cy, const int64_t* xy) {
  const Edge e = edge_up(pt, xy);
  uint64_t rem;
  const int64_t floor_height = e.vy + polygons::floor_div((__int128) (e.uy - e.vy) * (px - e.vx), e.ux - e.vx, &rem);
  return cell_of(floor_height, s) == cy;
}
// all lanes of a group, in step: the cells of p's column from p's own upwards, run by run.  reduce(best) -> the winner
// of the lanes' winners, the same in every lane.  -> the first point of the winning edge, or kNone.  *tests += the
// entries of the runs visited, *cells += their number (the group's, counted by every lane alike)
template <class Reduce>
RJ_RHD uint32_t ray_walk(uint32_t lane, uint32_t width, const Top& p, const uint64_t* keys, const uint32_t* vals, uint64_t n, const int64_t* xy,
                         int s, Reduce reduce, uint64_t* tests, uint64_t* cells) {
  const uint64_t cx = cell_of(p.x, s);
  uint64_t at = polygons::lower_bound(keys, n, (cx << 32) | cell_of(p.y, s));
  while (at < n && (keys[at] >> 32) == cx) {
    // (the largest key of all has no key + 1: its run ends where the entries end, so `end > at` always and the walk ends)
    const uint64_t key = keys[at], end = key == kNoKey ? n : polygons::lower_bound(keys, n, key + 1);
    *tests += end - at;
    *cells += 1;
    const uint32_t best = reduce(run_scan(at, key, lane, width, p, keys, vals, n, xy));
    if (best != kNone && in_band(best, p.x, s, key & 0xFFFFFFFFull, xy)) return best;
    at = end;
  }
  return kNone;
}
// the ring of the ceiling edge that starts at point pt: its chain by a binary search of row_index (the last c with
// row[c] <= pt), the half-chain that walks it from its right end to its left
RJ_RHD uint32_t ring_of_edge(uint32_t pt, const uint32_t* row, uint64_t nc, const int64_t* xy, const uint32_t* ring_of_half) {
  uint64_t lo = 0, hi = nc;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (row[mid] <= pt)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t back = xy[2 * (uint64_t) pt] > xy[2 * (uint64_t) pt + 2] ? 0u : 1u;
  return ring_of_half[2 * (uint32_t) lo + back];
}
// the first state of the jumping for ring r (winner: for a hole, the first point of the edge that won, or kNone)
RJ_RHD void above_init(uint32_t r, uint32_t kind, uint32_t winner, const uint32_t* row, uint64_t nc, const int64_t* xy,
                       const uint32_t* ring_of_half, Jump* a, Jump* b) {
  uint32_t ring = kNone;
  const bool has = kind == polygons::kKindHole && winner != kNone;
  if (has) ring = ring_of_edge(winner, row, nc, xy, ring_of_half);
  polygons::jump_init(r, kind, has ? 0u : kNone, &ring, a, b);
}

// ---- 4. faces ---------------------------------------------------------------------------------------------------
// j a sorted member position where a polygon starts: its shell's face number (1-based) = pid[j] + 1
RJ_RHD void face_number(uint64_t j, const uint64_t* skeys, const uint32_t* start, const uint32_t* pid, uint32_t* face_of_ring) {
  if (skeys[j] != kNoKey && start[j]) face_of_ring[polygons::member_ring(skeys[j])] = pid[j] + 1;
}
// k in [0, n_faces): nothing beyond cap
RJ_RHD void face_emit(uint64_t k, const uint64_t* skeys, const uint32_t* first, const U128* xbase, const Ring* rings, const int32_t* in_left,
                      const int32_t* in_right, Face* out, uint64_t cap) {
  if (k >= cap) return;
  const uint32_t b = first[k], e = first[k + 1];
  const U128 a2 = rings::sub(xbase[e], xbase[b]);
  const uint32_t leader = rings[(uint32_t) (skeys[b] >> 32)].leader;
  out[k] = Face{leader, e - b - 1, in_left ? label_of(leader, in_left, in_right) : 0, 0, a2.lo, (int64_t) a2.hi};
}
// the face of ring r (J = the final states of the jumping)
RJ_RHD uint32_t ring_face(uint32_t r, const Jump* J, const uint32_t* face_of_ring) {
  const Jump j = J[r];
  return j.state == polygons::kFound ? face_of_ring[j.to] : 0;
}
// per half-chain: its face to left / right; -> bit 0: chain h >> 1 is dangling (told by its even half-chain), bit 1: a conflict
RJ_RHD uint32_t half_face(uint32_t h, const uint32_t* ring_of_half, const Jump* J, const uint32_t* face_of_ring, const Ring* rings,
                          const int32_t* in_left, const int32_t* in_right, int32_t* left, int32_t* right) {
  const uint32_t r = ring_of_half[h];
  const uint32_t f = r == kNone ? 0 : ring_face(r, J, face_of_ring);
  if (h & 1)
    right[h >> 1] = (int32_t) f;
  else
    left[h >> 1] = (int32_t) f;
  if (r == kNone) return 0;
  uint32_t what = 0;
  if (!(h & 1) && ring_face(ring_of_half[h ^ 1], J, face_of_ring) == f) what |= 1;
  if (in_left) {
    const int32_t want = f == 0 ? 0 : label_of(rings[J[r].to].leader, in_left, in_right);
    if (label_of(h, in_left, in_right) != want) what |= 2;
  }
  return what;
}

}  // namespace faces

#if defined(__HIPCC__)
// what a call reports besides its counts
struct FacesReport : StageMs {  // the ring stages; tops and kinds; the grid; the rays; parents and faces; all
  int shift;
  uint64_t registrations, ray_tests, cells;
};
// rj_map_faces behind its argument checks, on stream st (nc > 0).  *rmeta: the ring stages' Meta (the map check's status,
// the round budget); *pmeta: the jumping's round budget; *result: the counts.  Allocates and frees its scratch;
// synchronises the stream once, at the end.
hipError_t map_faces_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const int32_t* in_left,
                            const int32_t* in_right, int forced_shift, uint64_t face_cap, int32_t* left, int32_t* right, faces::Face* faces_out,
                            rings::Meta* rmeta, polygons::Meta* pmeta, faces::Meta* result, FacesReport* report);
#endif

}  // namespace rj
