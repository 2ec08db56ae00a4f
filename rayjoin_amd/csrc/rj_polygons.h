// rj_polygons.h -- the polygons of a set of face rings (rj_rings_polygons, include/rayjoin_amd.h; kernels in
// rj_polygons.hip): every hole ring assigned to the outer ring it lies in, every outer ring with its holes and the exact
// area of what they bound.  Integers only, and fully determined for every input, maps with inconsistent labels included.
//
// INPUT   the output of rj_map_rings with points: rings[n_rings] ascending (strictly) by ((uint32) face << 32) | leader,
//         ring_row[n_rings + 1] the CSR into ring_xy[2 n_points], every coordinate in [-2^46, 2^46).  Ring r is a closed
//         walk: point i is followed by i + 1, the last point by the first; its face is on the left of the walk.
//         n_rings <= 2^32 - 2, n_points < 2^32.  face and area2 are taken from the ring records as they stand.
// KINDS   none:  face == 0 -- the outside has no shell; counted in n_face0, in no polygon.
//         shell: face != 0 and area2 > 0.
//         hole:  face != 0 and area2 <= 0 (a ring of area 0 is a dangling tree inside its face: a boundary that the face
//                surrounds).
// TOP     the lexicographically largest (y, x) among a ring's points.  A ring without points has none.
// CEILING EDGES   a directed ring edge u -> v (a point slot and its successor) with v.x < u.x: the ring's face lies below
//         it.  Vertical and zero-length edges are never ceilings.  Only rings of a face != 0 have them.
// THE RING ABOVE A HOLE   hole H of face f with top p.  Its candidates: the ceiling edges of rings of face f (holes and
//         shells alike) with v.x <= p.x < u.x (half-open: the ray stands at p.x + epsilon and never meets a vertex, so
//         there is no vertex case and no vertical-edge case) and with their height at p.x strictly above p.y:
//         (u.y - v.y)(p.x - v.x) > (p.y - v.y)(u.x - v.x) (differences below 2^47, products below 2^94: int128).  The
//         winner: the smallest height at p.x; then the smaller slope (u.y - v.y) / (u.x - v.x), the edge that is lower just
//         right of the ray; then the smaller point slot of u.  All exact: the height is v.y + floor(n / d) + rem / d with
//         n = (u.y - v.y)(p.x - v.x), d = u.x - v.x -- integer parts first, then rem_a d_b against rem_b d_a; slopes
//         by cross-multiplication.  above(H) = the ring that holds the winner, nothing without a candidate (or a top).
//         No edge of H itself is a candidate (none of its points is higher than p), and the ring above has a point
//         strictly higher than p: tops rise strictly along above, it cannot cycle.
// PARENT  follow above from H until it reaches a shell: parent(H).  Where the walk ends at a hole with nothing above it,
//         H is an ORPHAN: no parent, counted in n_orphans (only where the labels are inconsistent: on a consistently
//         labelled planar map the ray from the top of a hole starts inside face f, and the first boundary it crosses
//         has f below it, so it belongs to a ring of the same connected region of f).  A shell is its own parent.
// POLYGONS   one per shell, ascending by shell index (the polygons of a face are contiguous, ordered by leader); members:
//         the shell, then its holes by ascending ring index; area2 = the shell's area2 plus its holes', an int128.
//
// Every step is one function per element that rj_polygons.hip runs as a grid-stride kernel and
// tests/hosttwin/polygons_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_order / check_coordinate   the input check; its status word stays on the device, an input that fails is
//                 not read further
//   ring_top / ring_kind   per ring, by a lane group (rings can have 100 000 points): its top and its kind
//   ring_mark     per ring: its index at its first point slot (inclusive max-scan: the ring of every point slot)
//   edge_strips   per point slot: is its edge a ceiling edge; its (edge, strip) incidences for every shift s in [16, 47],
//                 the strip of x being (uint64) (x + 2^46) >> s, an edge lying in strips strip(v.x) .. strip(u.x - 1)
//   pick_shift    once: the smallest s whose total is at most 2 E (E ceiling edges; s = 47 has one strip and total E), so
//                 the entries fit in 2 n_points slots whatever the input
//   entry_count / entry_fill   per slot: its incidences under that s (exclusive scan: where they go), then its entries:
//                 key ((uint64) (uint32) face << 32) | strip, value the point slot of u  (radix sort of the pairs)
//   above_scan    per hole, by a lane group: the run of key (face, strip(p.x)) by binary search, the exact candidate
//                 test and the exact order over it; `lower` reduces the lanes' winners
//   jump_init / jump_round   pointer jumping over above: per ring the next hole, or the shell found, or "ended without
//                 one".  Separate launches, at most kMaxRounds; a round in which no walk was on its way ends it
//   poly_key      per ring: parent[], the counts, ((uint64) shell << 32) | (r == shell ? 0 : r + 1) for a member, ~0 otherwise
//                 (radix sort of the keys: the members of a polygon become neighbours, the shell first)
//   member_mark   per sorted position: does a polygon start here, the member's area2  (exclusive scans: the polygon of
//                 every start, the int128 prefix of the areas modulo 2^128)
//   member_place / poly_emit   the two CSR arrays and the records; a polygon's area is the difference of two prefix entries
//
// COST   per hole the entries of its own (face, strip) bucket, plus the two sorts.  A face whose ceiling edges all lie in
// one strip (a shift forced up by one domain-wide edge, or many holes in one column) degrades to holes x edges of
// that face.
// Scratch per call: 72 bytes per point slot (the ring of the slot and its mark 8, incidence counts and offsets 16, two entry
// slots with their sorted form 2 x 24) and 96 per ring (top 16, kind 4, two jump states 16, member keys and their sorted form
// 16, polygon starts 12, areas and their scan 32), plus the sorts' and scans' temporary storage; allocated per call and freed.
#pragma once
#include <stdint.h>

#include "rj_rings.h"

namespace rj {
namespace polygons {

using rings::Ring;
using rings::U128;

constexpr uint32_t kNone = 0xFFFFFFFFu;  // RJ_POLY_NONE
constexpr uint64_t kNoKey = ~0ull;       // (no entry has it: a strip is below 2^31; no member: a shell is at most 2^32 - 3)
constexpr int kMaxRounds = 33;           // jumping steps: 2^32 rings at most
constexpr int kMinShift = 16, kMaxShift = 47, kShifts = kMaxShift - kMinShift + 1;
constexpr int64_t kHalfRange = (int64_t) 1 << 46;
constexpr uint32_t kKindNone = 0, kKindShell = 1, kKindHole = 2;
constexpr uint32_t kWalking = 0, kFound = 1, kEnded = 2;

struct alignas(16) Top {
  int64_t x, y;
};
struct Edge {  // the directed ring edge u -> v
  int64_t ux, uy, vx, vy;
};
struct Jump {  // the walk along above from a ring: kWalking: `to` is the next hole (or shell); kFound: `to` is the shell; kEnded
  uint32_t to, state;
};
struct Polygon {  // rj_polygon (32 bytes)
  int32_t face;
  uint32_t shell, n_holes, _pad;
  uint64_t area2_lo;
  int64_t area2_hi;
};
struct Counts {  // rj_polygons_counts
  uint64_t n_polygons, n_members, n_holes, n_orphans, n_face0;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t act[kMaxRounds];  // jumping: walks still on their way after round r
  uint32_t jump_done;        // the first round that was not needed: the final state is in buffer jump_done & 1
  uint32_t bad;              // the input check's status (kBad*); not 0: the input is not read further
  uint32_t unfinished;       // the round budget ran out (cannot happen)
  uint32_t shift;            // the strip width chosen: a strip is 2^shift units wide
  uint32_t _pad;
  uint64_t n_edges;          // E: the ceiling edges
  uint64_t n_entries;        // their (edge, strip) incidences under `shift`: at most 2 E
  uint64_t incid[kShifts];   // ... under every shift
  Counts counts;
};
// the caller's arrays and their capacities (parent: null or n_rings entries)
struct Out {
  uint32_t* parent;
  Polygon* polygons;
  uint32_t *poly_first, *poly_ring;
  uint64_t polygon_cap, member_cap;
};

RJ_RHD uint64_t ring_key(const Ring& g) { return ((uint64_t) (uint32_t) g.face << 32) | g.leader; }
RJ_RHD U128 area2_of(const Ring& g) { return U128{g.area2_lo, (uint64_t) g.area2_hi}; }

// ---- 0. the input check ------------------------------------------------------------------------------
// The largest code met is the input's status, 0: fine.  c in [0, n_rings]; r in [0, n_rings); every coordinate.
constexpr uint32_t kBadStart = 5, kBadEnd = 4, kBadRow = 3, kBadOrder = 2, kBadCoordinate = 1;
RJ_RHD uint32_t check_row(uint64_t c, const uint32_t* row, uint64_t nr, uint64_t np) {
  const uint32_t b = row[c];
  if (c == 0 && b != 0) return kBadStart;
  if (c == nr) return (uint64_t) b != np ? kBadEnd : 0;
  return row[c + 1] < b ? kBadRow : 0;
}
RJ_RHD uint32_t check_order(uint64_t r, const Ring* rings, uint64_t nr) {
  return r + 1 < nr && ring_key(rings[r]) >= ring_key(rings[r + 1]) ? kBadOrder : 0;
}
RJ_RHD uint32_t check_coordinate(int64_t v) { return v < -kHalfRange || v >= kHalfRange ? kBadCoordinate : 0; }

// ---- 1. tops and kinds ---------------------------------------------------------------------------------
RJ_RHD bool top_before(int64_t ax, int64_t ay, int64_t bx, int64_t by) { return ay != by ? ay < by : ax < bx; }
// lane `lane` of `width`: the largest (y, x) among points lane, lane + width, ... of ring r; -> false: none of them
RJ_RHD bool ring_top(uint32_t r, uint32_t lane, uint32_t width, const uint32_t* row, const int64_t* xy, Top* top) {
  const uint64_t b = row[r], e = row[(uint64_t) r + 1];
  bool has = false;
  Top t{0, 0};
  for (uint64_t i = b + lane; i < e; i += width) {
    const int64_t x = xy[2 * i], y = xy[2 * i + 1];
    if (!has || top_before(t.x, t.y, x, y)) t = Top{x, y};
    has = true;
  }
  *top = t;
  return has;
}
RJ_RHD uint32_t ring_kind(const Ring& g) {
  if (g.face == 0) return kKindNone;
  return g.area2_hi > 0 || (g.area2_hi == 0 && g.area2_lo != 0) ? kKindShell : kKindHole;
}

// ---- 2. the ring of every point slot ---------------------------------------------------------------------
// mark[] zeroed before; the inclusive max-scan of mark[] is ring_at[] (a ring without points marks nothing)
RJ_RHD void ring_mark(uint32_t r, const uint32_t* row, uint32_t* mark) {
  if (row[(uint64_t) r + 1] > row[r]) mark[row[r]] = r;
}
RJ_RHD Edge edge_at(uint64_t i, uint32_t r, const uint32_t* row, const int64_t* xy) {
  const uint64_t j = i + 1 == row[(uint64_t) r + 1] ? row[r] : i + 1;
  return Edge{xy[2 * i], xy[2 * i + 1], xy[2 * j], xy[2 * j + 1]};
}
RJ_RHD bool is_ceiling(const Ring& g, const Edge& e) { return g.face != 0 && e.vx < e.ux; }

// ---- 3. the strip width ------------------------------------------------------------------------------------
RJ_RHD uint64_t strip_of(int64_t x, int s) { return (uint64_t) (x + kHalfRange) >> s; }
RJ_RHD uint64_t strips_of(const Edge& e, int s) { return strip_of(e.ux - 1, s) - strip_of(e.vx, s) + 1; }
// per point slot: -> is its edge a ceiling edge; then acc[k] += its incidences under shift kMinShift + k
RJ_RHD bool edge_strips(uint64_t i, const uint32_t* ring_at, const Ring* rings, const uint32_t* row, const int64_t* xy, uint64_t* acc) {
  const uint32_t r = ring_at[i];
  const Edge e = edge_at(i, r, row, xy);
  if (!is_ceiling(rings[r], e)) return false;
  for (int k = 0; k < kShifts; k++) acc[k] += strips_of(e, kMinShift + k);
  return true;
}
// once, behind the totals
RJ_RHD void pick_shift(Meta* meta) {
  for (int k = 0; k < kShifts; k++)
    if (meta->incid[k] <= 2 * meta->n_edges || k == kShifts - 1) {
      meta->shift = (uint32_t) (kMinShift + k);
      meta->n_entries = meta->incid[k];
      return;
    }
}

// ---- 4. entries ----------------------------------------------------------------------------------------------
RJ_RHD uint64_t entry_count(uint64_t i, const uint32_t* ring_at, const Ring* rings, const uint32_t* row, const int64_t* xy, int shift) {
  const uint32_t r = ring_at[i];
  const Edge e = edge_at(i, r, row, xy);
  return is_ceiling(rings[r], e) ? strips_of(e, shift) : 0;
}
// off = the exclusive scan of the counts; nothing beyond cap (cannot happen: n_entries <= 2 E <= cap)
RJ_RHD void entry_fill(uint64_t i, const uint32_t* ring_at, const Ring* rings, const uint32_t* row, const int64_t* xy, int shift,
                       const uint64_t* off, uint64_t* keys, uint32_t* vals, uint64_t cap) {
  const uint32_t r = ring_at[i];
  const Edge e = edge_at(i, r, row, xy);
  const Ring g = rings[r];
  if (!is_ceiling(g, e)) return;
  const uint64_t first = strip_of(e.vx, shift), n = strips_of(e, shift), at = off[i];
  for (uint64_t k = 0; k < n && at + k < cap; k++) {
    keys[at + k] = ((uint64_t) (uint32_t) g.face << 32) | (first + k);
    vals[at + k] = (uint32_t) i;
  }
}

// ---- 5. the ring above a hole -----------------------------------------------------------------------------------
RJ_RHD bool candidate(const Edge& e, const Top& p) {
  if (!(e.vx <= p.x && p.x < e.ux)) return false;
  return (__int128) (e.uy - e.vy) * (p.x - e.vx) > (__int128) (p.y - e.vy) * (e.ux - e.vx);
}
// floor(n / d) and the remainder in [0, d): |n| < 2^94, 0 < d < 2^47, |n / d| < 2^47.  The quotient of the magnitudes is
// estimated in double (within 1 of the true one) and fixed up exactly in integers: no 128-bit division on the device.
RJ_RHD int64_t floor_div(__int128 n, int64_t d, uint64_t* rem) {
  const unsigned __int128 m = n < 0 ? (unsigned __int128) 0 - (unsigned __int128) n : (unsigned __int128) n;
  const double dm = (double) (uint64_t) (m >> 64) * 18446744073709551616.0 + (double) (uint64_t) m;
  uint64_t q = (uint64_t) (dm / (double) d);
  unsigned __int128 p = (unsigned __int128) q * (uint64_t) d;
  while (p > m) {
    q--;
    p -= (uint64_t) d;
  }
  unsigned __int128 r = m - p;
  while (r >= (uint64_t) d) {
    q++;
    r -= (uint64_t) d;
  }
  if (n >= 0 || r == 0) {
    *rem = (uint64_t) r;
    return n >= 0 ? (int64_t) q : -(int64_t) q;
  }
  *rem = (uint64_t) d - (uint64_t) r;
  return -(int64_t) q - 1;
}
// both candidates of the ray at px: does a (u at slot sa) win over b (u at slot sb)
RJ_RHD bool lower(const Edge& a, uint32_t sa, const Edge& b, uint32_t sb, int64_t px) {
  const int64_t da = a.ux - a.vx, db = b.ux - b.vx;
  uint64_t ra, rb;
  const int64_t ia = a.vy + floor_div((__int128) (a.uy - a.vy) * (px - a.vx), da, &ra);
  const int64_t ib = b.vy + floor_div((__int128) (b.uy - b.vy) * (px - b.vx), db, &rb);
  if (ia != ib) return ia < ib;
  const unsigned __int128 fa = (unsigned __int128) ra * (uint64_t) db, fb = (unsigned __int128) rb * (uint64_t) da;
  if (fa != fb) return fa < fb;
  const __int128 ka = (__int128) (a.uy - a.vy) * db, kb = (__int128) (b.uy - b.vy) * da;
  if (ka != kb) return ka < kb;
  return sa < sb;
}
// the winner of two winners (point slots of u; kNone: no candidate)
RJ_RHD uint32_t lower_slot(uint32_t sa, uint32_t sb, int64_t px, const uint32_t* ring_at, const uint32_t* row, const int64_t* xy) {
  if (sa == kNone || sb == kNone) return sa == kNone ? sb : sa;
  return lower(edge_at(sa, ring_at[sa], row, xy), sa, edge_at(sb, ring_at[sb], row, xy), sb, px) ? sa : sb;
}
// the first position in keys[0, n) whose key is not below `key`
RJ_RHD uint64_t lower_bound(const uint64_t* keys, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// lane `lane` of `width`, hole r with top p: the winner among entries lane, lane + width, ... of the run of its key
RJ_RHD uint32_t above_scan(uint32_t r, uint32_t lane, uint32_t width, const Top& p, const Ring* rings, const uint32_t* ring_at,
                           const uint32_t* row, const int64_t* xy, const uint64_t* keys, const uint32_t* vals, uint64_t n_entries, int shift) {
  const uint64_t key = ((uint64_t) (uint32_t) rings[r].face << 32) | strip_of(p.x, shift);
  uint32_t best = kNone;
  Edge be{0, 0, 0, 0};
  for (uint64_t k = lower_bound(keys, n_entries, key) + lane; k < n_entries && keys[k] == key; k += width) {
    const uint32_t s = vals[k];
    const Edge e = edge_at(s, ring_at[s], row, xy);
    if (!candidate(e, p)) continue;
    if (best == kNone || lower(e, s, be, best, p.x)) {
      best = s;
      be = e;
    }
  }
  return best;
}

// ---- 6. parents: pointer jumping over above ------------------------------------------------------------------------
// winner: the point slot that won for hole r (kNone: nothing above it); ignored for the other kinds
RJ_RHD void jump_init(uint32_t r, uint32_t kind, uint32_t winner, const uint32_t* ring_at, Jump* a, Jump* b) {
  Jump j{kNone, kEnded};
  if (kind == kKindShell) j = Jump{r, kFound};
  if (kind == kKindHole && winner != kNone) j = Jump{ring_at[winner], kWalking};
  a[r] = b[r] = j;
}
// one round, in -> out; true while the walk from i has not ended.  A walk that ended in the round before still has its
// old state in `out` (written two rounds ago): copied once, then both hold it.
RJ_RHD bool jump_round(uint32_t i, const Jump* in, Jump* out) {
  const Jump a = in[i];
  if (a.state != kWalking) {
    if (out[i].state == kWalking) out[i] = a;
    return false;
  }
  const Jump b = in[a.to];
  out[i] = b;
  return b.state == kWalking;
}
RJ_RHD bool round_needed(const uint32_t* count, int r) { return r == 0 || count[r - 1] != 0; }

// ---- 7. polygons ---------------------------------------------------------------------------------------------------
// J = the final states.  -> the ring's key among the members; parent[] where the caller has one; what: 0, or the counter
// the ring adds to (1: a hole with a parent, 2: an orphan, 3: a ring of face 0)
RJ_RHD uint64_t poly_key(uint32_t r, const uint32_t* kind, const Jump* J, uint32_t* parent, int* what) {
  const uint32_t k = kind[r];
  const Jump j = J[r];
  const uint32_t shell = j.state == kFound ? j.to : kNone;
  if (parent) parent[r] = shell;
  *what = k == kKindNone ? 3 : (k == kKindHole ? (shell == kNone ? 2 : 1) : 0);
  if (shell == kNone) return kNoKey;
  return ((uint64_t) shell << 32) | (r == shell ? 0u : r + 1);
}
RJ_RHD uint32_t member_ring(uint64_t key) { return (uint32_t) key ? (uint32_t) key - 1 : (uint32_t) (key >> 32); }
// j in [0, nr]: sorted key j is member j's (the keys of no member sort behind the members); entry nr closes the scans
RJ_RHD void member_mark(uint64_t j, uint64_t nr, const uint64_t* skeys, const Ring* rings, uint32_t* start, U128* area_at, Meta* meta) {
  const uint64_t key = j < nr ? skeys[j] : kNoKey;
  if (key == kNoKey) {
    start[j] = 0;
    area_at[j] = U128{0, 0};
    return;
  }
  start[j] = (uint32_t) key == 0 ? 1 : 0;
  area_at[j] = area2_of(rings[member_ring(key)]);
  if (j + 1 == nr || skeys[j + 1] == kNoKey) meta->counts.n_members = j + 1;
}
// j in [0, nr]; pid = the exclusive scan of start[]: the polygon that starts at j, and at nr the number of polygons.
// first[] (nr + 1 entries): where every polygon starts among the members, closed by n_members
RJ_RHD void member_place(uint64_t j, uint64_t nr, const uint64_t* skeys, const uint32_t* start, const uint32_t* pid, uint32_t* first,
                         const Out& o, Meta* meta) {
  if (j == nr) {
    first[pid[j]] = (uint32_t) meta->counts.n_members;
    meta->counts.n_polygons = pid[j];
    return;
  }
  if (skeys[j] == kNoKey) return;
  if (start[j]) first[pid[j]] = (uint32_t) j;
  if (j < o.member_cap) o.poly_ring[j] = member_ring(skeys[j]);
}
// p in [0, n_polygons]; xbase = the exclusive scan of area_at[] (modulo 2^128; a polygon's own sum fits)
RJ_RHD void poly_emit(uint64_t p, const uint64_t* skeys, const uint32_t* first, const U128* xbase, const Ring* rings, const Out& o,
                      const Meta* meta) {
  const uint64_t n_polygons = meta->counts.n_polygons;
  if (p == n_polygons) {
    if (n_polygons <= o.polygon_cap && o.poly_first) o.poly_first[p] = first[p];
    return;
  }
  if (p >= o.polygon_cap) return;
  const uint32_t b = first[p], e = first[p + 1];
  const U128 a2 = rings::sub(xbase[e], xbase[b]);
  Polygon g;
  g.shell = (uint32_t) (skeys[b] >> 32);
  g.face = rings[g.shell].face;
  g.n_holes = e - b - 1;
  g._pad = 0;
  g.area2_lo = a2.lo;
  g.area2_hi = (int64_t) a2.hi;
  o.polygons[p] = g;
  o.poly_first[p] = b;
}

}  // namespace polygons

#if defined(__HIPCC__)
// rj_rings_polygons behind its argument checks, on stream st: *result = the device's Meta (counts, the input check's
// status, the chosen shift, the round budget).  Allocates and frees its scratch; synchronises the stream once, at the end.
hipError_t rings_polygons_device(hipStream_t st, const rings::Ring* rings, uint64_t n_rings, const uint32_t* ring_row, const int64_t* ring_xy,
                                 uint64_t n_points, const polygons::Out& out, polygons::Meta* result);
#endif

}  // namespace rj
