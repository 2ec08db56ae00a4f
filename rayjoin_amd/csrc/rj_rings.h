// rj_rings.h -- the face rings of a chain map (rj_map_rings, include/rayjoin_amd.h; kernels in rj_rings.hip): the
// closed boundaries that the chains of a map form, every ring with its face, its half-chains in walk order, its points
// and twice its signed area.  Integers only.
//
// INPUT   a chain map as rj_upload_map_dev takes it: xy[2 np], row_index[nc + 1], left[nc], right[nc] (int32); left is
//         the face on the left of a chain walked from its first point to its last, y up.  nc < 2^31, np < 2^32, and
//         2 (np - nc) < 2^32 (every ring point has a 32-bit slot).
// HALF-CHAINS   h = 2 c is chain c walked forward, its face left[c]; h = 2 c + 1 is chain c walked backward, its face
//         right[c]; h ^ 1 is the twin of h.  A chain whose points are all equal is SKIPPED: its two half-chains belong
//         to no ring, it is counted in n_skipped.
// INCIDENCES   incidence h is the start vertex of half-chain h (the chain's first point for 2 c, its last for 2 c + 1);
//         its direction (dx, dy) points to the first point of the chain, walking inward from that end, that differs
//         from the end point (zero-length edges are stepped over).
// ORDER AT A JUNCTION   a junction is the set of incidences on one integer point, ordered counter-clockwise from the
//         positive x axis, exactly: half-plane 0 (dy > 0, or dy == 0 and dx > 0) before half-plane 1; inside a
//         half-plane a before b when cross(a, b) = a.dx b.dy - a.dy b.dx > 0 (differences below 2^47, the cross product
//         below 2^95: int128); equal directions by ascending h (only where chains overlap: the result is still fully
//         determined, but its rings may mix faces).  Any degree: ONE sort of all incidences by (y, x, half-plane, cross,
//         h) orders every junction, there is no per-junction loop and no degree cap.
// SUCCESSOR   half-chain h arrives at the junction of incidence h ^ 1.  With that junction's order o_0 .. o_{d-1} and
//         h ^ 1 = o_k: next(h) = o_{(k - 1) mod d}, the clockwise neighbour of the twin, which keeps the face on the
//         left.  At a dead end (d = 1) next(h) = h ^ 1.  next is a permutation of the half-chains that are not skipped;
//         its cycles are the RINGS.
// A RING   leader: its smallest h.  face: the leader's face.  RJ_RING_MIXED in flags when some half-chain of the ring
//         has another face.  Its half-chains in walk order from the leader.  Its points: every half-chain's points in
//         its direction without its last point (point count = edge count, the first point is not repeated).  area2: the
//         sum of cross(a, b) over consecutive point pairs including the closing pair, a two's-complement int128 as in
//         rj_overlay_face (bounded by 2^125): positive = counter-clockwise = the outer boundary of its face, negative = a
//         hole of its face or a boundary of face 0.
// RING ORDER   ascending by ((uint64) (uint32) face << 32) | leader: the rings of a face are contiguous.
//
// Every step is one function per element that rj_rings.hip runs as a grid-stride kernel and
// tests/hosttwin/rings_twin.cc runs as a plain loop (a test-only twin, never a fallback):
//
//   check_row / check_coordinate   the map check, its status word stays on the device
//   incidence     per h: the point and the direction of incidence h (all zero: skipped)
//   (one merge sort of the h's by inc_before: the incidences of a junction become neighbours, counter-clockwise)
//   junction_head per sorted position: the inverse permutation, and its own position where a junction starts
//   (inclusive max-scan: every position learns where its junction starts)
//   junction_last per sorted position: the last position of a junction, left at the junction's start
//   next_of       per h: next(h); the first links of the pointer doubling
//   cyc_round     pointer doubling for the smallest h of every cycle.  A round in which no minimum changed ends it: then
//                 mn[i] <= mn[i + 2^r] all the way round the cycle, so all windows of one orbit of that step hold the
//                 same minimum, and these windows cover the cycle.  Separate launches, at most kMaxRounds.
//   rank_init / rank_round   the cycle opened in front of its leader and ranked by pointer jumping: half-chains and
//                 points from h to the end of its ring, so position = the leader's totals - h's
//   ring_key      per h: ((uint32) face << 32) | h for a leader (kNoKey otherwise, and for face 0 under RJ_RINGS_SKIP_FACE0)
//   (radix sort of the keys: ring r's leader; ring_slot: its totals; exclusive scan: the two CSRs)
//   half_points / half_store   per h, by a lane group: its points to their slots, coalesced, reversed for odd h; the
//                 int128 cross sum of its edges (the closing pair of a half-chain is its last edge) at its slot
//   (exclusive scan of the cross sums in slot order, modulo 2^128: a ring's area2 is the difference of two entries)
//   ring_emit     per ring: the record and its two CSR entries, the counts
//
// Scratch per call: 352 bytes per chain (per half-chain: 32 incidence, 20 sort and junctions, 4 next, 16 links, 32 ranking,
// 4 ring index, 4 mixed flag, 32 totals and their scan, 32 cross sums and their scan; the ring keys and their sorted form
// live in the dead sort and junction arrays) plus the sorts' and scans' temporary
// storage; allocated per call and freed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "rj_pipeline.h"  // (StageMs: what the reports of the map pipelines, in the headers that include this one, derive from)
#define RJ_RHD __host__ __device__ __forceinline__
#else
#define RJ_RHD inline
#endif

namespace rj {
namespace rings {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kNoKey = ~0ull;  // (no ring has it: h <= 2^32 - 2)
constexpr int kMaxRounds = 33;      // doubling steps: 2^32 half-chains at most
constexpr uint32_t kSkipFace0 = 1u, kNoPoints = 2u, kMixed = 1u;  // RJ_RINGS_SKIP_FACE0, RJ_RINGS_NO_POINTS, RJ_RING_MIXED

struct alignas(16) Inc {  // incidence h: its point, its direction into the chain (0, 0: the chain is skipped)
  int64_t x, y, dx, dy;
};
struct Link {  // pointer doubling round a cycle: where the window ends, the smallest h in it
  uint32_t succ, mn;
};
struct alignas(16) Node {  // the walk from h to the end of its opened ring
  uint32_t succ;           // the half-chain behind what is summed here (kNone: the walk has ended)
  uint32_t cnt, pts;       // half-chains and points (= edges) summed
  uint32_t _pad;
};
struct Slots {
  uint64_t halves, points;
};
struct U128 {  // modulo 2^128
  uint64_t lo, hi;
};
struct Ring {  // rj_ring (32 bytes)
  int32_t face;
  uint32_t flags, leader, _pad;
  uint64_t area2_lo;
  int64_t area2_hi;
};
struct Counts {  // rj_rings_counts
  uint64_t n_rings, n_halves, n_points, n_mixed, n_skipped;
};
// what the stages leave for each other and for the host (device memory, zeroed before the first stage)
struct Meta {
  uint32_t changed[kMaxRounds];  // doubling: minima that changed in round r
  uint32_t cyc_done;             // the first round that was not needed: the final links are in buffer cyc_done & 1
  uint32_t act[kMaxRounds];      // ranking: walks still on their way after round r
  uint32_t rank_done;
  uint32_t bad_map;  // the map check's status (kBad*); not 0: the map is not read and every incidence is skipped
  uint32_t unfinished;  // a round budget ran out (cannot happen)
  Counts counts;
};
// the caller's arrays and their capacities
struct Out {
  Ring* rings;
  uint32_t *ring_first, *ring_half, *ring_row;  // (ring_row, ring_xy: null under RJ_RINGS_NO_POINTS)
  int64_t* ring_xy;
  uint64_t ring_cap, half_cap, point_cap;
};

RJ_RHD U128 add(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
  return r;
}
RJ_RHD U128 sub(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo - b.lo;
  r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
  return r;
}
RJ_RHD U128 limbs(__int128 v) { return U128{(uint64_t) v, (uint64_t) (v >> 64)}; }
RJ_RHD __int128 cross(int64_t ax, int64_t ay, int64_t bx, int64_t by) { return (__int128) ax * by - (__int128) ay * bx; }

// (left null: a map without labels, every face 0 -- rj_faces.h runs the ring stages that way)
RJ_RHD int32_t face_of(uint32_t h, const int32_t* left, const int32_t* right) { return !left ? 0 : ((h & 1) ? right[h >> 1] : left[h >> 1]); }
RJ_RHD uint32_t edges_of(uint32_t h, const uint32_t* row) { return row[(h >> 1) + 1] - row[h >> 1] - 1; }
RJ_RHD bool skipped(const Inc& a) { return a.dx == 0 && a.dy == 0; }
RJ_RHD bool same_point(const Inc& a, const Inc& b) { return a.x == b.x && a.y == b.y; }

// ---- 0. the map check ------------------------------------------------------------------------------
// rj_upload_map_dev's checks with one difference: a chain of ONE point is allowed (an output map has them without
// RJ_OVM_DROP_DEGENERATE; it is skipped like every chain whose points are all equal).  The largest code met is the
// map's status, 0: the map is fine.  c in [0, nc]; every coordinate.
constexpr uint32_t kBadStart = 4, kBadEnd = 3, kBadEmptyChain = 2, kBadCoordinate = 1;
RJ_RHD uint32_t check_row(uint64_t c, const uint32_t* row, uint64_t nc, uint64_t np) {
  const uint32_t b = row[c];
  if (c == 0 && b != 0) return kBadStart;
  if (c == nc) return (uint64_t) b != np ? kBadEnd : 0;
  return row[c + 1] <= b ? kBadEmptyChain : 0;
}
RJ_RHD uint32_t check_coordinate(int64_t v) { return v < -((int64_t) 1 << 46) || v >= ((int64_t) 1 << 46) ? kBadCoordinate : 0; }

// ---- 1. incidences ---------------------------------------------------------------------------------
// -> true when chain h >> 1 is skipped (the caller counts the even h's).  bad_map: the map failed its check, nothing of
// it is read and every incidence is skipped.
RJ_RHD bool incidence(uint32_t h, const int64_t* xy, const uint32_t* row, bool bad_map, Inc* inc) {
  Inc r{0, 0, 0, 0};
  if (!bad_map) {
    const uint64_t b = row[h >> 1], e = row[(h >> 1) + 1];  // the chain's points: [b, e)
    const bool back = h & 1;
    const uint64_t p = back ? e - 1 : b;
    r.x = xy[2 * p];
    r.y = xy[2 * p + 1];
    for (uint64_t k = 1; k < e - b; k++) {
      const uint64_t q = back ? p - k : p + k;
      const int64_t dx = xy[2 * q] - r.x, dy = xy[2 * q + 1] - r.y;
      if (dx != 0 || dy != 0) {
        r.dx = dx;
        r.dy = dy;
        break;
      }
    }
  }
  inc[h] = r;
  return skipped(r);
}

// the order of the one sort: by point (y, then x), counter-clockwise from the positive x axis, then h; skipped
// incidences behind everything else.  A strict weak order: inside a half-plane the directions span less than 180 degrees.
RJ_RHD int half_plane(const Inc& a) { return (a.dy > 0 || (a.dy == 0 && a.dx > 0)) ? 0 : 1; }
RJ_RHD bool inc_before(uint32_t ha, uint32_t hb, const Inc* inc) {
  const Inc a = inc[ha], b = inc[hb];
  const bool sa = skipped(a), sb = skipped(b);
  if (sa != sb) return sb;
  if (sa) return ha < hb;
  if (a.y != b.y) return a.y < b.y;
  if (a.x != b.x) return a.x < b.x;
  const int pa = half_plane(a), pb = half_plane(b);
  if (pa != pb) return pa < pb;
  const __int128 cr = cross(a.dx, a.dy, b.dx, b.dy);
  if (cr != 0) return cr > 0;
  return ha < hb;
}

// ---- 2. junctions ----------------------------------------------------------------------------------
// sorted position j holds incidence sv[j].  pos = the inverse; head[j] = j where a junction starts, else 0: the
// inclusive max-scan of head[] is, per position, where its junction starts (a skipped incidence is a junction of its own)
RJ_RHD void junction_head(uint32_t j, const uint32_t* sv, const Inc* inc, uint32_t* pos, uint32_t* head) {
  const uint32_t h = sv[j];
  pos[h] = j;
  const Inc a = inc[h];
  const bool first = j == 0 || skipped(a) || !same_point(a, inc[sv[j - 1]]);  // (skipped ones sort last: j - 1 is none of them)
  head[j] = first ? j : 0;
}
// begin = the scanned head[]; the last position of every junction goes to last_of[its first position]
RJ_RHD void junction_last(uint32_t j, uint32_t ni, const uint32_t* sv, const Inc* inc, const uint32_t* begin, uint32_t* last_of) {
  const Inc a = inc[sv[j]];
  bool last = j + 1 == ni || skipped(a);
  if (!last) {
    const Inc b = inc[sv[j + 1]];
    last = skipped(b) || !same_point(a, b);
  }
  if (last) last_of[begin[j]] = j;
}

// ---- 3. next, and the smallest h of every cycle ----------------------------------------------------------------
RJ_RHD void next_of(uint32_t h, const uint32_t* sv, const Inc* inc, const uint32_t* pos, const uint32_t* begin, const uint32_t* last_of,
                    uint32_t* next, Link* a, Link* b) {
  uint32_t n = h;  // (a skipped half-chain: a cycle of its own that nothing reads)
  if (!skipped(inc[h])) {
    const uint32_t k = pos[h ^ 1], first = begin[k];
    n = sv[k > first ? k - 1 : last_of[first]];
  }
  next[h] = n;
  a[h] = b[h] = Link{n, h};
}
// one round of pointer doubling, in -> out; true when the minimum of i's window changed
RJ_RHD bool cyc_round(uint32_t i, const Link* in, Link* out) {
  const Link a = in[i], b = in[a.succ];
  out[i] = Link{b.succ, a.mn < b.mn ? a.mn : b.mn};
  return b.mn < a.mn;
}
RJ_RHD bool round_needed(const uint32_t* count, int r) { return r == 0 || count[r - 1] != 0; }

// ---- 4. the ring opened in front of its leader, ranked ----------------------------------------------------------
// F = the final links
RJ_RHD void rank_init(uint32_t h, const Link* F, const uint32_t* next, const Inc* inc, const uint32_t* row, Node* a, Node* b) {
  Node n{kNone, 0, 0, 0};
  if (!skipped(inc[h])) {
    n.succ = next[h] == F[h].mn ? kNone : next[h];
    n.cnt = 1;
    n.pts = edges_of(h, row);
  }
  a[h] = b[h] = n;
}
// one round of pointer jumping, in -> out; true while the walk from i has not reached its end.  A walk that ended in
// the round before still has its old state in `out` (written two rounds ago): copied once, then both hold it.
RJ_RHD bool rank_round(uint32_t i, const Node* in, Node* out) {
  Node a = in[i];
  if (a.succ == kNone) {
    if (out[i].succ != kNone) out[i] = a;
    return false;
  }
  const Node b = in[a.succ];
  a.cnt += b.cnt;
  a.pts += b.pts;
  a.succ = b.succ;
  out[i] = a;
  return a.succ != kNone;
}

// ---- 5. the rings in their order -------------------------------------------------------------------------------
RJ_RHD uint64_t ring_key(uint32_t h, const Link* F, const Inc* inc, const int32_t* left, const int32_t* right, uint32_t flags) {
  if (skipped(inc[h]) || F[h].mn != h) return kNoKey;
  const int32_t face = face_of(h, left, right);
  if ((flags & kSkipFace0) && face == 0) return kNoKey;
  return ((uint64_t) (uint32_t) face << 32) | h;
}
// r in [0, ni]: sorted key r is ring r's (the keys of no ring sort behind the rings); total[ni] = 0 closes the scan
RJ_RHD void ring_slot(uint32_t r, uint32_t ni, const uint64_t* skeys, const Node* N, uint32_t* ring_of, Slots* total, Meta* meta) {
  const uint64_t key = r < ni ? skeys[r] : kNoKey;
  if (key == kNoKey) {
    total[r] = Slots{0, 0};
    return;
  }
  const uint32_t leader = (uint32_t) key;
  ring_of[leader] = r;
  total[r] = Slots{N[leader].cnt, N[leader].pts};
  if (r + 1 == ni || skeys[r + 1] == kNoKey) meta->counts.n_rings = (uint64_t) r + 1;
}

// ---- 6. half-chains and points to their slots -------------------------------------------------------------------
// base = the exclusive scan of total[].  -> the ring of h (kNone: h is in no ring that is kept), its slot among the
// half-chains and its first point slot
RJ_RHD uint32_t half_slots(uint32_t h, const Link* F, const Inc* inc, const Node* N, const uint32_t* ring_of, const Slots* base,
                           uint64_t* slot, uint64_t* pslot) {
  if (skipped(inc[h])) return kNone;
  const uint32_t leader = F[h].mn, r = ring_of[leader];
  if (r == kNone) return kNone;
  *slot = base[r].halves + (N[leader].cnt - N[h].cnt);
  *pslot = base[r].points + (N[leader].pts - N[h].pts);
  return r;
}
// lane `lane` of `width`: edges lane, lane + width, ... of half-chain h in its direction -- the first point of each to
// its slot (nothing beyond point_cap; ring_xy null: no points), -> the sum of their cross products
RJ_RHD U128 half_points(uint32_t h, uint32_t lane, uint32_t width, const int64_t* xy, const uint32_t* row, uint64_t pslot, int64_t* ring_xy,
                        uint64_t point_cap) {
  const uint64_t b = row[h >> 1], e = row[(h >> 1) + 1];
  const bool back = h & 1;
  __int128 sum = 0;
  for (uint64_t k = lane; k + 1 < e - b; k += width) {
    const uint64_t p = back ? e - 1 - k : b + k, q = back ? p - 1 : p + 1;
    const int64_t px = xy[2 * p], py = xy[2 * p + 1];
    sum += cross(px, py, xy[2 * q], xy[2 * q + 1]);
    if (ring_xy && pslot + k < point_cap) {
      ring_xy[2 * (pslot + k)] = px;
      ring_xy[2 * (pslot + k) + 1] = py;
    }
  }
  return limbs(sum);
}
// once per half-chain, with the sum of all its lanes: cross[] (zeroed before) and mixed[] (zeroed before) are scratch
RJ_RHD void half_store(uint32_t h, uint32_t r, uint64_t slot, uint32_t ni, U128 sum, const uint64_t* skeys, const int32_t* left,
                       const int32_t* right, U128* cross_at, uint32_t* mixed, uint32_t* ring_half, uint64_t half_cap) {
  if (slot >= ni) return;  // (cannot happen: the slots of the half-chains are a permutation of [0, n_halves))
  cross_at[slot] = sum;
  if (slot < half_cap) ring_half[slot] = h;
  if (face_of(h, left, right) != (int32_t) (uint32_t) (skeys[r] >> 32)) mixed[r] = 1;  // (every writer stores the same word)
}

// ---- 7. the ring records --------------------------------------------------------------------------------------
// r in [0, n_rings]; xbase = the exclusive scan of cross_at[] over ni + 1 entries (modulo 2^128; a ring's own sum fits).
// -> true for a mixed ring (the caller counts them); r == n_rings: the CSRs' last entries and the totals
RJ_RHD bool ring_emit(uint32_t r, const uint64_t* skeys, const Slots* base, const U128* xbase, const uint32_t* mixed, const Out& o, Meta* meta) {
  const uint64_t n_rings = meta->counts.n_rings;
  const Slots at = base[r];
  if (r == n_rings) {
    meta->counts.n_halves = at.halves;
    meta->counts.n_points = at.points;
    if (n_rings <= o.ring_cap) {
      if (o.ring_first) o.ring_first[r] = (uint32_t) at.halves;
      if (o.ring_row) o.ring_row[r] = (uint32_t) at.points;
    }
    return false;
  }
  const bool mix = mixed[r] != 0;
  if (r < o.ring_cap) {
    const U128 a2 = sub(xbase[base[r + 1].halves], xbase[at.halves]);
    Ring g;
    g.face = (int32_t) (uint32_t) (skeys[r] >> 32);
    g.flags = mix ? kMixed : 0;
    g.leader = (uint32_t) skeys[r];
    g._pad = 0;
    g.area2_lo = a2.lo;
    g.area2_hi = (int64_t) a2.hi;
    o.rings[r] = g;
    o.ring_first[r] = (uint32_t) at.halves;
    if (o.ring_row) o.ring_row[r] = (uint32_t) at.points;
  }
  return mix;
}

}  // namespace rings

#if defined(__HIPCC__)
// rj_map_rings behind its argument checks, on stream st: *result = the device's Meta (counts, the map check's status, the
// round budget).  Allocates and frees its scratch; synchronises the stream once, at the end.
hipError_t map_rings_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row_index, const int32_t* left,
                            const int32_t* right, uint64_t nc, uint32_t flags, const rings::Out& out, rings::Meta* result);
// the same stages enqueued without a wait, in the caller's scratch (rj_rings.hip has the contract): rj_map_faces runs them
// in front of its own, with left and right null
hipError_t map_rings_enqueue(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row_index, const int32_t* left,
                             const int32_t* right, uint64_t nc, uint32_t flags, const rings::Out& out, char* scratch, size_t* bytes,
                             rings::Meta** meta_dev);
#endif

}  // namespace rj
