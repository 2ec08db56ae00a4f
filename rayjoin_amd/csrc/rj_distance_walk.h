// rj_distance_walk.h -- the ONE traversal of the two distance queries over the 64-ary implicit LBVH of rj_device.h:
// k_nearest (rj_nearest.hip, a best-so-far search) and k_within (rj_within.hip, a fixed-bound search) are this walk with
// three hooks each.  The prune is rj_nearest.h's (cell_of / box_lb2 / admits / box_empty).  Device only, gfx950 only
// (wave = 64 lanes).
//
// SHAPE   One wave takes 64 consecutive points of the (possibly Morton-ordered) set, one per lane, and walks the tree
// depth-first with ONE stack in LDS.  Every lane has its own bound ub2 (rj_nearest.h: d^2 <= 2^32 ub2); what the lanes
// share is the order of the walk and every load.
//   * A node's 64 children are one coalesced load, lane = child.  A child is pushed while SOME lane admits it
//     (admits(ub2, box_lb2) of the header, per lane, the child's box broadcast): exact per lane, so a wave of scattered
//     points -- a shuffled set without the Morton order -- still opens only what one of its points needs.
//   * In front of the per-lane ballots sits the hook `near_group`, one lane-parallel test of all 64 boxes: it may only
//     shorten the loop, never dismiss a box that some lane admits, and every box it keeps is still tested per lane.
//   * Where a kept child lands inside its batch -- which sibling is popped first -- is the hook `place`.  The order is a
//     heuristic only; any order gives the same result.
//   * A popped entry carries its box.  With RETEST the lanes test it again against the bounds as they are NOW, and an entry
//     that no lane admits any more is dropped without a load; without it (a bound that never tightens) only a leaf block's
//     box is tested, for the lanes that skip its slots.
//   * A leaf block's 64 boxes are one coalesced load; slot after slot the box is broadcast and, where some lane admits it,
//     the segment of the slot is loaded (one address for the wave) and handed to the hook `slot`.  EVERY lane calls it,
//     with its own `adm`: a body may ballot.  The bound goes in by reference: a body may tighten its lane's bound inside
//     the block, slot by slot.
//   * Padding slots (inside a block under "leaf_order" 1, and behind the last block) and the nodes above nothing but
//     padding have the empty box: excluded explicitly by box_empty -- an unlimited bound admits everything, and a zero
//     segment at the origin would be a phantom edge.
//
// STACK   A pop removes one entry and pushes at most the 64 children of that node, all one level lower; a batch of
// children is consumed completely before anything below it is touched.  From the <= 64 entries of the top level the
// stack therefore holds at most 64 + 63 (top - 1) entries: 64 at the start, and 63 more for every level descended.
// That is k_pip's discipline and k_pip's bound (kPipStack, rj_device.h; simulated in tests/test_stack_bounds.py).
// Every push is still checked against the capacity and raises the query's fault word (kFaultNearestStack,
// kFaultWithinStack -> RJ_E_INTERNAL) instead of writing past the stack.
//
// The hooks are lambdas that capture the kernel's own locals.  (A policy object that owns the per-lane state -- bound,
// best candidate, point -- and is passed by reference costs k_nearest 12 VGPRs and one wave per SIMD.)
#pragma once
#include "rj_nearest.h"

namespace rj {
namespace dwalk {

using namespace nearest;

constexpr int kWaves = 4;          // waves per block
constexpr int kStack = kPipStack;  // 64 + 63 (kMaxTop - 1) and four to spare: see STACK above

struct Stack {  // per wave, LDS; 20 bytes per entry: 6400 B
  uint4 box[kStack];      // {x0, y0, x1, y1} of the node
  uint32_t code[kStack];  // level << 28 | index
};
// 64 points, one per lane
struct Group {
  bool live;                   // the lane has a point
  uint64_t ip;                 // its number in the caller's order
  int64_t px, py;
  int32_t qx, qy;              // its cell
  int32_t gx0, gy0, gx1, gy1;  // the box of the group's cells (wave-uniform)
};
struct Stats {  // the instrumented kernels: [0] .. [3] of NearestArgs::stats
  unsigned long long leaf = 0, cand = 0, nodes = 0, wave_leaf = 0;
};

__device__ __noinline__ void raise_fault(uint32_t* word) {
  // a plain store (idempotent), not an atomic: the word is pinned host memory the device writes directly
  __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the head of group g of the n points pts, taken in `order` (null: as given)
__device__ __forceinline__ Group load_group(const int64_t* pts, const uint32_t* order, uint64_t n, uint64_t g, int lane) {
  Group G;
  const uint64_t ipos = g * 64 + lane;
  G.live = ipos < n;
  G.ip = order ? (G.live ? order[ipos] : 0) : ipos;
  G.px = 0, G.py = 0;
  if (G.live) {
    G.px = pts[2 * G.ip];
    G.py = pts[2 * G.ip + 1];
  }
  G.qx = cell_of(G.px), G.qy = cell_of(G.py);
  G.gx0 = wave_min(G.live ? G.qx : kEmptyMin), G.gx1 = wave_max(G.live ? G.qx : kEmptyMax);
  G.gy0 = wave_min(G.live ? G.qy : kEmptyMin), G.gy1 = wave_max(G.live ? G.qy : kEmptyMax);
  return G;
}

// The walk of one group, see SHAPE.  ub2: this lane's bound.  The hooks:
//   near_group(box) -> bool                     this lane's box may lie near the group (always true: no such test)
//   place(keep, n, box, mine, lane) -> int      of the n kept children (mask keep; mine: this lane's is one, box: it) the
//                                               position of this lane's in the batch; the highest is popped first
//   slot(adm, seg, eid)                         a slot that some lane admits; adm: this lane does
template <bool STATS, bool RETEST, class NearGroup, class Place, class Slot>
__device__ __forceinline__ void walk_group(const DeviceBvh& T, Stack& L, const Group& G, int stack_cap, uint32_t* fault_word, int lane, uint64_t& ub2,
                                           NearGroup near_group, Place place, Slot slot, Stats& st) {
  const bool live = G.live;
  const int32_t qx = G.qx, qy = G.qy;
  int sp = 0;

  // the children of a node (lane = child; b: this lane's, `have`: it exists) onto the stack
  auto push_children = [&](int lvl, uint32_t first, const QBox& b, bool have) {
    uint64_t keep = 0;
    for (uint64_t um = __ballot(have && !box_empty(b.x0, b.x1) && near_group(b)); um; um &= um - 1) {
      const int c = __builtin_ctzll(um);
      const uint64_t lb2 = box_lb2(bcast(b.x0, c), bcast(b.y0, c), bcast(b.x1, c), bcast(b.y1, c), qx, qy);
      if (__ballot(live && admits(ub2, lb2))) keep |= 1ull << c;
    }
    const int n = __popcll(keep);
    if (sp + n > stack_cap) {
      if (lane == 0) raise_fault(fault_word);
      return;
    }
    const bool mine = (keep >> lane) & 1;
    const int at = sp + place(keep, n, b, mine, lane);
    if (mine) {
      L.box[at] = make_uint4((uint32_t) b.x0, (uint32_t) b.y0, (uint32_t) b.x1, (uint32_t) b.y1);
      L.code[at] = ((uint32_t) lvl << 28) | (first + (uint32_t) lane);
    }
    sp += n;
    wave_lds_fence();
  };

  push_children(T.top, 0u, T.lvl[T.top][lane], (uint32_t) lane < T.nlvl[T.top]);
  while (sp > 0) {
    --sp;
    const uint4 eb = L.box[sp];
    const uint32_t e = (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) L.code[sp]);
    const int lvl = (int) (e >> 28);
    const uint32_t idx = e & 0x0FFFFFFFu;
    // the lanes that admit the entry: stale?  (RETEST: the bounds have tightened since the push)
    bool want = true;
    if (RETEST || lvl <= 1) {
      const int32_t ex0 = __builtin_amdgcn_readfirstlane((int32_t) eb.x), ey0 = __builtin_amdgcn_readfirstlane((int32_t) eb.y);
      const int32_t ex1 = __builtin_amdgcn_readfirstlane((int32_t) eb.z), ey1 = __builtin_amdgcn_readfirstlane((int32_t) eb.w);
      want = live && admits(ub2, box_lb2(ex0, ey0, ex1, ey1, qx, qy));
      if (RETEST && !__ballot(want)) continue;
    }
    if (lvl > 1) {
      if (STATS) st.nodes++;
      push_children(lvl - 1, idx * 64u, T.lvl[lvl - 1][(uint64_t) idx * 64 + lane], true);
      continue;
    }
    if (STATS) st.leaf += (unsigned long long) __popcll(__ballot(want)), st.wave_leaf++;  // (per point: the lanes that admit the block)
    const uint64_t slot0 = (uint64_t) idx * 64;
    const QBox bb = T.box0[slot0 + lane];  // one base segment per lane
    for (uint64_t um = __ballot(!box_empty(bb.x0, bb.x1) && near_group(bb)); um; um &= um - 1) {
      const int j = __builtin_ctzll(um);
      const uint64_t lb2 = box_lb2(bcast(bb.x0, j), bcast(bb.y0, j), bcast(bb.x1, j), bcast(bb.y1, j), qx, qy);
      const bool adm = want && admits(ub2, lb2);
      const uint64_t am = __ballot(adm);
      if (!am) continue;
      if (STATS) st.cand += (unsigned long long) __popcll(am);
      slot(adm, T.sseg[slot0 + j], T.seid[slot0 + j]);  // (one address for the wave)
    }
  }
}

// the grid of a traversal over n > 0 points.  By size (blocks <= 0): a block per four groups up to 16 blocks per CU -- as
// many as the LDS lets be resident on a CU run, the rest queue behind them -- and the grid-stride loop takes what is left
inline dim3 grid_for(uint64_t n, int blocks, int cus) {
  const uint64_t ngroups = (n + 63) / 64;
  const uint64_t full = (ngroups + kWaves - 1) / kWaves;
  uint64_t grid = blocks > 0 ? (uint64_t) blocks : (uint64_t) (cus > 0 ? cus : 256) * 16;
  if (grid > full) grid = full;
  return dim3((uint32_t) grid);
}

}  // namespace dwalk
}  // namespace rj
