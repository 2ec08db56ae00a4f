// rj_nearest.hip -- the traversal of rj_nearest_query: a best-so-far search over the 64-ary implicit LBVH of rj_device.h
// with the exact predicate of rj_nearest.h.  gfx950 only (wave = 64 lanes).
//
// SHAPE   One wave takes 64 consecutive points of the (possibly Morton-ordered) set, one per lane, and walks the tree
// depth-first with ONE stack in LDS.  The lanes keep their own best candidate and their own bound ub2 (rj_nearest.h:
// d^2 <= 2^32 ub2); what they share is the order of the walk and every load.
//   * A node's 64 children are one coalesced load, lane = child.  A child is pushed while SOME lane admits it
//     (admits(ub2, box_lb2) of the header, per lane, the child's box broadcast): exact per lane, so a wave of scattered
//     points -- a shuffled set without the Morton order -- still opens only what one of its points needs.
//   * The children are pushed so that the one nearest to the centre of the group's cells is popped first: the first leaf
//     a group sees is then the one around it, and the bounds are tight before the second pop.  The order is a heuristic
//     only; any order gives the same result.
//   * A popped entry carries its box: the lanes test it again against the bounds as they are NOW, and an entry that no
//     lane admits any more is dropped without a load.
//   * A leaf block's 64 boxes are one coalesced load; slot after slot the box is broadcast, and the segment of a slot is
//     loaded (one address for the wave) and evaluated exactly only by the lanes that admit its box.  A lane's bound
//     tightens inside the block, slot by slot.
//   * Padding slots (inside a block under "leaf_order" 1, and behind the last block) and the nodes above nothing but
//     padding have the empty box: excluded explicitly by box_empty -- before the first candidate the bound admits
//     everything, and a zero segment at the origin would be a phantom edge.
//
// STACK   A pop removes one entry and pushes at most the 64 children of that node, all one level lower; a batch of
// children is consumed completely before anything below it is touched.  From the <= 64 entries of the top level the
// stack therefore holds at most 64 + 63 (top - 1) entries: 64 at the start, and 63 more for every level descended.
// That is k_pip's discipline and k_pip's bound (kPipStack, rj_device.h; simulated in tests/test_stack_bounds.py).
// Every push is still checked against the capacity and raises the handle's fault word kFaultNearestStack
// (-> RJ_E_INTERNAL) instead of writing past the stack.
//
// No result depends on the grid, on which wave takes which points, on the order of the points or on the order of the
// leaves: a lane ends with the minimum of a total order (closer() of the header: distance, then eid) over every edge that
// was not dismissed, and the prune dismisses only what is strictly farther than something the lane already holds.
#include "rj_nearest.h"

namespace rj {

using namespace nearest;

namespace {

constexpr int kNearestWaves = 4;          // waves per block
constexpr int kNearestStack = kPipStack;  // 64 + 63 (kMaxTop - 1) and four to spare: see STACK above

struct NearestWaveLds {  // 20 bytes per entry: 6400 B per wave
  uint4 box[kNearestStack];     // {x0, y0, x1, y1} of the node
  uint32_t code[kNearestStack]; // level << 28 | index
};

__device__ __noinline__ void raise_nearest_fault(uint32_t* fault) {
  // a plain store (idempotent), not an atomic: the word is pinned host memory the device writes directly
  __hip_atomic_store(fault + kFaultNearestStack, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t bcast64(uint64_t v, int src_lane_uniform) {
  const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int32_t) (uint32_t) v, src_lane_uniform);
  const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int32_t) (uint32_t) (v >> 32), src_lane_uniform);
  return ((uint64_t) hi << 32) | lo;
}
// squared distance in cells from the cell (cx, cy) to a box that is not empty: the key of the pop order
__device__ __forceinline__ uint64_t centre_key(const QBox& b, int32_t cx, int32_t cy) {
  const int32_t ax = b.x0 - cx > cx - b.x1 ? b.x0 - cx : cx - b.x1, ay = b.y0 - cy > cy - b.y1 ? b.y0 - cy : cy - b.y1;
  const uint32_t gx = ax > 0 ? (uint32_t) ax : 0u, gy = ay > 0 ? (uint32_t) ay : 0u;
  return (uint64_t) gx * gx + (uint64_t) gy * gy;
}

template <bool STATS>
__global__ __launch_bounds__(64 * kNearestWaves) void k_nearest(NearestArgs A) {
  __shared__ NearestWaveLds lds[kNearestWaves];
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  NearestWaveLds& L = lds[wib];
  const DeviceBvh& T = A.bvh;
  const uint64_t ngroups = (A.n + 63) / 64;
  const int stack_cap = STATS && A.stack_cap < kNearestStack ? A.stack_cap : kNearestStack;  // (lowered only by tests of the fault path)
  const bool limited = A.max_dist >= 0;
  unsigned long long st_leaf = 0, st_cand = 0, st_nodes = 0, st_wave_leaf = 0;

  for (uint64_t g = (uint64_t) blockIdx.x * kNearestWaves + wib; g < ngroups; g += (uint64_t) gridDim.x * kNearestWaves) {
    const uint64_t ipos = g * 64 + lane;
    const bool live = ipos < A.n;
    const uint64_t ip = A.order ? (live ? A.order[ipos] : 0) : ipos;
    int64_t px = 0, py = 0;
    if (live) {
      px = A.pts[2 * ip];
      py = A.pts[2 * ip + 1];
    }
    const int32_t qx = cell_of(px), qy = cell_of(py);
    // the centre of the group's cells: where the pop order looks from
    const int32_t cx = (int32_t) (((int64_t) wave_min(live ? qx : kEmptyMin) + wave_max(live ? qx : kEmptyMax)) >> 1);
    const int32_t cy = (int32_t) (((int64_t) wave_min(live ? qy : kEmptyMin) + wave_max(live ? qy : kEmptyMax)) >> 1);
    Cand best = Cand{kMissEid, 0, 0, 0};
    double best_d2 = 0.0;
    uint64_t ub2 = ub2_of_max_dist(A.max_dist);
    int sp = 0;

    // the children of a node (lane = child; b: this lane's, `have`: it exists) onto the stack, see SHAPE
    auto push_children = [&](int lvl, uint32_t first, const QBox& b, bool have) {
      uint64_t keep = 0;
      for (uint64_t um = __ballot(have && !box_empty(b.x0, b.x1)); um; um &= um - 1) {
        const int c = __builtin_ctzll(um);
        const uint64_t lb2 = box_lb2(bcast(b.x0, c), bcast(b.y0, c), bcast(b.x1, c), bcast(b.y1, c), qx, qy);
        if (__ballot(live && admits(ub2, lb2))) keep |= 1ull << c;
      }
      const int n = __popcll(keep);
      if (sp + n > stack_cap) {
        if (lane == 0) raise_nearest_fault(A.fault);
        return;
      }
      const bool mine = (keep >> lane) & 1;
      const uint64_t key = mine ? centre_key(b, cx, cy) : 0;
      int nearer = 0;  // kept siblings that pop before this one: a smaller key, or an equal one and a lower index
      for (uint64_t um = keep; um; um &= um - 1) {
        const int c = __builtin_ctzll(um);
        const uint64_t kc = bcast64(key, c);
        nearer += (kc < key || (kc == key && c < lane)) ? 1 : 0;
      }
      if (mine) {
        const int at = sp + n - 1 - nearer;
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
      const int32_t ex0 = __builtin_amdgcn_readfirstlane((int32_t) eb.x), ey0 = __builtin_amdgcn_readfirstlane((int32_t) eb.y);
      const int32_t ex1 = __builtin_amdgcn_readfirstlane((int32_t) eb.z), ey1 = __builtin_amdgcn_readfirstlane((int32_t) eb.w);
      // stale?  (the bounds have tightened since the push)
      const bool want = live && admits(ub2, box_lb2(ex0, ey0, ex1, ey1, qx, qy));
      if (!__ballot(want)) continue;
      const int lvl = (int) (e >> 28);
      const uint32_t idx = e & 0x0FFFFFFFu;
      if (lvl > 1) {
        if (STATS) st_nodes++;
        push_children(lvl - 1, idx * 64u, T.lvl[lvl - 1][(uint64_t) idx * 64 + lane], true);
        continue;
      }
      if (STATS) st_leaf += (unsigned long long) __popcll(__ballot(want)), st_wave_leaf++;  // (per point: the lanes that admit the block)
      const uint64_t slot0 = (uint64_t) idx * 64;
      const QBox bb = T.box0[slot0 + lane];  // one base segment per lane
      for (uint64_t um = __ballot(!box_empty(bb.x0, bb.x1)); um; um &= um - 1) {
        const int j = __builtin_ctzll(um);
        const uint64_t lb2 = box_lb2(bcast(bb.x0, j), bcast(bb.y0, j), bcast(bb.x1, j), bcast(bb.y1, j), qx, qy);
        const bool adm = want && admits(ub2, lb2);
        const uint64_t am = __ballot(adm);
        if (!am) continue;
        if (STATS) st_cand += (unsigned long long) __popcll(am);
        const Seg s = T.sseg[slot0 + j];  // (one address for the wave)
        const uint32_t eid = T.seid[slot0 + j];
        if (adm) {
          const Cand c = candidate(s, eid, px, py);
          if (!limited || within(c, A.max_dist)) {
            const double d2 = approx_d2(c);
            if (best.eid == kMissEid || closer(c, d2, best, best_d2, true)) {
              best = c;
              best_d2 = d2;
              const uint64_t u = ub2_of(c, d2);
              ub2 = u < ub2 ? u : ub2;
            }
          }
        }
      }
    }
    if (live) {
      const bool hit = best.eid != kMissEid;
      A.eid[ip] = best.eid;
      if (A.rec) A.rec[ip] = hit ? record_of(best) : record_miss();
      if (A.dist) A.dist[ip] = hit ? dist_of(best) : dist_miss();
    }
  }
  if (STATS && lane == 0 && A.stats) {
    atomicAdd(&A.stats[0], st_leaf);
    atomicAdd(&A.stats[1], st_cand);
    atomicAdd(&A.stats[2], st_nodes);
    atomicAdd(&A.stats[3], st_wave_leaf);
  }
}

}  // namespace

hipError_t launch_nearest(hipStream_t st, const NearestArgs& a, bool stats, int blocks, int cus) {
  if (a.n == 0) return hipSuccess;
  const uint64_t ngroups = (a.n + 63) / 64;
  const uint64_t full = (ngroups + kNearestWaves - 1) / kNearestWaves;
  // by size: a block per four groups up to 16 blocks per CU (6400 B of LDS per wave: 6 blocks of four waves are resident
  // on a CU, the rest queue behind them); the grid-stride loop takes what is left
  uint64_t grid = blocks > 0 ? (uint64_t) blocks : (uint64_t) (cus > 0 ? cus : 256) * 16;
  if (grid > full) grid = full;
  if (stats)
    hipLaunchKernelGGL(k_nearest<true>, dim3((uint32_t) grid), dim3(64 * kNearestWaves), 0, st, a);
  else
    hipLaunchKernelGGL(k_nearest<false>, dim3((uint32_t) grid), dim3(64 * kNearestWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace rj
