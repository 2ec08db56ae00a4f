// rj_knearest.hip -- the traversal of rj_knearest_query: a k-best-so-far search over the 64-ary implicit LBVH of
// rj_device.h with the exact predicate of rj_nearest.h and the lists of rj_knearest.h.  gfx950 only (wave = 64 lanes).
//
// THE WALK is rj_distance_walk.h's (SHAPE, STACK), with RETEST, and k_nearest's in everything but the body of a slot: no
// test against the group's box (the bounds differ from lane to lane), the children pushed so that the one nearest to the
// centre of the group's cells is popped first (centre_key, as in rj_nearest.hip), the fault word kFaultKNearestStack.
// What is k_knearest's own:
//   * THE LISTS   A lane's list of at most k candidates lives in global memory, in the slab of its wave: 6 k rows of 64
//     words, the lane is the column (rj_knearest.h: List, stride 64), so a wave's access to one word of one slot is one
//     row of 512 bytes.  Registers hold the number held and, of the worst held candidate, its slot, its double and its
//     bound only (Held: the candidate itself is loaded where the doubles cannot tell); there is no array in registers
//     that a runtime value indexes.  A lane reads nothing but what it wrote itself, in program order: no fence.
//   * A wave takes many groups in its grid-stride loop and re-uses its slab for each.  The number held starts at 0 with
//     every group and is the only thing that says which slots are live: nothing of one group's lists is seen by the next.
//   * The bound of a lane is bound_of its list: max_dist's while it holds fewer than k, then the worst's.  It only falls,
//     so a popped entry that no lane admits any more is dropped (RETEST).
//   * After the walk every live lane writes its row by selection (order_step): at most k steps over at most k slots.
//
// DUPLICATES   The walk hands a lane every edge AT MOST ONCE: a leaf slot holds one edge, every slot belongs to one leaf
// block, every block is reached through one chain of parents, and a popped entry is never pushed again -- the fact that
// rj_within_query's exact pair lists rest on.  k_nearest would not notice an edge offered twice; here it would enter the
// list twice and push a true neighbour out.
//
// No result depends on the grid, on which wave takes which points, on the order of the points or on the order of the
// leaves: a lane ends with the first k of a total order (rj_knearest.h) over every qualifying edge that was not
// dismissed, and the prune dismisses only what is strictly farther than k edges the lane already holds.
#include "rj_distance_walk.h"
#include "rj_knearest.h"

namespace rj {

using namespace knearest;

namespace {

constexpr int kBlocksPerCu = 4;  // blocks of four waves resident on a CU: four waves per SIMD at up to 128 VGPRs

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
__global__ __launch_bounds__(64 * dwalk::kWaves) void k_knearest(KNearestArgs A) {
  __shared__ dwalk::Stack lds[dwalk::kWaves];
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  const uint64_t ngroups = (A.n + 63) / 64;
  const int stack_cap = STATS && A.stack_cap < dwalk::kStack ? A.stack_cap : dwalk::kStack;  // (lowered only by tests of the fault path)
  const bool limited = A.max_dist >= 0;
  const uint32_t k = A.k;
  const uint64_t base = ub2_of_max_dist(A.max_dist);
  // this lane's column of this wave's slab
  const List list{A.slab + ((uint64_t) blockIdx.x * dwalk::kWaves + wib) * (list_words(k) * 64) + lane, 64};
  dwalk::Stats st;
  unsigned long long st_entered = 0;  // (per wave)

  for (uint64_t g = (uint64_t) blockIdx.x * dwalk::kWaves + wib; g < ngroups; g += (uint64_t) gridDim.x * dwalk::kWaves) {
    const dwalk::Group G = dwalk::load_group(A.pts, A.order, A.n, g, lane);
    // the centre of the group's cells: where the pop order looks from
    const int32_t cx = (int32_t) (((int64_t) G.gx0 + G.gx1) >> 1), cy = (int32_t) (((int64_t) G.gy0 + G.gy1) >> 1);
    Held H = held_none();
    uint64_t ub2 = base;
    dwalk::walk_group<STATS, true>(
        A.bvh, lds[wib], G, stack_cap, A.fault + kFaultKNearestStack, lane, ub2, [](const QBox&) { return true; },
        [&](uint64_t keep, int n, const QBox& b, bool mine, int ln) {
          const uint64_t key = mine ? centre_key(b, cx, cy) : 0;
          int nearer = 0;  // kept siblings that pop before this one: a smaller key, or an equal one and a lower index
          for (uint64_t um = keep; um; um &= um - 1) {
            const int c = __builtin_ctzll(um);
            const uint64_t kc = bcast64(key, c);
            nearer += (kc < key || (kc == key && c < ln)) ? 1 : 0;
          }
          return n - 1 - nearer;
        },
        [&](bool adm, const Seg& s, uint32_t eid) {
          bool entered = false;
          if (adm) {
            const Cand c = candidate(s, eid, G.px, G.py);
            if (!limited || within(c, A.max_dist)) entered = insert(list, H, k, c, approx_d2(c), true);
            if (entered) ub2 = bound_of(H, k, base);
          }
          if (STATS) st_entered += (unsigned long long) __popcll(__ballot(entered));  // (every lane is here: wave-uniform)
        },
        st);
    if (G.live) {
      const uint64_t row = G.ip * k;  // (n < 2^32 and k <= 32: 64 bits hold it)
      for (uint32_t j = 0; j < H.count; j++) {
        const Cand c = order_step(list, j, H.count, true);
        A.eid[row + j] = c.eid;
        if (A.rec) A.rec[row + j] = record_of(c);
        if (A.dist) A.dist[row + j] = dist_of(c);
      }
      for (uint32_t j = H.count; j < k; j++) {
        A.eid[row + j] = kMissEid;
        if (A.rec) A.rec[row + j] = record_miss();
        if (A.dist) A.dist[row + j] = dist_miss();
      }
      if (A.count) A.count[G.ip] = H.count;
    }
  }
  if (STATS && lane == 0 && A.stats) {
    atomicAdd(&A.stats[0], st.leaf);
    atomicAdd(&A.stats[1], st.cand);
    atomicAdd(&A.stats[2], st.nodes);
    atomicAdd(&A.stats[3], st.wave_leaf);
    atomicAdd(&A.stats[4], st_entered);
  }
}

}  // namespace

dim3 knearest_grid(uint64_t n, int blocks, int cus) {
  const dim3 by_groups = dwalk::grid_for(n, blocks, cus);  // (a block per four groups at most, or what the caller set)
  const uint32_t resident = (uint32_t) (cus > 0 ? cus : 256) * kBlocksPerCu;
  return blocks > 0 || by_groups.x <= resident ? by_groups : dim3(resident);
}

uint64_t knearest_slab_bytes(uint32_t k, dim3 grid) { return (uint64_t) grid.x * dwalk::kWaves * 64 * list_words(k) * sizeof(uint64_t); }

hipError_t launch_knearest(hipStream_t st, const KNearestArgs& a, dim3 grid, bool stats) {
  if (a.n == 0) return hipSuccess;
  if (stats)
    hipLaunchKernelGGL(k_knearest<true>, grid, dim3(64 * dwalk::kWaves), 0, st, a);
  else
    hipLaunchKernelGGL(k_knearest<false>, grid, dim3(64 * dwalk::kWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace rj
