// rj_nearest.hip -- the traversal of rj_nearest_query: a best-so-far search over the 64-ary implicit LBVH of rj_device.h
// with the exact predicate of rj_nearest.h.  gfx950 only (wave = 64 lanes).
//
// THE WALK is rj_distance_walk.h's (SHAPE, STACK), with RETEST.  What is k_nearest's own:
//   * every lane keeps its best candidate and tightens its bound ub2 with it (rj_nearest.h: ub2_of), slot by slot;
//   * there is no test against the group's box (near_group: always true): the bounds differ from lane to lane;
//   * the children are pushed so that the one nearest to the centre of the group's cells is popped first (centre_key):
//     the first leaf a group sees is then the one around it, and the bounds are tight before the second pop;
//   * the fault word is kFaultNearestStack.
//
// No result depends on the grid, on which wave takes which points, on the order of the points or on the order of the
// leaves: a lane ends with the minimum of a total order (closer() of the header: distance, then eid) over every edge that
// was not dismissed, and the prune dismisses only what is strictly farther than something the lane already holds.
#include "rj_distance_walk.h"

namespace rj {

using namespace nearest;

namespace {

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
__global__ __launch_bounds__(64 * dwalk::kWaves) void k_nearest(NearestArgs A) {
  __shared__ dwalk::Stack lds[dwalk::kWaves];
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  const uint64_t ngroups = (A.n + 63) / 64;
  const int stack_cap = STATS && A.stack_cap < dwalk::kStack ? A.stack_cap : dwalk::kStack;  // (lowered only by tests of the fault path)
  const bool limited = A.max_dist >= 0;
  dwalk::Stats st;

  for (uint64_t g = (uint64_t) blockIdx.x * dwalk::kWaves + wib; g < ngroups; g += (uint64_t) gridDim.x * dwalk::kWaves) {
    const dwalk::Group G = dwalk::load_group(A.pts, A.order, A.n, g, lane);
    // the centre of the group's cells: where the pop order looks from
    const int32_t cx = (int32_t) (((int64_t) G.gx0 + G.gx1) >> 1), cy = (int32_t) (((int64_t) G.gy0 + G.gy1) >> 1);
    Cand best = Cand{kMissEid, 0, 0, 0};
    double best_d2 = 0.0;
    uint64_t ub2 = ub2_of_max_dist(A.max_dist);
    dwalk::walk_group<STATS, true>(
        A.bvh, lds[wib], G, stack_cap, A.fault + kFaultNearestStack, lane, ub2, [](const QBox&) { return true; },
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
          if (!adm) return;
          const Cand c = candidate(s, eid, G.px, G.py);
          if (!limited || within(c, A.max_dist)) {
            const double d2 = approx_d2(c);
            if (best.eid == kMissEid || closer(c, d2, best, best_d2, true)) {
              best = c;
              best_d2 = d2;
              const uint64_t u = ub2_of(c, d2);
              ub2 = u < ub2 ? u : ub2;
            }
          }
        },
        st);
    if (G.live) {
      const bool hit = best.eid != kMissEid;
      A.eid[G.ip] = best.eid;
      if (A.rec) A.rec[G.ip] = hit ? record_of(best) : record_miss();
      if (A.dist) A.dist[G.ip] = hit ? dist_of(best) : dist_miss();
    }
  }
  if (STATS && lane == 0 && A.stats) {
    atomicAdd(&A.stats[0], st.leaf);
    atomicAdd(&A.stats[1], st.cand);
    atomicAdd(&A.stats[2], st.nodes);
    atomicAdd(&A.stats[3], st.wave_leaf);
  }
}

}  // namespace

hipError_t launch_nearest(hipStream_t st, const NearestArgs& a, bool stats, int blocks, int cus) {
  if (a.n == 0) return hipSuccess;
  const dim3 grid = dwalk::grid_for(a.n, blocks, cus);  // (6400 B of LDS per wave: 6 blocks of four waves are resident on a CU)
  if (stats)
    hipLaunchKernelGGL(k_nearest<true>, grid, dim3(64 * dwalk::kWaves), 0, st, a);
  else
    hipLaunchKernelGGL(k_nearest<false>, grid, dim3(64 * dwalk::kWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace rj
