// rj_within.hip -- the device work of rj_within_query: a fixed-bound search over the 64-ary implicit LBVH of rj_device.h
// with the exact predicate of rj_nearest.h, and the pipeline that makes a CSR of what it finds (rj_within.h: ORDER).
// gfx950 only (wave = 64 lanes).
//
// k_within   THE WALK is rj_distance_walk.h's (SHAPE, STACK), without RETEST: the bound never tightens -- ub2 =
// ub2_of_max_dist(max_dist) is wave-uniform -- so there is no pop order (a kept child lands by rank_below), no stale test
// at the pop and no candidate held per lane.  What is k_within's own:
//   * the test in front of the per-lane ballots: all 64 boxes, lane-parallel, against the box of the group's cells
//     (group_lb2, rj_within.h: a lower bound of every lane's lower bound);
//   * the body of a slot: the lanes that admit it evaluate candidate and within_filtered; a lane that hits counts the
//     hit and puts the key (ORIGINAL point number << 32) | eid into the wave's staging buffer in LDS, which is flushed 64
//     keys at a time with one atomicAdd per flush (k_lsi's lsi_flush_hits): positions at or behind the capacity are
//     counted and not written.  At the end of a group every live lane writes its count;
//   * the fault word is kFaultWithinStack.
//
// BEHIND IT   an exclusive scan of the counts (rocPRIM) gives the offsets, a small reduction the points hit and the
// longest list; the counting call ends there.  Otherwise, if the pairs fit, a radix sort of the keys over
// [0, key_bits(n)) and k_within_out, one pair per lane: the eid is the key's low word, record and distance are recomputed
// from the base map's segments in eid order and the point.
//
// No result depends on the grid, on which wave takes which points, on the order of the points or of the leaves: the set
// of keys is the set of pairs that pass an exact test which the prune never pre-empts (it dismisses only boxes whose
// lower bound exceeds max_dist), and a sorted set has one order.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_distance_walk.h"
#include "rj_within.h"

namespace rj {

using namespace nearest;
using namespace within;

namespace {

constexpr int kWithinStage = 128;  // keys of the staging buffer: below 64 in front of a slot, at most 64 more behind it

struct WithinWaveLds {  // the walk's stack and 8 bytes per key: 7424 B per wave
  dwalk::Stack stack;
  uint64_t keys[kWithinStage];
};

struct WithinMeta {
  unsigned long long appended;  // what the flushes counted
  unsigned long long n_points_hit, max_per_point;
};

// the top n (<= 64) keys of the wave's staging buffer go out behind ONE atomic; a position at or behind the capacity is
// counted and not written
__device__ __forceinline__ void within_flush(WithinWaveLds& L, int& nk, int n, unsigned long long* counter, uint64_t* keys, uint64_t cap, int lane) {
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(counter, (unsigned long long) n);
  base = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) (uint32_t) (base >> 32)) << 32) |
         (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) (uint32_t) base);
  if (lane < n) {
    const uint64_t k = L.keys[nk - n + lane];
    const unsigned long long pos = base + (unsigned long long) lane;
    if (pos < cap) keys[pos] = k;
  }
  nk -= n;
  wave_lds_fence();
}

struct WithinKernelArgs {
  WithinArgs a;
  uint32_t* cnt;     // [n]
  uint64_t* keys;    // [capacity], null in the counting call
  WithinMeta* meta;
};

template <bool STATS>
__global__ __launch_bounds__(64 * dwalk::kWaves) void k_within(WithinKernelArgs K) {
  __shared__ WithinWaveLds lds[dwalk::kWaves];
  const WithinArgs& A = K.a;
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  WithinWaveLds& L = lds[wib];
  const uint64_t ngroups = (A.n + 63) / 64;
  const int stack_cap = STATS && A.stack_cap < dwalk::kStack ? A.stack_cap : dwalk::kStack;  // (lowered only by tests of the fault path)
  const uint64_t bound = ub2_of_max_dist(A.max_dist);
  const double m2 = approx_m2(A.max_dist);
  const bool filling = K.keys != nullptr;
  dwalk::Stats st;
  unsigned long long st_pairs = 0;
  int nk = 0;  // wave-uniform fill of L.keys

  for (uint64_t g = (uint64_t) blockIdx.x * dwalk::kWaves + wib; g < ngroups; g += (uint64_t) gridDim.x * dwalk::kWaves) {
    const dwalk::Group G = dwalk::load_group(A.pts, A.order, A.n, g, lane);
    uint32_t count = 0;
    uint64_t ub2 = bound;
    dwalk::walk_group<STATS, false>(
        A.bvh, L.stack, G, stack_cap, A.fault + kFaultWithinStack, lane, ub2,
        [&](const QBox& b) { return admits(bound, group_lb2(b.x0, b.y0, b.x1, b.y1, G.gx0, G.gy0, G.gx1, G.gy1)); },
        [](uint64_t keep, int, const QBox&, bool, int) { return rank_below(keep); },
        [&](bool adm, const Seg& s, uint32_t eid) {
          const bool hit = adm && within_filtered(candidate(s, eid, G.px, G.py), A.max_dist, m2, true);
          count += hit ? 1u : 0u;
          if (!filling) return;
          const uint64_t hm = __ballot(hit);
          if (!hm) return;
          if (hit) L.keys[nk + rank_below(hm)] = pair_key((uint32_t) G.ip, eid);
          nk += __popcll(hm);
          wave_lds_fence();
          if (STATS) st_pairs += (unsigned long long) __popcll(hm);
          if (nk >= 64) within_flush(L, nk, 64, &K.meta->appended, K.keys, A.capacity, lane);
        },
        st);
    if (G.live) K.cnt[G.ip] = count;
  }
  if (nk > 0) within_flush(L, nk, nk, &K.meta->appended, K.keys, A.capacity, lane);
  if (STATS && lane == 0 && A.stats) {
    atomicAdd(&A.stats[0], st.leaf);
    atomicAdd(&A.stats[1], st.cand);
    atomicAdd(&A.stats[2], st.nodes);
    atomicAdd(&A.stats[3], st.wave_leaf);
    atomicAdd(&A.stats[4], st_pairs);
  }
}

// the points with a list and the longest list: one atomic each per block
__global__ __launch_bounds__(kThreads) void k_within_totals(const uint32_t* __restrict__ cnt, uint64_t n, WithinMeta* meta) {
  __shared__ uint32_t longest[kThreads / 64];
  uint32_t hit = 0, most = 0;
  RJ_GRID_STRIDE(i, n) {
    const uint32_t c = cnt[i];
    hit += c ? 1u : 0u;
    most = c > most ? c : most;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t) __shfl_down(most, d, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0) longest[threadIdx.x >> 6] = most;
  const uint32_t sum = block_sum(hit);  // (its barrier also publishes `longest`)
  if (threadIdx.x == 0) {
    for (int w = 0; w < kThreads / 64; w++) most = longest[w] > most ? longest[w] : most;
    if (sum) atomicAdd(&meta->n_points_hit, (unsigned long long) sum);
    if (most) atomicMax(&meta->max_per_point, (unsigned long long) most);
  }
}

// one pair per lane: the eid, and record and distance from the base map's segment in eid order and the point
__global__ __launch_bounds__(kThreads) void k_within_out(const uint64_t* __restrict__ sorted, uint64_t n_pairs, const Seg* __restrict__ seg,
                                                          const int64_t* __restrict__ pts, uint32_t* __restrict__ eid, Near* __restrict__ rec,
                                                          double* __restrict__ dist) {
  RJ_GRID_STRIDE(k, n_pairs) {
    const uint64_t key = sorted[k];
    const uint32_t e = key_eid(key), p = key_point(key);
    eid[k] = e;
    if (rec || dist) {
      const Cand c = candidate(seg[e], e, pts[2 * (uint64_t) p], pts[2 * (uint64_t) p + 1]);
      if (rec) rec[k] = record_of(c);
      if (dist) dist[k] = dist_of(c);
    }
  }
}

}  // namespace

hipError_t within_device(hipStream_t st, const WithinArgs& a, bool stats, int blocks, int cus, StageEvents* ev, WithinResult* result) {
  *result = WithinResult{};
  const uint64_t n = a.n, cap = a.capacity;
  char *block = nullptr, *sort_block = nullptr;
  hipError_t e = hipSuccess;
  do {
    // what is sized by the points and by the capacity
    TempSize scan_temp;
    scan_temp([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), st);
    });
    if ((e = scan_temp.error) != hipSuccess) break;
    WithinMeta* meta;
    uint32_t* cnt;
    uint64_t *scanned, *keys;
    void* temp;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<WithinMeta>(1);
      cnt = A.take<uint32_t>(n + 1);
      scanned = A.take<uint64_t>(n + 1);
      temp = A.take<char>(scan_temp.bytes);
      keys = A.take<uint64_t>(cap);  // (the counting call: none)
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    // 1. the traversal
    if ((e = ev->mark(1, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(WithinMeta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(cnt + n, 0, sizeof(uint32_t), st)) != hipSuccess) break;
    if (n) {
      WithinKernelArgs K{a, cnt, cap ? keys : nullptr, meta};
      const dim3 grid = dwalk::grid_for(n, blocks, cus);  // (7424 B of LDS per wave: 5 blocks of four waves are resident on a CU)
      if (stats)
        hipLaunchKernelGGL(k_within<true>, grid, dim3(64 * dwalk::kWaves), 0, st, K);
      else
        hipLaunchKernelGGL(k_within<false>, grid, dim3(64 * dwalk::kWaves), 0, st, K);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    if ((e = ev->mark(2, st)) != hipSuccess) break;
    // 2. the offsets and the counts
    size_t tb = scan_temp.bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) cnt, scanned, (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), st)) != hipSuccess) break;
    if (n) {
      hipLaunchKernelGGL(k_within_totals, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, (const uint32_t*) cnt, n, meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    WithinMeta m;
    uint64_t n_pairs = 0;
    if ((e = hipMemcpyAsync(&m, meta, sizeof(m), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(&n_pairs, scanned + n, sizeof(n_pairs), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if (a.offsets && (e = hipMemcpyAsync(a.offsets, scanned, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // the first sync: how many pairs there are
    result->counts = Counts{n_pairs, m.n_points_hit, m.max_per_point};
    result->appended = cap ? m.appended : n_pairs;
    // 3. the sort and the outputs
    if (cap && n_pairs <= cap && result->appended == n_pairs) {
      if (n_pairs) {
        const int bits = key_bits(n);
        TempSize sort_temp;
        sort_temp([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) n_pairs, 0, bits, st); });
        if ((e = sort_temp.error) != hipSuccess) break;
        uint64_t* sorted;
        void* stemp;
        Carve B;
        auto carve_sort = [&]() {
          B.used = 0;
          sorted = B.take<uint64_t>(n_pairs);
          stemp = B.take<char>(sort_temp.bytes);
        };
        carve_sort();
        if ((e = hipMalloc((void**) &sort_block, B.used)) != hipSuccess) break;
        B.base = sort_block;
        carve_sort();
        tb = sort_temp.bytes;
        if ((e = rocprim::radix_sort_keys(stemp, tb, (const uint64_t*) keys, sorted, (size_t) n_pairs, 0, bits, st)) != hipSuccess) break;
        hipLaunchKernelGGL(k_within_out, dim3(blocks_for(n_pairs, 4096)), dim3(kThreads), 0, st, (const uint64_t*) sorted, n_pairs, a.seg, a.pts, a.eid, a.rec, a.dist);
        if ((e = hipGetLastError()) != hipSuccess) break;
      }
      result->emitted = true;
    }
    if ((e = ev->mark(3, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the last sync: nothing of this call runs when its scratch goes
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  const hipError_t fa = hipFree(block), fb = hipFree(sort_block);
  return e != hipSuccess ? e : (fa != hipSuccess ? fa : fb);
}

}  // namespace rj
