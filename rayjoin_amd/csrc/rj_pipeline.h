// rj_pipeline.h -- what the multi-stage device pipelines share (rj_stitch.hip, rj_strip.hip, rj_overlay.hip,
// rj_overlay_map.hip, rj_rings.hip, rj_grid.hip, rj_polygons.hip, rj_ringmap.hip, rj_crossings.hip, rj_simplify.hip,
// rj_faces.hip, rj_eliminate.hip, rj_dissolve.hip, rj_neighbours.hip, rj_node.hip and rj_snap.hip through rj_cut_pipeline.h, and their callers in
// rj_api.hip): the launch width, the grid-stride loop, the carving of one scratch block, the grow-only block itself,
// the block-wide sum and the counter update behind it, the largest of rocPRIM's temporary sizes, and the stage times
// of a call with the events that measure them.  No state, no .hip file of its own.  HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rj {

constexpr int kThreads = 256;
typedef unsigned long long ull;  // what the 64-bit atomics take

// blocks of kThreads for n items, at least one, at most cap_blocks (the grid-stride loop takes the rest)
inline int blocks_for(uint64_t n, int cap_blocks) {
  uint64_t b = (n + kThreads - 1) / kThreads;
  return (int) (b < 1 ? 1 : (b > (uint64_t) cap_blocks ? (uint64_t) cap_blocks : b));
}

#define RJ_GRID_STRIDE(i, n) \
  for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < (n); i += (uint64_t) gridDim.x * blockDim.x)

// one allocation, carved into 256-byte aligned arrays: sizes first (base null, `used` is the block's size), then the
// pointers (the same takes again with base set)
struct Carve {
  char* base = nullptr;
  size_t used = 0;
  template <typename T>
  T* take(uint64_t count) {
    used = (used + 255) & ~(size_t) 255;
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += count * sizeof(T);
    return p;
  }
};

// a grow-only block that stays with its owner: nothing happens while it is large enough (no per-call hipMalloc /
// hipFree: hipFree waits for the device and unmaps).  A failed allocation leaves no block: null, zero bytes.
inline hipError_t grow_block(char** block, size_t* bytes, size_t need) {
  if (need <= *bytes) return hipSuccess;
  (void) hipFree(*block);
  *block = nullptr;
  *bytes = 0;
  const hipError_t e = hipMalloc((void**) block, need);
  if (e != hipSuccess) {
    *block = nullptr;
    return e;
  }
  *bytes = need;
  return hipSuccess;
}

// the sum of `mine` over the block, in thread 0: one atomic per block behind it (27 k same-address atomics, one per
// wave of a 1.7 M-incidence map, were 90 % of the stitch's ranking round).  Blocks of kThreads.
__device__ __forceinline__ uint32_t block_sum(uint32_t mine) {
  __shared__ uint32_t part[kThreads / 64];
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  uint32_t sum = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; w++) sum += part[w];
  return sum;
}
// *counter += the block's sum of `mine`: one atomic per block, none for a sum of zero.  Every thread of the block calls.
__device__ __forceinline__ void count_to(uint64_t* counter, uint32_t mine) {
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd((ull*) counter, (ull) sum);
  __syncthreads();  // (block_sum's partial sums are free again)
}

// the temporary storage of a pipeline's rocPRIM calls: one line per call that it will make -- the call itself with a
// null temp, as `[&](size_t& b) { return rocprim::...(nullptr, b, ...); }` -- then `bytes` is the largest size and
// `error` the first failure (no query is made behind one)
struct TempSize {
  size_t bytes = 0;
  hipError_t error = hipSuccess;
  template <class Query>
  void operator()(Query&& query) {
    if (error != hipSuccess) return;
    size_t b = 0;
    error = query(b);
    if (error == hipSuccess && b > bytes) bytes = b;
  }
};

// what the five stages of a call took and, in entry 5, the whole call, in ms.  -1: not measured -- no call yet, a call
// refused before its first stage, or a stage that was not reached.  A pipeline's report derives from it.
struct StageMs {
  float ms[6] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
};
// the six events around the five stages of a call, destroyed with the scope: mark(k) in front of stage k, mark(5) behind
// the last stage
struct StageEvents {
  hipEvent_t ev[6] = {};
  ~StageEvents() {
    for (hipEvent_t e : ev)
      if (e) (void) hipEventDestroy(e);
  }
  hipError_t create() {
    for (hipEvent_t& e : ev)
      if (hipError_t r = hipEventCreate(&e)) return r;
    return hipSuccess;
  }
  hipError_t mark(int k, hipStream_t st) { return hipEventRecord(ev[k], st); }
  // behind a sync that event `reached` lies in front of: stage k = ev[k] -> ev[k + 1] for the stages reached, entry 5 =
  // ev[0] -> ev[reached]; the other entries stay as they are
  void times(int reached, float ms[6]) const {
    for (int k = 0; k < reached; k++) (void) hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    if (reached > 0) (void) hipEventElapsedTime(&ms[5], ev[0], ev[reached]);
  }
};

}  // namespace rj
