// rj_node.hip -- noding a chain map on the device (rj_node.h has the definition and the stages).  The pipeline is
// rj_cut_pipeline.h's, shared with rj_snap.hip; here are the candidates kernel and what the pipeline takes from this
// call (NodeCuts).  One thread per record makes the four tests and the hits of a wave are appended with one atomic
// (ballot and rank, as k_cx_pairs appends).
#include <hip/hip_runtime.h>

#include "rj_cut_pipeline.h"
#include "rj_node.h"
#include "rj_pipeline.h"

namespace rj {

using namespace node;

namespace {

// One thread per record, a wave's lanes on 64 consecutive records: the four tests, then one atomic for the wave's hits.
// Hit t of lane l goes behind the hits of the tests before t and the hits of test t in the lanes below l.
__global__ __launch_bounds__(kThreads) void k_nd_cands(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy,
                                                       const Record* __restrict__ rec, uint64_t n_rec, Cut* __restrict__ cand, uint64_t cap, Meta* meta) {
  if (meta->bad) return;
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
  uint32_t used = 0, proper = 0, equal = 0;
  for (uint64_t r0 = blockIdx.x * (uint64_t) blockDim.x + (threadIdx.x & ~63u); r0 < n_rec; r0 += stride) {  // (wave-uniform)
    const uint64_t r = r0 + lane;
    bool hit[4] = {false, false, false, false};
    Cut cut[4];
    if (r < n_rec) {
      const Record R = rec[r];
      proper += R.kind == crossings::kProper;
      equal += R.kind == crossings::kEqual;
      if (cuts(R.kind)) {
        used++;
        const uint64_t pe = R.eid[0] + crossings::chain_of(R.eid[0], row, nc), pf = R.eid[1] + crossings::chain_of(R.eid[1], row, nc);
        const Edge E{xy[2 * pe], xy[2 * pe + 1], xy[2 * pe + 2], xy[2 * pe + 3]}, F{xy[2 * pf], xy[2 * pf + 1], xy[2 * pf + 2], xy[2 * pf + 3]};
#pragma unroll
        for (int t = 0; t < 4; t++) hit[t] = candidate(t, R.eid[0], R.eid[1], E, F, pe, pf, &cut[t]);
      }
    }
    uint64_t hm[4];
    uint32_t total = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      hm[t] = __ballot(hit[t]);
      total += (uint32_t) __popcll(hm[t]);
    }
    if (!total) continue;
    ull base = 0;
    if (lane == 0) base = atomicAdd((ull*) &meta->n_cand, (ull) total);
    base = ((ull) __builtin_amdgcn_readfirstlane((uint32_t) (base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t) base);
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const ull pos = base + (ull) __popcll(hm[t] & ((1ull << lane) - 1));
      if (hit[t] && pos < cap) cand[pos] = cut[t];
      base += (ull) __popcll(hm[t]);
    }
  }
  count_to(&meta->counts.n_used, used);
  count_to(&meta->counts.n_proper, proper);
  count_to(&meta->counts.n_equal, equal);
}

// what rj_cut_pipeline.h takes from this call: a cut of 16 bytes that names its point by the input point's number
struct NodeCuts {
  using Cut = node::Cut;
  using Meta = node::Meta;
  struct Before {
    __host__ __device__ bool operator()(const Cut& a, const Cut& b) const { return cut_before(a, b); }
  };
  static RJ_RHD bool head(uint64_t i, const Cut* s) { return cut_head(i, s); }
  static RJ_RHD bool run_first(uint64_t i, const Cut* s) { return node::run_first(i, s); }
  static RJ_RHD bool run_last(uint64_t i, uint64_t n, const Cut* s) { return node::run_last(i, n, s); }
  static RJ_RHD uint32_t edge(const Cut& c) { return c.edge; }
  static RJ_RHD void point(const Cut& c, const int64_t* xy, int64_t* q) {
    q[0] = xy[2 * (uint64_t) c.src];
    q[1] = xy[2 * (uint64_t) c.src + 1];
  }
  static RJ_RHD void totals(uint64_t np, uint64_t nc, uint64_t n_cuts, uint32_t flags, uint64_t capacity, Counts* counts, uint32_t* emit) {
    node::totals(np, nc, n_cuts, flags, capacity, counts, emit);
  }
  static void launch_cands(int blocks, hipStream_t st, const uint32_t* row, uint64_t nc, const int64_t* xy, const Record* rec, uint64_t n_rec, Cut* cand,
                           uint64_t cap, Meta* meta) {
    hipLaunchKernelGGL(k_nd_cands, dim3(blocks), dim3(kThreads), 0, st, row, nc, xy, rec, n_rec, cand, cap, meta);
  }
};

}  // namespace

hipError_t map_node_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec_dev, uint64_t n_rec,
                           uint32_t flags, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Meta* result, NodeReport* report) {
  return cut::run<NodeCuts>(st, xy, np, row, nc, rec_dev, n_rec, flags, capacity, out_xy, out_row, origin, result, report);
}

}  // namespace rj
