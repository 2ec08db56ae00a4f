// rj_snap.hip -- cutting a chain map at its touches, overlaps and rounded proper crossings on the device (rj_snap.h has
// the definition and the stages).  The pipeline is rj_cut_pipeline.h's, shared with rj_node.hip; here are the candidates
// kernel and what the pipeline takes from this call (SnapCuts).  One thread per record makes the four tests of a touch
// or the rounded point of a proper crossing -- two 26-step divisions per coordinate on 128-bit integers, no call and no
// floating point -- and the hits of a wave are appended with one atomic (ballot and rank).  A cut carries its point, not
// a source index: 32 bytes with its two key words.
#include <hip/hip_runtime.h>

#include "rj_cut_pipeline.h"
#include "rj_node.h"
#include "rj_pipeline.h"
#include "rj_snap.h"

namespace rj {

using namespace snap;

namespace {

// One thread per record, a wave's lanes on 64 consecutive records: the cuts of the record (at most two whatever its
// kind), then one atomic for the wave's hits.  Hit t of lane l goes behind the hits of slot 0 (for t = 1) and the hits
// of slot t in the lanes below l.
__global__ __launch_bounds__(kThreads) void k_sn_cands(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy,
                                                       const Record* __restrict__ rec, uint64_t n_rec, Cut* __restrict__ cand, uint64_t cap, Meta* meta) {
  if (meta->bad) return;
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
  uint32_t used = 0, proper = 0, equal = 0, exact = 0, at_end = 0, stale = 0;
  for (uint64_t r0 = blockIdx.x * (uint64_t) blockDim.x + (threadIdx.x & ~63u); r0 < n_rec; r0 += stride) {  // (wave-uniform)
    const uint64_t r = r0 + lane;
    int k = 0;
    Cut c0, c1;
    if (r < n_rec) {
      const Record R = rec[r];
      proper += R.kind == crossings::kProper;
      equal += R.kind == crossings::kEqual;
      if (R.kind != crossings::kEqual) {
        const uint64_t pe = R.eid[0] + crossings::chain_of(R.eid[0], row, nc), pf = R.eid[1] + crossings::chain_of(R.eid[1], row, nc);
        const Edge E{xy[2 * pe], xy[2 * pe + 1], xy[2 * pe + 2], xy[2 * pe + 3]}, F{xy[2 * pf], xy[2 * pf + 1], xy[2 * pf + 2], xy[2 * pf + 3]};
        if (node::cuts(R.kind)) {
          used++;
          k = touch_cuts(R.eid[0], R.eid[1], E, F, &c0, &c1);
        } else {
          const Proper p = proper_point(E, F);
          uint32_t ends;
          k = proper_cuts(R.eid[0], R.eid[1], E, F, p, &c0, &c1, &ends);
          stale += p.stale;
          exact += p.exact;
          at_end += ends;
        }
      }
    }
    const uint64_t h0 = __ballot(k > 0), h1 = __ballot(k > 1);
    const uint32_t n0 = (uint32_t) __popcll(h0), total = n0 + (uint32_t) __popcll(h1);
    if (!total) continue;
    ull base = 0;
    if (lane == 0) base = atomicAdd((ull*) &meta->n_cand, (ull) total);
    base = ((ull) __builtin_amdgcn_readfirstlane((uint32_t) (base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t) base);
    const ull below = (1ull << lane) - 1, p0 = base + (ull) __popcll(h0 & below), p1 = base + n0 + (ull) __popcll(h1 & below);
    if (k > 0 && p0 < cap) cand[p0] = c0;
    if (k > 1 && p1 < cap) cand[p1] = c1;
  }
  count_to(&meta->counts.n_used, used);
  count_to(&meta->counts.n_proper, proper);
  count_to(&meta->counts.n_equal, equal);
  count_to(&meta->counts.n_exact, exact);
  count_to(&meta->counts.n_at_end, at_end);
  count_to(&meta->counts.n_stale, stale);
}

// what rj_cut_pipeline.h takes from this call: a cut of 32 bytes that carries its point
struct SnapCuts {
  using Cut = snap::Cut;
  using Meta = snap::Meta;
  struct Before {
    __host__ __device__ bool operator()(const Cut& a, const Cut& b) const { return cut_before(a, b); }
  };
  static RJ_RHD bool head(uint64_t i, const Cut* s) { return cut_head(i, s); }
  static RJ_RHD bool run_first(uint64_t i, const Cut* s) { return snap::run_first(i, s); }
  static RJ_RHD bool run_last(uint64_t i, uint64_t n, const Cut* s) { return snap::run_last(i, n, s); }
  static RJ_RHD uint32_t edge(const Cut& c) { return cut_edge(c); }
  static RJ_RHD void point(const Cut& c, const int64_t*, int64_t* q) {
    q[0] = c.qx;
    q[1] = c.qy;
  }
  static RJ_RHD void totals(uint64_t np, uint64_t nc, uint64_t n_cuts, uint32_t flags, uint64_t capacity, Counts* counts, uint32_t* emit) {
    snap::totals(np, nc, n_cuts, flags, capacity, counts, emit);
  }
  static void launch_cands(int blocks, hipStream_t st, const uint32_t* row, uint64_t nc, const int64_t* xy, const Record* rec, uint64_t n_rec, Cut* cand,
                           uint64_t cap, Meta* meta) {
    hipLaunchKernelGGL(k_sn_cands, dim3(blocks), dim3(kThreads), 0, st, row, nc, xy, rec, n_rec, cand, cap, meta);
  }
};

}  // namespace

hipError_t map_snap_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec_dev, uint64_t n_rec,
                           uint32_t flags, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Meta* result, SnapReport* report) {
  return cut::run<SnapCuts>(st, xy, np, row, nc, rec_dev, n_rec, flags, capacity, out_xy, out_row, origin, result, report);
}

}  // namespace rj
