// rj_snap.hip -- cutting a chain map at its touches, overlaps and rounded proper crossings on the device (rj_snap.h has
// the definition and the stages).  The pipeline has the shape of rj_node.hip: every kernel is a grid-stride loop over
// one of rj_snap.h's per-element functions; rocPRIM does the merge sort of the candidates and the two scans.  One thread
// per record makes the four tests of a touch or the rounded point of a proper crossing -- two 26-step divisions per
// coordinate on 128-bit integers, no call and no floating point -- and the hits of a wave are appended with one atomic
// (ballot and rank).  A cut carries its point, not a source index: 32 bytes with its two key words.  The candidate array
// has the 2 n_rec slots a call can fill, the unused ones hold all ones and sort to the end, so that no size has to be
// read back: the stream is synchronised once, at the end, for the counts.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <string.h>

#include "rj_node.h"
#include "rj_pipeline.h"
#include "rj_snap.h"

namespace rj {

using namespace snap;

namespace {

typedef unsigned long long ull;

struct CutBefore {
  __host__ __device__ bool operator()(const Cut& a, const Cut& b) const { return cut_before(a, b); }
};

__device__ __forceinline__ void count_to(uint64_t* counter, uint32_t mine) {
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd((ull*) counter, (ull) sum);
  __syncthreads();  // (block_sum's partial sums are free again)
}

__global__ __launch_bounds__(kThreads) void k_sn_check(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy, uint64_t np,
                                                       const Record* __restrict__ rec, uint64_t n_rec, uint32_t flags, Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, crossings::check_row(c, row, nc, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, crossings::check_coordinate(xy[i]));
  if (flags & kDropLast) RJ_GRID_STRIDE(c, nc) bad = max(bad, node::check_chain(c, row, np, xy));
  RJ_GRID_STRIDE(r, n_rec) bad = max(bad, node::check_record(r, rec, np - nc, row, nc, xy));
  if (bad) atomicMax(&meta->bad, bad);
}
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
__global__ __launch_bounds__(kThreads) void k_sn_heads(uint64_t n, const Cut* __restrict__ s, uint32_t* __restrict__ keep, const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, n) keep[i] = cut_head(i, s) ? 1u : 0u;
}
// first[e], last[e]: the numbers of the kept cuts of e (zeroed before: edges without a cut keep 0, 0)
__global__ __launch_bounds__(kThreads) void k_sn_runs(uint64_t n, const Cut* __restrict__ s, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ kidx, uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                      const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, n) {
    const uint32_t e = cut_edge(s[i]);
    if (e == kNoEdge) continue;
    if (run_first(i, s)) first[e] = kidx[i];
    if (run_last(i, n, s)) last[e] = kidx[i] + keep[i];
  }
}
// cnt[e] = last[e] - first[e] in place of last[e], entry ne closes the scan; the counts that need no scan
__global__ __launch_bounds__(kThreads) void k_sn_count(uint64_t ne, const uint32_t* __restrict__ first, uint32_t* __restrict__ cnt, uint64_t n,
                                                       const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kidx, uint64_t np, uint64_t nc,
                                                       uint32_t flags, uint64_t capacity, Meta* meta) {
  if (meta->bad) return;
  uint32_t cut_edges = 0, most = 0;
  RJ_GRID_STRIDE(e, ne + 1) {
    const uint32_t k = e < ne ? cnt[e] - first[e] : 0;
    cnt[e] = k;
    cut_edges += k != 0;
    most = max(most, k);
  }
  for (int d = 32; d >= 1; d >>= 1) most = max(most, (uint32_t) __shfl_down(most, d, 64));
  if ((threadIdx.x & 63) == 0 && most) atomicMax((ull*) &meta->counts.n_max_cuts, (ull) most);
  count_to(&meta->counts.n_cut_edges, cut_edges);
  if (blockIdx.x == 0 && threadIdx.x == 0) totals(np, nc, n ? (uint64_t) kidx[n - 1] + keep[n - 1] : 0, flags, capacity, &meta->counts, &meta->emit);
}
// the two scatters and the row: nothing is written unless the output fits
__global__ __launch_bounds__(kThreads) void k_sn_points(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                        const uint32_t* __restrict__ prefix, uint32_t flags, int64_t* __restrict__ out_xy,
                                                        uint32_t* __restrict__ out_row, uint32_t* __restrict__ origin, const Meta* meta) {
  if (meta->bad || !meta->emit) return;
  RJ_GRID_STRIDE(c, nc + 1) out_row[c] = (uint32_t) node::row_slot(c, row, prefix, flags);
  RJ_GRID_STRIDE(p, np) {
    const uint64_t c = node::point_chain(p, row, nc);
    const bool last = p + 1 == row[c + 1];
    if (last && (flags & kDropLast)) continue;
    const uint64_t slot = node::point_slot(p, c, prefix, flags);
    out_xy[2 * slot] = xy[2 * p];
    out_xy[2 * slot + 1] = xy[2 * p + 1];
    if (origin && !last) origin[flags & kDropLast ? slot : slot - c] = (uint32_t) (p - c);
  }
}
__global__ __launch_bounds__(kThreads) void k_sn_cuts(uint64_t n, const Cut* __restrict__ s, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ kidx, const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ row, uint64_t nc, uint32_t flags,
                                                      int64_t* __restrict__ out_xy, uint32_t* __restrict__ origin, const Meta* meta) {
  if (meta->bad || !meta->emit) return;
  RJ_GRID_STRIDE(i, n) {
    if (!keep[i]) continue;
    const Cut cut = s[i];
    const uint32_t e = cut_edge(cut);
    const uint64_t c = crossings::chain_of(e, row, nc), slot = node::cut_slot(kidx[i], e, c, first, prefix, flags);
    out_xy[2 * slot] = cut.qx;
    out_xy[2 * slot + 1] = cut.qy;
    if (origin) origin[flags & kDropLast ? slot : slot - c] = e;
  }
}

struct Events {
  hipEvent_t ev[6] = {};
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) (void) hipEventDestroy(e);
  }
  hipError_t create() {
    for (hipEvent_t& e : ev)
      if (hipError_t r = hipEventCreate(&e)) return r;
    return hipSuccess;
  }
  hipError_t mark(int k, hipStream_t st) { return hipEventRecord(ev[k], st); }
};

}  // namespace

hipError_t map_snap_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec_dev, uint64_t n_rec,
                           uint32_t flags, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Meta* result, SnapReport* report) {
  memset(result, 0, sizeof(Meta));
  for (float& m : report->ms) m = -1.0f;
  const Record* rec = static_cast<const Record*>(rec_dev);
  const uint64_t ne = np - nc, n = 2 * n_rec;  // every candidate a call can have
  Events ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  char* block = nullptr;
  bool done = false;
  do {
    Meta* meta;
    Cut *cand, *sorted;
    uint32_t *keep, *kidx, *first, *cnt, *prefix;
    void* temp;
    TempSize temp_size;
    if (n) {
      temp_size([&](size_t& b) { return rocprim::merge_sort(nullptr, b, (const Cut*) nullptr, (Cut*) nullptr, (size_t) n, CutBefore{}, st); });
      temp_size([&](size_t& b) {
        return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, 0u, (size_t) n, rocprim::plus<uint32_t>(), st);
      });
    }
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, 0u, (size_t) (ne + 1), rocprim::plus<uint32_t>(), st);
    });
    if ((e = temp_size.error) != hipSuccess) break;
    Carve S;
    auto carve = [&]() {
      S.used = 0;
      meta = S.take<Meta>(1);
      cand = S.take<Cut>(n); sorted = S.take<Cut>(n);
      keep = S.take<uint32_t>(n); kidx = S.take<uint32_t>(n);
      first = S.take<uint32_t>(ne); cnt = S.take<uint32_t>(ne + 1); prefix = S.take<uint32_t>(ne + 1);
      temp = S.take<char>(temp_size.bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, S.used)) != hipSuccess) break;
    S.base = block;
    carve();
    // 1. the check
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    const uint64_t widest = 2 * np > n_rec ? (2 * np > nc + 1 ? 2 * np : nc + 1) : n_rec;
    hipLaunchKernelGGL(k_sn_check, dim3(blocks_for(widest, 2048)), dim3(kThreads), 0, st, row, nc, xy, np, rec, n_rec, flags, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the candidates, 3. sorted; the kept cuts numbered
    if (n) {
      if ((e = hipMemsetAsync(cand, 0xFF, sizeof(Cut) * n, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_sn_cands, dim3(blocks_for(n_rec, 2048)), dim3(kThreads), 0, st, row, nc, xy, rec, n_rec, cand, n, meta);
    }
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    if (ne && (e = hipMemsetAsync(first, 0, 4 * ne, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(cnt, 0, 4 * (ne + 1), st)) != hipSuccess) break;
    if (n) {
      size_t tb = temp_size.bytes;
      if ((e = rocprim::merge_sort(temp, tb, (const Cut*) cand, sorted, (size_t) n, CutBefore{}, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_sn_heads, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, keep, (const Meta*) meta);
      tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) keep, kidx, 0u, (size_t) n, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
    }
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the cuts per edge, scanned
    if (n)
      hipLaunchKernelGGL(k_sn_runs, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, (const uint32_t*) keep, (const uint32_t*) kidx,
                         first, cnt, (const Meta*) meta);
    hipLaunchKernelGGL(k_sn_count, dim3(blocks_for(ne + 1, 4096)), dim3(kThreads), 0, st, ne, (const uint32_t*) first, cnt, n, (const uint32_t*) keep,
                       (const uint32_t*) kidx, np, nc, flags, capacity, meta);
    {
      size_t tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) cnt, prefix, 0u, (size_t) (ne + 1), rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
    }
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 5. the two scatters
    hipLaunchKernelGGL(k_sn_points, dim3(blocks_for(np > nc + 1 ? np : nc + 1, 4096)), dim3(kThreads), 0, st, xy, np, row, nc, (const uint32_t*) prefix, flags,
                       out_xy, out_row, origin, (const Meta*) meta);
    if (n)
      hipLaunchKernelGGL(k_sn_cuts, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, (const uint32_t*) keep, (const uint32_t*) kidx,
                         (const uint32_t*) first, (const uint32_t*) prefix, row, nc, flags, out_xy, origin, (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the one sync: the counts, and nothing of this call runs when its scratch goes
    done = e == hipSuccess;
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (done) {
    for (int k = 0; k < 5; k++) (void) hipEventElapsedTime(&report->ms[k], ev.ev[k], ev.ev[k + 1]);
    (void) hipEventElapsedTime(&report->ms[5], ev.ev[0], ev.ev[5]);
  }
  const hipError_t fe = hipFree(block);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
