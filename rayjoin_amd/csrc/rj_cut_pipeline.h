// rj_cut_pipeline.h -- the pipeline that rj_map_node and rj_map_snap share (rj_node.h and rj_snap.h have the definitions
// and the stages): the input check, the candidates, their merge sort and the kept cuts, the cuts per edge and their
// scan, the two scatters.  Every kernel is a grid-stride loop over per-element functions of rj_node.h or of the
// policy; rocPRIM does the merge sort and the two scans.  The candidate array has the 2 n_rec slots a call can fill,
// the unused ones hold all ones and sort to the end, so that no size has to be read back: the stream is synchronised
// once, at the end, for the counts.  The cuts of an edge are neighbours behind the sort: their number and every cut's
// rank are differences of scanned flags, and both scatters -- one thread per input point, one per kept cut -- are
// fully parallel.
//
// A policy P is a type of rj_node.hip or rj_snap.hip; what the two calls do not share comes from it:
//   Cut, Meta, Before          the candidate, what the stages leave for each other (bad, emit, n_cand, counts) and the
//                              sort's order
//   head, run_first, run_last  the per-element functions of the sorted cuts
//   edge, point                a cut's edge and its point (from the input points or from the cut itself)
//   totals                     the counts behind the scans
//   launch_cands               the launch of the candidates kernel, which is the policy's own
// HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <string.h>

#include "rj_node.h"
#include "rj_pipeline.h"

namespace rj {
namespace cut {

template <class P>
__global__ __launch_bounds__(kThreads) void k_check(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy, uint64_t np,
                                                    const node::Record* __restrict__ rec, uint64_t n_rec, uint32_t flags, typename P::Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, crossings::check_row(c, row, nc, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, crossings::check_coordinate(xy[i]));
  if (flags & node::kDropLast) RJ_GRID_STRIDE(c, nc) bad = max(bad, node::check_chain(c, row, np, xy));
  RJ_GRID_STRIDE(r, n_rec) bad = max(bad, node::check_record(r, rec, np - nc, row, nc, xy));
  if (bad) atomicMax(&meta->bad, bad);
}
template <class P>
__global__ __launch_bounds__(kThreads) void k_heads(uint64_t n, const typename P::Cut* __restrict__ s, uint32_t* __restrict__ keep,
                                                    const typename P::Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, n) keep[i] = P::head(i, s) ? 1u : 0u;
}
// first[e], last[e]: the numbers of the kept cuts of e (zeroed before: edges without a cut keep 0, 0)
template <class P>
__global__ __launch_bounds__(kThreads) void k_runs(uint64_t n, const typename P::Cut* __restrict__ s, const uint32_t* __restrict__ keep,
                                                   const uint32_t* __restrict__ kidx, uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                   const typename P::Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, n) {
    const uint32_t e = P::edge(s[i]);
    if (e == node::kNoEdge) continue;
    if (P::run_first(i, s)) first[e] = kidx[i];
    if (P::run_last(i, n, s)) last[e] = kidx[i] + keep[i];
  }
}
// cnt[e] = last[e] - first[e] in place of last[e], entry ne closes the scan; the counts that need no scan
template <class P>
__global__ __launch_bounds__(kThreads) void k_count(uint64_t ne, const uint32_t* __restrict__ first, uint32_t* __restrict__ cnt, uint64_t n,
                                                    const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kidx, uint64_t np, uint64_t nc,
                                                    uint32_t flags, uint64_t capacity, typename P::Meta* meta) {
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
  if (blockIdx.x == 0 && threadIdx.x == 0) P::totals(np, nc, n ? (uint64_t) kidx[n - 1] + keep[n - 1] : 0, flags, capacity, &meta->counts, &meta->emit);
}
// the two scatters and the row: nothing is written unless the output fits
template <class P>
__global__ __launch_bounds__(kThreads) void k_points(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                     const uint32_t* __restrict__ prefix, uint32_t flags, int64_t* __restrict__ out_xy,
                                                     uint32_t* __restrict__ out_row, uint32_t* __restrict__ origin, const typename P::Meta* meta) {
  if (meta->bad || !meta->emit) return;
  RJ_GRID_STRIDE(c, nc + 1) out_row[c] = (uint32_t) node::row_slot(c, row, prefix, flags);
  RJ_GRID_STRIDE(p, np) {
    const uint64_t c = node::point_chain(p, row, nc);
    const bool last = p + 1 == row[c + 1];
    if (last && (flags & node::kDropLast)) continue;
    const uint64_t slot = node::point_slot(p, c, prefix, flags);
    out_xy[2 * slot] = xy[2 * p];
    out_xy[2 * slot + 1] = xy[2 * p + 1];
    if (origin && !last) origin[flags & node::kDropLast ? slot : slot - c] = (uint32_t) (p - c);
  }
}
template <class P>
__global__ __launch_bounds__(kThreads) void k_cuts(uint64_t n, const typename P::Cut* __restrict__ s, const uint32_t* __restrict__ keep,
                                                   const uint32_t* __restrict__ kidx, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ prefix, const int64_t* __restrict__ xy, const uint32_t* __restrict__ row,
                                                   uint64_t nc, uint32_t flags, int64_t* __restrict__ out_xy, uint32_t* __restrict__ origin,
                                                   const typename P::Meta* meta) {
  if (meta->bad || !meta->emit) return;
  RJ_GRID_STRIDE(i, n) {
    if (!keep[i]) continue;
    const typename P::Cut cut = s[i];
    const uint32_t e = P::edge(cut);
    const uint64_t c = crossings::chain_of(e, row, nc), slot = node::cut_slot(kidx[i], e, c, first, prefix, flags);
    P::point(cut, xy, out_xy + 2 * slot);
    if (origin) origin[flags & node::kDropLast ? slot : slot - c] = e;
  }
}

// rj_map_node / rj_map_snap behind their argument checks, on stream st: *result = the device's Meta, *times = what the
// stages took.  Allocates and frees its scratch; synchronises the stream once, at the end.
template <class P>
hipError_t run(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, const void* rec_dev, uint64_t n_rec, uint32_t flags,
               uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, typename P::Meta* result, StageMs* times) {
  using Cut = typename P::Cut;
  using Meta = typename P::Meta;
  using Before = typename P::Before;
  memset(result, 0, sizeof(Meta));
  *times = StageMs{};
  const node::Record* rec = static_cast<const node::Record*>(rec_dev);
  const uint64_t ne = np - nc, n = 2 * n_rec;  // every candidate a call can have
  StageEvents ev;
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
      temp_size([&](size_t& b) { return rocprim::merge_sort(nullptr, b, (const Cut*) nullptr, (Cut*) nullptr, (size_t) n, Before{}, st); });
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
    hipLaunchKernelGGL(k_check<P>, dim3(blocks_for(widest, 2048)), dim3(kThreads), 0, st, row, nc, xy, np, rec, n_rec, flags, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the candidates, 3. sorted; the kept cuts numbered
    if (n) {
      if ((e = hipMemsetAsync(cand, 0xFF, sizeof(Cut) * n, st)) != hipSuccess) break;
      P::launch_cands(blocks_for(n_rec, 2048), st, row, nc, xy, rec, n_rec, cand, n, meta);
    }
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    if (ne && (e = hipMemsetAsync(first, 0, 4 * ne, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(cnt, 0, 4 * (ne + 1), st)) != hipSuccess) break;
    if (n) {
      size_t tb = temp_size.bytes;
      if ((e = rocprim::merge_sort(temp, tb, (const Cut*) cand, sorted, (size_t) n, Before{}, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_heads<P>, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, keep, (const Meta*) meta);
      tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) keep, kidx, 0u, (size_t) n, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
    }
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the cuts per edge, scanned
    if (n)
      hipLaunchKernelGGL(k_runs<P>, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, (const uint32_t*) keep, (const uint32_t*) kidx,
                         first, cnt, (const Meta*) meta);
    hipLaunchKernelGGL(k_count<P>, dim3(blocks_for(ne + 1, 4096)), dim3(kThreads), 0, st, ne, (const uint32_t*) first, cnt, n, (const uint32_t*) keep,
                       (const uint32_t*) kidx, np, nc, flags, capacity, meta);
    {
      size_t tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) cnt, prefix, 0u, (size_t) (ne + 1), rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
    }
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 5. the two scatters
    hipLaunchKernelGGL(k_points<P>, dim3(blocks_for(np > nc + 1 ? np : nc + 1, 4096)), dim3(kThreads), 0, st, xy, np, row, nc, (const uint32_t*) prefix, flags,
                       out_xy, out_row, origin, (const Meta*) meta);
    if (n)
      hipLaunchKernelGGL(k_cuts<P>, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, n, (const Cut*) sorted, (const uint32_t*) keep, (const uint32_t*) kidx,
                         (const uint32_t*) first, (const uint32_t*) prefix, xy, row, nc, flags, out_xy, origin, (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the one sync: the counts, and nothing of this call runs when its scratch goes
    done = e == hipSuccess;
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (done) ev.times(5, times->ms);
  const hipError_t fe = hipFree(block);
  return e != hipSuccess ? e : fe;
}

}  // namespace cut
}  // namespace rj
