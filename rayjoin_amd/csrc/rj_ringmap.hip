// rj_ringmap.hip -- the chain map of a set of labelled rings on the device (rj_ringmap.h has the definition and the
// stages).  Every kernel is a grid-stride loop over one of rj_ringmap.h's per-element functions; rocPRIM does the two
// merge sorts (the point slots by canonical edge, the odd half-edges by start point), the merge of the even and the odd
// half-edges and the five scans.  The number of unique edges stays on the device: every array is sized by the point
// slots, and the arrays of half-edges end in fillers that sort last.  The rounds of the two pointer-doubling passes are
// separate launches with a fixed bound: a round that is not needed returns at once, no kernel waits on another block,
// nothing spins on device memory.  The input check's status word stays on the device (an input that fails it is not read
// further); the host reads one Meta at the end.  Every half-edge stores its own point into its 16-byte slot: the
// chains are linked lists until the ranking, there is no run of consecutive source points for a lane group to copy.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_pipeline.h"
#include "rj_ringmap.h"

namespace rj {

using namespace ringmap;

namespace {

struct SegBefore {
  const Seg* seg;
  const uint32_t* dir;
  __host__ __device__ bool operator()(const uint32_t& a, const uint32_t& b) const { return seg_before(a, b, seg, dir); }
};
struct HalfBefore {
  const Seg* E;
  __host__ __device__ bool operator()(const uint32_t& a, const uint32_t& b) const { return half_before(a, b, E); }
};
struct SlotsSum {
  __host__ __device__ Slots operator()(const Slots& a, const Slots& b) const { return Slots{a.halves + b.halves, a.points + b.points}; }
};

__global__ __launch_bounds__(kThreads) void k_rm_check(const uint32_t* __restrict__ row, uint64_t nr, const int64_t* __restrict__ xy, uint64_t np,
                                                       Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nr + 1) bad = max(bad, check_row(c, row, nr, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, check_coordinate(xy[i]));
  if (bad) atomicMax(&meta->bad, bad);
}
__global__ __launch_bounds__(kThreads) void k_rm_mark(uint64_t nr, const uint32_t* __restrict__ row, uint32_t* __restrict__ mark, const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(r, nr) ring_mark((uint32_t) r, row, mark);
}
__global__ __launch_bounds__(kThreads) void k_rm_seg(uint64_t n, const uint32_t* __restrict__ ring_at, const uint32_t* __restrict__ row,
                                                     const int64_t* __restrict__ xy, Seg* __restrict__ seg, uint32_t* __restrict__ dir,
                                                     uint32_t* __restrict__ iota, Meta* meta) {
  const bool bad = meta->bad != 0;
  uint32_t zero = 0;
  RJ_GRID_STRIDE(i, n) {
    zero += seg_of(i, bad, ring_at, row, xy, seg, dir) == kZero && !bad ? 1u : 0u;
    iota[i] = (uint32_t) i;
  }
  count_to(&meta->counts.n_zero_edges, zero);
}
__global__ __launch_bounds__(kThreads) void k_rm_head(uint64_t n, const uint32_t* __restrict__ sv, const Seg* __restrict__ seg,
                                                      const uint32_t* __restrict__ dir, uint32_t* __restrict__ head) {
  RJ_GRID_STRIDE(j, n) group_head(j, sv, seg, dir, head);
}
__global__ __launch_bounds__(kThreads) void k_rm_fill(uint64_t n, const uint32_t* __restrict__ sv, const uint32_t* __restrict__ dir,
                                                      const uint32_t* __restrict__ head, const uint32_t* __restrict__ gid,
                                                      const uint32_t* __restrict__ ring_at, const void* __restrict__ face, uint64_t stride,
                                                      uint32_t* __restrict__ ghead, int32_t* __restrict__ gleft, int32_t* __restrict__ gright,
                                                      uint32_t* __restrict__ gconf, Meta* meta) {
  RJ_GRID_STRIDE(j, n) group_fill(j, sv, dir, head, gid, ring_at, face, stride, ghead, gleft, gright, gconf);
  if (blockIdx.x == 0 && threadIdx.x == 0) meta->n_groups = gid[n - 1];
}
__global__ __launch_bounds__(kThreads) void k_rm_keep(uint64_t n, const int32_t* __restrict__ gleft, const int32_t* __restrict__ gright,
                                                      const uint32_t* __restrict__ gconf, uint32_t flags, uint32_t* __restrict__ keep, Meta* meta) {
  const uint64_t n_groups = meta->n_groups;
  uint32_t conflicts = 0, dissolved = 0;
  RJ_GRID_STRIDE(g, n + 1) {
    int what;
    group_keep(g, n_groups, gleft, gright, gconf, flags, keep, &what);
    conflicts += what & 1;
    dissolved += (what >> 1) & 1;
  }
  count_to(&meta->counts.n_conflicts, conflicts);
  count_to(&meta->counts.n_dissolved, dissolved);
}
__global__ __launch_bounds__(kThreads) void k_rm_edges(uint64_t n, const uint32_t* __restrict__ sv, const Seg* __restrict__ seg,
                                                       const uint32_t* __restrict__ ghead, const int32_t* __restrict__ gleft,
                                                       const int32_t* __restrict__ gright, const uint32_t* __restrict__ keep,
                                                       const uint32_t* __restrict__ eidx, Seg* __restrict__ E, int32_t* __restrict__ eleft,
                                                       int32_t* __restrict__ eright, Meta* meta) {
  const uint64_t n_groups = meta->n_groups;
  RJ_GRID_STRIDE(g, n_groups) edge_emit(g, sv, seg, ghead, gleft, gright, keep, eidx, E, eleft, eright);
  if (blockIdx.x == 0 && threadIdx.x == 0) meta->counts.n_edges = eidx[n];
}
__global__ __launch_bounds__(kThreads) void k_rm_seed(uint64_t n, uint32_t* __restrict__ even, uint32_t* __restrict__ odd, const Meta* meta) {
  const uint64_t ne = meta->counts.n_edges;
  RJ_GRID_STRIDE(k, n) half_seed(k, ne, even, odd);
}
__global__ __launch_bounds__(kThreads) void k_rm_pos(const uint32_t* __restrict__ S, uint32_t* __restrict__ pos, const Meta* meta) {
  const uint64_t nh = 2 * meta->counts.n_edges;
  RJ_GRID_STRIDE(k, nh) half_pos(k, S, pos);
}
__global__ __launch_bounds__(kThreads) void k_rm_next(const uint32_t* __restrict__ S, const uint32_t* __restrict__ pos, const Seg* __restrict__ E,
                                                      const int32_t* __restrict__ eleft, const int32_t* __restrict__ eright,
                                                      uint32_t* __restrict__ next, const Meta* meta) {
  const uint64_t nh = 2 * meta->counts.n_edges;
  RJ_GRID_STRIDE(h, nh) next[h] = next_of((uint32_t) h, nh, S, pos, E, eleft, eright);
}
__global__ __launch_bounds__(kThreads) void k_rm_walk_init(const uint32_t* __restrict__ next, Walk* __restrict__ a, Walk* __restrict__ b,
                                                           const Meta* meta) {
  const uint64_t nh = 2 * meta->counts.n_edges;
  RJ_GRID_STRIDE(h, nh) walk_init((uint32_t) h, next, a, b);
}
// one round of pass `pass`; a round that is not needed returns at once and leaves its number behind
__global__ __launch_bounds__(kThreads) void k_rm_walk_round(const Walk* __restrict__ in, Walk* __restrict__ out, Meta* meta, int pass, int r) {
  if (!round_needed(meta->act[pass], r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !meta->done[pass]) meta->done[pass] = (uint32_t) r;
    return;
  }
  const uint64_t nh = 2 * meta->counts.n_edges;
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, nh) mine += walk_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&meta->act[pass][r], sum);
}
// behind the last round: every round ran (the final state is in buffer rounds & 1), and the last must have found nothing to do
__global__ void k_rm_rounds_done(Meta* meta, int rounds, int pass) {
  if (!meta->done[pass]) {
    meta->done[pass] = (uint32_t) rounds;
    if (meta->act[pass][rounds - 1]) meta->unfinished = 1;
  }
}
// (the final buffer of the first pass is read and written in place: every h reads its own entry, then writes it)
__global__ __launch_bounds__(kThreads) void k_rm_cut_init(const uint32_t* __restrict__ next, Walk* w0, Walk* w1, const Meta* meta) {
  const uint64_t nh = 2 * meta->counts.n_edges;
  const Walk* F = (meta->done[0] & 1) ? w1 : w0;
  RJ_GRID_STRIDE(h, nh) cut_init((uint32_t) h, F, next, w0, w1);
}
__global__ __launch_bounds__(kThreads) void k_rm_total(uint64_t n2, const Walk* __restrict__ w0, const Walk* __restrict__ w1,
                                                       const uint32_t* __restrict__ next, Slots* __restrict__ total, Meta* meta) {
  const uint64_t nh = 2 * meta->counts.n_edges;
  const Walk* W = (meta->done[1] & 1) ? w1 : w0;
  uint32_t closed = 0;
  RJ_GRID_STRIDE(h, n2 + 1) closed += chain_total(h, nh, W, next, total) ? 1u : 0u;
  count_to(&meta->counts.n_closed, closed);
}
__global__ __launch_bounds__(kThreads) void k_rm_place(const Walk* __restrict__ w0, const Walk* __restrict__ w1, const Slots* __restrict__ base,
                                                       const Seg* __restrict__ E, const int32_t* __restrict__ eleft,
                                                       const int32_t* __restrict__ eright, Out o, Meta* meta) {
  if (meta->unfinished) return;  // (no slots without a finished ranking)
  const uint64_t nh = 2 * meta->counts.n_edges;
  const Walk* W = (meta->done[1] & 1) ? w1 : w0;
  RJ_GRID_STRIDE(h, nh + 1) chain_place(h, nh, W, base, E, eleft, eright, o, meta);
}

// rings without points: no edge, no chain; the row's one entry where the caller has an array and the input passed its check
__global__ void k_rm_empty(Out o, const Meta* meta) {
  if (!meta->bad && o.row) o.row[0] = 0;
}

}  // namespace

hipError_t rings_map_device(hipStream_t st, const uint32_t* row, const int64_t* xy, uint64_t n, const void* face, uint64_t stride, uint64_t nr,
                            uint32_t flags, const Out& out, Meta* result) {
  memset(result, 0, sizeof(Meta));
  const uint64_t n1 = n + 1, n2 = 2 * n, n21 = 2 * n + 1;
  int rounds = 1;  // walks of up to 2^(rounds - 1) half-edges
  while ((1ull << (rounds - 1)) < n2 && rounds < kMaxRounds) rounds++;
  TempSize temp_size;
  if (n) {
    temp_size([&](size_t& b) {
      return rocprim::merge_sort(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, SegBefore{nullptr, nullptr}, st);
    });
    temp_size([&](size_t& b) {
      return rocprim::merge_sort(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, HalfBefore{nullptr}, st);
    });
    temp_size([&](size_t& b) {
      return rocprim::merge(nullptr, b, (const uint32_t*) nullptr, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, (size_t) n,
                            HalfBefore{nullptr}, st);
    });
    temp_size([&](size_t& b) {
      return rocprim::inclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, rocprim::maximum<uint32_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::inclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, rocprim::plus<uint32_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, 0u, (size_t) n1, rocprim::plus<uint32_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const Slots*) nullptr, (Slots*) nullptr, Slots{0, 0}, (size_t) n21, SlotsSum(), st);
    });
    if (temp_size.error != hipSuccess) return temp_size.error;
  }
  const size_t temp_bytes = temp_size.bytes;
  // ---- scratch: one allocation, carved (sizes first, then the pointers), freed at the end ----------------------
  Meta* meta;
  uint32_t *mark, *ring_at, *dir, *iota, *sv, *head, *gid, *ghead, *gconf, *keep, *eidx, *even, *odd, *sodd, *S, *pos, *next;
  int32_t *gleft, *gright, *eleft, *eright;
  Seg *seg, *E;
  Walk *w0, *w1;
  Slots *total, *base;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    meta = A.take<Meta>(1);
    mark = A.take<uint32_t>(n); ring_at = A.take<uint32_t>(n);
    seg = A.take<Seg>(n); dir = A.take<uint32_t>(n);
    iota = A.take<uint32_t>(n); sv = A.take<uint32_t>(n);
    head = A.take<uint32_t>(n); gid = A.take<uint32_t>(n);
    ghead = A.take<uint32_t>(n); gleft = A.take<int32_t>(n); gright = A.take<int32_t>(n); gconf = A.take<uint32_t>(n);
    keep = A.take<uint32_t>(n1); eidx = A.take<uint32_t>(n1);
    E = A.take<Seg>(n); eleft = A.take<int32_t>(n); eright = A.take<int32_t>(n);
    even = A.take<uint32_t>(n); odd = A.take<uint32_t>(n); sodd = A.take<uint32_t>(n);
    S = A.take<uint32_t>(n2); pos = A.take<uint32_t>(n2); next = A.take<uint32_t>(n2);
    w0 = A.take<Walk>(n2); w1 = A.take<Walk>(n2);
    total = A.take<Slots>(n21); base = A.take<Slots>(n21);
    temp = A.take<char>(temp_bytes);
  };
  carve();
  char* scratch = nullptr;
  hipError_t e = hipMalloc((void**) &scratch, A.used);
  if (e != hipSuccess) return e;
  A.base = scratch;
  carve();
  const int B = blocks_for(n, 4096), B2 = blocks_for(n21, 4096), Br = blocks_for(n2, 2048);
  do {
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_rm_check, dim3(blocks_for(2 * n > nr + 1 ? 2 * n : nr + 1, 2048)), dim3(kThreads), 0, st, row, nr, xy, n, meta);
    if (n == 0) {
      hipLaunchKernelGGL(k_rm_empty, dim3(1), dim3(1), 0, st, out, (const Meta*) meta);
    } else {
      // 1. the ring of every point slot; 2. canonical edges, the first sort
      if ((e = hipMemsetAsync(mark, 0, 4 * (size_t) n, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_rm_mark, dim3(blocks_for(nr, 4096)), dim3(kThreads), 0, st, nr, row, mark, (const Meta*) meta);
      size_t tb = temp_bytes;
      if ((e = rocprim::inclusive_scan(temp, tb, (const uint32_t*) mark, ring_at, (size_t) n, rocprim::maximum<uint32_t>(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_rm_seg, dim3(B), dim3(kThreads), 0, st, n, (const uint32_t*) ring_at, row, xy, seg, dir, iota, meta);
      tb = temp_bytes;
      if ((e = rocprim::merge_sort(temp, tb, (const uint32_t*) iota, sv, (size_t) n, SegBefore{seg, dir}, st)) != hipSuccess) break;
      // 3. unique edges, the kept ones numbered
      hipLaunchKernelGGL(k_rm_head, dim3(B), dim3(kThreads), 0, st, n, (const uint32_t*) sv, (const Seg*) seg, (const uint32_t*) dir, head);
      tb = temp_bytes;
      if ((e = rocprim::inclusive_scan(temp, tb, (const uint32_t*) head, gid, (size_t) n, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
      if ((e = hipMemsetAsync(gleft, 0, 4 * (size_t) n, st)) != hipSuccess) break;
      if ((e = hipMemsetAsync(gright, 0, 4 * (size_t) n, st)) != hipSuccess) break;
      if ((e = hipMemsetAsync(gconf, 0, 4 * (size_t) n, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_rm_fill, dim3(B), dim3(kThreads), 0, st, n, (const uint32_t*) sv, (const uint32_t*) dir, (const uint32_t*) head,
                         (const uint32_t*) gid, (const uint32_t*) ring_at, face, stride, ghead, gleft, gright, gconf, meta);
      hipLaunchKernelGGL(k_rm_keep, dim3(B), dim3(kThreads), 0, st, n, (const int32_t*) gleft, (const int32_t*) gright, (const uint32_t*) gconf,
                         flags, keep, meta);
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) keep, eidx, 0u, (size_t) n1, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_rm_edges, dim3(B), dim3(kThreads), 0, st, n, (const uint32_t*) sv, (const Seg*) seg, (const uint32_t*) ghead,
                         (const int32_t*) gleft, (const int32_t*) gright, (const uint32_t*) keep, (const uint32_t*) eidx, E, eleft, eright, meta);
      // 4. half-edges by start point; 5. next
      hipLaunchKernelGGL(k_rm_seed, dim3(B), dim3(kThreads), 0, st, n, even, odd, (const Meta*) meta);
      tb = temp_bytes;
      if ((e = rocprim::merge_sort(temp, tb, (const uint32_t*) odd, sodd, (size_t) n, HalfBefore{E}, st)) != hipSuccess) break;
      tb = temp_bytes;
      if ((e = rocprim::merge(temp, tb, (const uint32_t*) even, (const uint32_t*) sodd, S, (size_t) n, (size_t) n, HalfBefore{E}, st)) != hipSuccess)
        break;
      hipLaunchKernelGGL(k_rm_pos, dim3(B2), dim3(kThreads), 0, st, (const uint32_t*) S, pos, (const Meta*) meta);
      hipLaunchKernelGGL(k_rm_next, dim3(B2), dim3(kThreads), 0, st, (const uint32_t*) S, (const uint32_t*) pos, (const Seg*) E,
                         (const int32_t*) eleft, (const int32_t*) eright, next, (const Meta*) meta);
      // 6. heads and leaders, then the closed walks opened and ranked
      hipLaunchKernelGGL(k_rm_walk_init, dim3(B2), dim3(kThreads), 0, st, (const uint32_t*) next, w0, w1, (const Meta*) meta);
      for (int r = 0; r < rounds; r++)
        hipLaunchKernelGGL(k_rm_walk_round, dim3(Br), dim3(kThreads), 0, st, (const Walk*) ((r & 1) ? w1 : w0), (r & 1) ? w0 : w1, meta, 0, r);
      hipLaunchKernelGGL(k_rm_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 0);
      hipLaunchKernelGGL(k_rm_cut_init, dim3(B2), dim3(kThreads), 0, st, (const uint32_t*) next, w0, w1, (const Meta*) meta);
      for (int r = 0; r < rounds; r++)
        hipLaunchKernelGGL(k_rm_walk_round, dim3(Br), dim3(kThreads), 0, st, (const Walk*) ((r & 1) ? w1 : w0), (r & 1) ? w0 : w1, meta, 1, r);
      hipLaunchKernelGGL(k_rm_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 1);
      if ((e = hipGetLastError()) != hipSuccess) break;
      // 7. chains: numbers and first points by one scan, then every half-edge to its slot
      hipLaunchKernelGGL(k_rm_total, dim3(B2), dim3(kThreads), 0, st, n2, (const Walk*) w0, (const Walk*) w1, (const uint32_t*) next, total, meta);
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const Slots*) total, base, Slots{0, 0}, (size_t) n21, SlotsSum(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_rm_place, dim3(B2), dim3(kThreads), 0, st, (const Walk*) w0, (const Walk*) w1, (const Slots*) base, (const Seg*) E,
                         (const int32_t*) eleft, (const int32_t*) eright, out, meta);
    }
    if ((e = hipGetLastError()) != hipSuccess) break;
    // the one read-back
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);  // (nothing of this call still runs when its scratch goes)
  const hipError_t fe = hipFree(scratch);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
