// rj_polygons.hip -- the polygons of a set of face rings on the device (rj_polygons.h has the definition and the stages).
// Every kernel is a grid-stride loop over one of rj_polygons.h's per-element functions; rocPRIM does the two radix sorts
// (the (face, strip) entries of the ceiling edges, the member keys) and the four scans.  The rounds of the pointer jumping
// are separate launches with a fixed bound: a round that is not needed returns at once, no kernel waits on another
// block, nothing spins on device memory.  The input check's status word, the number of ceiling edges and the strip width
// stay on the device (an input that fails the check is not read further); the host reads one Meta at the end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_pipeline.h"
#include "rj_polygons.h"

namespace rj {

using namespace polygons;

namespace {

constexpr int kTopGroup = 8;  // lanes per ring for its top (as k_rg_place: the rings of an overlay's output map are short)
#ifndef RJ_PG_ABOVE_GROUP
#define RJ_PG_ABOVE_GROUP 8
#endif
constexpr int kAboveGroup = RJ_PG_ABOVE_GROUP;  // lanes per hole over its bucket (8 against a full wave: DESIGN.md has both times)

struct U128Sum {
  __host__ __device__ U128 operator()(const U128& a, const U128& b) const { return rings::add(a, b); }
};

__global__ __launch_bounds__(kThreads) void k_pg_check(const Ring* __restrict__ rings, uint64_t nr, const uint32_t* __restrict__ row,
                                                       const int64_t* __restrict__ xy, uint64_t np, Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nr + 1) bad = max(bad, check_row(c, row, nr, np));
  RJ_GRID_STRIDE(r, nr) bad = max(bad, check_order(r, rings, nr));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, check_coordinate(xy[i]));
  if (bad) atomicMax(&meta->bad, bad);
}
// a group of kTopGroup lanes per ring
__global__ __launch_bounds__(kThreads) void k_pg_tops(uint32_t nr, const Ring* __restrict__ rings, const uint32_t* __restrict__ row,
                                                      const int64_t* __restrict__ xy, Top* __restrict__ top, uint32_t* __restrict__ kind,
                                                      uint32_t* __restrict__ mark, const Meta* meta) {
  if (meta->bad) return;
  const uint32_t lane = threadIdx.x & (kTopGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kTopGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kTopGroup;
  for (uint64_t r = g0; r < nr; r += gstride) {  // (the same trips for all lanes of a group)
    Top t;
    int has = ring_top((uint32_t) r, lane, kTopGroup, row, xy, &t) ? 1 : 0;
    for (int d = kTopGroup / 2; d >= 1; d >>= 1) {
      const int64_t ox = __shfl_xor((long long) t.x, d, kTopGroup), oy = __shfl_xor((long long) t.y, d, kTopGroup);
      const int oh = __shfl_xor(has, d, kTopGroup);
      if (oh && (!has || top_before(t.x, t.y, ox, oy))) t = Top{ox, oy};
      has |= oh;
    }
    if (lane == 0) {
      top[r] = t;
      kind[r] = ring_kind(rings[r]);
      ring_mark((uint32_t) r, row, mark);
    }
  }
}
// per point slot: the ceiling edges counted, their incidences under every shift summed
__global__ __launch_bounds__(kThreads) void k_pg_strips(uint64_t np, const uint32_t* __restrict__ ring_at, const Ring* __restrict__ rings,
                                                        const uint32_t* __restrict__ row, const int64_t* __restrict__ xy, Meta* meta) {
  if (meta->bad) return;
  __shared__ uint64_t part[kThreads / 64][kShifts];
  uint64_t acc[kShifts];
  for (int k = 0; k < kShifts; k++) acc[k] = 0;
  uint32_t edges = 0;
  RJ_GRID_STRIDE(i, np) edges += edge_strips(i, ring_at, rings, row, xy, acc) ? 1u : 0u;
  for (int k = 0; k < kShifts; k++) {
    uint64_t v = acc[k];
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t) __shfl_down((long long) v, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  const uint32_t sum = block_sum(edges);  // (its barrier also publishes part[])
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->n_edges, (unsigned long long) sum);
  if (threadIdx.x < kShifts) {
    uint64_t v = 0;
    for (int w = 0; w < kThreads / 64; w++) v += part[w][threadIdx.x];
    if (v) atomicAdd((unsigned long long*) &meta->incid[threadIdx.x], (unsigned long long) v);
  }
}
__global__ void k_pg_shift(Meta* meta) {
  if (!meta->bad) pick_shift(meta);
}
__global__ __launch_bounds__(kThreads) void k_pg_count(uint64_t np, const uint32_t* __restrict__ ring_at, const Ring* __restrict__ rings,
                                                       const uint32_t* __restrict__ row, const int64_t* __restrict__ xy,
                                                       uint64_t* __restrict__ cnt, const Meta* meta) {
  const bool bad = meta->bad != 0;
  const int shift = (int) meta->shift;
  RJ_GRID_STRIDE(i, np) cnt[i] = bad ? 0 : entry_count(i, ring_at, rings, row, xy, shift);
}
__global__ __launch_bounds__(kThreads) void k_pg_fill(uint64_t np, const uint32_t* __restrict__ ring_at, const Ring* __restrict__ rings,
                                                      const uint32_t* __restrict__ row, const int64_t* __restrict__ xy,
                                                      const uint64_t* __restrict__ off, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                      uint64_t cap, const Meta* meta) {
  if (meta->bad) return;
  const int shift = (int) meta->shift;
  RJ_GRID_STRIDE(i, np) entry_fill(i, ring_at, rings, row, xy, shift, off, keys, vals, cap);
}
// a group of kAboveGroup lanes per ring: a hole's bucket scanned, the lanes' winners reduced, the first state of the jumping
__global__ __launch_bounds__(kThreads) void k_pg_above(uint32_t nr, uint64_t cap, const Ring* __restrict__ rings, const uint32_t* __restrict__ row,
                                                       const int64_t* __restrict__ xy, const Top* __restrict__ top,
                                                       const uint32_t* __restrict__ kind, const uint32_t* __restrict__ ring_at,
                                                       const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, Jump* __restrict__ ja,
                                                       Jump* __restrict__ jb, const Meta* meta) {
  if (meta->bad) return;
  const int shift = (int) meta->shift;
  const uint64_t n_entries = meta->n_entries < cap ? meta->n_entries : cap;
  const uint32_t lane = threadIdx.x & (kAboveGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kAboveGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kAboveGroup;
  for (uint64_t r = g0; r < nr; r += gstride) {  // (the same trips for all lanes of a group)
    const uint32_t k = kind[r];
    uint32_t best = kNone;
    if (k == kKindHole && row[r + 1] > row[r]) {
      const Top p = top[r];
      best = above_scan((uint32_t) r, lane, kAboveGroup, p, rings, ring_at, row, xy, keys, vals, n_entries, shift);
      for (int d = kAboveGroup / 2; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t) __shfl_xor((int) best, d, kAboveGroup);
        best = lower_slot(best, other, p.x, ring_at, row, xy);
      }
    }
    if (lane == 0) jump_init((uint32_t) r, k, best, ring_at, ja, jb);
  }
}
// one round of pointer jumping; a round that is not needed returns at once and leaves its number behind
__global__ __launch_bounds__(kThreads) void k_pg_jump_round(uint32_t nr, const Jump* __restrict__ in, Jump* __restrict__ out, Meta* meta, int r) {
  if (meta->bad) return;
  if (!round_needed(meta->act, r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !meta->jump_done) meta->jump_done = (uint32_t) r;
    return;
  }
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, nr) mine += jump_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&meta->act[r], sum);
}
// behind the last round: every round ran (the final state is in buffer rounds & 1), and the last must have found nothing to do
__global__ void k_pg_rounds_done(Meta* meta, int rounds) {
  if (meta->bad || meta->jump_done) return;
  meta->jump_done = (uint32_t) rounds;
  if (meta->act[rounds - 1]) meta->unfinished = 1;
}
__global__ __launch_bounds__(kThreads) void k_pg_keys(uint32_t nr, const uint32_t* __restrict__ kind, const Jump* __restrict__ j0,
                                                      const Jump* __restrict__ j1, uint32_t* __restrict__ parent, uint64_t* __restrict__ keys,
                                                      Meta* meta) {
  const bool skip = meta->bad || meta->unfinished;
  const Jump* J = (meta->jump_done & 1) ? j1 : j0;
  uint32_t holes = 0, orphans = 0, face0 = 0;
  RJ_GRID_STRIDE(r, nr) {
    if (skip) {
      keys[r] = kNoKey;
      continue;
    }
    int what = 0;
    keys[r] = poly_key((uint32_t) r, kind, J, parent, &what);
    holes += what == 1;
    orphans += what == 2;
    face0 += what == 3;
  }
  uint32_t sum = block_sum(holes);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_holes, (unsigned long long) sum);
  __syncthreads();  // (block_sum's shared words are read by thread 0 until here)
  sum = block_sum(orphans);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_orphans, (unsigned long long) sum);
  __syncthreads();
  sum = block_sum(face0);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_face0, (unsigned long long) sum);
}
__global__ __launch_bounds__(kThreads) void k_pg_mark(uint64_t nr, const uint64_t* __restrict__ skeys, const Ring* __restrict__ rings,
                                                      uint32_t* __restrict__ start, U128* __restrict__ area_at, Meta* meta) {
  RJ_GRID_STRIDE(j, nr + 1) member_mark(j, nr, skeys, rings, start, area_at, meta);
}
__global__ __launch_bounds__(kThreads) void k_pg_place(uint64_t nr, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ start,
                                                       const uint32_t* __restrict__ pid, uint32_t* __restrict__ first, Out o, Meta* meta) {
  RJ_GRID_STRIDE(j, nr + 1) member_place(j, nr, skeys, start, pid, first, o, meta);
}
__global__ __launch_bounds__(kThreads) void k_pg_emit(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ first,
                                                      const U128* __restrict__ xbase, const Ring* __restrict__ rings, Out o, const Meta* meta) {
  const uint64_t n_polygons = meta->counts.n_polygons;  // (<= n_rings: first has n_rings + 1 entries)
  RJ_GRID_STRIDE(p, n_polygons + 1) poly_emit(p, skeys, first, xbase, rings, o, meta);
}

}  // namespace

hipError_t rings_polygons_device(hipStream_t st, const Ring* rings, uint64_t nr64, const uint32_t* row, const int64_t* xy, uint64_t np,
                                 const Out& out, Meta* result) {
  memset(result, 0, sizeof(Meta));
  const Out o = out;
  if (nr64 == 0) {  // no polygons: the CSR's one entry, where the caller has an array
    hipError_t e = hipSuccess;
    if (o.poly_first) e = hipMemsetAsync(o.poly_first, 0, 4, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  }
  const uint32_t nr = (uint32_t) nr64;
  const uint64_t n1 = nr64 + 1, cap = 2 * np, np1 = np ? np : 1, cap1 = cap ? cap : 1;
  int rounds = 1;  // walks of up to 2^(rounds - 1) steps
  while ((1ull << (rounds - 1)) < nr64 && rounds < kMaxRounds) rounds++;
  TempSize temp_size;
  temp_size([&](size_t& b) {
    return rocprim::inclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) np1, rocprim::maximum<uint32_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) np1, rocprim::plus<uint64_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (const uint32_t*) nullptr, (uint32_t*) nullptr,
                                     (size_t) cap1, 0, 64, st);
  });
  temp_size([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) nr, 0, 64, st); });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (uint32_t) 0, (size_t) n1, rocprim::plus<uint32_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const U128*) nullptr, (U128*) nullptr, U128{0, 0}, (size_t) n1, U128Sum(), st);
  });
  if (temp_size.error != hipSuccess) return temp_size.error;
  const size_t temp_bytes = temp_size.bytes;
  // ---- scratch: one allocation, carved (sizes first, then the pointers), freed at the end ----------------------
  Meta* meta;
  Top* top;
  uint32_t *kind, *mark, *ring_at, *evals, *esvals, *start, *pid, *first;
  uint64_t *cnt, *off, *ekeys, *eskeys, *pkeys, *pskeys;
  Jump *j0, *j1;
  U128 *area_at, *xbase;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    meta = A.take<Meta>(1);
    top = A.take<Top>(nr);
    kind = A.take<uint32_t>(nr);
    mark = A.take<uint32_t>(np1); ring_at = A.take<uint32_t>(np1);
    cnt = A.take<uint64_t>(np1); off = A.take<uint64_t>(np1);
    ekeys = A.take<uint64_t>(cap1); eskeys = A.take<uint64_t>(cap1);
    evals = A.take<uint32_t>(cap1); esvals = A.take<uint32_t>(cap1);
    j0 = A.take<Jump>(nr); j1 = A.take<Jump>(nr);
    pkeys = A.take<uint64_t>(nr); pskeys = A.take<uint64_t>(nr);
    start = A.take<uint32_t>(n1); pid = A.take<uint32_t>(n1); first = A.take<uint32_t>(n1);
    area_at = A.take<U128>(n1); xbase = A.take<U128>(n1);
    temp = A.take<char>(temp_bytes);
  };
  carve();
  char* scratch = nullptr;
  hipError_t e = hipMalloc((void**) &scratch, A.used);
  if (e != hipSuccess) return e;
  A.base = scratch;
  carve();
  const int B = blocks_for(nr, 4096), Br = blocks_for(nr, 2048), Bp = blocks_for(np, 2048);
  do {
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(mark, 0, 4 * (size_t) np1, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(ekeys, 0xFF, 8 * (size_t) cap1, st)) != hipSuccess) break;  // (kNoKey: behind the entries when sorted)
    // 0. the check; 1. tops and kinds; 2. the ring of every point slot
    const uint64_t widest = 2 * np > n1 ? 2 * np : n1;
    hipLaunchKernelGGL(k_pg_check, dim3(blocks_for(widest, 2048)), dim3(kThreads), 0, st, rings, nr64, row, xy, np, meta);
    hipLaunchKernelGGL(k_pg_tops, dim3(blocks_for((uint64_t) nr * kTopGroup, 8192)), dim3(kThreads), 0, st, nr, rings, row, xy, top, kind, mark,
                       (const Meta*) meta);
    size_t tb = temp_bytes;
    if ((e = rocprim::inclusive_scan(temp, tb, (const uint32_t*) mark, ring_at, (size_t) np1, rocprim::maximum<uint32_t>(), st)) != hipSuccess) break;
    // 3. the strip width; 4. the entries, sorted
    hipLaunchKernelGGL(k_pg_strips, dim3(Bp), dim3(kThreads), 0, st, np, (const uint32_t*) ring_at, rings, row, xy, meta);
    hipLaunchKernelGGL(k_pg_shift, dim3(1), dim3(1), 0, st, meta);
    hipLaunchKernelGGL(k_pg_count, dim3(Bp), dim3(kThreads), 0, st, np, (const uint32_t*) ring_at, rings, row, xy, cnt, (const Meta*) meta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint64_t*) cnt, off, (uint64_t) 0, (size_t) np1, rocprim::plus<uint64_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_pg_fill, dim3(Bp), dim3(kThreads), 0, st, np, (const uint32_t*) ring_at, rings, row, xy, (const uint64_t*) off, ekeys, evals,
                       cap, (const Meta*) meta);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint64_t*) ekeys, eskeys, (const uint32_t*) evals, esvals, (size_t) cap1, 0, 64, st)) !=
        hipSuccess)
      break;
    // 5. the ring above every hole; 6. parents
    hipLaunchKernelGGL(k_pg_above, dim3(blocks_for((uint64_t) nr * kAboveGroup, 8192)), dim3(kThreads), 0, st, nr, cap, rings, row, xy,
                       (const Top*) top, (const uint32_t*) kind, (const uint32_t*) ring_at, (const uint64_t*) eskeys, (const uint32_t*) esvals, j0, j1,
                       (const Meta*) meta);
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_pg_jump_round, dim3(Br), dim3(kThreads), 0, st, nr, (const Jump*) ((r & 1) ? j1 : j0), (r & 1) ? j0 : j1, meta, r);
    hipLaunchKernelGGL(k_pg_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds);
    if ((e = hipGetLastError()) != hipSuccess) break;
    // 7. polygons
    hipLaunchKernelGGL(k_pg_keys, dim3(Br), dim3(kThreads), 0, st, nr, (const uint32_t*) kind, (const Jump*) j0, (const Jump*) j1, o.parent, pkeys,
                       meta);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_keys(temp, tb, (const uint64_t*) pkeys, pskeys, (size_t) nr, 0, 64, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_pg_mark, dim3(B), dim3(kThreads), 0, st, nr64, (const uint64_t*) pskeys, rings, start, area_at, meta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) start, pid, (uint32_t) 0, (size_t) n1, rocprim::plus<uint32_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_pg_place, dim3(B), dim3(kThreads), 0, st, nr64, (const uint64_t*) pskeys, (const uint32_t*) start, (const uint32_t*) pid,
                       first, o, meta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const U128*) area_at, xbase, U128{0, 0}, (size_t) n1, U128Sum(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_pg_emit, dim3(Br), dim3(kThreads), 0, st, (const uint64_t*) pskeys, (const uint32_t*) first, (const U128*) xbase, rings, o,
                       (const Meta*) meta);
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
