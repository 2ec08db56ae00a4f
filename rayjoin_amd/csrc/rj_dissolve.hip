// rj_dissolve.hip -- merging faces by class and re-joining chains on the device (rj_dissolve.h has the definition and the
// stages).  Everything but two passes is over chains, chain sides or half-chains: rocPRIM's merge sort of the 2 nc chain
// ends, its radix sort and sum by key of the 2 nc sides, its scan of the totals, and a grid-stride kernel per function of
// rj_dissolve.h.  The two passes over the points are the check with the chain sums (reads 16 np bytes) and the scatter
// (reads 16 np, writes 16 n_points: the hot path).  Both give a chain to a group of kGroup = 8 lanes: consecutive lanes take
// consecutive points, 16 bytes each, so a group's step is one 128-byte line read and one written, forwards or -- for an
// odd half-chain -- backwards, which is the same line.  A lane per output point with a search for its chain was the
// other shape: it would balance a map of few long chains better, at a dependent binary search per point (the walk
// offsets are per half-chain, not monotone in the input order, so the wave-step trick of rj_eliminate.hip does not
// carry over); maps that come out of an overlay or an eliminate round have millions of chains of 2 .. 12 points, where
// a group of 8 wastes less than a wave and needs no search at all.  A chain of 100 000 points is one group's 12 500
// steps: slow for that chain, correct, and the other groups do not wait for it beyond the kernel's end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <string.h>

#include "rj_dissolve.h"
#include "rj_pipeline.h"

namespace rj {

using namespace dissolve;

namespace {

constexpr int kGroup = 8;  // lanes per chain in the two passes over the points

struct HalfBefore {
  const Pt* start;
  __host__ __device__ bool operator()(const uint32_t& a, const uint32_t& b) const { return half_before(a, b, start); }
};
struct SideSum {
  __host__ __device__ Side operator()(const Side& a, const Side& b) const { return side_add(a, b); }
};
struct SlotsSum {
  __host__ __device__ Slots operator()(const Slots& a, const Slots& b) const { return Slots{a.halves + b.halves, a.points + b.points}; }
};

// 1. the check, the classes, what is kept, the chain sums
__global__ __launch_bounds__(kThreads) void k_ds_chains(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row,
                                                        const int32_t* __restrict__ left, const int32_t* __restrict__ right, uint64_t nc,
                                                        const int32_t* __restrict__ table, uint64_t n_labels, uint32_t flags, int32_t* __restrict__ cl,
                                                        int32_t* __restrict__ cr, U128* __restrict__ S, uint32_t* __restrict__ state, Meta* meta) {
  uint32_t bad = 0, n[4] = {0, 0, 0, 0};  // dropped, kept, skipped; unmapped
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, rings::check_row(c, row, nc, np));
  const uint32_t lane = threadIdx.x & (kGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kGroup;
  for (uint64_t c = g0; c < nc; c += gstride) {  // (the same trips for all lanes of a group)
    i128 sum = 0;
    bool differs = false;
    chain_scan(c, lane, kGroup, xy, row, np, &bad, &sum, &differs);
    U128 s = rings::limbs(sum);
    uint32_t d = differs ? 1u : 0u;
    for (int w = kGroup / 2; w >= 1; w >>= 1) {
      U128 other;
      other.lo = (uint64_t) __shfl_xor((long long) s.lo, w, kGroup);
      other.hi = (uint64_t) __shfl_xor((long long) s.hi, w, kGroup);
      s = rings::add(s, other);
      d |= (uint32_t) __shfl_xor((int) d, w, kGroup);
    }
    if (lane == 0) {
      uint32_t unmapped;
      const uint32_t st = chain_finish(c, left, right, table, n_labels, flags, eliminate::value(s), d != 0, cl, cr, S, state, &unmapped);
      n[0] += st == kDropped;
      n[1] += st == kKept;
      n[2] += st == kSkipped;
      n[3] += unmapped;
    }
  }
  if (bad) atomicMax(&meta->bad, bad);
  count_to(&meta->counts.n_dropped, n[0]);
  count_to(&meta->counts.n_kept, n[1]);
  count_to(&meta->counts.n_skipped, n[2]);
  count_to(&meta->counts.n_unmapped, n[3]);
}

// 2. chain ends by start point, next
__global__ __launch_bounds__(kThreads) void k_ds_seed(const int64_t* __restrict__ xy, const uint32_t* __restrict__ row, uint64_t nh,
                                                      const uint32_t* __restrict__ state, uint32_t* __restrict__ seed, Pt* __restrict__ start,
                                                      const Meta* meta) {
  const bool off = refused(*meta);  // (all fillers: nothing reads the map)
  RJ_GRID_STRIDE(h, nh) {
    if (off)
      seed[h] = kNone;
    else
      half_seed((uint32_t) h, state, xy, row, seed, start);
  }
}
__global__ __launch_bounds__(kThreads) void k_ds_pos(const uint32_t* __restrict__ order, uint32_t* __restrict__ pos, const Meta* meta) {
  if (refused(*meta)) return;
  RJ_GRID_STRIDE(k, 2 * meta->counts.n_kept) half_pos(k, order, pos);
}
__global__ __launch_bounds__(kThreads) void k_ds_next(uint64_t nh, const uint32_t* __restrict__ state, const uint32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ pos, const Pt* __restrict__ start, const int32_t* __restrict__ cl,
                                                      const int32_t* __restrict__ cr, uint32_t* __restrict__ next, const Meta* meta) {
  if (refused(*meta)) return;
  const uint64_t kept = 2 * meta->counts.n_kept;
  RJ_GRID_STRIDE(h, nh) next[h] = state[h >> 1] == kKept ? next_of((uint32_t) h, kept, order, pos, start, cl, cr) : kNone;
}

// 3. the walks
__global__ __launch_bounds__(kThreads) void k_ds_walk_init(uint64_t nh, const uint32_t* __restrict__ next, const uint32_t* __restrict__ row,
                                                           Walk* __restrict__ a, Walk* __restrict__ b, const Meta* meta) {
  if (refused(*meta)) return;
  RJ_GRID_STRIDE(h, nh) walk_init((uint32_t) h, next, row, a, b);
}
// one round of pass `pass`; a round that is not needed returns at once and leaves its number behind
__global__ __launch_bounds__(kThreads) void k_ds_walk_round(uint64_t nh, const Walk* __restrict__ in, Walk* __restrict__ out, Meta* meta, int pass, int r) {
  if (refused(*meta)) return;
  if (!ringmap::round_needed(meta->act[pass], r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !meta->done[pass]) meta->done[pass] = (uint32_t) r;
    return;
  }
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, nh) mine += ringmap::walk_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&meta->act[pass][r], sum);
}
// behind the last round: every round ran (the final state is in buffer rounds & 1), and the last must have found nothing to do
__global__ void k_ds_rounds_done(Meta* meta, int rounds, int pass) {
  if (refused(*meta)) return;
  if (!meta->done[pass]) {
    meta->done[pass] = (uint32_t) rounds;
    if (meta->act[pass][rounds - 1]) meta->unfinished = 1;
  }
}
// (the final buffer of the first pass is read and written in place: every h reads its own entry, then writes it)
__global__ __launch_bounds__(kThreads) void k_ds_cut_init(uint64_t nh, const uint32_t* __restrict__ next, const uint32_t* __restrict__ row, Walk* w0,
                                                          Walk* w1, const Meta* meta) {
  if (refused(*meta)) return;
  const Walk* F = (meta->done[0] & 1) ? w1 : w0;
  RJ_GRID_STRIDE(h, nh) cut_init((uint32_t) h, F, next, row, w0, w1);
}

// 4. the class records
__global__ __launch_bounds__(kThreads) void k_ds_sides(uint64_t nh, const uint32_t* __restrict__ state, const int32_t* __restrict__ cl,
                                                       const int32_t* __restrict__ cr, const U128* __restrict__ S, uint32_t* __restrict__ keys,
                                                       Side* __restrict__ vals, const Meta* meta) {
  const bool off = refused(*meta);
  RJ_GRID_STRIDE(i, nh) {
    keys[i] = off ? kZeroKey : side_key(i, state, cl, cr);
    vals[i] = off ? Side{U128{0, 0}, 0} : side_val(i, S);
  }
}

// 5. totals, the scan, the scatter
__global__ __launch_bounds__(kThreads) void k_ds_total(uint64_t nh, const uint32_t* __restrict__ state, const Walk* __restrict__ w0,
                                                       const Walk* __restrict__ w1, const uint32_t* __restrict__ next, const uint32_t* __restrict__ row,
                                                       Slots* __restrict__ total, Meta* meta) {
  const bool off = refused(*meta) || meta->unfinished;
  const Walk* W = (meta->done[1] & 1) ? w1 : w0;
  uint32_t closed = 0;
  RJ_GRID_STRIDE(h, nh + 1) {
    if (off)
      total[h] = Slots{0, 0};
    else
      closed += chain_total(h, nh, state, W, next, row, total) ? 1u : 0u;
  }
  count_to(&meta->counts.n_closed, closed);
}
__global__ void k_ds_counts(uint64_t nh, const Slots* __restrict__ base, const uint32_t* __restrict__ keys, Out o, Meta* meta) {
  if (refused(*meta) || meta->unfinished) return;
  meta->counts.n_chains = base[nh].halves;
  meta->counts.n_points = base[nh].points;
  meta->counts.n_classes = eliminate::count_faces(meta->n_keys, keys);
  meta->emit = fits(meta->counts, o) ? 1 : 0;
  // (a map that keeps no chain fits capacities of 0, the sizing call's, whose arrays may be null)
  if (meta->emit && o.row) o.row[meta->counts.n_chains] = (uint32_t) meta->counts.n_points;
}
__global__ __launch_bounds__(kThreads) void k_ds_place(const int64_t* __restrict__ xy, const uint32_t* __restrict__ row, uint64_t nc,
                                                       const uint32_t* __restrict__ state, const int32_t* __restrict__ cl, const int32_t* __restrict__ cr,
                                                       const Walk* __restrict__ w0, const Walk* __restrict__ w1, const Slots* __restrict__ base,
                                                       const uint32_t* __restrict__ keys, const Side* __restrict__ sums, Out o, const Meta* meta) {
  if (!meta->emit) return;
  const Walk* W = (meta->done[1] & 1) ? w1 : w0;
  if (o.classes) RJ_GRID_STRIDE(k, meta->counts.n_classes) o.classes[k] = record_of(k, keys, sums);
  const uint32_t lane = threadIdx.x & (kGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kGroup;
  for (uint64_t c = g0; c < nc; c += gstride) chain_place(c, lane, kGroup, xy, row, state, cl, cr, W, base, o);
}

}  // namespace

hipError_t map_dissolve_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                               const int32_t* class_table, uint64_t n_labels, uint32_t flags, const Out& out, int point_blocks, Meta* result,
                               DissolveReport* report) {
  memset(result, 0, sizeof(Meta));
  *report = DissolveReport{};
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  const uint64_t nh = 2 * nc, nh1 = nh + 1;  // half-chains, chain sides
  int rounds = 1;                            // walks of up to 2^(rounds - 1) half-chains
  while ((1ull << (rounds - 1)) < nh && rounds < kMaxRounds) rounds++;
  char* block = nullptr;
  bool done = false;
  do {
    Meta* meta;
    U128* S;
    int32_t *cl, *cr;
    uint32_t *state, *seed, *order, *pos, *next, *key_in, *key_out, *keys;
    Pt* start;
    Walk *w0, *w1;
    Slots *total, *base;
    Side *val_in, *val_out, *sums;
    void* temp;
    TempSize temp_size;
    temp_size([&](size_t& b) {
      return rocprim::merge_sort(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) nh, HalfBefore{nullptr}, st);
    });
    temp_size([&](size_t& b) {
      return rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (const Side*) nullptr, (Side*) nullptr, (size_t) nh, 0, 32,
                                       st);
    });
    temp_size([&](size_t& b) {
      return rocprim::reduce_by_key(nullptr, b, (const uint32_t*) nullptr, (const Side*) nullptr, (size_t) nh, (uint32_t*) nullptr, (Side*) nullptr,
                                    (uint64_t*) nullptr, SideSum(), rocprim::equal_to<uint32_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const Slots*) nullptr, (Slots*) nullptr, Slots{0, 0}, (size_t) nh1, SlotsSum(), st);
    });
    if ((e = temp_size.error) != hipSuccess) break;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<Meta>(1);
      S = A.take<U128>(nc); cl = A.take<int32_t>(nc); cr = A.take<int32_t>(nc); state = A.take<uint32_t>(nc);
      start = A.take<Pt>(nh); seed = A.take<uint32_t>(nh); order = A.take<uint32_t>(nh); pos = A.take<uint32_t>(nh); next = A.take<uint32_t>(nh);
      w0 = A.take<Walk>(nh); w1 = A.take<Walk>(nh);
      total = A.take<Slots>(nh1); base = A.take<Slots>(nh1);
      key_in = A.take<uint32_t>(nh); key_out = A.take<uint32_t>(nh); keys = A.take<uint32_t>(nh);
      val_in = A.take<Side>(nh); val_out = A.take<Side>(nh); sums = A.take<Side>(nh);
      temp = A.take<char>(temp_size.bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    const int half_blocks = blocks_for(nh1, 4096), round_blocks = blocks_for(nh, 2048), group_blocks = blocks_for(nc * kGroup, 16384);
    size_t tb;
    // 1. the check, the classes, what is kept, the chain sums
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_ds_chains, dim3(group_blocks), dim3(kThreads), 0, st, xy, np, row, left, right, nc, class_table, n_labels, flags, cl, cr, S, state, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the chain ends sorted by start point, next
    hipLaunchKernelGGL(k_ds_seed, dim3(half_blocks), dim3(kThreads), 0, st, xy, row, nh, (const uint32_t*) state, seed, start, (const Meta*) meta);
    tb = temp_size.bytes;
    if ((e = rocprim::merge_sort(temp, tb, (const uint32_t*) seed, order, (size_t) nh, HalfBefore{start}, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_ds_pos, dim3(half_blocks), dim3(kThreads), 0, st, (const uint32_t*) order, pos, (const Meta*) meta);
    hipLaunchKernelGGL(k_ds_next, dim3(half_blocks), dim3(kThreads), 0, st, nh, (const uint32_t*) state, (const uint32_t*) order, (const uint32_t*) pos,
                       (const Pt*) start, (const int32_t*) cl, (const int32_t*) cr, next, (const Meta*) meta);
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    // 3. heads and leaders, then the closed walks opened and ranked
    hipLaunchKernelGGL(k_ds_walk_init, dim3(half_blocks), dim3(kThreads), 0, st, nh, (const uint32_t*) next, row, w0, w1, (const Meta*) meta);
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_ds_walk_round, dim3(round_blocks), dim3(kThreads), 0, st, nh, (const Walk*) ((r & 1) ? w1 : w0), (r & 1) ? w0 : w1, meta, 0, r);
    hipLaunchKernelGGL(k_ds_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 0);
    hipLaunchKernelGGL(k_ds_cut_init, dim3(half_blocks), dim3(kThreads), 0, st, nh, (const uint32_t*) next, row, w0, w1, (const Meta*) meta);
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_ds_walk_round, dim3(round_blocks), dim3(kThreads), 0, st, nh, (const Walk*) ((r & 1) ? w1 : w0), (r & 1) ? w0 : w1, meta, 1, r);
    hipLaunchKernelGGL(k_ds_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 1);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the class records: the kept sides by class, their sums
    hipLaunchKernelGGL(k_ds_sides, dim3(half_blocks), dim3(kThreads), 0, st, nh, (const uint32_t*) state, (const int32_t*) cl, (const int32_t*) cr,
                       (const U128*) S, key_in, val_in, (const Meta*) meta);
    tb = temp_size.bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t*) key_in, key_out, (const Side*) val_in, val_out, (size_t) nh, 0, 32, st)) != hipSuccess) break;
    tb = temp_size.bytes;
    if ((e = rocprim::reduce_by_key(temp, tb, (const uint32_t*) key_out, (const Side*) val_out, (size_t) nh, keys, sums, &meta->n_keys, SideSum(),
                                    rocprim::equal_to<uint32_t>(), st)) != hipSuccess)
      break;
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 5. chain numbers and first points by one scan, then every kept chain to its slots
    hipLaunchKernelGGL(k_ds_total, dim3(half_blocks), dim3(kThreads), 0, st, nh, (const uint32_t*) state, (const Walk*) w0, (const Walk*) w1,
                       (const uint32_t*) next, row, total, meta);
    tb = temp_size.bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const Slots*) total, base, Slots{0, 0}, (size_t) nh1, SlotsSum(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_ds_counts, dim3(1), dim3(1), 0, st, nh, (const Slots*) base, (const uint32_t*) keys, out, meta);
    hipLaunchKernelGGL(k_ds_place, dim3(point_blocks > 0 ? point_blocks : group_blocks), dim3(kThreads), 0, st, xy, row, nc, (const uint32_t*) state,
                       (const int32_t*) cl, (const int32_t*) cr, (const Walk*) w0, (const Walk*) w1, (const Slots*) base, (const uint32_t*) keys,
                       (const Side*) sums, out, (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the one sync: the counts, and nothing of this call runs when its scratch goes
    done = e == hipSuccess;
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (done && !refused(*result)) ev.times(5, report->ms);
  const hipError_t fe = hipFree(block);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
