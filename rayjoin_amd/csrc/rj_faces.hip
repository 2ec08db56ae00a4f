// rj_faces.hip -- the faces of a chain map from its geometry, on the device (rj_faces.h has the definition and the stages).
// The ring stages of rj_rings.hip run first, without labels and without points, in this call's scratch; every kernel here
// is a grid-stride loop over one of rj_faces.h's per-element functions (or rj_polygons.h's, for the jumping and the
// members); rocPRIM does the two radix sorts (the registrations by cell, the member keys) and the five scans.  The grid's
// shift is chosen on the device, the registration slots are sized by their bound: nothing is read back before the end.
// The rounds of the pointer jumping are separate launches with a fixed bound; no kernel waits on another block.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_faces.h"
#include "rj_pipeline.h"

namespace rj {

using namespace faces;

namespace {

constexpr int kTopGroup = 8;    // lanes per chain for its top (as k_pg_tops)
#ifndef RJ_FC_RAY_GROUP
#define RJ_FC_RAY_GROUP 8
#endif
constexpr int kRayGroup = RJ_FC_RAY_GROUP;  // lanes per hole over a cell's run: a run holds a few edges at the default shift

struct U128Sum {
  __host__ __device__ U128 operator()(const U128& a, const U128& b) const { return rings::add(a, b); }
};
struct SegMax {
  __host__ __device__ SegTop operator()(const SegTop& a, const SegTop& b) const { return seg_max(a, b); }
};

__device__ __forceinline__ bool skip(const rings::Meta* rmeta) { return rmeta->bad_map || rmeta->unfinished; }

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t) __shfl_down((long long) v, d, 64);
  return v;
}

// a group of kTopGroup lanes per chain; the last point of every chain marked
__global__ __launch_bounds__(kThreads) void k_fc_tops(uint64_t nc, const uint32_t* __restrict__ row, const int64_t* __restrict__ xy,
                                                      Top* __restrict__ chain_top, uint8_t* __restrict__ islast, const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  const uint32_t lane = threadIdx.x & (kTopGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kTopGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kTopGroup;
  for (uint64_t c = g0; c < nc; c += gstride) {  // (the same trips for all lanes of a group)
    Top t;
    int has = polygons::ring_top((uint32_t) c, lane, kTopGroup, row, xy, &t) ? 1 : 0;
    for (int d = kTopGroup / 2; d >= 1; d >>= 1) {
      const int64_t ox = __shfl_xor((long long) t.x, d, kTopGroup), oy = __shfl_xor((long long) t.y, d, kTopGroup);
      const int oh = __shfl_xor(has, d, kTopGroup);
      if (oh && (!has || polygons::top_before(t.x, t.y, ox, oy))) t = Top{ox, oy};
      has |= oh;
    }
    if (lane == 0) {
      chain_top[c] = t;
      last_mark(c, row, islast);
    }
  }
}
__global__ __launch_bounds__(kThreads) void k_fc_slots(const uint32_t* __restrict__ ring_first, const uint32_t* __restrict__ ring_half,
                                                       const Top* __restrict__ chain_top, uint32_t* __restrict__ ring_of_half,
                                                       SegTop* __restrict__ seg, const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  const uint64_t n_rings = rmeta->counts.n_rings, n_halves = rmeta->counts.n_halves;
  RJ_GRID_STRIDE(s, n_halves) slot_seg(s, ring_first, ring_half, n_rings, chain_top, ring_of_half, seg);
}
__global__ __launch_bounds__(kThreads) void k_fc_kinds(const Ring* __restrict__ rings, uint32_t* __restrict__ kind, const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  RJ_GRID_STRIDE(r, rmeta->counts.n_rings) kind[r] = ring_kind(rings[r]);
}
// per point: the ceiling edges counted, their extents and their registrations under every shift summed
__global__ __launch_bounds__(kThreads) void k_fc_scan(uint64_t np, const uint8_t* __restrict__ islast, const int64_t* __restrict__ xy, Meta* meta,
                                                      const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  __shared__ uint64_t part[kThreads / 64][kShifts + 2];
  uint64_t acc[kShifts], ext_lo = 0, ext_hi = 0;
  for (int k = 0; k < kShifts; k++) acc[k] = 0;
  uint32_t edges = 0;
  RJ_GRID_STRIDE(i, np) edges += edge_scan(i, islast, xy, acc, &ext_lo, &ext_hi) ? 1u : 0u;
  for (int k = 0; k < kShifts + 2; k++) {
    uint64_t v = k < kShifts ? acc[k] : (k == kShifts ? ext_lo : ext_hi);
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t o = (uint64_t) __shfl_down((long long) v, d, 64);
      v = k < kShifts ? clamp_add(v, o) : v + o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  const uint32_t sum = block_sum(edges);  // (its barrier also publishes part[])
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->n_ceil, (unsigned long long) sum);
  if (threadIdx.x < kShifts + 2) {
    const int k = (int) threadIdx.x;
    uint64_t v = 0;
    for (int w = 0; w < kThreads / 64; w++) v = k < kShifts ? clamp_add(v, part[w][k]) : v + part[w][k];
    uint64_t* to = k < kShifts ? &meta->regs[k] : (k == kShifts ? &meta->extent_lo : &meta->extent_hi);
    if (v) atomicAdd((unsigned long long*) to, (unsigned long long) v);  // (at most 2048 blocks of at most 2^37 each)
  }
}
__global__ void k_fc_shift(Meta* meta, int forced, const rings::Meta* rmeta) {
  if (!skip(rmeta)) pick_shift(meta, forced);
}
__global__ __launch_bounds__(kThreads) void k_fc_count(uint64_t np, const uint8_t* __restrict__ islast, const int64_t* __restrict__ xy,
                                                       uint64_t* __restrict__ cnt, const Meta* meta, const rings::Meta* rmeta) {
  const bool off = skip(rmeta);
  const int shift = (int) meta->shift;
  RJ_GRID_STRIDE(i, np + 1) cnt[i] = off || i == np ? 0 : reg_count_at(i, islast, xy, shift);
}
__global__ __launch_bounds__(kThreads) void k_fc_fill(uint64_t np, const int64_t* __restrict__ xy, const uint64_t* __restrict__ off,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint64_t cap, const Meta* meta,
                                                      const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  const int shift = (int) meta->shift;
  const uint64_t n = meta->n_regs < cap ? meta->n_regs : cap;  // (n_regs <= cap: pick_shift's bound)
  RJ_GRID_STRIDE(r, n) reg_at(r, off, np, xy, shift, &keys[r], &vals[r]);
}
struct GroupLower {
  int64_t px;
  const int64_t* xy;
  __device__ uint32_t operator()(uint32_t best) const {
    for (int d = kRayGroup / 2; d >= 1; d >>= 1) {
      const uint32_t other = (uint32_t) __shfl_xor((int) best, d, kRayGroup);
      best = lower_pt(best, other, px, xy);
    }
    return best;
  }
};
// a group of kRayGroup lanes per ring: a hole's ray walked up its column, the first state of the jumping
__global__ __launch_bounds__(kThreads) void k_fc_above(uint64_t cap, uint64_t nc, const uint32_t* __restrict__ row, const int64_t* __restrict__ xy,
                                                       const uint32_t* __restrict__ ring_first, const SegTop* __restrict__ segs,
                                                       const uint32_t* __restrict__ kind, const uint32_t* __restrict__ ring_of_half,
                                                       const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, Jump* __restrict__ ja,
                                                       Jump* __restrict__ jb, Meta* meta, const rings::Meta* rmeta) {
  if (skip(rmeta)) return;
  const int shift = (int) meta->shift;
  const uint64_t n = meta->n_regs < cap ? meta->n_regs : cap, nr = rmeta->counts.n_rings;
  const uint32_t lane = threadIdx.x & (kRayGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kRayGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kRayGroup;
  uint64_t tests = 0, cells = 0;
  for (uint64_t r = g0; r < nr; r += gstride) {  // (the same trips for all lanes of a group)
    const uint32_t k = kind[r];
    uint32_t best = kNone;
    if (k == polygons::kKindHole) {
      const Top p = segs[ring_first[r + 1] - 1].top;
      best = ray_walk(lane, kRayGroup, p, keys, vals, n, xy, shift, GroupLower{p.x, xy}, &tests, &cells);
    }
    if (lane == 0) above_init((uint32_t) r, k, best, row, nc, xy, ring_of_half, ja, jb);
  }
  if (lane != 0) tests = cells = 0;  // (every lane of a group counted the same)
  tests = wave_sum64(tests);
  cells = wave_sum64(cells);
  if ((threadIdx.x & 63) == 0) {
    if (tests) atomicAdd((unsigned long long*) &meta->ray_tests, (unsigned long long) tests);
    if (cells) atomicAdd((unsigned long long*) &meta->cells, (unsigned long long) cells);
  }
}
// one round of pointer jumping; a round that is not needed returns at once and leaves its number behind
__global__ __launch_bounds__(kThreads) void k_fc_jump_round(const Jump* __restrict__ in, Jump* __restrict__ out, polygons::Meta* pmeta,
                                                            const rings::Meta* rmeta, int r) {
  if (skip(rmeta)) return;
  if (!polygons::round_needed(pmeta->act, r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !pmeta->jump_done) pmeta->jump_done = (uint32_t) r;
    return;
  }
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, rmeta->counts.n_rings) mine += polygons::jump_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&pmeta->act[r], sum);
}
__global__ void k_fc_rounds_done(polygons::Meta* pmeta, const rings::Meta* rmeta, int rounds) {
  if (skip(rmeta) || pmeta->jump_done) return;
  pmeta->jump_done = (uint32_t) rounds;
  if (pmeta->act[rounds - 1]) pmeta->unfinished = 1;
}
// ni keys: those behind the rings are kNoKey
__global__ __launch_bounds__(kThreads) void k_fc_keys(uint32_t ni, const uint32_t* __restrict__ kind, const Jump* __restrict__ j0,
                                                      const Jump* __restrict__ j1, uint64_t* __restrict__ keys, polygons::Meta* pmeta, Meta* meta,
                                                      const rings::Meta* rmeta) {
  const bool off = skip(rmeta) || pmeta->unfinished;
  const Jump* J = (pmeta->jump_done & 1) ? j1 : j0;
  const uint64_t nr = off ? 0 : rmeta->counts.n_rings;
  uint32_t holes = 0, outer = 0;
  RJ_GRID_STRIDE(r, ni) {
    if (r >= nr) {
      keys[r] = polygons::kNoKey;
      continue;
    }
    int what = 0;
    keys[r] = polygons::poly_key((uint32_t) r, kind, J, nullptr, &what);
    holes += what == 1;
    outer += what == 2;
  }
  uint32_t sum = block_sum(holes);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_holes, (unsigned long long) sum);
  __syncthreads();  // (block_sum's shared words are read by thread 0 until here)
  sum = block_sum(outer);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_outer, (unsigned long long) sum);
}
__global__ __launch_bounds__(kThreads) void k_fc_mark(uint64_t ni, const uint64_t* __restrict__ skeys, const Ring* __restrict__ rings,
                                                      uint32_t* __restrict__ start, U128* __restrict__ area_at, polygons::Meta* pmeta) {
  RJ_GRID_STRIDE(j, ni + 1) polygons::member_mark(j, ni, skeys, rings, start, area_at, pmeta);
}
__global__ __launch_bounds__(kThreads) void k_fc_place(uint64_t ni, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ start,
                                                       const uint32_t* __restrict__ pid, uint32_t* __restrict__ first,
                                                       uint32_t* __restrict__ face_of_ring, polygons::Meta* pmeta) {
  const polygons::Out none{nullptr, nullptr, nullptr, nullptr, 0, 0};
  RJ_GRID_STRIDE(j, ni + 1) {
    polygons::member_place(j, ni, skeys, start, pid, first, none, pmeta);
    if (j < ni) face_number(j, skeys, start, pid, face_of_ring);
  }
}
__global__ __launch_bounds__(kThreads) void k_fc_emit(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ first,
                                                      const U128* __restrict__ xbase, const Ring* __restrict__ rings,
                                                      const int32_t* __restrict__ in_left, const int32_t* __restrict__ in_right, Face* out,
                                                      uint64_t cap, const polygons::Meta* pmeta) {
  if (!out) return;
  RJ_GRID_STRIDE(k, pmeta->counts.n_polygons) face_emit(k, skeys, first, xbase, rings, in_left, in_right, out, cap);
}
__global__ __launch_bounds__(kThreads) void k_fc_halves(uint32_t ni, const uint32_t* __restrict__ ring_of_half, const Jump* __restrict__ j0,
                                                        const Jump* __restrict__ j1, const uint32_t* __restrict__ face_of_ring,
                                                        const Ring* __restrict__ rings, const int32_t* __restrict__ in_left,
                                                        const int32_t* __restrict__ in_right, int32_t* __restrict__ left,
                                                        int32_t* __restrict__ right, const polygons::Meta* pmeta, Meta* meta,
                                                        const rings::Meta* rmeta) {
  if (skip(rmeta) || pmeta->unfinished) return;  // (RJ_E_INVALID and RJ_E_INTERNAL write nothing)
  const Jump* J = (pmeta->jump_done & 1) ? j1 : j0;
  uint32_t dangling = 0, conflicts = 0;
  RJ_GRID_STRIDE(h, ni) {
    const uint32_t what = half_face((uint32_t) h, ring_of_half, J, face_of_ring, rings, in_left, in_right, left, right);
    dangling += what & 1;
    conflicts += what >> 1;
  }
  uint32_t sum = block_sum(dangling);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_dangling, (unsigned long long) sum);
  __syncthreads();
  sum = block_sum(conflicts);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_conflicts, (unsigned long long) sum);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta->counts.n_faces = pmeta->counts.n_polygons;
    meta->counts.n_rings = rmeta->counts.n_rings;
    meta->counts.n_skipped = rmeta->counts.n_skipped;
  }
}

}  // namespace

hipError_t map_faces_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc64, const int32_t* in_left,
                            const int32_t* in_right, int forced_shift, uint64_t face_cap, int32_t* left, int32_t* right, Face* faces_out,
                            rings::Meta* rmeta_out, polygons::Meta* pmeta_out, Meta* result, FacesReport* report) {
  memset(rmeta_out, 0, sizeof(rings::Meta));
  memset(pmeta_out, 0, sizeof(polygons::Meta));
  memset(result, 0, sizeof(Meta));
  *report = FacesReport{};
  const uint32_t nc = (uint32_t) nc64, ni = 2 * nc;
  const uint64_t n1 = (uint64_t) ni + 1, ne = np - nc64, cap = reg_cap(ne), np1 = np + 1;
  int rounds = 1;  // walks of up to 2^(rounds - 1) steps
  while ((1ull << (rounds - 1)) < ni && rounds < kMaxRounds) rounds++;
  // the ring stages' scratch, sized by themselves
  size_t ring_bytes = 0;
  rings::Meta* rmeta = nullptr;
  const rings::Out no_out{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  hipError_t e = map_rings_enqueue(st, xy, np, row, nullptr, nullptr, nc64, rings::kNoPoints, no_out, nullptr, &ring_bytes, &rmeta);
  if (e != hipSuccess) return e;
  TempSize temp_size;
  temp_size([&](size_t& b) { return rocprim::inclusive_scan(nullptr, b, (const SegTop*) nullptr, (SegTop*) nullptr, (size_t) ni, SegMax(), st); });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) np1, rocprim::plus<uint64_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (const uint32_t*) nullptr, (uint32_t*) nullptr,
                                     (size_t) cap, 0, 64, st);
  });
  temp_size([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) ni, 0, 64, st); });
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
  polygons::Meta* pmeta;
  char* ring_scratch;
  Ring* rings;
  uint32_t *ring_first, *ring_half, *ring_of_half, *kind, *evals, *esvals, *start, *pid, *first, *face_of_ring;
  Top* chain_top;
  SegTop *seg, *segs;
  uint8_t* islast;
  uint64_t *cnt, *off, *ekeys, *eskeys, *pkeys, *pskeys;
  Jump *j0, *j1;
  U128 *area_at, *xbase;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    meta = A.take<Meta>(1);
    pmeta = A.take<polygons::Meta>(1);
    ring_scratch = A.take<char>(ring_bytes);
    rings = A.take<Ring>(ni);
    ring_first = A.take<uint32_t>(n1); ring_half = A.take<uint32_t>(ni); ring_of_half = A.take<uint32_t>(ni);
    chain_top = A.take<Top>(nc);
    seg = A.take<SegTop>(ni); segs = A.take<SegTop>(ni);
    kind = A.take<uint32_t>(ni);
    islast = A.take<uint8_t>(np);
    cnt = A.take<uint64_t>(np1); off = A.take<uint64_t>(np1);
    ekeys = A.take<uint64_t>(cap); eskeys = A.take<uint64_t>(cap);
    evals = A.take<uint32_t>(cap); esvals = A.take<uint32_t>(cap);
    j0 = A.take<Jump>(ni); j1 = A.take<Jump>(ni);
    pkeys = A.take<uint64_t>(ni); pskeys = A.take<uint64_t>(ni);
    start = A.take<uint32_t>(n1); pid = A.take<uint32_t>(n1); first = A.take<uint32_t>(n1);
    area_at = A.take<U128>(n1); xbase = A.take<U128>(n1);
    face_of_ring = A.take<uint32_t>(ni);
    temp = A.take<char>(temp_bytes);
  };
  carve();
  char* scratch = nullptr;
  if ((e = hipMalloc((void**) &scratch, A.used)) != hipSuccess) return e;
  A.base = scratch;
  carve();
  hipEvent_t ev[6];
  int n_ev = 0;
  for (; n_ev < 6; n_ev++)
    if ((e = hipEventCreate(&ev[n_ev])) != hipSuccess) break;
  int reached = -1;  // the last event recorded
  auto stamp = [&](int k) {
    if (e == hipSuccess && (e = hipEventRecord(ev[k], st)) == hipSuccess) reached = k;
  };
  const int B = blocks_for(ni, 4096), Br = blocks_for(ni, 2048), Bp = blocks_for(np1, 2048);
  const rings::Out ring_out{rings, ring_first, ring_half, nullptr, nullptr, ni, ni, 0};
  if (e == hipSuccess) do {
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(pmeta, 0, sizeof(polygons::Meta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(islast, 0, (size_t) np, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(ring_of_half, 0xFF, 4 * (size_t) ni, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(face_of_ring, 0, 4 * (size_t) ni, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(seg, 0xFF, sizeof(SegTop) * (size_t) ni, st)) != hipSuccess) break;  // (slots behind the rings': a ring of their own)
    if ((e = hipMemsetAsync(ekeys, 0xFF, 8 * (size_t) cap, st)) != hipSuccess) break;           // (kNoKey: behind the registrations when sorted)
    stamp(0);
    // 1. the rings, without labels and without points
    if ((e = map_rings_enqueue(st, xy, np, row, nullptr, nullptr, nc64, rings::kNoPoints, ring_out, ring_scratch, &ring_bytes, &rmeta)) != hipSuccess)
      break;
    stamp(1);
    // 2. tops and kinds
    hipLaunchKernelGGL(k_fc_tops, dim3(blocks_for(nc64 * kTopGroup, 8192)), dim3(kThreads), 0, st, nc64, row, xy, chain_top, islast,
                       (const rings::Meta*) rmeta);
    hipLaunchKernelGGL(k_fc_slots, dim3(B), dim3(kThreads), 0, st, (const uint32_t*) ring_first, (const uint32_t*) ring_half, (const Top*) chain_top,
                       ring_of_half, seg, (const rings::Meta*) rmeta);
    size_t tb = temp_bytes;
    if ((e = rocprim::inclusive_scan(temp, tb, (const SegTop*) seg, segs, (size_t) ni, SegMax(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_fc_kinds, dim3(B), dim3(kThreads), 0, st, (const Ring*) rings, kind, (const rings::Meta*) rmeta);
    stamp(2);
    // 3. the grid: its shift, the registrations, sorted
    hipLaunchKernelGGL(k_fc_scan, dim3(Bp), dim3(kThreads), 0, st, np, (const uint8_t*) islast, xy, meta, (const rings::Meta*) rmeta);
    hipLaunchKernelGGL(k_fc_shift, dim3(1), dim3(1), 0, st, meta, forced_shift, (const rings::Meta*) rmeta);
    hipLaunchKernelGGL(k_fc_count, dim3(Bp), dim3(kThreads), 0, st, np, (const uint8_t*) islast, xy, cnt, (const Meta*) meta,
                       (const rings::Meta*) rmeta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint64_t*) cnt, off, (uint64_t) 0, (size_t) np1, rocprim::plus<uint64_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_fc_fill, dim3(blocks_for(cap, 4096)), dim3(kThreads), 0, st, np, xy, (const uint64_t*) off, ekeys, evals, cap,
                       (const Meta*) meta, (const rings::Meta*) rmeta);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint64_t*) ekeys, eskeys, (const uint32_t*) evals, esvals, (size_t) cap, 0, 64, st)) !=
        hipSuccess)
      break;
    stamp(3);
    // 4. the first ceiling edge above every hole's top
    hipLaunchKernelGGL(k_fc_above, dim3(blocks_for((uint64_t) ni * kRayGroup, 8192)), dim3(kThreads), 0, st, cap, nc64, row, xy,
                       (const uint32_t*) ring_first, (const SegTop*) segs, (const uint32_t*) kind, (const uint32_t*) ring_of_half,
                       (const uint64_t*) eskeys, (const uint32_t*) esvals, j0, j1, meta, (const rings::Meta*) rmeta);
    stamp(4);
    // 5. parents; faces
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_fc_jump_round, dim3(Br), dim3(kThreads), 0, st, (const Jump*) ((r & 1) ? j1 : j0), (r & 1) ? j0 : j1, pmeta,
                         (const rings::Meta*) rmeta, r);
    hipLaunchKernelGGL(k_fc_rounds_done, dim3(1), dim3(1), 0, st, pmeta, (const rings::Meta*) rmeta, rounds);
    if ((e = hipGetLastError()) != hipSuccess) break;
    hipLaunchKernelGGL(k_fc_keys, dim3(Br), dim3(kThreads), 0, st, ni, (const uint32_t*) kind, (const Jump*) j0, (const Jump*) j1, pkeys, pmeta, meta,
                       (const rings::Meta*) rmeta);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_keys(temp, tb, (const uint64_t*) pkeys, pskeys, (size_t) ni, 0, 64, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_fc_mark, dim3(B), dim3(kThreads), 0, st, (uint64_t) ni, (const uint64_t*) pskeys, (const Ring*) rings, start, area_at, pmeta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) start, pid, (uint32_t) 0, (size_t) n1, rocprim::plus<uint32_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_fc_place, dim3(B), dim3(kThreads), 0, st, (uint64_t) ni, (const uint64_t*) pskeys, (const uint32_t*) start,
                       (const uint32_t*) pid, first, face_of_ring, pmeta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const U128*) area_at, xbase, U128{0, 0}, (size_t) n1, U128Sum(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_fc_emit, dim3(Br), dim3(kThreads), 0, st, (const uint64_t*) pskeys, (const uint32_t*) first, (const U128*) xbase,
                       (const Ring*) rings, in_left, in_right, faces_out, face_cap, (const polygons::Meta*) pmeta);
    hipLaunchKernelGGL(k_fc_halves, dim3(Br), dim3(kThreads), 0, st, ni, (const uint32_t*) ring_of_half, (const Jump*) j0, (const Jump*) j1,
                       (const uint32_t*) face_of_ring, (const Ring*) rings, in_left, in_right, left, right, (const polygons::Meta*) pmeta, meta,
                       (const rings::Meta*) rmeta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    stamp(5);
    // the one read-back
    if ((e = hipMemcpyAsync(rmeta_out, rmeta, sizeof(rings::Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(pmeta_out, pmeta, sizeof(polygons::Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);  // (nothing of this call still runs when its scratch goes)
  if (e == hipSuccess) {
    for (int k = 0; k < 5 && k < reached; k++) (void) hipEventElapsedTime(&report->ms[k], ev[k], ev[k + 1]);
    if (reached == 5) (void) hipEventElapsedTime(&report->ms[5], ev[0], ev[5]);
    report->shift = (int) result->shift;
    report->registrations = result->n_regs;
    report->ray_tests = result->ray_tests;
    report->cells = result->cells;
  }
  for (int k = 0; k < n_ev; k++) (void) hipEventDestroy(ev[k]);
  const hipError_t fe = hipFree(scratch);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
