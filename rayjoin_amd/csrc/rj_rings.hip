// rj_rings.hip -- the face rings of a chain map on the device (rj_rings.h has the definition and the stages).
// Every kernel is a grid-stride loop over one of rj_rings.h's per-element functions; rocPRIM does the merge sort that
// orders the junctions, the radix sort of the ring keys and the four scans.  The rounds of the pointer doubling and of
// the ranking are separate launches with a fixed bound: a round that is not needed returns at once, no kernel waits on
// another block, nothing spins on device memory.  The map check's status word stays on the device (a map that fails
// it is not read); the host reads one Meta at the end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_pipeline.h"
#include "rj_rings.h"

namespace rj {

using namespace rings;

namespace {

constexpr int kGroup = 8;  // lanes per half-chain in the placement kernel (the chains of an overlay's output map are short)

struct IncBefore {
  const Inc* inc;
  __host__ __device__ bool operator()(const uint32_t& a, const uint32_t& b) const { return inc_before(a, b, inc); }
};
struct SlotsSum {
  __host__ __device__ Slots operator()(const Slots& a, const Slots& b) const { return Slots{a.halves + b.halves, a.points + b.points}; }
};
struct U128Sum {
  __host__ __device__ U128 operator()(const U128& a, const U128& b) const { return add(a, b); }
};

__global__ __launch_bounds__(kThreads) void k_rg_check(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                       Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, check_row(c, row, nc, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, check_coordinate(xy[i]));
  if (bad) atomicMax(&meta->bad_map, bad);
}
__global__ __launch_bounds__(kThreads) void k_rg_incidence(uint32_t ni, const int64_t* __restrict__ xy, const uint32_t* __restrict__ row,
                                                           Inc* __restrict__ inc, uint32_t* __restrict__ iota, Meta* meta) {
  const bool bad = meta->bad_map != 0;
  uint32_t skipped_chains = 0;
  RJ_GRID_STRIDE(h, ni) {
    const bool s = incidence((uint32_t) h, xy, row, bad, inc);
    skipped_chains += s && !(h & 1) ? 1u : 0u;
    iota[h] = (uint32_t) h;
  }
  const uint32_t sum = block_sum(skipped_chains);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_skipped, (unsigned long long) sum);
}
__global__ __launch_bounds__(kThreads) void k_rg_head(uint32_t ni, const uint32_t* __restrict__ sv, const Inc* __restrict__ inc,
                                                      uint32_t* __restrict__ pos, uint32_t* __restrict__ head) {
  RJ_GRID_STRIDE(j, ni) junction_head((uint32_t) j, sv, inc, pos, head);
}
__global__ __launch_bounds__(kThreads) void k_rg_last(uint32_t ni, const uint32_t* __restrict__ sv, const Inc* __restrict__ inc,
                                                      const uint32_t* __restrict__ begin, uint32_t* __restrict__ last_of) {
  RJ_GRID_STRIDE(j, ni) junction_last((uint32_t) j, ni, sv, inc, begin, last_of);
}
__global__ __launch_bounds__(kThreads) void k_rg_next(uint32_t ni, const uint32_t* __restrict__ sv, const Inc* __restrict__ inc,
                                                      const uint32_t* __restrict__ pos, const uint32_t* __restrict__ begin,
                                                      const uint32_t* __restrict__ last_of, uint32_t* __restrict__ next, Link* __restrict__ a,
                                                      Link* __restrict__ b) {
  RJ_GRID_STRIDE(h, ni) next_of((uint32_t) h, sv, inc, pos, begin, last_of, next, a, b);
}
// one round of pointer doubling; a round that is not needed returns at once and leaves its number behind
__global__ __launch_bounds__(kThreads) void k_rg_cyc_round(uint32_t ni, const Link* __restrict__ in, Link* __restrict__ out, Meta* meta, int r) {
  if (!round_needed(meta->changed, r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !meta->cyc_done) meta->cyc_done = (uint32_t) r;
    return;
  }
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, ni) mine += cyc_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&meta->changed[r], sum);
}
__global__ __launch_bounds__(kThreads) void k_rg_rank_round(uint32_t ni, const Node* __restrict__ in, Node* __restrict__ out, Meta* meta, int r) {
  if (!round_needed(meta->act, r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !meta->rank_done) meta->rank_done = (uint32_t) r;
    return;
  }
  uint32_t mine = 0;
  RJ_GRID_STRIDE(i, ni) mine += rank_round((uint32_t) i, in, out) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd(&meta->act[r], sum);
}
// behind the last round: every round ran (the final state is in buffer rounds & 1), and the last must have found nothing to do
__global__ void k_rg_rounds_done(Meta* meta, int rounds, int ranking) {
  uint32_t* done = ranking ? &meta->rank_done : &meta->cyc_done;
  const uint32_t* count = ranking ? meta->act : meta->changed;
  if (!*done) {
    *done = (uint32_t) rounds;
    if (count[rounds - 1]) meta->unfinished = 1;
  }
}
__global__ __launch_bounds__(kThreads) void k_rg_rank_init(uint32_t ni, const Link* __restrict__ l0, const Link* __restrict__ l1, const Meta* meta,
                                                           const uint32_t* __restrict__ next, const Inc* __restrict__ inc,
                                                           const uint32_t* __restrict__ row, Node* __restrict__ a, Node* __restrict__ b) {
  const Link* F = (meta->cyc_done & 1) ? l1 : l0;
  RJ_GRID_STRIDE(h, ni) rank_init((uint32_t) h, F, next, inc, row, a, b);
}
__global__ __launch_bounds__(kThreads) void k_rg_keys(uint32_t ni, const Link* __restrict__ l0, const Link* __restrict__ l1, const Meta* meta,
                                                      const Inc* __restrict__ inc, const int32_t* __restrict__ left,
                                                      const int32_t* __restrict__ right, uint32_t flags, uint64_t* __restrict__ keys) {
  const Link* F = (meta->cyc_done & 1) ? l1 : l0;
  RJ_GRID_STRIDE(h, ni) keys[h] = ring_key((uint32_t) h, F, inc, left, right, flags);
}
__global__ __launch_bounds__(kThreads) void k_rg_slot(uint32_t ni, const uint64_t* __restrict__ skeys, const Node* __restrict__ n0,
                                                      const Node* __restrict__ n1, uint32_t* __restrict__ ring_of, Slots* __restrict__ total,
                                                      Meta* meta) {
  const Node* N = (meta->rank_done & 1) ? n1 : n0;
  RJ_GRID_STRIDE(r, (uint64_t) ni + 1) ring_slot((uint32_t) r, ni, skeys, N, ring_of, total, meta);
}
// a group of kGroup lanes per half-chain: consecutive lanes copy consecutive points (16 bytes each) to consecutive slots
__global__ __launch_bounds__(kThreads) void k_rg_place(uint32_t ni, const int64_t* __restrict__ xy, const uint32_t* __restrict__ row,
                                                       const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                       const Link* __restrict__ l0, const Link* __restrict__ l1, const Node* __restrict__ n0,
                                                       const Node* __restrict__ n1, const Meta* meta, const Inc* __restrict__ inc,
                                                       const uint32_t* __restrict__ ring_of, const Slots* __restrict__ base,
                                                       const uint64_t* __restrict__ skeys, U128* __restrict__ cross_at, uint32_t* __restrict__ mixed,
                                                       Out o) {
  if (meta->bad_map || meta->unfinished) return;  // (a map that failed its check is not read; no slots without a finished ranking)
  const Link* F = (meta->cyc_done & 1) ? l1 : l0;
  const Node* N = (meta->rank_done & 1) ? n1 : n0;
  const uint32_t lane = threadIdx.x & (kGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kGroup;
  for (uint64_t h = g0; h < ni; h += gstride) {  // (the same trips for all lanes of a group)
    uint64_t slot = 0, pslot = 0;
    const uint32_t r = half_slots((uint32_t) h, F, inc, N, ring_of, base, &slot, &pslot);
    if (r == kNone) continue;
    U128 sum = half_points((uint32_t) h, lane, kGroup, xy, row, pslot, o.ring_xy, o.point_cap);
    for (int d = kGroup / 2; d >= 1; d >>= 1) {
      U128 other;
      other.lo = (uint64_t) __shfl_xor((long long) sum.lo, d, kGroup);
      other.hi = (uint64_t) __shfl_xor((long long) sum.hi, d, kGroup);
      sum = add(sum, other);
    }
    if (lane == 0) half_store((uint32_t) h, r, slot, ni, sum, skeys, left, right, cross_at, mixed, o.ring_half, o.half_cap);
  }
}
__global__ __launch_bounds__(kThreads) void k_rg_emit(uint32_t ni, const uint64_t* __restrict__ skeys, const Slots* __restrict__ base,
                                                      const U128* __restrict__ xbase, const uint32_t* __restrict__ mixed, Out o, Meta* meta) {
  if (meta->bad_map || meta->unfinished) return;  // (a refused map writes nothing, not even the CSRs' one entry of no rings)
  const uint64_t n_rings = meta->counts.n_rings;  // (<= ni: base and xbase have ni + 1 entries)
  uint32_t mine = 0;
  RJ_GRID_STRIDE(r, n_rings + 1) mine += ring_emit((uint32_t) r, skeys, base, xbase, mixed, o, meta) ? 1u : 0u;
  const uint32_t sum = block_sum(mine);
  if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*) &meta->counts.n_mixed, (unsigned long long) sum);
}

}  // namespace

// the stages of rj_map_rings enqueued on st without a wait (nc64 > 0).  scratch null: only *bytes, the scratch this map
// needs, is set.  Otherwise the stages run in `scratch` (that many bytes), *meta_dev is where their Meta lies in it, and
// the caller waits for the stream before it reads that or lets the scratch go.  left / right null: every face is 0 (the
// rings then ascend by leader alone).
hipError_t map_rings_enqueue(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right,
                             uint64_t nc64, uint32_t flags, const Out& out, char* scratch, size_t* bytes, Meta** meta_dev) {
  Out o = out;
  if (flags & kNoPoints) {
    o.ring_row = nullptr;
    o.ring_xy = nullptr;
    o.point_cap = 0;
  }
  const uint32_t nc = (uint32_t) nc64, ni = 2 * nc;
  const uint64_t n1 = (uint64_t) ni + 1;
  int rounds = 1;  // rings of up to 2^(rounds - 1) half-chains
  while ((1ull << (rounds - 1)) < ni && rounds < kMaxRounds) rounds++;
  TempSize temp_size;
  temp_size([&](size_t& b) {
    return rocprim::merge_sort(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) ni, IncBefore{nullptr}, st);
  });
  temp_size([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) ni, 0, 64, st); });
  temp_size([&](size_t& b) {
    return rocprim::inclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) ni, rocprim::maximum<uint32_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const Slots*) nullptr, (Slots*) nullptr, Slots{0, 0}, (size_t) n1, SlotsSum(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const U128*) nullptr, (U128*) nullptr, U128{0, 0}, (size_t) n1, U128Sum(), st);
  });
  if (temp_size.error != hipSuccess) return temp_size.error;
  const size_t temp_bytes = temp_size.bytes;
  // ---- scratch: one allocation, carved (sizes first, then the pointers), freed at the end ----------------------
  Meta* meta;
  Inc* inc;
  uint32_t *junction, *next, *ring_of, *mixed;
  Link *l0, *l1;
  Node *n0, *nb;
  Slots *total, *base;
  U128 *cross_at, *xbase;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    meta = A.take<Meta>(1);
    inc = A.take<Inc>(ni);
    junction = A.take<uint32_t>(5 * (uint64_t) ni);
    next = A.take<uint32_t>(ni);
    l0 = A.take<Link>(ni); l1 = A.take<Link>(ni);
    n0 = A.take<Node>(ni); nb = A.take<Node>(ni);
    ring_of = A.take<uint32_t>(ni);
    mixed = A.take<uint32_t>(n1);
    total = A.take<Slots>(n1); base = A.take<Slots>(n1);
    cross_at = A.take<U128>(n1); xbase = A.take<U128>(n1);
    temp = A.take<char>(temp_bytes);
  };
  carve();
  *bytes = A.used;
  if (!scratch) return hipSuccess;
  A.base = scratch;
  carve();
  *meta_dev = meta;
  hipError_t e = hipSuccess;
  // the five junction arrays are dead once next[] is known: the ring keys and their sorted form live there later
  uint32_t *iota = junction, *sv = junction + ni, *pos = junction + 2 * (uint64_t) ni, *head = junction + 3 * (uint64_t) ni,
           *begin = junction + 4 * (uint64_t) ni, *last_of = head;  // (head[] is dead behind its scan)
  uint64_t *keys = reinterpret_cast<uint64_t*>(junction), *skeys = keys + ni;
  const int B = blocks_for(ni, 4096), Br = blocks_for(ni, 2048);
  do {
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_rg_check, dim3(blocks_for(2 * np > nc64 + 1 ? 2 * np : nc64 + 1, 2048)), dim3(kThreads), 0, st, xy, np, row, nc64, meta);
    // 1. incidences, the one sort
    hipLaunchKernelGGL(k_rg_incidence, dim3(Br), dim3(kThreads), 0, st, ni, xy, row, inc, iota, meta);
    size_t tb = temp_bytes;
    if ((e = rocprim::merge_sort(temp, tb, (const uint32_t*) iota, sv, (size_t) ni, IncBefore{inc}, st)) != hipSuccess) break;
    // 2. junctions; 3. next
    hipLaunchKernelGGL(k_rg_head, dim3(B), dim3(kThreads), 0, st, ni, (const uint32_t*) sv, (const Inc*) inc, pos, head);
    tb = temp_bytes;
    if ((e = rocprim::inclusive_scan(temp, tb, (const uint32_t*) head, begin, (size_t) ni, rocprim::maximum<uint32_t>(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_rg_last, dim3(B), dim3(kThreads), 0, st, ni, (const uint32_t*) sv, (const Inc*) inc, (const uint32_t*) begin, last_of);
    hipLaunchKernelGGL(k_rg_next, dim3(B), dim3(kThreads), 0, st, ni, (const uint32_t*) sv, (const Inc*) inc, (const uint32_t*) pos,
                       (const uint32_t*) begin, (const uint32_t*) last_of, next, l0, l1);
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_rg_cyc_round, dim3(Br), dim3(kThreads), 0, st, ni, (const Link*) ((r & 1) ? l1 : l0), (r & 1) ? l0 : l1, meta, r);
    hipLaunchKernelGGL(k_rg_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 0);
    // 4. ranking
    hipLaunchKernelGGL(k_rg_rank_init, dim3(B), dim3(kThreads), 0, st, ni, (const Link*) l0, (const Link*) l1, (const Meta*) meta,
                       (const uint32_t*) next, (const Inc*) inc, row, n0, nb);
    for (int r = 0; r < rounds; r++)
      hipLaunchKernelGGL(k_rg_rank_round, dim3(Br), dim3(kThreads), 0, st, ni, (const Node*) ((r & 1) ? nb : n0), (r & 1) ? n0 : nb, meta, r);
    hipLaunchKernelGGL(k_rg_rounds_done, dim3(1), dim3(1), 0, st, meta, rounds, 1);
    if ((e = hipGetLastError()) != hipSuccess) break;
    // 5. the rings in their order, the two CSRs
    hipLaunchKernelGGL(k_rg_keys, dim3(B), dim3(kThreads), 0, st, ni, (const Link*) l0, (const Link*) l1, (const Meta*) meta, (const Inc*) inc,
                       left, right, flags, keys);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_keys(temp, tb, (const uint64_t*) keys, skeys, (size_t) ni, 0, 64, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(ring_of, 0xFF, 4 * (size_t) ni, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(mixed, 0, 4 * (size_t) n1, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(cross_at, 0, sizeof(U128) * (size_t) n1, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_rg_slot, dim3(B), dim3(kThreads), 0, st, ni, (const uint64_t*) skeys, (const Node*) n0, (const Node*) nb, ring_of, total,
                       meta);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const Slots*) total, base, Slots{0, 0}, (size_t) n1, SlotsSum(), st)) != hipSuccess) break;
    // 6. half-chains and points to their slots; 7. areas and records
    hipLaunchKernelGGL(k_rg_place, dim3(blocks_for((uint64_t) ni * kGroup, 8192)), dim3(kThreads), 0, st, ni, xy, row, left, right, (const Link*) l0,
                       (const Link*) l1, (const Node*) n0, (const Node*) nb, (const Meta*) meta, (const Inc*) inc, (const uint32_t*) ring_of,
                       (const Slots*) base, (const uint64_t*) skeys, cross_at, mixed, o);
    tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const U128*) cross_at, xbase, U128{0, 0}, (size_t) n1, U128Sum(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_rg_emit, dim3(Br), dim3(kThreads), 0, st, ni, (const uint64_t*) skeys, (const Slots*) base, (const U128*) xbase,
                       (const uint32_t*) mixed, o, meta);
    e = hipGetLastError();
  } while (0);
  return e;
}

hipError_t map_rings_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right,
                            uint64_t nc64, uint32_t flags, const Out& out, Meta* result) {
  memset(result, 0, sizeof(Meta));
  if (nc64 == 0) {  // no rings: the CSRs' one entry, where the caller has arrays
    hipError_t e = hipSuccess;
    if (out.ring_first) e = hipMemsetAsync(out.ring_first, 0, 4, st);
    if (e == hipSuccess && out.ring_row && !(flags & kNoPoints)) e = hipMemsetAsync(out.ring_row, 0, 4, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  }
  size_t bytes = 0;
  Meta* meta = nullptr;
  hipError_t e = map_rings_enqueue(st, xy, np, row, left, right, nc64, flags, out, nullptr, &bytes, &meta);
  if (e != hipSuccess) return e;
  char* scratch = nullptr;
  if ((e = hipMalloc((void**) &scratch, bytes)) != hipSuccess) return e;
  e = map_rings_enqueue(st, xy, np, row, left, right, nc64, flags, out, scratch, &bytes, &meta);
  // the one read-back
  if (e == hipSuccess) e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);  // (nothing of this call still runs when its scratch goes)
  const hipError_t fe = hipFree(scratch);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
