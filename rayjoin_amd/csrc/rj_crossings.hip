// rj_crossings.hip -- the crossings inside one chain map on the device (rj_crossings.h has the definition and the
// stages).  Every kernel but the pair pass is a grid-stride loop over one of rj_crossings.h's per-element functions;
// rocPRIM does the two radix sorts (the registrations by cell, the hits by edge pair; rj_kernels.h's wrappers), the two
// scans and the selection of the work items.  The grid is sparse: sorted (cell, eid) pairs, a run of equal cells is a
// cell's list, and no table over the cells exists.  In the pair pass a wave owns one work item -- up to kRowBlock rows
// of a run -- and its lanes take the columns behind them, 64 at a time; hits are appended with one atomic per wave
// (ballot and rank, as k_lsi_grid appends).  Scratch comes in three blocks, each sized by what the host has just read:
// the edges, the registrations, the hits.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <string.h>

#include "rj_crossings.h"
#include "rj_kernels.h"
#include "rj_pipeline.h"

namespace rj {

using namespace crossings;

namespace {

constexpr int kSums = kShifts + 2;  // the registrations per shift, then the two halves of the extent
static_assert(offsetof(Meta, extent_hi) == offsetof(Meta, regs) + 8 * (kSums - 1), "the sums are one run of words");
static_assert(offsetof(Meta, counts) + 8 == offsetof(Meta, counts.n_proper) && offsetof(Meta, counts.n_equal) == offsetof(Meta, counts.n_proper) + 24,
              "the four kinds are one run of words");

// dst[k] += the block's sum of acc[k]; the first n_clamped sums stop at kClamp (at most 4096 blocks add one each: no
// 64-bit counter overflows).  Blocks of kThreads.
template <int N>
__device__ __forceinline__ void block_add(const ull (&acc)[N], ull* dst, int n_clamped) {
  __shared__ ull part[kThreads / 64][N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    ull v = acc[k];
    for (int d = 32; d >= 1; d >>= 1) {
      const ull o = __shfl_down(v, d, 64);
      v = k < n_clamped ? clamp_add(v, o) : v + o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    ull sum = 0;
    for (int w = 0; w < kThreads / 64; w++) sum = k < n_clamped ? clamp_add(sum, part[w][k]) : sum + part[w][k];
    if (sum) atomicAdd(dst + k, sum);
  }
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t) __builtin_amdgcn_readfirstlane((uint32_t) (v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t) v);
}

__global__ void k_cx_noop() {}

__global__ __launch_bounds__(kThreads) void k_cx_check(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy, uint64_t np,
                                                       Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, check_row(c, row, nc, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, check_coordinate(xy[i]));
  if (bad) atomicMax(&meta->bad, bad);
}
// the edges, and behind them what the choice of the shift needs: zero edges, extents, registrations at every shift
__global__ __launch_bounds__(kThreads) void k_cx_edges(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy, uint64_t ne,
                                                       Edge* __restrict__ edges, Meta* meta) {
  if (meta->bad) return;
  ull acc[kSums], zero[1] = {0};
#pragma unroll
  for (int k = 0; k < kSums; k++) acc[k] = 0;
  RJ_GRID_STRIDE(e, ne) {
    const Edge E = edge_of(e, row, nc, xy);
    edges[e] = E;
    if (is_zero(E)) {
      zero[0]++;
      continue;
    }
#pragma unroll
    for (int k = 0; k < kShifts; k++) acc[k] = clamp_add(acc[k], reg_count(E, kMinShift + k));
    const uint64_t ext = extent_of(E);
    acc[kShifts] += ext & 0xFFFFFFFFull;
    acc[kShifts + 1] += ext >> 32;
  }
  block_add(acc, (ull*) meta->regs, kShifts);
  block_add(zero, (ull*) &meta->counts.n_zero_edges, 0);
}
// cnt[e] at the chosen shift; entry ne closes the scan
__global__ __launch_bounds__(kThreads) void k_cx_count(const Edge* __restrict__ edges, uint64_t ne, int s, uint64_t* __restrict__ cnt) {
  RJ_GRID_STRIDE(e, ne + 1) cnt[e] = e < ne && !is_zero(edges[e]) ? reg_count(edges[e], s) : 0;
}
__global__ __launch_bounds__(kThreads) void k_cx_regs(uint64_t n, const uint64_t* __restrict__ off, uint64_t ne, const Edge* __restrict__ edges, int s,
                                                      uint64_t* __restrict__ key, uint32_t* __restrict__ eid) {
  RJ_GRID_STRIDE(r, n) reg_at(r, off, ne, edges, s, &key[r], &eid[r]);
}
__global__ __launch_bounds__(kThreads) void k_cx_heads(uint64_t n, const uint64_t* __restrict__ key, uint64_t* __restrict__ head) {
  RJ_GRID_STRIDE(r, n) head[r] = run_head(r, key);
}
__global__ __launch_bounds__(kThreads) void k_cx_items(uint64_t n, const uint64_t* __restrict__ key, const uint64_t* __restrict__ start,
                                                       uint8_t* __restrict__ flag, Meta* meta) {
  ull tests[1] = {0}, longest = 0;
  RJ_GRID_STRIDE(r, n) {
    uint64_t k;
    flag[r] = item_flag(r, n, key, start, &k) ? 1 : 0;
    if (k) tests[0] = clamp_add(tests[0], run_tests(k));
    longest = k > longest ? k : longest;
  }
  if (longest) atomicMax((ull*) &meta->largest_run, longest);
  block_add(tests, (ull*) &meta->pair_tests, 1);
}
// (only behind a refused call) the first run of the largest length
__global__ __launch_bounds__(kThreads) void k_cx_largest(uint64_t n, const uint64_t* __restrict__ key, const uint64_t* __restrict__ start, Meta* meta) {
  const uint64_t want = meta->largest_run;
  RJ_GRID_STRIDE(r, n) {
    uint64_t k;
    (void) item_flag(r, n, key, start, &k);
    if (k == want) atomicMin((ull*) &meta->largest_at, (ull) start[r]);
  }
}

// One wave per work item.  Item p: the rows [p, p + kRowBlock) of its run, every row i against the columns j > i of the
// run.  The lanes hold 64 consecutive columns; the rows go by one at a time, wave-uniform.  key[], eid[]: the sorted
// registrations; hits beyond `cap` are counted, not stored.
__global__ __launch_bounds__(kThreads) void k_cx_pairs(const uint64_t* __restrict__ items, const uint64_t* __restrict__ key,
                                                       const uint32_t* __restrict__ eid, uint64_t n, const Edge* __restrict__ edges, int s,
                                                       uint64_t* __restrict__ hit, uint32_t* __restrict__ hit_kind, uint64_t cap, Meta* meta) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_items = meta->n_items;
  const uint64_t wave = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
  ull kinds[4] = {0, 0, 0, 0};
  for (uint64_t it = wave; it < n_items; it += nwaves) {
    const uint64_t p = uniform64(items[it]);
    const uint64_t ck = key[p];
    for (uint64_t j0 = p + 1;; j0 += 64) {
      const uint64_t j = j0 + lane;
      const bool valid = j < n && key[j] == ck;
      const uint64_t vm = __ballot(valid);  // (a run is contiguous: the valid lanes are the first ones)
      if (!vm) break;
      uint32_t eb = 0;
      Edge b{0, 0, 0, 0};
      if (valid) {
        eb = eid[j];
        b = edges[eb];
      }
      const uint64_t last = j0 + (uint64_t) __popcll(vm) - 1, i_end = row_limit(p, last);
      const uint64_t mine = valid ? row_limit(p, j) : p;
      for (uint64_t i = p; i < i_end; i++) {
        const uint32_t ea = eid[i];
        const Edge a = edges[ea];
        const uint32_t kind = i < mine ? pair_kind(a, b, ck, s) : kNone;
        const uint64_t hm = __ballot(kind != kNone);
        if (hm) {
          ull base = 0;
          if (lane == 0) base = atomicAdd((ull*) &meta->counts.n_found, (ull) __popcll(hm));
          base = uniform64(base);
          const ull pos = base + (ull) __popcll(hm & ((1ull << lane) - 1));
          if (kind != kNone) {
            kinds[kind - 1]++;
            if (pos < cap) {
              hit[pos] = hit_key(ea, eb);
              hit_kind[pos] = kind;
            }
          }
        }
      }
      if (vm != ~0ull) break;  // the run ended inside these columns
    }
  }
  block_add(kinds, (ull*) &meta->counts.n_proper, 0);
}
__global__ __launch_bounds__(kThreads) void k_cx_emit(uint64_t n, const uint64_t* __restrict__ hit, const uint32_t* __restrict__ hit_kind,
                                                      uint4* __restrict__ out) {
  RJ_GRID_STRIDE(r, n) out[r] = make_uint4((uint32_t) (hit[r] >> 32), (uint32_t) hit[r], hit_kind[r], 0u);
}

}  // namespace

hipError_t warm_crossings_kernels(hipStream_t st) {
  hipLaunchKernelGGL(k_cx_noop, dim3(1), dim3(1), 0, st);
  return hipGetLastError();
}

hipError_t map_crossings_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint64_t capacity, void* out,
                                const CrossingsTuning& tuning, Meta* result, CrossingsReport* report) {
  memset(result, 0, sizeof(Meta));
  memset(report, 0, sizeof(*report));
  for (float& m : report->ms) m = -1.0f;
  const uint64_t ne = np - nc;
  result->counts.n_edges = ne;
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  char *blockA = nullptr, *blockB = nullptr, *blockC = nullptr;
  int marks = 0;
  do {
    // ---- A. the check, the edges, the sums behind the choice of the shift -----------------------------------------
    Meta* meta;
    Edge* edges;
    uint64_t *cnt, *off;
    void* tempA;
    TempSize sizeA;
    sizeA([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) (ne + 1), rocprim::plus<uint64_t>(), st);
    });
    if ((e = sizeA.error) != hipSuccess) break;
    Carve A;
    auto carveA = [&]() {
      A.used = 0;
      meta = A.take<Meta>(1);
      edges = A.take<Edge>(ne);
      cnt = A.take<uint64_t>(ne + 1); off = A.take<uint64_t>(ne + 1);
      tempA = A.take<char>(sizeA.bytes);
    };
    carveA();
    if ((e = hipMalloc((void**) &blockA, A.used)) != hipSuccess) break;
    A.base = blockA;
    carveA();
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_cx_check, dim3(blocks_for(2 * np > nc + 1 ? 2 * np : nc + 1, 2048)), dim3(kThreads), 0, st, row, nc, xy, np, meta);
    if (ne) hipLaunchKernelGGL(k_cx_edges, dim3(blocks_for(ne, 2048)), dim3(kThreads), 0, st, row, nc, xy, ne, edges, meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    marks = 1;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // sync 1: the grid's size
    result->counts.n_edges = ne;
    const uint64_t n_live = ne - result->counts.n_zero_edges;
    if (result->bad || n_live < 2) break;  // (fewer than two edges: no pair)
    const int s = tuning.shift ? tuning.shift
                               : choose_shift(result->extent_lo, result->extent_hi, result->regs, n_live, ne, tuning.extent_factor, tuning.reg_factor);
    const uint64_t R = result->regs[s - kMinShift];
    report->shift = s;
    report->registrations = R;
    if (R >= kClamp) {  // (a forced shift only: the chosen one is bounded by the edges)
      report->over_budget = true;
      break;
    }
    // ---- B. the registrations, sorted by cell; runs and work items ---------------------------------------------
    uint64_t *kin, *kout, *start;
    uint32_t *vin, *vout;
    uint8_t* flag;
    void* tempB;
    TempSize sizeB;
    const unsigned end_bit = (unsigned) (32 + 47 - s);  // a cell coordinate has 47 - s bits
    sizeB([&](size_t& b) { return sort_pairs_u64_u32(st, nullptr, b, nullptr, nullptr, nullptr, nullptr, R, 0, end_bit); });
    sizeB([&](size_t& b) {
      return rocprim::inclusive_scan(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) R, rocprim::maximum<uint64_t>(), st);
    });
    sizeB([&](size_t& b) {
      return rocprim::select(nullptr, b, rocprim::counting_iterator<uint64_t>(0), (const uint8_t*) nullptr, (uint64_t*) nullptr, (uint64_t*) nullptr,
                             (size_t) R, st);
    });
    if ((e = sizeB.error) != hipSuccess) break;
    Carve B;
    auto carveB = [&]() {
      B.used = 0;
      kin = B.take<uint64_t>(R); kout = B.take<uint64_t>(R);  // (kin: the keys, then the run heads, then the work items)
      vin = B.take<uint32_t>(R); vout = B.take<uint32_t>(R);
      start = B.take<uint64_t>(R);
      flag = B.take<uint8_t>(R);
      tempB = B.take<char>(sizeB.bytes);
    };
    carveB();
    if ((e = hipMalloc((void**) &blockB, B.used)) != hipSuccess) break;
    B.base = blockB;
    carveB();
    const int BR = blocks_for(R, 4096);
    hipLaunchKernelGGL(k_cx_count, dim3(blocks_for(ne + 1, 4096)), dim3(kThreads), 0, st, (const Edge*) edges, ne, s, cnt);
    size_t tb = sizeA.bytes;
    if ((e = rocprim::exclusive_scan(tempA, tb, (const uint64_t*) cnt, off, (uint64_t) 0, (size_t) (ne + 1), rocprim::plus<uint64_t>(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_cx_regs, dim3(BR), dim3(kThreads), 0, st, R, (const uint64_t*) off, ne, (const Edge*) edges, s, kin, vin);
    tb = sizeB.bytes;
    if ((e = sort_pairs_u64_u32(st, tempB, tb, kin, kout, vin, vout, R, 0, end_bit)) != hipSuccess) break;
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    uint64_t *head = kin, *items = kin;
    hipLaunchKernelGGL(k_cx_heads, dim3(BR), dim3(kThreads), 0, st, R, (const uint64_t*) kout, head);
    tb = sizeB.bytes;
    if ((e = rocprim::inclusive_scan(tempB, tb, (const uint64_t*) head, start, (size_t) R, rocprim::maximum<uint64_t>(), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_cx_items, dim3(BR), dim3(kThreads), 0, st, R, (const uint64_t*) kout, (const uint64_t*) start, flag, meta);
    tb = sizeB.bytes;
    if ((e = rocprim::select(tempB, tb, rocprim::counting_iterator<uint64_t>(0), (const uint8_t*) flag, items, &meta->n_items, (size_t) R, st)) != hipSuccess)
      break;
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    marks = 3;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // sync 2: the pair tests
    result->counts.n_edges = ne;
    report->pair_tests = result->pair_tests;
    report->largest_run = result->largest_run;
    report->n_items = result->n_items;
    if (result->pair_tests > tuning.pair_budget) {  // the guard: name the largest cell, launch nothing more
      report->over_budget = true;
      if ((e = hipMemsetAsync(&meta->largest_at, 0xFF, 8, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_cx_largest, dim3(BR), dim3(kThreads), 0, st, R, (const uint64_t*) kout, (const uint64_t*) start, meta);
      uint64_t at = 0;
      if ((e = hipMemcpyAsync(&at, &meta->largest_at, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;
      if (at < R) {
        if ((e = hipMemcpyAsync(&report->largest_cell, kout + at, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
        e = hipStreamSynchronize(st);
      }
      break;
    }
    // ---- C. the pair pass; the hits sorted into the caller's array --------------------------------------------
    const uint64_t cap = capacity < result->pair_tests ? capacity : result->pair_tests;  // (no more hits than tests)
    uint64_t *hit, *hit_sorted;
    uint32_t *hit_kind, *kind_sorted;
    void* tempC;
    TempSize sizeC;
    if (cap) sizeC([&](size_t& b) { return sort_pairs_u64_u32(st, nullptr, b, nullptr, nullptr, nullptr, nullptr, cap, 0, 64); });
    if ((e = sizeC.error) != hipSuccess) break;
    Carve C;
    auto carveC = [&]() {
      C.used = 0;
      hit = C.take<uint64_t>(cap); hit_sorted = C.take<uint64_t>(cap);
      hit_kind = C.take<uint32_t>(cap); kind_sorted = C.take<uint32_t>(cap);
      tempC = C.take<char>(sizeC.bytes);
    };
    carveC();
    if ((e = hipMalloc((void**) &blockC, C.used ? C.used : 1)) != hipSuccess) break;
    C.base = blockC;
    carveC();
    if (result->n_items)
      hipLaunchKernelGGL(k_cx_pairs, dim3(blocks_for(result->n_items * 64, 4096)), dim3(kThreads), 0, st, (const uint64_t*) items, (const uint64_t*) kout,
                         (const uint32_t*) vout, R, (const Edge*) edges, s, hit, hit_kind, cap, meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    marks = 4;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // sync 3: the number of hits
    result->counts.n_edges = ne;
    const uint64_t found = result->counts.n_found;
    if (found && found <= capacity) {
      tb = sizeC.bytes;
      if ((e = sort_pairs_u64_u32(st, tempC, tb, hit, hit_sorted, hit_kind, kind_sorted, found, 0, 64)) != hipSuccess) break;
      hipLaunchKernelGGL(k_cx_emit, dim3(blocks_for(found, 4096)), dim3(kThreads), 0, st, found, (const uint64_t*) hit_sorted, (const uint32_t*) kind_sorted,
                         (uint4*) out);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    marks = 5;
    e = hipStreamSynchronize(st);  // sync 4: nothing of this call runs when its scratch goes
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (e == hipSuccess) ev.times(marks, report->ms);
  hipError_t fe = hipFree(blockA);
  const hipError_t fb = hipFree(blockB), fc = hipFree(blockC);
  if (fe == hipSuccess) fe = fb != hipSuccess ? fb : fc;
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
