// rj_simplify.hip -- thinning the chains of a map on the device (rj_simplify.h has the definition and the stages).
// Every kernel is a grid-stride loop over one of rj_simplify.h's per-element functions; rocPRIM does the one scan.  The
// pins of a closed chain are two reductions by one wave per chain (64 interior points a step, a butterfly of
// (128-bit value, index) pairs): no stage is serial in the points of a chain.  A round is three kernels: the weights of
// the round's points are stored, every candidate is decided from the stored weights and the links as they were, then
// the removed points are unlinked and the next round's work list is written -- the candidates that stayed and the
// unpinned neighbours of the removed points, each once (a round stamp per point, one atomicExch), appended with one
// atomic per wave (ballot and rank, as k_nd_cands appends).  The first round looks at every point; a later one at its
// list, so it costs what it has to look at, not np.  The host reads the round's two numbers (points removed, size of
// the next list) once per round: that sync ends the loop and sizes the next launch.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <string.h>

#include <chrono>

#include "rj_node.h"
#include "rj_pipeline.h"
#include "rj_simplify.h"

namespace rj {

using namespace simplify;

namespace {

// the best of the wave's 64 pairs, in every lane (`better` orders distinct points strictly: all lanes agree)
__device__ __forceinline__ Best wave_best(Best mine) {
  for (int d = 32; d >= 1; d >>= 1) {
    Best other;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = (uint32_t) __shfl_xor((int) (uint32_t) (mine.value >> (32 * k)), d, 64);
    other.value = ((u128) w[3] << 96) | ((u128) w[2] << 64) | ((u128) w[1] << 32) | w[0];
    other.index = (uint32_t) __shfl_xor((int) mine.index, d, 64);
    if (better(other, mine)) mine = other;
  }
  return mine;
}

__global__ __launch_bounds__(kThreads) void k_sp_check(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy, uint64_t np,
                                                       Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, crossings::check_row(c, row, nc, np));
  RJ_GRID_STRIDE(i, 2 * np) bad = max(bad, crossings::check_coordinate(xy[i]));
  if (bad) atomicMax(&meta->bad, bad);
}
// per point: live, pinned where it ends its chain; its links
__global__ __launch_bounds__(kThreads) void k_sp_links(const uint32_t* __restrict__ row, uint64_t nc, uint64_t np, uint8_t* __restrict__ flag,
                                                       uint32_t* __restrict__ prev, uint32_t* __restrict__ next, const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(p, np) {
    const uint64_t c = node::point_chain(p, row, nc), b = row[c], e = row[c + 1];
    flag[p] = chain_end(p, b, e) ? kLive | kPinned : kLive;
    links_of(p, b, e, &prev[p], &next[p]);
  }
}
// One wave per chain (behind k_sp_links: an interior point's flag is written by its chain's wave alone).
__global__ __launch_bounds__(kThreads) void k_sp_pins(const uint32_t* __restrict__ row, uint64_t nc, const int64_t* __restrict__ xy,
                                                      uint8_t* __restrict__ flag, Meta* meta) {
  if (meta->bad) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
  uint32_t closed = 0, extra = 0;
  for (uint64_t c = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) >> 6; c < nc; c += waves) {  // (wave-uniform)
    const uint64_t b = row[c], e = row[c + 1];
    if (!is_closed(b, e, xy)) continue;
    closed += lane == 0;
    Best m1 = no_best(), m2 = no_best();
    for (uint64_t q = b + 1 + lane; q + 1 < e; q += 64) {
      const Best v = far_of(b, q, xy);
      if (better(v, m1)) m1 = v;
    }
    m1 = wave_best(m1);
    if (!pins(m1)) continue;
    for (uint64_t q = b + 1 + lane; q + 1 < e; q += 64) {
      const Best v = wide_of(b, m1.index, q, xy);
      if (better(v, m2)) m2 = v;
    }
    m2 = wave_best(m2);
    if (lane == 0) {
      flag[m1.index] |= kPinned;
      extra++;
      if (pins(m2)) {
        flag[m2.index] |= kPinned;
        extra++;
      }
    }
  }
  count_to(&meta->counts.n_closed, closed);
  count_to(&meta->counts.n_pinned_extra, extra);
}

// item i of a round: the i-th point of its work list, or point i where the round looks at every point
__device__ __forceinline__ uint64_t item_of(const uint32_t* list, uint64_t i) { return list ? (uint64_t) list[i] : i; }

// the round's stored weights; its two numbers start at 0 (`into`: the list that k_sp_unlink will write)
__global__ __launch_bounds__(kThreads) void k_sp_weigh(const uint32_t* __restrict__ list, uint64_t n, const int64_t* __restrict__ xy,
                                                       const uint8_t* __restrict__ flag, const uint32_t* __restrict__ prev,
                                                       const uint32_t* __restrict__ next, uint64_t tol_lo, uint64_t tol_hi, u128* __restrict__ stored,
                                                       int into, Meta* meta) {
  if (meta->bad) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta->removed = 0;
    meta->n_list[into] = 0;
  }
  const u128 tol = tolerance(tol_lo, tol_hi);
  RJ_GRID_STRIDE(i, n) {
    const uint64_t p = item_of(list, i);
    stored[p] = stored_weight(p, xy, flag, prev, next, tol);
  }
}
__global__ __launch_bounds__(kThreads) void k_sp_decide(const uint32_t* __restrict__ list, uint64_t n, const u128* __restrict__ stored,
                                                        const uint32_t* __restrict__ prev, const uint32_t* __restrict__ next, uint8_t* __restrict__ goes,
                                                        const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, n) goes[i] = removes(item_of(list, i), stored, prev, next) ? 1 : 0;
}
// One thread per item, a wave's lanes on 64 consecutive items: a removed point is unlinked and offers its two
// neighbours to the next list, a candidate that stays offers itself; whoever stamps a point first appends it.  One
// atomic per wave; offer t of lane l goes behind the offers before t and the offers t of the lanes below l.
__global__ __launch_bounds__(kThreads) void k_sp_unlink(const uint32_t* __restrict__ list, uint64_t n, const uint8_t* __restrict__ goes, uint8_t* flag,
                                                        uint32_t* prev, uint32_t* next, u128* stored, uint32_t* stamp, uint32_t round,
                                                        uint32_t* __restrict__ out, uint64_t cap, int into, Meta* meta) {
  if (meta->bad) return;
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
  uint32_t removed = 0;
  for (uint64_t i0 = blockIdx.x * (uint64_t) blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (wave-uniform)
    const uint64_t i = i0 + lane;
    bool hit[3] = {false, false, false};
    uint32_t q[3] = {0, 0, 0};
    if (i < n) {
      const uint64_t p = item_of(list, i);
      if (goes[i]) {
        q[0] = prev[p];
        q[1] = next[p];
        unlink(p, flag, prev, next);
        stored[p] = kNoWeight;
        removed++;
        if (out) {
          hit[0] = needs_weight(q[0], flag) && atomicExch(&stamp[q[0]], round) != round;
          hit[1] = needs_weight(q[1], flag) && atomicExch(&stamp[q[1]], round) != round;
        }
      } else if (out && stored[p] != kNoWeight) {
        q[2] = (uint32_t) p;
        hit[2] = atomicExch(&stamp[p], round) != round;
      }
    }
    uint64_t hm[3];
    uint32_t total = 0;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      hm[t] = __ballot(hit[t]);
      total += (uint32_t) __popcll(hm[t]);
    }
    if (!total) continue;
    ull base = 0;
    if (lane == 0) base = atomicAdd((ull*) &meta->n_list[into], (ull) total);
    base = ((ull) __builtin_amdgcn_readfirstlane((uint32_t) (base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t) base);
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const ull pos = base + (ull) __popcll(hm[t] & ((1ull << lane) - 1));
      if (hit[t] && pos < cap) out[pos] = q[t];
      base += (ull) __popcll(hm[t]);
    }
  }
  count_to(&meta->removed, removed);
}

__global__ __launch_bounds__(kThreads) void k_sp_live(uint64_t np, const uint8_t* __restrict__ flag, uint32_t* __restrict__ keep, const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(p, np) keep[p] = is_live(p, flag);
}
__global__ void k_sp_totals(uint64_t np, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ slot, uint64_t capacity, Meta* meta) {
  if (meta->bad) return;
  totals(np, (uint64_t) slot[np - 1] + keep[np - 1], capacity, &meta->counts, &meta->emit);
}
// the scatter and the row: nothing is written unless the output fits
__global__ __launch_bounds__(kThreads) void k_sp_scatter(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                         const uint32_t* __restrict__ keep, const uint32_t* __restrict__ slot,
                                                         int64_t* __restrict__ out_xy, uint32_t* __restrict__ out_row, uint32_t* __restrict__ origin,
                                                         const Meta* meta) {
  if (meta->bad || !meta->emit) return;
  const uint64_t total = meta->counts.n_points;
  RJ_GRID_STRIDE(c, nc + 1) out_row[c] = (uint32_t) row_slot(c, row, nc, slot, total);
  RJ_GRID_STRIDE(p, np) {
    if (!keep[p]) continue;
    const uint64_t k = slot[p];
    out_xy[2 * k] = xy[2 * p];
    out_xy[2 * k + 1] = xy[2 * p + 1];
    if (origin) origin[k] = (uint32_t) p;
  }
}

}  // namespace

hipError_t map_simplify_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, uint64_t nc, uint64_t tol_lo, uint64_t tol_hi,
                               bool all_points, uint64_t capacity, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, Meta* result,
                               SimplifyReport* report) {
  memset(result, 0, sizeof(Meta));
  *report = SimplifyReport{};
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  char* block = nullptr;
  bool done = false;
  uint64_t n_rounds = 0, n_max_round = 0;
  do {
    Meta* meta;
    uint32_t *prev, *next, *stamp, *list[2];
    u128* stored;
    uint8_t *flag, *goes;
    void* temp;
    TempSize temp_size;
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, 0u, (size_t) np, rocprim::plus<uint32_t>(), st);
    });
    if ((e = temp_size.error) != hipSuccess) break;
    Carve S;
    auto carve = [&]() {
      S.used = 0;
      meta = S.take<Meta>(1);
      stored = S.take<u128>(np);
      prev = S.take<uint32_t>(np); next = S.take<uint32_t>(np); stamp = S.take<uint32_t>(np);
      list[0] = S.take<uint32_t>(np); list[1] = S.take<uint32_t>(np);
      flag = S.take<uint8_t>(np); goes = S.take<uint8_t>(np);
      temp = S.take<char>(temp_size.bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, S.used)) != hipSuccess) break;
    S.base = block;
    carve();
    // 1. the check
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_sp_check, dim3(blocks_for(2 * np > nc + 1 ? 2 * np : nc + 1, 2048)), dim3(kThreads), 0, st, row, nc, xy, np, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the links, the pins
    if ((e = hipMemsetAsync(stamp, 0, 4 * np, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_sp_links, dim3(blocks_for(np, 4096)), dim3(kThreads), 0, st, row, nc, np, flag, prev, next, (const Meta*) meta);
    hipLaunchKernelGGL(k_sp_pins, dim3(blocks_for(64 * nc, 4096)), dim3(kThreads), 0, st, row, nc, xy, flag, meta);
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    // 3. the rounds
    int cur = 0;
    uint64_t n = np;  // the round's items
    bool whole = true, bad = false;
    for (uint32_t round = 1; n; round++) {
      const auto t0 = std::chrono::steady_clock::now();
      const uint32_t* items = whole ? nullptr : list[cur];
      const int into = 1 - cur;
      const int blocks = blocks_for(n, 4096);
      hipLaunchKernelGGL(k_sp_weigh, dim3(blocks), dim3(kThreads), 0, st, items, n, xy, (const uint8_t*) flag, (const uint32_t*) prev, (const uint32_t*) next,
                         tol_lo, tol_hi, stored, into, meta);
      hipLaunchKernelGGL(k_sp_decide, dim3(blocks), dim3(kThreads), 0, st, items, n, (const u128*) stored, (const uint32_t*) prev, (const uint32_t*) next, goes,
                         (const Meta*) meta);
      hipLaunchKernelGGL(k_sp_unlink, dim3(blocks), dim3(kThreads), 0, st, items, n, (const uint8_t*) goes, flag, prev, next, stored, stamp, round,
                         all_points ? (uint32_t*) nullptr : list[into], np, into, meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
      if (round == 1 && (e = ev.mark(3, st)) != hipSuccess) break;
      if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // the round's sync: did it remove anything, how long is the next list
      report->n_syncs++;
      const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (round <= (uint32_t) SimplifyReport::kRounds) {
        report->round_list[round - 1] = n;
        report->round_ms[round - 1] = ms;
      } else {
        report->late_list += n;
        report->late_ms += ms;
        report->late_rounds++;
      }
      if (round > 1 && !all_points) {
        report->list_sum += n;
        report->list_max = n > report->list_max ? n : report->list_max;
      }
      if ((bad = result->bad != 0) || !result->removed) break;
      n_rounds++;
      n_max_round = result->removed > n_max_round ? result->removed : n_max_round;
      if (!all_points) {
        whole = false;
        cur = into;
        n = result->n_list[into] < np ? result->n_list[into] : np;
      }
    }
    if (e != hipSuccess) break;
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 4. the slots, the counts, the scatter (the two lists are free: the flags and their scan)
    uint32_t *keep = list[0], *slot = list[1];
    if (!bad) {
      hipLaunchKernelGGL(k_sp_live, dim3(blocks_for(np, 4096)), dim3(kThreads), 0, st, np, (const uint8_t*) flag, keep, (const Meta*) meta);
      size_t tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) keep, slot, 0u, (size_t) np, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_sp_totals, dim3(1), dim3(1), 0, st, np, (const uint32_t*) keep, (const uint32_t*) slot, capacity, meta);
      hipLaunchKernelGGL(k_sp_scatter, dim3(blocks_for(np > nc + 1 ? np : nc + 1, 4096)), dim3(kThreads), 0, st, xy, np, row, nc, (const uint32_t*) keep,
                         (const uint32_t*) slot, out_xy, out_row, origin, (const Meta*) meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the last sync: the counts, and nothing of this call runs when its scratch goes
    report->n_syncs++;
    done = e == hipSuccess;
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (done) {
    result->counts.n_rounds = n_rounds;
    result->counts.n_max_round = n_max_round;
    ev.times(5, report->ms);
  }
  const hipError_t fe = hipFree(block);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
