// rj_window.hip -- the device work of rj_window_query: a traversal of the 64-ary implicit LBVH of rj_device.h shaped for
// rectangles, with the exact predicate of rj_window.h, and the pipeline that makes a CSR of what it finds (rj_within.h:
// ORDER).  gfx950 only (wave = 64 lanes).
//
// k_window   This is not the walk of rj_distance_walk.h: there a lane is a point and the wave shares the walk.  A window
// returns tens to millions of edges; HERE A WAVE IS A WINDOW AND A LANE IS A CHILD OR A LEAF SLOT.
//   * A work item, one per wave at a time from a grid-stride loop, is (window, group of 64 consecutive entries of the start
//     level): the 64 boxes are one coalesced load and are tested against the window in one compare and one ballot, exactly
//     as the children of a node are further down.  (Per ENTRY of the start level a million small windows would pay up to 64
//     items each for one reject; per group they pay one.)  The start level: window_start_level, rj_window.h.
//   * An entry whose box lies INSIDE the window (window::box_inside) hands out its whole slot range with no test at all:
//     the lanes stride over the slots [idx 64^lvl, (idx + 1) 64^lvl), the padding test is box_empty on box0, every real slot
//     appends its key; the segments are never loaded.  An entry that OVERLAPS without being inside is pushed.
//   * The stack is k_pip's discipline (rj_device.h: kPipStack): pop one entry, push at most its 64 children, one level
//     lower.  Every push is checked against the capacity and raises kFaultWindowStack (-> RJ_E_INTERNAL) instead of writing
//     past the stack; the item is given up, and a call with such an item sorts and writes nothing.  The popped entry is
//     wave-uniform by readfirstlane.
//   * A popped leaf block: lane = slot.  A slot whose box lies inside is a hit without a test; one that overlaps loads its
//     segment T.sseg[slot] and runs window::meets.
//   * Hits go through the wave's staging buffer in LDS, flushed 64 keys at a time behind one atomic (within_flush's
//     shape); positions at or behind the capacity are counted, not written.  The counting call stages nothing.
//   * The per-window count is one integer atomicAdd per work item into cnt[w]: integer atomics only, so the counts -- and
//     behind the sort everything else -- are fully determined.
//
// BEHIND IT   what rj_within.hip does behind k_within, in a second copy (k_within's file and its resource report stay as
// they are): an exclusive scan of the counts gives the offsets, a small reduction the windows hit and the longest list; the
// counting call and an overflow end there.  Otherwise a radix sort of the keys over [0, key_bits(nw)) and k_window_out,
// one pair per lane: the eid is the key's low word, the flags are recomputed from the segment in eid order and the window.
//
// No result depends on the grid, the start level, the shortcut, which wave takes which item or the order of the leaves:
// the set of keys is the set of pairs that pass the exact test or lie below a box inside the window (rj_window.h:
// box_inside, where they pass it too), and a sorted set has one order.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "rj_window.h"

namespace rj {

using namespace window;

namespace {

constexpr int kWindowWaves = 4;    // waves per block
constexpr int kWindowStage = 128;  // keys of the staging buffer: below 64 in front of a step, at most 64 more behind it

struct WindowWaveLds {  // 4 bytes per stack entry and 8 per key: 2304 B per wave
  uint32_t code[kPipStack];  // level << 28 | index
  uint64_t keys[kWindowStage];
};

struct WindowMeta {
  unsigned long long appended;  // what the flushes counted
  unsigned long long n_windows_hit, max_per_window;
  unsigned long long gave_up;  // items given up at a push that the stack had no room for: nothing is sorted or written
};

struct WindowKernelArgs {
  WindowArgs a;
  uint32_t* cnt;   // [nw], zeroed
  uint64_t* keys;  // [capacity], null in the counting call
  WindowMeta* meta;
  int level;       // the start level, in [1, top]
  uint64_t groups; // ceil(nlvl[level] / 64)
};

__device__ __noinline__ void window_raise_fault(uint32_t* word) {
  // a plain store (idempotent), not an atomic: the word is pinned host memory the device writes directly
  __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) (uint32_t) (v >> 32)) << 32) |
         (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) (uint32_t) v);
}

// the top n (<= 64) keys of the wave's staging buffer go out behind ONE atomic; a position at or behind the capacity is
// counted and not written
__device__ __forceinline__ void window_flush(WindowWaveLds& L, int& nk, int n, unsigned long long* counter, uint64_t* keys, uint64_t cap, int lane) {
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(counter, (unsigned long long) n);
  base = uniform64(base);
  if (lane < n) {
    const uint64_t k = L.keys[nk - n + lane];
    const unsigned long long pos = base + (unsigned long long) lane;
    if (pos < cap) keys[pos] = k;
  }
  nk -= n;
  wave_lds_fence();
}

template <bool STATS>
__global__ __launch_bounds__(64 * kWindowWaves) void k_window(WindowKernelArgs K) {
  __shared__ WindowWaveLds lds[kWindowWaves];
  const WindowArgs& A = K.a;
  const DeviceBvh& T = A.bvh;
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  WindowWaveLds& L = lds[wib];
  const int stack_cap = STATS && A.stack_cap < kPipStack ? A.stack_cap : kPipStack;  // (lowered only by tests of the fault path)
  const bool filling = K.keys != nullptr;
  const uint64_t slots = (uint64_t) T.nlvl[1] * 64;  // the slots of the real leaf blocks (padding inside them: the empty box)
  const uint64_t items = A.nw * K.groups;
  unsigned long long st_nodes = 0, st_leaf = 0, st_exact = 0, st_inside = 0, st_pairs = 0;
  int nk = 0;  // wave-uniform fill of L.keys

  for (uint64_t it = (uint64_t) blockIdx.x * kWindowWaves + wib; it < items; it += (uint64_t) gridDim.x * kWindowWaves) {
    const uint64_t item = uniform64(it);
    const uint64_t w = item / K.groups, g = item - w * K.groups;
    Win W = {A.win[4 * w], A.win[4 * w + 1], A.win[4 * w + 2], A.win[4 * w + 3]};
    if (!normalise(&W)) continue;
    const QWin Q = quantise(W);
    uint32_t count = 0;  // wave-uniform: the pairs of this item
    int sp = 0;
    bool gave_up = false;

    // the lanes with `hit` append (window, eid)
    auto append = [&](bool hit, uint32_t eid) {
      const uint64_t hm = __ballot(hit);
      if (!hm) return;
      const int n = __popcll(hm);
      count += (uint32_t) n;
      if (!filling) return;
      if (hit) L.keys[nk + rank_below(hm)] = within::pair_key((uint32_t) w, eid);
      nk += n;
      wave_lds_fence();
      if (STATS) st_pairs += (unsigned long long) n;
      if (nk >= 64) window_flush(L, nk, 64, &K.meta->appended, K.keys, A.capacity, lane);
    };
    // every real slot of [first, end): below a box inside the window
    auto hand_out = [&](uint64_t first, uint64_t end) {
      end = end < slots ? end : slots;
      for (uint64_t base = first; base < end; base += 64) {
        const uint64_t slot = base + lane;
        bool real = false;
        uint32_t eid = 0;
        if (slot < end) {
          const QBox b = T.box0[slot];
          real = !nearest::box_empty(b.x0, b.x1);
          if (real) eid = T.seid[slot];
        }
        if (STATS) st_inside += (unsigned long long) __popcll(__ballot(real));
        append(real, eid);
      }
    };
    // 64 entries of level lvl >= 1 from index `first` (lane = entry; b: this lane's box, have: it exists): those inside
    // the window are handed out, those that overlap it otherwise go onto the stack
    auto take_entries = [&](int lvl, uint32_t first, const QBox& b, bool have) {
      const bool ov = have && box_overlaps(b.x0, b.y0, b.x1, b.y1, Q);
      const bool in = ov && A.contained && box_inside(b.x0, b.y0, b.x1, b.y1, Q);
      const uint64_t keep = __ballot(ov && !in);
      const int n = __popcll(keep);
      if (sp + n > stack_cap) {
        if (lane == 0) {
          window_raise_fault(A.fault + kFaultWindowStack);
          atomicAdd(&K.meta->gave_up, 1ull);
        }
        gave_up = true;
        return;
      }
      if (ov && !in) L.code[sp + rank_below(keep)] = ((uint32_t) lvl << 28) | (first + (uint32_t) lane);
      sp += n;
      wave_lds_fence();
      const int shift = 6 * lvl;  // an entry of level lvl covers 64^lvl slots
      for (uint64_t im = __ballot(in); im; im &= im - 1) {
        const uint64_t idx = (uint64_t) first + (uint64_t) __builtin_ctzll(im);
        hand_out(idx << shift, (idx + 1) << shift);
      }
    };

    if (STATS) st_nodes++;
    {
      const uint64_t at = g * 64 + lane;
      const bool have = at < T.nlvl[K.level];
      QBox b = {kEmptyMin, kEmptyMin, kEmptyMax, kEmptyMax};
      if (have) b = T.lvl[K.level][at];
      take_entries(K.level, (uint32_t) (g * 64), b, have);
    }
    while (sp > 0 && !gave_up) {
      --sp;
      const uint32_t e = (uint32_t) __builtin_amdgcn_readfirstlane((int32_t) L.code[sp]);
      const int lvl = (int) (e >> 28);
      const uint32_t idx = e & 0x0FFFFFFFu;
      if (lvl > 1) {
        if (STATS) st_nodes++;
        take_entries(lvl - 1, idx * 64u, T.lvl[lvl - 1][(uint64_t) idx * 64 + lane], true);
        continue;
      }
      // a leaf block: lane = slot
      if (STATS) st_leaf++;
      const uint64_t slot = (uint64_t) idx * 64 + lane;
      const QBox b = T.box0[slot];
      const bool ov = box_overlaps(b.x0, b.y0, b.x1, b.y1, Q);
      const bool in = ov && A.contained && box_inside(b.x0, b.y0, b.x1, b.y1, Q);
      bool hit = in;
      if (ov && !in) {
        uint32_t flags;
        hit = meets(T.sseg[slot], W, &flags);
      }
      if (STATS) st_exact += (unsigned long long) __popcll(__ballot(ov && !in)), st_inside += (unsigned long long) __popcll(__ballot(in));
      uint32_t eid = 0;
      if (hit) eid = T.seid[slot];
      append(hit, eid);
    }
    if (lane == 0 && count) atomicAdd(&K.cnt[w], count);
  }
  if (nk > 0) window_flush(L, nk, nk, &K.meta->appended, K.keys, A.capacity, lane);
  if (STATS && lane == 0 && A.stats) {
    atomicAdd(&A.stats[0], st_nodes);
    atomicAdd(&A.stats[1], st_leaf);
    atomicAdd(&A.stats[2], st_exact);
    atomicAdd(&A.stats[3], st_inside);
    atomicAdd(&A.stats[4], st_pairs);
  }
}

// the windows with a list and the longest list: one atomic each per block
__global__ __launch_bounds__(kThreads) void k_window_totals(const uint32_t* __restrict__ cnt, uint64_t n, WindowMeta* meta) {
  __shared__ uint32_t longest[kThreads / 64];
  uint32_t hit = 0, most = 0;
  RJ_GRID_STRIDE(i, n) {
    const uint32_t c = cnt[i];
    hit += c ? 1u : 0u;
    most = c > most ? c : most;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t) __shfl_down(most, d, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0) longest[threadIdx.x >> 6] = most;
  const uint32_t sum = block_sum(hit);  // (its barrier also publishes `longest`)
  if (threadIdx.x == 0) {
    for (int w = 0; w < kThreads / 64; w++) most = longest[w] > most ? longest[w] : most;
    if (sum) atomicAdd(&meta->n_windows_hit, (unsigned long long) sum);
    if (most) atomicMax(&meta->max_per_window, (unsigned long long) most);
  }
}

// one pair per lane: the eid, and the flags from the base map's segment in eid order and the window
__global__ __launch_bounds__(kThreads) void k_window_out(const uint64_t* __restrict__ sorted, uint64_t n_pairs, const Seg* __restrict__ seg,
                                                          const int64_t* __restrict__ win, uint32_t* __restrict__ eid, uint8_t* __restrict__ flags) {
  RJ_GRID_STRIDE(k, n_pairs) {
    const uint64_t key = sorted[k];
    const uint32_t e = within::key_eid(key);
    const uint64_t w = within::key_point(key);
    eid[k] = e;
    if (flags) {
      Win W = {win[4 * w], win[4 * w + 1], win[4 * w + 2], win[4 * w + 3]};
      flags[k] = normalise(&W) ? (uint8_t) end_flags(seg[e], W) : (uint8_t) 0;  // (a window with a pair is never empty)
    }
  }
}

}  // namespace

hipError_t window_device(hipStream_t st, const WindowArgs& a, bool stats, int blocks, int cus, StageEvents* ev, WindowResult* result) {
  *result = WindowResult{};
  const uint64_t n = a.nw, cap = a.capacity;
  char *block = nullptr, *sort_block = nullptr;
  hipError_t e = hipSuccess;
  do {
    // what is sized by the windows and by the capacity
    TempSize scan_temp;
    scan_temp([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), st);
    });
    if ((e = scan_temp.error) != hipSuccess) break;
    WindowMeta* meta;
    uint32_t* cnt;
    uint64_t *scanned, *keys;
    void* temp;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<WindowMeta>(1);
      cnt = A.take<uint32_t>(n + 1);
      scanned = A.take<uint64_t>(n + 1);
      temp = A.take<char>(scan_temp.bytes);
      keys = A.take<uint64_t>(cap);  // (the counting call: none)
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    // 1. the traversal
    if ((e = ev->mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(WindowMeta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(cnt, 0, (n + 1) * sizeof(uint32_t), st)) != hipSuccess) break;
    if (n) {
      const uint64_t waves = (uint64_t) (cus > 0 ? cus : 256) * 16;  // (four waves per SIMD)
      int level = a.start_level > 0 ? a.start_level : window_start_level(a.bvh, n, waves);
      level = level > a.bvh.top ? a.bvh.top : (level < 1 ? 1 : level);
      WindowKernelArgs K{a, cnt, cap ? keys : nullptr, meta, level, ((uint64_t) a.bvh.nlvl[level] + 63) / 64};
      // by size (blocks <= 0): a block per four items up to 16 blocks per CU; the grid-stride loop takes what is left
      const uint64_t items = n * K.groups, full = (items + kWindowWaves - 1) / kWindowWaves;
      uint64_t grid = blocks > 0 ? (uint64_t) blocks : (uint64_t) (cus > 0 ? cus : 256) * 16;
      if (grid > full) grid = full;
      if (K.groups) {
        if (stats)
          hipLaunchKernelGGL(k_window<true>, dim3((uint32_t) grid), dim3(64 * kWindowWaves), 0, st, K);
        else
          hipLaunchKernelGGL(k_window<false>, dim3((uint32_t) grid), dim3(64 * kWindowWaves), 0, st, K);
        if ((e = hipGetLastError()) != hipSuccess) break;
      }
    }
    if ((e = ev->mark(1, st)) != hipSuccess) break;
    // 2. the offsets and the counts
    size_t tb = scan_temp.bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) cnt, scanned, (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), st)) != hipSuccess) break;
    if (n) {
      hipLaunchKernelGGL(k_window_totals, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, (const uint32_t*) cnt, n, meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    WindowMeta m;
    uint64_t n_pairs = 0;
    if ((e = hipMemcpyAsync(&m, meta, sizeof(m), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(&n_pairs, scanned + n, sizeof(n_pairs), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    if (a.offsets && (e = hipMemcpyAsync(a.offsets, scanned, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // the first sync: how many pairs there are
    result->counts = Counts{n_pairs, m.n_windows_hit, m.max_per_window};
    result->appended = cap ? m.appended : n_pairs;
    // 3. the sort and the outputs
    if (cap && n_pairs <= cap && result->appended == n_pairs && !m.gave_up) {
      if (n_pairs) {
        const int bits = within::key_bits(n);
        TempSize sort_temp;
        sort_temp([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) n_pairs, 0, bits, st); });
        if ((e = sort_temp.error) != hipSuccess) break;
        uint64_t* sorted;
        void* stemp;
        Carve B;
        auto carve_sort = [&]() {
          B.used = 0;
          sorted = B.take<uint64_t>(n_pairs);
          stemp = B.take<char>(sort_temp.bytes);
        };
        carve_sort();
        if ((e = hipMalloc((void**) &sort_block, B.used)) != hipSuccess) break;
        B.base = sort_block;
        carve_sort();
        tb = sort_temp.bytes;
        if ((e = rocprim::radix_sort_keys(stemp, tb, (const uint64_t*) keys, sorted, (size_t) n_pairs, 0, bits, st)) != hipSuccess) break;
        hipLaunchKernelGGL(k_window_out, dim3(blocks_for(n_pairs, 4096)), dim3(kThreads), 0, st, (const uint64_t*) sorted, n_pairs, a.seg, a.win, a.eid, a.flags);
        if ((e = hipGetLastError()) != hipSuccess) break;
      }
      result->emitted = true;
    }
    if ((e = ev->mark(2, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the last sync: nothing of this call runs when its scratch goes
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  const hipError_t fa = hipFree(block), fb = hipFree(sort_block);
  return e != hipSuccess ? e : (fa != hipSuccess ? fa : fb);
}

}  // namespace rj
