// rj_eliminate.hip -- merging sliver faces into a neighbour on the device (rj_eliminate.h has the definition and the
// stages).  The chain sums are the one pass over the points: a lane per point, 64 consecutive points per wave step, a
// run of consecutive steps per wave.  The wave finds the chain of its first point by one binary search of row_index;
// from there on each step loads the starts of the next 64 chains (a chain has a point or more: none further can begin
// inside the step), ORs the starts that fall inside the step into a 64-bit mask, and a lane's chain is a population
// count away -- no dependent loads per point.  The grid is up to 16 384 blocks of short runs, which the block scheduler
// balances: profiles/eliminate_fullsize.txt has the stage at grids from 256 to 65 536 blocks (flat from 1 536 on, but
// slower at 2 048, where 8 192 waves of 7 per SIMD leave a second, nearly empty round).
// A lane takes the edge to the next point (handed down by the next lane: every point is loaded once), and a segmented
// scan by chain over the wave leaves every chain's partial sums in its last lane.  A
// chain that lies inside the 64 points is stored as it is; only a chain that crosses the wave's range adds its partial
// sums to the zeroed accumulators, 64 bits at a time with the carry added to the high word -- integer sums commute, so
// the result does not depend on the order.  Millions of chains of 2..12 points cost no atomics but at the two ends of a
// wave step; one chain of 100 000 points costs one set per wave step.  Behind that pass every stage is over chain sides
// or faces: rocPRIM sorts and sums by key, and a grid-stride kernel per function of rj_eliminate.h.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <string.h>

#include "rj_eliminate.h"
#include "rj_node.h"
#include "rj_pipeline.h"

namespace rj {

using namespace eliminate;

namespace {

struct SumOp {
  __host__ __device__ U128 operator()(const U128& a, const U128& b) const { return rings::add(a, b); }
};
struct BestOp {
  __host__ __device__ Cand operator()(const Cand& a, const Cand& b) const { return best_of(a, b); }
};
struct SameFrom {
  __host__ __device__ bool operator()(const uint64_t& a, const uint64_t& b) const { return from_of(a) == from_of(b); }
};

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t) __builtin_amdgcn_readfirstlane((uint32_t) (v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t) v);
}
// A wave's share of the np points: a run of whole steps of 64 consecutive points, [*s0, *s1) in steps.  Runs, not a
// grid stride: a wave that knows the chain of its last point knows where the next step starts.
__device__ __forceinline__ void wave_steps(uint64_t np, uint64_t* s0, uint64_t* s1) {
  const uint64_t steps = (np + 63) / 64, waves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
  const uint64_t wave = uniform64((blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) >> 6), per = (steps + waves - 1) / waves;
  *s0 = wave * per < steps ? wave * per : steps;
  *s1 = *s0 + per < steps ? *s0 + per : steps;
}
// The chains of the 64 points from p0 on, *c0 the chain of p0 (the wave's one binary search, before its first step):
// lane j loads the start of chain *c0 + 1 + j -- 64 chains hold 64 points or more, so no later chain starts inside the
// step --, the starts inside the step become a 64-bit mask (OR over the wave), and the chain of point p0 + lane is *c0 +
// the starts in (p0, p0 + lane].  -> that chain, its first point and its end from the loaded starts; *c0 becomes the
// chain of p0 + 64.  All 64 lanes call.  Stays inside [0, nc) and reads row[0 .. nc] only, whatever row holds (the
// check of a malformed row may still be running: the sums are garbage then, and nothing reads them).
__device__ __forceinline__ uint32_t wave_chains(uint64_t p0, uint32_t lane, const uint32_t* __restrict__ row, uint64_t nc, uint64_t* c0, uint32_t* first,
                                                uint32_t* end) {
  const uint64_t base = *c0, idx = base + 1 + lane;
  const uint32_t start = idx <= nc ? row[idx] : 0xFFFFFFFFu;
  const uint64_t off = (uint64_t) start - p0;
  uint64_t mask = off < 64 ? 1ull << off : 0;
  for (int d = 32; d >= 1; d >>= 1) mask |= (uint64_t) __shfl_xor((long long) mask, d, 64);
  uint64_t c = base + (uint64_t) __popcll(mask & ((2ull << lane) - 1));
  c = c < nc ? c : nc - 1;
  const uint32_t k = (uint32_t) (c - base);  // (0 .. 63 on a map that passes the check)
  const uint32_t before = (uint32_t) __shfl((int) start, (int) ((k - 1) & 63), 64), behind = (uint32_t) __shfl((int) start, (int) (k & 63), 64);
  *first = k == 0 ? row[base] : before;
  *end = behind;
  const uint64_t c_last = (uint32_t) __shfl((int) (uint32_t) c, 63, 64), end_last = (uint32_t) __shfl((int) behind, 63, 64);
  const uint64_t next = p0 + 64 < end_last ? c_last : c_last + 1;
  *c0 = next < nc ? next : nc - 1;
  return (uint32_t) c;
}
// acc += v modulo 2^128, from any number of waves at once
__device__ __forceinline__ void atomic_add128(U128* acc, U128 v) {
  const ull old = atomicAdd((ull*) &acc->lo, (ull) v.lo);
  const ull carry = (ull) (old + v.lo) < (ull) v.lo ? 1 : 0;
  if (v.hi + carry) atomicAdd((ull*) &acc->hi, (ull) (v.hi + carry));
}

// 1. the check and the chain sums.  S, L: zeroed.
__global__ __launch_bounds__(kThreads) void k_el_sums(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                      U128* __restrict__ S, U128* __restrict__ L, Meta* meta) {
  const uint32_t lane = threadIdx.x & 63;
  const longlong2* __restrict__ P = reinterpret_cast<const longlong2*>(xy);
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, rings::check_row(c, row, nc, np));
  uint64_t s0, s1;
  wave_steps(np, &s0, &s1);
  uint64_t c0 = s0 < s1 ? uniform64(node::point_chain(64 * s0, row, nc)) : 0;
  for (uint64_t step = s0; step < s1; step++) {  // (wave-uniform)
    const uint64_t p0 = 64 * step, p = p0 + lane;
    const bool in = p < np;
    longlong2 a = make_longlong2(0, 0);
    if (in) a = P[p];
    bad = max(bad, max(rings::check_coordinate(a.x), rings::check_coordinate(a.y)));
    longlong2 b;
    b.x = __shfl_down(a.x, 1, 64);
    b.y = __shfl_down(a.y, 1, 64);
    if (lane == 63 && p + 1 < np) b = P[p + 1];
    uint32_t first, end;
    uint32_t c = wave_chains(p0, lane, row, nc, &c0, &first, &end);
    if (!in) c = kNone;
    U128 s{0, 0};
    uint64_t len = 0;
    if (in && p + 1 < (uint64_t) end && p + 1 < np) {  // the edge p -> p + 1 of chain c
      s = rings::limbs(edge_cross(a.x, a.y, b.x, b.y));
      len = edge_length(a.x, a.y, b.x, b.y);
    }
    // the segmented scan: equal chains are neighbours, so an equal chain d lanes down has only equal chains between
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t oc = (uint32_t) __shfl_up((int) c, d, 64);
      U128 os;
      os.lo = (uint64_t) __shfl_up((long long) s.lo, d, 64);
      os.hi = (uint64_t) __shfl_up((long long) s.hi, d, 64);
      const uint64_t ol = (uint64_t) __shfl_up((long long) len, d, 64);
      if (lane >= (uint32_t) d && oc == c) {
        s = rings::add(s, os);
        len += ol;
      }
    }
    const uint32_t nxt = (uint32_t) __shfl_down((int) c, 1, 64);
    if (in && (lane == 63 || nxt != c)) {  // the last lane of chain c in this wave: 64 lengths below 2^48 fit 64 bits
      if ((uint64_t) first >= p0 && (uint64_t) end <= p0 + 64) {
        S[c] = s;
        L[c] = U128{len, 0};
      } else {
        atomic_add128(&S[c], s);
        atomic_add128(&L[c], U128{len, 0});
      }
    }
  }
  if (bad) atomicMax(&meta->bad, bad);
}

// 2. the faces
__global__ __launch_bounds__(kThreads) void k_el_sides(const int32_t* __restrict__ left, const int32_t* __restrict__ right, uint64_t nc,
                                                       const U128* __restrict__ S, uint32_t* __restrict__ keys, U128* __restrict__ vals, const Meta* meta) {
  if (meta->bad) return;
  RJ_GRID_STRIDE(i, 2 * nc) {
    keys[i] = side_key(i, left, right);
    vals[i] = side_sum(i, S);
  }
}
__global__ void k_el_count_faces(const uint32_t* __restrict__ keys, Meta* meta) {
  if (meta->bad) return;
  meta->counts.n_faces = count_faces(meta->n_keys, keys);
}

// 3. the pairs and the choice
__global__ __launch_bounds__(kThreads) void k_el_directed(const int32_t* __restrict__ left, const int32_t* __restrict__ right, uint64_t nc,
                                                          const U128* __restrict__ L, const uint32_t* __restrict__ keys, uint64_t* __restrict__ dir,
                                                          U128* __restrict__ vals, const Meta* meta) {
  if (meta->bad) return;
  const uint64_t nf = meta->counts.n_faces;
  RJ_GRID_STRIDE(i, 2 * nc) {
    dir[i] = directed_key(i, left, right, keys, nf);
    vals[i] = L[i >> 1];
  }
}
// dir[n]: the unique directed keys, kNoPair behind the n_dir that there are
__global__ __launch_bounds__(kThreads) void k_el_cands(const uint64_t* __restrict__ dir, const U128* __restrict__ w, uint64_t n, Cand* __restrict__ cand,
                                                       const Meta* meta) {
  if (meta->bad) return;
  const uint64_t n_dir = meta->n_dir;
  RJ_GRID_STRIDE(i, n) cand[i] = i < n_dir && dir[i] != kNoPair ? cand_of(dir[i], w[i]) : Cand{0, 0, kNoPair, kNoPair};
}
// best: kNone everywhere
__global__ __launch_bounds__(kThreads) void k_el_best(const uint64_t* __restrict__ run, const Cand* __restrict__ won, uint32_t* __restrict__ best,
                                                      const Meta* meta) {
  if (meta->bad) return;
  const uint64_t nf = meta->counts.n_faces;
  RJ_GRID_STRIDE(i, meta->n_best) {
    const uint32_t f = from_of(run[i]);
    if (f != kNone && f < nf) best[f] = to_of(won[i].dir);
  }
}

// 4. the pointers
__global__ __launch_bounds__(kThreads) void k_el_first(const U128* __restrict__ area2, const uint32_t* __restrict__ best, uint64_t tol_lo, uint64_t tol_hi,
                                                       uint32_t* __restrict__ first, const Meta* meta) {
  if (meta->bad) return;
  const u128 tol = tolerance(tol_lo, tol_hi);
  RJ_GRID_STRIDE(k, meta->counts.n_faces) first[k] = first_pointer((uint32_t) k, is_sliver(value(area2[k]), tol), best);
}
__global__ __launch_bounds__(kThreads) void k_el_mutual(const uint32_t* __restrict__ first, const U128* __restrict__ area2, uint32_t* __restrict__ ptr,
                                                        Meta* meta) {
  if (meta->bad) return;
  uint32_t mutual = 0;
  RJ_GRID_STRIDE(k, meta->counts.n_faces) {
    bool counted;
    ptr[k] = settle_mutual((uint32_t) k, first, area2, &counted);
    mutual += counted;
  }
  count_to(&meta->counts.n_mutual, mutual);
}
// round r; nothing moved in the round before: done
__global__ __launch_bounds__(kThreads) void k_el_jump(uint32_t* ptr, int r, Meta* meta) {
  if (meta->bad || (r > 0 && !meta->changed[r - 1])) return;
  bool moved = false;
  RJ_GRID_STRIDE(k, meta->counts.n_faces) moved |= jump((uint32_t) k, ptr);
  if (moved) meta->changed[r] = 1;
}
__global__ __launch_bounds__(kThreads) void k_el_flags(const U128* __restrict__ area2, const uint32_t* __restrict__ best, const uint32_t* __restrict__ ptr,
                                                       uint64_t tol_lo, uint64_t tol_hi, uint32_t* __restrict__ flag, Meta* meta) {
  if (meta->bad) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) meta->unfinished = meta->changed[kMaxRounds - 1];
  const u128 tol = tolerance(tol_lo, tol_hi);
  uint32_t n[4] = {0, 0, 0, 0};
  RJ_GRID_STRIDE(k, meta->counts.n_faces) {
    const i128 a = value(area2[k]);
    const uint32_t f = flags_of((uint32_t) k, is_sliver(a, tol), is_negative(a), best, ptr);
    flag[k] = f;
    n[0] += (f & kSliver) != 0;
    n[1] += (f & kEliminated) != 0;
    n[2] += (f & kIsland) != 0;
    n[3] += (f & kNegative) != 0;
  }
  count_to(&meta->counts.n_slivers, n[0]);
  count_to(&meta->counts.n_eliminated, n[1]);
  count_to(&meta->counts.n_islands, n[2]);
  count_to(&meta->counts.n_negative, n[3]);
}

// 5. the new labels; under kDrop the keep flags and the points of the kept chains
__global__ __launch_bounds__(kThreads) void k_el_relabel(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                         const uint32_t* __restrict__ row, uint64_t nc, const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ ptr, bool drop, int32_t* __restrict__ new_left,
                                                         int32_t* __restrict__ new_right, uint32_t* __restrict__ keep, uint32_t* __restrict__ points,
                                                         Meta* meta) {
  if (meta->bad) return;
  const uint64_t nf = meta->counts.n_faces;
  uint32_t dropped = 0;
  RJ_GRID_STRIDE(c, nc) {
    const int32_t l = left[c], r = right[c], nl = target_label(l, keys, nf, ptr), nr = target_label(r, keys, nf, ptr);
    const bool stays = !drop || keeps(l, r, nl, nr);
    new_left[c] = nl;
    new_right[c] = nr;
    keep[c] = stays ? 1u : 0u;
    points[c] = stays ? row[c + 1] - row[c] : 0u;
    dropped += !stays;
  }
  count_to(&meta->counts.n_dropped, dropped);
}
// slot / offset: the exclusive scans of keep / points under kDrop, unused without
__global__ void k_el_totals(uint64_t np, uint64_t nc, bool drop, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ points,
                            const uint32_t* __restrict__ slot, const uint32_t* __restrict__ offset, bool records, uint64_t face_cap, uint64_t chain_cap,
                            uint64_t point_cap, Meta* meta) {
  if (meta->bad) return;
  meta->counts.n_chains = drop ? (uint64_t) slot[nc - 1] + keep[nc - 1] : nc;
  meta->counts.n_points = drop ? (uint64_t) offset[nc - 1] + points[nc - 1] : np;
  meta->emit = !meta->unfinished && fits(meta->counts, records, drop, face_cap, chain_cap, point_cap) ? 1 : 0;
}
__global__ __launch_bounds__(kThreads) void k_el_emit(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc, bool drop,
                                                      const uint32_t* __restrict__ keys, const U128* __restrict__ area2,
                                                      const uint32_t* __restrict__ flag, const uint32_t* __restrict__ best,
                                                      const uint32_t* __restrict__ ptr, const int32_t* __restrict__ new_left,
                                                      const int32_t* __restrict__ new_right, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ slot, const uint32_t* __restrict__ offset, Face* __restrict__ faces,
                                                      int32_t* __restrict__ out_left, int32_t* __restrict__ out_right, int64_t* __restrict__ out_xy,
                                                      uint32_t* __restrict__ out_row, uint32_t* __restrict__ origin, const Meta* meta) {
  if (meta->bad || !meta->emit) return;
  if (faces) RJ_GRID_STRIDE(k, meta->counts.n_faces) faces[k] = record_of((uint32_t) k, keys, area2, flag[k], best, ptr);
  RJ_GRID_STRIDE(c, nc) {
    if (!keep[c]) continue;
    const uint64_t k = drop ? slot[c] : c;
    out_left[k] = new_left[c];
    out_right[k] = new_right[c];
    if (drop) {
      out_row[k] = offset[c];
      if (origin) origin[k] = (uint32_t) c;
    }
  }
  if (!drop) return;
  // (a map that loses every chain fits capacities of 0, the sizing call's, whose arrays may be null: nothing to write then)
  if (blockIdx.x == 0 && threadIdx.x == 0 && out_row) out_row[meta->counts.n_chains] = (uint32_t) meta->counts.n_points;
  const uint32_t lane = threadIdx.x & 63;
  const longlong2* __restrict__ P = reinterpret_cast<const longlong2*>(xy);
  longlong2* __restrict__ Q = reinterpret_cast<longlong2*>(out_xy);
  uint64_t s0, s1;
  wave_steps(np, &s0, &s1);
  uint64_t c0 = s0 < s1 ? uniform64(node::point_chain(64 * s0, row, nc)) : 0;
  for (uint64_t step = s0; step < s1; step++) {  // (wave-uniform; the map has passed the check)
    const uint64_t p0 = 64 * step, p = p0 + lane;
    uint32_t first, end;
    const uint32_t c = wave_chains(p0, lane, row, nc, &c0, &first, &end);
    if (p < np && keep[c]) Q[(uint64_t) offset[c] + (p - first)] = P[p];
  }
}

}  // namespace

hipError_t map_eliminate_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                                uint64_t tol_lo, uint64_t tol_hi, uint32_t flags, uint64_t face_cap, uint64_t chain_cap, uint64_t point_cap, Face* faces,
                                int32_t* out_left, int32_t* out_right, int64_t* out_xy, uint32_t* out_row, uint32_t* origin, int point_blocks,
                                Meta* result, EliminateReport* report) {
  memset(result, 0, sizeof(Meta));
  *report = EliminateReport{};
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  const bool drop = (flags & kDrop) != 0;
  const uint64_t ns = 2 * nc;  // chain sides: the most faces, directed pairs and candidates there can be
  char* block = nullptr;
  bool done = false;
  do {
    Meta* meta;
    U128 *S, *L, *val_in, *val_out, *area2;
    uint32_t *key_in, *key_out, *keys, *best, *first, *ptr, *flag, *keep, *points, *slot, *offset;
    uint64_t *dir_in, *dir_out, *run;
    Cand *cand, *won;
    int32_t *new_left, *new_right;
    void* temp;
    TempSize temp_size;
    temp_size([&](size_t& b) {
      return rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (const U128*) nullptr, (U128*) nullptr, (size_t) ns, 0, 32,
                                       st);
    });
    temp_size([&](size_t& b) {
      return rocprim::reduce_by_key(nullptr, b, (const uint32_t*) nullptr, (const U128*) nullptr, (size_t) ns, (uint32_t*) nullptr, (U128*) nullptr,
                                    (uint64_t*) nullptr, SumOp(), rocprim::equal_to<uint32_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (const U128*) nullptr, (U128*) nullptr, (size_t) ns, 0, 64,
                                       st);
    });
    temp_size([&](size_t& b) {
      return rocprim::reduce_by_key(nullptr, b, (const uint64_t*) nullptr, (const U128*) nullptr, (size_t) ns, (uint64_t*) nullptr, (U128*) nullptr,
                                    (uint64_t*) nullptr, SumOp(), rocprim::equal_to<uint64_t>(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::reduce_by_key(nullptr, b, (const uint64_t*) nullptr, (const Cand*) nullptr, (size_t) ns, (uint64_t*) nullptr, (Cand*) nullptr,
                                    (uint64_t*) nullptr, BestOp(), SameFrom(), st);
    });
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, 0u, (size_t) nc, rocprim::plus<uint32_t>(), st);
    });
    if ((e = temp_size.error) != hipSuccess) break;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<Meta>(1);
      S = A.take<U128>(nc); L = A.take<U128>(nc);
      val_in = A.take<U128>(ns); val_out = A.take<U128>(ns); area2 = A.take<U128>(ns);
      key_in = A.take<uint32_t>(ns); key_out = A.take<uint32_t>(ns); keys = A.take<uint32_t>(ns);
      dir_in = A.take<uint64_t>(ns); dir_out = A.take<uint64_t>(ns); run = A.take<uint64_t>(ns);
      cand = A.take<Cand>(ns); won = A.take<Cand>(ns);
      best = A.take<uint32_t>(ns); first = A.take<uint32_t>(ns); ptr = A.take<uint32_t>(ns); flag = A.take<uint32_t>(ns);
      new_left = A.take<int32_t>(nc); new_right = A.take<int32_t>(nc);
      keep = A.take<uint32_t>(nc); points = A.take<uint32_t>(nc); slot = A.take<uint32_t>(nc); offset = A.take<uint32_t>(nc);
      temp = A.take<char>(temp_size.bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    const int side_blocks = blocks_for(ns, 4096), chain_blocks = blocks_for(nc, 4096);
    size_t tb;
    // 1. the check and the chain sums (the accumulators are one zeroed stretch: S, L)
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(S, 0, (size_t) ((char*) (L + nc) - (char*) S), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_el_sums, dim3(point_blocks > 0 ? point_blocks : blocks_for(np > nc + 1 ? np : nc + 1, 16384)), dim3(kThreads), 0, st, xy, np, row, nc, S, L, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the faces: the labels ascending, their areas
    hipLaunchKernelGGL(k_el_sides, dim3(side_blocks), dim3(kThreads), 0, st, left, right, nc, (const U128*) S, key_in, val_in, (const Meta*) meta);
    tb = temp_size.bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t*) key_in, key_out, (const U128*) val_in, val_out, (size_t) ns, 0, 32, st)) != hipSuccess) break;
    tb = temp_size.bytes;
    if ((e = rocprim::reduce_by_key(temp, tb, (const uint32_t*) key_out, (const U128*) val_out, (size_t) ns, keys, area2, &meta->n_keys, SumOp(),
                                    rocprim::equal_to<uint32_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_el_count_faces, dim3(1), dim3(1), 0, st, (const uint32_t*) keys, meta);
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    // 3. the directed pairs with their weights (the sums reuse the first sort's values), the best of every face
    hipLaunchKernelGGL(k_el_directed, dim3(side_blocks), dim3(kThreads), 0, st, left, right, nc, (const U128*) L, (const uint32_t*) keys, dir_in, val_in,
                       (const Meta*) meta);
    tb = temp_size.bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint64_t*) dir_in, dir_out, (const U128*) val_in, val_out, (size_t) ns, 0, 64, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(dir_in, 0xFF, 8 * ns, st)) != hipSuccess) break;  // (the unique keys go where the unsorted ones were: kNoPair behind them)
    tb = temp_size.bytes;
    if ((e = rocprim::reduce_by_key(temp, tb, (const uint64_t*) dir_out, (const U128*) val_out, (size_t) ns, dir_in, val_in, &meta->n_dir, SumOp(),
                                    rocprim::equal_to<uint64_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_el_cands, dim3(side_blocks), dim3(kThreads), 0, st, (const uint64_t*) dir_in, (const U128*) val_in, ns, cand, (const Meta*) meta);
    tb = temp_size.bytes;
    if ((e = rocprim::reduce_by_key(temp, tb, (const uint64_t*) dir_in, (const Cand*) cand, (size_t) ns, run, won, &meta->n_best, BestOp(), SameFrom(),
                                    st)) != hipSuccess)
      break;
    if ((e = hipMemsetAsync(best, 0xFF, 4 * ns, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_el_best, dim3(side_blocks), dim3(kThreads), 0, st, (const uint64_t*) run, (const Cand*) won, best, (const Meta*) meta);
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the pointers: mutual pairs settled, then jumping in place
    hipLaunchKernelGGL(k_el_first, dim3(side_blocks), dim3(kThreads), 0, st, (const U128*) area2, (const uint32_t*) best, tol_lo, tol_hi, first,
                       (const Meta*) meta);
    hipLaunchKernelGGL(k_el_mutual, dim3(side_blocks), dim3(kThreads), 0, st, (const uint32_t*) first, (const U128*) area2, ptr, meta);
    for (int r = 0; r < kMaxRounds; r++) hipLaunchKernelGGL(k_el_jump, dim3(side_blocks), dim3(kThreads), 0, st, ptr, r, meta);
    hipLaunchKernelGGL(k_el_flags, dim3(side_blocks), dim3(kThreads), 0, st, (const U128*) area2, (const uint32_t*) best, (const uint32_t*) ptr, tol_lo, tol_hi,
                       flag, meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 5. the new labels, what stays, the output
    hipLaunchKernelGGL(k_el_relabel, dim3(chain_blocks), dim3(kThreads), 0, st, left, right, row, nc, (const uint32_t*) keys, (const uint32_t*) ptr, drop,
                       new_left, new_right, keep, points, meta);
    if (drop) {
      tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) keep, slot, 0u, (size_t) nc, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
      tb = temp_size.bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint32_t*) points, offset, 0u, (size_t) nc, rocprim::plus<uint32_t>(), st)) != hipSuccess) break;
    }
    hipLaunchKernelGGL(k_el_totals, dim3(1), dim3(1), 0, st, np, nc, drop, (const uint32_t*) keep, (const uint32_t*) points, (const uint32_t*) slot,
                       (const uint32_t*) offset, faces != nullptr, face_cap, chain_cap, point_cap, meta);
    const uint64_t widest = drop && np > ns ? np : ns;
    hipLaunchKernelGGL(k_el_emit, dim3(point_blocks > 0 ? point_blocks : blocks_for(widest, 4096)), dim3(kThreads), 0, st, xy, np, row, nc, drop, (const uint32_t*) keys, (const U128*) area2,
                       (const uint32_t*) flag, (const uint32_t*) best, (const uint32_t*) ptr, (const int32_t*) new_left, (const int32_t*) new_right,
                       (const uint32_t*) keep, (const uint32_t*) slot, (const uint32_t*) offset, faces, out_left, out_right, out_xy, out_row, origin,
                       (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the one sync: the counts, and nothing of this call runs when its scratch goes
    done = e == hipSuccess;
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  if (done) ev.times(5, report->ms);
  const hipError_t fe = hipFree(block);
  return e != hipSuccess ? e : fe;
}

}  // namespace rj
