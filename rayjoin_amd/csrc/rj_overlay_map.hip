// rj_overlay_map.hip -- the overlay's output map on the device (rj_overlay_map.h has the semantics and the per-edge
// rule), and the checks of a map that arrives in device memory (rj_upload_map_dev).
//   1. k_ovm_emit<false>  one lane per edge, 64 consecutive edges per wave, the wave-wide record search of the face table:
//                         the points and the pieces each wave emits, both maps' waves in one array.
//   2. rocPRIM exclusive scan of (points, pieces) over the waves: every wave's first slots.  No atomics for slots.
//   3. k_ovm_emit<true>   the same rule again, storing: a point at its slot, a piece's first slot (its row_index entry),
//                         its origin and its two face keys ((face 0 << 32) | face 1 per side, kNoKey without a face).
//   4. rocPRIM radix sort + unique of the keys: the unique keys are face_pairs, a side's id is its key's rank + 1.
//   5. k_ovm_label        left / right of every piece by binary search, face_pairs, the counts.
// RJ_OVM_DROP_DEGENERATE: 3 stores into scratch (with the piece of every point), k_ovm_keep flags the pieces with at
// least two points, a second scan gives the kept pieces their slots, k_ovm_label / k_ovm_compact_points move them out.
// RJ_OVM_MERGE_PIECES (rj_overlay_map.h: pieces_join) takes the same staging: k_ovm_join gives every staged piece
// (points it adds, 1 when it starts a chain) -- with RJ_OVM_DROP_DEGENERATE against the kept piece before it, which a
// max-scan of the kept pieces' indices finds --, one scan of those gives a piece its chain and its first point slot,
// k_ovm_merge_label / k_ovm_merge_points move the run starts and the points out: once, whether or not pieces are dropped.
// rj_overlay_map_op runs the same passes with k_ovm_emit_op: the body of k_ovm_emit with the pieces and the face keys of an
// overlay operation (rj_overlay_ops.h) in place of the intersection's; the operation is a kernel argument.
// No host loop over edges, pieces or records; the host reads the three counts at the end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/rayjoin_amd.h"
#include "rj_kernels.h"
#include "rj_overlay_map.h"
#include "rj_overlay_dev.h"
#include "rj_overlay_ops.h"
#include "rj_pipeline.h"

namespace rj {

using namespace overlay;

namespace {

struct Slots {
  uint64_t points, chains;
};
struct SlotsSum {
  __host__ __device__ Slots operator()(const Slots& a, const Slots& b) const { return Slots{a.points + b.points, a.chains + b.chains}; }
};

// where the emit pass stores: the caller's arrays, or scratch with room for everything when pieces are dropped later
struct Stage {
  int64_t* xy;
  uint32_t *row, *origin, *point_piece;  // (origin, point_piece: may be null)
  uint64_t* keys;                        // two per piece, room for every piece
  uint64_t point_cap, chain_cap;
};

// which pieces an edge emits and the keys of their sides: the intersection's hard-wired rule (rj_overlay_map.h) for
// rj_overlay_map, an operation (rj_overlay_ops.h) for rj_overlay_map_op.  The operation lives in scalar registers.
struct RuleIntersection {
  template <class S, class P>
  __device__ __forceinline__ void edge(int im, uint64_t e, uint32_t c, uint64_t lo, uint64_t hi, int32_t tail, const int64_t* pts,
                                       const uint32_t* edge_begin, const int32_t* left, const int32_t* right, const Rec48* xs,
                                       const int32_t* vertex_face, S&& start, P&& point) const {
    edge_emit(im, e, c, lo, hi, tail, pts, edge_begin, left, right, xs, vertex_face, start, point);
  }
  __device__ __forceinline__ uint64_t key(int im, int32_t mine, int32_t label) const { return side_key(im, mine, label); }
};
struct RuleOp {
  Op op;
  template <class S, class P>
  __device__ __forceinline__ void edge(int im, uint64_t e, uint32_t c, uint64_t lo, uint64_t hi, int32_t tail, const int64_t* pts,
                                       const uint32_t* edge_begin, const int32_t* left, const int32_t* right, const Rec48* xs,
                                       const int32_t* vertex_face, S&& start, P&& point) const {
    edge_emit(im, e, c, lo, hi, tail, pts, edge_begin, left, right, xs, vertex_face, op, start, point);
  }
  __device__ __forceinline__ uint64_t key(int im, int32_t mine, int32_t label) const { return side_key(im, mine, label, op); }
};

// kWrite 0: (points, pieces) of each wave to wave_count; 1: store from wave_base.  Every lane of a wave runs the loop
// body the same number of times (lanes beyond ne emit nothing).
// (nwaves, wave0, wstride come from the kernel: with blockDim / gridDim read here the compiler fetched the launch
//  geometry the generic way and the intersection's kernels lost 0.1 ms of 1.56 on 30.8 M edges)
template <bool kWrite, class Rule>
__device__ __forceinline__ void ovm_emit(const Rule rule, uint64_t nwaves, uint64_t wave0, uint64_t wstride, int im,
                                         const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                         const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                         const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs, uint64_t n,
                                         const int32_t* __restrict__ vertex_face, Slots* __restrict__ wave_count,
                                         const Slots* __restrict__ wave_base, const Stage& out) {
  const int lane = threadIdx.x & 63;
  for (uint64_t w = wave0; w < nwaves; w += wstride) {
    const uint64_t e0 = w * 64, e_end = e0 + 64 < ne ? e0 + 64 : ne;
    const uint64_t e = e0 + lane;
    const bool valid = e < ne;
    const uint64_t wlo = wave_first_record(xs, n, im, e0, lane), whi = wave_first_record(xs, n, im, e_end, lane);
    uint32_t c = 0;
    uint64_t lo = wlo, hi = wlo;
    int32_t tail = 0;
    uint64_t m = 0;  // points in the low word, pieces in the high word (both below 2^32 over a whole map)
    if (valid) {
      c = edge_chain[e];
      lo = first_record_at(xs, wlo, whi, im, e);
      hi = first_record_at(xs, lo, whi, im, e + 1);
      tail = tail_label(xs, n, im, hi, c, edge_begin, vertex_face);
      rule.edge(im, e, c, lo, hi, tail, pts, edge_begin, left, right, xs, vertex_face, [&](int32_t) { m += 1ull << 32; },
                [&](int64_t, int64_t) { m += 1; });
    }
    uint64_t incl = m;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t u = (uint64_t) __shfl_up((long long) incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (!kWrite) {
      if (lane == 63) wave_count[w] = Slots{incl & 0xFFFFFFFFull, incl >> 32};
      continue;
    }
    if (!m) continue;
    const Slots base = wave_base[w];
    uint64_t pslot = base.points + ((incl - m) & 0xFFFFFFFFull), cslot = base.chains + ((incl - m) >> 32);
    const int32_t l = left[c], r = right[c];
    rule.edge(
        im, e, c, lo, hi, tail, pts, edge_begin, left, right, xs, vertex_face,
        [&](int32_t label) {
          if (cslot < out.chain_cap) {
            out.row[cslot] = (uint32_t) pslot;
            if (out.origin) out.origin[cslot] = ((uint32_t) im << 31) | c;
          }
          out.keys[2 * cslot] = rule.key(im, l, label);  // (cslot < max_pieces of both maps: the buffer's size)
          out.keys[2 * cslot + 1] = rule.key(im, r, label);
          cslot++;
        },
        [&](int64_t x, int64_t y) {
          if (pslot < out.point_cap) {
            out.xy[2 * pslot] = x;
            out.xy[2 * pslot + 1] = y;
            if (out.point_piece) out.point_piece[pslot] = (uint32_t) (cslot - 1);
          }
          pslot++;
        });
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_ovm_emit(int im, const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                                       const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                                       const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs,
                                                       uint64_t n, const int32_t* __restrict__ vertex_face, Slots* __restrict__ wave_count,
                                                       const Slots* __restrict__ wave_base, Stage out) {
  const uint64_t nwaves = (ne + 63) / 64;
  const uint64_t wave0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / 64;
  const uint64_t wstride = (uint64_t) gridDim.x * blockDim.x / 64;
  ovm_emit<kWrite>(RuleIntersection{}, nwaves, wave0, wstride, im, pts, edge_chain, edge_begin, left, right, ne, xs, n, vertex_face,
                   wave_count, wave_base, out);
}

// the same pass under an operation (rj_overlay_map_op): how / by are kernel arguments
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_ovm_emit_op(int im, const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                                          const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                                          const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs,
                                                          uint64_t n, const int32_t* __restrict__ vertex_face, Slots* __restrict__ wave_count,
                                                          const Slots* __restrict__ wave_base, Stage out, uint32_t how, uint32_t by) {
  const uint64_t nwaves = (ne + 63) / 64;
  const uint64_t wave0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / 64;
  const uint64_t wstride = (uint64_t) gridDim.x * blockDim.x / 64;
  ovm_emit<kWrite>(RuleOp{make_op(how, by)}, nwaves, wave0, wstride, im, pts, edge_chain, edge_begin, left, right, ne, xs, n, vertex_face,
                   wave_count, wave_base, out);
}

// totals[0] = every wave's points and pieces; the sentinel of the staged row array
__global__ void k_ovm_totals(const Slots* __restrict__ wave_count, const Slots* __restrict__ wave_base, uint64_t nwaves, Slots* totals,
                             Stage out) {
  Slots t{0, 0};
  if (nwaves) t = SlotsSum()(wave_base[nwaves - 1], wave_count[nwaves - 1]);
  *totals = t;
  if (out.row && t.chains <= out.chain_cap) out.row[t.chains] = (uint32_t) t.points;  // (a sizing call has no arrays)
}

__device__ __forceinline__ uint64_t face_count(const uint64_t* ukeys, uint64_t nu) { return nu && ukeys[nu - 1] == kNoKey ? nu - 1 : nu; }
__device__ __forceinline__ int32_t face_id(const uint64_t* ukeys, uint64_t nf, uint64_t key) {
  return key == kNoKey ? 0 : (int32_t) (key_index(ukeys, nf, key) + 1);
}

// per staged piece: (its points, 1) when it stays, (0, 0) when it has fewer than two points; zeros beyond the pieces
__global__ __launch_bounds__(kThreads) void k_ovm_keep(const uint32_t* __restrict__ row, const Slots* __restrict__ totals, uint64_t bound,
                                                       Slots* __restrict__ kept) {
  const uint64_t nch = totals->chains;
  RJ_GRID_STRIDE(i, bound) {
    const uint64_t len = i < nch ? (uint64_t) (row[i + 1] - row[i]) : 0;
    kept[i] = len >= 2 ? Slots{len, 1} : Slots{0, 0};
  }
}

// left / right of every piece, face_pairs, the three counts.  kept == null: the pieces are where the emit pass stored
// them (row_index and origin too); else piece i moves to kept_base[i] when kept[i].chains.
__global__ __launch_bounds__(kThreads) void k_ovm_label(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ ukeys,
                                                        const uint64_t* __restrict__ n_unique, const Slots* __restrict__ totals,
                                                        const uint32_t* __restrict__ staged_row, const uint32_t* __restrict__ staged_origin,
                                                        const Slots* __restrict__ kept, const Slots* __restrict__ kept_base, OverlayMapOut out,
                                                        uint64_t* __restrict__ counts) {
  const uint64_t nf = face_count(ukeys, *n_unique), nch = totals->chains;
  const uint64_t i0 = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x, stride = (uint64_t) gridDim.x * blockDim.x;
  if (i0 == 0) {
    Slots t = *totals;
    if (kept) {
      t = nch ? SlotsSum()(kept_base[nch - 1], kept[nch - 1]) : Slots{0, 0};
      if (out.row_index && t.chains <= out.chain_cap) out.row_index[t.chains] = (uint32_t) t.points;
    }
    counts[0] = t.chains;
    counts[1] = t.points;
    counts[2] = nf;
  }
  for (uint64_t i = i0; i < nch; i += stride) {
    uint64_t to = i;
    if (kept) {
      if (!kept[i].chains) continue;
      to = kept_base[i].chains;
    }
    if (to >= out.chain_cap) continue;
    out.left[to] = face_id(ukeys, nf, keys[2 * i]);
    out.right[to] = face_id(ukeys, nf, keys[2 * i + 1]);
    if (kept) {
      out.row_index[to] = (uint32_t) kept_base[i].points;
      if (out.origin) out.origin[to] = staged_origin[i];
    }
  }
  const uint64_t lim = nf < out.face_cap ? nf : out.face_cap;
  for (uint64_t i = i0; i < lim; i += stride) {
    out.face_pairs[2 * i] = (int32_t) (uint32_t) (ukeys[i] >> 32);
    out.face_pairs[2 * i + 1] = (int32_t) (uint32_t) ukeys[i];
  }
}

// the points of the kept pieces, to their places
__global__ __launch_bounds__(kThreads) void k_ovm_compact_points(const int64_t* __restrict__ staged_xy, const uint32_t* __restrict__ staged_row,
                                                                 const uint32_t* __restrict__ point_piece, const Slots* __restrict__ totals,
                                                                 const Slots* __restrict__ kept, const Slots* __restrict__ kept_base,
                                                                 int64_t* __restrict__ xy, uint64_t point_cap) {
  const uint64_t np = totals->points;
  RJ_GRID_STRIDE(j, np) {
    const uint32_t i = point_piece[j];
    if (!kept[i].chains) continue;
    const uint64_t to = kept_base[i].points + (j - staged_row[i]);
    if (to < point_cap) {
      xy[2 * to] = staged_xy[2 * j];
      xy[2 * to + 1] = staged_xy[2 * j + 1];
    }
  }
}

// ---- RJ_OVM_MERGE_PIECES ------------------------------------------------------------------------------------------
// staged piece i -> i + 1 when RJ_OVM_DROP_DEGENERATE keeps it, else 0: the exclusive max-scan of these is, per piece,
// 1 + the kept piece before it (0: none)
struct KeptIndex {
  const uint32_t* row;
  const Slots* totals;
  __host__ __device__ uint32_t operator()(uint32_t i) const {
    return (uint64_t) i < totals->chains && row[i + 1] - row[i] >= 2 ? i + 1 : 0;
  }
};
using KeptIndexIt = rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, KeptIndex, uint32_t>;

// per staged piece: (the points it adds, 1 when it starts a chain of the merged map).  A piece that joins the one before
// it (pieces_join, rj_overlay_map.h) adds its points but the first and starts nothing; kDrop: a piece with fewer than two
// points adds nothing, and "before" is prev_kept[i] - 1.  Zeros beyond the pieces.
// (a piece has at least one point, so (0 or more points, no start) always means: leave out the piece's first point)
template <bool kDrop>
__global__ __launch_bounds__(kThreads) void k_ovm_join(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ row,
                                                       const uint32_t* __restrict__ origin, const int64_t* __restrict__ xy,
                                                       const uint32_t* __restrict__ prev_kept, const Slots* __restrict__ totals,
                                                       uint64_t bound, Slots* __restrict__ adds) {
  const uint64_t nch = totals->chains;
  RJ_GRID_STRIDE(i, bound) {
    Slots s{0, 0};
    if (i < nch) {
      const uint32_t first = row[i];
      const uint64_t len = (uint64_t) (row[i + 1] - first);
      if (!kDrop || len >= 2) {
        const uint64_t before = kDrop ? (uint64_t) prev_kept[i] : i;  // 1 + the piece before; 0: none
        bool join = false;
        if (before) {
          const uint64_t a = before - 1;
          const uint64_t last = (uint64_t) row[a + 1] - 1;
          join = pieces_join(origin[a], keys[2 * a], keys[2 * a + 1], xy + 2 * last, origin[i], keys[2 * i], keys[2 * i + 1],
                             xy + 2 * (uint64_t) first);
        }
        s = join ? Slots{len - 1, 0} : Slots{len, 1};
      }
    }
    adds[i] = s;
  }
}

// k_ovm_label for the merged map: the pieces that start a chain carry its row_index entry, faces and origin
__global__ __launch_bounds__(kThreads) void k_ovm_merge_label(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ ukeys,
                                                               const uint64_t* __restrict__ n_unique, const Slots* __restrict__ totals,
                                                               const uint32_t* __restrict__ staged_origin, const Slots* __restrict__ adds,
                                                               const Slots* __restrict__ adds_base, OverlayMapOut out,
                                                               uint64_t* __restrict__ counts) {
  const uint64_t nf = face_count(ukeys, *n_unique), nch = totals->chains;
  const uint64_t i0 = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x, stride = (uint64_t) gridDim.x * blockDim.x;
  if (i0 == 0) {
    const Slots t = nch ? SlotsSum()(adds_base[nch - 1], adds[nch - 1]) : Slots{0, 0};
    if (out.row_index && t.chains <= out.chain_cap) out.row_index[t.chains] = (uint32_t) t.points;
    counts[0] = t.chains;
    counts[1] = t.points;
    counts[2] = nf;
  }
  for (uint64_t i = i0; i < nch; i += stride) {
    if (!adds[i].chains) continue;
    const uint64_t to = adds_base[i].chains;
    if (to >= out.chain_cap) continue;
    out.left[to] = face_id(ukeys, nf, keys[2 * i]);
    out.right[to] = face_id(ukeys, nf, keys[2 * i + 1]);
    out.row_index[to] = (uint32_t) adds_base[i].points;
    if (out.origin) out.origin[to] = staged_origin[i];
  }
  const uint64_t lim = nf < out.face_cap ? nf : out.face_cap;
  for (uint64_t i = i0; i < lim; i += stride) {
    out.face_pairs[2 * i] = (int32_t) (uint32_t) (ukeys[i] >> 32);
    out.face_pairs[2 * i + 1] = (int32_t) (uint32_t) ukeys[i];
  }
}

// the staged points to their places in the merged map: a lane per point, its 16 bytes in one load and one store,
// consecutive lanes on consecutive points (of a run: consecutive slots too).  The first point of a piece that starts no
// chain stays behind: the duplicate of the point before it, or the one point of a dropped piece.
typedef long long Point16 __attribute__((ext_vector_type(2), aligned(8)));  // (the caller's xy is an int64 array)
__global__ __launch_bounds__(kThreads) void k_ovm_merge_points(const int64_t* __restrict__ staged_xy, const uint32_t* __restrict__ staged_row,
                                                               const uint32_t* __restrict__ point_piece, const Slots* __restrict__ totals,
                                                               const Slots* __restrict__ adds, const Slots* __restrict__ adds_base,
                                                               int64_t* __restrict__ xy, uint64_t point_cap) {
  const uint64_t np = totals->points;
  RJ_GRID_STRIDE(j, np) {
    const uint32_t i = point_piece[j];
    const uint64_t at = j - staged_row[i], skip = adds[i].chains ? 0 : 1;
    if (at < skip) continue;
    const uint64_t to = adds_base[i].points + at - skip;
    if (to < point_cap) *reinterpret_cast<Point16*>(xy + 2 * to) = *reinterpret_cast<const Point16*>(staged_xy + 2 * j);
  }
}

// one pass over map im: the intersection's kernel, or the operation's when there is one
template <bool kWrite>
void launch_emit(hipStream_t st, const OverlayOp* op, int im, const OverlayFacesMap& m, const rj_xsect* xs, uint64_t n, const int32_t* vertex_face,
                 Slots* wave_count, const Slots* wave_base, const Stage& stage) {
  const dim3 grid(blocks_for(64 * ((m.ne + 63) / 64), 8192));  // a lane per edge, whole waves
  if (op)
    hipLaunchKernelGGL(k_ovm_emit_op<kWrite>, grid, dim3(kThreads), 0, st, im, m.pts, m.edge_chain, m.edge_begin, (const int32_t*) m.left,
                       (const int32_t*) m.right, m.ne, (const Rec48*) xs, n, vertex_face, wave_count, wave_base, stage, op->how, op->by);
  else
    hipLaunchKernelGGL(k_ovm_emit<kWrite>, grid, dim3(kThreads), 0, st, im, m.pts, m.edge_chain, m.edge_begin, (const int32_t*) m.left,
                       (const int32_t*) m.right, m.ne, (const Rec48*) xs, n, vertex_face, wave_count, wave_base, stage);
}
// (prev_kept: null unless drop)
void launch_join(hipStream_t st, bool drop, const uint64_t* keys, const uint32_t* row, const uint32_t* origin, const int64_t* xy,
                 const uint32_t* prev_kept, const Slots* totals, uint64_t bound, Slots* adds) {
  const dim3 grid(blocks_for(bound, 4096));
  if (drop) hipLaunchKernelGGL(k_ovm_join<true>, grid, dim3(kThreads), 0, st, keys, row, origin, xy, prev_kept, totals, bound, adds);
  else hipLaunchKernelGGL(k_ovm_join<false>, grid, dim3(kThreads), 0, st, keys, row, origin, xy, prev_kept, totals, bound, adds);
}

// rj_upload_map_dev: what rj_upload_map checks in host loops, and edge_begin[c] = row_index[c] - c.  *status = the
// largest kMapBad* code met (0: the map is fine; the order rj_upload_map checks in); edge_begin is only meaningful then.
__global__ __launch_bounds__(kThreads) void k_map_check(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row_index,
                                                        uint64_t nc, uint32_t* __restrict__ edge_begin, uint32_t* status) {
  uint32_t bad = 0;
  const uint64_t i0 = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x, stride = (uint64_t) gridDim.x * blockDim.x;
  for (uint64_t c = i0; c <= nc; c += stride) {
    const uint32_t b = row_index[c];
    if (c == 0 && b != 0) bad = max(bad, kMapBadStart);
    if (c == nc && (uint64_t) b != np) bad = max(bad, kMapBadEnd);
    if (c < nc && (uint64_t) row_index[c + 1] < (uint64_t) b + 2) bad = max(bad, kMapBadShortChain);
    edge_begin[c] = (uint32_t) (b - c);
  }
  for (uint64_t i = i0; i < 2 * np; i += stride)
    if (xy[i] < -((int64_t) 1 << 46) || xy[i] >= ((int64_t) 1 << 46)) bad = max(bad, kMapBadCoordinate);
  if (bad) atomicMax(status, bad);
}

}  // namespace

hipError_t map_check_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row_index, uint64_t nc, uint32_t* edge_begin,
                            uint32_t* status_dev, uint32_t* status) {
  hipError_t e = hipMemsetAsync(status_dev, 0, 4, st);
  if (e != hipSuccess) return e;
  const uint64_t work = 2 * np > nc + 1 ? 2 * np : nc + 1;
  hipLaunchKernelGGL(k_map_check, dim3(blocks_for(work, 2048)), dim3(kThreads), 0, st, xy, np, row_index, nc, edge_begin, status_dev);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(status, status_dev, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

hipError_t overlay_map_device(hipStream_t st, const OverlayFacesMap maps[2], const uint64_t np[2], const rj_xsect* const xsects[2], uint64_t n,
                              const int32_t* const vertex_face[2], bool drop, bool merge, const OverlayMapOut& o, uint64_t counts[3],
                              char** scratch, size_t* scratch_bytes, const OverlayOp* op) {
  const uint64_t waves[2] = {(maps[0].ne + 63) / 64, (maps[1].ne + 63) / 64}, nwaves = waves[0] + waves[1];
  const uint64_t piece_bound = max_pieces(maps[0].nc, n) + max_pieces(maps[1].nc, n);
  const uint64_t point_bound = max_points(np[0], n) + max_points(np[1], n);
  const uint64_t nkeys = 2 * piece_bound;
  TempSize temp_size;
  temp_size([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) nkeys, 0, 64, st); });
  temp_size([&](size_t& b) {
    return rocprim::unique(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (uint64_t*) nullptr, (size_t) nkeys,
                           rocprim::equal_to<uint64_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const Slots*) nullptr, (Slots*) nullptr, Slots{0, 0}, (size_t) (nwaves + 1), SlotsSum(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const Slots*) nullptr, (Slots*) nullptr, Slots{0, 0}, (size_t) (piece_bound + 1), SlotsSum(), st);
  });
  if (merge && drop)
    temp_size([&](size_t& b) {
      return rocprim::exclusive_scan(nullptr, b, KeptIndexIt(rocprim::counting_iterator<uint32_t>(0), KeptIndex{nullptr, nullptr}),
                                     (uint32_t*) nullptr, 0u, (size_t) (piece_bound + 1), rocprim::maximum<uint32_t>(), st);
    });
  if (temp_size.error != hipSuccess) return temp_size.error;
  const size_t temp_bytes = temp_size.bytes;
  const bool staged = drop || merge;
  Slots *wcount, *wbase, *totals, *kept = nullptr, *kept_base = nullptr;
  uint64_t *keys, *sorted, *ukeys, *nu, *counts_dev;
  int64_t* staged_xy = nullptr;
  uint32_t *staged_row = nullptr, *staged_origin = nullptr, *point_piece = nullptr, *prev_kept = nullptr;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    wcount = A.take<Slots>(nwaves + 1);
    wbase = A.take<Slots>(nwaves + 1);
    totals = A.take<Slots>(1);
    nu = A.take<uint64_t>(1);
    counts_dev = A.take<uint64_t>(3);
    keys = A.take<uint64_t>(nkeys + 2);
    sorted = A.take<uint64_t>(nkeys + 2);
    ukeys = A.take<uint64_t>(nkeys + 2);
    temp = A.take<char>(temp_bytes);
    if (staged) {  // (kept, kept_base: with merge, what the pieces add and where)
      kept = A.take<Slots>(piece_bound + 1);
      kept_base = A.take<Slots>(piece_bound + 1);
      staged_xy = A.take<int64_t>(2 * point_bound + 2);
      staged_row = A.take<uint32_t>(piece_bound + 1);
      staged_origin = A.take<uint32_t>(piece_bound + 1);
      point_piece = A.take<uint32_t>(point_bound + 1);
    }
    if (merge && drop) prev_kept = A.take<uint32_t>(piece_bound + 1);
  };
  carve();
  hipError_t e = grow_block(scratch, scratch_bytes, A.used);
  if (e != hipSuccess) return e;
  A.base = *scratch;
  carve();
  Stage stage;
  if (staged) stage = Stage{staged_xy, staged_row, staged_origin, point_piece, keys, point_bound, piece_bound};
  else stage = Stage{o.xy, o.row_index, o.origin, nullptr, keys, o.point_cap, o.chain_cap};
  if ((e = hipMemsetAsync(keys, 0xFF, 8 * nkeys, st)) != hipSuccess) return e;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t at = 0;  // map im's waves: [at, at + waves[im]) of the wave arrays
    for (int im = 0; im < 2; im++) {
      const OverlayFacesMap& m = maps[im];
      if (m.ne) {
        if (pass == 0) launch_emit<false>(st, op, im, m, xsects[im], n, vertex_face[im], wcount + at, nullptr, stage);
        else launch_emit<true>(st, op, im, m, xsects[im], n, vertex_face[im], nullptr, wbase + at, stage);
        if ((e = hipGetLastError()) != hipSuccess) return e;
      }
      at += waves[im];
    }
    if (pass == 0 && nwaves) {
      size_t sb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, sb, wcount, wbase, Slots{0, 0}, (size_t) nwaves, SlotsSum(), st)) != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL(k_ovm_totals, dim3(1), dim3(1), 0, st, (const Slots*) wcount, (const Slots*) wbase, nwaves, totals, stage);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = temp_bytes;
  if (nkeys) {
    if ((e = rocprim::radix_sort_keys(temp, tb, keys, sorted, (size_t) nkeys, 0, 64, st)) != hipSuccess) return e;
    tb = temp_bytes;
    if ((e = rocprim::unique(temp, tb, sorted, ukeys, nu, (size_t) nkeys, rocprim::equal_to<uint64_t>(), st)) != hipSuccess) return e;
  } else if ((e = hipMemsetAsync(nu, 0, 8, st)) != hipSuccess) {
    return e;
  }
  if (merge) {
    if (drop && piece_bound) {
      tb = temp_bytes;
      e = rocprim::exclusive_scan(temp, tb, KeptIndexIt(rocprim::counting_iterator<uint32_t>(0), KeptIndex{staged_row, totals}), prev_kept, 0u,
                                  (size_t) piece_bound, rocprim::maximum<uint32_t>(), st);
      if (e != hipSuccess) return e;
    }
    launch_join(st, drop, keys, staged_row, staged_origin, staged_xy, prev_kept, totals, piece_bound, kept);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (piece_bound) {
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, kept, kept_base, Slots{0, 0}, (size_t) piece_bound, SlotsSum(), st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ovm_merge_points, dim3(blocks_for(point_bound, 8192)), dim3(kThreads), 0, st, (const int64_t*) staged_xy,
                       (const uint32_t*) staged_row, (const uint32_t*) point_piece, (const Slots*) totals, (const Slots*) kept,
                       (const Slots*) kept_base, o.xy, o.point_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ovm_merge_label, dim3(blocks_for(piece_bound > nkeys ? piece_bound : nkeys, 4096)), dim3(kThreads), 0, st,
                       (const uint64_t*) keys, (const uint64_t*) ukeys, (const uint64_t*) nu, (const Slots*) totals,
                       (const uint32_t*) staged_origin, (const Slots*) kept, (const Slots*) kept_base, o, counts_dev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if (drop) {
    hipLaunchKernelGGL(k_ovm_keep, dim3(blocks_for(piece_bound, 4096)), dim3(kThreads), 0, st, (const uint32_t*) staged_row,
                       (const Slots*) totals, piece_bound, kept);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (piece_bound) {
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, kept, kept_base, Slots{0, 0}, (size_t) piece_bound, SlotsSum(), st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ovm_compact_points, dim3(blocks_for(point_bound, 8192)), dim3(kThreads), 0, st, (const int64_t*) staged_xy,
                       (const uint32_t*) staged_row, (const uint32_t*) point_piece, (const Slots*) totals, (const Slots*) kept,
                       (const Slots*) kept_base, o.xy, o.point_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!merge) {
    hipLaunchKernelGGL(k_ovm_label, dim3(blocks_for(piece_bound > nkeys ? piece_bound : nkeys, 4096)), dim3(kThreads), 0, st,
                       (const uint64_t*) keys, (const uint64_t*) ukeys, (const uint64_t*) nu, (const Slots*) totals,
                       (const uint32_t*) staged_row, (const uint32_t*) staged_origin, (const Slots*) kept, (const Slots*) kept_base, o,
                       counts_dev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // the one read-back: the three counts
  if ((e = hipMemcpyAsync(counts, counts_dev, 24, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

}  // namespace rj
