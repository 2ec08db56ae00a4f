// rj_overlay.hip -- the overlay's face table on the device (rj_overlay.h has the semantics and the per-edge rule).
//   1. k_ovf_contrib  one lane per edge of a map, 64 consecutive edges per wave.  The sub-segments of one piece lie on
//                     neighbouring edges and share a key, so a segmented scan across the wave sums them on chip: a lane
//                     stores the piece it closes (or the wave's open part), its head piece and the pieces between its
//                     own cuts -- about one value per piece instead of one per edge.  Two passes: the first counts what
//                     each wave stores, a scan over the waves gives each its slots, the second stores (one atomic per
//                     wave on one word was 12 ns a wave: 4.5 of 6.3 ms on a 24 M-edge map).  The buffer has
//                     max_contributions() entries per map, pre-filled with a key that sorts last.
//   2. rocPRIM radix sort of the 64-bit (face 0, face 1) keys carrying the int128 as two limbs.
//   3. rocPRIM reduce_by_key (integer sums: exact, any order gives the same bits) and k_ovf_emit: the rows, the count.
// rj_overlay_faces_op runs the same passes with k_ovf_contrib_op: the body of k_ovf_contrib with the selection and the face
// keys of an overlay operation (rj_overlay_ops.h) in place of the intersection's; the operation is a kernel argument.
// No host loop over edges, pieces or records; the host reads one word at the end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/rayjoin_amd.h"
#include "rj_kernels.h"
#include "rj_overlay.h"
#include "rj_overlay_dev.h"
#include "rj_overlay_ops.h"
#include "rj_pipeline.h"

namespace rj {

using namespace overlay;

namespace {

static_assert(sizeof(Rec48) == sizeof(rj_xsect) && sizeof(Area2) == 16 && sizeof(rj_overlay_face) == 24, "layouts");

struct Area2Sum {
  __host__ __device__ Area2 operator()(const Area2& a, const Area2& b) const { return add(a, b); }
};

__device__ __forceinline__ __int128 shfl_up128(__int128 v, int d) {
  const uint64_t lo = (uint64_t) v;
  const int64_t hi = (int64_t) (v >> 64);
  const uint64_t lo2 = (uint64_t) __shfl_up((long long) lo, d, 64);
  const int64_t hi2 = (int64_t) __shfl_up((long long) hi, d, 64);
  return (__int128) (((unsigned __int128) (uint64_t) hi2 << 64) | lo2);
}

// which sub-segments contribute, and to which keys: the intersection's hard-wired rule (rj_overlay.h) for rj_overlay_faces,
// an operation (rj_overlay_ops.h) for rj_overlay_faces_op.  The operation lives in scalar registers: wave-uniform.
struct RuleIntersection {
  __device__ __forceinline__ int sides(int, int32_t l, int32_t r, int32_t label) const { return overlay::sides(label, l, r); }
  template <class F>
  __device__ __forceinline__ void emit(int im, int32_t l, int32_t r, int32_t label, __int128 v, F&& f) const {
    overlay::emit_sides(im, l, r, label, v, f);
  }
};
struct RuleOp {
  Op op;
  __device__ __forceinline__ int sides(int im, int32_t l, int32_t r, int32_t label) const { return overlay::sides(im, l, r, label, op); }
  template <class F>
  __device__ __forceinline__ void emit(int im, int32_t l, int32_t r, int32_t label, __int128 v, F&& f) const {
    overlay::emit_sides(im, l, r, label, v, op, f);
  }
};

// one map's contributions (kWrite 0: what each wave stores, to wave_count; 1: store them from wave_base).  Every lane of a wave runs the loop body the same number of times (lanes beyond ne take part
// in the shuffles as empty segments).
// (nwaves, wave0, wstride come from the kernel: with blockDim / gridDim read here the compiler fetched the launch
//  geometry the generic way and the intersection's kernels lost 0.1 ms of 1.56 on 30.8 M edges)
template <bool kWrite, class Rule>
__device__ __forceinline__ void ovf_contrib(const Rule rule, uint64_t nwaves, uint64_t wave0, uint64_t wstride, int im,
                                            const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                            const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                            const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs, uint64_t n,
                                            const int32_t* __restrict__ vertex_face, uint64_t* __restrict__ keys, Area2* __restrict__ vals,
                                            uint32_t* __restrict__ wave_count, const uint64_t* __restrict__ wave_base, uint64_t cap) {
  const int lane = threadIdx.x & 63;
  for (uint64_t w = wave0; w < nwaves; w += wstride) {
    const uint64_t e0 = w * 64, e_end = e0 + 64 < ne ? e0 + 64 : ne;
    const uint64_t e = e0 + lane;
    const bool valid = e < ne;
    // the records of the wave's edges: two searches per wave, the lanes' searches stay inside that range
    const uint64_t wlo = wave_first_record(xs, n, im, e0, lane), whi = wave_first_record(xs, n, im, e_end, lane);
    uint32_t c = 0;
    uint64_t lo = wlo, hi = wlo;
    int32_t l = 0, r = 0, tail = 0;
    bool reset = true;
    __int128 a = 0;
    if (valid) {
      c = edge_chain[e];
      lo = first_record_at(xs, wlo, whi, im, e);
      hi = first_record_at(xs, lo, whi, im, e + 1);
      l = left[c];
      r = right[c];
      tail = tail_label(xs, n, im, hi, c, edge_begin, vertex_face);
      reset = lo < hi || edge_begin[c] == e;  // a piece starts inside this edge (at its last cut) or with the chain
      a = lo < hi ? tail_part(pts, e, c, xs[hi - 1]) : whole_edge(pts, e, c);
    }
    // segmented inclusive scan: s = what the piece open at the end of this lane has gathered inside the wave
    __int128 s = a;
    bool f = reset;
    for (int d = 1; d < 64; d <<= 1) {
      const __int128 su = shfl_up128(s, d);
      const bool fu = __shfl_up((int) f, d, 64) != 0;
      if (lane >= d) {
        if (!f) s += su;
        f = f || fu;
      }
    }
    const bool next_resets = __shfl_down((int) reset, 1, 64) != 0;
    const bool emit_open = valid && (lane == 63 || next_resets);  // the piece ends here, or the wave does
    // slots: count, then store
    uint32_t m = 0;
    int32_t head = 0;
    if (valid) {
      if (emit_open) m += rule.sides(im, l, r, tail);
      if (lo < hi) {
        head = head_label(e, c, vertex_face);
        m += rule.sides(im, l, r, head);
        for (uint64_t k = lo; k + 1 < hi; k++) m += rule.sides(im, l, r, xs[k].mid);
      }
    }
    uint32_t incl = m;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (!kWrite) {
      if (lane == 63) wave_count[w] = incl;
      continue;
    }
    uint64_t slot = wave_base[w] + incl - m;
    auto store = [&](uint64_t key, __int128 v) {
      if (slot < cap) {  // (max_contributions bounds the map's total; never past its part of the buffer)
        keys[slot] = key;
        vals[slot] = to_limbs(v);
      }
      slot++;
    };
    if (m) {
      if (emit_open) rule.emit(im, l, r, tail, s, store);
      if (lo < hi) {
        rule.emit(im, l, r, head, head_part(pts, e, c, xs[lo]), store);
        for (uint64_t k = lo; k + 1 < hi; k++) rule.emit(im, l, r, xs[k].mid, middle_part(xs[k], xs[k + 1]), store);
      }
    }
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_ovf_contrib(int im, const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                                          const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                                          const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs,
                                                          uint64_t n, const int32_t* __restrict__ vertex_face, uint64_t* __restrict__ keys,
                                                          Area2* __restrict__ vals, uint32_t* __restrict__ wave_count,
                                                          const uint64_t* __restrict__ wave_base, uint64_t cap) {
  const uint64_t nwaves = (ne + 63) / 64;
  const uint64_t wave0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / 64;
  const uint64_t wstride = (uint64_t) gridDim.x * blockDim.x / 64;
  ovf_contrib<kWrite>(RuleIntersection{}, nwaves, wave0, wstride, im, pts, edge_chain, edge_begin, left, right, ne, xs, n, vertex_face,
                      keys, vals, wave_count, wave_base, cap);
}

// the same pass under an operation (rj_overlay_faces_op): how / by are kernel arguments
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_ovf_contrib_op(int im, const int64_t* __restrict__ pts, const uint32_t* __restrict__ edge_chain,
                                                             const uint32_t* __restrict__ edge_begin, const int32_t* __restrict__ left,
                                                             const int32_t* __restrict__ right, uint64_t ne, const Rec48* __restrict__ xs,
                                                             uint64_t n, const int32_t* __restrict__ vertex_face, uint64_t* __restrict__ keys,
                                                             Area2* __restrict__ vals, uint32_t* __restrict__ wave_count,
                                                             const uint64_t* __restrict__ wave_base, uint64_t cap, uint32_t how, uint32_t by) {
  const uint64_t nwaves = (ne + 63) / 64;
  const uint64_t wave0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / 64;
  const uint64_t wstride = (uint64_t) gridDim.x * blockDim.x / 64;
  ovf_contrib<kWrite>(RuleOp{make_op(how, by)}, nwaves, wave0, wstride, im, pts, edge_chain, edge_begin, left, right, ne, xs, n, vertex_face,
                      keys, vals, wave_count, wave_base, cap);
}

// rows out: the unique keys but the trailing kNoKey run, at most `capacity` of them; the true count to *n_rows
__global__ __launch_bounds__(kThreads) void k_ovf_emit(const uint64_t* __restrict__ ukeys, const Area2* __restrict__ sums,
                                                       const uint64_t* __restrict__ n_unique, uint64_t capacity,
                                                       rj_overlay_face* __restrict__ out, uint64_t* n_rows) {
  const uint64_t u = *n_unique;
  const uint64_t rows = (u && ukeys[u - 1] == kNoKey) ? u - 1 : u;
  const uint64_t lim = rows < capacity ? rows : capacity;
  const uint64_t i0 = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x;
  if (i0 == 0) *n_rows = rows;
  for (uint64_t i = i0; i < lim; i += (uint64_t) gridDim.x * blockDim.x) {
    const uint64_t k = ukeys[i];
    rj_overlay_face row;
    row.face[0] = (int32_t) (uint32_t) (k >> 32);
    row.face[1] = (int32_t) (uint32_t) k;
    row.area2_lo = sums[i].lo;
    row.area2_hi = sums[i].hi;
    out[i] = row;
  }
}

// one pass over map im: the intersection's kernel, or the operation's when there is one
template <bool kWrite>
void launch_contrib(hipStream_t st, const OverlayOp* op, int im, const OverlayFacesMap& m, const rj_xsect* xs, uint64_t n,
                    const int32_t* vertex_face, uint64_t* keys, Area2* vals, uint32_t* wave_count, const uint64_t* wave_base, uint64_t cap) {
  const dim3 grid(blocks_for(64 * ((m.ne + 63) / 64), 8192));  // a lane per edge, whole waves
  if (op)
    hipLaunchKernelGGL(k_ovf_contrib_op<kWrite>, grid, dim3(kThreads), 0, st, im, m.pts, m.edge_chain, m.edge_begin, (const int32_t*) m.left,
                       (const int32_t*) m.right, m.ne, (const Rec48*) xs, n, vertex_face, keys, vals, wave_count, wave_base, cap, op->how, op->by);
  else
    hipLaunchKernelGGL(k_ovf_contrib<kWrite>, grid, dim3(kThreads), 0, st, im, m.pts, m.edge_chain, m.edge_begin, (const int32_t*) m.left,
                       (const int32_t*) m.right, m.ne, (const Rec48*) xs, n, vertex_face, keys, vals, wave_count, wave_base, cap);
}

__global__ void k_ovf_noop() {}

}  // namespace

hipError_t warm_overlay_kernels(hipStream_t st) {
  hipLaunchKernelGGL(k_ovf_noop, dim3(1), dim3(1), 0, st);
  return hipGetLastError();
}

hipError_t overlay_faces_device(hipStream_t st, const OverlayFacesMap maps[2], const rj_xsect* const xsects[2], uint64_t n,
                                const int32_t* const vertex_face[2], uint64_t capacity, rj_overlay_face* out, uint64_t* n_rows,
                                char** scratch, size_t* scratch_bytes, const OverlayOp* op) {
  uint64_t total = 0;
  for (int im = 0; im < 2; im++) total += max_contributions(maps[im].ne, maps[im].nc, n);
  const uint64_t max_waves = (maps[0].ne > maps[1].ne ? maps[0].ne : maps[1].ne) / 64 + 1;
  TempSize temp_size;
  temp_size([&](size_t& b) {
    return rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (const Area2*) nullptr, (Area2*) nullptr,
                                     (size_t) total, 0, 64, st);
  });
  temp_size([&](size_t& b) {
    return rocprim::reduce_by_key(nullptr, b, (const uint64_t*) nullptr, (const Area2*) nullptr, (size_t) total, (uint64_t*) nullptr,
                                  (Area2*) nullptr, (uint64_t*) nullptr, Area2Sum(), rocprim::equal_to<uint64_t>(), st);
  });
  temp_size([&](size_t& b) {
    return rocprim::exclusive_scan(nullptr, b, (const uint32_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) max_waves,
                                   rocprim::plus<uint64_t>(), st);
  });
  if (temp_size.error != hipSuccess) return temp_size.error;
  const size_t temp_bytes = temp_size.bytes;
  uint64_t *kin, *kout, *nu, *rows;
  Area2 *vin, *vout;
  uint32_t* wcount;
  uint64_t* wbase;
  void* temp;
  Carve A;
  auto carve = [&]() {
    A.used = 0;
    wcount = A.take<uint32_t>(max_waves);
    wbase = A.take<uint64_t>(max_waves);
    nu = A.take<uint64_t>(1);
    rows = A.take<uint64_t>(1);
    kin = A.take<uint64_t>(total);
    kout = A.take<uint64_t>(total);
    vin = A.take<Area2>(total);
    vout = A.take<Area2>(total);
    temp = A.take<char>(temp_bytes);
  };
  carve();
  hipError_t e = grow_block(scratch, scratch_bytes, A.used);
  if (e != hipSuccess) return e;
  A.base = *scratch;
  carve();
  // (the unique keys and their sums reuse the sort's input arrays: reduce_by_key reads kout / vout)
  uint64_t* ukeys = kin;
  Area2* usums = vin;
  if ((e = hipMemsetAsync(kin, 0xFF, 8 * total, st)) != hipSuccess) return e;
  uint64_t at = 0;  // map im stores into [at, at + max_contributions) of the buffer
  for (int im = 0; im < 2; im++) {
    const OverlayFacesMap& m = maps[im];
    const uint64_t part = max_contributions(m.ne, m.nc, n);
    if (m.ne) {
      const uint64_t waves = (m.ne + 63) / 64;
      launch_contrib<false>(st, op, im, m, xsects[im], n, vertex_face[im], kin + at, vin + at, wcount, nullptr, part);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      size_t sb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, sb, wcount, wbase, (uint64_t) 0, (size_t) waves, rocprim::plus<uint64_t>(), st)) != hipSuccess)
        return e;
      launch_contrib<true>(st, op, im, m, xsects[im], n, vertex_face[im], kin + at, vin + at, wcount, wbase, part);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    at += part;
  }
  size_t tb = temp_bytes;
  if ((e = rocprim::radix_sort_pairs(temp, tb, kin, kout, vin, vout, (size_t) total, 0, 64, st)) != hipSuccess) return e;
  tb = temp_bytes;
  if ((e = rocprim::reduce_by_key(temp, tb, kout, vout, (size_t) total, ukeys, usums, nu, Area2Sum(), rocprim::equal_to<uint64_t>(),
                                  st)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_ovf_emit, dim3(blocks_for(capacity < total ? capacity : total, 4096)), dim3(kThreads), 0, st, ukeys, usums, nu,
                     capacity, out, rows);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the one read-back: the row count
  if ((e = hipMemcpyAsync(n_rows, rows, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

}  // namespace rj
