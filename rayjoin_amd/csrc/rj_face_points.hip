// rj_face_points.hip -- per-face counts, sums and members of located points on the device (rj_face_points.h has the
// definition, the limb arithmetic and the stages).  The table pass is the hot path: one pass that reads every label once
// and every value once, 4 and 8 bytes per lane and trip, consecutive lanes on consecutive points.  A wave cuts its 64
// points into runs of equal labels with one ballot; with values the lanes of a run are summed by a segmented scan over
// shuffles (six steps, no LDS), without values the run's count and first point are lane arithmetic and nothing is
// shuffled at all.  Only the last lane of a run searches the face and issues the run's atomics, so a face that holds
// millions of coherent points sees one set of atomics per 64 of them, and the points outside every face (label 0, most
// points of a typical query) none: they are counted per lane and added once per block.  Every accumulator is an integer
// add, min or max: no arrival order, grid or wave layout changes a result.  The universe of the faces, where the caller
// gives none, is a rocPRIM select of the run heads' keys, a radix sort and a unique over the heads only; the offsets are a
// rocPRIM scan; the members a stable rocPRIM radix sort of (face number, point number) over the bits that hold n_faces.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <string.h>

#include "rj_face_points.h"
#include "rj_neighbours.h"
#include "rj_pipeline.h"

namespace rj {

using namespace face_points;

namespace {

static_assert(kWave == 64 && kThreads % kWave == 0, "the table pass cuts its runs where a wave64 starts");

// the run heads among the points: what the select keeps, and the key it keeps of them
struct HeadFlag {
  const int32_t* label;
  __host__ __device__ bool operator()(const uint32_t& i) const { return is_head(i, label); }
};
struct HeadKey {
  const int32_t* label;
  __host__ __device__ uint32_t operator()(const uint32_t& i) const { return head_key(i, label); }
};
// n_points of face k, 0 behind the faces (the scan's entry n_faces is the total)
struct PointsOf {
  const Acc* acc;
  const Meta* meta;
  __host__ __device__ uint64_t operator()(const uint64_t& k) const { return k < meta->counts.n_faces ? acc[k].n : 0; }
};

// 1. the universe
__global__ __launch_bounds__(kThreads) void k_fp_universe(const int32_t* __restrict__ face_label, uint64_t nfl, uint32_t* __restrict__ keys, Meta* meta) {
  bool bad = false;
  RJ_GRID_STRIDE(k, nfl) {
    bad = bad || universe_bad(k, face_label);
    keys[k] = universe_key(k, face_label);
  }
  if (bad) atomicMax(&meta->bad, kBadUniverse);
  if (blockIdx.x == 0 && threadIdx.x == 0) meta->counts.n_faces = nfl;
}
__global__ void k_fp_count_faces(const uint32_t* __restrict__ keys, Meta* meta) { meta->counts.n_faces = eliminate::count_faces(meta->n_keys, keys); }

// 2. the table pass
__global__ __launch_bounds__(kThreads) void k_fp_init(Acc* __restrict__ acc, uint64_t cap) { RJ_GRID_STRIDE(k, cap) acc[k] = acc_empty(); }

template <bool kValues>
__global__ __launch_bounds__(kThreads) void k_fp_table(const int32_t* __restrict__ label, uint64_t n, const int64_t* __restrict__ value, uint64_t stride,
                                                       const uint32_t* __restrict__ keys, Acc* acc, Meta* meta) {
  if (meta->bad) return;  // (the same for every thread)
  const uint64_t nf = meta->counts.n_faces;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t step = (uint64_t) gridDim.x * blockDim.x;  // (a multiple of kWave: every trip of a wave starts at one)
  uint32_t outside = 0, unmatched = 0, heads = 0;
  // the same trips for all lanes of a wave: the ballot and the shuffles below need them all
  for (uint64_t base = blockIdx.x * (uint64_t) blockDim.x + (threadIdx.x - lane); base < n; base += step) {
    const uint64_t i = base + lane;
    const bool active = i < n;
    const int32_t mine = active ? label[i] : 0;
    int32_t before = __shfl_up(mine, 1, kWave);
    if (lane == 0 && base > 0) before = label[base - 1];
    const bool head = active && (i == 0 || mine != before);  // is_head
    heads += head ? 1u : 0u;
    // seg_head: a run starts at a head and where the wave starts; the lanes behind the last point stand alone
    const uint64_t starts = __ballot(!active || lane == 0 || head);
    const uint32_t first_lane = 63u - (uint32_t) __clzll((long long) (starts & (~0ull >> (63u - lane))));
    const bool last = active && (lane == kWave - 1 || ((starts >> (lane + 1)) & 1ull));
    Part p{0, kNoPoint, 0, 0, INT64_MAX, INT64_MIN};
    if (kValues) {
      if (active) p = part_of(i, value, stride);
      // the inclusive scan of the run's lanes: lane l takes the piece that ends d lanes in front where that is still its run
      for (uint32_t d = 1; d < kWave; d <<= 1) {
        Part q{0, kNoPoint, 0, 0, 0, 0};  // (n and first of a run are lane arithmetic: below)
        q.lo = (uint64_t) __shfl_up((long long) p.lo, d, kWave);
        q.hi = __shfl_up((long long) p.hi, d, kWave);
        q.min = __shfl_up((long long) p.min, d, kWave);
        q.max = __shfl_up((long long) p.max, d, kWave);
        if (lane >= first_lane + d) p = part_add(q, p);
      }
    }
    if (last) {
      p.n = lane - first_lane + 1;
      p.first = (uint32_t) (i - (lane - first_lane));
      const int where = run_apply(p, mine, kValues, keys, nf, acc);
      outside += where == kOutside ? p.n : 0u;
      unmatched += where == kUnmatched ? p.n : 0u;
    }
  }
  // (the sums of a block stay below n < 2^32)
  count_to(&meta->counts.n_outside, outside);
  count_to(&meta->counts.n_unmatched, unmatched);
  count_to(&meta->counts.n_runs, heads);
}

// 3. the records and the offsets
__global__ void k_fp_totals(uint64_t n, uint32_t flags, uint64_t face_cap, uint64_t member_cap, Meta* meta) {
  if (meta->bad) return;
  meta->counts.n_members = n - meta->counts.n_outside - meta->counts.n_unmatched;
  meta->emit = fits(meta->counts, (flags & kMembers) != 0, face_cap, member_cap) ? 1 : 0;
}
// scanned[nf + 1]: the exclusive scan of n_points (null without kMembers)
__global__ __launch_bounds__(kThreads) void k_fp_emit(const uint32_t* __restrict__ keys, const Acc* __restrict__ acc, const uint64_t* __restrict__ scanned,
                                                      Face* __restrict__ faces, uint64_t* __restrict__ offsets, const Meta* meta) {
  if (!meta->emit) return;
  const uint64_t nf = meta->counts.n_faces;
  if (faces) RJ_GRID_STRIDE(k, nf) faces[k] = face_record(k, keys, acc);
  // (a call without a face fits capacities of 0, the sizing call's, whose arrays may be null)
  if (scanned && offsets) RJ_GRID_STRIDE(k, nf + 1) offsets[k] = scanned[k];
}

// 4. the members
__global__ __launch_bounds__(kThreads) void k_fp_member_keys(const int32_t* __restrict__ label, uint64_t n, const uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ key, const Meta* meta) {
  if (!meta->emit) return;
  const uint64_t nf = meta->counts.n_faces;
  RJ_GRID_STRIDE(i, n) key[i] = member_key(i, label, keys, nf);
}
__global__ __launch_bounds__(kThreads) void k_fp_members(const uint32_t* __restrict__ sorted, uint32_t* __restrict__ members, const Meta* meta) {
  if (!meta->emit) return;
  RJ_GRID_STRIDE(i, meta->counts.n_members) members[i] = sorted[i];
}

__global__ __launch_bounds__(kThreads) void k_nb_labels(const neighbours::Face* __restrict__ faces, uint64_t nf, int32_t* __restrict__ label) {
  RJ_GRID_STRIDE(k, nf) label[k] = faces[k].label;
}

}  // namespace

hipError_t face_points_device(hipStream_t st, const int32_t* label, uint64_t n, const int64_t* value, uint64_t value_stride, const int32_t* face_label,
                              uint64_t n_face_labels, uint32_t flags, uint64_t face_cap, uint64_t member_cap, Face* faces, uint64_t* offsets, uint32_t* members,
                              int table_blocks, Meta* result, FacePointsReport* report) {
  memset(result, 0, sizeof(Meta));
  *report = FacePointsReport{};
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  const bool universe = face_label != nullptr, with_members = (flags & kMembers) != 0;
  const rocprim::counting_iterator<uint32_t> point(0);
  char *block = nullptr, *face_block = nullptr;
  do {
    Meta* meta;
    uint32_t *heads = nullptr, *heads_sorted = nullptr, *keys = nullptr, *mkey_in = nullptr, *mkey_out = nullptr, *sorted = nullptr;
    Acc* acc = nullptr;
    uint64_t* scanned = nullptr;
    void *temp = nullptr, *face_temp = nullptr;
    // what is sized by the points: the compaction's room without a universe (the number of heads is not known in front of
    // it), the members' keys and sorted point numbers under the flag
    // (member_cap == 0: there is no member to write, or the call overflows -- nothing is sorted, as in the sizing call)
    const uint64_t n_select = universe ? 0 : n, n_sort = with_members && member_cap ? n : 0;
    TempSize temp_size;
    if (n_select)
      temp_size([&](size_t& b) {
        return rocprim::select(nullptr, b, rocprim::make_transform_iterator(point, HeadKey{label}), rocprim::make_transform_iterator(point, HeadFlag{label}),
                               (uint32_t*) nullptr, (uint64_t*) nullptr, (size_t) n, st);
      });
    if (n_sort)
      temp_size([&](size_t& b) {
        return rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, point, (uint32_t*) nullptr, (size_t) n, 0, 32, st);
      });
    if ((e = temp_size.error) != hipSuccess) break;
    const size_t temp_bytes = temp_size.bytes;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<Meta>(1);
      heads = A.take<uint32_t>(n_select);
      mkey_in = A.take<uint32_t>(n_sort); mkey_out = A.take<uint32_t>(n_sort); sorted = A.take<uint32_t>(n_sort);
      temp = A.take<char>(temp_bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    // what is sized by the faces: their keys and accumulators, the scanned offsets; without a universe the sort of the heads
    uint64_t cap = 0;  // the faces there is room for
    size_t face_temp_bytes = 0;
    auto face_scratch = [&](uint64_t n_faces_most, uint64_t n_heads) -> hipError_t {
      cap = n_faces_most;
      TempSize ts;
      if (n_heads) {
        ts([&](size_t& b) { return rocprim::radix_sort_keys(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n_heads, 0, 32, st); });
        ts([&](size_t& b) {
          return rocprim::unique(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (uint64_t*) nullptr, (size_t) n_heads, rocprim::equal_to<uint32_t>(),
                                 st);
        });
      }
      if (with_members)
        ts([&](size_t& b) {
          return rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), PointsOf{nullptr, nullptr}),
                                         (uint64_t*) nullptr, (uint64_t) 0, (size_t) (cap + 1), rocprim::plus<uint64_t>(), st);
        });
      if (ts.error != hipSuccess) return ts.error;
      Carve B;
      auto carve_faces = [&]() {
        B.used = 0;
        keys = B.take<uint32_t>(cap);
        acc = B.take<Acc>(cap);
        scanned = B.take<uint64_t>(with_members ? cap + 1 : 0);
        heads_sorted = B.take<uint32_t>(n_heads);
        face_temp = B.take<char>(ts.bytes);
      };
      carve_faces();
      if (hipError_t r = hipMalloc((void**) &face_block, B.used ? B.used : 1)) return r;
      B.base = face_block;
      carve_faces();
      face_temp_bytes = ts.bytes;
      return hipSuccess;
    };
    size_t tb;
    // 1. the universe: given and checked, or the unique keys of the run heads
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    if (universe) {
      if ((e = face_scratch(n_face_labels, 0)) != hipSuccess) break;
      hipLaunchKernelGGL(k_fp_universe, dim3(blocks_for(n_face_labels, 4096)), dim3(kThreads), 0, st, face_label, n_face_labels, keys, meta);
    } else {
      if (n) {
        tb = temp_bytes;
        if ((e = rocprim::select(temp, tb, rocprim::make_transform_iterator(point, HeadKey{label}), rocprim::make_transform_iterator(point, HeadFlag{label}), heads,
                                 &meta->n_heads, (size_t) n, st)) != hipSuccess)
          break;
      }
      if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // the extra sync: how many run heads there are
      const uint64_t n_heads = result->n_heads;
      if ((e = face_scratch(n_heads, n_heads)) != hipSuccess) break;
      if (n_heads) {
        tb = face_temp_bytes;
        if ((e = rocprim::radix_sort_keys(face_temp, tb, (const uint32_t*) heads, heads_sorted, (size_t) n_heads, 0, 32, st)) != hipSuccess) break;
        tb = face_temp_bytes;
        if ((e = rocprim::unique(face_temp, tb, (const uint32_t*) heads_sorted, keys, &meta->n_keys, (size_t) n_heads, rocprim::equal_to<uint32_t>(), st)) !=
            hipSuccess)
          break;
      }
      hipLaunchKernelGGL(k_fp_count_faces, dim3(1), dim3(1), 0, st, (const uint32_t*) keys, meta);
    }
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the table pass
    hipLaunchKernelGGL(k_fp_init, dim3(blocks_for(cap, 4096)), dim3(kThreads), 0, st, acc, cap);
    const int grid = table_blocks > 0 ? table_blocks : blocks_for(n, 4096);
    if (value)
      hipLaunchKernelGGL(k_fp_table<true>, dim3(grid), dim3(kThreads), 0, st, label, n, value, value_stride, (const uint32_t*) keys, acc, meta);
    else
      hipLaunchKernelGGL(k_fp_table<false>, dim3(grid), dim3(kThreads), 0, st, label, n, value, value_stride, (const uint32_t*) keys, acc, meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    // 3. the records and the offsets
    hipLaunchKernelGGL(k_fp_totals, dim3(1), dim3(1), 0, st, n, flags, face_cap, member_cap, meta);
    if (with_members) {
      tb = face_temp_bytes;
      if ((e = rocprim::exclusive_scan(face_temp, tb, rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), PointsOf{acc, meta}), scanned,
                                       (uint64_t) 0, (size_t) (cap + 1), rocprim::plus<uint64_t>(), st)) != hipSuccess)
        break;
    }
    hipLaunchKernelGGL(k_fp_emit, dim3(blocks_for(cap + 1, 4096)), dim3(kThreads), 0, st, (const uint32_t*) keys, (const Acc*) acc, (const uint64_t*) scanned, faces,
                       offsets, (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the members: the points by face number, stable, over the bits that hold every number up to the faces' room
    if (n_sort) {
      hipLaunchKernelGGL(k_fp_member_keys, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, label, n, (const uint32_t*) keys, mkey_in, (const Meta*) meta);
      tb = temp_bytes;
      if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t*) mkey_in, mkey_out, point, sorted, (size_t) n, 0, key_bits(cap), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_fp_members, dim3(blocks_for(n, 4096)), dim3(kThreads), 0, st, (const uint32_t*) sorted, members, (const Meta*) meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the last sync: the counts, and nothing of this call runs when its scratch goes
    if (e == hipSuccess && !result->bad) ev.times(5, report->ms);
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  const hipError_t fe = hipFree(block), ff = hipFree(face_block);
  return e != hipSuccess ? e : (fe != hipSuccess ? fe : ff);
}

hipError_t neighbours_labels_device(hipStream_t st, const void* nb_faces, uint64_t n_faces, int32_t* label) {
  hipLaunchKernelGGL(k_nb_labels, dim3(blocks_for(n_faces, 4096)), dim3(kThreads), 0, st, reinterpret_cast<const neighbours::Face*>(nb_faces), n_faces, label);
  return hipGetLastError();
}

}  // namespace rj
