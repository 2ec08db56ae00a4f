// rj_neighbours.hip -- the face adjacency table of a chain map on the device (rj_neighbours.h has the definition and the
// stages).  One pass reads the points: the check with the chain sums S and L, a group of kGroup = 8 lanes per chain as in
// rj_dissolve.hip -- consecutive lanes take consecutive points, 16 bytes each, so a group's step is one 128-byte line (and
// the first 16 bytes of the next, for the edge of its last lane).  Everything behind it is over chain sides, chain ends
// or directed pairs: rocPRIM's radix sorts and sums by key, under RJ_NB_VERTEX its merge sort of the 4 nc incidences by
// (point, label) and two scans, and a grid-stride kernel per function of rj_neighbours.h.  The per-face counters are
// integer atomics: their sums do not depend on the order.  The directed pairs of the nodes are only known on the device,
// so under RJ_NB_VERTEX the host reads their number once, behind the node stage, and sizes the scratch of the last stage
// by it; rook only, that scratch is 2 nc pairs and the call synchronises once, at the end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <string.h>

#include "rj_neighbours.h"
#include "rj_pipeline.h"

namespace rj {

using namespace neighbours;

namespace {

constexpr int kGroup = 8;  // lanes per chain in the pass over the points

struct FaceAdd {
  __host__ __device__ FaceSum operator()(const FaceSum& a, const FaceSum& b) const { return face_add(a, b); }
};
struct PairAdd {
  __host__ __device__ PairSum operator()(const PairSum& a, const PairSum& b) const { return pair_add(a, b); }
};
// what a sorted chain side adds to its face, what a sorted directed key adds to its pair: read where the sums by key need
// them, so that the sorts move 4 bytes per element and not the sums themselves
struct SideVal {
  const int32_t *left, *right;
  const U128 *S, *L;
  __host__ __device__ FaceSum operator()(const uint32_t& side) const { return side_val(side, left, right, S, L); }
};
struct PairVal {
  const U128* L;
  __host__ __device__ PairSum operator()(const uint32_t& side) const { return pair_val(side, L); }
};
struct FlagsAdd {
  __host__ __device__ Flags operator()(const Flags& a, const Flags& b) const { return flags_add(a, b); }
};
struct SatAdd {
  __host__ __device__ uint64_t operator()(const uint64_t& a, const uint64_t& b) const { return saturating_add(a, b); }
};
struct IncBefore {
  const Pt* pts;
  const uint32_t* key;
  __host__ __device__ bool operator()(const uint32_t& a, const uint32_t& b) const { return inc_before(a, b, pts, key); }
};

// 1. the check and the chain sums
__global__ __launch_bounds__(kThreads) void k_nb_sums(const int64_t* __restrict__ xy, uint64_t np, const uint32_t* __restrict__ row, uint64_t nc,
                                                      U128* __restrict__ S, U128* __restrict__ L, Meta* meta) {
  uint32_t bad = 0;
  RJ_GRID_STRIDE(c, nc + 1) bad = max(bad, rings::check_row(c, row, nc, np));
  const uint32_t lane = threadIdx.x & (kGroup - 1);
  const uint64_t g0 = (blockIdx.x * (uint64_t) blockDim.x + threadIdx.x) / kGroup, gstride = (uint64_t) gridDim.x * blockDim.x / kGroup;
  for (uint64_t c = g0; c < nc; c += gstride) {  // (the same trips for all lanes of a group)
    i128 sum = 0;
    u128 len = 0;
    chain_sums(c, lane, kGroup, xy, row, np, &bad, &sum, &len);
    U128 s = rings::limbs(sum), l = limbs(len);
    for (int w = kGroup / 2; w >= 1; w >>= 1) {
      U128 os, ol;
      os.lo = (uint64_t) __shfl_xor((long long) s.lo, w, kGroup);
      os.hi = (uint64_t) __shfl_xor((long long) s.hi, w, kGroup);
      ol.lo = (uint64_t) __shfl_xor((long long) l.lo, w, kGroup);
      ol.hi = (uint64_t) __shfl_xor((long long) l.hi, w, kGroup);
      s = rings::add(s, os);
      l = rings::add(l, ol);
    }
    if (lane == 0) {
      S[c] = s;
      L[c] = l;
    }
  }
  if (bad) atomicMax(&meta->bad, bad);
}

// 2. the faces
__global__ __launch_bounds__(kThreads) void k_nb_sides(const int32_t* __restrict__ left, const int32_t* __restrict__ right, uint64_t ns,
                                                       uint32_t* __restrict__ key, uint32_t* __restrict__ side) {
  RJ_GRID_STRIDE(i, ns) {
    key[i] = eliminate::side_key(i, left, right);
    side[i] = (uint32_t) i;
  }
}
__global__ void k_nb_count_faces(const uint32_t* __restrict__ keys, Meta* meta) { meta->counts.n_faces = eliminate::count_faces(meta->n_keys, keys); }

// 3. the edge pairs
__global__ __launch_bounds__(kThreads) void k_nb_edges(const int32_t* __restrict__ left, const int32_t* __restrict__ right, uint64_t ns,
                                                       const uint32_t* __restrict__ keys, uint64_t* __restrict__ key, uint32_t* __restrict__ side,
                                                       const Meta* meta) {
  const uint64_t nf = meta->counts.n_faces;
  RJ_GRID_STRIDE(i, ns) {
    key[i] = eliminate::directed_key(i, left, right, keys, nf);
    side[i] = (uint32_t) i;
  }
}

// 4. the nodes
__global__ __launch_bounds__(kThreads) void k_nb_ends(const int64_t* __restrict__ xy, const uint32_t* __restrict__ row, const int32_t* __restrict__ left,
                                                      const int32_t* __restrict__ right, uint64_t ns, Pt* __restrict__ pts, uint32_t* __restrict__ ikey,
                                                      const Meta* meta) {
  const bool off = meta->bad != 0;  // (a malformed row: no point is read)
  RJ_GRID_STRIDE(h, ns) pts[h] = off ? Pt{0, 0} : end_point(h, xy, row);
  RJ_GRID_STRIDE(j, 2 * ns) ikey[j] = inc_key(j, left, right);
}
__global__ __launch_bounds__(kThreads) void k_nb_flags(uint64_t ni, const uint32_t* __restrict__ order, const Pt* __restrict__ pts,
                                                       const uint32_t* __restrict__ ikey, Flags* __restrict__ mine) {
  RJ_GRID_STRIDE(k, ni) mine[k] = flags_val(inc_flags(k, order, pts, ikey));
}
__global__ __launch_bounds__(kThreads) void k_nb_place(uint64_t ni, const uint32_t* __restrict__ order, const uint32_t* __restrict__ ikey,
                                                       const Flags* __restrict__ mine, const Flags* __restrict__ before, const uint32_t* __restrict__ keys,
                                                       uint32_t* __restrict__ slot_face, uint32_t* __restrict__ slot_node, uint32_t* __restrict__ node_start,
                                                       Meta* meta) {
  if (meta->bad) return;
  const uint64_t nf = meta->counts.n_faces;
  RJ_GRID_STRIDE(k, ni) {
    inc_place(k, order, ikey, mine, before, keys, nf, slot_face, slot_node, node_start);
    if (k + 1 == ni) {  // the totals, and the end of the last node
      const Flags all = flags_add(before[k], mine[k]);
      meta->n_slots = all.uniq;
      meta->counts.n_nodes = all.head;
      node_start[all.head] = all.uniq;
    }
  }
}
// count[ni + 1]: m - 1 for a slot, 0 behind the slots (the scan's last entry is the total)
__global__ __launch_bounds__(kThreads) void k_nb_pair_counts(uint64_t ni, const uint32_t* __restrict__ slot_node, const uint32_t* __restrict__ node_start,
                                                             uint64_t* __restrict__ count, Meta* meta) {
  const uint64_t n_slots = meta->n_slots;
  uint32_t most = 0;
  RJ_GRID_STRIDE(u, ni + 1) {
    const uint32_t m = u < n_slots ? labels_at(u, slot_node, node_start) : 1u;
    count[u] = m - 1;
    most = max(most, u < n_slots ? m : 0u);
  }
  if (most) atomicMax(&meta->max_labels, most);
}
__global__ void k_nb_raw(uint64_t ni, const uint64_t* __restrict__ at, Meta* meta) {
  if (meta->bad) return;
  meta->counts.n_node_pairs_raw = at[ni];
  meta->counts.max_labels_at_node = meta->max_labels;
}
// the keys of the last stage: the edge keys where they are not there yet (from != key), then the node pairs of every slot
__global__ __launch_bounds__(kThreads) void k_nb_fill(uint64_t ns, const uint64_t* __restrict__ edge_key,
                                                      const uint32_t* __restrict__ slot_face, const uint32_t* __restrict__ slot_node,
                                                      const uint32_t* __restrict__ node_start, const uint64_t* __restrict__ at, uint64_t* __restrict__ key,
                                                      uint32_t* __restrict__ side, const Meta* meta) {
  RJ_GRID_STRIDE(i, ns) {
    key[i] = edge_key[i];
    side[i] = (uint32_t) i;
  }
  RJ_GRID_STRIDE(u, meta->n_slots) node_pairs(u, slot_face, slot_node, node_start, ns + at[u], key, side);
}

// 5. the table.  n_edge, n_vertex: zeroed
__global__ __launch_bounds__(kThreads) void k_nb_tally(const uint64_t* __restrict__ dir, const PairSum* __restrict__ sums, uint32_t* __restrict__ n_edge,
                                                       uint32_t* __restrict__ n_vertex, Meta* meta) {
  if (meta->bad) return;
  const uint64_t n_entries = count_entries(meta->n_dir, dir);
  uint32_t pairs[2] = {0, 0};
  RJ_GRID_STRIDE(i, n_entries) {
    const uint32_t f = eliminate::from_of(dir[i]), g = eliminate::to_of(dir[i]);
    const bool edge = is_edge(sums[i]);
    atomicAdd(edge ? &n_edge[f] : &n_vertex[f], 1u);
    if (f < g) pairs[edge ? 0 : 1]++;
  }
  count_to(&meta->counts.n_edge_pairs, pairs[0]);
  count_to(&meta->counts.n_vertex_pairs, pairs[1]);
}
__global__ void k_nb_totals(const uint64_t* __restrict__ dir, uint64_t face_cap, uint64_t entry_cap, Meta* meta) {
  if (meta->bad) return;
  meta->counts.n_entries = count_entries(meta->n_dir, dir);
  meta->emit = fits(meta->counts, face_cap, entry_cap) ? 1 : 0;
}
__global__ __launch_bounds__(kThreads) void k_nb_emit(const uint32_t* __restrict__ keys, const FaceSum* __restrict__ fsum, const uint32_t* __restrict__ n_edge,
                                                      const uint32_t* __restrict__ n_vertex, const uint64_t* __restrict__ dir,
                                                      const PairSum* __restrict__ sums, Face* __restrict__ faces, uint64_t* __restrict__ offsets,
                                                      Entry* __restrict__ entries, const Meta* meta) {
  if (!meta->emit) return;
  const uint64_t nf = meta->counts.n_faces, n_entries = meta->counts.n_entries;
  if (faces) RJ_GRID_STRIDE(k, nf) faces[k] = face_record(k, keys, fsum, n_edge, n_vertex);
  // (a map without a face fits capacities of 0, the sizing call's, whose arrays may be null)
  if (offsets) RJ_GRID_STRIDE(k, nf + 1) offsets[k] = face_offset(k, dir, n_entries);
  RJ_GRID_STRIDE(i, n_entries) entries[i] = entry_of(i, dir, sums, keys);
}

}  // namespace

hipError_t map_neighbours_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc,
                                 uint32_t flags, uint64_t face_cap, uint64_t entry_cap, Face* faces, uint64_t* offsets, Entry* entries, int point_blocks,
                                 Meta* result, NeighboursReport* report) {
  memset(result, 0, sizeof(Meta));
  *report = NeighboursReport{};
  StageEvents ev;
  hipError_t e = ev.create();
  if (e != hipSuccess) return e;
  const bool vertex = (flags & kVertex) != 0;
  const uint64_t ns = 2 * nc, ni = vertex ? 4 * nc : 0, ni1 = ni + 1;  // chain sides and chain ends; incidences
  char *block = nullptr, *pair_block = nullptr;
  do {
    Meta* meta;
    U128 *S, *L;
    uint32_t *fkey_in, *fkey_out, *side_in, *side_out, *keys, *n_edge, *n_vertex, *ikey, *order, *slot_face, *slot_node, *node_start, *from_in, *from_out;
    FaceSum* fsum;
    uint64_t *edge_key, *count, *at, *key_in, *key_out, *dir;
    PairSum* sums;
    Pt* pts;
    Flags *mine, *before;
    void *temp, *pair_temp;
    TempSize temp_size;
    temp_size([&](size_t& b) {
      return rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*) nullptr, (uint32_t*) nullptr, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) ns, 0,
                                       32, st);
    });
    temp_size([&](size_t& b) {
      return rocprim::reduce_by_key(nullptr, b, (const uint32_t*) nullptr, rocprim::make_transform_iterator((const uint32_t*) nullptr, SideVal{}), (size_t) ns,
                                    (uint32_t*) nullptr, (FaceSum*) nullptr, (uint64_t*) nullptr, FaceAdd(), rocprim::equal_to<uint32_t>(), st);
    });
    if (vertex) {
      temp_size([&](size_t& b) {
        return rocprim::merge_sort(nullptr, b, rocprim::counting_iterator<uint32_t>(0), (uint32_t*) nullptr, (size_t) ni, IncBefore{nullptr, nullptr}, st);
      });
      temp_size([&](size_t& b) {
        return rocprim::exclusive_scan(nullptr, b, (const Flags*) nullptr, (Flags*) nullptr, Flags{0, 0}, (size_t) ni, FlagsAdd(), st);
      });
      temp_size([&](size_t& b) {
        return rocprim::exclusive_scan(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (uint64_t) 0, (size_t) ni1, SatAdd(), st);
      });
    }
    if ((e = temp_size.error) != hipSuccess) break;
    const size_t temp_bytes = temp_size.bytes;
    size_t pair_temp_bytes = 0;
    Carve A;
    auto carve = [&]() {
      A.used = 0;
      meta = A.take<Meta>(1);
      S = A.take<U128>(nc); L = A.take<U128>(nc);
      fkey_in = A.take<uint32_t>(ns); fkey_out = A.take<uint32_t>(ns); side_in = A.take<uint32_t>(ns); side_out = A.take<uint32_t>(ns);
      keys = A.take<uint32_t>(ns);
      fsum = A.take<FaceSum>(ns);
      n_edge = A.take<uint32_t>(2 * ns); n_vertex = n_edge + ns;  // (one zeroed stretch)
      edge_key = A.take<uint64_t>(vertex ? ns : 0);
      pts = A.take<Pt>(vertex ? ns : 0); node_start = A.take<uint32_t>(vertex ? ns + 1 : 0);
      ikey = A.take<uint32_t>(ni); order = A.take<uint32_t>(ni); slot_face = A.take<uint32_t>(ni); slot_node = A.take<uint32_t>(ni);
      mine = A.take<Flags>(ni); before = A.take<Flags>(ni);
      count = A.take<uint64_t>(vertex ? ni1 : 0); at = A.take<uint64_t>(vertex ? ni1 : 0);
      temp = A.take<char>(temp_bytes);
    };
    carve();
    if ((e = hipMalloc((void**) &block, A.used)) != hipSuccess) break;
    A.base = block;
    carve();
    // the scratch of the last stage: n_pairs directed keys with their sums, in, out and unique
    uint64_t n_pairs = 0;
    auto pair_scratch = [&](uint64_t n) -> hipError_t {
      n_pairs = n;
      TempSize ts;
      ts([&](size_t& b) {
        return rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*) nullptr, (uint64_t*) nullptr, (const uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, 0,
                                         64, st);
      });
      ts([&](size_t& b) {
        return rocprim::reduce_by_key(nullptr, b, (const uint64_t*) nullptr, rocprim::make_transform_iterator((const uint32_t*) nullptr, PairVal{}), (size_t) n,
                                      (uint64_t*) nullptr, (PairSum*) nullptr, (uint64_t*) nullptr, PairAdd(), rocprim::equal_to<uint64_t>(), st);
      });
      if (ts.error != hipSuccess) return ts.error;
      Carve B;
      auto carve_pairs = [&]() {
        B.used = 0;
        key_in = B.take<uint64_t>(n); key_out = B.take<uint64_t>(n); dir = B.take<uint64_t>(n);
        from_in = B.take<uint32_t>(n); from_out = B.take<uint32_t>(n); sums = B.take<PairSum>(n);
        pair_temp = B.take<char>(ts.bytes);
      };
      carve_pairs();
      if (hipError_t r = hipMalloc((void**) &pair_block, B.used)) return r;
      B.base = pair_block;
      carve_pairs();
      pair_temp_bytes = ts.bytes;
      return hipSuccess;
    };
    if (!vertex) {
      if ((e = pair_scratch(ns)) != hipSuccess) break;
      edge_key = key_in;
    }
    const int side_blocks = blocks_for(ns, 4096), inc_blocks = blocks_for(ni1, 4096), group_blocks = blocks_for(nc * kGroup, 16384);
    size_t tb;
    // 1. the check and the chain sums
    if ((e = ev.mark(0, st)) != hipSuccess) break;
    if ((e = hipMemsetAsync(meta, 0, sizeof(Meta), st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_nb_sums, dim3(point_blocks > 0 ? point_blocks : group_blocks), dim3(kThreads), 0, st, xy, np, row, nc, S, L, meta);
    if ((e = ev.mark(1, st)) != hipSuccess) break;
    // 2. the faces: the sides by label, their sums
    hipLaunchKernelGGL(k_nb_sides, dim3(side_blocks), dim3(kThreads), 0, st, left, right, ns, fkey_in, side_in);
    tb = temp_bytes;
    if ((e = rocprim::radix_sort_pairs(temp, tb, (const uint32_t*) fkey_in, fkey_out, (const uint32_t*) side_in, side_out, (size_t) ns, 0, 32, st)) != hipSuccess)
      break;
    tb = temp_bytes;
    if ((e = rocprim::reduce_by_key(temp, tb, (const uint32_t*) fkey_out, rocprim::make_transform_iterator((const uint32_t*) side_out, SideVal{left, right, S, L}),
                                    (size_t) ns, keys, fsum, &meta->n_keys, FaceAdd(), rocprim::equal_to<uint32_t>(), st)) != hipSuccess)
      break;
    hipLaunchKernelGGL(k_nb_count_faces, dim3(1), dim3(1), 0, st, (const uint32_t*) keys, meta);
    if ((e = ev.mark(2, st)) != hipSuccess) break;
    // 3. the edge pairs: the directed key of every side with its length
    // (under RJ_NB_VERTEX the keys wait in edge_key, and k_nb_fill numbers the sides again: from_in is not there yet)
    hipLaunchKernelGGL(k_nb_edges, dim3(side_blocks), dim3(kThreads), 0, st, left, right, ns, (const uint32_t*) keys, edge_key, vertex ? side_in : from_in,
                       (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(3, st)) != hipSuccess) break;
    // 4. the nodes: the incidences by (point, label), the distinct ones in slots, the pairs of every slot
    if (vertex) {
      hipLaunchKernelGGL(k_nb_ends, dim3(side_blocks), dim3(kThreads), 0, st, xy, row, left, right, ns, pts, ikey, (const Meta*) meta);
      tb = temp_bytes;
      if ((e = rocprim::merge_sort(temp, tb, rocprim::counting_iterator<uint32_t>(0), order, (size_t) ni, IncBefore{pts, ikey}, st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_nb_flags, dim3(inc_blocks), dim3(kThreads), 0, st, ni, (const uint32_t*) order, (const Pt*) pts, (const uint32_t*) ikey, mine);
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const Flags*) mine, before, Flags{0, 0}, (size_t) ni, FlagsAdd(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_nb_place, dim3(inc_blocks), dim3(kThreads), 0, st, ni, (const uint32_t*) order, (const uint32_t*) ikey, (const Flags*) mine,
                         (const Flags*) before, (const uint32_t*) keys, slot_face, slot_node, node_start, meta);
      hipLaunchKernelGGL(k_nb_pair_counts, dim3(inc_blocks), dim3(kThreads), 0, st, ni, (const uint32_t*) slot_node, (const uint32_t*) node_start, count, meta);
      tb = temp_bytes;
      if ((e = rocprim::exclusive_scan(temp, tb, (const uint64_t*) count, at, (uint64_t) 0, (size_t) ni1, SatAdd(), st)) != hipSuccess) break;
      hipLaunchKernelGGL(k_nb_raw, dim3(1), dim3(1), 0, st, ni, (const uint64_t*) at, meta);
      if ((e = hipGetLastError()) != hipSuccess) break;
      if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) break;  // the extra sync: how many node pairs there are
      if (refused(*result)) break;  // (e is hipSuccess: the caller reads why in *result)
      if ((e = pair_scratch(ns + result->counts.n_node_pairs_raw)) != hipSuccess) break;
      hipLaunchKernelGGL(k_nb_fill, dim3(blocks_for(ns > ni ? ns : ni, 4096)), dim3(kThreads), 0, st, ns, (const uint64_t*) edge_key,
                         (const uint32_t*) slot_face, (const uint32_t*) slot_node, (const uint32_t*) node_start, (const uint64_t*) at, key_in, from_in,
                         (const Meta*) meta);
    }
    if ((e = ev.mark(4, st)) != hipSuccess) break;
    // 5. the table: one sort and one sum of all directed keys, the counters of every face, the output
    tb = pair_temp_bytes;
    if ((e = rocprim::radix_sort_pairs(pair_temp, tb, (const uint64_t*) key_in, key_out, (const uint32_t*) from_in, from_out, (size_t) n_pairs, 0, 64, st)) !=
        hipSuccess)
      break;
    tb = pair_temp_bytes;
    if ((e = rocprim::reduce_by_key(pair_temp, tb, (const uint64_t*) key_out, rocprim::make_transform_iterator((const uint32_t*) from_out, PairVal{L}),
                                    (size_t) n_pairs, dir, sums, &meta->n_dir, PairAdd(), rocprim::equal_to<uint64_t>(), st)) != hipSuccess)
      break;
    if ((e = hipMemsetAsync(n_edge, 0, 4 * 2 * ns, st)) != hipSuccess) break;
    hipLaunchKernelGGL(k_nb_tally, dim3(blocks_for(n_pairs, 4096)), dim3(kThreads), 0, st, (const uint64_t*) dir, (const PairSum*) sums, n_edge, n_vertex, meta);
    hipLaunchKernelGGL(k_nb_totals, dim3(1), dim3(1), 0, st, (const uint64_t*) dir, face_cap, entry_cap, meta);
    hipLaunchKernelGGL(k_nb_emit, dim3(blocks_for(n_pairs, 4096)), dim3(kThreads), 0, st, (const uint32_t*) keys, (const FaceSum*) fsum, (const uint32_t*) n_edge,
                       (const uint32_t*) n_vertex, (const uint64_t*) dir, (const PairSum*) sums, faces, offsets, entries, (const Meta*) meta);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = ev.mark(5, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(result, meta, sizeof(Meta), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);  // the last sync: the counts, and nothing of this call runs when its scratch goes
    if (e == hipSuccess && !refused(*result)) ev.times(5, report->ms);
  } while (0);
  if (e != hipSuccess) (void) hipStreamSynchronize(st);
  const hipError_t fe = hipFree(block), fp = hipFree(pair_block);
  return e != hipSuccess ? e : (fe != hipSuccess ? fe : fp);
}

}  // namespace rj
