// rj_overlay_dev.h -- what the overlay's device passes share (rj_overlay.hip: the face table, rj_overlay_map.hip: the
// output map): the wave-wide record search; and what rj_api.hip calls in rj_overlay_map.hip.  HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rayjoin_amd.h"
#include "rj_kernels.h"
#include "rj_overlay.h"

namespace rj {
namespace overlay {

// first record whose eid[im] >= eid, found by the whole wave: 64 probes per step (a dependent load per 64x narrowing,
// where one lane's binary search makes one per halving -- those serial loads were most of this pass).  Wave-uniform.
__device__ __forceinline__ uint64_t wave_first_record(const Rec48* __restrict__ xs, uint64_t n, int im, uint64_t eid, int lane) {
  uint64_t b = 0, e = n;  // the answer lies in [b, e]
  while (e - b > 64) {
    const uint64_t step = (e - b + 63) / 64, probe = b + (uint64_t) lane * step;
    const bool below = probe < e && (uint64_t) xs[probe].eid[im] < eid;
    const uint64_t k = (uint64_t) __popcll(__ballot(below));  // the probes below eid are a prefix
    const uint64_t nb = k ? b + (k - 1) * step + 1 : b, ne = b + k * step < e ? b + k * step : e;
    b = nb;
    e = ne;
  }
  const bool below = b + lane < e && (uint64_t) xs[b + lane].eid[im] < eid;
  return b + (uint64_t) __popcll(__ballot(below));
}

}  // namespace overlay

// The overlay's output map (rj_overlay_map.hip, rj_overlay_map.h): the caller's arrays and their capacities.
struct OverlayMapOut {
  int64_t* xy;
  uint32_t* row_index;
  int32_t *left, *right, *face_pairs;
  uint32_t* origin;
  uint64_t chain_cap, point_cap, face_cap;
};
// np[im]: points of map im; counts = {chains, points, faces}, the true counts (read back with the stream's one sync);
// nothing is written beyond a capacity.  drop: leave out the pieces with fewer than two points.  merge: adjacent pieces
// that join (pieces_join, rj_overlay_map.h) leave as one chain, after drop.  op == null: the
// intersection's own emit kernels (rj_overlay_map); else the operation's (rj_overlay_map_op) -- every other stage is shared.
hipError_t overlay_map_device(hipStream_t st, const OverlayFacesMap maps[2], const uint64_t np[2], const rj_xsect* const xsects[2], uint64_t n,
                              const int32_t* const vertex_face[2], bool drop, bool merge, const OverlayMapOut& out, uint64_t counts[3],
                              char** scratch, size_t* scratch_bytes, const OverlayOp* op = nullptr);

// rj_upload_map_dev's checks in one kernel (nc > 0): *status = 0 or the first failure in rj_upload_map's order; also
// fills edge_begin[nc + 1] (row_index[c] - c), valid when *status == 0.  Synchronises the stream.
constexpr uint32_t kMapBadStart = 4, kMapBadEnd = 3, kMapBadShortChain = 2, kMapBadCoordinate = 1;
hipError_t map_check_device(hipStream_t st, const int64_t* xy, uint64_t np, const uint32_t* row_index, uint64_t nc, uint32_t* edge_begin,
                            uint32_t* status_dev, uint32_t* status);

}  // namespace rj
