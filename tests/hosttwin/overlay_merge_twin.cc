// Test-only host twin of RJ_OVM_MERGE_PIECES: pieces_join of rayjoin_amd/csrc/rj_overlay_map.h -- the very source
// k_ovm_join of rj_overlay_map.hip runs -- driven the way the device drives it: over the STAGED pieces (the output map
// without any flag), with RJ_OVM_DROP_DEGENERATE a piece of fewer than two points adds nothing and "the piece before" is
// the kept piece before; per piece (points added, 1 when it starts a chain), a serial exclusive scan of those, then every
// point and every run start to its slot.  Never linked into the product; the product path is HIP.
#include <cstdint>
#include <vector>

#include "rj_overlay_map.h"

using namespace rj::overlay;

// the staged map: xy, row[nc + 1], left, right (face ids), origin.  counts[2] = chains, points of the merged map (the
// true counts); returns 1 when one exceeds its capacity (nothing is written beyond a capacity)
extern "C" int overlay_merge_twin(const int64_t* xy, const uint32_t* row, const int32_t* left, const int32_t* right, const uint32_t* origin,
                                  uint64_t nc, int drop, uint64_t chain_cap, uint64_t point_cap, int64_t* out_xy, uint32_t* out_row,
                                  int32_t* out_left, int32_t* out_right, uint32_t* out_origin, uint64_t* counts) {
  std::vector<uint64_t> add_points(nc + 1, 0), add_chains(nc + 1, 0), base_points(nc + 1, 0), base_chains(nc + 1, 0);
  uint64_t before = 0;  // 1 + the piece before (with drop: the kept piece before); 0: none
  for (uint64_t i = 0; i < nc; i++) {
    const uint64_t len = row[i + 1] - row[i];
    if (drop && len < 2) continue;
    bool join = false;
    if (before) {
      const uint64_t a = before - 1;
      join = pieces_join(origin[a], left[a], right[a], xy + 2 * ((uint64_t) row[a + 1] - 1), origin[i], left[i], right[i],
                         xy + 2 * (uint64_t) row[i]);
    }
    add_points[i] = join ? len - 1 : len;
    add_chains[i] = join ? 0 : 1;
    before = i + 1;
  }
  for (uint64_t i = 0; i < nc; i++) {
    base_points[i + 1] = base_points[i] + add_points[i];
    base_chains[i + 1] = base_chains[i] + add_chains[i];
  }
  for (uint64_t i = 0; i < nc; i++) {
    const uint64_t skip = add_chains[i] ? 0 : 1;  // the first point of a piece that starts no chain stays behind
    for (uint64_t at = skip; at < (uint64_t) (row[i + 1] - row[i]); at++) {
      const uint64_t to = base_points[i] + at - skip;
      if (to < point_cap) {
        out_xy[2 * to] = xy[2 * ((uint64_t) row[i] + at)];
        out_xy[2 * to + 1] = xy[2 * ((uint64_t) row[i] + at) + 1];
      }
    }
    if (!add_chains[i] || base_chains[i] >= chain_cap) continue;
    out_row[base_chains[i]] = (uint32_t) base_points[i];
    out_left[base_chains[i]] = left[i];
    out_right[base_chains[i]] = right[i];
    out_origin[base_chains[i]] = origin[i];
  }
  if (base_chains[nc] <= chain_cap) out_row[base_chains[nc]] = (uint32_t) base_points[nc];
  counts[0] = base_chains[nc];
  counts[1] = base_points[nc];
  return base_chains[nc] > chain_cap || base_points[nc] > point_cap ? 1 : 0;
}

// the rule alone, on face ids
extern "C" int overlay_merge_joins(uint32_t origin_a, int32_t left_a, int32_t right_a, const int64_t* last_a, uint32_t origin_b, int32_t left_b,
                                   int32_t right_b, const int64_t* first_b) {
  return pieces_join(origin_a, left_a, right_a, last_a, origin_b, left_b, right_b, first_b) ? 1 : 0;
}
