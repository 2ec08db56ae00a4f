// Test-only host twin of the overlay's face table: the per-edge functions of rayjoin_amd/csrc/rj_overlay.h -- the very
// source the HIP kernels of rj_overlay.hip run -- driven by a plain loop over the edges, one contribution per sub-segment
// side (no merging inside a wave), std::sort and a serial sum.  Never linked into the product; the product path is HIP.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "rj_overlay.h"

using namespace rj::overlay;

extern "C" int overlay_faces_twin(const int64_t* const pts[2], const uint32_t* const row_index[2], const uint64_t nc[2],
                                  const int32_t* const left[2], const int32_t* const right[2], const void* const xsects[2],
                                  const int32_t* const vertex_face[2], uint64_t n, uint64_t capacity, int32_t* out_face,
                                  uint64_t* out_lo, int64_t* out_hi, uint64_t* n_rows) {
  std::vector<std::pair<uint64_t, __int128>> c;
  for (int im = 0; im < 2; im++) {
    std::vector<uint32_t> eb(nc[im] + 1), chain;
    for (uint64_t k = 0; k <= nc[im]; k++) eb[k] = (uint32_t) (row_index[im][k] - k);
    const uint64_t ne = nc[im] ? eb[nc[im]] : 0;
    chain.resize(ne);
    for (uint64_t k = 0; k < nc[im]; k++)
      for (uint32_t e = eb[k]; e < eb[k + 1]; e++) chain[e] = (uint32_t) k;
    const Rec48* xs = static_cast<const Rec48*>(xsects[im]);
    for (uint64_t e = 0; e < ne; e++)
      edge_contributions(im, e, pts[im], chain.data(), eb.data(), left[im], right[im], xs, n, vertex_face[im],
                         [&](uint64_t key, __int128 v) { c.emplace_back(key, v); });
  }
  std::sort(c.begin(), c.end(), [](const std::pair<uint64_t, __int128>& a, const std::pair<uint64_t, __int128>& b) { return a.first < b.first; });
  uint64_t rows = 0;
  for (size_t i = 0; i < c.size();) {
    size_t j = i;
    __int128 s = 0;
    for (; j < c.size() && c[j].first == c[i].first; j++) s += c[j].second;
    if (rows < capacity) {
      out_face[2 * rows] = (int32_t) (uint32_t) (c[i].first >> 32);
      out_face[2 * rows + 1] = (int32_t) (uint32_t) c[i].first;
      const Area2 a = to_limbs(s);
      out_lo[rows] = a.lo;
      out_hi[rows] = a.hi;
    }
    rows++;
    i = j;
  }
  *n_rows = rows;
  return rows > capacity ? 1 : 0;
}
