// Test-only host twin of the overlay's output map: edge_emit of rayjoin_amd/csrc/rj_overlay_map.h -- the very source the
// HIP kernels of rj_overlay_map.hip run -- driven by a plain loop over the edges, std::sort + std::unique for the face
// numbering and a serial pass for the drop flag.  Never linked into the product; the product path is HIP.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rj_overlay_map.h"

using namespace rj::overlay;

// counts[3] = chains, points, faces (the true counts); returns 1 when one of them exceeds its capacity (nothing is
// written beyond any capacity)
extern "C" int overlay_map_twin(const int64_t* const pts[2], const uint32_t* const row_index[2], const uint64_t nc[2],
                                const int32_t* const left[2], const int32_t* const right[2], const void* const xsects[2],
                                const int32_t* const vertex_face[2], uint64_t n, int drop, uint64_t chain_cap, uint64_t point_cap,
                                uint64_t face_cap, int64_t* xy, uint32_t* out_row, int32_t* out_left, int32_t* out_right,
                                int32_t* face_pairs, uint32_t* origin, uint64_t* counts) {
  std::vector<int64_t> raw_xy;
  std::vector<uint64_t> raw_row, keys;  // keys: two per piece
  std::vector<uint32_t> raw_origin;
  for (int im = 0; im < 2; im++) {
    std::vector<uint32_t> eb(nc[im] + 1), chain;
    for (uint64_t k = 0; k <= nc[im]; k++) eb[k] = (uint32_t) (row_index[im][k] - k);
    const uint64_t ne = nc[im] ? eb[nc[im]] : 0;
    chain.resize(ne);
    for (uint64_t k = 0; k < nc[im]; k++)
      for (uint32_t e = eb[k]; e < eb[k + 1]; e++) chain[e] = (uint32_t) k;
    const Rec48* xs = static_cast<const Rec48*>(xsects[im]);
    for (uint64_t e = 0; e < ne; e++) {
      const uint32_t c = chain[e];
      const uint64_t lo = first_record_at(xs, 0, n, im, e), hi = first_record_at(xs, lo, n, im, e + 1);
      const int32_t tail = tail_label(xs, n, im, hi, c, eb.data(), vertex_face[im]);
      edge_emit(
          im, e, c, lo, hi, tail, pts[im], eb.data(), left[im], right[im], xs, vertex_face[im],
          [&](int32_t label) {
            raw_row.push_back(raw_xy.size() / 2);
            raw_origin.push_back(((uint32_t) im << 31) | c);
            keys.push_back(side_key(im, left[im][c], label));
            keys.push_back(side_key(im, right[im][c], label));
          },
          [&](int64_t x, int64_t y) {
            raw_xy.push_back(x);
            raw_xy.push_back(y);
          });
    }
  }
  raw_row.push_back(raw_xy.size() / 2);
  std::vector<uint64_t> uk(keys);
  std::sort(uk.begin(), uk.end());
  uk.erase(std::unique(uk.begin(), uk.end()), uk.end());
  if (!uk.empty() && uk.back() == kNoKey) uk.pop_back();
  const uint64_t nf = uk.size();
  for (uint64_t k = 0; k < nf && k < face_cap; k++) {
    face_pairs[2 * k] = (int32_t) (uint32_t) (uk[k] >> 32);
    face_pairs[2 * k + 1] = (int32_t) (uint32_t) uk[k];
  }
  uint64_t chains = 0, points = 0;
  for (uint64_t i = 0; i + 1 < raw_row.size(); i++) {
    const uint64_t b = raw_row[i], len = raw_row[i + 1] - b;
    if (drop && len < 2) continue;
    if (chains < chain_cap) {
      out_row[chains] = (uint32_t) points;
      out_left[chains] = keys[2 * i] == kNoKey ? 0 : (int32_t) (key_index(uk.data(), nf, keys[2 * i]) + 1);
      out_right[chains] = keys[2 * i + 1] == kNoKey ? 0 : (int32_t) (key_index(uk.data(), nf, keys[2 * i + 1]) + 1);
      if (origin) origin[chains] = raw_origin[i];
    }
    for (uint64_t k = 0; k < len; k++)
      if (points + k < point_cap) {
        xy[2 * (points + k)] = raw_xy[2 * (b + k)];
        xy[2 * (points + k) + 1] = raw_xy[2 * (b + k) + 1];
      }
    chains++;
    points += len;
  }
  if (chains <= chain_cap) out_row[chains] = (uint32_t) points;
  counts[0] = chains;
  counts[1] = points;
  counts[2] = nf;
  return chains > chain_cap || points > point_cap || nf > face_cap ? 1 : 0;
}
