// Test-only host twin of the overlay operations: side_key / emit_sides / edge_contributions / edge_emit of
// rayjoin_amd/csrc/rj_overlay_ops.h -- the very source the HIP kernels k_ovf_contrib_op (rj_overlay.hip) and k_ovm_emit_op
// (rj_overlay_map.hip) run -- driven by plain loops over the edges like overlay_faces_twin.cc and overlay_map_twin.cc:
// std::sort and a serial sum for the face table; std::sort + std::unique for the face numbering and a serial pass for the
// drop flag for the output map.  Never linked into the product; the product path is HIP.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "rj_overlay_ops.h"

using namespace rj::overlay;

// 1 when how / by name an operation, and what selected() says of a pair (the truth table, for the tests)
extern "C" int overlay_ops_selected(uint32_t how, int32_t f0, int32_t f1) { return how < kHowCount && selected(how, f0, f1) ? 1 : 0; }

// the face table under (how, by): rows ascending by key; returns 1 when there are more than `capacity`
extern "C" int overlay_ops_faces_twin(const int64_t* const pts[2], const uint32_t* const row_index[2], const uint64_t nc[2],
                                  const int32_t* const left[2], const int32_t* const right[2], const void* const xsects[2],
                                  const int32_t* const vertex_face[2], uint64_t n, uint64_t capacity, int32_t* out_face,
                                  uint64_t* out_lo, int64_t* out_hi, uint64_t* n_rows, uint32_t how, uint32_t by) {
  const Op op = make_op(how, by);
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
      edge_contributions(im, e, pts[im], chain.data(), eb.data(), left[im], right[im], xs, n, vertex_face[im], op,
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

// the output map under (how, by).  counts[3] = chains, points, faces (the true counts); returns 1 when one of them exceeds its capacity (nothing is
// written beyond any capacity)
extern "C" int overlay_ops_map_twin(const int64_t* const pts[2], const uint32_t* const row_index[2], const uint64_t nc[2],
                                const int32_t* const left[2], const int32_t* const right[2], const void* const xsects[2],
                                const int32_t* const vertex_face[2], uint64_t n, int drop, uint64_t chain_cap, uint64_t point_cap,
                                uint64_t face_cap, int64_t* xy, uint32_t* out_row, int32_t* out_left, int32_t* out_right,
                                int32_t* face_pairs, uint32_t* origin, uint64_t* counts, uint32_t how, uint32_t by) {
  const Op op = make_op(how, by);
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
          im, e, c, lo, hi, tail, pts[im], eb.data(), left[im], right[im], xs, vertex_face[im], op,
          [&](int32_t label) {
            raw_row.push_back(raw_xy.size() / 2);
            raw_origin.push_back(((uint32_t) im << 31) | c);
            keys.push_back(side_key(im, left[im][c], label, op));
            keys.push_back(side_key(im, right[im][c], label, op));
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
