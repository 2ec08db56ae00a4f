// Host twin of rj_neighbours.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_neighbours.h run as plain loops, in the device's stage order -- the check and the chain sums, the
// sides sorted and summed by label, the edge keys, under kVertex the incidences sorted by (point, label), their flags,
// slots and node pairs, then all directed keys sorted and summed, the counters of every face and the output.
// tests/test_neighbours.py holds it equal to the plain-Python definition (tests/neighbours_ref.py);
// tests/test_gpu_neighbours.py holds the device equal to both.  With NEIGHBOURS_TWIN_MAIN it is a stand-alone program that
// reads cases with their answers from a file: what a host sanitizer run is made of.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_neighbours.h"

using namespace rj::neighbours;
namespace el = rj::eliminate;
namespace rg = rj::rings;

extern "C" {

// -> 0, 1 (flags, sizes, a malformed map, too many node pairs: *counts holds n_node_pairs_raw then) or 3 (a count above its
// capacity: *counts holds the true counts, nothing is written), the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  faces
// may be null; offsets and entries where their capacities are 0.
int neighbours_twin(const int64_t* xy, uint64_t np, const uint32_t* row, const int32_t* left, const int32_t* right, uint64_t nc, uint32_t flags,
                    uint64_t face_cap, uint64_t entry_cap, Face* faces, uint64_t* offsets, Entry* entries, Counts* counts) {
  memset(counts, 0, sizeof(Counts));
  if (flags & ~kVertex) return 1;
  const bool vertex = (flags & kVertex) != 0;
  if (nc >= (1ull << 31) || np >= (1ull << 32) || nc > np || 2 * (np - nc) >= (1ull << 32) || (nc == 0 && np != 0)) return 1;
  if (vertex && nc >= (1ull << 30)) return 1;
  if (((face_cap || entry_cap) && !offsets) || (entry_cap && !entries)) return 1;
  if (nc == 0) {
    if (offsets) offsets[0] = 0;
    return 0;
  }
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. the check, the chain sums
  for (uint64_t c = 0; c <= nc; c++) meta.bad = std::max(meta.bad, rg::check_row(c, row, nc, np));
  if (meta.bad) return 1;
  std::vector<U128> S(nc), L(nc);
  for (uint64_t c = 0; c < nc; c++) {
    i128 s = 0;
    u128 l = 0;
    chain_sums(c, 0, 1, xy, row, np, &meta.bad, &s, &l);
    S[c] = rg::limbs(s);
    L[c] = limbs(l);
  }
  if (meta.bad) return 1;
  // 2. the faces: the sides sorted by key, the unique keys, their sums
  const uint64_t ns = 2 * nc;
  std::vector<uint32_t> side(ns);
  std::iota(side.begin(), side.end(), 0u);
  std::stable_sort(side.begin(), side.end(), [&](uint32_t a, uint32_t b) { return el::side_key(a, left, right) < el::side_key(b, left, right); });
  std::vector<uint32_t> keys;
  std::vector<FaceSum> fsum;
  for (uint32_t i : side) {
    const uint32_t k = el::side_key(i, left, right);
    const FaceSum v = side_val(i, left, right, S.data(), L.data());
    if (keys.empty() || keys.back() != k) {
      keys.push_back(k);
      fsum.push_back(v);
    } else {
      fsum.back() = face_add(fsum.back(), v);
    }
  }
  meta.n_keys = keys.size();
  const uint64_t nf = meta.counts.n_faces = el::count_faces(meta.n_keys, keys.data());
  // 3. the edge pairs
  std::vector<uint64_t> key(ns);
  std::vector<uint32_t> from(ns);  // the chain side that gave a key, kNoSide for a node's
  for (uint64_t i = 0; i < ns; i++) {
    key[i] = el::directed_key(i, left, right, keys.data(), nf);
    from[i] = (uint32_t) i;
  }
  // 4. the nodes
  if (vertex) {
    const uint64_t ni = 4 * nc;
    std::vector<Pt> pts(ns);
    std::vector<uint32_t> ikey(ni), order(ni), slot_face(ni), slot_node(ni), node_start(ns + 1);
    for (uint64_t h = 0; h < ns; h++) pts[h] = end_point(h, xy, row);
    for (uint64_t j = 0; j < ni; j++) ikey[j] = inc_key(j, left, right);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return inc_before(a, b, pts.data(), ikey.data()); });
    std::vector<Flags> mine(ni), before(ni);
    Flags run{0, 0};
    for (uint64_t k = 0; k < ni; k++) {
      mine[k] = flags_val(inc_flags(k, order.data(), pts.data(), ikey.data()));
      before[k] = run;
      run = flags_add(run, mine[k]);
    }
    for (uint64_t k = 0; k < ni; k++)
      inc_place(k, order.data(), ikey.data(), mine.data(), before.data(), keys.data(), nf, slot_face.data(), slot_node.data(), node_start.data());
    meta.n_slots = run.uniq;
    meta.counts.n_nodes = run.head;
    node_start[run.head] = run.uniq;
    std::vector<uint64_t> at(meta.n_slots + 1);
    uint64_t total = 0;
    for (uint64_t u = 0; u < meta.n_slots; u++) {
      const uint32_t m = labels_at(u, slot_node.data(), node_start.data());
      meta.max_labels = std::max(meta.max_labels, m);
      at[u] = total;
      total = saturating_add(total, m - 1);
    }
    meta.counts.n_node_pairs_raw = total;
    meta.counts.max_labels_at_node = meta.max_labels;
    if (refused(meta)) {
      counts->n_node_pairs_raw = total;
      return 1;
    }
    key.resize(ns + total);
    from.resize(ns + total);
    for (uint64_t u = 0; u < meta.n_slots; u++) node_pairs(u, slot_face.data(), slot_node.data(), node_start.data(), ns + at[u], key.data(), from.data());
  }
  // 5. the table: all directed keys sorted and summed, the counters of every face, the output: all or nothing
  std::vector<uint64_t> by(key.size());
  std::iota(by.begin(), by.end(), 0ull);
  std::stable_sort(by.begin(), by.end(), [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
  std::vector<uint64_t> dir;
  std::vector<PairSum> sums;
  for (uint64_t i : by) {
    if (dir.empty() || dir.back() != key[i]) {
      dir.push_back(key[i]);
      sums.push_back(pair_val(from[i], L.data()));
    } else {
      sums.back() = pair_add(sums.back(), pair_val(from[i], L.data()));
    }
  }
  meta.n_dir = dir.size();
  const uint64_t n_entries = meta.counts.n_entries = count_entries(meta.n_dir, dir.data());
  std::vector<uint32_t> n_edge(nf, 0), n_vertex(nf, 0);
  for (uint64_t i = 0; i < n_entries; i++) {
    const uint32_t f = el::from_of(dir[i]), g = el::to_of(dir[i]);
    const bool edge = is_edge(sums[i]);
    (edge ? n_edge : n_vertex)[f]++;
    if (f < g) (edge ? meta.counts.n_edge_pairs : meta.counts.n_vertex_pairs)++;
  }
  *counts = meta.counts;
  if (!fits(meta.counts, face_cap, entry_cap)) return 3;
  if (faces)
    for (uint64_t k = 0; k < nf; k++) faces[k] = face_record(k, keys.data(), fsum.data(), n_edge.data(), n_vertex.data());
  if (offsets)
    for (uint64_t k = 0; k <= nf; k++) offsets[k] = face_offset(k, dir.data(), n_entries);
  for (uint64_t i = 0; i < n_entries; i++) entries[i] = entry_of(i, dir.data(), sums.data(), keys.data());
  return 0;
}

}  // extern "C"

#if defined(NEIGHBOURS_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_neighbours.py writes, case after case:
//   np nc flags | xy[2 np] row[nc + 1] left[nc] right[nc] | status counts[7]
//   | n_faces x (label n_sides n_edge_nbrs n_vertex_nbrs area2_lo area2_hi perimeter_lo perimeter_hi outer_lo outer_hi)
//   | offsets[n_faces + 1] | n_entries x (label face n_chains n_nodes w_lo w_hi)       (the outputs only where status is 0)
// Every case runs as the sizing call, then with the exact capacities and records.
static bool more(FILE* f, long long* v) { return fscanf(f, "%lld", v) == 1; }
static unsigned long long word(FILE* f) {
  unsigned long long v = 0;
  if (fscanf(f, "%llu", &v) != 1) exit(2);
  return v;
}
static long long num(FILE* f) {
  long long v = 0;
  if (fscanf(f, "%lld", &v) != 1) exit(2);
  return v;
}
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  int failures = 0, cases = 0;
  long long first;
  while (more(f, &first)) {
    const uint64_t np = (uint64_t) first, nc = word(f);
    const uint32_t flags = (uint32_t) word(f);
    std::vector<int64_t> xy(2 * np);
    std::vector<uint32_t> row(nc + 1);
    std::vector<int32_t> left(nc), right(nc);
    for (auto& v : xy) v = num(f);
    for (auto& v : row) v = (uint32_t) word(f);
    for (auto& v : left) v = (int32_t) num(f);
    for (auto& v : right) v = (int32_t) num(f);
    const int want_status = (int) num(f);
    uint64_t want[7];
    for (auto& v : want) v = word(f);
    Counts c0, c1;
    const int s0 = neighbours_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, flags, 0, 0, nullptr, nullptr, nullptr, &c0);
    bool ok = !memcmp(&c0, want, sizeof(want));
    if (want_status != 0) {
      ok = ok && s0 == want_status;
    } else {
      ok = ok && (s0 == 0 || s0 == 3);
      const uint64_t nf = c0.n_faces, ne = c0.n_entries;
      std::vector<Face> faces(nf);
      std::vector<uint64_t> offsets(nf + 1);
      std::vector<Entry> entries(ne);
      const int s1 = neighbours_twin(xy.data(), np, row.data(), left.data(), right.data(), nc, flags, nf, ne, faces.data(), offsets.data(), entries.data(), &c1);
      ok = ok && s1 == 0 && !memcmp(&c1, want, sizeof(want));
      for (uint64_t k = 0; k < nf; k++) {
        Face w;
        w.label = (int32_t) num(f);
        w.n_sides = (uint32_t) word(f);
        w.n_edge_nbrs = (uint32_t) word(f);
        w.n_vertex_nbrs = (uint32_t) word(f);
        w.area2_lo = word(f);
        w.area2_hi = num(f);
        w.perimeter_lo = word(f);
        w.perimeter_hi = word(f);
        w.outer_lo = word(f);
        w.outer_hi = word(f);
        const Face& g = faces[k];
        ok = ok && g.label == w.label && g.n_sides == w.n_sides && g.n_edge_nbrs == w.n_edge_nbrs && g.n_vertex_nbrs == w.n_vertex_nbrs &&
             g.area2_lo == w.area2_lo && g.area2_hi == w.area2_hi && g.perimeter_lo == w.perimeter_lo && g.perimeter_hi == w.perimeter_hi &&
             g.outer_lo == w.outer_lo && g.outer_hi == w.outer_hi;
      }
      for (uint64_t k = 0; k <= nf; k++) ok = (offsets[k] == word(f)) && ok;
      for (uint64_t i = 0; i < ne; i++) {
        Entry w;
        w.label = (int32_t) num(f);
        w.face = (uint32_t) word(f);
        w.n_chains = (uint32_t) word(f);
        w.n_nodes = (uint32_t) word(f);
        w.w_lo = word(f);
        w.w_hi = word(f);
        const Entry& g = entries[i];
        ok = ok && g.label == w.label && g.face == w.face && g.n_chains == w.n_chains && g.n_nodes == w.n_nodes && g.w_lo == w.w_lo && g.w_hi == w.w_hi;
      }
    }
    printf("case %d: %llu chains, %llu points, flags %u -> %llu faces, %llu entries: %s\n", cases, (unsigned long long) nc, (unsigned long long) np, flags,
           (unsigned long long) c0.n_faces, (unsigned long long) c0.n_entries, ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
