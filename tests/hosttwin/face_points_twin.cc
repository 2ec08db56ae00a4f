// Host twin of rj_face_points.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_face_points.h run as plain loops, in the device's stage order -- the universe checked or made from the
// sorted keys of the run heads, the table pass with its runs cut at every head and at every multiple of kWave, the records,
// the scanned offsets, the members by a stable sort of their face numbers.  tests/test_face_points.py holds it equal to the
// plain-Python definition (tests/face_points_ref.py); tests/test_gpu_face_points.py holds the device equal to both.  With
// FACE_POINTS_TWIN_MAIN it is a stand-alone program that reads cases with their answers from a file: what a host sanitizer
// run is made of.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "rj_face_points.h"

using namespace rj::face_points;
namespace el = rj::eliminate;

extern "C" {

// -> 0, 1 (flags, sizes, null arrays, a bad universe) or 3 (a count above its capacity: *counts holds the true counts,
// nothing is written), the values of RJ_OK, RJ_E_INVALID, RJ_E_OVERFLOW.  face_label null: no universe.  faces may be
// null; offsets and members are only looked at under kMembers.
int face_points_twin(const int32_t* label, uint64_t n, const int64_t* value, uint64_t stride, const int32_t* face_label, uint64_t nfl, uint32_t flags,
                     uint64_t face_cap, uint64_t member_cap, Face* faces, uint64_t* offsets, uint32_t* members, Counts* counts) {
  if (!counts) return 1;
  memset(counts, 0, sizeof(Counts));
  if (flags & ~kMembers) return 1;
  const bool with_members = (flags & kMembers) != 0;
  if (n && !label) return 1;
  if (n >= kMaxPoints || nfl >= kMaxPoints) return 1;
  if (value && stride == 0) return 1;
  if (nfl && !face_label) return 1;
  if (!with_members && member_cap) return 1;
  if ((face_cap && (with_members ? !offsets : !faces)) || (member_cap && !members)) return 1;
  Meta meta;
  memset(&meta, 0, sizeof(meta));
  // 1. the universe
  std::vector<uint32_t> keys;
  if (face_label) {
    keys.resize(nfl);
    for (uint64_t k = 0; k < nfl; k++) {
      if (universe_bad(k, face_label)) meta.bad = kBadUniverse;
      keys[k] = universe_key(k, face_label);
    }
    if (meta.bad) return 1;
    meta.counts.n_faces = nfl;
  } else {
    std::vector<uint32_t> heads;
    for (uint64_t i = 0; i < n; i++)
      if (is_head(i, label)) heads.push_back(head_key(i, label));
    meta.n_heads = heads.size();
    std::sort(heads.begin(), heads.end());
    heads.erase(std::unique(heads.begin(), heads.end()), heads.end());
    keys = heads;
    meta.n_keys = keys.size();
    meta.counts.n_faces = el::count_faces(meta.n_keys, keys.data());
  }
  const uint64_t nf = meta.counts.n_faces;
  // 2. the table pass: the lanes of a run one after the other, the run's last one applies it
  std::vector<Acc> acc(nf, acc_empty());
  Part p{};
  for (uint64_t i = 0; i < n; i++) {
    if (is_head(i, label)) meta.counts.n_runs++;
    const Part mine = part_of(i, value, stride);
    p = seg_head(i, label) ? mine : part_add(p, mine);
    if (i + 1 == n || seg_head(i + 1, label)) {
      const int where = run_apply(p, label[i], value != nullptr, keys.data(), nf, acc.data());
      if (where == kOutside) meta.counts.n_outside += p.n;
      if (where == kUnmatched) meta.counts.n_unmatched += p.n;
    }
  }
  // 3. the totals; all or nothing; the records and the offsets
  meta.counts.n_members = n - meta.counts.n_outside - meta.counts.n_unmatched;
  *counts = meta.counts;
  if (!fits(meta.counts, with_members, face_cap, member_cap)) return 3;
  if (faces)
    for (uint64_t k = 0; k < nf; k++) faces[k] = face_record(k, keys.data(), acc.data());
  if (with_members && offsets) {
    uint64_t at = 0;
    for (uint64_t k = 0; k < nf; k++) {
      offsets[k] = at;
      at += acc[k].n;
    }
    offsets[nf] = at;
  }
  // 4. the members: a stable sort of the points by member_key; the points that are no member fall off the end
  if (with_members && meta.counts.n_members) {
    std::vector<uint32_t> key(n), order(n);
    for (uint64_t i = 0; i < n; i++) key[i] = member_key(i, label, keys.data(), nf);
    const uint32_t mask = key_bits(nf) >= 32 ? 0xFFFFFFFFu : (1u << key_bits(nf)) - 1u;  // (the bits that the sort looks at)
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
    for (uint64_t i = 0; i < meta.counts.n_members; i++) members[i] = order[i];
  }
  return 0;
}

}  // extern "C"

#if defined(FACE_POINTS_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_face_points.py writes, case after case:
//   n stride has_values has_universe nfl flags (nv where has_values) | label[n] | value[nv] | face_label[nfl]
//   | status counts[5] | n_faces x (label first n_points sum_lo sum_hi min max) | under kMembers offsets[n_faces + 1] members[n_members]
//   (the outputs only where status is 0).  Every case runs as the sizing call, then with the exact capacities and records.
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
    const uint64_t n = (uint64_t) first, stride = word(f);
    const bool has_values = word(f) != 0, has_universe = word(f) != 0;
    const uint64_t nfl = word(f);
    const uint32_t flags = (uint32_t) word(f);
    const uint64_t nv = has_values ? word(f) : 0;
    std::vector<int32_t> label(n), universe(nfl + 1);  // (an empty universe is still an array)
    std::vector<int64_t> value(nv + 1);
    for (auto& v : label) v = (int32_t) num(f);
    for (uint64_t i = 0; i < nv; i++) value[i] = num(f);
    for (uint64_t k = 0; k < nfl; k++) universe[k] = (int32_t) num(f);
    const int want_status = (int) num(f);
    uint64_t want[5];
    for (auto& v : want) v = word(f);
    const int64_t* vp = has_values ? value.data() : nullptr;
    const int32_t* up = has_universe ? universe.data() : nullptr;
    Counts c0, c1;
    const int s0 = face_points_twin(label.data(), n, vp, stride, up, nfl, flags, 0, 0, nullptr, nullptr, nullptr, &c0);
    bool ok = !memcmp(&c0, want, sizeof(want));
    if (want_status != 0) {
      ok = ok && s0 == want_status;
    } else {
      ok = ok && (s0 == 0 || s0 == 3);
      const bool with_members = (flags & kMembers) != 0;
      const uint64_t nf = c0.n_faces, nm = with_members ? c0.n_members : 0;
      std::vector<Face> faces(nf);
      std::vector<uint64_t> offsets(nf + 1);
      std::vector<uint32_t> members(nm);
      const int s1 = face_points_twin(label.data(), n, vp, stride, up, nfl, flags, nf, nm, faces.data(), offsets.data(), members.data(), &c1);
      ok = ok && s1 == 0 && !memcmp(&c1, want, sizeof(want));
      for (uint64_t k = 0; k < nf; k++) {
        Face w;
        w.label = (int32_t) num(f);
        w.first = (uint32_t) word(f);
        w.n_points = word(f);
        w.sum_lo = word(f);
        w.sum_hi = num(f);
        w.min = num(f);
        w.max = num(f);
        const Face& g = faces[k];
        ok = ok && g.label == w.label && g.first == w.first && g.n_points == w.n_points && g.sum_lo == w.sum_lo && g.sum_hi == w.sum_hi && g.min == w.min &&
             g.max == w.max;
      }
      if (with_members) {
        for (uint64_t k = 0; k <= nf; k++) ok = (offsets[k] == word(f)) && ok;
        for (uint64_t i = 0; i < nm; i++) ok = (members[i] == word(f)) && ok;
      }
    }
    printf("case %d: %llu points, flags %u -> %llu faces, %llu members: %s\n", cases, (unsigned long long) n, flags, (unsigned long long) c0.n_faces,
           (unsigned long long) c0.n_members, ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
