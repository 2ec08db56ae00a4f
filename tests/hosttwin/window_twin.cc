// Host twin of rj_window.hip (test infrastructure, never a fallback): the per-element functions of
// rayjoin_amd/csrc/rj_window.h run as a brute force over ALL edges, through the device's own pipeline -- every window is
// normalised and quantised; every edge with its own quantised box goes through box_overlaps (the prune), box_inside (the
// containment shortcut: a hit without a test) and meets; a hit is counted and appended as a key while there is room; the
// counts are scanned; the keys are sorted over key_bits(nw) bits only, stably; eid and flags are recomputed from the sorted
// keys.  Windows and edges are taken in ascending or in descending order (the result must not depend on it), with or
// without the shortcut, with or without the prune.  tests/test_window.py holds it equal to the plain-Python definition
// (tests/window_ref.py); tests/test_gpu_window.py holds the device equal to it.  With WINDOW_TWIN_MAIN it is a stand-alone
// program that reads cases with their answers from a file: what a host sanitizer run is made of.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rj_window.h"

using namespace rj::window;
using rj::Seg;
using rj::nearest::cell_of;
using rj::within::key_bits;
using rj::within::key_eid;
using rj::within::key_point;
using rj::within::pair_key;

extern "C" {

// seg[ne][4] = (ax, ay, bx, by) in eid order; win[nw][4].  capacity 0: the counting call.  offsets[nw + 1], flags and work
// ([0] pairs tested exactly, [1] pairs handed out by containment) may be null; eid may be null in the counting call.
// counts[3] = n_pairs, n_windows_hit, max_per_window.  -> 0; 1 for a bad nw or capacity or a null pointer (nothing
// written); 3 when the pairs do not fit (counts and offsets written, nothing else).
int window_twin(const int64_t* seg, uint64_t ne, const int64_t* win, uint64_t nw, int reverse, int contained, int prune, uint64_t capacity, uint64_t* offsets,
                uint32_t* eid, uint8_t* flags, uint64_t* counts, uint64_t* work) {
  if (nw >= kMaxWindows || capacity >= kMaxWindows || !counts || (nw && !win) || (capacity && !eid)) return 1;
  std::vector<int32_t> bx0(ne), by0(ne), bx1(ne), by1(ne);
  for (uint64_t e = 0; e < ne; e++) {
    const int64_t* s = seg + 4 * e;
    bx0[e] = cell_of(s[0] < s[2] ? s[0] : s[2]), bx1[e] = cell_of(s[0] < s[2] ? s[2] : s[0]);
    by0[e] = cell_of(s[1] < s[3] ? s[1] : s[3]), by1[e] = cell_of(s[1] < s[3] ? s[3] : s[1]);
  }
  std::vector<uint32_t> cnt(nw + 1, 0);
  std::vector<uint64_t> keys(capacity);
  uint64_t appended = 0, tested = 0, handed = 0;
  for (uint64_t t = 0; t < nw; t++) {
    const uint64_t i = reverse ? nw - 1 - t : t;
    Win W = {win[4 * i], win[4 * i + 1], win[4 * i + 2], win[4 * i + 3]};
    if (!normalise(&W)) continue;
    const QWin Q = quantise(W);
    for (uint64_t k = 0; k < ne; k++) {
      const uint64_t e = reverse ? ne - 1 - k : k;
      if (prune && !box_overlaps(bx0[e], by0[e], bx1[e], by1[e], Q)) continue;
      bool hit;
      if (contained && box_inside(bx0[e], by0[e], bx1[e], by1[e], Q)) {
        hit = true;
        handed++;
      } else {
        const Seg s = {seg[4 * e], seg[4 * e + 1], seg[4 * e + 2], seg[4 * e + 3]};
        uint32_t f;
        hit = meets(s, W, &f);
        tested++;
      }
      if (!hit) continue;
      cnt[i]++;
      if (appended < capacity) keys[appended] = pair_key((uint32_t) i, (uint32_t) e);
      appended++;  // (a position at or behind the capacity is counted and not written)
    }
  }
  // the scan and the totals
  std::vector<uint64_t> scanned(nw + 1, 0);
  uint64_t hit = 0, longest = 0;
  for (uint64_t i = 0; i < nw; i++) {
    scanned[i + 1] = scanned[i] + cnt[i];
    hit += cnt[i] != 0;
    longest = cnt[i] > longest ? cnt[i] : longest;
  }
  const uint64_t n_pairs = scanned[nw];
  if (n_pairs != appended) return 5;
  counts[0] = n_pairs, counts[1] = hit, counts[2] = longest;
  if (work) work[0] = tested, work[1] = handed;
  if (offsets) memcpy(offsets, scanned.data(), (nw + 1) * sizeof(uint64_t));
  if (!capacity) return 0;
  if (n_pairs > capacity) return 3;
  // the sort over the bits in use, and the outputs from the sorted keys
  const int bits = key_bits(nw);
  const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
  keys.resize(n_pairs);
  std::stable_sort(keys.begin(), keys.end(), [mask](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });
  for (uint64_t k = 0; k < n_pairs; k++) {
    const uint32_t e = key_eid(keys[k]), w = key_point(keys[k]);
    eid[k] = e;
    if (!flags) continue;
    if (e >= ne || w >= nw) return 5;  // (a mutated key: nothing to recompute from)
    Win W = {win[4 * (uint64_t) w], win[4 * (uint64_t) w + 1], win[4 * (uint64_t) w + 2], win[4 * (uint64_t) w + 3]};
    const Seg s = {seg[4 * (uint64_t) e], seg[4 * (uint64_t) e + 1], seg[4 * (uint64_t) e + 2], seg[4 * (uint64_t) e + 3]};
    flags[k] = normalise(&W) ? (uint8_t) end_flags(s, W) : (uint8_t) 0;
  }
  return 0;
}

// the exact predicate alone on one segment and one window as given (normalised here): -1 no, otherwise the flags
int window_meets(const int64_t* s, const int64_t* w) {
  Win W = {w[0], w[1], w[2], w[3]};
  if (!normalise(&W)) return -1;
  uint32_t f;
  return meets(Seg{s[0], s[1], s[2], s[3]}, W, &f) ? (int) f : -1;
}
// the clamp: w is normalised in place; -> 0 when it lists nothing
int window_normalise(int64_t* w) {
  Win W = {w[0], w[1], w[2], w[3]};
  const bool live = normalise(&W);
  w[0] = W.x0, w[1] = W.y0, w[2] = W.x1, w[3] = W.y1;
  return live ? 1 : 0;
}
// the two box functions for the box b = {x0, y0, x1, y1} in cells against the window w as given: bit 0 overlaps, bit 1
// inside; -1: the window lists nothing
int window_box(const int32_t* b, const int64_t* w) {
  Win W = {w[0], w[1], w[2], w[3]};
  if (!normalise(&W)) return -1;
  const QWin Q = quantise(W);
  return (box_overlaps(b[0], b[1], b[2], b[3], Q) ? 1 : 0) | (box_inside(b[0], b[1], b[2], b[3], Q) ? 2 : 0);
}

}  // extern "C"

#if defined(WINDOW_TWIN_MAIN)
// argv[1]: a file of whitespace-separated integers that tests/test_window.py writes, case after case:
//   ne nw n_pairs | seg[ne][4] | win[nw][4] | offsets[nw + 1] | n_pairs x (eid flags)
// Every case runs in both orders, with and without the shortcut and the prune, at a capacity of one more; then the
// counting call and, where there are two pairs, the overflow at one less.
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
  while (fscanf(f, "%lld", &first) == 1) {
    const uint64_t ne = (uint64_t) first, nw = (uint64_t) num(f), n_pairs = (uint64_t) num(f);
    std::vector<int64_t> seg(4 * ne), win(4 * nw);
    for (auto& v : seg) v = num(f);
    for (auto& v : win) v = num(f);
    std::vector<uint64_t> want_off(nw + 1);
    for (auto& v : want_off) v = (uint64_t) num(f);
    std::vector<uint32_t> want_eid(n_pairs);
    std::vector<uint8_t> want_flags(n_pairs);
    for (uint64_t k = 0; k < n_pairs; k++) want_eid[k] = (uint32_t) num(f), want_flags[k] = (uint8_t) num(f);
    bool ok = true;
    for (int variant = 0; variant < 8; variant++) {
      const int rev = variant & 1, con = (variant >> 1) & 1, pru = (variant >> 2) & 1;
      std::vector<uint64_t> off(nw + 1), off2(nw + 1);
      std::vector<uint32_t> eid(n_pairs + 1);
      std::vector<uint8_t> flags(n_pairs + 1);
      uint64_t counts[3] = {0, 0, 0}, counted[3] = {0, 0, 0};
      ok = ok && window_twin(seg.data(), ne, win.data(), nw, rev, con, pru, n_pairs + 1, off.data(), eid.data(), flags.data(), counts, nullptr) == 0 &&
           counts[0] == n_pairs && off == want_off;
      for (uint64_t k = 0; ok && k < n_pairs; k++) ok = eid[k] == want_eid[k] && flags[k] == want_flags[k];
      ok = ok && window_twin(seg.data(), ne, win.data(), nw, rev, con, pru, 0, off2.data(), nullptr, nullptr, counted, nullptr) == 0 && off2 == want_off &&
           counted[0] == n_pairs;
      if (n_pairs > 1)
        ok = ok && window_twin(seg.data(), ne, win.data(), nw, rev, con, pru, n_pairs - 1, off2.data(), eid.data(), nullptr, counted, nullptr) == 3 &&
             counted[0] == n_pairs;
    }
    printf("case %d: %llu edges, %llu windows, %llu pairs: %s\n", cases, (unsigned long long) ne, (unsigned long long) nw, (unsigned long long) n_pairs,
           ok ? "ok" : "MISMATCH");
    failures += !ok;
    cases++;
  }
  fclose(f);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
#endif
