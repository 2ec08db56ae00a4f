"""Every edge within a distance of each point on the CPU: the plain-Python definition (tests/within_ref.py) on the hand cases
of tests/within_cases.py with the answers written out; the host twin of the device's pipeline
(tests/hosttwin/within_twin.cc compiling rayjoin_amd/csrc/rj_within.h on rj_nearest.h) against that definition in both
orders, with and without the double filter and the prune: the hand cases and a few hundred random small maps at 2^10, 2^30
and 2^46 scale with integer lattices where ties abound; the counting call and the overflow; the filter against exact
fractions around its margins; the group's lower bound below every point's; the bits of the key; three mutations of a
scratch copy of the header, each caught by a named hand case; the twin as a stand-alone program under the host sanitizers.
The GPU side is tests/test_gpu_within.py."""
import ctypes as C
import math
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref as NR  # noqa: E402
import within_cases as WC  # noqa: E402
import within_ref as WR  # noqa: E402
from test_nearest import CXX, NEAR_DTYPE, check_dist, random_map, seg_array, tuples_of  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "within_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
VARIANTS = [(reverse, filt, prune) for reverse in (0, 1) for filt in (0, 1) for prune in (0, 1)]
OK, INVALID, OVERFLOW = 0, 1, 3
CANARY32, CANARY_F = 0x5B5B5B5B, -7.0


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_within.h"), os.path.join(CSRC, "rj_nearest.h"), os.path.join(CSRC, "rj_predicates.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libwithin_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(CXX + ["-fPIC", "-shared", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.within_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 6
    L.within_in_or_out.argtypes = [C.c_double, C.c_double]
    L.within_key_bits.argtypes = [C.c_uint64]
    L.within_pair_key.argtypes = [C.c_uint32, C.c_uint32]
    L.within_pair_key.restype = C.c_uint64
    L.within_group_lb2.argtypes = [C.c_void_p, C.c_void_p]
    L.within_point_lb2.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.within_group_lb2.restype = L.within_point_lb2.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def call_twin(L, seg, points, max_dist, reverse=0, filt=1, prune=1, capacity=None, records=True, dist=True, offsets=True):
    """the raw call with canaries behind every array -> (rc, counts, offsets, eid, rec, dist, evaluated); capacity None: the
    counting call first, then the exact capacity"""
    seg = np.ascontiguousarray(seg, dtype=np.int64).reshape(-1, 4)
    pts = np.ascontiguousarray(points, dtype=np.int64).reshape(-1, 2)
    n = len(pts)
    counts = np.zeros(3, np.uint64)
    if capacity is None:
        rc = L.within_twin(seg.ctypes.data, len(seg), pts.ctypes.data, n, max_dist, reverse, filt, prune, 0, None, None, None, None, counts.ctypes.data, None)
        assert rc == OK
        capacity = int(counts[0])
    off = np.full(n + 2, 0x5B5B5B5B5B5B5B5B, np.uint64)
    eid, rec, dst = np.full(capacity + 1, CANARY32, np.uint32), np.zeros(capacity + 1, NEAR_DTYPE), np.full(capacity + 1, CANARY_F)
    rec.view(np.uint32)[:] = CANARY32
    evaluated = np.zeros(n + 1, np.uint64)
    counts[:] = 77
    rc = L.within_twin(seg.ctypes.data, len(seg), pts.ctypes.data, n, max_dist, reverse, filt, prune, capacity, off.ctypes.data if offsets else None,
                       eid.ctypes.data, rec.ctypes.data if records else None, dst.ctypes.data if dist else None, counts.ctypes.data, evaluated.ctypes.data)
    assert off[n + 1] == 0x5B5B5B5B5B5B5B5B and eid[capacity] == CANARY32 and dst[capacity] == CANARY_F and (rec.view(np.uint32)[10 * capacity:] == CANARY32).all()
    return rc, [int(v) for v in counts], off[:n + 1], eid[:capacity], rec[:capacity], dst[:capacity], evaluated[:n]


def run_twin(L, seg, points, max_dist, reverse=0, filt=1, prune=1, want_evaluated=False):
    """-> (per-point lists of tuples, dist per pair, counts[, evaluated]); offsets, eids and counts are checked for consistency"""
    rc, counts, off, eid, rec, dst, evaluated = call_twin(L, seg, points, max_dist, reverse, filt, prune)
    assert rc == OK
    n_pairs = counts[0]
    assert off[0] == 0 and off[-1] == n_pairs == len(eid) and (np.diff(off.astype(np.int64)) >= 0).all()
    assert eid.tolist() == rec["eid"].tolist()
    flat = tuples_of(rec)
    lists = [flat[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    lens = [len(r) for r in lists]
    assert counts == [n_pairs, sum(v > 0 for v in lens), max(lens, default=0)]
    out = (lists, dst, counts)
    return out + (evaluated,) if want_evaluated else out


def check_case(L, c, variants=VARIANTS):
    edges = NR.edges_of(c.pts, c.row)
    seg = seg_array(edges)
    want = WR.within_all(c.points, edges, c.max_dist)
    for reverse, filt, prune in variants:
        got, dist, _ = run_twin(L, seg, c.points, c.max_dist, reverse, filt, prune)
        assert got == want, (reverse, filt, prune)
        check_dist([t for row in got for t in row], dist)
    return want


# ---- the definition and the twin on the hand cases ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_definition_gives_the_written_answers(name):
    c = WC.HAND[name]
    assert WR.within_all(c.points, NR.edges_of(c.pts, c.row), c.max_dist) == c.want


@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_twin_gives_the_written_answers(twin, name):
    assert check_case(twin, WC.HAND[name]) == WC.HAND[name].want


def test_the_required_cases_are_there():
    assert {"three_four_five_in", "three_four_five_out", "non_integer_d2_in", "non_integer_d2_out", "zero_on_vertex_of_three_chains", "zero_on_interior_point",
            "chain_vertex_tie", "zero_length_edge", "dot_is_zero", "dot_is_l", "extremes_all", "cells_one_apart_in", "cells_one_apart_out", "cells_two_apart_in",
            "cells_two_apart_out", "empty_between", "one_edge", "one_point"} <= set(WC.HAND)
    c = WC.HAND["extremes_all"]
    assert c.max_dist == 1 << 48 and all(len(w) == len(NR.edges_of(c.pts, c.row)) for w in c.want)
    assert all(len(w) == 3 for w in WC.HAND["zero_on_vertex_of_three_chains"].want)
    assert [len(w) for w in WC.HAND["empty_between"].want] == [1, 0, 1]


# ---- refusals, the counting call and the overflow -------------------------------------------------------------------------
def test_refusals_counting_call_and_overflow(twin):
    c = WC.HAND["zero_on_vertex_of_three_chains"]
    seg = seg_array(NR.edges_of(c.pts, c.row))
    pts = np.array(c.points * 2 + [(1000, 1000)], np.int64)  # lists of 3, 3 and 0
    counts, out = np.full(3, 77, np.uint64), np.zeros(8, np.uint32)
    for md, cap, cnt, eid in [(-1, 8, counts, out), ((1 << 48) + 1, 8, counts, out), (0, 1 << 32, counts, out), (0, 8, None, out), (0, 8, counts, None)]:
        assert twin.within_twin(seg.ctypes.data, 3, pts.ctypes.data, 3, md, 0, 1, 1, cap, None, None if eid is None else eid.ctypes.data, None, None,
                                None if cnt is None else cnt.ctypes.data, None) == INVALID
        assert (counts == 77).all() and not out.any()
    for v in VARIANTS:
        rc, cnts, off, eid, rec, dst, _ = call_twin(twin, seg, pts, 0, *v, capacity=0)
        assert rc == OK and cnts == [6, 2, 3] and off.tolist() == [0, 3, 6, 6]
        rc, cnts, off, eid, rec, dst, _ = call_twin(twin, seg, pts, 0, *v, capacity=5)  # one short: true counts and offsets, nothing else
        assert rc == OVERFLOW and cnts == [6, 2, 3] and off.tolist() == [0, 3, 6, 6]
        assert (eid == CANARY32).all() and (rec.view(np.uint32) == CANARY32).all() and (dst == CANARY_F).all()
        rc, cnts, off, eid, rec, dst, _ = call_twin(twin, seg, pts, 0, *v, capacity=6, records=False, dist=False, offsets=False)
        assert rc == OK and eid.tolist() == [0, 1, 2, 0, 1, 2] and (rec.view(np.uint32) == CANARY32).all() and (dst == CANARY_F).all()
    # no points: zero counts, offsets[0] = 0
    rc, cnts, off, *_ = call_twin(twin, seg, np.zeros((0, 2), np.int64), 5, capacity=4)
    assert rc == OK and cnts == [0, 0, 0] and off.tolist() == [0]


# ---- random small maps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [10, 30, 46])
@pytest.mark.parametrize("lattice", [False, True], ids=["uniform", "lattice"])
def test_random_small_maps(twin, scale, lattice):
    rng = random.Random(2000 * scale + lattice)
    pairs = shared = longest = 0
    for k in range(60):
        nc = random_map(rng, scale, lattice)
        edges = NR.edges_of(nc.pts, nc.row)
        # radii: 0, the distance of some edge from the first point rounded down and up (equality and its neighbours), everything
        d2 = NR.d2_of(*NR.point_edge(*nc.points[0], edges[rng.randrange(len(edges))]))
        root = math.isqrt(d2.numerator // d2.denominator)
        for m in (0, root, min(root + 1, 1 << 48), 1 << 48 if k % 10 == 0 else root // 2):
            c = WC.Case(nc.pts, nc.row, nc.points, m, None)
            want = check_case(twin, c, VARIANTS if k % 6 == 0 else [(0, 1, 1), (1, 1, 1), (1, 0, 0)])
            pairs += sum(len(w) for w in want)
            longest = max(longest, max(len(w) for w in want))
            if m == 0:
                shared += sum(len(w) > 1 for w in want)
            if m == 1 << 48:
                assert all(len(w) == len(edges) for w in want)
    assert pairs > 1000 and longest >= 5, (pairs, longest)
    assert not lattice or shared > 100, shared  # (the lattices are there for the points on shared vertices)


# ---- the filter ---------------------------------------------------------------------------------------------------------
def test_filter_never_decides_against_the_exact_test(twin):
    """in_or_out on doubles within 2^-50 of d^2 and 2^-53 of max_dist^2, as the header's bound assumes: its verdict, where it
    gives one, is the exact one -- around the margins, at equality, at zero"""
    rng = random.Random(5)
    decided = undecided = 0
    for _ in range(20000):
        m = rng.choice((1, 2, 3, 1000, (1 << 24) + 1, (1 << 48) - 1, 1 << 48, rng.randrange(1, 1 << 48)))
        m2 = m * m
        # an exact d^2 near m^2: a relative offset of up to 2^-44 either way, or none
        off = rng.choice((0, 0, 1, -1)) * Fraction(rng.randrange(1, 1 << 10), 1 << rng.randrange(44, 70))
        d2 = m2 * (1 + off)
        # what the device may hold: anything within 2^-50 of d^2
        seen = float(d2 * (1 + Fraction(rng.randrange(-(1 << 9), (1 << 9) + 1), 1 << 60)))
        assert abs(Fraction(seen) - d2) <= d2 / (1 << 50)
        f = twin.within_in_or_out(seen, float(m) * float(m))
        if f:
            decided += 1
            assert (f > 0) == (d2 <= m2), (m, off, f)
        else:
            undecided += 1
    assert decided > 2000 and undecided > 2000, (decided, undecided)
    assert twin.within_in_or_out(0.0, 0.0) == 0 and twin.within_in_or_out(1.0 / (1 << 95), 0.0) == -1 and twin.within_in_or_out(0.0, 1.0) == 1
    assert twin.within_in_or_out(25.0, 25.0) == 0  # equality is the exact test's


# ---- the wave-uniform reject and the key ----------------------------------------------------------------------------------
def test_group_lower_bound_is_below_every_point_of_the_group(twin):
    rng = random.Random(13)
    positive = 0
    for _ in range(2000):
        half = 1 << rng.choice((18, 22, 30, 46))
        r = lambda: rng.randint(-half, half - 1)  # noqa: E731
        s = np.array([r(), r(), r(), r()], dtype=np.int64)
        span = rng.choice((0, 1 << 16, 1 << 20, half))
        cx, cy = r(), r()
        pts = [(max(-half, min(half - 1, cx + rng.randint(-span, span))), max(-half, min(half - 1, cy + rng.randint(-span, span)))) for _ in range(8)]
        cells = [((x + (1 << 46)) >> 16, (y + (1 << 46)) >> 16) for x, y in pts]
        g = np.array([min(c[0] for c in cells), min(c[1] for c in cells), max(c[0] for c in cells), max(c[1] for c in cells)], dtype=np.int32)
        lb = twin.within_group_lb2(s.ctypes.data, g.ctypes.data)
        per_point = [twin.within_point_lb2(s.ctypes.data, x, y) for x, y in pts]
        assert lb <= min(per_point)
        positive += lb > 0
        one = np.array([cells[0][0], cells[0][1], cells[0][0], cells[0][1]], dtype=np.int32)  # a group of one cell: the point's own bound
        assert twin.within_group_lb2(s.ctypes.data, one.ctypes.data) == per_point[0]
    assert positive > 300


def test_key_bits_and_packing(twin):
    assert [twin.within_key_bits(n) for n in (0, 1, 2, 3, 4, 5, 64, 65, 4097, (1 << 32) - 1)] == [32, 32, 33, 34, 34, 35, 38, 39, 45, 64]
    assert twin.within_pair_key(0, 7) == 7 and twin.within_pair_key(3, 0xFFFFFFFE) == (3 << 32) | 0xFFFFFFFE
    assert twin.within_pair_key(0xFFFFFFFF, 1) == (0xFFFFFFFF << 32) | 1


def test_the_prune_only_saves_work(twin):
    from rayjoin_amd import maps, synth
    m = maps.Context([synth.lattice_map(12, 5, 3)]).load().maps[0]
    seg, pts = m.segments(), m.pts[:300]
    md = 3 << 16
    full, _, _, n_full = run_twin(twin, seg, pts, md, prune=0, want_evaluated=True)
    pruned, _, _, n_pruned = run_twin(twin, seg, pts, md, prune=1, want_evaluated=True)
    assert full == pruned and (n_full == len(seg)).all() and sum(len(r) for r in full) > 300
    assert n_pruned.mean() < len(seg) / 4, (n_pruned.mean(), len(seg))


# ---- mutations of the header, each caught by a hand case -----------------------------------------------------------------
MUTATIONS = [
    # (tag, the text, its replacement, the hand case that catches it)
    ("filter_margin", "constexpr double kOut = 1.0 + 0x1p-48;", "constexpr double kOut = 1.0 - 0x1p-40;", "three_four_five_in"),
    ("key_bits_one_less", "return 32 + b;", "return 31 + b;", "second_point_smaller_eid"),
    ("key_shift", "return ((uint64_t) point << 32) | eid;", "return ((uint64_t) point << 31) | eid;", "second_point_smaller_eid"),
]


@pytest.mark.parametrize("tag,old,new,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught(tag, old, new, name, tmp_path):
    text = open(os.path.join(CSRC, "rj_within.h")).read()
    assert text.count(old) == 1
    with open(tmp_path / "rj_within.h", "w") as f:
        f.write(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mut_" + tag)
    c = WC.HAND[name]
    seg = seg_array(NR.edges_of(c.pts, c.row))
    flat = [t for row in c.want for t in row]
    wrong = []
    for v in VARIANTS:
        rc, counts, off, eid, rec, _, _ = call_twin(L, seg, c.points, c.max_dist, *v, capacity=len(flat) + 2)
        n = min(counts[0], len(eid))
        if rc != OK or tuples_of(rec[:n]) != flat or off.tolist() != WR.csr_of(c.want)[0]:
            wrong.append(v)
    assert wrong, "the mutant %s survives the hand case %s" % (tag, name)


# ---- the stand-alone twin under the host sanitizers ----------------------------------------------------------------------
def case_text(c):
    edges = NR.edges_of(c.pts, c.row)
    offsets, flat = WR.csr_of(c.want)
    words = [len(edges), len(c.points), c.max_dist, len(flat)] + [v for e in edges for v in e] + [v for p in c.points for v in p] + offsets
    for eid, where, num, den in flat:
        words += [eid, where, num & 0xFFFFFFFFFFFFFFFF, num >> 64, den & 0xFFFFFFFFFFFFFFFF, den >> 64]
    return " ".join(str(int(v)) for v in words)


def test_standalone_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "within_twin_san")
    subprocess.check_call(CXX[:1] + ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-DWITHIN_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(case_text(WC.HAND[k]) for k in sorted(WC.HAND)) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 failures" % len(WC.HAND) in r.stdout and "runtime error" not in r.stderr
