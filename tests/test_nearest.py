"""The nearest edge of a map for every point on the CPU: the plain-Python definition (tests/nearest_ref.py) on the hand
cases of tests/nearest_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/nearest_twin.cc compiling rayjoin_amd/csrc/rj_nearest.h) against that definition in both edge orders, with
and without the double filter and the prune: the hand cases and a few hundred random small maps at 2^10, 2^30 and 2^46 scale
with integer lattices where ties abound; the wide multiply and compare against Python integers; the box lower bound
strictly below the true distance and tight to two cells; dist within 2^-50; three mutations of a scratch copy of the header,
each caught by a named hand case; the twin as a stand-alone program under the host sanitizers.  The GPU side is
tests/test_gpu_nearest.py."""
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
import nearest_cases as NC  # noqa: E402
import nearest_ref as NR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "nearest_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
NEAR_DTYPE = np.dtype([("eid", "<u4"), ("where", "<u4"), ("num_lo", "<u8"), ("num_hi", "<i8"), ("den_lo", "<u8"), ("den_hi", "<u8")])
assert NEAR_DTYPE.itemsize == 40
VARIANTS = [(reverse, filt, prune) for reverse in (0, 1) for filt in (0, 1) for prune in (0, 1)]
CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"]


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_nearest.h"), os.path.join(CSRC, "rj_predicates.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libnearest_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(CXX + ["-fPIC", "-shared", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.nearest_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.nearest_wide_cmp.argtypes = [C.c_void_p] * 4
    L.nearest_wide_mul.argtypes = L.nearest_wide_mul3.argtypes = [C.c_void_p] * 3
    L.nearest_wide_mul.restype = L.nearest_wide_mul3.restype = None
    L.nearest_box_lb2.argtypes = L.nearest_ub2.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.nearest_box_lb2.restype = L.nearest_ub2.restype = C.c_uint64
    L.nearest_ub2_of_max_dist.argtypes = [C.c_int64]
    L.nearest_ub2_of_max_dist.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def seg_array(edges):
    return np.array(edges, dtype=np.int64).reshape(-1, 4)


def tuples_of(rec):
    """NEAR_DTYPE rows -> the (eid, where, num, den) tuples of nearest_ref, num signed"""
    return [(int(r["eid"]), int(r["where"]), (int(r["num_hi"]) << 64) + int(r["num_lo"]), (int(r["den_hi"]) << 64) + int(r["den_lo"])) for r in rec]


def run_twin(L, seg, points, max_dist=-1, reverse=0, filt=1, prune=1, want_evaluated=False):
    """-> (tuples, dist[, evaluated]); the eid array must equal the records' eids"""
    seg = np.ascontiguousarray(seg, dtype=np.int64).reshape(-1, 4)
    pts = np.ascontiguousarray(points, dtype=np.int64).reshape(-1, 2)
    n = len(pts)
    eid, rec, dist = np.full(n + 1, 0x5B5B5B5B, np.uint32), np.zeros(n + 1, NEAR_DTYPE), np.full(n + 1, -7.0)
    evaluated = np.zeros(n + 1, np.uint64)
    rc = L.nearest_twin(seg.ctypes.data, len(seg), pts.ctypes.data, n, max_dist, reverse, filt, prune, eid.ctypes.data, rec.ctypes.data, dist.ctypes.data,
                        evaluated.ctypes.data)
    assert rc == 0 and eid[n] == 0x5B5B5B5B and dist[n] == -7.0
    assert eid[:n].tolist() == rec["eid"][:n].tolist()
    out = (tuples_of(rec[:n]), dist[:n])
    return out + (evaluated[:n],) if want_evaluated else out


def check_dist(got, dist):
    """dist against Python integers: |dist - sqrt(N / D)| <= 2^-50 sqrt(N / D), that is dist^2 D within N (1 -+ 2^-50)^2, in exact
    fractions of the double; +inf on a miss"""
    for (eid, where, num, den), d in zip(got, dist):
        if eid == NR.MISS:
            assert d == math.inf
            continue
        d2, f = NR.d2_of(where, num, den), Fraction(float(d))
        eps = Fraction(1, 1 << 50)
        assert d2 * (1 - eps) ** 2 <= f * f <= d2 * (1 + eps) ** 2, (d2, d)
        if d2 > 0:  # (and against the integer square root of the scaled fraction: 100 bits behind the point)
            root = math.isqrt((d2.numerator << 200) // d2.denominator)
            assert abs(f * (1 << 100) - root) <= root * eps + 1


def check_case(L, c, variants=VARIANTS):
    seg = seg_array(NR.edges_of(c.pts, c.row))
    want = NR.nearest_all(c.points, NR.edges_of(c.pts, c.row), c.max_dist)
    for reverse, filt, prune in variants:
        got, dist = run_twin(L, seg, c.points, c.max_dist, reverse, filt, prune)
        assert got == want, (reverse, filt, prune)
        check_dist(got, dist)
    return want


# ---- the definition and the twin on the hand cases ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_definition_gives_the_written_answers(name):
    c = NC.HAND[name]
    assert NR.nearest_all(c.points, NR.edges_of(c.pts, c.row), c.max_dist) == c.want


@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_twin_gives_the_written_answers(twin, name):
    assert check_case(twin, NC.HAND[name]) == NC.HAND[name].want


def test_refusal_of_a_max_dist_above_the_limit(twin):
    seg, pts = seg_array([(0, 0, 1, 1)]), np.zeros((1, 2), np.int64)
    out = np.zeros(4, np.uint32)
    assert twin.nearest_twin(seg.ctypes.data, 1, pts.ctypes.data, 1, (1 << 48) + 1, 0, 1, 1, out.ctypes.data, None, None, None) == 1
    assert twin.nearest_twin(seg.ctypes.data, 1, pts.ctypes.data, 1, 1 << 48, 0, 1, 1, out.ctypes.data, None, None, None) == 0


# ---- random small maps --------------------------------------------------------------------------------------------------
def random_map(rng, scale, lattice):
    """a few chains and points: coordinates k * step for small k on a lattice (ties abound), else uniform at the scale"""
    half = 1 << scale
    if lattice:
        step = max(1, half // 8)
        coord = lambda: rng.randint(-7, 7) * step  # noqa: E731
    else:
        coord = lambda: rng.randint(-half, half - 1)  # noqa: E731
    chains = [[(coord(), coord()) for _ in range(rng.randint(2, 6))] for _ in range(rng.randint(1, 5))]
    points = [(coord(), coord()) for _ in range(12)]
    if lattice:  # (and the map's own vertices: distance 0, shared ends)
        points += [p for ch in chains for p in ch][:8]
    return NC.case(chains, points, [None] * len(points))


@pytest.mark.parametrize("scale", [10, 30, 46])
@pytest.mark.parametrize("lattice", [False, True], ids=["uniform", "lattice"])
def test_random_small_maps(twin, scale, lattice):
    rng = random.Random(1000 * scale + lattice)
    ties = 0
    for _ in range(60):
        c = random_map(rng, scale, lattice)
        edges = NR.edges_of(c.pts, c.row)
        want = check_case(twin, c, VARIANTS if _ % 6 == 0 else [(0, 1, 1), (1, 1, 1), (1, 0, 0)])
        # with max_dist at the distance of the first point's answer, rounded down: some qualify, some do not
        d2 = NR.d2_of(*want[0][1:])
        m = math.isqrt(d2.numerator // d2.denominator)
        check_case(twin, c._replace(max_dist=m), [(0, 1, 1), (1, 0, 1)])
        for (x, y), w in zip(c.points, want):
            best = NR.d2_of(*w[1:])
            ties += sum(NR.d2_of(*NR.point_edge(x, y, e)) == best for e in edges) > 1
    assert not lattice or ties > 200, ties  # (the lattices are there for the ties)


# ---- the wide arithmetic ------------------------------------------------------------------------------------------------
def limbs(v, n):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(n)], dtype=np.uint64)


def test_wide_multiply_and_compare_against_python_integers(twin):
    rng = random.Random(7)
    out = np.zeros(5, np.uint64)

    def value(a):
        return sum(int(v) << (64 * k) for k, v in enumerate(a))
    for bits_n, bits_d in [(190, 95), (192, 128), (64, 64), (1, 1)]:
        for _ in range(400):
            n1, n2 = rng.getrandbits(bits_n), rng.getrandbits(bits_n)
            d1, d2 = rng.getrandbits(bits_d) | 1, rng.getrandbits(bits_d) | 1
            kind = rng.randrange(4)
            if kind == 0:  # equal products: N1 D2 == N2 D1
                g, a, b = rng.getrandbits(bits_n // 2), rng.getrandbits(bits_d // 2) | 1, rng.getrandbits(bits_d // 2) | 1
                n1, d1, n2, d2 = g * a, a, g * b, b
            elif kind == 1:  # one apart
                n2, d2 = n1 + rng.choice((-1, 1)) if n1 else 1, d1
            a, b = n1 * d2, n2 * d1
            A, B, Cc, D = limbs(n1, 3), limbs(d2, 2), limbs(n2, 3), limbs(d1, 2)
            assert twin.nearest_wide_cmp(A.ctypes.data, B.ctypes.data, Cc.ctypes.data, D.ctypes.data) == (a > b) - (a < b)
            twin.nearest_wide_mul3(A.ctypes.data, B.ctypes.data, out.ctypes.data)
            assert value(out) == a
            x, y = rng.getrandbits(128), rng.getrandbits(128)
            X, Y = limbs(x, 2), limbs(y, 2)
            twin.nearest_wide_mul(X.ctypes.data, Y.ctypes.data, out.ctypes.data)
            assert value(out) == x * y
    top = (1 << 64) - 1  # every limb full: the carries
    twin.nearest_wide_mul3(limbs((1 << 192) - 1, 3).ctypes.data, limbs((1 << 128) - 1, 2).ctypes.data, out.ctypes.data)
    assert value(out) == ((1 << 192) - 1) * ((1 << 128) - 1) and top


# ---- the prune ----------------------------------------------------------------------------------------------------------
def test_box_lower_bound_is_strictly_below_and_tight_to_two_cells(twin):
    rng = random.Random(11)
    cell = 1 << 16
    positive = 0
    for k in range(3000):
        scale = rng.choice((18, 22, 30, 46))
        half = 1 << scale
        r = lambda: rng.randint(-half, half - 1)  # noqa: E731
        ax, ay, px, py = r(), r(), r(), r()
        kind = k % 3  # a point-like edge, an axis-parallel edge (its box is the edge: the bound must be tight), any edge
        if kind == 0:
            bx, by = ax, ay
        elif kind == 1:
            bx, by = (r(), ay) if rng.random() < 0.5 else (ax, r())
        else:
            bx, by = r(), r()
        s = np.array([ax, ay, bx, by], dtype=np.int64)
        lb2 = twin.nearest_box_lb2(s.ctypes.data, px, py)
        d2 = NR.d2_of(*NR.point_edge(px, py, (ax, ay, bx, by)))
        assert lb2 == 0 or (lb2 << 32) < d2  # strictly below the true distance
        assert (lb2 << 32) <= d2
        positive += lb2 > 0
        if kind != 2:  # d <= (sqrt(lb2) + 2 sqrt 2) cells, squared with the root rounded up
            root = math.isqrt(lb2) + 1
            assert d2 <= (root + 3) ** 2 * cell * cell, (lb2, d2)
        ub2 = twin.nearest_ub2(s.ctypes.data, px, py)  # the bound of the same edge as a held candidate: above, and close
        assert d2 <= (ub2 << 32) and (ub2 << 32) <= d2 * (1 + Fraction(1, 1 << 39)) + (2 << 32)
        assert (ub2 == 0) == (d2 == 0)
    assert positive > 1000
    for m in (0, 1, 65535, 65536, 65537, 1 << 40, (1 << 48) - 1, 1 << 48):
        u = twin.nearest_ub2_of_max_dist(m)
        assert u == min((m * m + (1 << 32) - 1) >> 32, (1 << 64) - 1)
    assert twin.nearest_ub2_of_max_dist(-1) == twin.nearest_ub2_of_max_dist(-(1 << 62)) == (1 << 64) - 1


def test_the_prune_only_saves_work(twin):
    """on a lattice with the points on its vertices the pruned brute force evaluates a handful of edges per point and gives
    what the full one gives"""
    from rayjoin_amd import maps, synth
    m = maps.Context([synth.lattice_map(12, 5, 3)]).load().maps[0]
    seg, pts = m.segments(), m.pts[:300]
    full, _, n_full = run_twin(twin, seg, pts, prune=0, want_evaluated=True)
    pruned, _, n_pruned = run_twin(twin, seg, pts, prune=1, want_evaluated=True)
    assert full == pruned and (n_full == len(seg)).all()
    assert n_pruned.mean() < len(seg) / 4, (n_pruned.mean(), len(seg))


# ---- mutations of the header, each caught by a hand case -----------------------------------------------------------------
MUTATIONS = [
    # (tag, the text, its replacement, the hand case that catches it)
    ("prune_gt", "return ub2 >= lb2;", "return ub2 > lb2;", "vertex_of_three_chains"),
    ("gap_g", "return g > 1 ? (uint32_t) (g - 1) : 0u;", "return g > 0 ? (uint32_t) g : 0u;", "cells_two_apart_decoy"),
    ("tie_larger", "(c == 0 && a.eid < b.eid)", "(c == 0 && a.eid > b.eid)", "interior_chain_vertex"),
]


@pytest.mark.parametrize("tag,old,new,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught(tag, old, new, name, tmp_path):
    text = open(os.path.join(CSRC, "rj_nearest.h")).read()
    assert text.count(old) == 1
    with open(tmp_path / "rj_nearest.h", "w") as f:
        f.write(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mut_" + tag)
    c = NC.HAND[name]
    seg = seg_array(NR.edges_of(c.pts, c.row))
    wrong = [v for v in VARIANTS if run_twin(L, seg, c.points, c.max_dist, *v)[0] != c.want]
    assert wrong, "the mutant %s survives the hand case %s" % (tag, name)


# ---- the stand-alone twin under the host sanitizers ----------------------------------------------------------------------
def case_text(c):
    edges = NR.edges_of(c.pts, c.row)
    words = [len(edges), len(c.points), c.max_dist] + [v for e in edges for v in e] + [v for p in c.points for v in p]
    for eid, where, num, den in c.want:
        words += [eid, where, num & 0xFFFFFFFFFFFFFFFF, num >> 64, den & 0xFFFFFFFFFFFFFFFF, den >> 64]
    return " ".join(str(int(v)) for v in words)


def test_standalone_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "nearest_twin_san")
    subprocess.check_call(CXX[:1] + ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-DNEAREST_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(case_text(NC.HAND[k]) for k in sorted(NC.HAND)) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 failures" % len(NC.HAND) in r.stdout and "runtime error" not in r.stderr
