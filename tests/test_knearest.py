"""The k nearest edges of a map for every point on the CPU: the host twin of the device's per-element functions
(tests/hosttwin/knearest_twin.cc compiling rayjoin_amd/csrc/rj_knearest.h) against the plain-Python definition
(tests/knearest_ref.py) with the edges offered ascending, descending and shuffled, with and without the double filter and
the prune, and with the list at the strides 1 and 64: the hand cases of tests/nearest_cases.py at k = 1, 2, 3 and 32; a map
of 5 edges at k = 8; a hub vertex of six chains at k = 5; the near-tie and the exact-tie fan of tests/distance_cases.py at
k = 17, the cut inside the tie; random small maps on lattices where ties abound; k = 1 equal to tests/nearest_ref.py
everywhere; three mutations of a scratch copy of the header, each caught; the twin as a stand-alone program under the host
sanitizers.  The GPU side is tests/test_gpu_knearest.py."""
import collections
import ctypes as C
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distance_cases as DC  # noqa: E402
import knearest_ref as KR  # noqa: E402
import nearest_cases as NC  # noqa: E402
import nearest_ref as NR  # noqa: E402
from test_nearest import CXX, NEAR_DTYPE, check_dist, random_map, seg_array, tuples_of  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "knearest_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
HEADERS = ("rj_knearest.h", "rj_nearest.h", "rj_predicates.h")
KS = (1, 2, 3, 32)
Answer = collections.namedtuple("Answer", "count eid rec dist entered")


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libknearest_twin%s.so" % tag)
    deps = [SRC] + [os.path.join(hdr_dir if os.path.exists(os.path.join(hdr_dir, h)) else CSRC, h) for h in HEADERS]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(CXX + ["-fPIC", "-shared", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.knearest_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 5
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def run_twin(L, seg, points, k, max_dist=-1, offer=None, filt=1, prune=1, stride=1):
    """-> Answer of arrays shaped as rj_knearest_query's: count [n], eid, rec, dist [n, k]; entered [n]"""
    seg = np.ascontiguousarray(seg, dtype=np.int64).reshape(-1, 4)
    pts = np.ascontiguousarray(points, dtype=np.int64).reshape(-1, 2)
    n = len(pts)
    if offer is not None:
        offer = np.ascontiguousarray(offer, np.uint32)
        assert sorted(offer.tolist()) == list(range(len(seg)))
    count, entered = np.full(n + 1, 0x5B5B5B5B, np.uint32), np.zeros(n + 1, np.uint64)
    eid, rec, dist = np.full(n * k + 1, 0x5B5B5B5B, np.uint32), np.zeros(n * k + 1, NEAR_DTYPE), np.full(n * k + 1, -7.0)
    rc = L.knearest_twin(seg.ctypes.data, len(seg), pts.ctypes.data, n, k, max_dist, None if offer is None else offer.ctypes.data, filt, prune, stride,
                         count.ctypes.data, eid.ctypes.data, rec.ctypes.data, dist.ctypes.data, entered.ctypes.data)
    assert rc == 0 and count[n] == 0x5B5B5B5B and eid[n * k] == 0x5B5B5B5B and dist[n * k] == -7.0
    return Answer(count[:n], eid[:n * k].reshape(n, k), rec[:n * k].reshape(n, k), dist[:n * k].reshape(n, k), entered[:n])


def rows_of(a):
    """Answer -> per point the (eid, where, num, den) tuples of its valid entries, with everything an Answer must satisfy
    beside them: the eid array equal to the records' eids, the entries behind the count the miss, no eid twice in a row"""
    n, k = a.eid.shape
    assert np.array_equal(a.eid, a.rec["eid"]) and (a.count <= k).all()
    behind = np.arange(k)[None, :] >= a.count[:, None]
    assert (a.eid[behind] == NR.MISS).all() and (a.eid[~behind] != NR.MISS).all()
    assert not a.rec[behind].view(np.uint32).reshape(-1, 10)[:, 1:].any()
    assert np.isinf(a.dist[behind]).all() and (a.dist[behind] > 0).all() and np.isfinite(a.dist[~behind]).all()
    rows = [tuples_of(a.rec[i, :a.count[i]]) for i in range(n)]
    assert all(len({t[0] for t in r}) == len(r) for r in rows)
    return rows


def offers(ne, rng):
    """the orders the edges are offered in: ascending, descending, shuffled"""
    return [None, np.arange(ne - 1, -1, -1), np.array(rng.sample(range(ne), ne))]


def check(L, seg, points, k, max_dist=-1, full=True, want=None):
    """the twin in every variant == the definition; -> the definition's rows"""
    edges = [tuple(int(v) for v in e) for e in np.asarray(seg).reshape(-1, 4)]
    want = KR.knearest_all(points, edges, k, max_dist) if want is None else want
    if k == 1:
        assert [r[0] if r else (NR.MISS, 0, 0, 0) for r in want] == NR.nearest_all(points, edges, max_dist)
    rng = random.Random(len(edges) * 31 + k)
    variants = [(o, f, p, s) for o in range(3) for f in (1, 0) for p in (1, 0) for s in (1, 64)]
    for o, filt, prune, stride in variants if full else [variants[0], variants[11], variants[20]]:
        a = run_twin(L, seg, points, k, max_dist, offers(len(edges), rng)[o], filt, prune, stride)
        assert rows_of(a) == want, (o, filt, prune, stride)
        assert a.count.tolist() == [len(r) for r in want] and (a.entered >= a.count).all()
        for i, r in enumerate(want[:50]):
            check_dist(r, a.dist[i, :len(r)])
    return want


def case_seg(c):
    return seg_array(NR.edges_of(c.pts, c.row))


# ---- the hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_hand_cases(twin, name, k):
    c = NC.HAND[name]
    want = check(twin, case_seg(c), c.points, k, c.max_dist)
    assert [r[0] if r else NC.MISS for r in want] == c.want  # (the first of every row is the written answer)
    ne = len(case_seg(c))
    assert all(len(r) <= min(k, ne) for r in want) and (c.max_dist >= 0 or all(len(r) == min(k, ne) for r in want))


def test_fewer_edges_than_k(twin):
    """a base map of 5 edges at k = 8: count 5, then misses"""
    c = NC.case([[(0, 0), (10, 0), (10, 10)], [(50, 50), (60, 50)], [(-7, 3), (-7, 9), (-20, 9)]], [(1, 1), (55, 49), (-7, 9), (1000, -1000)], [None] * 4)
    want = check(twin, case_seg(c), c.points, 8)
    assert [len(r) for r in want] == [5] * 4
    a = run_twin(twin, case_seg(c), c.points, 8)
    assert (a.count == 5).all() and (a.eid[:, 5:] == NR.MISS).all() and sorted(a.eid[0, :5].tolist()) == list(range(5))
    # ... and within 12 units: of (1, 1) the corner chain (1, 9) and the ends (-7, 3) and (-7, 9) (sqrt 68, sqrt 128); of
    # (55, 49) its own edge; of (-7, 9) its two edges and the end (0, 0) (sqrt 130); of the far point nothing
    assert [len(r) for r in check(twin, case_seg(c), c.points, 8, max_dist=12)] == [4, 1, 3, 0]


def hub_case():
    """a decoy edge, then six chains whose middle vertex is the hub (0, 0): the 12 edges 1 .. 12 at distance 0 from it"""
    spokes = [((-9, 0), (9, 0)), ((0, -9), (0, 9)), ((-9, -9), (9, 9)), ((-9, 9), (9, -9)), ((-9, 4), (9, -4)), ((4, -9), (-4, 9))]
    return NC.case([[(100, 100), (120, 100)]] + [[a, (0, 0), b] for a, b in spokes], [(0, 0), (1, 0)], [None] * 2)


def test_hub_vertex_of_six_chains(twin):
    c = hub_case()
    want = check(twin, case_seg(c), c.points, 5)
    assert [t[0] for t in want[0]] == [1, 2, 3, 4, 5] and all(NR.d2_of(*t[1:]) == 0 for t in want[0])
    assert [t[0] for t in check(twin, case_seg(c), c.points, 12)[0]] == list(range(1, 13))
    assert [t[0] for t in check(twin, case_seg(c), c.points, 13)[0]] == list(range(1, 13)) + [0]
    assert [len(r) for r in check(twin, case_seg(c), c.points, 32, max_dist=0)] == [12, 1]  # ((1, 0) lies on edge 2 alone)


# ---- the fans: the cut lies inside the tie -----------------------------------------------------------------------------------
def fan(kind, seed=0):
    rng = np.random.default_rng(60 + seed)
    return DC.tie_fan(rng) if kind == "tie" else DC.equal_fan(rng)


@pytest.mark.parametrize("kind", ["tie", "equal"])
def test_fans_at_k_17(twin, kind):
    f = fan(kind)
    seg = seg_array(f.edges)
    d2 = [NR.d2_of(*NR.point_edge(f.P[0], f.P[1], e)) for e in f.edges]
    assert DC.inseparable(d2) and len(f.edges) >= 64  # the doubles order nothing here
    want = check(twin, seg, [f.P], 17)[0]
    if kind == "equal":  # equal as rationals, different in every limb: the 17 smallest eids
        assert len(set(d2)) == 1 and len({(t[2], t[3]) for t in want}) > 8 and [t[0] for t in want] == list(range(17))
    else:  # all different, by less than a double can tell: the exact order, which is not the eids'
        assert len(set(d2)) == len(d2)
        assert [t[0] for t in want] == sorted(range(len(d2)), key=lambda e: d2[e])[:17] != sorted(t[0] for t in want)
    m = f.m or f.h + 1
    for md, n_want in ((m - 1, 0), (m, 17), (1 << 48, 17)):
        assert len(check(twin, seg, [f.P], 17, max_dist=md, full=False)[0]) == n_want
    check(twin, seg, [f.P, (f.P[0] + 1, f.P[1]), (f.P[0], f.P[1] - 3)], 32, full=False)


# ---- random small maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [10, 30, 46])
@pytest.mark.parametrize("lattice", [False, True], ids=["uniform", "lattice"])
def test_random_small_maps(twin, scale, lattice):
    rng = random.Random(2000 * scale + lattice)
    cut_in_tie = 0
    for it in range(40):
        c = random_map(rng, scale, lattice)
        seg = case_seg(c)
        k = rng.choice((1, 2, 3, 4, 5, 32))
        want = check(twin, seg, c.points, k, full=it % 8 == 0)
        # with max_dist at the distance of the first point's last entry, rounded down: the counts differ from point to point
        d2 = NR.d2_of(*want[0][-1][1:])
        limited = check(twin, seg, c.points, k, max_dist=math.isqrt(d2.numerator // d2.denominator), full=False)
        assert all(len(a) <= len(b) for a, b in zip(limited, want))
        for (x, y), r in zip(c.points, want):  # the last entry ties with an edge that stayed outside
            last = NR.d2_of(*r[-1][1:])
            held = {t[0] for t in r}
            cut_in_tie += any(e not in held and NR.d2_of(*NR.point_edge(x, y, edge)) == last for e, edge in enumerate(NR.edges_of(c.pts, c.row)))
    print("rows whose cut lies inside a tie: %d" % cut_in_tie)
    assert not lattice or cut_in_tie > 50, cut_in_tie  # (the lattices are there for the ties; 800 rows)


def test_refusals(twin):
    seg, pts = seg_array([(0, 0, 1, 1)]), np.zeros((1, 2), np.int64)
    out = np.zeros(64, np.uint32)
    call = lambda k, md: twin.knearest_twin(seg.ctypes.data, 1, pts.ctypes.data, 1, k, md, None, 1, 1, 1, None, out.ctypes.data, None, None, None)  # noqa: E731
    assert [call(0, -1), call(33, -1), call(1, (1 << 48) + 1)] == [1, 1, 1] and call(32, 1 << 48) == 0 and call(1, -1) == 0


# ---- mutations of the header -----------------------------------------------------------------------------------------------
MUTATIONS = [
    # the worst of a list taken for its first: the nearest held edge is the one that is replaced
    ("worst_is_first", "if (slot_before(L, ws, dw, s, ds, filter)) ws = s, dw = ds;", "if (slot_before(L, s, ds, ws, dw, filter)) ws = s, dw = ds;"),
    # the bound taken from some held candidate, not the worst: edges are dismissed that belong among the k
    ("bound_of_slot_0", "H.ub2 = ub2_of(slot_cand(L, ws), dw);", "H.ub2 = ub2_of(slot_cand(L, 0), slot_d2(L, 0));"),
    # the selection forgets to keep what it displaced
    ("order_drops_a_slot", "if (s != j) slot_put(L, s, slot_cand(L, j), slot_d2(L, j));", ""),
]


@pytest.mark.parametrize("tag,old,new", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught(tag, old, new, tmp_path):
    text = open(os.path.join(CSRC, "rj_knearest.h")).read()
    assert text.count(old) == 1
    with open(tmp_path / "rj_knearest.h", "w") as f:
        f.write(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mut_" + tag)
    c = random_map(random.Random(5), 30, False)
    c = c._replace(points=c.points + [(p[0] + 3, p[1] - 2) for p in c.pts])
    seg = case_seg(c)
    want = KR.knearest_all(c.points, NR.edges_of(c.pts, c.row), 3)
    rng = random.Random(1)
    wrong = 0
    for offer in offers(len(seg), rng):
        a = run_twin(L, seg, c.points, 3, offer=offer)
        wrong += [tuples_of(a.rec[i, :a.count[i]]) for i in range(len(c.points))] != want
    assert wrong, "the mutant %s survives" % tag


# ---- the stand-alone twin under the host sanitizers ----------------------------------------------------------------------
def case_text(seg, points, k, max_dist, want):
    words = [len(seg), len(points), k, max_dist] + [int(v) for v in np.asarray(seg).reshape(-1)] + [int(v) for p in points for v in p]
    for row in want:
        words.append(len(row))
        for eid, where, num, den in row:
            words += [eid, where, num & 0xFFFFFFFFFFFFFFFF, num >> 64, den & 0xFFFFFFFFFFFFFFFF, den >> 64]
    return " ".join(str(int(v)) for v in words)


def test_standalone_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "knearest_twin_san")
    subprocess.check_call(CXX[:1] + ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-DKNEAREST_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    cases = []
    for name in sorted(NC.HAND):
        c = NC.HAND[name]
        for k in (2, 32):
            cases.append((case_seg(c), c.points, k, c.max_dist))
    h = hub_case()
    cases.append((case_seg(h), h.points, 5, -1))
    for kind in ("tie", "equal"):
        f = fan(kind)
        cases.append((seg_array(f.edges), [f.P], 17, -1))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(case_text(s, p, k, md, KR.knearest_all(p, [tuple(int(v) for v in e) for e in s], k, md)) for s, p, k, md in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 failures" % len(cases) in r.stdout and "runtime error" not in r.stderr
