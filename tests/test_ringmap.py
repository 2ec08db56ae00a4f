"""Rings to map on the CPU: the plain-Python definition (tests/ringmap_ref.py) on the hand-built ring sets of
tests/ringmap_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/ringmap_twin.cc compiling rayjoin_amd/csrc/rj_ringmap.h) against that definition, every array and every
count, on all cases, on the rings of every map of tests/rings_cases.py and of 60 random planar maps; the round trip
map -> rings -> map -> rings, which gives the same rings and, a second time, the same map; dissolve on maps whose faces are
renamed to two groups; maps.rings_of_polygons; the contract of the call.  The GPU side is tests/test_gpu_ringmap.py.

Mutations of a scratch copy of rj_ringmap.h, and the tests here that fail under each (154 tests at the time; the test of the numpy canonical form came later):
  the keep rule reversed (a > W[a ^ 1].at): 121 -- the twin against the definition on 23 hand cases (all but the ones
      without a chain), on all 15 ring-case maps, on all 60 planar maps, the 20 dissolve cases, both long loops, the overflow test
  the smallest slot replaced by the largest (every slot of a kind writes its face): 2 -- the hand cases "twice" and "label-change"
  the label check at degree 2 dropped: 1 -- the hand case "label-change" (one chain for two; no consistent planar map has
      such a vertex, so no generated map can catch it)
  the closed leader the largest half-edge instead of the smallest: 60 -- 16 hand cases (every loop, "hole", "corners", ...),
      11 ring-case maps, 13 planar maps, 18 dissolve cases, both long loops"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ringmap_cases as MC  # noqa: E402
import ringmap_ref as MR  # noqa: E402
import rings_cases as K  # noqa: E402
import rings_planar as P  # noqa: E402
import rings_ref as D  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "ringmap_twin.cc")
HDRS = [os.path.join(ROOT, "rayjoin_amd", "csrc", name) for name in ("rj_ringmap.h", "rj_rings.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "libringmap_twin.so")
PLANAR_SEEDS = tuple(range(60))
CANARY = -7


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.ringmap_twin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64] + \
        [C.c_void_p] * 6
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_map(L, rings, dissolve=False, caps=None, stride=4, flags=None):
    """-> (status, dict of the arrays cut to min(count, capacity) and the counts, (rounds of the two passes)).  caps None:
    room for everything these rings can give.  Behind every capacity lie canaries that must survive."""
    row, xy, face = rings
    row, xy = np.ascontiguousarray(row, np.uint32), np.ascontiguousarray(xy, np.int64).reshape(-1, 2)
    face = np.ascontiguousarray(face)
    n = len(xy)
    cc, pc = caps if caps is not None else (n, 2 * n)
    oxy, orow = np.full((pc + 3, 2), CANARY, np.int64), np.full(cc + 1 + 3, 0xFFFFFFFF, np.uint32)
    left, right = np.full(cc + 3, CANARY, np.int32), np.full(cc + 3, CANARY, np.int32)
    counts, stats = np.zeros(7, np.uint64), np.zeros(2, np.uint64)
    rc = L.ringmap_twin(row.ctypes.data, xy.ctypes.data, n, face.ctypes.data, stride, len(row) - 1, (1 if dissolve else 0) if flags is None else flags,
                        cc, pc, oxy.ctypes.data, orow.ctypes.data, left.ctypes.data, right.ctypes.data, counts.ctypes.data, stats.ctypes.data)
    c = dict(zip(MR.COUNTS, (int(v) for v in counts)))
    k = min(c["n_chains"], cc)
    kp = min(c["n_points"], pc)
    assert (oxy[pc:] == CANARY).all() and (orow[cc + 1:] == 0xFFFFFFFF).all() and (left[cc:] == CANARY).all() and (right[cc:] == CANARY).all()
    if c["n_chains"] > cc:
        assert orow[cc] == 0xFFFFFFFF  # (the closing entry belongs to a row that fits)
    got = dict(xy=oxy[:kp], row_index=orow[:k + 1] if c["n_chains"] <= cc else orow[:k], left=left[:k], right=right[:k], counts=c)
    return rc, got, tuple(int(v) for v in stats)


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """-> (rings, dissolve, the written answer, the definition's answer): computed once, shared, left unchanged"""
    rings, dissolve, want = MC.HAND[name]()
    return rings, dissolve, want, MR.rings_map_ref(*rings, dissolve=dissolve)


@functools.lru_cache(maxsize=None)
def long_cases():
    return MC.long_loops()


def rings_of_map(m):
    """a chain map -> (its rings by the definition of tests/rings_ref.py as the three arrays of a ring set, the rings dict)"""
    rg = D.rings_ref(*m)
    return (rg["ring_row"], rg["ring_xy"], rg["rings"]["face"].astype(np.int32)), rg


def canon_of(rg):
    return MR.canonical_rings(rg["rings"]["face"].tolist(), rg["ring_row"], rg["ring_xy"], D.area2_of(rg["rings"]))


def canon_np_of(rg):
    """canon_of in numpy, for ring sets too large for the Python loop; the point sequences as bytes"""
    return MR.canonical_rings_np(rg["rings"]["face"].tolist(), rg["ring_row"], rg["ring_xy"], D.area2_of(rg["rings"]))


@functools.lru_cache(maxsize=None)
def planar_case(seed):
    """-> (the map, its rings as a ring set, the rings dict, the definition's map of these rings)"""
    m, _ = P.draw_planar(seed)
    rings, rg = rings_of_map(m)
    return m, rings, rg, MR.rings_map_ref(*rings)


@functools.lru_cache(maxsize=None)
def ring_case_maps():
    return K.all_cases()


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.HAND))
def test_definition_gives_the_written_answers(name):
    _, _, want, ref = hand_case(name)
    MR.assert_same_map(ref, want, name)
    assert ref["counts"]["n_points"] == ref["counts"]["n_edges"] + ref["counts"]["n_chains"]


def test_the_hand_cases_say_what_they_claim():
    assert hand_case("rect")[3]["counts"]["n_chains"] == 3 and len(K.rect_output_map()[2]) == 5
    assert hand_case("squares-equal")[3]["counts"]["n_chains"] == 3 and hand_case("squares-equal-dissolve")[3]["counts"]["n_chains"] == 1
    assert hand_case("label-change")[3]["counts"] == dict(n_chains=2, n_points=7, n_edges=5, n_closed=0, n_zero_edges=0, n_conflicts=1, n_dissolved=0)
    assert hand_case("touching")[3]["counts"]["n_closed"] == 0 and hand_case("twice")[3]["counts"]["n_conflicts"] == 3
    odd = hand_case("odd-faces")[3]
    assert set(odd["left"].tolist()) | set(odd["right"].tolist()) == set(P.ODD_FACES)
    xy = hand_case("corners")[0][1]
    assert int(xy.min()) == -(1 << 46) and int(xy.max()) == (1 << 46) - 1
    for n in MC.LOOP_SIZES:  # the rotated start is not where the chain starts, and the two orientations swap the faces
        a, b = hand_case("loop-%d-ccw" % n), hand_case("loop-%d-cw" % n)
        assert a[3]["counts"] == dict(n_chains=1, n_points=n + 1, n_edges=n, n_closed=1, n_zero_edges=0, n_conflicts=0, n_dissolved=0)
        assert tuple(a[3]["xy"][0]) != tuple(a[0][1][0]) and np.array_equal(a[3]["xy"], b[3]["xy"])
        assert (a[3]["left"][0], a[3]["right"][0]) == (b[3]["right"][0], b[3]["left"][0]) and {int(a[3]["left"][0]), int(a[3]["right"][0])} == {0, 4}


# ---- the twin against the definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.HAND))
def test_twin_equals_the_definition_on_the_hand_cases(twin, name):
    rings, dissolve, _, ref = hand_case(name)
    rc, got, _ = twin_map(twin, rings, dissolve)
    assert rc == 0
    MR.assert_same_map(got, ref, name)


@pytest.mark.parametrize("name", ["ccw", "cw"])
def test_twin_on_the_long_loops_has_the_answer_of_the_construction(twin, name):
    rings, dissolve, want = long_cases()["loop-%d-%s" % (MC.LONG_LOOP, name)]
    rc, got, rounds = twin_map(twin, rings, dissolve)
    assert rc == 0
    MR.assert_same_map(got, want, name)
    assert rounds[0] >= 17 and rounds[1] >= 17  # (2^17 > 100 003: the minimum and the ranking took their doubling steps)


@pytest.mark.parametrize("name", sorted(K.HAND) + ["necklace-%d" % n for n in K.NECKLACE_SIZES])
def test_twin_equals_the_definition_on_the_rings_of_the_ring_cases(twin, name):
    m = ring_case_maps()[name]
    rings, rg = rings_of_map(m)
    ref = MR.rings_map_ref(*rings)
    rc, got, _ = twin_map(twin, rings)
    assert rc == 0
    MR.assert_same_map(got, ref, name)
    assert ref["counts"]["n_conflicts"] == 0 and ref["counts"]["n_chains"] <= len(m[2]), name
    check_round_trips(twin, rg, ref, name)
    # reading the faces of the ring records in place gives the same
    rc, got, _ = twin_map(twin, (rings[0], rings[1], rg["rings"]), stride=D.RING_DTYPE.itemsize)
    assert rc == 0
    MR.assert_same_map(got, ref, name)


def check_round_trips(twin, rg, ref, what):
    """the three properties: no conflicts; the rings of the map of the rings are the rings (canonically: cyclic point sequences
    without repeated points, with faces and areas); a second round trip reproduces the map array for array"""
    assert ref["counts"]["n_conflicts"] == 0, what
    rg2 = D.rings_ref(*MR.as_map(ref))
    assert canon_of(rg2) == canon_of(rg), what
    assert rg2["counts"]["n_mixed"] == rg["counts"]["n_mixed"] and rg2["counts"]["n_skipped"] == 0, what
    rings2 = (rg2["ring_row"], rg2["ring_xy"], rg2["rings"]["face"].astype(np.int32))
    rc, again, _ = twin_map(twin, rings2)
    assert rc == 0
    ref2 = dict(ref, counts=dict(ref["counts"], n_zero_edges=0))  # (the zero-length edges of the source are gone after one trip)
    MR.assert_same_map(again, ref2, what)


@pytest.mark.parametrize("seed", PLANAR_SEEDS)
def test_twin_equals_the_definition_on_random_planar_maps_and_the_round_trips_hold(twin, seed):
    m, rings, rg, ref = planar_case(seed)
    rc, got, _ = twin_map(twin, rings)
    assert rc == 0
    MR.assert_same_map(got, ref, seed)
    assert ref["counts"]["n_chains"] <= len(m[2]), seed
    check_round_trips(twin, rg, ref, seed)


def test_numpy_canonical_form_equals_the_python_one():
    """on the rings of every ring-case map (zero-length edges, a star and a touching vertex that pass their smallest point
    more than once) and of ten planar maps"""
    cases = [rings_of_map(m)[1] for m in ring_case_maps().values()] + [planar_case(seed)[2] for seed in PLANAR_SEEDS[:10]]
    repeated = 0
    for rg in cases:
        slow = sorted((f, a2, np.array(pts, np.int64).reshape(-1, 2).tobytes()) for f, a2, pts in canon_of(rg))
        assert canon_np_of(rg) == slow
        repeated += sum(1 for _, _, pts in canon_of(rg) if len(pts) > 1 and pts.count(min(pts)) > 1)
    assert repeated >= 3


def test_planar_seeds_have_closed_chains_junctions_and_both_kinds_of_range():
    """what the seeds must contain, so that the tests on them cannot run empty"""
    closed = fewer = full = 0
    for seed in PLANAR_SEEDS:
        m, _, _, ref = planar_case(seed)
        closed += ref["counts"]["n_closed"]
        fewer += ref["counts"]["n_chains"] < len(m[2])
        full += int(np.abs(m[0]).max()) > (1 << 45)
    assert closed >= 10 and fewer >= 10 and 10 <= full <= 50, (closed, fewer, full)


@pytest.mark.parametrize("seed", PLANAR_SEEDS[:20])
def test_dissolve_on_two_groups_leaves_no_inner_chain_and_keeps_the_area_sums(twin, seed):
    """the faces renamed to two groups (0 stays 0): with dissolve no chain has the same group on both sides, and the rings
    of the dissolved map have the groups' area sums"""
    m = P.draw_planar(seed)[0]
    group = lambda f: np.where(f == 0, 0, 1 + (f % 2)).astype(np.int32)  # noqa: E731
    renamed = (m[0], m[1], group(m[2]), group(m[3]))
    rings, rg = rings_of_map(renamed)
    ref = MR.rings_map_ref(*rings, dissolve=True)
    rc, got, _ = twin_map(twin, rings, dissolve=True)
    assert rc == 0
    MR.assert_same_map(got, ref, seed)
    assert (got["left"] != got["right"]).all() and got["counts"]["n_conflicts"] == 0, seed
    plain = MR.rings_map_ref(*rings)
    assert got["counts"]["n_dissolved"] == plain["counts"]["n_edges"] - got["counts"]["n_edges"], seed
    sums = {f: a for f, a in P.face_sums(D.rings_ref(*MR.as_map(got))).items() if a != 0}
    assert sums == {f: a for f, a in P.face_sums(rg).items() if a != 0}, seed


# ---- maps.rings_of_polygons -------------------------------------------------------------------------------------------------
def test_rings_of_polygons_turns_shells_counter_clockwise_and_holes_clockwise():
    shell_cw, hole_ccw = [(0, 0), (0, 10), (10, 10), (10, 0)], [(3, 3), (6, 3), (6, 6), (3, 6)]
    row, xy, face = maps.rings_of_polygons([(1, shell_cw, [hole_ccw]), (2, np.array(hole_ccw), [])])
    assert row.dtype == np.uint32 and xy.dtype == np.int64 and face.dtype == np.int32
    assert row.tolist() == [0, 4, 8, 12] and face.tolist() == [1, 1, 2]
    assert xy.tolist() == [list(p) for p in shell_cw[::-1] + hole_ccw[::-1] + hole_ccw]
    # the same polygons, already oriented, stay as they are -- and give the map of the square with a hole
    rings, _, want, _ = hand_case("hole")
    again = maps.rings_of_polygons([(1, rings[1][0:4], [rings[1][4:8]]), (2, rings[1][8:12], [])])
    assert all(np.array_equal(a, b) for a, b in zip(again, rings))
    MR.assert_same_map(MR.rings_map_ref(*again), want)
    # orientation at the ends of the range: the shoelace sum needs more than 64 bits
    T = (1 << 46) - 1
    big = [(T, T), (T, -T - 1), (-T - 1, -T - 1), (-T - 1, T)]  # clockwise
    assert maps.rings_of_polygons([(5, big, [])])[1].tolist() == [list(p) for p in big[::-1]]
    assert maps.rings_of_polygons([])[0].tolist() == [0]


def test_rings_of_polygons_raises_for_area_zero():
    with pytest.raises(ValueError, match="shell"):
        maps.rings_of_polygons([(1, [(0, 0), (5, 5), (9, 9)], [])])
    with pytest.raises(ValueError, match="hole 0"):
        maps.rings_of_polygons([(1, [(0, 0), (9, 0), (0, 9)], [[(1, 1), (2, 2)]])])


# ---- the contract of the call ----------------------------------------------------------------------------------------------
def test_each_capacity_one_short_overflows_with_the_true_counts(twin):
    rings, dissolve, want, _ = hand_case("squares-different")
    true = (want["counts"]["n_chains"], want["counts"]["n_points"])
    rc, got, _ = twin_map(twin, rings, caps=(0, 0))  # the sizing call
    assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == want["counts"]
    for short in range(2):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, got, _ = twin_map(twin, rings, caps=caps)
        assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == want["counts"], short
        assert np.array_equal(got["xy"], want["xy"][:caps[1]]) and np.array_equal(got["left"], want["left"][:caps[0]])
        assert np.array_equal(got["right"], want["right"][:caps[0]]) and np.array_equal(got["row_index"], want["row_index"][:len(got["row_index"])])
    rc, got, _ = twin_map(twin, rings, caps=true)
    assert rc == 0
    MR.assert_same_map(got, want)


def bad_inputs():
    """(what, (ring_row, ring_xy, ring_face), stride, flags): each RJ_E_INVALID, each rejected before anything is read through it"""
    row, xy, face = hand_case("hole")[0]
    late, short, down = row.copy(), row.copy(), row.copy()
    late[0], short[-1], down[1] = 1, row[-1] - 1, 9
    far = xy.copy()
    far[far == 10] = 1 << 46
    low = xy.copy()
    low[low == 0] = -(1 << 46) - 1
    return [("ring_row does not start at 0", (late, xy, face), 4, 0), ("ring_row does not end at n_points", (short, xy, face), 4, 0),
            ("ring_row decreases", (down, xy, face), 4, 0), ("a coordinate of 2^46", (row, far, face), 4, 0),
            ("a coordinate below -2^46", (row, low, face), 4, 0), ("stride 0", (row, xy, face), 0, 0), ("stride 2", (row, xy, face), 2, 0),
            ("stride 6", (row, xy, face), 6, 0), ("flag 2", (row, xy, face), 4, 2), ("flag 2^31", (row, xy, face), 4, 1 << 31)]


def test_bad_input_is_invalid(twin):
    for what, rings, stride, flags in bad_inputs():
        rc, got, _ = twin_map(twin, rings, stride=stride, flags=flags)
        assert rc == _capi.RJ_E_INVALID and got["counts"] == dict.fromkeys(MR.COUNTS, 0), what
        assert (got["xy"] == CANARY).all(), what
    rc, got, _ = twin_map(twin, (np.zeros(1, np.uint32), np.zeros((0, 2), np.int64), np.zeros(0, np.int32)))  # n_rings == 0
    assert rc == 0 and got["counts"] == dict.fromkeys(MR.COUNTS, 0) and got["row_index"].tolist() == [0]


def test_symbol_counts_and_flags():
    assert "rj_rings_map" in _capi.SYMBOLS and hasattr(_capi.load(), "rj_rings_map")
    assert _capi.RINGS_MAP_COUNTS == MR.COUNTS and _capi.RJ_RMAP_DISSOLVE == 1
    assert issubclass(_capi.RingsMapOverflow, _capi.RayJoinError)
