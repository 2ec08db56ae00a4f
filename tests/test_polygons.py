"""Polygons of face rings on the CPU: the plain-Python definition (tests/polygons_ref.py) on the hand-built maps of
tests/polygons_cases.py with the answers written out; on laminar families of nested rectangles whose parents are known from
the construction; the host twin of the device's per-element functions (tests/hosttwin/polygons_twin.cc compiling
rayjoin_amd/csrc/rj_polygons.h) against that definition, every array and every count, on all cases and on the helper
output maps of the overlay tests' pairs for every operation; on the raw ring sets of tests/polygons_soups.py -- ray orders
that only exact arithmetic at 2^46 decides, tops at every lane position, rings of 100 003 points, records without points,
faces outside 31 bits, areas whose prefix needs all 128 bits -- twin = definition = the construction's answer, with the
conditions that keep each of them from running empty.  The GPU side is tests/test_gpu_polygons.py."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from rayjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import polygons_cases as PC  # noqa: E402
import polygons_ref as PR  # noqa: E402
import polygons_soups as PS  # noqa: E402
import rings_cases as K  # noqa: E402
import rings_ref as D  # noqa: E402
from test_overlay_ops import OPS  # noqa: E402
from test_rings import as_map, helper_maps  # noqa: E402
from test_rings import twin_lib as rings_twin_lib  # noqa: E402
from test_rings import twin_rings  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "polygons_twin.cc")
HDRS = [os.path.join(ROOT, "rayjoin_amd", "csrc", name) for name in ("rj_polygons.h", "rj_rings.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "libpolygons_twin.so")
NONE = PR.NONE
STATS = ("shift", "n_entries", "n_edges", "rounds", "longest_bucket")


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.polygons_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_polygons(L, rings, ring_row, ring_xy, flags=0, caps=None, parent=True):
    """-> (status, dict of the arrays cut to min(count, capacity) and the counts, dict of STATS).  caps None: room for
    everything these rings can give"""
    rings = np.ascontiguousarray(rings, D.RING_DTYPE)
    row = np.ascontiguousarray(ring_row, np.uint32)
    xy = np.ascontiguousarray(ring_xy, np.int64).reshape(-1, 2)
    n = len(rings)
    pc, mc = caps if caps is not None else (n, n)
    par = np.full(n, 0xABABABAB, np.uint32)
    polys = np.zeros(pc, PR.POLYGON_DTYPE)
    polys["face"] = -7
    first, ring = np.full(pc + 1, 0xFFFFFFFF, np.uint32), np.full(mc, 0xFFFFFFFF, np.uint32)
    counts, stats = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    rc = L.polygons_twin(rings.ctypes.data, n, row.ctypes.data, xy.ctypes.data, len(xy), flags, pc, mc, par.ctypes.data if parent else None,
                         polys.ctypes.data, first.ctypes.data, ring.ctypes.data, counts.ctypes.data, stats.ctypes.data)
    c = dict(zip(PR.COUNTS, (int(v) for v in counts)))
    k = min(c["n_polygons"], pc)
    got = dict(parent=par, polygons=polys[:k], poly_first=first[:k + 1], poly_ring=ring[:min(c["n_members"], mc)], counts=c)
    return rc, got, dict(zip(STATS, (int(v) for v in stats)))


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """-> (rings of the map, the definition's polygons): computed once, shared, left unchanged"""
    rg = D.rings_ref(*PC.HAND[name]())
    return rg, PR.polygons_ref(rg["rings"], rg["ring_row"], rg["ring_xy"])


@functools.lru_cache(maxsize=None)
def span_case():
    rg = D.rings_ref(*PC.domain_span())
    return rg, PR.polygons_ref(rg["rings"], rg["ring_row"], rg["ring_xy"])


@functools.lru_cache(maxsize=None)
def laminar_case(seed):
    """-> (rings, the definition's polygons, the construction's parents); the linear map goes round with the seed"""
    name = sorted(PC.LINEAR_MAPS)[seed % len(PC.LINEAR_MAPS)]
    m, info = PC.laminar(seed, PC.LINEAR_MAPS[name])
    rg = D.rings_ref(*m)
    return rg, PR.polygons_ref(rg["rings"], rg["ring_row"], rg["ring_xy"]), PC.laminar_parents(info, rg["rings"], rg["ring_row"], rg["ring_xy"],
                                                                                              D.area2_of(rg["rings"]))


def args_of(rg):
    return rg["rings"], rg["ring_row"], rg["ring_xy"]


def summary(p):
    """[(face, shell, [holes], area2)] of a polygons dict"""
    first = p["poly_first"].tolist()
    return [(int(g["face"]), int(g["shell"]), p["poly_ring"][first[k] + 1:first[k + 1]].tolist(), a2)
            for k, (g, a2) in enumerate(zip(p["polygons"], PR.area2_of(p["polygons"])))]


# ---- the definition against the written answers -----------------------------------------------------------------------
def test_square_with_hole_dangling_and_star():
    """rings of the square with a hole: 0 the outside, 1 face 1's outer ring (200), 2 its hole (-18), 3 face 2's ring (18)"""
    _, p = hand_case("hole")
    assert summary(p) == [(1, 1, [2], 182), (2, 3, [], 18)] and p["parent"].tolist() == [NONE, 1, 1, 3]
    assert p["poly_first"].tolist() == [0, 2, 3] and p["poly_ring"].tolist() == [1, 2, 3]
    assert p["counts"] == dict(n_polygons=2, n_members=3, n_holes=1, n_orphans=0, n_face0=1)
    # the dangling chain lies in the outside: the zero-area walk along it is part of face 0's ring
    _, p = hand_case("dangling")
    assert summary(p) == [(1, 1, [], 32)] and p["counts"] == dict(n_polygons=1, n_members=1, n_holes=0, n_orphans=0, n_face0=1)
    rg, p = hand_case("star")
    assert D.area2_of(rg["rings"]) == [0] and p["counts"] == dict(n_polygons=0, n_members=0, n_holes=0, n_orphans=0, n_face0=1)
    assert p["poly_first"].tolist() == [0] and p["parent"].tolist() == [NONE]


def test_multi_part_face_has_three_polygons_each_hole_in_the_smallest_shell_round_it():
    """rings by (face, leader): 0, 1 the outside of the two squares; face 1: 2 square A [0, 20]^2, 3 its hole [5, 15]^2, 4
    square B, 5 its hole, 6 the island [7, 13]^2 inside A's hole, 7 the island's hole [9, 11]^2; face 2: 8 the ring inside A's
    hole, 9 its hole round the island; 10 face 3; 11 face 4.  Ring 7 lies inside A as well: the island is the smaller shell."""
    rg, p = hand_case("multi-part")
    assert rg["rings"]["face"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4]
    assert p["parent"].tolist() == [NONE, NONE, 2, 2, 4, 4, 6, 6, 8, 8, 10, 11]
    assert summary(p) == [(1, 2, [3], 800 - 200), (1, 4, [5], 800 - 200), (1, 6, [7], 72 - 8), (2, 8, [9], 200 - 72), (3, 10, [], 200), (4, 11, [], 8)]
    assert p["counts"] == dict(n_polygons=6, n_members=10, n_holes=4, n_orphans=0, n_face0=2)


@pytest.mark.parametrize("k", PC.COLUMN_SIZES)
def test_hole_column_is_one_polygon_of_k_holes(twin, k):
    """ring 1 is the shell, rings 2 .. k + 1 its holes; above(hole j) = hole j + 1: the walk of hole 0 has k steps"""
    rg, p = hand_case("column-%d" % k)
    assert p["parent"].tolist() == [NONE] + [1] * (k + 1) + list(range(k + 2, 2 * k + 2))
    assert summary(p)[0] == (1, 1, list(range(2, k + 2)), 2 * (k + 30) * (10 * k + 30) - 32 * k)
    kinds, above = PR.above_of(*args_of(rg))
    assert above[2:k + 2] == list(range(3, k + 2)) + [1]
    rc, got, stats = twin_polygons(twin, *args_of(rg))
    assert rc == 0
    PR.assert_same_polygons(got, p, k)
    assert stats["rounds"] >= (k - 1).bit_length() and (k != 1000 or stats["rounds"] >= 10)


def test_ray_degeneracies_have_the_written_parents():
    """every hole lies in the one shell (ring 1); what the ray meets first, by the definition"""
    for name, holes, first_above in (("below-hole-vertex", 2, [3, 1]), ("equal-heights", 2, [3, 1]), ("neither-covers", 2, [1, 1]),
                                     ("below-vertical-edges", 4, None), ("repeated-top", 2, [3, 1])):
        rg, p = hand_case(name)
        assert p["parent"].tolist()[:holes + 2] == [NONE] + [1] * (holes + 1), name
        assert p["counts"]["n_orphans"] == 0 and summary(p)[0][:3] == (1, 1, list(range(2, holes + 2))), name
        if first_above is not None:
            assert PR.above_of(*args_of(rg))[1][2:4] == first_above, name
    # the two touching triangles are one ring of face 1; the flatter of the two edges that start at (4, 10) wins
    rg, _ = hand_case("equal-heights")
    row = rg["ring_row"].tolist()
    assert row[4] - row[3] == 6
    # the hole under the left edge meets the hole above it, the hole under the right edge meets the shell
    rg, _ = hand_case("below-vertical-edges")
    above = PR.above_of(*args_of(rg))[1]
    tops = {r: max((int(y), int(x)) for x, y in rg["ring_xy"][rg["ring_row"][r]:rg["ring_row"][r + 1]]) for r in range(2, 6)}
    low_right, low_left = (r for r in sorted(tops, key=lambda r: -tops[r][1]) if tops[r][0] == 4)
    assert tops[low_right] == (4, 4) and tops[above[low_right]] == (14, 8) and tops[low_left] == (4, -6) and above[low_left] == 1


def test_touching_shells_and_touching_holes():
    _, p = hand_case("touching-shells")
    assert p["parent"].tolist() == [NONE, 1, 2, 1, 2, 5, 6]
    assert summary(p) == [(1, 1, [3], 3200 - 800), (1, 2, [4], 3200 - 800), (2, 5, [], 800), (3, 6, [], 800)]
    rg, p = hand_case("touching-holes")
    assert D.area2_of(rg["rings"])[2] == -400 and summary(p) == [(1, 1, [2], 80000 - 400), (2, 3, [], 200), (2, 4, [], 200)]


def test_an_orphan_has_no_parent_and_no_polygon():
    _, p = hand_case("orphan")
    assert p["counts"] == dict(n_polygons=0, n_members=0, n_holes=0, n_orphans=1, n_face0=1)
    assert p["parent"].tolist() == [NONE, NONE] and p["poly_first"].tolist() == [0]


# ---- the twin against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in PC.HAND if not n.startswith("column-")))
def test_twin_equals_the_definition_on_the_hand_cases(twin, name):
    rg, p = hand_case(name)
    rc, got, _ = twin_polygons(twin, *args_of(rg))
    assert rc == 0
    PR.assert_same_polygons(got, p, name)
    rc, got, _ = twin_polygons(twin, *args_of(rg), parent=False)  # parent is optional
    assert rc == 0 and got["counts"] == p["counts"] and (got["parent"] == 0xABABABAB).all()


def test_domain_wide_edge_forces_the_shift_up(twin):
    """coordinates at -2^46 and 2^46 - 1: the shell's top edge lies in 2^31 strips of 2^16 units.  E = 2 n + 1 ceiling
    edges (the shell's, every hole's bottom, the top of every ring inside a hole); the smallest s with 2^(47 - s) + 2 n
    at most 2 E"""
    rg, p = span_case()
    n = PC.SPAN_HOLES
    assert int(rg["ring_xy"].min()) == -(1 << 46) and int(rg["ring_xy"].max()) == (1 << 46) - 1
    assert p["parent"].tolist() == [NONE] + [1] * (n + 1) + list(range(n + 2, 2 * n + 2)) and p["counts"]["n_orphans"] == 0
    rc, got, stats = twin_polygons(twin, *args_of(rg))
    assert rc == 0
    PR.assert_same_polygons(got, p)
    assert stats["n_edges"] == 2 * n + 1 and stats["shift"] == PC.SPAN_SHIFT == 36 and stats["n_entries"] == 2 * n + (1 << 11)
    assert stats["longest_bucket"] >= n  # every hole's bottom edge and the shell's top share one strip
    # without the long edge the narrowest strips do
    rc, _, stats = twin_polygons(twin, *args_of(hand_case("column-64")[0]))
    assert rc == 0 and stats["shift"] == 16


LAMINAR_GPU_SEEDS = tuple(range(8))
LAMINAR_SEEDS = tuple(range(40))


@pytest.mark.parametrize("seed", LAMINAR_SEEDS)
def test_laminar_families_have_the_parents_of_the_construction(twin, seed):
    rg, p, want = laminar_case(seed)
    assert p["counts"]["n_orphans"] == 0 and np.array_equal(p["parent"], want), seed
    assert p["counts"]["n_polygons"] == len(rg["rings"]) // 2 and p["counts"]["n_holes"] + p["counts"]["n_face0"] == p["counts"]["n_polygons"]
    rc, got, _ = twin_polygons(twin, *args_of(rg))
    assert rc == 0
    PR.assert_same_polygons(got, p, seed)


def test_laminar_seeds_are_deep_multi_part_and_a_few_hundred_rings():
    """what the seeds of the GPU test must contain, so that test cannot run empty"""
    rings = deepest = multi = 0
    for seed in LAMINAR_GPU_SEEDS:
        rg, p, _ = laminar_case(seed)
        rings += len(rg["rings"])
        faces = p["polygons"]["face"].tolist()
        multi += sum(1 for f in (1, 2, 3) if faces.count(f) > 1)
        kinds, above = PR.above_of(*args_of(rg))
        for r in range(len(above)):
            d, at = 0, r
            while above[at] is not None and kinds[at] == "hole":
                at, d = above[at], d + 1
            deepest = max(deepest, d)
    assert rings > 800 and multi == 3 * len(LAMINAR_GPU_SEEDS) and deepest >= 2, (rings, multi, deepest)


@pytest.mark.parametrize("name", ["sample", "rings", "nested"])
def test_twin_equals_the_definition_on_the_helper_output_maps(oracle, twin, name):
    seen = holes = 0
    for what, om in helper_maps(oracle, name):
        rg = D.rings_ref(*as_map(om), skip_face0=what[3])  # (with and without the rings of face 0)
        want = PR.polygons_ref(*args_of(rg))
        rc, got, _ = twin_polygons(twin, *args_of(rg))
        assert rc == 0, what
        PR.assert_same_polygons(got, want, what)
        if name != "nested":
            assert want["counts"]["n_orphans"] == 0, what
        seen += 1
        holes += want["counts"]["n_holes"]
    assert seen == 4 * len(OPS) and (holes > 0 or name != "rings")  # (the rings pair: 47 holes under (union, pair))


# ---- raw ring sets: tests/polygons_soups.py ------------------------------------------------------------------------------
SLIVER_SEEDS = tuple(range(8))
FAN_SEEDS = tuple(range(6))
CARRY_SQUARES = 20_000
BIG_FIELD_SIDE = 520
SOUPS = {"sliver": PS.sliver_ceilings, "fan": PS.slope_fan, "tops": PS.top_sweep, "long": PS.long_rings, "degenerate": PS.degenerate_records,
         "carry": PS.carry_field}


@functools.lru_cache(maxsize=None)
def soup_case(kind, *args):
    """-> ((rings, ring_row, ring_xy), info, the expected polygons): the definition's, and for the carry field (where the
    definition is quadratic) the construction's; computed once, shared with the GPU tests, left unchanged"""
    rings, row, xy, info = SOUPS[kind](*args)
    want = PS.answer_from_parents(rings, info["parent"]) if kind == "carry" else PR.polygons_ref(rings, row, xy)
    return (rings, row, xy), info, want


def is_candidate(u, v, p, num=int):
    """the test of candidate() in Python integers, or in floats"""
    return v[0] <= p[0] < u[0] and num(u[1] - v[1]) * num(p[0] - v[0]) > num(p[1] - v[1]) * num(u[0] - v[0])


def height_at(u, v, px, num=Fraction):
    return num(v[1]) + num(u[1] - v[1]) * num(px - v[0]) / num(u[0] - v[0])


def check_twin(twin, args, want, what):
    rc, got, stats = twin_polygons(twin, *args)
    assert rc == 0, what
    PR.assert_same_polygons(got, want, what)
    return stats


@pytest.mark.parametrize("seed", SLIVER_SEEDS)
def test_sliver_soup_is_decided_by_exact_products_and_remainders(twin, seed):
    """heights p.y + t / d with d near 2^45 and t in [-2, 5]: candidate() compares two products near 2^90 that differ by t,
    two candidates differ by about 2^-45 (the step rem_a d_b against rem_b d_a of lower()), half of the edges fall (a
    negative n in floor_div).  The seed conditions: per hole a quarter of its edges are candidates and a quarter are not;
    the candidate test in floats decides at least one edge differently; the float heights order at least one pair of
    candidates differently; a falling edge is a candidate; the bucket of a hole holds all its edges."""
    args, info, want = soup_case("sliver", seed)
    stats = check_twin(twin, args, want, seed)
    flips = orders = falling = 0
    for _, p, edges in info["holes"]:
        cands = [e for e in edges if e[2] > 0]
        assert 4 * len(cands) >= len(edges) and 4 * (len(edges) - len(cands)) >= len(edges), seed
        for u, v, t, d in edges:
            assert is_candidate(u, v, p) == (t > 0) and height_at(u, v, p[0]) == p[1] + Fraction(t, d) and u[0] - v[0] == d
            flips += is_candidate(u, v, p, float) != (t > 0)
        falling += sum(1 for u, v, _, _ in cands if u[1] < v[1])
        hs = [(Fraction(t, d), height_at(u, v, p[0], float)) for u, v, t, d in cands]
        orders += sum(1 for a, b in itertools.combinations(hs, 2) if (a[0] < b[0]) != (a[1] < b[1]))
    assert flips >= 1 and orders >= 1 and falling >= 1, (seed, flips, orders, falling)
    assert stats["longest_bucket"] >= len(info["holes"][0][2]) and stats["shift"] >= 40
    assert want["counts"]["n_holes"] >= len(info["holes"]) and want["counts"]["n_polygons"] > 100


@pytest.mark.parametrize("seed", FAN_SEEDS)
def test_slope_fan_is_decided_by_exact_slopes_then_slots(twin, seed):
    """per hole a fan of candidates of exactly equal height (an integer with n = 0, a half, an integer with n = dy dx)
    whose neighbouring slopes differ by 1 / (dx_a dx_b), the cross products of lower() by 1, 2 or 4; the lowest slope comes
    more than once, and in the first fan once more with twice the length: the ring of the smallest slot is the ring above.
    The seed conditions:
    every fan edge is a candidate of the fan's height, the copies and the collinear edge among them; the cross products
    of lower() in floats order at least one neighbouring pair differently; the winners fall and rise."""
    args, info, want = soup_case("fan", seed)
    check_twin(twin, args, want, seed)
    _, above = PR.above_of(*args)
    flips, signs = 0, set()
    for g, n_ties, det in zip(info["groups"], (4, 2, 2), (1, 2, 4)):
        p = g["p"]
        for _, u, v in g["edges"]:
            assert is_candidate(u, v, p) and height_at(u, v, p[0]) == g["height"], seed
        assert len(g["ties"]) == n_ties and g["above"] == min(g["ties"]) and above[g["hole"]] == g["above"], seed
        assert int(want["parent"][g["hole"]]) == g["above"], seed
        by_ring = {r: (u, v) for r, u, v in g["edges"]}
        lengths = {by_ring[r][0][0] - by_ring[r][1][0] for r in g["ties"]}
        assert len(lengths) == (2 if n_ties == 4 else 1)  # (the collinear edge of double length)
        for a, b in g["pairs"]:
            (ua, va), (ub, vb) = g["edges"][a][1:], g["edges"][b][1:]
            dya, dxa, dyb, dxb = ua[1] - va[1], ua[0] - va[0], ub[1] - vb[1], ub[0] - vb[0]
            assert abs(dya * dxb - dyb * dxa) == det
            flips += (dya * dxb < dyb * dxa) != (float(dya) * float(dxb) < float(dyb) * float(dxa))
        u, v = by_ring[g["above"]]
        signs.add(u[1] > v[1])
    assert flips >= 1 and signs == {False, True}, (seed, flips, signs)
    assert info["groups"][1]["height"].denominator == 2 and info["groups"][2]["p"][0] > info["groups"][2]["edges"][0][2][0]


def test_top_sweep_has_the_top_at_every_lane_position(twin):
    """rings of 1 to 1000 points, the top at every index: a ring whose top comes out as any other of its points -- the point
    of equal y and smaller x among them -- has the decoy above it.  Every lane position of a group of 8 holds a top, and
    a point of equal y sits in another one."""
    args, info, want = soup_case("tops")
    PR.assert_same_polygons(PS.answer_from_parents(args[0], info["parent"]), want)
    check_twin(twin, args, want, "tops")
    assert {t % 8 for _, _, t, _ in info["holes"]} == set(range(8)) and {n for _, n, _, _ in info["holes"]} == set(PS.TOP_SIZES)
    assert all((twin_at is None) == (n == 1) and (n == 1 or twin_at % 8 != t % 8) for _, n, t, twin_at in info["holes"])
    assert want["counts"] == dict(n_polygons=len(info["holes"]) + 1, n_members=2 * len(info["holes"]) + 1, n_holes=len(info["holes"]), n_orphans=0,
                                  n_face0=0)
    assert int(np.abs(args[2]).max()) == PS.LIM
    # the decoy does its work: with the equal-y point as the top the ring above is the decoy
    rings, row, xy = args
    ring, n, t, twin_at = next(h for h in info["holes"] if h[1] == 17)
    moved = xy.copy()
    moved[int(row[ring]) + t, 0] -= 20
    assert int(PR.polygons_ref(rings, row, moved)["parent"][ring]) != int(want["parent"][ring])


def test_long_rings_have_the_top_late_and_the_winning_edge_deep(twin):
    args, info, want = soup_case("long")
    PR.assert_same_polygons(PS.answer_from_parents(args[0], info["parent"]), want)
    check_twin(twin, args, want, "long")
    row = args[1].tolist()
    assert sorted(b - a for a, b in zip(row, row[1:])) == [2, 2, 4, PS.LONG, PS.LONG] and want["parent"].tolist() == [1, 1, 2, 3, 4]


@pytest.mark.parametrize("faces", PS.DEGENERATE_FACES)
def test_degenerate_records(twin, faces):
    """a column of 40 holes without a shell (orphans by walks of up to 39 steps and the end), the same column with one,
    rings without points of every kind as the first, a middle and the last ring of their face, a one-point ring; faces
    outside [0, 2^31) order as unsigned"""
    args, info, want = soup_case("degenerate", faces)
    PR.assert_same_polygons(PS.answer_from_parents(args[0], info["parent"]), want, faces)
    stats = check_twin(twin, args, want, faces)
    assert want["counts"] == PS.DEGENERATE_COUNTS, faces
    kinds, above = PR.above_of(*args)
    steps, at = 0, info["column"][0]
    while above[at] is not None:
        at, steps = above[at], steps + 1
    assert steps >= 32 and kinds[at] == "hole" and stats["rounds"] >= 6, (faces, steps)
    rings, row, _ = args
    empty = np.flatnonzero(np.diff(row.astype(np.int64)) == 0).tolist()
    assert len(empty) == 9 and empty[0] == 0 and empty[-1] == len(rings) - 1 and int(row[-2]) == int(row[-1])
    key = (rings["face"].astype(np.int64) & 0xFFFFFFFF) << 32 | rings["leader"]
    assert (np.diff(key) > 0).all() and set(rings["face"].tolist()) == {0, *faces}


@pytest.mark.parametrize("salt", [0, 1])
def test_carry_field_sums_int128_areas_over_many_members(twin, salt):
    """20 000 polygons of a shell of 2^65 and a hole of -2 (2^32 - 2)(2^32 - 3) in three faces: 40 000 members, 39
    blocks of the device's int128 scan (rocPRIM's default configuration for a 16-byte type that is no built-in integer:
    256 threads of 16 / (16 / 4) = 4 items, 1024 to a block; 3584 with the tuning for gfx942, 1280 with the one for an
    unknown target).  The prefix crosses a multiple of 2^64 at every member.  With salt 0 the low words never carry (2^65
    has none, the holes' add up to 20 000 (10 x 2^32 - 12)); salt 1 adds a pseudo-random low word to every recorded shell
    area, and the low words of the prefix carry into the high ones at about half of the shells."""
    args, info, want = soup_case("carry", CARRY_SQUARES, salt)
    check_twin(twin, args, want, salt)
    n = CARRY_SQUARES
    crossings = carries = prefix = 0
    for a in info["areas"]:
        crossings += (prefix + a) >> 64 != prefix >> 64
        carries += (prefix & PS.M64) + (a & PS.M64) > PS.M64 and a > 0
        prefix += a
    assert 2 * crossings >= n and len(info["areas"]) == 2 * n and (salt == 0 or 4 * carries >= n), (crossings, carries)
    assert want["counts"] == dict(n_polygons=n, n_members=2 * n, n_holes=n, n_orphans=0, n_face0=0)
    if salt == 0:
        assert set(PR.area2_of(want["polygons"])) == {10 * (1 << 32) - 12}
    # the definition itself on a field that is small enough for it
    small, small_info, _ = soup_case("carry", 300, salt)
    PR.assert_same_polygons(PS.answer_from_parents(small[0], small_info["parent"]), PR.polygons_ref(*small), salt)


def test_an_edge_that_ends_on_a_strip_boundary_has_no_entry_beyond_it(twin):
    """the ceiling edge (65536, 9) -> (65526, 9) lies in strips strip(v.x) .. strip(u.x - 1): one entry under shift 16, although
    u.x starts the next strip (an entry there would change no answer -- p.x < u.x fails for every ray of that strip --
    only the count of entries that the shift is chosen by)"""
    rings, row, xy, index = PS.pack([(1, 0, -7, PS._triangle(65530, 5)[0]), (1, 1, 1, [(65536, 9), (65526, 9)])])
    want = PR.polygons_ref(rings, row, xy)
    stats = check_twin(twin, (rings, row, xy), want, "boundary")
    assert want["parent"].tolist() == [1, 1] and (65536 + PS.LIM) % (1 << 16) == 0
    assert stats["shift"] == 16 and stats["n_edges"] == 2 and stats["n_entries"] == 2, stats


@functools.lru_cache(maxsize=None)
def big_field_case():
    """PC.hole_field(520) -> (the map, its rings by the rings twin, their polygons and stats by the polygons twin): once for
    the CPU and the GPU test (the twin takes seconds: each of 270 400 holes against the 521 ceiling edges of its bucket)"""
    m = PC.hole_field(BIG_FIELD_SIDE)
    rc, rg, _ = twin_rings(rings_twin_lib(), m)
    assert rc == 0
    rc, got, stats = twin_polygons(twin_lib(), *args_of(rg))
    assert rc == 0
    return m, rg, got, stats


def check_hole_field(rings, got, stats, n):
    """the construction's answer of PC.hole_field with n holes, and the counts written out"""
    PR.assert_same_polygons(got, PS.hole_field_answer(rings, n))
    assert got["counts"] == dict(n_polygons=n + 1, n_members=2 * n + 1, n_holes=n, n_orphans=0, n_face0=1)
    assert int(got["polygons"]["n_holes"][0]) == n and (got["parent"][1:n + 2] == 1).all() and stats["shift"] == 16


def test_hole_field_of_270400_holes_on_the_twin_has_the_parents_of_the_construction():
    """540 802 rings: more than the 262 144 that one grid of the device's lane groups of 8 covers"""
    _, rg, got, stats = big_field_case()
    n = BIG_FIELD_SIDE * BIG_FIELD_SIDE
    assert len(rg["rings"]) == 2 * n + 2 > 2 * 262144 and stats["longest_bucket"] == BIG_FIELD_SIDE + 1
    check_hole_field(rg["rings"], got, stats, n)


# ---- the contract of the call ----------------------------------------------------------------------------------------------
def test_each_capacity_one_short_overflows_with_the_true_counts(twin):
    rg, p = hand_case("multi-part")
    true = (p["counts"]["n_polygons"], p["counts"]["n_members"])
    rc, got, _ = twin_polygons(twin, *args_of(rg), caps=(0, 0))  # the sizing call
    assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == p["counts"] and np.array_equal(got["parent"], p["parent"])
    for short in range(2):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, got, _ = twin_polygons(twin, *args_of(rg), caps=caps)
        assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == p["counts"], short
        assert np.array_equal(got["polygons"], p["polygons"][:caps[0]]) and np.array_equal(got["poly_ring"], p["poly_ring"][:caps[1]])
    rc, got, _ = twin_polygons(twin, *args_of(rg), caps=true)
    assert rc == 0
    PR.assert_same_polygons(got, p)


def bad_inputs():
    """(what, rings, ring_row, ring_xy, flags): each RJ_E_INVALID"""
    rg = D.rings_ref(*K.square_with_hole())
    rings, row, xy = args_of(rg)
    short = row.copy()
    short[-1] -= 1
    far = xy.copy()
    far[far == 10] = 1 << 46
    return [("ring_row does not end at n_points", rings, short, xy, 0), ("a coordinate of 2^46", rings, row, far, 0),
            ("rings out of order", rings[[0, 2, 1, 3]], row, xy, 0), ("flags", rings, row, xy, 1)]


def test_bad_input_is_invalid(twin):
    for what, rings, row, xy, flags in bad_inputs():
        rc, got, _ = twin_polygons(twin, rings, row, xy, flags)
        assert rc == _capi.RJ_E_INVALID and got["counts"] == dict.fromkeys(PR.COUNTS, 0), what
    rc, got, _ = twin_polygons(twin, np.zeros(0, D.RING_DTYPE), np.zeros(1, np.uint32), np.zeros((0, 2), np.int64))  # n_rings == 0
    assert rc == 0 and got["counts"] == dict.fromkeys(PR.COUNTS, 0) and got["poly_first"].tolist() == [0]


def test_symbol_record_and_counts():
    assert "rj_rings_polygons" in _capi.SYMBOLS and hasattr(_capi.load(), "rj_rings_polygons")
    assert _capi.POLYGON_DTYPE == PR.POLYGON_DTYPE and _capi.POLYGON_DTYPE.itemsize == 32
    assert _capi.POLYGONS_COUNTS == PR.COUNTS and _capi.RJ_POLY_NONE == NONE
    assert issubclass(_capi.PolygonsOverflow, _capi.RayJoinError)
