"""Thinning the chains of a map on the CPU: the plain-Python definition (tests/simplify_ref.py) on the hand-built maps
of tests/simplify_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/simplify_twin.cc compiling rayjoin_amd/csrc/rj_simplify.h) against that definition, every array and
every count, over the work list and over all points, with and without origin: the hand cases, 40 random maps of open
and closed chains on small lattices at three tolerances each (0 and 2^128 - 1 among them), one chain of 5 000 points;
the properties that the header states (no unpinned point at or below the tolerance is left, a second call removes
nothing, 2^128 - 1 leaves the pinned points alone, the pins of the output are the pins of the input); the contract of
the call; the twin as a stand-alone program.  The GPU side is tests/test_gpu_simplify.py.

Mutations of a scratch copy of rj_simplify.h (RJ_SIMPLIFY_HEADER_DIR points the twin's build at it), and the tests here
that fail under each (328 tests at the time; a named case fails in the twin test, most also in the properties):
  is_candidate with < for <=: 126 -- "peak-at", "negative-at", "big-at", "equal-weights" and every case at tolerance 0
      ("collinear-100", "line-then-off", "spike", "square-mid-zero", "one-point-chains", "vertical-and-right-to-left",
      "chain-boundary-closed"), the sizing test, the work-list test, the long chain and the random maps
  the hash dropped from the key (tie_of returns p): 93 -- "collinear-100", "line-then-off", the work-list test, the
      sizing test, the long chain and the random maps (their rounds, and the points kept where equal weights meet)
  a neighbour taken across a chain boundary (chain_first true for the map's first point only): 164 -- "chain-boundary",
      "chain-boundary-closed", the sizing test, the stand-alone program, every random map
  m2 not pinned (wide_of gives every point the value 0): 133 -- "square", "square-mid-zero", "square-mid-huge",
      "chain-boundary-closed", the sizing test, the random maps with a closed chain that is no line
  only one neighbour compared (removes() without the test of next[p]): 113 -- "collinear-100", "equal-weights",
      "line-then-off", "ring-of-one-place", "staircase-200", the work-list test, the sizing test, the long chain and the
      random maps (adjacent points go in one round and the links break)
  magnitude() without the absolute value (a negative cross product becomes a number above every weight): 145 --
      "peak-at", "negative-at", "equal-weights", "square-mid-zero", "square-mid-huge", "staircase-200", the work-list test,
      the sizing test, the long chain and the random maps"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simplify_cases as SC  # noqa: E402
import simplify_ref as SR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "simplify_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HDR_DIR = os.environ.get("RJ_SIMPLIFY_HEADER_DIR", CSRC)  # (a scratch copy: the mutation runs)
HDRS = [os.path.join(HDR_DIR, "rj_simplify.h"), os.path.join(CSRC, "rj_crossings.h"), os.path.join(CSRC, "rj_rings.h")]
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
MUTANT = "" if "RJ_SIMPLIFY_HEADER_DIR" not in os.environ else "_mutant"
OUT = os.path.join(BUILD, "libsimplify_twin%s.so" % MUTANT)
CANARY = 0x5B5B5B5B5B5B5B5B
OK, INVALID, OVERFLOW = 0, 1, 3
HUGE = SC.HUGE
LONG = 5000
LONG_TOLS = (0, 50, HUGE)


def stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


def twin_lib():
    os.makedirs(BUILD, exist_ok=True)
    if stale(OUT):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", HDR_DIR, "-I", CSRC, "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.simplify_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.simplify_twin_last.argtypes = [C.c_void_p]
    L.simplify_twin_last.restype = None
    return L


def twin_last(L):
    """-> (the rounds that the twin's last call ran, the one that found nothing included; its work lists behind the first, summed)"""
    out = np.zeros(2, np.uint64)
    L.simplify_twin_last(out.ctypes.data)
    return int(out[0]), int(out[1])


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_simplify(L, m, tol, flags=0, capacity=None, origin=True, all_points=False):
    """-> (status, out_xy, out_row, origin, counts).  capacity None: the sizing call, then the exact capacity.  Behind the
    capacity lie canaries that must survive; an overflow or a refusal must leave every output as it was."""
    xy, row = np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32)
    nc = max(0, len(row) - 1)
    counts = np.zeros(6, np.uint64)

    def call(cap, out_xy, out_row, org):
        return L.simplify_twin(xy.ctypes.data, len(xy), row.ctypes.data, nc, tol & (2 ** 64 - 1), tol >> 64, flags, int(all_points), cap,
                               out_xy.ctypes.data if out_xy is not None else None, out_row.ctypes.data if out_row is not None else None,
                               org.ctypes.data if org is not None else None, counts.ctypes.data)

    def named():
        return dict(zip(SR.COUNTS, (int(v) for v in counts)))
    if capacity is None:
        rc = call(0, None, None, None)
        if rc not in (OK, OVERFLOW):
            return rc, None, None, None, named()
        capacity = int(counts[0])
    out_xy = np.full((capacity + 2, 2), CANARY, np.int64)
    out_row = np.full(nc + 3, 0x5B5B5B5B, np.uint32)
    org = np.full(capacity + 2, 0x5B5B5B5B, np.uint32) if origin else None
    rc = call(capacity, out_xy, out_row, org)
    c = named()
    assert (out_xy[capacity:] == CANARY).all() and (out_row[nc + 1:] == 0x5B5B5B5B).all()
    if rc != OK:
        assert (out_xy == CANARY).all() and (out_row == 0x5B5B5B5B).all() and (org is None or (org == 0x5B5B5B5B).all())
        return rc, None, None, None, c
    assert org is None or (org[c["n_points"]:] == 0x5B5B5B5B).all()
    return rc, out_xy[:c["n_points"]], out_row[:nc + 1], org[:c["n_points"]] if origin else None, c


def same(got, want):
    """(status, out_xy, out_row, origin, counts) of the twin against simplify_ref's (out_xy, out_row, origin, counts)"""
    rc, xy, row, org, c = got
    assert rc == OK and c == want[3]
    assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1]) and (org is None or np.array_equal(org, want[2]))


@functools.lru_cache(maxsize=None)
def map_of(kind, key):
    """the map of a case: computed once, shared, never changed"""
    return {"hand": lambda: SC.chain_arrays(SC.HAND[key][0]), "random": lambda: SC.random_map(key), "long": lambda: SC.long_chain(key),
            "collinear": lambda: SC.chain_arrays(SC.collinear(key)), "staircase": lambda: SC.chain_arrays(SC.staircase(key))}[kind]()


@functools.lru_cache(maxsize=None)
def thinned(kind, key, tol):
    """the definition's answer: computed once, shared, never changed"""
    m = map_of(kind, key)
    return SR.simplify_ref(m[0], m[1], tol)


RANDOM = [("random", s, t) for s in SC.SEEDS for t in SC.tols(s)]
EVERY = [("hand", n, SC.HAND[n][1]) for n in sorted(SC.HAND)] + RANDOM + [("long", LONG, t) for t in LONG_TOLS]


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.HAND))
def test_definition_gives_the_written_answer(name):
    chains, tol, kept, (n_rounds, n_closed, n_pinned_extra) = SC.HAND[name]
    xy, row, origin, c = thinned("hand", name, tol)
    m = map_of("hand", name)
    assert origin.tolist() == kept and np.array_equal(xy, m[0][kept])
    assert (c["n_rounds"], c["n_closed"], c["n_pinned_extra"]) == (n_rounds, n_closed, n_pinned_extra)
    assert c["n_points"] == len(kept) and c["n_removed"] == len(m[0]) - len(kept) and len(row) == len(chains) + 1
    assert (c["n_max_round"] == 0) == (c["n_removed"] == 0) and c["n_max_round"] * c["n_rounds"] >= c["n_removed"]


def test_definition_hashed_ties_thin_a_line_in_few_rounds():
    """10 000 collinear points go in 19 rounds (one per round under a tie-break by index)"""
    c = thinned("collinear", 10000, 0)[3]
    assert (c["n_points"], c["n_rounds"]) == (2, 19)


def test_random_maps_are_worth_their_time():
    """closed chains with one and with two extra pins and with none, ties, tolerances that remove some points and not all"""
    cs = [thinned(*w)[3] for w in RANDOM]
    assert sum(c["n_closed"] for c in cs) > 100 and sum(c["n_pinned_extra"] for c in cs) > 100
    assert sum(1 for c in cs if c["n_closed"] * 2 > c["n_pinned_extra"]) > 10
    assert sum(1 for w, c in zip(RANDOM, cs) if 0 < w[2] < HUGE and 0 < c["n_removed"] and c["n_points"] > 30) > 10
    assert max(c["n_rounds"] for c in cs) >= 10 and sum(c["n_removed"] for c in cs) > 20000


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_twin(twin, what):
    m, want = map_of(*what[:2]), thinned(*what)
    same(twin_simplify(twin, m, what[2]), want)
    same(twin_simplify(twin, m, what[2], all_points=True), want)
    same(twin_simplify(twin, m, what[2], origin=False), want)


def test_twin_work_lists_are_short(twin):
    """the staircase: every point is a candidate to the end, the list of round k is what is left; the long chain at 50:
    behind the first round the nine lists together hold 9 816 points, two passes where all points cost nine"""
    same(twin_simplify(twin, map_of("hand", "staircase-200"), HUGE, capacity=200), thinned("hand", "staircase-200", HUGE))
    assert twin_last(twin) == (198, 197 * 198 // 2)
    same(twin_simplify(twin, map_of("long", LONG), 50, capacity=LONG), thinned("long", LONG, 50))
    rounds, looked = twin_last(twin)
    assert rounds == thinned("long", LONG, 50)[3]["n_rounds"] + 1 == 10 and 0 < looked < 2 * LONG
    same(twin_simplify(twin, map_of("long", LONG), 50, capacity=LONG, all_points=True), thinned("long", LONG, 50))
    assert twin_last(twin) == (rounds, 0)


# ---- the properties ------------------------------------------------------------------------------------------------------
def pinned_of(xy, row):
    pts = [tuple(p) for p in np.asarray(xy).tolist()]
    out = set()
    for b, e in zip(row[:-1].tolist(), row[1:].tolist()):
        out |= SR.pins_of(pts, b, e)[0]
    return out


def properties(simplify, m, tol):
    """simplify(map, tol) -> (xy, row, origin)"""
    xy, row, origin = simplify(m, tol)
    pins_in, pins_out = pinned_of(*m), pinned_of(xy, row)
    assert {int(origin[k]) for k in pins_out} == pins_in  # the pins of the output are the pins of the input
    assert (np.diff(origin.astype(np.int64)) > 0).all() and np.array_equal(xy, np.asarray(m[0])[origin])
    assert np.array_equal(origin[row[:-1]], m[1][:-1]) and np.array_equal(origin[row[1:] - 1], m[1][1:] - 1)  # every chain keeps its ends
    pts = [tuple(p) for p in xy.tolist()]
    for k in range(len(pts)):
        if k not in pins_out:
            assert abs(SR.cross(pts[k - 1], pts[k], pts[k + 1])) > tol
    if tol == HUGE:
        assert set(range(len(pts))) == pins_out
    xy2, row2, origin2 = simplify((xy, row), tol)
    assert np.array_equal(xy2, xy) and np.array_equal(row2, row) and np.array_equal(origin2, np.arange(len(xy)))


@pytest.mark.parametrize("what", EVERY, ids=str)
def test_properties(twin, what):
    def by_twin(m, tol):
        rc, xy, row, origin, _ = twin_simplify(twin, m, tol)
        assert rc == OK
        return xy, row, origin
    properties(by_twin, map_of(*what[:2]), what[2])
    properties(lambda m, tol: SR.simplify_ref(m[0], m[1], tol)[:3], map_of(*what[:2]), what[2])


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_one_short(twin):
    m, want = map_of("random", 5), thinned("random", 5, 60)
    n = want[3]["n_points"]
    assert 0 < want[3]["n_removed"] < len(m[0]) - 2 * (len(m[1]) - 1)
    rc, _, _, _, c = twin_simplify(twin, m, 60, capacity=0)
    assert rc == OVERFLOW and c == want[3]
    same(twin_simplify(twin, m, 60, capacity=n), want)
    rc, _, _, _, c = twin_simplify(twin, m, 60, capacity=n - 1)  # (twin_simplify checks that nothing was written)
    assert rc == OVERFLOW and c == want[3]
    same(twin_simplify(twin, m, 60, capacity=n + 5), want)


def test_no_chains(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32))
    rc, xy, row, org, c = twin_simplify(twin, empty, 5)
    assert rc == OK and len(xy) == 0 and row.tolist() == [0] and c == dict.fromkeys(SR.COUNTS, 0)
    same((rc, xy, row, org, c), SR.simplify_ref(empty[0], empty[1], 5))
    points = SC.chain_arrays([[(1, 1)], [(2, 2)]])
    same(twin_simplify(twin, points, HUGE), SR.simplify_ref(points[0], points[1], HUGE))


def refused(twin, m, tol=0, flags=0):
    """the definition refuses it, and so does the twin"""
    with pytest.raises(SR.Invalid):
        SR.simplify_ref(m[0], m[1], tol, flags)
    return twin_simplify(twin, m, tol, flags)[0] == INVALID and twin_simplify(twin, m, tol, flags, capacity=len(m[0]))[0] == INVALID


def test_bad_input(twin):
    xy, row = SC.chain_arrays([[(0, 0), (1, 0)], [(2, 0), (3, 0)], [(4, 0), (5, 0)]])
    assert twin_simplify(twin, (xy, row), 0)[0] == OK
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        assert refused(twin, (xy, np.array(bad_row, np.uint32)))
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert refused(twin, (bad, row))
    assert refused(twin, (xy, row), flags=1) and refused(twin, (xy, row), flags=1 << 31)


# ---- the stand-alone program ----------------------------------------------------------------------------------------------
def test_stand_alone_twin_program():
    """the twin with its own main (what a host sanitizer build is made from: -fsanitize=address,undefined on this very
    command line), run as a program of its own: the work list against all points, and a second call that removes nothing"""
    exe = os.path.join(BUILD, "simplify_twin_main%s" % MUTANT)
    os.makedirs(BUILD, exist_ok=True)
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DSIMPLIFY_TWIN_MAIN", "-I", HDR_DIR, "-I", CSRC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == 5 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
