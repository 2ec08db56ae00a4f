"""Cutting a chain map at its rounded proper crossings on the CPU: the plain-Python definition (tests/snap_ref.py) on
the hand-built maps of tests/snap_cases.py with the answers written out; the host twin of the device's per-element
functions (tests/hosttwin/snap_twin.cc compiling rayjoin_amd/csrc/rj_snap.h) against that definition, every array and
every count, with and without RJ_SNAP_DROP_LAST: the hand cases, 63 / 64 / 65 records, stars of 65 and 129 edges through
one half-integer point, one long edge with 300 crossings and 300 T-junctions, every map of tests/node_cases.py, the
soups of the crossings and the noding tests, 20 maps of random segments; the wide arithmetic at +-2^46 against Python
integers; the properties of one round; the rounds (clean within 8 on every soup, a fan that is not after 2); the
contract of the call; mutations of a scratch copy of the header, each of which the hand cases catch.  The GPU side is
tests/test_gpu_snap.py.

The mutations (test_header_mutations_are_caught applies them; RJ_SNAP_HEADER_DIR points the twin's build at the copy):
  halves rounded down (2 R >= den <-> 2 R > den in both directions): "half", "half-reversed", "half-one-reversed", "shallow-ties", "steep"
  the minor offset dropped from the key: "minor-tie", "minor-tie-reversed"
  q laid off from f's first point instead of e's: "x" and every other proper crossing.  (Computing q consistently from f
      -- f's direction with f's parameter -- gives the same point by definition: rnd is applied to the exact
      coordinate, which does not depend on the edge.  "From the lower-numbered edge" fixes the computation, not the
      value; the mutation that can be caught is the inconsistent one.)
  the end-point drop removed: "at-end"
  the stale test removed: "stale-t", "stale-apart", "wrong-kinds" ("stale-parallel" would divide by zero: the mutant
      keeps the den == 0 test)"""
import ctypes as C
import functools
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_cases as CC  # noqa: E402
import crossings_ref as CR  # noqa: E402
import node_cases as NC  # noqa: E402
import node_ref as NR  # noqa: E402
import snap_cases as SC  # noqa: E402
import snap_ref as SR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "snap_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
CANARY = 0x5B5B5B5B5B5B5B5B
RECORD = np.dtype([("eid", np.uint32, 2), ("kind", np.uint32), ("_pad", np.uint32)])
OK, INVALID, OVERFLOW = 0, 1, 3
DROP_LAST = 1
LONG_EDGE = 300
L = 1 << 46


def twin_lib(header_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libsnap_twin%s.so" % tag)
    hdrs = [os.path.join(header_dir, "rj_snap.h")] + [os.path.join(CSRC, h) for h in ("rj_node.h", "rj_crossings.h", "rj_rings.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", header_dir, "-I", CSRC, "-o", out, SRC])
    lib = C.CDLL(out)
    lib.snap_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    lib.snap_point.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.snap_point.restype = None
    return lib


@pytest.fixture(scope="module")
def twin():
    return twin_lib(os.environ.get("RJ_SNAP_HEADER_DIR", CSRC), "" if "RJ_SNAP_HEADER_DIR" not in os.environ else "_env")


def record_array(records):
    out = np.zeros(len(records), RECORD)
    for k, (e, f, kind) in enumerate(records):
        out[k] = ((e, f), kind, 0)
    return out


def twin_snap(lib, m, records, flags=0, capacity=None, origin=True):
    """-> (status, out_xy, out_row, origin, counts).  capacity None: the sizing call, then the exact capacity.  Behind the
    capacity lie canaries that must survive; an overflow or a refusal must leave every output as it was."""
    xy, row = np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32)
    rec = records if isinstance(records, np.ndarray) else record_array(records)
    nc = max(0, len(row) - 1)
    counts = np.zeros(len(SR.COUNTS), np.uint64)

    def call(cap, out_xy, out_row, org):
        return lib.snap_twin(xy.ctypes.data, len(xy), row.ctypes.data, nc, rec.ctypes.data if len(rec) else None, len(rec), flags, cap,
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
    assert org is None or (org[c["n_edges"]:] == 0x5B5B5B5B).all()
    return rc, out_xy[:c["n_points"]], out_row[:nc + 1], org[:c["n_edges"]] if origin else None, c


def same(got, want):
    """(status, out_xy, out_row, origin, counts) of the twin against snap_ref's (out_xy, out_row, origin, counts)"""
    rc, xy, row, org, c = got
    assert rc == OK and c == want[3]
    assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1]) and (org is None or np.array_equal(org, want[2]))


MAKERS = {"hand": lambda key: SC.chain_arrays(SC.HAND[key][0]), "comb": SC.comb, "star": SC.star, "long": lambda key: SC.long_mixed(key)[0],
          "segments": SC.random_segments, "fan": lambda key: SC.fan(), "node-hand": lambda key: NC.chain_arrays(NC.HAND[key][0]),
          "wall": NC.wall_map, "soup": NC.soup, "closed-soup": NC.closed_soup, "node-long": lambda key: NC.long_edge(key)[0],
          "crossings-soup": CC.soup}


@functools.lru_cache(maxsize=None)
def records_of(kind, key):
    """-> (the map, its records as tuples -- a hand case's own where it has some, else the crossings by definition --, the
    crossings' counts): computed once, shared, never changed"""
    m = MAKERS[kind](key)
    records, counts = CR.map_crossings_ref(*m)
    if kind == "hand" and SC.HAND[key][3] is not None:
        records = SC.HAND[key][3]
    return m, records, counts


@functools.lru_cache(maxsize=None)
def snapped(kind, key, drop_last=False):
    m, records, _ = records_of(kind, key)
    return SR.snap_ref(m[0], m[1], records, drop_last)


@functools.lru_cache(maxsize=None)
def rounds_of(kind, key, max_rounds=8, drop_last=False):
    m, _, _ = records_of(kind, key)
    return SR.snap_rounds_ref(m[0], m[1], max_rounds, drop_last)


GRAIN = [("comb", n) for n in SC.RECORD_COUNTS] + [("star", k) for k in SC.STARS] + [("long", LONG_EDGE)]
NODE_MAPS = [("node-hand", n) for n in sorted(NC.HAND)] + [("wall", k) for k in sorted(NC.WALLS)] + [("node-long", 300)]
SOUPS = [(kind, s) for kind in ("crossings-soup", "soup", "closed-soup") for s in range(40)]
SEGMENTS = [("segments", s) for s in SC.SEGMENT_SEEDS]


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.HAND))
def test_definition_gives_the_written_answer(name):
    want_xy, want_row = SC.chain_arrays(SC.HAND[name][1])
    got = snapped("hand", name)
    assert np.array_equal(got[0], want_xy) and np.array_equal(got[1], want_row)
    assert {k: got[3][k] for k in SC.HAND[name][2]} == SC.HAND[name][2]
    assert got[3]["n_points"] == len(want_xy) and got[3]["n_edges"] == len(want_xy) - (len(want_row) - 1) == len(got[2])
    assert (np.diff(got[2].astype(np.int64)) >= 0).all()


def test_definition_on_the_grain_cases():
    """the star's crossings all round to one point; the long edge carries 600 cuts in the written order, 43 of them both a
    vertex and a rounded crossing"""
    for k in SC.STARS:
        _, records, counts = records_of("star", k)
        got = snapped("star", k)
        assert counts["n_proper"] == len(records) == k * (k - 1) // 2 and got[3]["n_cuts"] == got[3]["n_cut_edges"] == k and got[3]["n_max_cuts"] == 1
        assert got[0].reshape(-1, 3, 2)[:, 1].tolist() == [[1, 1]] * k
    for n in SC.RECORD_COUNTS:
        assert len(records_of("comb", n)[1]) == n and snapped("comb", n)[3]["n_max_cuts"] == n
    want = SC.long_mixed(LONG_EDGE)[1]
    got = snapped("long", LONG_EDGE)
    assert [tuple(p) for p in got[0][:len(want)].tolist()] == want and got[3]["n_max_cuts"] == 2 * LONG_EDGE and got[3]["n_proper"] == LONG_EDGE
    assert got[3]["n_used"] == LONG_EDGE + len(range(0, LONG_EDGE, 7))


def test_the_end_to_end_answer_of_the_two_squares():
    """two overlapping squares: one round, 4 chains, 3 bounded faces of 24, 8 and 24 (twice their areas)"""
    import faces_ref as FR
    import ringmap_ref as RM
    ring_xy = np.array([p for r in SC.TWO_SQUARES for p in r], np.int64)
    ring_row = np.array([0, 4, 8], np.uint32)
    xy, row = NC.closed_chains(ring_row, ring_xy)
    xy, row, rounds, clean, _ = SR.snap_rounds_ref(xy, row, 8, True)
    assert clean and len(rounds) == 1 and rounds[0]["snap"]["n_exact"] == 2
    cm = RM.rings_map_ref(row, xy, np.array([1, 2], np.int32))
    assert cm["counts"]["n_chains"] == 4
    faces = FR.faces_ref(cm["xy"], cm["row_index"])
    assert sorted(FR.area2_of(faces["faces"])) == [8, 24, 24]


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.HAND))
def test_twin_hand_cases(twin, name):
    m, records, _ = records_of("hand", name)
    same(twin_snap(twin, m, records), snapped("hand", name))
    same(twin_snap(twin, m, records, origin=False), snapped("hand", name))
    if name in SC.CLOSED:
        same(twin_snap(twin, m, records, DROP_LAST), snapped("hand", name, True))


@pytest.mark.parametrize("what", GRAIN + SEGMENTS, ids=str)
def test_twin_grain_and_random_segments(twin, what):
    m, records, _ = records_of(*what)
    same(twin_snap(twin, m, records), snapped(*what))


@pytest.mark.parametrize("what", SOUPS, ids=str)
def test_twin_soups(twin, what):
    m, records, _ = records_of(*what)
    same(twin_snap(twin, m, records), snapped(*what))
    if what[0] == "closed-soup":
        same(twin_snap(twin, m, records, DROP_LAST), snapped(*what, True))


def without_proper(records):
    return [r for r in records if r[2] != SR.PROPER]


@pytest.mark.parametrize("what", NODE_MAPS + [("soup", s) for s in range(40)] + [("closed-soup", s) for s in range(0, 40, 4)], ids=str)
def test_records_without_proper_give_map_node_bit_for_bit(twin, what):
    """the property that ties the call to rj_map_node: its definition (tests/node_ref.py) on the same records, every array
    and the eight shared counts, from the twin and from the definition here"""
    m, records, _ = records_of(*what)
    records = without_proper(records)
    for drop_last in (False, True) if what[0] in ("wall", "closed-soup") else (False,):
        want = NR.node_ref(m[0], m[1], records, drop_last)
        for got in (twin_snap(twin, m, records, DROP_LAST if drop_last else 0)[1:], SR.snap_ref(m[0], m[1], records, drop_last)):
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
            assert {k: got[3][k] for k in NR.COUNTS} == want[3] and got[3]["n_exact"] == got[3]["n_at_end"] == got[3]["n_stale"] == 0


# ---- the wide arithmetic ---------------------------------------------------------------------------------------------------
def wide_pairs(n=2000, seed=3):
    """crossing pairs with coordinates near +-2^46: both diagonals of a box as wide as the range, every end moved by up to
    64 units, in all four direction combinations; every fourth pair is built around a centre so that the crossing point
    is an exact half in both coordinates"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        j = lambda: rng.randrange(64)  # noqa: E731
        if k % 4 == 3:
            cx, cy = rng.randrange(-64, 64), rng.randrange(-64, 64)  # the centre (cx + 1/2, cy + 1/2)
            a, c = (-L + j(), -L + j()), (-L + j(), L - 1 - j())
            e, f = [a, (2 * cx + 1 - a[0], 2 * cy + 1 - a[1])], [c, (2 * cx + 1 - c[0], 2 * cy + 1 - c[1])]
        else:
            e, f = [(-L + j(), -L + j()), (L - 1 - j(), L - 1 - j())], [(-L + j(), L - 1 - j()), (L - 1 - j(), -L + j())]
        if k & 1:
            e.reverse()
        if k & 2 and k % 4 != 3 or k % 8 == 7:
            f.reverse()
        out.append((e, f))
    return out


def test_the_wide_arithmetic_against_python_integers(twin):
    halves = negative = 0
    for e, f in wide_pairs():
        want = SR.crossing_point(e[0], e[1], f[0], f[1])
        assert want is not None
        ea, fa, out = np.array(e, np.int64).ravel(), np.array(f, np.int64).ravel(), np.zeros(4, np.int64)
        twin.snap_point(ea.ctypes.data, fa.ctypes.data, out.ctypes.data)
        assert out.tolist() == [0, int(want[1]), want[0][0], want[0][1]], (e, f)
        r, s = (e[1][0] - e[0][0], e[1][1] - e[0][1]), (f[1][0] - f[0][0], f[1][1] - f[0][1])
        den, tn = r[0] * s[1] - r[1] * s[0], (f[0][0] - e[0][0]) * s[1] - (f[0][1] - e[0][1]) * s[0]
        halves += (2 * r[0] * tn) % den == 0 and (r[0] * tn) % den != 0
        negative += r[0] < 0
    assert halves >= 400 and negative >= 900  # the cases are what they claim to be


# ---- the properties of one round ------------------------------------------------------------------------------------------
def chains_of(xy, row):
    return [xy[b:e].tolist() for b, e in zip(row[:-1], row[1:])]


@pytest.mark.parametrize("what", [("hand", n) for n in sorted(SC.HAND)] + GRAIN + SOUPS[::3] + SEGMENTS[::2], ids=str)
def test_properties(twin, what):
    """the output has the same chains: the input's points in order with points inserted between them; every inserted point
    lies in the closed box of its edge -- and, for a proper crossing's point, of the other edge too --; no two consecutive
    equal points are inserted and none equals an end of its edge; a map without records comes back as a copy"""
    m, records, _ = records_of(*what)
    rc, xy, row, origin, counts = twin_snap(twin, m, records)
    assert rc == OK and len(row) == len(m[1])
    first_point = [p for c in range(len(m[1]) - 1) for p in range(m[1][c], m[1][c + 1] - 1)]
    src = np.asarray(m[0]).reshape(-1, 2).tolist()
    k = 0  # the output edge that starts at the point looked at
    for chain, new in zip(chains_of(np.asarray(m[0]).reshape(-1, 2), m[1]), chains_of(xy, row)):
        at = 0
        for i, p in enumerate(new):
            if i + 1 == len(new) or i == 0 or origin[k] != origin[k - 1]:  # an input point: the chain's last, or the first of an input edge
                assert p == chain[at]
                at += 1
            else:
                a, b = src[first_point[origin[k]]], src[first_point[origin[k]] + 1]
                assert min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])
                assert p != new[i - 1] and p != a and p != b
            k += i + 1 < len(new)
        assert at == len(chain)
    assert k == counts["n_edges"]
    for e, f, kind in records:
        if kind == SR.PROPER:
            hit = SR.crossing_point(src[first_point[e]], src[first_point[e] + 1], src[first_point[f]], src[first_point[f] + 1])
            for g in (e, f) if hit is not None else ():
                a, b = src[first_point[g]], src[first_point[g] + 1]
                assert min(a[0], b[0]) <= hit[0][0] <= max(a[0], b[0]) and min(a[1], b[1]) <= hit[0][1] <= max(a[1], b[1])
    same(twin_snap(twin, m, []), SR.snap_ref(m[0], m[1], []))
    rc, xy0, row0, _, c0 = twin_snap(twin, m, [])
    assert np.array_equal(xy0, np.asarray(m[0]).reshape(-1, 2)) and np.array_equal(row0, m[1]) and c0["n_cuts"] == 0


def test_a_clean_map_gives_a_copy(twin):
    for what in (("soup", 0), ("segments", 0), ("hand", "bow-tie")):
        xy, row, _, clean, remaining = rounds_of(*what)
        assert clean
        records, _ = CR.map_crossings_ref(xy, row)
        rc, xy2, row2, _, c = twin_snap(twin, (xy, row), records)
        assert rc == OK and np.array_equal(xy2, xy) and np.array_equal(row2, row) and c["n_cuts"] == 0 and c["n_equal"] == remaining["n_equal"]


# ---- the rounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", SOUPS + SEGMENTS, ids=str)
def test_rounds_are_clean_within_eight(what):
    xy, row, rounds, clean, remaining = rounds_of(*what)
    assert clean and len(rounds) <= 8 and SR.dirty(remaining) == 0
    assert all(SR.dirty(r["crossings"]) > 0 for r in rounds)
    records, counts = CR.map_crossings_ref(xy, row)
    assert counts == remaining and all(k == SR.EQUAL for _, _, k in records)


@pytest.mark.parametrize("what", [("soup", 3), ("closed-soup", 5), ("segments", 1)], ids=str)
def test_the_twin_follows_the_rounds(twin, what):
    """round by round: the twin on the definition's records of the round's input gives the round's output"""
    m, _, _ = records_of(*what)
    xy, row = np.asarray(m[0]).reshape(-1, 2), m[1]
    want = rounds_of(*what)
    for r in want[2]:
        records, counts = CR.map_crossings_ref(xy, row)
        assert counts == r["crossings"]
        rc, xy, row, _, c = twin_snap(twin, (xy, row), records)
        assert rc == OK and c == r["snap"]
    assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1])


def test_a_fan_is_not_clean_after_two_rounds():
    xy, row, rounds, clean, remaining = rounds_of("fan", 0, 2)
    assert not clean and len(rounds) == 2 and SR.dirty(remaining) > 0
    _, counts = CR.map_crossings_ref(xy, row)
    assert counts == remaining
    full = rounds_of("fan", 0, 20)
    assert full[3] and 8 < len(full[2]) <= 20  # (clean in the end, slowly: the default cap of 8 reports it as not clean too)
    assert not rounds_of("fan", 0)[3] and len(rounds_of("fan", 0)[2]) == 8
    assert rounds_of("fan", 0, 0)[2] == [] and np.array_equal(rounds_of("fan", 0, 0)[0], SC.fan()[0])


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_one_short(twin):
    for what, flags in ((("segments", 2), 0), (("closed-soup", 1), 0), (("closed-soup", 1), DROP_LAST)):
        m, records, _ = records_of(*what)
        want = snapped(*what, bool(flags))
        n = want[3]["n_points"]
        assert want[3]["n_cuts"] > 0
        rc, _, _, _, c = twin_snap(twin, m, records, flags, capacity=0)
        assert rc == OVERFLOW and c == want[3]
        same(twin_snap(twin, m, records, flags, capacity=n), want)
        rc, _, _, _, c = twin_snap(twin, m, records, flags, capacity=n - 1)  # (twin_snap checks that nothing was written)
        assert rc == OVERFLOW and c == want[3]
        same(twin_snap(twin, m, records, flags, capacity=n + 5), want)


def test_no_chains_and_no_records(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32))
    rc, xy, row, org, c = twin_snap(twin, empty, [])
    assert rc == OK and len(xy) == 0 and row.tolist() == [0] and c == dict.fromkeys(SR.COUNTS, 0)
    assert twin_snap(twin, empty, [(0, 1, 1)])[0] == INVALID
    m, _, _ = records_of("hand", "x")
    same(twin_snap(twin, m, []), SR.snap_ref(m[0], m[1], []))
    points = NC.chain_arrays([[(1, 1)], [(2, 2)]])
    same(twin_snap(twin, points, []), SR.snap_ref(points[0], points[1], []))


def refused(twin, m, records, flags=0):
    """the definition refuses it (it knows no flag but the one), and so does the twin"""
    if flags < 2:
        with pytest.raises(SR.Invalid):
            SR.snap_ref(m[0], m[1], records, bool(flags))
    return twin_snap(twin, m, records, flags)[0] == INVALID


def test_bad_input(twin):
    """every RJ_E_INVALID of rj_map_node, on its test's map with a proper crossing's kind where a kind is free"""
    m, records, _ = records_of("node-hand", "two-cuts-reversed")
    xy, row = m
    assert records == [(0, 1, 2), (0, 2, 2)] and twin_snap(twin, m, records)[0] == OK
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        assert refused(twin, (xy, np.array(bad_row, np.uint32)), [])
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert refused(twin, (bad, row), records)
    assert refused(twin, m, records, flags=2) and refused(twin, m, records, flags=3)
    for bad_records in ([(1, 0, 1)], [(1, 1, 1)], [(0, 3, 1)], [(0, 1, 0)], [(0, 1, 5)],  # eid order, eid range, kind
                        [(0, 2, 1), (0, 1, 1)], [(0, 1, 1), (0, 1, 1)], [(1, 2, 1), (0, 2, 2)]):  # not strictly ascending
        assert refused(twin, m, bad_records)
    zero = NC.chain_arrays(NC.HAND["zero-edge-and-one-point-chain"][0])
    assert twin_snap(twin, zero, [(1, 2, 1)])[0] == OK
    for bad_records in ([(0, 2, 1)], [(1, 3, 1)]):  # a zero-length edge named first, second
        assert refused(twin, zero, bad_records)
    # RJ_SNAP_DROP_LAST: an open chain, a one-point chain
    assert refused(twin, m, records, flags=DROP_LAST)
    closed = NC.chain_arrays([[(0, 0), (4, 0), (0, 4), (0, 0)], [(2, 2)]])
    assert refused(twin, closed, [], flags=DROP_LAST) and twin_snap(twin, closed, [])[0] == OK


# ---- the header's mutations ----------------------------------------------------------------------------------------------
MUTATIONS = {
    "halves-down": [("return d >= 0 ? Q + (2 * R >= den ? 1 : 0)", "return d >= 0 ? Q + (2 * R > den ? 1 : 0)"),
                    (": -Q - (2 * R > den ? 1 : 0);", ": -Q - (2 * R >= den ? 1 : 0);")],
    "no-minor-key": [("((major & 0x7FFFull) << 47) | minor, qx, qy}", "((major & 0x7FFFull) << 47), qx, qy}")],
    "q-from-f": [("p.qx = E.ax + rounded_part(rx,", "p.qx = F.ax + rounded_part(rx,"), ("p.qy = E.ay + rounded_part(ry,", "p.qy = F.ay + rounded_part(ry,")],
    "no-end-drop": [("const bool end_e = crossings::is_end(E, p.qx, p.qy), end_f = crossings::is_end(F, p.qx, p.qy);", "const bool end_e = false, end_f = false;")],
    "no-stale-test": [("if (den == 0 || tn <= 0 || tn >= den || un <= 0 || un >= den) return p;", "if (den == 0) return p;")],
}
CAUGHT_BY = {"halves-down": ("half", "half-reversed", "half-one-reversed", "negative-half", "shallow-ties", "steep"), "no-minor-key": ("minor-tie", "minor-tie-reversed"),
             "q-from-f": ("x", "half", "mixed", "extreme"), "no-end-drop": ("at-end",), "no-stale-test": ("stale-t", "stale-apart", "wrong-kinds")}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_header_mutations_are_caught(name, tmp_path):
    """the twin built from a scratch copy of rj_snap.h with one rule broken differs from the definition on the hand cases
    named for it (and the unbroken header does not: test_twin_hand_cases)"""
    with open(os.path.join(CSRC, "rj_snap.h")) as f:
        text = f.read()
    for old, new in MUTATIONS[name]:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    with open(tmp_path / "rj_snap.h", "w") as f:
        f.write(text)
    lib = twin_lib(str(tmp_path), "_mutant_" + name.replace("-", "_"))
    try:
        for case in CAUGHT_BY[name]:
            m, records, _ = records_of("hand", case)
            rc, xy, row, _, c = twin_snap(lib, m, records)
            want = snapped("hand", case)
            assert rc != OK or not (np.array_equal(xy, want[0]) and np.array_equal(row, want[1]) and c == want[3]), case
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
