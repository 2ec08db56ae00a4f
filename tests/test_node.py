"""Noding a chain map on the CPU: the plain-Python definition (tests/node_ref.py) on the hand-built maps of
tests/node_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/node_twin.cc compiling rayjoin_amd/csrc/rj_node.h) against that definition, every array and every
count, with and without RJ_NODE_DROP_LAST: the hand cases, the brick walls, 40 random soups and their closed forms, one
long edge with 300 T-junctions in scrambled order; the properties that make noding worth calling (no touch and no
overlap is left, no proper crossing is added, a second call inserts nothing, no records: a copy); the contract of the
call.  The GPU side is tests/test_gpu_node.py.

Mutations of a scratch copy of rj_node.h (RJ_NODE_HEADER_DIR points the twin's build at it), and the tests here that
fail under each (155 tests at the time):
  the is_end test dropped from inside() (an edge's own end point becomes a cut of it): 35 -- "inside-shared-end" in the
      twin and in the properties, 33 soups
  the in_box test dropped from inside() (collinear vertices beyond an edge's end cut it): 79 -- "inside-shared-end",
      "one-inside-another", "partial-overlap" and its opposite form, "three-squares", the two walls with cuts, each in
      the twin and in the properties, 35 soups and 30 soups' properties, the sizing test, the record that does not fit
  offset_on by x alone (no y on a vertical edge): 52 -- "vertical", "vertical-downward", "rim-vertical" in the twin and
      in the properties, 24 soups and 22 soups' properties (the walls' vertical borders carry one cut each: they pass)
  offset_on without the absolute value: 65 -- "right-to-left", "skew-right-to-left", "vertical-downward", "rim-vertical",
      the long edge, each in the twin and in the properties, 29 soups and 26 soups' properties
  cut_head true for every cut (duplicates kept): 46 -- "three-chains-one-vertex", "three-squares", the two walls with
      cuts, the long edge (every seventh foot is there twice), the sizing test, 40 soups
  cut_before without the distance: 76 -- "two-cuts-reversed", "one-inside-another", "right-to-left",
      "skew-right-to-left", "vertical", "rim", "rim-vertical", the long edge, each in the twin and in the properties, 32
      soups and 28 soups' properties"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_ref as CR  # noqa: E402
import node_cases as NC  # noqa: E402
import node_ref as NR  # noqa: E402
import ringmap_ref as RM  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "node_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HDR_DIR = os.environ.get("RJ_NODE_HEADER_DIR", CSRC)  # (a scratch copy: the mutation runs)
HDRS = [os.path.join(HDR_DIR, "rj_node.h"), os.path.join(CSRC, "rj_crossings.h"), os.path.join(CSRC, "rj_rings.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "libnode_twin%s.so" % ("" if "RJ_NODE_HEADER_DIR" not in os.environ else "_mutant"))
CANARY = 0x5B5B5B5B5B5B5B5B
RECORD = np.dtype([("eid", np.uint32, 2), ("kind", np.uint32), ("_pad", np.uint32)])
OK, INVALID, OVERFLOW = 0, 1, 3
DROP_LAST = 1
LONG_EDGE = 300


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", HDR_DIR, "-I", CSRC, "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.node_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def record_array(records):
    out = np.zeros(len(records), RECORD)
    for k, (e, f, kind) in enumerate(records):
        out[k] = ((e, f), kind, 0)
    return out


def twin_node(L, m, records, flags=0, capacity=None, origin=True):
    """-> (status, out_xy, out_row, origin, counts).  capacity None: the sizing call, then the exact capacity.  Behind the
    capacity lie canaries that must survive; an overflow or a refusal must leave every output as it was."""
    xy, row = np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32)
    rec = records if isinstance(records, np.ndarray) else record_array(records)
    nc = max(0, len(row) - 1)
    counts = np.zeros(8, np.uint64)

    def call(cap, out_xy, out_row, org):
        return L.node_twin(xy.ctypes.data, len(xy), row.ctypes.data, nc, rec.ctypes.data if len(rec) else None, len(rec), flags, cap,
                           out_xy.ctypes.data if out_xy is not None else None, out_row.ctypes.data if out_row is not None else None,
                           org.ctypes.data if org is not None else None, counts.ctypes.data)

    def named():
        return dict(zip(NR.COUNTS, (int(v) for v in counts)))
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
    """(status, out_xy, out_row, origin, counts) of the twin against node_ref's (out_xy, out_row, origin, counts)"""
    rc, xy, row, org, c = got
    assert rc == OK and c == want[3]
    assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1]) and (org is None or np.array_equal(org, want[2]))


@functools.lru_cache(maxsize=None)
def records_of(kind, key):
    """-> (the map, its crossings by definition as tuples, their counts): computed once, shared, never changed"""
    m = {"hand": lambda: NC.chain_arrays(NC.HAND[key][0]), "wall": lambda: NC.wall_map(key), "soup": lambda: NC.soup(key),
         "closed-soup": lambda: NC.closed_soup(key), "long": lambda: NC.long_edge(key)[0]}[kind]()
    records, counts = CR.map_crossings_ref(*m)
    return m, records, counts


@functools.lru_cache(maxsize=None)
def noded(kind, key, drop_last=False):
    m, records, _ = records_of(kind, key)
    return NR.node_ref(m[0], m[1], records, drop_last)


def hand_want(name):
    chains, want_chains, (n_cuts, n_cut_edges, n_max_cuts, n_used, n_proper, n_equal) = NC.HAND[name]
    xy, row = NC.chain_arrays(want_chains)
    counts = dict(n_points=len(xy), n_edges=len(xy) - len(chains), n_cuts=n_cuts, n_cut_edges=n_cut_edges, n_max_cuts=n_max_cuts, n_used=n_used,
                  n_proper=n_proper, n_equal=n_equal)
    return xy, row, counts


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_definition_gives_the_written_answer(name):
    xy, row, counts = hand_want(name)
    got = noded("hand", name)
    assert np.array_equal(got[0], xy) and np.array_equal(got[1], row) and got[3] == counts
    assert len(got[2]) == counts["n_edges"] and (np.diff(got[2].astype(np.int64)) >= 0).all()


def test_definition_on_the_brick_walls():
    """the written numbers of the 5 x 4 wall: 54 touches, 27 overlaps and 16 equal edges among the rings as given, 30
    cuts; its chain map has 57 crossings before and none after, 57 chains and 67 edges"""
    _, records, counts = records_of("wall", (5, 4, 10, 6, 5))
    assert (counts["n_touch"], counts["n_overlap"], counts["n_equal"], counts["n_proper"]) == (54, 27, 16, 0)
    for key, cuts in NC.WALLS.items():
        assert noded("wall", key)[3]["n_cuts"] == noded("wall", key, True)[3]["n_cuts"] == cuts
    ring_row, ring_xy, ring_face = NC.brick_rings(5, 4, 10, 6, 5)
    before = RM.rings_map_ref(ring_row, ring_xy, ring_face)
    assert CR.map_crossings_ref(before["xy"], before["row_index"])[1]["n_found"] == 57
    xy, row, _, c = noded("wall", (5, 4, 10, 6, 5), True)
    after = RM.rings_map_ref(row, xy, ring_face)
    assert (after["counts"]["n_chains"], after["counts"]["n_edges"], after["counts"]["n_conflicts"]) == (57, 67, 0)
    assert CR.map_crossings_ref(after["xy"], after["row_index"])[1]["n_found"] == 0


def test_soups_are_worth_their_time():
    """no soup is empty of work (423 cuts in all), and one edge can carry several cuts"""
    cuts = [noded("soup", s)[3] for s in NC.SOUP_SEEDS]
    assert all(c["n_cuts"] > 0 for c in cuts) and max(c["n_max_cuts"] for c in cuts) >= 3
    assert sum(c["n_proper"] for c in cuts) > 0 and sum(c["n_equal"] for c in cuts) > 0
    assert sum(c["n_cuts"] for c in cuts) == 423


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_twin_hand_cases(twin, name):
    m, records, _ = records_of("hand", name)
    same(twin_node(twin, m, records), noded("hand", name))
    same(twin_node(twin, m, records, origin=False), noded("hand", name))
    if name in NC.CLOSED:
        same(twin_node(twin, m, records, DROP_LAST), noded("hand", name, True))


@pytest.mark.parametrize("key", sorted(NC.WALLS))
def test_twin_brick_walls(twin, key):
    m, records, _ = records_of("wall", key)
    same(twin_node(twin, m, records), noded("wall", key))
    same(twin_node(twin, m, records, DROP_LAST), noded("wall", key, True))


@pytest.mark.parametrize("seed", NC.SOUP_SEEDS)
def test_twin_soups(twin, seed):
    m, records, _ = records_of("soup", seed)
    same(twin_node(twin, m, records), noded("soup", seed))
    m, records, _ = records_of("closed-soup", seed)
    same(twin_node(twin, m, records), noded("closed-soup", seed))
    same(twin_node(twin, m, records, DROP_LAST), noded("closed-soup", seed, True))


def test_twin_long_edge(twin):
    m, records, _ = records_of("long", LONG_EDGE)
    want = noded("long", LONG_EDGE)
    assert [tuple(p) for p in want[0][:LONG_EDGE + 2].tolist()] == NC.long_edge(LONG_EDGE)[1]
    assert want[3]["n_cuts"] == want[3]["n_max_cuts"] == LONG_EDGE and want[3]["n_cut_edges"] == 1 and want[3]["n_used"] == LONG_EDGE + LONG_EDGE // 7
    same(twin_node(twin, m, records), want)


# ---- the properties ------------------------------------------------------------------------------------------------------
def properties(node, m, records, counts):
    """node(map, records, flags) -> (xy, row); for N = node(M, crossings(M)): crossings(N) has no touch and no overlap and
    no more proper crossings than M; node(N, crossings(N)) inserts nothing and equals N; with no records N' = M"""
    xy, row = node(m, records, 0)
    again, again_counts = CR.map_crossings_ref(xy, row)
    assert again_counts["n_touch"] == 0 and again_counts["n_overlap"] == 0 and again_counts["n_proper"] <= counts["n_proper"]
    xy2, row2 = node((xy, row), again, 0)
    assert np.array_equal(xy2, xy) and np.array_equal(row2, row)
    xy0, row0 = node(m, [], 0)
    assert np.array_equal(xy0, np.asarray(m[0]).reshape(-1, 2)) and np.array_equal(row0, m[1])


@pytest.mark.parametrize("what", [("hand", n) for n in sorted(NC.HAND)] + [("wall", k) for k in sorted(NC.WALLS)] +
                         [("soup", s) for s in NC.SOUP_SEEDS] + [("long", LONG_EDGE)], ids=str)
def test_properties(twin, what):
    m, records, counts = records_of(*what)

    def node(m, records, flags):
        rc, xy, row, _, _ = twin_node(twin, m, records, flags)
        assert rc == OK
        return xy, row
    properties(node, m, records, counts)
    properties(lambda m, r, f: NR.node_ref(m[0], m[1], r, bool(f))[:2], m, records, counts)


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_one_short(twin):
    m, records, _ = records_of("wall", (4, 3, 9, 4, 2))
    for flags in (0, DROP_LAST):
        want = noded("wall", (4, 3, 9, 4, 2), bool(flags))
        n = want[3]["n_points"]
        rc, _, _, _, c = twin_node(twin, m, records, flags, capacity=0)
        assert rc == OVERFLOW and c == want[3]
        same(twin_node(twin, m, records, flags, capacity=n), want)
        rc, _, _, _, c = twin_node(twin, m, records, flags, capacity=n - 1)  # (twin_node checks that nothing was written)
        assert rc == OVERFLOW and c == want[3]
        same(twin_node(twin, m, records, flags, capacity=n + 5), want)


def test_no_chains_and_no_records(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32))
    rc, xy, row, org, c = twin_node(twin, empty, [])
    assert rc == OK and len(xy) == 0 and row.tolist() == [0] and c == dict.fromkeys(NR.COUNTS, 0)
    assert twin_node(twin, empty, [(0, 1, 2)])[0] == INVALID
    m, _, _ = records_of("hand", "t")
    same(twin_node(twin, m, []), NR.node_ref(m[0], m[1], []))
    points = NC.chain_arrays([[(1, 1)], [(2, 2)]])
    same(twin_node(twin, points, []), NR.node_ref(points[0], points[1], []))


def refused(twin, m, records, flags=0):
    """the definition refuses it (it knows no flag but the one), and so does the twin"""
    if flags < 2:
        with pytest.raises(NR.Invalid):
            NR.node_ref(m[0], m[1], records, bool(flags))
    return twin_node(twin, m, records, flags)[0] == INVALID


def test_bad_input(twin):
    m, records, _ = records_of("hand", "two-cuts-reversed")
    xy, row = m
    assert records == [(0, 1, 2), (0, 2, 2)] and twin_node(twin, m, records)[0] == OK
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        assert refused(twin, (xy, np.array(bad_row, np.uint32)), [])
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert refused(twin, (bad, row), records)
    assert refused(twin, m, records, flags=2) and refused(twin, m, records, flags=3)
    for bad_records in ([(1, 0, 2)], [(1, 1, 2)], [(0, 3, 2)], [(0, 1, 0)], [(0, 1, 5)],  # eid order, eid range, kind
                        [(0, 2, 2), (0, 1, 2)], [(0, 1, 2), (0, 1, 2)], [(1, 2, 1), (0, 2, 2)]):  # not strictly ascending
        assert refused(twin, m, bad_records)
    zero = NC.chain_arrays(NC.HAND["zero-edge-and-one-point-chain"][0])
    assert twin_node(twin, zero, [(1, 2, 2)])[0] == OK
    for bad_records in ([(0, 2, 2)], [(1, 3, 2)]):  # a zero-length edge named first, second
        assert refused(twin, zero, bad_records)
    # RJ_NODE_DROP_LAST: an open chain, a one-point chain
    assert refused(twin, m, records, flags=DROP_LAST)
    closed = NC.chain_arrays([[(0, 0), (4, 0), (0, 4), (0, 0)], [(2, 2)]])
    assert refused(twin, closed, [], flags=DROP_LAST) and twin_node(twin, closed, [])[0] == OK


def test_a_record_that_does_not_fit_the_geometry_cuts_nothing(twin):
    """records of a cutting kind over edges that do not touch: counted in n_used, no point leaves its edge"""
    m, _, _ = records_of("hand", "proper-only")
    rc, xy, row, _, c = twin_node(twin, m, [(0, 1, 2)])
    assert rc == OK and np.array_equal(xy, m[0]) and c["n_used"] == 1 and c["n_cuts"] == 0
    m = NC.chain_arrays([[(0, 0), (4, 0)], [(6, 0), (9, 0)], [(2, 1), (2, 5)]])  # collinear apart; a stem that stops short
    want = NR.node_ref(m[0], m[1], [(0, 1, 3), (0, 2, 2)])
    same(twin_node(twin, m, [(0, 1, 3), (0, 2, 2)]), want)
    assert want[3]["n_cuts"] == 0 and want[3]["n_used"] == 2


# ---- the host helper -------------------------------------------------------------------------------------------------------
def test_closed_chains_of_rings():
    from rayjoin_amd import maps
    ring_row, ring_xy, _ = NC.brick_rings(3, 2, 4, 4, 2)
    row, xy = maps.closed_chains_of_rings(ring_row, ring_xy)
    want_xy, want_row = NC.closed_chains(ring_row, ring_xy)
    assert row.dtype == np.uint32 and xy.dtype == np.int64 and np.array_equal(row, want_row) and np.array_equal(xy, want_xy)
    row, xy = maps.closed_chains_of_rings([0, 1, 3], [(5, 5), (1, 2), (3, 4)])  # a ring of one point, a ring of two
    assert row.tolist() == [0, 2, 5] and xy.tolist() == [[5, 5], [5, 5], [1, 2], [3, 4], [1, 2]]
    row, xy = maps.closed_chains_of_rings(np.zeros(1, np.uint32), np.zeros((0, 2), np.int64))
    assert row.tolist() == [0] and xy.shape == (0, 2)
    for bad in ([0, 2, 2, 3], [0, 0, 3]):
        with pytest.raises(ValueError, match="empty"):
            maps.closed_chains_of_rings(bad, [(0, 0), (1, 1), (2, 2)])
    with pytest.raises(ValueError):
        maps.closed_chains_of_rings([0, 2], [(0, 0), (1, 1), (2, 2)])
