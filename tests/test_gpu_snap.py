"""Cutting a chain map at its rounded proper crossings on the device (rj_map_snap, ops.map_snap, ops.map_snap_rounds,
ops.snap_rings, the Snap methods) against the plain-Python definition (tests/snap_ref.py), every array and every count,
with and without RJ_SNAP_DROP_LAST and with edge_origin: the hand maps of tests/snap_cases.py, 63 / 64 / 65 records, stars
of 65 and 129 edges through one half-integer point (more equal cuts on one point than a wave has lanes), one long edge
with 300 crossings and 300 T-junctions, 10 soups and 5 maps of random segments, at the exact capacity and one short;
the records both from the definition of the crossings (uploaded) and from rj_map_crossings itself (kept on the device).
The rounds driver against snap_rounds_ref round by round, on 5 soups and on the fan that is not clean after two rounds.
A call with touches and overlaps only against ops.map_node.  Then what it is for: two overlapping squares and three
overlapping triangles through snap_rings, rings_map and Faces().  The refusals, the stage times and the handle's state.
The CPU side is tests/test_snap.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_ref as CR  # noqa: E402
import faces_ref as FR  # noqa: E402
import node_cases as NC  # noqa: E402
import ringmap_ref as RM  # noqa: E402
import snap_cases as SC  # noqa: E402
import snap_ref as SR  # noqa: E402
from test_snap import GRAIN, record_array, records_of, rounds_of, snapped, without_proper  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


class DeviceMap:
    """a chain map (xy, row_index) in device buffers"""

    def __init__(self, h, m):
        xy, row = np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32)
        self.n_points, self.n_chains = len(xy), max(0, len(row) - 1)
        self.bufs = [h.alloc(16 * max(1, len(xy))).from_host(xy), h.alloc(4 * max(1, len(row))).from_host(row)]

    def args(self):
        return (self.bufs[0], self.n_points, self.bufs[1], self.n_chains)

    def free(self):
        for b in self.bufs:
            b.free()


def device_snap(h, m, records, drop_last=False, edge_origin=True):
    """-> (out_xy, out_row, origin, counts) through ops.map_snap; records: tuples to upload, or None: rj_map_crossings'"""
    dm = DeviceMap(h, m)
    try:
        nm = ops.map_snap(h, *dm.args(), records=None if records is None else record_array(records).astype(_capi.CROSSING_DTYPE),
                          drop_last=drop_last, edge_origin=edge_origin)
        try:
            assert nm.n_chains == dm.n_chains and nm.drop_last == drop_last
            return nm.to_host() + (nm.counts,)
        finally:
            nm.free()
    finally:
        dm.free()


def same(got, want):
    assert got[3] == want[3]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[2] is None or np.array_equal(got[2], want[2]))


def check(h, kind, key, drop_last=False, own_records=True):
    m, records, _ = records_of(kind, key)
    want = snapped(kind, key, drop_last)
    same(device_snap(h, m, records, drop_last), want)
    if own_records:
        same(device_snap(h, m, None, drop_last), want)
    return want


def exact_capacity_and_one_short(h, m, records, want, flags=0):
    """the raw call with canaries behind every array: written in full at the exact capacity, untouched one short"""
    dm = DeviceMap(h, m)
    rec = h.alloc(16 * max(1, len(records))).from_host(record_array(records))
    nc, n, ne = dm.n_chains, want[3]["n_points"], want[3]["n_edges"]
    try:
        with pytest.raises(_capi.SnapOverflow) as e:  # the sizing call
            h.map_snap(*dm.args(), rec, len(records), flags, 0, None, None)
        assert e.value.counts == want[3] and e.value.code == _capi.RJ_E_OVERFLOW
        for cap in (n, n - 1):
            bufs = [h.alloc(16 * cap + 32).from_host(np.full(4 * cap + 8, CANARY, np.uint32)),
                    h.alloc(4 * (nc + 1) + 32).from_host(np.full(nc + 9, CANARY, np.uint32)),
                    h.alloc(4 * cap + 32).from_host(np.full(cap + 8, CANARY, np.uint32))]
            try:
                if cap == n:
                    assert h.map_snap(*dm.args(), rec, len(records), flags, cap, *bufs) == want[3]
                    same((bufs[0].to_host(np.int64, 2 * n).reshape(-1, 2), bufs[1].to_host(np.uint32, nc + 1), bufs[2].to_host(np.uint32, ne), want[3]), want)
                    assert (bufs[0].to_host(np.uint32)[4 * cap:] == CANARY).all() and (bufs[1].to_host(np.uint32)[nc + 1:] == CANARY).all()
                    assert (bufs[2].to_host(np.uint32)[ne:] == CANARY).all()
                else:
                    with pytest.raises(_capi.SnapOverflow) as e:
                        h.map_snap(*dm.args(), rec, len(records), flags, cap, *bufs)
                    assert e.value.counts == want[3]
                    assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
            finally:
                for b in bufs:
                    b.free()
    finally:
        rec.free()
        dm.free()


# ---- the device against the definition and the written answers -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.HAND))
def test_hand_cases(handle, name):
    own = SC.HAND[name][3] is None  # (a case with records of its own: rj_map_crossings' would be others)
    want = check(handle, "hand", name, own_records=own)
    xy, row = SC.chain_arrays(SC.HAND[name][1])
    assert np.array_equal(want[0], xy) and np.array_equal(want[1], row) and {k: want[3][k] for k in SC.HAND[name][2]} == SC.HAND[name][2]
    if name in SC.CLOSED:
        check(handle, "hand", name, True)
    m, records, _ = records_of("hand", name)
    same(device_snap(handle, m, records, edge_origin=False), want)
    if want[3]["n_cuts"]:
        exact_capacity_and_one_short(handle, m, records, want)


@pytest.mark.parametrize("what", GRAIN, ids=str)
def test_grain(handle, what):
    """63, 64, 65 records: a wave less one lane, a full wave, a wave and one lane; the stars: 2080 and 8256 records that all
    cut at one point, 64 and 128 equal cuts per edge of which one stays; the long edge: 600 cuts on one edge from two
    kinds of records in scrambled order, 43 of them twice"""
    want = check(handle, *what)
    if what[0] == "long":
        first = SC.long_mixed(what[1])[1]
        assert [tuple(p) for p in want[0][:len(first)].tolist()] == first
    m, records, _ = records_of(*what)
    exact_capacity_and_one_short(handle, m, records, want)


@pytest.mark.parametrize("seed", range(10))
def test_soups(handle, seed):
    check(handle, "soup", seed)
    check(handle, "crossings-soup", seed)
    want = check(handle, "closed-soup", seed, True)
    m, records, _ = records_of("closed-soup", seed)
    if want[3]["n_cuts"]:
        exact_capacity_and_one_short(handle, m, records, want, _capi.RJ_SNAP_DROP_LAST)


@pytest.mark.parametrize("seed", range(5))
def test_random_segments(handle, seed):
    want = check(handle, "segments", seed)
    m, records, _ = records_of("segments", seed)
    assert want[3]["n_proper"] > 50 and want[3]["n_max_cuts"] >= 5
    exact_capacity_and_one_short(handle, m, records, want)


@pytest.mark.parametrize("what", [("node-hand", n) for n in sorted(NC.HAND)] + [("wall", k) for k in sorted(NC.WALLS)] + [("soup", s) for s in range(6)] +
                         [("node-long", 300)], ids=str)
def test_touches_and_overlaps_alone_equal_map_node(handle, what):
    """on records without a proper crossing the call is rj_map_node: both on the device, every array, the eight shared counts"""
    m, records, _ = records_of(*what)
    rec = record_array(without_proper(records)).astype(_capi.CROSSING_DTYPE)
    dm = DeviceMap(handle, m)
    try:
        for drop_last in (False, True) if what[0] == "wall" else (False,):
            sm = ops.map_snap(handle, *dm.args(), records=rec, drop_last=drop_last, edge_origin=True)
            nm = ops.map_node(handle, *dm.args(), records=rec, drop_last=drop_last, edge_origin=True)
            assert all(np.array_equal(a, b) for a, b in zip(sm.to_host(), nm.to_host()))
            assert {k: sm.counts[k] for k in _capi.NODE_COUNTS} == nm.counts and sm.counts["n_exact"] == sm.counts["n_at_end"] == sm.counts["n_stale"] == 0
            sm.free()
            nm.free()
    finally:
        dm.free()


# ---- the rounds ------------------------------------------------------------------------------------------------------------
def check_rounds(h, what, max_rounds=8, drop_last=False):
    m, _, _ = records_of(*what)
    want = rounds_of(*what, max_rounds, drop_last)
    dm = DeviceMap(h, m)
    try:
        nm = ops.map_snap_rounds(h, *dm.args(), max_rounds=max_rounds, drop_last=drop_last)
        xy, row, _ = nm.to_host()
        assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1])
        assert nm.rounds == want[2] and nm.clean == want[3] and nm.remaining == want[4] and nm.drop_last == drop_last
        nm.free()
    finally:
        dm.free()
    return want


@pytest.mark.parametrize("what", [("soup", 3), ("soup", 8), ("crossings-soup", 1), ("closed-soup", 5), ("segments", 1)], ids=str)
def test_rounds_on_soups(handle, what):
    want = check_rounds(handle, what)
    assert want[3] and 1 <= len(want[2]) <= 8
    if what[0] == "closed-soup":
        check_rounds(handle, what, drop_last=True)


def test_rounds_on_the_fan_and_on_a_clean_map(handle):
    want = check_rounds(handle, ("fan", 0), max_rounds=2)
    assert not want[3] and len(want[2]) == 2 and SR.dirty(want[4]) > 0
    assert check_rounds(handle, ("fan", 0), max_rounds=0)[2] == []
    want = check_rounds(handle, ("hand", "no-crossing"))  # nothing to cut: a copy that the caller owns
    assert want[3] and want[2] == []


# ---- what it is for ----------------------------------------------------------------------------------------------------------
def rings_of(polys, unit):
    ring_row = np.cumsum([0] + [len(r) for r in polys]).astype(np.uint32)
    return ring_row, np.array([p for r in polys for p in r], np.int64) * unit, np.arange(1, len(polys) + 1, dtype=np.int32)


@pytest.mark.parametrize("name, unit", [("two-squares", 1 << 16), ("three-triangles", 1)])
def test_overlapping_polygons_become_a_planar_map_with_faces(handle, name, unit):
    ring_row, ring_xy, ring_face = rings_of(SC.TWO_SQUARES if name == "two-squares" else SC.THREE_TRIANGLES, unit)
    # by definition: closed chains, the rounds, the chain map of the rings, its faces
    cxy, crow = NC.closed_chains(ring_row, ring_xy)
    wxy, wrow, wrounds, wclean, _ = SR.snap_rounds_ref(cxy, crow, 8, True)
    wmap = RM.rings_map_ref(wrow, wxy, ring_face)
    wfaces = FR.faces_ref(wmap["xy"], wmap["row_index"])
    assert wclean and CR.map_crossings_ref(wmap["xy"], wmap["row_index"])[1]["n_found"] == 0
    # on the device
    row_buf, xy_buf, n_points, clean, rounds = ops.snap_rings(handle, ring_row, ring_xy)
    face = handle.alloc(4 * len(ring_face)).from_host(ring_face)
    dm = None
    try:
        assert clean and rounds == wrounds and n_points == len(wxy)
        assert np.array_equal(xy_buf.to_host(np.int64, 2 * n_points).reshape(-1, 2), wxy) and np.array_equal(row_buf.to_host(np.uint32, len(wrow)), wrow)
        dm = ops.rings_map(handle, row_buf, xy_buf, n_points, face, len(ring_face))
        records, counts = dm.Crossings(handle)
        assert len(records) == 0 and counts["n_found"] == 0 and dm.counts["n_chains"] == wmap["counts"]["n_chains"]
        fm = dm.Faces(handle)
        got = sorted(FR.area2_of(fm.faces_to_host()))
        assert got == sorted(FR.area2_of(wfaces["faces"])) and fm.counts["n_faces"] == wfaces["counts"]["n_faces"]
        if name == "two-squares":
            assert dm.counts["n_chains"] == 4 and got == [8 * unit * unit, 24 * unit * unit, 24 * unit * unit] and len(rounds) == 1
        else:
            assert len(got) > 3
        fm.free()
    finally:
        if dm is not None:
            dm.free()
        for b in (row_buf, xy_buf, face):
            b.free()


# ---- the contract ------------------------------------------------------------------------------------------------------
def refused(h, m, records, flags=0, word=None):
    dm = DeviceMap(h, m)
    rec = h.alloc(16 * max(1, len(records))).from_host(record_array(records))
    n = dm.n_points + 2 * len(records)
    bufs = [h.alloc(16 * n).from_host(np.full(4 * n, CANARY, np.uint32)), h.alloc(4 * (dm.n_chains + 1)).from_host(np.full(dm.n_chains + 1, CANARY, np.uint32))]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_snap(*dm.args(), rec, len(records), flags, n, *bufs)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
    finally:
        for b in bufs + [rec]:
            b.free()
        dm.free()


def test_refusals(handle):
    m, records, _ = records_of("node-hand", "two-cuts-reversed")
    xy, row = m
    assert records == [(0, 1, 2), (0, 2, 2)]
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        refused(handle, (xy, np.array(bad_row, np.uint32)), [], word="row_index")
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        refused(handle, (bad, row), records, word="coordinate")
    refused(handle, m, records, flags=2, word="flags")
    for bad_records in ([(1, 0, 1)], [(1, 1, 1)], [(0, 3, 1)], [(0, 1, 0)], [(0, 1, 5)]):
        refused(handle, m, bad_records, word="kind in 1..4")
    for bad_records in ([(0, 2, 1), (0, 1, 1)], [(0, 1, 1), (0, 1, 1)], [(1, 2, 1), (0, 2, 2)]):
        refused(handle, m, bad_records, word="ascend")
    zero = NC.chain_arrays(NC.HAND["zero-edge-and-one-point-chain"][0])
    for bad_records in ([(0, 2, 1)], [(1, 3, 1)]):
        refused(handle, zero, bad_records, word="zero length")
    refused(handle, m, records, flags=_capi.RJ_SNAP_DROP_LAST, word="RJ_SNAP_DROP_LAST")
    refused(handle, NC.chain_arrays([[(0, 0), (4, 0), (0, 4), (0, 0)], [(2, 2)]]), [], flags=_capi.RJ_SNAP_DROP_LAST, word="RJ_SNAP_DROP_LAST")
    dm = DeviceMap(handle, m)
    with pytest.raises(_capi.RayJoinError) as e:  # points wanted, nowhere to put them
        handle.map_snap(*dm.args(), None, 0, 0, 8, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # records announced, none given
        handle.map_snap(*dm.args(), None, 2, 0, 0, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:
        handle.map_snap(*dm.args(), dm.bufs[0], 1 << 31, 0, 0, None, None)
    assert e.value.code == _capi.RJ_E_INVALID and "2^31" in str(e.value)
    dm.free()


def test_no_chains(handle):
    row = handle.alloc(4).from_host(np.array([CANARY], np.uint32))
    assert handle.map_snap(None, 0, None, 0, None, 0, 0, 0, None, row) == dict.fromkeys(_capi.SNAP_COUNTS, 0)
    assert row.to_host(np.uint32, 1)[0] == 0
    row.free()


# ---- the wrappers, the stage times, the handle ----------------------------------------------------------------------------------
def test_chain_map_snap_noded_map_snap_and_stage_times(handle):
    """DeviceChainMap.Snap on the chain map of the two squares as given (their borders cross), DeviceNodedMap.Snap on what
    map_node leaves of it; the stage times of the last call"""
    ring_row, ring_xy, ring_face = rings_of(SC.TWO_SQUARES, 1 << 10)
    bufs = [handle.alloc(4 * len(ring_row)).from_host(ring_row), handle.alloc(16 * len(ring_xy)).from_host(ring_xy), handle.alloc(4 * len(ring_face)).from_host(ring_face)]
    dm = ops.rings_map(handle, bufs[0], bufs[1], len(ring_xy), bufs[2], len(ring_face))
    try:
        host = dm.to_host()[0]
        want = SR.snap_rounds_ref(host.pts, host.row_index)
        nm = dm.Snap(handle)
        us = [handle.get_option("snap_last_us%d" % k) for k in range(6)]
        assert all(v >= 0 for v in us) and us[5] >= max(us[:5])
        xy, row, _ = nm.to_host()
        assert np.array_equal(xy, want[0]) and np.array_equal(row, want[1]) and nm.clean and nm.rounds == want[2] and len(nm.rounds) == 1
        nm.free()
        noded = dm.Node(handle)
        assert noded.counts["n_proper"] == 2
        nm = noded.Snap(handle, max_rounds=3)
        assert np.array_equal(nm.to_host()[0], want[0]) and nm.clean
        nm.free()
        noded.free()
    finally:
        dm.free()
        for b in bufs:
            b.free()


def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_output_map_snap_equals_the_definition():
    """an overlay's output map: one map_snap on the device's own records against the definition on the same records, and
    Snap()'s first round is that call"""
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        records, counts = om.Crossings(ov.h)
        host = om.to_host()[0]
        want = SR.snap_ref(host.pts, host.row_index, [(int(r["eid"][0]), int(r["eid"][1]), int(r["kind"])) for r in records])
        sm = ops.map_snap(ov.h, om.xy, om.n_points, om.row_index, om.n_chains, records=records, edge_origin=True)
        same(sm.to_host() + (sm.counts,), want)
        sm.free()
        nm = om.Snap(ov.h, max_rounds=4)
        assert nm.n_chains == om.n_chains and isinstance(nm.clean, bool) and len(nm.rounds) <= 4
        if SR.dirty(counts):
            assert nm.rounds[0] == dict(crossings=counts, snap=want[3])
            if len(nm.rounds) == 1:
                assert np.array_equal(nm.to_host()[0], want[0]) and np.array_equal(nm.to_host()[1], want[1])
        else:
            assert nm.rounds == [] and nm.clean and np.array_equal(nm.to_host()[0], host.pts)
        nm.free()
        om.free()
    finally:
        dctx.close()


def test_the_handle_stays_as_it_was():
    """an LSI query's result and rj_get_plan's text are the same before and after snapping calls on the handle"""
    import json
    dctx = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        lsi = ops.LSILBVH(dctx)
        lsi.Init(4 * (dctx.get_map(0).n_edges + dctx.get_map(1).n_edges))
        lsi.Query(1)
        before = lsi.get_pairs().copy()
        plan = json.dumps(dctx.handle.get_plan(), sort_keys=True)
        same(device_snap(dctx.handle, records_of("segments", 0)[0], None), snapped("segments", 0))
        check_rounds(dctx.handle, ("soup", 3))
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
