"""Noding a chain map on the device (rj_map_node, ops.map_node, ops.node_rings, DeviceChainMap.Node, DeviceOutputMap.Node)
against the plain-Python definition (tests/node_ref.py), every array and every count, with and without
RJ_NODE_DROP_LAST and with edge_origin: the hand maps and the brick walls of tests/node_cases.py, 10 random soups and
their closed forms, one long edge with 5 000 T-junctions in scrambled order; the records both from the definition of
the crossings (uploaded) and from rj_map_crossings itself (kept on the device).  Then what noding is for: the rings of
a brick wall and of three squares that miss their neighbours' corners, noded, give a chain map without crossings and
conflicts, whose polygons are the input rings with their exact areas -- and the same rings as given do not.  The
properties (no touch and no overlap left, no proper crossing added, a second call inserts nothing, no records: a
copy), the contract on the device (sizing call, exact capacity, one short with canaries, every refusal), the wrappers,
the stage times and the handle's state.  The CPU side is tests/test_node.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_ref as CR  # noqa: E402
import node_cases as NC  # noqa: E402
import node_ref as NR  # noqa: E402
from test_node import noded, record_array, records_of  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A
LONG_EDGE = 5000
BIG_WALL = (5, 4, 10, 6, 5)


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


def device_node(h, m, records, drop_last=False, edge_origin=True):
    """-> (out_xy, out_row, origin, counts) through ops.map_node; records: tuples to upload, or None: rj_map_crossings'"""
    dm = DeviceMap(h, m)
    try:
        nm = ops.map_node(h, *dm.args(), records=None if records is None else record_array(records).astype(_capi.CROSSING_DTYPE),
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


def check(h, kind, key, drop_last=False):
    m, records, _ = records_of(kind, key)
    want = noded(kind, key, drop_last)
    same(device_node(h, m, records, drop_last), want)
    same(device_node(h, m, None, drop_last), want)
    return want


# ---- the device against the definition and the written answers -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_hand_cases(handle, name):
    want = check(handle, "hand", name)
    xy, row = NC.chain_arrays(NC.HAND[name][1])
    assert np.array_equal(want[0], xy) and np.array_equal(want[1], row)
    if name in NC.CLOSED:
        check(handle, "hand", name, True)
    m, records, _ = records_of("hand", name)
    same(device_node(handle, m, records, edge_origin=False), want)


@pytest.mark.parametrize("key", sorted(NC.WALLS))
def test_brick_walls(handle, key):
    assert check(handle, "wall", key)[3]["n_cuts"] == NC.WALLS[key]
    assert check(handle, "wall", key, True)[3]["n_cuts"] == NC.WALLS[key]


@pytest.mark.parametrize("seed", range(10))
def test_soups(handle, seed):
    check(handle, "soup", seed)
    check(handle, "closed-soup", seed)
    check(handle, "closed-soup", seed, True)


def test_long_edge(handle):
    """5 000 cuts on one edge, arriving in scrambled order, every seventh twice: as many threads as cuts, no loop over them"""
    want = check(handle, "long", LONG_EDGE)
    assert [tuple(p) for p in want[0][:LONG_EDGE + 2].tolist()] == NC.long_edge(LONG_EDGE)[1]
    assert want[3]["n_cuts"] == want[3]["n_max_cuts"] == LONG_EDGE and want[3]["n_cut_edges"] == 1


# ---- the properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [("wall", BIG_WALL), ("hand", "proper-at-a-vertex"), ("soup", 0), ("soup", 1), ("soup", 2), ("long", 300)], ids=str)
def test_properties(handle, what):
    """all on the device: N = node(M, crossings(M)); crossings(N) has no touch, no overlap and no more proper crossings;
    node(N, crossings(N)) inserts nothing and equals N; node(M, no records) equals M"""
    m, _, before = records_of(*what)
    dm = DeviceMap(handle, m)
    nm = ops.map_node(handle, *dm.args())
    try:
        records, after = ops.map_crossings(handle, nm.xy, nm.n_points, nm.row_index, nm.n_chains)
        assert after["n_touch"] == 0 and after["n_overlap"] == 0 and after["n_proper"] <= before["n_proper"]
        again = ops.map_node(handle, nm.xy, nm.n_points, nm.row_index, nm.n_chains, records=records)
        assert again.counts["n_cuts"] == 0 and again.n_points == nm.n_points
        assert all(np.array_equal(a, b) for a, b in zip(again.to_host()[:2], nm.to_host()[:2]))
        again.free()
        copy = ops.map_node(handle, *dm.args(), records=np.zeros(0, _capi.CROSSING_DTYPE), edge_origin=True)
        xy, row, origin = copy.to_host()
        assert np.array_equal(xy, m[0]) and np.array_equal(row, m[1]) and np.array_equal(origin, np.arange(len(m[0]) - (len(m[1]) - 1)))
        assert copy.counts == dict(NR.node_ref(m[0], m[1], [])[3])
        copy.free()
    finally:
        nm.free()
        dm.free()


# ---- what noding is for ----------------------------------------------------------------------------------------------------
def three_squares(unit=1 << 20):
    """two squares side by side and a third on top, each missing its neighbours' corner vertices -> (ring_row, ring_xy, ring_face)"""
    sq = lambda x, y: [(x, y), (x + 4, y), (x + 4, y + 4), (x, y + 4)]  # noqa: E731
    return np.array([0, 4, 8, 12], np.uint32), np.array(sq(0, 0) + sq(4, 0) + sq(2, 4), np.int64) * unit, np.array([1, 2, 3], np.int32)


def area2_of(ring_row, ring_xy):
    out = []
    for b, e in zip(ring_row[:-1], ring_row[1:]):
        p = [(int(x), int(y)) for x, y in ring_xy[b:e].tolist()]
        out.append(sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(p, p[1:] + p[:1])))
    return out


def chain_map_of(h, ring_row_buf, ring_xy_buf, n_points, ring_face):
    face = h.alloc(4 * len(ring_face)).from_host(ring_face)
    try:
        return ops.rings_map(h, ring_row_buf, ring_xy_buf, n_points, face, len(ring_face))
    finally:
        face.free()


@pytest.mark.parametrize("name", ["brick-wall", "three-squares"])
def test_noded_rings_give_a_planar_map_with_the_input_polygons(handle, name):
    ring_row, ring_xy, ring_face = NC.brick_rings(*BIG_WALL, unit=1 << 16) if name == "brick-wall" else three_squares()
    # as given: the chain map has crossings
    bufs = [handle.alloc(4 * len(ring_row)).from_host(ring_row), handle.alloc(16 * len(ring_xy)).from_host(ring_xy)]
    raw = chain_map_of(handle, bufs[0], bufs[1], len(ring_xy), ring_face)
    _, counts = raw.Crossings(handle)
    assert counts["n_found"] == (57 if name == "brick-wall" else 5) and counts["n_proper"] == 0
    raw.free()
    for b in bufs:
        b.free()
    # noded: none, and every input ring is a polygon again
    row_buf, xy_buf, n_points, node_counts = ops.node_rings(handle, ring_row, ring_xy)
    assert node_counts["n_cuts"] == (30 if name == "brick-wall" else 3) and node_counts["n_proper"] == 0 and n_points == len(ring_xy) + node_counts["n_cuts"]
    dm = chain_map_of(handle, row_buf, xy_buf, n_points, ring_face)
    try:
        records, counts = dm.Crossings(handle)
        assert len(records) == 0 and counts["n_found"] == 0 and dm.counts["n_conflicts"] == 0
        if name == "brick-wall":
            assert (dm.counts["n_chains"], dm.counts["n_edges"]) == (57, 67)
        rings = dm.Rings(handle)
        polys = rings.Polygons(handle)
        got = sorted((int(f), a2, len(holes)) for f, a2, _, holes in polys.polygons(rings))
        assert got == [(int(f), a2, 0) for f, a2 in zip(ring_face, area2_of(ring_row, ring_xy))]
        polys.free()
        rings.free()
    finally:
        dm.free()
        row_buf.free()
        xy_buf.free()


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_exact_capacity_and_one_short(handle):
    key = (4, 3, 9, 4, 2)
    m, records, _ = records_of("wall", key)
    dm = DeviceMap(handle, m)
    rec = handle.alloc(16 * len(records)).from_host(record_array(records))
    nc = dm.n_chains
    try:
        for flags in (0, _capi.RJ_NODE_DROP_LAST):
            want = noded("wall", key, bool(flags))
            n = want[3]["n_points"]
            with pytest.raises(_capi.NodeOverflow) as e:  # the sizing call
                handle.map_node(*dm.args(), rec, len(records), flags, 0, None, None)
            assert e.value.counts == want[3] and e.value.code == _capi.RJ_E_OVERFLOW
            for cap in (n, n - 1):
                bufs = [handle.alloc(16 * cap + 32).from_host(np.full(4 * cap + 8, CANARY, np.uint32)),
                        handle.alloc(4 * (nc + 1) + 32).from_host(np.full(nc + 9, CANARY, np.uint32)),
                        handle.alloc(4 * cap + 32).from_host(np.full(cap + 8, CANARY, np.uint32))]
                if cap == n:
                    assert handle.map_node(*dm.args(), rec, len(records), flags, cap, *bufs) == want[3]
                    got = (bufs[0].to_host(np.int64, 2 * n).reshape(-1, 2), bufs[1].to_host(np.uint32, nc + 1), bufs[2].to_host(np.uint32, want[3]["n_edges"]),
                           want[3])
                    same(got, want)
                    assert (bufs[0].to_host(np.uint32)[4 * cap:] == CANARY).all() and (bufs[1].to_host(np.uint32)[nc + 1:] == CANARY).all()
                    assert (bufs[2].to_host(np.uint32)[want[3]["n_edges"]:] == CANARY).all()
                else:
                    with pytest.raises(_capi.NodeOverflow) as e:
                        handle.map_node(*dm.args(), rec, len(records), flags, cap, *bufs)
                    assert e.value.counts == want[3]
                    assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
                for b in bufs:
                    b.free()
    finally:
        rec.free()
        dm.free()


def refused(h, m, records, flags=0, word=None):
    dm = DeviceMap(h, m)
    rec = h.alloc(16 * max(1, len(records))).from_host(record_array(records))
    n = dm.n_points + 2 * len(records)
    bufs = [h.alloc(16 * n).from_host(np.full(4 * n, CANARY, np.uint32)), h.alloc(4 * (dm.n_chains + 1)).from_host(np.full(dm.n_chains + 1, CANARY, np.uint32))]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_node(*dm.args(), rec, len(records), flags, n, *bufs)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
    finally:
        for b in bufs + [rec]:
            b.free()
        dm.free()


def test_refusals(handle):
    m, records, _ = records_of("hand", "two-cuts-reversed")
    xy, row = m
    assert records == [(0, 1, 2), (0, 2, 2)]
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        refused(handle, (xy, np.array(bad_row, np.uint32)), [], word="row_index")
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        refused(handle, (bad, row), records, word="coordinate")
    refused(handle, m, records, flags=2, word="flags")
    for bad_records in ([(1, 0, 2)], [(1, 1, 2)], [(0, 3, 2)], [(0, 1, 0)], [(0, 1, 5)]):
        refused(handle, m, bad_records, word="kind in 1..4")
    for bad_records in ([(0, 2, 2), (0, 1, 2)], [(0, 1, 2), (0, 1, 2)], [(1, 2, 1), (0, 2, 2)]):
        refused(handle, m, bad_records, word="ascend")
    zero = NC.chain_arrays(NC.HAND["zero-edge-and-one-point-chain"][0])
    for bad_records in ([(0, 2, 2)], [(1, 3, 2)]):
        refused(handle, zero, bad_records, word="zero length")
    refused(handle, m, records, flags=_capi.RJ_NODE_DROP_LAST, word="RJ_NODE_DROP_LAST")
    refused(handle, NC.chain_arrays([[(0, 0), (4, 0), (0, 4), (0, 0)], [(2, 2)]]), [], flags=_capi.RJ_NODE_DROP_LAST, word="RJ_NODE_DROP_LAST")
    dm = DeviceMap(handle, m)
    with pytest.raises(_capi.RayJoinError) as e:  # points wanted, nowhere to put them
        handle.map_node(*dm.args(), None, 0, 0, 8, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # records announced, none given
        handle.map_node(*dm.args(), None, 2, 0, 0, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:
        handle.map_node(*dm.args(), dm.bufs[0], 1 << 31, 0, 0, None, None)
    assert e.value.code == _capi.RJ_E_INVALID and "2^31" in str(e.value)
    dm.free()


def test_no_chains_and_a_record_that_does_not_fit(handle):
    row = handle.alloc(4).from_host(np.array([CANARY], np.uint32))
    assert handle.map_node(None, 0, None, 0, None, 0, 0, 0, None, row) == dict.fromkeys(_capi.NODE_COUNTS, 0)
    assert row.to_host(np.uint32, 1)[0] == 0
    row.free()
    m, _, _ = records_of("hand", "proper-only")
    got = device_node(handle, m, [(0, 1, 2)])  # a touch record over a proper crossing: counted, no point leaves its edge
    same(got, NR.node_ref(m[0], m[1], [(0, 1, 2)]))
    assert got[3]["n_used"] == 1 and got[3]["n_cuts"] == 0 and np.array_equal(got[0], m[0])


# ---- the wrappers, the stage times, the handle ----------------------------------------------------------------------------------
def test_chain_map_node_and_stage_times(handle):
    """DeviceChainMap.Node on the chain map of the three squares as given: its left / right stay valid -- the noded map
    through face_rings has one ring per square and one outside"""
    ring_row, ring_xy, ring_face = three_squares()
    bufs = [handle.alloc(4 * len(ring_row)).from_host(ring_row), handle.alloc(16 * len(ring_xy)).from_host(ring_xy)]
    dm = chain_map_of(handle, bufs[0], bufs[1], len(ring_xy), ring_face)
    try:
        host = dm.to_host()[0]
        ref_records, _ = CR.map_crossings_ref(host.pts, host.row_index)
        want = NR.node_ref(host.pts, host.row_index, ref_records)
        nm = dm.Node(handle, edge_origin=True)
        same(nm.to_host() + (nm.counts,), want)
        us = [handle.get_option("node_last_us%d" % k) for k in range(6)]
        assert all(v >= 0 for v in us) and us[5] >= max(us[:5])
        nm.free()
    finally:
        dm.free()
        for b in bufs:
            b.free()


def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_output_map_node_equals_the_definition():
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        records, _ = om.Crossings(ov.h)
        host = om.to_host()[0]
        want = NR.node_ref(host.pts, host.row_index, [(int(r["eid"][0]), int(r["eid"][1]), int(r["kind"])) for r in records])
        for kw in (dict(), dict(records=records)):
            nm = om.Node(ov.h, edge_origin=True, **kw)
            same(nm.to_host() + (nm.counts,), want)
            nm.free()
        om.free()
    finally:
        dctx.close()


def test_the_handle_stays_as_it_was():
    """an LSI query's result and rj_get_plan's text are the same before and after a noding call on the handle"""
    import json
    dctx = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        lsi = ops.LSILBVH(dctx)
        lsi.Init(4 * (dctx.get_map(0).n_edges + dctx.get_map(1).n_edges))
        lsi.Query(1)
        before = lsi.get_pairs().copy()
        plan = json.dumps(dctx.handle.get_plan(), sort_keys=True)
        same(device_node(dctx.handle, records_of("wall", BIG_WALL)[0], None), noded("wall", BIG_WALL))
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
