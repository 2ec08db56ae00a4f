"""Thinning the chains of a map on the device (rj_map_simplify, ops.map_simplify, DeviceChainMap.Simplify,
DeviceOutputMap.Simplify) against the host twin and the plain-Python definition (tests/simplify_ref.py), every array and
every count, with and without origin, over the work list and -- the debug option "simplify_all_points" -- over all
points in every round: the hand maps of tests/simplify_cases.py (the triangle near +-2^46 whose weight needs the high
word of the tolerance among them), the 40 random maps at three tolerances each, one chain of 5 000 points (it crosses
waves and blocks), a closed chain of 3 000 points (the pin reductions take 47 steps of a wave), the staircase that loses
one point per round.  Then the contract on the device (sizing call, exact capacity, one short with canaries, every
refusal), the wrappers end to end (the sample pair's output map, thinned, checked, installed, queried), a second call
that removes nothing, the stage times and the handle's state.  The CPU side is tests/test_simplify.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simplify_cases as SC  # noqa: E402
import simplify_ref as SR  # noqa: E402
from test_simplify import LONG, LONG_TOLS, OK, map_of, thinned, twin_last, twin_lib, twin_simplify  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A
HUGE = SC.HUGE
RING = 3000


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


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


def device_simplify(h, m, tol, origin=True, all_points=False):
    """-> (out_xy, out_row, origin, counts) through ops.map_simplify"""
    dm = DeviceMap(h, m)
    h.set_debug_option("simplify_all_points", 1 if all_points else 0)
    try:
        sm = ops.map_simplify(h, *dm.args(), tol, origin=origin)
        try:
            assert sm.n_chains == dm.n_chains
            return sm.to_host() + (sm.counts,)
        finally:
            sm.free()
    finally:
        h.set_debug_option("simplify_all_points", 0)
        dm.free()


def same(got, want):
    assert got[3] == want[3]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[2] is None or np.array_equal(got[2], want[2]))


def check(h, twin, m, tol, want):
    """the device over all points, the twin and the device over its work list: each the definition's answer; the device
    ran the twin's rounds (one sync each, one at the end) over work lists of the twin's sizes"""
    same(device_simplify(h, m, tol, all_points=True), want)
    rc, xy, row, origin, counts = twin_simplify(twin, m, tol, capacity=max(1, len(m[0])))
    assert rc == OK
    same((xy, row, origin, counts), want)
    same(device_simplify(h, m, tol), want)
    rounds, looked = twin_last(twin)
    assert (h.get_option("simplify_last_syncs"), h.get_option("simplify_last_list_sum")) == (rounds + 1, looked)


def ring(n):
    """a closed chain of n points on a lattice circle, walked twice around: many ties in both pin reductions"""
    k = np.arange(n - 1)
    t = 4 * np.pi * k / (n - 1)
    pts = np.stack([np.rint(300 * np.cos(t)), np.rint(300 * np.sin(t))], 1).astype(np.int64)
    return np.concatenate([pts, pts[:1]]), np.array([0, n], np.uint32)


# ---- the device against the twin, the definition and the written answers -------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.HAND))
def test_hand_cases(handle, twin, name):
    tol, kept = SC.HAND[name][1], SC.HAND[name][2]
    want = thinned("hand", name, tol)
    assert want[2].tolist() == kept
    m = map_of("hand", name)
    check(handle, twin, m, tol, want)
    same(device_simplify(handle, m, tol, origin=False), want)


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_random_maps(handle, twin, seed):
    for tol in SC.tols(seed):
        check(handle, twin, map_of("random", seed), tol, thinned("random", seed, tol))


@pytest.mark.parametrize("tol", LONG_TOLS)
def test_long_chain(handle, twin, tol):
    """5 000 points of one chain: 20 waves, 20 blocks; neighbours in different blocks decide against each other"""
    want = thinned("long", LONG, tol)
    assert want[3]["n_max_round"] > 1000
    check(handle, twin, map_of("long", LONG), tol, want)


@pytest.mark.parametrize("tol", (0, 40, HUGE))
def test_long_ring(handle, twin, tol):
    """a closed chain of 3 000 points: each pin reduction is 47 strides of a wave and a butterfly, with ties"""
    m = ring(RING)
    want = SR.simplify_ref(m[0], m[1], tol)
    assert want[3]["n_closed"] == 1 and want[3]["n_pinned_extra"] == 2 and (tol != HUGE or want[3]["n_points"] == 4)
    check(handle, twin, m, tol, want)


def test_staircase(handle, twin):
    """one point per round, 198 rounds; every point stays a candidate, so the list of round k is all that is left"""
    want = thinned("hand", "staircase-200", HUGE)
    check(handle, twin, map_of("hand", "staircase-200"), HUGE, want)
    assert want[3]["n_rounds"] == 198
    assert handle.get_option("simplify_last_syncs") == 199  # one per round, one at the end: the last list is empty
    assert handle.get_option("simplify_round_list0") == 200 and handle.get_option("simplify_round_list1") == 197
    assert handle.get_option("simplify_last_list_max") == 197 and handle.get_option("simplify_last_list_sum") == 197 * 198 // 2
    assert handle.get_option("simplify_late_rounds") == 198 - 10 and handle.get_option("simplify_late_list") == 188 * 189 // 2


def test_work_list_against_all_points(handle):
    """the same arrays and counts both ways; behind the first round the nine work lists together are less than two passes
    over the points, where all points cost one pass per round"""
    m, want = map_of("long", LONG), thinned("long", LONG, 50)
    listed = device_simplify(handle, m, 50)
    looked, syncs = handle.get_option("simplify_last_list_sum"), handle.get_option("simplify_last_syncs")
    everything = device_simplify(handle, m, 50, all_points=True)
    same(listed, want)
    same(everything, want)
    same(listed, everything)
    assert handle.get_option("simplify_last_list_sum") == 0 and handle.get_debug_option("simplify_all_points") == 0
    assert handle.get_option("simplify_last_syncs") == syncs == want[3]["n_rounds"] + 2
    assert [handle.get_option("simplify_round_list%d" % k) for k in range(3)] == [LONG] * 3
    assert 0 < looked < 2 * LONG


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_exact_capacity_and_one_short(handle):
    m, want = map_of("random", 5), thinned("random", 5, 60)
    dm = DeviceMap(handle, m)
    nc, n = dm.n_chains, want[3]["n_points"]
    try:
        with pytest.raises(_capi.SimplifyOverflow) as e:  # the sizing call
            handle.map_simplify(*dm.args(), 60, 0, None, None)
        assert e.value.counts == want[3] and e.value.code == _capi.RJ_E_OVERFLOW
        for cap in (n, n - 1, n + 3):
            for with_origin in (True, False):
                bufs = [handle.alloc(16 * cap + 32).from_host(np.full(4 * cap + 8, CANARY, np.uint32)),
                        handle.alloc(4 * (nc + 1) + 32).from_host(np.full(nc + 9, CANARY, np.uint32)),
                        handle.alloc(4 * cap + 32).from_host(np.full(cap + 8, CANARY, np.uint32))]
                args = bufs if with_origin else bufs[:2]
                if cap >= n:
                    assert handle.map_simplify(*dm.args(), 60, cap, *args) == want[3]
                    got = (bufs[0].to_host(np.int64, 2 * n).reshape(-1, 2), bufs[1].to_host(np.uint32, nc + 1), bufs[2].to_host(np.uint32, n), want[3])
                    same(got if with_origin else got[:2] + (None, want[3]), want)
                    assert (bufs[0].to_host(np.uint32)[4 * n:] == CANARY).all() and (bufs[1].to_host(np.uint32)[nc + 1:] == CANARY).all()
                    assert (bufs[2].to_host(np.uint32)[n if with_origin else 0:] == CANARY).all()
                else:
                    with pytest.raises(_capi.SimplifyOverflow) as e:
                        handle.map_simplify(*dm.args(), 60, cap, *args)
                    assert e.value.counts == want[3]
                    assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
                for b in bufs:
                    b.free()
    finally:
        dm.free()


def refused(h, m, tol=0, flags=0, word=None):
    dm = DeviceMap(h, m)
    n = dm.n_points
    bufs = [h.alloc(16 * n).from_host(np.full(4 * n, CANARY, np.uint32)), h.alloc(4 * (dm.n_chains + 1)).from_host(np.full(dm.n_chains + 1, CANARY, np.uint32)),
            h.alloc(4 * n).from_host(np.full(n, CANARY, np.uint32))]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_simplify(*dm.args(), tol, n, *bufs, flags=flags)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
    finally:
        for b in bufs:
            b.free()
        dm.free()


def test_refusals(handle):
    xy, row = SC.chain_arrays([[(0, 0), (1, 0), (2, 0)], [(2, 0), (3, 0)], [(4, 0), (5, 0)]])
    for bad_row in ([1, 3, 5, 7], [0, 3, 5, 6], [0, 3, 3, 7], [0, 5, 3, 7]):
        refused(handle, (xy, np.array(bad_row, np.uint32)), word="row_index")
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        refused(handle, (bad, row), word="coordinate")
    refused(handle, (xy, row), flags=1, word="flags")
    refused(handle, (xy, row), flags=1 << 31, word="flags")
    dm = DeviceMap(handle, (xy, row))
    with pytest.raises(_capi.RayJoinError) as e:  # points wanted, nowhere to put them
        handle.map_simplify(*dm.args(), 0, 8, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # points without chains
        handle.map_simplify(dm.bufs[0], 3, None, 0, 0, 0, None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    for tol in (-1, 1 << 128):
        with pytest.raises(ValueError):
            handle.map_simplify(*dm.args(), tol, 0, None, None)
    dm.free()


def test_no_chains(handle):
    row = handle.alloc(4).from_host(np.array([CANARY], np.uint32))
    assert handle.map_simplify(None, 0, None, 0, 7, 0, None, row) == dict.fromkeys(_capi.SIMPLIFY_COUNTS, 0)
    assert row.to_host(np.uint32, 1)[0] == 0
    row.free()
    points = SC.chain_arrays([[(1, 1)], [(2, 2)]])
    same(device_simplify(handle, points, HUGE), SR.simplify_ref(points[0], points[1], HUGE))


# ---- a second call, the stage times ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [("long", LONG, 50), ("random", 11, 17), ("random", 9, HUGE), ("hand", "square-mid-zero", 0)], ids=str)
def test_a_second_call_removes_nothing(handle, what):
    dm = DeviceMap(handle, map_of(*what[:2]))
    first = ops.map_simplify(handle, *dm.args(), what[2])
    try:
        assert first.counts["n_removed"] > 0
        again = ops.map_simplify(handle, first.xy, first.n_points, first.row_index, first.n_chains, what[2], origin=True)
        assert again.counts["n_removed"] == 0 and again.counts["n_rounds"] == 0 and again.n_points == first.n_points
        assert all(np.array_equal(a, b) for a, b in zip(again.to_host()[:2], first.to_host()[:2]))
        assert np.array_equal(again.to_host()[2], np.arange(first.n_points))
        again.free()
        us = [handle.get_option("simplify_last_us%d" % k) for k in range(6)]
        assert all(v >= 0 for v in us) and us[5] >= max(us[:5]) and handle.get_option("simplify_last_syncs") == 2
    finally:
        first.free()
        dm.free()


# ---- the wrappers, the handle ----------------------------------------------------------------------------------------------
def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_output_map_thinned_checked_installed_queried():
    """the sample pair's output map -> Simplify(tol, check=True) -> InstallMap -> a PIP query; tol is the median weight of
    the map's own interior points, so about half of them are candidates at the start"""
    from test_gpu_overlay_merge import overlay_of
    ctx = _sample_context()
    dctx, ov = overlay_of(ctx, None)
    d2 = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        host = om.to_host()[0]
        pts, row = [tuple(p) for p in host.pts.tolist()], host.row_index.tolist()
        weights = sorted(abs(SR.cross(pts[p - 1], pts[p], pts[p + 1])) for b, e in zip(row, row[1:]) for p in range(b + 1, e - 1))
        assert len(weights) > 1000
        tol = weights[len(weights) // 2]
        want = SR.simplify_ref(host.pts, host.row_index, tol)
        assert len(weights) // 4 < want[3]["n_removed"] < len(weights)
        sm, crossings = om.Simplify(ov.h, tol, check=True)
        assert isinstance(sm, ops.DeviceChainMap) and sm.n_chains == om.n_chains
        got = sm.to_host()[0]
        assert np.array_equal(got.pts, want[0]) and np.array_equal(got.row_index, want[1])
        assert np.array_equal(got.left, host.left) and np.array_equal(got.right, host.right)
        assert {k: sm.counts[k] for k in SR.COUNTS} == want[3] and sm.counts["n_edges"] == want[3]["n_points"] - om.n_chains
        assert set(crossings) == set(_capi.CROSSINGS_COUNTS) and crossings["n_edges"] == sm.counts["n_edges"]
        assert crossings == sm.Crossings(ov.h)[1]
        om.free()  # (the thinned map owns its own left / right)
        rings = sm.Rings(ov.h)
        assert rings.n_rings > 0
        rings.free()
        d2.InstallMap(0, sm)
        sm.free()
        assert np.array_equal(d2.get_map(0).pts, want[0])
        d2.BuildIndex(0)
        pip = ops.PIPLBVH(d2)
        query = d2.get_map(1).pts
        pip.Init(len(query))
        pip.Query(1)
        faces = pip.get_face_ids()
        assert len(faces) == len(query) and (faces >= 0).all() and len(set(faces.tolist())) > 10
    finally:
        dctx.close()
        d2.close()


def test_chain_map_simplify_keeps_the_faces(handle):
    """DeviceChainMap.Simplify on the chain map of a 4 x 3 wall of squares with mid-side points: every border loses its
    mid-side points, the rings of the thinned map are the same faces with the same areas"""
    unit, rings, faces = 1 << 20, [], []
    for j in range(3):
        for i in range(4):
            x, y = 4 * i, 4 * j
            rings += [(x, y), (x + 2, y), (x + 4, y), (x + 4, y + 2), (x + 4, y + 4), (x + 2, y + 4), (x, y + 4), (x, y + 2)]
            faces.append(1 + len(faces))
    ring_row, ring_xy, ring_face = np.arange(0, 8 * 12 + 1, 8).astype(np.uint32), np.array(rings, np.int64) * unit, np.array(faces, np.int32)
    bufs = [handle.alloc(4 * len(ring_row)).from_host(ring_row), handle.alloc(16 * len(ring_xy)).from_host(ring_xy), handle.alloc(4 * len(ring_face)).from_host(ring_face)]
    dm = ops.rings_map(handle, bufs[0], bufs[1], len(ring_xy), bufs[2], len(ring_face))
    try:
        sm, crossings = dm.Simplify(handle, 0, check=True)
        host, _ = dm.to_host()
        want = SR.simplify_ref(host.pts, host.row_index, 0)
        got = sm.to_host()[0]
        assert np.array_equal(got.pts, want[0]) and np.array_equal(got.row_index, want[1]) and want[3]["n_removed"] > 0
        assert crossings["n_found"] == 0
        r0, r1 = dm.Rings(handle), sm.Rings(handle)
        p0, p1 = r0.Polygons(handle), r1.Polygons(handle)
        areas = [sorted((int(f), a2) for f, a2, _, _ in p.polygons(r)) for p, r in ((p0, r0), (p1, r1))]
        assert areas[0] == areas[1] == [(f, 2 * 16 * unit * unit) for f in faces]
        assert r1.n_points < r0.n_points
        for x in (p0, p1, r0, r1, sm):
            x.free()
    finally:
        dm.free()
        for b in bufs:
            b.free()


def test_the_handle_stays_as_it_was():
    """an LSI query's result and rj_get_plan's text are the same before and after a thinning call on the handle"""
    import json
    dctx = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        lsi = ops.LSILBVH(dctx)
        lsi.Init(4 * (dctx.get_map(0).n_edges + dctx.get_map(1).n_edges))
        lsi.Query(1)
        before = lsi.get_pairs().copy()
        plan = json.dumps(dctx.handle.get_plan(), sort_keys=True)
        same(device_simplify(dctx.handle, map_of("long", LONG), 50), thinned("long", LONG, 50))
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
