"""Crossings inside one map on the device (rj_map_crossings, ops.map_crossings, DeviceChainMap.Crossings,
DeviceOutputMap.Crossings, DeviceContext.Crossings) against the plain-Python definition (tests/crossings_ref.py), every
record and every count: the hand cases and the grid shapes of tests/crossings_cases.py at the chosen shift and at the
forced shifts 15, 33 and 47, stars through one cell (runs longer than a row block), 10 random soups, 6 planar maps with
and without chains thrown across them; the contract (sizing call, exact capacity, one short with canaries, malformed
maps, flags), the guard, the wrappers, the map that rings_map makes of two overlapping squares, the sample pair's own
output map, and the handle's state.  The CPU side is tests/test_crossings.py.

What rj_map_crossings finds on the sample pair's output map (drop_degenerate and merge on) is asserted EQUAL to the
definition on the same map read back, not zero: the count is a finding (cut points are truncated to integers), reported in
DESIGN.md."""
import json
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_cases as CC  # noqa: E402
import crossings_ref as CR  # noqa: E402
from test_crossings import ALL_HAND, hand_case, planar_case, soup_case, star_case, thrown_case  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
SHIFTS = (15, 33, 47)
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


def tuples(records):
    return [(int(r["eid"][0]), int(r["eid"][1]), int(r["kind"])) for r in records]


def device_crossings(h, m, shift=0, **kw):
    """-> (records as tuples, counts) through ops.map_crossings, at a forced shift or the chosen one"""
    dm = DeviceMap(h, m)
    h.set_debug_option("cross_shift", shift)
    try:
        records, counts = ops.map_crossings(h, *dm.args(), **kw)
        assert (records["_pad"] == 0).all()
        return tuples(records), counts
    finally:
        h.set_debug_option("cross_shift", 0)
        dm.free()


# ---- the device against the definition and the written answers -------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_HAND)
def test_hand_cases(handle, name):
    m, want, counts, (ref, ref_counts) = hand_case(name)
    got, c = device_crossings(handle, m)
    assert got == ref == want and c == ref_counts == counts


@pytest.mark.parametrize("shift", SHIFTS)
def test_hand_cases_at_forced_shifts(handle, shift):
    for name in sorted(CC.HAND) + sorted(CC.GRID):
        m, want, counts, _ = hand_case(name)
        got, c = device_crossings(handle, m, shift)
        assert got == want and c == counts, name
    assert handle.get_option("cross_last_shift") == shift


def test_rim_cases_in_one_cell(handle):
    for name in ("diagonal-proper", "diagonal-none", "diagonal-both", "diagonal-touch", "diagonal-miss", "touch-at-the-rim"):
        m, want, counts, _ = hand_case(name)
        got, c = device_crossings(handle, m, 47)
        assert got == want and c == counts, name


@pytest.mark.parametrize("n", CC.STAR_SIZES)
def test_star_in_one_cell(handle, n):
    m, want, counts = star_case(n)
    for shift in (0, 47):
        got, c = device_crossings(handle, m, shift)
        assert got == want and c == counts
        assert handle.get_option("cross_last_largest_cell") == n and handle.get_option("cross_last_pair_tests") == n * (n - 1) // 2
        assert handle.get_option("cross_last_items") == (n + 63) // 64


def test_two_long_edges_give_one_record(handle):
    m, want, counts, _ = hand_case("two-long")
    got, c = device_crossings(handle, m, 15)
    assert got == want and len(got) == 1 and handle.get_option("cross_last_pair_tests") > 1000


@pytest.mark.parametrize("seed", range(10))
def test_soups(handle, seed):
    m, (records, counts) = soup_case(seed)
    got, c = device_crossings(handle, m)
    assert got == records and c == counts
    if seed < 3:
        for shift in (15, 22, 47):
            got, c = device_crossings(handle, m, shift)
            assert got == records and c == counts


@pytest.mark.parametrize("seed", range(6))
def test_planar_maps_with_and_without_thrown_chains(handle, seed):
    m = planar_case(seed)
    got, c = device_crossings(handle, m)
    assert got == [] and c["n_found"] == 0 and c["n_edges"] == len(m[0]) - (len(m[1]) - 1)
    m, (records, counts) = thrown_case(seed)
    got, c = device_crossings(handle, m)
    assert got == records and c == counts and counts["n_found"] > 0


def test_factors_do_not_change_the_result(handle):
    m, (records, counts) = soup_case(3)
    try:
        for ext, reg in ((1, 2), (4, 8), (64, 1)):
            handle.set_debug_option("cross_extent_factor", ext)
            handle.set_debug_option("cross_reg_factor", reg)
            got, c = device_crossings(handle, m)
            assert got == records and c == counts
    finally:
        handle.set_debug_option("cross_extent_factor", 0)
        handle.set_debug_option("cross_reg_factor", 0)


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_exact_capacity_and_one_short(handle):
    m, (records, counts) = soup_case(1)
    n = counts["n_found"]
    dm = DeviceMap(handle, m)
    try:
        with pytest.raises(_capi.CrossingsOverflow) as e:  # the sizing call
            handle.map_crossings(*dm.args(), 0, None)
        assert e.value.counts == counts and e.value.code == _capi.RJ_E_OVERFLOW
        canary = np.full(8, CANARY, np.uint32)
        for cap in (n, n - 1):
            buf = handle.alloc(16 * cap + 32)
            handle._check(_capi.load().rj_memcpy_h2d(handle.h, buf.ptr + 16 * cap, canary.ctypes.data, 32))
            if cap == n:
                assert handle.map_crossings(*dm.args(), cap, buf) == counts
                assert tuples(buf.to_host(_capi.CROSSING_DTYPE, n)) == records
            else:
                with pytest.raises(_capi.CrossingsOverflow) as e:
                    handle.map_crossings(*dm.args(), cap, buf)
                assert e.value.counts == counts
            assert (buf.to_host(np.uint32, 4 * cap + 8)[4 * cap:] == CANARY).all()
            buf.free()
    finally:
        dm.free()


def test_malformed_maps_and_flags(handle):
    xy, row = hand_case("x")[0]
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        dm = DeviceMap(handle, (xy, np.array(bad_row, np.uint32)))
        with pytest.raises(_capi.RayJoinError) as e:
            handle.map_crossings(*dm.args(), 0, None)
        assert e.value.code == _capi.RJ_E_INVALID and "row_index" in str(e.value)
        dm.free()
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        dm = DeviceMap(handle, (bad, row))
        with pytest.raises(_capi.RayJoinError) as e:
            handle.map_crossings(*dm.args(), 0, None)
        assert e.value.code == _capi.RJ_E_INVALID and "coordinate" in str(e.value)
        dm.free()
    dm = DeviceMap(handle, (xy, row))
    with pytest.raises(_capi.RayJoinError) as e:
        handle.map_crossings(*dm.args(), 0, None, flags=1)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # records wanted, nowhere to put them
        handle.map_crossings(*dm.args(), 4, None)
    assert e.value.code == _capi.RJ_E_INVALID
    dm.free()
    for bad_shift in (1, 14, 48, -1):
        with pytest.raises(_capi.RayJoinError) as e:
            handle.set_debug_option("cross_shift", bad_shift)
        assert e.value.code == _capi.RJ_E_INVALID


def test_guard(handle):
    handle.set_debug_option("cross_pair_budget", 100)
    try:
        chains, _, _ = CC.star(30)
        dm = DeviceMap(handle, CC.chain_arrays(chains))
        with pytest.raises(_capi.RayJoinError) as e:
            handle.map_crossings(*dm.args(), 0, None)
        assert e.value.code == _capi.RJ_E_INVALID and "435 pair tests" in str(e.value) and "holds 30 edges" in str(e.value)
        assert "largest cell (%d, %d)" % (1 << 31, 1 << 31) in str(e.value)  # (shift 15: the cell of (2^14, 2^14) is 2^46 >> 15)
        dm.free()
        m, want, counts = CC.chain_arrays(CC.star(10)[0]), CC.star(10)[1], None
        got, c = device_crossings(handle, m)
        assert got == want and c["n_found"] == 45
    finally:
        handle.set_debug_option("cross_pair_budget", 0)


# ---- the wrappers ------------------------------------------------------------------------------------------------------
def test_overlapping_squares_through_rings_map(handle):
    """two squares of one layer that overlap: rings_map cuts chains at shared vertices only, so their edges cross -- two
    PROPER records"""
    U = 1 << 20
    sq = lambda x, y: [(x * U, y * U), ((x + 4) * U, y * U), ((x + 4) * U, (y + 4) * U), (x * U, (y + 4) * U)]  # noqa: E731
    xy = np.array(sq(0, 0) + sq(2, 2), np.int64)
    bufs = [handle.alloc(12).from_host(np.array([0, 4, 8], np.uint32)), handle.alloc(128).from_host(xy),
            handle.alloc(8).from_host(np.array([1, 2], np.int32))]
    dm = ops.rings_map(handle, bufs[0], bufs[1], 8, bufs[2], 2)
    try:
        records, counts = dm.Crossings(handle)
        host = dm.to_host()[0]
        ref, ref_counts = CR.map_crossings_ref(host.pts, host.row_index)
        assert tuples(records) == ref and counts == ref_counts
        assert counts["n_found"] == counts["n_proper"] == 2 and dm.counts["n_conflicts"] == 0
    finally:
        dm.free()
        for b in bufs:
            b.free()


def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_sample_pair_output_map_equals_the_definition():
    """(equality, not zero: see the module docstring)"""
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        records, counts = om.Crossings(ov.h)
        host = om.to_host()[0]
        ref, ref_counts = CR.map_crossings_ref(host.pts, host.row_index)
        print("sample pair output map: %d chains, %d edges, crossings %s" % (om.n_chains, counts["n_edges"], counts))
        assert tuples(records) == ref and counts == ref_counts
        om.free()
    finally:
        dctx.close()


def test_input_maps_through_the_context_and_the_handle_stays_as_it_was():
    """DeviceContext.Crossings on both input maps of the sample pair (planar: nothing found); rj_get_plan's text and an LSI
    query's result are the same before and after"""
    dctx = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        lsi = ops.LSILBVH(dctx)
        lsi.Init(4 * (dctx.get_map(0).n_edges + dctx.get_map(1).n_edges))
        lsi.Query(1)
        before = lsi.get_pairs().copy()
        plan = json.dumps(dctx.handle.get_plan(), sort_keys=True)
        for im in range(2):
            m = dctx.get_map(im)
            records, counts = dctx.Crossings(im)
            ref, ref_counts = CR.map_crossings_ref(m.pts, m.row_index)
            assert tuples(records) == ref == [] and counts == ref_counts and counts["n_edges"] == m.n_edges
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
