"""Faces of a chain map on the device (rj_map_faces, ops.map_faces, DeviceChainMap.Faces) against the plain-Python
definition (tests/faces_ref.py) or, where the map is too large for the Python loop, the host twin
(tests/hosttwin/faces_twin.cc), array for array: the hand cases of tests/faces_cases.py; the random planar maps of
tests/rings_planar.py, half of them stretched to +-2^46, each at the default shift of the grid, at 15 and at 47 with equal
results; equality with the device's OWN composition (rj_map_rings with one constant label, then rj_rings_polygons' parent[]) on
those maps and on an overlay's output map; a ring of 100 003 points; a column of 70 000 isolated unit squares (more than
2^16 holes in one column of the grid, a jumping depth of 70 000) with the bound on the candidate tests that only the
bucketing in y keeps; more rings than one launch covers; the label check; faces_dev NULL, overflow with canaries, the
refusals, and a PIP query that answers the same before and after a call.  The CPU side is tests/test_faces.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faces_cases as FC  # noqa: E402
import faces_ref as FR  # noqa: E402
import rings_planar as P  # noqa: E402
from test_faces import CORNER_WALKS, SEEDS, SHIFTS, hand_case, unit_column_walk, planar_case, swapped_labels, twin_faces, twin_lib  # noqa: E402
from test_gpu_overlay_merge import overlay_of  # noqa: E402
from test_overlay_map import pair  # noqa: E402
from test_rings import FIELD  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
COLUMN = 70_000


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


class DeviceLines:
    """unlabelled linework (xy, row_index) in device buffers, with optional labels"""

    def __init__(self, h, xy, row, labels=None):
        xy, row = np.ascontiguousarray(xy, np.int64).reshape(-1, 2), np.ascontiguousarray(row, np.uint32)
        self.n_points, self.n_chains = len(xy), len(row) - 1
        self.xy, self.row = h.alloc(16 * max(1, len(xy))).from_host(xy), h.alloc(4 * len(row)).from_host(row)
        self.labels = None
        if labels is not None:
            self.labels = tuple(h.alloc(4 * max(1, self.n_chains)).from_host(np.ascontiguousarray(a, np.int32)) for a in labels)

    def args(self):
        return (self.xy, self.n_points, self.row, self.n_chains)

    def free(self):
        for b in (self.xy, self.row) + (self.labels or ()):
            b.free()


def device_faces(h, xy, row, labels=None, shift=0, records=True):
    """-> (dict(left, right, faces, counts) of ops.map_faces, the shift the grid had)"""
    dl = DeviceLines(h, xy, row, labels)
    h.set_debug_option("faces_shift", shift)
    try:
        fm = ops.map_faces(h, *dl.args(), labels=dl.labels, records=records)
        try:
            m, counts = fm.to_host()
            assert np.array_equal(m.pts, np.asarray(xy).reshape(-1, 2)) and np.array_equal(m.row_index, row)
            got = dict(left=m.left.astype(np.int32), right=m.right.astype(np.int32), faces=fm.faces_to_host() if records else None,
                       counts={k: counts[k] for k in FR.COUNTS})
            return got, h.get_option("faces_last_shift")
        finally:
            fm.free()
    finally:
        h.set_debug_option("faces_shift", 0)
        dl.free()


def composition(h, xy, row):
    """the device's own composition: rj_map_rings with the constant label 1, rj_rings_polygons' parent[] -> (left, right): per
    half-chain the rank of its ring's shell among the shells (1-based), 0 where the ring has none"""
    nc = len(row) - 1
    ones = np.ones(nc, np.int32)
    dl = DeviceLines(h, xy, row, (ones, ones))
    try:
        r = ops.face_rings(h, dl.xy, dl.n_points, dl.row, dl.labels[0], dl.labels[1], nc)
        try:
            p = r.Polygons(h)
            parent = p.to_host()["parent"]
            p.free()
            rg = r.to_host()
        finally:
            r.free()
    finally:
        dl.free()
    assert np.all(np.diff(rg["rings"]["leader"].astype(np.int64)) > 0)  # one label: the rings ascend by leader
    shells = np.flatnonzero(parent == np.arange(len(parent)))
    number = np.zeros(len(parent) + 1, np.int32)
    number[shells] = np.arange(1, len(shells) + 1)
    ring_face = number[np.where(parent == NONE, len(parent), parent)]
    face_of_half = np.zeros(2 * nc, np.int32)
    ring_of_slot = np.repeat(np.arange(len(parent)), np.diff(rg["ring_first"].astype(np.int64)))
    face_of_half[rg["ring_half"]] = ring_face[ring_of_slot]
    return face_of_half[0::2], face_of_half[1::2]


# ---- device against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.HAND))
def test_hand_cases_equal_the_definition(handle, name):
    xy, row, answer, want = hand_case(name)
    for shift in SHIFTS:
        got, _ = device_faces(handle, xy, row, shift=shift)
        FR.assert_same_faces(got, want, (name, shift))
    assert got["left"].tolist() == answer["left"] and got["right"].tolist() == answer["right"] and FR.area2_of(got["faces"]) == answer["area2"]


@pytest.mark.parametrize("seed", SEEDS)
def test_planar_maps_equal_the_definition_at_every_shift_and_the_composition(handle, seed):
    m, info, want = planar_case(seed)
    used = set()
    for shift in SHIFTS:
        got, s = device_faces(handle, m[0], m[1], shift=shift)
        FR.assert_same_faces(got, want, (seed, shift))
        assert s >= max(shift, 15) and handle.get_option("faces_last_registrations") <= 4 * (len(m[0]) - len(m[2])) + 1024
        used.add(s)
    assert 47 in used and len(used) >= 2, seed
    left, right = composition(handle, m[0], m[1])
    assert np.array_equal(left, want["left"]) and np.array_equal(right, want["right"]), seed
    checked, _ = device_faces(handle, m[0], m[1], labels=(m[2], m[3]))
    assert checked["counts"]["n_conflicts"] == 0 and np.array_equal(checked["left"], want["left"]), seed


def test_half_of_the_planar_maps_span_the_coordinate_range():
    full = [s for s in SEEDS if planar_case(s)[1]["full_range"]]
    assert 10 <= len(full) <= 30
    assert all(int(np.abs(planar_case(s)[0][0]).max()) > 1 << 45 for s in full)


def test_overlay_output_map_equals_the_composition(handle, twin):
    """the union map of the ring pair (47 holes).  Equality with the composition is promised where the map has no overlapping
    or equal edges -- there no two candidates tie beyond the slope -- and this map has none (the nested pair's map has)"""
    gs, _ = pair("rings")
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, how="union", by="pair")
        try:
            crossings = om.Crossings(ov.h)[1]
            assert crossings["n_overlap"] == 0 and crossings["n_equal"] == 0
            m = om.to_host()[0]
            xy, row = np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32)
            fm = ops.map_faces(ov.h, om.xy, om.n_points, om.row_index, om.n_chains, labels=(om.left, om.right))
            try:
                hm, counts = fm.to_host()
                left, right = composition(ov.h, xy, row)
                assert np.array_equal(hm.left, left) and np.array_equal(hm.right, right) and counts["n_faces"] > 100 and counts["n_holes"] > 40
                rc, want, _ = twin_faces(twin, xy, row, labels=(m.left.astype(np.int32), m.right.astype(np.int32)))
                assert rc == 0 and {k: counts[k] for k in FR.COUNTS} == want["counts"] and np.array_equal(fm.faces_to_host(), want["faces"])
                assert counts["n_conflicts"] == 0  # the overlay's own labels describe the partition of its geometry
            finally:
                fm.free()
        finally:
            om.free()
    finally:
        dctx.close()


# ---- device against the twin, where the Python loop is too slow -------------------------------------------------------------
def test_a_ring_of_100_003_points(handle, twin):
    m = P.long_chains()
    rc, want, _ = twin_faces(twin, m[0], m[1], labels=(m[2], m[3]))
    assert rc == 0 and want["counts"]["n_faces"] == 2 and want["counts"]["n_conflicts"] == 0 and want["counts"]["n_dangling"] == 1
    assert want["left"].tolist() == [1, 0, 1] and want["right"].tolist() == [0, 0, 2]
    got, _ = device_faces(handle, m[0], m[1], labels=(m[2], m[3]))
    FR.assert_same_faces(got, want)


def test_more_rings_than_one_launch_covers(handle, twin):
    """triangle_field in units of 2^12: the grid's cells are at least 2^15 wide, and a field drawn in single units would lie
    in one of them -- every hole against every edge.  Scaled maps fill the coordinate range."""
    xy, row, _, _ = P.triangle_field(FIELD)
    xy = xy * 4096
    rc, want, stats = twin_faces(twin, xy, row)
    assert stats["cells"] > FIELD and stats["ray_tests"] < 200 * FIELD
    assert rc == 0 and want["counts"]["n_rings"] == 2 * FIELD > 1 << 20 and want["counts"]["n_outer"] == FIELD
    got, _ = device_faces(handle, xy, row)
    FR.assert_same_faces(got, want)


@pytest.mark.parametrize("name", sorted(CORNER_WALKS))
def test_the_run_of_the_largest_key_ends(handle, name):
    """components inside the corner cells of the range at the default shift and at a forced 15 (tests/test_faces.py has the
    same on the host, where it ran first): the faces, and the walk's own counters"""
    xy, row, _, want = hand_case(name)
    for shift in (0, 15):
        got, s = device_faces(handle, xy, row, shift=shift)
        FR.assert_same_faces(got, want, (name, shift))
        assert s == 15 and (handle.get_option("faces_last_ray_tests"), handle.get_option("faces_last_cells")) == CORNER_WALKS[name], (name, shift)


def test_a_map_in_single_units_lies_in_one_cell(handle):
    """the floor of the grid, pinned on the device: 64 squares in unit coordinates lie in one cell of 2^15 and cost holes x
    edges; the same map in units of 2^12 costs two runs of four per ray"""
    n = 64
    xy, row = FC.diamond_column(n)
    unit, scaled = unit_column_walk(n)
    got, s = device_faces(handle, xy, row)
    assert s == 15 and (handle.get_option("faces_last_ray_tests"), handle.get_option("faces_last_cells")) == unit
    big, s = device_faces(handle, xy * 4096, row)
    assert s == 15 and (handle.get_option("faces_last_ray_tests"), handle.get_option("faces_last_cells")) == scaled
    assert np.array_equal(got["left"], big["left"]) and np.array_equal(got["right"], big["right"]) and got["counts"] == big["counts"]
    assert got["right"].tolist() == list(range(1, n + 1)) and not got["left"].any()


def test_column_of_squares_is_bucketed_in_y(handle):
    """70 000 unit squares standing on a corner, one above the other: every outside is a hole whose ray meets the next
    square's lowest corner, so above runs up the whole column and every outside ends in face 0; left is 0, right k + 1.
    All 4 n edges are ceiling edges in one column of the grid.  With a bucket per column every hole tests them all:
    n_holes x ceilings.  The bound asks for an eighth of that; what a ray really meets is one cell's run, or two."""
    xy, row = FC.diamond_column(COLUMN)
    got, shift = device_faces(handle, xy, row)
    k = np.arange(COLUMN)
    assert np.array_equal(got["left"], np.zeros(COLUMN, np.int32)) and np.array_equal(got["right"], (k + 1).astype(np.int32))
    assert got["counts"] == dict(n_faces=COLUMN, n_rings=2 * COLUMN, n_holes=0, n_outer=COLUMN, n_skipped=0, n_dangling=0, n_conflicts=0)
    assert got["faces"]["leader"].tolist() == (2 * k + 1).tolist() and FR.area2_of(got["faces"]) == [4] * COLUMN
    # counted from the input: the holes (one outside per square), the ceiling edges whose cells lie in the rays' column
    n_holes = len(row) - 1
    a, b = xy.reshape(-1, 5, 2)[:, :-1], xy.reshape(-1, 5, 2)[:, 1:]
    ceiling = a[..., 0] != b[..., 0]
    column = (int(xy[0, 0]) + (1 << 46)) >> shift
    in_column = ceiling & ((np.minimum(a[..., 0], b[..., 0]) + (1 << 46)) >> shift == column) & ((np.maximum(a[..., 0], b[..., 0]) - 1 + (1 << 46)) >> shift == column)
    n_ceilings = int(in_column.sum())
    assert n_holes == COLUMN > 1 << 16 and n_ceilings == 4 * COLUMN
    tests, cells = handle.get_option("faces_last_ray_tests"), handle.get_option("faces_last_cells")
    print("ray tests %d, cells %d, shift %d, bound %d" % (tests, cells, shift, n_holes * n_ceilings // 8))
    assert 0 < tests < n_holes * n_ceilings // 8 and cells >= n_holes
    us = [handle.get_option("faces_last_us%d" % i) for i in range(6)]
    assert all(v >= 0 for v in us) and us[5] >= max(us[:5])


# ---- the label check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7, 23])
def test_label_check_counts_a_swapped_chain(handle, seed):
    m, _, want = planar_case(seed)
    labels = swapped_labels(m, want)
    checked = FR.faces_ref(m[0], m[1], *labels)
    got, _ = device_faces(handle, m[0], m[1], labels=labels)
    FR.assert_same_faces(got, checked, seed)
    assert got["counts"]["n_conflicts"] == checked["counts"]["n_conflicts"] > 0


def test_chain_map_faces_checks_its_own_labels(handle):
    """DeviceChainMap.Faces: a map made from labelled rings, its faces recomputed, its own labels checked; the result is a
    chain map that Rings() takes"""
    m, _, want = planar_case(3)
    dl = DeviceLines(handle, m[0], m[1], (m[2], m[3]))
    try:
        cm = ops.DeviceChainMap(dl.xy, dl.row, dl.labels[0], dl.labels[1], dict(n_chains=dl.n_chains, n_points=dl.n_points))
        fm = cm.Faces(handle, check=True)
        try:
            assert fm.counts["n_conflicts"] == 0 and fm.counts["n_faces"] == want["counts"]["n_faces"]
            r = fm.Rings(handle, points=False)
            assert r.to_host()["counts"]["n_mixed"] == 0
            r.free()
        finally:
            fm.free()
    finally:
        dl.free()


# ---- the contract ------------------------------------------------------------------------------------------------------
def raw_call(h, dl, cap, faces=True, in_left=None, in_right=None, flags=0, canary=-7):
    """rj_map_faces into arrays filled with canaries -> (left, right, records [cap + 2], the counts or the error)"""
    nc = dl.n_chains
    left, right = h.alloc(4 * max(1, nc)).from_host(np.full(max(1, nc), canary, np.int32)), h.alloc(4 * max(1, nc)).from_host(np.full(max(1, nc), canary, np.int32))
    rec = np.zeros(cap + 2, FR.FACE_DTYPE)
    rec["leader"] = 0xABABABAB
    fb = h.alloc(rec.nbytes).from_host(rec)
    try:
        try:
            out = h.map_faces(*dl.args(), left, right, fb if faces else None, cap, in_left, in_right, flags)
        except _capi.RayJoinError as e:
            out = e
        return left.to_host(np.int32, nc), right.to_host(np.int32, nc), fb.to_host(FR.FACE_DTYPE, cap + 2), out
    finally:
        for b in (left, right, fb):
            b.free()


def test_null_records_overflow_and_refusals(handle):
    xy, row, _, want = hand_case("island-lake-island")
    dl = DeviceLines(handle, xy, row, (np.zeros(4, np.int32), np.zeros(4, np.int32)))
    try:
        left, right, rec, out = raw_call(handle, dl, 0, faces=False)  # no records: the capacity is ignored, nothing overflows
        assert out == want["counts"] and np.array_equal(left, want["left"]) and np.array_equal(right, want["right"])
        assert np.all(rec["leader"] == 0xABABABAB)
        left, right, rec, out = raw_call(handle, dl, 2)  # overflow: true counts, left / right complete, nothing behind the capacity
        assert isinstance(out, _capi.FacesOverflow) and out.counts == want["counts"]
        assert np.array_equal(left, want["left"]) and np.array_equal(right, want["right"])
        assert np.array_equal(rec[:2], want["faces"][:2]) and np.all(rec["leader"][2:] == 0xABABABAB)
        left, right, rec, out = raw_call(handle, dl, 4)
        assert out == want["counts"] and np.array_equal(rec[:4], want["faces"]) and np.all(rec["leader"][4:] == 0xABABABAB)
        for kw in (dict(in_left=dl.labels[0]), dict(in_right=dl.labels[1]), dict(flags=1), dict(flags=1 << 31)):
            left, right, rec, out = raw_call(handle, dl, 4, **kw)
            assert isinstance(out, _capi.RayJoinError) and out.code == _capi.RJ_E_INVALID, kw
            assert np.all(left == -7) and np.all(right == -7) and np.all(rec["leader"] == 0xABABABAB), kw
    finally:
        dl.free()
    for bad_row in ([1, 5, 10, 15, 20], [0, 5, 10, 15, 19], [0, 5, 5, 15, 20], [0, 10, 5, 15, 20]):
        dl = DeviceLines(handle, xy, np.array(bad_row, np.uint32))
        try:
            left, right, rec, out = raw_call(handle, dl, 4)
            assert isinstance(out, _capi.RayJoinError) and out.code == _capi.RJ_E_INVALID, bad_row
            assert np.all(left == -7) and np.all(right == -7) and np.all(rec["leader"] == 0xABABABAB), bad_row
        finally:
            dl.free()
    xy, row, _, _ = hand_case("triangle")
    for at, v, fine in ((1, 1 << 46, False), (2, -(1 << 46) - 1, False), (1, (1 << 46) - 1, True), (2, -(1 << 46), True)):
        far = xy.copy()
        far[at, 0] = v  # a corner of the triangle pulled out to the range's edge, or just past it
        dl = DeviceLines(handle, far, row)
        try:
            left, right, rec, out = raw_call(handle, dl, 4)
            if fine:
                assert out == FR.faces_ref(far, row)["counts"] and left.tolist() == [1] and right.tolist() == [0], v
            else:
                assert isinstance(out, _capi.RayJoinError) and out.code == _capi.RJ_E_INVALID and np.all(left == -7), v
        finally:
            dl.free()


def test_no_state_of_the_handle_changes():
    """an uploaded map and its index answer a PIP query identically before and after a call, options included"""
    ctx = maps.Context([synth.lattice_map(6, 90, 1), synth.lattice_map(14, 40, 2)]).load()
    dctx = ops.DeviceContext(ctx, 0).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        pip = ops.PIPLBVH(dctx)
        pip.Init(ctx.maps[1].n_points)
        pip.Query(1)
        before = (pip.get_closest_eids().copy(), pip.get_face_ids().copy())
        m = ctx.maps[0]
        got, _ = device_faces(dctx.handle, m.pts, m.row_index, labels=(m.left.astype(np.int32), m.right.astype(np.int32)))
        assert got["counts"]["n_faces"] > 0 and got["counts"]["n_conflicts"] == 0
        pip.Query(1)
        assert np.array_equal(pip.get_closest_eids(), before[0]) and np.array_equal(pip.get_face_ids(), before[1])
        assert dctx.handle.get_debug_option("faces_shift") == 0
    finally:
        dctx.close()
