"""The prepared points of an uploaded map (rj_upload_map: every vertex quantised, the extent of every 64 of them) and the
PIP walk that reads them (k_pip_walk2 over a range of the query map's own vertices, "pip_last_prepared" 1 / 2).  The
prepared head must change nothing: closest edges and face ids equal the oracle's on every point of every range, equal
what the same points give as a caller-owned array (the int64 head, report 0), and the walk hands the same number of
points to the rest list -- the group extents, and with them the traversals and their stack overflows, are the same.

USCounty x BlockGroup stand-ins at 0.4: 4.76 M query points, the smallest size at which the handle chooses two points
per lane (four 128-position groups per resident wave)."""
import numpy as np
import pytest

from rayjoin_amd import _capi, maps, synth

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
EMPTY_MIN, EMPTY_MAX = 0x7FFFFFFF, -1


class World:
    pass


@pytest.fixture(scope="module")
def world(oracle):
    oracle.lib().rjo_set_num_threads(16)
    w = World()
    ctx = maps.Context([synth.standin("USCounty", 0.4), synth.standin("BlockGroup", 0.4)]).load()
    w.b, w.q = ctx.maps
    w.np = w.q.n_points
    assert w.np % 64 != 0  # (the last extent block is a partial one)
    w.m0 = oracle.Map(w.b.pts, w.b.row_index, w.b.left, w.b.right)
    w.want = oracle.pip_grid(w.m0, 0, w.q.pts, 512)
    w.want_faces = w.m0.face_ids(w.want)
    # the query map moved up until its top rows lie above everything the base map has: the rays of those points miss
    top_b, top_q = int(w.b.pts[:, 1].max()), int(w.q.pts[:, 1].max())
    shift = (top_b - top_q) + ((1 << 46) - 1 - top_b) // 2
    assert shift > 0 and top_q + shift < (1 << 46)
    w.up = w.q.pts + np.array([0, shift], dtype=np.int64)
    w.want_up = oracle.pip_grid(w.m0, 0, w.up, 512)
    w.want_up_faces = w.m0.face_ids(w.want_up)
    assert 1000 < int((w.want_up == MISS).sum()) < w.np // 4
    # the base map in slot 1 (pip.h:44-46: the tie rules depend on which map asks)
    w.want_b1 = oracle.pip_grid(w.m0, 1, w.q.pts, 512)
    w.want_b1_faces = w.m0.face_ids(w.want_b1)
    return w


def _handle(w, skyline=None, query_pts=None):
    h = _capi.Handle(0)
    if skyline is not None:
        h.set_option("skyline", skyline)
    h.upload_map(0, w.b.pts, w.b.row_index, w.b.left, w.b.right)
    h.upload_map(1, w.q.pts if query_pts is None else query_pts, w.q.row_index, w.q.left, w.q.right)
    h.build_lbvh(0)
    h.set_option("pip_walk", 2)
    return h


def _query(h, n, pts_dev=None, begin=0, base=0):
    """-> (closest, faces, pip_last_prepared) of one synchronous query into freshly poisoned arrays; two points per lane"""
    closest, faces = h.alloc(4 * n), h.alloc(4 * n)
    try:
        closest.from_host(np.full(n, 0xDEADBEEF, dtype=np.uint32))
        faces.from_host(np.full(n, -7, dtype=np.int32))
        h.pip_query(base, 1 - base, pts_dev, begin, n, closest, faces)
        assert h.get_option("pip_last_walk_points") == 2 and h.get_option("pip_last_passes") == 3
        p = h.get_plan()["pip"]
        assert p["first_pass"]["kernel"] == "k_pip_walk2" and p["prepared_points"] == h.get_option("pip_last_prepared")
        return closest.to_host(np.uint32), faces.to_host(np.int32), h.get_option("pip_last_prepared")
    finally:
        closest.free(); faces.free()


def _expect_extents(pts):
    """the per-64 {min x, max x, min y, 0} of (pts + 2^46) >> 16, positions past the end counting for nothing"""
    q = ((pts + (1 << 46)) >> 16).astype(np.int32)
    nb = (len(q) + 63) // 64
    pad = nb * 64 - len(q)
    x_lo = np.concatenate([q[:, 0], np.full(pad, EMPTY_MIN, dtype=np.int32)]).reshape(nb, 64).min(axis=1)
    x_hi = np.concatenate([q[:, 0], np.full(pad, EMPTY_MAX, dtype=np.int32)]).reshape(nb, 64).max(axis=1)
    y_lo = np.concatenate([q[:, 1], np.full(pad, EMPTY_MIN, dtype=np.int32)]).reshape(nb, 64).min(axis=1)
    return q, np.stack([x_lo, x_hi, y_lo, np.zeros(nb, dtype=np.int32)], axis=1)


def _ranges(w):
    """(name, pt_begin, n, report): the whole map, an aligned interior range that ends in mid-group, a misaligned one"""
    n_all = w.np if w.np % 128 else w.np - 1
    n_in = w.np - 64 * 100 - 1000
    n_in -= 1 if n_in % 64 == 0 else 0
    assert n_all % 128 and n_in % 64
    return [("whole", 0, n_all, 2), ("aligned", 64 * 100, n_in, 2), ("misaligned", 64 * 100 + 17, n_in, 1)]


def test_prepared_ranges_equal_the_oracle_and_the_callers_array(world):
    w = world
    h = _handle(w)
    try:
        for name, begin, n, report in _ranges(w):
            ce, cf, rep = _query(h, n, None, begin)
            assert rep == report, name
            assert np.array_equal(ce, w.want[begin:begin + n]), name
            assert np.array_equal(cf, w.want_faces[begin:begin + n]), name
            # the same points as a caller-owned array: the int64 head, identical arrays
            d = h.alloc(16 * n).from_host(w.q.pts[begin:begin + n])
            try:
                ae, af, rep = _query(h, n, d, 0)
                assert rep == 0 and np.array_equal(ae, ce) and np.array_equal(af, cf), name
                if name == "whole":  # ... and both through a forced permutation
                    h.set_option("query_order", 2)
                    for pts_dev in (d, None):
                        oe, of, rep = _query(h, n, pts_dev, 0)
                        assert rep == 0 and h.get_option("query_last_ordered") == 1
                        assert np.array_equal(oe, ce) and np.array_equal(of, cf)
                    h.set_option("query_order", 1)
            finally:
                d.free()
    finally:
        h.close()


def test_the_rest_list_is_the_same_with_either_head(world):
    """An equal count of points left to the rest list means the same groups outgrew the stack: the traversal was not
    loosened.  With the whole stack (next to) nothing is left; with one entry most groups leave the walk (more than half
    of the points: tests/test_gpu_stack.py)."""
    w = world
    h = _handle(w)
    d = h.alloc(16 * w.np).from_host(w.q.pts)
    try:
        left = {}
        for cap in (0, 1):
            h.set_debug_option("walk_stack", cap)
            e1, f1, rep = _query(h, w.np, None, 0)
            own = h.get_option("pip_rest")
            assert rep == 2
            e0, f0, rep = _query(h, w.np, d, 0)
            assert rep == 0 and h.get_option("pip_rest") == own, cap
            assert np.array_equal(e1, w.want) and np.array_equal(e0, w.want) and np.array_equal(f1, f0)
            left[cap] = own
        assert left[1] > w.np // 2 and left[0] < w.np // 100
    finally:
        d.free()
        h.close()


def test_groups_with_lanes_above_the_skyline_compute_their_extent(world):
    w = world
    h = _handle(w, skyline=1, query_pts=w.up)
    try:
        assert h.get_option("skyline_used0") == 1
        for name, begin, n, report in _ranges(w):
            ce, cf, rep = _query(h, n, None, begin)
            assert rep == report, name
            assert np.array_equal(ce, w.want_up[begin:begin + n]), name
            assert np.array_equal(cf, w.want_up_faces[begin:begin + n]), name
    finally:
        h.close()


def test_a_new_map_in_the_slot_brings_its_own_prepared_points(world):
    w = world
    h = _handle(w)
    xy = row = left = right = None
    try:
        ce, _, rep = _query(h, w.np, None, 0)
        assert rep == 2 and np.array_equal(ce, w.want)
        # from the host
        h.upload_map(1, w.up, w.q.row_index, w.q.left, w.q.right)
        qpts, qext = h.map_prepared(1)
        want_q, want_x = _expect_extents(w.up)
        assert np.array_equal(qpts, want_q) and np.array_equal(qext, want_x)
        ce, cf, rep = _query(h, w.np, None, 0)
        assert rep == 2 and np.array_equal(ce, w.want_up) and np.array_equal(cf, w.want_up_faces)
        # from device memory
        xy = h.alloc(16 * w.np).from_host(w.q.pts)
        row = h.alloc(4 * len(w.q.row_index)).from_host(np.ascontiguousarray(w.q.row_index, dtype=np.uint32))
        left = h.alloc(4 * len(w.q.left)).from_host(np.ascontiguousarray(w.q.left).astype(np.int32))
        right = h.alloc(4 * len(w.q.right)).from_host(np.ascontiguousarray(w.q.right).astype(np.int32))
        h.upload_map_dev(1, xy, w.np, row, left, right, len(w.q.left))
        ce, cf, rep = _query(h, w.np, None, 0)
        assert rep == 2 and np.array_equal(ce, w.want) and np.array_equal(cf, w.want_faces)
    finally:
        for d in (xy, row, left, right):
            if d is not None:
                d.free()
        h.close()


def test_map_0_as_the_query_map(world):
    w = world
    h = _capi.Handle(0)
    try:
        h.upload_map(0, w.q.pts, w.q.row_index, w.q.left, w.q.right)
        h.upload_map(1, w.b.pts, w.b.row_index, w.b.left, w.b.right)
        h.build_lbvh(1)
        h.set_option("pip_walk", 2)
        for name, begin, n, report in _ranges(w):
            ce, cf, rep = _query(h, n, None, begin, base=1)
            assert rep == report, name
            assert np.array_equal(ce, w.want_b1[begin:begin + n]), name
            assert np.array_equal(cf, w.want_b1_faces[begin:begin + n]), name
    finally:
        h.close()


def test_prepared_arrays_against_numpy(world):
    """(x + 2^46) >> 16 per vertex and min / max / min per 64 positions, the last partial block and the corners of the
    coordinate range included; a map of fewer than 64 vertices is one partial block"""
    w = world
    h = _capi.Handle(0)
    try:
        h.upload_map(1, w.q.pts, w.q.row_index, w.q.left, w.q.right)
        qpts, qext = h.map_prepared(1)
        want_q, want_x = _expect_extents(w.q.pts)
        assert qpts.shape == (w.np, 2) and qext.shape == ((w.np + 63) // 64, 4)
        assert np.array_equal(qpts, want_q) and np.array_equal(qext, want_x)
        lo, hi = -(1 << 46), (1 << 46) - 1
        rng = np.random.default_rng(5)
        for n in (2, 63, 64, 65, 200):
            pts = rng.integers(lo, hi + 1, size=(n, 2), dtype=np.int64)
            pts[0], pts[-1] = (lo, hi), (hi, lo)
            h.upload_map(0, pts, np.array([0, n], dtype=np.uint32), np.array([1]), np.array([0]))
            qpts, qext = h.map_prepared(0)
            want_q, want_x = _expect_extents(pts)
            assert np.array_equal(qpts, want_q) and np.array_equal(qext, want_x), n
    finally:
        h.close()
