"""The nearest edge of a map for every point on the device (rj_nearest_query, Handle.nearest_query, ops.NearestLBVH) against
the host twin's brute force over all edges (tests/hosttwin/nearest_twin.cc, held to the plain-Python definition by
tests/test_nearest.py), array for array: the hand cases of tests/nearest_cases.py as a caller's array and as the query
map's vertices; trees of one, two and three levels; the point counts around a wave; "leaf_order" 0 and 1; shuffled points;
any grid; the fuzz over lattices and ring maps with five kinds of point sets, unlimited and with max_dist at the median
distance; rec_dev and dist_dev NULL in every combination with canaries; every refusal with the outputs untouched; the
traversal's visit count; the stage times and the handle's state.  No call may fault: a raised fault word is
RJ_E_INTERNAL, which fails whatever test it appears in."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_cases as NC  # noqa: E402
import nearest_ref as NR  # noqa: E402
from test_nearest import NEAR_DTYPE, check_dist, run_twin, tuples_of, twin_lib  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY32, CANARY_F = 0x5A5A5A5A, -12345.5
TIMES = ["nearest_last_us%d" % k for k in range(3)]
assert _capi.NEAR_DTYPE == NEAR_DTYPE and _capi.MISS_EID == NR.MISS


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


@pytest.fixture(scope="module")
def dctx():
    d = ops.DeviceContext(maps.Context([]), 0)
    yield d
    d.close()


def scaled(pts, row, map_id=0):
    z = np.zeros(len(row) - 1, np.int64)
    return maps.ScaledMap(map_id, np.array(pts, np.int64).reshape(-1, 2), np.array(row, np.uint32), z, z)


def points_map(points):
    """the points as the vertices of a query map: one chain (a chain has two points at least)"""
    p = np.array(points, np.int64).reshape(-1, 2)
    if len(p) < 2:
        p = np.concatenate([p, p])
    return scaled(p, [0, len(p)], 1)


def install(dctx, base, query=None, leaf_order=None):
    """base becomes map 0 with its index, query (or a two-point stand-in) map 1; -> the base's segments in eid order"""
    dctx.ctx.set_map(0, base)
    dctx.ctx.set_map(1, query if query is not None else points_map([(0, 0)]))
    if leaf_order is not None:
        dctx.handle.set_option("leaf_order", leaf_order)
    dctx.LoadToDevice()
    dctx.BuildIndex(0)
    return base.segments()


def levels_of(dctx):
    return [i for i in dctx.handle.get_plan()["index"] if i["map"] == 0][0]["levels"]


def device_nearest(dctx, points=None, n=None, max_dist=None, records=True, dist=True, begin=0):
    """-> (tuples or eids, dist or None) through ops.NearestLBVH: points None = the n vertices of the query map from `begin`"""
    nn = len(points) if points is not None else n
    q = ops.NearestLBVH(dctx)
    q.Init(nn)
    try:
        got_n = q.Query(1, query_points=points, point_range=None if points is not None else (begin, begin + nn), max_dist=max_dist, records=records,
                        dist=dist)
        assert got_n == nn
        eids = q.get_eids()
        if records:
            t = q.exact(q.get_records())
            assert [v[0] for v in t] == eids.tolist() and q.nums() == [v[2] for v in t]
        else:
            with pytest.raises(ValueError):
                q.get_records()
        return (t if records else eids.tolist()), (q.get_dist() if dist else None)
    finally:
        q.free()


def check_against_twin(dctx, twin, seg, points, max_dist=None, as_vertices=False):
    """device == twin, array for array, and dist within 2^-50 of the exact value; -> the tuples"""
    points = np.ascontiguousarray(points, np.int64).reshape(-1, 2)
    want, _ = run_twin(twin, seg, points, -1 if max_dist is None else max_dist)
    got, dist = device_nearest(dctx, None if as_vertices else points, len(points), max_dist)
    assert got == want
    check_dist(got[:300], dist[:300])
    miss = np.array([t[0] == NR.MISS for t in got])
    assert (np.isinf(dist) == miss).all() and (dist[~miss] >= 0).all()
    return got


def base_lattice(G, k, seed):
    return maps.Context([synth.lattice_map(G, k, seed)]).load().maps[0]


def extent(m):
    return m.pts[:, 0].min(), m.pts[:, 1].min(), m.pts[:, 0].max(), m.pts[:, 1].max()


def uniform_points(m, n, rng, grow=0.05):
    """uniform over the map's extent and a little beyond it, inside the scaled range"""
    x0, y0, x1, y1 = (int(v) for v in extent(m))
    gx, gy = int((x1 - x0) * grow), int((y1 - y0) * grow)
    p = np.stack([rng.integers(x0 - gx, x1 + gx, n), rng.integers(y0 - gy, y1 + gy, n)], 1).astype(np.int64)
    return np.clip(p, -(1 << 46), (1 << 46) - 1)


def shrunk(m, shift):
    """the map at 2^-shift of its size around the origin: room for points far outside it"""
    return maps.ScaledMap(m.map_id, m.pts >> shift, m.row_index, m.left, m.right)


# ---- the hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_hand_cases(dctx, twin, name):
    c = NC.HAND[name]
    seg = install(dctx, scaled(c.pts, c.row), points_map(c.points))
    md = None if c.max_dist < 0 else c.max_dist
    for as_vertices in (False, True):
        assert check_against_twin(dctx, twin, seg, c.points, md, as_vertices) == c.want


# ---- tree heights and point counts ---------------------------------------------------------------------------------------
def three_level_lattice():
    k, G = 16, 1
    while 2 * G * (G + 1) * k <= 64 * 4096:  # the smallest lattice with more than 4 096 leaf blocks
        G += 1
    return G, k


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tree_heights(dctx, twin, levels):
    G, k = {1: (2, 5), 2: (12, 16)}.get(levels) or three_level_lattice()
    base = base_lattice(G, k, 5)
    assert {1: base.n_edges <= 64, 2: 4000 < base.n_edges < 6000, 3: base.n_edges > 64 * 4096}[levels]
    rng = np.random.default_rng(levels)
    pts = np.concatenate([uniform_points(base, 1700, rng), base.pts[rng.integers(0, base.n_points, 300)]])
    seg = install(dctx, base, points_map(pts))
    assert levels_of(dctx) == levels
    check_against_twin(dctx, twin, seg, pts)
    check_against_twin(dctx, twin, seg, pts, as_vertices=True)


@functools.lru_cache(maxsize=None)
def mid_map():
    base = base_lattice(12, 16, 5)
    pts = uniform_points(base, 4097, np.random.default_rng(9))
    pts[::7] = base.pts[:len(pts[::7])]  # (some on vertices)
    return base, pts


@pytest.fixture
def mid(dctx):
    """the two-level lattice, installed, with 4 097 points as its query map"""
    base, pts = mid_map()
    return base, install(dctx, base, points_map(pts), leaf_order=1), pts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_point_counts(dctx, twin, mid, n):
    _, seg, pts = mid
    check_against_twin(dctx, twin, seg, pts[:n])
    check_against_twin(dctx, twin, seg, pts[:n], as_vertices=True)


def test_any_grid_and_stage_times(dctx, twin, mid):
    _, seg, pts = mid
    h = dctx.handle
    want = check_against_twin(dctx, twin, seg, pts)
    us = [h.get_option(t) for t in TIMES]
    assert all(v >= 0 for v in us) and us[2] >= us[1]
    try:
        for blocks in (1, 3, 17):
            h.set_debug_option("nearest_blocks", blocks)
            assert device_nearest(dctx, pts)[0] == want
    finally:
        h.set_debug_option("nearest_blocks", 0)


def test_shuffled_points_give_the_permuted_outputs(dctx, twin, mid):
    _, seg, pts = mid
    pts = pts[:4096]
    perm = np.random.default_rng(3).permutation(len(pts))
    a, da = device_nearest(dctx, pts)
    b, db = device_nearest(dctx, pts[perm])
    assert [a[i] for i in perm] == b and (da[perm] == db).all()
    assert a == run_twin(twin, seg, pts)[0]


def test_leaf_order_does_not_change_the_result(dctx, twin):
    base = base_lattice(12, 16, 6)
    pts = uniform_points(base, 1500, np.random.default_rng(4))
    got = []
    try:
        for lo in (0, 1):
            seg = install(dctx, base, points_map(pts), leaf_order=lo)
            got.append(check_against_twin(dctx, twin, seg, pts))
            got.append(check_against_twin(dctx, twin, seg, pts, max_dist=1 << 36, as_vertices=True))
    finally:
        dctx.handle.set_option("leaf_order", 1)
    assert got[0] == got[2] and got[1] == got[3]


# ---- fuzz ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(dctx, twin, seed):
    rng = np.random.default_rng(100 + seed)
    if seed % 2 == 0:
        G = int(rng.integers(14, 22))
        g = synth.lattice_map(G, int(rng.integers(10, 20)), seed)
    else:
        g = synth.ring_map(int(rng.integers(200, 600)), int(rng.integers(6000, 18000)), seed)
    base = shrunk(maps.Context([g]).load().maps[0], 4)
    assert 5000 <= base.n_edges <= 20000
    n = 4096
    x0, y0, x1, y1 = (int(v) for v in extent(base))
    segs = base.segments()
    pick = rng.integers(0, len(segs), n)
    sets = {
        "vertices": base.pts[rng.integers(0, base.n_points, n)],
        "midpoints": np.stack([(segs[pick, 0] + segs[pick, 2]) // 2, (segs[pick, 1] + segs[pick, 3]) // 2], 1),
        "uniform": uniform_points(base, n, rng),
        "far_outside": np.stack([rng.integers(x1 + 3 * (x1 - x0), x1 + 4 * (x1 - x0), n), rng.integers(y0 - 2 * (y1 - y0), y0 - (y1 - y0), n)], 1),
        "vertical_line": np.stack([np.full(n, (x0 + x1) // 2), rng.integers(y0, y1, n)], 1),
    }
    assert all(abs(int(v)) < (1 << 46) for p in sets.values() for v in (p.min(), p.max()))
    install(dctx, base)
    for name, pts in sets.items():
        pts = np.ascontiguousarray(pts, np.int64)
        got = check_against_twin(dctx, twin, segs, pts)
        if name == "vertices":
            assert all(NR.d2_of(*t[1:]) == 0 for t in got[:200])
        d = sorted(NR.d2_of(*t[1:]) for t in got)
        median = math.isqrt(math.ceil(d[n // 2]) - 1) + 1 if d[n // 2] > 0 else 0  # the median distance, rounded up
        limited = check_against_twin(dctx, twin, segs, pts, max_dist=median)
        misses = sum(t[0] == NR.MISS for t in limited)
        # (about half miss; fewer where many distances are equal or below one unit: the vertices, the rounded midpoints)
        assert misses <= n // 2 and (name in ("vertices", "midpoints") or misses > n // 4), (name, misses)


# ---- the ordering that finds no memory ---------------------------------------------------------------------------------
def test_fallback_to_the_given_order(dctx, twin, mid):
    """the ordering of Y fails (as without memory): Y is taken as given and not tried again; a PIP query over another, shorter
    caller array X in between leaves nothing of its order behind for the next query over Y"""
    _, seg, pts = mid
    h = dctx.handle
    perm = np.random.default_rng(5).permutation(4096)
    y_host, x_host = np.ascontiguousarray(pts[:4096][perm]), np.ascontiguousarray(pts[:1000][::-1])
    want = run_twin(twin, seg, y_host)[0]
    Y, X = h.alloc(16 * 4096).from_host(y_host), h.alloc(16 * 1000).from_host(x_host)
    eid, rec, closest = h.alloc(4 * 4096), h.alloc(40 * 4096), h.alloc(4 * 4096)
    try:
        h.set_debug_option("nearest_order_nomem", 1)
        h.nearest_query(0, 1, Y, 0, 4096, eid, rec)
        h.set_debug_option("nearest_order_nomem", 0)
        assert tuples_of(rec.to_host(NEAR_DTYPE)) == want
        for _ in range(3):
            h.pip_query(0, 1, X, 0, 1000, closest)
            rec.from_host(np.zeros(4096, NEAR_DTYPE))
            h.nearest_query(0, 1, Y, 0, 4096, eid, rec)  # remembered: the given order, whatever the PIP query left
            assert tuples_of(rec.to_host(NEAR_DTYPE)) == want
            assert h.get_plan()["pip"]["points"] == 1000
        h.nearest_query(0, 1, X, 0, 1000, eid, rec)  # another array is ordered as usual
        assert tuples_of(rec.to_host(NEAR_DTYPE, 1000)) == run_twin(twin, seg, x_host)[0]
    finally:
        h.set_debug_option("nearest_order_nomem", 0)
        for b in (Y, X, eid, rec, closest):
            b.free()


# ---- the optional outputs ------------------------------------------------------------------------------------------------
def test_null_records_and_dist_in_every_combination(dctx, twin, mid):
    _, seg, pts = mid
    h = dctx.handle
    n = 200
    pts = pts[:n]
    want, _ = run_twin(twin, seg, pts, 1 << 40)
    src = h.alloc(16 * n).from_host(pts)
    eid, rec, dist = h.alloc(4 * (n + 4)), h.alloc(40 * (n + 4)), h.alloc(8 * (n + 4))
    try:
        for with_rec in (False, True):
            for with_dist in (False, True):
                eid.from_host(np.full(n + 4, CANARY32, np.uint32))
                rec.from_host(np.full(10 * (n + 4), CANARY32, np.uint32))
                dist.from_host(np.full(n + 4, CANARY_F))
                h.nearest_query(0, 1, src, 0, n, eid, rec if with_rec else None, dist if with_dist else None, max_dist=1 << 40)
                e, r, d = eid.to_host(np.uint32), rec.to_host(NEAR_DTYPE), dist.to_host(np.float64)
                assert e[:n].tolist() == [t[0] for t in want] and (e[n:] == CANARY32).all()
                assert (r.view(np.uint32)[10 * n:] == CANARY32).all() and (d[n:] == CANARY_F).all()
                assert tuples_of(r[:n]) == want if with_rec else (r.view(np.uint32) == CANARY32).all()
                if with_dist:
                    check_dist(want, d[:n])
                else:
                    assert (d == CANARY_F).all()
    finally:
        for b in (src, eid, rec, dist):
            b.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dctx, mid):
    base, _, pts = mid
    h = dctx.handle
    n = 100
    src = h.alloc(16 * n).from_host(pts[:n])
    eid, rec, dist = h.alloc(4 * n), h.alloc(40 * n), h.alloc(8 * n)
    eid.from_host(np.full(n, CANARY32, np.uint32))
    rec.from_host(np.full(10 * n, CANARY32, np.uint32))
    dist.from_host(np.full(n, CANARY_F))
    np_query = dctx.ctx.get_map(1).n_points
    plan, options = h.get_plan(), [h.get_option(o) for o in ("leaf_order", "stats", "query_order")]
    bad = [
        dict(base=0, query=0), dict(base=2, query=1), dict(base=-1, query=0), dict(base=1, query=1),
        dict(base=1, query=0),                       # map 1 has no index
        dict(eid=None),                              # a null eid_dev with n > 0
        dict(pts=None, begin=np_query - n + 1),      # a range that leaves the query map
        dict(pts=None, begin=np_query + 5),
        dict(pts=None, begin=(1 << 64) - 50),        # ... and one whose end wraps
        dict(max_dist=(1 << 48) + 1),
        dict(n=1 << 32), dict(pts=None, begin=0, n=1 << 32),  # n >= 2^32
    ]
    try:
        for kw in bad:
            with pytest.raises(_capi.RayJoinError) as ei:
                h.nearest_query(kw.get("base", 0), kw.get("query", 1), kw.get("pts", src), kw.get("begin", 0), kw.get("n", n), kw.get("eid", eid), rec, dist,
                                max_dist=kw.get("max_dist", -1))
            assert ei.value.code == _capi.RJ_E_INVALID and "rj_nearest_query" in str(ei.value), kw
            assert (eid.to_host(np.uint32) == CANARY32).all() and (rec.to_host(np.uint32) == CANARY32).all() and (dist.to_host(np.float64) == CANARY_F).all()
            assert h.get_option(TIMES[2]) == -1
        # n == 0 is fine and writes nothing, whatever the pointers are
        h.nearest_query(0, 1, src, 0, 0, None, None, None)
        h.nearest_query(0, 1, None, np_query, 0, eid, rec, dist)
        assert (eid.to_host(np.uint32) == CANARY32).all() and (rec.to_host(np.uint32) == CANARY32).all() and (dist.to_host(np.float64) == CANARY_F).all()
        # the largest max_dist is accepted; the handle is what it was
        h.nearest_query(0, 1, src, 0, n, eid, rec, dist, max_dist=1 << 48)
        assert (eid.to_host(np.uint32) != CANARY32).all()
        assert h.get_plan() == plan and [h.get_option(o) for o in ("leaf_order", "stats", "query_order")] == options
    finally:
        for b in (src, eid, rec, dist):
            b.free()


# ---- a traversal, not a scan -------------------------------------------------------------------------------------------
def test_the_traversal_prunes(dctx, twin):
    base = base_lattice(22, 16, 8)
    assert base.n_edges >= 16000
    seg = install(dctx, base, scaled(base.pts, base.row_index, 1))
    h = dctx.handle
    h.set_option("stats", 1)
    try:
        got, _ = device_nearest(dctx, None, base.n_points)
        s = h.last_stats_raw()
    finally:
        h.set_option("stats", 0)
    assert got == run_twin(twin, seg, base.pts)[0] and all(NR.d2_of(*t[1:]) == 0 for t in got[::50])
    leaf_visits, exact, nodes = s[0], s[1], s[2]
    print("leaf visits %d (%.2f per point), exact evaluations %d (%.2f per point), nodes expanded %d" %
          (leaf_visits, leaf_visits / base.n_points, exact, exact / base.n_points, nodes))
    assert exact >= base.n_points and nodes > 0
    # no fault: the call returned without RJ_E_INTERNAL (it would have raised), its stages were timed, the next call is fine
    assert h.get_option(TIMES[2]) >= 0 and h.get_option(TIMES[1]) >= 0
    assert device_nearest(dctx, base.pts[:100])[0] == got[:100]
    assert leaf_visits * 64 < base.n_points * base.n_edges / 8, (leaf_visits, base.n_points, base.n_edges)
