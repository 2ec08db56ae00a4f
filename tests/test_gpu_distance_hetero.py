"""rj_nearest_query and rj_within_query on the device over the inputs of tests/distance_cases.py, against the host twins
(held to the Python definition on the same inputs by tests/test_distance_hetero.py), array for array -- eids, the 40-byte
records, dist within 2^-50 on a sample, and for within the offsets, the counts, n_points_hit and max_per_point: every
heterogeneous family of tests/skewed_pairs.py, both bases, every point set (the `vertices` as a range of the query map that
begins off a wave's border, the others as caller arrays), unlimited and with max_dist at the median distance, every query
twice; within at 0, at the median, at one large distance per family, on the whole knot of `outlier` and on every pair of
`long_long`, with the capacity that just fits and the overflow one short of it; the near-tie and the exact-tie fan in
every lane of a wave under both leaf orders and grids of 1 and 3 blocks; ranges of equal length and different begin, and a
PIP query in between, on one handle's caches; within's lists against nearest's answer.  Nothing here lowers a stack
capacity or provokes a fault: the refusals stay in tests/test_gpu_nearest.py and tests/test_gpu_within.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distance_cases as DC  # noqa: E402
import nearest_ref as NR  # noqa: E402
import skewed_pairs as S  # noqa: E402
import test_nearest as TN  # noqa: E402
import test_within as TW  # noqa: E402
from test_gpu_nearest import device_nearest, install, points_map, scaled  # noqa: E402
from test_gpu_within import Buffers, device_answer, lists_of, same  # noqa: E402
from test_nearest import check_dist, tuples_of  # noqa: E402

pytestmark = pytest.mark.gpu

PAIR_LIMIT = 1 << 21   # pairs of a within call at most: the points are cut, never the distance
FAMILY_BASES = [(name, base) for name in S.NAMES for base in (0, 1)]
IDS = ["%s-%d" % fb for fb in FAMILY_BASES]
SCENES = [("tie", "single"), ("tie", "replicated"), ("equal", "single"), ("equal", "replicated")]


@pytest.fixture(scope="module")
def near():
    return TN.twin_lib()


@pytest.fixture(scope="module")
def wtwin():
    return TW.twin_lib()


@pytest.fixture(scope="module")
def dctx():
    d = ops.DeviceContext(maps.Context([]), 0)
    yield d
    d.close()


def as_map(m, map_id):
    return maps.ScaledMap(map_id, m.pts, m.row_index, m.left, m.right)


def install_family(dctx, name, base):
    ctx, seg, sets = DC.family_sets(name, base)
    install(dctx, as_map(ctx.maps[base], 0), as_map(ctx.maps[1 - base], 1), leaf_order=1)
    return ctx, seg, sets


_nearest_want = {}


def nearest_want(near, name, base, k):
    """the nearest twin's unlimited answer for a set, once: (points, tuples, dist, the median distance rounded up)"""
    if (name, base, k) not in _nearest_want:
        ctx, seg, sets = DC.family_sets(name, base)
        pts = np.ascontiguousarray(DC.points_of(ctx, base, sets, k))
        t, d = TN.run_twin(near, seg, pts)
        _nearest_want[name, base, k] = (pts, t, d, DC.median_up(d))
    return _nearest_want[name, base, k]


def how_of(sets, k, pts, m=None):
    """the arguments that send a set to the device: a range of the query map for `vertices`, else the caller's array"""
    m = len(pts) if m is None else m
    return dict(points=None, n=m, begin=sets[k][0]) if k == "vertices" else dict(points=pts[:m])


def check_nearest(got, dist, want):
    assert got == want
    pick = np.unique(np.linspace(0, len(want) - 1, 64).astype(np.int64))
    check_dist([got[i] for i in pick], dist[pick])
    miss = np.array([t[0] == NR.MISS for t in got])
    assert (np.isinf(dist) == miss).all() and (dist[~miss] >= 0).all()


def within_want(wtwin, seg, pts, md):
    """the within twin's answer on as many of the points, from the first, as keep the call within PAIR_LIMIT pairs"""
    rc, counts, off, *_ = TW.call_twin(wtwin, seg, pts, md, capacity=0)
    assert rc in (TW.OK, TW.OVERFLOW)
    m = int(np.searchsorted(off.astype(np.int64), PAIR_LIMIT, side="right")) - 1
    assert m >= 1
    if m < len(pts):
        pts = pts[:m]
    rc, counts, off, eid, rec, dist, _ = TW.call_twin(wtwin, seg, pts, md, capacity=int(off[m]))
    assert rc == TW.OK and 0 <= counts[0] <= PAIR_LIMIT
    return m, dict(off=off, eid=eid, rec=rec, dist=dist, counts=dict(zip(_capi.WITHIN_COUNTS, counts)))


# ---- nearest: every family, both bases, every point set ----------------------------------------------------------------------
@pytest.mark.parametrize("name,base", FAMILY_BASES, ids=IDS)
def test_nearest_on_a_family(dctx, near, name, base):
    ctx, seg, sets = install_family(dctx, name, base)
    points = 0
    for k in sets:
        pts, unlimited, dist, median = nearest_want(near, name, base, k)
        limited = TN.run_twin(near, seg, pts, median)[0]
        misses = sum(t[0] == NR.MISS for t in limited)
        assert misses <= len(pts) // 2   # (the median's definition; fewer where distances are equal: 0 on the base's vertices)
        for md, want in ((None, unlimited), (median, limited)):
            for rep in range(2):   # (the second goes by whatever ordering the first cached)
                got, d = device_nearest(dctx, max_dist=md, **how_of(sets, k, pts))
                check_nearest(got, d, want)
                points += len(pts)
    print("COVER nearest %s base %d: %d edges, %d sets, %d points" % (name, base, len(seg), len(sets), points))


# ---- within: the same sets ---------------------------------------------------------------------------------------------------
def fill_and_overflow(dctx, sets, k, pts, md, want):
    """one filling call with the capacity exactly n_pairs and one overflow call one short of it, on the raw handle with
    canaries: the first fills everything and nothing behind it, the second gives the true counts and offsets and leaves the
    pair arrays alone"""
    h = dctx.handle
    n, n_pairs = len(pts), want["counts"]["n_pairs"]
    src = None if k == "vertices" else h.alloc(16 * n).from_host(pts)
    begin = sets[k][0] if k == "vertices" else 0
    B = Buffers(h, n, n_pairs)
    try:
        counts = h.within_query(0, 1, src, begin, n, md, n_pairs, B.off, B.eid, B.rec, B.dist)
        off, e, r, d = B.host()
        assert counts == want["counts"] and np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == 0x5A5A5A5A5A5A5A5A
        assert np.array_equal(e[:n_pairs], want["eid"]) and np.array_equal(r[:n_pairs], want["rec"]) and B.pairs_untouched(n_pairs)
        check_dist(tuples_of(r[:64]), d[:64])
        B.fill()
        with pytest.raises(_capi.WithinOverflow) as ei:
            h.within_query(0, 1, src, begin, n, md, n_pairs - 1, B.off, B.eid, B.rec, B.dist)
        assert ei.value.code == _capi.RJ_E_OVERFLOW and ei.value.counts == want["counts"]
        off = B.host()[0]
        assert np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == 0x5A5A5A5A5A5A5A5A and B.pairs_untouched()
    finally:
        if src is not None:
            src.free()
        B.free()


def within_calls(near, wtwin, name, base):
    """-> (set, label, max_dist, m, the twin's answer on the first m points) of every within call of a family, with the
    conditions on the twin's answer asserted: a set that tests nothing fails here, before the device is asked"""
    ctx, seg, sets = DC.family_sets(name, base)
    long_ones = set(DC.long_edges(ctx.maps[base]).tolist())
    for k in sets:
        pts, _, _, median = nearest_want(near, name, base, k)
        radii = [("median", median), ("large", DC.LARGE[name])]
        if k == "on_base":
            radii.append(("zero", 0))
        if k == "knot":
            radii += [("knot units", DC.KNOT_DIST[0]), ("knot cells", DC.KNOT_DIST[1])]
        if name == "long_long" and k == "shuffled":
            radii.append(("everything", 1 << 48))
        for label, md in radii:
            m, want = within_want(wtwin, seg, pts[:65] if label == "everything" else pts, md)
            off = want["off"].astype(np.int64)
            lens = np.diff(off)
            n_pairs = want["counts"]["n_pairs"]
            assert 1 <= n_pairs <= PAIR_LIMIT, (k, label, n_pairs)
            if label == "zero":   # the edges that meet the vertex (several, except on long_long's free-standing segments)
                assert (lens[:len(lens) // 2] >= 1).all() and ((lens >= 2).any() or name == "long_long")
            elif label == "median":
                assert n_pairs > 1 and (m < len(pts) or (lens > 0).sum() > m // 2)
            elif label == "large" and k == "along_long_edges":
                assert np.mean([bool(long_ones & set(want["eid"][off[i]:off[i + 1]].tolist())) for i in range(m)]) >= 0.9
            elif label == "knot cells":   # every point lists the whole knot
                knot = DC.knot_edges(ctx, ctx.maps[base])
                assert m == len(pts) and want["counts"]["max_per_point"] >= lens.min() >= len(knot) > 800 and (base == 1 or len(knot) > 1000)
                assert all(np.isin(knot, want["eid"][off[i]:off[i + 1]]).all() for i in range(0, m, 37))
            elif label == "everything":
                assert m == 65 and want["counts"] == dict(n_pairs=65 * len(seg), n_points_hit=65, max_per_point=len(seg))
            yield k, label, md, m, want


@pytest.mark.parametrize("name,base", FAMILY_BASES, ids=IDS)
def test_within_on_a_family(dctx, near, wtwin, name, base):
    ctx, seg, sets = install_family(dctx, name, base)
    points = pairs = 0
    for k, label, md, m, want in within_calls(near, wtwin, name, base):
        pts = nearest_want(near, name, base, k)[0]
        same(device_answer(dctx, max_dist=md, **how_of(sets, k, pts, m)), want)
        if label == "median":
            fill_and_overflow(dctx, sets, k, pts[:m], md, want)
        points += m
        pairs += want["counts"]["n_pairs"]
    print("COVER within %s base %d: %d edges, %d sets, %d points, %d pairs" % (name, base, len(seg), len(sets), points, pairs))


# ---- the fans: the wide compare in every lane --------------------------------------------------------------------------------
def scene(kind, how):
    rng = np.random.default_rng(50 + SCENES.index((kind, how)))   # (the scenes of tests/test_distance_hetero.py)
    return DC.single_scene(kind, rng) if how == "single" else DC.replicated_scene(kind, rng)


@pytest.mark.parametrize("kind,how", SCENES, ids=["%s-%s" % s for s in SCENES])
def test_fans(dctx, near, wtwin, kind, how):
    sc = scene(kind, how)
    pts = np.ascontiguousarray(sc.points)
    n = len(pts)
    assert n >= 64
    base, query = scaled(sc.pts, sc.row), points_map(pts)
    seg = base.segments()
    want, _ = TN.run_twin(near, seg, pts)
    for i, t in enumerate(want):   # (the twin's edge is one of the centre's own fan; the smallest eid of an equal fan)
        own = sc.fan_eids[i % len(sc.fans)]
        assert t[0] in own and (kind == "tie" or t[0] == own.min())
    fan = sc.fans[0]
    m = fan.m or fan.h + 1
    lists = {md: within_want(wtwin, seg, pts, md)[1] for md in (m - 1, m, m + 1)}
    for md, w in lists.items():   # none, all, all
        assert np.array_equal(np.diff(w["off"].astype(np.int64)), [0 if md == m - 1 else len(sc.fan_eids[i % len(sc.fans)]) for i in range(n)])
    h = dctx.handle
    try:
        for lo in (0, 1):
            install(dctx, base, query, leaf_order=lo)
            for blocks in (0, 1, 3):
                h.set_debug_option("nearest_blocks", blocks)
                h.set_debug_option("within_blocks", blocks)
                for as_vertices in (False, True):
                    where = dict(points=None, n=n) if as_vertices else dict(points=pts)
                    got, d = device_nearest(dctx, **where)
                    check_nearest(got, d, want)
                    for md, w in lists.items():
                        same(device_answer(dctx, max_dist=md, **where), w)
    finally:
        h.set_debug_option("nearest_blocks", 0)
        h.set_debug_option("within_blocks", 0)
        h.set_option("leaf_order", 1)


# ---- ranges and the caches that the queries share on one handle ----------------------------------------------------------------
def test_ranges_and_shared_caches_on_one_handle(dctx, near, wtwin, oracle):
    """the query map is a shuffled vertex set, so every range of more than 64 of its vertices is incoherent and goes through
    a Morton permutation that the handle keeps under (begin, n) -- for the distance queries and PIP alike"""
    ctx = S.family("skew_lattice")
    bm = ctx.maps[0]
    q = ctx.maps[1].pts[np.random.default_rng(77).permutation(ctx.maps[1].n_points)[:3000]]
    seg = install(dctx, as_map(bm, 0), points_map(q), leaf_order=1)
    h = dctx.handle
    n, b, b2 = 1000, 37, 1003
    md = DC.median_up(TN.run_twin(near, seg, q[b:b + n])[1])

    def nearest_over(begin, m):
        got, d = device_nearest(dctx, None, m, begin=begin)
        assert h.get_option("query_last_ordered") == 1
        check_nearest(got, d, TN.run_twin(near, seg, q[begin:begin + m])[0])
    nearest_over(b, n)
    nearest_over(b2, n)    # the same length at another begin: the cached order of [b, b + n) is not this range's
    nearest_over(b, n)
    same(device_answer(dctx, None, n, md, begin=b), within_want(wtwin, seg, q[b:b + n], md)[1])
    assert h.get_option("query_last_ordered") == 1
    same(device_answer(dctx, None, n, md, begin=b2), within_want(wtwin, seg, q[b2:b2 + n], md)[1])
    # a PIP query over the same range, then nearest again
    ob = oracle.Map(bm.pts, bm.row_index, bm.left, bm.right)
    pip = ops.PIPLBVH(dctx)
    pip.Init(n)
    try:
        for begin in (b, b2, b):
            pip.Query(1, point_range=(begin, begin + n))
            assert np.array_equal(pip.get_closest_eids(), oracle.pip_brute(ob, 1, np.ascontiguousarray(q[begin:begin + n])))
            nearest_over(begin, n)
    finally:
        pip.closest.free()
        pip.faces.free()
    # ranges that end at the last vertex: the same length, and another one
    nearest_over(len(q) - n, n)
    nearest_over(len(q) - 777, 777)
    same(device_answer(dctx, None, 777, md, begin=len(q) - 777), within_want(wtwin, seg, q[len(q) - 777:], md)[1])
    nearest_over(1, len(q) - 1)


# ---- within's lists against nearest's answer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", [("rings_frame", 0), ("outlier", 1)])
def test_within_contains_nearest(dctx, near, name, base):
    """the list at max_dist d holds nearest's eid exactly for the points whose nearest distance is <= d, and its first entry
    of the smallest distance is that eid"""
    ctx, seg, sets = install_family(dctx, name, base)
    checked = 0
    for k in ("shuffled", "random", "along_long_edges"):
        pts, _, _, median = nearest_want(near, name, base, k)
        pts = pts[:300]
        got = device_answer(dctx, pts, max_dist=median)
        nearest, _ = device_nearest(dctx, pts)
        lists = lists_of(got)
        for row, t in zip(lists, nearest):
            inside = NR.d2_of(*t[1:]) <= median * median
            assert (t in row) == inside and (t[0] in [r[0] for r in row]) == inside
            if row:
                assert t == min(row, key=lambda r: (NR.d2_of(*r[1:]), r[0]))
                checked += 1
        assert any(not row for row in lists) or k == "along_long_edges"
    assert checked > 300
