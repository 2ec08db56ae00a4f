"""The k nearest edges of a map for every point on the device (rj_knearest_query, Handle.knearest_query, ops.KNearestLBVH)
against the host twin's brute force over all edges (tests/hosttwin/knearest_twin.cc, held to the plain-Python definition by
tests/test_knearest.py), array for array -- the counts, the eids, the 40-byte records, and dist within 2^-50 on a sample:
the hand cases as a caller's array and as the query map's vertices; trees of one, two and three levels; the point counts
around a wave; k from 1 to 32; k = 1 against rj_nearest_query bit for bit; max_dist at the median distance under grids of
1, 3 and 17 blocks (one block: a single wave re-uses its slab over every group); shuffled points; "leaf_order" 0 and 1; a
fuzz over lattices and ring maps; two heterogeneous families and the replicated fans of tests/distance_cases.py at k = 17;
consistency with rj_within_query on device outputs alone; every output NULL in every combination with canaries; every
refusal with the outputs untouched; the traversal's visit count.  No call may fault: a raised fault word is
RJ_E_INTERNAL, which fails whatever test it appears in."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distance_cases as DC  # noqa: E402
import nearest_cases as NC  # noqa: E402
import nearest_ref as NR  # noqa: E402
import test_knearest as TK  # noqa: E402
from test_gpu_nearest import (base_lattice, extent, install, levels_of, mid_map, points_map, scaled, shrunk, three_level_lattice,  # noqa: E402
                              uniform_points)
from test_nearest import NEAR_DTYPE, check_dist, tuples_of  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY32, CANARY_F = 0x5A5A5A5A, -12345.5
TIMES = ["knearest_last_us%d" % k for k in range(3)]
assert _capi.KNEAREST_MAX_K == 32


@pytest.fixture(scope="module")
def twin():
    return TK.twin_lib()


@pytest.fixture(scope="module")
def dctx():
    d = ops.DeviceContext(maps.Context([]), 0)
    yield d
    d.close()


@pytest.fixture
def mid(dctx):
    """the two-level lattice of tests/test_gpu_nearest.py, installed, with 4 097 points as its query map"""
    base, pts = mid_map()
    return base, install(dctx, base, points_map(pts), leaf_order=1), pts


def device_knearest(dctx, k, points=None, n=None, max_dist=None, records=True, dist=True, begin=0):
    """-> TK.Answer through ops.KNearestLBVH: points None = the n vertices of the query map from `begin`"""
    nn = len(points) if points is not None else n
    q = ops.KNearestLBVH(dctx)
    q.Init(nn, k)
    try:
        got_n = q.Query(1, query_points=points, point_range=None if points is not None else (begin, begin + nn), max_dist=max_dist, records=records, dist=dist)
        assert got_n == nn
        a = TK.Answer(q.get_counts(), q.get_eids(), q.get_records() if records else None, q.get_dist() if dist else None, None)
        assert a.eid.shape == (nn, k) and a.count.shape == (nn,)
        indptr, flat = q.to_csr()
        assert indptr[-1] == a.count.sum() == len(flat) and np.array_equal(flat, a.eid[a.eid != NR.MISS])
        if records and nn:
            assert q.exact(a.rec[:1])[0] == tuples_of(a.rec[0])
        return a
    finally:
        q.free()


def same(got, want, sample=40):
    """device == twin, array for array; dist within 2^-50 of the exact value on a sample of rows"""
    assert np.array_equal(got.count, want.count)
    assert np.array_equal(got.eid, want.eid)
    if got.rec is not None:
        assert np.array_equal(got.rec, want.rec)
    if got.dist is not None:
        assert np.array_equal(np.isinf(got.dist), want.eid == NR.MISS) and (got.dist >= 0).all()
        for i in np.unique(np.linspace(0, len(want.count) - 1, sample).astype(np.int64)):
            check_dist(tuples_of(want.rec[i, :want.count[i]]), got.dist[i, :want.count[i]])


def check_against_twin(dctx, twin, seg, points, k, max_dist=None, as_vertices=False, begin=0):
    points = np.ascontiguousarray(points, np.int64).reshape(-1, 2)
    want = TK.run_twin(twin, seg, points, k, -1 if max_dist is None else max_dist)
    TK.rows_of(want)
    got = device_knearest(dctx, k, None if as_vertices else points, len(points), max_dist, begin=begin)
    same(got, want)
    return got


def median_of(twin, seg, pts):
    """the median of the nearest distances, rounded up: about half of the points have no edge within it"""
    return DC.median_up(TK.run_twin(twin, seg, pts, 1).dist[:, 0])


# ---- the hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.HAND))
def test_hand_cases(dctx, twin, name):
    c = NC.HAND[name]
    seg = install(dctx, scaled(c.pts, c.row), points_map(c.points))
    md = None if c.max_dist < 0 else c.max_dist
    for k in TK.KS:
        for as_vertices in (False, True):
            got = check_against_twin(dctx, twin, seg, c.points, k, md, as_vertices)
            assert [tuples_of(got.rec[i, :1])[0] if got.count[i] else NC.MISS for i in range(len(c.points))] == c.want


def test_fewer_edges_than_k_and_the_hub(dctx, twin):
    c = TK.hub_case()
    seg = install(dctx, scaled(c.pts, c.row), points_map(c.points))
    got = check_against_twin(dctx, twin, seg, c.points, 5)
    assert got.eid[0].tolist() == [1, 2, 3, 4, 5]
    got = check_against_twin(dctx, twin, seg, c.points, 32, as_vertices=True)
    assert (got.count == 13).all() and (got.eid[:, 13:] == NR.MISS).all()


# ---- tree heights, point counts, k ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tree_heights(dctx, twin, levels):
    G, k = {1: (2, 5), 2: (12, 16)}.get(levels) or three_level_lattice()
    base = base_lattice(G, k, 5)
    rng = np.random.default_rng(levels)
    pts = np.concatenate([uniform_points(base, 1700, rng), base.pts[rng.integers(0, base.n_points, 300)]])
    seg = install(dctx, base, points_map(pts))
    assert levels_of(dctx) == levels
    check_against_twin(dctx, twin, seg, pts, 4)
    check_against_twin(dctx, twin, seg, pts, 4, as_vertices=True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_point_counts(dctx, twin, mid, n):
    _, seg, pts = mid
    check_against_twin(dctx, twin, seg, pts[:n], 3)
    check_against_twin(dctx, twin, seg, pts[:n], 3, as_vertices=True)


@pytest.mark.parametrize("k", [1, 2, 8, 31, 32])
def test_every_k(dctx, twin, mid, k):
    _, seg, pts = mid
    got = check_against_twin(dctx, twin, seg, pts, k)
    assert (got.count == k).all()
    us = [dctx.handle.get_option(t) for t in TIMES]
    assert all(v >= 0 for v in us) and us[2] >= us[1]


def test_k_1_is_rj_nearest_query_bit_for_bit(dctx, twin, mid):
    _, seg, pts = mid
    h = dctx.handle
    n = len(pts)
    src = h.alloc(16 * n).from_host(pts)
    bufs = [h.alloc(4 * n), h.alloc(40 * n), h.alloc(8 * n), h.alloc(4 * n), h.alloc(40 * n), h.alloc(8 * n), h.alloc(4 * n)]
    e1, r1, d1, ek, rk, dk, ck = bufs
    try:
        for md in (-1, median_of(twin, seg, pts)):
            for b in bufs:
                b.from_host(np.full(b.nbytes // 4, CANARY32, np.uint32))
            h.nearest_query(0, 1, src, 0, n, e1, r1, d1, max_dist=md)
            h.knearest_query(0, 1, src, 0, n, 1, ek, ck, rk, dk, max_dist=md)
            for a, b in ((e1, ek), (r1, rk), (d1, dk)):
                assert np.array_equal(a.to_host(np.uint32), b.to_host(np.uint32))
            count = ck.to_host(np.uint32)
            assert np.array_equal(count, (ek.to_host(np.uint32) != NR.MISS).astype(np.uint32))
            assert set(count.tolist()) == ({1} if md < 0 else {0, 1})
    finally:
        for b in [src] + bufs:
            b.free()


# ---- counts from 0 to k within one call, on any grid ---------------------------------------------------------------------
def test_median_distance_on_any_grid(dctx, twin, mid):
    """with "knearest_blocks" 1 a single block's four waves take every group in turn and re-use their slabs: a stale slot
    would show as a wrong row"""
    _, seg, pts = mid
    h = dctx.handle
    k = 6
    md = 2 * median_of(twin, seg, pts)
    want = TK.run_twin(twin, seg, pts, k, md)
    assert {0, k} <= set(want.count.tolist()) and len(set(want.count.tolist())) >= 4, sorted(set(want.count.tolist()))
    same(device_knearest(dctx, k, pts, max_dist=md), want)
    try:
        for blocks in (1, 3, 17):
            h.set_debug_option("knearest_blocks", blocks)
            same(device_knearest(dctx, k, pts, max_dist=md), want)
            same(device_knearest(dctx, k, None, len(pts), max_dist=md), want)
        h.set_debug_option("knearest_blocks", 1)  # (... and a k that changes between two calls over the same slab size rule)
        for kk in (32, 1, 17):
            same(device_knearest(dctx, kk, pts, max_dist=md), TK.run_twin(twin, seg, pts, kk, md))
    finally:
        h.set_debug_option("knearest_blocks", 0)


def test_the_scratch_goes_by_the_grid_and_k_not_by_n(dctx, mid):
    """3072 k bytes per wave of the grid (64 lists of k slots of 48 bytes), four waves per block"""
    _, _, pts = mid
    h = dctx.handle
    try:
        for blocks in (3, 5):
            h.set_debug_option("knearest_blocks", blocks)
            for k in (1, 16):
                for n in (blocks * 256, 2000, 4097):
                    device_knearest(dctx, k, pts[:n])
                    assert h.get_option("knearest_last_scratch_bytes") == blocks * 4 * 3072 * k
    finally:
        h.set_debug_option("knearest_blocks", 0)
    device_knearest(dctx, 16, pts)  # by size: a block per four groups here, never more than the resident blocks of the chip
    assert h.get_option("knearest_last_scratch_bytes") == ((4097 + 255) // 256) * 4 * 3072 * 16
    with pytest.raises(_capi.RayJoinError):
        h.knearest_query(0, 1, None, 0, 10, 0, None)
    assert h.get_option("knearest_last_scratch_bytes") == 0


def test_shuffled_points_give_the_permuted_rows(dctx, twin, mid):
    _, seg, pts = mid
    pts = pts[:4096]
    perm = np.random.default_rng(3).permutation(len(pts))
    a = device_knearest(dctx, 5, pts)
    b = device_knearest(dctx, 5, pts[perm])
    assert np.array_equal(a.count[perm], b.count) and np.array_equal(a.eid[perm], b.eid) and np.array_equal(a.rec[perm], b.rec)
    assert np.array_equal(a.dist[perm], b.dist)
    same(a, TK.run_twin(twin, seg, pts, 5))


def test_leaf_order_does_not_change_the_result(dctx, twin):
    base = base_lattice(12, 16, 6)
    pts = uniform_points(base, 1500, np.random.default_rng(4))
    got = []
    try:
        for lo in (0, 1):
            seg = install(dctx, base, points_map(pts), leaf_order=lo)
            got.append(check_against_twin(dctx, twin, seg, pts, 7))
            got.append(check_against_twin(dctx, twin, seg, pts, 7, max_dist=1 << 36, as_vertices=True))
    finally:
        dctx.handle.set_option("leaf_order", 1)
    for a, b in ((got[0], got[2]), (got[1], got[3])):
        assert np.array_equal(a.eid, b.eid) and np.array_equal(a.rec, b.rec) and np.array_equal(a.dist, b.dist)


# ---- fuzz ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(dctx, twin, seed):
    """the maps and the five kinds of point sets of tests/test_gpu_nearest.py's fuzz, k drawn from 1 .. 32"""
    rng = np.random.default_rng(100 + seed)
    if seed % 2 == 0:
        G = int(rng.integers(14, 22))
        g = synth.lattice_map(G, int(rng.integers(10, 20)), seed)
    else:
        g = synth.ring_map(int(rng.integers(200, 600)), int(rng.integers(6000, 18000)), seed)
    base = shrunk(maps.Context([g]).load().maps[0], 4)
    assert 5000 <= base.n_edges <= 20000
    n = 1024
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
        k = int(rng.integers(1, 33))
        got = check_against_twin(dctx, twin, segs, pts, k)
        assert (got.count == k).all()
        limited = check_against_twin(dctx, twin, segs, pts, k, max_dist=median_of(twin, segs, pts))
        assert (limited.count == 0).sum() <= n // 2 and (name in ("vertices", "midpoints") or (limited.count == 0).sum() > n // 4), name


# ---- heterogeneous maps and the fans ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", [("outlier", 0), ("thin_band", 1)])
def test_on_a_family(dctx, twin, name, base):
    from test_gpu_distance_hetero import as_map
    ctx, seg, sets = DC.family_sets(name, base)
    install(dctx, as_map(ctx.maps[base], 0), as_map(ctx.maps[1 - base], 1), leaf_order=1)
    rng = np.random.default_rng(7 + base)
    for s in sets:
        pts = np.ascontiguousarray(DC.points_of(ctx, base, sets, s))
        k = int(rng.integers(2, 33))
        where = dict(as_vertices=True, begin=sets[s][0]) if s == "vertices" else {}
        check_against_twin(dctx, twin, seg, pts, k, **where)
        check_against_twin(dctx, twin, seg, pts, k, max_dist=median_of(twin, seg, pts), **where)


@pytest.mark.parametrize("kind", ["tie", "equal"])
def test_replicated_fans_at_k_17(dctx, twin, kind):
    """72 centres, each with a fan of its own whose 64 or more edges a double cannot order (tie) or that are equal as
    rationals (equal): the cut at 17 lies inside the tie in every lane"""
    sc = DC.replicated_scene(kind, np.random.default_rng(50 + 2 * (kind == "equal") + 1))
    pts = np.ascontiguousarray(sc.points)
    base, query = scaled(sc.pts, sc.row), points_map(pts)
    seg = base.segments()
    want = TK.run_twin(twin, seg, pts, 17)
    for i in range(len(pts)):  # (the rows are of the centre's own fan; the 17 smallest eids of an equal fan)
        own = sc.fan_eids[i]
        assert np.isin(want.eid[i], own).all() and (kind == "tie" or want.eid[i].tolist() == own[:17].tolist())
    h = dctx.handle
    try:
        for lo in (0, 1):
            install(dctx, base, query, leaf_order=lo)
            for blocks in (0, 1):
                h.set_debug_option("knearest_blocks", blocks)
                same(device_knearest(dctx, 17, pts), want)
                same(device_knearest(dctx, 17, None, len(pts)), want)
    finally:
        h.set_debug_option("knearest_blocks", 0)
        h.set_option("leaf_order", 1)


# ---- against rj_within_query, on device outputs alone ----------------------------------------------------------------------
def test_consistent_with_within(dctx, twin, mid):
    from fractions import Fraction
    _, seg, pts = mid
    pts = pts[:1500]
    k = 4
    md = 3 * median_of(twin, seg, pts)
    kn = device_knearest(dctx, k, pts, max_dist=md)
    w = ops.WithinLBVH(dctx)
    w.Init(len(pts), 0)
    try:
        w.Query(1, query_points=pts, max_dist=md)
        off, rec = w.get_offsets().astype(np.int64), w.get_records()
    finally:
        w.free()

    def key(r):
        num, den = (int(r["num_hi"]) << 64) + int(r["num_lo"]), (int(r["den_hi"]) << 64) + int(r["den_lo"])
        return (Fraction(num * num, den) if r["where"] == 0 else Fraction(num), int(r["eid"]))
    shorter = longer = 0
    for i in range(len(pts)):
        lst = rec[off[i]:off[i + 1]]
        row = kn.rec[i, :kn.count[i]]
        assert kn.count[i] == min(k, len(lst))
        if len(lst) <= k:
            assert sorted(row["eid"].tolist()) == lst["eid"].tolist()
            shorter += 1
        else:
            assert np.isin(row["eid"], lst["eid"]).all()
            last = key(row[-1])
            assert all(key(r) > last for r in lst[~np.isin(lst["eid"], row["eid"])])
            longer += 1
        assert [key(r) for r in row] == sorted(key(r) for r in row)
    assert shorter > 100 and longer > 100, (shorter, longer)


# ---- the optional outputs ------------------------------------------------------------------------------------------------
def test_null_outputs_in_every_combination(dctx, twin, mid):
    _, seg, pts = mid
    h = dctx.handle
    n, k, pad = 200, 3, 4
    pts = pts[:n]
    want = TK.run_twin(twin, seg, pts, k, 1 << 40)
    src = h.alloc(16 * n).from_host(pts)
    cnt, eid, rec, dist = h.alloc(4 * (n + pad)), h.alloc(4 * (n * k + pad)), h.alloc(40 * (n * k + pad)), h.alloc(8 * (n * k + pad))
    try:
        for with_cnt in (False, True):
            for with_rec in (False, True):
                for with_dist in (False, True):
                    cnt.from_host(np.full(n + pad, CANARY32, np.uint32))
                    eid.from_host(np.full(n * k + pad, CANARY32, np.uint32))
                    rec.from_host(np.full(10 * (n * k + pad), CANARY32, np.uint32))
                    dist.from_host(np.full(n * k + pad, CANARY_F))
                    h.knearest_query(0, 1, src, 0, n, k, eid, cnt if with_cnt else None, rec if with_rec else None, dist if with_dist else None,
                                     max_dist=1 << 40)
                    c, e, r, d = cnt.to_host(np.uint32), eid.to_host(np.uint32), rec.to_host(NEAR_DTYPE), dist.to_host(np.float64)
                    assert np.array_equal(e[:n * k].reshape(n, k), want.eid) and (e[n * k:] == CANARY32).all()
                    assert (c[n:] == CANARY32).all() and (r.view(np.uint32)[10 * n * k:] == CANARY32).all() and (d[n * k:] == CANARY_F).all()
                    assert np.array_equal(c[:n], want.count) if with_cnt else (c == CANARY32).all()
                    assert np.array_equal(r[:n * k].reshape(n, k), want.rec) if with_rec else (r.view(np.uint32) == CANARY32).all()
                    if with_dist:
                        same(TK.Answer(want.count, want.eid, None, d[:n * k].reshape(n, k), None), want)
                    else:
                        assert (d == CANARY_F).all()
    finally:
        for b in (src, cnt, eid, rec, dist):
            b.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dctx, mid):
    base, _, pts = mid
    h = dctx.handle
    n, k = 100, 4
    src = h.alloc(16 * n).from_host(pts[:n])
    cnt, eid, rec, dist = h.alloc(4 * n), h.alloc(4 * n * k), h.alloc(40 * n * k), h.alloc(8 * n * k)
    cnt.from_host(np.full(n, CANARY32, np.uint32))
    eid.from_host(np.full(n * k, CANARY32, np.uint32))
    rec.from_host(np.full(10 * n * k, CANARY32, np.uint32))
    dist.from_host(np.full(n * k, CANARY_F))

    def untouched():
        return ((cnt.to_host(np.uint32) == CANARY32).all() and (eid.to_host(np.uint32) == CANARY32).all() and (rec.to_host(np.uint32) == CANARY32).all() and
                (dist.to_host(np.float64) == CANARY_F).all())
    np_query = dctx.ctx.get_map(1).n_points
    plan, options = h.get_plan(), [h.get_option(o) for o in ("leaf_order", "stats", "query_order")]
    bad = [
        dict(base=0, query=0), dict(base=2, query=1), dict(base=-1, query=0), dict(base=1, query=1),
        dict(base=1, query=0),                       # map 1 has no index
        dict(eid=None),                              # a null eid_dev with n > 0
        dict(k=0), dict(k=33), dict(k=(1 << 32) - 1),
        dict(pts=None, begin=np_query - n + 1),      # a range that leaves the query map
        dict(pts=None, begin=np_query + 5),
        dict(pts=None, begin=(1 << 64) - 50),        # ... and one whose end wraps
        dict(max_dist=(1 << 48) + 1),
        dict(n=1 << 32), dict(pts=None, begin=0, n=1 << 32),  # n >= 2^32
    ]
    try:
        h.knearest_query(0, 1, src, 0, n, k, eid, cnt, rec, dist)  # (a good call first: the stage times are set)
        assert h.get_option(TIMES[2]) >= 0 and not untouched()
        cnt.from_host(np.full(n, CANARY32, np.uint32))
        eid.from_host(np.full(n * k, CANARY32, np.uint32))
        rec.from_host(np.full(10 * n * k, CANARY32, np.uint32))
        dist.from_host(np.full(n * k, CANARY_F))
        for kw in bad:
            with pytest.raises(_capi.RayJoinError) as ei:
                h.knearest_query(kw.get("base", 0), kw.get("query", 1), kw.get("pts", src), kw.get("begin", 0), kw.get("n", n), kw.get("k", k),
                                 kw.get("eid", eid), cnt, rec, dist, max_dist=kw.get("max_dist", -1))
            assert ei.value.code == _capi.RJ_E_INVALID and "rj_knearest_query" in str(ei.value), kw
            assert untouched(), kw
            assert h.get_option(TIMES[2]) == -1
        # n == 0 is fine and writes nothing, whatever the pointers are
        h.knearest_query(0, 1, src, 0, 0, k, None, None, None, None)
        h.knearest_query(0, 1, None, np_query, 0, k, eid, cnt, rec, dist)
        assert untouched()
        # the largest max_dist and the largest k are accepted; the handle is what it was
        h.knearest_query(0, 1, src, 0, n, k, eid, cnt, rec, dist, max_dist=1 << 48)
        assert (eid.to_host(np.uint32) != CANARY32).all() and (cnt.to_host(np.uint32) == k).all()
        assert h.get_plan() == plan and [h.get_option(o) for o in ("leaf_order", "stats", "query_order")] == options
    finally:
        for b in (src, cnt, eid, rec, dist):
            b.free()


# ---- a traversal, not a scan -------------------------------------------------------------------------------------------
def test_the_traversal_prunes(dctx, twin):
    base = base_lattice(22, 16, 8)
    assert base.n_edges >= 16000
    seg = install(dctx, base, scaled(base.pts, base.row_index, 1))
    h = dctx.handle
    n, k = base.n_points, 4
    h.set_option("stats", 1)
    try:
        got = device_knearest(dctx, k, None, n)
        s = h.last_stats_raw()
    finally:
        h.set_option("stats", 0)
    same(got, TK.run_twin(twin, seg, base.pts, k))
    assert (got.dist[:, 0] == 0).all()  # (every point is a vertex of the base map)
    leaf_visits, exact, nodes, entered = s[0], s[1], s[2], s[4]
    print("leaf visits %d (%.2f per point), exact evaluations %d (%.2f per point), nodes expanded %d, entered a list %d (%.2f per point)" %
          (leaf_visits, leaf_visits / n, exact, exact / n, nodes, entered, entered / n))
    assert exact >= entered >= got.count.sum() == n * k and nodes > 0
    # no fault: the call returned without RJ_E_INTERNAL (it would have raised), its stages were timed, the next call is fine
    assert h.get_option(TIMES[2]) >= 0 and h.get_option(TIMES[1]) >= 0
    assert np.array_equal(device_knearest(dctx, k, base.pts[:100]).eid, got.eid[:100])
    assert leaf_visits * 64 < n * base.n_edges / 8, (leaf_visits, n, base.n_edges)
