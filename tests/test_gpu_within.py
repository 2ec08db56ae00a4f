"""Every edge of a map within a distance of each point on the device (rj_within_query, Handle.within_query, ops.WithinLBVH)
against the host twin's brute force over all edges (tests/hosttwin/within_twin.cc, held to the plain-Python definition by
tests/test_within.py), array for array -- offsets, eids, records, and dist within 2^-50: the hand cases of
tests/within_cases.py as a caller's array and as the query map's vertices; trees of one, two and three levels; the point
counts around a wave; any grid; shuffled points; "leaf_order" 0 and 1; lists of thousands of edges; the capacity that just
fits, the overflow at one less and the counting call, with canaries; rec_dev and dist_dev NULL in every combination; every
refusal with the outputs and the counts untouched; the handle's state; the agreement with rj_nearest_query; the
traversal's visit count; the fault word of a stack that is too small; the fuzz over lattices and ring maps with five kinds
of point sets.  No other call may fault: a raised fault word is RJ_E_INTERNAL, which fails whatever test it appears in."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref as NR  # noqa: E402
import test_nearest as TN  # noqa: E402
import test_within as TW  # noqa: E402
import within_cases as WC  # noqa: E402
from test_gpu_nearest import (base_lattice, extent, install, levels_of, points_map, scaled, shrunk, three_level_lattice,  # noqa: E402
                              uniform_points)
from test_nearest import NEAR_DTYPE, check_dist, tuples_of  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY32, CANARY64, CANARY_F = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, -12345.5
TIMES = ["within_last_us%d" % k for k in range(4)]


@pytest.fixture(scope="module")
def twin():
    return TW.twin_lib()


@pytest.fixture(scope="module")
def nearest_twin():
    return TN.twin_lib()


@pytest.fixture(scope="module")
def dctx():
    d = ops.DeviceContext(maps.Context([]), 0)
    yield d
    d.close()


def twin_answer(twin, seg, points, max_dist):
    """-> dict(off, eid, rec, dist, counts) of the exact twin"""
    rc, counts, off, eid, rec, dist, _ = TW.call_twin(twin, seg, points, max_dist, capacity=64 * len(points))  # (a brute force: once, if it fits)
    if rc == TW.OVERFLOW:
        rc, counts, off, eid, rec, dist, _ = TW.call_twin(twin, seg, points, max_dist, capacity=counts[0])
    assert rc == TW.OK
    eid, rec, dist = eid[:counts[0]], rec[:counts[0]], dist[:counts[0]]
    return dict(off=off, eid=eid, rec=rec, dist=dist, counts=dict(zip(_capi.WITHIN_COUNTS, counts)))


def device_answer(dctx, points=None, n=None, max_dist=0, records=True, dist=True, capacity=0, begin=0):
    """the same through ops.WithinLBVH (capacity 0: the counting call sizes the arrays); points None = the n vertices of the
    query map from `begin`"""
    nn = len(points) if points is not None else n
    q = ops.WithinLBVH(dctx)
    q.Init(nn, capacity)
    try:
        n_pairs = q.Query(1, query_points=points, point_range=None if points is not None else (begin, begin + nn), max_dist=max_dist, records=records,
                          dist=dist)
        indptr, eids = q.to_csr()
        assert len(eids) == n_pairs == q.counts()["n_pairs"] and indptr.dtype == np.int64 and (indptr == q.get_offsets().astype(np.int64)).all()
        if not records:
            with pytest.raises(ValueError):
                q.get_records()
        return dict(off=q.get_offsets(), eid=eids, rec=q.get_records() if records else None, dist=q.get_dist() if dist else None, counts=q.counts())
    finally:
        q.free()


def same(got, want):
    """array for array; dist of a sample within 2^-50 of the exact value, every dist finite and not negative"""
    assert got["counts"] == want["counts"]
    assert np.array_equal(got["off"], want["off"]) and np.array_equal(got["eid"], want["eid"])
    if got["rec"] is not None:
        assert np.array_equal(got["rec"], want["rec"]) and np.array_equal(got["rec"]["eid"], got["eid"])
    if got["dist"] is not None:
        assert len(got["dist"]) == len(want["dist"]) and np.isfinite(got["dist"]).all() and (got["dist"] >= 0).all()
        pick = np.unique(np.linspace(0, max(0, len(want["eid"]) - 1), 300).astype(np.int64))[:len(want["eid"])]
        check_dist(tuples_of(want["rec"][pick]), got["dist"][pick])
    off = got["off"].astype(np.int64)
    for i in np.flatnonzero(np.diff(off) > 1)[:200]:  # ascending inside a point
        assert (np.diff(got["eid"][off[i]:off[i + 1]].astype(np.int64)) > 0).all()


def check_against_twin(dctx, twin, seg, points, max_dist, as_vertices=False, want=None):
    points = np.ascontiguousarray(points, np.int64).reshape(-1, 2)
    want = want or twin_answer(twin, seg, points, max_dist)
    got = device_answer(dctx, None if as_vertices else points, len(points), max_dist)
    same(got, want)
    return got


def lists_of(ans):
    flat = tuples_of(ans["rec"])
    return [flat[int(ans["off"][i]):int(ans["off"][i + 1])] for i in range(len(ans["off"]) - 1)]


def mean_edge_length(seg):
    return int(np.hypot((seg[:, 2] - seg[:, 0]).astype(np.float64), (seg[:, 3] - seg[:, 1]).astype(np.float64)).mean())


# ---- the hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_hand_cases(dctx, twin, name):
    c = WC.HAND[name]
    seg = install(dctx, scaled(c.pts, c.row), points_map(c.points))
    for as_vertices in (False, True):
        got = check_against_twin(dctx, twin, seg, c.points, c.max_dist, as_vertices)
        assert lists_of(got) == c.want


# ---- tree heights and point counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tree_heights(dctx, twin, levels):
    G, k = {1: (2, 5), 2: (12, 16)}.get(levels) or three_level_lattice()
    base = base_lattice(G, k, 5)
    rng = np.random.default_rng(levels)
    pts = np.concatenate([uniform_points(base, 1700, rng), base.pts[rng.integers(0, base.n_points, 300)]])
    seg = install(dctx, base, points_map(pts))
    assert levels_of(dctx) == levels
    md = 4 * mean_edge_length(seg)
    want = twin_answer(twin, seg, pts, md)
    assert want["counts"]["n_pairs"] > 2000 and want["counts"]["max_per_point"] >= 4
    check_against_twin(dctx, twin, seg, pts, md, want=want)
    check_against_twin(dctx, twin, seg, pts, md, as_vertices=True, want=want)


@functools.lru_cache(maxsize=None)
def mid_map():
    base = base_lattice(12, 16, 5)
    pts = uniform_points(base, 4097, np.random.default_rng(9))
    pts[::7] = base.pts[:len(pts[::7])]  # (some on vertices)
    return base, pts, 4 * mean_edge_length(base.segments())


@pytest.fixture
def mid(dctx):
    """the two-level lattice, installed, with 4 097 points as its query map, and four mean edge lengths"""
    base, pts, md = mid_map()
    return base, install(dctx, base, points_map(pts), leaf_order=1), pts, md


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_point_counts(dctx, twin, mid, n):
    _, seg, pts, md = mid
    check_against_twin(dctx, twin, seg, pts[:n], md)
    check_against_twin(dctx, twin, seg, pts[:n], md, as_vertices=True)


def test_any_grid_and_stage_times(dctx, twin, mid):
    _, seg, pts, md = mid
    h = dctx.handle
    want = check_against_twin(dctx, twin, seg, pts, md)
    us = [h.get_option(t) for t in TIMES]
    assert all(v >= 0 for v in us) and us[3] >= us[1] and us[3] >= us[2]
    try:
        for blocks in (1, 3, 17):
            h.set_debug_option("within_blocks", blocks)
            same(device_answer(dctx, pts, max_dist=md), want)
    finally:
        h.set_debug_option("within_blocks", 0)


def test_shuffled_points_give_the_permuted_lists(dctx, twin, mid):
    _, seg, pts, md = mid
    pts = pts[:4096]
    perm = np.random.default_rng(3).permutation(len(pts))
    a, b = device_answer(dctx, pts, max_dist=md), device_answer(dctx, np.ascontiguousarray(pts[perm]), max_dist=md)
    same(a, twin_answer(twin, seg, pts, md))
    ao, bo = a["off"].astype(np.int64), b["off"].astype(np.int64)
    assert (np.diff(bo) == np.diff(ao)[perm]).all()
    gather = np.concatenate([np.arange(ao[i], ao[i + 1]) for i in perm])
    assert np.array_equal(b["eid"], a["eid"][gather]) and np.array_equal(b["rec"], a["rec"][gather]) and np.array_equal(b["dist"], a["dist"][gather])


def test_leaf_order_does_not_change_the_result(dctx, twin):
    base = base_lattice(12, 16, 6)
    pts = uniform_points(base, 1500, np.random.default_rng(4))
    md = 3 * mean_edge_length(base.segments())
    got = []
    try:
        for lo in (0, 1):
            seg = install(dctx, base, points_map(pts), leaf_order=lo)
            got.append(check_against_twin(dctx, twin, seg, pts, md))
            got.append(check_against_twin(dctx, twin, seg, pts, md // 2, as_vertices=True))
    finally:
        dctx.handle.set_option("leaf_order", 1)
    for a, b in ((got[0], got[2]), (got[1], got[3])):
        assert np.array_equal(a["off"], b["off"]) and np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["dist"], b["dist"])


def test_long_lists(dctx, twin, mid):
    """64 points, every edge within 2^48 of each: lists of thousands of edges, dozens of staging flushes per point"""
    base, seg, pts, _ = mid
    got = check_against_twin(dctx, twin, seg, pts[:64], 1 << 48)
    ne = base.n_edges
    assert ne > 4000 and got["counts"] == dict(n_pairs=64 * ne, n_points_hit=64, max_per_point=ne)
    assert np.array_equal(got["eid"].reshape(64, ne), np.broadcast_to(np.arange(ne, dtype=np.uint32), (64, ne)))


# ---- the capacity --------------------------------------------------------------------------------------------------------
class Buffers:
    """offsets, eid, rec and dist in device memory with canaries in every word, `extra` entries behind the capacity"""

    def __init__(self, h, n, capacity, extra=4):
        self.n, self.cap = n, capacity + extra
        self.off, self.eid, self.rec, self.dist = h.alloc(8 * (n + 2)), h.alloc(4 * self.cap), h.alloc(40 * self.cap), h.alloc(8 * self.cap)
        self.fill()

    def fill(self):
        self.off.from_host(np.full(self.n + 2, CANARY64, np.uint64))
        self.eid.from_host(np.full(self.cap, CANARY32, np.uint32))
        self.rec.from_host(np.full(10 * self.cap, CANARY32, np.uint32))
        self.dist.from_host(np.full(self.cap, CANARY_F))

    def host(self):
        return self.off.to_host(np.uint64), self.eid.to_host(np.uint32), self.rec.to_host(NEAR_DTYPE), self.dist.to_host(np.float64)

    def pairs_untouched(self, behind=0):
        _, e, r, d = self.host()
        return (e[behind:] == CANARY32).all() and (r.view(np.uint32)[10 * behind:] == CANARY32).all() and (d[behind:] == CANARY_F).all()

    def free(self):
        for b in (self.off, self.eid, self.rec, self.dist):
            b.free()


def test_capacity_overflow_and_the_counting_call(dctx, twin, mid):
    _, seg, pts, md = mid
    h = dctx.handle
    n = 300
    pts = pts[:n]
    want = twin_answer(twin, seg, pts, md)
    n_pairs = want["counts"]["n_pairs"]
    assert n_pairs > n
    src = h.alloc(16 * n).from_host(pts)
    B = Buffers(h, n, n_pairs)
    try:
        # exactly enough
        counts = h.within_query(0, 1, src, 0, n, md, n_pairs, B.off, B.eid, B.rec, B.dist)
        off, e, r, d = B.host()
        assert counts == want["counts"] and np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64
        assert np.array_equal(e[:n_pairs], want["eid"]) and np.array_equal(r[:n_pairs], want["rec"]) and B.pairs_untouched(n_pairs)
        check_dist(tuples_of(r[:200]), d[:200])
        # one short: the true counts and offsets, the pair arrays untouched
        B.fill()
        with pytest.raises(_capi.WithinOverflow) as ei:
            h.within_query(0, 1, src, 0, n, md, n_pairs - 1, B.off, B.eid, B.rec, B.dist)
        assert ei.value.code == _capi.RJ_E_OVERFLOW and ei.value.counts == want["counts"]
        off = B.host()[0]
        assert np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 and B.pairs_untouched()
        assert h.get_option(TIMES[3]) >= 0
        # ... and without offsets
        B.fill()
        with pytest.raises(_capi.WithinOverflow) as ei:
            h.within_query(0, 1, src, 0, n, md, 1, None, B.eid, B.rec, B.dist)
        assert ei.value.counts == want["counts"] and (B.host()[0] == CANARY64).all() and B.pairs_untouched()
        # the counting call: the offsets of the filling call and nothing else, whatever the pair pointers are
        for ptrs in ((None, None, None), (B.eid, B.rec, B.dist)):
            B.fill()
            counts = h.within_query(0, 1, src, 0, n, md, 0, B.off, *ptrs)
            off = B.host()[0]
            assert counts == want["counts"] and np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 and B.pairs_untouched()
        B.fill()
        assert h.within_query(0, 1, src, 0, n, md, 0) == want["counts"] and (B.host()[0] == CANARY64).all()
        # ops: Count gives the per-point counts; Query grows from a capacity that is too small, once, and refuses to when told not to
        q = ops.WithinLBVH(dctx)
        q.Init(n, 7)
        try:
            assert np.array_equal(q.Count(1, query_points=pts, max_dist=md), np.diff(want["off"]))
            with pytest.raises(_capi.WithinOverflow):
                q.Query(1, query_points=pts, max_dist=md, grow=False)
            assert q.Query(1, query_points=pts, max_dist=md) == n_pairs and q.capacity == n_pairs
            assert np.array_equal(q.get_eids(), want["eid"]) and np.array_equal(q.get_records(), want["rec"])
        finally:
            q.free()
    finally:
        src.free()
        B.free()


def test_null_records_and_dist_in_every_combination(dctx, twin, mid):
    _, seg, pts, md = mid
    h = dctx.handle
    n = 200
    pts = pts[:n]
    want = twin_answer(twin, seg, pts, md)
    n_pairs = want["counts"]["n_pairs"]
    src = h.alloc(16 * n).from_host(pts)
    B = Buffers(h, n, n_pairs)
    try:
        for with_off in (False, True):
            for with_rec in (False, True):
                for with_dist in (False, True):
                    B.fill()
                    counts = h.within_query(0, 1, src, 0, n, md, n_pairs + 2, B.off if with_off else None, B.eid, B.rec if with_rec else None,
                                            B.dist if with_dist else None)
                    off, e, r, d = B.host()
                    assert counts == want["counts"] and np.array_equal(e[:n_pairs], want["eid"]) and (e[n_pairs:] == CANARY32).all()
                    assert np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 if with_off else (off == CANARY64).all()
                    assert (r.view(np.uint32)[10 * n_pairs:] == CANARY32).all() and (d[n_pairs:] == CANARY_F).all()
                    assert np.array_equal(r[:n_pairs], want["rec"]) if with_rec else (r.view(np.uint32) == CANARY32).all()
                    if with_dist:
                        check_dist(tuples_of(want["rec"][:200]), d[:200])
                    else:
                        assert (d == CANARY_F).all()
    finally:
        src.free()
        B.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(dctx, mid):
    _, _, pts, md = mid
    h = dctx.handle
    n, cap = 100, 50
    src = h.alloc(16 * n).from_host(pts[:n])
    B = Buffers(h, n, cap)
    np_query = dctx.ctx.get_map(1).n_points
    plan, options = h.get_plan(), [h.get_option(o) for o in ("leaf_order", "stats", "query_order")]
    counts = (C.c_uint64 * 3)(77, 78, 79)
    bad = [
        dict(base=0, query=0), dict(base=2, query=1), dict(base=-1, query=0), dict(base=1, query=1),
        dict(base=1, query=0),                       # map 1 has no index
        dict(counts=None),                           # a null counts
        dict(eid=None),                              # pair_capacity > 0 with a null eid_dev
        dict(pts=None, begin=np_query - n + 1),      # a range that leaves the query map
        dict(pts=None, begin=np_query + 5),
        dict(pts=None, begin=(1 << 64) - 50),        # ... and one whose end wraps
        dict(n=1 << 32), dict(pts=None, begin=0, n=1 << 32),  # n >= 2^32
        dict(cap=1 << 32),                           # pair_capacity >= 2^32
        dict(max_dist=-1), dict(max_dist=-(1 << 62)), dict(max_dist=(1 << 48) + 1),
    ]
    try:
        h.within_query(0, 1, src, 0, n, md, 0)  # (a call that worked: the stage times are set)
        assert h.get_option(TIMES[3]) >= 0
        for kw in bad:
            rc = h.L.rj_within_query(h.h, kw.get("base", 0), kw.get("query", 1), _capi._ptr(kw.get("pts", src)), kw.get("begin", 0), kw.get("n", n),
                                     kw.get("max_dist", md), kw.get("cap", cap), _capi._ptr(B.off), _capi._ptr(kw.get("eid", B.eid)), _capi._ptr(B.rec),
                                     _capi._ptr(B.dist), kw.get("counts", counts))
            assert rc == _capi.RJ_E_INVALID and b"rj_within_query" in h.L.rj_last_error_string(h.h), kw
            assert list(counts) == [77, 78, 79] and (B.host()[0] == CANARY64).all() and B.pairs_untouched(), kw
            assert h.get_option(TIMES[3]) == -1
        # n == 0 is fine: zero counts, offsets[0] = 0, nothing else
        for args in ((src, 0), (None, np_query)):
            B.fill()
            assert h.within_query(0, 1, args[0], args[1], 0, md, cap, B.off, B.eid, B.rec, B.dist) == dict(n_pairs=0, n_points_hit=0, max_per_point=0)
            off = B.host()[0]
            assert off[0] == 0 and (off[1:] == CANARY64).all() and B.pairs_untouched() and h.get_option(TIMES[3]) == -1
        assert h.within_query(0, 1, src, 0, 0, md, 0) == dict(n_pairs=0, n_points_hit=0, max_per_point=0)
        # the largest max_dist and 0 are accepted; the handle is what it was
        assert h.within_query(0, 1, src, 0, n, 1 << 48, 0)["n_points_hit"] == n
        h.within_query(0, 1, src, 0, n, 0, 0)
        assert h.get_plan() == plan and [h.get_option(o) for o in ("leaf_order", "stats", "query_order")] == options
    finally:
        src.free()
        B.free()


# ---- the agreement with rj_nearest_query -----------------------------------------------------------------------------------
def test_consistent_with_nearest(dctx, twin, mid):
    """for the same points and max_dist rj_nearest_query misses exactly where the list is empty, and otherwise gives the
    list's minimum by distance, then eid"""
    _, seg, pts, md = mid
    pts = pts[:600]
    md = md // 3
    got = device_answer(dctx, pts, max_dist=md)
    q = ops.NearestLBVH(dctx)
    q.Init(len(pts))
    try:
        q.Query(1, query_points=pts, max_dist=md)
        near = q.exact(q.get_records())
    finally:
        q.free()
    lists = lists_of(got)
    empty = sum(not row for row in lists)
    assert 20 < empty < len(pts) - 20, empty
    for row, t in zip(lists, near):
        assert (t[0] == NR.MISS) == (not row)
        if row:
            assert t == min(row, key=lambda r: (NR.d2_of(*r[1:]), r[0]))


# ---- a traversal, not a scan -------------------------------------------------------------------------------------------
def test_the_traversal_prunes(dctx, twin):
    base = base_lattice(22, 16, 8)
    assert base.n_edges >= 16000
    seg = install(dctx, base, scaled(base.pts, base.row_index, 1))
    md = mean_edge_length(seg)
    h = dctx.handle
    h.set_option("stats", 1)
    try:
        got = device_answer(dctx, None, base.n_points, md)
        s = h.last_stats_raw()
    finally:
        h.set_option("stats", 0)
    same(got, twin_answer(twin, seg, base.pts, md))
    leaf_visits, exact, nodes, pairs = s[0], s[1], s[2], s[4]
    print("leaf visits %d (%.2f per point), exact evaluations %d (%.2f per point), nodes expanded %d, pairs %d" %
          (leaf_visits, leaf_visits / base.n_points, exact, exact / base.n_points, nodes, pairs))
    assert pairs == got["counts"]["n_pairs"] >= base.n_points and exact >= pairs and nodes > 0
    assert h.get_option(TIMES[3]) >= 0 and h.get_option(TIMES[1]) >= 0
    assert leaf_visits * 64 < base.n_points * base.n_edges / 8, (leaf_visits, base.n_points, base.n_edges)


def test_a_stack_that_is_too_small_is_an_internal_error(dctx, twin, mid):
    """the instrumented kernel with a stack of one entry (the debug knob of tests/test_gpu_stack.py): the checked push raises
    the call's fault word instead of writing past the stack, the call is RJ_E_INTERNAL, and the next call is fine"""
    _, seg, pts, md = mid
    h = dctx.handle
    src = h.alloc(16 * 500).from_host(pts[:500])
    try:
        h.set_option("stats", 1)
        h.set_debug_option("stack_cap", 1)
        with pytest.raises(_capi.RayJoinError) as ei:
            h.within_query(0, 1, src, 0, 500, md, 0)
        assert ei.value.code == _capi.RJ_E_INTERNAL and "k_within" in str(ei.value) and h.get_option(TIMES[3]) == -1
    finally:
        h.set_debug_option("stack_cap", 1 << 30)
        h.set_option("stats", 0)
        src.free()
    check_against_twin(dctx, twin, seg, pts[:500], md)


# ---- fuzz ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(dctx, twin, nearest_twin, seed):
    """the maps and point sets of test_gpu_nearest.test_fuzz; the radii come from the twin's nearest distances, and the
    conditions on the lists are asserted on the TWIN's answer, so that a set that tests nothing fails loudly.  far_outside:
    with the median nearest distance as the radius half of the points have no edge within it by the median's definition --
    "about half" is 30 to 70 % here, for the sample the median is taken from and the ties -- and "long" is a mean of 64 edges
    or more among the others, a full staging buffer per point"""
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
        "far_outside": np.stack([rng.integers(x1 + 3 * (x1 - x0), x1 + 4 * (x1 - x0), n), rng.integers(y0 - 2 * (y1 - y0), y0 - (y1 - y0), n)], 1)[:256],
        "vertical_line": np.stack([np.full(n, (x0 + x1) // 2), rng.integers(y0, y1, n)], 1),
    }
    install(dctx, base)

    def median_nearest(pts):
        d = np.sort(TN.run_twin(nearest_twin, segs, pts[::8])[1])  # (of every eighth point: a brute force)
        return float(d[len(d) // 2])
    for name, pts in sets.items():
        pts = np.ascontiguousarray(pts, np.int64)
        m = len(pts)
        if name == "vertices":
            md = 0
        elif name == "far_outside":
            md = math.ceil(median_nearest(pts))
        else:
            md = math.ceil(2 * median_nearest(pts))
        want = twin_answer(twin, segs, pts, md)
        lens = np.diff(want["off"].astype(np.int64))
        empty, several, total = (lens == 0).mean(), (lens >= 2).mean(), int(lens.sum())
        print("%s: max_dist %d, %d pairs, empty %.3f, two or more %.3f, longest %d" % (name, md, total, empty, several, lens.max()))
        if name == "vertices":
            assert (lens >= 2).all()
        elif name == "far_outside":
            assert 0.3 <= empty <= 0.7 and lens[lens > 0].mean() >= 64 and total <= 1 << 20, (name, empty, total)
        elif name != "midpoints":  # (its median is below one unit: asserted only against the twin)
            assert 0.02 <= empty <= 0.5 and several >= 0.5 and total <= 256 * m, (name, empty, several, total)
        same(device_answer(dctx, pts, max_dist=md), want)
