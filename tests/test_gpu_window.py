"""The edges of a map that meet each rectangle on the device (rj_window_query, Handle.window_query, ops.WindowLBVH) against
the host twin's brute force over all edges (tests/hosttwin/window_twin.cc, held to the plain-Python definition by
tests/test_window.py), array for array -- offsets, eids, flags, counts: the hand cases of tests/window_cases.py; trees of
one, two and three levels; lattice and ring maps; "leaf_order" 0 and 1; the window counts around a wave; windows from below
a quantum to the whole map; lists of 63 / 64 / 65 / 129 and thousands of pairs; every start level, the shortcut on and off,
any grid, shuffled windows; the containment counters; the capacity that just fits, the overflow at one less and the counting
call, with canaries; flags_dev and offsets_dev NULL in every combination; every refusal with the outputs and the counts
untouched; the handle's state and a following PIP / LSI query; point windows against rj_within_query at max_dist 0; the
fault word of a stack that is too small; the fuzz over lattices and ring maps with the five window kinds mixed.  No other
call may fault: a raised fault word is RJ_E_INTERNAL, which fails whatever test it appears in."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_window as TW  # noqa: E402
import window_cases as WC  # noqa: E402
from test_gpu_nearest import base_lattice, extent, install, levels_of, scaled, shrunk, three_level_lattice  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY32, CANARY64, CANARY8 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0x5A
TIMES = ["window_last_us%d" % k for k in range(3)]
KINDS = ("tiny", "edge", "leaf", "quarter", "whole")
LO, HI = -(1 << 46), (1 << 46) - 1
NONE = dict(n_pairs=0, n_windows_hit=0, max_per_window=0)


@pytest.fixture(scope="module")
def twin():
    return TW.twin_lib()


@pytest.fixture(scope="module")
def dctx():
    d = ops.DeviceContext(maps.Context([]), 0)
    yield d
    d.close()


def twin_answer(twin, seg, windows):
    """-> dict(off, eid, flags, counts) of the exact twin"""
    rc, counts, off, eid, flg, _ = TW.call_twin(twin, seg, windows)
    assert rc == TW.OK
    return dict(off=off, eid=eid, flags=flg, counts=dict(zip(_capi.WINDOW_COUNTS, counts)))


def device_answer(dctx, windows, flags=True, capacity=0):
    """the same through ops.WindowLBVH (capacity 0: the counting call sizes the arrays)"""
    windows = np.ascontiguousarray(windows, np.int64).reshape(-1, 4)
    q = ops.WindowLBVH(dctx)
    q.Init(len(windows), capacity)
    try:
        n_pairs = q.Query(0, windows, flags=flags)
        indptr, eids = q.to_csr()
        assert len(eids) == n_pairs == q.counts()["n_pairs"] and indptr.dtype == np.int64 and (indptr == q.get_offsets().astype(np.int64)).all()
        if not flags:
            with pytest.raises(ValueError):
                q.get_flags()
        return dict(off=q.get_offsets(), eid=eids, flags=q.get_flags() if flags else None, counts=q.counts())
    finally:
        q.free()


def same(got, want):
    assert got["counts"] == want["counts"]
    assert np.array_equal(got["off"], want["off"]) and np.array_equal(got["eid"], want["eid"])
    if got["flags"] is not None:
        assert np.array_equal(got["flags"], want["flags"])


def check_against_twin(dctx, twin, seg, windows, want=None):
    want = want or twin_answer(twin, seg, windows)
    got = device_answer(dctx, windows)
    same(got, want)
    return got


def lists_of(ans):
    flat = list(zip(ans["eid"].tolist(), ans["flags"].tolist()))
    return [flat[int(ans["off"][i]):int(ans["off"][i + 1])] for i in range(len(ans["off"]) - 1)]


def mean_edge_length(seg):
    return max(1, int(np.hypot((seg[:, 2] - seg[:, 0]).astype(np.float64), (seg[:, 3] - seg[:, 1]).astype(np.float64)).mean()))


def windows_of(base, rng, kind, n):
    """n windows of one kind over the map: below a quantum (2^16), about an edge, about a leaf block (64 edges: eight edge
    lengths), a quarter of the map, the whole map and more; the small ones half on vertices, half anywhere"""
    x0, y0, x1, y1 = (int(v) for v in extent(base))
    edge = mean_edge_length(base.segments())
    half = {"tiny": 1 << 14, "edge": edge // 2 + 1, "leaf": 4 * edge, "quarter": max(x1 - x0, y1 - y0) // 4, "whole": max(x1 - x0, y1 - y0)}[kind]
    c = np.stack([rng.integers(x0, x1 + 1, n), rng.integers(y0, y1 + 1, n)], 1)
    on = rng.random(n) < 0.5
    c[on] = base.pts[rng.integers(0, base.n_points, int(on.sum()))]
    if kind == "whole":
        c[:] = ((x0 + x1) // 2, (y0 + y1) // 2)
    hx, hy = rng.integers(0, half + 1, n) if kind != "whole" else np.full(n, half), rng.integers(0, half + 1, n) if kind != "whole" else np.full(n, half)
    w = np.stack([c[:, 0] - hx, c[:, 1] - hy, c[:, 0] + hx, c[:, 1] + hy], 1).astype(np.int64)
    return np.clip(w, LO, HI)


def mixed_windows(base, rng, per_kind):
    w = np.concatenate([windows_of(base, rng, k, per_kind if k not in ("quarter", "whole") else max(1, per_kind // 8)) for k in KINDS])
    return np.ascontiguousarray(w[rng.permutation(len(w))])


# ---- the hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_hand_cases(dctx, twin, name):
    c = WC.HAND[name]
    seg = install(dctx, scaled(c.pts, c.row))
    assert lists_of(check_against_twin(dctx, twin, seg, c.windows)) == c.want


# ---- tree heights, maps, leaf orders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_tree_heights(dctx, twin, levels):
    G, k = {1: (2, 5), 2: (12, 16)}.get(levels) or three_level_lattice()
    base = base_lattice(G, k, 5)
    assert {1: base.n_edges <= 64, 2: 4000 < base.n_edges < 6000, 3: base.n_edges > 64 * 4096}[levels]
    seg = install(dctx, base)
    assert levels_of(dctx) == levels
    windows = mixed_windows(base, np.random.default_rng(levels), 60)
    want = twin_answer(twin, seg, windows)
    assert want["counts"]["n_pairs"] > 2 * base.n_edges and want["counts"]["n_windows_hit"] > len(windows) // 2
    assert {0, 1, 2, 3} <= set(want["flags"].tolist()) or levels == 1
    check_against_twin(dctx, twin, seg, windows, want=want)


@functools.lru_cache(maxsize=None)
def mid_map():
    base = base_lattice(12, 16, 5)
    return base, mixed_windows(base, np.random.default_rng(9), 80)


@pytest.fixture
def mid(dctx):
    """the two-level lattice, installed, and 260 mixed windows"""
    base, windows = mid_map()
    return base, install(dctx, base, leaf_order=1), windows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_window_counts(dctx, twin, mid, n):
    _, seg, windows = mid
    assert len(windows) >= 257
    check_against_twin(dctx, twin, seg, windows[:n])


@pytest.mark.parametrize("kind", KINDS)
def test_window_sizes(dctx, twin, mid, kind):
    base, seg, _ = mid
    windows = windows_of(base, np.random.default_rng(5), kind, 8 if kind in ("quarter", "whole") else 200)
    got = check_against_twin(dctx, twin, seg, windows)
    lens = np.diff(got["off"].astype(np.int64))
    if kind == "tiny":
        assert (windows[:, 2] - windows[:, 0] < 1 << 16).all() and 0 < (lens > 0).sum() and lens.max() <= 8
    if kind == "whole":
        assert (lens == base.n_edges).all() and (got["flags"] == 3).all()


@pytest.mark.parametrize("kind", ["lattice", "rings"])
def test_leaf_order_does_not_change_the_result(dctx, twin, kind):
    g = synth.lattice_map(12, 16, 6) if kind == "lattice" else synth.ring_map(300, 9000, 6)
    base = maps.Context([g]).load().maps[0]
    windows = mixed_windows(base, np.random.default_rng(4), 50)
    got = []
    try:
        for lo in (0, 1):
            seg = install(dctx, base, leaf_order=lo)
            got.append(check_against_twin(dctx, twin, seg, windows))
    finally:
        dctx.handle.set_option("leaf_order", 1)
    same(got[0], got[1])
    assert got[0]["counts"]["n_pairs"] > base.n_edges


def test_list_lengths_across_the_staging_flush(dctx, twin):
    """one straight chain of 4 000 edges of length s: the window from s / 2 to s / 2 + (L - 1) s meets exactly L edges"""
    s, ne = 3 << 15, 4000
    pts = [(k * s - (ne // 2) * s, 7) for k in range(ne + 1)]
    seg = install(dctx, scaled(pts, [0, len(pts)]))
    x = pts[100][0]
    lengths = [63, 64, 65, 129, 3000, 1, 128, 127]
    windows = np.array([(x + s // 2, 0, x + s // 2 + (L - 1) * s, 14) for L in lengths], np.int64)
    got = check_against_twin(dctx, twin, seg, windows)
    assert np.diff(got["off"].astype(np.int64)).tolist() == lengths and got["counts"]["max_per_window"] == 3000
    # edge 100 + k: its first point lies in the window from k = 1 on, its second point up to k = L - 2
    assert all(row == [(100 + k, (1 if k >= 1 else 0) | (2 if k <= L - 2 else 0)) for k in range(L)] for row, L in zip(lists_of(got), lengths))


# ---- independence --------------------------------------------------------------------------------------------------------
def test_start_level_shortcut_grid_and_order_do_not_change_the_result(dctx, twin):
    G, k = three_level_lattice()
    base = base_lattice(G, k, 5)
    seg = install(dctx, base)
    top = levels_of(dctx)
    assert top == 3
    windows = mixed_windows(base, np.random.default_rng(12), 40)
    want = twin_answer(twin, seg, windows)
    h = dctx.handle
    try:
        for level in range(0, top + 2):  # (0: by rule; top + 1: clamped to the top)
            for contained in (1, 0):
                h.set_debug_option("window_start_level", level)
                h.set_debug_option("window_contained", contained)
                same(device_answer(dctx, windows), want)
        us = [h.get_option(t) for t in TIMES]
        assert all(v >= 0 for v in us) and us[2] >= us[0] and us[2] >= us[1]
        h.set_debug_option("window_start_level", 0)
        for blocks in (1, 3, 17):
            for contained in (1, 0):
                h.set_debug_option("window_blocks", blocks)
                h.set_debug_option("window_contained", contained)
                same(device_answer(dctx, windows), want)
    finally:
        h.set_debug_option("window_start_level", 0)
        h.set_debug_option("window_contained", 1)
        h.set_debug_option("window_blocks", 0)
    # shuffled windows: the lists of a window do not change
    perm = np.random.default_rng(3).permutation(len(windows))
    a, b = want, device_answer(dctx, np.ascontiguousarray(windows[perm]))
    ao, bo = a["off"].astype(np.int64), b["off"].astype(np.int64)
    assert (np.diff(bo) == np.diff(ao)[perm]).all()
    gather = np.concatenate([np.arange(ao[i], ao[i + 1]) for i in perm])
    assert np.array_equal(b["eid"], a["eid"][gather]) and np.array_equal(b["flags"], a["flags"][gather])


def test_a_window_around_the_map_is_handed_out_without_a_test(dctx, twin, mid):
    base, seg, _ = mid
    x0, y0, x1, y1 = (int(v) for v in extent(base))
    m = (1 << 16) + 5
    window = np.array([(x0 - m, y0 - m, x1 + m, y1 + m)], np.int64)
    ne = base.n_edges
    h = dctx.handle
    got = {}
    try:
        h.set_option("stats", 1)
        for contained in (1, 0):
            h.set_debug_option("window_contained", contained)
            got[contained] = (device_answer(dctx, window), h.last_stats_raw())
    finally:
        h.set_debug_option("window_contained", 1)
        h.set_option("stats", 0)
    want = twin_answer(twin, seg, window)
    for contained in (1, 0):
        ans, s = got[contained]
        same(ans, want)
        assert np.array_equal(ans["eid"], np.arange(ne, dtype=np.uint32)) and (ans["flags"] == 3).all() and s[4] == ne
        assert (s[2], s[3]) == ((0, ne) if contained else (ne, 0)), (contained, s[:5])
    assert got[1][1][1] == 0 and got[0][1][1] >= (ne + 63) // 64  # (under the shortcut no leaf block is loaded; without it, every one)


# ---- the capacity --------------------------------------------------------------------------------------------------------
class Buffers:
    """offsets, eid and flags in device memory with canaries in every word, `extra` entries behind the capacity"""

    def __init__(self, h, n, capacity, extra=4):
        self.n, self.cap = n, capacity + extra
        self.off, self.eid, self.flags = h.alloc(8 * (n + 2)), h.alloc(4 * self.cap), h.alloc(self.cap)
        self.fill()

    def fill(self):
        self.off.from_host(np.full(self.n + 2, CANARY64, np.uint64))
        self.eid.from_host(np.full(self.cap, CANARY32, np.uint32))
        self.flags.from_host(np.full(self.cap, CANARY8, np.uint8))

    def host(self):
        return self.off.to_host(np.uint64), self.eid.to_host(np.uint32), self.flags.to_host(np.uint8)

    def pairs_untouched(self, behind=0):
        _, e, f = self.host()
        return (e[behind:] == CANARY32).all() and (f[behind:] == CANARY8).all()

    def free(self):
        for b in (self.off, self.eid, self.flags):
            b.free()


def test_capacity_overflow_and_the_counting_call(dctx, twin, mid):
    _, seg, windows = mid
    h = dctx.handle
    n = 200
    windows = np.ascontiguousarray(windows[:n])
    want = twin_answer(twin, seg, windows)
    n_pairs = want["counts"]["n_pairs"]
    assert n_pairs > n
    src = h.alloc(32 * n).from_host(windows)
    B = Buffers(h, n, n_pairs)
    try:
        # exactly enough
        counts = h.window_query(0, src, n, n_pairs, B.off, B.eid, B.flags)
        off, e, f = B.host()
        assert counts == want["counts"] and np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64
        assert np.array_equal(e[:n_pairs], want["eid"]) and np.array_equal(f[:n_pairs], want["flags"]) and B.pairs_untouched(n_pairs)
        # one short: the true counts and offsets, the pair arrays untouched
        B.fill()
        with pytest.raises(_capi.WindowOverflow) as ei:
            h.window_query(0, src, n, n_pairs - 1, B.off, B.eid, B.flags)
        assert ei.value.code == _capi.RJ_E_OVERFLOW and ei.value.counts == want["counts"]
        off = B.host()[0]
        assert np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 and B.pairs_untouched()
        assert h.get_option(TIMES[2]) >= 0
        # ... and without offsets
        B.fill()
        with pytest.raises(_capi.WindowOverflow) as ei:
            h.window_query(0, src, n, 1, None, B.eid, B.flags)
        assert ei.value.counts == want["counts"] and (B.host()[0] == CANARY64).all() and B.pairs_untouched()
        # the counting call: the offsets of the filling call and nothing else, whatever the pair pointers are
        for ptrs in ((None, None), (B.eid, B.flags)):
            B.fill()
            counts = h.window_query(0, src, n, 0, B.off, *ptrs)
            off = B.host()[0]
            assert counts == want["counts"] and np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 and B.pairs_untouched()
        B.fill()
        assert h.window_query(0, src, n, 0) == want["counts"] and (B.host()[0] == CANARY64).all()
        # flags_dev and offsets_dev NULL in every combination
        for with_off in (False, True):
            for with_flags in (False, True):
                B.fill()
                counts = h.window_query(0, src, n, n_pairs + 2, B.off if with_off else None, B.eid, B.flags if with_flags else None)
                off, e, f = B.host()
                assert counts == want["counts"] and np.array_equal(e[:n_pairs], want["eid"]) and (e[n_pairs:] == CANARY32).all()
                assert np.array_equal(off[:n + 1], want["off"]) and off[n + 1] == CANARY64 if with_off else (off == CANARY64).all()
                assert np.array_equal(f[:n_pairs], want["flags"]) and (f[n_pairs:] == CANARY8).all() if with_flags else (f == CANARY8).all()
        # ops: Count gives the per-window counts; Query grows from a capacity that is too small, once, and refuses to when told not to
        for cap0 in (7, 0):
            q = ops.WindowLBVH(dctx)
            q.Init(n, cap0)
            try:
                assert np.array_equal(q.Count(0, windows), np.diff(want["off"]))
                with pytest.raises(_capi.WindowOverflow) as ei:
                    q.Query(0, windows, grow=False)
                assert ei.value.counts == want["counts"]
                assert q.Query(0, windows) == n_pairs and q.capacity == n_pairs
                assert np.array_equal(q.get_eids(), want["eid"]) and np.array_equal(q.get_flags(), want["flags"])
                assert q.Query(0, windows, grow=False) == n_pairs  # (it fits now)
            finally:
                q.free()
    finally:
        src.free()
        B.free()


class DeviceArray:
    """what ops.WindowLBVH needs of a device tensor: data_ptr() and shape, over memory of the handle's"""

    def __init__(self, h, a):
        self.buf, self.shape = h.alloc(max(1, a.nbytes)).from_host(a), a.shape

    def data_ptr(self):
        return self.buf.data_ptr()


def test_windows_in_device_memory(dctx, twin, mid):
    _, seg, windows = mid
    t = DeviceArray(dctx.handle, np.ascontiguousarray(windows[:100]))
    q = ops.WindowLBVH(dctx)
    q.Init(100, 0)
    try:
        assert np.array_equal(q.Count(0, t), np.diff(twin_answer(twin, seg, windows[:100])["off"]))
        q.Query(0, t)
        same(dict(off=q.get_offsets(), eid=q.get_eids(), flags=q.get_flags(), counts=q.counts()), twin_answer(twin, seg, windows[:100]))
    finally:
        q.free()
        t.buf.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(dctx, mid):
    _, _, windows = mid
    h = dctx.handle
    n, cap = 100, 50
    src = h.alloc(32 * n).from_host(np.ascontiguousarray(windows[:n]))
    B = Buffers(h, n, cap)
    plan, options = h.get_plan(), [h.get_option(o) for o in ("leaf_order", "stats", "query_order")]
    counts = (C.c_uint64 * 3)(77, 78, 79)
    bad = [
        dict(base=2), dict(base=-1),
        dict(base=1),                  # map 1 has no index
        dict(counts=None),             # a null counts
        dict(win=None),                # nw > 0 with a null win_dev
        dict(eid=None),                # pair_capacity > 0 with a null eid_dev
        dict(n=1 << 32), dict(n=(1 << 64) - 1),  # nw >= 2^32
        dict(cap=1 << 32),             # pair_capacity >= 2^32
    ]
    try:
        h.window_query(0, src, n, 0)  # (a call that worked: the stage times are set)
        assert h.get_option(TIMES[2]) >= 0
        for kw in bad:
            rc = h.L.rj_window_query(h.h, kw.get("base", 0), _capi._ptr(kw.get("win", src)), kw.get("n", n), kw.get("cap", cap), _capi._ptr(B.off),
                                     _capi._ptr(kw.get("eid", B.eid)), _capi._ptr(B.flags), kw.get("counts", counts))
            assert rc == _capi.RJ_E_INVALID and b"rj_window_query" in h.L.rj_last_error_string(h.h), kw
            assert list(counts) == [77, 78, 79] and (B.host()[0] == CANARY64).all() and B.pairs_untouched(), kw
            assert h.get_option(TIMES[2]) == -1
        # nw == 0 is fine, with or without an array: zero counts, offsets[0] = 0, nothing else
        for win in (src, None):
            B.fill()
            assert h.window_query(0, win, 0, cap, B.off, B.eid, B.flags) == NONE
            off = B.host()[0]
            assert off[0] == 0 and (off[1:] == CANARY64).all() and B.pairs_untouched() and h.get_option(TIMES[2]) == -1
        assert h.window_query(0, src, 0, 0) == NONE
        assert h.get_plan() == plan and [h.get_option(o) for o in ("leaf_order", "stats", "query_order")] == options
    finally:
        src.free()
        B.free()


# ---- the handle's state ----------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_of_the_handle():
    """plan, options and a following rj_pip_query / rj_lsi_query are what they were without the window call"""
    ctx = maps.Context([synth.lattice_map(6, 90, 1), synth.lattice_map(14, 40, 2)]).load()
    d = ops.DeviceContext(ctx, 0).LoadToDevice()
    try:
        d.BuildIndex(0)
        h = d.handle

        def lsi_and_pip():
            lsi = ops.LSILBVH(d)
            lsi.Init(1 << 20)
            lsi.Query(1)
            pip = ops.PIPLBVH(d)
            pip.Init(ctx.maps[1].n_points)
            pip.Query(1)
            return lsi.get_pairs(), pip.get_closest_eids(), pip.get_face_ids()
        before = lsi_and_pip()
        plan, options = h.get_plan(), [h.get_option(o) for o in ("leaf_order", "stats", "query_order", "pip_walk", "timers")]
        windows = mixed_windows(ctx.maps[0], np.random.default_rng(1), 40)
        q = ops.WindowLBVH(d)
        q.Init(len(windows), 0)
        try:
            assert q.Query(0, windows) > ctx.maps[0].n_edges
        finally:
            q.free()
        assert h.get_plan() == plan and [h.get_option(o) for o in ("leaf_order", "stats", "query_order", "pip_walk", "timers")] == options
        after = lsi_and_pip()
        assert len(before[0]) > 100 and all(np.array_equal(a, b) for a, b in zip(before, after))
    finally:
        d.close()


def test_point_windows_equal_within_at_distance_zero(dctx, mid):
    base, _, _ = mid
    rng = np.random.default_rng(8)
    pts = np.concatenate([base.pts[rng.integers(0, base.n_points, 400)], base.pts[:100] + 1]).astype(np.int64)
    got = device_answer(dctx, np.concatenate([pts, pts], 1))
    w = ops.WithinLBVH(dctx)
    w.Init(len(pts), 0)
    try:
        n_pairs = w.Query(1, query_points=pts, max_dist=0, records=False, dist=False)
        assert n_pairs == got["counts"]["n_pairs"] >= 800 and np.array_equal(w.get_offsets(), got["off"]) and np.array_equal(w.get_eids(), got["eid"])
    finally:
        w.free()


def test_a_stack_that_is_too_small_is_an_internal_error(dctx, twin, mid):
    """the instrumented kernel with a stack of one entry (the debug knob of tests/test_gpu_stack.py): the checked push raises
    the call's fault word instead of writing past the stack, the call is RJ_E_INTERNAL, and the next call is fine"""
    _, seg, windows = mid
    h = dctx.handle
    windows = np.ascontiguousarray(windows[:200])
    src = h.alloc(32 * 200).from_host(windows)
    B = Buffers(h, 200, 1 << 16)
    try:
        h.set_option("stats", 1)
        h.set_debug_option("stack_cap", 1)
        with pytest.raises(_capi.RayJoinError) as ei:
            h.window_query(0, src, 200, 1 << 16, B.off, B.eid, B.flags)
        assert ei.value.code == _capi.RJ_E_INTERNAL and "k_window" in str(ei.value) and h.get_option(TIMES[2]) == -1
        assert B.pairs_untouched()
    finally:
        h.set_debug_option("stack_cap", 1 << 30)
        h.set_option("stats", 0)
        src.free()
        B.free()
    check_against_twin(dctx, twin, seg, windows)


# ---- fuzz ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_fuzz(dctx, twin, seed):
    rng = np.random.default_rng(500 + seed)
    if seed % 2 == 0:
        g = synth.lattice_map(int(rng.integers(14, 22)), int(rng.integers(10, 20)), seed)
    else:
        g = synth.ring_map(int(rng.integers(200, 600)), int(rng.integers(6000, 18000)), seed)
    base = maps.Context([g]).load().maps[0]
    if seed % 3 == 0:
        base = shrunk(base, 4)
    assert 5000 <= base.n_edges <= 20000
    seg = install(dctx, base, leaf_order=seed % 4 != 3)
    try:
        windows = mixed_windows(base, rng, 100)
        # a few that are empty, reach outside the domain, or are points and lines
        extra = windows[:8].copy()
        extra[0, 2] = extra[0, 0] - 1
        extra[1] = (LO - 5, LO - 5, HI + 5, HI + 5)
        extra[2, 2:] = extra[2, :2]
        extra[3, 2] = extra[3, 0]
        extra[4] = (HI + 1, LO, HI + 9, HI)
        # around the middle of three long edges, two units each way: the edge passes within one unit of it, its ends lie outside
        long_edges = np.flatnonzero(np.maximum(np.abs(seg[:, 2] - seg[:, 0]), np.abs(seg[:, 3] - seg[:, 1])) > 16)[:3]
        mid = np.stack([(seg[long_edges, 0] + seg[long_edges, 2]) // 2, (seg[long_edges, 1] + seg[long_edges, 3]) // 2], 1)
        extra[5:8] = np.concatenate([mid - 2, mid + 2], 1)
        windows = np.concatenate([windows, extra])
        want = twin_answer(twin, seg, windows)
        lens = np.diff(want["off"].astype(np.int64))
        print("%d edges, %d windows, %d pairs, empty %.3f, longest %d" % (base.n_edges, len(windows), lens.sum(), (lens == 0).mean(), lens.max()))
        # asserted on the TWIN's answer, so that a set that tests nothing fails loudly: of the added windows the empty one and the one beside
        # the domain list nothing and the one around the domain every edge; of the others, the small windows on vertices and the large ones have a list
        assert lens.max() == base.n_edges and (lens[-8:-3] == [0, base.n_edges, lens[-6], lens[-5], 0]).all() and (lens > 0).mean() > 0.3
        assert {0, 1, 2, 3} <= set(want["flags"].tolist())
        same(device_answer(dctx, windows), want)
    finally:
        dctx.handle.set_option("leaf_order", 1)
