"""The index on HETEROGENEOUS maps (tests/skewed_pairs.py: dense in one corner, squeezed into a few cells by an outlier,
crossed by domain-long edges, flat inside one height bucket) against the brute-force oracle, bit for bit: LSI pairs and
records, closest edges and face ids through every first pass (tree walk, column index, exact kernel alone) -- and, read
from the handle's own reports, WHICH path answered: the column build that declines on a frame ("wanted, not built"), the
skyline filled from the leaf boxes with its "too wide" word set, the re-count of the strip build, the lazy column build
at an incoherent query, the candidate-list overflow ("pip_rest"), strips of 2^15 / 2^16 / 2^17 quanta; then the device
grid, the overlay on the two overlay-valid families, and a fuzz over random compositions.  The properties the families
are there for are asserted on the CPU by tests/test_skewed_pairs.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skewed_pairs as S  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("eid", "x_num", "x_den", "y_num", "y_den", "mid_point_polygon_id")
N_RANDOM = 20000


@pytest.fixture(scope="module", autouse=True)
def _threads(oracle):
    """rj_oracle.c runs on one thread unless told otherwise (brute force is most of this module's time)"""
    was = oracle.num_threads()
    oracle.lib().rjo_set_num_threads(16)
    yield
    oracle.lib().rjo_set_num_threads(was)


_want = {}


def want_of(oracle, name):
    """the oracle's side of a family, once per module: maps, brute-force pairs, and per base map the three query point
    sets (the other map's vertices; a shuffled copy; uniform random points over the whole domain, most of them far from
    every edge of the dense part) with their closest edges by brute force"""
    if name not in _want:
        ctx = S.family(name)
        om = S.oracle_maps(oracle, ctx)
        w = dict(ctx=ctx, om=om, pairs=oracle.lsi_brute(om[0], om[1]), pts={}, closest={})
        rng = np.random.default_rng(len(name))
        for base in (0, 1):
            q = ctx.maps[1 - base].pts
            sets = {"vertices": None, "shuffled": np.ascontiguousarray(q[rng.permutation(len(q))]),
                    "random": np.ascontiguousarray(rng.integers(maps.INTERNAL_MIN, maps.INTERNAL_MAX, size=(N_RANDOM, 2)))}
            for k, p in sets.items():
                w["pts"][base, k] = p
                w["closest"][base, k] = oracle.pip_brute(om[base], 1 - base, q if p is None else p)
        _want[name] = w
    return _want[name]


def upload(h, ctx):
    for i in (0, 1):
        m = ctx.maps[i]
        h.upload_map(i, m.pts, m.row_index, m.left, m.right)


class Points:
    """the three point sets of one base map on the device, with output arrays"""

    def __init__(self, h, w, base):
        self.h, self.w, self.base = h, w, base
        self.dev = {k: (None if w["pts"][base, k] is None else h.alloc(16 * len(w["pts"][base, k])).from_host(w["pts"][base, k]))
                    for k in ("vertices", "shuffled", "random")}
        n = max(len(w["closest"][base, k]) for k in self.dev)
        self.closest, self.faces = h.alloc(4 * n), h.alloc(4 * n)

    def check(self, which, what, reps=2):
        """each query runs twice: the second run uses whatever the first built (permutations, lists, the lazy index)"""
        h, base = self.h, self.base
        want = self.w["closest"][base, which]
        n = len(want)
        for rep in range(reps):
            h.pip_query(base, 1 - base, self.dev[which], 0, n, self.closest, self.faces)
            got = self.closest.to_host(np.uint32, n)
            assert np.array_equal(got, want), (what, which, rep, int((got != want).sum()))
            assert np.array_equal(self.faces.to_host(np.int32, n), self.w["om"][base].face_ids(want)), (what, which, rep, "faces")


def shape_of(m):
    """what rj_build_lbvh decides by: (most chains are closed rings, mean chain length below 16)"""
    row = m.row_index.astype(np.int64)
    closed = np.all(m.pts[row[:-1]] == m.pts[row[1:] - 1], axis=1)
    return 2 * int(closed.sum()) >= m.n_chains, m.n_edges // m.n_chains < 16


def declines(m):
    return any(S.column_entries(m, sh) is None for sh in S.STRIP_SHIFTS)


# ---- LSI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_lsi_pairs_and_records_equal_brute_force(oracle, name):
    w = want_of(oracle, name)
    ctx, om, want = w["ctx"], w["om"], w["pairs"]
    ref = oracle.lsi_points(om[0], om[1], want)
    assert np.all(ref["mid_point_polygon_id"] != -2)   # (every brute-force pair is an intersection for the point routine too)
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        cap = len(want) + 1024
        pairs, recs = h.alloc(8 * cap), h.alloc(48 * cap)
        for base in (0, 1):
            q = ctx.maps[1 - base]
            for ysort in (1, 0):
                h.set_option("leaf_ysort", ysort)
                h.build_lbvh(base)
                for segments in (1, 2):
                    h.set_option("lsi_segments", segments)
                    what = (name, base, ysort, segments)
                    n = h.lsi_query(base, 1 - base, 0, q.n_edges, cap, pairs)
                    assert n == len(want), what
                    h.sort_pairs(pairs, n)
                    assert np.array_equal(pairs.to_host(np.uint32, 2 * n).reshape(-1, 2), want), what
                    assert h.get_option("lsi_last_segments") in (1, segments)
            for split in (0, 1):
                h.set_option("lsi_points_split", split)
                h.lsi_points(pairs, len(want), recs)
                assert h.get_option("lsi_points_last_split") == split
                got = recs.to_host(_capi.XSECT_DTYPE, len(want))
                for f in FIELDS:
                    assert np.array_equal(got[f], ref[f]), (name, base, split, f, int((got[f] != ref[f]).reshape(len(got), -1).any(axis=1).sum()))
            print(name, "base", base, "occ_permille", h.get_option("occ_permille%d" % base), "pairs", len(want))
    finally:
        h.close()


def test_lsi_shards_and_overflow_on_the_skewed_lattice(oracle):
    """8 chain-range shards balanced by EDGE COUNT: most of them lie inside the dense corner, the last ones hold a coarse
    lattice each; their union is the whole.  A capacity one short returns RJ_E_OVERFLOW with the true count."""
    w = want_of(oracle, "skew_lattice")
    ctx, want = w["ctx"], w["pairs"]
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        pairs = h.alloc(8 * (len(want) + 64))
        for base in (0, 1):
            q = ctx.maps[1 - base]
            h.build_lbvh(base)
            parts = []
            for c0, c1 in q.shard_chain_ranges(8):
                qb, qe = q.chain_range_to_eids(c0, c1)
                n = h.lsi_query(base, 1 - base, qb, qe, len(want) + 64, pairs)
                parts.append(pairs.to_host(np.uint32, 2 * n).reshape(-1, 2).copy())
            assert sum(len(p) > 0 for p in parts) >= 6
            assert np.array_equal(oracle.sort_pairs(np.concatenate(parts)), want), base
            for short in (len(want) - 1, 7):
                with pytest.raises(_capi.QueueOverflow) as e:
                    h.lsi_query(base, 1 - base, 0, q.n_edges, short, pairs)
                assert e.value.n_found == len(want) and e.value.code == _capi.RJ_E_OVERFLOW, (base, short)
    finally:
        h.close()


# ---- PIP: every first pass, and which one answered --------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_pip_through_every_first_pass_says_which_path_answered(oracle, name):
    w = want_of(oracle, name)
    ctx = w["ctx"]
    rest_seen = {}
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        for base in (0, 1):
            m = ctx.maps[base]
            rings, short = shape_of(m)
            no_columns = declines(m)
            P = Points(h, w, base)
            for columns in (-1, 0, 1):
                for sky in (-1, 0, 1):
                    h.set_option("pip_columns", columns)
                    h.set_option("skyline", sky)
                    h.build_lbvh(base)
                    used = h.get_option("pip_columns_used%d" % base)
                    want_used = 0 if (columns == 0 or no_columns) else 1 if columns == 1 else int(rings or short)
                    assert used == want_used, (name, base, columns, rings, short, no_columns)
                    assert h.get_option("skyline_used%d" % base) == (1 if sky == 1 or (sky < 0 and rings) else 0), (name, base, columns, sky)
                    why = h.get_plan()["index"][base]["columns_why"]
                    assert ("wanted, not built" in why) == (no_columns and (columns == 1 or (columns < 0 and (rings or short)))), (name, base, columns, why)
                    for walk in (0, 1, 2):
                        for wp in (1, 2):
                            h.set_option("pip_walk", walk)
                            h.set_option("pip_walk_points", wp)
                            for which in ("vertices", "shuffled", "random"):
                                what = (name, base, columns, sky, walk, wp)
                                P.check(which, what)
                                passes = h.get_option("pip_last_passes")
                                assert passes == (1 if walk == 0 else 3 if walk == 2 else passes) and passes in (1, 3), what
                                if passes == 3:
                                    assert h.get_option("pip_last_columns") == used, what
                                    rest = h.get_option("pip_rest")
                                    assert 0 <= rest <= len(w["closest"][base, which]), what
                                    if walk == 2 and which == "vertices":
                                        rest_seen[base, used] = max(rest_seen.get((base, used), 0), rest)
                                assert h.get_option("pip_columns_used%d" % base) == used   # (no lazy build below 2^22 points)
            h.set_option("skyline", -1)
            h.set_option("pip_walk", 2)
            if not no_columns:   # every strip width, where columns are built
                h.set_option("pip_columns", 1)
                for shift in (0, 15, 16, 17):
                    h.set_debug_option("strip_shift", shift)
                    h.build_lbvh(base)
                    assert h.get_option("pip_columns_used%d" % base) == 1
                    got_shift = h.get_option("pip_column_shift%d" % base)
                    assert got_shift == (shift or got_shift) and got_shift in S.STRIP_SHIFTS
                    assert h.get_option("pip_column_entries%d" % base) == S.column_entries(m, got_shift), (name, base, shift)
                    for which in ("vertices", "shuffled", "random"):
                        P.check(which, (name, base, "strip_shift", shift))
                        assert h.get_option("pip_last_columns") == 1 and h.get_option("pip_last_passes") == 3
                h.set_debug_option("strip_shift", 0)
            h.set_option("pip_walk", 1)
        print(name, "pip_rest under pip_walk 2, by (base, columns used):", rest_seen)
        if name in ("outlier", "thin_band"):
            # nearly all edges share a few Morton keys / one height bucket: candidate lists overflow, k_pip takes the points over
            assert all(rest_seen[base, 0] > 0 for base in (0, 1)), rest_seen
    finally:
        h.close()


def test_two_points_per_lane_on_the_skewed_lattice(oracle):
    """k_pip_walk2 takes query sets that fill every resident wave with four 128-position groups (2048 points per resident
    block: 4.2 M on a chip of 256 CUs and 8 blocks each; the test asserts from the handle that the kernel ran): 4.4 M points
    over skew_lattice, half of them uniform over the domain and half in the dense corner (held to the grid oracle, which
    equals brute force on this family -- tests/test_skewed_pairs.py -- and to brute force on a sample), one and two points
    per lane.  "pip_columns" 0: a set of 2^22 incoherent points would otherwise build the column index."""
    w = want_of(oracle, "skew_lattice")
    ctx, om = w["ctx"], w["om"]
    rng = np.random.default_rng(77)
    n = 4_400_000
    pts = np.ascontiguousarray(rng.integers(maps.INTERNAL_MIN, maps.INTERNAL_MAX, size=(n, 2)))
    pts[: n // 2] = ctx.maps[1].pts[rng.integers(0, ctx.maps[1].n_points, n // 2)] + rng.integers(-2000, 2001, size=(n // 2, 2))   # half of them in the dense corner
    want = oracle.pip_grid(om[0], 0, pts, 256)
    sample = rng.permutation(n)[:20000]
    assert np.array_equal(want[sample], oracle.pip_brute(om[0], 1, np.ascontiguousarray(pts[sample])))
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        h.set_option("pip_columns", 0)
        h.build_lbvh(0)
        assert h.get_option("pip_columns_used0") == 0
        d, closest, faces = h.alloc(16 * n).from_host(pts), h.alloc(4 * n), h.alloc(4 * n)
        h.set_option("pip_walk", 2)
        for wp in (2, 1, 2):
            h.set_option("pip_walk_points", wp)
            for rep in range(2):
                h.pip_query(0, 1, d, 0, n, closest, faces)
                assert h.get_option("pip_last_walk_points") == wp and h.get_option("pip_last_columns") == 0
                assert np.array_equal(closest.to_host(np.uint32, n), want), (wp, rep)
                assert np.array_equal(faces.to_host(np.int32, n), om[0].face_ids(want)), (wp, rep)
    finally:
        h.close()


# ---- the column build that declines -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rings_frame", "short_chains_frame"])
def test_declined_columns_leave_the_tree_and_a_partial_skyline(oracle, name):
    w = want_of(oracle, name)
    ctx, om = w["ctx"], w["om"]
    m = ctx.maps[0]
    rings, short = shape_of(m)
    assert (rings or short) and declines(m)
    rng = np.random.default_rng(5)
    R, lo = maps.INTERNAL_RANGE, maps.INTERNAL_MIN
    # points above everything (over the frame's top edge: certain misses), and points anywhere inside the frame
    fb, top = ctx.skew["frame_box"], ctx.skew["frame_top"]   # (a box inside the frame; the frame's highest y)
    above = np.stack([rng.integers(lo, maps.INTERNAL_MAX, 4000), lo + (R * rng.uniform(top + 0.0005, min(top + 0.02, 0.9995), 4000)).astype(np.int64)], 1)
    inside = lo + (R * rng.uniform(fb[0] + 0.001, fb[2] - 0.001, size=(8000, 2))).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate([above, inside]))
    want = oracle.pip_brute(om[0], 1, pts)
    assert np.all(want[:4000] == _capi.MISS_EID) and np.all(want[4000:] != _capi.MISS_EID)   # (inside the frame its top edge is above every point)
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        P = Points(h, w, 0)
        d, closest, faces = h.alloc(16 * len(pts)).from_host(pts), h.alloc(4 * len(pts)), h.alloc(4 * len(pts))
        for columns in (-1, 1):
            # include/rayjoin_amd.h ("pip_columns"): a segment over more than 1024 strips is no error, forced or not -- RJ_OK,
            # "pip_columns_used" 0, and the plan says why
            for sky in (-1, 1):
                h.set_option("pip_columns", columns)
                h.set_option("skyline", sky)
                h.build_lbvh(0)
                assert h.get_option("pip_columns_used0") == 0 and h.get_option("pip_column_shift0") == 0
                assert "wanted, not built" in h.get_plan()["index"][0]["columns_why"]
                assert h.get_option("skyline_used0") == (1 if sky == 1 or rings else 0), (name, columns, sky)
                for walk in (1, 2, 0):
                    h.set_option("pip_walk", walk)
                    for rep in range(2):
                        h.pip_query(0, 1, d, 0, len(pts), closest, faces)
                        assert np.array_equal(closest.to_host(np.uint32), want), (name, columns, sky, walk, rep)
                        assert np.array_equal(faces.to_host(np.int32), om[0].face_ids(want)), (name, columns, sky, walk, rep)
                        assert h.get_option("pip_last_columns") == 0 or walk == 0
                    for which in ("vertices", "random"):
                        P.check(which, (name, columns, sky, walk))
    finally:
        h.close()


# ---- the strip build's re-count, and scratch that regrows -------------------------------------------------------------------
def test_strip_build_counts_again_when_the_estimate_was_short(oracle):
    """One handle: a small homogeneous ring map with columns (its scratch block is sized by it), then skew_rings at strips of
    2^15 quanta -- far more entries than the build's estimate of min(2 slots, 2.5 edges + 64), so the scratch block moves
    and the counts are taken again in the new one -- then the small map again.  "pip_column_entries" is the count the host
    computes from the edges' quantised boxes (one entry per strip a box touches: k_strip_count)."""
    w = want_of(oracle, "skew_rings")
    ctx = w["ctx"]
    sc = ctx.scaling
    g = synth.ring_map(400, 4000, 391)
    small = maps.ScaledMap(0, sc.scale(g.points), g.row_index, g.chains[:, 3], g.chains[:, 4])
    q = ctx.maps[1]
    o_small = oracle.Map(small.pts, small.row_index, small.left, small.right)
    want_small = oracle.pip_brute(o_small, 1, q.pts)
    h = _capi.Handle(0)
    try:
        h.upload_map(1, q.pts, q.row_index, q.left, q.right)
        closest, faces = h.alloc(4 * q.n_points), h.alloc(4 * q.n_points)

        def build_and_check(m, om, want, shift):
            h.upload_map(0, m.pts, m.row_index, m.left, m.right)
            h.set_debug_option("strip_shift", shift)
            h.build_lbvh(0)
            assert h.get_option("pip_columns_used0") == 1 and h.get_option("skyline_used0") == 1
            got_shift = h.get_option("pip_column_shift0")
            assert got_shift == (shift or got_shift)
            entries = h.get_option("pip_column_entries0")
            assert entries == S.column_entries(m, got_shift), (entries, got_shift)
            for rep in range(2):
                h.pip_query(0, 1, None, 0, q.n_points, closest, faces)
                assert h.get_option("pip_last_columns") == 1
                assert np.array_equal(closest.to_host(np.uint32), want), (shift, rep)
                assert np.array_equal(faces.to_host(np.int32), om.face_ids(want)), (shift, rep)
            return entries, h.get_option("leaf_slots0")

        build_and_check(small, o_small, want_small, 0)
        big = ctx.maps[0]
        entries, slots = build_and_check(big, w["om"][0], w["closest"][0, "vertices"], 15)
        assert entries > min(2 * slots, 5 * big.n_edges // 2 + 64), (entries, slots)   # the estimate was short: the re-count branch
        build_and_check(small, o_small, want_small, 0)
        build_and_check(big, w["om"][0], w["closest"][0, "vertices"], 17)
    finally:
        h.close()


# ---- the lazy column build --------------------------------------------------------------------------------------------------
def _lazy_handle(ctx, **options):
    h = _capi.Handle(0)
    upload(h, ctx)
    h.set_option("pip_columns", -1)
    for k, v in options.items():
        h.set_option(k, v)
    h.set_debug_option("lazy_columns_min", 1000)
    return h


def test_lazy_columns_on_the_skewed_lattice(oracle):
    """long chains: no columns at the build; the first incoherent caller array builds them and the plan says so"""
    w = want_of(oracle, "skew_lattice")
    h = _lazy_handle(w["ctx"])
    try:
        for base in (0, 1):
            h.build_lbvh(base)
            assert h.get_option("pip_columns_used%d" % base) == 0
            P = Points(h, w, base)
            P.check("vertices", ("lazy", base))      # the map's own, coherent vertices: nothing is built
            assert h.get_option("pip_columns_used%d" % base) == 0 and h.get_option("pip_last_columns") == 0
            P.check("random", ("lazy", base))
            ix = h.get_plan()["index"][base]
            assert ix["columns"] and "incoherent" in ix["columns_why"], ix
            assert h.get_option("pip_columns_used%d" % base) == 1 and h.get_option("pip_last_columns") == 1
            assert h.get_option("pip_column_entries%d" % base) == S.column_entries(w["ctx"].maps[base], h.get_option("pip_column_shift%d" % base))
            assert h.get_option("query_last_ordered") == 0
            for which in ("shuffled", "vertices", "random"):
                P.check(which, ("lazy, built", base))
                assert h.get_option("pip_last_columns") == 1
    finally:
        h.close()


def test_lazy_columns_decline_on_the_framed_rings(oracle):
    """the build declined already; every incoherent query tries again, declines again and sorts its points: exact answers on
    consecutive queries, and the skyline the build filled from the leaf boxes stays in use"""
    w = want_of(oracle, "rings_frame")
    h = _lazy_handle(w["ctx"])
    try:
        h.build_lbvh(0)
        assert h.get_option("pip_columns_used0") == 0 and h.get_option("skyline_used0") == 1
        P = Points(h, w, 0)
        for which in ("random", "shuffled", "random", "vertices"):
            P.check(which, ("lazy, declined", which))
            assert h.get_option("pip_columns_used0") == 0 and h.get_option("pip_last_columns") == 0
            assert h.get_option("skyline_used0") == 1
            assert "wanted, not built" in h.get_plan()["index"][0]["columns_why"]
    finally:
        h.close()


def test_lazy_columns_keep_a_skyline_the_build_filled(oracle):
    """"skyline" 1 on a lattice: filled at the build from the leaf boxes.  The lazy column build passes no skyline of its own
    and used to switch the filled one off ("skyline_used" flipped to 0 without a rebuild)."""
    ctx = maps.Context([synth.lattice_map(14, 60, 51), synth.lattice_map(30, 25, 52)]).load()
    b, q = ctx.maps
    ob = oracle.Map(b.pts, b.row_index, b.left, b.right)
    rnd = np.ascontiguousarray(synth.generate_pip_queries(ctx.bb, ctx.scaling, 30000, 7))
    want_rnd, want_own = oracle.pip_brute(ob, 1, rnd), oracle.pip_brute(ob, 1, q.pts)
    h = _lazy_handle(ctx, skyline=1)
    try:
        h.build_lbvh(0)
        assert h.get_option("pip_columns_used0") == 0 and h.get_option("skyline_used0") == 1
        d = h.alloc(16 * len(rnd)).from_host(rnd)
        n_out = max(len(rnd), q.n_points)
        closest, faces = h.alloc(4 * n_out), h.alloc(4 * n_out)
        for rep in range(2):
            h.pip_query(0, 1, d, 0, len(rnd), closest, faces)
            assert np.array_equal(closest.to_host(np.uint32, len(rnd)), want_rnd), rep
            assert np.array_equal(faces.to_host(np.int32, len(rnd)), ob.face_ids(want_rnd)), rep
            assert h.get_option("pip_columns_used0") == 1 and h.get_option("pip_last_columns") == 1
            assert h.get_option("skyline_used0") == 1, "the lazy column build switched a filled skyline off"
            assert h.get_plan()["index"][0]["skyline"] is True
        h.pip_query(0, 1, None, 0, q.n_points, closest, faces)
        assert np.array_equal(closest.to_host(np.uint32, q.n_points), want_own)
    finally:
        h.close()


# ---- the device grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["skew_lattice", "thin_band", "outlier"])
def test_device_grid_with_nearly_all_edges_in_a_handful_of_cells(oracle, name):
    w = want_of(oracle, name)
    ctx, om, brute = w["ctx"], w["om"], w["pairs"]
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        dctx.BuildIndex(1)
        for g in (256, 2048):
            want = oracle.lsi_grid(om[0], om[1], g)["eid"]
            if name == "outlier":   # long x long crossings: the grid path's own subset (the reference's wrap regime), not brute force
                assert len(want) < len(brute)
            else:
                assert np.array_equal(want, brute)
            assert dctx.BuildGrid(g) > 0
            lsi = ops.LSIGrid(dctx)
            lsi.Init(len(brute) + 64)
            assert lsi.Query() == len(want), (name, g)
            assert np.array_equal(lsi.get_pairs(), want), (name, g)
            lb = ops.LSILBVH(dctx)
            lb.Init(len(brute) + 64)
            lb.Query(1)
            assert np.array_equal(lb.get_pairs(), brute), (name, g)
            for qm in (1, 0):
                base = 1 - qm
                pts = ctx.maps[qm].pts
                want_e = oracle.pip_grid(om[base], base, pts, g)
                assert np.array_equal(want_e, w["closest"][base, "vertices"])
                pip = ops.PIPGrid(dctx)
                pip.Init(max(len(pts), N_RANDOM))
                pip.Query(qm)
                assert np.array_equal(pip.get_closest_eids(), want_e), (name, g, qm)
                assert np.array_equal(pip.get_face_ids(), om[base].face_ids(want_e)), (name, g, qm)
                lbp = ops.PIPLBVH(dctx)
                lbp.Init(len(pts))
                lbp.Query(qm)
                assert np.array_equal(lbp.get_closest_eids(), want_e), (name, g, qm)
                rnd = w["pts"][base, "random"]
                pip.Query(qm, query_points=rnd)
                assert np.array_equal(pip.get_closest_eids(), w["closest"][base, "random"]), (name, g, qm, "random")
    finally:
        dctx.close()


# ---- the overlay on the overlay-valid families ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.OVERLAY_VALID)
def test_overlay_tables_maps_and_a_cascade(oracle, name):
    import overlay_faces_ref as F
    import overlay_ops_ref as R
    from test_gpu_overlay_fuzz import assert_records, check_cascade, oracle_pipeline, second_context, third_lattice
    from test_gpu_overlay_hard import run_overlay
    from test_gpu_overlay_map import counts_of, host_arrays
    from test_gpu_overlay_ops import as_rows, raw_op_map, raw_op_rows
    from test_overlay_map import assert_same_map
    ctx = S.family(name)
    assert ctx.skew["grid_ok"]
    gsize = 256
    pairs, xs, pip = oracle_pipeline(oracle, ctx, gsize, False)
    all_ = R.all_pieces(ctx.maps, xs, pip)
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx, None, len(pairs))
        assert_records(ov, xs, pip, (name,))
        cascaded = False
        for how, by in (("intersection", "pair"), ("union", "map0")):
            want_rows = R.face_rows(all_, how, by)
            assert len(want_rows) >= 100
            if (how, by) == ("intersection", "pair"):
                assert as_rows(ov.FaceTable()) == F.rows(F.face_table(ctx.maps, xs, pip)), (name, "without _op")
                assert raw_op_rows(ov, how, by, len(want_rows) + 8) == want_rows, (name, how, by)
            else:
                assert as_rows(ov.FaceTable(how=how, by=by)) == want_rows, (name, how, by)
            for drop in (False, True):
                want = R.output_map(all_, how, by, drop_degenerate=drop)
                om = raw_op_map(ov, how, by, drop) if (how, by) == ("intersection", "pair") else ov.OutputMap(drop_degenerate=drop, how=how, by=by)
                assert (om.n_chains, om.n_points, om.n_faces) == counts_of(want), (name, how, by, drop)
                assert_same_map(host_arrays(om), want)
                if drop and by == "map0":   # the union by map 0, pieces dropped, as map 0 of a second overlay with a third lattice
                    third = third_lattice(ctx, 6, 120, 393)
                    d2 = ops.DeviceContext(second_context(ctx, None, third)).LoadToDevice()
                    try:
                        d2.InstallMap(0, om)
                        om.free()
                        check_cascade(oracle, ctx, d2, want, third, gsize, False, (name, "cascade"))
                        cascaded = True
                    finally:
                        d2.close()
                else:
                    om.free()
        assert cascaded
    finally:
        dctx.close()


# ---- fuzz: random compositions ----------------------------------------------------------------------------------------------
def fuzz_one(oracle, rng, what):
    """one random heterogeneous pair with the knobs of tests/fuzz_more.py drawn at random, against brute force"""
    from test_gpu_fuzz import _maps
    from test_gpu_overlay_fuzz import _draw_small   # (the five kinds of test_gpu_fuzz._draw, drawn smaller: brute force stays at seconds)
    ctx = S.fuzz_pair(rng, lambda r: _maps(r, _draw_small))
    m = ctx.maps
    om = S.oracle_maps(oracle, ctx)
    want_pairs = oracle.lsi_brute(om[0], om[1])
    h = _capi.Handle(0)
    try:
        upload(h, ctx)
        cap = max(1024, len(want_pairs) + 64)
        pairs = h.alloc(8 * cap)
        for base in (0, 1):
            q = m[1 - base]
            want = oracle.pip_brute(om[base], 1 - base, q.pts)
            shuffled = np.ascontiguousarray(q.pts[rng.permutation(q.n_points)])
            want_sh = oracle.pip_brute(om[base], 1 - base, shuffled)
            closest, faces = h.alloc(4 * q.n_points), h.alloc(4 * q.n_points)
            dsh = h.alloc(16 * q.n_points).from_host(shuffled)
            knobs = {"leaf_ysort": int(rng.integers(0, 2)), "lsi_segments": int(rng.integers(1, 3)), "pip_columns": int(rng.integers(-1, 2)),
                     "pip_walk_points": int(rng.integers(1, 3))}
            for k, v in knobs.items():
                h.set_option(k, v)
            lazy = int(rng.integers(0, 2)) * 64
            h.set_debug_option("lazy_columns_min", lazy)
            h.build_lbvh(base)
            tag = what + (base, tuple(sorted(knobs.items())), lazy, m[0].n_edges, m[1].n_edges, ctx.skew["frame"])
            if base in ctx.skew["frame"]:
                assert h.get_option("pip_columns_used%d" % base) == 0, tag
            n = h.lsi_query(base, 1 - base, 0, q.n_edges, cap, pairs)
            h.sort_pairs(pairs, n)
            assert np.array_equal(pairs.to_host(np.uint32, 2 * n).reshape(-1, 2), want_pairs), tag
            for rep in range(2):
                for dev, w in ((None, want), (dsh, want_sh)):
                    h.pip_query(base, 1 - base, dev, 0, q.n_points, closest, faces)
                    assert np.array_equal(closest.to_host(np.uint32, q.n_points), w), (tag, rep, dev is not None)
                    assert np.array_equal(faces.to_host(np.int32, q.n_points), om[base].face_ids(w)), (tag, rep, dev is not None)
    finally:
        h.close()
    return m[0].n_edges, m[1].n_edges, len(want_pairs), ctx.skew["frame"]


FUZZ_SEEDS = [201, 202, 203, 204, 205, 206]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_compositions_equal_brute_force(oracle, seed):
    rng = np.random.default_rng(seed)
    for k in range(3):
        print(seed, k, fuzz_one(oracle, rng, (seed, k)))
