"""RJ_OVM_MERGE_PIECES on the device (rj_overlay_map / rj_overlay_map_op with the flag, ops.MapOverlay.OutputMap(merge=True),
polyover_exec -merge) on the families of tests/overlay_merge_pairs.py, through the LBVH and the -mode=grid record sources:
the merged arrays equal the plain-Python definition (tests/overlay_merge_ref.py) applied to the device's OWN unmerged
arrays, array for array; overflow, the sizing call, the flag check; the cascade through a merged map.  The CPU side is
tests/test_overlay_merge.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_merge_pairs as P  # noqa: E402
import overlay_merge_ref as G  # noqa: E402
from test_gpu_overlay_map import host_arrays, run_overlay  # noqa: E402
from test_overlay_map import PAIRS, assert_same_map, pair  # noqa: E402
from test_overlay_ops import code  # noqa: E402

pytestmark = pytest.mark.gpu

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")
MERGE, DROP = _capi.RJ_OVM_MERGE_PIECES, _capi.RJ_OVM_DROP_DEGENERATE
# clip, two unions, (identity, map1), and the plain intersection through the call without _op (None)
CALLS = [("intersection", "map0"), ("union", "map0"), ("union", "pair"), ("identity", "map1"), None]


def overlay_of(ctx, grid_size):
    """-> (dctx, ov) with a queue that holds every intersection (the tie families have more intersections than edges)"""
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    edges = sum(dctx.get_map(im).n_edges for im in range(2))
    ov = ops.MapOverlay(dctx, grid_size).Init(max(1.0, 4096.0 / edges))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    return dctx, ov


def raw_map(ov, call, flags, caps=None):
    """the call itself (rj_overlay_map for call None, else rj_overlay_map_op), a sizing call first when caps is None"""
    op = None if call is None else code(*call)
    args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(flags))
    if caps is None:
        try:
            caps = ov.h.overlay_map(*args, (0, 0, 0), None, None, None, None, None, None, op=op)
        except _capi.MapOverflow as e:
            caps = e.counts
    cc, pc, fc = (int(v) for v in caps)
    bufs = [ov.h.alloc(16 * max(1, pc)), ov.h.alloc(4 * (cc + 1)), ov.h.alloc(4 * max(1, cc)), ov.h.alloc(4 * max(1, cc)),
            ov.h.alloc(8 * max(1, fc)), ov.h.alloc(4 * max(1, cc))]
    counts = ov.h.overlay_map(*args, (cc, pc, fc), *bufs, op=op)
    return ops.DeviceOutputMap(*bufs, counts, bool(flags & DROP), bool(flags & MERGE))


def _arrays(ov, call, flags):
    om = raw_map(ov, call, flags)
    got = host_arrays(om)
    counts = (om.n_chains, om.n_points, om.n_faces)
    om.free()
    return got, counts


def _check_family(ctx, gsize, name, facts):
    for grid_size in (None, gsize):
        source = "grid" if grid_size else "lbvh"
        dctx, ov = overlay_of(ctx, grid_size)
        try:
            assert ov.n_xsects > 0 or name == "waves-ring1000"
            for call in CALLS:
                for drop in (0, DROP):
                    what = (name, source, call, drop)
                    unmerged, true = _arrays(ov, call, drop)
                    want = G.merged_map(unmerged, np_form=true[0] > 50000)  # (the lattice pair; test_overlay_merge holds the forms equal)
                    got, counts = _arrays(ov, call, drop | MERGE)
                    # the sizing call (inside raw_map) returned the merged counts, and so did the filling call
                    assert counts == (len(want["left"]), len(want["xy"]), true[2]), what
                    assert_same_map(got, want)
                    assert counts[2] == true[2] and np.array_equal(got["face_pairs"], unmerged["face_pairs"]), what
                    if drop:
                        assert np.diff(got["row_index"].astype(np.int64)).min(initial=2) >= 2, what
                    if call == P.CLIP and drop and "clip_chains" in facts and grid_size:
                        assert counts[0] == facts["clip_chains"], what  # (-mode=grid records are the oracle's)
            if "clip_chains" in facts:  # through ops, on either record source
                om = ov.OutputMap(drop_degenerate=True, how="intersection", by="map0", merge=True)
                assert om.merged and om.drop_degenerate and om.n_chains == facts["clip_chains"], (name, source)
                om.free()
        finally:
            dctx.close()


@pytest.mark.parametrize("name", P.NAMES)
def test_merged_arrays_equal_the_definition_on_the_families(oracle, name):
    facts = P.preconditions(oracle, name)
    ctx, gsize = P.family(name)
    _check_family(ctx, gsize, name, facts)


@pytest.mark.parametrize("name", PAIRS)
def test_merged_arrays_equal_the_definition_on_the_four_pairs(name):
    gs, gsize = pair(name)
    _check_family(maps.Context(gs).load(), gsize, name, {})


def test_each_capacity_one_short_overflows_with_the_true_merged_counts(oracle):
    """comb-64 (a run that ends on a wave boundary) and ties-0 (the most dropped pieces): chains and points one short"""
    for name in ("comb-64", "ties-0"):
        ctx, gsize = P.family(name)
        dctx, ov = overlay_of(ctx, None)
        try:
            for call in (P.CLIP, ("identity", "map1"), None):
                for drop in (0, DROP):
                    flags = drop | MERGE
                    want, true = _arrays(ov, call, flags)
                    unmerged_counts = _arrays(ov, call, drop)[1]
                    assert true[0] <= unmerged_counts[0] and true[1] <= unmerged_counts[1], (name, call, drop)
                    if name == "comb-64":  # the staged and the final counts differ
                        assert true[0] < unmerged_counts[0] and true[1] < unmerged_counts[1], (call, drop)
                    args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], flags)
                    op = None if call is None else code(*call)
                    with pytest.raises(_capi.MapOverflow) as e:  # the sizing call
                        ov.h.overlay_map(*args, (0, 0, 0), None, None, None, None, None, None, op=op)
                    assert e.value.counts == true and e.value.code == _capi.RJ_E_OVERFLOW
                    canary = np.full(4, 0x5A5A5A5A, np.uint32)
                    for short in range(3):
                        cc, pc, fc = (v - (1 if i == short else 0) for i, v in enumerate(true))
                        bufs = []
                        for nbytes in (16 * pc, 4 * (cc + 1), 4 * cc, 4 * cc, 8 * fc, 4 * cc):
                            b = ov.h.alloc(nbytes + 16)
                            ov.h._check(_capi.load().rj_memcpy_h2d(ov.h.h, b.ptr + nbytes, canary.ctypes.data, 16))
                            bufs.append((b, nbytes))
                        with pytest.raises(_capi.MapOverflow) as e:
                            ov.h.overlay_map(*args, (cc, pc, fc), *[b for b, _ in bufs], op=op)
                        assert e.value.counts == true, (name, call, drop, short)
                        for b, nbytes in bufs:
                            assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary), (name, call, drop, short)
                            b.free()
                    exact = raw_map(ov, call, flags, caps=true)
                    assert_same_map(host_arrays(exact), want)
                    exact.free()
        finally:
            dctx.close()


def test_unknown_flag_bits_stay_invalid():
    gs, _ = pair("sample")
    dctx = ops.DeviceContext(maps.Context(gs).load()).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1])
        for flags in (4, 4 | MERGE, 8 | DROP, 0x80000000):
            for op in (None, code("union", "pair")):
                with pytest.raises(_capi.RayJoinError) as e:
                    ov.h.overlay_map(*args, flags, (0, 0, 0), None, None, None, None, None, None, op=op)
                assert e.value.code == _capi.RJ_E_INVALID and "unknown flags" in str(e.value) and not isinstance(e.value, _capi.MapOverflow)
        om = ov.OutputMap(merge=True, drop_degenerate=True)  # the handle still works
        assert om.merged and om.n_chains > 0
        om.free()
    finally:
        dctx.close()


def test_disjoint_maps_merge_to_nothing_and_whole_chains_stay_whole():
    a = synth.lattice_map(3, 5, 81, bbox=(-120.0, 30.0, -110.0, 40.0))
    b = synth.lattice_map(4, 5, 82, bbox=(-100.0, 30.0, -90.0, 40.0))
    dctx = ops.DeviceContext(maps.Context([a, b]).load()).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        assert ov.n_xsects == 0
        for drop in (False, True):
            om = ov.OutputMap(drop_degenerate=drop, merge=True)
            assert (om.n_chains, om.n_points, om.n_faces) == (0, 0, 0) and om.row_index.to_host(np.uint32, 1).tolist() == [0]
            om.free()
            whole, merged = ov.OutputMap(drop_degenerate=drop, how="union"), ov.OutputMap(drop_degenerate=drop, how="union", merge=True)
            assert_same_map(host_arrays(merged), host_arrays(whole))  # uncut chains: nothing joins
            whole.free()
            merged.free()
    finally:
        dctx.close()


def test_cascade_through_the_merged_clip(oracle):
    """(A clip B) x C on the three general-position lattices of tests/test_gpu_overlay_map.py: the merged clip (with drop)
    installed as map 0 gives the face table of the same cascade through the unmerged clip, row for row, and the same
    number of intersections -- with fewer chains and points in between"""
    A, B, Cg = synth.lattice_map(6, 30, 71), synth.lattice_map(9, 20, 72), synth.lattice_map(4, 45, 73)
    gsize = 256
    bb = [min(g.bb[0] for g in (A, B, Cg)), min(g.bb[1] for g in (A, B, Cg)), max(g.bb[2] for g in (A, B, Cg)),
          max(g.bb[3] for g in (A, B, Cg))]
    sc = maps.Scaling(bb)

    def scaled(i, g):
        return maps.ScaledMap(i, sc.scale(g.points), g.row_index, g.chains[:, 3], g.chains[:, 4])

    def context(m0, m1):
        ctx = maps.Context([None, None])
        ctx.scaling = sc
        ctx.set_map(0, m0)
        ctx.set_map(1, m1)
        return ctx

    d1 = ops.DeviceContext(context(scaled(0, A), scaled(1, B))).LoadToDevice()
    try:
        ov1 = run_overlay(d1, gsize)
        results = {}
        for merge in (False, True):
            om = ov1.OutputMap(drop_degenerate=True, how="intersection", by="map0", merge=merge)
            d2 = ops.DeviceContext(context(None, scaled(1, Cg)))
            try:
                d2.LoadToDevice()
                d2.InstallMap(0, om)
                ov2 = run_overlay(d2, gsize)
                t = ov2.FaceTable()
                results[merge] = (om.n_chains, om.n_points, ov2.n_xsects,
                                  [(int(a), int(b), int(c)) for a, b, c in zip(t["face0"], t["face1"], t["area2"])])
            finally:
                om.free()
                d2.close()
        plain, merged = results[False], results[True]
        assert merged[0] < plain[0] and merged[1] < plain[1] and plain[0] - merged[0] == plain[1] - merged[1]
        assert merged[2] == plain[2] > 10
        assert merged[3] == plain[3] and len(merged[3]) > 10
    finally:
        d1.close()


def test_polyover_exec_merge(oracle, tmp_path):
    """-merge applies to -output_map: the file's chains are the merged device map's"""
    p0, p1 = os.path.join(D, "map0.cdb"), os.path.join(D, "map1.cdb")
    ctx = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        want = host_arrays(ov.OutputMap(how="intersection", by="map0", merge=True))
        plain = ov.OutputMap(how="intersection", by="map0")
        assert len(want["left"]) < plain.n_chains
    finally:
        dctx.close()
    omp = str(tmp_path / "om.cdb")
    r = subprocess.run([EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-xsect_factor", "1.0", "-by", "map0", "-merge", "-output_map", omp],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    g = maps.read_cdb(omp)
    assert g.n_chains == len(want["left"]) and np.array_equal(g.row_index, want["row_index"])
    assert np.array_equal(g.chains[:, 3], want["left"]) and np.array_equal(g.chains[:, 4], want["right"])
    assert np.abs(g.points - ctx.scaling.unscale(want["xy"])).max() <= 1e-6
