"""The overlay's output map on the device (rj_overlay_map, ops.MapOverlay.OutputMap, polyover_exec -output_map) and maps
uploaded from device memory (rj_upload_map_dev, ops.DeviceContext.InstallMap) against the plain-Python helper
(tests/overlay_map_ref.py) fed the CPU oracle's records: the same arrays, bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_map_ref as M  # noqa: E402
from test_overlay_map import PAIRS, assert_same_map, pair  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")

pytestmark = pytest.mark.gpu


def run_overlay(dctx, grid_size=None):
    ov = ops.MapOverlay(dctx, grid_size).Init(1.0)
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    return ov


def host_arrays(om):
    m, face_pairs, origin = om.to_host()
    return dict(xy=m.pts, row_index=m.row_index, left=m.left.astype(np.int32), right=m.right.astype(np.int32), face_pairs=face_pairs,
                origin=origin)


def counts_of(want):
    return (len(want["left"]), len(want["xy"]), len(want["face_pairs"]))


@pytest.mark.parametrize("name", PAIRS)
def test_device_map_equals_the_helper(oracle, name):
    gs, gsize = pair(name)
    ctx = maps.Context(gs).load()
    xs, pip = F.oracle_records(oracle, ctx, gsize)
    for grid_size in (gsize, None):
        dctx = ops.DeviceContext(ctx).LoadToDevice()
        try:
            ov = run_overlay(dctx, grid_size)
            dxs, dpip = [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)]
            table = ov.FaceTable()
            for drop in (False, True):
                om = ov.OutputMap(drop_degenerate=drop)
                got = host_arrays(om)
                # the chain walk over the device's own records and vertex faces
                own = M.output_map(ctx.maps, dxs, dpip, drop_degenerate=drop)
                assert (om.n_chains, om.n_points, om.n_faces) == counts_of(own)
                assert_same_map(got, own)
                # -mode=grid records are the oracle's, bit for bit; the LBVH's too but on the nested pair (two touching
                # pairs at shared vertices the grid does not find)
                if grid_size or name != "nested":
                    assert ov.n_xsects == len(xs[0])
                    assert_same_map(got, M.output_map(ctx.maps, xs, pip, drop_degenerate=drop))
                # face k is row k - 1 of the face table
                assert np.array_equal(got["face_pairs"][:, 0], table["face0"]) and np.array_equal(got["face_pairs"][:, 1], table["face1"])
                if name == "nested" and grid_size:
                    assert own["n_one_point"] == 264 and (om.n_chains == 1359 - 264 if drop else om.n_chains == 1359)
                om.free()
        finally:
            dctx.close()


def test_each_capacity_one_short_overflows_with_the_true_counts(oracle):
    gs, gsize = pair("sample")
    ctx = maps.Context(gs).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        for drop in (False, True):
            full = ov.OutputMap(drop_degenerate=drop)
            true = (full.n_chains, full.n_points, full.n_faces)
            want = host_arrays(full)
            # the sizing call: all capacities 0, no arrays
            with pytest.raises(_capi.MapOverflow) as e:
                ov.h.overlay_map(ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(drop), (0, 0, 0), None, None,
                                 None, None, None, None)
            assert e.value.counts == true and e.value.code == _capi.RJ_E_OVERFLOW
            for short in range(3):
                caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
                with pytest.raises(_capi.MapOverflow) as e:
                    ov.OutputMap(drop_degenerate=drop, capacities=caps)
                assert e.value.counts == true
            # nothing beyond a capacity: arrays one entry longer than the short capacities keep their canary
            cc, pc, fc = true[0] - 1, true[1] - 1, true[2] - 1
            canary = np.full(4, 0x5A5A5A5A, np.uint32)
            bufs = []
            for nbytes in (16 * pc, 4 * (cc + 1), 4 * cc, 4 * cc, 8 * fc, 4 * cc):
                b = ov.h.alloc(nbytes + 16)
                ov.h._check(_capi.load().rj_memcpy_h2d(ov.h.h, b.ptr + nbytes, canary.ctypes.data, 16))
                bufs.append((b, nbytes))
            with pytest.raises(_capi.MapOverflow):
                ov.h.overlay_map(ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(drop), (cc, pc, fc),
                                 *[b for b, _ in bufs])
            for b, nbytes in bufs:
                assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary)
                b.free()
            exact = ov.OutputMap(drop_degenerate=drop, capacities=true)
            assert_same_map(host_arrays(exact), want)
    finally:
        dctx.close()


def test_disjoint_maps_and_a_map_inside_one_face(oracle):
    # disjoint: no intersection, no vertex inside the other map -> an empty map
    a = synth.lattice_map(3, 5, 81, bbox=(-120.0, 30.0, -110.0, 40.0))
    b = synth.lattice_map(4, 5, 82, bbox=(-100.0, 30.0, -90.0, 40.0))
    dctx = ops.DeviceContext(maps.Context([a, b]).load()).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        for drop in (False, True):
            om = ov.OutputMap(drop_degenerate=drop)
            assert ov.n_xsects == 0 and (om.n_chains, om.n_points, om.n_faces) == (0, 0, 0)
            assert om.row_index.to_host(np.uint32, 1).tolist() == [0]
    finally:
        dctx.close()
    # map 1 inside the one face of map 0: n == 0, every chain of map 1 whole, none of map 0
    big = synth.lattice_map(1, 8, 83, bbox=(-130.0, 20.0, -80.0, 50.0), vertex_jitter=0.0)
    small = synth.lattice_map(3, 5, 84, bbox=(-110.0, 30.0, -100.0, 40.0))
    ctx = maps.Context([big, small]).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        assert ov.n_xsects == 0
        dxs, dpip = [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)]
        for drop in (False, True):
            got = host_arrays(ov.OutputMap(drop_degenerate=drop))
            assert_same_map(got, M.output_map(ctx.maps, dxs, dpip, drop_degenerate=drop))
            m1 = ctx.maps[1]
            assert np.array_equal(got["xy"], m1.pts) and np.array_equal(got["row_index"], m1.row_index)
            assert got["face_pairs"].tolist() == [[1, f] for f in range(1, 10)]
            assert np.array_equal(got["left"], m1.left.astype(np.int32)) and np.array_equal(got["right"], m1.right.astype(np.int32))
            assert np.array_equal(got["origin"], (1 << 31) | np.arange(m1.n_chains, dtype=np.uint32))
    finally:
        dctx.close()


def _queries(h, b, q):
    """LSI pairs (sorted), PIP closest edges and faces of map 1 against map 0, and the plan's index entry"""
    h.build_lbvh(0)
    cap = b.n_edges + q.n_edges
    pairs, closest, faces = h.alloc(8 * cap), h.alloc(4 * q.n_points), h.alloc(4 * q.n_points)
    n = h.lsi_query(0, 1, 0, q.n_edges, cap, pairs)
    h.sort_pairs(pairs, n)
    h.pip_query(0, 1, None, 0, q.n_points, closest, faces)
    plan = h.get_plan()
    return (pairs.to_host(np.uint32, 2 * n).reshape(-1, 2), closest.to_host(np.uint32, q.n_points), faces.to_host(np.int32, q.n_points),
            plan["index"])


def _upload_dev(h, im, m, xy=None, row_index=None):
    xy = m.pts if xy is None else xy
    row_index = m.row_index if row_index is None else row_index
    bufs = [h.alloc(max(16, xy.nbytes)).from_host(xy), h.alloc(4 * len(row_index)).from_host(row_index),
            h.alloc(4 * m.n_chains).from_host(m.left.astype(np.int32)), h.alloc(4 * m.n_chains).from_host(m.right.astype(np.int32))]
    try:
        h.upload_map_dev(im, bufs[0], xy.shape[0], bufs[1], bufs[2], bufs[3], m.n_chains)
    finally:
        for b in bufs:  # (copied device to device: the caller's arrays may go)
            b.free()


def test_upload_map_dev_equals_upload_map():
    ctx = maps.Context([synth.lattice_map(12, 60, 91), synth.lattice_map(20, 25, 92)]).load()
    b, q = ctx.maps
    h = _capi.Handle(0)
    try:
        h.upload_map(0, b.pts, b.row_index, b.left, b.right)
        h.upload_map(1, q.pts, q.row_index, q.left, q.right)
        want = _queries(h, b, q)
        assert len(want[0]) > 100
        _upload_dev(h, 0, b)
        assert not h.get_plan()["index"][0]["built"]  # the index of the map that was there is gone
        _upload_dev(h, 1, q)
        assert h.map_num_edges(0) == b.n_edges and h.map_num_points(1) == q.n_points
        got = _queries(h, b, q)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w)
        assert got[3] == want[3] and got[3][0]["built"]  # the index plan: levels, slots, leaf order, columns
    finally:
        h.close()


def test_upload_map_dev_refuses_what_upload_map_refuses():
    ctx = maps.Context([synth.lattice_map(12, 60, 91), synth.lattice_map(20, 25, 92)]).load()
    b, q = ctx.maps
    h = _capi.Handle(0)
    try:
        h.upload_map(0, b.pts, b.row_index, b.left, b.right)
        h.upload_map(1, q.pts, q.row_index, q.left, q.right)
        want = _queries(h, b, q)
        r_start = q.row_index.copy(); r_start[0] = 1
        r_end = q.row_index.copy(); r_end[-1] -= 1
        r_short = q.row_index.copy(); r_short[1] = r_short[0] + 1
        xy_big = q.pts.copy(); xy_big[7, 1] = 1 << 46
        xy_small = q.pts.copy(); xy_small[3, 0] = -(1 << 46) - 1
        for kw, text in ((dict(row_index=r_start), "start at 0"), (dict(row_index=r_end), "end at np"),
                         (dict(row_index=r_short), "fewer than 2 points"), (dict(xy=xy_big), "scaled range"),
                         (dict(xy=xy_small), "scaled range")):
            with pytest.raises(_capi.RayJoinError) as e:
                _upload_dev(h, 1, q, **kw)
            assert e.value.code == _capi.RJ_E_INVALID and text in str(e.value), str(e.value)
            # the same input through the host entry point is refused too
            with pytest.raises(_capi.RayJoinError) as e2:
                h.upload_map(1, kw.get("xy", q.pts), kw.get("row_index", q.row_index), q.left, q.right)
            assert e2.value.code == _capi.RJ_E_INVALID
        edge = q.pts.copy(); edge[3, 0] = -(1 << 46); edge[7, 1] = (1 << 46) - 1  # the range's ends are inside
        _upload_dev(h, 1, q, xy=edge)
        # the handle still works: the maps again, the same answers
        _upload_dev(h, 1, q)
        got = _queries(h, b, q)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w)
    finally:
        h.close()


def test_cascade_a_x_b_then_x_c(oracle):
    """(A x B) x C without the geometry leaving the GPU: lattices in general position, ONE Scaling over the three boxes.
    Records, vertex faces and FaceTable() of the second overlay equal the CPU oracle pipeline run on the helper's
    A x B map.  (Areas of the three-way table only approximate the two-way areas: the second overlay's cut points are
    truncated again; asserted here: equality with the oracle run, and positivity.)"""
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

    # CPU: the helper's A x B, then the oracle pipeline on (A x B) x C
    ctx1 = context(scaled(0, A), scaled(1, B))
    xs1, pip1 = F.oracle_records(oracle, ctx1, gsize)
    ab = M.output_map(ctx1.maps, xs1, pip1, drop_degenerate=True)
    assert counts_of(ab) == (481, int(ab["row_index"][-1]), 216) and ab["n_one_point"] == 0
    ctx2 = context(M.as_scaled_map(ab, 0), scaled(1, Cg))
    want_rows, xs2, pip2 = F.oracle_face_rows(oracle, ctx2, gsize)
    assert len(xs2[0]) == 133 and len(want_rows) == 326 and all(a > 0 for _, _, a in want_rows)

    # GPU: A x B, installed as map 0 from device memory, x C
    d1 = ops.DeviceContext(ctx1).LoadToDevice()
    d2 = ops.DeviceContext(context(None, scaled(1, Cg)))
    try:
        ov1 = run_overlay(d1, gsize)
        om = ov1.OutputMap(drop_degenerate=True)
        assert_same_map(host_arrays(om), ab)
        d2.LoadToDevice()
        d2.InstallMap(0, om)
        om.free()
        installed = d2.get_map(0)
        assert np.array_equal(installed.pts, ab["xy"]) and np.array_equal(installed.row_index, ab["row_index"])
        ov2 = run_overlay(d2, gsize)
        assert ov2.n_xsects == 133
        for im in range(2):
            assert np.array_equal(ov2.get_xsects(im), xs2[im])
            assert np.array_equal(ov2.get_vertex_faces(im), np.asarray(pip2[im], dtype=np.int32))
        t = ov2.FaceTable()
        got_rows = [(int(a), int(b), int(c)) for a, b, c in zip(t["face0"], t["face1"], t["area2"])]
        assert got_rows == want_rows and all(a > 0 for _, _, a in got_rows)
        # and the three-way output map itself
        abc = ov2.OutputMap(drop_degenerate=True)
        assert_same_map(host_arrays(abc), M.output_map(ctx2.maps, xs2, pip2, drop_degenerate=True))
    finally:
        d1.close()
        d2.close()


def _phases(stderr):
    return re.findall(r"^ - (.*): [-+.e0-9]+ ms$", stderr, flags=re.M)


@pytest.mark.parametrize("name", ["sample", "lattice"])
def test_polyover_exec_output_map(oracle, tmp_path, name):
    """-output_map writes the device map as a CDB file that maps.read_cdb loads: chain and point counts and face ids are
    the device map's; end points are numbered over the distinct scaled end points in first-use order.  Without the flag
    -output and the stderr phases are what they were."""
    gs, gsize = pair(name)
    if name == "sample":
        p0, p1 = os.path.join(D, "map0.cdb"), os.path.join(D, "map1.cdb")
    else:
        p0, p1 = str(tmp_path / "a.cdb"), str(tmp_path / "b.cdb")
        maps.write_cdb(p0, gs[0], "%.9f")
        maps.write_cdb(p1, gs[1], "%.9f")
    ctx = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load()
    xs, pip = F.oracle_records(oracle, ctx, gsize)
    want = M.output_map(ctx.maps, xs, pip)
    out, omp = str(tmp_path / "o.txt"), str(tmp_path / "om.cdb")
    base = [EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-xsect_factor", "1.0"]
    r = subprocess.run(base + ["-output", out, "-output_map", omp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert " - Compute output map: " in r.stderr and " - Write output map: " in r.stderr
    g = maps.read_cdb(omp)
    assert g.n_chains == len(want["left"]) and g.points.shape[0] == len(want["xy"])
    assert np.array_equal(g.row_index, want["row_index"])
    assert np.array_equal(g.chains[:, 3], want["left"]) and np.array_equal(g.chains[:, 4], want["right"])
    ids = {}
    ends = []
    for k in range(len(want["left"])):
        b, e = int(want["row_index"][k]), int(want["row_index"][k + 1])
        ends.append([ids.setdefault(tuple(want["xy"][p].tolist()), len(ids)) for p in (b, e - 1)])
    assert np.array_equal(g.chains[:, 1:3], np.array(ends))
    assert np.abs(g.points - ctx.scaling.unscale(want["xy"])).max() <= 1e-6  # ("%.6f" of the unscaled points)
    # without the flag: the same -output bytes, the phases of before (the parent's list, in its order)
    out2 = str(tmp_path / "o2.txt")
    r2 = subprocess.run(base + ["-output", out2], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "output map" not in r2.stderr.lower() and r2.stdout == r.stdout
    assert open(out2, "rb").read() == open(out, "rb").read()
    assert _phases(r2.stderr) == ["Read map 0", "Read map 1", "Create App", "Load Data", "Init", "Build Index", "Intersection edges",
                                  "Map 0: Locate vertices in other map", "Map 1: Locate vertices in other map",
                                  "Computer output polygons", "Check result", "Write to file"]
    assert [p for p in _phases(r.stderr) if "output map" not in p] == _phases(r2.stderr)
