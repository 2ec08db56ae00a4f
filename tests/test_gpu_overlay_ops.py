"""The overlay operations on the device (rj_overlay_faces_op, rj_overlay_map_op, ops.MapOverlay.FaceTable / OutputMap with
how= / by=, polyover_exec -how / -by) against the plain-Python helper (tests/overlay_ops_ref.py) fed the CPU oracle's
records: the same arrays and the same int128 areas, bit for bit, for all 5 x 3 operations."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
from test_gpu_overlay_map import _phases, counts_of, host_arrays, run_overlay  # noqa: E402
from test_overlay_map import PAIRS, assert_same_map, pair  # noqa: E402
from test_overlay_ops import COUNTS, OPS, _invariants, code  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")

pytestmark = pytest.mark.gpu


def as_rows(t):
    return [(int(a), int(b), int(c)) for a, b, c in zip(t["face0"], t["face1"], t["area2"])]


def raw_op_map(ov, how, by, drop):
    """rj_overlay_map_op called with the operation's codes (also for (intersection, pair), which ops routes to the call
    without _op): a sizing call, then the arrays"""
    args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(drop))
    try:
        caps = ov.h.overlay_map(*args, (0, 0, 0), None, None, None, None, None, None, op=code(how, by))
    except _capi.MapOverflow as e:
        caps = e.counts
    cc, pc, fc = caps
    bufs = [ov.h.alloc(16 * max(1, pc)), ov.h.alloc(4 * (cc + 1)), ov.h.alloc(4 * max(1, cc)), ov.h.alloc(4 * max(1, cc)),
            ov.h.alloc(8 * max(1, fc)), ov.h.alloc(4 * max(1, cc))]
    counts = ov.h.overlay_map(*args, caps, *bufs, op=code(how, by))
    return ops.DeviceOutputMap(*bufs, counts, drop)


def raw_op_rows(ov, how, by, cap):
    out = ov.h.alloc(_capi.FACE_DTYPE.itemsize * max(1, cap))
    try:
        n = ov.h.overlay_faces(ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], cap, out, op=code(how, by))
        return as_rows(ops.face_table_from_rows(out.to_host(_capi.FACE_DTYPE, n), ov.ctx_.ctx.scaling))
    finally:
        out.free()


@pytest.mark.parametrize("name", PAIRS)
def test_device_arrays_equal_the_helper_for_every_operation(oracle, name):
    gs, gsize = pair(name)
    ctx = maps.Context(gs).load()
    xs, pip = F.oracle_records(oracle, ctx, gsize)
    all_oracle = R.all_pieces(ctx.maps, xs, pip)
    cache = {}  # the helper's answers on the oracle's records serve both record sources (a long Python loop on the lattice pair)

    def helper(all_, fn, *key):
        if all_ is not all_oracle:
            return fn(all_, *key)
        if (fn, key) not in cache:
            cache[fn, key] = fn(all_, *key)
        return cache[fn, key]

    for grid_size in (gsize, None):
        dctx = ops.DeviceContext(ctx).LoadToDevice()
        try:
            ov = run_overlay(dctx, grid_size)
            # -mode=grid records are the oracle's, bit for bit; the LBVH's too but on the nested pair (two touching pairs
            # at shared vertices the grid does not find): there the helper walks the device's own records
            if grid_size or name != "nested":
                assert ov.n_xsects == len(xs[0])
                all_ = all_oracle
            else:
                all_ = R.all_pieces(ctx.maps, [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)])
            tables = {}
            for how, by in OPS:
                want_rows = helper(all_, R.face_rows, how, by)
                tables[how, by] = as_rows(ov.FaceTable(how=how, by=by))
                assert tables[how, by] == want_rows, (how, by)
                for drop in (False, True):
                    want = helper(all_, R.output_map, how, by, drop)
                    om = ov.OutputMap(drop_degenerate=drop, how=how, by=by)
                    assert (om.n_chains, om.n_points, om.n_faces) == counts_of(want), (how, by, drop)
                    assert_same_map(host_arrays(om), want)
                    om.free()
                # the rows are the map's faces, in its order
                assert [r[:2] for r in want_rows] == [tuple(p) for p in want["face_pairs"].tolist()]
            # (intersection, pair) through the _op calls themselves, and the calls without _op: the same bits
            for drop in (False, True):
                new, old = raw_op_map(ov, "intersection", "pair", drop), ov.OutputMap(drop_degenerate=drop)
                assert_same_map(host_arrays(new), host_arrays(old))
                new.free()
                old.free()
            assert raw_op_rows(ov, "intersection", "pair", len(tables["intersection", "pair"])) == as_rows(ov.FaceTable())
            # the exact invariants, on the device's tables
            _invariants(ctx, all_, lambda how, by: tables[how, by])
            if name in COUNTS and grid_size:
                om = ov.OutputMap(how="union")
                assert (om.n_chains, om.n_faces) == (COUNTS[name][2], COUNTS[name][7])
                om.free()
        finally:
            dctx.close()


def test_each_capacity_one_short_overflows_with_the_true_counts(oracle):
    gs, gsize = pair("sample")
    ctx = maps.Context(gs).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        for how, by in (("union", "pair"), ("difference", "pair"), ("intersection", "map0"), ("intersection", "pair")):
            for drop in (False, True):
                full = raw_op_map(ov, how, by, drop)
                true = (full.n_chains, full.n_points, full.n_faces)
                want = host_arrays(full)
                args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(drop))
                with pytest.raises(_capi.MapOverflow) as e:  # the sizing call
                    ov.h.overlay_map(*args, (0, 0, 0), None, None, None, None, None, None, op=code(how, by))
                assert e.value.counts == true and e.value.code == _capi.RJ_E_OVERFLOW
                # nothing beyond a capacity: arrays one entry longer than the short capacities keep their canary
                canary = np.full(4, 0x5A5A5A5A, np.uint32)
                for short in range(3):
                    cc, pc, fc = (v - (1 if i == short else 0) for i, v in enumerate(true))
                    bufs = []
                    for nbytes in (16 * pc, 4 * (cc + 1), 4 * cc, 4 * cc, 8 * fc, 4 * cc):
                        b = ov.h.alloc(nbytes + 16)
                        ov.h._check(_capi.load().rj_memcpy_h2d(ov.h.h, b.ptr + nbytes, canary.ctypes.data, 16))
                        bufs.append((b, nbytes))
                    with pytest.raises(_capi.MapOverflow) as e:
                        ov.h.overlay_map(*args, (cc, pc, fc), *[b for b, _ in bufs], op=code(how, by))
                    assert e.value.counts == true
                    for b, nbytes in bufs:
                        assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary)
                        b.free()
                if (how, by) != ("intersection", "pair"):
                    exact = ov.OutputMap(drop_degenerate=drop, capacities=true, how=how, by=by)
                    assert_same_map(host_arrays(exact), want)
                full.free()
            rows = raw_op_rows(ov, how, by, 4096)
            with pytest.raises(_capi.QueueOverflow) as e:
                raw_op_rows(ov, how, by, len(rows) - 1)
            assert e.value.n_found == len(rows)
            assert raw_op_rows(ov, how, by, len(rows)) == rows
            if (how, by) != ("intersection", "pair"):
                with pytest.raises(_capi.QueueOverflow):
                    ov.FaceTable(capacity=len(rows) - 1, how=how, by=by)
    finally:
        dctx.close()


def test_disjoint_maps_and_a_map_inside_one_face(oracle):
    # disjoint: n == 0, no vertex inside the other map.  The union returns both maps whole, the intersection nothing
    a = synth.lattice_map(3, 5, 81, bbox=(-120.0, 30.0, -110.0, 40.0))
    b = synth.lattice_map(4, 5, 82, bbox=(-100.0, 30.0, -90.0, 40.0))
    ctx = maps.Context([a, b]).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        assert ov.n_xsects == 0
        all_ = R.all_pieces(ctx.maps, [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)])
        m0, m1 = ctx.maps
        for drop in (False, True):
            om = raw_op_map(ov, "intersection", "pair", drop)
            assert (om.n_chains, om.n_points, om.n_faces) == (0, 0, 0) and om.row_index.to_host(np.uint32, 1).tolist() == [0]
            got = host_arrays(ov.OutputMap(drop_degenerate=drop, how="union"))
            assert np.array_equal(got["xy"], np.concatenate([m0.pts, m1.pts]))
            assert np.array_equal(got["row_index"], np.r_[m0.row_index, m1.row_index[1:] + m0.n_points].astype(np.uint32))
            assert got["face_pairs"].tolist() == [[0, f] for f in range(1, 17)] + [[f, 0] for f in range(1, 10)]
            # map 1's faces are numbered first ((0, f) sorts before (f, 0)), map 0's after them
            assert np.array_equal(got["left"], np.r_[np.where(m0.left != 0, m0.left + 16, 0), m1.left].astype(np.int32))
            assert np.array_equal(got["right"], np.r_[np.where(m0.right != 0, m0.right + 16, 0), m1.right].astype(np.int32))
            for how, by in OPS:
                assert_same_map(host_arrays(ov.OutputMap(drop_degenerate=drop, how=how, by=by)), R.output_map(all_, how, by, drop))
        assert as_rows(ov.FaceTable(how="union")) == [(0, f, F.shoelace2(m1, f)) for f in range(1, 17)] + [
            (f, 0, F.shoelace2(m0, f)) for f in range(1, 10)]
        assert len(ov.FaceTable(how="symmetric_difference")) == 25 and len(ov.FaceTable(how="intersection", by="map0")) == 0
    finally:
        dctx.close()
    # map 1 inside the one face of map 0: n == 0; the difference is map 0's face with map 1's outline as a hole
    big = synth.lattice_map(1, 8, 83, bbox=(-130.0, 20.0, -80.0, 50.0), vertex_jitter=0.0)
    small = synth.lattice_map(3, 5, 84, bbox=(-110.0, 30.0, -100.0, 40.0))
    ctx = maps.Context([big, small]).load()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        assert ov.n_xsects == 0
        all_ = R.all_pieces(ctx.maps, [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)])
        for how, by in OPS:
            assert as_rows(ov.FaceTable(how=how, by=by)) == R.face_rows(all_, how, by)
            for drop in (False, True):
                assert_same_map(host_arrays(ov.OutputMap(drop_degenerate=drop, how=how, by=by)), R.output_map(all_, how, by, drop))
        inner = sum(F.shoelace2(ctx.maps[1], f) for f in range(1, 10))
        assert as_rows(ov.FaceTable(how="difference")) == [(1, 0, F.shoelace2(ctx.maps[0], 1) - inner)]
        assert as_rows(ov.FaceTable(how="intersection", by="map0")) == [(1, 0, inner)]
        assert as_rows(ov.FaceTable(how="identity", by="map0")) == [(1, 0, F.shoelace2(ctx.maps[0], 1))]
    finally:
        dctx.close()


def test_unknown_how_and_by_are_invalid(oracle):
    gs, _ = pair("sample")
    dctx = ops.DeviceContext(maps.Context(gs).load()).LoadToDevice()
    try:
        ov = run_overlay(dctx)
        args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1])
        out = ov.h.alloc(24 * 1024)
        for op in ((5, 0), (0, 3), (0xFFFFFFFF, 0), (1, 0xFFFFFFFF)):
            with pytest.raises(_capi.RayJoinError) as e:
                ov.h.overlay_faces(*args, 1024, out, op=op)
            assert e.value.code == _capi.RJ_E_INVALID and ("unknown how" in str(e.value) or "unknown by" in str(e.value))
            with pytest.raises(_capi.RayJoinError) as e:
                ov.h.overlay_map(*args, 0, (0, 0, 0), None, None, None, None, None, None, op=op)
            assert e.value.code == _capi.RJ_E_INVALID and not isinstance(e.value, _capi.MapOverflow)
        with pytest.raises(ValueError):
            ov.FaceTable(how="xor")
        with pytest.raises(ValueError):
            ov.OutputMap(by="map2")
        assert len(ov.FaceTable(how="union")) == 223  # the handle still works
    finally:
        dctx.close()


def test_cascade_a_minus_b_then_x_c(oracle):
    """(A - B) x C without the geometry leaving the GPU: InstallMap of OutputMap(how="difference", drop_degenerate=True),
    then an overlay with a third lattice finds the oracle pipeline's records, vertex faces and face table on the helper's
    A - B map.  ONE Scaling over the three boxes."""
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

    ctx1 = context(scaled(0, A), scaled(1, B))
    xs1, pip1 = F.oracle_records(oracle, ctx1, gsize)
    diff = R.output_map(R.all_pieces(ctx1.maps, xs1, pip1), "difference", "pair", drop_degenerate=True)
    assert len(diff["left"]) > 10 and all(b == 0 for _, b in diff["face_pairs"].tolist())
    ctx2 = context(M.as_scaled_map(diff, 0), scaled(1, Cg))
    want_rows, xs2, pip2 = F.oracle_face_rows(oracle, ctx2, gsize)
    assert len(xs2[0]) > 10 and len(want_rows) > 10

    d1 = ops.DeviceContext(ctx1).LoadToDevice()
    d2 = ops.DeviceContext(context(None, scaled(1, Cg)))
    try:
        ov1 = run_overlay(d1, gsize)
        om = ov1.OutputMap(how="difference", drop_degenerate=True)
        assert_same_map(host_arrays(om), diff)
        d2.LoadToDevice()
        d2.InstallMap(0, om)
        om.free()
        ov2 = run_overlay(d2, gsize)
        assert ov2.n_xsects == len(xs2[0])
        for im in range(2):
            assert np.array_equal(ov2.get_xsects(im), xs2[im])
            assert np.array_equal(ov2.get_vertex_faces(im), np.asarray(pip2[im], dtype=np.int32))
        assert as_rows(ov2.FaceTable()) == want_rows
        all2 = R.all_pieces(ctx2.maps, xs2, pip2)
        assert as_rows(ov2.FaceTable(how="union")) == R.face_rows(all2, "union", "pair")
        assert_same_map(host_arrays(ov2.OutputMap(how="identity", by="map0", drop_degenerate=True)),
                        R.output_map(all2, "identity", "map0", drop_degenerate=True))
    finally:
        d1.close()
        d2.close()


def _face_text(rows, scaling):
    return F.text(rows, scaling)


def test_polyover_exec_how_and_by(oracle, tmp_path):
    """-how / -by apply to -face_table and -output_map; without them both files and the phases are what they were"""
    gs, gsize = pair("sample")
    p0, p1 = os.path.join(D, "map0.cdb"), os.path.join(D, "map1.cdb")
    ctx = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load()
    xs, pip = F.oracle_records(oracle, ctx, gsize)
    all_ = R.all_pieces(ctx.maps, xs, pip)
    base = [EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-xsect_factor", "1.0"]

    def run(tag, extra):
        out, ft, omp = (str(tmp_path / (tag + s)) for s in (".o.txt", ".faces.txt", ".om.cdb"))
        r = subprocess.run(base + ["-output", out, "-face_table", ft, "-output_map", omp] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r, open(out, "rb").read(), open(ft).read(), omp

    plain = run("plain", [])
    for tag, extra, how, by in (("union", ["-how", "union"], "union", "pair"), ("clip", ["-by=map0"], "intersection", "map0"),
                                ("diff", ["-how=difference", "-by", "pair"], "difference", "pair")):
        r, out_bytes, ft, omp = run(tag, extra)
        assert ft == _face_text(R.face_rows(all_, how, by), ctx.scaling)
        want = R.output_map(all_, how, by)
        g = maps.read_cdb(omp)
        assert g.n_chains == len(want["left"]) and np.array_equal(g.row_index, want["row_index"])
        assert np.array_equal(g.chains[:, 3], want["left"]) and np.array_equal(g.chains[:, 4], want["right"])
        assert np.abs(g.points - ctx.scaling.unscale(want["xy"])).max() <= 1e-6
        assert out_bytes == plain[1] and _phases(r.stderr) == _phases(plain[0].stderr)  # -output: the host writer's file
    # the intersection by name is the intersection; the files without the flags are the calls' without _op
    r, out_bytes, ft, omp = run("named", ["-how", "intersection", "-by", "pair"])
    assert ft == plain[2] == F.text(F.rows(F.face_table(ctx.maps, xs, pip)), ctx.scaling)
    assert open(omp, "rb").read() == open(plain[3], "rb").read()
    bad = subprocess.run(base + ["-how", "xor", "-face_table", str(tmp_path / "x.txt")], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "bad value 'xor' for -how" in bad.stderr
