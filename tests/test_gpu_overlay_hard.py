"""The overlay on the device on the hard input families (tests/overlay_hard_pairs.py): first the per-edge records and
the vertex faces against the oracle, field by field -- the check that pins the order of cuts that coincide along an edge
(k_xsect_order_runs against the oracle's ovl_cmp) and the mid-point faces of two equal cut points -- then the face table
and the output map of all 5 x 3 operations against the plain-Python helper (tests/overlay_ops_ref.py), bit for bit,
through the LBVH and the -mode=grid record sources.  The CPU side is tests/test_overlay_hard.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_hard_pairs as H  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
from test_gpu_overlay_map import counts_of, host_arrays  # noqa: E402
from test_gpu_overlay_ops import as_rows, raw_op_map, raw_op_rows  # noqa: E402
from test_overlay_map import assert_same_map  # noqa: E402
from test_overlay_ops import OPS, _invariants, code  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("eid", "x_num", "y_num", "x_den", "y_den", "mid_point_polygon_id")


def run_overlay(dctx, grid_size, n_expected):
    """test_gpu_overlay_map.run_overlay with a queue that holds n_expected intersections (the tie families have more
    intersections than edges)"""
    edges = sum(dctx.get_map(im).n_edges for im in range(2))
    ov = ops.MapOverlay(dctx, grid_size).Init(max(1.0, (n_expected + 64) / edges))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    return ov


def assert_same_records(ov, oracle, ctx, pairs, gsize, what):
    """the device's records of both maps and its vertex faces against the oracle's, field by field"""
    om = H.oracle_maps(oracle, ctx)
    assert ov.n_xsects == len(pairs), what
    for im in range(2):
        want = oracle.overlay_edge_xsects(om[0], om[1], im, pairs, gsize)
        got = ov.get_xsects(im)
        for name in FIELDS:
            same = got[name] == want[name]
            assert same.all(), what + (im, name, "first at record %d" % int(np.flatnonzero(~same.reshape(len(got), -1).all(axis=1))[0]))
        want_faces = om[1 - im].face_ids(oracle.pip_brute(om[1 - im], im, ctx.maps[im].pts))
        assert np.array_equal(ov.get_vertex_faces(im), want_faces), what + (im, "vertex faces")


@pytest.mark.parametrize("name", H.NAMES)
def test_device_records_tables_and_maps_equal_the_oracle_and_the_helper(oracle, name):
    ctx, gsize = H.family(name)
    xs, pip, brute = H.preconditions(oracle, ctx, gsize)  # (grid pairs == brute pairs, so xs serves both sources)
    all_ = R.all_pieces(ctx.maps, xs, pip)
    want_rows = {op: R.face_rows(all_, *op) for op in OPS}
    want_maps = {(op, drop): R.output_map(all_, *op, drop_degenerate=drop) for op in OPS for drop in (False, True)}
    # ops routes (intersection, pair) to the calls without _op: the helpers that existed before the operations.  The same
    # bits unless a chain has one face on both sides (the tie families; rj_overlay_ops.h says which pieces differ and how)
    old = ("intersection", "pair")
    op_rows = want_rows[old]
    want_rows[old] = F.rows(F.face_table(ctx.maps, xs, pip))
    H.assert_rows_without_op(ctx, want_rows[old], op_rows)
    op_maps = {drop: want_maps[old, drop] for drop in (False, True)}
    for drop in (False, True):
        want_maps[old, drop] = M.output_map(ctx.maps, xs, pip, drop_degenerate=drop)
        if not H.same_face_chains(ctx):
            assert_same_map(op_maps[drop], want_maps[old, drop])
    for grid_size in (None, gsize):
        source = "grid" if grid_size else "lbvh"
        dctx = ops.DeviceContext(ctx).LoadToDevice()
        try:
            ov = run_overlay(dctx, grid_size, len(brute))
            assert_same_records(ov, oracle, ctx, brute, gsize, (name, source))
            tables = {}
            for how, by in OPS:
                tables[how, by] = as_rows(ov.FaceTable(how=how, by=by))
                assert tables[how, by] == want_rows[how, by], (name, source, how, by)
                for drop in (False, True):
                    want = want_maps[(how, by), drop]
                    om = ov.OutputMap(drop_degenerate=drop, how=how, by=by)
                    assert (om.n_chains, om.n_points, om.n_faces) == counts_of(want), (name, source, how, by, drop)
                    got = host_arrays(om)
                    assert_same_map(got, want)
                    om.free()
                # face_pairs row k - 1 is table row k
                assert [r[:2] for r in tables[how, by]] == [tuple(p) for p in got["face_pairs"].tolist()], (name, source, how, by)
            # (intersection, pair) through the _op calls themselves
            tables[old] = raw_op_rows(ov, *old, len(op_rows) + 8)
            assert tables[old] == op_rows, (name, source)
            for drop in (False, True):
                new = raw_op_map(ov, *old, drop)
                assert (new.n_chains, new.n_points, new.n_faces) == counts_of(op_maps[drop]), (name, source, drop)
                assert_same_map(host_arrays(new), op_maps[drop])
                new.free()
            _invariants(ctx, all_, lambda how, by: tables[how, by])
        finally:
            dctx.close()


def test_each_capacity_one_short_overflows_with_the_true_counts_on_the_ties(oracle):
    """the input with the most dropped pieces: the staged and the final counts differ most"""
    ctx, gsize = H.family("ties-0")
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx, None, 851)
        assert ov.n_xsects == 851
        for how, by in (("union", "pair"), ("difference", "pair"), ("intersection", "map0"), ("intersection", "pair")):
            for drop in (False, True):
                full = raw_op_map(ov, how, by, drop)
                true = (full.n_chains, full.n_points, full.n_faces)
                want = host_arrays(full)
                args = (ov.xsects[0], ov.xsects[1], ov.n_xsects, ov.faces[0], ov.faces[1], int(drop))
                with pytest.raises(_capi.MapOverflow) as e:  # the sizing call
                    ov.h.overlay_map(*args, (0, 0, 0), None, None, None, None, None, None, op=code(how, by))
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
                        ov.h.overlay_map(*args, (cc, pc, fc), *[b for b, _ in bufs], op=code(how, by))
                    assert e.value.counts == true, (how, by, drop, short)
                    for b, nbytes in bufs:
                        assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary), (how, by, drop, short)
                        b.free()
                if (how, by) != ("intersection", "pair"):  # (ops routes that one to the call without _op)
                    exact = ov.OutputMap(drop_degenerate=drop, capacities=true, how=how, by=by)
                    assert_same_map(host_arrays(exact), want)
                    exact.free()
                full.free()
            rows = raw_op_rows(ov, how, by, 4096)
            with pytest.raises(_capi.QueueOverflow) as e:
                raw_op_rows(ov, how, by, len(rows) - 1)
            assert e.value.n_found == len(rows)
            assert raw_op_rows(ov, how, by, len(rows)) == rows
    finally:
        dctx.close()
