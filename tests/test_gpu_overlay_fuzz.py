"""Randomised pairs through the whole overlay on the device (the net tests/test_gpu_fuzz.py is for the LSI / PIP queries):
the generator of that module drawn smaller, and with probability 1/4 an integer pair of random chains on a tiny lattice
(coincident cuts, shared vertices; tests/overlay_hard_pairs.py's tie family with random chain count, length and span).
Per pair: the per-edge records and the vertex faces against the oracle, then the face table and the output map against
the plain-Python helper (tests/overlay_ops_ref.py) for (intersection, pair), (union, pair) and three more operations
drawn at random, both drop flags, through the LBVH or -mode=grid.  Where a drawn output map (dropped pieces left out) has
at least 16 chains it is installed as map 0 of a second overlay with a third lattice, whose records, vertex faces and
table must be the oracle pipeline's on the helper's map.  tests/overlay_fuzz_more.py runs more seeds by hand."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_hard_pairs as H  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
from test_gpu_fuzz import _maps  # noqa: E402
from test_gpu_overlay_hard import FIELDS, run_overlay  # noqa: E402
from test_gpu_overlay_map import counts_of, host_arrays  # noqa: E402
from test_gpu_overlay_ops import as_rows, raw_op_map, raw_op_rows  # noqa: E402
from test_overlay_map import assert_same_map  # noqa: E402
from test_overlay_ops import OPS  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE_CAP = 40000     # edges of a pair: the plain-Python walk stays at seconds
EXTRA_OPS = 3        # operations drawn per pair besides (intersection, pair) and (union, pair)
GSIZES = (64, 256, 1024)


def _draw_small(rng):
    """the five kinds of tests/test_gpu_fuzz.py's _draw with smaller counts (and fewer density bumps under the ring maps:
    tabulating 400 of them costs a second per map whatever its size)"""
    kind = rng.integers(0, 5)
    seed = int(rng.integers(1, 1 << 30))
    if kind == 0:
        n = int(rng.integers(50, 600))
        return synth.ring_map(n, n * int(rng.integers(4, 30)), seed, fill=float(rng.uniform(0.05, 0.6)), sigma=float(rng.uniform(0.3, 1.3)),
                              clusters=40)
    if kind == 1:
        return synth.gaussian_polygons(int(rng.integers(200, 2500)), seed, polysize=float(rng.uniform(0.002, 0.05)))
    if kind == 2:
        return synth.lattice_map(int(rng.integers(3, 20)), int(rng.integers(2, 20)), seed)
    if kind == 3:
        G, k = int(rng.integers(3, 7)), int(rng.integers(3, 12))
        return synth.nested_refinement(synth.lattice_map(G, k, seed), G, k, int(rng.integers(2, 5)), int(rng.integers(3, 9)), seed=seed + 1)
    n = int(rng.integers(1000, 4500))   # many tiny rings
    return synth.ring_map(n, n * 4, seed, fill=0.5, sigma=0.4, clusters=40)


def draw_pair(rng):
    """-> (ctx, kind): two scaled maps under one Scaling"""
    if rng.random() < 0.25:  # integer chains: steps of at most 3 units on a lattice of +-span
        ms = []
        for im in range(2):
            pts, row, left, right = synth.adversarial_chains(int(rng.integers(10, 120)), int(rng.integers(2, 12)), int(rng.integers(4, 30)),
                                                             int(rng.integers(1, 1 << 30)))
            ms.append(maps.ScaledMap(im, pts, row, left, right))
        ctx = maps.Context([None, None])
        ctx.scaling = maps.Scaling(synth.US_BBOX)
        ctx.maps = ms
        return ctx, "ties"
    gs = []
    while len(gs) < 2:  # tests/test_gpu_fuzz.py's generator (its check that the loader accepts the map), drawn smaller
        g = _maps(rng, _draw_small)
        if g.n_edges <= EDGE_CAP // 2:
            gs.append(g)
    return maps.Context(gs).load(), "float"


def oracle_pipeline(oracle, ctx, gsize, use_grid):
    """(pairs, records of both maps, vertex faces) of the oracle: pairs by brute force for the LBVH, by the grid for
    -mode=grid; vertex faces by brute force (what both device queries return)"""
    om = H.oracle_maps(oracle, ctx)
    pairs = oracle.lsi_grid(om[0], om[1], gsize)["eid"] if use_grid else oracle.lsi_brute(om[0], om[1])
    xs = [oracle.overlay_edge_xsects(om[0], om[1], im, pairs, gsize) for im in range(2)]
    pip = [om[1 - im].face_ids(oracle.pip_brute(om[1 - im], im, ctx.maps[im].pts)) for im in range(2)]
    return pairs, xs, pip


def assert_records(ov, xs, pip, what):
    assert ov.n_xsects == len(xs[0]), what
    for im in range(2):
        got = ov.get_xsects(im)
        for name in FIELDS:
            assert np.array_equal(got[name], xs[im][name]), what + (im, name)
        assert np.array_equal(ov.get_vertex_faces(im), pip[im]), what + (im, "vertex faces")


def check_pair(oracle, rng, what):
    ctx, kind = draw_pair(rng)
    use_grid = bool(rng.integers(0, 2))
    gsize = int(rng.choice(GSIZES))
    source = "grid-%d" % gsize if use_grid else "lbvh"
    what = what + (kind, ctx.maps[0].n_edges, ctx.maps[1].n_edges, source)
    pairs, xs, pip = oracle_pipeline(oracle, ctx, gsize, use_grid)
    all_ = R.all_pieces(ctx.maps, xs, pip)
    drawn = [OPS[0], OPS[3]] + [OPS[int(i)] for i in rng.choice([i for i in range(len(OPS)) if i not in (0, 3)], EXTRA_OPS, replace=False)]
    assert drawn[:2] == [("intersection", "pair"), ("union", "pair")]
    third_draw = (int(rng.integers(4, 10)), int(rng.integers(80, 140)), int(rng.integers(1, 1 << 30)))
    cascade = None
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = run_overlay(dctx, gsize if use_grid else None, len(pairs))
        assert_records(ov, xs, pip, what)
        for how, by in drawn:
            tag = what + (how, by)
            want_rows = R.face_rows(all_, how, by)
            if (how, by) == ("intersection", "pair"):  # the calls without _op (kept: a chain with one face on both sides)
                assert as_rows(ov.FaceTable()) == F.rows(F.face_table(ctx.maps, xs, pip)), tag + ("without _op",)
                assert raw_op_rows(ov, how, by, len(want_rows) + 8) == want_rows, tag
            else:
                assert as_rows(ov.FaceTable(how=how, by=by)) == want_rows, tag
            for drop in (False, True):
                want = R.output_map(all_, how, by, drop_degenerate=drop)
                if (how, by) == ("intersection", "pair"):
                    old = ov.OutputMap(drop_degenerate=drop)
                    assert_same_map(host_arrays(old), M.output_map(ctx.maps, xs, pip, drop_degenerate=drop))
                    old.free()
                    om = raw_op_map(ov, how, by, drop)
                else:
                    om = ov.OutputMap(drop_degenerate=drop, how=how, by=by)
                assert (om.n_chains, om.n_points, om.n_faces) == counts_of(want), tag + (drop,)
                assert_same_map(host_arrays(om), want)
                # (float pairs only: the pair's Scaling has to hold the third lattice too, and the integer pairs fill 2^-40 of theirs)
                if drop and cascade is None and kind == "float" and om.n_chains >= 16:
                    cascade = (how, by, want)
                    third = third_lattice(ctx, *third_draw)
                    second = second_context(ctx, None, third)
                    d2 = ops.DeviceContext(second).LoadToDevice()
                    try:
                        d2.InstallMap(0, om)
                        om.free()
                        check_cascade(oracle, ctx, d2, want, third, gsize, use_grid, tag + ("cascade",))
                    finally:
                        d2.close()
                else:
                    om.free()
    finally:
        dctx.close()
    return kind, source, cascade is not None


def third_lattice(ctx, G, k, seed):
    """a lattice over the middle 70 % of the pair's box: with its vertex jitter (0.3 of a cell, G >= 4) it stays inside
    the box, so the pair's Scaling holds it; k >= 80 keeps its edges below 1/256 of the scaled range"""
    x0, y0, x1, y1 = ctx.bb
    third = synth.lattice_map(G, k, seed, bbox=(x0 + 0.15 * (x1 - x0), y0 + 0.15 * (y1 - y0), x1 - 0.15 * (x1 - x0), y1 - 0.15 * (y1 - y0)))
    assert third.bb[0] >= x0 and third.bb[1] >= y0 and third.bb[2] <= x1 and third.bb[3] <= y1
    return third


def second_context(ctx, m0, third):
    c = maps.Context([None, None])
    c.scaling = ctx.scaling
    c.set_map(0, m0)
    c.set_map(1, maps.ScaledMap(1, ctx.scaling.scale(third.points), third.row_index, third.chains[:, 3], third.chains[:, 4]))
    return c


def check_cascade(oracle, ctx, d2, want, third, gsize, use_grid, tag):
    """the second overlay, output map x third lattice, against the oracle pipeline on the helper's output map"""
    ctx2 = second_context(ctx, M.as_scaled_map(want, 0), third)
    pairs2, xs2, pip2 = oracle_pipeline(oracle, ctx2, gsize, use_grid)
    ov2 = run_overlay(d2, gsize if use_grid else None, len(pairs2))
    assert_records(ov2, xs2, pip2, tag)
    assert as_rows(ov2.FaceTable()) == F.rows(F.face_table(ctx2.maps, xs2, pip2)), tag


SEEDS = [101, 102, 103, 104, 105, 106]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_pairs_through_the_overlay_equal_the_oracle_and_the_helper(oracle, seed):
    rng = np.random.default_rng(seed)
    for k in range(4):
        print(seed, k, check_pair(oracle, rng, (seed, k)))
