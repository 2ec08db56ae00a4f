#!/usr/bin/env python3
"""rj_map_simplify at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/node_fullsize_check.py; profiles/simplify_fullsize.txt holds its output):

  --map NAME [--scale S]   a stand-in of rayjoin_amd.synth (USCounty 7.1 M edges, BlockGroup 28.8 M: lattices;
                           WaterBodiesLike: 2.4 M isolated rings, the lake-shaped map)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges)
  --staircase N            the N-point staircase of tests/simplify_cases.py at 2^128 - 1: one point per round, the serial
                           worst case (no tolerances, no twin)

For a map: three tolerances at which roughly 10 %, 50 % and 90 % of the points that can go at all do go (the ends of
every chain and the pins of closed chains never go: 2^128 - 1 removes the rest), found by bisection with the host twin on
a sub-sample of whole chains.  Each call is timed once warm (the second of two equal calls): the HIP-event time of
every stage, the host's time of each of the first ten rounds against the points the round looked at, the later rounds
summed, the rounds, the host syncs, the crossings of the result (rj_map_crossings on it, timed too, and rj_map_node's time with its records where there are
any), and the device's output against the host twin on a sub-sample of whole chains (every chain is thinned on its own,
so the twin runs on the sample alone and is compared with those chains of the device's full output).  Beside them, for
scale, rj_map_crossings on the input map."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simplify_cases as SC  # noqa: E402
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402
from test_simplify import OK, twin_lib, twin_simplify  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--staircase", type=int, default=0)
ap.add_argument("--sample-points", type=int, default=200000, help="points of the chains that the twin thins too")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("check", "links+pins", "round 1", "later rounds", "scan+scatter", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def tolerances(twin, sub):
    """-> [(share, tol)]: the tolerances at which the twin removes about 10 %, 50 %, 90 % of what 2^128 - 1 removes of the sample"""
    def removed(tol):
        rc, _, _, _, c = twin_simplify(twin, sub, tol, capacity=0)
        return c["n_removed"]
    most, out = removed(SC.HUGE), []
    for share in (0.1, 0.5, 0.9):
        lo, hi = 0.0, 96.0  # log2 of the tolerance: a weight is below 2^95
        for _ in range(14):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if removed(int(2.0 ** mid)) < share * most else (lo, mid)
        out.append((share, int(2.0 ** hi)))
    return out


def timed_simplify(h, d_xy, n_points, d_row, n_chains, tol, bufs):
    for _ in range(2):
        t0 = time.perf_counter()
        counts = h.map_simplify(d_xy, n_points, d_row, n_chains, tol, n_points, *bufs)
        wall = (time.perf_counter() - t0) * 1e3
    return counts, wall


def report(h, counts, wall, n_points):
    ms = [h.get_option("simplify_last_us%d" % k) / 1000.0 for k in range(6)]
    say("    %s" % counts)
    say("    ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, ms)) + "  | wall %.3f, host syncs %d" % (wall, h.get_option("simplify_last_syncs")))
    rounds = min(10, h.get_option("simplify_last_syncs") - 1)
    say("    rounds  " + "  ".join("%d: %d pts %.3f ms" % (k + 1, h.get_option("simplify_round_list%d" % k), h.get_option("simplify_round_us%d" % k) / 1000.0)
                                 for k in range(rounds)))
    late = h.get_option("simplify_late_rounds")
    if late:
        say("    rounds 11..%d: %d pts in all (%.1f a round, %.5f of np), %.3f ms in all, %.4f ms a round" % (
            10 + late, h.get_option("simplify_late_list"), h.get_option("simplify_late_list") / late, h.get_option("simplify_late_list") / late / n_points,
            h.get_option("simplify_late_us") / 1000.0, h.get_option("simplify_late_us") / 1000.0 / late))
    say("    work lists behind round 1: %d pts in all = %.3f passes over np, the longest %d" % (
        h.get_option("simplify_last_list_sum"), h.get_option("simplify_last_list_sum") / n_points, h.get_option("simplify_last_list_max")))
    return ms


def crossings_of(h, d_xy, n_points, d_row, n_chains):
    """-> (counts, ms of the whole call); a map that rj_map_crossings refuses (its pair budget) has n_found -1"""
    for _ in range(2):
        try:
            c = h.map_crossings(d_xy, n_points, d_row, n_chains, 0, None)
        except _capi.CrossingsOverflow as e:
            c = e.counts
        except _capi.RayJoinError as e:
            say("    rj_map_crossings refuses: %s" % e)
            return dict.fromkeys(_capi.CROSSINGS_COUNTS, -1), float("nan")
    return c, h.get_option("cross_last_us5") / 1000.0


def node_ms_of(h, d_xy, n_points, d_row, n_chains, found):
    """rj_map_node with the map's records, for scale (sizing calls: nothing is written)"""
    rec = h.alloc(16 * max(1, found))
    h.map_crossings(d_xy, n_points, d_row, n_chains, found, rec)
    for _ in range(2):
        try:
            h.map_node(d_xy, n_points, d_row, n_chains, rec, found, 0, 0, None, None)
        except _capi.NodeOverflow:
            pass
    rec.free()
    return h.get_option("node_last_us5") / 1000.0


def run_map(h, name, xy, row, d_xy=None, d_row=None):
    n_points, n_chains = len(xy), len(row) - 1
    say("%s: %d chains, %d points, %d edges" % (name, n_chains, n_points, n_points - n_chains))
    if d_xy is None:
        d_xy, d_row = h.alloc(16 * n_points).from_host(xy), h.alloc(4 * (n_chains + 1)).from_host(row)
    before, cross_ms = crossings_of(h, d_xy, n_points, d_row, n_chains)
    say("  rj_map_crossings on the input: n_found %d, %.3f ms; rj_map_node with its records (sizing call): %.3f ms" % (
        before["n_found"], cross_ms, node_ms_of(h, d_xy, n_points, d_row, n_chains, before["n_found"])))
    step = max(1, n_chains // max(1, int(n_chains * a.sample_points / n_points)))
    sample = np.arange(0, n_chains, step)
    sub_row = np.concatenate([[0], np.cumsum(row[sample + 1].astype(np.int64) - row[sample])]).astype(np.uint32)
    sub_xy = np.concatenate([xy[row[c]:row[c + 1]] for c in sample])
    twin = twin_lib()
    bufs = [h.alloc(16 * n_points), h.alloc(4 * (n_chains + 1)), h.alloc(4 * n_points)]
    for share, tol in tolerances(twin, (sub_xy, sub_row)):
        counts, wall = timed_simplify(h, d_xy, n_points, d_row, n_chains, tol, bufs)
        say("  tol %d (aimed at %d %% of the points that can go): %.1f %% of all points go" % (tol, round(100 * share), 100.0 * counts["n_removed"] / n_points))
        ms = report(h, counts, wall, n_points)
        after, after_ms = crossings_of(h, bufs[0], counts["n_points"], bufs[1], n_chains)
        say("    crossings of the result: %s, %.3f ms; the call / rj_map_crossings on the input: %.2f" % (
            {k: after[k] for k in ("n_found", "n_proper", "n_touch", "n_overlap", "n_equal")}, after_ms, ms[5] / cross_ms))
        out_row = bufs[1].to_host(np.uint32, n_chains + 1).astype(np.int64)
        out_xy = bufs[0].to_host(np.int64, 2 * counts["n_points"]).reshape(-1, 2)
        origin = bufs[2].to_host(np.uint32, counts["n_points"])
        rc, t_xy, t_row, t_origin, _ = twin_simplify(twin, (sub_xy, sub_row), tol, capacity=len(sub_xy))
        assert rc == OK
        for k, c in enumerate(sample):
            got, want = slice(out_row[c], out_row[c + 1]), slice(int(t_row[k]), int(t_row[k + 1]))
            assert np.array_equal(out_xy[got], t_xy[want]) and np.array_equal(origin[got] - row[c], t_origin[want] - sub_row[k]), (name, tol, c)
        say("    equal to the host twin on %d sampled chains (%d points in, %d out)" % (len(sample), len(sub_xy), len(t_xy)))
    for b in bufs:
        b.free()


h = _capi.Handle(0)
if a.staircase:
    xy, row = SC.chain_arrays(SC.staircase(a.staircase))
    d_xy, d_row = h.alloc(16 * len(xy)).from_host(xy), h.alloc(8).from_host(row)
    bufs = [h.alloc(16 * len(xy)), h.alloc(8), None]
    say("staircase of %d points at 2^128 - 1 (one point per round: serial by definition)" % a.staircase)
    t0 = time.perf_counter()
    counts = h.map_simplify(d_xy, len(xy), d_row, 1, SC.HUGE, len(xy), *bufs)
    wall = (time.perf_counter() - t0) * 1e3
    assert counts["n_points"] == 2 and counts["n_rounds"] == a.staircase - 2 and counts["n_max_round"] == 1, counts
    report(h, counts, wall, len(xy))
    say("    %.4f ms a round" % (wall / counts["n_rounds"]))
elif a.map:
    t0 = time.perf_counter()
    m = maps.Context([synth.standin(a.map, a.scale)]).load().maps[0]
    say("(generated in %.1f s)" % (time.perf_counter() - t0))
    run_map(h, "%s%s" % (a.map, "" if a.scale == 1.0 else " at scale %g" % a.scale), np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32))
else:
    h.close()
    g0, k0, g1, k1 = a.overlay
    dctx = ops.DeviceContext(maps.Context([synth.lattice_map(g0, k0, 31), synth.lattice_map(g1, k1, 32)]).load()).LoadToDevice()
    edges = [dctx.get_map(im).n_edges for im in range(2)]
    ov = ops.MapOverlay(dctx, None).Init(max(0.2, 4096.0 / sum(edges)))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    om = ov.OutputMap(drop_degenerate=True, merge=True)
    host = om.to_host()[0]
    h = ov.h
    run_map(h, "output map of lattice_map(%d, %d) x lattice_map(%d, %d), merged" % (g0, k0, g1, k1), np.ascontiguousarray(host.pts, np.int64),
            np.ascontiguousarray(host.row_index, np.uint32), om.xy, om.row_index)
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
