#!/usr/bin/env python3
"""rj_map_eliminate at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/simplify_fullsize_check.py; profiles/eliminate_fullsize.txt holds its output):

  --map NAME [--scale S]   a stand-in of rayjoin_amd.synth (BlockGroup: 28.8 M edges)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges, the stand-ins of USCounty x BlockGroup)

tol is --times (default 2) of the median face area, taken from the records of a call at tol 0.  One cold call, then
three warm ones with RJ_ELIM_DROP and records: the minimum of the three per stage (HIP events), the counts, the chain-sum
pass's bytes (16 np) over its time against the achievable HBM rate of profiles/r06_fetch_calibration.txt (6 225 GB/s),
and the device's output against the host twin on the whole map: every count, label, record and kept chain.  --sweep: the
chain-sum stage and the scatter stage once more at a range of grids of the two passes over the points (the debug option
"elim_point_blocks"), the same counts required of each."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402
from test_eliminate import OK, faces_of, twin_eliminate, twin_lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--times", type=float, default=2.0, help="tol as a multiple of the median face area")
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--sweep", action="store_true", help="also the chain-sum stage at a range of grids (the debug option elim_point_blocks)")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("check+chain sums", "faces", "pairs+choice", "pointers", "labels+scatter", "all")
STREAM_GBS = 6225.0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run_map(h, name, host, dev):
    """host = (xy, row, left, right) numpy; dev = the same as device arrays"""
    n_points, n_chains = len(host[0]), len(host[1]) - 1
    say("%s: %d chains, %d points, %d edges" % (name, n_chains, n_points, n_points - n_chains))
    args = (dev[0], n_points, dev[1], dev[2], dev[3], n_chains)
    first = ops.map_eliminate(h, *args, 0, drop=False, faces=True)
    rec = first.faces_to_host()
    first.free()
    areas = np.sort(np.array([(int(r["area2_hi"]) << 64) | int(r["area2_lo"]) for r in rec], dtype=object))
    median = int(areas[len(areas) // 2])
    tol = int(median * a.times)
    say("  %d faces, median area2 %d; tol = %g x median = %d" % (len(rec), median, a.times, tol))
    try:
        c = h.map_eliminate(*args, tol, (0, 0, 0), None, None, flags=_capi.RJ_ELIM_DROP)
    except _capi.EliminateOverflow as e:
        c = e.counts
    caps = (c["n_faces"], c["n_chains"], c["n_points"])
    bufs = [h.alloc(4 * max(1, caps[1])), h.alloc(4 * max(1, caps[1])), h.alloc(16 * max(1, caps[2])), h.alloc(4 * (caps[1] + 1)), h.alloc(4 * max(1, caps[1])),
            h.alloc(32 * max(1, caps[0]))]
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        counts = h.map_eliminate(*args, tol, caps, *bufs, flags=_capi.RJ_ELIM_DROP)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option("elim_last_us%d" % s) / 1000.0 for s in range(6)]
        if k:
            best = ms if best is None else [min(x, y) for x, y in zip(best, ms)]
    say("  %s" % counts)
    say("  first call %.3f ms wall; three warm calls %s ms wall" % (walls[0], ", ".join("%.3f" % w for w in walls[1:])))
    say("  the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, best)))
    gbs = 16.0 * n_points / (best[0] * 1e-3) / 1e9
    say("  the chain-sum pass: %d bytes of points in %.3f ms = %.0f GB/s = %.2f of the achievable %.0f GB/s" % (16 * n_points, best[0], gbs, gbs / STREAM_GBS,
                                                                                                               STREAM_GBS))
    if not a.no_twin:
        t0 = time.perf_counter()
        rc, want, wc = twin_eliminate(twin_lib(), host, tol, _capi.RJ_ELIM_DROP, capacities=caps)
        assert rc == OK and wc == counts, (rc, wc, counts)
        n, npts = counts["n_chains"], counts["n_points"]
        assert np.array_equal(bufs[0].to_host(np.int32, n), want.left) and np.array_equal(bufs[1].to_host(np.int32, n), want.right)
        assert np.array_equal(bufs[2].to_host(np.int64, 2 * npts).reshape(-1, 2), want.xy) and np.array_equal(bufs[3].to_host(np.uint32, n + 1), want.row_index)
        assert np.array_equal(bufs[4].to_host(np.uint32, n), want.origin)
        assert faces_of(bufs[5].to_host(_capi.ELIM_FACE_DTYPE, counts["n_faces"])) == want.faces
        say("  equal to the host twin on the whole map (%.1f s): every count, label, record and kept chain" % (time.perf_counter() - t0))
    if a.sweep:
        say("  the chain-sum stage (its two memsets, the check and the kernel) and the labels+scatter stage by the grid of the two point passes")
        say("  (rj_set_debug_option \"elim_point_blocks\"; 0: the default, by size), HIP events, the minimum of three warm calls, ms:")
        for blocks in (256, 512, 1024, 1536, 1792, 2048, 3072, 4096, 8192, 16384, 32768, 65536, 0):
            h.set_debug_option("elim_point_blocks", blocks)
            got = []
            for k in range(4):
                assert h.map_eliminate(*args, tol, caps, *bufs, flags=_capi.RJ_ELIM_DROP) == counts
                if k:
                    got.append((h.get_option("elim_last_us0") / 1000.0, h.get_option("elim_last_us4") / 1000.0))
            say("    %6d blocks: chain sums %.3f  labels+scatter %.3f" % (blocks, min(g[0] for g in got), min(g[1] for g in got)))
        h.set_debug_option("elim_point_blocks", 0)
    for b in bufs:
        b.free()


if a.map:
    h = _capi.Handle(0)
    m = maps.Context([synth.standin(a.map, a.scale)]).load().maps[0]
    host = (np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32), np.ascontiguousarray(m.left, np.int32),
            np.ascontiguousarray(m.right, np.int32))
    dev = [h.alloc(max(4, arr.nbytes)).from_host(arr) for arr in host]
    run_map(h, "%s%s" % (a.map, "" if a.scale == 1.0 else " at scale %g" % a.scale), host, dev)
else:
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
    hm = om.to_host()[0]
    host = (np.ascontiguousarray(hm.pts, np.int64), np.ascontiguousarray(hm.row_index, np.uint32), np.ascontiguousarray(hm.left, np.int32),
            np.ascontiguousarray(hm.right, np.int32))
    run_map(ov.h, "output map of lattice_map(%d, %d) x lattice_map(%d, %d), merged" % (g0, k0, g1, k1), host, (om.xy, om.row_index, om.left, om.right))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
