#!/usr/bin/env python3
"""rj_map_neighbours at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/dissolve_fullsize_check.py; profiles/neighbours_fullsize.txt holds its output):

  --map NAME [--scale S]   a stand-in of rayjoin_amd.synth (BlockGroup: 28.8 M edges)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges, the stand-ins of USCounty x BlockGroup)

Two runs per input, rook only and with RJ_NB_VERTEX.  Each: one cold call, then three warm ones with records -- the
minimum of the three per stage (HIP events), the counts, the point pass's bytes (16 np read) over its time against the
achievable HBM rate of profiles/r06_fetch_calibration.txt (6 225 GB/s), and the device's output against the host twin on
the whole map.  The yardstick, in the same process on the same input: rj_map_eliminate with tol 0 and without
RJ_ELIM_DROP, which makes the same chain sums, face sort and pair sort -- the minimum of three warm calls per stage."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402
from test_neighbours import ENTRY_DTYPE, FACE_DTYPE, OK, twin_lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("check+chain sums", "faces", "edge pairs", "nodes", "table", "all")
ELIM_STAGES = ("check+chain sums", "faces", "pairs+choice", "pointers", "labels", "all")
STREAM_GBS = 6225.0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def eliminate_yardstick(h, dev, n_points, n_chains):
    """rj_map_eliminate, tol 0, no RJ_ELIM_DROP, with records: the minimum of three warm calls per stage"""
    try:
        c = h.map_eliminate(dev[0], n_points, dev[1], dev[2], dev[3], n_chains, 0, (0, 0, 0), None, None)
    except _capi.EliminateOverflow as e:
        c = e.counts
    bufs = [h.alloc(4 * max(1, n_chains)), h.alloc(4 * max(1, n_chains)), h.alloc(32 * max(1, c["n_faces"]))]
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        h.map_eliminate(dev[0], n_points, dev[1], dev[2], dev[3], n_chains, 0, (c["n_faces"], n_chains, 0), bufs[0], bufs[1], faces_dev=bufs[2])
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option("elim_last_us%d" % s) / 1000.0 for s in range(6)]
        if k:
            best = ms if best is None else [min(x, y) for x, y in zip(best, ms)]
    for b in bufs:
        b.free()
    say("  the yardstick rj_map_eliminate (tol 0, no drop, records) on the same input: three warm calls %s ms wall" % ", ".join("%.3f" % w for w in walls[1:]))
    say("  the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(ELIM_STAGES, best)))
    return best


def run(h, name, host, dev, flags, yard):
    n_points, n_chains = len(host[0]), len(host[1]) - 1
    say("%s, %s: %d chains, %d points, %d edges" % (name, "RJ_NB_VERTEX" if flags else "rook only", n_chains, n_points, n_points - n_chains))
    args = (dev[0], n_points, dev[1], dev[2], dev[3], n_chains)
    try:
        c = h.map_neighbours(*args, (0, 0), flags=flags)
    except _capi.NeighboursOverflow as e:
        c = e.counts
    caps = (c["n_faces"], c["n_entries"])
    bufs = [h.alloc(64 * max(1, caps[0])), h.alloc(8 * (caps[0] + 1)), h.alloc(32 * max(1, caps[1]))]
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        counts = h.map_neighbours(*args, caps, *bufs, flags=flags)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option("neighbours_last_us%d" % s) / 1000.0 for s in range(6)]
        if k:
            best = ms if best is None else [min(x, y) for x, y in zip(best, ms)]
    say("  %s" % counts)
    say("  first call %.3f ms wall; three warm calls %s ms wall" % (walls[0], ", ".join("%.3f" % w for w in walls[1:])))
    say("  the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, best)))
    gbs = 16 * n_points / (best[0] * 1e-3) / 1e9
    say("  the point pass: %d bytes read in %.3f ms = %.0f GB/s = %.2f of the achievable %.0f GB/s" % (16 * n_points, best[0], gbs, gbs / STREAM_GBS, STREAM_GBS))
    say("  against the yardstick: all %.3f ms to rj_map_eliminate's %.3f ms (%.2f x); the point pass %.3f to %.3f ms" % (best[5], yard[5], best[5] / yard[5],
                                                                                                                      best[0], yard[0]))
    if not a.no_twin:
        t0 = time.perf_counter()
        nf, ne = caps
        faces, offsets, entries, wc = np.zeros(nf, FACE_DTYPE), np.zeros(nf + 1, np.uint64), np.zeros(ne, ENTRY_DTYPE), np.zeros(len(_capi.NEIGHBOURS_COUNTS), np.uint64)
        rc = twin_lib().neighbours_twin(host[0].ctypes.data, n_points, host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, n_chains, flags, nf, ne,
                                        faces.ctypes.data, offsets.ctypes.data, entries.ctypes.data, wc.ctypes.data)
        assert rc == OK and dict(zip(_capi.NEIGHBOURS_COUNTS, (int(v) for v in wc))) == counts, (rc, wc, counts)
        assert np.array_equal(bufs[0].to_host(np.uint8, 64 * nf), faces.view(np.uint8))  # (the records have no padding: byte for byte)
        assert np.array_equal(bufs[1].to_host(np.uint64, nf + 1), offsets)
        assert np.array_equal(bufs[2].to_host(np.uint8, 32 * ne), entries.view(np.uint8))
        say("  equal to the host twin on the whole map (%.1f s): every count, record, offset and entry" % (time.perf_counter() - t0))
    for b in bufs:
        b.free()


def run_all(h, name, host, dev):
    say(name)
    yard = eliminate_yardstick(h, dev, len(host[0]), len(host[1]) - 1)
    run(h, name, host, dev, 0, yard)
    run(h, name, host, dev, _capi.RJ_NB_VERTEX, yard)


if a.map:
    h = _capi.Handle(0)
    m = maps.Context([synth.standin(a.map, a.scale)]).load().maps[0]
    host = (np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32), np.ascontiguousarray(m.left, np.int32),
            np.ascontiguousarray(m.right, np.int32))
    dev = [h.alloc(max(4, arr.nbytes)).from_host(arr) for arr in host]
    run_all(h, "%s%s" % (a.map, "" if a.scale == 1.0 else " at scale %g" % a.scale), host, dev)
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
    run_all(ov.h, "the output map of lattice_map(%d, %d) x lattice_map(%d, %d), merged" % (g0, k0, g1, k1), host, (om.xy, om.row_index, om.left, om.right))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
