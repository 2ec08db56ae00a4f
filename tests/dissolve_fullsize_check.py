#!/usr/bin/env python3
"""rj_map_dissolve at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/eliminate_fullsize_check.py; profiles/dissolve_fullsize.txt holds its output):

  --map NAME [--scale S]   a stand-in of rayjoin_amd.synth (BlockGroup: 28.8 M edges)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges, the stand-ins of USCounty x BlockGroup)

Three runs per input: Join (identity classes, RJ_DISS_KEEP_EQUAL); a dissolve to about 50 classes, 1 + f % 50; the
Join of the map after one rj_map_eliminate round with RJ_ELIM_DROP at twice the median face area.  Each: one cold call,
then three warm ones with records, origin and chain_out -- the minimum of the three per stage (HIP events), the counts,
the scatter stage's bytes (16 np read + 16 n_points written) over its time against the achievable HBM rate of
profiles/r06_fetch_calibration.txt (6 225 GB/s), in the same process the minimum of three warm runs of the composition
there was before (rj_map_rings + rj_rings_map on the map with its labels already replaced by classes: the relabelling
itself is not counted, which favours the composition), and the device's output against the host twin on the whole map."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402
from test_dissolve import OK, records_of, twin_dissolve, twin_lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--no-composition", action="store_true")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("check+classes+keep", "ends+next", "walks", "class records", "totals+scatter", "all")
STREAM_GBS = 6225.0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def composition_ms(h, host, table, dissolve):
    """the minimum of three warm runs of face_rings + rings_map on the map relabelled by class, wall ms around both calls
    (each ends with its own sync)"""
    cl, cr = (host[2], host[3]) if table is None else (table[host[2]], table[host[3]])
    dev = [h.alloc(max(4, arr.nbytes)).from_host(np.ascontiguousarray(arr)) for arr in (host[0], host[1], cl.astype(np.int32), cr.astype(np.int32))]
    n_points, n_chains = len(host[0]), len(host[1]) - 1
    walls, counts = [], None
    for _ in range(4):
        t0 = time.perf_counter()
        rings = ops.face_rings(h, dev[0], n_points, dev[1], dev[2], dev[3], n_chains)
        t1 = time.perf_counter()
        cm = rings.Map(h, dissolve=dissolve)
        walls.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        counts = dict(cm.counts)
        cm.free()
        rings.free()
    for b in dev:
        b.free()
    best = min(walls[1:])
    return best[0], best[1], counts


def run(h, name, host, dev, table, flags):
    """host = (xy, row, left, right) numpy; dev = the same as device arrays; table: numpy int32 or None"""
    n_points, n_chains = len(host[0]), len(host[1]) - 1
    say("%s: %d chains, %d points, %d edges" % (name, n_chains, n_points, n_points - n_chains))
    tab = None if table is None else h.alloc(4 * len(table)).from_host(table)
    args = (dev[0], n_points, dev[1], dev[2], dev[3], n_chains, tab, 0 if table is None else len(table))
    try:
        c = h.map_dissolve(*args, (0, 0, 0), None, None, None, None, flags=flags)
    except _capi.DissolveOverflow as e:
        c = e.counts
    caps = (c["n_classes"], c["n_chains"], c["n_points"])
    bufs = [h.alloc(4 * max(1, caps[1])), h.alloc(4 * max(1, caps[1])), h.alloc(16 * max(1, caps[2])), h.alloc(4 * (caps[1] + 1)), h.alloc(4 * max(1, caps[1])),
            h.alloc(4 * max(1, n_chains)), h.alloc(24 * max(1, caps[0]))]
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        counts = h.map_dissolve(*args, caps, *bufs, flags=flags)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option("dissolve_last_us%d" % s) / 1000.0 for s in range(6)]
        if k:
            best = ms if best is None else [min(x, y) for x, y in zip(best, ms)]
    say("  %s" % counts)
    say("  first call %.3f ms wall; three warm calls %s ms wall" % (walls[0], ", ".join("%.3f" % w for w in walls[1:])))
    say("  the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, best)))
    moved = 16 * n_points + 16 * counts["n_points"]
    gbs = moved / (best[4] * 1e-3) / 1e9
    say("  the totals+scatter stage: %d bytes read and written in %.3f ms = %.0f GB/s = %.2f of the achievable %.0f GB/s" % (moved, best[4], gbs,
                                                                                                                            gbs / STREAM_GBS, STREAM_GBS))
    if not a.no_composition:
        both, rings_only, cc = composition_ms(h, host, table, dissolve=not flags)
        say("  the composition rj_map_rings + rj_rings_map on the same input: %.3f ms wall (rj_map_rings %.3f), the minimum of three warm runs; %d chains, "
            "%d conflicts -- rj_map_dissolve: %.3f ms wall, %.1f x" % (both, rings_only, cc["n_chains"], cc["n_conflicts"], min(walls[1:]), both / min(walls[1:])))
    if not a.no_twin:
        t0 = time.perf_counter()
        rc, want, wc = twin_dissolve(twin_lib(), host, table, flags, capacities=caps)
        assert rc == OK and wc == counts, (rc, wc, counts)
        n, npts = counts["n_chains"], counts["n_points"]
        assert np.array_equal(bufs[0].to_host(np.int32, n), want.left) and np.array_equal(bufs[1].to_host(np.int32, n), want.right)
        assert np.array_equal(bufs[2].to_host(np.int64, 2 * npts).reshape(-1, 2), want.xy) and np.array_equal(bufs[3].to_host(np.uint32, n + 1), want.row_index)
        assert np.array_equal(bufs[4].to_host(np.uint32, n), want.origin) and np.array_equal(bufs[5].to_host(np.uint32, n_chains), want.chain_out)
        assert records_of(bufs[6].to_host(_capi.DISS_CLASS_DTYPE, counts["n_classes"])) == want.classes
        say("  equal to the host twin on the whole map (%.1f s): every count, class, record, origin and point" % (time.perf_counter() - t0))
    for b in bufs + ([tab] if tab is not None else []):
        b.free()


def run_all(h, name, host, dev):
    top = int(max(host[2].max(), host[3].max()))
    f = np.arange(top + 1, dtype=np.int64)
    table = (1 + f % 50).astype(np.int32)
    table[0] = 0
    run(h, "Join of " + name, host, dev, None, _capi.RJ_DISS_KEEP_EQUAL)
    run(h, "Dissolve to 1 + f % 50 of " + name, host, dev, table, 0)
    n_points, n_chains = len(host[0]), len(host[1]) - 1
    first = ops.map_eliminate(h, dev[0], n_points, dev[1], dev[2], dev[3], n_chains, 0, drop=False, faces=True)
    rec = first.faces_to_host()
    first.free()
    areas = np.sort(np.array([(int(r["area2_hi"]) << 64) | int(r["area2_lo"]) for r in rec], dtype=object))
    tol = 2 * int(areas[len(areas) // 2])
    em = ops.map_eliminate(h, dev[0], n_points, dev[1], dev[2], dev[3], n_chains, tol, drop=True)
    hm = em.to_host()[0]
    ehost = (np.ascontiguousarray(hm.pts, np.int64), np.ascontiguousarray(hm.row_index, np.uint32), np.ascontiguousarray(hm.left, np.int32),
             np.ascontiguousarray(hm.right, np.int32))
    run(h, "Join of one eliminate round (tol = 2 x median area2, %d faces eliminated) of %s" % (em.counts["n_eliminated"], name), ehost,
        (em.xy, em.row_index, em.left, em.right), None, _capi.RJ_DISS_KEEP_EQUAL)
    em.free()


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
