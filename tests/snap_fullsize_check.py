#!/usr/bin/env python3
"""rj_map_snap at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/node_fullsize_check.py; profiles/snap_fullsize.txt holds its output).  Every time is the "all" HIP-event time of a
call, the minimum of three warm calls (a first call goes before them).

  --map NAME               a stand-in of rayjoin_amd.synth (BlockGroup: 28.8 M edges)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges)
      the one comparison with a baseline: rj_map_snap against rj_map_node on the same map and the same records of
      rj_map_crossings.  Without a proper crossing the outputs must be equal, array for array; the times are written down.
  --pair BASE QUERY        the two stand-ins of the benchmark's pair concatenated into ONE chain map (their borders cross
                           each other: polygon soup), cut in rounds as ops.map_snap_rounds does, by hand so that every
                           call is timed: per round the check's counts and milliseconds and the cut's counts and
                           milliseconds; the rounds to clean, or what remained at --max-rounds.  Then ops.map_snap_rounds on
                           a window of the map (the --window-edges edges of the chains nearest to one of its crossings) against
                           tests/snap_ref.py's snap_rounds_ref, round for round.  Where rj_map_crossings refuses the map
                           (its pair budget), that is said and only the window runs."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import snap_ref as SR  # noqa: E402
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--pair", nargs=2)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--max-rounds", type=int, default=8)
ap.add_argument("--window-edges", type=int, default=2500)
ap.add_argument("--window-any", action="store_true", help="accept a window without a crossing")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("check", "candidates", "sort+kept", "per edge+scan", "scatters", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def crossings_of(h, d_xy, n_points, d_row, n_chains):
    """-> (records buffer or None, counts, the minimum "all" ms of three warm filling calls)"""
    try:
        c = h.map_crossings(d_xy, n_points, d_row, n_chains, 0, None)
    except _capi.CrossingsOverflow as e:
        c = e.counts
    rec = h.alloc(16 * max(1, c["n_found"]))
    ms = []
    for _ in range(4):
        c = h.map_crossings(d_xy, n_points, d_row, n_chains, max(1, c["n_found"]), rec)
        ms.append(h.get_option("cross_last_us5") / 1000.0)
    return rec, c, min(ms[1:])


def cut(h, call, option, overflow, d_xy, n_points, d_row, n_chains, rec, n_rec):
    """rj_map_node or rj_map_snap -> (out xy, out row, counts, the stage ms of the fastest of three warm calls)"""
    try:
        n_out = call(d_xy, n_points, d_row, n_chains, rec, n_rec, 0, 0, None, None)["n_points"]
    except overflow as e:
        n_out = e.counts["n_points"]
    o_xy, o_row = h.alloc(16 * max(1, n_out)), h.alloc(4 * (n_chains + 1))
    best = None
    for k in range(4):
        counts = call(d_xy, n_points, d_row, n_chains, rec, n_rec, 0, n_out, o_xy, o_row)
        ms = [h.get_option(option % s) / 1000.0 for s in range(6)]
        if k > 0 and (best is None or ms[5] < best[5]):
            best = ms
    return o_xy, o_row, counts, best


def baseline(h, name, d_xy, n_points, d_row, n_chains):
    say("%s: %d chains, %d points, %d edges" % (name, n_chains, n_points, n_points - n_chains))
    rec, c, cross_ms = crossings_of(h, d_xy, n_points, d_row, n_chains)
    say("  rj_map_crossings: %s; %.3f ms" % (c, cross_ms))
    n_xy, n_row, node, node_ms = cut(h, h.map_node, "node_last_us%d", _capi.NodeOverflow, d_xy, n_points, d_row, n_chains, rec, c["n_found"])
    s_xy, s_row, snap, snap_ms = cut(h, h.map_snap, "snap_last_us%d", _capi.SnapOverflow, d_xy, n_points, d_row, n_chains, rec, c["n_found"])
    say("  rj_map_node: %s" % node)
    say("    ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, node_ms)))
    say("  rj_map_snap: %s" % snap)
    say("    ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, snap_ms)))
    equal = {k: snap[k] for k in _capi.NODE_COUNTS} == node and np.array_equal(s_row.to_host(np.uint32, n_chains + 1), n_row.to_host(np.uint32, n_chains + 1)) \
        and np.array_equal(s_xy.to_host(np.int64, 2 * snap["n_points"]), n_xy.to_host(np.int64, 2 * node["n_points"]))
    say("  rj_map_snap / rj_map_node: %.3f; the outputs are %s" % (snap_ms[5] / node_ms[5], "EQUAL, array for array" if equal else "DIFFERENT"))
    assert c["n_proper"] > 0 or equal
    for b in (rec, n_xy, n_row, s_xy, s_row):
        b.free()


def rounds(h, d_xy, n_points, d_row, n_chains):
    cur = None
    for r in range(a.max_rounds + 1):
        rec, c, cross_ms = crossings_of(h, d_xy, n_points, d_row, n_chains)
        dirty = SR.dirty(c)
        say("  check %d: %s; %.3f ms" % (r, {k: c[k] for k in ("n_found", "n_proper", "n_touch", "n_overlap", "n_equal")}, cross_ms))
        if dirty == 0 or r == a.max_rounds:
            rec.free()
            say("  clean after %d cutting rounds" % r if dirty == 0 else "  NOT clean after %d cutting rounds: %d crossings of a cutting kind remain" % (r, dirty))
            break
        o_xy, o_row, snap, ms = cut(h, h.map_snap, "snap_last_us%d", _capi.SnapOverflow, d_xy, n_points, d_row, n_chains, rec, c["n_found"])
        say("  cut %d: %s" % (r + 1, snap))
        say("    ms  " + "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, ms)))
        rec.free()
        if cur is not None:
            for b in cur:
                b.free()
        cur, d_xy, d_row, n_points = (o_xy, o_row), o_xy, o_row, snap["n_points"]


def a_crossing(h, d_xy, n_points, d_row, n_chains, xy, row):
    """-> the first point of the first edge of the middle record of rj_map_crossings, or None where there is no record"""
    try:
        rec, c, _ = crossings_of(h, d_xy, n_points, d_row, n_chains)
    except _capi.RayJoinError:
        return None
    records = rec.to_host(_capi.CROSSING_DTYPE, c["n_found"])
    rec.free()
    if not len(records):
        return None
    e = int(records[len(records) // 2]["eid"][0])
    c = int(np.searchsorted(row[:-1].astype(np.int64) - np.arange(n_chains), e, side="right")) - 1
    return xy[e + c]


def window(h, xy, row, mid):
    """the chains whose boxes lie nearest to `mid` (a point where two edges cross, or the middle of the map), about
    --window-edges edges of them, through ops.map_snap_rounds and through the definition"""
    first, last = row[:-1].astype(np.int64), row[1:].astype(np.int64)
    lo, hi = np.minimum.reduceat(xy, first, axis=0), np.maximum.reduceat(xy, first, axis=0)
    away = np.maximum(np.maximum(lo - mid, mid - hi), 0).max(axis=1)  # from mid to the chain's box
    order = np.argsort(away, kind="stable")
    take = np.sort(order[:int(np.searchsorted(np.cumsum((last - first - 1)[order]), a.window_edges)) + 1])
    w_xy = np.concatenate([xy[first[c]:last[c]] for c in take]) - mid  # (moved to the origin: the same geometry)
    w_row = np.concatenate([[0], np.cumsum((last - first)[take])]).astype(np.uint32)
    want = SR.snap_rounds_ref(w_xy, w_row, a.max_rounds)
    bufs = [h.alloc(16 * len(w_xy)).from_host(np.ascontiguousarray(w_xy)), h.alloc(4 * len(w_row)).from_host(w_row)]
    nm = ops.map_snap_rounds(h, bufs[0], len(w_xy), bufs[1], len(w_row) - 1, max_rounds=a.max_rounds)
    got = nm.to_host()
    equal = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and nm.rounds == want[2] and nm.clean == want[3] and nm.remaining == want[4]
    say("  window of %d chains, %d edges round a crossing: %d cutting rounds, clean %s, per round (crossings of a cutting kind, cuts) %s; the device %s the definition" % (
        len(take), len(w_xy) - len(take), len(nm.rounds), nm.clean, [(SR.dirty(r["crossings"]), r["snap"]["n_cuts"]) for r in nm.rounds],
        "EQUALS" if equal else "DIFFERS FROM"))
    assert equal and (len(nm.rounds) > 0 or a.window_any)


if a.pair:
    ctx = maps.Context([synth.standin(a.pair[0], a.scale), synth.standin(a.pair[1], a.scale)]).load()
    m0, m1 = ctx.maps
    xy = np.ascontiguousarray(np.concatenate([m0.pts, m1.pts]), np.int64)
    row = np.concatenate([m0.row_index, np.asarray(m1.row_index[1:], np.int64) + len(m0.pts)]).astype(np.uint32)
    h = _capi.Handle(0)
    d_xy, d_row = h.alloc(16 * len(xy)).from_host(xy), h.alloc(4 * len(row)).from_host(row)
    say("%s + %s in one chain map: %d chains, %d points, %d edges" % (a.pair[0], a.pair[1], len(row) - 1, len(xy), len(xy) - len(row) + 1))
    try:
        rounds(h, d_xy, len(xy), d_row, len(row) - 1)
    except _capi.RayJoinError as e:
        if e.code != _capi.RJ_E_INVALID:
            raise
        say("  rj_map_crossings refuses the whole map: %s" % e)
    at = a_crossing(h, d_xy, len(xy), d_row, len(row) - 1, xy, row)
    window(h, xy, row, np.median(xy[row[:-1].astype(np.int64)], axis=0).astype(np.int64) if at is None else at)
elif a.map:
    m = maps.Context([synth.standin(a.map, a.scale)]).load().maps[0]
    xy, row = np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32)
    h = _capi.Handle(0)
    baseline(h, a.map, h.alloc(16 * len(xy)).from_host(xy), len(xy), h.alloc(4 * len(row)).from_host(row), len(row) - 1)
else:
    g0, k0, g1, k1 = a.overlay
    dctx = ops.DeviceContext(maps.Context([synth.lattice_map(g0, k0, 31), synth.lattice_map(g1, k1, 32)]).load()).LoadToDevice()
    ov = ops.MapOverlay(dctx, None).Init(max(0.2, 4096.0 / sum(dctx.get_map(im).n_edges for im in range(2))))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    om = ov.OutputMap(drop_degenerate=True, merge=True)
    baseline(ov.h, "output map of lattice_map(%d, %d) x lattice_map(%d, %d), merged" % (g0, k0, g1, k1), om.xy, om.n_points, om.row_index, om.n_chains)
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
