#!/usr/bin/env python3
"""rj_window_query at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/within_fullsize_check.py; profiles/window_fullsize.txt holds its output).

Without --step it is a driver: one child process per base map (--bases, default USCounty and the ring map
WaterBodiesLike), each under its own `timeout`, and it stops at the first child that fails.

A step (--step --base NAME) loads the map, builds the index and takes four shapes of windows in ONE process: a 1024 x 1024
tiling of the extent, a 16 x 16 tiling, one window over everything, and 2^20 point windows on vertices.  Per shape, with
the containment shortcut on at the start level of the rule and at every level the tree has, and with the shortcut off at
the level of the rule: the counting call and the filling call (offsets, eids, flags) -- one cold call each, then the minimum
of three warm ones per stage (HIP events, "window_last_us0" .. 2) -- pairs per second and the share of sort + outputs.  Two
comparisons in the same process: the point windows against rj_within_query at max_dist 0 over the same points (the arrays
must be equal), and the window over everything against a device-to-device copy of ne 8-byte keys, the floor of a path that
streams the keys once.  Verified on the host: for a sample of windows per shape the twin's brute force over ALL edges
(tests/hosttwin/window_twin.cc) equals the device's lists with their flags; every list ascends; the counts agree."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", action="store_true", help="run one base map in this process")
ap.add_argument("--base", default="USCounty")
ap.add_argument("--bases", default="USCounty,WaterBodiesLike")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--sample", type=int, default=48)
ap.add_argument("--limit", type=int, default=540, help="seconds a step may take")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()

if not a.step:
    for base in a.bases.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", "--base", base, "--scale", str(a.scale), "--sample",
               str(a.sample)] + (["--out", a.out] if a.out else [])
        rc = subprocess.call(cmd)
        if rc:
            print("the step of %s ended with status %d: stopping" % (base, rc), flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_window as TW  # noqa: E402
from rayjoin_amd import maps, ops, synth  # noqa: E402

STAGES = ("traversal", "sort + outputs", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


twin = TW.twin_lib()
base = maps.Context([synth.standin(a.base, a.scale)]).load().maps[0]
dctx = ops.DeviceContext(maps.Context([]), 0)
dctx.ctx.set_map(0, base)
z = np.zeros(1, np.int64)
dctx.ctx.set_map(1, maps.ScaledMap(1, np.zeros((2, 2), np.int64), np.array([0, 2], np.uint32), z, z))
dctx.LoadToDevice()
dctx.BuildIndex(0)
h = dctx.handle
ne = base.n_edges
seg = base.segments()
top = [i for i in h.get_plan()["index"] if i["map"] == 0][0]["levels"]
x0, y0, x1, y1 = (int(v) for v in (base.pts[:, 0].min(), base.pts[:, 1].min(), base.pts[:, 0].max(), base.pts[:, 1].max()))
say("%s%s: %d edges (index: %d levels, %d leaf slots)" % (a.base, "" if a.scale == 1.0 else " at scale %g" % a.scale, ne, top, h.get_option("leaf_slots0")))


def tiling(k):
    xs, ys = np.linspace(x0, x1 + 1, k + 1).astype(np.int64), np.linspace(y0, y1 + 1, k + 1).astype(np.int64)
    gx, gy = np.meshgrid(np.arange(k), np.arange(k))
    gx, gy = gx.ravel(), gy.ravel()
    return np.ascontiguousarray(np.stack([xs[gx], ys[gy], xs[gx + 1] - 1, ys[gy + 1] - 1], 1))


rng = np.random.default_rng(23)
verts = np.ascontiguousarray(base.pts[rng.integers(0, base.n_points, 1 << 20)], np.int64)
margin = 1 << 17
SHAPES = [("a 1024 x 1024 tiling of the extent", tiling(1024)), ("a 16 x 16 tiling of the extent", tiling(16)),
          ("one window over everything", np.array([(x0 - margin, y0 - margin, x1 + margin, y1 + margin)], np.int64)),
          ("2^20 point windows on vertices", np.concatenate([verts, verts], 1))]


def best_of(call, option, n):
    """one cold call, three warm ones -> (the cold wall ms, the minimum per stage of the warm ones)"""
    best, cold = None, 0.0
    for k in range(4):
        t0 = time.perf_counter()
        call()
        if k == 0:
            cold = (time.perf_counter() - t0) * 1e3
        else:
            ms = [h.get_option(option % s) / 1000.0 for s in range(n)]
            best = ms if best is None else [min(p, q) for p, q in zip(best, ms)]
    return cold, best


def ascends(off, eid):
    lens = np.diff(off)
    first = np.zeros(max(1, len(eid)), bool)
    first[off[:-1][lens > 0]] = True
    return len(eid) < 2 or bool(((np.diff(eid.astype(np.int64)) > 0) | first[1:len(eid)]).all())


for what, win in SHAPES:
    nw = len(win)
    src = h.alloc(32 * nw).from_host(win)
    offsets = h.alloc(8 * (nw + 1))
    counts = h.window_query(0, src, nw, 0, offsets)
    n_pairs = counts["n_pairs"]
    say("  %s: %d windows, n_pairs %d, n_windows_hit %d, max_per_window %d" % (what, nw, n_pairs, counts["n_windows_hit"], counts["max_per_window"]))
    eid, flags = h.alloc(4 * max(1, n_pairs)), h.alloc(max(1, n_pairs))
    table = {}
    for contained, level in [(1, 0)] + [(1, lv) for lv in range(1, top + 1)] + [(0, 0)]:
        h.set_debug_option("window_contained", contained)
        h.set_debug_option("window_start_level", level)
        cold_c, t_count = best_of(lambda: h.window_query(0, src, nw, 0, offsets), "window_last_us%d", 3)
        cold_f, t_fill = best_of(lambda: h.window_query(0, src, nw, max(1, n_pairs), offsets, eid, flags), "window_last_us%d", 3)
        table[(contained, level)] = (t_count, t_fill)
        say("    shortcut %s, start level %s: counting call ms  %s  (first call %.3f wall) | filling call ms  %s  (first call %.3f wall); "
            "%.1f M pairs per second, sort + outputs %.0f %% of the filling call"
            % ("on" if contained else "OFF", level if level else "by rule", "  ".join("%s %.3f" % (s, v) for s, v in zip(STAGES, t_count)), cold_c,
               "  ".join("%s %.3f" % (s, v) for s, v in zip(STAGES, t_fill)), cold_f, n_pairs / max(t_fill[2], 1e-6) / 1e3, 100.0 * t_fill[1] / max(t_fill[2], 1e-6)))
    h.set_debug_option("window_contained", 1)
    h.set_debug_option("window_start_level", 0)
    levels = {lv: table[(1, lv)][1][2] for lv in range(1, top + 1)}
    best_level = min(levels, key=levels.get)
    say("    the filling call by start level: %s; the rule takes %.3f ms, the best level (%d) %.3f ms%s"
        % (", ".join("%d: %.3f ms" % kv for kv in sorted(levels.items())), table[(1, 0)][1][2], best_level, levels[best_level],
           "" if table[(1, 0)][1][2] <= 1.1 * levels[best_level] else ": THE RULE LOSES"))
    h.set_option("stats", 1)
    h.window_query(0, src, nw, max(1, n_pairs), offsets, eid, flags)
    s = h.last_stats_raw()
    h.set_option("stats", 0)
    say("    at the rule's level: %d nodes expanded, %d leaf blocks loaded, %d pairs tested exactly, %d handed out by containment, %d appended" % tuple(s[:5]))
    assert s[4] == n_pairs
    # the host's check
    t0 = time.perf_counter()
    off = offsets.to_host(np.uint64, nw + 1).astype(np.int64)
    e_host, f_host = eid.to_host(np.uint32, n_pairs), flags.to_host(np.uint8, n_pairs)
    lens = np.diff(off)
    assert off[0] == 0 and off[nw] == n_pairs and (lens >= 0).all() and int(lens.max()) == counts["max_per_window"] and int((lens > 0).sum()) == counts["n_windows_hit"]
    assert ascends(off, e_host), "a list does not ascend"
    pick = np.unique(np.concatenate([rng.choice(np.flatnonzero(lens > 0), min(a.sample // 2, int((lens > 0).sum())), replace=False),
                                     rng.choice(nw, min(a.sample // 2, nw), replace=False)]))
    rc, t_counts, t_off, t_eid, t_flags, _ = TW.call_twin(twin, seg, win[pick])
    assert rc == TW.OK
    t_off = t_off.astype(np.int64)
    for k, i in enumerate(pick):
        assert np.array_equal(e_host[off[i]:off[i + 1]], t_eid[t_off[k]:t_off[k + 1]]) and np.array_equal(f_host[off[i]:off[i + 1]], t_flags[t_off[k]:t_off[k + 1]]), int(i)
    say("    equal to the twin's brute force over all %d edges on a sample of %d windows, %d of them with a list; every list ascends (%.1f s)"
        % (ne, len(pick), int((lens[pick] > 0).sum()), time.perf_counter() - t0))
    if nw == 1:
        assert n_pairs == ne and np.array_equal(e_host, np.arange(ne, dtype=np.uint32)) and (f_host == 3).all()
        a_buf, b_buf = h.alloc(8 * ne), h.alloc(8 * ne)
        walls = []
        for _ in range(4):
            t0 = time.perf_counter()
            b_buf.from_device(a_buf, 8 * ne)
            walls.append((time.perf_counter() - t0) * 1e3)
        floor = min(walls[1:])
        say("    the floor of the streaming path, a device-to-device copy of %d 8-byte keys: %.3f ms wall (minimum of three warm copies); the counting call's "
            "traversal is %.1f x that, the filling call's %.1f x, the whole filling call %.1f x"
            % (ne, floor, table[(1, 0)][0][0] / floor, table[(1, 0)][1][0] / floor, table[(1, 0)][1][2] / floor))
        a_buf.free()
        b_buf.free()
    if what.endswith("on vertices"):
        pts = h.alloc(16 * nw).from_host(verts)
        w_off, w_eid = h.alloc(8 * (nw + 1)), h.alloc(4 * max(1, n_pairs))
        got = {}
        cold, t_within = best_of(lambda: got.update(h.within_query(0, 1, pts, 0, nw, 0, max(1, n_pairs), w_off, w_eid)), "within_last_us%d", 4)
        assert got["n_pairs"] == n_pairs and np.array_equal(w_off.to_host(np.uint64, nw + 1).astype(np.int64), off) and np.array_equal(w_eid.to_host(np.uint32, n_pairs), e_host)
        t_win = table[(1, 0)][1]
        say("    rj_within_query at max_dist 0 over the same points (offsets and eids, the arrays are equal): ms  ordering %.3f  traversal %.3f  sort + outputs %.3f  "
            "all %.3f (first call %.3f wall); rj_window_query all %.3f ms: %s"
            % (t_within[0], t_within[1], t_within[2], t_within[3], cold, t_win[2],
               "rj_window_query LOSES by %.2f x" % (t_win[2] / t_within[3]) if t_win[2] > t_within[3] else "rj_within_query LOSES by %.2f x" % (t_within[3] / t_win[2])))
        for b in (pts, w_off, w_eid):
            b.free()
    for b in (src, offsets, eid, flags):
        b.free()
dctx.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
