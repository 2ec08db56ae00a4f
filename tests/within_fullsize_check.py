#!/usr/bin/env python3
"""rj_within_query at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/nearest_fullsize_check.py; profiles/within_fullsize.txt holds its output).

Without --step it is a driver: one child process per base map (--bases, default USCounty and the ring map
WaterBodiesLike, each against the vertices of --query, default BlockGroup: 29.7 M points), each under its own `timeout`,
and it stops at the first child that fails.

A step (--step --base NAME) loads the pair, builds the index and, for max_dist = one and four mean edge lengths of the base
map, takes in ONE process: rj_nearest_query with that max_dist (the yardstick), the counting call of rj_within_query and
the filling call at the exact capacity with records and distances -- one cold call each, then the minimum of three warm ones
per stage (HIP events) -- and one instrumented filling call for the visit counts.  It reports n_pairs and the counts, the
stage times, and the ratio to the yardstick per stage.  Verified on the host: for a sample of points, half of them with a
list and half of them any, the edges within max_dist (1 + 1e-9) in float64 over ALL edges in numpy, the exact decision
among them in Python integers (tests/within_ref.py), equal to the device's list with its records; and rj_nearest_query's
eid a miss exactly where the list is empty, else a member of the list, for every point."""
import argparse
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", action="store_true", help="run one base map in this process")
ap.add_argument("--base", default="USCounty")
ap.add_argument("--bases", default="USCounty,WaterBodiesLike")
ap.add_argument("--query", default="BlockGroup")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--sample", type=int, default=300)
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--limit", type=int, default=540, help="seconds a step may take")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()

if not a.step:
    for base in a.bases.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", "--base", base, "--query", a.query, "--scale", str(a.scale),
               "--sample", str(a.sample), "--threads", str(a.threads)] + (["--out", a.out] if a.out else [])
        rc = subprocess.call(cmd)
        if rc:
            print("the step of %s ended with status %d: stopping" % (base, rc), flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import within_ref as WR  # noqa: E402
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

W_STAGES = ("ordering", "traversal", "sort + outputs", "all")
N_STAGES = ("ordering", "traversal", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def exact(rec):
    return [(int(r["eid"]), int(r["where"]), (int(r["num_hi"]) << 64) + int(r["num_lo"]), (int(r["den_hi"]) << 64) + int(r["den_lo"])) for r in rec]


ctx = maps.Context([synth.standin(a.base, a.scale), synth.standin(a.query, a.scale)]).load()
dctx = ops.DeviceContext(ctx).LoadToDevice()
h = dctx.handle
dctx.BuildIndex(0)
base = ctx.maps[0]
pts = np.ascontiguousarray(ctx.maps[1].pts, np.int64).reshape(-1, 2)
n, ne = len(pts), base.n_edges
seg = base.segments()
sf = seg.astype(np.float64)
mean_len = int(np.hypot(sf[:, 2] - sf[:, 0], sf[:, 3] - sf[:, 1]).mean())
say("%s x %s%s: %d points against %d edges (index: %d levels); the mean edge length = %d"
    % (a.base, a.query, "" if a.scale == 1.0 else " at scale %g" % a.scale, n, ne, [i for i in h.get_plan()["index"] if i["map"] == 0][0]["levels"], mean_len))
near_eid = h.alloc(4 * n)
offsets = h.alloc(8 * (n + 1))
ax, ay = sf[:, 0].copy(), sf[:, 1].copy()
dx, dy = sf[:, 2] - ax, sf[:, 3] - ay
ll = np.maximum(dx * dx + dy * dy, 1.0)


def best_of(call, names, option):
    """one cold call, three warm ones -> (the cold wall ms, the warm wall ms, the minimum per stage)"""
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option(option % s) / 1000.0 for s in range(len(names))]
        if k:
            best = ms if best is None else [min(p, q) for p, q in zip(best, ms)]
    return walls[0], walls[1:], best


def report(what, cold, warm, names, best):
    say("    %s: first call %.3f ms wall; three warm calls %s ms wall" % (what, cold, ", ".join("%.3f" % w for w in warm)))
    say("      the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (t, v) for t, v in zip(names, best)))


def near_edges(p, max_dist):
    """the edges within max_dist (1 + 1e-9) of p in float64, over all edges"""
    ex, ey = p[0] - ax, p[1] - ay
    t = np.clip((ex * dx + ey * dy) / ll, 0.0, 1.0)
    ex -= t * dx
    ey -= t * dy
    return np.nonzero(ex * ex + ey * ey <= (max_dist * (1 + 1e-9)) ** 2 + 1.0)[0]


for factor in (1, 4):
    md = factor * mean_len
    say("  max_dist = %d mean edge length%s = %d" % (factor, "" if factor == 1 else "s", md))
    cold, warm, t_near = best_of(lambda: h.nearest_query(0, 1, None, 0, n, near_eid, None, None, max_dist=md), N_STAGES, "nearest_last_us%d")
    report("rj_nearest_query, the yardstick (eids only)", cold, warm, N_STAGES, t_near)
    counts = {}
    cold, warm, t_count = best_of(lambda: counts.update(h.within_query(0, 1, None, 0, n, md, 0, offsets)), W_STAGES, "within_last_us%d")
    report("rj_within_query, the counting call (offsets and counts)", cold, warm, W_STAGES, t_count)
    n_pairs = counts["n_pairs"]
    say("      n_pairs %d, n_points_hit %d, max_per_point %d: %.3f pairs per point, %.2f per point with a list"
        % (n_pairs, counts["n_points_hit"], counts["max_per_point"], n_pairs / n, n_pairs / max(1, counts["n_points_hit"])))
    eid, rec, dist = h.alloc(4 * max(1, n_pairs)), h.alloc(40 * max(1, n_pairs)), h.alloc(8 * max(1, n_pairs))
    cold, warm, t_fill = best_of(lambda: h.within_query(0, 1, None, 0, n, md, max(1, n_pairs), offsets, eid, rec, dist), W_STAGES, "within_last_us%d")
    report("rj_within_query, the filling call (offsets, eids, records, distances)", cold, warm, W_STAGES, t_fill)
    cold, warm, t_eids = best_of(lambda: h.within_query(0, 1, None, 0, n, md, max(1, n_pairs), offsets, eid), W_STAGES, "within_last_us%d")
    report("rj_within_query, the filling call (offsets and eids only)", cold, warm, W_STAGES, t_eids)
    h.set_option("stats", 1)
    h.within_query(0, 1, None, 0, n, md, max(1, n_pairs), offsets, eid, rec, dist)
    s = h.last_stats_raw()
    h.set_option("stats", 0)
    waves = (n + 63) // 64
    say("      per point: %.2f leaf blocks visited, %.2f edges evaluated exactly; per wave of 64 points: %.2f nodes expanded, %.2f leaf blocks loaded; %d pairs appended"
        % (s[0] / n, s[1] / n, s[2] / waves, s[3] / waves, s[4]))
    assert s[4] == n_pairs
    say("      against the yardstick: traversal %.2f x (counting) and %.2f x (filling); all %.2f x (counting), %.2f x (eids only), %.2f x (with records and distances); "
        "sort + outputs is %.0f %% of the filling call"
        % (t_count[1] / t_near[1], t_fill[1] / t_near[1], t_count[3] / t_near[2], t_eids[3] / t_near[2], t_fill[3] / t_near[2], 100.0 * t_fill[2] / t_fill[3]))
    beyond = t_fill[3] - t_near[2] - t_fill[2]
    say("      %s" % ("LOSES to rj_nearest_query by %.3f ms more than the sort's share: the traversal costs it" % beyond if t_fill[1] > 1.05 * t_near[1]
                      else "the traversal keeps up with rj_nearest_query: what the call costs beyond it is the scan, the sort and the outputs"))
    # the host's check
    t0 = time.perf_counter()
    off = offsets.to_host(np.uint64, n + 1).astype(np.int64)
    e_host, r_host, d_host = eid.to_host(np.uint32, n_pairs), rec.to_host(_capi.NEAR_DTYPE, n_pairs), dist.to_host(np.float64, n_pairs)
    lens = np.diff(off)
    assert off[0] == 0 and off[n] == n_pairs and (lens >= 0).all() and int(lens.max()) == counts["max_per_point"] and int((lens > 0).sum()) == counts["n_points_hit"]
    assert np.array_equal(r_host["eid"], e_host) and np.isfinite(d_host).all() and (d_host <= md * (1 + 1e-9)).all()
    first = np.zeros(max(1, n_pairs), bool)
    first[off[:-1][lens > 0]] = True  # (the first pair of every list)
    assert ((np.diff(e_host.astype(np.int64)) > 0) | first[1:n_pairs]).all(), "a list does not ascend"
    ne_host = near_eid.to_host(np.uint32, n)
    assert np.array_equal(ne_host == _capi.MISS_EID, lens == 0), "rj_nearest_query misses elsewhere"
    rng = np.random.default_rng(17)
    hit = np.flatnonzero(lens > 0)
    pick = np.unique(np.concatenate([rng.choice(hit, min(a.sample // 2, len(hit)), replace=False), rng.choice(n, min(a.sample // 2, n), replace=False)]))
    with ThreadPoolExecutor(a.threads) as ex:
        cands = list(ex.map(lambda i: near_edges(pts[i].astype(np.float64), md), pick))
    for i, c in zip(pick, cands):
        px, py = int(pts[i][0]), int(pts[i][1])
        ids = sorted(int(v) for v in c)
        want = [(e, w, nu, de) for e in ids for (_, w, nu, de) in WR.within(px, py, [tuple(int(v) for v in seg[e])], md)]
        got = exact(r_host[off[i]:off[i + 1]])
        assert got == want, (int(i), got, want)
        assert int(ne_host[i]) in [g[0] for g in got] if got else ne_host[i] == _capi.MISS_EID
    say("      equal to the host on a sample of %d points, %d of them with a list (float64 candidates over all %d edges in numpy, the exact decision in Python "
        "integers); every list ascends; rj_nearest_query misses exactly where the list is empty, for all %d points (%.1f s)"
        % (len(pick), int((lens[pick] > 0).sum()), ne, n, time.perf_counter() - t0))
    for b in (eid, rec, dist):
        b.free()
for b in (near_eid, offsets):
    b.free()
dctx.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
