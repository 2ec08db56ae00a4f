#!/usr/bin/env python3
"""rj_nearest_query at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/face_points_fullsize_check.py; profiles/nearest_fullsize.txt holds its output):

  --base NAME --query NAME [--scale S]   two stand-ins of rayjoin_amd.synth: the nearest edge of the base map for every
                                         vertex of the query map.  bench.py's pairs: USCounty x BlockGroup (29.7 M points),
                                         WaterBodiesLike x BlockGroup

Per pair: the points in the order of the query map (they follow their chains: coherent), the same points fully shuffled as
a caller's array under "query_order" 1 (the handle sorts them once and keeps the Morton order) and under "query_order" 0
(as given); each unlimited and with max_dist at about one mean edge length of the base map.  One cold call, then the
minimum of three warm ones per stage (HIP events), then one instrumented call for the visit counts.  Beside them, from
the same process: rj_pip_query of the same points over the same index (RJ_T_PIP_KERNEL, the minimum of three warm calls),
and a torch float64 brute force over all edges on 1 024 of the points, scaled to the point count.  Verified on the host:
for a random sample of points the candidates within 1 + 1e-9 of the float64 minimum over ALL edges in numpy, the exact
choice among them in Python integers (tests/nearest_ref.py), equal to the device's eid, where, num and den; and the
shuffled runs equal to the ordered one, point for point."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref as NR  # noqa: E402
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--base", default="USCounty")
ap.add_argument("--query", default="BlockGroup")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--sample", type=int, default=500)
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("ordering", "traversal", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def exact(rec):
    return [(int(r["eid"]), int(r["where"]), (int(r["num_hi"]) << 64) + int(r["num_lo"]), (int(r["den_hi"]) << 64) + int(r["den_lo"])) for r in rec]


if not a.no_torch:  # (torch opens the device first, as in bench.py)
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
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
say("%s x %s%s: %d points against %d edges (index: %d levels); max_dist = the mean edge length = %d"
    % (a.base, a.query, "" if a.scale == 1.0 else " at scale %g" % a.scale, n, ne, [i for i in h.get_plan()["index"] if i["map"] == 0][0]["levels"], mean_len))
eid, rec, dist = h.alloc(4 * n), h.alloc(40 * n), h.alloc(8 * n)
face = h.alloc(4 * n)


def run(what, src, max_dist):
    """-> (the records on the host, the traversal's best ms)"""
    best, walls = None, []
    for k in range(4):
        t0 = time.perf_counter()
        h.nearest_query(0, 1, src, 0, n, eid, rec, dist, max_dist=max_dist)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = [h.get_option("nearest_last_us%d" % s) / 1000.0 for s in range(3)]
        if k:
            best = ms if best is None else [min(p, q) for p, q in zip(best, ms)]
    h.set_option("stats", 1)
    h.nearest_query(0, 1, src, 0, n, eid, rec, dist, max_dist=max_dist)
    s = h.last_stats_raw()
    h.set_option("stats", 0)
    r = rec.to_host(_capi.NEAR_DTYPE, n)
    say("  %s, %s" % (what, "unlimited" if max_dist < 0 else "max_dist %d" % max_dist))
    say("    first call %.3f ms wall; three warm calls %s ms wall" % (walls[0], ", ".join("%.3f" % w for w in walls[1:])))
    say("    the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (t, v) for t, v in zip(STAGES, best)))
    say("    per point: %.2f leaf blocks visited, %.2f edges evaluated exactly; per wave of 64 points: %.2f nodes expanded, %.2f leaf blocks loaded; %d misses"
        % (s[0] / n, s[1] / n, s[2] / ((n + 63) // 64), s[3] / ((n + 63) // 64), int((r["eid"] == _capi.MISS_EID).sum())))
    return r, best


def pip_ms(src):
    best = None
    for k in range(4):
        h.pip_query(0, 1, src, 0, n, eid, face)
        if k:
            ms = h.last_ms(_capi.RJ_T_PIP_KERNEL)
            best = ms if best is None else min(best, ms)
    return best


ax, ay = sf[:, 0].copy(), sf[:, 1].copy()
dx, dy = sf[:, 2] - ax, sf[:, 3] - ay
ll = np.maximum(dx * dx + dy * dy, 1.0)


def candidates(p):
    """the edges within 1 + 1e-9 of the float64 minimum over all edges"""
    ex, ey = p[0] - ax, p[1] - ay
    t = np.clip((ex * dx + ey * dy) / ll, 0.0, 1.0)
    ex -= t * dx
    ey -= t * dy
    d2 = ex * ex + ey * ey
    return np.nonzero(d2 <= d2.min() * (1 + 1e-9) ** 2 + 1e-300)[0]


def verify(r, points, max_dist):
    t0 = time.perf_counter()
    pick = np.random.default_rng(17).choice(n, min(a.sample, n), replace=False)
    with ThreadPoolExecutor(a.threads) as ex:
        cands = list(ex.map(lambda i: candidates(points[i].astype(np.float64)), pick))
    got = exact(r[pick])
    for i, c, g in zip(pick, cands, got):
        px, py = int(points[i][0]), int(points[i][1])
        best, best_d2 = (NR.MISS, 0, 0, 0), None
        for e in sorted(int(v) for v in c):
            where, num, den = NR.point_edge(px, py, tuple(int(v) for v in seg[e]))
            d2 = NR.d2_of(where, num, den)
            if max_dist >= 0 and d2 > max_dist * max_dist:
                continue
            if best_d2 is None or d2 < best_d2:
                best, best_d2 = (e, where, num, den), d2
        assert g == best, (int(i), g, best)
    say("    equal to the host on a sample of %d points (float64 candidates over all %d edges in numpy, the exact choice in Python integers; %.1f s)"
        % (len(pick), ne, time.perf_counter() - t0))


def torch_yardstick(points):
    import torch
    dev = torch.device("cuda:0")
    S = torch.from_numpy(sf).to(dev)
    tax, tay = S[:, 0].contiguous(), S[:, 1].contiguous()
    tdx, tdy = S[:, 2] - tax, S[:, 3] - tay
    tl = torch.clamp(tdx * tdx + tdy * tdy, min=1.0)
    P = torch.from_numpy(points[:1024].astype(np.float64)).to(dev)
    chunk = max(1, min(64, (1 << 27) // max(1, ne)))

    def once():
        out = []
        for k in range(0, len(P), chunk):
            ex, ey = P[k:k + chunk, 0:1] - tax, P[k:k + chunk, 1:2] - tay
            t = torch.clamp((ex * tdx + ey * tdy) / tl, 0.0, 1.0)
            ex, ey = ex - t * tdx, ey - t * tdy
            out.append(torch.argmin(ex * ex + ey * ey, dim=1))
        return torch.cat(out)
    best = None
    for k in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once()
        e1.record()
        torch.cuda.synchronize()
        if k:
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
    say("  the torch yardstick: a float64 brute force over all %d edges (argmin only: inexact, no ties, no record) takes %.3f ms for %d points, "
        "that is %.0f ms scaled to all %d" % (ne, best, len(P), best * n / len(P), n))
    del S, P
    torch.cuda.empty_cache()


ordered = {}
for md in (-1, mean_len):
    r, best = run("query order (the vertices of the query map)", None, md)
    verify(r, pts, md)
    ordered[md] = (r.copy(), best)
t_pip = pip_ms(None)
say("  rj_pip_query of the same points over the same index: %.3f ms (RJ_T_PIP_KERNEL, the minimum of three warm calls); rj_nearest_query's traversal is "
    "%.2f x that unlimited, %.2f x with max_dist" % (t_pip, ordered[-1][1][1] / t_pip, ordered[mean_len][1][1] / t_pip))
perm = np.random.default_rng(11).permutation(n)
shuffled = np.ascontiguousarray(pts[perm])
src = h.alloc(16 * n).from_host(shuffled)
for qo, what in ((1, "fully shuffled, a caller's array, \"query_order\" 1 (sorted once, the Morton order cached)"), (0, "fully shuffled, \"query_order\" 0 (as given)")):
    h.set_option("query_order", qo)
    for md in (-1, mean_len):
        r, best = run(what, src, md)
        assert np.array_equal(r, ordered[md][0][perm]), "the shuffled run differs from the ordered one"
        say("    equal to the ordered run, point for point; the traversal is %.2f x the ordered one" % (best[1] / ordered[md][1][1]))
    t = pip_ms(src)
    say("  rj_pip_query of the shuffled points under \"query_order\" %d: %.3f ms" % (qo, t))
h.set_option("query_order", 1)
if not a.no_torch:
    torch_yardstick(pts)
for b in (eid, rec, dist, face, src):
    b.free()
dctx.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
