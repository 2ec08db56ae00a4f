#!/usr/bin/env python3
"""rj_knearest_query at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/nearest_fullsize_check.py; profiles/knearest_fullsize.txt holds its output).

Without --step it is a driver: one child process per base map (--bases, default USCounty and the ring map
WaterBodiesLike, each against the vertices of --query, default BlockGroup: 29.7 M points), each under its own `timeout`,
and it stops at the first child that fails.

A step (--step --base NAME) loads the pair, builds the index and takes the points fully shuffled as a caller's array under
"query_order" 1: the handle sorts them once and every call goes through the cached Morton order.  In ONE process, unlimited
and with max_dist at one mean edge length of the base map: rj_nearest_query (the yardstick, all three arrays);
rj_knearest_query at k = 1, 4 and 16 with all four arrays; with the distance also rj_within_query, the counting call and
the filling call with records and distances.  One cold call each, then the minimum of three warm ones per stage (HIP
events), and one instrumented call per k for the visit counts.  It reports the ratio to rj_nearest_query per k, the scratch
bytes and stats [0] .. [4] per point, and writes LOSES with the factor where k = 1 is slower than rj_nearest_query or a
limited run is slower than rj_within_query's filling call.  Verified: at k = 1 the three arrays equal rj_nearest_query's,
byte for byte, over all points; every run on a sample of points against the host twin's brute force over ALL edges
(tests/hosttwin/knearest_twin.cc), count, eids and records."""
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
ap.add_argument("--sample", type=int, default=128)
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
import test_knearest as TK  # noqa: E402
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

KS = (1, 4, 16)
N_STAGES = ("ordering", "traversal", "all")
W_STAGES = ("ordering", "traversal", "sort + outputs", "all")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


twin = TK.twin_lib()
ctx = maps.Context([synth.standin(a.base, a.scale), synth.standin(a.query, a.scale)]).load()
dctx = ops.DeviceContext(ctx).LoadToDevice()
h = dctx.handle
dctx.BuildIndex(0)
base = ctx.maps[0]
n, ne = ctx.maps[1].n_points, base.n_edges
pts = np.ascontiguousarray(np.ascontiguousarray(ctx.maps[1].pts, np.int64).reshape(-1, 2)[np.random.default_rng(11).permutation(n)])
seg = base.segments()
sf = seg.astype(np.float64)
mean_len = int(np.hypot(sf[:, 2] - sf[:, 0], sf[:, 3] - sf[:, 1]).mean())
del sf
say("%s x %s%s: %d points against %d edges (index: %d levels); max_dist = the mean edge length = %d"
    % (a.base, a.query, "" if a.scale == 1.0 else " at scale %g" % a.scale, n, ne, [i for i in h.get_plan()["index"] if i["map"] == 0][0]["levels"], mean_len))
say("  the points fully shuffled, a caller's array, \"query_order\" 1: sorted once, every call through the cached Morton order")
h.set_option("query_order", 1)
kmax = max(KS)
src = h.alloc(16 * n).from_host(pts)
n_eid, n_rec, n_dist = h.alloc(4 * n), h.alloc(40 * n), h.alloc(8 * n)
cnt, eid, rec, dist = h.alloc(4 * n), h.alloc(4 * n * kmax), h.alloc(40 * n * kmax), h.alloc(8 * n * kmax)
pick = np.sort(np.random.default_rng(17).choice(n, min(a.sample, n), replace=False))


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


def rows(buf, dtype, i, k):
    """row i of a device array of rows of k entries"""
    out = np.empty(k, dtype)
    h._check(_capi.load().rj_memcpy_d2h(h.h, out.ctypes.data, buf.ptr + i * k * out.itemsize, out.nbytes))
    return out


def verify(k, md):
    """count, eids and records of the sampled points against the twin's brute force over all edges"""
    t0 = time.perf_counter()
    parts = np.array_split(pick, a.threads)
    with ThreadPoolExecutor(a.threads) as ex:
        want = list(ex.map(lambda p: TK.run_twin(twin, seg, pts[p], k, md), parts))
    counts = cnt.to_host(np.uint32, n)
    for p, w in zip(parts, want):
        for j, i in enumerate(p):
            i = int(i)
            assert counts[i] == w.count[j], (i, counts[i], w.count[j])
            assert np.array_equal(rows(eid, np.uint32, i, k), w.eid[j]) and np.array_equal(rows(rec, _capi.NEAR_DTYPE, i, k), w.rec[j]), i
            d = rows(dist, np.float64, i, k)
            assert np.array_equal(np.isinf(d), w.eid[j] == _capi.MISS_EID) and np.allclose(d[:w.count[j]], w.dist[j, :w.count[j]], rtol=1e-14, atol=0)
    say("      equal to the host twin's brute force over all %d edges on a sample of %d points: counts, eids, records (%.1f s)" % (ne, len(pick), time.perf_counter() - t0))
    return counts


for md in (-1, mean_len):
    say("  %s" % ("unlimited" if md < 0 else "max_dist %d" % md))
    cold, warm, t_near = best_of(lambda: h.nearest_query(0, 1, src, 0, n, n_eid, n_rec, n_dist, max_dist=md), N_STAGES, "nearest_last_us%d")
    report("rj_nearest_query, the yardstick (eids, records, distances)", cold, warm, N_STAGES, t_near)
    t_fill = None
    if md >= 0:
        wc = {}
        offsets = h.alloc(8 * (n + 1))
        cold, warm, t_count = best_of(lambda: wc.update(h.within_query(0, 1, src, 0, n, md, 0, offsets)), W_STAGES, "within_last_us%d")
        report("rj_within_query, the counting call (offsets and counts)", cold, warm, W_STAGES, t_count)
        cap = max(1, wc["n_pairs"])
        w_eid, w_rec, w_dist = h.alloc(4 * cap), h.alloc(40 * cap), h.alloc(8 * cap)
        cold, warm, t_fill = best_of(lambda: h.within_query(0, 1, src, 0, n, md, cap, offsets, w_eid, w_rec, w_dist), W_STAGES, "within_last_us%d")
        report("rj_within_query, the filling call (offsets, eids, records, distances)", cold, warm, W_STAGES, t_fill)
        say("      n_pairs %d, n_points_hit %d, max_per_point %d" % (wc["n_pairs"], wc["n_points_hit"], wc["max_per_point"]))
        for b in (offsets, w_eid, w_rec, w_dist):
            b.free()
    for k in KS:
        call = lambda: h.knearest_query(0, 1, src, 0, n, k, eid, cnt, rec, dist, max_dist=md)  # noqa: E731
        cold, warm, t_k = best_of(call, N_STAGES, "knearest_last_us%d")
        report("rj_knearest_query, k = %d (counts, eids, records, distances)" % k, cold, warm, N_STAGES, t_k)
        scratch = h.get_option("knearest_last_scratch_bytes")
        h.set_option("stats", 1)
        call()
        s = h.last_stats_raw()
        h.set_option("stats", 0)
        waves = (n + 63) // 64
        say("      scratch %d bytes (%.1f MiB; the outputs: %.1f MiB); per point: %.2f leaf blocks visited, %.2f edges evaluated exactly, %.2f entered a list; "
            "per wave of 64 points: %.2f nodes expanded, %.2f leaf blocks loaded" % (scratch, scratch / 2 ** 20, n * (4 + 52 * k) / 2 ** 20, s[0] / n, s[1] / n, s[4] / n, s[2] / waves, s[3] / waves))
        ratio = t_k[1] / t_near[1]
        say("      the traversal is %.2f x rj_nearest_query's (%.3f against %.3f ms)%s" % (ratio, t_k[1], t_near[1], "  -- LOSES by %.2f x at k = 1" % ratio if k == 1 and ratio > 1 else ""))
        if t_fill is not None:
            r = t_k[2] / t_fill[3]
            say("      the call is %.2f x rj_within_query's filling call (%.3f against %.3f ms)%s" % (r, t_k[2], t_fill[3], "  -- LOSES by %.2f x" % r if r > 1 else ""))
        counts = verify(k, md)
        say("      counts: %d points with k edges, %d with fewer, %d with none" % ((counts == k).sum(), ((counts < k) & (counts > 0)).sum(), (counts == 0).sum()))
        if k == 1:
            for what, x, y, dt in (("eids", n_eid, eid, np.uint32), ("records", n_rec, rec, np.uint32), ("distances", n_dist, dist, np.uint64)):
                m = x.nbytes // np.dtype(dt).itemsize
                assert np.array_equal(x.to_host(dt, m), y.to_host(dt, m)), what
            assert np.array_equal(counts, (n_eid.to_host(np.uint32, n) != _capi.MISS_EID).astype(np.uint32))
            say("      at k = 1 the eids, the records and the distances of all %d points equal rj_nearest_query's byte for byte" % n)
for b in (src, n_eid, n_rec, n_dist, cnt, eid, rec, dist):
    b.free()
dctx.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
