#!/usr/bin/env python3
"""The overlay's output map at FULL size (BASELINE config 4, USCounty x Zipcode stand-ins), not collected by pytest:
rj_overlay_map against the helper's numpy form (tests/overlay_map_ref.output_map_np, fed the device's own records and
vertex faces) -- the three counts, every array, and a sample of chains walked by the plain-Python helper -- and its wall
time next to rj_overlay_faces measured in the same process on the same inputs.  --host_path also runs polyover_exec on
the same maps and reports its phases "Write to file" (the host writer, printing included), "Compute output map" and
"Write output map"."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, synth  # noqa: E402
import overlay_map_ref as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m0", default="USCounty")
ap.add_argument("--m1", default="Zipcode")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sample", type=int, default=200)
ap.add_argument("--host_path", action="store_true")
a = ap.parse_args()
graphs = [synth.standin(a.m0, a.scale), synth.standin(a.m1, a.scale)]
ctx = maps.Context(graphs).load()
m = ctx.maps
h = _capi.Handle(0)
for im in range(2):
    h.upload_map(im, m[im].pts, m[im].row_index, m[im].left, m[im].right)
h.build_lbvh(0)
h.build_lbvh(1)
cap = int(0.2 * (m[0].n_edges + m[1].n_edges))
pairs = h.alloc(8 * cap)
n = h.lsi_query(1, 0, 0, m[0].n_edges, cap, pairs)
fc = [h.alloc(4 * m[i].n_points) for i in range(2)]
cl = [h.alloc(4 * m[i].n_points) for i in range(2)]
for im in range(2):
    h.pip_query(1 - im, im, None, 0, m[im].n_points, cl[im], fc[im])
xs = [h.alloc(48 * max(1, n)) for _ in range(2)]
for im in range(2):
    h.overlay_edge_xsects(im, pairs, n, xs[im])
h.sync()


def timed(fn):
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, [round(v, 3) for v in ms]


rcap = 4 * n + m[0].n_chains + m[1].n_chains + 1024
rows = h.alloc(_capi.FACE_DTYPE.itemsize * rcap)
nrows, faces_ms = timed(lambda: h.overlay_faces(xs[0], xs[1], n, fc[0], fc[1], rcap, rows))
args = (xs[0], xs[1], n, fc[0], fc[1])
out = {"map0_edges": m[0].n_edges, "map1_edges": m[1].n_edges, "intersections": n, "face_rows": int(nrows), "face_table_ms": faces_ms,
       "face_table_ms_best": min(faces_ms)}
try:
    h.overlay_map(*args, 0, (0, 0, 0), None, None, None, None, None, None)
    counts = (0, 0, 0)
except _capi.MapOverflow as e:
    counts = e.counts
cc, pc, fcap = counts
bufs = [h.alloc(16 * max(1, pc)), h.alloc(4 * (cc + 1)), h.alloc(4 * max(1, cc)), h.alloc(4 * max(1, cc)), h.alloc(8 * max(1, fcap)),
        h.alloc(4 * max(1, cc))]
dxs = [xs[im].to_host(_capi.XSECT_DTYPE, n) for im in range(2)]
dpip = [fc[im].to_host(np.int32, m[im].n_points) for im in range(2)]
ok = True
for drop in (0, 1):
    got_counts, ms = timed(lambda: h.overlay_map(*args, drop, (cc, pc, fcap), *bufs))
    k, p, f = got_counts
    got = dict(xy=bufs[0].to_host(np.int64, 2 * p).reshape(-1, 2), row_index=bufs[1].to_host(np.uint32, k + 1),
               left=bufs[2].to_host(np.int32, k), right=bufs[3].to_host(np.int32, k),
               face_pairs=bufs[4].to_host(np.int32, 2 * f).reshape(-1, 2), origin=bufs[5].to_host(np.uint32, k))
    want = M.output_map_np(m, dxs, dpip, drop_degenerate=bool(drop))
    same = {name: bool(got[name].shape == want[name].shape and np.array_equal(got[name], want[name]))
            for name in ("xy", "row_index", "left", "right", "face_pairs", "origin")}
    tag = "drop" if drop else "flags0"
    out["map_%s_ms" % tag] = ms
    out["map_%s_ms_best" % tag] = min(ms)
    out["map_%s_counts" % tag] = [int(k), int(p), int(f)]
    out["map_%s_counts_equal_helper" % tag] = (int(k), int(p), int(f)) == (len(want["left"]), len(want["xy"]), len(want["face_pairs"]))
    out["map_%s_arrays_equal_helper" % tag] = same
    out["one_point_pieces"] = want["n_one_point"]
    ok = ok and out["map_%s_counts_equal_helper" % tag] and all(same.values())
    if not drop:
        # a sample of source chains walked by the plain-Python helper (sub-maps of one chain each, its records and faces)
        rng = np.random.default_rng(5)
        sampled = bad = 0
        first_of = {}
        for i, o in enumerate(got["origin"].tolist()):
            first_of.setdefault(o, i)
        for im in range(2):
            cut_chains = np.unique(np.searchsorted(m[im].row_index.astype(np.int64)[1:] - 1 - np.arange(m[im].n_chains),
                                                   dxs[im]["eid"][:, im].astype(np.int64), side="right"))
            pick = np.r_[rng.choice(m[im].n_chains, a.sample // 4), rng.choice(cut_chains, min(len(cut_chains), a.sample // 4))]
            for c in pick.tolist():
                b, e = int(m[im].row_index[c]), int(m[im].row_index[c + 1])
                sub = maps.ScaledMap(im, m[im].pts[b:e], np.array([0, e - b], np.uint32), m[im].left[c:c + 1], m[im].right[c:c + 1])
                rec = dxs[im][(dxs[im]["eid"][:, im] >= b - c) & (dxs[im]["eid"][:, im] < e - 1 - c)].copy()
                rec["eid"][:, im] -= b - c
                empty = maps.ScaledMap(1 - im, np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int64))
                none = np.zeros(0, np.int32)
                if im == 0:
                    walked = M.pieces([sub, empty], [rec, rec[:0]], [dpip[0][b:e], none])
                else:
                    walked = M.pieces([empty, sub], [rec[:0], rec], [none, dpip[1][b:e]])
                sampled += 1
                i0 = first_of.get((im << 31) | c)
                if i0 is None:
                    bad += len(walked) != 0
                    continue
                for j, q in enumerate(walked):
                    i = i0 + j
                    pts = got["xy"][int(got["row_index"][i]):int(got["row_index"][i + 1])].tolist()
                    pairs_lr = [tuple(got["face_pairs"][v - 1].tolist()) if v else None for v in (int(got["left"][i]), int(got["right"][i]))]
                    want_lr = [M.ordered_pair(im, mine, q[4]) if mine else None for mine in (q[2], q[3])]
                    bad += int(got["origin"][i]) != ((im << 31) | c) or pts != [list(t) for t in q[5]] or pairs_lr != want_lr
        out["sampled_chains"] = sampled
        out["sampled_chains_off"] = int(bad)
        ok = ok and bad == 0
h.close()
out["map_over_face_table"] = round(out["map_flags0_ms_best"] / out["face_table_ms_best"], 2)

if a.host_path:
    with tempfile.TemporaryDirectory() as d:
        for i, g in enumerate(graphs):
            maps.serialize_bin(g, os.path.join(d, "m%d.bin" % i))  # (load_from finds <dir>/<path>.bin and reads no text)
        r = subprocess.run([os.path.join(ROOT, "rayjoin_amd", "polyover_exec"), "-poly1", "m0", "-poly2", "m1", "-serialize", d, "-mode", "lbvh",
                            "-check=false", "-output", os.path.join(d, "out.cdb"), "-output_map", os.path.join(d, "om.cdb")],
                           capture_output=True, text=True, timeout=1500)
        out["polyover_exec_rc"] = r.returncode
        out["polyover_exec_ms"] = {k: float(v) for k, v in re.findall(r"^ - (.*): ([-+.e0-9]+) ms$", r.stderr, flags=re.M)}
        if r.returncode:
            out["polyover_exec_stderr"] = r.stderr[-1000:]
        ok = ok and r.returncode == 0
out["ok"] = bool(ok)
print(json.dumps(out))
sys.exit(0 if ok else 1)
