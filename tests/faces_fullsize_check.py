#!/usr/bin/env python3
"""rj_map_faces at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/simplify_fullsize_check.py; profiles/faces_fullsize.txt holds its output):

  --map NAME               a stand-in of rayjoin_amd.synth (USCounty 7.1 M edges, BlockGroup 28.8 M: lattices, one hole;
                           WaterBodiesLike: 2.4 M isolated rings, every outer boundary a hole of face 0)
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 gives 10.5 M edges)

For the map: rj_map_faces, the minimum of three warm calls (a first call goes before them), with the stage times, the grid's
shift, the registrations, the candidate tests and the cells that rays visited of the fastest; the host twin on a sub-sample of
whole connected components (--sample-chains: the first chains of a map of isolated rings, the whole map where it is one
component and small enough), compared through what does not depend on the numbering: which sides lie in face 0, and the area
of the face on each side.  Then, in a process of its own under `timeout 60` and never retried, the composition the call
replaces -- rj_map_rings with one constant label, rj_rings_polygons -- on the same map: the minimum of three warm filling
calls (the sizing calls are not counted), and its faces against rj_map_faces', side for side; or the point at which it was
abandoned."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--sample-chains", type=int, default=20000)
ap.add_argument("--twin-edges", type=int, default=12_000_000, help="a map of one component goes to the twin whole below this size")
ap.add_argument("--composition", action="store_true", help="(the child process) time the composition and compare")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("rings", "tops+kinds", "grid", "rays", "parents+faces", "all")
NONE = 0xFFFFFFFF
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def build():
    """-> (handle, name, host xy, host row, device xy, device row, what to keep alive)"""
    if a.map:
        m = maps.Context([synth.standin(a.map, 1.0)]).load().maps[0]
        xy, row = np.ascontiguousarray(m.pts, np.int64), np.ascontiguousarray(m.row_index, np.uint32)
        h = _capi.Handle(0)
        return h, a.map, xy, row, h.alloc(16 * len(xy)).from_host(xy), h.alloc(4 * len(row)).from_host(row), None
    g0, k0, g1, k1 = a.overlay
    dctx = ops.DeviceContext(maps.Context([synth.lattice_map(g0, k0, 31), synth.lattice_map(g1, k1, 32)]).load()).LoadToDevice()
    ov = ops.MapOverlay(dctx, None).Init(max(0.2, 4096.0 / sum(dctx.get_map(im).n_edges for im in range(2))))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    om = ov.OutputMap(drop_degenerate=True, merge=True)
    host = om.to_host()[0]
    name = "output map of lattice_map(%d, %d) x lattice_map(%d, %d), merged" % (g0, k0, g1, k1)
    return ov.h, name, np.ascontiguousarray(host.pts, np.int64), np.ascontiguousarray(host.row_index, np.uint32), om.xy, om.row_index, (dctx, ov, om)


def faces_call(h, d_xy, n_points, d_row, n_chains, left, right):
    t0 = time.perf_counter()
    counts = h.map_faces(d_xy, n_points, d_row, n_chains, left, right)
    wall = (time.perf_counter() - t0) * 1e3
    return counts, wall, [h.get_option("faces_last_us%d" % k) / 1000.0 for k in range(6)], dict(
        shift=h.get_option("faces_last_shift"), registrations=h.get_option("faces_last_registrations"),
        ray_tests=h.get_option("faces_last_ray_tests"), cells=h.get_option("faces_last_cells"))


def composition_faces(h, d_xy, n_points, d_row, n_chains):
    """-> (left, right as the composition numbers them: the rank of the shell among the shells, the minimum ms of three warm
    filling calls of rj_map_rings + rj_rings_polygons, the two parts of that minimum)"""
    ones = h.alloc(4 * n_chains).from_host(np.ones(n_chains, np.int32))
    best = None
    for k in range(4):
        t0 = time.perf_counter()
        r = ops.face_rings(h, d_xy, n_points, d_row, ones, ones, n_chains, capacities=None if k == 0 else caps_r)
        t1 = time.perf_counter()
        if k == 0:
            caps_r = (r.counts["n_rings"], r.counts["n_halves"], r.counts["n_points"])
            say("  composition: %s" % r.counts)
        p = r.Polygons(h, capacities=None if k == 0 else caps_p)
        t2 = time.perf_counter()
        if k == 0:
            caps_p = (p.counts["n_polygons"], p.counts["n_members"])
            say("  composition: %s" % p.counts)
        ms = ((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3)
        say("  composition call %d%s: %.3f ms (rj_map_rings %.3f, rj_rings_polygons %.3f)" % (k, " (with its sizing calls)" if k == 0 else "", *ms))
        if k > 0 and (best is None or ms[0] < best[0]):
            best = ms
        if k < 3:
            p.free()
            r.free()
    parent = p.parent.to_host(np.uint32, r.counts["n_rings"])
    first = r.ring_first.to_host(np.uint32, r.counts["n_rings"] + 1).astype(np.int64)
    half = r.ring_half.to_host(np.uint32, r.counts["n_halves"])
    p.free()
    r.free()
    ones.free()
    shells = np.flatnonzero(parent == np.arange(len(parent)))
    number = np.zeros(len(parent) + 1, np.int32)
    number[shells] = np.arange(1, len(shells) + 1)
    ring_face = number[np.where(parent == NONE, len(parent), parent)]
    face_of_half = np.zeros(2 * n_chains, np.int32)
    face_of_half[half] = ring_face[np.repeat(np.arange(len(parent)), np.diff(first))]
    return face_of_half[0::2], face_of_half[1::2], best


def side_areas(left, right, faces):
    """per side the area2 of its face as a float pair (exact below 2^53 per limb), 0 for face 0"""
    lo = np.concatenate([[0], faces["area2_lo"]]).astype(np.uint64)
    hi = np.concatenate([[0], faces["area2_hi"]]).astype(np.int64)
    return lo[left], hi[left], lo[right], hi[right]


h, name, xy, row, d_xy, d_row, keep = build()
n_points, n_chains = len(xy), len(row) - 1
left, right = h.alloc(4 * n_chains), h.alloc(4 * n_chains)
if a.composition:
    c_left, c_right, best = composition_faces(h, d_xy, n_points, d_row, n_chains)
    h.map_faces(d_xy, n_points, d_row, n_chains, left, right)
    same = np.array_equal(left.to_host(np.int32, n_chains), c_left) and np.array_equal(right.to_host(np.int32, n_chains), c_right)
    say("  composition, the minimum of three warm calls: %.3f ms (rj_map_rings %.3f, rj_rings_polygons %.3f); its faces %s rj_map_faces', side for side" % (
        *best, "EQUAL" if same else "DIFFER FROM"))
    sys.exit(0 if same else 3)

say("%s: %d chains, %d points, %d edges" % (name, n_chains, n_points, n_points - n_chains))
runs = [faces_call(h, d_xy, n_points, d_row, n_chains, left, right) for _ in range(4)]
counts = runs[0][0]
say("  rj_map_faces: %s" % counts)
say("  first call %.3f ms wall; three warm calls %s ms wall" % (runs[0][1], ", ".join("%.3f" % r[1] for r in runs[1:])))
warm = min(runs[1:], key=lambda r: r[1])
say("  the fastest warm call: %.3f ms wall; ms  %s" % (warm[1], "  ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, warm[2]))))
say("  grid: shift %(shift)d, %(registrations)d registrations, %(ray_tests)d candidate tests, %(cells)d cells visited" % warm[3]
    + " (%.1f tests a ray)" % (warm[3]["ray_tests"] / max(1, counts["n_holes"] + counts["n_outer"])))
faces = h.alloc(32 * max(1, counts["n_faces"]))
h.map_faces(d_xy, n_points, d_row, n_chains, left, right, faces, counts["n_faces"])
g_left, g_right, g_faces = left.to_host(np.int32, n_chains), right.to_host(np.int32, n_chains), faces.to_host(_capi.MAP_FACE_DTYPE, counts["n_faces"])
# the host twin on whole components
from test_faces import twin_faces, twin_lib  # noqa: E402
isolated = counts["n_rings"] == 2 * n_chains  # every chain a closed ring of its own
if isolated or n_points - n_chains <= a.twin_edges:
    k = min(n_chains, a.sample_chains) if isolated else n_chains
    t0 = time.perf_counter()
    rc, want, _ = twin_faces(twin_lib(), xy[:row[k]], row[:k + 1])
    assert rc == 0
    got, ref = side_areas(g_left[:k], g_right[:k], g_faces), side_areas(want["left"], want["right"], want["faces"])
    same = all(np.array_equal(x, y) for x, y in zip(got, ref)) and np.array_equal(g_left[:k] == 0, want["left"] == 0) and np.array_equal(g_right[:k] == 0, want["right"] == 0)
    if not isolated:
        same = same and np.array_equal(g_left, want["left"]) and np.array_equal(g_right, want["right"]) and np.array_equal(g_faces, want["faces"])
    say("  host twin on %s (%d chains, %.1f s): %s" % ("the first components" if isolated else "the whole map", k, time.perf_counter() - t0,
                                                  "equal (the sides in face 0, the area of the face on every side%s)" % ("" if isolated else ", every array") if same else "DIFFERENT"))
    assert same
else:
    say("  host twin: not run (one component of %d edges)" % (n_points - n_chains))
# the composition, in its own process, at most 60 s, once
cmd = ["timeout", "-k", "10", "60", sys.executable, os.path.abspath(__file__), "--composition"] + (["--map", a.map] if a.map else ["--overlay"] + [str(v) for v in a.overlay])
t0 = time.perf_counter()
r = subprocess.run(cmd, capture_output=True, text=True)
for line in r.stdout.splitlines():
    if line.startswith("  composition"):
        say(line)
if r.returncode in (124, 137):
    say("  composition: ABANDONED after 60 s (after the lines above)")
elif r.returncode != 0:
    say("  composition: its process ended with status %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or ""))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
sys.exit(r.returncode)  # (a caller that chains maps stops behind a composition that was abandoned or failed)
