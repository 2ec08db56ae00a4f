#!/usr/bin/env python3
"""rj_map_crossings at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/overlay_fullsize_check.py; profiles/crossings_fullsize.txt holds its output):

  --map NAME [--scale S]   a stand-in of rayjoin_amd.synth (USCounty, BlockGroup: lattices, planar by construction,
                           n_found == 0 is asserted; WaterBodiesLike: isolated rings) -- the chosen shift, the
                           registrations per edge, the largest cell, the pair tests and the HIP-event time of every stage,
                           with the two factors of the choice at their defaults, halved and doubled; beside it, for
                           orientation only, the map's first rj_build_lbvh.
  --overlay G0 K0 G1 K1    the output map (drop_degenerate, merge) of lattice_map(G0, K0) x lattice_map(G1, K1), seeds 31
                           and 32 (330 20 700 5 is tests/overlay_midsize_check.py's pair): what Crossings finds on it.
  --sample                 the same on tests/golden/sample_pair."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--map")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--overlay", type=int, nargs=4)
ap.add_argument("--sample", action="store_true")
ap.add_argument("--extent-factors", type=int, nargs="*", help="further extent factors to try (registration factor at its default)")
a = ap.parse_args()
STAGES = ("edges+sums", "registrations+sort", "runs+items", "pairs", "hits", "all")
FACTORS = ((0, 0), (4, 0), (16, 0), (0, 2), (0, 8))  # (extent, registrations); 0: the default (8, 4)
if a.extent_factors:
    FACTORS = tuple((f, 0) for f in a.extent_factors)


def report(h):
    r = {k: h.get_option("cross_last_" + k) for k in ("shift", "registrations", "largest_cell", "pair_tests", "items")}
    r["ms"] = {name: round(h.get_option("cross_last_us%d" % k) / 1000.0, 3) for k, name in enumerate(STAGES)}
    return r


def crossings_rows(h, xy, n_points, row, n_chains, n_edges):
    rows = []
    for ext, reg in ((0, 0),) + FACTORS:  # (the first call is the warm-up and is not reported)
        h.set_debug_option("cross_extent_factor", ext)
        h.set_debug_option("cross_reg_factor", reg)
        t0 = time.perf_counter()
        try:
            counts = h.map_crossings(xy, n_points, row, n_chains, 0, None)
        except _capi.CrossingsOverflow as e:
            counts = e.counts
        wall = (time.perf_counter() - t0) * 1e3
        r = report(h)
        r.update(extent_factor=ext or "default", reg_factor=reg or "default", n_found=counts["n_found"], kinds=[counts[k] for k in _capi.CROSSINGS_COUNTS[1:5]],
                 n_zero_edges=counts["n_zero_edges"], registrations_per_edge=round(r["registrations"] / max(1, n_edges), 3), wall_ms=round(wall, 3))
        rows.append(r)
    h.set_debug_option("cross_extent_factor", 0)
    h.set_debug_option("cross_reg_factor", 0)
    return rows[1:]


if a.map:
    t0 = time.perf_counter()
    m = maps.Context([synth.standin(a.map, a.scale)]).load().maps[0]
    gen_s = time.perf_counter() - t0
    h = _capi.Handle(0)
    xy = h.alloc(16 * m.n_points).from_host(np.ascontiguousarray(m.pts, np.int64))
    row = h.alloc(4 * (m.n_chains + 1)).from_host(np.ascontiguousarray(m.row_index, np.uint32))
    rows = crossings_rows(h, xy, m.n_points, row, m.n_chains, m.n_edges)
    h.upload_map(0, m.pts, m.row_index, m.left, m.right)
    h.build_lbvh(0)
    out = dict(map=a.map, scale=a.scale, edges=m.n_edges, chains=m.n_chains, generated_s=round(gen_s, 1), first_build_lbvh_ms=round(h.last_ms(_capi.RJ_T_BUILD), 3),
               runs=rows)
    print(json.dumps(out))
    if a.map in synth.STANDINS:
        assert all(r["n_found"] == 0 for r in rows), "a lattice stand-in is planar by construction"
else:
    if a.sample:
        d = os.path.join(ROOT, "tests", "golden", "sample_pair")
        gs, name = [maps.read_cdb(os.path.join(d, "map0.cdb")), maps.read_cdb(os.path.join(d, "map1.cdb"))], "sample_pair"
    else:
        g0, k0, g1, k1 = a.overlay
        gs, name = [synth.lattice_map(g0, k0, 31), synth.lattice_map(g1, k1, 32)], "lattice_map(%d, %d) x lattice_map(%d, %d)" % (g0, k0, g1, k1)
    dctx = ops.DeviceContext(maps.Context(gs).load()).LoadToDevice()
    edges = [dctx.get_map(im).n_edges for im in range(2)]
    ov = ops.MapOverlay(dctx, None).Init(max(0.2, 4096.0 / sum(edges)))
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    out = dict(pair=name, input_edges=edges, intersections=int(ov.n_xsects))
    for im in range(2):
        _, c = dctx.Crossings(im)
        out["input_map%d" % im] = {k: c[k] for k in ("n_found", "n_edges", "n_zero_edges")}
    for merge in (False, True):
        om = ov.OutputMap(drop_degenerate=True, merge=merge)
        rows = crossings_rows(ov.h, om.xy, om.n_points, om.row_index, om.n_chains, om.n_points - om.n_chains)
        records, counts = om.Crossings(ov.h)
        out["output_map_merge_%d" % int(merge)] = dict(chains=om.n_chains, edges=om.n_points - om.n_chains, counts=counts, first_records=[
            (int(r["eid"][0]), int(r["eid"][1]), int(r["kind"])) for r in records[:8]], run=rows[0])
        om.free()
    print(json.dumps(out))
    dctx.close()
