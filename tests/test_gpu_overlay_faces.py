"""The overlay's face table on the device (rj_overlay_faces, ops.MapOverlay.FaceTable, polyover_exec -face_table) against
the plain-Python oracle (tests/overlay_faces_ref.py): the same rows and the same int128 areas, bit for bit."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
from test_overlay_faces import geometry_pair  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")

pytestmark = pytest.mark.gpu


def _pair(name):
    if name == "sample":
        return [maps.read_cdb(os.path.join(D, "map0.cdb")), maps.read_cdb(os.path.join(D, "map1.cdb"))], 512
    if name == "lattice":
        return [synth.lattice_map(3, 90, 61), synth.lattice_map(400, 1, 62)], 1024
    if name == "rings":
        return [synth.ring_map(60, 900, seed=63), synth.lattice_map(6, 30, 64)], 256
    if name == "nested":
        base = synth.lattice_map(5, 24, 65)
        return [base, synth.nested_refinement(base, 5, 24, 3, 10, seed=66)], 512
    raise KeyError(name)


def device_table(ctx, grid_size=None, capacity=None):
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    try:
        ov = ops.MapOverlay(dctx, grid_size).Init(1.0)
        ov.BuildIndex()
        ov.IntersectEdge(0)
        ov.LocateVerticesInOtherMap(0)
        ov.LocateVerticesInOtherMap(1)
        ov.ComputeOutputPolygons()
        t = ov.FaceTable(capacity)
        return t, ov.n_xsects, [ov.get_xsects(im) for im in range(2)], [ov.get_vertex_faces(im) for im in range(2)]
    finally:
        dctx.close()


def as_rows(t):
    return [(int(a), int(b), int(c)) for a, b, c in zip(t["face0"], t["face1"], t["area2"])]


@pytest.mark.parametrize("pair", ["sample", "lattice", "rings", "nested"])
def test_device_table_equals_the_oracle(oracle, pair):
    gs, gsize = _pair(pair)
    ctx = maps.Context(gs).load()
    want, xs, _ = F.oracle_face_rows(oracle, ctx, gsize)
    assert len(want) > 3
    # -mode=grid records (the oracle's, bit for bit): the oracle pipeline's table
    got_grid, n, dxs, dpip = device_table(ctx, grid_size=gsize)
    assert n == len(xs[0])
    assert as_rows(got_grid) == want
    # LBVH records: the chain walk over the device's own records and vertex faces
    got, n, dxs, dpip = device_table(ctx)
    assert as_rows(got) == F.rows(F.face_table(ctx.maps, dxs, dpip))
    if pair != "nested":  # (on the nested pair the LBVH finds two touching pairs at shared vertices the grid does not)
        assert n == len(xs[0]) and as_rows(got) == want
    k = 0.5 * float(ctx.scaling.rrx) * float(ctx.scaling.rry)
    assert np.array_equal(got["area"], np.array([float(a) * k for _, _, a in as_rows(got)]))


def test_rows_of_each_face_sum_to_its_area(oracle):
    g0, g1 = geometry_pair()
    ctx = maps.Context([g0, g1]).load()
    got = device_table(ctx)[0]
    rows = as_rows(got)
    assert rows == F.oracle_face_rows(oracle, ctx, 256)[0]
    assert all(a > 0 for _, _, a in rows)
    per0 = {}
    for f0, _, a in rows:
        per0[f0] = per0.get(f0, 0) + a
    assert sorted(per0) == list(range(1, 17))
    for f0, s in per0.items():
        want = F.shoelace2(ctx.maps[0], f0)
        assert abs(s - want) <= 1e-9 * want, f0


def test_capacity_one_short_overflows_with_the_true_count():
    gs, _ = _pair("sample")
    ctx = maps.Context(gs).load()
    full = device_table(ctx)[0]
    with pytest.raises(_capi.QueueOverflow) as e:
        device_table(ctx, capacity=len(full) - 1)
    assert e.value.n_found == len(full)
    exact = device_table(ctx, capacity=len(full))[0]
    assert as_rows(exact) == as_rows(full)


def test_disjoint_maps_and_a_map_inside_one_face():
    # disjoint: no intersection, no vertex inside the other map -> no row
    a = synth.lattice_map(3, 5, 81, bbox=(-120.0, 30.0, -110.0, 40.0))
    b = synth.lattice_map(4, 5, 82, bbox=(-100.0, 30.0, -90.0, 40.0))
    t, n = device_table(maps.Context([a, b]).load())[:2]
    assert n == 0 and len(t) == 0
    # map 1 inside the one face of map 0: n == 0, one row per face of map 1 with its whole area
    big = synth.lattice_map(1, 8, 83, bbox=(-130.0, 20.0, -80.0, 50.0), vertex_jitter=0.0)
    small = synth.lattice_map(3, 5, 84, bbox=(-110.0, 30.0, -100.0, 40.0))
    ctx = maps.Context([big, small]).load()
    t, n = device_table(ctx)[:2]
    assert n == 0
    assert as_rows(t) == [(1, f1, F.shoelace2(ctx.maps[1], f1)) for f1 in range(1, 10)]


@pytest.mark.parametrize("pair", ["sample", "lattice"])
def test_polyover_exec_face_table(oracle, tmp_path, pair):
    """-face_table writes the oracle's text; the unordered pairs are the output map's "Total faces"; without the flag
    the stderr phases and the output file are what they were"""
    gs, gsize = _pair(pair)
    if pair == "sample":
        p0, p1 = os.path.join(D, "map0.cdb"), os.path.join(D, "map1.cdb")
    else:
        p0, p1 = str(tmp_path / "a.cdb"), str(tmp_path / "b.cdb")
        maps.write_cdb(p0, gs[0], "%.9f")
        maps.write_cdb(p1, gs[1], "%.9f")
    ctx = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load()
    want, _, _ = F.oracle_face_rows(oracle, ctx, gsize)
    out, ft = str(tmp_path / "o.txt"), str(tmp_path / "faces.txt")
    r = subprocess.run([EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-output", out, "-xsect_factor", "1.0",
                        "-face_table", ft], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert " - Compute face table: " in r.stderr
    assert open(ft).read() == F.text(want, ctx.scaling)
    total_faces = int(re.search(r"Total faces: (\d+)", r.stderr).group(1))
    assert len({(min(a, b), max(a, b)) for a, b, _ in want}) == total_faces
    out2 = str(tmp_path / "o2.txt")
    r2 = subprocess.run([EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-output", out2, "-xsect_factor", "1.0"],
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "face table" not in r2.stderr
    assert open(out2).read() == open(out).read()


def test_uscounty_zipcode_face_table_full_size():
    """BASELINE config 4 (USCounty x Zipcode stand-ins) at full size: every face of map 0 that is not on the map's
    border is covered by map 1, and its rows sum to its own shoelace area (exact ints); no row's area is negative.
    Child process (30 M-segment maps); prints the stage's time."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlay_faces_fullsize_check.py")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(out)
    assert out["rows"] > 10000 and out["intersections"] > 10000
    assert out["negative_rows"] == 0 and out["interior_faces_checked"] > 1000
    assert out["interior_faces_off"] == 0 and out["border_faces_over"] == 0
