"""Polygons of face rings on the device (rj_rings_polygons, DeviceRings.Polygons, polyover_exec -polygons) against the
plain-Python definition (tests/polygons_ref.py), array for array: the cases of tests/polygons_cases.py (hand cases, hole
columns, ray degeneracies, the domain-wide edge, laminar families with construction-known parents), the rings of the
device's OWN output maps of the overlay tests' pairs (five calls, drop and merge on and off) with the exact area invariant
against the device's own face table, the rings of fuzzed overlays; against the host twin where the input is too large for
the Python loop (the lattice pair's clip, more rings than one grid covers, more than 2^16 holes in one face); the raw ring
sets of tests/polygons_soups.py against the answers tests/test_polygons.py holds the definition, the twin and the
constructions equal on; overflow with canaries, the sizing call, no rings, malformed input; the command line.  The CPU
side is tests/test_polygons.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_hard_pairs as H  # noqa: E402
import polygons_cases as PC  # noqa: E402
import polygons_ref as PR  # noqa: E402
import polygons_soups as PS  # noqa: E402
import rings_planar as P  # noqa: E402
import rings_ref as D  # noqa: E402
import test_gpu_overlay_fuzz as FZ  # noqa: E402
from test_gpu_overlay_hard import run_overlay  # noqa: E402
from test_gpu_overlay_merge import CALLS, DROP, MERGE, overlay_of, raw_map  # noqa: E402
from test_gpu_rings import FUZZ_EDGE_CAP, DeviceMap  # noqa: E402
from test_overlay_map import pair  # noqa: E402
from test_overlay_ops import OPS  # noqa: E402
from test_polygons import BIG_FIELD_SIDE, CARRY_SQUARES, FAN_SEEDS, LAMINAR_GPU_SEEDS, SLIVER_SEEDS, big_field_case, check_hole_field, soup_case  # noqa: E402
from test_polygons import args_of, bad_inputs, hand_case, laminar_case, span_case, twin_lib, twin_polygons  # noqa: E402
from test_rings import FIELD  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")
NONE = PR.NONE


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


def upload_rings(h, rings, ring_row, ring_xy):
    """the three arrays of rj_map_rings that rj_rings_polygons reads -> an ops.DeviceRings (no half-chains)"""
    rings = np.ascontiguousarray(rings, D.RING_DTYPE)
    row = np.ascontiguousarray(ring_row, np.uint32)
    xy = np.ascontiguousarray(ring_xy, np.int64).reshape(-1, 2)
    counts = dict(n_rings=len(rings), n_halves=0, n_points=len(xy), n_mixed=0, n_skipped=0)
    return ops.DeviceRings(h.alloc(32 * max(1, len(rings))).from_host(rings), h.alloc(4 * (len(rings) + 1)), h.alloc(4),
                           h.alloc(4 * len(row)).from_host(row), h.alloc(16 * max(1, len(xy))).from_host(xy), counts)


def device_polygons(h, rings, ring_row, ring_xy):
    r = upload_rings(h, rings, ring_row, ring_xy)
    try:
        p = r.Polygons(h)
        got = p.to_host()
        p.free()
        return got
    finally:
        r.free()


def polygons_of_rings(h, r):
    """(the rings on the host, the device's polygons of them) of a DeviceRings; frees it"""
    try:
        p = r.Polygons(h)
        got = p.to_host()
        p.free()
        return r.to_host(), got
    finally:
        r.free()


def face_sums(p):
    sums = {}
    for f, a2 in zip(p["polygons"]["face"].tolist(), PR.area2_of(p["polygons"])):
        sums[f] = sums.get(f, 0) + a2
    return sums


# ---- device against the definition ------------------------------------------------------------------------------------
def test_hand_cases_equal_the_definition(handle):
    for name in sorted(PC.HAND):
        rg, want = hand_case(name)
        PR.assert_same_polygons(device_polygons(handle, *args_of(rg)), want, name)
    _, p = hand_case("multi-part")
    assert p["counts"]["n_polygons"] == 6 and hand_case("column-1000")[1]["counts"]["n_holes"] == 1000 and hand_case("orphan")[1]["counts"]["n_orphans"] == 1


def test_domain_wide_edge(handle):
    rg, want = span_case()
    PR.assert_same_polygons(device_polygons(handle, *args_of(rg)), want)


@pytest.mark.parametrize("seed", LAMINAR_GPU_SEEDS)
def test_laminar_families_have_the_parents_of_the_construction(handle, seed):
    rg, want, parents = laminar_case(seed)
    got = device_polygons(handle, *args_of(rg))
    PR.assert_same_polygons(got, want, seed)
    assert np.array_equal(got["parent"], parents) and got["counts"]["n_orphans"] == 0


@pytest.mark.parametrize("name", ["sample", "rings", "nested"])
def test_own_output_maps_equal_the_definition(name):
    """the rings of the device's own output maps: the five calls, drop and merge on and off, with and without the rings of
    face 0.  On the pairs in general position there is no orphan and the polygons of face k sum to row k - 1 of the device's
    own face table, exactly."""
    gs, _ = pair(name)
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    holes = 0
    try:
        for call in CALLS:
            how, by = call if call is not None else ("intersection", "pair")
            table = ov.FaceTable(how=how, by=by)
            for flags in (0, DROP, MERGE, DROP | MERGE):
                what = (name, call, flags)
                om = raw_map(ov, call, flags)
                rg, got = polygons_of_rings(ov.h, om.Rings(ov.h, skip_face0=bool(flags & MERGE)))
                om.free()
                PR.assert_same_polygons(got, PR.polygons_ref(*args_of(rg)), what)
                holes += got["counts"]["n_holes"]
                if name == "nested":
                    continue
                assert got["counts"]["n_orphans"] == 0 and rg["counts"]["n_mixed"] == 0, what
                sums = face_sums(got)
                assert [sums[k + 1] for k in range(len(table))] == [int(a) for a in table["area2"]] and len(sums) == len(table), what
        assert holes > 0 or name == "sample"
    finally:
        dctx.close()


def test_polygons_of_an_output_map_with_points():
    """DevicePolygons.polygons: the (union, pair) map of the rings pair has 47 holes; every polygon's points are its
    members', their shoelace sums add up to its area2"""
    gs, _ = pair("rings")
    ctx = maps.Context(gs).load()
    dctx, ov = overlay_of(ctx, None)
    try:
        om = ov.OutputMap(how="union", by="pair", drop_degenerate=True, merge=True)
        r = om.Rings(ov.h, skip_face0=True)
        p = r.Polygons(ov.h)
        assert p.n_holes == 47 and p.n_orphans == 0 and p.n_face0 == 0 and p.n_members == p.n_polygons + p.n_holes
        polys = p.polygons(r)
        assert len(polys) == p.n_polygons and sum(len(holes) for _, _, _, holes in polys) == 47
        for face, a2, shell, holes in polys:
            assert face >= 1 and a2 > 0 and P.shoelace(shell) > 0 and all(P.shoelace(hh) <= 0 for hh in holes)
            assert P.shoelace(shell) + sum(P.shoelace(hh) for hh in holes) == a2
        unscaled = p.polygons(r, ctx.scaling)
        assert unscaled[0][1] == polys[0][1] and np.allclose(unscaled[0][2], ctx.scaling.unscale(polys[0][2]))
        with pytest.raises(RuntimeError):
            om.Rings(ov.h, points=False).Polygons(ov.h)
        p.free()
        r.free()
        om.free()
    finally:
        dctx.close()


def test_lattice_clip_equals_the_host_twin():
    gs, _ = pair("lattice")
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    try:
        om = raw_map(ov, ("intersection", "map0"), 0)
        rg, got = polygons_of_rings(ov.h, om.Rings(ov.h))
        om.free()
    finally:
        dctx.close()
    rc, want, _ = twin_polygons(twin_lib(), *args_of(rg))
    assert rc == 0 and rg["counts"]["n_rings"] == 10
    PR.assert_same_polygons(got, want)
    assert got["counts"]["n_orphans"] == 0


# ---- the contract of the call ------------------------------------------------------------------------------------------
def test_each_capacity_one_short_overflows_and_writes_nothing_beyond(handle):
    rg, want = hand_case("multi-part")
    true = (want["counts"]["n_polygons"], want["counts"]["n_members"])
    n = len(rg["rings"])
    r = upload_rings(handle, *args_of(rg))
    args = (r.rings, r.n_rings, r.ring_row, r.ring_xy, r.n_points, 0)
    canary = np.full(4, 0x5A5A5A5A, np.uint32)
    try:
        parent = handle.alloc(4 * n)
        with pytest.raises(_capi.PolygonsOverflow) as e:  # the sizing call; parent is written in full all the same
            handle.rings_polygons(*args, (0, 0), parent, None, None, None)
        assert e.value.counts == want["counts"] and e.value.code == _capi.RJ_E_OVERFLOW
        assert np.array_equal(parent.to_host(np.uint32, n), want["parent"])
        parent.free()
        for short in range(2):
            pc, mc = (v - (1 if i == short else 0) for i, v in enumerate(true))
            bufs = []
            for nbytes in (4 * n, 32 * pc, 4 * (pc + 1), 4 * mc):
                b = handle.alloc(nbytes + 16)
                handle._check(_capi.load().rj_memcpy_h2d(handle.h, b.ptr + nbytes, canary.ctypes.data, 16))
                bufs.append((b, nbytes))
            with pytest.raises(_capi.PolygonsOverflow) as e:
                handle.rings_polygons(*args, (pc, mc), *[b for b, _ in bufs])
            assert e.value.counts == want["counts"], short
            for b, nbytes in bufs:
                assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary), short
            assert np.array_equal(bufs[0][0].to_host(np.uint32, n), want["parent"])
            assert np.array_equal(bufs[1][0].to_host(_capi.POLYGON_DTYPE, pc), want["polygons"][:pc])
            assert np.array_equal(bufs[3][0].to_host(np.uint32, mc), want["poly_ring"][:mc])
            for b, _ in bufs:
                b.free()
            with pytest.raises(_capi.PolygonsOverflow):
                r.Polygons(handle, capacities=(pc, mc))
        exact = r.Polygons(handle, capacities=true)
        PR.assert_same_polygons(exact.to_host(), want)
        exact.free()
    finally:
        r.free()


def test_no_rings_flags_and_malformed_input(handle):
    first = handle.alloc(4).from_host(np.array([7], np.uint32))
    c = handle.rings_polygons(None, 0, None, None, 0, 0, (0, 0), None, None, first, None)
    assert c == dict.fromkeys(PR.COUNTS, 0) and first.to_host(np.uint32, 1).tolist() == [0]
    first.free()
    for what, rings, row, xy, flags in bad_inputs():
        r = upload_rings(handle, rings, row, xy)
        try:
            with pytest.raises(_capi.RayJoinError) as e:
                handle.rings_polygons(r.rings, r.n_rings, r.ring_row, r.ring_xy, r.n_points, flags, (0, 0), None, None, None, None)
            assert e.value.code == _capi.RJ_E_INVALID and not isinstance(e.value, _capi.PolygonsOverflow), what
        finally:
            r.free()
    rg, want = hand_case("hole")  # the handle still works
    PR.assert_same_polygons(device_polygons(handle, *args_of(rg)), want)


# ---- grid-stride loops ------------------------------------------------------------------------------------------------
def device_rings_and_polygons(h, m):
    dm = DeviceMap(h, m)
    try:
        return polygons_of_rings(h, ops.face_rings(h, *dm.args()))
    finally:
        dm.free()


def test_more_rings_than_one_grid_covers_equal_the_host_twin(handle):
    """P.triangle_field with a face of its own per chain: 1 060 000 rings, more than the 1 048 576 threads of the largest
    grid -- every loop over the rings makes a second trip.  Every third chain is digitised clockwise: an orphan."""
    xy, row, _, _ = P.triangle_field(FIELD)
    m = (xy, row, np.arange(1, FIELD + 1, dtype=np.int32), np.zeros(FIELD, np.int32))
    rg, got = device_rings_and_polygons(handle, m)
    assert rg["counts"]["n_rings"] == 2 * FIELD > 4096 * 256
    rc, want, _ = twin_polygons(twin_lib(), *args_of(rg))
    assert rc == 0
    PR.assert_same_polygons(got, want)
    back = FIELD // 3
    assert got["counts"] == dict(n_polygons=FIELD - back, n_members=FIELD - back, n_holes=0, n_orphans=back, n_face0=FIELD)


def test_one_face_with_more_than_65536_holes_equals_the_host_twin(handle):
    m = PC.hole_field()
    rg, got = device_rings_and_polygons(handle, m)
    n = len(m[2]) - 1
    rc, want, stats = twin_polygons(twin_lib(), *args_of(rg))
    assert rc == 0 and n > 1 << 16
    PR.assert_same_polygons(got, want)
    assert got["counts"] == dict(n_polygons=n + 1, n_members=2 * n + 1, n_holes=n, n_orphans=0, n_face0=1)
    assert int(got["polygons"]["n_holes"][0]) == n and (got["parent"][1:n + 2] == 1).all() and stats["shift"] == 16


def test_hole_field_of_270400_holes_makes_a_second_trip_of_the_lane_groups(handle):
    """PC.hole_field(520): 540 802 rings, 270 400 of them holes with a ring above, more than the 262 144 rings that one grid
    of k_pg_above (8192 blocks of 256 threads, 8 lanes to a ring) covers.  The device's rings are the rings twin's, so the
    polygons twin's answer of tests/test_polygons.py serves; and the construction: every hole's parent is ring 1."""
    m, rg_twin, want, stats = big_field_case()
    rg, got = device_rings_and_polygons(handle, m)
    D.assert_same_rings(rg, rg_twin)
    n = BIG_FIELD_SIDE * BIG_FIELD_SIDE
    assert rg["counts"]["n_rings"] == 2 * n + 2 > 2 * (8192 * 256 // 8)
    PR.assert_same_polygons(got, want)
    check_hole_field(rg["rings"], got, stats, n)


# ---- raw ring sets: the answers of tests/test_polygons.py ------------------------------------------------------------------
def check_soup(h, kind, *args):
    rings, want = soup_case(kind, *args)[::2]
    got = device_polygons(h, *rings)
    PR.assert_same_polygons(got, want, (kind,) + args)
    return got


@pytest.mark.parametrize("seed", SLIVER_SEEDS)
def test_sliver_soups_equal_the_definition(handle, seed):
    """products near 2^90 that differ by at most 5, heights that differ by 2^-45, falling edges: candidate(), floor_div()
    and lower() on the device, the winners of 8 lanes reduced over buckets of about 490 near-ties"""
    check_soup(handle, "sliver", seed)


@pytest.mark.parametrize("seed", FAN_SEEDS)
def test_slope_fans_equal_the_definition(handle, seed):
    """equal heights: the slope step and the slot step of lower(), within a lane and across lanes"""
    got = check_soup(handle, "fan", seed)
    for g in soup_case("fan", seed)[1]["groups"]:
        assert int(got["parent"][g["hole"]]) == g["above"], seed


def test_top_sweep_equals_the_definition(handle):
    """k_pg_tops: rings shorter than, as long as and longer than the lane group, the top at every lane position"""
    got = check_soup(handle, "tops")
    assert np.array_equal(got["parent"], soup_case("tops")[1]["parent"])


def test_long_rings_equal_the_definition(handle):
    got = check_soup(handle, "long")
    assert got["parent"].tolist() == [1, 1, 2, 3, 4]


@pytest.mark.parametrize("faces", PS.DEGENERATE_FACES)
def test_degenerate_records_equal_the_definition(handle, faces):
    """walks that end at an orphan after up to 39 steps (a state that has ended, copied by jump_round), rings without
    points as the first and the last record, faces outside [0, 2^31) in the entry keys and the ring order"""
    got = check_soup(handle, "degenerate", faces)
    assert got["counts"] == PS.DEGENERATE_COUNTS


@pytest.mark.parametrize("salt", [0, 1])
def test_carry_field_equals_the_construction(handle, salt):
    """40 000 members: 39 blocks of rocPRIM's scan of the int128 areas (1024 items to a block for a 16-byte type); with
    salt 1 the low words of the prefix carry into the high ones at about half of the shells"""
    got = check_soup(handle, "carry", CARRY_SQUARES, salt)
    assert got["counts"]["n_polygons"] == CARRY_SQUARES and got["counts"]["n_orphans"] == 0


# ---- the rings of fuzzed overlays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [303, 317, 322])
def test_polygons_of_fuzzed_overlays_equal_the_definition(oracle, seed):
    """one pair of tests/test_gpu_overlay_fuzz.py's draw (an integer pair with overlapping chains and two in general
    position): the polygons of the rings of the device's output maps of (intersection, pair) and one more operation"""
    cap, FZ.EDGE_CAP = FZ.EDGE_CAP, FUZZ_EDGE_CAP
    try:
        rng = np.random.default_rng(seed)
        ctx, kind = FZ.draw_pair(rng)
    finally:
        FZ.EDGE_CAP = cap
    use_grid = bool(rng.integers(0, 2))
    gsize = int(rng.choice(FZ.GSIZES))
    drawn = [None, OPS[int(rng.integers(1, len(OPS)))]]
    om = H.oracle_maps(oracle, ctx)
    pairs = oracle.lsi_grid(om[0], om[1], gsize)["eid"] if use_grid else oracle.lsi_brute(om[0], om[1])
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    rings = 0
    try:
        ov = run_overlay(dctx, gsize if use_grid else None, len(pairs))
        for call in drawn:
            for flags in (0, DROP | MERGE):
                omap = raw_map(ov, call, flags)
                rg, got = polygons_of_rings(ov.h, omap.Rings(ov.h))
                omap.free()
                PR.assert_same_polygons(got, PR.polygons_ref(*args_of(rg)), (seed, kind, call, flags))
                rings += rg["counts"]["n_rings"]
                if kind == "float":
                    assert got["counts"]["n_orphans"] == 0, (seed, call, flags)
    finally:
        dctx.close()
    print(seed, kind, rings)
    assert rings > 100 and kind == ("ties" if seed == 303 else "float")


# ---- the command line ---------------------------------------------------------------------------------------------------
def parse_polygons(path):
    """-> [(f0, f1, area2, [ring point counts])]"""
    out = []
    for line in open(path):
        f0, f1, a2, rest = line.split(" ", 3)
        assert rest.startswith("POLYGON ((") and rest.rstrip().endswith("))"), line
        rings = rest.strip()[len("POLYGON (("):-2].split("), (")
        pts = [[tuple(float(v) for v in p.split()) for p in ring.split(", ")] for ring in rings]
        assert all(len(r) >= 2 and r[0] == r[-1] and all(len(p) == 2 for p in r) for r in pts), line
        out.append((int(f0), int(f1), int(a2), [len(r) for r in pts]))
    return out


@pytest.mark.parametrize("extra", [[], ["-how", "union", "-by", "pair", "-merge"]])
def test_polyover_exec_polygons(tmp_path, extra):
    """-polygons on the sample pair: the file parses, and per (f0, f1) its areas are the -face_table's"""
    p0, p1 = os.path.join(GOLDEN, "map0.cdb"), os.path.join(GOLDEN, "map1.cdb")
    out, table = str(tmp_path / "polygons.txt"), str(tmp_path / "table.txt")
    r = subprocess.run([EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-xsect_factor", "1.0", "-polygons", out, "-face_table", table] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Polygons: " in r.stderr, r.stderr
    polys = parse_polygons(out)
    sums = {}
    for f0, f1, a2, _ in polys:
        assert a2 > 0
        sums[(f0, f1)] = sums.get((f0, f1), 0) + a2
    sc = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load().scaling
    k = 0.5 * float(sc.rrx) * float(sc.rry)
    rows = [line.split() for line in open(table)]
    assert len(rows) == len(sums) > 50 and [(int(a), int(b)) for a, b, _ in rows] == sorted(sums)
    assert [float(v) for _, _, v in rows] == [float(sums[key]) * k for key in sorted(sums)]
