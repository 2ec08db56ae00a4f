"""Rings to map on the device (rj_rings_map, ops.rings_map, DeviceRings.Map, DeviceChainMap, polyover_exec -coarse_map)
against the plain-Python definition (tests/ringmap_ref.py), array for array, on the hand cases of tests/ringmap_cases.py;
against the host twin where the Python walk is too slow (loops of 100 003 edges, 70 000 disjoint triangles -- more closed
walks than one trip of a grid covers and more than 2^16 leaders --, more than 2^16 dangling edges on one junction); on the
rings of the device's OWN output maps of the overlay tests' pairs (five calls, drop and merge on and off): no conflicts,
the same rings back, never more chains; the same on the nested pair and all 13 families of tests/overlay_hard_pairs.py
wherever rj_map_rings reports no mixed ring, and the device equal to the definition, conflicts included, on the maps that have
one; end to end: the map installed, indexed and queried, and the face table of a further overlay; overflow with canaries, the sizing call, no rings, every malformed input (each rejected by the input check before
anything is read through it), the faces of ring records read in place.  The CPU side is tests/test_ringmap.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_hard_pairs as H  # noqa: E402
import ringmap_cases as MC  # noqa: E402
import ringmap_ref as MR  # noqa: E402
import rings_ref as D  # noqa: E402
from test_gpu_overlay_map import run_overlay  # noqa: E402
from test_gpu_overlay_merge import CALLS, DROP, MERGE, overlay_of, raw_map  # noqa: E402
from test_overlay_faces import _rect_pair  # noqa: E402
from test_overlay_map import pair  # noqa: E402
from test_ringmap import bad_inputs, canon_np_of, canon_of, hand_case, long_cases, twin_lib, twin_map  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
EXE = os.path.join(ROOT, "rayjoin_amd", "polyover_exec")
FIELD = 70_000    # disjoint triangles: 420 000 half-edges, 140 000 closed walks, 70 000 chains
SPOKES = 70_000   # two-point rings on one hub


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


class DeviceRingSet:
    """a ring set (ring_row, ring_xy, ring_face: int32 labels, or RING_DTYPE records to be read in place) in device buffers"""

    def __init__(self, h, rings):
        row, xy, face = rings
        row, xy, face = np.ascontiguousarray(row, np.uint32), np.ascontiguousarray(xy, np.int64).reshape(-1, 2), np.ascontiguousarray(face)
        self.n_points, self.n_rings, self.stride = len(xy), len(row) - 1, face.dtype.itemsize
        self.bufs = [h.alloc(4 * len(row)).from_host(row), h.alloc(16 * max(1, len(xy))).from_host(xy),
                     h.alloc(max(4, face.nbytes)).from_host(face)]

    def args(self, stride=None):
        row, xy, face = self.bufs
        return (row, xy, self.n_points, face, self.stride if stride is None else stride, self.n_rings)

    def free(self):
        for b in self.bufs:
            b.free()


def host_map(dm):
    m, counts = dm.to_host()
    return dict(xy=m.pts, row_index=m.row_index, left=m.left.astype(np.int32), right=m.right.astype(np.int32), counts=counts)


def device_map(h, rings, dissolve=False):
    ds = DeviceRingSet(h, rings)
    try:
        row, xy, n, face, stride, nr = ds.args()
        dm = ops.rings_map(h, row, xy, n, face, nr, face_stride=stride, dissolve=dissolve)
        got = host_map(dm)
        dm.free()
        return got
    finally:
        ds.free()


# ---- device against the definition, and against the twin ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.HAND))
def test_hand_cases_equal_the_definition(handle, name):
    rings, dissolve, want, ref = hand_case(name)
    got = device_map(handle, rings, dissolve)
    MR.assert_same_map(got, ref, name)
    MR.assert_same_map(got, want, name)


@pytest.mark.parametrize("name", ["ccw", "cw"])
def test_long_loops_equal_the_construction(handle, name):
    """one closed walk of 100 003 half-edges and its twin: 17 doubling steps for the minimum, 17 for the ranking"""
    rings, dissolve, want = long_cases()["loop-%d-%s" % (MC.LONG_LOOP, name)]
    got = device_map(handle, rings, dissolve)
    MR.assert_same_map(got, want, name)
    rc, twin, _ = twin_map(twin_lib(), rings, dissolve)
    assert rc == 0
    MR.assert_same_map(got, twin, name)


def test_triangle_field_equals_the_host_twin(handle):
    """70 000 loops of 3 edges: 210 000 point slots, 420 000 half-edges, 140 000 closed walks -- more leaders than 2^16"""
    rings = MC.triangle_rings(FIELD)
    rc, want, _ = twin_map(twin_lib(), rings)
    assert rc == 0 and want["counts"] == dict(n_chains=FIELD, n_points=4 * FIELD, n_edges=3 * FIELD, n_closed=FIELD, n_zero_edges=0, n_conflicts=0,
                                              n_dissolved=0)
    got = device_map(handle, rings)
    MR.assert_same_map(got, want)
    # closed forms: every chain is a triangle read from its lower left corner upwards; the face lies on the right of that
    # for a counter-clockwise ring, on the left for the clockwise third
    xy = got["xy"].reshape(FIELD, 4, 2)
    assert (xy[:, 0] == xy[:, 3]).all() and (xy[:, 1, 0] == xy[:, 0, 0]).all() and (xy[:, 1, 1] == xy[:, 0, 1] + 6).all()
    assert ((got["left"] == 0) != (got["right"] == 0)).all() and int((got["left"] != 0).sum()) == len(range(2, FIELD, 3))


def test_one_junction_of_70000_dangling_edges_equals_the_host_twin(handle):
    """more than 2^16 rings that share one point: every half-edge ends at the hub or at a tip, 70 000 chains of one edge"""
    rings = MC.junction_rings(SPOKES)
    rc, want, _ = twin_map(twin_lib(), rings)
    assert rc == 0 and want["counts"]["n_chains"] == SPOKES and want["counts"]["n_edges"] == SPOKES and want["counts"]["n_conflicts"] == 0
    got = device_map(handle, rings)
    MR.assert_same_map(got, want)
    assert (got["left"] == got["right"]).all() and sorted(got["left"].tolist()) == list(range(1, SPOKES + 1))
    dissolved = device_map(handle, rings, dissolve=True)
    assert dissolved["counts"] == dict(want["counts"], n_chains=0, n_points=0, n_edges=0, n_dissolved=SPOKES)


# ---- the rings of the device's own output maps ------------------------------------------------------------------------------------
def rings_host(r):
    got = r.to_host()
    return got, canon_of(got)


@pytest.mark.parametrize("name", ["sample", "rings"])
def test_maps_of_own_rings_have_the_same_rings_and_no_more_chains(name):
    """DeviceRings.Map on the rings of the device's own output maps: no conflict, the rings of the new map are the source's
    (canonically), and it has at most the source's chains.  The definition agrees on the smallest of them."""
    gs, _ = pair(name)
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    checked = 0
    try:
        for call in CALLS:
            for flags in (0, DROP, MERGE, DROP | MERGE):
                what = (name, call, flags)
                om = raw_map(ov, call, flags)
                r = om.Rings(ov.h)
                dm = r.Map(ov.h)
                assert dm.counts["n_conflicts"] == 0 and dm.n_chains <= om.n_chains, what
                src, src_canon = rings_host(r)
                r2 = dm.Rings(ov.h)
                assert rings_host(r2)[1] == src_canon, what
                if call is None and flags == 0:
                    ref = MR.rings_map_ref(src["ring_row"], src["ring_xy"], src["rings"]["face"])
                    MR.assert_same_map(host_map(dm), ref, what)
                    checked += 1
                for b in (r2, dm, r, om):
                    b.free()
    finally:
        dctx.close()
    assert checked == 1


# maps without a mixed ring among the 20 of every family (five calls, drop and merge on and off): a property of the family's
# geometry and labels that rj_map_rings reports, counted before this test was written
UNMIXED = {"nested": 4, "ties-0": 0, "ties-1": 0, "ties-2": 0, "ties-3": 0, "ties_corner": 0, "big_ids": 0, "many_cuts-a": 12, "many_cuts-b": 12,
           "waves-63x65": 0, "waves-64x128": 20, "waves-321x40": 0, "waves-ring1000": 20, "waves-193x64": 0}
REF_SLOTS = 12_000  # ring points up to which the Python definition is run on a map with mixed rings


@pytest.mark.parametrize("name", ["nested"] + H.NAMES)
def test_maps_of_own_rings_on_the_hard_families(name):
    """the nested pair and every family of tests/overlay_hard_pairs.py, the device's own output maps.  The round trip is
    promised for a planar subdivision with consistent labels: on every map for which rj_map_rings reports no mixed ring there
    is no conflict, the same rings come back and there are no more chains.  The other maps have chains that overlap (the
    tie families are random integer chains that cross themselves; the nested pair shares chains between its maps) or labels
    that change along a ring: nothing is promised there but a determined result, and the device equals the definition on
    every one of them that is small enough for the Python walk."""
    assert set(UNMIXED) == {"nested"} | set(H.NAMES)
    ctx = maps.Context(pair("nested")[0]).load() if name == "nested" else H.family(name)[0]
    dctx, ov = overlay_of(ctx, None)
    unmixed = against_ref = conflicts = 0
    try:
        for call in CALLS:
            for flags in (0, DROP, MERGE, DROP | MERGE):
                what = (name, call, flags)
                om = raw_map(ov, call, flags)
                r = om.Rings(ov.h)
                dm = r.Map(ov.h)
                src = r.to_host()
                if r.n_mixed == 0:
                    unmixed += 1
                    assert dm.counts["n_conflicts"] == 0 and dm.n_chains <= om.n_chains, what
                    r2 = dm.Rings(ov.h)
                    assert canon_np_of(r2.to_host()) == canon_np_of(src), what
                    r2.free()
                elif r.n_points <= REF_SLOTS:
                    against_ref += 1
                    conflicts += dm.counts["n_conflicts"] > 0
                    MR.assert_same_map(host_map(dm), MR.rings_map_ref(src["ring_row"], src["ring_xy"], src["rings"]["face"]), what)
                for b in (dm, r, om):
                    b.free()
    finally:
        dctx.close()
    print(name, "unmixed", unmixed, "against the definition", against_ref, "with conflicts", conflicts)
    assert unmixed == UNMIXED[name]
    if name.startswith(("ties", "big_ids")):  # every map of a tie family has conflicts and is held to the definition
        assert against_ref == conflicts == 20


@pytest.fixture(scope="module")
def lattice():
    gs, _ = pair("lattice")
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    yield ov
    dctx.close()


def test_merged_lattice_intersection_gets_strictly_fewer_chains_and_equals_the_twin(lattice):
    """the lattice pair's merged intersection map: merging never joins pieces of different source chains, the rings do"""
    om = raw_map(lattice, None, DROP | MERGE)
    r = om.Rings(lattice.h)
    dm = r.Map(lattice.h)
    try:
        assert dm.counts["n_conflicts"] == 0 and 0 < dm.n_chains < om.n_chains
        src = r.to_host()
        got = host_map(dm)
        rc, want, _ = twin_map(twin_lib(), (src["ring_row"], src["ring_xy"], src["rings"]), stride=D.RING_DTYPE.itemsize)
        assert rc == 0
        MR.assert_same_map(got, want)
        # the same rings back, canonically: faces, areas and the cyclic point sequences of all 154 487 rings
        r2 = dm.Rings(lattice.h)
        back = r2.to_host()
        r2.free()
        assert len(back["rings"]) == len(src["rings"]) > 150000 and canon_np_of(back) == canon_np_of(src)
    finally:
        for b in (dm, r, om):
            b.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _context(scaling, m0, m1):
    ctx = maps.Context([None, None])
    ctx.scaling = scaling
    ctx.set_map(0, m0)
    ctx.set_map(1, m1)
    return ctx


def test_installed_map_answers_point_queries_as_its_source_does():
    """the sample pair's output map (drop, unmerged) and the map of its rings, each installed as map 0 and indexed: the faces
    of 600 query points that lie on no edge of the source are the same"""
    gs, _ = pair("sample")
    ctx = maps.Context(gs).load()
    dctx, ov = overlay_of(ctx, None)
    d2 = ops.DeviceContext(_context(ctx.scaling, None, ctx.maps[1]))
    try:
        om = ov.OutputMap(drop_degenerate=True)
        r = om.Rings(ov.h)
        dm = r.Map(ov.h)
        src = om.to_host()[0]
        seg = src.segments().astype(object)
        rng = np.random.default_rng(5)
        lo, hi = src.pts.min(axis=0), src.pts.max(axis=0)
        pts = np.stack([rng.integers(int(lo[0]), int(hi[0]), 600), rng.integers(int(lo[1]), int(hi[1]), 600)], axis=1).astype(np.int64)
        keep = np.ones(len(pts), bool)
        for k, (px, py) in enumerate(pts.tolist()):  # exact: collinear with an edge and inside its box
            cr = (seg[:, 2] - seg[:, 0]) * (py - seg[:, 1]) - (seg[:, 3] - seg[:, 1]) * (px - seg[:, 0])
            on = (cr == 0) & (np.minimum(seg[:, 0], seg[:, 2]) <= px) & (px <= np.maximum(seg[:, 0], seg[:, 2])) & \
                (np.minimum(seg[:, 1], seg[:, 3]) <= py) & (py <= np.maximum(seg[:, 1], seg[:, 3]))
            keep[k] = not on.any()
        pts = pts[keep]
        assert len(pts) > 550
        d2.LoadToDevice()
        faces = []
        for m in (om, dm):
            d2.InstallMap(0, m)
            d2.BuildIndex(0)
            pip = ops.PIPLBVH(d2)
            pip.Init(len(pts))
            pip.Query(1, pts)
            faces.append(pip.get_face_ids())
        assert np.array_equal(faces[0], faces[1]) and len(set(faces[0].tolist())) > 20
        assert d2.get_map(0).n_chains == dm.n_chains < om.n_chains
        for b in (dm, r, om):
            b.free()
    finally:
        dctx.close()
        d2.close()


def test_face_table_of_a_further_overlay_is_the_same_on_the_rectangle_pair():
    """M = the two-rectangle pair's intersection map, M' the map of its rings (3 chains for 5), B a square with corners on the
    lattice: every cut point of (M, B) and (M', B) is a lattice point, and the two face tables are equal row for row"""
    ctx, U = _rect_pair()
    ctx.scaling = maps.Scaling((0.0, 0.0, 1.0, 1.0))
    sq = np.array([[1, 3], [5, 3], [5, 5], [1, 5], [1, 3]], np.int64) * U
    B = maps.ScaledMap(1, sq, np.array([0, 5], np.uint32), np.array([7], np.int64), np.array([0], np.int64))
    d1 = ops.DeviceContext(ctx).LoadToDevice()
    d2 = ops.DeviceContext(_context(ctx.scaling, None, B))
    try:
        ov = run_overlay(d1)
        om = ov.OutputMap(drop_degenerate=True)
        r = om.Rings(ov.h)
        dm = r.Map(ov.h)
        assert (om.n_chains, dm.n_chains) == (5, 3)
        d2.LoadToDevice()
        tables = []
        for m in (om, dm):
            d2.InstallMap(0, m)
            t = run_overlay(d2).FaceTable()
            tables.append([(int(a), int(b), int(c)) for a, b, c in zip(t["face0"], t["face1"], t["area2"])])
        # [2, 3] x [3, 4] of face 1 and [3, 4] x [3, 4] of face 2 lie in B: U^2 each
        assert tables[0] == tables[1] == [(1, 7, 2 * U * U), (2, 7, 2 * U * U)]
        for b in (dm, r, om):
            b.free()
    finally:
        d1.close()
        d2.close()


# ---- the contract of the call ------------------------------------------------------------------------------------------------------
def test_each_capacity_one_short_overflows_and_writes_nothing_beyond(handle):
    rings, _, want, _ = hand_case("squares-different")
    true = (want["counts"]["n_chains"], want["counts"]["n_points"])
    ds = DeviceRingSet(handle, rings)
    try:
        with pytest.raises(_capi.RingsMapOverflow) as e:  # the sizing call
            handle.rings_map(*ds.args(), 0, (0, 0), None, None, None, None)
        assert e.value.counts == want["counts"] and e.value.code == _capi.RJ_E_OVERFLOW
        canary = np.full(4, 0x5A5A5A5A, np.uint32)
        for short in range(2):
            cc, pc = (v - (1 if i == short else 0) for i, v in enumerate(true))
            bufs = []
            for nbytes in (16 * pc, 4 * (cc + 1), 4 * cc, 4 * cc):
                b = handle.alloc(nbytes + 16)
                handle._check(_capi.load().rj_memcpy_h2d(handle.h, b.ptr + nbytes, canary.ctypes.data, 16))
                bufs.append((b, nbytes))
            with pytest.raises(_capi.RingsMapOverflow) as e:
                handle.rings_map(*ds.args(), 0, (cc, pc), *[b for b, _ in bufs])
            assert e.value.counts == want["counts"], short
            for b, nbytes in bufs:
                assert np.array_equal(b.to_host(np.uint32, nbytes // 4 + 4)[-4:], canary), short
            assert np.array_equal(bufs[0][0].to_host(np.int64, 2 * pc).reshape(-1, 2), want["xy"][:pc]), short
            assert np.array_equal(bufs[2][0].to_host(np.int32, cc), want["left"][:cc]), short
            for b, _ in bufs:
                b.free()
            with pytest.raises(_capi.RingsMapOverflow):
                row, xy, n, face, stride, nr = ds.args()
                ops.rings_map(handle, row, xy, n, face, nr, capacities=(cc, pc))
        row, xy, n, face, stride, nr = ds.args()
        exact = ops.rings_map(handle, row, xy, n, face, nr, capacities=true)
        MR.assert_same_map(host_map(exact), want)
        exact.free()
    finally:
        ds.free()


def test_no_rings_bad_input_and_the_stride(handle):
    # n_rings == 0: no chains, the row's one entry
    row = handle.alloc(4).from_host(np.array([7], np.uint32))
    c = handle.rings_map(None, None, 0, None, 4, 0, 0, (0, 0), None, row, None, None)
    assert c == dict.fromkeys(MR.COUNTS, 0) and row.to_host(np.uint32, 1).tolist() == [0]
    row.free()
    empty = ops.rings_map(handle, None, None, 0, None, 0)
    assert empty.n_chains == 0 and empty.to_host()[0].n_chains == 0
    empty.free()
    # rings without a point: the same; and a rejected input leaves the caller's row alone
    for ring_row, ok in (([0, 0, 0], True), ([1, 0, 0], False)):
        ds = DeviceRingSet(handle, (np.array(ring_row, np.uint32), np.zeros((0, 2), np.int64), np.array([3, 4], np.int32)))
        row = handle.alloc(4).from_host(np.array([7], np.uint32))
        try:
            if ok:
                assert handle.rings_map(*ds.args(), 0, (0, 0), None, row, None, None) == dict.fromkeys(MR.COUNTS, 0)
            else:
                with pytest.raises(_capi.RayJoinError) as e:
                    handle.rings_map(*ds.args(), 0, (0, 0), None, row, None, None)
                assert e.value.code == _capi.RJ_E_INVALID
            assert row.to_host(np.uint32, 1).tolist() == [0 if ok else 7]
        finally:
            row.free()
            ds.free()
    # every malformed input: RJ_E_INVALID, no overflow, nothing read through it
    for what, rings, stride, flags in bad_inputs():
        ds = DeviceRingSet(handle, rings)
        try:
            with pytest.raises(_capi.RayJoinError) as e:
                handle.rings_map(*ds.args(stride), flags, (0, 0), None, None, None, None)
            assert e.value.code == _capi.RJ_E_INVALID and not isinstance(e.value, _capi.RingsMapOverflow), what
        finally:
            ds.free()
    with pytest.raises(_capi.RayJoinError) as e:  # n_points >= 2^31: refused before any array is looked at
        handle.rings_map(1, 1, 1 << 31, 1, 4, 1, 0, (0, 0), None, None, None, None)
    assert e.value.code == _capi.RJ_E_INVALID and "2^31" in str(e.value)
    # the handle still works; stride 4 over a label array and stride 32 over ring records give the same map
    rings, _, want, _ = hand_case("hole")
    records = np.zeros(len(rings[2]), D.RING_DTYPE)
    records["face"], records["leader"], records["area2_lo"] = rings[2], 0x7FFFFFFF, 0xFFFFFFFFFFFFFFFF
    MR.assert_same_map(device_map(handle, rings), want)
    MR.assert_same_map(device_map(handle, (rings[0], rings[1], records)), want)


def test_polyover_exec_coarse_map(tmp_path):
    """-coarse_map on the sample pair: the file parses and holds, in fewer chains, the rings of the chains of -output_map's
    file that have two points or more (its degenerate pieces are left out here as -coarse_map leaves them out); without the
    flag nothing of it shows"""
    p0, p1 = os.path.join(SAMPLE, "map0.cdb"), os.path.join(SAMPLE, "map1.cdb")
    omp, cmp_ = str(tmp_path / "om.cdb"), str(tmp_path / "cm.cdb")
    base = [EXE, "-poly1", p0, "-poly2", p1, "-mode", "lbvh", "-xsect_factor", "1.0", "-output_map", omp]
    r = subprocess.run(base + ["-coarse_map", cmp_], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert " - Compute coarse map: " in r.stderr and " - Write coarse map: " in r.stderr and "Coarse map: " in r.stderr
    ctx = maps.Context([maps.read_cdb(p0), maps.read_cdb(p1)]).load()

    def rings_of_file(path):
        """-> (chains with two points or more, the canonical rings of these chains)"""
        g = maps.read_cdb(path)
        xy = ctx.scaling.scale(g.points)  # ("%.6f" of the unscaled points: equal points of the device map stay equal in the file)
        row = g.row_index.astype(np.int64)
        keep = np.flatnonzero(np.diff(row) >= 2)  # (-output_map's file has the degenerate pieces, -coarse_map's source not)
        pts = np.concatenate([xy[row[c]:row[c + 1]] for c in keep])
        new_row = np.concatenate([[0], np.cumsum(np.diff(row)[keep])]).astype(np.uint32)
        rg = D.rings_ref(pts, new_row, g.chains[keep, 3].astype(np.int32), g.chains[keep, 4].astype(np.int32))
        return len(keep), canon_of(rg)

    n_om, rings_om = rings_of_file(omp)
    n_cm, rings_cm = rings_of_file(cmp_)
    assert rings_cm == rings_om and 0 < maps.read_cdb(cmp_).n_chains == n_cm < n_om and len(rings_cm) > 20
    r2 = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "coarse" not in r2.stderr.lower()
