"""Who owns the device buffers of the Python layer, on the CPU: the real rayjoin_amd.ops functions driven by a fake handle
whose alloc returns recording buffers and whose library calls are scripted, and the counted call of _capi.Handle driven
by a stub library.  Neither the library nor a GPU is needed.

Every sized site (a sizing call with zero capacities, the allocation of the outputs, the call itself) is checked for
  (a) the capacities and the byte sizes that the second call receives -- written out here as literals from the formulas;
  (b) a failing call: every allocated buffer freed exactly once, the exception unchanged;
  (c) the same for an exception that is no RayJoinError and for a failing k-th alloc, for every k -- this is the behaviour
      that the buffer owner (ops._Owned) added: before it, such buffers waited for the garbage collector;
  (d) success: nothing freed but the temporaries, the result holds the outputs, its free() frees each once, a second
      free() nothing more;
  (e) staging buffers freed on success and failure alike, the caller's arrays never."""
from types import SimpleNamespace

import numpy as np
import pytest

from rayjoin_amd import _capi, ops


class FakeBuffer:
    """what Handle.alloc returns, recording: like DeviceBuffer, only the first free() releases"""

    def __init__(self, nbytes=0):
        self.nbytes, self.live, self.frees, self.free_calls, self.copies = int(nbytes), True, 0, 0, []

    def free(self):
        self.free_calls += 1
        if self.live:
            self.live = False
            self.frees += 1

    def from_host(self, arr):
        self.copies.append(("host", np.asarray(arr).nbytes))
        return self

    def from_device(self, src, nbytes):
        self.copies.append(("device", src, int(nbytes)))
        return self

    def to_host(self, dtype, count=None):
        return np.zeros(int(count), dtype)


class FakeHandle:
    """alloc records its buffers (the fail_alloc-th raises); every other method pops its next scripted outcome and returns
    or raises it, recording (name, args, kw)"""

    def __init__(self, script, fail_alloc=None):
        self.script, self.fail_alloc, self.bufs, self.calls = {k: list(v) for k, v in script.items()}, fail_alloc, [], []
        self.alloc_error = _capi.RayJoinError(_capi.RJ_E_NOMEM, "no memory")

    def alloc(self, nbytes):
        if self.fail_alloc == len(self.bufs):
            raise self.alloc_error
        self.bufs.append(FakeBuffer(nbytes))
        return self.bufs[-1]

    def __getattr__(self, name):
        if name not in self.script:
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append((name, args, kw))
            outcome = self.script[name].pop(0)
            if isinstance(outcome, BaseException):
                raise outcome
            return outcome
        return call

    def last(self, name):
        return [c for c in self.calls if c[0] == name][-1][1:]


def counts(names, **kw):
    return dict(dict.fromkeys(names, 0), **kw)


def inputs():
    """the caller's device arrays: never to be freed by the code under test"""
    return SimpleNamespace(**{k: FakeBuffer() for k in ("xy", "row", "left", "right", "a", "b", "c", "d", "e")})


def overlay(h, i):
    ov = object.__new__(ops.MapOverlay)
    ov.h, ov.located, ov.xsects, ov.faces, ov.n_xsects = h, [True, True], [i.a, i.b], [i.c, i.d], 5
    return ov


def device_rings(i):
    return ops.DeviceRings(i.a, i.b, i.c, i.d, i.e, counts(_capi.RINGS_COUNTS, n_rings=3, n_halves=5, n_points=7))


class Site:
    """One sized entry point.  run(h, i) makes the call; `method` is the handle's call it sizes (`sized`: the counts of the
    sizing call, None where there is none) and `ok` what the call returns; `pre` scripts the other calls on the way; allocs
    lists (nbytes, "out" | "tmp") in allocation order; holds names the result's attribute of every "out" buffer; caps /
    outs pick the capacities and the output arrays out of (args, kw) of the last call, want_caps / want_outs are their
    literals (the byte size of every array, None where none goes)."""

    def __init__(self, name, run, method, overflow, sized, ok, allocs, holds, caps, want_caps, outs, want_outs, pre=None):
        self.__dict__.update(locals())

    def script(self, final, sizing="raises"):
        s = {k: list(v) for k, v in (self.pre or {}).items()}
        first = [] if self.sized is None else [self.overflow("too small", self.sized) if sizing == "raises" else self.sized]
        s[self.method] = s.get(self.method, []) + first + [final]
        return s


NODE_OK = counts(_capi.NODE_COUNTS, n_points=13, n_edges=11)
SNAP_OK = counts(_capi.SNAP_COUNTS, n_points=13, n_edges=11)
CROSS3 = counts(_capi.CROSSINGS_COUNTS, n_found=3, n_touch=3)
RINGS_OK = counts(_capi.RINGS_COUNTS, n_rings=3, n_halves=5, n_points=7)
POLY_OK = counts(_capi.POLYGONS_COUNTS, n_polygons=2, n_members=3)
RMAP_OK = counts(_capi.RINGS_MAP_COUNTS, n_chains=3, n_points=11)
ELIM_OK = counts(_capi.ELIMINATE_COUNTS, n_faces=4, n_chains=3, n_points=11)
DISS_OK = counts(_capi.DISSOLVE_COUNTS, n_classes=2, n_chains=3, n_points=11)
NB_OK = counts(_capi.NEIGHBOURS_COUNTS, n_faces=3, n_entries=5)
FP_OK = counts(_capi.FACE_POINTS_COUNTS, n_faces=3, n_members=7)
FACES_OK = counts(_capi.MAP_FACES_COUNTS, n_faces=3, n_rings=3)

SITES = [
    # chains 3, points 11, faces 2: xy 16 * 11, row_index 4 * (3 + 1), left / right 4 * 3, face_pairs 8 * 2, origin 4 * 3
    Site("OutputMap", lambda h, i: overlay(h, i).OutputMap(drop_degenerate=True), "overlay_map", _capi.MapOverflow, (3, 11, 2), (3, 11, 2),
         [(176, "out"), (16, "out"), (12, "out"), (12, "out"), (16, "out"), (12, "out")], ("xy", "row_index", "left", "right", "face_pairs", "origin"),
         lambda a, kw: a[6], (3, 11, 2), lambda a, kw: a[7:13], [176, 16, 12, 12, 16, 12]),
    # 5 records of 16 bytes; the records come back on the host, so the buffer is a temporary
    Site("map_crossings", lambda h, i: ops.map_crossings(h, i.xy, 9, i.row, 2), "map_crossings", _capi.CrossingsOverflow,
         counts(_capi.CROSSINGS_COUNTS, n_found=5), counts(_capi.CROSSINGS_COUNTS, n_found=5), [(80, "tmp")], None,
         lambda a, kw: a[4], 5, lambda a, kw: a[5:6], [80]),
    # 5 points: xy 16 * 5, row_index 4 * (2 + 1), origin 4 * 5
    Site("map_simplify", lambda h, i: ops.map_simplify(h, i.xy, 9, i.row, 2, 10, origin=True), "map_simplify", _capi.SimplifyOverflow,
         counts(_capi.SIMPLIFY_COUNTS, n_points=5), counts(_capi.SIMPLIFY_COUNTS, n_points=5), [(80, "out"), (12, "out"), (20, "out")],
         ("xy", "row_index", "origin"), lambda a, kw: a[5], 5, lambda a, kw: a[6:9], [80, 12, 20]),
    # 3 records of 16 bytes stay on the device for the call; 13 points: xy 16 * 13, row_index 4 * (2 + 1), edge_origin 4 * 13
    Site("map_node", lambda h, i: ops.map_node(h, i.xy, 9, i.row, 2, edge_origin=True), "map_node", _capi.NodeOverflow, NODE_OK, NODE_OK,
         [(48, "tmp"), (208, "out"), (12, "out"), (52, "out")], ("xy", "row_index", "edge_origin"),
         lambda a, kw: a[7], 13, lambda a, kw: a[8:11], [208, 12, 52], pre=dict(map_crossings=[CROSS3, CROSS3])),
    Site("map_snap", lambda h, i: ops.map_snap(h, i.xy, 9, i.row, 2, edge_origin=True), "map_snap", _capi.SnapOverflow, SNAP_OK, SNAP_OK,
         [(48, "tmp"), (208, "out"), (12, "out"), (52, "out")], ("xy", "row_index", "edge_origin"),
         lambda a, kw: a[7], 13, lambda a, kw: a[8:11], [208, 12, 52], pre=dict(map_crossings=[CROSS3, CROSS3])),
    # rings 3, half-chains 5, points 7: rings 32 * 3, ring_first 4 * (3 + 1), ring_half 4 * 5, ring_row 4 * (3 + 1), ring_xy 16 * 7
    Site("face_rings", lambda h, i: ops.face_rings(h, i.xy, 9, i.row, i.left, i.right, 2), "map_rings", _capi.RingsOverflow, RINGS_OK, RINGS_OK,
         [(96, "out"), (16, "out"), (20, "out"), (16, "out"), (112, "out")], ("rings", "ring_first", "ring_half", "ring_row", "ring_xy"),
         lambda a, kw: a[7], (3, 5, 7), lambda a, kw: a[8:13], [96, 16, 20, 16, 112]),
    # of 3 rings, polygons 2, members 3: parent 4 * 3, polygons 32 * 2, poly_first 4 * (2 + 1), poly_ring 4 * 3
    Site("Polygons", lambda h, i: device_rings(i).Polygons(h), "rings_polygons", _capi.PolygonsOverflow, POLY_OK, POLY_OK,
         [(12, "out"), (64, "out"), (12, "out"), (12, "out")], ("parent", "polygons_", "poly_first", "poly_ring"),
         lambda a, kw: a[6], (2, 3), lambda a, kw: a[7:11], [12, 64, 12, 12]),
    # chains 3, points 11: xy 16 * 11, row_index 4 * (3 + 1), left / right 4 * 3
    Site("rings_map", lambda h, i: ops.rings_map(h, i.a, i.b, 7, i.c, 3), "rings_map", _capi.RingsMapOverflow, RMAP_OK, RMAP_OK,
         [(176, "out"), (16, "out"), (12, "out"), (12, "out")], ("xy", "row_index", "left", "right"),
         lambda a, kw: a[7], (3, 11), lambda a, kw: a[8:12], [176, 16, 12, 12]),
    # faces 4, chains 3, points 11: as rings_map, then origin 4 * 3 and the records 32 * 4; the call takes left, right, xy, row_index
    Site("map_eliminate", lambda h, i: ops.map_eliminate(h, i.xy, 9, i.row, i.left, i.right, 2, 5, faces=True), "map_eliminate",
         _capi.EliminateOverflow, ELIM_OK, ELIM_OK, [(176, "out"), (16, "out"), (12, "out"), (12, "out"), (12, "out"), (128, "out")],
         ("xy", "row_index", "left", "right", "origin", "faces"), lambda a, kw: a[7], (4, 3, 11), lambda a, kw: a[8:14], [12, 12, 176, 16, 12, 128]),
    # the host table of 3 classes is staged (4 * 3); classes 2, chains 3, points 11 of 2 input chains: as rings_map, then origin 4 * 3,
    # chain_out 4 * 2, the records 24 * 2; the call takes left, right, xy, row_index, origin, chain_out, records
    Site("map_dissolve", lambda h, i: ops.map_dissolve(h, i.xy, 9, i.row, i.left, i.right, 2, classes=np.array([0, 1, 1]), records=True, origin=True),
         "map_dissolve", _capi.DissolveOverflow, DISS_OK, DISS_OK,
         [(12, "tmp"), (176, "out"), (16, "out"), (12, "out"), (12, "out"), (12, "out"), (8, "out"), (48, "out")],
         ("xy", "row_index", "left", "right", "origin", "chain_out", "classes"), lambda a, kw: a[8], (2, 3, 11), lambda a, kw: a[9:16],
         [12, 12, 176, 16, 12, 8, 48]),
    # faces 3, entries 5: the records 64 * 3, offsets 8 * (3 + 1), entries 32 * 5
    Site("map_neighbours", lambda h, i: ops.map_neighbours(h, i.xy, 9, i.row, i.left, i.right, 2, vertex=True), "map_neighbours",
         _capi.NeighboursOverflow, NB_OK, NB_OK, [(192, "out"), (32, "out"), (160, "out")], ("faces", "offsets", "entries"),
         lambda a, kw: a[6], (3, 5), lambda a, kw: a[7:10], [192, 32, 160]),
    # faces 3, members 7: the records 48 * 3, offsets 8 * (3 + 1), members 4 * 7
    Site("face_points", lambda h, i: ops.face_points(h, i.a, 9, members=True), "face_points", _capi.FacePointsOverflow, FP_OK, FP_OK,
         [(144, "out"), (32, "out"), (28, "out")], ("faces", "offsets", "members"),
         lambda a, kw: a[2], (3, 7), lambda a, kw: [kw.get("faces_dev"), kw.get("offsets_dev"), kw.get("members_dev")], [144, 32, 28]),
    # one call, no sizing: copies xy 16 * 9 and row_index 4 * (2 + 1), left / right 4 * 2, room for 2 * 2 records of 32 bytes until
    # the call returns, then the 3 records 32 * 3
    Site("map_faces", lambda h, i: ops.map_faces(h, i.xy, 9, i.row, 2), "map_faces", _capi.FacesOverflow, None, FACES_OK,
         [(144, "out"), (12, "out"), (8, "out"), (8, "out"), (128, "tmp"), (96, "out")], ("xy", "row_index", "left", "right", None, "faces"),
         lambda a, kw: a[7], 4, lambda a, kw: list(a[:1]) + list(a[2:3]) + list(a[4:7]), [144, 12, 8, 8, 128]),
]
BY_NAME = {s.name: s for s in SITES}
site_param = pytest.mark.parametrize("site", SITES, ids=[s.name for s in SITES])


def assert_untouched(i):
    assert all(b.free_calls == 0 for b in vars(i).values()), "a caller's array was freed"


@site_param
@pytest.mark.parametrize("sizing", ["raises", "returns"])
def test_second_call_gets_the_sized_buffers(site, sizing):
    """(a): the sizing call runs once with zero capacities; the call after it gets the capacities of its counts and arrays
    of the sizes the formulas give, whether the sizing call raised its overflow class or returned"""
    h, i = FakeHandle(site.script(site.ok, sizing)), inputs()
    site.run(h, i)
    main = [c for c in h.calls if c[0] == site.method]
    assert len(main) == (1 if site.sized is None else 2) and not h.script[site.method]
    if site.sized is not None:
        zero = site.caps(*main[0][1:])
        assert zero == (0 if isinstance(site.want_caps, int) else (0,) * len(site.want_caps))
        assert all(b is None for b in site.outs(*main[0][1:]))
    args, kw = h.last(site.method)
    assert site.caps(args, kw) == site.want_caps
    assert [b.nbytes for b in site.outs(args, kw)] == site.want_outs
    assert [b.nbytes for b in h.bufs] == [n for n, _ in site.allocs]
    assert_untouched(i)


@site_param
@pytest.mark.parametrize("error", [_capi.RayJoinError(_capi.RJ_E_HIP, "the call failed"), RuntimeError("not the library's")],
                         ids=["RayJoinError", "RuntimeError"])
def test_failing_call_frees_every_buffer_once(site, error):
    """(b) and, for the RuntimeError, (c): the buffers of a failed call are freed at once, each once, whatever was raised --
    for anything but a RayJoinError that is new with the buffer owner"""
    h, i = FakeHandle(site.script(error)), inputs()
    with pytest.raises(type(error)) as caught:
        site.run(h, i)
    assert caught.value is error
    before_the_call = len(site.allocs) - (1 if site.name == "map_faces" else 0)  # (its records are allocated behind the call)
    assert len(h.bufs) == before_the_call and all(b.free_calls == 1 for b in h.bufs)
    assert_untouched(i)


@site_param
def test_failing_alloc_frees_the_buffers_before_it(site):
    """(c): the k-th alloc raises, for every k -- the k buffers before it are freed at once, each once (new with the buffer
    owner: a list literal that failed half way left them to the garbage collector)"""
    for k in range(len(site.allocs)):
        h, i = FakeHandle(site.script(site.ok), fail_alloc=k), inputs()
        with pytest.raises(_capi.RayJoinError) as caught:
            site.run(h, i)
        assert caught.value is h.alloc_error
        assert len(h.bufs) == k and all(b.free_calls == 1 for b in h.bufs), k
        assert_untouched(i)


@site_param
def test_success_hands_the_outputs_to_the_result(site):
    """(d): on success only the temporaries are freed, the result holds every output, its free() frees each exactly once
    and a second free() nothing more"""
    h, i = FakeHandle(site.script(site.ok)), inputs()
    res = site.run(h, i)
    kinds = [kind for _, kind in site.allocs]
    assert [b.free_calls for b in h.bufs] == [1 if kind == "tmp" else 0 for kind in kinds]
    if site.holds is not None:
        outs = [b for b, kind in zip(h.bufs, kinds) if kind == "out"]
        assert [getattr(res, name) for name in site.holds if name is not None] == outs
        res.free()
        assert all(b.frees == 1 and b.free_calls == 1 for b in h.bufs)
        res.free()
        assert all(b.frees == 1 for b in h.bufs)
    assert_untouched(i)


def test_special_cases_of_the_sized_sites():
    """what the sites keep for themselves: face_points without records or members allocates nothing and takes the counts
    of its second call raised or returned; map_eliminate without drop copies xy / row_index and passes no map arrays; an
    empty map gets a one-entry row_index from the host"""
    over = _capi.FacePointsOverflow("too small", FP_OK)
    for second in (over, FP_OK):
        h, i = FakeHandle(dict(face_points=[over, second])), inputs()
        res = ops.face_points(h, i.a, 9, records=False)
        assert not h.bufs and res.counts == FP_OK and len(h.calls) == 2 and h.last("face_points")[0][2] == (0, 0)
        assert (res.faces, res.offsets, res.members) == (None, None, None)

    h, i = FakeHandle(dict(map_eliminate=[_capi.EliminateOverflow("too small", ELIM_OK), ELIM_OK])), inputs()
    res = ops.map_eliminate(h, i.xy, 9, i.row, i.left, i.right, 2, 5, drop=False)
    args, kw = h.last("map_eliminate")
    assert [b.nbytes for b in h.bufs] == [176, 16, 12, 12] and args[7] == (0, 3, 11) and kw == dict(flags=0)
    assert args[8:] == (h.bufs[2], h.bufs[3], None, None, None, None)
    assert h.bufs[0].copies == [("device", i.xy, 16 * 9)] and h.bufs[1].copies == [("device", i.row, 4 * 3)]
    assert res.origin is None and res.faces is None

    empty = counts(_capi.ELIMINATE_COUNTS)
    h, i = FakeHandle(dict(map_eliminate=[empty, empty])), inputs()
    ops.map_eliminate(h, i.xy, 0, i.row, i.left, i.right, 0, 5)
    assert [b.nbytes for b in h.bufs] == [16, 4, 4, 4, 4] and h.bufs[1].copies == [("host", 4)]
    h, i = FakeHandle(dict(map_faces=[counts(_capi.MAP_FACES_COUNTS)])), inputs()
    ops.map_faces(h, i.xy, 0, i.row, 0, records=False)
    assert [b.nbytes for b in h.bufs] == [16, 4, 4, 4] and h.bufs[1].copies == [("host", 4)]


# (e) staging: what a call uploads for its own use is freed on success and on failure alike

HOST_MAP = SimpleNamespace(pts=np.zeros((9, 2), np.int64), row_index=np.array([0, 4, 9], np.uint32), left=np.zeros(2, np.int64),
                           right=np.ones(2, np.int64), n_points=9, n_chains=2)
RING_ROW, RING_XY = np.array([0, 3, 6], np.uint32), np.arange(12, dtype=np.int64).reshape(6, 2)  # closed: 8 points, 2 chains
CLEAN = counts(_capi.CROSSINGS_COUNTS)


def device_context(h):
    dctx = object.__new__(ops.DeviceContext)
    dctx.handle, dctx.installed, dctx.ctx = h, [None, None], SimpleNamespace(get_map=lambda im: HOST_MAP)
    return dctx


def query(cls, *init, **kw):
    """run(h): an operator of class cls over 3 host points"""
    def run(h):
        q = cls(SimpleNamespace(handle=h))
        q.Init(*init)
        return q.Query(1, np.zeros((3, 2), np.int64), **kw)
    return run


# name -> (run(h), the failing method and its script on success, the sizes of the staging buffers, the number of buffers a success keeps)
STAGED = {
    # the host map: xy 16 * 9, row_index 4 * (2 + 1), left / right 4 * 2
    "DeviceContext.Rings": (lambda h: device_context(h).Rings(0), dict(map_rings=[RINGS_OK, RINGS_OK]), [144, 12, 8, 8], 5),
    "DeviceContext.Crossings": (lambda h: device_context(h).Crossings(0), dict(map_crossings=[CROSS3, CROSS3]), [144, 12, 48], 0),
    # the closed rings: xy 16 * 8, row_index 4 * (2 + 1)
    "node_rings": (lambda h: ops.node_rings(h, RING_ROW, RING_XY), dict(map_crossings=[CLEAN], map_node=[NODE_OK, NODE_OK]), [128, 12], 2),
    "snap_rings": (lambda h: ops.snap_rings(h, RING_ROW, RING_XY), dict(map_crossings=[CLEAN], map_snap=[SNAP_OK, SNAP_OK]), [128, 12], 2),
    # 3 host records of 16 bytes
    "map_node(records=)": (lambda h: ops.map_node(h, FakeBuffer(), 9, FakeBuffer(), 2, records=np.zeros(3, _capi.CROSSING_DTYPE)),
                           dict(map_node=[NODE_OK, NODE_OK]), [48], 2),
    "map_snap(records=)": (lambda h: ops.map_snap(h, FakeBuffer(), 9, FakeBuffer(), 2, records=np.zeros(3, _capi.CROSSING_DTYPE)),
                           dict(map_snap=[SNAP_OK, SNAP_OK]), [48], 2),
    # 3 points of 16 bytes, behind the operator's own buffers
    "PIPLBVH.Query": (query(ops.PIPLBVH, 5), dict(pip_query=[None]), [48], 2),
    "PIPGrid.Query": (query(ops.PIPGrid, 5), dict(pip_query_grid=[None]), [48], 2),
    "NearestLBVH.Query": (query(ops.NearestLBVH, 5), dict(nearest_query=[None]), [48], 3),
    "WithinLBVH.Query": (query(ops.WithinLBVH, 5, 4, max_dist=7), dict(within_query=[counts(_capi.WITHIN_COUNTS, n_pairs=2)]), [48], 4),
}


@pytest.mark.parametrize("name", sorted(STAGED))
@pytest.mark.parametrize("error", [None, _capi.RayJoinError(_capi.RJ_E_HIP, "the call failed"), RuntimeError("not the library's")],
                         ids=["success", "RayJoinError", "RuntimeError"])
def test_staging_is_freed_either_way(name, error):
    """(e): the temporaries of a call -- a host map, closed rings, host records, query points -- are freed exactly once when
    the last library call succeeds and when it raises; the result's buffers stay on success and go on failure"""
    run, script, staged, kept = STAGED[name]
    script = {k: list(v) for k, v in script.items()}
    if error is not None:
        last = list(script)[-1]
        script[last][-1] = error
    h = FakeHandle(script)
    if error is None:
        run(h)
    else:
        with pytest.raises(type(error)) as caught:
            run(h)
        assert caught.value is error
    staging = [b for b in h.bufs if b.free_calls]
    if error is None or "Query" in name:  # (an operator keeps its own buffers through a failed Query)
        assert sorted(b.nbytes for b in staging) == sorted(staged)
        assert len(h.bufs) - len(staging) == kept
    else:
        assert len(staging) == len(h.bufs)
    assert all(b.free_calls == 1 for b in staging)


def test_dissolve_frees_its_class_table_but_not_the_callers():
    """(e): a host classes= table is staged and freed; a (device array, n) table is the caller's and stays"""
    h, i = FakeHandle(dict(map_dissolve=[DISS_OK, DISS_OK])), inputs()
    ops.map_dissolve(h, i.xy, 9, i.row, i.left, i.right, 2, classes=np.array([0, 1, 1]))
    assert [b.free_calls for b in h.bufs] == [1, 0, 0, 0, 0] and h.last("map_dissolve")[0][6] is h.bufs[0]
    h, i = FakeHandle(dict(map_dissolve=[DISS_OK, DISS_OK])), inputs()
    ops.map_dissolve(h, i.xy, 9, i.row, i.left, i.right, 2, classes=(i.a, 3))
    assert [b.free_calls for b in h.bufs] == [0, 0, 0, 0] and h.last("map_dissolve")[0][6:8] == (i.a, 3)
    assert_untouched(i)


# the counted call of _capi.Handle, over a stub library

class StubLibrary:
    """every rj_* function fills the counts array (its last argument, or the one before two op words) and returns rc"""

    def __init__(self, rc, values):
        self.rc, self.values, self.calls = rc, values, []

    def rj_last_error_string(self, h):
        return b"what went wrong"

    def __getattr__(self, name):
        def fn(h, *args):
            self.calls.append((name, args))
            arr = [a for a in args if hasattr(a, "_length_")][0]
            assert len(arr) == len(self.values), "the counts array must be as long as the names"
            for k, v in enumerate(self.values):
                arr[k] = v
            return self.rc
        return fn


def stub_handle(rc, values):
    h = object.__new__(_capi.Handle)
    h.L, h.h = StubLibrary(rc, values), 0  # (h = 0: close() / __del__ have nothing to destroy)
    return h


# wrapper -> (names, overflow class, positional arguments with every capacity tuple in place)
COUNTED = {
    "map_rings": (_capi.RINGS_COUNTS, _capi.RingsOverflow, (1, 9, 2, 3, 4, 2, 0, (1, 2, 3), 5, 6, 7, 8, 9)),
    "rings_polygons": (_capi.POLYGONS_COUNTS, _capi.PolygonsOverflow, (1, 3, 2, 3, 7, 0, (1, 2), 4, 5, 6, 7)),
    "rings_map": (_capi.RINGS_MAP_COUNTS, _capi.RingsMapOverflow, (1, 2, 7, 3, 4, 3, 0, (1, 2), 4, 5, 6, 7)),
    "map_crossings": (_capi.CROSSINGS_COUNTS, _capi.CrossingsOverflow, (1, 9, 2, 2, 4, 3)),
    "map_node": (_capi.NODE_COUNTS, _capi.NodeOverflow, (1, 9, 2, 2, 3, 1, 0, 4, 5, 6)),
    "map_snap": (_capi.SNAP_COUNTS, _capi.SnapOverflow, (1, 9, 2, 2, 3, 1, 0, 4, 5, 6)),
    "map_simplify": (_capi.SIMPLIFY_COUNTS, _capi.SimplifyOverflow, (1, 9, 2, 2, 5, 4, 5, 6)),
    "map_faces": (_capi.MAP_FACES_COUNTS, _capi.FacesOverflow, (1, 9, 2, 2, 3, 4)),
    "map_eliminate": (_capi.ELIMINATE_COUNTS, _capi.EliminateOverflow, (1, 9, 2, 3, 4, 2, 5, (1, 2, 3), 5, 6)),
    "map_dissolve": (_capi.DISSOLVE_COUNTS, _capi.DissolveOverflow, (1, 9, 2, 3, 4, 2, 5, 3, (1, 2, 3), 5, 6, 7, 8)),
    "map_neighbours": (_capi.NEIGHBOURS_COUNTS, _capi.NeighboursOverflow, (1, 9, 2, 3, 4, 2, (1, 2))),
    "face_points": (_capi.FACE_POINTS_COUNTS, _capi.FacePointsOverflow, (1, 9, (1, 2))),
    "within_query": (_capi.WITHIN_COUNTS, _capi.WithinOverflow, (0, 1, 2, 0, 9, 7)),
}


@pytest.mark.parametrize("name", sorted(COUNTED))
def test_counted_call_names_raises_and_checks(name):
    names, overflow, args = COUNTED[name]
    values = list(range(11, 11 + len(names)))
    got = getattr(stub_handle(_capi.RJ_OK, values), name)(*args)
    assert list(got.items()) == list(zip(names, values))  # exactly the names, in the *_COUNTS order
    with pytest.raises(overflow) as e:
        getattr(stub_handle(_capi.RJ_E_OVERFLOW, values), name)(*args)
    assert type(e.value) is overflow and e.value.code == _capi.RJ_E_OVERFLOW and list(e.value.counts.items()) == list(zip(names, values))
    assert "what went wrong" in str(e.value)
    for rc in (_capi.RJ_E_HIP, _capi.RJ_E_INVALID):
        with pytest.raises(_capi.RayJoinError) as e:
            getattr(stub_handle(rc, [0] * len(names)), name)(*args)
        assert type(e.value) is _capi.RayJoinError and e.value.code == rc


@pytest.mark.parametrize("name, refusal, field, attr", [("map_dissolve", _capi.DissolveUnmapped, "n_unmapped", "n_unmapped"),
                                                        ("map_neighbours", _capi.NeighboursNodePairs, "n_node_pairs_raw", "n_node_pairs_raw")])
def test_the_two_refusals_stay_with_their_calls(name, refusal, field, attr):
    """RJ_E_INVALID with the count set is the call's own refusal, carrying the count; with a zero count, and from any
    other call with the same counts, it is a plain RayJoinError"""
    names, _, args = COUNTED[name]
    values = [5 if n == field else 0 for n in names]
    with pytest.raises(refusal) as e:
        getattr(stub_handle(_capi.RJ_E_INVALID, values), name)(*args)
    assert getattr(e.value, attr) == 5 and e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:
        getattr(stub_handle(_capi.RJ_E_INVALID, [0] * len(names)), name)(*args)
    assert type(e.value) is _capi.RayJoinError and e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # (a nonzero count with another failure is no refusal)
        getattr(stub_handle(_capi.RJ_E_HIP, values), name)(*args)
    assert type(e.value) is _capi.RayJoinError and e.value.code == _capi.RJ_E_HIP


@pytest.mark.parametrize("name, at", [("map_simplify", 4), ("map_eliminate", 6)])
def test_tol_goes_as_two_words_or_not_at_all(name, at):
    """tol 0, 2^64 and 2^128 - 1 reach the library as (low, high) 64-bit words; -1 and 2^128 are a ValueError before any call"""
    names, _, args = COUNTED[name]
    for tol, words in ((0, (0, 0)), (1 << 64, (0, 1)), ((1 << 128) - 1, ((1 << 64) - 1, (1 << 64) - 1))):
        h = stub_handle(_capi.RJ_OK, [0] * len(names))
        getattr(h, name)(*args[:at], tol, *args[at + 1:])
        assert h.L.calls[0][1][at:at + 2] == words
    for tol in (-1, 1 << 128):
        h = stub_handle(_capi.RJ_OK, [0] * len(names))
        with pytest.raises(ValueError, match=r"tol must lie in \[0, 2\^128\), not %d" % tol):
            getattr(h, name)(*args[:at], tol, *args[at + 1:])
        assert not h.L.calls


@pytest.mark.parametrize("op", [None, (1, 2)])
def test_overlay_map_counts_are_a_tuple(op):
    args = (1, 2, 5, 3, 4, 0, (1, 2, 3), 5, 6, 7, 8, 9)
    h = stub_handle(_capi.RJ_OK, [3, 11, 2])
    assert h.overlay_map(*args, op=op) == (3, 11, 2)
    assert h.L.calls[0][0] == ("rj_overlay_map" if op is None else "rj_overlay_map_op")
    assert h.L.calls[0][1][-2:] == (1, 2) if op else hasattr(h.L.calls[0][1][-1], "_length_")
    with pytest.raises(_capi.MapOverflow) as e:
        stub_handle(_capi.RJ_E_OVERFLOW, [3, 11, 2]).overlay_map(*args, op=op)
    assert e.value.counts == (3, 11, 2) and type(e.value.counts) is tuple and e.value.code == _capi.RJ_E_OVERFLOW
