"""The Python layer's buffer ownership on the device, on the smoke pair (lattice_map(6, 90, 1) x lattice_map(14, 40, 2)), the
smallest input on which every pipeline has work: the nine map methods that DeviceOutputMap and DeviceChainMap share give
the same results on the same four arrays and leave no buffer behind once their results are freed, and the entry points
that take a capacity raise their overflow class with the true counts, and leave no buffer behind, when it is one short.
Live buffers are counted by wrapping Handle.alloc and DeviceBuffer.free here.  The CPU side is tests/test_ops_ownership.py."""
import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def overlay():
    """(dctx, ov): the overlay of the smoke pair up to ComputeOutputPolygons"""
    ctx = maps.Context([synth.lattice_map(6, 90, 1), synth.lattice_map(14, 40, 2)]).load()
    dctx = ops.DeviceContext(ctx, 0).LoadToDevice()
    ov = ops.MapOverlay(dctx).Init(1.0)
    ov.BuildIndex()
    ov.IntersectEdge(0)
    ov.LocateVerticesInOtherMap(0)
    ov.LocateVerticesInOtherMap(1)
    ov.ComputeOutputPolygons()
    yield dctx, ov
    dctx.close()


@pytest.fixture
def live(monkeypatch):
    """the DeviceBuffers allocated and not yet freed, as a set"""
    alive, alloc, free = set(), _capi.Handle.alloc, _capi.DeviceBuffer.free

    def counted_alloc(self, nbytes):
        buf = alloc(self, nbytes)
        alive.add(buf)
        return buf

    def counted_free(self):
        if self.ptr:
            alive.discard(self)
        free(self)

    monkeypatch.setattr(_capi.Handle, "alloc", counted_alloc)
    monkeypatch.setattr(_capi.DeviceBuffer, "free", counted_free)
    return alive


def flat(x):
    """a host result as a flat list of arrays"""
    if x is None:
        return []
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in flat(v)]
    if isinstance(x, maps.ScaledMap):
        return [x.pts, x.row_index, x.left, x.right]
    return [np.asarray(x)]


def image(res):
    """everything a method's result holds, read back to the host"""
    if isinstance(res, ops.DeviceNeighbours):
        return flat([res.to_host(), res.faces_to_host(), res.counts])
    if isinstance(res, ops.DeviceNodedMap):
        return flat([res.to_host(), res.counts, getattr(res, "rounds", None), getattr(res, "clean", None)])
    if isinstance(res, ops.DeviceEliminatedMap):
        return flat([res.to_host(), res.faces_to_host(), res.origin_to_host(), res.rounds])
    if isinstance(res, ops.DeviceDissolvedMap) and res.classes is not None:
        return flat([res.to_host(), res.classes_to_host(), res.origin_to_host(), res.chain_out_to_host()])
    return flat(res.to_host() if hasattr(res, "to_host") else res)


def same(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.dtype != y.dtype or x.shape != y.shape:
            return False
        names = [n for n in (x.dtype.names or ()) if not n.startswith("_")]  # (padding is not part of a record)
        if not (all(np.array_equal(x[n], y[n]) for n in names) if names else np.array_equal(x, y)):
            return False
    return True


def test_shared_methods_agree_and_leave_nothing(overlay, live):
    """overlay -> OutputMap(drop_degenerate=True); each of the nine shared methods on the DeviceOutputMap and on a
    DeviceChainMap over the same four arrays: equal host results, method by method, and no live buffer once every
    result and the map are freed"""
    dctx, ov = overlay
    h = ov.h
    area2 = sorted(int(v) for v in ov.FaceTable()["area2"])
    assert not live
    om = ov.OutputMap(drop_degenerate=True)
    assert len(live) == 6
    cm = ops.DeviceChainMap(om.xy, om.row_index, om.left, om.right, dict(n_chains=om.n_chains, n_points=om.n_points))
    pts = om.to_host()[0].pts.astype(np.float64)
    d = np.diff(pts, axis=0)
    tol_points = int(np.median(np.abs(d[:-1, 0] * d[1:, 1] - d[:-1, 1] * d[1:, 0])))  # about every other point goes
    tol_faces = area2[len(area2) // 4]  # a quarter of the faces are slivers
    classes = (np.arange(om.n_faces + 1) % 3).astype(np.int32)
    methods = [("Rings", lambda m: m.Rings(h)), ("Crossings", lambda m: m.Crossings(h)), ("Node", lambda m: m.Node(h, edge_origin=True)),
               ("Snap", lambda m: m.Snap(h)), ("Simplify", lambda m: m.Simplify(h, tol_points)), ("Eliminate", lambda m: m.Eliminate(h, tol_faces, faces=True)),
               ("Dissolve", lambda m: m.Dissolve(h, classes, records=True, origin=True)), ("Join", lambda m: m.Join(h)),
               ("Neighbours", lambda m: m.Neighbours(h, vertex=True))]
    assert [name for name, _ in methods] == ["Rings", "Crossings", "Node", "Snap", "Simplify", "Eliminate", "Dissolve", "Join", "Neighbours"]
    for name, call in methods:
        assert getattr(type(om), name) is getattr(type(cm), name), name  # written once
        results = [call(om), call(cm)]
        images = [image(r) for r in results]
        assert images[0] and same(*images), name
        for r in results:
            if hasattr(r, "free"):
                r.free()
                r.free()  # (harmless)
        assert len(live) == 6, name
    om.free()
    assert not live


def stacked(dctx, h):
    """both input maps as one chain map in device memory -- its chains cross -> (xy, n_points, row_index, n_chains), buffers"""
    m = [dctx.get_map(im) for im in range(2)]
    xy = np.concatenate([m[0].pts, m[1].pts])
    row = np.concatenate([m[0].row_index, m[1].row_index[1:] + np.uint32(m[0].n_points)]).astype(np.uint32)
    bufs = [h.alloc(16 * len(xy)).from_host(xy), h.alloc(4 * len(row)).from_host(row)]
    return (bufs[0], len(xy), bufs[1], len(row) - 1), bufs


def test_one_short_raises_the_true_counts_and_leaves_nothing(overlay, live):
    """the eight entry points that take a capacity, each with one capacity one short of the true count: the overflow class
    with the true counts, and no buffer left"""
    dctx, ov = overlay
    h = ov.h
    keep = []  # what the cases read: freed at the end

    def short(call, cls, true):
        before = len(live)
        with pytest.raises(cls) as e:
            call()
        assert e.value.counts == true and e.value.code == _capi.RJ_E_OVERFLOW and len(live) == before, cls.__name__

    om = ov.OutputMap(drop_degenerate=True)
    keep.append(om)
    true = (om.n_chains, om.n_points, om.n_faces)
    short(lambda: ov.OutputMap(drop_degenerate=True, capacities=(true[0] - 1, true[1], true[2])), _capi.MapOverflow, true)

    six = (om.xy, om.n_points, om.row_index, om.left, om.right, om.n_chains)
    rings = ops.face_rings(h, *six)
    keep.append(rings)
    c = rings.counts
    short(lambda: ops.face_rings(h, *six, capacities=(c["n_rings"] - 1, c["n_halves"], c["n_points"])), _capi.RingsOverflow, c)

    polygons = rings.Polygons(h)
    keep.append(polygons)
    c = polygons.counts
    short(lambda: rings.Polygons(h, capacities=(c["n_polygons"] - 1, c["n_members"])), _capi.PolygonsOverflow, c)

    back = rings.Map(h)
    keep.append(back)
    c = back.counts
    short(lambda: ops.rings_map(h, rings.ring_row, rings.ring_xy, rings.n_points, rings.rings, rings.n_rings, face_stride=_capi.RING_DTYPE.itemsize,
                                capacities=(c["n_chains"] - 1, c["n_points"])), _capi.RingsMapOverflow, c)

    four = (om.xy, om.n_points, om.row_index, om.n_chains)
    simple = ops.map_simplify(h, *four, 1 << 40)
    keep.append(simple)
    short(lambda: ops.map_simplify(h, *four, 1 << 40, capacity=simple.n_points - 1), _capi.SimplifyOverflow, simple.counts)

    crossed, bufs = stacked(dctx, h)
    records, c = ops.map_crossings(h, *crossed)
    assert c["n_found"] == len(records) > 0
    short(lambda: ops.map_crossings(h, *crossed, capacity=c["n_found"] - 1), _capi.CrossingsOverflow, c)
    for call, cls in ((ops.map_node, _capi.NodeOverflow), (ops.map_snap, _capi.SnapOverflow)):
        cut = call(h, *crossed, records=records)
        keep.append(cut)
        short(lambda: call(h, *crossed, records=records, capacity=cut.n_points - 1), cls, cut.counts)
        short(lambda: call(h, *crossed, capacity=cut.n_points - 1), cls, cut.counts)  # (the records made on the device)

    for r in keep + bufs:
        r.free()
    assert not live
