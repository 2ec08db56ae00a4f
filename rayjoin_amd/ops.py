"""Host-side mirror of the reference's query operators for -mode=lbvh (and -mode=grid), on top of the C ABI.

  LSILBVH(ctx).Init(max_n_xsects); .Query(query_map_id); .get_xsects(); .CopyTo()
      -- src/app/lsi.h:8-43, src/app/lsi_lbvh.h:17-98
  PIPLBVH(ctx).Init(n_points); .Query(query_map_id, query_points); .get_closest_eids()
      -- src/app/pip.h:9-38, src/app/pip_lbvh.h:14-142
  DeviceContext.LoadToDevice()/BuildIndex()
      -- src/context.h:76-88, src/run_query.cu:273-290 ("Build Index")

  LSIGrid / PIPGrid + DeviceContext.BuildGrid(grid_size): the uniform-grid operators
      -- src/app/lsi_grid.h:80-131, src/app/pip_grid.h:14-70, src/grid/uniform_grid.h:132-349
  MapOverlay(ctx).Init(); .BuildIndex(); .IntersectEdge(); .LocateVerticesInOtherMap(im);
      .ComputeOutputPolygons(); .get_xsects(im); .FaceTable(); .OutputMap()
      -- src/app/map_overlay.h:19-29, src/app/map_overlay_lbvh.h:25-265 (grid_size: MapOverlayGrid);
         FaceTable is the overlay's answer computed on the device (rj_overlay_faces), OutputMap the output map as
         device arrays (rj_overlay_map); DeviceContext.InstallMap makes one an input map again (rj_upload_map_dev);
         how= / by= on both choose another overlay operation: union, difference, ..., clip (rj_overlay_*_op)
  face_rings(handle, ...) / DeviceOutputMap.Rings(handle) / DeviceContext.Rings(im) -> DeviceRings; .polygons()
      -- the closed boundaries of a chain map's faces, stitched on the device (rj_map_rings): what a consumer of an
         output map needs to draw or export a face
  rings_map(handle, ...) / DeviceRings.Map(handle) -> DeviceChainMap; .to_host(); .Rings(handle)
      -- the way back (rj_rings_map): labelled rings, the user's polygons (maps.rings_of_polygons) or the library's own
         DeviceRings, become a chain map with maximal chains that DeviceContext.InstallMap takes
  map_crossings(handle, ...) / DeviceOutputMap.Crossings(handle) / DeviceChainMap.Crossings(handle) /
      DeviceContext.Crossings(im) -> (records, counts)
      -- the check that a chain map is a planar subdivision (rj_map_crossings): every pair of edges of ONE map that
         meets elsewhere than in a shared end point, exactly, on the device -- before InstallMap of user polygons,
         between two overlays.  The reference never validates a map (src/map/map.h:162-233)
  map_node(handle, ...) / DeviceOutputMap.Node(handle) / DeviceChainMap.Node(handle) -> DeviceNodedMap; node_rings(handle, ...)
      -- the repair behind that check where it is exact (rj_map_node): every edge cut at the vertices that lie inside it,
         so that T-junctions and half-shared borders (RJ_CROSS_TOUCH, RJ_CROSS_OVERLAP) become shared vertices and equal
         edges; node_rings takes the user's rings to the arrays rings_map takes.  Proper crossings are counted, not moved
  map_snap(handle, ...) -> DeviceNodedMap; map_snap_rounds(handle, ...) / DeviceOutputMap.Snap(handle) /
      DeviceChainMap.Snap(handle) / DeviceNodedMap.Snap(handle) -> DeviceNodedMap with rounds, clean, remaining; snap_rings(handle, ...)
      -- the repair of proper crossings too (rj_map_snap): map_node plus a cut at the rounded point of every
         RJ_CROSS_PROPER record; map_snap_rounds repeats the check and the cut until the map is clean or a round cap is
         hit and reports both -- overlapping polygons, self-crossing rings and overlay outputs with crossings become
         planar linework whose faces map_faces labels.  That the rounds end is measured, not guaranteed
  map_simplify(handle, ...) -> DeviceSimplifiedMap; DeviceOutputMap.Simplify(handle, tol) / DeviceChainMap.Simplify(handle, tol)
      -> DeviceChainMap
      -- what makes a map smaller (rj_map_simplify): the chains thinned by effective area, Visvalingam-Whyatt in rounds on
         the device.  A border that two faces share is one chain: both polygons are thinned identically, no sliver or gap
         opens, the ends of every chain stay, left / right stay valid.  It may push a chain across another one: check=True
         also returns the counts of Crossings() on the result
  map_faces(handle, ...) / DeviceChainMap.Faces(handle, check=) / DeviceNodedMap.Faces(handle) -> DeviceFacedMap
      -- the label side (rj_map_faces): the faces of a chain map computed from its geometry alone, a face number on each
         side of every chain, the face records with exact areas; check=True tells whether a map's own labels describe the
         partition its geometry has (counts["n_conflicts"])
  map_dissolve(handle, ...) / DeviceOutputMap.Dissolve(handle, classes) / DeviceChainMap.Dissolve(handle, classes) /
      .Join(handle) -> DeviceDissolvedMap
      -- Dissolve (rj_map_dissolve): faces that share a class become one face, the borders between them go, and the
      chains that meet two by two with the same classes become one chain; Join keeps every chain and only re-joins
  map_eliminate(handle, ...) / map_eliminate_rounds(handle, ...) / DeviceOutputMap.Eliminate(handle, tol) /
      DeviceChainMap.Eliminate(handle, tol) -> DeviceEliminatedMap
      -- what removes slivers (rj_map_eliminate): every face of at most tol joins the neighbour it shares the longest
         border with, exactly, on the device; the chains between merged faces are dropped, rounds repeat the call
  map_neighbours(handle, ...) / DeviceOutputMap.Neighbours(handle, vertex=) / DeviceChainMap.Neighbours(handle, vertex=)
      -> DeviceNeighbours
      -- the face adjacency table (rj_map_neighbours): which faces touch which, the integer length of the shared border,
         the chains that make it, with vertex=True the nodes where two faces meet and the faces that meet only at a
         vertex; CSR over the faces, to_csr() for a sparse matrix
  face_points(handle, labels, n, values=, faces=, members=) / PIPLBVH.Summarize(values=, faces=, members=) -> DeviceFacePoints
      -- per face the count, the exact sum, min, max and the members of located points (rj_face_points), rows as DeviceNeighbours' faces
  NearestLBVH(ctx).Init(n_points); .Query(query_map_id, query_points, max_dist=); .get_eids(); .get_records(); .get_dist()
      -- the nearest edge of the indexed map for every point and its exact distance (rj_nearest_query): Near, sjoin_nearest,
         the join within a distance
  KNearestLBVH(ctx).Init(n_points, k); .Query(query_map_id, query_points, k=, max_dist=); .get_counts(); .get_eids();
      .get_records(); .get_dist(); .to_csr()
      -- the k (1 .. 32) nearest edges of the indexed map for every point, nearest first, as (n, k) arrays with a count per
         row (rj_knearest_query): the closest-count of Near and Generate Near Table, the candidates of map matching
  WithinLBVH(ctx).Init(n_points, pair_capacity); .Query(query_map_id, query_points, max_dist=, grow=); .Count(...); .get_offsets();
      .get_eids(); .get_records(); .get_dist(); .to_csr(); .counts()
      -- every edge of the indexed map within max_dist of each point, as a CSR over the points (rj_within_query): dwithin,
         Select by distance, Generate Near Table (all)
  WindowLBVH(ctx).Init(n_windows, pair_capacity); .Query(base_map_id, windows, flags=, grow=); .Count(...); .get_offsets();
      .get_eids(); .get_flags(); .to_csr(); .counts()
      -- every edge of the indexed map that meets each closed rectangle (x0, y0, x1, y1), as a CSR over the windows
         (rj_window_query): the bounding-box select, sindex.query(box), the linework of a tile

Same names, argument meaning and error behaviour, with two deliberate differences recorded in
DESIGN.md: LSI pairs are always evaluated as (e1 = map-0 edge, e2 = map-1 edge) so results
equal -mode=grid bit for bit, and a full queue raises QueueOverflow instead of being undefined
behaviour (src/util/queue.h:37 only asserts)."""
import numpy as np

from . import _capi
from .maps import Context


class _Owned:
    """The DeviceBuffers of a call while it runs, as a context manager: alloc(nbytes) records the buffer, and leaving the
    block -- by any exception, or at its end -- frees every buffer still owned, each once.  release() hands them to the
    caller: an output's owner releases when its call has succeeded, a staging temporary's owner never does."""

    def __init__(self, handle):
        self.handle, self.bufs = handle, []

    def alloc(self, nbytes):
        self.bufs.append(self.handle.alloc(nbytes))
        return self.bufs[-1]

    def release(self):
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        bufs, self.bufs = self.bufs, []
        for b in bufs:
            b.free()


def _sizing_counts(call, overflow, *args, **kw):
    """The counts of a sizing call (zero capacities, no arrays in args), whether it returned them or raised `overflow` with them"""
    try:
        return call(*args, **kw)
    except overflow as e:
        return e.counts


def _over_points(op, query_map_id, query_points, point_range, call):
    """call(device points or None, begin, n) for a query operator (its h, ctx_, n_alloc) over int64[n,2] scaled host points,
    staged for the call and freed behind it, or over the query map's own vertices, optionally a [begin, end) sub-range (a
    shard) -> (n, what call returned)"""
    if query_points is not None:
        pts = np.ascontiguousarray(query_points, dtype=np.int64).reshape(-1, 2)
        n = pts.shape[0]
        assert n <= op.n_alloc
        with _Owned(op.h) as tmp:
            return n, call(tmp.alloc(16 * max(1, n)).from_host(pts), 0, n)
    b, e = point_range if point_range is not None else (0, op.ctx_.get_map(query_map_id).n_points)
    n = e - b
    assert n <= op.n_alloc
    return n, call(None, b, n)


def _stage_map(own, m, sides):
    """The host image of a map in temporaries of `own` -> [xy, row_index] and, with sides, [.., left, right]"""
    cols = [(m.pts, np.int64, 16 * max(1, m.n_points)), (m.row_index, np.uint32, 4 * (m.n_chains + 1))]
    if sides:
        cols += [(m.left, np.int32, 4 * max(1, m.n_chains)), (m.right, np.int32, 4 * max(1, m.n_chains))]
    return [own.alloc(nbytes).from_host(np.ascontiguousarray(a, dtype=dtype)) for a, dtype, nbytes in cols]


class _OwnsBuffers:
    """An object that owns device buffers: _buffers names the attributes that hold them (None: not there).  free() frees
    them; a second free() is harmless, as DeviceBuffer.free is."""
    _buffers = ()

    def free(self):
        for name in self._buffers:
            if getattr(self, name) is not None:
                getattr(self, name).free()


class DeviceContext:
    """A maps.Context plus its GPU residency: uploads both maps, owns the rj_handle."""

    def __init__(self, ctx, device_id=0):
        assert isinstance(ctx, Context)
        self.ctx = ctx
        self.handle = _capi.Handle(device_id)
        self.loaded = [False, False]
        self.indexed = [False, False]
        self.installed = [None, None]  # maps that came from device memory (InstallMap) instead of ctx

    def LoadToDevice(self):
        for im in range(2):
            m = self.ctx.get_map(im)
            if m is not None:
                self.handle.upload_map(im, m.pts, m.row_index, m.left, m.right)
                self.installed[im] = None
                self.loaded[im] = True
                self.indexed[im] = False
        return self

    def InstallMap(self, im, output_map):
        """An ops.DeviceOutputMap (MapOverlay.OutputMap(drop_degenerate=True)) or an ops.DeviceChainMap (rings_map, DeviceRings.Map)
        becomes map `im` of this context without
        leaving the GPU (rj_upload_map_dev), so that another MapOverlay can run: (A x B) x C.  The output map's faces
        are the new map's faces.  Its coordinates are scaled integers: the caller is responsible for ONE Scaling over
        all layers -- this context's Scaling must be the one the output map was computed under, and the other map of
        this context must have been scaled by it too (maps.Context over every layer's bounding box).  The output map
        may belong to another DeviceContext on the same device and can be freed afterwards.  get_map(im) then
        returns the host image of the installed map (read back once, here)."""
        om = output_map
        self.handle.upload_map_dev(im, om.xy, om.n_points, om.row_index, om.left, om.right, om.n_chains)
        self.installed[im] = om.to_host()[0]
        self.installed[im].map_id = im
        self.loaded[im] = True
        self.indexed[im] = False
        return self

    def BuildIndex(self, base_map_id):
        self.handle.build_lbvh(base_map_id)
        self.indexed[base_map_id] = True
        return self.handle.last_ms(_capi.RJ_T_BUILD)

    def BuildGrid(self, grid_size, map_ids=(0, 1)):
        """UniformGrid::AddMapsToGrid (both maps, LSI) / AddMapToGrid (base map only, PIP)."""
        ms = 0.0
        for im in map_ids:
            self.handle.build_grid(im, grid_size)
            ms += self.handle.last_ms(_capi.RJ_T_BUILD)
        return ms

    def get_map(self, im):
        return self.installed[im] if self.installed[im] is not None else self.ctx.get_map(im)

    def Rings(self, im, **kw):
        """face_rings of input map `im` (its host image goes to temporaries on the device): the boundaries of its faces"""
        m = self.get_map(im)
        with _Owned(self.handle) as tmp:
            xy, row_index, left, right = _stage_map(tmp, m, True)
            return face_rings(self.handle, xy, m.n_points, row_index, left, right, m.n_chains, **kw)

    def Crossings(self, im, **kw):
        """map_crossings of input map `im` (its host image goes to temporaries on the device): empty when the map is a
        planar subdivision"""
        m = self.get_map(im)
        with _Owned(self.handle) as tmp:
            xy, row_index = _stage_map(tmp, m, False)
            return map_crossings(self.handle, xy, m.n_points, row_index, m.n_chains, **kw)

    def close(self):
        self.handle.close()


class LSILBVH:
    def __init__(self, dctx):
        self.ctx_ = dctx
        self.h = dctx.handle
        self.capacity = 0
        self.queue = None
        self.n_xsects = 0

    def Init(self, max_n_xsects):
        self.capacity = int(max_n_xsects)
        self.queue = self.h.alloc(8 * max(1, self.capacity))

    def Query(self, query_map_id, eid_range=None):
        """Intersect every edge (or the eid sub-range: a shard) of map `query_map_id` with the
        indexed other map.  Synchronous.  Returns the number of intersections."""
        base = 1 - query_map_id
        qb, qe = eid_range if eid_range is not None else (0, self.ctx_.get_map(query_map_id).n_edges)
        try:
            self.n_xsects = self.h.lsi_query(base, query_map_id, qb, qe, self.capacity, self.queue)
        except _capi.QueueOverflow as e:
            self.n_xsects = min(e.n_found, self.capacity)
            raise
        return self.n_xsects

    def get_pairs(self, sort=True):
        """(eid map 0, eid map 1) pairs on the host; sorted = the checker's canonical order."""
        if sort:
            self.h.sort_pairs(self.queue, self.n_xsects)
        return self.queue.to_host(np.uint32, 2 * self.n_xsects).reshape(-1, 2)

    def get_xsects(self, sort=True):
        """The reference's 48-byte Intersection records for the current result."""
        if sort:
            self.h.sort_pairs(self.queue, self.n_xsects)
        out = self.h.alloc(48 * max(1, self.n_xsects))
        self.h.lsi_points(self.queue, self.n_xsects, out)
        rec = out.to_host(_capi.XSECT_DTYPE, self.n_xsects)
        out.free()
        return rec

    CopyTo = get_xsects


class PIPLBVH:
    _query = "pip_query"  # the handle's call that Query makes

    def __init__(self, dctx):
        self.ctx_ = dctx
        self.h = dctx.handle
        self.closest = None
        self.faces = None
        self.n = 0

    def Init(self, n_points):
        self.n_alloc = int(n_points)
        self.closest = self.h.alloc(4 * max(1, self.n_alloc))
        self.faces = self.h.alloc(4 * max(1, self.n_alloc))

    def Query(self, query_map_id, query_points=None, point_range=None):
        """query_points: int64[n,2] scaled host points, or None for the query map's own vertices
        (RunPIPQuery, src/run_query.cu:346), optionally a [begin, end) sub-range (a shard)."""
        query = getattr(self.h, self._query)
        self.n, _ = _over_points(self, query_map_id, query_points, point_range,
                                 lambda buf, b, n: query(1 - query_map_id, query_map_id, buf, b, n, self.closest, self.faces))
        return self.n

    def get_closest_eids(self):
        return self.closest.to_host(np.uint32, self.n)

    def get_face_ids(self):
        return self.faces.to_host(np.int32, self.n)

    def Summarize(self, values=None, value_stride=1, faces=None, members=False, **kw):
        """face_points over the face ids of the last Query, on the device, as a DeviceFacePoints: per face of the base map
        how many of the queried points it holds, the exact sum, min and max of values[i * value_stride] (int64 in device
        memory) and, with members, which points.  faces: the labels of the faces as a device int32 array or a
        (device array, count) pair -- DeviceNeighbours.labels(handle) of the base map, so that the rows here are the
        rows of its adjacency table."""
        return face_points(self.h, self.faces, self.n, values=values, value_stride=value_stride, faces=faces, members=members, **kw)


class _DistanceQuery:
    """What NearestLBVH, KNearestLBVH and WithinLBVH share: the per-row outputs (eid, exact record, distance in double; `rows_`: how many
    the last call filled) and the freeing of the device buffers."""

    def __init__(self, dctx):
        self.ctx_ = dctx
        self.h = dctx.handle
        self.eids = self.records = self.dist = None
        self.n = self.rows_ = 0
        self.has_records = self.has_dist = False

    def get_eids(self):
        return self.eids.to_host(np.uint32, self.rows_)

    def get_records(self):
        """-> NEAR_DTYPE rows; ValueError after a Query with records=False"""
        if not self.has_records:
            raise ValueError("the last Query ran with records=False")
        return self.records.to_host(_capi.NEAR_DTYPE, self.rows_)

    def get_dist(self):
        if not self.has_dist:
            raise ValueError("the last Query ran with dist=False")
        return self.dist.to_host(np.float64, self.rows_)

    @staticmethod
    def exact(records):
        """NEAR_DTYPE rows -> [(eid, where, num, den)] with num (signed) and den as Python ints: d^2 = num^2 / den where
        `where` is 0, num / den (den = 1) at an end"""
        return [(int(r["eid"]), int(r["where"]), (int(r["num_hi"]) << 64) + int(r["num_lo"]), (int(r["den_hi"]) << 64) + int(r["den_lo"])) for r in records]

    def _free(self, *names):
        for name in names:
            if getattr(self, name) is not None:
                getattr(self, name).free()
                setattr(self, name, None)


class NearestLBVH(_DistanceQuery):
    """The nearest edge of the indexed base map for every query point (rj_nearest_query), mirroring PIPLBVH: the eid, the
    exact record (which end or the interior, and d^2 as a rational) and the distance in double, one row per point."""

    def Init(self, n_points):
        self.n_alloc = int(n_points)
        self.eids = self.h.alloc(4 * max(1, self.n_alloc))
        self.records = self.h.alloc(_capi.NEAR_DTYPE.itemsize * max(1, self.n_alloc))
        self.dist = self.h.alloc(8 * max(1, self.n_alloc))

    def Query(self, query_map_id, query_points=None, point_range=None, max_dist=None, records=True, dist=True):
        """query_points: int64[n,2] scaled host points, or None for the query map's own vertices, optionally a [begin, end)
        sub-range (a shard).  max_dist (scaled units, None: unlimited): only edges within it qualify, the others' points
        miss.  records / dist: whether the call fills them.  Returns the number of points."""
        md = -1 if max_dist is None else int(max_dist)
        rec, dst = (self.records if records else None), (self.dist if dist else None)
        n, _ = _over_points(self, query_map_id, query_points, point_range,
                            lambda buf, b, n: self.h.nearest_query(1 - query_map_id, query_map_id, buf, b, n, self.eids, rec, dst, md))
        self.n = self.rows_ = n
        self.has_records, self.has_dist = bool(records), bool(dist)
        return n

    def nums(self):
        """-> the exact num of every record as a list of Python ints"""
        return [t[2] for t in self.exact(self.get_records())]

    def free(self):
        self._free("eids", "records", "dist")


class KNearestLBVH(_DistanceQuery):
    """The k nearest edges of the indexed base map for every query point (rj_knearest_query), mirroring NearestLBVH: (n, k)
    arrays -- row i holds point i's edges nearest first, equal distances to the smaller eid -- of the eid, the exact record
    and the distance in double, and the count of every row; the entries of a row behind its count are the miss."""

    def __init__(self, dctx):
        super().__init__(dctx)
        self.counts = None
        self.n_alloc = self.k_alloc = self.k = 0

    def Init(self, n_points, k):
        self.free()
        self.n_alloc, self.k_alloc = int(n_points), int(k)
        assert 1 <= self.k_alloc <= _capi.KNEAREST_MAX_K
        rows = max(1, self.n_alloc * self.k_alloc)
        self.counts = self.h.alloc(4 * max(1, self.n_alloc))
        self.eids = self.h.alloc(4 * rows)
        self.records = self.h.alloc(_capi.NEAR_DTYPE.itemsize * rows)
        self.dist = self.h.alloc(8 * rows)

    def Query(self, query_map_id, query_points=None, point_range=None, k=None, max_dist=None, records=True, dist=True):
        """query_points: int64[n,2] scaled host points, or None for the query map's own vertices, optionally a [begin, end)
        sub-range (a shard).  k (None: Init's): how many edges per point, at most Init's.  max_dist (scaled units, None:
        unlimited): only edges within it qualify.  records / dist: whether the call fills them.  Returns the number of
        points."""
        k = self.k_alloc if k is None else int(k)
        assert k <= self.k_alloc
        md = -1 if max_dist is None else int(max_dist)
        rec, dst = (self.records if records else None), (self.dist if dist else None)
        n, _ = _over_points(self, query_map_id, query_points, point_range,
                            lambda buf, b, n: self.h.knearest_query(1 - query_map_id, query_map_id, buf, b, n, k, self.eids, self.counts, rec, dst, md))
        self.n, self.k, self.rows_ = n, k, n * k
        self.has_records, self.has_dist = bool(records), bool(dist)
        return n

    def get_counts(self):
        """-> uint32[n]: the valid entries of every row"""
        return self.counts.to_host(np.uint32, self.n)

    def get_eids(self):
        return super().get_eids().reshape(self.n, self.k)

    def get_records(self):
        return super().get_records().reshape(self.n, self.k)

    def get_dist(self):
        return super().get_dist().reshape(self.n, self.k)

    @staticmethod
    def exact(records):
        """(n, k) NEAR_DTYPE rows -> per row [(eid, where, num, den)] as _DistanceQuery.exact gives them"""
        return [_DistanceQuery.exact(row) for row in records]

    def to_csr(self):
        """-> (indptr int64[n + 1], eids uint32[sum of the counts]): the valid entries of every row, nearest first"""
        counts, eids = self.get_counts(), self.get_eids()
        indptr = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        return indptr, eids[np.arange(self.k)[None, :] < counts[:, None]]

    def free(self):
        self._free("counts", "eids", "records", "dist")
        self.n_alloc = self.k_alloc = 0


class WithinLBVH(_DistanceQuery):
    """Every edge of the indexed base map within max_dist of each query point (rj_within_query), mirroring NearestLBVH: a
    CSR over the points -- offsets, and one row per pair: the eid (ascending per point), the exact record and the distance."""

    def __init__(self, dctx):
        super().__init__(dctx)
        self.offsets = None
        self.n_pairs = 0
        self.n_alloc = self.capacity = 0
        self.counts_ = dict.fromkeys(_capi.WITHIN_COUNTS, 0)

    def Init(self, n_points, pair_capacity):
        self.free()
        self.n_alloc = int(n_points)
        self.offsets = self.h.alloc(8 * (self.n_alloc + 1))
        self._alloc_pairs(int(pair_capacity))

    def _alloc_pairs(self, capacity):
        self._free("eids", "records", "dist")
        self.capacity = capacity
        self.eids = self.h.alloc(4 * max(1, capacity))
        self.records = self.h.alloc(_capi.NEAR_DTYPE.itemsize * max(1, capacity))
        self.dist = self.h.alloc(8 * max(1, capacity))

    def _call(self, query_map_id, query_points, point_range, max_dist, capacity, rec, dst):
        eids = self.eids if capacity else None
        return _over_points(self, query_map_id, query_points, point_range,
                            lambda buf, b, n: self.h.within_query(1 - query_map_id, query_map_id, buf, b, n, max_dist, capacity, self.offsets, eids, rec, dst))

    def _set(self, n, n_pairs, counts, records, dist):
        self.n, self.n_pairs, self.rows_, self.counts_ = n, n_pairs, n_pairs, counts
        self.has_records, self.has_dist = bool(records), bool(dist)

    def Query(self, query_map_id, query_points=None, point_range=None, max_dist=0, records=True, dist=True, grow=True):
        """query_points: int64[n,2] scaled host points, or None for the query map's own vertices, optionally a [begin, end)
        sub-range (a shard).  max_dist (scaled units, 0 .. 2^48): every edge with d <= max_dist is listed.  records / dist:
        whether the call fills them.  grow: on an overflow (or with a capacity of 0) the pair arrays are allocated again at
        the true count and the call repeats once; otherwise _capi.WithinOverflow with the true counts.  Returns n_pairs."""
        self.n_pairs = self.rows_ = 0
        self.has_records = self.has_dist = False
        args = (query_map_id, query_points, point_range, int(max_dist))
        if self.capacity == 0:  # (a capacity of 0 is the counting call: it sizes the arrays)
            n, counts = self._call(*args, 0, None, None)
            if counts["n_pairs"] and not grow:
                raise _capi.WithinOverflow("rj_within_query: %d pairs; capacity 0" % counts["n_pairs"], counts)
            if counts["n_pairs"]:
                self._alloc_pairs(counts["n_pairs"])
        if self.capacity:
            try:
                n, counts = self._call(*args, self.capacity, self.records if records else None, self.dist if dist else None)
            except _capi.WithinOverflow as e:
                if not grow:
                    raise
                self._alloc_pairs(e.counts["n_pairs"])
                n, counts = self._call(*args, self.capacity, self.records if records else None, self.dist if dist else None)
        self._set(n, counts["n_pairs"], counts, records, dist)
        return self.n_pairs

    def Count(self, query_map_id, query_points=None, point_range=None, max_dist=0):
        """the counting call: how many edges lie within max_dist of each point -> uint64[n]; nothing but the offsets and the
        counts is written"""
        n, counts = self._call(query_map_id, query_points, point_range, int(max_dist), 0, None, None)
        self._set(n, 0, counts, False, False)
        return np.diff(self.get_offsets())

    def get_offsets(self):
        return self.offsets.to_host(np.uint64, self.n + 1)

    def to_csr(self):
        """-> (indptr int64[n + 1], eids uint32[n_pairs]): row i lists the edges within the distance of point i, ascending"""
        return self.get_offsets().astype(np.int64), self.get_eids()

    def counts(self):
        """the counts of the last call: n_pairs, n_points_hit, max_per_point"""
        return dict(self.counts_)

    def free(self):
        self._free("offsets", "eids", "records", "dist")
        self.capacity = 0


class WindowLBVH(_OwnsBuffers):
    """The edges of the indexed base map that meet each window (rj_window_query): a CSR over the windows -- offsets, and one
    row per pair: the eid (ascending per window) and the flags byte (bit 0: the edge's first point lies in the window,
    bit 1: its second point does)."""
    _buffers = ("offsets", "eids", "flags")

    def __init__(self, dctx):
        self.ctx_ = dctx
        self.h = dctx.handle
        self.offsets = self.eids = self.flags = None
        self.n = self.n_pairs = self.n_alloc = self.capacity = 0
        self.has_flags = False
        self.counts_ = dict.fromkeys(_capi.WINDOW_COUNTS, 0)

    def Init(self, n_windows, pair_capacity):
        self.free()
        self.n_alloc = int(n_windows)
        self.offsets = self.h.alloc(8 * (self.n_alloc + 1))
        self._alloc_pairs(int(pair_capacity))

    def _alloc_pairs(self, capacity):
        for name in ("eids", "flags"):
            if getattr(self, name) is not None:
                getattr(self, name).free()
        self.capacity = capacity
        self.eids = self.h.alloc(4 * max(1, capacity))
        self.flags = self.h.alloc(max(1, capacity))

    def _over_windows(self, windows, call):
        """call(device windows, n) over an (n, 4) int64 host array, staged for the call and freed behind it, or over a
        contiguous int64 device tensor of that shape (anything with data_ptr() and shape) -> (n, what call returned)"""
        if hasattr(windows, "data_ptr"):
            shape = tuple(windows.shape)
            assert len(shape) == 2 and shape[1] == 4
            assert not hasattr(windows, "is_contiguous") or (windows.is_contiguous() and windows.element_size() == 8)
            n = int(shape[0])
            assert n <= self.n_alloc
            return n, call(windows, n)
        win = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 4)
        n = win.shape[0]
        assert n <= self.n_alloc
        with _Owned(self.h) as tmp:
            return n, call(tmp.alloc(32 * max(1, n)).from_host(win), n)

    def _call(self, base_map_id, windows, capacity, flags):
        eids = self.eids if capacity else None
        return self._over_windows(windows, lambda buf, n: self.h.window_query(base_map_id, buf, n, capacity, self.offsets, eids, flags))

    def Query(self, base_map_id, windows, flags=True, grow=True):
        """windows: (n, 4) int64 (x0, y0, x1, y1), closed rectangles in scaled coordinates, a host array or a device tensor.
        flags: whether the call fills them.  grow: on an overflow (or with a capacity of 0) the pair arrays are allocated
        again at the true count and the call repeats once; otherwise _capi.WindowOverflow with the true counts.  Returns
        n_pairs."""
        self.n_pairs, self.has_flags = 0, False
        if self.capacity and not grow:
            n, counts = self._call(base_map_id, windows, self.capacity, self.flags if flags else None)
        else:  # the counted call: the counting call of a capacity of 0, or a call whose overflow carries the true counts
            eids, fl = (self.eids, self.flags if flags else None) if self.capacity else (None, None)
            n, counts = self._over_windows(windows, lambda buf, n: _sizing_counts(self.h.window_query, _capi.WindowOverflow, base_map_id, buf, n,
                                                                                  self.capacity, self.offsets, eids, fl))
            if counts["n_pairs"] > self.capacity:
                if not grow:
                    raise _capi.WindowOverflow("rj_window_query: %d pairs; capacity 0" % counts["n_pairs"], counts)
                self._alloc_pairs(counts["n_pairs"])  # the sized call: once more at the true count
                n, counts = self._call(base_map_id, windows, self.capacity, self.flags if flags else None)
        self.n, self.n_pairs, self.counts_, self.has_flags = n, counts["n_pairs"], counts, bool(flags)
        return self.n_pairs

    def Count(self, base_map_id, windows):
        """the counting call: how many edges meet each window -> uint64[n]; nothing but the offsets and the counts is written"""
        n, counts = self._call(base_map_id, windows, 0, None)
        self.n, self.n_pairs, self.counts_, self.has_flags = n, 0, counts, False
        return np.diff(self.get_offsets())

    def get_offsets(self):
        return self.offsets.to_host(np.uint64, self.n + 1)

    def get_eids(self):
        return self.eids.to_host(np.uint32, self.n_pairs)

    def get_flags(self):
        """-> uint8 per pair; ValueError after a Query with flags=False"""
        if not self.has_flags:
            raise ValueError("the last Query ran with flags=False")
        return self.flags.to_host(np.uint8, self.n_pairs)

    def to_csr(self):
        """-> (indptr int64[n + 1], eids uint32[n_pairs]): row i lists the edges that meet window i, ascending"""
        return self.get_offsets().astype(np.int64), self.get_eids()

    def counts(self):
        """the counts of the last call: n_pairs, n_windows_hit, max_per_window"""
        return dict(self.counts_)

    def free(self):
        super().free()
        self.offsets = self.eids = self.flags = None
        self.capacity = 0


class LSIGrid(LSILBVH):
    """-mode=grid LSI (src/app/lsi_grid.h): needs DeviceContext.BuildGrid(g) for both maps.
    The grid holds both maps, so the result does not depend on query_map_id and there is no
    eid sub-range (the reference's LSIGrid::Query ignores its query_map_id too, lsi_grid.h:103-104)."""

    def Query(self, query_map_id=1, eid_range=None):
        if eid_range is not None:
            raise ValueError("LSIGrid has no eid sub-ranges: the grid joins the two whole maps")
        try:
            self.n_xsects = self.h.lsi_query_grid(self.capacity, self.queue)
        except _capi.QueueOverflow as e:
            self.n_xsects = min(e.n_found, self.capacity)
            raise
        return self.n_xsects


class PIPGrid(PIPLBVH):
    """-mode=grid PIP (src/app/pip_grid.h): needs DeviceContext.BuildGrid(g, (base_map_id,))."""
    _query = "pip_query_grid"


FACE_TABLE_DTYPE = np.dtype([("face0", "<i4"), ("face1", "<i4"), ("area2", object), ("area", "<f8")])


class MapOverlay:
    """The overlay stages of MapOverlayLBVH (src/app/map_overlay.h:19-29), or of MapOverlayGrid with grid_size set, on
    both maps of a DeviceContext, and the face table: which face of map 0 overlaps which face of map 1, and by how much."""

    def __init__(self, dctx, grid_size=None):
        self.ctx_ = dctx
        self.h = dctx.handle
        self.grid_size = grid_size
        self.n_xsects = 0
        self.xsects = [None, None]

    def Init(self, xsect_factor=0.2):
        """map_overlay_lbvh.h:25-40: a queue of xsect_factor * (edges of both maps) intersections"""
        m = [self.ctx_.get_map(im) for im in range(2)]
        self.capacity = int(xsect_factor * (m[0].n_edges + m[1].n_edges))
        self.pairs = self.h.alloc(8 * max(1, self.capacity))
        self.closest = [self.h.alloc(4 * max(1, m[im].n_points)) for im in range(2)]
        self.faces = [self.h.alloc(4 * max(1, m[im].n_points)) for im in range(2)]
        self.located = [False, False]
        return self

    def BuildIndex(self):
        for im in range(2):
            if self.grid_size:
                self.h.build_grid(im, self.grid_size)
            else:
                self.h.build_lbvh(im)
                self.ctx_.indexed[im] = True

    def IntersectEdge(self, query_map_id=0):
        """every edge of map query_map_id against the other map; returns the number of intersections"""
        if self.grid_size:
            self.n_xsects = self.h.lsi_query_grid(self.capacity, self.pairs)
        else:
            qe = self.ctx_.get_map(query_map_id).n_edges
            self.n_xsects = self.h.lsi_query(1 - query_map_id, query_map_id, 0, qe, self.capacity, self.pairs)
        return self.n_xsects

    def LocateVerticesInOtherMap(self, query_map_id):
        np_ = self.ctx_.get_map(query_map_id).n_points
        fn = self.h.pip_query_grid if self.grid_size else self.h.pip_query
        fn(1 - query_map_id, query_map_id, None, 0, np_, self.closest[query_map_id], self.faces[query_map_id])
        self.located[query_map_id] = True

    def ComputeOutputPolygons(self):
        """the per-map records, ordered along every edge, with their mid-point faces (rj_overlay_edge_xsects)"""
        for im in range(2):
            self.xsects[im] = self.h.alloc(48 * max(1, self.n_xsects))
            self.h.overlay_edge_xsects(im, self.pairs, self.n_xsects, self.xsects[im])

    def get_xsects(self, im):
        return self.xsects[im].to_host(_capi.XSECT_DTYPE, self.n_xsects)

    def get_vertex_faces(self, im):
        return self.faces[im].to_host(np.int32, self.ctx_.get_map(im).n_points)

    def FaceTable(self, capacity=None, how="intersection", by="pair"):
        """rows (face0, face1, area2, area) ascending by (face0, face1): area2 is twice the overlap's signed area in
        scaled units^2, exact (a Python int); area is in input units (area2 / 2 * rrx * rry of the context's Scaling).
        how ("intersection", "union", "difference", "symmetric_difference", "identity") selects the (face of map 0, face
        of map 1) pairs that are faces of the result, by ("pair", "map0", "map1") what names a face (rj_overlay_faces_op):
        with another how a row's face may be 0 ("outside that map"), with by="map0" face1 is always 0.  The defaults
        are rj_overlay_faces."""
        if not (self.located[0] and self.located[1]) or self.xsects[0] is None:
            raise RuntimeError("MapOverlay.FaceTable needs LocateVerticesInOtherMap(0), (1) and ComputeOutputPolygons() first")
        op = overlay_op(how, by)
        cap = int(capacity) if capacity is not None else max(64, 2 * self.n_xsects + 64)
        while True:
            out = self.h.alloc(_capi.FACE_DTYPE.itemsize * max(1, cap))
            try:
                n = self.h.overlay_faces(self.xsects[0], self.xsects[1], self.n_xsects, self.faces[0], self.faces[1], cap, out, op)
                break
            except _capi.QueueOverflow as e:
                if capacity is not None:
                    raise
                out.free()
                cap = e.n_found
        raw = out.to_host(_capi.FACE_DTYPE, n)
        out.free()
        return face_table_from_rows(raw, self.ctx_.ctx.scaling)

    def OutputMap(self, drop_degenerate=False, capacities=None, how="intersection", by="pair", merge=False):
        """The output map as a DeviceOutputMap (rj_overlay_map): the pieces the CDB writer keeps, in its order, in scaled
        integers, faces numbered by the ordered pair (face of map 0, face of map 1) -- face k is row k - 1 of
        FaceTable().  drop_degenerate leaves out the pieces with fewer than two points (what an input map may not have:
        DeviceContext.InstallMap).  capacities = (chains, points, faces): MapOverflow with the true counts when one is
        too small; left open, a sizing call finds them.  how / by as FaceTable (rj_overlay_map_op): a piece is kept
        when the faces on its two sides differ; how="intersection", by="map0" clips map 0 to where map 1 covers and
        keeps map 0's face ids (face_pairs[k - 1] = (f0, 0)).  merge (RJ_OVM_MERGE_PIECES) joins adjacent pieces of one
        source chain that have the same two faces and touch into one chain, after drop_degenerate: a chain that forty
        dissolved boundaries cut leaves as one chain again; the faces and their numbers do not change.  Without it every
        piece is a chain of its own."""
        if not (self.located[0] and self.located[1]) or self.xsects[0] is None:
            raise RuntimeError("MapOverlay.OutputMap needs LocateVerticesInOtherMap(0), (1) and ComputeOutputPolygons() first")
        flags = (_capi.RJ_OVM_DROP_DEGENERATE if drop_degenerate else 0) | (_capi.RJ_OVM_MERGE_PIECES if merge else 0)
        op = overlay_op(how, by)
        args = (self.xsects[0], self.xsects[1], self.n_xsects, self.faces[0], self.faces[1], flags)
        if capacities is None:
            capacities = _sizing_counts(self.h.overlay_map, _capi.MapOverflow, *args, (0, 0, 0), None, None, None, None, None, None, op=op)
        cc, pc, fc = (int(v) for v in capacities)
        with _Owned(self.h) as own:
            bufs = [own.alloc(16 * max(1, pc)), own.alloc(4 * (cc + 1)), own.alloc(4 * max(1, cc)), own.alloc(4 * max(1, cc)),
                    own.alloc(8 * max(1, fc)), own.alloc(4 * max(1, cc))]
            counts = self.h.overlay_map(*args, (cc, pc, fc), *bufs, op=op)
            own.release()
        return DeviceOutputMap(*bufs, counts, drop_degenerate, merge)


class _ChainMapOps(_OwnsBuffers):
    """What every labelled chain map in device memory offers, over its xy, n_points, row_index, left, right, n_chains: the
    host image and the map operations, each on the device with a result of its own."""

    def _scaled_map(self):
        from .maps import ScaledMap
        return ScaledMap(0, self.xy.to_host(np.int64, 2 * self.n_points).reshape(-1, 2), self.row_index.to_host(np.uint32, self.n_chains + 1),
                         self.left.to_host(np.int32, self.n_chains).astype(np.int64), self.right.to_host(np.int32, self.n_chains).astype(np.int64))

    def Rings(self, handle, **kw):
        """face_rings of this map: the closed boundaries of its faces, on the device (of an overlay's output map, face k is
        row k - 1 of FaceTable())"""
        return face_rings(handle, self.xy, self.n_points, self.row_index, self.left, self.right, self.n_chains, **kw)

    def Crossings(self, handle, **kw):
        """map_crossings of this map, on the device: overlapping or self-crossing polygons show here, and whether an output
        map still has no crossings (its cut points are truncated to integers)"""
        return map_crossings(handle, self.xy, self.n_points, self.row_index, self.n_chains, **kw)

    def Node(self, handle, **kw):
        """map_node of this map, on the device: its edges cut at the vertices that lie inside them (left / right stay valid)"""
        return map_node(handle, self.xy, self.n_points, self.row_index, self.n_chains, **kw)

    def Snap(self, handle, **kw):
        """map_snap_rounds of this map, on the device: cut at its touches, overlaps and rounded proper crossings until a check
        finds none (.clean) or max_rounds is hit; the chains stay, so left / right stay valid as chain labels"""
        return map_snap_rounds(handle, self.xy, self.n_points, self.row_index, self.n_chains, **kw)

    def Simplify(self, handle, tol, check=False, capacity=None):
        """map_simplify of this map, on the device, as a DeviceChainMap of its own (copies of left / right: the chains do not
        change): what InstallMap, Rings() and Crossings() take; its counts are those of rj_map_simplify with n_chains and
        n_edges.  check: -> (the map, the counts of Crossings() on it) -- thinning can push a chain across another one"""
        return _simplified_chain_map(handle, self, tol, check, capacity)

    def Eliminate(self, handle, tol, rounds=1, faces=False):
        """map_eliminate of this map, on the device, as a DeviceEliminatedMap of its own: every face of area2 <= tol merged
        into the neighbour with the longest shared border, the chains between merged faces dropped.  rounds > 1: repeated
        (map_eliminate_rounds) until a round eliminates nothing or `rounds` have run; .rounds holds the counts of each"""
        args = (self.xy, self.n_points, self.row_index, self.left, self.right, self.n_chains, tol)
        if int(rounds) <= 1:
            return map_eliminate(handle, *args, drop=True, faces=faces)
        return map_eliminate_rounds(handle, *args, max_rounds=rounds, faces=faces)

    def Dissolve(self, handle, classes=None, **kw):
        """map_dissolve of this map, on the device, as a DeviceDissolvedMap of its own: the faces merged by class (classes: an
        int32 table indexed by label, on the device or as a numpy array; None: the labels themselves), the borders between
        faces of one class dropped, the chains that meet two by two with equal classes joined"""
        return map_dissolve(handle, self.xy, self.n_points, self.row_index, self.left, self.right, self.n_chains, classes=classes, **kw)

    def Join(self, handle, **kw):
        """Dissolve with identity classes and keep_equal: no chain goes, the chains that meet two by two are joined"""
        return self.Dissolve(handle, None, keep_equal=True, **kw)

    def Neighbours(self, handle, vertex=False, **kw):
        """map_neighbours of this map, on the device, as a DeviceNeighbours: which faces touch which, along how much border
        and (vertex=True) at how many nodes, with the faces that meet only at a vertex"""
        return map_neighbours(handle, self.xy, self.n_points, self.row_index, self.left, self.right, self.n_chains, vertex=vertex, **kw)


class DeviceOutputMap(_ChainMapOps):
    """The overlay's output map in device memory (rj_overlay_map): xy (int64 x,y pairs, scaled units), row_index
    (uint32, n_chains + 1), left / right (int32 output face ids), face_pairs (int32 pairs: face k is face_pairs[k - 1])
    and origin (uint32: (im << 31) | source chain) as DeviceBuffers, the counts, and the flags it was computed under
    (drop_degenerate, merged)."""
    _buffers = ("xy", "row_index", "left", "right", "face_pairs", "origin")

    def __init__(self, xy, row_index, left, right, face_pairs, origin, counts, drop_degenerate, merged=False):
        self.xy, self.row_index, self.left, self.right, self.face_pairs, self.origin = xy, row_index, left, right, face_pairs, origin
        self.n_chains, self.n_points, self.n_faces = (int(v) for v in counts)
        self.drop_degenerate = bool(drop_degenerate)
        self.merged = bool(merged)

    def to_host(self):
        """-> (maps.ScaledMap of the output map, face_pairs int32 [n_faces, 2], origin uint32 [n_chains])"""
        return self._scaled_map(), self.face_pairs.to_host(np.int32, 2 * self.n_faces).reshape(-1, 2), self.origin.to_host(np.uint32, self.n_chains)


def map_crossings(handle, xy, n_points, row_index, n_chains, capacity=None):
    """The crossings inside one chain map in device memory (rj_map_crossings; xy int64 pairs, row_index uint32 as
    rj_upload_map_dev takes them; a chain may have a single point) -> (records, counts) on the host: records a
    CROSSING_DTYPE array, one per pair of edges that meets elsewhere than in a shared end point (eid[0] < eid[1], kind
    RJ_CROSS_PROPER / TOUCH / OVERLAP / EQUAL), ascending by (eid[0], eid[1]); counts a dict (CROSSINGS_COUNTS).  No
    record: the map is a planar subdivision.  capacity: CrossingsOverflow with the true counts when it is too small;
    left open, a sizing call finds it."""
    with _Owned(handle) as tmp:
        buf, counts = _crossings_on_device(tmp, xy, n_points, row_index, n_chains, capacity)
        return (np.zeros(0, _capi.CROSSING_DTYPE) if buf is None else buf.to_host(_capi.CROSSING_DTYPE, counts["n_found"])), counts


def _crossings_on_device(own, xy, n_points, row_index, n_chains, capacity=None):
    """map_crossings whose records stay on the device, in a buffer of `own` -> (a DeviceBuffer of counts["n_found"] records,
    counts); no buffer where a sizing call found no record"""
    args = (xy, n_points, row_index, n_chains)
    if capacity is None:
        c = _sizing_counts(own.handle.map_crossings, _capi.CrossingsOverflow, *args, 0, None)
        if c["n_found"] == 0:
            return None, c
        capacity = c["n_found"]
    capacity = int(capacity)
    buf = own.alloc(_capi.CROSSING_DTYPE.itemsize * max(1, capacity))
    return buf, own.handle.map_crossings(*args, capacity, buf)


def map_simplify(handle, xy, n_points, row_index, n_chains, tol, origin=False, capacity=None):
    """A chain map in device memory with its chains thinned by effective area (rj_map_simplify) as a DeviceSimplifiedMap.
    tol: a Python int in [0, 2^128), twice an area in scaled units^2 (the unit of FaceTable()'s area2): in rounds, every
    unpinned point whose triangle with its two neighbours has at most that doubled area goes, the least first.  The ends of
    every chain stay, and a closed chain keeps a triangle: chains, their number and their order do not change, and the
    caller's left / right arrays go with the result as they are.  origin: also the input point of every output point.
    capacity (points): SimplifyOverflow with the true counts when it is too small; left open, a sizing call finds it."""
    args = (xy, n_points, row_index, n_chains, tol)
    if capacity is None:
        capacity = _sizing_counts(handle.map_simplify, _capi.SimplifyOverflow, *args, 0, None, None)["n_points"]
    capacity = int(capacity)
    with _Owned(handle) as own:
        bufs = [own.alloc(16 * max(1, capacity)), own.alloc(4 * (int(n_chains) + 1)), own.alloc(4 * max(1, capacity)) if origin else None]
        counts = handle.map_simplify(*args, capacity, *bufs)
        own.release()
    return DeviceSimplifiedMap(*bufs, counts, n_chains)


class DeviceSimplifiedMap(_OwnsBuffers):
    """A thinned chain map in device memory (rj_map_simplify): xy (int64 x,y pairs), row_index (uint32, n_chains + 1) and,
    where asked for, origin (uint32 per output point: its input point) as DeviceBuffers, and the counts n_points,
    n_removed, n_rounds, n_closed, n_pinned_extra, n_max_round."""
    _buffers = ("xy", "row_index", "origin")

    def __init__(self, xy, row_index, origin, counts, n_chains):
        self.xy, self.row_index, self.origin = xy, row_index, origin
        self.counts = dict(counts)
        self.n_points, self.n_chains = int(counts["n_points"]), int(n_chains)

    def to_host(self):
        """-> (xy int64 [n_points, 2], row_index uint32 [n_chains + 1], origin uint32 [n_points] or None)"""
        return (self.xy.to_host(np.int64, 2 * self.n_points).reshape(-1, 2), self.row_index.to_host(np.uint32, self.n_chains + 1),
                self.origin.to_host(np.uint32, self.n_points) if self.origin is not None else None)


def _simplified_chain_map(handle, m, tol, check, capacity):
    """DeviceOutputMap.Simplify / DeviceChainMap.Simplify: the thinned map with device copies of m's left / right"""
    sm = map_simplify(handle, m.xy, m.n_points, m.row_index, m.n_chains, tol, capacity=capacity)
    with _Owned(handle) as own:
        own.bufs += [sm.xy, sm.row_index]  # (the thinned map's buffers become the chain map's)
        sides = [own.alloc(4 * max(1, m.n_chains)).from_device(b, 4 * m.n_chains) for b in (m.left, m.right)]
        counts = dict(sm.counts, n_chains=m.n_chains, n_edges=sm.n_points - m.n_chains)
        out = DeviceChainMap(sm.xy, sm.row_index, sides[0], sides[1], counts)
        res = (out, out.Crossings(handle)[1]) if check else out
        own.release()
    return res


def _records_on_device(own, xy, n_points, row_index, n_chains, records):
    """The records that map_node / map_snap take, in a temporary of `own` -> (a DeviceBuffer or None, their number).  records:
    the host CROSSING_DTYPE array, uploaded; None: rj_map_crossings runs here and its records stay on the device"""
    if records is None:
        rec, c = _crossings_on_device(own, xy, n_points, row_index, n_chains)
        return rec, c["n_found"]
    records = np.ascontiguousarray(records, dtype=_capi.CROSSING_DTYPE)
    n_rec = len(records)
    return (own.alloc(_capi.CROSSING_DTYPE.itemsize * n_rec).from_host(records) if n_rec else None), n_rec


def _cuts_call(call, overflow, handle, xy, n_points, row_index, n_chains, rec, n_rec, flags, edge_origin, capacity):
    """handle.map_node or handle.map_snap (call, with its overflow class) with the records in device memory (rec may be None
    with n_rec == 0) -> DeviceNodedMap.  capacity None: a sizing call finds it.  The three buffers are freed on an error"""
    args = (xy, n_points, row_index, n_chains, rec, n_rec, flags)
    if capacity is None:
        capacity = _sizing_counts(call, overflow, *args, 0, None, None)["n_points"]
    capacity = int(capacity)
    with _Owned(handle) as own:
        bufs = [own.alloc(16 * max(1, capacity)), own.alloc(4 * (int(n_chains) + 1)), own.alloc(4 * max(1, capacity)) if edge_origin else None]
        counts = call(*args, capacity, *bufs)
        own.release()
    return DeviceNodedMap(*bufs, counts, n_chains, bool(flags & _capi.RJ_NODE_DROP_LAST))  # (RJ_SNAP_DROP_LAST is the same bit)


def map_node(handle, xy, n_points, row_index, n_chains, records=None, drop_last=False, edge_origin=False, capacity=None):
    """A chain map in device memory with every edge cut at the vertices that lie inside it (rj_map_node) as a
    DeviceNodedMap: the exact repair of T-junctions and half-shared borders, the RJ_CROSS_TOUCH and RJ_CROSS_OVERLAP
    records of map_crossings.  records: the host CROSSING_DTYPE array that map_crossings returned for this very map; None:
    rj_map_crossings runs here and its records stay on the device.  Chains, their number and their order do not change: the
    caller's left / right arrays go with the result as they are.  drop_last (RJ_NODE_DROP_LAST) takes closed chains (first
    point == last) and writes each without its last point, the ring layout that rings_map takes.  edge_origin: also the
    input edge of every output edge.  counts["n_proper"]: the crossings that noding cannot repair.  capacity (points):
    NodeOverflow with the true counts when it is too small; left open, a sizing call finds it."""
    with _Owned(handle) as tmp:
        rec, n_rec = _records_on_device(tmp, xy, n_points, row_index, n_chains, records)
        return _cuts_call(handle.map_node, _capi.NodeOverflow, handle, xy, n_points, row_index, n_chains, rec, n_rec,
                          _capi.RJ_NODE_DROP_LAST if drop_last else 0, edge_origin, capacity)


def _snap_call(handle, xy, n_points, row_index, n_chains, rec, n_rec, flags, edge_origin, capacity):
    """rj_map_snap with the records in device memory (rec may be None with n_rec == 0) -> DeviceNodedMap"""
    return _cuts_call(handle.map_snap, _capi.SnapOverflow, handle, xy, n_points, row_index, n_chains, rec, n_rec, flags, edge_origin, capacity)


def map_snap(handle, xy, n_points, row_index, n_chains, records=None, drop_last=False, edge_origin=False, capacity=None):
    """map_node that also cuts at proper crossings (rj_map_snap), as a DeviceNodedMap with the wider counts (SNAP_COUNTS):
    every RJ_CROSS_PROPER record cuts both of its edges at the crossing point rounded to integers (halves toward
    +infinity), the other kinds cut as in map_node.  One call: the rounding can make new crossings -- map_snap_rounds
    repeats it.  records, drop_last, edge_origin, capacity: as map_node (SnapOverflow past the capacity)."""
    with _Owned(handle) as tmp:
        rec, n_rec = _records_on_device(tmp, xy, n_points, row_index, n_chains, records)
        return _snap_call(handle, xy, n_points, row_index, n_chains, rec, n_rec, _capi.RJ_SNAP_DROP_LAST if drop_last else 0, edge_origin, capacity)


def map_snap_rounds(handle, xy, n_points, row_index, n_chains, max_rounds=8, drop_last=False):
    """A chain map in device memory cut until it has no crossing left, or max_rounds times: map_crossings, then map_snap
    on its records, again on the result, every intermediate map freed.  It stops when a check finds no RJ_CROSS_PROPER,
    TOUCH or OVERLAP record (EQUAL records are edges stored twice: rings_map's business) or when max_rounds cutting
    calls were made; one last check then tells what is left.  -> a DeviceNodedMap with three more attributes: rounds, a
    list of dict(crossings=the check's counts, snap=the cut's counts) per cutting call; clean, whether the last check
    found nothing to cut; remaining, that last check's counts.  The rounds converge in practice (two or three on
    ordinary input) but nothing guarantees it: read clean.  edge_origin is not composed across rounds and not returned.
    drop_last: the input's chains are closed (first point == last) and stay so through every round -- each round's input
    is a valid map --; a final copying call (rj_map_snap with RJ_SNAP_DROP_LAST and no records) writes them without
    their last point, the ring layout rings_map takes.  Without a cutting round the result is such a copy as well: the
    caller owns it either way."""
    flags = _capi.RJ_SNAP_DROP_LAST if drop_last else 0
    rounds, cur = [], None
    try:
        while True:
            at = (xy, n_points, row_index) if cur is None else (cur.xy, cur.n_points, cur.row_index)
            with _Owned(handle) as tmp:
                rec, c = _crossings_on_device(tmp, at[0], at[1], at[2], n_chains)
                if c["n_proper"] + c["n_touch"] + c["n_overlap"] == 0 or len(rounds) >= max_rounds:
                    break
                nm = _snap_call(handle, at[0], at[1], at[2], n_chains, rec, c["n_found"], 0, False, None)
            rounds.append(dict(crossings=c, snap=nm.counts))
            if cur is not None:
                cur.free()
            cur = nm
        if cur is None or drop_last:
            at = (xy, n_points, row_index) if cur is None else (cur.xy, cur.n_points, cur.row_index)
            nm = _snap_call(handle, at[0], at[1], at[2], n_chains, None, 0, flags, False, None)
            if cur is not None:
                cur.free()
            cur = nm
    except BaseException:
        if cur is not None:
            cur.free()
        raise
    cur.rounds, cur.clean, cur.remaining = rounds, c["n_proper"] + c["n_touch"] + c["n_overlap"] == 0, c
    return cur


class DeviceNodedMap(_OwnsBuffers):
    """A noded chain map in device memory (rj_map_node): xy (int64 x,y pairs), row_index (uint32, n_chains + 1) and, where
    asked for, edge_origin (uint32 per output edge: its input edge) as DeviceBuffers, the counts n_points, n_edges, n_cuts,
    n_cut_edges, n_max_cuts, n_used, n_proper, n_equal (from map_snap also n_exact, n_at_end, n_stale), and drop_last: the
    chains are rings without their closing point.  From map_snap_rounds also rounds, clean and remaining."""
    _buffers = ("xy", "row_index", "edge_origin")

    def __init__(self, xy, row_index, edge_origin, counts, n_chains, drop_last=False):
        self.xy, self.row_index, self.edge_origin = xy, row_index, edge_origin
        self.counts = dict(counts)
        self.n_points, self.n_chains, self.n_edges = int(counts["n_points"]), int(n_chains), int(counts["n_edges"])
        self.drop_last = bool(drop_last)

    def to_host(self):
        """-> (xy int64 [n_points, 2], row_index uint32 [n_chains + 1], edge_origin uint32 [n_edges] or None)"""
        return (self.xy.to_host(np.int64, 2 * self.n_points).reshape(-1, 2), self.row_index.to_host(np.uint32, self.n_chains + 1),
                self.edge_origin.to_host(np.uint32, self.n_edges) if self.edge_origin is not None else None)

    def Faces(self, handle, left=None, right=None):
        """map_faces of this map, on the device: the faces of the noded linework from its geometry alone, as a DeviceFacedMap.
        left / right (device int32 arrays, both or neither): the caller's labels, which noding left valid, to check"""
        if (left is None) != (right is None):
            raise ValueError("left and right go together")
        return map_faces(handle, self.xy, self.n_points, self.row_index, self.n_chains, labels=None if left is None else (left, right))

    def Snap(self, handle, **kw):
        """map_snap_rounds of this map (not one written with drop_last: its chains must be whole): the proper crossings
        that noding left are cut in rounds"""
        if self.drop_last:
            raise ValueError("a map written with drop_last has no closing points: snap before dropping them")
        return map_snap_rounds(handle, self.xy, self.n_points, self.row_index, self.n_chains, **kw)


def _stage_closed_rings(own, ring_row, ring_xy):
    """Host rings closed into chains (maps.closed_chains_of_rings) in temporaries of `own` -> (xy, n_points, row_index, n_chains)"""
    from .maps import closed_chains_of_rings
    row, xy = closed_chains_of_rings(ring_row, ring_xy)
    return own.alloc(16 * max(1, len(xy))).from_host(xy), len(xy), own.alloc(4 * len(row)).from_host(row), len(row) - 1


def node_rings(handle, ring_row, ring_xy):
    """Host rings (ring_row uint32 CSR, ring_xy int64 pairs: maps.rings_of_polygons) noded against each other on the
    device: closed into chains (maps.closed_chains_of_rings), uploaded, map_crossings, map_node with drop_last ->
    (ring_row buffer, ring_xy buffer, n_points, counts), ready for rings_map with the caller's unchanged ring_face.
    counts["n_proper"] is what noding could not repair: rings that cross each other properly."""
    with _Owned(handle) as tmp:
        nm = map_node(handle, *_stage_closed_rings(tmp, ring_row, ring_xy), drop_last=True)
    return nm.row_index, nm.xy, nm.n_points, nm.counts


def snap_rings(handle, ring_row, ring_xy, max_rounds=8):
    """node_rings for rings that may cross each other or themselves: closed into chains, uploaded, map_snap_rounds with
    drop_last -> (ring_row buffer, ring_xy buffer, n_points, clean, rounds), the first three ready for rings_map with the
    caller's unchanged ring_face -- where polygons overlapped, the labels of the chain map that comes out conflict
    (its counts tell) and map_faces labels the linework from its geometry.  clean / rounds: as map_snap_rounds."""
    with _Owned(handle) as tmp:
        nm = map_snap_rounds(handle, *_stage_closed_rings(tmp, ring_row, ring_xy), max_rounds=max_rounds, drop_last=True)
    return nm.row_index, nm.xy, nm.n_points, nm.clean, nm.rounds


def face_rings(handle, xy, n_points, row_index, left, right, n_chains, skip_face0=False, points=True, capacities=None):
    """The rings of a chain map in device memory (rj_map_rings; the arrays as rj_upload_map_dev takes them: int64 xy,
    uint32 row_index, int32 left / right) as a DeviceRings.  skip_face0 leaves out the rings of face 0 (the outside);
    points=False leaves out the points (ring_row, ring_xy).  capacities = (rings, half-chains, points): RingsOverflow with
    the true counts when one is too small; left open, a sizing call finds them."""
    flags = (_capi.RJ_RINGS_SKIP_FACE0 if skip_face0 else 0) | (0 if points else _capi.RJ_RINGS_NO_POINTS)
    args = (xy, n_points, row_index, left, right, n_chains, flags)
    if capacities is None:
        c = _sizing_counts(handle.map_rings, _capi.RingsOverflow, *args, (0, 0, 0), None, None, None, None, None)
        capacities = (c["n_rings"], c["n_halves"], c["n_points"])
    rc, hc, pc = (int(v) for v in capacities)
    with _Owned(handle) as own:
        bufs = [own.alloc(_capi.RING_DTYPE.itemsize * max(1, rc)), own.alloc(4 * (rc + 1)), own.alloc(4 * max(1, hc)),
                own.alloc(4 * (rc + 1)) if points else None, own.alloc(16 * max(1, pc)) if points else None]
        counts = handle.map_rings(*args, (rc, hc, pc), *bufs)
        own.release()
    return DeviceRings(*bufs, counts)


class DeviceRings(_OwnsBuffers):
    """The rings of a chain map in device memory (rj_map_rings): rings (RING_DTYPE rows, ascending by (face, leader)),
    ring_first (uint32 CSR of the rings into ring_half), ring_half (uint32 half-chains: 2 c = chain c forward, 2 c + 1
    backward), ring_row (uint32 CSR into ring_xy) and ring_xy (int64 x,y pairs, scaled units) as DeviceBuffers -- the last
    two None without points -- and the counts n_rings, n_halves, n_points, n_mixed, n_skipped."""
    _buffers = ("rings", "ring_first", "ring_half", "ring_row", "ring_xy")

    def __init__(self, rings, ring_first, ring_half, ring_row, ring_xy, counts):
        self.rings, self.ring_first, self.ring_half, self.ring_row, self.ring_xy = rings, ring_first, ring_half, ring_row, ring_xy
        self.counts = dict(counts)
        for name in _capi.RINGS_COUNTS:
            setattr(self, name, int(counts[name]))

    def to_host(self):
        """-> dict(rings, ring_first, ring_half, ring_row, ring_xy [n_points, 2], counts); ring_row / ring_xy None without points"""
        n = self.n_rings
        return dict(rings=self.rings.to_host(_capi.RING_DTYPE, n), ring_first=self.ring_first.to_host(np.uint32, n + 1),
                    ring_half=self.ring_half.to_host(np.uint32, self.n_halves),
                    ring_row=self.ring_row.to_host(np.uint32, n + 1) if self.ring_row is not None else None,
                    ring_xy=self.ring_xy.to_host(np.int64, 2 * self.n_points).reshape(-1, 2) if self.ring_xy is not None else None,
                    counts=dict(self.counts))

    def polygons(self, scaling=None):
        """{face: [(area2, points[n, 2]), ...]} on the host, the rings of a face in ring order: area2 exact (a Python int, in
        scaled units^2; positive = outer boundary, negative = hole), the points scaled integers, or input coordinates
        when the map's maps.Scaling is given"""
        if self.ring_xy is None:
            raise RuntimeError("DeviceRings.polygons needs the points (points=True)")
        host = self.to_host()
        out = {}
        row = host["ring_row"].astype(np.int64)
        for k, g in enumerate(host["rings"]):
            pts = host["ring_xy"][row[k]:row[k + 1]]
            if scaling is not None:
                pts = scaling.unscale(pts)
            out.setdefault(int(g["face"]), []).append(((int(g["area2_hi"]) << 64) | int(g["area2_lo"]), pts))
        return out

    def Polygons(self, handle, capacities=None):
        """The polygons of these rings as a DevicePolygons (rj_rings_polygons): every hole assigned to the outer ring it
        lies in, on the device.  Needs the points.  capacities = (polygons, members): PolygonsOverflow with the true
        counts when one is too small; left open, a sizing call finds them."""
        if self.ring_xy is None:
            raise RuntimeError("DeviceRings.Polygons needs the points (points=True)")
        args = (self.rings, self.n_rings, self.ring_row, self.ring_xy, self.n_points, 0)
        if capacities is None:
            c = _sizing_counts(handle.rings_polygons, _capi.PolygonsOverflow, *args, (0, 0), None, None, None, None)
            capacities = (c["n_polygons"], c["n_members"])
        pc, mc = (int(v) for v in capacities)
        with _Owned(handle) as own:
            bufs = [own.alloc(4 * max(1, self.n_rings)), own.alloc(_capi.POLYGON_DTYPE.itemsize * max(1, pc)), own.alloc(4 * (pc + 1)),
                    own.alloc(4 * max(1, mc))]
            counts = handle.rings_polygons(*args, (pc, mc), *bufs)
            own.release()
        return DevicePolygons(*bufs, self.n_rings, counts)

    def Map(self, handle, dissolve=False):
        """The chain map that these rings bound as a DeviceChainMap (rings_map): chains as long as the faces allow, whatever
        pieces the map they came from was cut into.  Reads the faces of the ring records in place.  Needs the points."""
        if self.ring_xy is None:
            raise RuntimeError("DeviceRings.Map needs the points (points=True)")
        return rings_map(handle, self.ring_row, self.ring_xy, self.n_points, self.rings, self.n_rings, face_stride=_capi.RING_DTYPE.itemsize,
                         dissolve=dissolve)


def rings_map(handle, ring_row, ring_xy, n_points, ring_face, n_rings, face_stride=4, dissolve=False, capacities=None):
    """The chain map that labelled rings bound (rj_rings_map, the inverse of face_rings) as a DeviceChainMap: ring_row (uint32
    CSR, n_rings + 1), ring_xy (int64 x,y pairs, scaled units) and ring_face in device memory; the face of ring r is the
    int32 at byte r * face_stride of ring_face (4: a plain int32 array, 32: RING_DTYPE records in place) and lies on the left
    of the ring's walk (shells counter-clockwise, holes clockwise: maps.rings_of_polygons).  dissolve (RJ_RMAP_DISSOLVE)
    leaves out every edge with the same face on both sides.  capacities = (chains, points): RingsMapOverflow with the
    true counts when one is too small; left open, a sizing call finds them."""
    flags = _capi.RJ_RMAP_DISSOLVE if dissolve else 0
    args = (ring_row, ring_xy, n_points, ring_face, face_stride, n_rings, flags)
    if capacities is None:
        c = _sizing_counts(handle.rings_map, _capi.RingsMapOverflow, *args, (0, 0), None, None, None, None)
        capacities = (c["n_chains"], c["n_points"])
    cc, pc = (int(v) for v in capacities)
    with _Owned(handle) as own:
        bufs = [own.alloc(16 * max(1, pc)), own.alloc(4 * (cc + 1)), own.alloc(4 * max(1, cc)), own.alloc(4 * max(1, cc))]
        counts = handle.rings_map(*args, (cc, pc), *bufs)
        own.release()
    return DeviceChainMap(*bufs, counts)


class DeviceChainMap(_ChainMapOps):
    """The chain map of a set of labelled rings in device memory (rj_rings_map): xy (int64 x,y pairs, scaled units),
    row_index (uint32, n_chains + 1), left / right (int32 faces) as DeviceBuffers -- the arrays rj_upload_map_dev takes, so
    DeviceContext.InstallMap takes it as it takes a DeviceOutputMap -- and the counts n_chains, n_points, n_edges, n_closed,
    n_zero_edges, n_conflicts, n_dissolved."""
    _buffers = ("xy", "row_index", "left", "right")

    def __init__(self, xy, row_index, left, right, counts):
        self.xy, self.row_index, self.left, self.right = xy, row_index, left, right
        self.counts = dict(counts)
        self.n_chains, self.n_points = int(counts["n_chains"]), int(counts["n_points"])

    def to_host(self):
        """-> (maps.ScaledMap of the map, the counts)"""
        return self._scaled_map(), dict(self.counts)

    def Faces(self, handle, check=False):
        """map_faces of this map, on the device: its faces computed from the geometry alone, as a DeviceFacedMap of its own.
        check: this map's own left / right go in as the labels to check -- counts["n_conflicts"] == 0 tells that they and
        the geometry describe the same partition, and the records' label is the given label of every computed face"""
        return map_faces(handle, self.xy, self.n_points, self.row_index, self.n_chains, labels=(self.left, self.right) if check else None)


def map_faces(handle, xy, n_points, row_index, n_chains, labels=None, records=True):
    """The faces of a chain map in device memory computed from its geometry alone (rj_map_faces; int64 xy, uint32
    row_index, no labels needed) as a DeviceFacedMap: a DeviceChainMap with copies of xy / row_index whose left / right are
    the computed faces -- 0 the unbounded face, k the k-th bounded face by its outer ring's leader half-chain -- so Rings(),
    Crossings(), Simplify() and DeviceContext.InstallMap take it.  labels = (left, right) device arrays: the labels to
    check, counts["n_conflicts"] the half-chains whose given label is not that of their computed face.  records: also the
    face records (.faces, MAP_FACE_DTYPE rows: leader, n_holes, label, area2).  One call of rj_map_faces either way: the
    records are written into room for 2 n_chains of them (no map has more rings; 64 bytes per chain until the call
    returns) and copied to a buffer of their own size.  counts: MAP_FACES_COUNTS with n_chains, n_points, n_edges.
    The grid of rj_map_faces has cells of at least 2^15 units: coordinates are expected scaled to the range, a map drawn
    in single units gets the same faces at the cost of every hole against every edge (rj_faces.h, UNITS)."""
    n_points, n_chains = int(n_points), int(n_chains)
    in_left, in_right = labels if labels is not None else (None, None)
    rec = _capi.MAP_FACE_DTYPE.itemsize
    faces = None
    with _Owned(handle) as own, _Owned(handle) as tmp:
        bufs = [own.alloc(16 * max(1, n_points)).from_device(xy, 16 * n_points), own.alloc(4 * (n_chains + 1)), own.alloc(4 * max(1, n_chains)),
                own.alloc(4 * max(1, n_chains))]
        if n_chains:
            bufs[1].from_device(row_index, 4 * (n_chains + 1))
        else:
            bufs[1].from_host(np.zeros(1, np.uint32))
        room = tmp.alloc(rec * max(1, 2 * n_chains)) if records else None
        counts = handle.map_faces(bufs[0], n_points, bufs[1], n_chains, bufs[2], bufs[3], room, 2 * n_chains, in_left, in_right)
        if records:
            faces = own.alloc(rec * max(1, counts["n_faces"]))
            if counts["n_faces"]:
                faces.from_device(room, rec * counts["n_faces"])
        own.release()
    return DeviceFacedMap(*bufs, dict(counts, n_chains=n_chains, n_points=n_points, n_edges=n_points - n_chains), faces)


class DeviceFacedMap(DeviceChainMap):
    """A chain map in device memory whose left / right are the faces that rj_map_faces computed, with faces (MAP_FACE_DTYPE rows
    as a DeviceBuffer, or None) and the counts n_faces, n_rings, n_holes, n_outer, n_skipped, n_dangling, n_conflicts."""
    _buffers = DeviceChainMap._buffers + ("faces",)

    def __init__(self, xy, row_index, left, right, counts, faces):
        super().__init__(xy, row_index, left, right, counts)
        self.faces, self.n_faces = faces, int(counts["n_faces"])

    def faces_to_host(self):
        """-> the face records (MAP_FACE_DTYPE), record k - 1 for face k"""
        return self.faces.to_host(_capi.MAP_FACE_DTYPE, self.n_faces)


def map_eliminate(handle, xy, n_points, row_index, left, right, n_chains, tol, drop=True, faces=False):
    """A labelled chain map in device memory with its sliver faces merged into a neighbour (rj_map_eliminate) as a
    DeviceEliminatedMap.  tol: a Python int in [0, 2^128), twice an area in scaled units^2: a face (a label other than 0)
    whose area2 lies in [0, tol] joins the neighbour it shares the longest border with -- ties to the smaller pair of
    labels, unsigned; two slivers that choose each other merge into the larger; chains of choices are followed to their
    root.  One call is one round: a merged group may still be at most tol (map_eliminate_rounds repeats).  drop
    (RJ_ELIM_DROP): the chains whose two labels became equal are left out, .origin holds the input chain of every output
    chain; without it the map keeps its chains and only left / right change (xy / row_index are copies).  faces: also the
    face records (.faces, ELIM_FACE_DTYPE rows ascending by unsigned label: label, target, best, flags, area2).  A sizing
    call finds the capacities.  counts: ELIMINATE_COUNTS with n_edges."""
    n_points, n_chains = int(n_points), int(n_chains)
    flags = _capi.RJ_ELIM_DROP if drop else 0
    args = (xy, n_points, row_index, left, right, n_chains, tol)
    c = _sizing_counts(handle.map_eliminate, _capi.EliminateOverflow, *args, (0, 0, 0), None, None, flags=flags)
    fc, cc, pc = c["n_faces"] if faces else 0, c["n_chains"], c["n_points"]
    origin = None
    with _Owned(handle) as own:
        bufs = [own.alloc(16 * max(1, pc)), own.alloc(4 * (cc + 1)), own.alloc(4 * max(1, cc)), own.alloc(4 * max(1, cc))]
        if drop:
            origin = own.alloc(4 * max(1, cc))
        else:
            if n_points:
                bufs[0].from_device(xy, 16 * n_points)
            if n_chains:
                bufs[1].from_device(row_index, 4 * (n_chains + 1))
        if not n_chains:
            bufs[1].from_host(np.zeros(1, np.uint32))
        records = own.alloc(_capi.ELIM_FACE_DTYPE.itemsize * max(1, fc)) if faces else None
        counts = handle.map_eliminate(*args, (fc, cc, pc), bufs[2], bufs[3], bufs[0] if drop else None, bufs[1] if drop else None, origin, records,
                                      flags=flags)
        own.release()
    return DeviceEliminatedMap(*bufs, dict(counts, n_edges=counts["n_points"] - counts["n_chains"]), records, origin)


def map_eliminate_rounds(handle, xy, n_points, row_index, left, right, n_chains, tol, max_rounds=8, faces=False):
    """map_eliminate with drop, repeated on its own result until a round has n_eliminated == 0 or max_rounds is hit -> the
    last round's DeviceEliminatedMap with .rounds, the counts of every round that ran (the last one eliminated nothing
    where the rounds ended: .rounds[-1]["n_eliminated"] == 0).  .origin is the last round's (chains of the round before)."""
    per_round, m = [], None
    args = (xy, n_points, row_index, left, right, n_chains)
    for _ in range(max(1, int(max_rounds))):
        nxt = map_eliminate(handle, *args, tol, drop=True, faces=faces)
        if m is not None:
            m.free()
        m = nxt
        per_round.append(dict(m.counts))
        if m.counts["n_eliminated"] == 0:
            break
        args = (m.xy, m.n_points, m.row_index, m.left, m.right, m.n_chains)
    m.rounds = per_round
    return m


class DeviceEliminatedMap(DeviceChainMap):
    """A chain map in device memory whose left / right are the targets that rj_map_eliminate gave, with faces
    (ELIM_FACE_DTYPE rows as a DeviceBuffer, or None), origin (uint32 per chain: its input chain; None without drop) and the
    counts n_faces, n_slivers, n_eliminated, n_islands, n_mutual, n_negative, n_chains, n_points, n_dropped, n_edges."""
    _buffers = DeviceChainMap._buffers + ("faces", "origin")

    def __init__(self, xy, row_index, left, right, counts, faces, origin):
        super().__init__(xy, row_index, left, right, counts)
        self.faces, self.origin, self.n_faces = faces, origin, int(counts["n_faces"])
        self.rounds = [dict(counts)]

    def faces_to_host(self):
        """-> the face records (ELIM_FACE_DTYPE), ascending by unsigned label"""
        return self.faces.to_host(_capi.ELIM_FACE_DTYPE, self.n_faces)

    def origin_to_host(self):
        return self.origin.to_host(np.uint32, self.n_chains)


def map_dissolve(handle, xy, n_points, row_index, left, right, n_chains, classes=None, keep_equal=False, records=False, origin=False):
    """A labelled chain map in device memory with its faces merged by class and its chains re-joined (rj_map_dissolve) as a
    DeviceDissolvedMap.  classes: an int32 table indexed by label (class of label f = classes[f], label 0 stays 0, a nonzero
    class may be 0: the face joins the outside), a DeviceBuffer (all of it), (device array, n_labels) or a numpy array;
    None: the labels themselves.  A chain whose two classes are equal is dropped unless keep_equal (RJ_DISS_KEEP_EQUAL:
    join only, nothing dissolves); the kept chains that meet two by two with the same classes become one chain, loops
    close.  left / right of the result are classes.  records: also the class records (.classes, DISS_CLASS_DTYPE rows
    ascending by unsigned label: label, n_sides, area2).  origin: also .origin (the leader's input chain of every output
    chain) and .chain_out ((k << 1) | reversed per input chain, 0xFFFFFFFF for a chain that went).  A sizing call finds
    the capacities.  counts: DISSOLVE_COUNTS with n_edges."""
    n_points, n_chains = int(n_points), int(n_chains)
    flags = _capi.RJ_DISS_KEEP_EQUAL if keep_equal else 0
    table, n_labels = None, 0
    with _Owned(handle) as own, _Owned(handle) as tmp:
        if isinstance(classes, tuple):
            table, n_labels = classes[0], int(classes[1])
        elif isinstance(classes, _capi.DeviceBuffer):
            table, n_labels = classes, classes.nbytes // 4
        elif classes is not None:
            host = np.ascontiguousarray(classes, np.int32)
            if host.ndim != 1 or len(host) == 0:
                raise ValueError("classes must be a one-dimensional table with an entry for label 0")
            table, n_labels = tmp.alloc(4 * len(host)).from_host(host), len(host)
        args = (xy, n_points, row_index, left, right, n_chains, table, n_labels)
        c = _sizing_counts(handle.map_dissolve, _capi.DissolveOverflow, *args, (0, 0, 0), None, None, None, None, flags=flags)
        kc, cc, pc = c["n_classes"] if records else 0, c["n_chains"], c["n_points"]
        bufs = [own.alloc(16 * max(1, pc)), own.alloc(4 * (cc + 1)), own.alloc(4 * max(1, cc)), own.alloc(4 * max(1, cc))]
        org, cout = (own.alloc(4 * max(1, cc)), own.alloc(4 * max(1, n_chains))) if origin else (None, None)
        recs = own.alloc(_capi.DISS_CLASS_DTYPE.itemsize * max(1, kc)) if records else None
        counts = handle.map_dissolve(*args, (kc, cc, pc), bufs[2], bufs[3], bufs[0], bufs[1], org, cout, recs, flags=flags)
        own.release()
    return DeviceDissolvedMap(*bufs, dict(counts, n_edges=counts["n_points"] - counts["n_chains"]), recs, org, cout, n_chains)


class DeviceDissolvedMap(DeviceChainMap):
    """A chain map in device memory whose left / right are the classes that rj_map_dissolve gave, with classes
    (DISS_CLASS_DTYPE rows as a DeviceBuffer, or None), origin (uint32 per chain: its leader's input chain, or None),
    chain_out (uint32 per INPUT chain, or None) and the counts n_kept, n_dropped, n_skipped, n_chains, n_points, n_closed,
    n_classes, n_unmapped, n_edges."""
    _buffers = DeviceChainMap._buffers + ("classes", "origin", "chain_out")

    def __init__(self, xy, row_index, left, right, counts, classes, origin, chain_out, n_input_chains):
        super().__init__(xy, row_index, left, right, counts)
        self.classes, self.origin, self.chain_out = classes, origin, chain_out
        self.n_classes, self.n_input_chains = int(counts["n_classes"]), int(n_input_chains)

    def classes_to_host(self):
        """-> the class records (DISS_CLASS_DTYPE), ascending by unsigned label"""
        return self.classes.to_host(_capi.DISS_CLASS_DTYPE, self.n_classes)

    def origin_to_host(self):
        return self.origin.to_host(np.uint32, self.n_chains)

    def chain_out_to_host(self):
        return self.chain_out.to_host(np.uint32, self.n_input_chains)


def map_neighbours(handle, xy, n_points, row_index, left, right, n_chains, vertex=False, records=True):
    """The face adjacency table of a labelled chain map in device memory (rj_map_neighbours) as a DeviceNeighbours, in CSR
    form over the faces (the nonzero labels, ascending as unsigned numbers): per face its neighbours with the integer
    length w of the shared border, the chains n_chains that make it and, with vertex (RJ_NB_VERTEX), the nodes n_nodes
    where the two meet -- a node is a chain end, so the map should be noded, and joined (Join) where pseudo-nodes matter;
    neighbours with n_chains == 0 meet only at a vertex.  records: also the face records (.faces, NB_FACE_DTYPE rows:
    label, n_sides, n_edge_nbrs, n_vertex_nbrs, area2, perimeter, outer).  A sizing call finds the capacities."""
    n_points, n_chains = int(n_points), int(n_chains)
    flags = _capi.RJ_NB_VERTEX if vertex else 0
    args = (xy, n_points, row_index, left, right, n_chains)
    c = _sizing_counts(handle.map_neighbours, _capi.NeighboursOverflow, *args, (0, 0), flags=flags)
    fc, ec = c["n_faces"], c["n_entries"]
    with _Owned(handle) as own:
        faces = own.alloc(_capi.NB_FACE_DTYPE.itemsize * max(1, fc)) if records else None
        offsets = own.alloc(8 * (fc + 1))
        entries = own.alloc(_capi.NB_ENTRY_DTYPE.itemsize * max(1, ec))
        counts = handle.map_neighbours(*args, (fc, ec), faces, offsets, entries, flags=flags)
        own.release()
    return DeviceNeighbours(faces, offsets, entries, counts)


class DeviceNeighbours(_OwnsBuffers):
    """The face adjacency table of a chain map in device memory (rj_map_neighbours): faces (NB_FACE_DTYPE rows as a
    DeviceBuffer, or None), offsets (uint64 [n_faces + 1]), entries (NB_ENTRY_DTYPE rows) and the counts n_faces, n_entries,
    n_edge_pairs, n_vertex_pairs, n_nodes, n_node_pairs_raw, max_labels_at_node."""
    _buffers = ("faces", "offsets", "entries")

    def __init__(self, faces, offsets, entries, counts):
        self.faces, self.offsets, self.entries = faces, offsets, entries
        self.counts = dict(counts)
        self.n_faces, self.n_entries = int(counts["n_faces"]), int(counts["n_entries"])

    def faces_to_host(self):
        """-> the face records (NB_FACE_DTYPE), ascending by unsigned label; ValueError for a table made with records=False"""
        if self.faces is None:
            raise ValueError("this table was made with records=False: it has no face records")
        return self.faces.to_host(_capi.NB_FACE_DTYPE, self.n_faces)

    def to_host(self):
        """-> (offsets uint64 [n_faces + 1], entries NB_ENTRY_DTYPE [n_entries])"""
        return self.offsets.to_host(np.uint64, self.n_faces + 1), self.entries.to_host(_capi.NB_ENTRY_DTYPE, self.n_entries)

    def to_csr(self):
        """-> (indptr int64 [n_faces + 1], indices int64 [n_entries]: the neighbours' face numbers, the entries themselves):
        what scipy.sparse.csr_matrix((weights, indices, indptr)) takes, with any column of the entries as the weights"""
        offsets, entries = self.to_host()
        return offsets.astype(np.int64), entries["face"].astype(np.int64), entries

    def labels(self, handle):
        """-> the labels of the face records as a device int32 array (a DeviceBuffer with .count = n_faces), copied out of the
        records on the device: what face_points and PIPLBVH.Summarize take as faces=.  The caller frees it."""
        if self.faces is None:
            raise ValueError("this table was made with records=False: it has no face records")
        out = handle.alloc(4 * max(1, self.n_faces))
        out.count = self.n_faces
        handle.neighbours_labels(self.faces, self.n_faces, out)
        return out


def face_points(handle, labels, n, values=None, value_stride=1, faces=None, members=False, records=True):
    """Per-face counts, sums and members of n located points in device memory (rj_face_points) as a DeviceFacePoints.
    labels: int32 per point, what a PIP query wrote (PIPLBVH.faces).  values: int64 in device memory, the value of point i
    at values[i * value_stride]; None: counts only.  faces: the universe -- a device int32 array with a .count, or a
    (device array, count) pair, strictly ascending as unsigned numbers and without 0 (DeviceNeighbours.labels); None: the
    distinct nonzero labels of the points.  members (RJ_FP_MEMBERS): also the CSR of the points of every face.  records:
    the face records (.faces, FP_FACE_DTYPE rows: label, first, n_points, sum, min, max).  A sizing call finds the capacities."""
    n = int(n)
    flags = _capi.RJ_FP_MEMBERS if members else 0
    universe, n_universe = (None, 0) if faces is None else (tuple(faces) if isinstance(faces, (tuple, list)) else (faces, faces.count))
    kw = dict(value_dev=values, value_stride=value_stride, face_label_dev=universe, n_face_labels=n_universe, flags=flags)
    c = _sizing_counts(handle.face_points, _capi.FacePointsOverflow, labels, n, (0, 0), **kw)
    fc, mc = c["n_faces"], c["n_members"] if members else 0
    with _Owned(handle) as own:
        recs = own.alloc(_capi.FP_FACE_DTYPE.itemsize * max(1, fc)) if records else None
        offsets, mem = (own.alloc(8 * (fc + 1)), own.alloc(4 * max(1, mc))) if members else (None, None)
        if records or members:
            counts = handle.face_points(labels, n, (fc, mc), faces_dev=recs, offsets_dev=offsets, members_dev=mem, **kw)
        else:  # (neither records nor members: the counts are all there is, and the call may raise them again)
            counts = _sizing_counts(handle.face_points, _capi.FacePointsOverflow, labels, n, (0, mc), faces_dev=None, offsets_dev=None,
                                    members_dev=None, **kw)
        own.release()
    return DeviceFacePoints(recs, offsets, mem, counts)


class DeviceFacePoints(_OwnsBuffers):
    """Per-face counts, sums and members of located points in device memory (rj_face_points): faces (FP_FACE_DTYPE rows as a
    DeviceBuffer, or None), under members offsets (uint64 [n_faces + 1]) and members (uint32 point numbers, ascending
    inside every face), else None, and the counts n_faces, n_members, n_outside, n_unmatched, n_runs."""
    _buffers = ("faces", "offsets", "members")

    def __init__(self, faces, offsets, members, counts):
        self.faces, self.offsets, self.members = faces, offsets, members
        self.counts = dict(counts)
        self.n_faces, self.n_members = int(counts["n_faces"]), int(counts["n_members"])

    def faces_to_host(self):
        """-> the face records (FP_FACE_DTYPE), ascending by unsigned label; ValueError for a table made with records=False"""
        if self.faces is None:
            raise ValueError("this table was made with records=False: it has no face records")
        return self.faces.to_host(_capi.FP_FACE_DTYPE, self.n_faces)

    def to_host(self):
        """-> (offsets uint64 [n_faces + 1], members uint32 [n_members]); ValueError for a table made without members"""
        if self.offsets is None:
            raise ValueError("this table was made with members=False: it has no member lists")
        return self.offsets.to_host(np.uint64, self.n_faces + 1), self.members.to_host(np.uint32, self.n_members)

    def to_csr(self):
        """-> (indptr int64 [n_faces + 1], indices int64 [n_members]: the point numbers): the faces x points incidence matrix
        as scipy.sparse.csr_matrix((ones, indices, indptr)) takes it"""
        offsets, members = self.to_host()
        return offsets.astype(np.int64), members.astype(np.int64)

    def sums(self):
        """-> the exact int128 sums of the faces as a list of Python ints"""
        f = self.faces_to_host()
        return [(int(hi) << 64) + int(lo) for lo, hi in zip(f["sum_lo"], f["sum_hi"])]


class DevicePolygons(_OwnsBuffers):
    """The polygons of a DeviceRings in device memory (rj_rings_polygons): parent (uint32 per ring: the shell's ring index
    for a hole, its own for a shell, RJ_POLY_NONE for a ring of face 0 and for an orphan), polygons (POLYGON_DTYPE rows,
    ascending by shell), poly_first (uint32 CSR of the polygons into poly_ring) and poly_ring (uint32 ring indices: the
    shell, then its holes) as DeviceBuffers, and the counts n_polygons, n_members, n_holes, n_orphans, n_face0."""
    _buffers = ("parent", "polygons_", "poly_first", "poly_ring")

    def __init__(self, parent, polygons, poly_first, poly_ring, n_rings, counts):
        self.parent, self.polygons_, self.poly_first, self.poly_ring = parent, polygons, poly_first, poly_ring
        self.n_rings = int(n_rings)
        self.counts = dict(counts)
        for name in _capi.POLYGONS_COUNTS:
            setattr(self, name, int(counts[name]))

    def to_host(self):
        """-> dict(parent, polygons, poly_first, poly_ring, counts)"""
        n = self.n_polygons
        return dict(parent=self.parent.to_host(np.uint32, self.n_rings), polygons=self.polygons_.to_host(_capi.POLYGON_DTYPE, n),
                    poly_first=self.poly_first.to_host(np.uint32, n + 1), poly_ring=self.poly_ring.to_host(np.uint32, self.n_members),
                    counts=dict(self.counts))

    def polygons(self, rings, scaling=None):
        """[(face, area2, shell_points[n, 2], [hole_points, ...])] on the host, in polygon order, of the DeviceRings these
        polygons were computed from: area2 exact (a Python int, scaled units^2), the points scaled integers, or input
        coordinates when the map's maps.Scaling is given"""
        host, rh = self.to_host(), rings.to_host()
        row = rh["ring_row"].astype(np.int64)

        def points(r):
            pts = rh["ring_xy"][row[r]:row[r + 1]]
            return scaling.unscale(pts) if scaling is not None else pts

        first, out = host["poly_first"].astype(np.int64), []
        for k, g in enumerate(host["polygons"]):
            members = host["poly_ring"][first[k]:first[k + 1]].tolist()
            out.append((int(g["face"]), (int(g["area2_hi"]) << 64) | int(g["area2_lo"]), points(members[0]), [points(r) for r in members[1:]]))
        return out


def overlay_op(how, by):
    """(how, by) names -> the RJ_OV_* pair of the _op calls; None for the defaults (the calls without _op)"""
    if how not in _capi.OVERLAY_HOW:
        raise ValueError("how must be one of %s, not %r" % (sorted(_capi.OVERLAY_HOW), how))
    if by not in _capi.OVERLAY_BY:
        raise ValueError("by must be one of %s, not %r" % (sorted(_capi.OVERLAY_BY), by))
    if how == "intersection" and by == "pair":
        return None
    return _capi.OVERLAY_HOW[how], _capi.OVERLAY_BY[by]


def face_table_from_rows(raw, scaling):
    """FACE_DTYPE rows -> FACE_TABLE_DTYPE (exact area2 as Python ints, area in input units)"""
    t = np.empty(len(raw), dtype=FACE_TABLE_DTYPE)
    t["face0"] = raw["face"][:, 0]
    t["face1"] = raw["face"][:, 1]
    a2 = [(int(hi) << 64) | int(lo) for lo, hi in zip(raw["area2_lo"].tolist(), raw["area2_hi"].tolist())]
    t["area2"] = a2
    k = 0.5 * float(scaling.rrx) * float(scaling.rry)
    t["area"] = [float(v) * k for v in a2]
    return t
