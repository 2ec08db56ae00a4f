"""ctypes binding of librayjoin_amd.so (include/rayjoin_amd.h).  No torch types cross this
boundary: device buffers are raw pointers (a torch tensor's data_ptr() or rj_dev_alloc memory).

The library is the only compute path: if it is missing or fails to load, importing the query
operators raises -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAYJOIN_AMD_LIB") or os.path.join(HERE, "librayjoin_amd.so")  # override: A/B builds

RJ_OK, RJ_E_INVALID, RJ_E_HIP, RJ_E_OVERFLOW, RJ_E_NOMEM, RJ_E_INTERNAL = 0, 1, 2, 3, 4, 5
RJ_EXCHANGE_HEAD_WORDS = 4
RJ_OVM_DROP_DEGENERATE = 1  # rj_overlay_map flags
RJ_OVM_MERGE_PIECES = 2
# rj_overlay_faces_op / rj_overlay_map_op: which (face of map 0, face of map 1) pairs are faces, and what names a face
RJ_OV_INTERSECTION, RJ_OV_UNION, RJ_OV_DIFFERENCE, RJ_OV_SYMDIFF, RJ_OV_IDENTITY = 0, 1, 2, 3, 4
RJ_OV_BY_PAIR, RJ_OV_BY_MAP0, RJ_OV_BY_MAP1 = 0, 1, 2
OVERLAY_HOW = {"intersection": RJ_OV_INTERSECTION, "union": RJ_OV_UNION, "difference": RJ_OV_DIFFERENCE,
               "symmetric_difference": RJ_OV_SYMDIFF, "identity": RJ_OV_IDENTITY}
OVERLAY_BY = {"pair": RJ_OV_BY_PAIR, "map0": RJ_OV_BY_MAP0, "map1": RJ_OV_BY_MAP1}
RJ_RINGS_SKIP_FACE0 = 1  # rj_map_rings flags
RJ_RINGS_NO_POINTS = 2
RJ_RING_MIXED = 1  # rj_ring flags
RJ_RMAP_DISSOLVE = 1  # rj_rings_map flags
RJ_CROSS_PROPER, RJ_CROSS_TOUCH, RJ_CROSS_OVERLAP, RJ_CROSS_EQUAL = 1, 2, 3, 4  # rj_crossing kinds
RJ_T_BUILD, RJ_T_LSI_KERNEL, RJ_T_PIP_KERNEL, RJ_T_LSI_POINTS, RJ_T_SORT, RJ_T_ORDER = 0, 1, 2, 3, 4, 5
RJ_T_BUILD_KEYS, RJ_T_BUILD_SORT, RJ_T_BUILD_LEAVES, RJ_T_BUILD_LEVELS, RJ_T_PIP_WALK, RJ_T_BUILD_RUNS = 6, 7, 8, 9, 10, 11
MISS_EID = 0xFFFFFFFF
KNEAREST_MAX_K = 32  # RJ_KNEAREST_MAX_K

XSECT_DTYPE = np.dtype(
    [("x_num", "<i8"), ("x_den", "<i8"), ("y_num", "<i8"), ("y_den", "<i8"),
     ("eid", "<u4", (2,)), ("mid_point_polygon_id", "<i4"), ("_pad", "<i4")])
# rj_overlay_face: (face of map 0, face of map 1), twice the overlap's signed area as a two's-complement int128
FACE_DTYPE = np.dtype([("face", "<i4", (2,)), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
# rj_ring: a closed boundary of a chain map -- its face, RJ_RING_MIXED, its smallest half-chain, twice its signed area
RING_DTYPE = np.dtype([("face", "<i4"), ("flags", "<u4"), ("leader", "<u4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
OVERLAY_MAP_COUNTS = ("n_chains", "n_points", "n_faces")  # (Handle.overlay_map gives and takes them as a plain tuple)
RINGS_COUNTS = ("n_rings", "n_halves", "n_points", "n_mixed", "n_skipped")
RJ_POLY_NONE = 0xFFFFFFFF  # rj_rings_polygons' parent of a ring of face 0 and of an orphan
# rj_polygon: one outer ring with its holes -- its face, the shell's ring index, its holes, twice its area
POLYGON_DTYPE = np.dtype([("face", "<i4"), ("shell", "<u4"), ("n_holes", "<u4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
POLYGONS_COUNTS = ("n_polygons", "n_members", "n_holes", "n_orphans", "n_face0")
RINGS_MAP_COUNTS = ("n_chains", "n_points", "n_edges", "n_closed", "n_zero_edges", "n_conflicts", "n_dissolved")
# rj_crossing: two edges of one map that meet elsewhere than in a shared end point (eid[0] < eid[1]), and how (RJ_CROSS_*)
CROSSING_DTYPE = np.dtype([("eid", "<u4", (2,)), ("kind", "<u4"), ("_pad", "<u4")])
CROSSINGS_COUNTS = ("n_found", "n_proper", "n_touch", "n_overlap", "n_equal", "n_edges", "n_zero_edges")
RJ_NODE_DROP_LAST = 1  # rj_map_node flags
NODE_COUNTS = ("n_points", "n_edges", "n_cuts", "n_cut_edges", "n_max_cuts", "n_used", "n_proper", "n_equal")
RJ_SNAP_DROP_LAST = 1  # rj_map_snap flags
SNAP_COUNTS = NODE_COUNTS + ("n_exact", "n_at_end", "n_stale")
# rj_snap_counts as one record (what a tool that keeps the counts of many rounds stores)
SNAP_COUNTS_DTYPE = np.dtype([(name, "<u8") for name in SNAP_COUNTS])
SIMPLIFY_COUNTS = ("n_points", "n_removed", "n_rounds", "n_closed", "n_pinned_extra", "n_max_round")
# rj_face: one face of rj_map_faces -- its shell's leader half-chain, its holes, its label, twice its area
MAP_FACE_DTYPE = np.dtype([("leader", "<u4"), ("n_holes", "<u4"), ("label", "<i4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
MAP_FACES_COUNTS = ("n_faces", "n_rings", "n_holes", "n_outer", "n_skipped", "n_dangling", "n_conflicts")
RJ_ELIM_DROP = 1  # rj_map_eliminate flags
RJ_ELIM_SLIVER, RJ_ELIM_ELIMINATED, RJ_ELIM_ISLAND, RJ_ELIM_NEGATIVE = 1, 2, 4, 8  # rj_elim_face flags
# rj_elim_face: one face (a label) of rj_map_eliminate -- the face it joins, the neighbour it chose, RJ_ELIM_*, twice its own area
ELIM_FACE_DTYPE = np.dtype([("label", "<i4"), ("target", "<i4"), ("best", "<i4"), ("flags", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
RJ_DISS_KEEP_EQUAL = 1  # rj_map_dissolve flags
# rj_diss_class: one class of rj_map_dissolve -- its label, the kept chain sides that carry it, twice its area
DISS_CLASS_DTYPE = np.dtype([("label", "<i4"), ("n_sides", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
DISSOLVE_COUNTS = ("n_kept", "n_dropped", "n_skipped", "n_chains", "n_points", "n_closed", "n_classes", "n_unmapped")
RJ_NB_VERTEX = 1  # rj_map_neighbours flags
# rj_nb_face: one face of rj_map_neighbours -- its label, the chain sides that carry it, its edge and vertex-only neighbours, twice
# its area, its perimeter and the part of it that borders label 0 (unsigned 128-bit integer lengths)
NB_FACE_DTYPE = np.dtype([("label", "<i4"), ("n_sides", "<u4"), ("n_edge_nbrs", "<u4"), ("n_vertex_nbrs", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8"),
                          ("perimeter_lo", "<u8"), ("perimeter_hi", "<u8"), ("outer_lo", "<u8"), ("outer_hi", "<u8")])
# rj_nb_entry: one neighbour of a face -- its label and face number, the chains and nodes the two share, the length of their border
NB_ENTRY_DTYPE = np.dtype([("label", "<i4"), ("face", "<u4"), ("n_chains", "<u4"), ("n_nodes", "<u4"), ("w_lo", "<u8"), ("w_hi", "<u8")])
NEIGHBOURS_COUNTS = ("n_faces", "n_entries", "n_edge_pairs", "n_vertex_pairs", "n_nodes", "n_node_pairs_raw", "max_labels_at_node")
RJ_FP_MEMBERS = 1  # rj_face_points flags
# rj_fp_face: one face of rj_face_points -- its label, its smallest point number (0xFFFFFFFF: none), its points, the exact sum of their
# values (a two's-complement int128), their min and max (INT64_MAX / INT64_MIN: no point, or no values)
FP_FACE_DTYPE = np.dtype([("label", "<i4"), ("first", "<u4"), ("n_points", "<u8"), ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("min", "<i8"), ("max", "<i8")])
FACE_POINTS_COUNTS = ("n_faces", "n_members", "n_outside", "n_unmatched", "n_runs")
# rj_near: the nearest edge of one point (rj_nearest_query) -- where 0: num = the signed cross product (a two's-complement int128), den = the
# squared length of the edge, d^2 = num^2 / den; where 1, 2 (first, second end): num = d^2, den = 1; a miss: eid = MISS_EID, the rest 0
NEAR_DTYPE = np.dtype([("eid", "<u4"), ("where", "<u4"), ("num_lo", "<u8"), ("num_hi", "<i8"), ("den_lo", "<u8"), ("den_hi", "<u8")])
WITHIN_COUNTS = ("n_pairs", "n_points_hit", "max_per_point")
WINDOW_COUNTS = ("n_pairs", "n_windows_hit", "max_per_window")
ELIMINATE_COUNTS = ("n_faces", "n_slivers", "n_eliminated", "n_islands", "n_mutual", "n_negative", "n_chains", "n_points", "n_dropped")

# every symbol include/rayjoin_amd.h declares: name -> (restype, argtypes)
_vp, _u64, _i64, _int = C.c_void_p, C.c_uint64, C.c_int64, C.c_int
SYMBOLS = {
    "rj_create": (_int, [_int, C.POINTER(_vp)]),
    "rj_destroy": (_int, [_vp]),
    "rj_set_stream": (_int, [_vp, _vp]),
    "rj_sync": (_int, [_vp]),
    "rj_last_error_string": (C.c_char_p, [_vp]),
    "rj_version": (C.c_char_p, []),
    "rj_upload_map": (_int, [_vp, _int, _vp, _u64, _vp, _vp, _vp, _u64]),
    "rj_upload_map_dev": (_int, [_vp, _int, _vp, _u64, _vp, _vp, _vp, _u64]),
    "rj_scale_points": (_int, [_vp, _vp, _u64, _vp, _int]),
    "rj_map_num_edges": (_int, [_vp, _int, C.POINTER(_u64)]),
    "rj_map_num_points": (_int, [_vp, _int, C.POINTER(_u64)]),
    "rj_map_points_dev": (_int, [_vp, _int, C.POINTER(_vp)]),
    "rj_map_prepared_dev": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(_vp)]),
    "rj_invalidate": (_int, [_vp]),
    "rj_map_runs": (_int, [_vp, _int, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rj_build_lbvh": (_int, [_vp, _int]),
    "rj_lsi_query": (_int, [_vp, _int, _int, _u64, _u64, _u64, _vp, C.POINTER(_u64)]),
    "rj_lsi_query_async": (_int, [_vp, _int, _int, _u64, _u64, _u64, _vp]),
    "rj_lsi_query_finish": (_int, [_vp, _u64, C.POINTER(_u64)]),
    "rj_lsi_count_to": (_int, [_vp, _vp]),
    "rj_lsi_count_async": (_int, [_vp, _int]),
    "rj_lsi_count_wait": (_int, [_vp, _int, _u64, C.POINTER(_u64)]),
    "rj_lsi_points": (_int, [_vp, _vp, _u64, _vp]),
    "rj_lsi_points_async": (_int, [_vp, _vp, _u64, _vp]),
    "rj_sort_pairs": (_int, [_vp, _vp, _u64]),
    "rj_comm_unique_id": (_int, [_vp]),
    "rj_comm_init": (_int, [_vp, _int, _int, _vp]),
    "rj_comm_destroy": (_int, [_vp]),
    "rj_allgather_pairs": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "rj_allgather_u32": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "rj_allgatherv_plan": (_int, [_vp, _int, _u64, _vp, C.POINTER(_u64)]),
    "rj_exchange_init": (_int, [_vp, _u64, _u64, _vp, _vp]),
    "rj_exchange_pairs_begin": (_int, [_vp, _int]),
    "rj_exchange_pairs_finish": (_int, [_vp, _int, _vp, _vp, C.POINTER(_u64)]),
    "rj_exchange_u32_begin": (_int, [_vp, _vp, _u64, _vp]),
    "rj_exchange_u32_finish": (_int, [_vp]),
    "rj_exchange_verdict": (_int, [_vp, _vp, _int, C.POINTER(_u64), C.POINTER(_int)]),
    "rj_last_ms_all": (_int, [_vp, _vp, _int]),
    "rj_overlay_edge_xsects": (_int, [_vp, _int, _vp, _u64, _vp]),
    "rj_overlay_faces": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "rj_overlay_map": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, C.c_uint32, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rj_overlay_faces_op": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64), C.c_uint32, C.c_uint32]),
    "rj_overlay_map_op": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, C.c_uint32, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32,
                                 C.c_uint32]),
    "rj_map_rings": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_uint32, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rj_rings_polygons": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.c_uint32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rj_rings_map": (_int, [_vp, _vp, _vp, _u64, _vp, _u64, _u64, C.c_uint32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rj_map_crossings": (_int, [_vp, _vp, _u64, _vp, _u64, C.c_uint32, _u64, _vp, _vp]),
    "rj_map_node": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, C.c_uint32, _u64, _vp, _vp, _vp, _vp]),
    "rj_map_snap": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, C.c_uint32, _u64, _vp, _vp, _vp, _vp]),
    "rj_map_simplify": (_int, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, C.c_uint32, _u64, _vp, _vp, _vp, _vp]),
    "rj_map_faces": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, C.c_uint32, _u64, _vp, _vp, _vp, _vp]),
    "rj_map_eliminate": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _u64, C.c_uint32, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rj_map_dissolve": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, C.c_uint32, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rj_map_neighbours": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_uint32, _u64, _u64, _vp, _vp, _vp, _vp]),
    "rj_face_points": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, C.c_uint32, _u64, _u64, _vp, _vp, _vp, _vp]),
    "rj_neighbours_labels": (_int, [_vp, _vp, _u64, _vp]),
    "rj_nearest_query": (_int, [_vp, _int, _int, _vp, _u64, _u64, _i64, _vp, _vp, _vp]),
    "rj_knearest_query": (_int, [_vp, _int, _int, _vp, _u64, _u64, C.c_uint32, _i64, _vp, _vp, _vp, _vp]),
    "rj_within_query": (_int, [_vp, _int, _int, _vp, _u64, _u64, _i64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rj_window_query": (_int, [_vp, _int, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "rj_pip_query": (_int, [_vp, _int, _int, _vp, _u64, _u64, _vp, _vp]),
    "rj_pip_query_async": (_int, [_vp, _int, _int, _vp, _u64, _u64, _vp, _vp]),
    "rj_build_grid": (_int, [_vp, _int, _int]),
    "rj_lsi_query_grid": (_int, [_vp, _u64, _vp, C.POINTER(_u64)]),
    "rj_pip_query_grid": (_int, [_vp, _int, _int, _vp, _u64, _u64, _vp, _vp]),
    "rj_last_ms": (_int, [_vp, _int, C.POINTER(C.c_float)]),
    "rj_last_stats": (_int, [_vp, C.POINTER(_u64)]),
    "rj_set_option": (_int, [_vp, C.c_char_p, _i64]),
    "rj_set_debug_option": (_int, [_vp, C.c_char_p, _i64]),
    "rj_get_debug_option": (_int, [_vp, C.c_char_p, C.POINTER(_i64)]),
    "rj_get_option": (_int, [_vp, C.c_char_p, C.POINTER(_i64)]),
    "rj_get_plan": (_int, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rj_dev_alloc": (_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "rj_dev_free": (_int, [_vp, _vp]),
    "rj_memcpy_h2d": (_int, [_vp, _vp, _vp, C.c_size_t]),
    "rj_memcpy_d2h": (_int, [_vp, _vp, _vp, C.c_size_t]),
    "rj_memcpy_d2d": (_int, [_vp, _vp, _vp, C.c_size_t]),
}


def kernel_source_hash():
    """sha256 (16 hex digits) of the HIP sources the query kernels are built from: profile artefacts
    (profiles/traffic.json) carry it, and bench.py only quotes them for the sources they measured."""
    import hashlib
    hsh = hashlib.sha256()
    for name in ("rj_kernels.hip", "rj_kernels.h", "rj_device.h", "rj_predicates.h", "rj_strip.hip"):
        with open(os.path.join(HERE, "csrc", name), "rb") as f:
            hsh.update(f.read())
    return hsh.hexdigest()[:16]


def exchange_verdict(counts, capacities):
    """rj_exchange_verdict: (status, max_count, first_bad) every rank concludes from the gathered (count, capacity) words"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    caps = np.ascontiguousarray(capacities, dtype=np.uint64)
    mx, bad = _u64(0), _int(-1)
    rc = load().rj_exchange_verdict(counts.ctypes.data, caps.ctypes.data, int(counts.shape[0]), C.byref(mx), C.byref(bad))
    return rc, mx.value, bad.value


def allgatherv_plan(counts, capacity):
    """rj_allgatherv_plan: (offsets, total, status) of an all-gather-v of `counts` elements per rank (host only)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    off = np.zeros(max(1, counts.shape[0]), dtype=np.uint64)
    total = _u64()
    rc = load().rj_allgatherv_plan(counts.ctypes.data, int(counts.shape[0]), int(capacity), off.ctypes.data, C.byref(total))
    return off[:counts.shape[0]], int(total.value), rc


def scale_points(bb, xy, fused=False):
    """rj_scale_points: Scaling(bb).ScaleX/ScaleY over xy (host code of the library, no GPU).
    fused=True reproduces the FMA that nvcc contracts the reference's device lambda into."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(bb, dtype=np.float64)
    out = np.empty(xy.shape, dtype=np.int64)
    rc = load().rj_scale_points(b.ctypes.data, xy.ctypes.data, xy.shape[0], out.ctypes.data, int(bool(fused)))
    if rc != RJ_OK:
        raise RayJoinError(rc, "rj_scale_points failed")
    return out


class RayJoinError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rayjoin_amd error %d: %s" % (code, msg))
        self.code = code


class CountsOverflow(RayJoinError):
    """RJ_E_OVERFLOW of a call that reports its true counts: the base of the calls' own classes below"""

    def __init__(self, msg, counts):
        super().__init__(RJ_E_OVERFLOW, msg)
        self.counts = counts


class MapOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_overlay_map: counts = (chains, points, faces), the true counts"""


class RingsOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_rings: counts = dict(n_rings, n_halves, n_points, n_mixed, n_skipped), the true counts"""


class PolygonsOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_rings_polygons: counts = dict(n_polygons, n_members, n_holes, n_orphans, n_face0), the true counts"""


class RingsMapOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_rings_map: counts = dict(n_chains, n_points, n_edges, n_closed, n_zero_edges, n_conflicts, n_dissolved),
    the true counts"""


class CrossingsOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_crossings: counts = dict(n_found, n_proper, n_touch, n_overlap, n_equal, n_edges, n_zero_edges),
    the true counts"""


class NodeOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_node: counts = dict(n_points, n_edges, n_cuts, n_cut_edges, n_max_cuts, n_used, n_proper, n_equal),
    the true counts"""


class SnapOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_snap: counts = a dict of SNAP_COUNTS (rj_node_counts' fields, n_exact, n_at_end, n_stale), the
    true counts"""


class FacesOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_faces: counts = dict(n_faces, n_rings, n_holes, n_outer, n_skipped, n_dangling, n_conflicts), the
    true counts; left / right are written in full"""


class SimplifyOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_simplify: counts = dict(n_points, n_removed, n_rounds, n_closed, n_pinned_extra, n_max_round),
    the true counts"""


class EliminateOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_eliminate: counts = a dict of ELIMINATE_COUNTS, the true counts; nothing is written"""


class DissolveOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_dissolve: counts = a dict of DISSOLVE_COUNTS, the true counts; nothing is written"""


class NeighboursOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_map_neighbours: counts = a dict of NEIGHBOURS_COUNTS, the true counts; nothing is written"""


class FacePointsOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_face_points: counts = a dict of FACE_POINTS_COUNTS, the true counts; nothing is written"""


class WithinOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_within_query: counts = a dict of WITHIN_COUNTS, the true counts; the offsets are written, the pairs are not"""


class WindowOverflow(CountsOverflow):
    """RJ_E_OVERFLOW of rj_window_query: counts = a dict of WINDOW_COUNTS, the true counts; the offsets are written, the pairs are not"""


class NeighboursNodePairs(RayJoinError):
    """RJ_E_INVALID of rj_map_neighbours under RJ_NB_VERTEX for n_node_pairs_raw >= 2^32: the count (it saturates at
    2^64 - 1); nothing is written"""

    def __init__(self, msg, n_node_pairs_raw):
        super().__init__(RJ_E_INVALID, msg)
        self.n_node_pairs_raw = n_node_pairs_raw


class DissolveUnmapped(RayJoinError):
    """RJ_E_INVALID of rj_map_dissolve for labels outside the class table: n_unmapped chain sides carry one; nothing is written"""

    def __init__(self, msg, n_unmapped):
        super().__init__(RJ_E_INVALID, msg)
        self.n_unmapped = n_unmapped


class QueueOverflow(RayJoinError):
    """RJ_E_OVERFLOW: n_found holds the true count (the reference only asserts, queue.h:37)."""

    def __init__(self, msg, n_found):
        super().__init__(RJ_E_OVERFLOW, msg)
        self.n_found = n_found


_lib = None


def load():
    """dlopen the HIP library.  Fails loudly when it has not been built (python -c 'import
    __graft_entry__ as g; g.build()' or make -C rayjoin_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("rayjoin_amd: %s is missing -- build the HIP extension first "
                              "(make -C rayjoin_amd/csrc); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        variant = bool(os.environ.get("RAYJOIN_AMD_LIB"))  # an A/B build of another revision may lack the newer entry points
        for name, (res, args) in SYMBOLS.items():
            if variant and not hasattr(L, name):
                continue
            fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    """void* of a numpy array (host), an int, None, or anything with data_ptr() (torch tensor)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


def _tol_words(tol):
    """a tolerance, a Python int in [0, 2^128) -> its (low, high) 64-bit words"""
    tol = int(tol)
    if not 0 <= tol < 1 << 128:
        raise ValueError("tol must lie in [0, 2^128), not %d" % tol)
    return tol & 0xFFFFFFFFFFFFFFFF, tol >> 64


class DeviceBuffer:
    """Device memory owned through the C ABI (rj_dev_alloc) for hosts without torch."""

    def __init__(self, handle, nbytes):
        self.handle = handle
        self.nbytes = int(nbytes)
        p = _vp()
        handle._check(load().rj_dev_alloc(handle.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def data_ptr(self):
        return self.ptr

    def to_host(self, dtype, count=None):
        dtype = np.dtype(dtype)
        count = self.nbytes // dtype.itemsize if count is None else int(count)
        out = np.empty(count, dtype=dtype)
        if count:
            self.handle._check(load().rj_memcpy_d2h(self.handle.h, out.ctypes.data, self.ptr,
                                                    count * dtype.itemsize))
        return out

    def from_host(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if arr.nbytes:
            self.handle._check(load().rj_memcpy_h2d(self.handle.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def from_device(self, src, nbytes):
        """the first nbytes of another device array (a DeviceBuffer, a tensor, an address)"""
        assert int(nbytes) <= self.nbytes
        if nbytes:
            self.handle._check(load().rj_memcpy_d2d(self.handle.h, self.ptr, _ptr(src), int(nbytes)))
        return self

    def free(self):
        if self.ptr:
            load().rj_dev_free(self.handle.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.handle.h:
                self.free()
        except Exception:
            pass


class Handle:
    """One per GPU (rj_create).  Thin, 1:1 with the C ABI."""

    def __init__(self, device_id=0):
        self.L = load()
        h = _vp()
        rc = self.L.rj_create(int(device_id), C.byref(h))
        if rc != RJ_OK:
            raise RayJoinError(rc, "rj_create(device %d) failed -- no usable HIP device?" % device_id)
        self.h = h.value
        self.device_id = device_id

    def close(self):
        if getattr(self, "h", None):
            self.L.rj_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc != RJ_OK:
            raise RayJoinError(rc, self.L.rj_last_error_string(self.h).decode())

    def _counted(self, fn, names, overflow, *args, tail=(), invalid=None):
        """fn(h, *args, counts, *tail) of a library call that reports len(names) uint64 counts -> the counts as a dict by
        name.  RJ_E_OVERFLOW raises `overflow` with that dict; invalid = (cls, name): RJ_E_INVALID with a nonzero count
        `name` raises cls with it; any other failure is _check's RayJoinError."""
        counts = (_u64 * len(names))()
        rc = fn(self.h, *args, counts, *tail)
        named = dict(zip(names, (int(v) for v in counts)))
        if rc == RJ_E_OVERFLOW:
            raise overflow(self.L.rj_last_error_string(self.h).decode(), named)
        if rc == RJ_E_INVALID and invalid is not None and named[invalid[1]]:
            raise invalid[0](self.L.rj_last_error_string(self.h).decode(), named[invalid[1]])
        self._check(rc)
        return named

    def set_stream(self, stream_ptr):
        self._check(self.L.rj_set_stream(self.h, stream_ptr))
        self._stream_ptr = stream_ptr  # (dist.PairExchange checks that its event and the kernels share a stream)

    def sync(self):
        self._check(self.L.rj_sync(self.h))

    def set_option(self, name, value):
        self._check(self.L.rj_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = _i64()
        self._check(self.L.rj_get_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def set_debug_option(self, name, value):
        """experiment knobs (grids, chunk sizes, run lengths: rj_set_debug_option)"""
        self._check(self.L.rj_set_debug_option(self.h, name.encode(), int(value)))

    def get_debug_option(self, name):
        v = _i64()
        self._check(self.L.rj_get_debug_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload_map(self, map_id, pts, row_index, left, right):
        pts = np.ascontiguousarray(pts, dtype=np.int64).reshape(-1, 2)
        row_index = np.ascontiguousarray(row_index, dtype=np.uint32)
        left = np.ascontiguousarray(left, dtype=np.int64)
        right = np.ascontiguousarray(right, dtype=np.int64)
        nc = left.shape[0]
        self._check(self.L.rj_upload_map(self.h, map_id, pts.ctypes.data, pts.shape[0],
                                         row_index.ctypes.data, left.ctypes.data, right.ctypes.data, nc))

    def upload_map_dev(self, map_id, xy_dev, n_points, row_index_dev, left_dev, right_dev, n_chains):
        """rj_upload_map_dev: the map from device arrays (int64 xy, uint32 row_index, int32 left / right)"""
        self._check(self.L.rj_upload_map_dev(self.h, map_id, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), _ptr(left_dev),
                                             _ptr(right_dev), int(n_chains)))

    def map_num_edges(self, map_id):
        n = _u64()
        self._check(self.L.rj_map_num_edges(self.h, map_id, C.byref(n)))
        return n.value

    def map_num_points(self, map_id):
        n = _u64()
        self._check(self.L.rj_map_num_points(self.h, map_id, C.byref(n)))
        return n.value

    def map_points_dev(self, map_id):
        p = _vp()
        self._check(self.L.rj_map_points_dev(self.h, map_id, C.byref(p)))
        return p.value

    def map_prepared(self, map_id):
        """-> (qpts [np, 2], qext [ceil(np / 64), 4]) int32 host copies of the map's prepared points, or None where the
        upload had no memory for them"""
        qp, qe = _vp(), _vp()
        self._check(self.L.rj_map_prepared_dev(self.h, map_id, C.byref(qp), C.byref(qe)))
        if not qp.value or not qe.value:
            return None
        n = self.map_num_points(map_id)
        qpts = np.empty((n, 2), dtype=np.int32)
        qext = np.empty(((n + 63) // 64, 4), dtype=np.int32)
        self._check(self.L.rj_memcpy_d2h(self.h, qpts.ctypes.data, qp.value, qpts.nbytes))
        self._check(self.L.rj_memcpy_d2h(self.h, qext.ctypes.data, qe.value, qext.nbytes))
        return qpts, qext

    def invalidate(self):
        self._check(self.L.rj_invalidate(self.h))

    def map_runs(self, map_id):
        """-> (piece_begin, piece_len, run_first) of the polyline runs cut for this map"""
        nr, npc = _u64(), _u64()
        self._check(self.L.rj_map_runs(self.h, map_id, None, None, None, C.byref(nr), C.byref(npc)))
        pb = np.zeros(npc.value, dtype=np.uint32)
        pl = np.zeros(npc.value, dtype=np.uint32)
        rf = np.zeros(nr.value + 1, dtype=np.uint32)
        self._check(self.L.rj_map_runs(self.h, map_id, pb.ctypes.data, pl.ctypes.data, rf.ctypes.data, None, None))
        return pb, pl, rf

    def build_lbvh(self, base_map_id):
        self._check(self.L.rj_build_lbvh(self.h, base_map_id))

    def lsi_query(self, base_map_id, query_map_id, qb, qe, capacity, pairs_dev):
        n = _u64()
        rc = self.L.rj_lsi_query(self.h, base_map_id, query_map_id, qb, qe, capacity, _ptr(pairs_dev), C.byref(n))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), n.value)
        self._check(rc)
        return n.value

    def lsi_query_async(self, base_map_id, query_map_id, qb, qe, capacity, pairs_dev):
        self._check(self.L.rj_lsi_query_async(self.h, base_map_id, query_map_id, qb, qe, capacity, _ptr(pairs_dev)))

    def lsi_query_finish(self, capacity):
        n = _u64()
        rc = self.L.rj_lsi_query_finish(self.h, capacity, C.byref(n))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), n.value)
        self._check(rc)
        return n.value

    def build_grid(self, map_id, grid_size):
        self._check(self.L.rj_build_grid(self.h, map_id, grid_size))

    def lsi_query_grid(self, capacity, pairs_dev):
        n = _u64()
        rc = self.L.rj_lsi_query_grid(self.h, capacity, _ptr(pairs_dev), C.byref(n))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), n.value)
        self._check(rc)
        return n.value

    def pip_query_grid(self, base_map_id, query_map_id, pts_dev, pt_begin, n, closest_dev, face_dev=None):
        self._check(self.L.rj_pip_query_grid(self.h, base_map_id, query_map_id, _ptr(pts_dev), pt_begin, n,
                                             _ptr(closest_dev), _ptr(face_dev)))

    def lsi_count_async(self, slot):
        self._check(self.L.rj_lsi_count_async(self.h, slot))

    def lsi_count_wait(self, slot, capacity):
        n = _u64()
        rc = self.L.rj_lsi_count_wait(self.h, slot, capacity, C.byref(n))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), n.value)
        self._check(rc)
        return n.value

    def lsi_count_to(self, n_found_dev):
        """device-side Queue::size: copy the last async LSI's count (u64) to device memory, on the stream"""
        self._check(self.L.rj_lsi_count_to(self.h, _ptr(n_found_dev)))

    def lsi_points(self, pairs_dev, n, out_dev):
        self._check(self.L.rj_lsi_points(self.h, _ptr(pairs_dev), n, _ptr(out_dev)))

    def lsi_points_async(self, pairs_dev, capacity, out_dev):
        """records of the last lsi_query_async, behind it on the stream (count read on the device)"""
        self._check(self.L.rj_lsi_points_async(self.h, _ptr(pairs_dev), capacity, _ptr(out_dev)))

    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = load().rj_comm_unique_id(buf)
        if rc != RJ_OK:
            raise RayJoinError(rc, "rj_comm_unique_id failed")
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.L.rj_comm_init(self.h, nranks, rank, buf))
        self.nranks = nranks

    def comm_destroy(self):
        self._check(self.L.rj_comm_destroy(self.h))

    def exchange_init(self, capacity, slot, buf0_dev, buf1_dev=None):
        self._check(self.L.rj_exchange_init(self.h, capacity, slot, _ptr(buf0_dev), _ptr(buf1_dev)))

    def exchange_pairs_begin(self, buf):
        self._check(self.L.rj_exchange_pairs_begin(self.h, buf))

    def exchange_pairs_finish(self, buf, nranks):
        """-> (counts list, device pointers of every rank's pairs, total); raises QueueOverflow on every rank alike"""
        counts = (_u64 * nranks)()
        slices = (_vp * nranks)()
        total = _u64()
        rc = self.L.rj_exchange_pairs_finish(self.h, buf, counts, slices, C.byref(total))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), total.value)
        self._check(rc)
        return list(counts), [s or 0 for s in slices], total.value

    def exchange_u32_begin(self, src_dev, n_per_rank, recv_dev):
        self._check(self.L.rj_exchange_u32_begin(self.h, _ptr(src_dev), n_per_rank, _ptr(recv_dev)))

    def exchange_u32_finish(self):
        self._check(self.L.rj_exchange_u32_finish(self.h))

    def _allgather(self, fn, src_dev, n_local, out_dev, out_capacity):
        counts = (_u64 * getattr(self, "nranks", 1))()
        tot = _u64()
        rc = fn(self.h, _ptr(src_dev), n_local, _ptr(out_dev), out_capacity, counts, C.byref(tot))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), tot.value)
        self._check(rc)
        return tot.value, list(counts)

    def allgather_pairs(self, pairs_dev, n_local, out_dev, out_capacity):
        return self._allgather(self.L.rj_allgather_pairs, pairs_dev, n_local, out_dev, out_capacity)

    def allgather_u32(self, src_dev, n_local, out_dev, out_capacity):
        return self._allgather(self.L.rj_allgather_u32, src_dev, n_local, out_dev, out_capacity)

    def overlay_edge_xsects(self, im, pairs_dev, n, xsects_dev):
        self._check(self.L.rj_overlay_edge_xsects(self.h, im, _ptr(pairs_dev), n, _ptr(xsects_dev)))

    def overlay_faces(self, xsects0_dev, xsects1_dev, n, vertex_face0_dev, vertex_face1_dev, capacity, out_dev, op=None):
        """rows of the face table into out_dev (FACE_DTYPE); returns the row count, QueueOverflow past capacity.
        op = (how, by): rj_overlay_faces_op; None: rj_overlay_faces"""
        nf = _u64()
        args = (self.h, _ptr(xsects0_dev), _ptr(xsects1_dev), n, _ptr(vertex_face0_dev), _ptr(vertex_face1_dev), capacity, _ptr(out_dev),
                C.byref(nf))
        rc = self.L.rj_overlay_faces(*args) if op is None else self.L.rj_overlay_faces_op(*args, int(op[0]), int(op[1]))
        if rc == RJ_E_OVERFLOW:
            raise QueueOverflow(self.L.rj_last_error_string(self.h).decode(), nf.value)
        self._check(rc)
        return nf.value

    def overlay_map(self, xsects0_dev, xsects1_dev, n, vertex_face0_dev, vertex_face1_dev, flags, capacities, xy_dev, row_index_dev,
                    left_dev, right_dev, face_pairs_dev, origin_dev=None, op=None):
        """rj_overlay_map into the caller's device arrays; capacities = (chains, points, faces).  Returns the counts
        (chains, points, faces); MapOverflow (with the true counts) past a capacity.  op = (how, by): rj_overlay_map_op"""
        cc, pc, fc = (int(v) for v in capacities)
        fn, tail = (self.L.rj_overlay_map, ()) if op is None else (self.L.rj_overlay_map_op, (int(op[0]), int(op[1])))
        try:
            return tuple(self._counted(fn, OVERLAY_MAP_COUNTS, MapOverflow, _ptr(xsects0_dev), _ptr(xsects1_dev), n, _ptr(vertex_face0_dev),
                                       _ptr(vertex_face1_dev), int(flags), cc, pc, fc, _ptr(xy_dev), _ptr(row_index_dev), _ptr(left_dev),
                                       _ptr(right_dev), _ptr(face_pairs_dev), _ptr(origin_dev), tail=tail).values())
        except MapOverflow as e:
            e.counts = tuple(e.counts.values())  # (this call's counts are a plain tuple, in and out)
            raise

    def map_rings(self, xy_dev, n_points, row_index_dev, left_dev, right_dev, n_chains, flags, capacities, rings_dev, ring_first_dev,
                  ring_half_dev, ring_row_dev, ring_xy_dev):
        """rj_map_rings of a chain map in device memory into the caller's device arrays; capacities = (rings, half-chains,
        points).  Returns the counts as a dict (RINGS_COUNTS); RingsOverflow (with the true counts) past a capacity."""
        rc, hc, pc = (int(v) for v in capacities)
        return self._counted(self.L.rj_map_rings, RINGS_COUNTS, RingsOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), _ptr(left_dev),
                             _ptr(right_dev), int(n_chains), int(flags), rc, hc, pc, _ptr(rings_dev), _ptr(ring_first_dev), _ptr(ring_half_dev),
                             _ptr(ring_row_dev), _ptr(ring_xy_dev))

    def rings_polygons(self, rings_dev, n_rings, ring_row_dev, ring_xy_dev, n_points, flags, capacities, parent_dev, polygons_dev,
                       poly_first_dev, poly_ring_dev):
        """rj_rings_polygons of rj_map_rings' arrays in device memory into the caller's device arrays; capacities =
        (polygons, members); parent_dev may be None.  Returns the counts as a dict (POLYGONS_COUNTS); PolygonsOverflow
        (with the true counts) past a capacity."""
        pc, mc = (int(v) for v in capacities)
        return self._counted(self.L.rj_rings_polygons, POLYGONS_COUNTS, PolygonsOverflow, _ptr(rings_dev), int(n_rings), _ptr(ring_row_dev),
                             _ptr(ring_xy_dev), int(n_points), int(flags), pc, mc, _ptr(parent_dev), _ptr(polygons_dev), _ptr(poly_first_dev),
                             _ptr(poly_ring_dev))

    def rings_map(self, ring_row_dev, ring_xy_dev, n_points, ring_face_dev, face_stride, n_rings, flags, capacities, xy_dev, row_index_dev,
                  left_dev, right_dev):
        """rj_rings_map of labelled rings in device memory (ring_face_dev read through face_stride bytes) into the caller's
        device arrays; capacities = (chains, points).  Returns the counts as a dict (RINGS_MAP_COUNTS); RingsMapOverflow
        (with the true counts) past a capacity."""
        cc, pc = (int(v) for v in capacities)
        return self._counted(self.L.rj_rings_map, RINGS_MAP_COUNTS, RingsMapOverflow, _ptr(ring_row_dev), _ptr(ring_xy_dev), int(n_points),
                             _ptr(ring_face_dev), int(face_stride), int(n_rings), int(flags), cc, pc, _ptr(xy_dev), _ptr(row_index_dev),
                             _ptr(left_dev), _ptr(right_dev))

    def map_crossings(self, xy_dev, n_points, row_index_dev, n_chains, capacity, out_dev, flags=0):
        """rj_map_crossings of a chain map in device memory into the caller's device array of `capacity` rj_crossing records
        (capacity 0, out_dev None: the sizing call).  Returns the counts as a dict (CROSSINGS_COUNTS); CrossingsOverflow (with
        the true counts) past the capacity."""
        return self._counted(self.L.rj_map_crossings, CROSSINGS_COUNTS, CrossingsOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev),
                             int(n_chains), int(flags), int(capacity), _ptr(out_dev))

    def map_node(self, xy_dev, n_points, row_index_dev, n_chains, cross_dev, n_cross, flags, capacity, out_xy_dev, out_row_index_dev,
                 edge_origin_dev=None):
        """rj_map_node of a chain map and its rj_map_crossings records, both in device memory, into the caller's device arrays
        of `capacity` points, n_chains + 1 row entries and (or None) n_edges origins (capacity 0, arrays None: the sizing
        call).  Returns the counts as a dict (NODE_COUNTS); NodeOverflow (with the true counts) past the capacity."""
        return self._counted(self.L.rj_map_node, NODE_COUNTS, NodeOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), int(n_chains),
                             _ptr(cross_dev), int(n_cross), int(flags), int(capacity), _ptr(out_xy_dev), _ptr(out_row_index_dev),
                             _ptr(edge_origin_dev))

    def map_snap(self, xy_dev, n_points, row_index_dev, n_chains, cross_dev, n_cross, flags, capacity, out_xy_dev, out_row_index_dev,
                 edge_origin_dev=None):
        """rj_map_snap of a chain map and its rj_map_crossings records, both in device memory, into the caller's device arrays
        of `capacity` points, n_chains + 1 row entries and (or None) n_edges origins (capacity 0, arrays None: the sizing
        call).  Returns the counts as a dict (SNAP_COUNTS); SnapOverflow (with the true counts) past the capacity."""
        return self._counted(self.L.rj_map_snap, SNAP_COUNTS, SnapOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), int(n_chains),
                             _ptr(cross_dev), int(n_cross), int(flags), int(capacity), _ptr(out_xy_dev), _ptr(out_row_index_dev),
                             _ptr(edge_origin_dev))

    def map_simplify(self, xy_dev, n_points, row_index_dev, n_chains, tol, capacity, out_xy_dev, out_row_index_dev, origin_dev=None, flags=0):
        """rj_map_simplify of a chain map in device memory into the caller's device arrays of `capacity` points, n_chains + 1
        row entries and (or None) `capacity` origins (capacity 0, arrays None: the sizing call); tol a Python int in
        [0, 2^128).  Returns the counts as a dict (SIMPLIFY_COUNTS); SimplifyOverflow (with the true counts) past the capacity."""
        return self._counted(self.L.rj_map_simplify, SIMPLIFY_COUNTS, SimplifyOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev),
                             int(n_chains), *_tol_words(tol), int(flags), int(capacity), _ptr(out_xy_dev), _ptr(out_row_index_dev), _ptr(origin_dev))

    def map_faces(self, xy_dev, n_points, row_index_dev, n_chains, left_dev, right_dev, faces_dev=None, face_capacity=0, in_left_dev=None,
                  in_right_dev=None, flags=0):
        """rj_map_faces of a chain map in device memory: the computed faces into left_dev / right_dev (n_chains int32 each) and,
        where faces_dev is given, `face_capacity` rj_face records; in_left_dev / in_right_dev: the labels to check, or None.
        Returns the counts as a dict (MAP_FACES_COUNTS); FacesOverflow (with the true counts) past the capacity."""
        return self._counted(self.L.rj_map_faces, MAP_FACES_COUNTS, FacesOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), int(n_chains),
                             _ptr(in_left_dev), _ptr(in_right_dev), int(flags), int(face_capacity), _ptr(left_dev), _ptr(right_dev), _ptr(faces_dev))

    def map_eliminate(self, xy_dev, n_points, row_index_dev, left_dev, right_dev, n_chains, tol, capacities, out_left_dev, out_right_dev,
                      out_xy_dev=None, out_row_index_dev=None, chain_origin_dev=None, faces_dev=None, flags=0):
        """rj_map_eliminate of a labelled chain map in device memory: the new labels into out_left_dev / out_right_dev and,
        under RJ_ELIM_DROP, the kept chains into out_xy_dev / out_row_index_dev / (or None) chain_origin_dev; where faces_dev
        is given, the rj_elim_face records.  capacities = (faces, chains, points); (0, 0, 0) with arrays None is the sizing
        call.  tol a Python int in [0, 2^128).  Returns the counts as a dict (ELIMINATE_COUNTS); EliminateOverflow (with the
        true counts) past a capacity."""
        tol_lo, tol_hi = _tol_words(tol)
        fc, cc, pc = (int(v) for v in capacities)
        return self._counted(self.L.rj_map_eliminate, ELIMINATE_COUNTS, EliminateOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev),
                             _ptr(left_dev), _ptr(right_dev), int(n_chains), tol_lo, tol_hi, int(flags), fc, cc, pc, _ptr(faces_dev), _ptr(out_left_dev),
                             _ptr(out_right_dev), _ptr(out_xy_dev), _ptr(out_row_index_dev), _ptr(chain_origin_dev))

    def map_dissolve(self, xy_dev, n_points, row_index_dev, left_dev, right_dev, n_chains, class_dev, n_labels, capacities, out_left_dev, out_right_dev,
                     out_xy_dev, out_row_index_dev, chain_origin_dev=None, chain_out_dev=None, classes_dev=None, flags=0):
        """rj_map_dissolve of a labelled chain map in device memory: the faces merged by class (class_dev: an int32 table of
        n_labels entries, or None for the labels themselves), the chains re-joined, into out_xy_dev / out_row_index_dev /
        out_left_dev / out_right_dev and (or None) chain_origin_dev, chain_out_dev [n_chains] and the rj_diss_class records
        classes_dev.  capacities = (classes, chains, points); (0, 0, 0) with arrays None is the sizing call.  Returns the counts
        as a dict (DISSOLVE_COUNTS); DissolveOverflow (with the true counts) past a capacity, DissolveUnmapped (with
        n_unmapped) for nonzero labels outside the table."""
        kc, cc, pc = (int(v) for v in capacities)
        return self._counted(self.L.rj_map_dissolve, DISSOLVE_COUNTS, DissolveOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev), _ptr(left_dev),
                             _ptr(right_dev), int(n_chains), _ptr(class_dev), int(n_labels), int(flags), kc, cc, pc, _ptr(classes_dev), _ptr(out_left_dev),
                             _ptr(out_right_dev), _ptr(out_xy_dev), _ptr(out_row_index_dev), _ptr(chain_origin_dev), _ptr(chain_out_dev),
                             invalid=(DissolveUnmapped, "n_unmapped"))

    def map_neighbours(self, xy_dev, n_points, row_index_dev, left_dev, right_dev, n_chains, capacities, faces_dev=None, offsets_dev=None, entries_dev=None,
                       flags=0):
        """rj_map_neighbours of a labelled chain map in device memory: the face adjacency table in CSR form -- the rj_nb_face
        records into faces_dev (or None), uint64 offsets_dev [faces + 1] and the rj_nb_entry rows entries_dev.  capacities =
        (faces, entries); (0, 0) with arrays None is the sizing call.  flags: RJ_NB_VERTEX for the nodes and the vertex-only
        neighbours.  Returns the counts as a dict (NEIGHBOURS_COUNTS); NeighboursOverflow (with the true counts) past a capacity,
        NeighboursNodePairs (with the count) where the nodes give 2^32 directed pairs or more."""
        fc, ec = (int(v) for v in capacities)
        return self._counted(self.L.rj_map_neighbours, NEIGHBOURS_COUNTS, NeighboursOverflow, _ptr(xy_dev), int(n_points), _ptr(row_index_dev),
                             _ptr(left_dev), _ptr(right_dev), int(n_chains), int(flags), fc, ec, _ptr(faces_dev), _ptr(offsets_dev), _ptr(entries_dev),
                             invalid=(NeighboursNodePairs, "n_node_pairs_raw"))

    def face_points(self, label_dev, n, capacities, value_dev=None, value_stride=1, face_label_dev=None, n_face_labels=0, faces_dev=None, offsets_dev=None,
                    members_dev=None, flags=0):
        """rj_face_points of n located points in device memory (label_dev: int32, what rj_pip_query wrote): per face the count,
        the exact int128 sum, min and max of value_dev[i * value_stride] (int64; None: no values) and the smallest point number
        as rj_fp_face records into faces_dev (or None); under RJ_FP_MEMBERS the uint64 offsets_dev [faces + 1] and the uint32
        point numbers members_dev of every face.  face_label_dev [n_face_labels] (int32, or None): the faces, strictly ascending
        as unsigned numbers, without 0 -- the label column of rj_map_neighbours' records; None: the distinct nonzero labels of
        the points.  capacities = (faces, members); (0, 0) with arrays None is the sizing call.  Returns the counts as a dict
        (FACE_POINTS_COUNTS); FacePointsOverflow (with the true counts) past a capacity."""
        fc, mc = (int(v) for v in capacities)
        return self._counted(self.L.rj_face_points, FACE_POINTS_COUNTS, FacePointsOverflow, _ptr(label_dev), int(n), _ptr(value_dev), int(value_stride),
                             _ptr(face_label_dev), int(n_face_labels), int(flags), fc, mc, _ptr(faces_dev), _ptr(offsets_dev), _ptr(members_dev))

    def neighbours_labels(self, faces_dev, n_faces, label_dev):
        """label_dev[k] = the label of record k of rj_map_neighbours' faces_dev, on the device (rj_neighbours_labels)"""
        self._check(self.L.rj_neighbours_labels(self.h, _ptr(faces_dev), int(n_faces), _ptr(label_dev)))

    def sort_pairs(self, pairs_dev, n):
        self._check(self.L.rj_sort_pairs(self.h, _ptr(pairs_dev), n))

    def pip_query(self, base_map_id, query_map_id, pts_dev, pt_begin, n, closest_dev, face_dev=None, sync=True):
        fn = self.L.rj_pip_query if sync else self.L.rj_pip_query_async
        self._check(fn(self.h, base_map_id, query_map_id, _ptr(pts_dev), pt_begin, n, _ptr(closest_dev), _ptr(face_dev)))

    def nearest_query(self, base_map_id, query_map_id, pts_dev, pt_begin, n, eid_dev, rec_dev=None, dist_dev=None, max_dist=-1):
        """rj_nearest_query: for n points (pts_dev: int64 pairs in device memory, or None for the vertices [pt_begin, pt_begin + n)
        of the query map) the eid of the nearest edge of the indexed base map into eid_dev (uint32, MISS_EID where none
        qualifies), the exact record into rec_dev (NEAR_DTYPE, or None) and sqrt(d^2) into dist_dev (float64, +inf on a
        miss, or None).  max_dist: negative = unlimited, else only edges with d <= max_dist qualify, exactly.  Synchronous."""
        self._check(self.L.rj_nearest_query(self.h, base_map_id, query_map_id, _ptr(pts_dev), int(pt_begin), int(n), int(max_dist), _ptr(eid_dev),
                                            _ptr(rec_dev), _ptr(dist_dev)))

    def knearest_query(self, base_map_id, query_map_id, pts_dev, pt_begin, n, k, eid_dev, count_dev=None, rec_dev=None, dist_dev=None, max_dist=-1):
        """rj_knearest_query: for n points (pts_dev: int64 pairs in device memory, or None for the vertices [pt_begin, pt_begin + n)
        of the query map) the eids of the k (1 .. KNEAREST_MAX_K) nearest edges of the indexed base map, nearest first, equal
        distances to the smaller eid, into row i of eid_dev (uint32 [n][k]); how many there are into count_dev (uint32 [n], or
        None), the exact records into rec_dev (NEAR_DTYPE [n][k], or None) and sqrt(d^2) into dist_dev (float64 [n][k], or
        None); the entries of a row behind its count are the miss (MISS_EID, a zero record, +inf).  max_dist: negative =
        unlimited, else only edges with d <= max_dist qualify, exactly.  Synchronous."""
        self._check(self.L.rj_knearest_query(self.h, base_map_id, query_map_id, _ptr(pts_dev), int(pt_begin), int(n), int(k), int(max_dist),
                                             _ptr(count_dev), _ptr(eid_dev), _ptr(rec_dev), _ptr(dist_dev)))

    def within_query(self, base_map_id, query_map_id, pts_dev, pt_begin, n, max_dist, pair_capacity=0, offsets_dev=None, eid_dev=None, rec_dev=None,
                     dist_dev=None):
        """rj_within_query: for n points (pts_dev: int64 pairs in device memory, or None for the vertices [pt_begin, pt_begin + n)
        of the query map) every edge of the indexed base map with d <= max_dist, exactly, as a CSR: the uint64 offsets_dev
        [n + 1] (or None) and, ascending per point, the eids into eid_dev (uint32), the exact records into rec_dev (NEAR_DTYPE, or
        None) and sqrt(d^2) into dist_dev (float64, or None), each of pair_capacity entries.  pair_capacity 0 is the counting
        call.  Returns the counts as a dict (WITHIN_COUNTS); WithinOverflow (with the true counts) past the capacity.
        Synchronous."""
        return self._counted(self.L.rj_within_query, WITHIN_COUNTS, WithinOverflow, base_map_id, query_map_id, _ptr(pts_dev), int(pt_begin), int(n),
                             int(max_dist), int(pair_capacity), _ptr(offsets_dev), _ptr(eid_dev), _ptr(rec_dev), _ptr(dist_dev))

    def window_query(self, base_map_id, win_dev, nw, pair_capacity=0, offsets_dev=None, eid_dev=None, flags_dev=None):
        """rj_window_query: for nw windows (win_dev: int64 (x0, y0, x1, y1) in device memory, closed rectangles in scaled
        coordinates) every edge of the indexed base map that shares a point with the window, exactly, as a CSR: the uint64
        offsets_dev [nw + 1] (or None) and, ascending per window, the eids into eid_dev (uint32) and one byte of flags into
        flags_dev (uint8, or None: bit 0 the first point lies in the window, bit 1 the second), each of pair_capacity
        entries.  pair_capacity 0 is the counting call.  Returns the counts as a dict (WINDOW_COUNTS); WindowOverflow (with
        the true counts) past the capacity.  Synchronous."""
        return self._counted(self.L.rj_window_query, WINDOW_COUNTS, WindowOverflow, base_map_id, _ptr(win_dev), int(nw), int(pair_capacity),
                             _ptr(offsets_dev), _ptr(eid_dev), _ptr(flags_dev))

    def last_ms(self, which):
        ms = C.c_float()
        self._check(self.L.rj_last_ms(self.h, which, C.byref(ms)))
        return ms.value

    def last_ms_all(self):
        """-> list of the last duration of every stage (RJ_T_* order), -1 where a stage has not run"""
        buf = (C.c_float * 12)()
        self._check(self.L.rj_last_ms_all(self.h, buf, 12))
        return list(buf)

    def get_plan(self):
        """rj_get_plan: what the last query of each kind ran and why (a dict)"""
        import json
        need = C.c_size_t(0)
        self._check(self.L.rj_get_plan(self.h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        self._check(self.L.rj_get_plan(self.h, buf, need.value + 1, None))
        return json.loads(buf.value.decode())

    def last_stats_raw(self):
        """the 16 counters as a list (what each slot means depends on the instrumented kernel that ran: rj_kernels.hip)"""
        s = (_u64 * 16)()
        self._check(self.L.rj_last_stats(self.h, s))
        return list(s)

    def last_stats(self):
        s = (_u64 * 16)()
        self._check(self.L.rj_last_stats(self.h, s))
        return dict(leaf_blocks=s[0], exact_tests=s[1], nodes_expanded=s[2], leaf_box_tests=s[3],
                    cyc_total=s[4], cyc_node=s[5], cyc_leaf=s[6], cyc_drain=s[7], merge_rounds=s[8],
                    cyc_max_wave=s[9], cyc_sched=s[10], cyc_head=s[11], cyc_tail=s[12], stale_pops=s[13], leaf_visits_without_candidates=s[14], leaf_interested_lanes=s[15],
                    walk_stack_max=s[8])  # (k_pip_walk<STATS>: the deepest stack any group reached; k_lsi: merge_rounds)
