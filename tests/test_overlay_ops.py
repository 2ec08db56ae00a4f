"""The overlay operations (union, difference, symmetric difference, identity; dissolved forms such as clip) on the CPU:
the plain-Python helper (tests/overlay_ops_ref.py: every piece of the chain walk, `how` / `by` applied afterwards) on
the two-rectangle pair with the answers written out by hand, the host twin of the device's per-edge rule
(tests/hosttwin/overlay_ops_twin.cc compiling rayjoin_amd/csrc/rj_overlay_ops.h) against that helper for all 5 x 3
operations, (intersection, pair) against the existing helpers, and the exact invariants that tie the operations
together.  The GPU side is tests/test_gpu_overlay_ops.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
from test_overlay_faces import _rect_pair  # noqa: E402
from test_overlay_map import assert_same_map, pair  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "overlay_ops_twin.cc")
HDRS = [os.path.join(ROOT, "rayjoin_amd", "csrc", h) for h in ("rj_overlay_ops.h", "rj_overlay_map.h", "rj_overlay.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "liboverlay_ops_twin.so")

SMALL = ["rect", "sample", "rings", "nested"]
OPS = [(how, by) for how in R.HOWS for by in R.BYS]
# pieces: all / intersection / union / difference / symdiff / identity (by pair) / intersection by map 0, and the rows
# of (union, pair) -- found by a prototype of these semantics before the device code existed
COUNTS = {"sample": (484, 416, 484, 52, 132, 439, 188, 223), "rings": (196, 95, 196, 7, 186, 99, 85, 109),
          "nested": (1588, 1359, 1588, 187, 419, 1452, 585, 499)}


def code(how, by):
    return _capi.OVERLAY_HOW[how], _capi.OVERLAY_BY[by]


_cache = {}


def records(oracle, name):
    """(ctx, xs, pip, every piece) of a pair, computed once per session"""
    if name not in _cache:
        if name == "rect":
            ctx, gsize = _rect_pair()[0], 64
        else:
            gs, gsize = pair(name)
            ctx = maps.Context(gs).load()
        xs, pip = F.oracle_records(oracle, ctx, gsize)
        _cache[name] = (ctx, xs, pip, R.all_pieces(ctx.maps, xs, pip))
    return _cache[name]


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    P2 = C.c_void_p * 2
    common = [P2, P2, C.POINTER(C.c_uint64), P2, P2, P2, P2, C.c_uint64]
    L.overlay_ops_faces_twin.argtypes = common + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32]
    L.overlay_ops_map_twin.argtypes = common + [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32]
    L.overlay_ops_selected.argtypes = [C.c_uint32, C.c_int32, C.c_int32]
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def _inputs(scaled_maps, xs, pip):
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    P2 = C.c_void_p * 2
    args = (P2(*[arr(m.pts, np.int64) for m in scaled_maps]), P2(*[arr(m.row_index, np.uint32) for m in scaled_maps]),
            (C.c_uint64 * 2)(*[m.n_chains for m in scaled_maps]), P2(*[arr(m.left, np.int32) for m in scaled_maps]),
            P2(*[arr(m.right, np.int32) for m in scaled_maps]), P2(*[arr(x, _capi.XSECT_DTYPE) if len(x) else None for x in xs]),
            P2(*[arr(p, np.int32) for p in pip]), len(xs[0]))
    return args, keep


def twin_rows(L, scaled_maps, xs, pip, how, by):
    args, keep = _inputs(scaled_maps, xs, pip)
    cap = 4 * len(xs[0]) + 2 * sum(m.n_edges for m in scaled_maps) + 4096
    face, lo, hi, nr = np.zeros(2 * cap, np.int32), np.zeros(cap, np.uint64), np.zeros(cap, np.int64), C.c_uint64(0)
    assert L.overlay_ops_faces_twin(*args, cap, face.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(nr), *code(how, by)) == 0
    return [(int(face[2 * i]), int(face[2 * i + 1]), (int(hi[i]) << 64) | int(lo[i])) for i in range(nr.value)]


def twin_map(L, scaled_maps, xs, pip, how, by, drop, caps=None):
    """-> (status, dict of the arrays cut to min(count, capacity), counts)"""
    args, keep = _inputs(scaled_maps, xs, pip)
    n = len(xs[0])
    if caps is None:
        caps = (2 * n + sum(m.n_chains for m in scaled_maps), 4 * n + sum(m.n_points for m in scaled_maps),
                2 * (2 * n + sum(m.n_chains for m in scaled_maps)))
    cc, pc, fc = caps
    xy, row = np.full((pc, 2), -7, np.int64), np.full(cc + 1, 0xFFFFFFFF, np.uint32)
    left, right, fp = np.full(cc, -7, np.int32), np.full(cc, -7, np.int32), np.full((fc, 2), -7, np.int32)
    origin, counts = np.full(cc, 0xFFFFFFFF, np.uint32), np.zeros(3, np.uint64)
    rc = L.overlay_ops_map_twin(*args, int(drop), cc, pc, fc, xy.ctypes.data, row.ctypes.data, left.ctypes.data, right.ctypes.data,
                                fp.ctypes.data, origin.ctypes.data, counts.ctypes.data, *code(how, by))
    k, p, f = (int(v) for v in counts)
    got = dict(xy=xy[:min(p, pc)], row_index=row[:min(k, cc) + 1] if k <= cc else row[:cc], left=left[:min(k, cc)],
               right=right[:min(k, cc)], face_pairs=fp[:min(f, fc)], origin=origin[:min(k, cc)])
    return rc, got, (k, p, f)


def counts_of(want):
    return (len(want["left"]), len(want["xy"]), len(want["face_pairs"]))


# ---- the helper on the two rectangles, by hand ---------------------------------------------------------------------------
# map 0: the square (0,0) (4,0) (4,4) (0,4) (0,0), face 1 on its left; cut at (4,2), (3,4), (2,4).  Its pieces:
#   P0 (0,0) (4,0) (4,2)        outside map 1 (label 0)
#   P1 (4,2) (4,4) (3,4)        in face 2 of map 1
#   P2 (3,4) (2,4)              between two cuts of one edge, mid-point in face 1
#   P3 (2,4) (0,4) (0,0)        label 0
# map 1: chain 0 (3,2) (6,2) (6,6) (3,6), face 2 left; chain 1 (3,6) (2,6) (2,2) (3,2), face 1 left; chain 2 (3,2) (3,6),
# face 1 left and face 2 right.  Their pieces:
#   P4 (3,2) (4,2)              inside map 0 (label 1)          P5 (4,2) (6,2) (6,6) (3,6)   label 0
#   P6 (3,6) (2,6) (2,4)        label 0                         P7 (2,4) (2,2) (3,2)         label 1
#   P8 (3,2) (3,4)              label 1                         P9 (3,4) (3,6)               label 0
PIECES = [[(0, 0), (4, 0), (4, 2)], [(4, 2), (4, 4), (3, 4)], [(3, 4), (2, 4)], [(2, 4), (0, 4), (0, 0)], [(3, 2), (4, 2)],
          [(4, 2), (6, 2), (6, 6), (3, 6)], [(3, 6), (2, 6), (2, 4)], [(2, 4), (2, 2), (3, 2)], [(3, 2), (3, 4)], [(3, 4), (3, 6)]]
ORIGIN = [0, 0, 0, 0, 1 << 31, 1 << 31, (1 << 31) | 1, (1 << 31) | 1, (1 << 31) | 2, (1 << 31) | 2]


def _hand(om, U, which, left, right, face_pairs):
    assert om["face_pairs"].tolist() == face_pairs
    assert om["xy"].tolist() == [[x * U, y * U] for k in which for x, y in PIECES[k]]
    assert om["row_index"].tolist() == np.r_[0, np.cumsum([len(PIECES[k]) for k in which])].tolist()
    assert om["left"].tolist() == left and om["right"].tolist() == right
    assert om["origin"].tolist() == [ORIGIN[k] for k in which]
    assert om["n_one_point"] == 0


def test_helper_on_two_rectangles_has_the_written_answers(oracle):
    ctx, U = _rect_pair()
    xs, pip = F.oracle_records(oracle, ctx, 64)
    all_ = R.all_pieces(ctx.maps, xs, pip)
    assert [p[5] for p in all_] == [[(x * U, y * U) for x, y in pc] for pc in PIECES]
    assert [p[4] for p in all_] == [0, 2, 1, 0, 1, 0, 0, 1, 1, 0]
    # union by pair: every piece; faces (0,1) -> 1, (0,2) -> 2, (1,0) -> 3, (1,1) -> 4, (1,2) -> 5.  P4's right side is
    # (face 1 of map 0, outside map 1) = 3, P9 separates map 1's two faces outside map 0
    _hand(R.output_map(all_, "union", "pair"), U, range(10), [3, 5, 4, 3, 5, 2, 1, 4, 4, 1], [0, 2, 1, 0, 3, 0, 0, 3, 5, 2],
          [[0, 1], [0, 2], [1, 0], [1, 1], [1, 2]])
    # areas in U^2 (the table holds twice that): [2,3]x[4,6]; [3,6]x[2,6] less [3,4]x[2,4]; the square less [2,4]x[2,4]
    assert R.face_rows(all_, "union", "pair") == [(0, 1, 4 * U * U), (0, 2, 20 * U * U), (1, 0, 24 * U * U), (1, 1, 4 * U * U),
                                                  (1, 2, 4 * U * U)]
    # difference: the one face (1,0); map 0's outer pieces have it on the left, map 1's inner pieces on the right
    _hand(R.output_map(all_, "difference", "pair"), U, [0, 3, 4, 7], [1, 1, 0, 0], [0, 0, 1, 1], [[1, 0]])
    assert R.face_rows(all_, "difference", "pair") == [(1, 0, 24 * U * U)]
    # clip (intersection by map 0): P8 has face 1 of map 0 on both sides and goes
    _hand(R.output_map(all_, "intersection", "map0"), U, [1, 2, 4, 7], [1, 1, 1, 1], [0, 0, 0, 0], [[1, 0]])
    assert R.face_rows(all_, "intersection", "map0") == [(1, 0, 8 * U * U)]
    # symmetric difference by pair: everything but P8 (both sides inside both maps)
    sym = R.output_map(all_, "symmetric_difference", "pair")
    assert sym["face_pairs"].tolist() == [[0, 1], [0, 2], [1, 0]] and sym["origin"].tolist() == [ORIGIN[k] for k in range(10) if k != 8]
    assert sym["left"].tolist() == [3, 0, 0, 3, 0, 2, 1, 0, 1] and sym["right"].tolist() == [0, 2, 1, 0, 3, 0, 0, 3, 2]
    # identity = all of map 0: the outside of map 0 has no face, so P5, P6, P9 go
    assert R.output_map(all_, "identity", "pair")["origin"].tolist() == [ORIGIN[k] for k in (0, 1, 2, 3, 4, 7, 8)]
    # union by map 1: map 0's boundary dissolves inside and outside map 1 alike: only map 1's chains stay, whole
    u1 = R.output_map(all_, "union", "map1")
    assert u1["origin"].tolist() == ORIGIN[4:] and u1["face_pairs"].tolist() == [[0, 1], [0, 2]]
    assert R.face_rows(all_, "union", "map1") == [(0, 1, 8 * U * U), (0, 2, 24 * U * U)]


def test_selected_is_the_table_of_the_issue(twin):
    want = {"intersection": lambda a, b: a and b, "union": lambda a, b: a or b, "difference": lambda a, b: a and not b,
            "symmetric_difference": lambda a, b: a != b, "identity": lambda a, b: a}
    for how, fn in want.items():
        for f0 in (0, 3, -1):
            for f1 in (0, 5, -1):
                assert bool(twin.overlay_ops_selected(_capi.OVERLAY_HOW[how], f0, f1)) == bool(fn(f0 != 0, f1 != 0)), (how, f0, f1)
                assert R.SELECTED[how](f0, f1) == bool(fn(f0 != 0, f1 != 0))
    assert twin.overlay_ops_selected(5, 1, 1) == 0


# ---- host twin == helper ---------------------------------------------------------------------------------------------------
def _twin_equals_helper(twin, ctx, xs, pip, all_, how, by):
    assert twin_rows(twin, ctx.maps, xs, pip, how, by) == R.face_rows(all_, how, by)
    for drop in (False, True):
        want = R.output_map(all_, how, by, drop_degenerate=drop)
        rc, got, counts = twin_map(twin, ctx.maps, xs, pip, how, by, drop)
        assert rc == 0 and counts == counts_of(want)
        assert_same_map(got, want)
    return want


@pytest.mark.parametrize("how,by", OPS)
@pytest.mark.parametrize("name", SMALL)
def test_host_twin_of_the_per_edge_rule_equals_the_helper(oracle, twin, name, how, by):
    ctx, xs, pip, all_ = records(oracle, name)
    _twin_equals_helper(twin, ctx, xs, pip, all_, how, by)


def test_host_twin_equals_the_helper_on_the_lattice_pair(oracle, twin):
    """many cuts per edge of map 0 (a long Python loop: one test for all operations)"""
    ctx, xs, pip, all_ = records(oracle, "lattice")
    for how, by in OPS:
        _twin_equals_helper(twin, ctx, xs, pip, all_, how, by)
    assert_same_map(R.output_map(all_, "intersection", "pair"), M.output_map(ctx.maps, xs, pip))
    assert R.face_rows(all_, "intersection", "pair") == F.rows(F.face_table(ctx.maps, xs, pip))
    _invariants(ctx, all_, lambda how, by: R.face_rows(all_, how, by))


@pytest.mark.parametrize("name", SMALL)
def test_intersection_by_pair_is_the_existing_overlay(oracle, twin, name):
    ctx, xs, pip, all_ = records(oracle, name)
    for drop in (False, True):
        want = M.output_map(ctx.maps, xs, pip, drop_degenerate=drop)
        assert_same_map(R.output_map(all_, "intersection", "pair", drop_degenerate=drop), want)
        assert_same_map(twin_map(twin, ctx.maps, xs, pip, "intersection", "pair", drop)[1], want)
    want = F.rows(F.face_table(ctx.maps, xs, pip))
    assert R.face_rows(all_, "intersection", "pair") == want
    assert twin_rows(twin, ctx.maps, xs, pip, "intersection", "pair") == want


def test_host_twin_overflow_reports_the_true_counts(oracle, twin):
    ctx, xs, pip, all_ = records(oracle, "sample")
    want = R.output_map(all_, "union", "pair")
    true = counts_of(want)
    for short in range(3):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, _, counts = twin_map(twin, ctx.maps, xs, pip, "union", "pair", False, caps)
        assert rc == 1 and counts == true
    rc, got, _ = twin_map(twin, ctx.maps, xs, pip, "union", "pair", False, true)
    assert rc == 0
    assert_same_map(got, want)


# ---- exact invariants ------------------------------------------------------------------------------------------------------
def _invariants(ctx, all_, rows_of):
    """rows_of(how, by) -> [(f0, f1, area2)]; all_: every piece of the same records (the conservation's right-hand side)"""
    rows = {how: rows_of(how, "pair") for how in R.HOWS}
    as_dict = {how: {(a, b): v for a, b, v in r} for how, r in rows.items()}
    for how in R.HOWS:
        assert len(as_dict[how]) == len(rows[how])
    i, u, d, s, ident = (as_dict[h] for h in R.HOWS)
    assert not set(i) & set(s) and {**i, **s} == u
    assert not set(i) & set(d) and {**i, **d} == ident
    assert all(b == 0 for _, b in d) and all((a == 0) != (b == 0) for a, b in s) and all(a != 0 and b != 0 for a, b in i)
    # conservation under (union, pair): the rows of a face sum to the face's area over its own cut boundary
    for im in range(2):
        m = ctx.maps[im]
        faces = {int(f) for f in np.r_[m.left, m.right].tolist() if f != 0}
        sums = {}
        for key, v in u.items():
            sums[key[im]] = sums.get(key[im], 0) + v
        sums.pop(0, None)
        want = R.cut_boundary_area2(all_, im)
        assert set(want) == faces and set(sums) <= faces
        assert {f: sums.get(f, 0) for f in faces} == want, im
    # clip: the row of a face is the sum of its intersection rows
    per0 = {}
    for (a, _), v in i.items():
        per0[a] = per0.get(a, 0) + v
    clip = rows_of("intersection", "map0")
    assert all(b == 0 for _, b, _ in clip)
    assert {a: v for a, _, v in clip} == per0 and len(clip) == len(per0)


@pytest.mark.parametrize("name", SMALL)
def test_exact_invariants_on_the_helpers_tables(oracle, name):
    ctx, xs, pip, all_ = records(oracle, name)
    _invariants(ctx, all_, lambda how, by: R.face_rows(all_, how, by))
    if name == "rect":  # exact cut points: the cut boundary's area is the input's shoelace area
        u = R.face_rows(all_, "union", "pair")
        assert sum(v for a, _, v in u if a == 1) == F.shoelace2(ctx.maps[0], 1)
        for g in (1, 2):
            assert sum(v for _, b, v in u if b == g) == F.shoelace2(ctx.maps[1], g)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_piece_counts_of_the_prototype(oracle, name):
    ctx, xs, pip, all_ = records(oracle, name)
    got = (len(all_),) + tuple(len(R.kept_pieces(all_, how, "pair")) for how in R.HOWS) + (
        len(R.kept_pieces(all_, "intersection", "map0")), len(R.face_rows(all_, "union", "pair")))
    assert got == COUNTS[name]


def test_symbols_and_constants():
    assert "rj_overlay_faces_op" in _capi.SYMBOLS and "rj_overlay_map_op" in _capi.SYMBOLS
    L = _capi.load()
    assert hasattr(L, "rj_overlay_faces_op") and hasattr(L, "rj_overlay_map_op")
    hdr = open(os.path.join(ROOT, "include", "rayjoin_amd.h")).read()
    for name, v in list(_capi.OVERLAY_HOW.items()) + list(_capi.OVERLAY_BY.items()):
        c = {"symmetric_difference": "RJ_OV_SYMDIFF", "pair": "RJ_OV_BY_PAIR", "map0": "RJ_OV_BY_MAP0", "map1": "RJ_OV_BY_MAP1"}.get(
            name, "RJ_OV_" + name.upper())
        assert "#define %s " % c in hdr and getattr(_capi, c) == v
        assert ("#define %s %du" % (c, v)) in " ".join(hdr.split())
