"""The overlay's output map in scaled integers on the CPU: the plain-Python helper (tests/overlay_map_ref.py, chains
walked like the output-map writer) on a hand-built pair with the answer written out, the host twin of the device's
per-edge rule (tests/hosttwin/overlay_map_twin.cc compiling rayjoin_amd/csrc/rj_overlay_map.h) against that helper,
and the helper against the CDB file overlay_ref.write_output_chain writes.  The GPU side is tests/test_gpu_overlay_map.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ref  # noqa: E402
from test_overlay_faces import _rect_pair  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
SRC = os.path.join(ROOT, "tests", "hosttwin", "overlay_map_twin.cc")
HDRS = [os.path.join(ROOT, "rayjoin_amd", "csrc", h) for h in ("rj_overlay_map.h", "rj_overlay.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "liboverlay_map_twin.so")

PAIRS = ["sample", "lattice", "rings", "nested"]
ARRAYS = ("xy", "row_index", "left", "right", "face_pairs", "origin")


def pair(name):
    """the four pairs of tests/test_gpu_overlay_faces.py"""
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


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    P2 = C.c_void_p * 2
    L.overlay_map_twin.argtypes = [P2, P2, C.POINTER(C.c_uint64), P2, P2, P2, P2, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64,
                                   C.c_uint64] + [C.c_void_p] * 7
    return L


def twin_map(L, scaled_maps, xs, pip, drop, caps=None):
    """-> (status, dict of the arrays cut to min(count, capacity), counts)"""
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    P2 = C.c_void_p * 2
    pts = P2(*[arr(m.pts, np.int64) for m in scaled_maps])
    ri = P2(*[arr(m.row_index, np.uint32) for m in scaled_maps])
    nc = (C.c_uint64 * 2)(*[m.n_chains for m in scaled_maps])
    le = P2(*[arr(m.left, np.int32) for m in scaled_maps])
    rt = P2(*[arr(m.right, np.int32) for m in scaled_maps])
    xp = P2(*[arr(x, _capi.XSECT_DTYPE) if len(x) else None for x in xs])
    vf = P2(*[arr(p, np.int32) for p in pip])
    n = len(xs[0])
    if caps is None:
        caps = (2 * n + sum(m.n_chains for m in scaled_maps), 4 * n + sum(m.n_points for m in scaled_maps),
                2 * (2 * n + sum(m.n_chains for m in scaled_maps)))
    cc, pc, fc = caps
    xy = np.full((pc, 2), -7, np.int64)
    row = np.full(cc + 1, 0xFFFFFFFF, np.uint32)
    left = np.full(cc, -7, np.int32)
    right = np.full(cc, -7, np.int32)
    fp = np.full((fc, 2), -7, np.int32)
    origin = np.full(cc, 0xFFFFFFFF, np.uint32)
    counts = np.zeros(3, np.uint64)
    rc = L.overlay_map_twin(pts, ri, nc, le, rt, xp, vf, n, int(drop), cc, pc, fc, xy.ctypes.data, row.ctypes.data, left.ctypes.data,
                            right.ctypes.data, fp.ctypes.data, origin.ctypes.data, counts.ctypes.data)
    k, p, f = (int(v) for v in counts)
    got = dict(xy=xy[:min(p, pc)], row_index=row[:min(k, cc) + 1] if k <= cc else row[:cc], left=left[:min(k, cc)],
               right=right[:min(k, cc)], face_pairs=fp[:min(f, fc)], origin=origin[:min(k, cc)])
    return rc, got, (k, p, f)


def assert_same_map(got, want):
    for name in ARRAYS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name


def test_helper_on_two_rectangles_has_the_written_answer(oracle):
    """map 0: the square [0,4]^2 (face 1); map 1: [2,6]^2 cut at x = 3 into face 1 (west) and face 2 (east): cuts at
    (4,2), (3,4), (2,4).  Kept pieces, by hand (units of U):
      map 0's square   (4,2) (4,4) (3,4)   in face 2 of map 1: left (1,2)
                       (3,4) (2,4)         between two cuts of one edge, mid-point in face 1: left (1,1)
      map 1 chain 0    (3,2) (4,2)         inside map 0: left (1,2)
      map 1 chain 1    (2,4) (2,2) (3,2)   left (1,1)
      map 1 chain 2    (3,2) (3,4)         left (1,1), right (1,2)
    faces: (1,1) -> 1, (1,2) -> 2"""
    ctx, U = _rect_pair()
    xs, pip = F.oracle_records(oracle, ctx, 64)
    om = M.output_map(ctx.maps, xs, pip)
    assert om["face_pairs"].tolist() == [[1, 1], [1, 2]]
    assert om["row_index"].tolist() == [0, 3, 5, 7, 10, 12]
    want_xy = [(4, 2), (4, 4), (3, 4), (3, 4), (2, 4), (3, 2), (4, 2), (2, 4), (2, 2), (3, 2), (3, 2), (3, 4)]
    assert om["xy"].tolist() == [[x * U, y * U] for x, y in want_xy]
    assert om["left"].tolist() == [2, 1, 2, 1, 1]
    assert om["right"].tolist() == [0, 0, 0, 0, 2]
    assert om["origin"].tolist() == [0, 0, 1 << 31, (1 << 31) | 1, (1 << 31) | 2]
    assert om["n_one_point"] == 0
    assert_same_map(M.output_map(ctx.maps, xs, pip, drop_degenerate=True), om)


def test_helper_drops_one_point_pieces_and_keeps_the_numbering():
    """a chain whose cut falls on its own vertex: the piece between the cut and the vertex is one point"""
    U = 1 << 20
    m0 = maps.ScaledMap(0, np.array([[0, 0], [2, 0], [4, 0]], np.int64) * U, np.array([0, 3], np.uint32), np.array([5], np.int64),
                        np.array([0], np.int64))
    m1 = maps.ScaledMap(1, np.array([[2, -1], [2, 1]], np.int64) * U, np.array([0, 2], np.uint32), np.array([0], np.int64),
                        np.array([0], np.int64))
    rec = np.zeros(2, _capi.XSECT_DTYPE)  # two cuts of map 0's first edge, both at its end vertex (2, 0)
    rec["x_num"], rec["y_num"], rec["x_den"], rec["y_den"] = 2 * U, 0, 1, 1
    rec["eid"] = [[0, 0], [0, 0]]
    rec["mid_point_polygon_id"] = [9, -1]
    xs = [rec, rec]  # (map 1 has no face on either side: none of its pieces is kept)
    pip = [np.array([7, 8, 8], np.int32), np.array([0, 0], np.int32)]
    full = M.output_map([m0, m1], xs, pip)
    # pieces: (0,0)-(2,0) in 7; (2,0)-(2,0) -> one point, in 9; (2,0) (2,0) (4,0) -> (2,0) (4,0), in 8
    assert full["row_index"].tolist() == [0, 2, 3, 5] and full["n_one_point"] == 1
    assert full["face_pairs"].tolist() == [[5, 7], [5, 8], [5, 9]]
    assert full["left"].tolist() == [1, 3, 2]
    drop = M.output_map([m0, m1], xs, pip, drop_degenerate=True)
    assert drop["row_index"].tolist() == [0, 2, 4]
    assert drop["xy"].tolist() == [[0, 0], [2 * U, 0], [2 * U, 0], [4 * U, 0]]
    assert drop["face_pairs"].tolist() == [[5, 7], [5, 8], [5, 9]] and drop["left"].tolist() == [1, 2]


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


_records = {}


def records(oracle, name):
    """(ctx, xs, pip, helper pieces) of a pair, computed once per session"""
    if name not in _records:
        gs, gsize = pair(name)
        ctx = maps.Context(gs).load()
        xs, pip = F.oracle_records(oracle, ctx, gsize)
        _records[name] = (ctx, xs, pip)
    return _records[name]


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("name", PAIRS + ["rect"])
def test_host_twin_of_the_per_edge_rule_equals_the_chain_walk(oracle, twin, name, drop):
    if name == "rect":
        ctx, _ = _rect_pair()
        xs, pip = F.oracle_records(oracle, ctx, 64)
    else:
        ctx, xs, pip = records(oracle, name)
    want = M.output_map(ctx.maps, xs, pip, drop_degenerate=drop)
    rc, got, counts = twin_map(twin, ctx.maps, xs, pip, drop)
    assert rc == 0
    assert counts == (len(want["left"]), len(want["xy"]), len(want["face_pairs"]))
    assert_same_map(got, want)
    if name == "nested":
        assert want["n_one_point"] == 264


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("name", PAIRS + ["rect"])
def test_numpy_form_of_the_helper_equals_the_walk(oracle, name, drop):
    """overlay_map_ref.output_map_np (what the full-size check uses) against output_map"""
    if name == "rect":
        ctx, _ = _rect_pair()
        xs, pip = F.oracle_records(oracle, ctx, 64)
    else:
        ctx, xs, pip = records(oracle, name)
    want = M.output_map(ctx.maps, xs, pip, drop_degenerate=drop)
    got = M.output_map_np(ctx.maps, xs, pip, drop_degenerate=drop)
    assert_same_map(got, want)
    assert got["n_one_point"] == want["n_one_point"]


def test_host_twin_on_the_one_point_piece(twin):
    U = 1 << 20
    m0 = maps.ScaledMap(0, np.array([[0, 0], [2, 0], [4, 0]], np.int64) * U, np.array([0, 3], np.uint32), np.array([5], np.int64),
                        np.array([0], np.int64))
    m1 = maps.ScaledMap(1, np.array([[2, -1], [2, 1]], np.int64) * U, np.array([0, 2], np.uint32), np.array([0], np.int64),
                        np.array([0], np.int64))
    rec = np.zeros(2, _capi.XSECT_DTYPE)
    rec["x_num"], rec["y_num"], rec["x_den"], rec["y_den"] = 2 * U, 0, 1, 1
    rec["mid_point_polygon_id"] = [9, -1]
    pip = [np.array([7, 8, 8], np.int32), np.array([0, 0], np.int32)]
    for drop in (False, True):
        want = M.output_map([m0, m1], [rec, rec], pip, drop_degenerate=drop)
        rc, got, _ = twin_map(twin, [m0, m1], [rec, rec], pip, drop)
        assert rc == 0
        assert_same_map(got, want)


def test_host_twin_overflow_reports_the_true_counts(oracle, twin):
    ctx, xs, pip = records(oracle, "sample")
    want = M.output_map(ctx.maps, xs, pip)
    true = (len(want["left"]), len(want["xy"]), len(want["face_pairs"]))
    for short in range(3):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, got, counts = twin_map(twin, ctx.maps, xs, pip, False, caps)
        assert rc == 1 and counts == true
    rc, got, counts = twin_map(twin, ctx.maps, xs, pip, False, true)
    assert rc == 0
    assert_same_map(got, want)


def read_file_chains(path):
    """[(point count, left id, right id)] of a CDB file"""
    rows = []
    with open(path) as f:
        lines = f.read().split("\n")
    i = 0
    while i < len(lines) and lines[i]:
        a = lines[i].split()
        rows.append((int(a[1]), int(a[4]), int(a[5])))
        i += 1 + int(a[1])
    return rows


# chains and faces of the file, ordered pairs, pieces with fewer than two points (worked out when the output map was defined)
TABLE = {"sample": (416, 189, 189, 0), "lattice": (309839, 154461, 154461, 0), "rings": (95, 69, 70, 0), "nested": (1359, 439, 439, 264)}


@pytest.mark.parametrize("name", PAIRS)
def test_integer_map_against_the_cdb_file(oracle, tmp_path, name):
    """chain count equals the file's; per-chain point counts equal the file's (not on the nested pair, where integer
    and double duplicate removal disagree at shared vertices); ordered pair -> the file's face id is a function"""
    gs, gsize = pair(name)
    ctx = maps.Context(gs).load()
    path = str(tmp_path / "o.cdb")
    (nch, nf), xs, pip = overlay_ref.oracle_overlay(oracle, ctx, path, gsize)
    om = M.output_map(ctx.maps, xs, pip)
    rows = read_file_chains(path)
    want_ch, want_f, want_pairs, want_one = TABLE[name]
    assert (nch, nf) == (want_ch, want_f) and len(rows) == nch
    assert len(om["left"]) == nch
    assert len(om["face_pairs"]) == want_pairs and om["n_one_point"] == want_one
    assert {tuple(p) for p in om["face_pairs"].tolist()} == set(F.face_table(ctx.maps, xs, pip))
    counts = np.diff(om["row_index"].astype(np.int64))
    if name != "nested":
        assert counts.tolist() == [r[0] for r in rows]
    else:
        assert int((counts == np.array([r[0] for r in rows])).sum()) == 697
    to_file = {}
    for (lp, rp), (_, fl, fr) in zip(om["pairs"], rows):
        for p, fid in ((lp, fl), (rp, fr)):
            if p is None:
                assert fid == 0
            else:
                assert fid != 0 and to_file.setdefault(p, fid) == fid


def test_symbols_and_flag():
    assert "rj_overlay_map" in _capi.SYMBOLS and "rj_upload_map_dev" in _capi.SYMBOLS
    L = _capi.load()
    assert hasattr(L, "rj_overlay_map") and hasattr(L, "rj_upload_map_dev")
    assert _capi.RJ_OVM_DROP_DEGENERATE == 1
