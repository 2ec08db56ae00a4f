"""The overlay's face table on the CPU: the plain-Python oracle (tests/overlay_faces_ref.py, chains walked like the
output-map writer) on a hand-built pair with known integer answers, and the host twin of the device's per-edge rule
(tests/hosttwin/overlay_faces_twin.cc compiling rayjoin_amd/csrc/rj_overlay.h) against that oracle: identical tables.
The GPU side is tests/test_gpu_overlay_faces.py."""
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

D = os.path.join(ROOT, "tests", "golden", "sample_pair")
SRC = os.path.join(ROOT, "tests", "hosttwin", "overlay_faces_twin.cc")
HDR = os.path.join(ROOT, "rayjoin_amd", "csrc", "rj_overlay.h")
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "liboverlay_faces_twin.so")


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDR), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    P2 = C.c_void_p * 2
    L.overlay_faces_twin.argtypes = [P2, P2, C.POINTER(C.c_uint64), P2, P2, P2, P2, C.c_uint64, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    return L


def twin_rows(L, scaled_maps, xs, pip):
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
    cap = 4 * n + 2 * sum(m.n_edges for m in scaled_maps) + 4096
    face = np.zeros(2 * cap, np.int32)
    lo = np.zeros(cap, np.uint64)
    hi = np.zeros(cap, np.int64)
    nr = C.c_uint64(0)
    assert L.overlay_faces_twin(pts, ri, nc, le, rt, xp, vf, n, cap, face.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(nr)) == 0
    k = nr.value
    return [(int(face[2 * i]), int(face[2 * i + 1]), (int(hi[i]) << 64) | int(lo[i])) for i in range(k)]


def geometry_pair():
    return (synth.lattice_map(4, 60, 71, bbox=(-100.0, 30.0, -90.0, 40.0)),
            synth.lattice_map(7, 40, 72, bbox=(-102.0, 28.0, -88.0, 42.0)))


def _scaled_ctx(m0, m1):
    ctx = maps.Context([None, None])
    ctx.set_map(0, m0)
    ctx.set_map(1, m1)
    return ctx


def _rect_pair():
    """map 0: the square [0,4]^2, face 1; map 1: the square [2,6]^2 cut at x = 3 into face 1 (west) and face 2 (east).
    Scaled coordinates in units of 2^30: every crossing is an integer point."""
    U = 1 << 30
    sq = np.array([[0, 0], [4, 0], [4, 4], [0, 4], [0, 0]], np.int64) * U
    m0 = maps.ScaledMap(0, sq, np.array([0, 5], np.uint32), np.array([1], np.int64), np.array([0], np.int64))
    a = [[3, 2], [6, 2], [6, 6], [3, 6]]   # face 2 on its left
    b = [[3, 6], [2, 6], [2, 2], [3, 2]]   # face 1 on its left
    c = [[3, 2], [3, 6]]                   # upwards: face 1 on the left, face 2 on the right
    pts = np.array(a + b + c, np.int64) * U
    m1 = maps.ScaledMap(1, pts, np.array([0, 4, 8, 10], np.uint32), np.array([2, 1, 1], np.int64), np.array([0, 0, 2], np.int64))
    return _scaled_ctx(m0, m1), U


def test_oracle_on_two_rectangles_has_the_integer_answer(oracle):
    ctx, U = _rect_pair()
    got, xs, pip = F.oracle_face_rows(oracle, ctx, 64)
    assert len(xs[0]) == 3  # (4,2) on map 0's east edge, (3,4) and (2,4) on its north edge
    # overlaps: [2,3] x [2,4] with face 1 and [3,4] x [2,4] with face 2, 2 U^2 each: area2 = 4 U^2
    assert got == [(1, 1, 4 * U * U), (1, 2, 4 * U * U)]


def test_oracle_rows_sum_to_the_faces_shoelace_area(oracle):
    """map 1 a lattice over a box strictly larger than map 0's: every face of map 0 is covered (short segments: the
    grid oracle finds every crossing at any grid size)"""
    g0, g1 = geometry_pair()
    ctx = maps.Context([g0, g1]).load()
    got, _, _ = F.oracle_face_rows(oracle, ctx, 256)
    assert all(a > 0 for _, _, a in got)
    per0 = {}
    for f0, _, a in got:
        per0[f0] = per0.get(f0, 0) + a
    for f0 in range(1, 17):
        want = F.shoelace2(ctx.maps[0], f0)
        assert abs(per0[f0] - want) <= 1e-9 * want, f0


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


@pytest.mark.parametrize("pair", ["sample", "lattice", "rect"])
def test_host_twin_of_the_per_edge_rule_equals_the_chain_walk(oracle, twin, pair):
    if pair == "rect":
        ctx, _ = _rect_pair()
        gs = 64
    elif pair == "sample":
        ctx = maps.Context([maps.read_cdb(os.path.join(D, "map0.cdb")), maps.read_cdb(os.path.join(D, "map1.cdb"))]).load()
        gs = 512
    else:
        ctx = maps.Context([synth.lattice_map(3, 90, 61), synth.lattice_map(200, 1, 62)]).load()
        gs = 1024
    want, xs, pip = F.oracle_face_rows(oracle, ctx, gs)
    assert len(want) > (1 if pair == "rect" else 20)
    got = twin_rows(twin, ctx.maps, xs, pip)
    assert got == want
    if pair == "lattice":  # many cuts per edge of map 0
        e = xs[0]["eid"][:, 0].astype(np.int64)
        assert (np.diff(e) == 0).sum() > 200


def test_unordered_pairs_are_the_output_maps_faces(oracle, tmp_path):
    """the {min, max} pairs of the table are what the writer numbers as faces ("Total faces")"""
    import overlay_ref
    ctx = maps.Context([maps.read_cdb(os.path.join(D, "map0.cdb")), maps.read_cdb(os.path.join(D, "map1.cdb"))]).load()
    (_, nfc), xs, pip = overlay_ref.oracle_overlay(oracle, ctx, str(tmp_path / "o.txt"), 512)
    rows = F.rows(F.face_table(ctx.maps, xs, pip))
    assert len({(min(a, b), max(a, b)) for a, b, _ in rows}) == nfc


def test_face_record_layout_and_symbol():
    assert _capi.FACE_DTYPE.itemsize == 24
    assert "rj_overlay_faces" in _capi.SYMBOLS
    assert hasattr(_capi.load(), "rj_overlay_faces")
