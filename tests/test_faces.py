"""Faces of a chain map on the CPU: the plain-Python definition (tests/faces_ref.py) on the hand-built maps of
tests/faces_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/faces_twin.cc compiling rayjoin_amd/csrc/rj_faces.h) against that definition, every array and every count,
on the hand cases and on the random planar maps of tests/rings_planar.py at the default shift and at both ends of its
range; on those maps the computed faces against the generator's construction-known faces (a bijection with 0 <-> 0, the face
count, every area, no conflict with the generator's labels); components inside the corner cells of the range, where a
cell's key is the largest there is; the floor of the grid on a map in single units; the label check on a swapped chain; the twin as a stand-alone
program.  The GPU side is tests/test_gpu_faces.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faces_cases as FC  # noqa: E402
import faces_ref as FR  # noqa: E402
import rings_planar as P  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "faces_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HDRS = [os.path.join(CSRC, name) for name in ("rj_faces.h", "rj_polygons.h", "rj_rings.h", "rj_crossings.h")]
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
OUT = os.path.join(BUILD, "libfaces_twin.so")
STATS = ("shift", "n_regs", "n_ceil", "ray_tests", "cells", "rounds")
SEEDS = list(range(40))
SHIFTS = (0, 15, 47)
NONE = FR.NONE


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


def twin_lib():
    os.makedirs(BUILD, exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC, "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.faces_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64] + [C.c_void_p] * 6
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_faces(L, xy, row_index, labels=None, shift=0, flags=0, cap=None, records=True):
    """-> (status, dict(left, right, faces cut to min(count, capacity), counts, above), dict of STATS).  cap None: room for every face"""
    xy = np.ascontiguousarray(xy, np.int64).reshape(-1, 2)
    row = np.ascontiguousarray(row_index, np.uint32)
    nc = len(row) - 1
    cap = 2 * nc if cap is None else cap
    il, ir = (None, None) if labels is None else (np.ascontiguousarray(labels[0], np.int32), np.ascontiguousarray(labels[1], np.int32))
    left, right = np.full(nc, -7, np.int32), np.full(nc, -7, np.int32)
    faces = np.zeros(cap + 1, FR.FACE_DTYPE)
    faces["leader"] = 0xABABABAB
    counts, stats, above = np.zeros(7, np.uint64), np.zeros(6, np.uint64), np.full(2 * nc + 1, 0xCDCDCDCD, np.uint32)
    rc = L.faces_twin(xy.ctypes.data, len(xy), row.ctypes.data, nc, il.ctypes.data if il is not None else None,
                      ir.ctypes.data if ir is not None else None, flags, shift, cap, left.ctypes.data, right.ctypes.data,
                      faces.ctypes.data if records else None, counts.ctypes.data, stats.ctypes.data, above.ctypes.data)
    c = dict(zip(FR.COUNTS, (int(v) for v in counts)))
    assert int(faces["leader"][cap]) == 0xABABABAB  # nothing behind the capacity
    got = dict(left=left, right=right, faces=faces[:min(c["n_faces"], cap)] if records else None, counts=c,
               above=[None if v == NONE else int(v) for v in above[:c["n_rings"]].tolist()])
    return rc, got, dict(zip(STATS, (int(v) for v in stats)))


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """-> (xy, row_index, the written answer, the definition's answer): computed once, shared, left unchanged"""
    xy, row, answer = FC.HAND[name]()
    return xy, row, answer, FR.faces_ref(xy, row)


@functools.lru_cache(maxsize=None)
def planar_case(seed):
    """-> (map, info, the definition's answer without labels)"""
    m, info = P.draw_planar(seed)
    return m, info, FR.faces_ref(m[0], m[1])


def swapped_labels(m, want):
    """the generator's labels with left / right of one chain exchanged: the first chain that bounds two different faces"""
    left, right = m[2].copy(), m[3].copy()
    c = next(c for c in range(len(left)) if want["left"][c] != want["right"][c])
    left[c], right[c] = right[c], left[c]
    return left, right


# ---- the definition against the written answers -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.HAND))
def test_definition_gives_the_written_answers(name):
    _, _, answer, got = hand_case(name)
    assert got["left"].tolist() == answer["left"] and got["right"].tolist() == answer["right"], name
    assert got["counts"] == answer["counts"], name
    assert FR.area2_of(got["faces"]) == answer["area2"] and not got["faces"]["label"].any(), name
    if answer["above"] is not None:
        assert got["above"] == answer["above"], name


def test_walk_of_length_two_and_the_half_open_rule_are_in_the_cases():
    """what the cases are for: a hole whose above is a hole; a top with two ceiling edges meeting exactly over it"""
    _, _, _, got = hand_case("island-lake-island")
    assert got["above"][5] == 7 and got["above"][7] == 2 and got["ring_face"][5] == got["ring_face"][7] == 2
    xy, _, _, _ = hand_case("shared-vertex")
    assert (5, 14) in [tuple(p) for p in xy.tolist()] and (5, 3) in [tuple(p) for p in xy.tolist()]


# ---- the twin against the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.HAND))
def test_twin_equals_the_definition_on_the_hand_cases(twin, name):
    xy, row, _, want = hand_case(name)
    for shift in SHIFTS:
        rc, got, stats = twin_faces(twin, xy, row, shift=shift)
        assert rc == 0, (name, shift)
        FR.assert_same_faces(got, want, (name, shift))
        assert got["above"] == want["above"], (name, shift)
        if len(row) > 1:
            assert stats["shift"] >= max(shift, 15), (name, shift)


CORNER_WALKS = {"corner-cell": (8, 2), "corner-cell-alone": (2, 1), "corner-cell-neighbour": (4, 2), "low-corner-cell": (8, 2)}


@pytest.mark.parametrize("name", sorted(CORNER_WALKS))
def test_the_run_of_the_largest_key_ends(twin, name):
    """components inside the corner cells of the range, at the default shift and at a forced 15: the cell of
    [2^46 - 2^15, 2^46)^2 has the largest key there is, and its run ends at the registrations' end -- the walk returns, with
    the definition's faces, having counted the entries of the runs it took (holes x the ceiling edges of their cell) and
    one cell per ray"""
    xy, row, _, want = hand_case(name)
    for shift in (0, 15):
        rc, got, stats = twin_faces(twin, xy, row, shift=shift)
        assert rc == 0 and stats["shift"] == 15, (name, shift)
        FR.assert_same_faces(got, want, (name, shift))
        assert got["above"] == want["above"], (name, shift)
        assert (stats["ray_tests"], stats["cells"]) == CORNER_WALKS[name], (name, shift)


def unit_column_walk(n):
    """diamond_column(n) drawn in single units, and in units of 2^12 -> what the rays cost in each, by the definition of the
    grid: in single units the map lies in ONE cell of the coarsest-allowed 2^15, every ray takes its run of all 4 n ceiling
    edges; in units of 2^12 every square has a cell row of its own (pitch 2^16), a ray takes its own cell's run of 4 and the
    next square's, the topmost ray only its own"""
    return (n * 4 * n, n), (8 * (n - 1) + 4, 2 * (n - 1) + 1)


def test_a_map_in_single_units_lies_in_one_cell(twin):
    """the floor of the grid, pinned: cells are at least 2^15 units wide, so a small map in unit coordinates gets the same
    faces at holes x edges candidate tests; scaled to the range it is bucketed"""
    n = 64
    xy, row = FC.diamond_column(n)
    unit, scaled = unit_column_walk(n)
    rc, got, stats = twin_faces(twin, xy, row)
    assert rc == 0 and stats["shift"] == 15 and (stats["ray_tests"], stats["cells"]) == unit
    rc, big, stats = twin_faces(twin, xy * 4096, row)
    assert rc == 0 and stats["shift"] == 15 and (stats["ray_tests"], stats["cells"]) == scaled
    assert np.array_equal(got["left"], big["left"]) and np.array_equal(got["right"], big["right"]) and got["counts"] == big["counts"]
    assert got["right"].tolist() == list(range(1, n + 1)) and not got["left"].any()


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_equals_the_definition_on_planar_maps(twin, seed):
    m, info, want = planar_case(seed)
    seen = set()
    for shift in SHIFTS:
        rc, got, stats = twin_faces(twin, m[0], m[1], shift=shift)
        assert rc == 0, (seed, shift)
        FR.assert_same_faces(got, want, (seed, shift))
        assert got["above"] == want["above"], (seed, shift)
        assert stats["n_regs"] <= 4 * stats["n_ceil"] + 1024
        seen.add(stats["shift"])
    assert 47 in seen and len(seen) >= 2, seed  # the grid really changed under the same answer


@pytest.mark.parametrize("seed", SEEDS)
def test_computed_faces_are_the_generators_faces(twin, seed):
    """relative to the generator's left / right (known from the construction, without rings): computed face -> generator
    label is a bijection with 0 <-> 0, the face count matches, every face's area2 is det x its triangles, and the generator's
    labels pass the label check"""
    m, info, want = planar_case(seed)
    assert want["counts"]["n_skipped"] == 0
    to_label = {}
    for side, given in (("left", m[2]), ("right", m[3])):
        for f, g in zip(want[side].tolist(), given.tolist()):
            assert to_label.setdefault(f, g) == g, seed
    n_faces = want["counts"]["n_faces"]
    bounded = {f: g for f, g in to_label.items() if f != 0}
    assert to_label.get(0, 0) == 0 and 0 not in bounded.values(), seed
    assert len(set(bounded.values())) == len(bounded) == n_faces == len([f for f in info["triangles"] if f != 0]), seed
    assert FR.area2_of(want["faces"]) == [info["det"] * info["triangles"][bounded[k + 1]] for k in range(n_faces)], seed
    checked = FR.faces_ref(m[0], m[1], m[2], m[3])
    assert checked["counts"]["n_conflicts"] == 0 and checked["faces"]["label"].tolist() == [bounded[k + 1] for k in range(n_faces)], seed
    rc, got, _ = twin_faces(twin, m[0], m[1], labels=(m[2], m[3]))
    assert rc == 0
    FR.assert_same_faces(got, checked, seed)


@pytest.mark.parametrize("seed", [0, 7, 23])
def test_label_check_counts_a_swapped_chain(twin, seed):
    m, _, want = planar_case(seed)
    left, right = swapped_labels(m, want)
    checked = FR.faces_ref(m[0], m[1], left, right)
    assert checked["counts"]["n_conflicts"] > 0
    rc, got, _ = twin_faces(twin, m[0], m[1], labels=(left, right))
    assert rc == 0
    FR.assert_same_faces(got, checked, seed)


# ---- the twin's contract ----------------------------------------------------------------------------------------------
def test_twin_contract(twin):
    xy, row, _, want = hand_case("island-lake-island")
    rc, got, _ = twin_faces(twin, xy, row, cap=2)  # overflow: true counts, left / right complete, two records
    assert rc == 3 and got["counts"] == want["counts"] and np.array_equal(got["left"], want["left"]) and np.array_equal(got["right"], want["right"])
    assert np.array_equal(got["faces"], want["faces"][:2])
    rc, got, _ = twin_faces(twin, xy, row, cap=0, records=False)  # no records: nothing overflows
    assert rc == 0 and got["counts"] == want["counts"] and np.array_equal(got["left"], want["left"])
    assert twin_faces(twin, xy, row, flags=1)[0] == 1
    bad = row.copy()
    bad[1] = bad[2]
    assert twin_faces(twin, xy, bad)[0] == 1
    far = xy.copy()
    far[0, 0] = 1 << 46
    assert twin_faces(twin, far, row)[0] == 1
    far[0, 0] = -(1 << 46)
    assert twin_faces(twin, far, row)[0] == 0


def test_stand_alone_twin_program():
    """the twin with its own main (what a host sanitizer build is made from: -fsanitize=address,undefined on this very
    command line), run as a program of its own: the hand map in its source at the default shift, 15 and 47"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "faces_twin_main")
    if _stale(exe):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DFACES_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "faces_twin ok" in r.stdout, r.stdout + r.stderr
