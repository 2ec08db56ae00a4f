"""RJ_OVM_MERGE_PIECES on the CPU: the families of tests/overlay_merge_pairs.py have the properties they are there for, the
host twin of the merge (tests/hosttwin/overlay_merge_twin.cc compiling pieces_join of rayjoin_amd/csrc/rj_overlay_map.h,
driven over the staged pieces the way the device drives it) equals the plain-Python definition
(tests/overlay_merge_ref.py) on every family for all 5 x 3 operations and both drop settings, the numpy form of the
definition equals the plain one, merging twice is merging once, and the constant.  The GPU side is
tests/test_gpu_overlay_merge.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_merge_pairs as P  # noqa: E402
import overlay_merge_ref as G  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
from test_overlay_map import PAIRS  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "overlay_merge_twin.cc")
HDRS = [os.path.join(ROOT, "rayjoin_amd", "csrc", h) for h in ("rj_overlay_map.h", "rj_overlay.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "liboverlay_merge_twin.so")
EVERY = P.NAMES + PAIRS


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.overlay_merge_twin.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    L.overlay_merge_joins.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_merge(L, om, drop, caps=None):
    """the twin on the staged map om (no flag) -> (status, the five arrays cut to min(count, capacity), (chains, points))"""
    xy = np.ascontiguousarray(om["xy"], np.int64)
    row, origin = np.ascontiguousarray(om["row_index"], np.uint32), np.ascontiguousarray(om["origin"], np.uint32)
    left, right = np.ascontiguousarray(om["left"], np.int32), np.ascontiguousarray(om["right"], np.int32)
    cc, pc = caps if caps is not None else (len(left), len(xy))
    out_xy, out_row = np.full((pc, 2), -7, np.int64), np.full(cc + 1, 0xFFFFFFFF, np.uint32)
    out_left, out_right, out_origin = np.full(cc, -7, np.int32), np.full(cc, -7, np.int32), np.full(cc, 0xFFFFFFFF, np.uint32)
    counts = np.zeros(2, np.uint64)
    rc = L.overlay_merge_twin(xy.ctypes.data, row.ctypes.data, left.ctypes.data, right.ctypes.data, origin.ctypes.data, len(left), int(drop),
                              cc, pc, out_xy.ctypes.data, out_row.ctypes.data, out_left.ctypes.data, out_right.ctypes.data,
                              out_origin.ctypes.data, counts.ctypes.data)
    k, p = (int(v) for v in counts)
    got = dict(xy=out_xy[:min(p, pc)], row_index=out_row[:k + 1] if k <= cc else out_row[:cc], left=out_left[:min(k, cc)],
               right=out_right[:min(k, cc)], origin=out_origin[:min(k, cc)])
    return rc, got, (k, p)


def assert_same_arrays(got, want):
    for name in G.MERGED:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("name", P.NAMES)
def test_family_has_the_property_it_is_there_for(oracle, name):
    P.preconditions(oracle, name)


def test_the_figures_the_families_were_chosen_by(oracle):
    """comb-300: 641 pieces of one chain, one chain after the merge; ties-0: one-point pieces with other faces between two
    pieces that join once they are gone"""
    assert P.preconditions(oracle, "comb-300") == {"clip_chains": 1}
    all_ = P.records(oracle, "comb-300")[4]
    assert len(R.output_map(all_, *P.CLIP)["left"]) == 641
    assert P.preconditions(oracle, "ties-0")["between"] >= 50


@pytest.mark.parametrize("name", EVERY)
def test_host_twin_equals_the_definition_for_every_operation(oracle, twin, name):
    all_ = P.records(oracle, name)[4]
    merged_something = False
    for how, by in P.HOWS_BYS:
        staged = R.output_map(all_, how, by)
        for drop in (False, True):
            unmerged = staged if not drop else R.output_map(all_, how, by, drop_degenerate=True)
            want = G.merged_map(unmerged)
            rc, got, counts = twin_merge(twin, staged, drop)
            assert rc == 0 and counts == (len(want["left"]), len(want["xy"])), (how, by, drop)
            assert_same_arrays(got, want)
            # the numpy form, and merging once more changes nothing
            assert_same_arrays(G.merged_map(unmerged, np_form=True), want)
            assert_same_arrays(G.merged_map(want, np_form=len(want["left"]) > 50000), want)  # (the lattice pair: 300 000 chains)
            if drop:
                assert np.diff(want["row_index"].astype(np.int64)).min(initial=2) >= 2, (how, by)
            merged_something |= len(want["left"]) < len(unmerged["left"])
    assert merged_something or name == "waves-ring1000"  # (the ring is not cut)


def test_definition_by_hand():
    """five chains: 1 joins 0; 2 touches 1 with another left face; 3 has 2's faces and origin but does not touch; 4 touches 3
    with another origin"""
    xy = [[0, 0], [1, 0], [1, 0], [2, 0], [2, 0], [3, 0], [4, 0], [5, 0], [5, 0], [6, 0]]
    om = dict(xy=np.array(xy, np.int64), row_index=np.array([0, 2, 4, 6, 8, 10], np.uint32), left=np.array([1, 1, 2, 2, 2], np.int32),
              right=np.array([0, 0, 0, 0, 0], np.int32), origin=np.array([7, 7, 7, 7, 8], np.uint32))
    m = G.merge_ref(*(om[n] for n in G.MERGED))
    assert m["xy"].tolist() == [[0, 0], [1, 0], [2, 0], [2, 0], [3, 0], [4, 0], [5, 0], [5, 0], [6, 0]]
    assert m["row_index"].tolist() == [0, 3, 5, 7, 9] and m["left"].tolist() == [1, 2, 2, 2] and m["origin"].tolist() == [7, 7, 7, 8]
    # a run of one-point chains on one point becomes a one-point chain; an empty map stays empty
    one = dict(xy=np.array([[3, 3]] * 3, np.int64), row_index=np.array([0, 1, 2, 3], np.uint32), left=np.array([4] * 3, np.int32),
               right=np.array([5] * 3, np.int32), origin=np.array([2] * 3, np.uint32))
    for fn in (G.merge_ref, G.merge_np):
        m = fn(*(one[n] for n in G.MERGED))
        assert m["xy"].tolist() == [[3, 3]] and m["row_index"].tolist() == [0, 1] and m["left"].tolist() == [4]
        e = fn(np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
        assert e["row_index"].tolist() == [0] and len(e["xy"]) == 0 and len(e["left"]) == 0


def test_the_rule_in_the_header(twin):
    p, q = np.array([5, -9], np.int64), np.array([5, -8], np.int64)
    j = twin.overlay_merge_joins
    assert j(3, 1, 2, p.ctypes.data, 3, 1, 2, p.ctypes.data) == 1
    assert j(3, 1, 2, p.ctypes.data, 3, 1, 2, q.ctypes.data) == 0  # do not touch
    assert j(3, 1, 2, p.ctypes.data, 3 | 1 << 31, 1, 2, p.ctypes.data) == 0  # another map
    assert j(3, 1, 2, p.ctypes.data, 4, 1, 2, p.ctypes.data) == 0  # another chain
    assert j(3, 1, 2, p.ctypes.data, 3, 0, 2, p.ctypes.data) == 0 and j(3, 1, 2, p.ctypes.data, 3, 1, 0, p.ctypes.data) == 0
    src = open(HDRS[0]).read()
    assert "pieces_join" in src and "pieces_join" in open(os.path.join(ROOT, "rayjoin_amd", "csrc", "rj_overlay_map.hip")).read()


def test_host_twin_overflow_reports_the_true_counts(oracle, twin):
    all_ = P.records(oracle, "comb-64")[4]
    staged = R.output_map(all_, "identity", "map1")
    want = G.merged_map(staged)
    true = (len(want["left"]), len(want["xy"]))
    for short in range(2):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, _, counts = twin_merge(twin, staged, False, caps)
        assert rc == 1 and counts == true
    rc, got, _ = twin_merge(twin, staged, False, true)
    assert rc == 0
    assert_same_arrays(got, want)


def test_constant_and_header():
    assert _capi.RJ_OVM_MERGE_PIECES == 2 and _capi.RJ_OVM_DROP_DEGENERATE == 1
    hdr = " ".join(open(os.path.join(ROOT, "include", "rayjoin_amd.h")).read().split())
    assert "#define RJ_OVM_MERGE_PIECES 2u" in hdr


def test_merge_kernels_keep_eight_waves_and_do_not_spill():
    """the merge's passes are streams over pieces and points: what hides their loads is waves in flight (the budget of
    tests/test_overlay_map_budgets.py, on the resource report of the build)"""
    from test_overlay_map_budgets import _kernels
    k = _kernels()
    for frag in ("k_ovm_joinILb0", "k_ovm_joinILb1", "k_ovm_merge_label", "k_ovm_merge_points"):
        hits = [v for name, v in k.items() if frag in name]
        assert len(hits) == 1, (frag, [n for n in k if "k_ovm" in n])
        assert hits[0]["VGPRs"] <= 64 and hits[0]["ScratchSize"] == 0 and hits[0]["Occupancy"] == 8, (frag, hits[0])
