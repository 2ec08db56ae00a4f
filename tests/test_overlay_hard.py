"""The overlay on the hard input families (tests/overlay_hard_pairs.py: coincident cuts, tens of cuts per edge, wave
boundaries, face ids next to 2^31, the corner of the scaled range) on the CPU: every family's preconditions, the three
host twins of the device's per-edge rules against the plain-Python helpers for all 5 x 3 operations and both drop
flags, bit for bit, and the numpy forms of the helpers (tests/overlay_ops_ref.py: output_map_np, face_rows_np -- what
the mid-size check on the device compares with) against the plain ones.  The GPU side is tests/test_gpu_overlay_hard.py."""
import os
import sys

import pytest

from rayjoin_amd import maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_faces_ref as F  # noqa: E402
import overlay_hard_pairs as H  # noqa: E402
import overlay_map_ref as M  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
import test_overlay_faces as TF  # noqa: E402
import test_overlay_map as TM  # noqa: E402
import test_overlay_ops as TO  # noqa: E402
from test_overlay_map import assert_same_map  # noqa: E402
from test_overlay_ops import OPS, _invariants, counts_of  # noqa: E402

_cache = {}


def records(oracle, name):
    """(ctx, gsize, xs, pip, every piece, brute-force pairs) of a family, preconditions asserted, once per session"""
    if name not in _cache:
        ctx, gsize = H.family(name)
        xs, pip, brute = H.preconditions(oracle, ctx, gsize)
        _cache[name] = (ctx, gsize, xs, pip, R.all_pieces(ctx.maps, xs, pip), brute)
    return _cache[name]


@pytest.fixture(scope="module")
def twins():
    return TF.twin_lib(), TM.twin_lib(), TO.twin_lib()


@pytest.mark.parametrize("name", H.NAMES)
def test_family_has_the_property_it_is_there_for(oracle, name):
    ctx, gsize = H.family(name)
    H.preconditions(oracle, ctx, gsize)


def test_the_tie_families_hold_what_the_four_pairs_do_not(oracle):
    """the figures the families were chosen by, with margin (seed 0: 851 pairs, 283 and 323 coincident cuts, 513 and 591
    mid-points, 801 one-point pieces)"""
    ctx, gsize, xs, pip, all_, brute = records(oracle, "ties-0")
    assert len(brute) == 851 and [H.coincident(xs, im) for im in range(2)] == [283, 323]
    assert [len(H.mid_points(xs, im)) for im in range(2)] == [513, 591]
    assert R.output_map(all_, "union", "pair")["n_one_point"] == 801
    # pieces that start and end at one point although they hold a vertex, and cuts AT a chain's shared vertex
    assert sum(1 for p in all_ if len(p[5]) >= 3 and len(set(p[5])) == 1) >= 20


@pytest.mark.parametrize("name", H.NAMES)
def test_host_twins_equal_the_helpers_for_every_operation(oracle, twins, name):
    ctx, gsize, xs, pip, all_, _ = records(oracle, name)
    faces_twin, map_twin, ops_twin = twins
    tables = {}
    for how, by in OPS:
        tables[how, by] = TO.twin_rows(ops_twin, ctx.maps, xs, pip, how, by)
        assert tables[how, by] == R.face_rows(all_, how, by), (how, by)
        for drop in (False, True):
            want = R.output_map(all_, how, by, drop_degenerate=drop)
            rc, got, counts = TO.twin_map(ops_twin, ctx.maps, xs, pip, how, by, drop)
            assert rc == 0 and counts == counts_of(want), (how, by, drop)
            assert_same_map(got, want)
    # (intersection, pair) through the helpers and the twins that existed before the operations
    # (on the tie families a few chains have one face on both sides: kept there, dropped by the operations)
    want_rows = F.rows(F.face_table(ctx.maps, xs, pip))
    H.assert_rows_without_op(ctx, want_rows, tables["intersection", "pair"])
    assert TF.twin_rows(faces_twin, ctx.maps, xs, pip) == want_rows
    assert H.same_face_chains(ctx) == name.startswith(("ties", "big_ids"))
    for drop in (False, True):
        want = M.output_map(ctx.maps, xs, pip, drop_degenerate=drop)
        if not H.same_face_chains(ctx):
            assert_same_map(R.output_map(all_, "intersection", "pair", drop_degenerate=drop), want)
        rc, got, counts = TM.twin_map(map_twin, ctx.maps, xs, pip, drop)
        assert rc == 0 and counts == counts_of(want)
        assert_same_map(got, want)
        assert_same_map(M.output_map_np(ctx.maps, xs, pip, drop_degenerate=drop), want)
    _invariants(ctx, all_, lambda how, by: tables[how, by])


def _np_forms_equal_the_plain_ones(ctx, xs, pip, all_):
    walk = R.walk_np(ctx.maps, xs, pip)
    sums = [R.piece_cross_sums_np(w) for w in walk]
    assert [int(v) for w in sums for v in w.tolist()] == [R.cross_sum(p[5]) for p in all_]
    for how, by in OPS:
        assert R.face_rows_np(ctx.maps, xs, pip, how, by, walk=walk, sums=sums) == R.face_rows(all_, how, by), (how, by)
        for drop in (False, True):
            want = R.output_map(all_, how, by, drop_degenerate=drop)
            got = R.output_map_np(ctx.maps, xs, pip, how, by, drop_degenerate=drop, walk=walk)
            assert_same_map(got, want)
            assert got["n_one_point"] == want["n_one_point"], (how, by, drop)
    # without the walk handed in
    assert R.face_rows_np(ctx.maps, xs, pip, "union", "pair") == R.face_rows(all_, "union", "pair")


@pytest.mark.parametrize("name", H.NAMES)
def test_numpy_forms_equal_the_plain_helpers_on_the_families(oracle, name):
    ctx, gsize, xs, pip, all_, _ = records(oracle, name)
    _np_forms_equal_the_plain_ones(ctx, xs, pip, all_)


@pytest.mark.parametrize("name", ["rect"] + TM.PAIRS)
def test_numpy_forms_equal_the_plain_helpers_on_the_existing_pairs(oracle, name):
    ctx, xs, pip, all_ = TO.records(oracle, name)
    _np_forms_equal_the_plain_ones(ctx, xs, pip, all_)


def test_numpy_keys_are_the_plain_keys():
    import numpy as np
    f = np.array([0, 0, 3, 3, (1 << 31) - 1, (1 << 31) - 1, 0], np.int64)
    g = np.array([0, 5, 0, 5, 0, (1 << 31) - 1, (1 << 31) - 1], np.int64)
    for how, by in OPS:
        want = [R.key_of((int(a), int(b)), how, by) for a, b in zip(f, g)]
        assert R._keys_np(f, g, how, by).tolist() == [-1 if k is None else R._sort_key(k) for k in want], (how, by)


def test_trimmed_and_keep_chains():
    from rayjoin_amd import synth
    g = synth.lattice_map(2, 6, 92)
    for n in (72, 66, 65, 61, 7, 6, 1):
        t = H.trimmed(g, n)
        assert t.n_edges == n and int(t.row_index[-1]) == t.n_points
        probe = maps.Context([t]).load().maps[0]
        assert probe.n_edges == n and (t.points == g.points[:t.n_points]).all()
        assert t.chains[:, 2].tolist() == (t.row_index[1:].astype(int) - 1).tolist()
