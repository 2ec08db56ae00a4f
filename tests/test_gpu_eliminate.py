"""Merging sliver faces into a neighbour on the device (rj_map_eliminate, ops.map_eliminate, ops.map_eliminate_rounds,
DeviceChainMap.Eliminate, DeviceOutputMap.Eliminate) against the plain-Python definition (tests/eliminate_ref.py), array
for array and count for count, with and without RJ_ELIM_DROP, with and without records: the hand maps of
tests/eliminate_cases.py, the structural maps (chains of 1, 2, 63 .. 66 and 1 000 points; 300 two-point chains in a row: many
chains in one wave; lengths at a square near 2^47), odd labels, the 12 generated planar maps, and the chains of 100 003
and 50 000 points of rings_planar.long_chains, where the choice of a face hangs on one unit of a length summed over
1 563 waves.  Then the contract on the device (sizing call, exact capacity, each capacity one short with canaries, every
refusal), the sample pair's overlay output map end to end, a second call after the rounds, the stage times and the
handle's state.  The CPU side is tests/test_eliminate.py."""
import functools
import json
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eliminate_cases as EC  # noqa: E402
import eliminate_ref as ER  # noqa: E402
import rings_planar as RP  # noqa: E402
from rings_cases import chain_map  # noqa: E402
from test_eliminate import EVERY, OK, SEEDS, arrays, faces_of, map_of, merged, planar_tol, same  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A
HUGE = ER.HUGE


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


class DeviceMap:
    """a labelled chain map in device buffers"""

    def __init__(self, h, m):
        xy, row, left, right = arrays(m)
        self.n_points, self.n_chains = len(xy), max(0, len(row) - 1)
        self.bufs = [h.alloc(16 * max(1, len(xy))).from_host(xy), h.alloc(4 * max(1, len(row))).from_host(row),
                     h.alloc(4 * max(1, len(left))).from_host(left), h.alloc(4 * max(1, len(right))).from_host(right)]

    def args(self):
        return (self.bufs[0], self.n_points, self.bufs[1], self.bufs[2], self.bufs[3], self.n_chains)

    def free(self):
        for b in self.bufs:
            b.free()


def result_of(em, drop, records):
    xy, row = em.xy.to_host(np.int64, 2 * em.n_points).reshape(-1, 2), em.row_index.to_host(np.uint32, em.n_chains + 1)
    counts = {k: em.counts[k] for k in ER.COUNTS}
    return ER.Result(faces=faces_of(em.faces_to_host()) if records else None, left=em.left.to_host(np.int32, em.n_chains),
                     right=em.right.to_host(np.int32, em.n_chains), xy=xy if drop else None, row_index=row if drop else None,
                     origin=em.origin_to_host() if drop else None, counts=counts), xy, row


def device_eliminate(h, m, tol, flags=0, records=True):
    """-> (OK, Result, counts) through ops.map_eliminate, the shape that test_eliminate.same compares"""
    dm = DeviceMap(h, m)
    drop = bool(flags & ER.DROP)
    try:
        em = ops.map_eliminate(h, *dm.args(), tol, drop=drop, faces=records)
        try:
            r, xy, row = result_of(em, drop, records)
            if not drop:  # the map is a copy of the input's
                assert np.array_equal(xy, arrays(m)[0]) and np.array_equal(row, arrays(m)[1]) and em.origin is None
            assert em.counts["n_edges"] == em.n_points - em.n_chains
            return OK, r, r.counts
        finally:
            em.free()
    finally:
        dm.free()


def check(h, what):
    m = map_of(*what[:2])
    for flags in (0, ER.DROP):
        want = merged(*what, flags)
        same(device_eliminate(h, m, what[2], flags), want)
        same(device_eliminate(h, m, what[2], flags, records=False), want, records=False)


# ---- the device against the definition and the written answers -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.HAND))
def test_hand_cases(handle, name):
    _, tol, faces, _, _ = EC.HAND[name]
    assert {f["label"]: (f["target"], f["best"], f["flags"], f["area2"]) for f in merged("hand", name, tol, 0).faces} == faces
    check(handle, ("hand", name, tol))


@pytest.mark.parametrize("what", [w for w in EVERY if w[0] not in ("hand", "planar")], ids=str)
def test_structural_maps(handle, what):
    check(handle, what)


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_maps(handle, seed):
    want = merged("planar", seed, planar_tol(seed), 0)
    assert want.counts["n_slivers"] >= 1
    check(handle, ("planar", seed, planar_tol(seed)))


def long_map():
    """rings_planar.long_chains (100 003, 50 000 and 100 083 points) with labels that make the lengths decide: the outer
    chain twice, between faces 1 | 3 and 1 | 6, and one edge of length 1 more between 1 and 3: best(1) = 3 only if both copies
    of the long chain sum to the same number, to the unit"""
    xy, row, _, _ = RP.long_chains()
    pts = [tuple(p) for p in xy.tolist()]
    c = [pts[row[k]:row[k + 1]] for k in range(3)]
    return chain_map([(c[0], 1, 3), ([(7, 7)], 9, 9), (c[1], 4, 5), (c[2], 1, 2), ([(0, 0), (1, 0)], 1, 3), (c[0], 1, 6)])


@functools.lru_cache(maxsize=None)
def long_answer():
    """(the map, the definition's answer at 2^128 - 1 under RJ_ELIM_DROP): computed once, shared, never changed"""
    m = long_map()
    return m, ER.eliminate_ref(*m, HUGE, ER.DROP)


@pytest.mark.parametrize("blocks", (1, 3, 64))
def test_any_grid_gives_the_same_result(handle, blocks):
    """the debug option "elim_point_blocks": with one block a wave runs through 1 370 steps of the long chains and hands the
    chain of its last point from step to step (at the default grid these maps give a wave one step); 3 blocks make runs
    that end inside chains"""
    handle.set_debug_option("elim_point_blocks", blocks)
    try:
        for what in (("lengths", None, 1 << 90), ("row", None, 1 << 100), ("planar", 3, planar_tol(3)), ("hand", "all-dropped", 1000)):
            check(handle, what)
        m, want = long_answer()
        same(device_eliminate(handle, m, HUGE, ER.DROP), want)
    finally:
        handle.set_debug_option("elim_point_blocks", 0)
    assert handle.get_debug_option("elim_point_blocks") == 0


def test_long_chains(handle):
    """the chain sums of 100 003 and 50 000 points against Python integers: every area2, and the weights through the choices"""
    m, want = long_answer()
    by = {f["label"]: f for f in want.faces}
    assert want.L[0] == want.L[5] > 1 << 42 and by[1]["best"] == 3 and abs(by[3]["area2"]) > 1 << 80 and want.counts["n_negative"] > 0
    same(device_eliminate(handle, m, HUGE, ER.DROP), want)
    same(device_eliminate(handle, m, 0, 0), ER.eliminate_ref(*m, 0, 0))


# ---- the contract ------------------------------------------------------------------------------------------------------
def canaried(h, n_bytes):
    words = n_bytes // 4 + 8
    return h.alloc(4 * words).from_host(np.full(words, CANARY, np.uint32))


def test_sizing_exact_capacity_and_one_short(handle):
    m, tol = map_of("planar", 3), planar_tol(3)
    dm = DeviceMap(handle, m)
    try:
        for flags in (0, ER.DROP):
            want = merged("planar", 3, tol, flags)
            c = want.counts
            caps = (c["n_faces"], c["n_chains"], c["n_points"])
            with pytest.raises(_capi.EliminateOverflow) as e:  # the sizing call
                handle.map_eliminate(*dm.args(), tol, (0, 0, 0), None, None, flags=flags)
            assert e.value.counts == c and e.value.code == _capi.RJ_E_OVERFLOW
            trials = [caps, tuple(v + 3 for v in caps)] + [tuple(v - (1 if j == k else 0) for j, v in enumerate(caps)) for k in range(3)]
            for fc, cc, pc in trials:
                for records in (True, False):
                    bufs = [canaried(handle, 4 * cc), canaried(handle, 4 * cc), canaried(handle, 16 * pc), canaried(handle, 4 * (cc + 1)),
                            canaried(handle, 4 * cc), canaried(handle, 32 * fc)]
                    fits = (not records or fc >= caps[0]) and cc >= caps[1] and (not flags or pc >= caps[2])
                    call = lambda: handle.map_eliminate(*dm.args(), tol, (fc, cc, pc), *bufs[:5], bufs[5] if records else None, flags=flags)  # noqa: E731
                    host = lambda: [b.to_host(np.uint32) for b in bufs]  # noqa: E731
                    if fits:
                        assert call() == c
                        ol, orr, oxy, orow, org, fac = host()
                        nf, n, npts = caps
                        got = ER.Result(faces=faces_of(fac[:8 * nf].view(_capi.ELIM_FACE_DTYPE)) if records else None, left=ol[:n].view(np.int32),
                                        right=orr[:n].view(np.int32), xy=oxy[:4 * npts].view(np.int64).reshape(-1, 2) if flags else None,
                                        row_index=orow[:n + 1] if flags else None, origin=org[:n] if flags else None, counts=c)
                        same((OK, got, c), want, records=records)
                        assert (ol[n:] == CANARY).all() and (orr[n:] == CANARY).all() and (fac[8 * nf if records else 0:] == CANARY).all()
                        if flags:
                            assert (oxy[4 * npts:] == CANARY).all() and (orow[n + 1:] == CANARY).all() and (org[n:] == CANARY).all()
                        else:
                            assert (oxy == CANARY).all() and (orow == CANARY).all() and (org == CANARY).all()
                    else:
                        with pytest.raises(_capi.EliminateOverflow) as e:
                            call()
                        assert e.value.counts == c
                        assert all((a == CANARY).all() for a in host())  # nothing is written
                    for b in bufs:
                        b.free()
    finally:
        dm.free()


def refused(h, m, tol=0, flags=0, word=None):
    dm = DeviceMap(h, m)
    n, nc = dm.n_points, dm.n_chains
    bufs = [canaried(h, 4 * nc), canaried(h, 4 * nc), canaried(h, 16 * n), canaried(h, 4 * (nc + 1)), canaried(h, 4 * nc), canaried(h, 64 * nc)]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_eliminate(*dm.args(), tol, (2 * nc, nc, n), *bufs, flags=flags)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
    finally:
        for b in bufs:
            b.free()
        dm.free()


def test_refusals(handle):
    m = chain_map([([(0, 0), (1, 0), (2, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    for bad_row in ([1, 3, 5, 7], [0, 3, 5, 6], [0, 3, 3, 7], [0, 5, 3, 7]):
        refused(handle, (m[0], np.array(bad_row, np.uint32), m[2], m[3]), flags=ER.DROP, word="row_index")
    for v in (1 << 46, -(1 << 46) - 1):
        bad = m[0].copy()
        bad[3, 1] = v
        refused(handle, (bad,) + m[1:], word="coordinate")
    for flags in (2, 3, 1 << 31):
        refused(handle, m, flags=flags, word="flags")
    dm = DeviceMap(handle, m)
    with pytest.raises(_capi.RayJoinError) as e:  # chains wanted, nowhere to put them
        handle.map_eliminate(*dm.args(), 0, (0, 3, 0), None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # points without chains
        handle.map_eliminate(dm.bufs[0], 3, None, None, None, 0, 0, (0, 0, 0), None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    with pytest.raises(_capi.RayJoinError) as e:  # labels missing
        handle.map_eliminate(dm.bufs[0], 7, dm.bufs[1], None, dm.bufs[3], 3, 0, (0, 0, 0), None, None)
    assert e.value.code == _capi.RJ_E_INVALID
    for tol in (-1, 1 << 128):
        with pytest.raises(ValueError):
            handle.map_eliminate(*dm.args(), tol, (0, 0, 0), None, None)
    # the size limits: more chains than points, np >= 2^32, nc >= 2^31, 2 (np - nc) >= 2^32 -- refused before anything is read
    for n_points, n_chains in ((2, 3), (1 << 32, 3), (1 << 31, 1 << 31), ((1 << 31) + 3, 3)):
        with pytest.raises(_capi.RayJoinError) as e:
            handle.map_eliminate(dm.bufs[0], n_points, dm.bufs[1], dm.bufs[2], dm.bufs[3], n_chains, 0, (0, 0, 0), None, None)
        assert e.value.code == _capi.RJ_E_INVALID
    dm.free()


def test_a_map_that_loses_every_chain(handle):
    """no face 0: everything merges into the outside face and RJ_ELIM_DROP leaves no chain.  That fits capacities of 0, so
    the sizing call, whose arrays are null, succeeds and writes nothing; the rounds end on the empty map"""
    m, tol, _, _, _ = EC.HAND["all-dropped"]
    want = merged("hand", "all-dropped", tol, ER.DROP)
    assert want.counts["n_chains"] == 0 and want.counts["n_dropped"] == 1
    dm = DeviceMap(handle, m)
    try:
        assert handle.map_eliminate(*dm.args(), tol, (0, 0, 0), None, None, flags=_capi.RJ_ELIM_DROP) == want.counts  # no overflow: it fits
        row = canaried(handle, 4)
        assert handle.map_eliminate(*dm.args(), tol, (0, 0, 0), None, None, None, row, flags=_capi.RJ_ELIM_DROP) == want.counts
        got = row.to_host(np.uint32)
        assert got[0] == 0 and (got[1:] == CANARY).all()
        row.free()
        same(device_eliminate(handle, m, tol, ER.DROP), want)
        em = ops.map_eliminate_rounds(handle, *dm.args(), tol)
        none = dict(dict.fromkeys(ER.COUNTS, 0), n_edges=0)
        assert em.rounds == [dict(want.counts, n_edges=0), none] and em.n_chains == 0 and em.n_points == 0
        assert em.row_index.to_host(np.uint32, 1)[0] == 0
        em.free()
    finally:
        dm.free()


def test_no_chains(handle):
    row = handle.alloc(4).from_host(np.array([CANARY], np.uint32))
    none = dict.fromkeys(_capi.ELIMINATE_COUNTS, 0)
    assert handle.map_eliminate(None, 0, None, None, None, 0, 7, (0, 0, 0), None, None) == none
    assert row.to_host(np.uint32, 1)[0] == CANARY
    assert handle.map_eliminate(None, 0, None, None, None, 0, 7, (0, 0, 0), None, None, None, row, flags=_capi.RJ_ELIM_DROP) == none
    assert row.to_host(np.uint32, 1)[0] == 0
    row.free()
    points = chain_map([([(1, 1)], 4, 0), ([(2, 2)], 0, 0)])
    same(device_eliminate(handle, points, HUGE, ER.DROP), ER.eliminate_ref(*points, HUGE, ER.DROP))


# ---- the rounds, the stage times ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 5, 9))
def test_a_call_after_the_rounds_eliminates_nothing(handle, seed):
    m, tol = map_of("planar", seed), planar_tol(seed)
    want, per_round = ER.rounds_ref(*m, tol, max_rounds=32)
    dm = DeviceMap(handle, m)
    try:
        em = ops.map_eliminate_rounds(handle, *dm.args(), tol, max_rounds=32, faces=True)
        assert em.rounds == [dict(c, n_edges=c["n_points"] - c["n_chains"]) for c in per_round] and em.rounds[-1]["n_eliminated"] == 0
        assert len(em.rounds) >= 2
        same((OK, result_of(em, True, True)[0], want.counts), want)
        again = em.Eliminate(handle, tol, faces=True)
        assert again.counts["n_eliminated"] == 0 and again.counts["n_dropped"] == 0 and again.n_chains == em.n_chains
        assert np.array_equal(again.origin_to_host(), np.arange(em.n_chains)) and np.array_equal(again.faces_to_host(), em.faces_to_host())
        us = [handle.get_option("elim_last_us%d" % k) for k in range(6)]
        assert all(v >= 0 for v in us) and us[5] >= max(us[:5])
        again.free()
        em.free()
    finally:
        dm.free()


# ---- the wrappers, the handle ----------------------------------------------------------------------------------------------
def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_output_map_end_to_end():
    """the sample pair's overlay output map -> Eliminate(tol): tol is the lower quartile of the definition's own face areas, so
    faces fall under it; the result has no more crossings than before, its labels still describe its geometry, and the
    summed area is what it was"""
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        host = om.to_host()[0]
        m = (host.pts, host.row_index, host.left, host.right)
        areas = sorted(f["area2"] for f in ER.eliminate_ref(*m, 0).faces if f["area2"] >= 0)
        assert len(areas) > 20
        tol = areas[len(areas) // 4]
        want = ER.eliminate_ref(*m, tol, ER.DROP)
        before = om.Crossings(ov.h)[1]["n_found"]
        faced = ops.map_faces(ov.h, om.xy, om.n_points, om.row_index, om.n_chains, labels=(om.left, om.right), records=False)
        conflicts = faced.counts["n_conflicts"]
        faced.free()
        em = om.Eliminate(ov.h, tol, faces=True)
        assert isinstance(em, ops.DeviceChainMap) and em.counts["n_eliminated"] > 0 and em.counts["n_dropped"] > 0
        same((OK, result_of(em, True, True)[0], {k: em.counts[k] for k in ER.COUNTS}), want)
        assert em.Crossings(ov.h)[1]["n_found"] <= before
        checked = em.Faces(ov.h, check=True)
        assert conflicts != 0 or checked.counts["n_conflicts"] == 0
        checked.free()
        after = ER.eliminate_ref(want.xy, want.row_index, want.left, want.right, 0)
        assert sum(f["area2"] for f in after.faces) == sum(f["area2"] for f in want.faces)
        rounds = om.Eliminate(ov.h, tol, rounds=8)
        assert rounds.rounds[0] == em.counts and (rounds.rounds[-1]["n_eliminated"] == 0 or len(rounds.rounds) == 8)
        rounds.free()
        rings = em.Rings(ov.h)
        assert rings.n_rings > 0
        rings.free()
        em.free()
        om.free()
    finally:
        dctx.close()


def test_the_handle_stays_as_it_was():
    """an LSI query's result, rj_get_plan's text and the options are the same before and after a call on the handle"""
    dctx = ops.DeviceContext(_sample_context()).LoadToDevice()
    try:
        dctx.BuildIndex(0)
        lsi = ops.LSILBVH(dctx)
        lsi.Init(4 * (dctx.get_map(0).n_edges + dctx.get_map(1).n_edges))
        lsi.Query(1)
        before = lsi.get_pairs().copy()
        names = ("leaf_order", "skyline", "pip_columns", "leaf_ysort", "pip_walk", "lsi_segments", "query_order", "timers", "stats")
        options = [dctx.handle.get_option(n) for n in names]
        plan = json.dumps(dctx.handle.get_plan(), sort_keys=True)
        assert dctx.handle.get_option("elim_last_us5") == -1
        same(device_eliminate(dctx.handle, map_of("planar", 3), planar_tol(3), ER.DROP), merged("planar", 3, planar_tol(3), ER.DROP))
        assert dctx.handle.get_option("elim_last_us5") >= 0
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan and [dctx.handle.get_option(n) for n in names] == options
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
