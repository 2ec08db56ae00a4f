"""Merging faces by class and re-joining chains on the device (rj_map_dissolve, ops.map_dissolve, DeviceChainMap.Dissolve /
.Join, DeviceOutputMap.Dissolve) against the plain-Python definition (tests/dissolve_ref.py), array for array and count
for count, with and without records, origin and chain_out: the hand maps of tests/dissolve_cases.py, the constructed maps
that cross a wave and a block (paths of up to 4 097 chains, loops, pairs of chains of 2 .. 1 000 points joined head to head
and tail to tail, the chains of 100 003 and 50 000 points of rings_planar.long_chains), odd labels, the 12 generated planar
maps under three class tables.  Then any grid of the point scatter, the device composition rings -> relabel -> rings_map
in canonical form, the sample pair's overlay output map end to end, Join after the eliminate rounds, the contract on the
device (sizing call, exact capacity, each capacity one short with canaries, every refusal, n_unmapped), the stage times
and the handle's state.  The CPU side is tests/test_dissolve.py."""
import json
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dissolve_cases as DC  # noqa: E402
import dissolve_ref as DR  # noqa: E402
import rings_planar as RP  # noqa: E402
from rings_cases import chain_map  # noqa: E402
from test_dissolve import EVERY, OK, SEEDS, TABLES, answer, arrays, input_of, joinable, planar, records_of, same, table_of  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A


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


def result_of(dm, records=True, origin=True):
    return DR.Result(classes=records_of(dm.classes_to_host()) if records else None, left=dm.left.to_host(np.int32, dm.n_chains),
                     right=dm.right.to_host(np.int32, dm.n_chains), xy=dm.xy.to_host(np.int64, 2 * dm.n_points).reshape(-1, 2),
                     row_index=dm.row_index.to_host(np.uint32, dm.n_chains + 1), origin=dm.origin_to_host() if origin else None,
                     chain_out=dm.chain_out_to_host() if origin else None, counts={k: dm.counts[k] for k in DR.COUNTS})


def device_dissolve(h, m, table=None, flags=0, records=True, origin=True):
    """-> (OK, Result, counts) through ops.map_dissolve, the shape that test_dissolve.same compares"""
    src = DeviceMap(h, m)
    try:
        dm = ops.map_dissolve(h, *src.args(), classes=table, keep_equal=bool(flags & DR.KEEP_EQUAL), records=records, origin=origin)
        try:
            assert isinstance(dm, ops.DeviceChainMap) and dm.counts["n_edges"] == dm.n_points - dm.n_chains
            assert (dm.classes is not None) == records and (dm.origin is not None) == origin == (dm.chain_out is not None)
            r = result_of(dm, records, origin)
            return OK, r, r.counts
        finally:
            dm.free()
    finally:
        src.free()


def check(h, what):
    m, table, flags = input_of(*what)
    want = answer(*what)
    same(device_dissolve(h, m, table, flags), want)
    same(device_dissolve(h, m, table, flags, records=False, origin=False), want, records=False, origin=False, chain_out=False)


# ---- the device against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_device_equals_the_definition(handle, what):
    check(handle, what)


@pytest.mark.parametrize("blocks", (1, 7))
def test_any_grid_gives_the_same_result(handle, blocks):
    """the debug option "dissolve_point_blocks": one block strides its 32 lane groups over every chain; 7 blocks make a
    stride that is no power of two"""
    handle.set_debug_option("dissolve_point_blocks", blocks)
    try:
        for what in (("hand", "squares-equal"), ("hand", "all-dissolve"), ("built", ("path", 4097)), ("built", ("loop", 1000)), ("built", ("pair", 65)),
                     ("built", ("pair", 1000)), ("built", ("long", 0)), ("built", ("long", 1)), ("planar", (3, 3, 0))):
            check(handle, what)
    finally:
        handle.set_debug_option("dissolve_point_blocks", 0)
    assert handle.get_debug_option("dissolve_point_blocks") == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_the_device_composition_gives_the_same_map(handle, seed):
    """face_rings -> the rings' faces relabelled -> rings_map with dissolve: the route there was before, on the device, in
    canonical form"""
    m = planar(seed)[0]
    src = DeviceMap(handle, m)
    try:
        rings = ops.face_rings(handle, *src.args())
        face = rings.rings.to_host(_capi.RING_DTYPE, rings.n_rings)["face"].astype(np.int64)
        for t in TABLES:
            table = table_of(m, t)
            ring_class = (face if table is None else np.where(face == 0, 0, table[np.clip(face, 0, len(table) - 1)])).astype(np.int32)
            buf = handle.alloc(4 * max(1, len(ring_class))).from_host(ring_class)
            comp = ops.rings_map(handle, rings.ring_row, rings.ring_xy, rings.n_points, buf, rings.n_rings, dissolve=True)
            dm = ops.map_dissolve(handle, *src.args(), classes=table)
            assert comp.counts["n_conflicts"] == 0
            a, b = result_of(dm, False, False), comp.to_host()[0]
            assert DR.canonical(a.xy, a.row_index, a.left, a.right) == DR.canonical(b.pts, b.row_index, b.left, b.right)
            for x in (buf, comp, dm):
                x.free()
        rings.free()
    finally:
        src.free()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------
def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_output_map_end_to_end():
    """the sample pair's overlay output map -> Dissolve to five classes and Join: both equal the definition, the joined map
    has the crossings of the input (the same edges), the dissolved one no more; Rings() of the result gives the class
    areas of the records; InstallMap takes the result"""
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        host = om.to_host()[0]
        m = (host.pts, host.row_index, host.left.astype(np.int32), host.right.astype(np.int32))
        f = np.arange(om.n_faces + 1)
        table = (1 + f % 5).astype(np.int32)
        table[0] = 0
        before = om.Crossings(ov.h)[1]["n_found"]
        dm = om.Dissolve(ov.h, table, records=True, origin=True)
        want = DR.dissolve_ref(*m, table, 0)
        assert isinstance(dm, ops.DeviceDissolvedMap) and want.counts["n_dropped"] > 0 and want.counts["n_chains"] < want.counts["n_kept"]
        same((OK, result_of(dm), {k: dm.counts[k] for k in DR.COUNTS}), want)
        assert dm.Crossings(ov.h)[1]["n_found"] <= before
        rings = dm.Rings(ov.h)
        sums = RP.face_sums(rings.to_host())
        assert rings.counts["n_mixed"] == 0
        assert {k: v for k, v in sums.items() if k != 0} == {int(r["label"]): (int(r["area2_hi"]) << 64) | int(r["area2_lo"]) for r in dm.classes_to_host()}
        rings.free()
        joined = om.Join(ov.h, origin=True)
        want = DR.dissolve_ref(*m, None, DR.KEEP_EQUAL)
        same((OK, result_of(joined, False), {k: joined.counts[k] for k in DR.COUNTS}), want, records=False)
        assert joined.Crossings(ov.h)[1]["n_found"] == before and joinable(want) == []
        simple = joined.Simplify(ov.h, 0)
        again = joined.Eliminate(ov.h, 0)
        assert simple.n_chains == joined.n_chains and again.n_chains <= joined.n_chains
        simple.free()
        again.free()
        joined.free()
        dctx.InstallMap(0, dm)
        got = dctx.get_map(0)
        assert np.array_equal(got.pts, want_xy(dm)) and len(got.row_index) == dm.n_chains + 1
        dm.free()
        om.free()
    finally:
        dctx.close()


def want_xy(dm):
    return dm.xy.to_host(np.int64, 2 * dm.n_points).reshape(-1, 2)


@pytest.mark.parametrize("seed", (0, 5, 9))
def test_join_after_the_eliminate_rounds_leaves_no_joinable_vertex(handle, seed):
    from test_eliminate import planar_tol
    from test_eliminate import map_of as eliminate_map
    m = eliminate_map("planar", seed)
    src = DeviceMap(handle, m)
    try:
        em = ops.map_eliminate_rounds(handle, *src.args(), planar_tol(seed), max_rounds=32)
        assert em.rounds[0]["n_dropped"] > 0
        jm = em.Join(handle, origin=True)
        r = result_of(jm, False)
        host = em.to_host()[0]
        before = DR.Result(xy=host.pts, row_index=host.row_index, left=host.left, right=host.right)
        assert len(joinable(before)) > 0 and joinable(r) == []
        assert jm.counts["n_dropped"] == 0 and jm.counts["n_kept"] + jm.counts["n_skipped"] == em.n_chains and jm.n_chains < em.n_chains
        same((OK, r, r.counts), DR.dissolve_ref(host.pts, host.row_index, host.left, host.right, None, DR.KEEP_EQUAL), records=False)
        jm.free()
        em.free()
    finally:
        src.free()


# ---- the contract ------------------------------------------------------------------------------------------------------
def canaried(h, n_bytes):
    words = n_bytes // 4 + 8
    return h.alloc(4 * words).from_host(np.full(words, CANARY, np.uint32))


def test_sizing_exact_capacity_and_one_short(handle):
    what = ("planar", (3, 3, 0))
    (m, table, flags), want = input_of(*what), answer(*what)
    c = want.counts
    caps = (c["n_classes"], c["n_chains"], c["n_points"])
    src = DeviceMap(handle, m)
    tab = handle.alloc(4 * len(table)).from_host(table)
    nc = src.n_chains
    try:
        with pytest.raises(_capi.DissolveOverflow) as e:  # the sizing call
            handle.map_dissolve(*src.args(), tab, len(table), (0, 0, 0), None, None, None, None)
        assert e.value.counts == c and e.value.code == _capi.RJ_E_OVERFLOW
        trials = [caps, tuple(v + 3 for v in caps)] + [tuple(v - (1 if j == k else 0) for j, v in enumerate(caps)) for k in range(3)]
        for kc, cc, pc in trials:
            for records in (True, False):
                bufs = [canaried(handle, 4 * cc), canaried(handle, 4 * cc), canaried(handle, 16 * pc), canaried(handle, 4 * (cc + 1)), canaried(handle, 4 * cc),
                        canaried(handle, 4 * nc), canaried(handle, 24 * kc)]
                fits = (not records or kc >= caps[0]) and cc >= caps[1] and pc >= caps[2]
                call = lambda: handle.map_dissolve(*src.args(), tab, len(table), (kc, cc, pc), *bufs[:6], bufs[6] if records else None)  # noqa: E731
                host = lambda: [b.to_host(np.uint32) for b in bufs]  # noqa: E731
                if fits:
                    assert call() == c
                    ol, orr, oxy, orow, org, cout, rec = host()
                    nk, n, npts = caps
                    got = DR.Result(classes=records_of(rec[:6 * nk].view(_capi.DISS_CLASS_DTYPE)) if records else None, left=ol[:n].view(np.int32),
                                    right=orr[:n].view(np.int32), xy=oxy[:4 * npts].view(np.int64).reshape(-1, 2), row_index=orow[:n + 1], origin=org[:n],
                                    chain_out=cout[:nc], counts=c)
                    same((OK, got, c), want, records=records)
                    assert (ol[n:] == CANARY).all() and (orr[n:] == CANARY).all() and (rec[6 * nk if records else 0:] == CANARY).all()
                    assert (oxy[4 * npts:] == CANARY).all() and (orow[n + 1:] == CANARY).all() and (org[n:] == CANARY).all() and (cout[nc:] == CANARY).all()
                else:
                    with pytest.raises(_capi.DissolveOverflow) as e:
                        call()
                    assert e.value.counts == c
                    assert all((a == CANARY).all() for a in host())  # nothing is written
                for b in bufs:
                    b.free()
    finally:
        tab.free()
        src.free()


def refused(h, m, table=None, flags=0, word=None, unmapped=0):
    src = DeviceMap(h, m)
    n, nc = src.n_points, src.n_chains
    tab = None if table is None else h.alloc(4 * max(1, len(table))).from_host(np.asarray(table, np.int32))
    bufs = [canaried(h, 4 * nc), canaried(h, 4 * nc), canaried(h, 16 * (n + nc)), canaried(h, 4 * (nc + 1)), canaried(h, 4 * nc), canaried(h, 4 * nc),
            canaried(h, 48 * nc)]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_dissolve(*src.args(), tab, 0 if table is None else len(table), (2 * nc, nc, n + nc), *bufs, flags=flags)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert getattr(e.value, "n_unmapped", 0) == unmapped
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
        assert h.get_option("dissolve_last_us0") == -1 and h.get_option("dissolve_last_us5") == -1
    finally:
        for b in bufs + ([tab] if tab is not None else []):
            b.free()
        src.free()


def test_refusals(handle):
    m = chain_map([([(0, 0), (1, 0), (2, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    same(device_dissolve(handle, m), DR.dissolve_ref(*m))
    assert handle.get_option("dissolve_last_us5") >= 0
    for bad_row in ([1, 3, 5, 7], [0, 3, 5, 6], [0, 3, 3, 7], [0, 5, 3, 7], [0, 3, 5, 8]):
        refused(handle, (m[0], np.array(bad_row, np.uint32), m[2], m[3]), word="row_index")
    for v in (1 << 46, -(1 << 46) - 1):
        bad = m[0].copy()
        bad[3, 1] = v
        refused(handle, (bad,) + m[1:], word="coordinate")
    for flags in (2, 3, 1 << 31):
        refused(handle, m, flags=flags, word="flags")
    refused(handle, m, table=[0, 5], word="class table", unmapped=2)  # label 2: the right of chain 1, the left of chain 2
    refused(handle, (m[0], m[1], np.array([-1, 1, 2], np.int32), m[3]), table=[0, 5, 5], word="class table", unmapped=1)
    for name in ("unmapped", "unmapped-negative"):
        k = DC.HAND[name]
        refused(handle, k["map"], table=k["classes"], unmapped=k["unmapped"])
        with pytest.raises(_capi.DissolveUnmapped) as e:
            device_dissolve(handle, k["map"], k["classes"])
        assert e.value.n_unmapped == k["unmapped"]
    src = DeviceMap(handle, m)
    try:
        for call in (lambda: handle.map_dissolve(*src.args(), None, 0, (0, 3, 0), None, None, None, None),  # chains wanted, nowhere to put them
                     lambda: handle.map_dissolve(*src.args(), None, 0, (0, 0, 9), None, None, None, None),  # points wanted
                     lambda: handle.map_dissolve(src.bufs[0], 3, None, None, None, 0, None, 0, (0, 0, 0), None, None, None, None),  # points without chains
                     lambda: handle.map_dissolve(src.bufs[0], 7, src.bufs[1], None, src.bufs[3], 3, None, 0, (0, 0, 0), None, None, None, None),  # labels missing
                     lambda: handle.map_dissolve(*src.args(), src.bufs[2], 0, (0, 0, 0), None, None, None, None)):  # a table without labels
            with pytest.raises(_capi.RayJoinError) as e:
                call()
            assert e.value.code == _capi.RJ_E_INVALID
        # the size limits: more chains than points, np >= 2^32, nc >= 2^31, 2 (np - nc) >= 2^32 -- refused before anything is read
        for n_points, n_chains in ((2, 3), (1 << 32, 3), (1 << 31, 1 << 31), ((1 << 31) + 3, 3)):
            with pytest.raises(_capi.RayJoinError) as e:
                handle.map_dissolve(src.bufs[0], n_points, src.bufs[1], src.bufs[2], src.bufs[3], n_chains, None, 0, (0, 0, 0), None, None, None, None)
            assert e.value.code == _capi.RJ_E_INVALID
    finally:
        src.free()


def test_a_map_where_everything_dissolves(handle):
    """that fits capacities of 0, so the sizing call, whose arrays are null, succeeds and writes nothing but the row's entry"""
    k, want = DC.HAND["all-dissolve"], answer("hand", "all-dissolve")
    src = DeviceMap(handle, k["map"])
    tab = handle.alloc(12).from_host(k["classes"])
    try:
        assert handle.map_dissolve(*src.args(), tab, 3, (0, 0, 0), None, None, None, None) == want.counts  # no overflow: it fits
        row = canaried(handle, 4)
        assert handle.map_dissolve(*src.args(), tab, 3, (0, 0, 0), None, None, None, row) == want.counts
        got = row.to_host(np.uint32)
        assert got[0] == 0 and (got[1:] == CANARY).all()
        row.free()
    finally:
        tab.free()
        src.free()


def test_no_chains(handle):
    row = handle.alloc(4).from_host(np.array([CANARY], np.uint32))
    none = dict.fromkeys(_capi.DISSOLVE_COUNTS, 0)
    assert handle.map_dissolve(None, 0, None, None, None, 0, None, 0, (0, 0, 0), None, None, None, None) == none
    assert row.to_host(np.uint32, 1)[0] == CANARY
    assert handle.map_dissolve(None, 0, None, None, None, 0, None, 0, (0, 0, 0), None, None, None, row, flags=_capi.RJ_DISS_KEEP_EQUAL) == none
    assert row.to_host(np.uint32, 1)[0] == 0
    row.free()
    points = chain_map([([(1, 1)], 4, 0), ([(2, 2)], 0, 0)])
    same(device_dissolve(handle, points, None, DR.KEEP_EQUAL), DR.dissolve_ref(*points, None, DR.KEEP_EQUAL))


# ---- the stage times, the handle ---------------------------------------------------------------------------------------------
def test_the_handle_stays_as_it_was():
    """an LSI query's result, rj_get_plan's text and the options are the same before and after a call on the handle; the stage
    times are -1 before the first call, not negative after one, and -1 again after a refused one"""
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
        assert [dctx.handle.get_option("dissolve_last_us%d" % k) for k in range(6)] == [-1] * 6
        what = ("planar", (3, 3, 0))
        same(device_dissolve(dctx.handle, *input_of(*what)), answer(*what))
        us = [dctx.handle.get_option("dissolve_last_us%d" % k) for k in range(6)]
        assert all(v >= 0 for v in us) and us[5] >= max(us[:5])
        with pytest.raises(_capi.DissolveUnmapped):
            device_dissolve(dctx.handle, DC.HAND["unmapped"]["map"], DC.HAND["unmapped"]["classes"])
        assert [dctx.handle.get_option("dissolve_last_us%d" % k) for k in range(6)] == [-1] * 6
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan and [dctx.handle.get_option(n) for n in names] == options
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
