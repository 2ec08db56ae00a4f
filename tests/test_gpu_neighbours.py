"""The face adjacency table of a chain map on the device (rj_map_neighbours, ops.map_neighbours, DeviceChainMap.Neighbours,
DeviceOutputMap.Neighbours) against the plain-Python definition (tests/neighbours_ref.py), array for array and count for
count, with and without RJ_NB_VERTEX and the records: the hand maps of tests/neighbours_cases.py, the constructed maps
whose keyed sums cross a wave and a block (one pair over up to 1 000 chains, hubs of up to 257 faces), the chains of
1 .. 1 000 points, odd labels, the 12 generated planar maps and 8 label matrices.  Then any grid of the point pass,
consistency with what exists (rj_map_eliminate's best, rj_map_dissolve's areas), the sample pair's overlay output map end
to end with Join and Dissolve, the contract on the device (sizing call, exact capacity, each capacity one short with
canaries, every refusal, no chains), the stage times and the handle's state.  The CPU side is tests/test_neighbours.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eliminate_ref as ER  # noqa: E402
import neighbours_ref as NR  # noqa: E402
from rings_cases import chain_map  # noqa: E402
from test_neighbours import BOTH, EVERY, OK, answer, arrays, entries_of, faces_of, longest_border, map_of, same  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A
assert _capi.NB_FACE_DTYPE.itemsize == 64 and _capi.NB_ENTRY_DTYPE.itemsize == 32 and _capi.NEIGHBOURS_COUNTS == NR.COUNTS


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


def result_of(nb, records=True):
    offsets, entries = nb.to_host()
    indptr, indices, rows = nb.to_csr()
    assert indptr.dtype == np.int64 and indptr.tolist() == offsets.tolist() and indices.tolist() == entries["face"].tolist() and len(rows) == nb.n_entries
    return NR.Result(faces=faces_of(nb.faces_to_host()) if records else None, offsets=[int(v) for v in offsets], entries=entries_of(entries),
                     counts={k: nb.counts[k] for k in NR.COUNTS})


def device_neighbours(h, m, flags=0, records=True):
    """-> (OK, Result, counts) through ops.map_neighbours, the shape that test_neighbours.same compares"""
    src = DeviceMap(h, m)
    try:
        nb = ops.map_neighbours(h, *src.args(), vertex=bool(flags & NR.VERTEX), records=records)
        try:
            assert isinstance(nb, ops.DeviceNeighbours) and (nb.faces is not None) == records
            if not records:
                with pytest.raises(ValueError):
                    nb.faces_to_host()
            r = result_of(nb, records)
            return OK, r, r.counts
        finally:
            nb.free()
    finally:
        src.free()


def check(h, what, flags):
    m, want = map_of(*what), answer(*what, flags)
    same(device_neighbours(h, m, flags), want)
    same(device_neighbours(h, m, flags, records=False), want, records=False)


# ---- the device against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_device_equals_the_definition(handle, what, flags):
    check(handle, what, flags)


@pytest.mark.parametrize("blocks", (1, 7))
def test_any_grid_gives_the_same_result(handle, blocks):
    """the debug option "neighbours_point_blocks": one block strides its 32 lane groups over every chain; 7 blocks make a
    stride that is no power of two"""
    handle.set_debug_option("neighbours_point_blocks", blocks)
    try:
        for what in (("hub", 257), ("pair", 1000), ("long", None), ("planar", 3)):
            for flags in BOTH:
                same(device_neighbours(handle, map_of(*what), flags), answer(*what, flags))
    finally:
        handle.set_debug_option("neighbours_point_blocks", 0)
    assert handle.get_debug_option("neighbours_point_blocks") == 0


# ---- consistency with what exists -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 5, 9))
def test_the_longest_border_is_eliminates_best(handle, seed):
    """rj_map_eliminate under tol = 2^128 - 1 without RJ_ELIM_DROP: every face of area2 >= 0 with a neighbour names its best;
    that is the arg-max of this table's entries by (largest w, smaller min, smaller max)"""
    from test_eliminate import map_of as eliminate_map
    m = eliminate_map("planar", seed)
    src = DeviceMap(handle, m)
    try:
        em = ops.map_eliminate(handle, *src.args(), ER.HUGE, drop=False, faces=True)
        nb = ops.map_neighbours(handle, *src.args())
        r, recs = result_of(nb), em.faces_to_host()
        assert len(recs) == nb.n_faces > 1 and nb.counts["n_edge_pairs"] > 0 and em.counts["n_eliminated"] > 0
        for k, f in enumerate(recs):
            best = longest_border(r, k)
            area2 = (int(f["area2_hi"]) << 64) | int(f["area2_lo"])
            assert int(f["label"]) == r.faces[k]["label"] and area2 == r.faces[k]["area2"]
            assert int(f["best"]) == (best if best is not None and area2 >= 0 else int(f["label"]))
        em.free()
        nb.free()
    finally:
        src.free()


@pytest.mark.parametrize("seed", (0, 5, 9))
def test_the_areas_are_dissolves(handle, seed):
    """rj_map_dissolve with identity classes and RJ_DISS_KEEP_EQUAL keeps every chain: its class records hold the same area2
    and the same number of sides"""
    m = map_of("planar", seed)
    src = DeviceMap(handle, m)
    try:
        dm = ops.map_dissolve(handle, *src.args(), keep_equal=True, records=True)
        nb = ops.map_neighbours(handle, *src.args())
        assert dm.counts["n_skipped"] == 0
        want = {int(c["label"]): ((int(c["area2_hi"]) << 64) | int(c["area2_lo"]), int(c["n_sides"])) for c in dm.classes_to_host()}
        assert {f["label"]: (f["area2"], f["n_sides"]) for f in result_of(nb).faces} == want and len(want) > 3
        dm.free()
        nb.free()
    finally:
        src.free()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------
def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def host_map(dm):
    host = dm.to_host()[0]
    return (host.pts, host.row_index, host.left.astype(np.int32), host.right.astype(np.int32))


def test_output_map_end_to_end():
    """the sample pair's overlay output map -> Neighbours with and without the flag, Join -> Neighbours(vertex=True), Dissolve
    to five classes -> Neighbours: each equals the definition on the same map; Join changes no pair and no border, and takes
    nodes away only"""
    from test_gpu_overlay_merge import overlay_of
    dctx, ov = overlay_of(_sample_context(), None)
    try:
        om = ov.OutputMap(drop_degenerate=True, merge=True)
        m = host_map(om)
        for vertex in (False, True):
            nb = om.Neighbours(ov.h, vertex=vertex)
            same((OK, result_of(nb), nb.counts), NR.neighbours_ref(*m, NR.VERTEX if vertex else 0))
            nb.free()
        before = NR.neighbours_ref(*m, NR.VERTEX)
        assert before.counts["n_edge_pairs"] > 100
        joined = om.Join(ov.h)
        nb = joined.Neighbours(ov.h, vertex=True)
        want = NR.neighbours_ref(*host_map(joined), NR.VERTEX)
        got = result_of(nb)
        same((OK, got, nb.counts), want)
        a, b = before.pairs(), got.pairs()
        assert joined.n_chains <= om.n_chains and nb.counts["n_nodes"] <= before.counts["n_nodes"]

        assert {k: v[0] for k, v in a.items() if v[1]} == {k: v[0] for k, v in b.items() if v[1]}  # the same edge pairs with the same borders
        assert all(k in a and v[2] <= a[k][2] for k, v in b.items()) and all(v[2] >= want.pairs()[k][2] for k, v in b.items())
        nb.free()
        joined.free()
        f = np.arange(om.n_faces + 1)
        table = (1 + f % 5).astype(np.int32)
        table[0] = 0
        dm = om.Dissolve(ov.h, table)
        nb = dm.Neighbours(ov.h, vertex=True)
        assert 0 < nb.n_faces <= 5
        same((OK, result_of(nb), nb.counts), NR.neighbours_ref(*host_map(dm), NR.VERTEX))
        nb.free()
        dm.free()
        om.free()
    finally:
        dctx.close()


# ---- the contract ------------------------------------------------------------------------------------------------------
def canaried(h, n_bytes):
    words = n_bytes // 4 + 8
    return h.alloc(4 * words).from_host(np.full(words, CANARY, np.uint32))


@pytest.mark.parametrize("flags", BOTH)
def test_sizing_exact_capacity_and_one_short(handle, flags):
    what = ("planar", 3)
    m, want = map_of(*what), answer(*what, flags)
    c = want.counts
    caps = (c["n_faces"], c["n_entries"])
    src = DeviceMap(handle, m)
    try:
        with pytest.raises(_capi.NeighboursOverflow) as e:  # the sizing call
            handle.map_neighbours(*src.args(), (0, 0), flags=flags)
        assert e.value.counts == c and e.value.code == _capi.RJ_E_OVERFLOW
        trials = [caps, tuple(v + 3 for v in caps)] + [tuple(v - (1 if j == k else 0) for j, v in enumerate(caps)) for k in range(2)]
        for fc, ec in trials:
            for records in (True, False):
                bufs = [canaried(handle, 64 * fc), canaried(handle, 8 * (fc + 1)), canaried(handle, 32 * ec)]
                fits = fc >= caps[0] and ec >= caps[1]
                call = lambda: handle.map_neighbours(*src.args(), (fc, ec), bufs[0] if records else None, bufs[1], bufs[2], flags=flags)  # noqa: E731
                host = lambda: [b.to_host(np.uint32) for b in bufs]  # noqa: E731
                if fits:
                    assert call() == c
                    rec, off, ent = host()
                    nf, ne = caps
                    got = NR.Result(faces=faces_of(rec[:16 * nf].view(_capi.NB_FACE_DTYPE)) if records else None,
                                    offsets=[int(v) for v in off[:2 * (nf + 1)].view(np.uint64)], entries=entries_of(ent[:8 * ne].view(_capi.NB_ENTRY_DTYPE)), counts=c)
                    same((OK, got, c), want, records=records)
                    assert (rec[16 * nf if records else 0:] == CANARY).all() and (off[2 * (nf + 1):] == CANARY).all() and (ent[8 * ne:] == CANARY).all()
                else:
                    with pytest.raises(_capi.NeighboursOverflow) as e:
                        call()
                    assert e.value.counts == c
                    assert all((a == CANARY).all() for a in host())  # nothing is written
                for b in bufs:
                    b.free()
    finally:
        src.free()


def refused(h, m, flags=0, word=None):
    src = DeviceMap(h, m)
    nc = src.n_chains
    bufs = [canaried(h, 64 * 2 * nc), canaried(h, 8 * (2 * nc + 1)), canaried(h, 32 * 16 * nc * nc)]
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.map_neighbours(*src.args(), (2 * nc, 16 * nc * nc), *bufs, flags=flags)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
        assert h.get_option("neighbours_last_us0") == -1 and h.get_option("neighbours_last_us5") == -1
    finally:
        for b in bufs:
            b.free()
        src.free()


def test_refusals(handle):
    m = chain_map([([(0, 0), (1, 0), (2, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    for flags in BOTH:
        same(device_neighbours(handle, m, flags), NR.neighbours_ref(*m, flags))
        assert handle.get_option("neighbours_last_us5") >= 0
        for bad_row in ([1, 3, 5, 7], [0, 3, 5, 6], [0, 3, 3, 7], [0, 5, 3, 7], [0, 3, 5, 8]):
            refused(handle, (m[0], np.array(bad_row, np.uint32), m[2], m[3]), flags, word="row_index")
        for v in (1 << 46, -(1 << 46) - 1, (1 << 63) - 1):
            bad = m[0].copy()
            bad[3, 1] = v
            refused(handle, (bad,) + m[1:], flags, word="coordinate")
    for flags in (2, 3, 1 << 31):
        refused(handle, m, flags=flags, word="flags")
    src = DeviceMap(handle, m)
    try:
        for call in (lambda: handle.map_neighbours(*src.args(), (3, 0)),  # faces wanted, nowhere to put the offsets
                     lambda: handle.map_neighbours(*src.args(), (0, 9)),  # entries wanted
                     lambda: handle.map_neighbours(*src.args(), (3, 9), None, src.bufs[1], None),  # entries wanted, offsets given
                     lambda: handle.map_neighbours(src.bufs[0], 3, None, None, None, 0, (0, 0)),  # points without chains
                     lambda: handle.map_neighbours(src.bufs[0], 7, src.bufs[1], None, src.bufs[3], 3, (0, 0))):  # labels missing
            with pytest.raises(_capi.RayJoinError) as e:
                call()
            assert e.value.code == _capi.RJ_E_INVALID
        # the size limits: more chains than points, np >= 2^32, nc >= 2^31, 2 (np - nc) >= 2^32, nc >= 2^30 with the flag -- refused before anything is read
        for n_points, n_chains, flags in ((2, 3, 0), (1 << 32, 3, 0), (1 << 31, 1 << 31, 0), ((1 << 31) + 3, 3, 0), (1 << 30, 1 << 30, _capi.RJ_NB_VERTEX)):
            with pytest.raises(_capi.RayJoinError) as e:
                handle.map_neighbours(src.bufs[0], n_points, src.bufs[1], src.bufs[2], src.bufs[3], n_chains, (0, 0), flags=flags)
            assert e.value.code == _capi.RJ_E_INVALID
    finally:
        src.free()


def test_too_many_node_pairs_are_refused(handle):
    """a hub of 65 537 faces at one vertex has 65 537 x 65 536 >= 2^32 directed pairs: RJ_E_INVALID with that count, nothing
    written, the timers at -1 -- the call ends behind its extra sync, before the scratch of the pairs exists -- and the
    handle works on; rook only the same map is an ordinary one"""
    import neighbours_cases as NC
    n = NC.LIMIT_HUB
    src = DeviceMap(handle, NC.limit_hub())
    bufs = [canaried(handle, 64 * n), canaried(handle, 8 * (n + 1)), canaried(handle, 32 * 16)]
    try:
        for caps, out in (((0, 0), (None, None, None)), ((n, 16), bufs)):
            with pytest.raises(_capi.NeighboursNodePairs) as e:
                handle.map_neighbours(*src.args(), caps, *out, flags=_capi.RJ_NB_VERTEX)
            assert e.value.code == _capi.RJ_E_INVALID and e.value.n_node_pairs_raw == n * (n - 1) >= 1 << 32 and "n_node_pairs_raw" in str(e.value)
            assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
            assert [handle.get_option("neighbours_last_us%d" % k) for k in range(6)] == [-1] * 6
        counts = (C.c_uint64 * len(NR.COUNTS))(*([7] * len(NR.COUNTS)))  # the C call itself: every other count is 0
        a = src.args()
        rc = handle.L.rj_map_neighbours(handle.h, _capi._ptr(a[0]), a[1], _capi._ptr(a[2]), _capi._ptr(a[3]), _capi._ptr(a[4]), a[5], _capi.RJ_NB_VERTEX, 0, 0,
                                        None, None, None, counts)
        assert rc == _capi.RJ_E_INVALID and dict(zip(NR.COUNTS, (int(v) for v in counts))) == dict(dict.fromkeys(NR.COUNTS, 0), n_node_pairs_raw=n * (n - 1))
        same(device_neighbours(handle, map_of("hub", 257), NR.VERTEX), answer("hub", 257, NR.VERTEX))  # the handle works on
        assert handle.get_option("neighbours_last_us5") >= 0
        c = handle.map_neighbours(*src.args(), (n, 0), *bufs[:2], None)  # rook only: n faces, no pair, the offsets all 0
        assert c == dict(dict.fromkeys(NR.COUNTS, 0), n_faces=n)
        assert not bufs[1].to_host(np.uint64, n + 1).any() and bufs[0].to_host(_capi.NB_FACE_DTYPE, n)["label"].tolist() == list(range(1, n + 1))
    finally:
        for b in bufs:
            b.free()
        src.free()


def test_no_chains_and_no_faces(handle):
    off = handle.alloc(8).from_host(np.array([CANARY, CANARY], np.uint32))
    none = dict.fromkeys(_capi.NEIGHBOURS_COUNTS, 0)
    for flags in BOTH:
        assert handle.map_neighbours(None, 0, None, None, None, 0, (0, 0), flags=flags) == none
        assert (off.to_host(np.uint32, 2) == CANARY).all()
    assert handle.map_neighbours(None, 0, None, None, None, 0, (0, 0), None, off, None, flags=_capi.RJ_NB_VERTEX) == none
    assert off.to_host(np.uint64, 1)[0] == 0
    off.free()
    # a map whose labels are all 0 fits capacities of 0: the sizing call succeeds, and with the offsets given writes their one entry
    m = chain_map([([(0, 0), (5, 5)], 0, 0), ([(5, 5)], 0, 0)])
    src = DeviceMap(handle, m)
    try:
        for flags in BOTH:
            want = NR.neighbours_ref(*m, flags)
            assert handle.map_neighbours(*src.args(), (0, 0), flags=flags) == want.counts
            same(device_neighbours(handle, m, flags), want)
    finally:
        src.free()


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
        assert [dctx.handle.get_option("neighbours_last_us%d" % k) for k in range(6)] == [-1] * 6
        what = ("planar", 3)
        for flags in BOTH:
            same(device_neighbours(dctx.handle, map_of(*what), flags), answer(*what, flags))
            us = [dctx.handle.get_option("neighbours_last_us%d" % k) for k in range(6)]
            assert all(v >= 0 for v in us) and us[5] >= max(us[:5])
        bad = chain_map([([(0, 0), (1 << 46, 0)], 1, 2)])
        src = DeviceMap(dctx.handle, bad)
        with pytest.raises(_capi.RayJoinError):
            dctx.handle.map_neighbours(*src.args(), (0, 0))
        src.free()
        assert [dctx.handle.get_option("neighbours_last_us%d" % k) for k in range(6)] == [-1] * 6
        assert json.dumps(dctx.handle.get_plan(), sort_keys=True) == plan and [dctx.handle.get_option(n) for n in names] == options
        lsi.Query(1)
        assert np.array_equal(lsi.get_pairs(), before) and len(before) > 100
    finally:
        dctx.close()
