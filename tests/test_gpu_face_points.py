"""Per-face counts, sums and members of located points on the device (rj_face_points, ops.face_points, PIPLBVH.Summarize,
DeviceNeighbours.labels) against the plain-Python definition (tests/face_points_ref.py), array for array and count for
count, with and without values, universe, RJ_FP_MEMBERS and the records: the hand cases of tests/face_points_cases.py, the
layouts on which the wave logic of the table pass can break at n = 1 .. 1 000 (one label, every label different, labels
that alternate, runs of 1 .. 130 points on every lane and across waves and blocks), 70 000 points of one face and of none,
unsigned label order, sums that leave 64 bits, strides, universes with empty faces and with missing labels, the Zipf-like
sweep in three orders.  Then any grid of the table pass, the members' properties, the contract on the device (sizing call,
exact capacity, each capacity one short with canaries, every refusal, bad universes, n == 0), the stage times, the handle's
state, and the sample pair end to end with rj_map_neighbours' rows.  The CPU side is tests/test_face_points.py."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi, maps, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import face_points_cases as FC  # noqa: E402
import face_points_ref as FR  # noqa: E402
from test_face_points import (HANDS, LAYOUTS, OK, answer, case_of, check_all_variants, check_members, faces_of, same, variant)  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(ROOT, "tests", "golden", "sample_pair")
CANARY = 0x5A5A5A5A
TIMES = ["face_points_last_us%d" % k for k in range(5)]
assert _capi.FP_FACE_DTYPE.itemsize == 48 and _capi.FACE_POINTS_COUNTS == FR.COUNTS and _capi.RJ_FP_MEMBERS == FR.MEMBERS


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


class DevicePoints:
    """a case in device buffers"""

    def __init__(self, h, c):
        self.n = len(c.labels)
        self.labels = h.alloc(4 * max(1, self.n)).from_host(c.labels)
        self.values = None if c.values is None else h.alloc(8 * max(1, len(c.values))).from_host(c.values)
        self.stride = c.stride
        self.universe = None
        if c.universe is not None:
            self.universe = h.alloc(4 * max(1, len(c.universe))).from_host(c.universe)
            self.universe.count = len(c.universe)

    def kw(self):
        return dict(value_dev=self.values, value_stride=self.stride, face_label_dev=self.universe, n_face_labels=self.universe.count if self.universe else 0)

    def free(self):
        for b in (self.labels, self.values, self.universe):
            if b is not None:
                b.free()


def result_of(fp, records=True):
    members_on = fp.offsets is not None
    offsets = members = None
    if members_on:
        off, mem = fp.to_host()
        indptr, indices = fp.to_csr()
        assert indptr.dtype == indices.dtype == np.int64 and indptr.tolist() == off.tolist() and indices.tolist() == mem.tolist()
        offsets, members = [int(v) for v in off], [int(v) for v in mem]
    faces = None
    if records:
        faces = faces_of(fp.faces_to_host())
        assert fp.sums() == [f["sum"] for f in faces]
    return FR.Result(faces=faces, offsets=offsets, members=members, counts={k: fp.counts[k] for k in FR.COUNTS})


def device_face_points(h, c, flags=0, records=True):
    """-> (OK, Result, counts) through ops.face_points, the shape that test_face_points.same compares"""
    src = DevicePoints(h, c)
    try:
        fp = ops.face_points(h, src.labels, src.n, values=src.values, value_stride=src.stride, faces=src.universe, members=bool(flags & FR.MEMBERS), records=records)
        try:
            assert isinstance(fp, ops.DeviceFacePoints) and (fp.faces is not None) == records and (fp.offsets is not None) == bool(flags & FR.MEMBERS)
            if not records:
                with pytest.raises(ValueError):
                    fp.faces_to_host()
            if not flags & FR.MEMBERS:
                with pytest.raises(ValueError):
                    fp.to_host()
            r = result_of(fp, records)
            return OK, r, r.counts
        finally:
            fp.free()
    finally:
        src.free()


# ---- the device against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", HANDS + LAYOUTS + [("big", "face"), ("big", "outside")], ids=str)
def test_device_equals_the_definition(handle, what):
    check_all_variants(lambda c, flags, records: device_face_points(handle, c, flags, records), what)


@pytest.mark.parametrize("seed", FC.SWEEP_SEEDS)
def test_sweep(handle, seed):
    for order in FC.ORDERS:
        check_all_variants(lambda c, flags, records: device_face_points(handle, c, flags, records), ("sweep", (seed, order)))


def test_device_gives_the_written_answers(handle):
    for name, k in sorted(FC.HAND.items()):
        rc, r, counts = device_face_points(handle, k["case"], FR.MEMBERS)
        assert r.faces == k["faces"] and r.offsets == k["offsets"] and r.members == k["members"] and counts == k["counts"], name


def raw_outputs(h, src, flags, caps):
    """the call with capacities caps into fresh buffers -> (counts, records, offsets, members) as host arrays"""
    fc, mc = caps
    bufs = [h.alloc(48 * max(1, fc)), h.alloc(8 * (fc + 1)), h.alloc(4 * max(1, mc))]
    try:
        counts = h.face_points(src.labels, src.n, caps, faces_dev=bufs[0], offsets_dev=bufs[1], members_dev=bufs[2], flags=flags, **src.kw())
        return counts, bufs[0].to_host(_capi.FP_FACE_DTYPE, fc), bufs[1].to_host(np.uint64, fc + 1), bufs[2].to_host(np.uint32, mc)
    finally:
        for b in bufs:
            b.free()


def test_any_grid_gives_the_same_result(handle):
    """the debug option "face_points_blocks": one block strides its four waves over every point; 3 and 7 blocks make strides
    that are no power of two.  5 000 points, Zipf-like, block-shuffled: every grid writes identical arrays"""
    rng = np.random.default_rng(99)
    names = np.concatenate([[0], rng.choice(np.arange(1, 100000), 150, replace=False) * rng.choice([-1, 1], 150)]).astype(np.int32)
    weight = 1.0 / np.arange(1, 152) ** 1.1
    labels = np.sort(names[rng.choice(151, 5000, p=weight / weight.sum())])
    pieces = np.split(labels, np.sort(rng.choice(np.arange(1, 5000), 60, replace=False)))
    c = FC.case(np.concatenate([pieces[j] for j in rng.permutation(len(pieces))]), FC.values_for(rng, 5000, 1))
    want = FR.face_points_ref(c.labels, c.values, 1, None, FR.MEMBERS)
    caps = (want.counts["n_faces"], want.counts["n_members"])
    src = DevicePoints(handle, c)
    try:
        outs = []
        for blocks in (0, 1, 2, 3, 7):
            handle.set_debug_option("face_points_blocks", blocks)
            outs.append(raw_outputs(handle, src, FR.MEMBERS, caps))
        for counts, rec, off, mem in outs:
            assert counts == want.counts and faces_of(rec) == want.faces and off.tolist() == want.offsets and mem.tolist() == want.members
            assert rec.tobytes() == outs[0][1].tobytes()
    finally:
        handle.set_debug_option("face_points_blocks", 0)
        src.free()
    assert handle.get_debug_option("face_points_blocks") == 0


@pytest.mark.parametrize("what", [("layout", ("runs", 0)), ("sweep", (5, "shuffled")), ("sweep", (8, "blocks")), ("hand", "universe")], ids=str)
def test_members(handle, what):
    """the members ascend inside every face, their concatenation is a permutation of the member points, first[k] ==
    members[offsets[k]]"""
    for universe in (False, True):
        c = variant(case_of(*what), True, universe)
        _, r, _ = device_face_points(handle, c, FR.MEMBERS)
        check_members(r)
        index = {f["label"]: k for k, f in enumerate(r.faces)}
        assert sorted(r.members) == [i for i, v in enumerate(c.labels) if int(v) in index]


# ---- the contract ------------------------------------------------------------------------------------------------------
def canaried(h, n_bytes):
    words = n_bytes // 4 + 8
    return h.alloc(4 * words).from_host(np.full(words, CANARY, np.uint32))


@pytest.mark.parametrize("flags", (0, FR.MEMBERS))
@pytest.mark.parametrize("universe", (False, True))
def test_sizing_exact_capacity_and_one_short(handle, flags, universe):
    what = ("sweep", (4, "blocks"))
    c, want = variant(case_of(*what), True, universe), answer(*what, True, universe, flags)
    k = want.counts
    caps = (k["n_faces"], k["n_members"] if flags else 0)
    assert caps[0] > 3 and k["n_members"] > 3
    src = DevicePoints(handle, c)
    try:
        with pytest.raises(_capi.FacePointsOverflow) as e:  # the sizing call
            handle.face_points(src.labels, src.n, (0, 0), flags=flags, **src.kw())
        assert e.value.counts == k and e.value.code == _capi.RJ_E_OVERFLOW
        trials = [caps, (caps[0] + 3, caps[1] + 3 if flags else 0)] + [tuple(v - (1 if j == i else 0) for j, v in enumerate(caps)) for i in range(2 if flags else 1)]
        for fc, mc in trials:
            for records in (True, False) if flags else (True,):
                bufs = [canaried(handle, 48 * fc), canaried(handle, 8 * (fc + 1)), canaried(handle, 4 * mc)]
                fits = fc >= caps[0] and mc >= caps[1]
                call = lambda: handle.face_points(src.labels, src.n, (fc, mc), faces_dev=bufs[0] if records else None, offsets_dev=bufs[1],  # noqa: E731
                                                  members_dev=bufs[2], flags=flags, **src.kw())
                host = lambda: [b.to_host(np.uint32) for b in bufs]  # noqa: E731
                if fits:
                    assert call() == k
                    rec, off, mem = host()
                    nf, nm = caps
                    got = FR.Result(faces=faces_of(rec[:12 * nf].view(_capi.FP_FACE_DTYPE)) if records else None,
                                    offsets=[int(v) for v in off[:2 * (nf + 1)].view(np.uint64)] if flags else None,
                                    members=[int(v) for v in mem[:nm]] if flags else None, counts=k)
                    same((OK, got, k), want, records=records)
                    assert (rec[12 * nf if records else 0:] == CANARY).all()
                    assert (off[2 * (nf + 1) if flags else 0:] == CANARY).all() and (mem[nm:] == CANARY).all()  # without the flag neither array is touched
                else:
                    with pytest.raises(_capi.FacePointsOverflow) as e:
                        call()
                    assert e.value.counts == k
                    assert all((a == CANARY).all() for a in host())  # nothing is written
                for b in bufs:
                    b.free()
    finally:
        src.free()


def refused(h, src, word=None, **kw):
    """the call with buffers for 8 faces and 8 members is refused, nothing is written, the stage times are -1"""
    bufs = [canaried(h, 48 * 8), canaried(h, 8 * 9), canaried(h, 4 * 8)]
    args = dict(dict(label_dev=src.labels, n=src.n, capacities=(8, 8), faces_dev=bufs[0], offsets_dev=bufs[1], members_dev=bufs[2], flags=FR.MEMBERS), **src.kw())
    args.update(kw)
    try:
        with pytest.raises(_capi.RayJoinError) as e:
            h.face_points(**args)
        assert e.value.code == _capi.RJ_E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in bufs)  # nothing is written
        assert [h.get_option(t) for t in TIMES] == [-1] * 5
    finally:
        for b in bufs:
            b.free()


def test_refusals(handle):
    c = FC.HAND["two-faces"]["case"]
    src = DevicePoints(handle, c)
    try:
        same(device_face_points(handle, c, FR.MEMBERS), answer("hand", "two-faces", True, False, FR.MEMBERS))
        assert all(handle.get_option(t) >= 0 for t in TIMES)
        for flags in (2, 3, 1 << 31):
            refused(handle, src, word="flags", flags=flags)
        refused(handle, src, word="label", label_dev=None)  # null labels with n > 0
        refused(handle, src, faces_dev=None, flags=0, capacities=(8, 0))  # a capacity without its array
        refused(handle, src, offsets_dev=None)
        refused(handle, src, members_dev=None)
        refused(handle, src, word="RJ_FP_MEMBERS", flags=0)  # member_capacity without the flag
        refused(handle, src, word="value_stride", value_stride=0)
        refused(handle, src, word="2^32", n=1 << 32)  # refused before anything is read
        refused(handle, src, face_label_dev=None, n_face_labels=3)
        counts_null = handle.L.rj_face_points(handle.h, src.labels.ptr, src.n, None, 1, None, 0, 0, 0, 0, None, None, None, None)
        assert counts_null == _capi.RJ_E_INVALID
        same(device_face_points(handle, c, 0), answer("hand", "two-faces", True, False, 0))  # the handle works on
        assert all(handle.get_option(t) >= 0 for t in TIMES)
    finally:
        src.free()


@pytest.mark.parametrize("name", sorted(FC.BAD_UNIVERSES))
def test_a_bad_universe_is_refused(handle, name):
    c = FC.HAND["two-faces"]["case"]
    src = DevicePoints(handle, FC.Case(c.labels, c.values, c.stride, np.array(FC.BAD_UNIVERSES[name], np.int32)))
    try:
        refused(handle, src, word="ascend")
        refused(handle, src, word="ascend", flags=0, capacities=(8, 0))
        with pytest.raises(_capi.RayJoinError) as e:  # the sizing call too
            handle.face_points(src.labels, src.n, (0, 0), **src.kw())
        assert e.value.code == _capi.RJ_E_INVALID
    finally:
        src.free()


def test_no_points(handle):
    none = dict.fromkeys(FR.COUNTS, 0)
    off = handle.alloc(8).from_host(np.array([CANARY, CANARY], np.uint32))
    for flags in (0, FR.MEMBERS):
        assert handle.face_points(None, 0, (0, 0), flags=flags) == none
        assert (off.to_host(np.uint32, 2) == CANARY).all()
    assert handle.face_points(None, 0, (0, 0), offsets_dev=off, flags=FR.MEMBERS) == none  # the offsets' one entry
    assert off.to_host(np.uint64, 1)[0] == 0
    off.free()
    for name in ("no-points", "no-points-universe", "all-outside", "empty-universe"):
        k = FC.HAND[name]
        for flags in (0, FR.MEMBERS):
            _, r, counts = device_face_points(handle, k["case"], flags)
            assert counts == k["counts"] and r.faces == k["faces"] and r.offsets == (k["offsets"] if flags else None)


# ---- end to end, the stage times, the handle -----------------------------------------------------------------------------------
def _sample_context():
    return maps.Context([maps.read_cdb(os.path.join(SAMPLE, "map0.cdb")), maps.read_cdb(os.path.join(SAMPLE, "map1.cdb"))]).load()


def test_sample_pair_end_to_end():
    """upload, build, PIPLBVH.Query of map 1's vertices; Summarize(x of the points by stride 2, the faces of map 0 as
    rj_map_neighbours numbers them, members) equals the definition applied to get_face_ids(), row for row of the adjacency
    table; the stage times are -1 before the first call and not negative after it; the index and the maps answer the same
    PIP query identically afterwards"""
    ctx = _sample_context()
    dctx = ops.DeviceContext(ctx).LoadToDevice()
    h = dctx.handle
    bufs = []
    try:
        dctx.BuildIndex(0)
        m0, m1 = ctx.maps[0], ctx.maps[1]
        pip = ops.PIPLBVH(dctx)
        pip.Init(m1.n_points)
        n = pip.Query(1)
        ids, eids = pip.get_face_ids().copy(), pip.get_closest_eids().copy()
        assert n == m1.n_points == len(ids) and [h.get_option(t) for t in TIMES] == [-1] * 5
        host = (np.ascontiguousarray(m0.pts, np.int64).reshape(-1, 2), np.ascontiguousarray(m0.row_index, np.uint32), np.ascontiguousarray(m0.left, np.int32),
                np.ascontiguousarray(m0.right, np.int32))
        bufs = [h.alloc(max(1, a.nbytes)).from_host(a) for a in host]
        nb = ops.map_neighbours(h, bufs[0], len(host[0]), bufs[1], bufs[2], bufs[3], len(host[2]))
        labels = nb.labels(h)
        bufs.append(labels)
        universe = nb.faces_to_host()["label"]
        assert labels.count == nb.n_faces and np.array_equal(labels.to_host(np.int32, nb.n_faces), universe)
        x = np.ascontiguousarray(m1.pts, np.int64).reshape(-1)
        for kw in (dict(values=h.map_points_dev(1), value_stride=2, faces=labels, members=True), dict(values=h.map_points_dev(1) + 8, value_stride=2, faces=labels),
                   dict(values=None, faces=None, members=True)):
            fp = pip.Summarize(**kw)
            vals = None if kw["values"] is None else (x if kw["values"] == h.map_points_dev(1) else x[1:])
            want = FR.face_points_ref(ids, vals, 2, universe if kw["faces"] is not None else None, FR.MEMBERS if kw.get("members") else 0)
            same((OK, result_of(fp), fp.counts), want)
            if kw["faces"] is not None:  # row k here is row k of the adjacency table
                assert fp.n_faces == nb.n_faces and np.array_equal(fp.faces_to_host()["label"], universe)
            us = [h.get_option(t) for t in TIMES]
            assert all(v >= 0 for v in us) and us[4] >= max(us[:4])
            fp.free()
        assert want.counts["n_members"] > 100 and want.counts["n_faces"] > 3
        assert pip.Query(1) == n and np.array_equal(pip.get_face_ids(), ids) and np.array_equal(pip.get_closest_eids(), eids)
        nb.free()
    finally:
        for b in bufs:
            b.free()
        dctx.close()
