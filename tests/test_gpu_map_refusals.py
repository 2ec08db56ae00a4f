"""What the seven entry points over a chain map say when the map fails its check (rj_map_rings, rj_map_crossings,
rj_map_node, rj_map_snap, rj_map_simplify, rj_map_faces, rj_map_eliminate): the whole message -- prefix, colon and text
-- for a row that does not start at 0, does not end at np or does not ascend and for a coordinate outside the scaled
range, and for rj_map_node / rj_map_snap the message about open chains under their DROP_LAST flag, each with the
flag's own name.  Nothing is written on a refusal: every output buffer keeps its canary.  The other tests of these
calls look for one word of each message."""
import os
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_node import record_array, records_of  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
BAD_ROWS = ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6])  # does not start at 0, does not end at np, does not ascend
BAD_COORDINATES = (1 << 46, -(1 << 46) - 1)

# per entry point: the messages of the three rows above, then that of the coordinates
MESSAGES = {
    "rj_map_rings": ["rj_map_rings: row_index must start at 0",
                     "rj_map_rings: row_index must end at np",
                     "rj_map_rings: row_index must ascend (a chain has no point)",
                     "rj_map_rings: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_crossings": ["rj_map_crossings: row_index must start at 0",
                         "rj_map_crossings: row_index must end at np",
                         "rj_map_crossings: row_index must ascend (a chain has no point)",
                         "rj_map_crossings: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_node": ["rj_map_node: row_index must start at 0",
                    "rj_map_node: row_index must end at np",
                    "rj_map_node: row_index must ascend (a chain has no point)",
                    "rj_map_node: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_snap": ["rj_map_snap: row_index must start at 0",
                    "rj_map_snap: row_index must end at np",
                    "rj_map_snap: row_index must ascend (a chain has no point)",
                    "rj_map_snap: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_simplify": ["rj_map_simplify: row_index must start at 0",
                        "rj_map_simplify: row_index must end at np",
                        "rj_map_simplify: row_index must ascend (a chain has no point)",
                        "rj_map_simplify: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_faces": ["rj_map_faces: row_index must start at 0",
                     "rj_map_faces: row_index must end at np",
                     "rj_map_faces: row_index must ascend (a chain has no point)",
                     "rj_map_faces: a coordinate lies outside the scaled range [-2^46, 2^46)"],
    "rj_map_eliminate": ["rj_map_eliminate: row_index must start at 0",
                         "rj_map_eliminate: row_index must end at np",
                         "rj_map_eliminate: row_index must ascend (a chain has no point)",
                         "rj_map_eliminate: a coordinate lies outside the scaled range [-2^46, 2^46)"],
}
DROP_LAST_MESSAGES = {
    "rj_map_node": "rj_map_node: RJ_NODE_DROP_LAST needs chains of two points or more whose first point equals the last",
    "rj_map_snap": "rj_map_snap: RJ_SNAP_DROP_LAST needs chains of two points or more whose first point equals the last",
}


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


def the_map():
    """the 3-chain, 6-point map of test_gpu_node.py::test_refusals and its records"""
    (xy, row), records, _ = records_of("hand", "two-cuts-reversed")
    assert xy.shape == (6, 2) and row.tolist() == [0, 2, 4, 6] and records == [(0, 1, 2), (0, 2, 2)]
    return xy, row, records


def call_of(name, h, xy, row, records, flags, bufs):
    """-> (the call on the map in device memory, its canaried output buffers); bufs collects every buffer to free"""
    def dev(a):
        bufs.append(h.alloc(max(4, a.nbytes)).from_host(a))
        return bufs[-1]

    def out(nbytes):
        bufs.append(h.alloc(nbytes).from_host(np.full(nbytes // 4, CANARY, np.uint32)))
        return bufs[-1]

    n, nc = len(xy), len(row) - 1
    dxy, drow = dev(np.ascontiguousarray(xy, np.int64)), dev(np.ascontiguousarray(row, np.uint32))
    if name == "rj_map_rings":
        left, right = dev(np.zeros(nc, np.int32)), dev(np.zeros(nc, np.int32))
        outs = [out(32 * 8), out(4 * 9), out(4 * 8), out(4 * 9), out(16 * 32)]
        return (lambda: h.map_rings(dxy, n, drow, left, right, nc, flags, (8, 8, 32), *outs)), outs
    if name == "rj_map_crossings":
        outs = [out(16 * 16)]
        return (lambda: h.map_crossings(dxy, n, drow, nc, 16, outs[0], flags=flags)), outs
    if name in ("rj_map_node", "rj_map_snap"):
        rec = dev(record_array(records)) if records else None
        outs = [out(16 * 16), out(4 * (nc + 1)), out(4 * 16)]
        entry = h.map_node if name == "rj_map_node" else h.map_snap
        return (lambda: entry(dxy, n, drow, nc, rec, len(records), flags, 16, *outs)), outs
    if name == "rj_map_simplify":
        outs = [out(16 * n), out(4 * (nc + 1)), out(4 * n)]
        return (lambda: h.map_simplify(dxy, n, drow, nc, 0, n, *outs, flags=flags)), outs
    if name == "rj_map_faces":
        left, right = dev(np.zeros(nc, np.int32)), dev(np.zeros(nc, np.int32))
        outs = [out(4 * nc), out(4 * nc), out(32 * 8)]
        return (lambda: h.map_faces(dxy, n, drow, nc, outs[0], outs[1], outs[2], 8, left, right, flags=flags)), outs
    assert name == "rj_map_eliminate"
    left, right = dev(np.zeros(nc, np.int32)), dev(np.zeros(nc, np.int32))
    outs = [out(4 * nc), out(4 * nc), out(16 * n), out(4 * (nc + 1)), out(4 * nc), out(32 * 2 * nc)]
    return (lambda: h.map_eliminate(dxy, n, drow, left, right, nc, 0, (2 * nc, nc, n), *outs, flags=flags | _capi.RJ_ELIM_DROP)), outs


def refused(name, h, xy, row, records, message, flags=0):
    bufs = []
    try:
        call, outs = call_of(name, h, xy, row, records, flags, bufs)
        with pytest.raises(_capi.RayJoinError) as e:
            call()
        print("%s -> %s" % (name, e.value))
        assert e.value.code == _capi.RJ_E_INVALID and str(e.value) == "rayjoin_amd error %d: %s" % (_capi.RJ_E_INVALID, message)
        assert all((b.to_host(np.uint32) == CANARY).all() for b in outs), name  # nothing is written
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", sorted(MESSAGES))
def test_the_map_check_refuses_with_the_whole_message(handle, name):
    xy, row, records = the_map()
    for bad_row, message in zip(BAD_ROWS, MESSAGES[name][:3]):
        refused(name, handle, xy, np.array(bad_row, np.uint32), [], message)
    for v in BAD_COORDINATES:
        bad = xy.copy()
        bad[3, 1] = v
        refused(name, handle, bad, row, records, MESSAGES[name][3])


@pytest.mark.parametrize("name", sorted(DROP_LAST_MESSAGES))
def test_drop_last_names_the_calls_own_flag(handle, name):
    xy, row, records = the_map()  # open chains
    flags = _capi.RJ_NODE_DROP_LAST if name == "rj_map_node" else _capi.RJ_SNAP_DROP_LAST
    refused(name, handle, xy, row, records, DROP_LAST_MESSAGES[name], flags=flags)
