"""The face adjacency table of a chain map on the CPU: the plain-Python definition (tests/neighbours_ref.py) on the maps of
tests/neighbours_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/neighbours_twin.cc compiling rayjoin_amd/csrc/rj_neighbours.h) against that definition, array for array
and count for count, with and without RJ_NB_VERTEX and the records: the hand cases, the constructed maps whose keyed sums
cross a wave and a block, the 12 generated planar maps, 8 label matrices whose answer comes from the matrix alone; the
properties (both directions equal, perimeter = outer + the sum of w, area2 and the longest border equal to
eliminate_ref's, rook only = flagged without the vertex-only entries); the contract of the call (sizing, exact capacity,
each capacity one short with canaries, every refusal, no chains); three mutations of a scratch copy of the header, each
caught by a hand case; the twin as a stand-alone program under the host sanitizers.  The GPU side is
tests/test_gpu_neighbours.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eliminate_cases as EC  # noqa: E402
import eliminate_ref as ER  # noqa: E402
import neighbours_cases as NC  # noqa: E402
import neighbours_ref as NR  # noqa: E402
import rings_planar as RP  # noqa: E402
from rings_cases import chain_map  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "neighbours_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HEADER = os.path.join(CSRC, "rj_neighbours.h")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
FACE_DTYPE = np.dtype([("label", "<i4"), ("n_sides", "<u4"), ("n_edge_nbrs", "<u4"), ("n_vertex_nbrs", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8"),
                       ("perimeter_lo", "<u8"), ("perimeter_hi", "<u8"), ("outer_lo", "<u8"), ("outer_hi", "<u8")])
ENTRY_DTYPE = np.dtype([("label", "<i4"), ("face", "<u4"), ("n_chains", "<u4"), ("n_nodes", "<u4"), ("w_lo", "<u8"), ("w_hi", "<u8")])
CANARY32, CANARY64 = 0x5B5B5B5B, 0x5B5B5B5B5B5B5B5B
OK, INVALID, OVERFLOW = 0, 1, 3
SEEDS = tuple(range(12))
MATRIX_SEEDS = tuple(range(8))
BOTH = (0, NR.VERTEX)
assert FACE_DTYPE.itemsize == 64 and ENTRY_DTYPE.itemsize == 32


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_neighbours.h")] + [os.path.join(CSRC, h) for h in ("rj_rings.h", "rj_ringmap.h", "rj_eliminate.h", "rj_dissolve.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libneighbours_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.neighbours_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def arrays(m):
    return (np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32), np.ascontiguousarray(m[2], np.int32),
            np.ascontiguousarray(m[3], np.int32))


def wide(lo, hi, signed=False):
    v = (int(hi) << 64) | int(lo)
    return v - (1 << 128) if signed and v >> 127 else v


def faces_of(rows):
    """FACE_DTYPE rows -> the dicts of neighbours_ref"""
    return [dict(label=int(r["label"]), n_sides=int(r["n_sides"]), n_edge_nbrs=int(r["n_edge_nbrs"]), n_vertex_nbrs=int(r["n_vertex_nbrs"]),
                 area2=wide(r["area2_lo"], int(r["area2_hi"]) % (1 << 64), True), perimeter=wide(r["perimeter_lo"], r["perimeter_hi"]),
                 outer=wide(r["outer_lo"], r["outer_hi"])) for r in rows]


def entries_of(rows):
    return [dict(label=int(r["label"]), face=int(r["face"]), n_chains=int(r["n_chains"]), n_nodes=int(r["n_nodes"]), w=wide(r["w_lo"], r["w_hi"])) for r in rows]


def ptr(a):
    return a.ctypes.data if a is not None else None


def twin_neighbours(L, m, flags=0, records=True, capacities=None):
    """-> (status, Result or None, counts).  capacities None: the sizing call, then the exact capacities; else (faces,
    entries).  Behind every capacity lie canaries that must survive; an overflow or a refusal leaves every output as it was."""
    xy, row, left, right = arrays(m)
    nc = max(0, len(row) - 1)
    counts = np.zeros(len(NR.COUNTS), np.uint64)

    def call(caps, faces, offsets, entries):
        return L.neighbours_twin(xy.ctypes.data, len(xy), row.ctypes.data, left.ctypes.data, right.ctypes.data, nc, flags, caps[0], caps[1], ptr(faces),
                                 ptr(offsets), ptr(entries), counts.ctypes.data)

    def named():
        return dict(zip(NR.COUNTS, (int(v) for v in counts)))
    if capacities is None:
        rc = call((0, 0), None, None, None)
        c = named()
        if rc not in (OK, OVERFLOW):
            return rc, None, c
        capacities = (c["n_faces"], c["n_entries"])
    fc, ec = capacities
    faces = np.zeros(fc + 2, FACE_DTYPE) if records else None
    if records:
        faces.view(np.uint32)[:] = CANARY32
    offsets, entries = np.full(fc + 3, CANARY64, np.uint64), np.zeros(ec + 2, ENTRY_DTYPE)
    entries.view(np.uint32)[:] = CANARY32
    rc = call(capacities, faces, offsets, entries)
    c = named()
    if rc != OK:
        assert all((a.view(np.uint32) == CANARY32).all() for a in (faces, offsets, entries) if a is not None)
        return rc, None, c
    nf, ne = c["n_faces"], c["n_entries"]
    assert faces is None or (faces.view(np.uint32)[16 * nf:] == CANARY32).all()
    assert (offsets[nf + 1:] == CANARY64).all() and (entries.view(np.uint32)[8 * ne:] == CANARY32).all()
    return rc, NR.Result(faces=faces_of(faces[:nf]) if records else None, offsets=[int(v) for v in offsets[:nf + 1]], entries=entries_of(entries[:ne]),
                         counts=c), c


def same(got, want, records=True):
    """(status, Result, counts) of the twin or the device against neighbours_ref's Result"""
    rc, r, c = got
    assert rc == OK and c == want.counts, (rc, c, want.counts)
    assert r.offsets == want.offsets and r.entries == want.entries
    assert not records or r.faces == want.faces


# ---- the inputs: computed once, shared, never changed ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planar(seed):
    return RP.draw_planar(seed)


@functools.lru_cache(maxsize=None)
def case_of(kind, key):
    """the written case (a dict with map, pairs, faces, counts) of the kinds that have one"""
    return {"hand": lambda: NC.HAND[key], "sqrt": NC.sqrt_answer, "pair": lambda: NC.pair_row(key), "hub": lambda: NC.hub(key)}[kind]()


@functools.lru_cache(maxsize=None)
def map_of(kind, key):
    if kind in ("hand", "sqrt", "pair", "hub"):
        return case_of(kind, key)["map"]
    return {"lengths": EC.lengths_map, "row": EC.two_point_row, "odd": RP.odd_faces, "long": RP.long_chains, "planar": lambda: planar(key)[0],
            "matrix": lambda: NC.matrix_case(key)[0]}[kind]()


@functools.lru_cache(maxsize=None)
def answer(kind, key, flags):
    return NR.neighbours_ref(*map_of(kind, key), flags)


WRITTEN = [("hand", n) for n in sorted(NC.HAND)] + [("sqrt", None)] + [("pair", n) for n in NC.PAIR_ROWS] + [("hub", n) for n in NC.HUBS]
SMALL = WRITTEN + [("lengths", None), ("row", None), ("odd", None)]
EVERY = SMALL + [("planar", s) for s in SEEDS] + [("matrix", s) for s in MATRIX_SEEDS]


# ---- the definition against the written answers -------------------------------------------------------------------------
def by_unsigned(f, g):
    return (f, g) if NR.unsigned(f) < NR.unsigned(g) else (g, f)


def check_pairs(r, pairs, flags):
    """pairs {(f, g): (w, n_chains, n_nodes)} over the unordered pairs as the flagged call gives them"""
    want = {}
    for (f, g), (w, n_chains, n_nodes) in pairs.items():
        if flags & NR.VERTEX or n_chains:
            want[(f, g)] = want[(g, f)] = (w, n_chains, n_nodes if flags & NR.VERTEX else 0)
    assert r.pairs() == want
    assert r.counts["n_entries"] == len(want)
    assert r.counts["n_edge_pairs"] == sum(1 for v in pairs.values() if v[1])
    assert r.counts["n_vertex_pairs"] == (sum(1 for v in pairs.values() if not v[1]) if flags & NR.VERTEX else 0)


def check_written(k, r, flags):
    check_pairs(r, k["pairs"], flags)
    assert [f["label"] for f in r.faces] == sorted(k["faces"], key=NR.unsigned) and r.counts["n_faces"] == len(k["faces"])
    assert {f["label"]: (f["n_sides"], f["area2"], f["perimeter"], f["outer"]) for f in r.faces} == k["faces"]
    for n, f in enumerate(r.faces):
        mine = r.entries[r.offsets[n]:r.offsets[n + 1]]
        assert [NR.unsigned(e["label"]) for e in mine] == sorted(NR.unsigned(e["label"]) for e in mine)
        assert all(r.faces[e["face"]]["label"] == e["label"] for e in mine)
        assert f["n_edge_nbrs"] == sum(1 for e in mine if e["n_chains"]) and f["n_vertex_nbrs"] == sum(1 for e in mine if not e["n_chains"])
    assert (r.counts["n_nodes"], r.counts["n_node_pairs_raw"], r.counts["max_labels_at_node"]) == (k["counts"] if flags & NR.VERTEX else (0, 0, 0))


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("what", WRITTEN, ids=str)
def test_definition_gives_the_written_answer(what, flags):
    check_written(case_of(*what), answer(*what, flags), flags)


def test_the_checkerboard_diagonals_are_vertex_only():
    r = answer("hand", "checkerboard", NR.VERTEX).pairs()
    assert r[(1, 4)] == r[(4, 1)] == r[(2, 3)] == r[(3, 2)] == (0, 0, 1) and len(r) == 12
    r = answer("hand", "checkerboard", 0).pairs()
    assert len(r) == 8 and (1, 4) not in r and (2, 3) not in r and all(v == (10, 1, 0) for v in r.values())


def test_entries_ascend_by_unsigned_label():
    r = answer("hand", "negative-labels", NR.VERTEX)
    assert [f["label"] for f in r.faces] == [3, 7, -5] and [e["label"] for e in r.entries[r.offsets[0]:r.offsets[1]]] == [7, -5]
    odd = answer("odd", None, NR.VERTEX)
    assert [NR.unsigned(f["label"]) for f in odd.faces] == sorted(NR.unsigned(f) for f in RP.ODD_FACES if f != 0)


@pytest.mark.parametrize("seed", MATRIX_SEEDS)
def test_the_matrix_answer(twin, seed):
    """w, n_chains and n_nodes of every pair from the label matrix alone, against the definition and the twin"""
    m, pairs = NC.matrix_case(seed)
    for flags in BOTH:
        check_pairs(answer("matrix", seed, flags), pairs, flags)
        rc, r, _ = twin_neighbours(twin, m, flags)
        assert rc == OK
        check_pairs(r, pairs, flags)


def vertex_only_directed(r):
    return sum(1 for e in r.entries if e["n_chains"] == 0)


def test_generated_maps_are_worth_their_time():
    """on these seeds the definition alone finds more than a thousand vertex-only directed pairs"""
    found = [vertex_only_directed(answer("planar", s, NR.VERTEX)) for s in (0, 1, 4, 7, 9)]
    assert all(v >= 1000 for v in found), found


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_twin(twin, what, flags):
    m, want = map_of(*what), answer(*what, flags)
    same(twin_neighbours(twin, m, flags), want)
    same(twin_neighbours(twin, m, flags, records=False), want, records=False)


# ---- the properties ------------------------------------------------------------------------------------------------------
def longest_border(r, k):
    """the arg-max of face k's edge entries by (largest w, smaller min, smaller max) of the face numbers -> a label or None"""
    mine = [e for e in r.entries[r.offsets[k]:r.offsets[k + 1]] if e["n_chains"]]
    if not mine:
        return None
    return min(mine, key=lambda e: (-e["w"], min(k, e["face"]), max(k, e["face"])))["label"]


def properties(r, rook, m):
    """r the flagged Result, rook the rook-only one, of map m"""
    pairs = r.pairs()
    assert all(pairs[(g, f)] == v for (f, g), v in pairs.items()) and all(f != g and f != 0 and g != 0 for f, g in pairs)
    for k, f in enumerate(r.faces):
        assert f["perimeter"] == f["outer"] + sum(e["w"] for e in r.entries[r.offsets[k]:r.offsets[k + 1]])
    el = ER.eliminate_ref(*m, ER.HUGE, 0)
    assert [(f["label"], f["area2"]) for f in r.faces] == [(f["label"], f["area2"]) for f in el.faces]
    for k, f in enumerate(el.faces):  # a face of negative area is no sliver and has no best: its record holds its own label
        best = longest_border(r, k)
        assert f["best"] == (best if best is not None and f["area2"] >= 0 else f["label"])
    kept = [e for e in r.entries if e["n_chains"]]
    assert rook.entries == [dict(e, n_nodes=0) for e in kept] and rook.counts["n_entries"] == len(kept)
    assert [dict(f, n_vertex_nbrs=0) for f in r.faces] == rook.faces
    assert rook.offsets == [sum(1 for e in r.entries[:o] if e["n_chains"]) for o in r.offsets]
    assert rook.counts == dict(r.counts, n_entries=len(kept), n_vertex_pairs=0, n_nodes=0, n_node_pairs_raw=0, max_labels_at_node=0)


@pytest.mark.parametrize("what", EVERY, ids=str)
def test_properties(twin, what):
    m = map_of(*what)
    properties(answer(*what, NR.VERTEX), answer(*what, 0), m)
    got = [twin_neighbours(twin, m, flags) for flags in (NR.VERTEX, 0)]
    assert got[0][0] == got[1][0] == OK
    properties(got[0][1], got[1][1], m)


# ---- the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BOTH)
def test_sizing_call_exact_capacity_and_one_short(twin, flags):
    what = ("planar", 3)
    m, want = map_of(*what), answer(*what, flags)
    c = want.counts
    assert c["n_faces"] > 3 and c["n_entries"] > 3
    caps = (c["n_faces"], c["n_entries"])
    rc, _, got = twin_neighbours(twin, m, flags, capacities=(0, 0))
    assert rc == OVERFLOW and got == c
    same(twin_neighbours(twin, m, flags, capacities=caps), want)
    same(twin_neighbours(twin, m, flags, capacities=tuple(v + 3 for v in caps)), want)
    for k in range(2):
        short = tuple(v - (1 if j == k else 0) for j, v in enumerate(caps))
        for records in (True, False):  # (the offsets need the face capacity with or without records)
            rc, _, got = twin_neighbours(twin, m, flags, records=records, capacities=short)  # (twin_neighbours checks that nothing was written)
            assert (rc, got) == (OVERFLOW, c)


def test_no_chains(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for flags in BOTH:
        rc, r, c = twin_neighbours(twin, empty, flags)
        assert rc == OK and c == dict.fromkeys(NR.COUNTS, 0) == NR.neighbours_ref(*empty, flags).counts and r.offsets == [0] and r.entries == []


def test_a_map_without_a_face(twin):
    """that fits capacities of 0, so the sizing call, whose arrays are null, succeeds and must write nothing"""
    m = chain_map([([(0, 0), (5, 5)], 0, 0), ([(5, 5)], 0, 0)])
    for flags in BOTH:
        want = NR.neighbours_ref(*m, flags)
        assert want.counts == dict(dict.fromkeys(NR.COUNTS, 0), n_nodes=2 if flags else 0) and want.offsets == [0]
        xy, row, left, right = arrays(m)
        counts = np.zeros(len(NR.COUNTS), np.uint64)
        rc = twin.neighbours_twin(xy.ctypes.data, 3, row.ctypes.data, left.ctypes.data, right.ctypes.data, 2, flags, 0, 0, None, None, None, counts.ctypes.data)
        assert rc == OK and dict(zip(NR.COUNTS, (int(v) for v in counts))) == want.counts
        same(twin_neighbours(twin, m, flags), want)


def refused(twin, m, flags=0):
    """the definition refuses it, and so does the twin"""
    with pytest.raises(NR.Invalid):
        NR.neighbours_ref(*m, flags)
    n = len(m[2])
    return twin_neighbours(twin, m, flags)[0] == INVALID and twin_neighbours(twin, m, flags, capacities=(2 * n, 16 * n * n))[0] == INVALID


def test_bad_input(twin):
    xy, row, left, right = chain_map([([(0, 0), (1, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    for flags in BOTH:
        assert twin_neighbours(twin, (xy, row, left, right), flags)[0] == OK
        for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6], [0, 2, 4, 7]):
            assert refused(twin, (xy, np.array(bad_row, np.uint32), left, right), flags)
        for v in (1 << 46, -(1 << 46) - 1, (1 << 63) - 1, -(1 << 63)):
            for at in ((3, 1), (0, 0), (5, 0)):
                bad = xy.copy()
                bad[at] = v
                assert refused(twin, (bad, row, left, right), flags)
        assert refused(twin, (xy[:2], row, left, right), flags)  # more chains than points
        assert refused(twin, (xy, np.zeros(1, np.uint32), left[:0], right[:0]), flags)  # points without chains
    for flags in (2, 3, 1 << 31):
        assert refused(twin, (xy, row, left, right), flags)
    counts = np.zeros(len(NR.COUNTS), np.uint64)
    args = [None, None, None, counts.ctypes.data]
    for n_points, n_chains, flags in ((1 << 32, 3, 0), (1 << 31, 1 << 31, 0), ((1 << 31) + 3, 3, 0), (2, 3, 0), (3, 0, 0), (1 << 30, 1 << 30, NR.VERTEX)):
        assert twin.neighbours_twin(None, n_points, None, None, None, n_chains, flags, 0, 0, *args) == INVALID  # the size limits: refused before anything is read
    xy, row, left, right = arrays((xy, row, left, right))
    for caps in ((3, 0), (0, 4), (3, 4)):  # a capacity without its array
        assert twin.neighbours_twin(xy.ctypes.data, 6, row.ctypes.data, left.ctypes.data, right.ctypes.data, 3, 0, *caps, *args) == INVALID


def test_too_many_node_pairs_are_refused(twin):
    """a hub of 65 537 faces at one vertex has 65 537 x 65 536 >= 2^32 directed pairs: refused with that count and nothing
    else, nothing written; rook only the same map is an ordinary one.  (The definition loops over every pair before it
    checks: the twin is asked directly.)"""
    m = NC.limit_hub()
    n = NC.LIMIT_HUB
    want = dict(dict.fromkeys(NR.COUNTS, 0), n_node_pairs_raw=n * (n - 1))
    assert n * (n - 1) >= NR.RAW_LIMIT > (n - 1) * (n - 2)
    for caps in (None, (n, 16), (n + 5, 0)):
        rc, _, c = twin_neighbours(twin, m, NR.VERTEX, capacities=caps)  # (twin_neighbours checks that nothing was written)
        assert rc == INVALID and c == want
    rc, r, c = twin_neighbours(twin, m, 0)
    assert rc == OK and c == dict(dict.fromkeys(NR.COUNTS, 0), n_faces=n) and r.entries == [] and r.offsets == [0] * (n + 1)
    assert [f["label"] for f in r.faces] == list(range(1, n + 1)) and all(f["perimeter"] == f["outer"] > 0 and f["n_sides"] == 1 for f in r.faces)


# ---- mutations of the header, each caught ------------------------------------------------------------------------------------
# name -> (the header, [(old, new)], the hand cases that catch it).  Every header of the directory is copied to a scratch
# directory that comes first on the include path, so the twin compiles the mutated copy and the repository's stays as it is.
MUTATIONS = {
    # a pair whose border has no length is no pair
    "zero-length-dropped": ("rj_neighbours.h", [("RJ_RHD bool is_edge(const PairSum& v) { return v.n_chains != 0; }",
                                                 "RJ_RHD bool is_edge(const PairSum& v) { return v.n_chains != 0 && (v.w_lo | v.w_hi) != 0; }")],
                            ("zero-length",)),
    # outside chains counted as neighbours: label 0 separates like any other, so the outside is one more face (the last
    # one: its key is the largest) and every outer border a shared one.  The rule is eliminate's, in rj_eliminate.h.
    "outside-counted": ("rj_eliminate.h", [("RJ_RHD bool separates(int32_t l, int32_t r) { return l != r && l != 0 && r != 0; }",
                                            "RJ_RHD bool separates(int32_t l, int32_t r) { return l != r; }"),
                                           ("return n_keys - (n_keys && keys[n_keys - 1] == kZeroKey ? 1 : 0); }", "return n_keys; }"),
                                           ("  if (label == 0) return kNone;\n", "")],
                        ("island", "longer")),
    # equal labels at a node are not recognised as one
    "duplicates-kept": ("rj_neighbours.h", [("other_key = key[i] != key[j];", "other_key = true;")], ("repeated-label",)),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_mutated_header_is_caught(name, tmp_path):
    header, edits, cases = MUTATIONS[name]
    for h in os.listdir(CSRC):
        if h.endswith(".h"):
            text = open(os.path.join(CSRC, h)).read()
            for old, new in edits if h == header else ():
                assert text.count(old) == 1, old
                text = text.replace(old, new)
            (tmp_path / h).write_text(text)
    L = twin_lib(str(tmp_path), "_mutant_" + name)
    os.remove(os.path.join(BUILD, "libneighbours_twin_mutant_%s.so" % name))
    for case in cases:
        rc, r, c = twin_neighbours(L, map_of("hand", case), NR.VERTEX)
        want = answer("hand", case, NR.VERTEX)
        assert rc == OK and not (r.faces == want.faces and r.entries == want.entries and c == want.counts)
    same(twin_neighbours(L, map_of("pair", 1), NR.VERTEX), answer("pair", 1, NR.VERTEX))  # (the same program otherwise: one open chain between two faces)


# ---- the stand-alone program under the host sanitizers ----------------------------------------------------------------------
def low(v):
    return v & (2 ** 64 - 1)


def case_text(m, flags, want, status):
    xy, row, left, right = arrays(m)
    out = [len(xy), len(row) - 1, flags] + xy.reshape(-1).tolist() + row.tolist() + left.tolist() + right.tolist()
    if status != OK:
        return " ".join(str(v) for v in out + [status] + [want[n] for n in NR.COUNTS])
    out += [OK] + [want.counts[n] for n in NR.COUNTS]
    for f in want.faces:
        out += [f["label"], f["n_sides"], f["n_edge_nbrs"], f["n_vertex_nbrs"], low(f["area2"]), (low(f["area2"] >> 64) + 2 ** 63) % 2 ** 64 - 2 ** 63,
                low(f["perimeter"]), f["perimeter"] >> 64, low(f["outer"]), f["outer"] >> 64]
    out += want.offsets
    for e in want.entries:
        out += [e["label"], e["face"], e["n_chains"], e["n_nodes"], low(e["w"]), e["w"] >> 64]
    return " ".join(str(v) for v in out)


def test_stand_alone_twin_program_under_sanitizers(tmp_path):
    """the twin with its own main, built with -fsanitize=address,undefined and run as a program of its own (nothing is
    loaded into Python under a sanitizer) over the small cases with and without the flag, and two refused maps"""
    exe = os.path.join(BUILD, "neighbours_twin_main_san")
    os.makedirs(BUILD, exist_ok=True)
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNEIGHBOURS_TWIN_MAIN",
                               "-I", CSRC, "-o", exe, SRC])
    lines = [case_text(map_of(*w), flags, answer(*w, flags), OK) for w in SMALL for flags in BOTH]
    xy, row, left, right = NC.HAND["longer"]["map"]
    wild = xy.copy()
    wild[1, 0] = (1 << 63) - 1  # an edge whose square would not fit 128 bits, were it ever squared
    none = dict.fromkeys(NR.COUNTS, 0)
    lines += [case_text((wild, row, left, right), flags, none, INVALID) for flags in BOTH]
    lines.append(case_text((xy, row, left, right), 2, none, INVALID))
    n = NC.LIMIT_HUB  # the hub that is refused for its node pairs, and the same map rook only
    lines.append(case_text(NC.limit_hub(), NR.VERTEX, dict(none, n_node_pairs_raw=n * (n - 1)), INVALID))
    lines.append(case_text(NC.limit_hub(), 0, NR.neighbours_ref(*NC.limit_hub(), 0), OK))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == len(lines) and "MISMATCH" not in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
