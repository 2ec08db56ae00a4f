"""Merging sliver faces into a neighbour on the CPU: the plain-Python definition (tests/eliminate_ref.py) on the hand-built
maps of tests/eliminate_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/eliminate_twin.cc compiling rayjoin_amd/csrc/rj_eliminate.h) against that definition, every array and
every count, with and without RJ_ELIM_DROP, with and without records: the hand cases, the structural maps (chains of
1 .. 1 000 points, 300 two-point chains in a row), odd labels, 12 generated planar maps whose face areas are known from
the generator alone; the chain sums and 2 000 random square roots at full range against math.isqrt; the contract of the
call (sizing, exact capacity, each capacity one short with canaries, every refusal); the properties (the area of a target
is the sum of what it took, no cycle survives, the rounds end); three mutations of a scratch copy of the header, each
caught by a hand case; the twin as a stand-alone program.  The GPU side is tests/test_gpu_eliminate.py."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eliminate_cases as EC  # noqa: E402
import eliminate_ref as ER  # noqa: E402
import rings_planar as RP  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "eliminate_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HEADER = os.path.join(CSRC, "rj_eliminate.h")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
FACE_DTYPE = np.dtype([("label", "<i4"), ("target", "<i4"), ("best", "<i4"), ("flags", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
CANARY32, CANARY64 = 0x5B5B5B5B, 0x5B5B5B5B5B5B5B5B
OK, INVALID, OVERFLOW = 0, 1, 3
HUGE = ER.HUGE
SEEDS = tuple(range(12))


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_eliminate.h"), os.path.join(CSRC, "rj_rings.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libeliminate_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.eliminate_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64,
                                 C.c_uint64, C.c_uint64] + [C.c_void_p] * 7
    L.eliminate_twin_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.eliminate_twin_sums.restype = None
    L.eliminate_twin_isqrt.argtypes = [C.c_uint64, C.c_uint64]
    L.eliminate_twin_isqrt.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def arrays(m):
    return (np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32), np.ascontiguousarray(m[2], np.int32),
            np.ascontiguousarray(m[3], np.int32))


def faces_of(records):
    """FACE_DTYPE rows -> the dicts of eliminate_ref"""
    return [dict(label=int(r["label"]), target=int(r["target"]), best=int(r["best"]), flags=int(r["flags"]),
                 area2=(int(r["area2_hi"]) << 64) | int(r["area2_lo"])) for r in records]


def ptr(a):
    return a.ctypes.data if a is not None else None


def twin_eliminate(L, m, tol, flags=0, records=True, capacities=None, origin=True):
    """-> (status, Result or None, counts).  capacities None: the sizing call, then the exact capacities; else (faces,
    chains, points).  Behind every capacity lie canaries that must survive; an overflow or a refusal leaves every output
    as it was."""
    xy, row, left, right = arrays(m)
    nc, drop = max(0, len(row) - 1), bool(flags & ER.DROP)
    counts = np.zeros(9, np.uint64)

    def call(caps, faces, ol, orr, oxy, orow, org):
        return L.eliminate_twin(xy.ctypes.data, len(xy), row.ctypes.data, left.ctypes.data, right.ctypes.data, nc, tol & (2 ** 64 - 1), tol >> 64, flags,
                                caps[0], caps[1], caps[2], ptr(faces), ptr(ol), ptr(orr), ptr(oxy), ptr(orow), ptr(org), counts.ctypes.data)

    def named():
        return dict(zip(ER.COUNTS, (int(v) for v in counts)))
    if capacities is None:
        rc = call((0, 0, 0), None, None, None, None, None, None)
        c = named()
        if rc not in (OK, OVERFLOW):
            return rc, None, c
        if nc == 0:
            none = np.zeros(0, np.int32)
            return rc, ER.Result(faces=[] if records else None, left=none, right=none, xy=np.zeros((0, 2), np.int64) if drop else None,
                                 row_index=np.zeros(1, np.uint32) if drop else None, origin=np.zeros(0, np.uint32) if drop and origin else None, counts=c), c
        capacities = (c["n_faces"], c["n_chains"], c["n_points"])
    fc, cc, pc = capacities
    faces = np.zeros(fc + 2, FACE_DTYPE) if records else None
    if records:
        faces.view(np.uint32)[:] = CANARY32
    ol, orr = np.full(cc + 2, CANARY32, np.uint32).view(np.int32), np.full(cc + 2, CANARY32, np.uint32).view(np.int32)
    oxy, orow, org = np.full((pc + 2, 2), CANARY64, np.int64), np.full(cc + 3, CANARY32, np.uint32), np.full(cc + 2, CANARY32, np.uint32) if origin else None
    rc = call(capacities, faces, ol, orr, oxy, orow, org)
    c = named()
    untouched = [(a.view(np.uint32) == CANARY32).all() for a in (faces, ol, orr, oxy, orow, org) if a is not None]
    if rc != OK:
        assert all(untouched)
        return rc, None, c
    nf, n, npts = c["n_faces"], c["n_chains"], c["n_points"]
    assert (ol.view(np.uint32)[n:] == CANARY32).all() and (orr.view(np.uint32)[n:] == CANARY32).all()
    assert faces is None or (faces.view(np.uint32)[8 * nf:] == CANARY32).all()
    if drop:
        assert (oxy[npts:] == CANARY64).all() and (orow[n + 1:] == CANARY32).all() and (org is None or (org[n:] == CANARY32).all())
    else:
        assert (oxy == CANARY64).all() and (orow == CANARY32).all() and (org is None or (org == CANARY32).all())
    return rc, ER.Result(faces=faces_of(faces[:nf]) if records else None, left=ol[:n].copy(), right=orr[:n].copy(), xy=oxy[:npts] if drop else None,
                         row_index=orow[:n + 1] if drop else None, origin=org[:n] if drop and origin else None, counts=c), c


def same(got, want, records=True, origin=True):
    """(status, Result, counts) of the twin or the device against eliminate_ref's Result"""
    rc, r, c = got
    assert rc == OK and c == want.counts
    assert np.array_equal(r.left, want.left) and np.array_equal(r.right, want.right)
    assert not records or r.faces == want.faces
    if want.xy is not None:
        assert np.array_equal(r.xy, want.xy) and np.array_equal(r.row_index, want.row_index) and (not origin or np.array_equal(r.origin, want.origin))
    else:
        assert r.xy is None


@functools.lru_cache(maxsize=None)
def map_of(kind, key):
    """the map of a case: computed once, shared, never changed"""
    return {"hand": lambda: EC.HAND[key][0], "lengths": EC.lengths_map, "row": EC.two_point_row, "sqrt": EC.sqrt_map, "odd": RP.odd_faces,
            "planar": lambda: planar(key)[0]}[kind]()


@functools.lru_cache(maxsize=None)
def planar(seed):
    return RP.planar_grid_map(np.random.default_rng(seed), 12, 10, RP.P_CHOICES[seed % 7], True, RP.SHEAR, (0, 0))


def planar_tol(seed):
    return 2 * planar(seed)[1]["det"]


@functools.lru_cache(maxsize=None)
def merged(kind, key, tol, flags):
    """the definition's answer: computed once, shared, never changed"""
    return ER.eliminate_ref(*map_of(kind, key), tol, flags)


STRUCTURAL = [("lengths", None, t) for t in (0, 1 << 90, HUGE)] + [("row", None, t) for t in (0, 1 << 100, HUGE)] + \
    [("sqrt", None, HUGE), ("odd", None, 0), ("odd", None, 3600), ("odd", None, HUGE)]
EVERY = [("hand", n, EC.HAND[n][1]) for n in sorted(EC.HAND)] + STRUCTURAL + [("planar", s, planar_tol(s)) for s in SEEDS]


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.HAND))
def test_definition_gives_the_written_answer(name):
    m, tol, faces, n_mutual, n_dropped = EC.HAND[name]
    for flags in (0, ER.DROP):
        r = merged("hand", name, tol, flags)
        assert {f["label"]: (f["target"], f["best"], f["flags"], f["area2"]) for f in r.faces} == faces
        assert [f["label"] for f in r.faces] == sorted(faces, key=ER.unsigned)
        c, nc = r.counts, len(m[2])
        assert c["n_faces"] == len(faces) and c["n_mutual"] == n_mutual and c["n_dropped"] == (n_dropped if flags else 0)
        assert c["n_slivers"] == sum(1 for v in faces.values() if v[2] & EC.SLIVER) and c["n_islands"] == sum(1 for v in faces.values() if v[2] & EC.ISLAND)
        assert c["n_eliminated"] == sum(1 for v in faces.values() if v[2] & EC.ELIMINATED)
        assert c["n_negative"] == sum(1 for v in faces.values() if v[2] & EC.NEGATIVE)
        assert c["n_chains"] == nc - c["n_dropped"] == len(r.left)
        target = {f: v[0] for f, v in faces.items()}
        target[0] = 0
        kept = [k for k in range(nc) if not (flags and m[2][k] != m[3][k] and target[int(m[2][k])] == target[int(m[3][k])])]
        assert r.left.tolist() == [target[int(m[2][k])] for k in kept] and r.right.tolist() == [target[int(m[3][k])] for k in kept]
        if flags:
            assert r.origin.tolist() == kept and c["n_points"] == len(r.xy) == sum(int(m[1][k + 1] - m[1][k]) for k in kept)
            assert all(np.array_equal(r.xy[r.row_index[j]:r.row_index[j + 1]], m[0][m[1][k]:m[1][k + 1]]) for j, k in enumerate(kept))


def test_definition_lengths_at_a_square():
    """d^2 = k^2 - 1, k^2, k^2 + 1 for k near 2^47, the longest edge there is, the shortest"""
    r = merged("sqrt", None, HUGE, 0)
    assert r.L == [k for _, _, k in EC.SQRT_EDGES] and EC.K > (1 << 47) - (1 << 26)


def test_hand_dangles_survive_the_drop():
    m = EC.HOLE
    r = merged("hand", "hole-and-dangles", 2, ER.DROP)
    dangles = [k for k in range(len(m[2])) if m[2][k] == m[3][k]]
    assert len(dangles) == 2 and set(dangles) <= set(r.origin.tolist())
    assert [(int(r.left[j]), int(r.right[j])) for j, k in enumerate(r.origin.tolist()) if k in dangles] == [(1, 1), (1, 1)]


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_twin(twin, what):
    m = map_of(*what[:2])
    for flags in (0, ER.DROP):
        want = merged(*what, flags)
        same(twin_eliminate(twin, m, what[2], flags), want)
        same(twin_eliminate(twin, m, what[2], flags, records=False, origin=False), want, records=False, origin=False)


@pytest.mark.parametrize("kind", ["lengths", "row", "sqrt"])
def test_twin_chain_sums(twin, kind):
    xy, row, _, _ = arrays(map_of(kind, None))
    nc = len(row) - 1
    S, L = np.zeros((nc, 2), np.uint64), np.zeros((nc, 2), np.uint64)
    twin.eliminate_twin_sums(xy.ctypes.data, row.ctypes.data, nc, S.ctypes.data, L.ctypes.data)
    want_S, want_L = ER.chain_sums([tuple(p) for p in xy.tolist()], row.tolist())
    assert [(int(hi) << 64 | int(lo)) for lo, hi in S] == [s % (1 << 128) for s in want_S]
    assert [(int(hi) << 64 | int(lo)) for lo, hi in L] == want_L


def test_twin_square_roots_at_full_range(twin):
    """2 000 random edges with both differences anywhere below 2^47, and the values round every square of a few"""
    rng = np.random.default_rng(2)
    d = rng.integers(-EC.SIDE, EC.SIDE + 1, size=(2000, 2))
    values = [int(dx) ** 2 + int(dy) ** 2 for dx, dy in d.tolist()]
    values += [k * k + e for k in (1, 2, 3, 1 << 32, (1 << 32) + 1, 94906265, 94906266, EC.K, EC.SIDE, 199032864766428) for e in (-1, 0, 1)] + [0]
    assert max(values) < 1 << 95
    for v in values:
        assert twin.eliminate_twin_isqrt(v & (2 ** 64 - 1), v >> 64) == math.isqrt(v)


# ---- the generated maps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_generated_map_areas_are_the_generators(seed):
    """area2 of every face = det x its triangle count, which the generator knows without any chain: an independent check of
    the area rule.  Every seed has a sliver (a face of one or two triangles)"""
    info, r = planar(seed)[1], merged("planar", seed, planar_tol(seed), 0)
    assert {f["label"]: f["area2"] for f in r.faces} == {f: info["det"] * n for f, n in info["triangles"].items() if f != 0}
    assert r.counts["n_slivers"] >= 1 and r.counts["n_negative"] == 0
    assert r.counts["n_slivers"] == sum(1 for f, n in info["triangles"].items() if f != 0 and n <= 2)


def test_generated_maps_are_worth_their_time():
    cs = [merged("planar", s, planar_tol(s), 0).counts for s in SEEDS]
    assert any(c["n_mutual"] > 0 for c in cs) and all(c["n_eliminated"] > 0 for c in cs)
    assert any(c["n_eliminated"] > c["n_mutual"] + 1 for c in cs)


# ---- the properties ------------------------------------------------------------------------------------------------------
def properties(eliminate, m, tol):
    """eliminate(map, tol, flags) -> Result"""
    m = arrays(m)
    r = eliminate(m, tol, ER.DROP)
    by_label = {f["label"]: f for f in r.faces}
    took = {}
    for f in r.faces:
        took[f["target"]] = took.get(f["target"], 0) + f["area2"]
        assert by_label[f["target"]]["target"] == f["target"]  # a target is a root: no cycle, no path left
        assert not f["flags"] & ER.ELIMINATED or f["flags"] & ER.SLIVER
    again = eliminate((r.xy, r.row_index, r.left, r.right), tol, ER.DROP)
    after = {f["label"]: f["area2"] for f in again.faces}
    # the area of a target is the sum of what it took, nobody else is left (a target all of whose chains went had no area)
    assert set(after) <= set(took) and all(after.get(t, 0) == a for t, a in took.items())
    assert all(a != b for a, b, k in zip(r.left.tolist(), r.right.tolist(), r.origin.tolist()) if m[2][k] != m[3][k])
    plain = eliminate(m, tol, 0)
    assert plain.faces == r.faces and np.array_equal(plain.left[r.origin], r.left) and np.array_equal(plain.right[r.origin], r.right)


@pytest.mark.parametrize("what", EVERY, ids=str)
def test_properties(twin, what):
    def by_twin(m, tol, flags):
        rc, r, _ = twin_eliminate(twin, m, tol, flags)
        assert rc == OK
        return r
    properties(by_twin, map_of(*what[:2]), what[2])
    properties(lambda m, tol, flags: ER.eliminate_ref(*m, tol, flags), map_of(*what[:2]), what[2])


@pytest.mark.parametrize("seed", SEEDS)
def test_rounds_end(seed):
    r, per_round = ER.rounds_ref(*map_of("planar", seed), planar_tol(seed), max_rounds=32)
    assert per_round[-1]["n_eliminated"] == 0 and 2 <= len(per_round) < 32
    assert all(not f["flags"] & ER.SLIVER or f["flags"] & ER.ISLAND for f in r.faces)  # what is left under tol has nobody to join


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_one_short(twin):
    m, tol = map_of("planar", 3), planar_tol(3)
    for flags in (0, ER.DROP):
        want = merged("planar", 3, tol, flags)
        c = want.counts
        assert c["n_eliminated"] > 0 and (not flags or 0 < c["n_dropped"] < len(m[2]))
        caps = (c["n_faces"], c["n_chains"], c["n_points"])
        rc, _, got = twin_eliminate(twin, m, tol, flags, capacities=(0, 0, 0))
        assert rc == OVERFLOW and got == c
        same(twin_eliminate(twin, m, tol, flags, capacities=caps), want)
        same(twin_eliminate(twin, m, tol, flags, capacities=tuple(v + 3 for v in caps)), want)
        for k in range(3):
            short = tuple(v - (1 if j == k else 0) for j, v in enumerate(caps))
            rc, _, got = twin_eliminate(twin, m, tol, flags, capacities=short)  # (twin_eliminate checks that nothing was written)
            assert (rc, got) == ((OK, c) if k == 2 and not flags else (OVERFLOW, c))
        same(twin_eliminate(twin, m, tol, flags, records=False, capacities=(0,) + caps[1:]), want, records=False)  # no records: no face capacity


def test_no_chains(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for flags in (0, ER.DROP):
        rc, _, c = twin_eliminate(twin, empty, 5, flags)
        assert rc == OK and c == dict.fromkeys(ER.COUNTS, 0) == ER.eliminate_ref(*empty, 5, flags).counts
    points = EC.chain_map([([(1, 1)], 4, 0), ([(2, 2)], 0, 0)])
    same(twin_eliminate(twin, points, HUGE, ER.DROP), ER.eliminate_ref(*points, HUGE, ER.DROP))


def refused(twin, m, tol=0, flags=0):
    """the definition refuses it, and so does the twin"""
    with pytest.raises(ER.Invalid):
        ER.eliminate_ref(*m, tol, flags)
    n = len(m[2])
    return twin_eliminate(twin, m, tol, flags)[0] == INVALID and twin_eliminate(twin, m, tol, flags, capacities=(2 * n, n, len(m[0])))[0] == INVALID


def test_bad_input(twin):
    xy, row, left, right = EC.chain_map([([(0, 0), (1, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    assert twin_eliminate(twin, (xy, row, left, right), 0)[0] == OK
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        assert refused(twin, (xy, np.array(bad_row, np.uint32), left, right))
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert refused(twin, (bad, row, left, right))
    assert refused(twin, (xy, row, left, right), flags=2) and refused(twin, (xy, row, left, right), flags=1 << 31)
    assert refused(twin, (xy, row, left, right), flags=3)
    assert refused(twin, (xy[:2], row, left, right))  # more chains than points
    assert refused(twin, (xy, np.zeros(1, np.uint32), left[:0], right[:0]))  # points without chains
    counts = np.zeros(9, np.uint64)
    for n_points, n_chains in ((1 << 32, 3), (1 << 31, 1 << 31), ((1 << 31) + 3, 3), (2, 3), (3, 0)):  # the size limits: refused before anything is read
        assert twin.eliminate_twin(None, n_points, None, None, None, n_chains, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None, counts.ctypes.data) == INVALID
    assert twin.eliminate_twin(None, (1 << 31) + 2, None, None, None, 3, 0, 0, 4, 0, 0, 0, None, None, None, None, None, None, counts.ctypes.data) == INVALID


def test_a_map_that_loses_every_chain(twin):
    """no face 0: everything merges into the outside face and RJ_ELIM_DROP leaves no chain.  That fits capacities of 0, so
    the sizing call, whose arrays are null, succeeds and must write nothing; the rounds end on the empty map"""
    m, tol, _, _, _ = EC.HAND["all-dropped"]
    want = merged("hand", "all-dropped", tol, ER.DROP)
    assert want.counts["n_chains"] == want.counts["n_points"] == 0 and want.counts["n_dropped"] == 1 and want.row_index.tolist() == [0]
    xy, row, left, right = arrays(m)
    counts = np.zeros(9, np.uint64)
    rc = twin.eliminate_twin(xy.ctypes.data, 5, row.ctypes.data, left.ctypes.data, right.ctypes.data, 1, tol, 0, ER.DROP, 0, 0, 0, None, None, None, None,
                             None, None, counts.ctypes.data)
    assert rc == OK and dict(zip(ER.COUNTS, (int(v) for v in counts))) == want.counts
    same(twin_eliminate(twin, m, tol, ER.DROP), want)
    same(twin_eliminate(twin, m, tol, ER.DROP, capacities=(2, 0, 0)), want)
    same(twin_eliminate(twin, m, tol, ER.DROP, records=False, origin=False, capacities=(0, 0, 0)), want, records=False, origin=False)
    last, per_round = ER.rounds_ref(*m, tol)
    assert [c["n_eliminated"] for c in per_round] == [1, 0] and per_round[1] == dict.fromkeys(ER.COUNTS, 0) and len(last.left) == 0


# ---- mutations of the header, each caught ------------------------------------------------------------------------------------
MUTATIONS = {
    # the tie between two borders of one length goes to the larger pair
    "tie-order": ("return a.pair < b.pair;", "return a.pair > b.pair;", "equal-borders"),
    # the smaller face of a mutual pair stays
    "mutual-winner": ("const bool stays = mine != other ? mine > other : k < g;", "const bool stays = mine != other ? mine < other : k < g;",
                      "mutual-larger-stays"),
    # a face of exactly tol is no sliver
    "at-tol": ("return !is_negative(area2) && (u128) area2 <= tol;", "return !is_negative(area2) && (u128) area2 < tol;", "longer-border"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_mutated_header_is_caught(name, tmp_path):
    old, new, case = MUTATIONS[name]
    text = open(HEADER).read()
    assert text.count(old) == 1
    (tmp_path / "rj_eliminate.h").write_text(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mutant_" + name)
    os.remove(os.path.join(BUILD, "libeliminate_twin_mutant_%s.so" % name))
    m, tol = EC.HAND[case][0], EC.HAND[case][1]
    rc, r, _ = twin_eliminate(L, m, tol, 0)
    assert rc == OK and r.faces != merged("hand", case, tol, 0).faces
    same(twin_eliminate(L, EC.HAND["row-of-three-tighter"][0], 59, 0), merged("hand", "row-of-three-tighter", 59, 0))  # (the same program otherwise)


# ---- the build's resource report ---------------------------------------------------------------------------------------------
def test_chain_sum_kernel_does_not_spill():
    """k_el_sums, the pass over every point: no scratch, no spilled register, 7 waves per SIMD or more (the build writes
    rayjoin_amd/csrc/resource_usage_eliminate.txt: -Rpass-analysis=kernel-resource-usage)"""
    import re
    report = os.path.join(CSRC, "resource_usage_eliminate.txt")
    assert os.path.exists(report), "no resource report: build the library first (__graft_entry__.build)"
    found, name = {}, None
    for line in open(report):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            found[name][m.group(1).strip()] = int(m.group(2))
    hits = [v for n, v in found.items() if "k_el_sums" in n]
    assert len(hits) == 1, sorted(n for n in found if "k_el" in n)
    assert hits[0]["ScratchSize"] == 0 and hits[0]["SGPRs Spill"] == 0 and hits[0]["VGPRs Spill"] == 0 and hits[0]["Occupancy"] >= 7, hits[0]


# ---- the stand-alone program ----------------------------------------------------------------------------------------------
def test_stand_alone_twin_program():
    """the twin with its own main (what a host sanitizer build is made from: -fsanitize=address,undefined on this very
    command line), run as a program of its own: five tolerances, with and without RJ_ELIM_DROP, the areas before and after;
    a map that loses every chain through the sizing call with null arrays"""
    exe = os.path.join(BUILD, "eliminate_twin_main")
    os.makedirs(BUILD, exist_ok=True)
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DELIMINATE_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == 11 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
