"""Crossings inside one map on the CPU: the plain-Python definition (tests/crossings_ref.py) on the hand-built maps of
tests/crossings_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/crossings_twin.cc compiling rayjoin_amd/csrc/rj_crossings.h) against that definition, every record and
every count: all hand cases at the chosen shift and at the forced shifts 15, 20, 33 and 47, 40 random soups, 20 planar
maps of tests/rings_planar.py (no crossing) and the same maps with chains thrown across them, the shapes that try the
grid, the contract of the call and the guard.  The GPU side is tests/test_gpu_crossings.py.

Mutations of a scratch copy of rj_crossings.h (RJ_CROSSINGS_HEADER_DIR points the twin's build at it), and the tests
here that fail under each (380 tests at the time):
  the anchor cell taken as min instead of max (pair_kind): 67 -- 21 hand cases at forced shifts (the pairs whose
      edges start in different cells), "across-zero" and "two-long-mixed-sign" at the chosen shift, 4 rim cases
      (diagonal-proper, -both, -touch, touch-at-the-rim at shift 46), 30 soups, 7 thrown-chain maps, the edge over a
      thousand cells, the factors test, the sizing test
  `<` made `<=` in the collinear branch (end to end counts as an overlap): 102 -- all 20 planar maps, all 20
      thrown-chain maps, all 40 soups, "bend-in-chain", "corner-collinear" and its reversed form, "junction", the same
      four at every forced shift
  the closed-box test made open (in_box): 64 -- every touch on an axis-parallel edge ("t", "t-end-of-second",
      "vertex-on-neighbour", "touch-on-a-corner", "touch-at-the-rim") at every shift, all 40 soups
  the i < j loop made i <= j (row_limit): 310 -- every map with a live edge: each is reported equal to itself
  the second zero sign not looked at (o2 == 0 dropped from relate): 49 -- "vertex-on-neighbour" and
      "touch-at-the-rim" at every shift, all 40 soups
  a work item every 65 rows instead of every 64 (item_flag): 48 -- the stars of 65, 128, 129 and 200 edges, 31 soups
      and 11 thrown-chain maps with a cell of more than 64 edges"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_cases as CC  # noqa: E402
import crossings_ref as CR  # noqa: E402
import rings_planar as P  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "crossings_twin.cc")
HDR_DIR = os.environ.get("RJ_CROSSINGS_HEADER_DIR", os.path.join(ROOT, "rayjoin_amd", "csrc"))  # (a scratch copy: the mutation runs)
HDRS = [os.path.join(HDR_DIR, "rj_crossings.h"), os.path.join(ROOT, "rayjoin_amd", "csrc", "rj_rings.h")]
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "libcrossings_twin%s.so" % ("" if "RJ_CROSSINGS_HEADER_DIR" not in os.environ else "_mutant"))
SHIFTS = (15, 20, 33, 47)
SOUP_SEEDS = tuple(range(40))
PLANAR_SEEDS = tuple(range(20))
CANARY = 0xABABABAB
RECORD = np.dtype([("eid", np.uint32, 2), ("kind", np.uint32), ("_pad", np.uint32)])
OK, INVALID, OVERFLOW = 0, 1, 3


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", HDR_DIR, "-I", os.path.dirname(HDRS[1]), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.crossings_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                 C.c_uint64, C.c_uint64, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def twin_crossings(L, m, capacity=None, shift=0, budget=0, flags=0, factors=(0, 0)):
    """-> (status, records cut to min(n_found, capacity) as tuples, counts, stats).  capacity None: the sizing call, then
    the exact capacity.  Behind the capacity lie canaries that must survive."""
    xy, row = np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32)
    nc = len(row) - 1 if len(row) else 0
    counts, stats = np.zeros(7, np.uint64), np.zeros(6, np.uint64)

    def call(cap, out):
        return L.crossings_twin(xy.ctypes.data, len(xy), row.ctypes.data, nc, flags, cap, out.ctypes.data if out is not None else None, counts.ctypes.data,
                                shift, budget, factors[0], factors[1], stats.ctypes.data)
    if capacity is None:
        rc = call(0, None)
        if rc not in (OK, OVERFLOW):
            return rc, [], dict(zip(CR.COUNTS, (int(v) for v in counts))), tuple(int(v) for v in stats)
        capacity = int(counts[0])
    out = np.full(capacity + 3, CANARY, np.uint32).repeat(4).view(RECORD)
    rc = call(capacity, out)
    c = dict(zip(CR.COUNTS, (int(v) for v in counts)))
    assert (out[capacity:].view(np.uint32) == CANARY).all()
    got = out[:min(c["n_found"], capacity)] if rc == OK else out[:0]
    return rc, [(int(r["eid"][0]), int(r["eid"][1]), int(r["kind"])) for r in got], c, tuple(int(v) for v in stats)


def want_counts(records, ne, zero):
    c = dict.fromkeys(CR.COUNTS, 0)
    c.update(n_found=len(records), n_edges=ne, n_zero_edges=zero)
    for _, _, k in records:
        c[CR.KIND_NAME[k]] += 1
    return c


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """-> (the map, the written records, the written counts, the definition's answer): computed once, shared"""
    if name in CC.HAND:
        chains, want, zero = CC.HAND[name]
        m = CC.as_map(chains)
    elif name in CC.ABSOLUTE:
        m, want, zero = CC.absolute_map(name)
    else:
        m, want, zero = CC.grid_map(name)
    return m, want, want_counts(want, len(m[0]) - (len(m[1]) - 1), zero), CR.map_crossings_ref(*m)


@functools.lru_cache(maxsize=None)
def star_case(n):
    chains, want, zero = CC.star(n)
    return CC.chain_arrays(chains), want, want_counts(want, n, zero)


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    m = CC.soup(seed)
    return m, CR.map_crossings_ref(*m)


@functools.lru_cache(maxsize=None)
def planar_case(seed):
    m, _ = P.draw_planar(seed)
    return m[0], m[1]


@functools.lru_cache(maxsize=None)
def thrown_case(seed):
    m = CC.throw_chains(planar_case(seed), seed)
    return m, CR.map_crossings_ref(*m)


ALL_HAND = sorted(CC.HAND) + sorted(CC.ABSOLUTE) + sorted(CC.GRID)


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_HAND)
def test_definition_gives_the_written_answer(name):
    _, want, counts, (records, got_counts) = hand_case(name)
    assert records == want and got_counts == counts


def test_soups_hold_every_kind():
    """the random maps are worth their time: across the seeds every kind occurs, and zero edges"""
    total = dict.fromkeys(CR.COUNTS, 0)
    for seed in SOUP_SEEDS[:10]:
        for k, v in soup_case(seed)[1][1].items():
            total[k] += v
    assert all(total[k] > 0 for k in ("n_proper", "n_touch", "n_overlap", "n_equal", "n_zero_edges"))


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_HAND)
def test_twin_hand_cases(twin, name):
    m, want, counts, _ = hand_case(name)
    rc, got, c, _ = twin_crossings(twin, m)
    assert rc == OK and got == want and c == counts


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", sorted(CC.HAND) + sorted(CC.GRID))
def test_twin_hand_cases_at_forced_shifts(twin, name, shift):
    m, want, counts, _ = hand_case(name)
    rc, got, c, stats = twin_crossings(twin, m, shift=shift)
    assert rc == OK and got == want and c == counts
    if want:
        assert stats[0] == shift


def test_forced_shifts_change_the_grid(twin):
    """shift 15 means thousands of cells for a hand case, shift 47 one"""
    m = hand_case("x")[0]
    regs = [twin_crossings(twin, m, shift=s)[3][1] for s in SHIFTS]
    assert regs[0] > 1000 and regs[-1] == 3 and sorted(regs, reverse=True) == regs


@pytest.mark.parametrize("name", ["diagonal-proper", "diagonal-none", "diagonal-both", "diagonal-touch", "diagonal-miss", "touch-at-the-rim"])
def test_twin_rim_cases_in_one_cell(twin, name):
    """(domain-long edges: only the widest shifts keep their registrations few)"""
    m, want, counts, _ = hand_case(name)
    for shift in (46, 47):
        rc, got, c, _ = twin_crossings(twin, m, shift=shift)
        assert rc == OK and got == want and c == counts


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_twin_soups(twin, seed):
    m, (records, counts) = soup_case(seed)
    rc, got, c, _ = twin_crossings(twin, m)
    assert rc == OK and got == records and c == counts
    if seed % 4 == 0:
        for shift in (15, 22, 47):
            rc, got, c, _ = twin_crossings(twin, m, shift=shift)
            assert rc == OK and got == records and c == counts


@pytest.mark.parametrize("seed", PLANAR_SEEDS)
def test_twin_planar_maps_have_no_crossing(twin, seed):
    m = planar_case(seed)
    rc, got, c, _ = twin_crossings(twin, m)
    assert rc == OK and got == [] and c["n_found"] == 0 and c["n_edges"] == len(m[0]) - (len(m[1]) - 1)


@pytest.mark.parametrize("seed", PLANAR_SEEDS)
def test_twin_planar_maps_with_thrown_chains(twin, seed):
    m, (records, counts) = thrown_case(seed)
    rc, got, c, _ = twin_crossings(twin, m)
    assert rc == OK and got == records and c == counts
    assert counts["n_found"] > 0


# ---- the shapes that try the grid -------------------------------------------------------------------------------------------
def test_long_edge_spans_a_thousand_cells(twin):
    m, want, counts, _ = hand_case("long-last-cell")
    rc, got, c, stats = twin_crossings(twin, m, shift=15)
    assert rc == OK and got == want and stats[1] > 1000


def test_two_long_edges_give_one_record(twin):
    m, want, counts, _ = hand_case("two-long")
    rc, got, c, stats = twin_crossings(twin, m, shift=15)
    assert rc == OK and got == want and len(got) == 1
    assert stats[2] == 2 and stats[3] > 1000  # thousands of cells hold both edges: the pair is tested in one of them


@pytest.mark.parametrize("n", CC.STAR_SIZES)
def test_twin_star_in_one_cell(twin, n):
    """runs longer than a row block, with lengths on both sides of a multiple of 64"""
    m, want, counts = star_case(n)
    for shift in (0, 15, 47):
        rc, got, c, stats = twin_crossings(twin, m, shift=shift)
        assert rc == OK and got == want and c == counts
        assert stats[2] == n and stats[3] == n * (n - 1) // 2 and stats[4] == (n + 63) // 64


def test_choice_of_shift_does_not_change_the_result(twin):
    m, (records, counts) = soup_case(3)
    for factors in ((1, 2), (4, 8), (1, 8), (64, 1)):
        rc, got, c, _ = twin_crossings(twin, m, factors=factors)
        assert rc == OK and got == records and c == counts


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_overflow(twin):
    m, (records, counts) = soup_case(1)
    n = counts["n_found"]
    assert n > 3
    rc, got, c, _ = twin_crossings(twin, m, capacity=0)
    assert rc == OVERFLOW and c == counts
    rc, got, c, _ = twin_crossings(twin, m, capacity=n)
    assert rc == OK and got == records and c == counts
    rc, got, c, _ = twin_crossings(twin, m, capacity=n - 1)  # (twin_crossings checks the canaries behind the capacity)
    assert rc == OVERFLOW and c == counts
    rc, got, c, _ = twin_crossings(twin, m, capacity=n + 5)
    assert rc == OK and got == records


def test_bad_input(twin):
    xy, row = hand_case("x")[0]
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6]):
        assert twin_crossings(twin, (xy, np.array(bad_row, np.uint32)))[0] == INVALID
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert twin_crossings(twin, (bad, row))[0] == INVALID
    assert twin_crossings(twin, (xy, row), flags=1)[0] == INVALID
    assert twin_crossings(twin, (xy, row))[0] == OK


def test_guard(twin):
    for n, refused in ((30, True), (10, False)):
        chains, want, _ = CC.star(n)
        rc, got, c, stats = twin_crossings(twin, CC.chain_arrays(chains), budget=100)
        assert (rc == INVALID) == refused and stats[5] == (1 if refused else 0) and stats[3] == n * (n - 1) // 2
        if not refused:
            assert got == want
