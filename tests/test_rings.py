"""Face rings of a chain map on the CPU: the plain-Python definition (tests/rings_ref.py) on hand-built maps with the
answers written out; the host twin of the device's per-element functions (tests/hosttwin/rings_twin.cc compiling
rayjoin_amd/csrc/rj_rings.h) against that definition, every array and every count, on the hand cases, on the helper
output maps of the overlay tests' pairs for every operation, and on the lattice pair's clip; the exact invariants that tie
the rings to the face table.  On the generated maps of tests/rings_planar.py: random planar subdivisions whose faces and
areas are known without the rings (union-find over lattice triangles), one junction of thousands of incidences, one ring of
exactly 2^k half-chains, chains of 100 000 points, face ids outside [0, 2^31), more than 2^20 half-chains.  The GPU side is
tests/test_gpu_rings.py."""
import functools
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rayjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_merge_ref as G  # noqa: E402
import overlay_ops_ref as R  # noqa: E402
import rings_cases as K  # noqa: E402
import rings_planar as P  # noqa: E402
import rings_ref as D  # noqa: E402
from test_overlay_map import records as pair_records  # noqa: E402
from test_overlay_ops import OPS, records  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "rings_twin.cc")
HDR = os.path.join(ROOT, "rayjoin_amd", "csrc", "rj_rings.h")
OUT = os.path.join(ROOT, "tests", "hosttwin", "_build", "librings_twin.so")
SKIP0, NOPTS = _capi.RJ_RINGS_SKIP_FACE0, _capi.RJ_RINGS_NO_POINTS


def twin_lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDR), "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.rings_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                             C.c_uint64] + [C.c_void_p] * 7
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def as_map(om):
    """an output-map dict of the overlay helpers -> (xy, row_index, left, right)"""
    return (np.ascontiguousarray(om["xy"], np.int64).reshape(-1, 2), np.ascontiguousarray(om["row_index"], np.uint32),
            np.ascontiguousarray(om["left"], np.int32), np.ascontiguousarray(om["right"], np.int32))


def twin_rings(L, m, flags=0, caps=None):
    """-> (status, dict of the arrays cut to min(count, capacity) and the counts, (doubling rounds, ranking rounds)).
    caps None: room for everything a map of this size can give"""
    xy, row, left, right = (np.ascontiguousarray(a) for a in m)
    nc, npts = len(left), len(xy)
    if caps is None:
        caps = (2 * nc, 2 * nc, 2 * (npts - nc))
    rc_, hc, pc = caps
    rings = np.zeros(rc_, D.RING_DTYPE)
    rings["face"] = -7
    first, half = np.full(rc_ + 1, 0xFFFFFFFF, np.uint32), np.full(hc, 0xFFFFFFFF, np.uint32)
    rrow, rxy = np.full(rc_ + 1, 0xFFFFFFFF, np.uint32), np.full((pc, 2), -7, np.int64)
    counts, stats = np.zeros(5, np.uint64), np.zeros(2, np.uint64)
    rc = L.rings_twin(xy.ctypes.data, npts, row.ctypes.data, left.ctypes.data, right.ctypes.data, nc, flags, rc_, hc, pc, rings.ctypes.data,
                      first.ctypes.data, half.ctypes.data, rrow.ctypes.data, rxy.ctypes.data, counts.ctypes.data, stats.ctypes.data)
    c = dict(zip(D.COUNTS, (int(v) for v in counts)))
    n, points = min(c["n_rings"], rc_), not (flags & NOPTS)
    got = dict(rings=rings[:n], ring_first=first[:n + 1], ring_half=half[:min(c["n_halves"], hc)], ring_row=rrow[:n + 1] if points else None,
               ring_xy=rxy[:min(c["n_points"], pc)] if points else None, counts=c)
    if not points:  # nothing was written there
        assert (rrow == 0xFFFFFFFF).all() and (rxy == -7).all()
    return rc, got, (int(stats[0]), int(stats[1]))


def summary(m, **kw):
    """[(face, leader, mixed, half-chains, area2)] of the definition"""
    return [(f, le, mx, hs, a2) for f, le, mx, hs, _, a2 in D.ring_list(*m)[0]]


# ---- the definition on hand-built maps, answers by hand --------------------------------------------------------------------
def test_two_rectangles_have_the_written_rings():
    """chains of the output map (units of U): 0 (4,2) (4,4) (3,4) [2|0]; 1 (3,4) (2,4) [1|0]; 2 (3,2) (4,2) [2|0];
    3 (2,4) (2,2) (3,2) [1|0]; 4 (3,2) (3,4) [1|2].  Face 2's ring: map 1 chain 0 forward (h = 4), map 0's first piece forward
    (h = 0), map 1 chain 2 backward (h = 9); from its leader 0: 0, 9, 4 -- the 1 x 2 rectangle [3,4] x [2,4], area2 = 4 U^2.
    Face 1: 2, 6, 8 round [2,3] x [2,4], 4 U^2.  Face 0: the backward half-chains 1, 5, 7, 3 clockwise round [2,4] x [2,4]:
    -8 U^2."""
    U = 1 << 20
    m = K.rect_output_map(U)
    assert summary(m) == [(0, 1, False, [1, 5, 7, 3], -8 * U * U), (1, 2, False, [2, 6, 8], 4 * U * U), (2, 0, False, [0, 9, 4], 4 * U * U)]
    ref = D.rings_ref(*m)
    assert ref["ring_first"].tolist() == [0, 4, 7, 10] and ref["ring_row"].tolist() == [0, 6, 10, 14]
    assert ref["ring_xy"][10:].tolist() == [[4 * U, 2 * U], [4 * U, 4 * U], [3 * U, 4 * U], [3 * U, 2 * U]]
    assert ref["ring_xy"][:6].tolist() == [[x * U, y * U] for x, y in [(3, 4), (4, 4), (4, 2), (3, 2), (2, 2), (2, 4)]]
    assert ref["counts"] == dict(n_rings=3, n_halves=10, n_points=14, n_mixed=0, n_skipped=0)
    assert D.area2_of(ref["rings"]) == [-8 * U * U, 4 * U * U, 4 * U * U]
    skip = D.rings_ref(*m, skip_face0=True)
    assert skip["rings"]["leader"].tolist() == [2, 0] and skip["ring_half"].tolist() == [2, 6, 8, 0, 9, 4] and skip["counts"]["n_points"] == 8


def test_hole_dangling_crossing_closed():
    # a square with a square hole: face 1 has one positive and one negative ring
    assert summary(K.square_with_hole()) == [(0, 1, False, [1], -200), (1, 0, False, [0], 200), (1, 3, False, [3], -18), (2, 2, False, [2], 18)]
    # a dangling chain: next = twin at its free end; the outside walks out along it and back
    m = K.dangling()
    nxt = D.successor(m[0], m[1])[0]
    assert nxt[2] == 3 and nxt[3] == 1 and nxt[1] == 2 and nxt[0] == 0
    assert summary(m) == [(0, 1, False, [1, 2, 3], -32), (1, 0, False, [0], 32)]
    assert D.rings_ref(*m)["ring_xy"].tolist() == [[0, 0], [0, 4], [4, 4], [4, 0], [0, 0], [-3, -3], [0, 0], [4, 0], [4, 4], [0, 4]]
    # a vertex of degree 4: the outside passes it twice, every square closes on itself
    assert summary(K.crossing()) == [(0, 1, False, [1, 3], -64), (1, 0, False, [0], 32), (2, 2, False, [2], 32)]
    assert summary(K.closed_chain()) == [(0, 1, False, [1], -36), (7, 0, False, [0], 36)]


def test_zero_length_edges_and_one_point_chains():
    m = K.zero_length_edges()
    assert summary(m) == [(0, 1, False, [1, 5, 3], -36), (1, 0, False, [0, 2, 4], 36)]
    ref = D.rings_ref(*m)
    assert ref["ring_xy"][5:].tolist() == [[0, 0], [0, 0], [6, 0], [0, 6], [0, 0]]  # (point count = edge count, zero edges included)
    m = K.one_point_chain()
    ref = D.rings_ref(*m)
    assert ref["counts"] == dict(n_rings=2, n_halves=2, n_points=6, n_mixed=0, n_skipped=2)
    assert ref["ring_half"].tolist() == [1, 0]


def test_star_of_forty_spokes_is_one_ring():
    m = K.star(40)
    (ring,) = summary(m)
    assert ring[0] == 0 and ring[1] == 0 and not ring[2] and sorted(ring[3]) == list(range(80)) and ring[4] == 0
    assert ring[3][:4] == [0, 1, 79, 78]  # out along spoke 0 and back, then the clockwise neighbour at the hub: spoke 39, digitised towards the hub (79 leaves it)


@pytest.mark.parametrize("n", K.NECKLACE_SIZES)
def test_necklace_has_two_rings(twin, n):
    m, area2 = K.necklace(n)
    assert area2 > 0
    rc, got, rounds = twin_rings(twin, m)
    assert rc == 0 and got["counts"] == dict(n_rings=2, n_halves=2 * n, n_points=6 * n, n_mixed=0, n_skipped=0)
    assert got["rings"]["face"].tolist() == [0, 1] and D.area2_of(got["rings"]) == [-area2, area2]
    assert got["ring_first"].tolist() == [0, n, 2 * n] and got["ring_row"].tolist() == [0, 3 * n, 6 * n]
    assert rounds[0] >= int(np.ceil(np.log2(n))) + 1  # the doubling cannot know sooner
    D.assert_same_rings(got, D.rings_ref(*m), n)


# ---- the twin against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.HAND))
def test_twin_equals_the_definition_on_the_hand_cases(twin, name):
    m = K.HAND[name]()
    for flags in (0, SKIP0, NOPTS, SKIP0 | NOPTS):
        rc, got, _ = twin_rings(twin, m, flags)
        assert rc == 0
        D.assert_same_rings(got, D.rings_ref(*m, skip_face0=bool(flags & SKIP0), points=not flags & NOPTS), (name, flags))


def test_empty_map(twin):
    m = K.chain_map([])
    rc, got, _ = twin_rings(twin, m)
    assert rc == 0 and got["counts"] == dict.fromkeys(D.COUNTS, 0) and got["ring_first"].tolist() == [0] and got["ring_row"].tolist() == [0]
    D.assert_same_rings(got, D.rings_ref(*m))


def helper_maps(oracle, name):
    """(what, map) over all 15 operations, drop on and off, and merged"""
    _, _, _, all_ = records(oracle, name)
    for how, by in OPS:
        for drop in (False, True):
            om = R.output_map(all_, how, by, drop_degenerate=drop)
            yield (name, how, by, drop, False), om
            yield (name, how, by, drop, True), G.merged_map(om)


@pytest.mark.parametrize("name", ["sample", "rings", "nested"])
def test_twin_equals_the_definition_on_the_helper_output_maps(oracle, twin, name):
    seen = 0
    for what, om in helper_maps(oracle, name):
        m = as_map(om)
        rc, got, _ = twin_rings(twin, m)
        assert rc == 0, what
        D.assert_same_rings(got, D.rings_ref(*m), what)
        seen += 1
    assert seen == 60


_lattice = {}


def lattice_map(oracle, how, by, merged=False):
    key = (how, by, merged)
    if key not in _lattice:
        ctx, xs, pip = pair_records(oracle, "lattice")
        if "walk" not in _lattice:
            _lattice["walk"] = R.walk_np(ctx.maps, xs, pip)
        om = R.output_map_np(ctx.maps, xs, pip, how, by, walk=_lattice["walk"])
        _lattice[key] = G.merged_map(om, np_form=True) if merged else om
    return _lattice[key]


def test_twin_equals_the_definition_on_the_lattice_clip(oracle, twin):
    """3 785 chains, 10 rings, the longest of 1 727 half-chains: at least 11 doubling rounds"""
    m = as_map(lattice_map(oracle, "intersection", "map0"))
    want = D.rings_ref(*m)
    rc, got, rounds = twin_rings(twin, m)
    assert rc == 0
    D.assert_same_rings(got, want)
    longest = int(np.diff(want["ring_first"].astype(np.int64)).max())
    assert len(m[2]) > 3000 and longest > 1024 and rounds[0] >= 11 and rounds[1] >= 11
    assert want["counts"]["n_mixed"] == 0


# ---- invariants ----------------------------------------------------------------------------------------------------------
def face_sums(got):
    sums = {}
    for f, a2 in zip(got["rings"]["face"].tolist(), D.area2_of(got["rings"])):
        sums[f] = sums.get(f, 0) + a2
    return sums


def check_areas(got, rows, what):
    """the rings of face k sum to row k - 1 of the face table, exactly; every face has a ring"""
    assert got["counts"]["n_mixed"] == 0, what
    sums = face_sums(got)
    sums.pop(0, None)
    assert sorted(sums) == list(range(1, len(rows) + 1)), what
    assert [sums[k + 1] for k in range(len(rows))] == [r[2] for r in rows], what


@pytest.mark.parametrize("name", ["sample", "rings"])
def test_ring_areas_sum_to_the_face_table(oracle, twin, name):
    _, _, _, all_ = records(oracle, name)
    rows = {op: R.face_rows(all_, *op) for op in OPS}
    for what, om in helper_maps(oracle, name):
        rc, got, _ = twin_rings(twin, as_map(om), NOPTS)
        assert rc == 0
        check_areas(got, rows[what[1:3]], what)


@pytest.mark.parametrize("op", [("intersection", "map0"), ("intersection", "pair")])
def test_ring_areas_sum_to_the_face_table_on_the_lattice(oracle, twin, op):
    ctx, xs, pip = pair_records(oracle, "lattice")
    lattice_map(oracle, *op)
    rows = R.face_rows_np(ctx.maps, xs, pip, *op, walk=_lattice["walk"])
    for merged in (False, True):
        rc, got, _ = twin_rings(twin, as_map(lattice_map(oracle, *op, merged=merged)), NOPTS)
        assert rc == 0
        check_areas(got, rows, (op, merged))


def test_prototype_counts(oracle, twin):
    """what the definition gives on three maps: rings, rings of face 0, holes (negative rings) of other faces"""
    def facts(m):
        rc, got, _ = twin_rings(twin, m, NOPTS)
        assert rc == 0
        a2, face = np.array(D.area2_of(got["rings"]), dtype=object), got["rings"]["face"]
        return len(m[2]), got["counts"]["n_rings"], int((face == 0).sum()), int(((face != 0) & (a2 < 0)).sum())

    _, _, _, sample = records(oracle, "sample")
    assert facts(as_map(R.output_map(sample, "intersection", "pair"))) == (416, 190, 1, 0)
    ctx, _, _, rings = records(oracle, "rings")
    assert facts(as_map(R.output_map(rings, "union", "pair")))[:2] == (196, 157)
    assert facts(as_map(R.output_map(rings, "union", "pair")))[3] == 47
    m0 = ctx.maps[0]
    got = facts((m0.pts, m0.row_index, m0.left.astype(np.int32), m0.right.astype(np.int32)))
    assert got[:2] == (60, 120) and got[3] == 0


def test_overlapping_chains_give_mixed_rings_like_the_definition(oracle, twin):
    _, _, _, all_ = records(oracle, "nested")
    m = as_map(R.output_map(all_, "intersection", "pair"))
    rc, got, _ = twin_rings(twin, m)
    want = D.rings_ref(*m)
    assert rc == 0 and got["counts"]["n_mixed"] == want["counts"]["n_mixed"] > 0
    assert int((got["rings"]["flags"] & _capi.RJ_RING_MIXED).astype(bool).sum()) == got["counts"]["n_mixed"]


# ---- overflow and flags -----------------------------------------------------------------------------------------------
def test_each_capacity_one_short_overflows_with_the_true_counts(oracle, twin):
    _, _, _, all_ = records(oracle, "sample")
    m = as_map(R.output_map(all_, "union", "pair"))
    want = D.rings_ref(*m)
    true = tuple(want["counts"][k] for k in ("n_rings", "n_halves", "n_points"))
    rc, got, _ = twin_rings(twin, m, caps=(0, 0, 0))  # the sizing call
    assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == want["counts"]
    for short in range(3):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(true))
        rc, got, _ = twin_rings(twin, m, caps=caps)
        assert rc == _capi.RJ_E_OVERFLOW and got["counts"] == want["counts"], short
    rc, got, _ = twin_rings(twin, m, caps=true)
    assert rc == 0
    D.assert_same_rings(got, want)
    # without points the point capacity does not count
    rc, got, _ = twin_rings(twin, m, NOPTS, caps=(true[0], true[1], 0))
    assert rc == 0 and got["counts"] == want["counts"]
    D.assert_same_rings(got, D.rings_ref(*m, points=False))
    rc, _, _ = twin_rings(twin, m, 4)
    assert rc == _capi.RJ_E_INVALID


def test_symbol_record_and_flags():
    assert "rj_map_rings" in _capi.SYMBOLS and hasattr(_capi.load(), "rj_map_rings")
    assert _capi.RING_DTYPE == D.RING_DTYPE and _capi.RING_DTYPE.itemsize == 32
    assert (_capi.RJ_RINGS_SKIP_FACE0, _capi.RJ_RINGS_NO_POINTS, _capi.RJ_RING_MIXED) == (1, 2, 1)
    assert _capi.RINGS_COUNTS == D.COUNTS


# ---- generated maps (tests/rings_planar.py) ------------------------------------------------------------------------------
# the planar seeds the GPU test runs, and a dozen more for the twin
PLANAR_GPU_SEEDS = (4, 5, 6, 7, 9, 13, 18, 28)
PLANAR_SEEDS = PLANAR_GPU_SEEDS + (1, 2, 3, 8, 10, 11, 12, 14, 15, 16, 17, 19)
GENERATED = {"fan-300": lambda: P.fan(300), "fan-3000": lambda: P.fan(3000), "sliver-fan-300": lambda: P.sliver_fan(300),
             "sliver-fan-3000": lambda: P.sliver_fan(3000), "tie-fan-200": lambda: P.tie_fan(200), "tie-fan-1500": lambda: P.tie_fan(1500),
             "long-chains": P.long_chains, "odd-faces": P.odd_faces}
GENERATED.update({"path-%d" % n: functools.partial(P.path, n) for n in (64, 65, 32768, 32769)})


@functools.lru_cache(maxsize=None)
def planar_case(seed):
    """-> (map, info, the definition's answer, the definition's answer under SKIP0 | NOPTS): computed once, shared, left unchanged"""
    m, info = P.draw_planar(seed)
    return m, info, D.rings_ref(*m), D.rings_ref(*m, skip_face0=True, points=False)


@functools.lru_cache(maxsize=None)
def generated_case(name):
    """-> (map, the definition's answer): computed once, shared, left unchanged"""
    m = GENERATED[name]()
    return m, D.rings_ref(*m)


def fan_walk(n):
    """the one ring of P.fan(n), written out: chain c < n is the spoke to (T, T - c), chain n - 1 + k the spoke to (T - k, T);
    counter-clockwise at the hub the chains are n - 1, ..., 0, n, ..., 2 n - 2.  The walk leaves the hub along chain 0, comes
    back, and takes the clockwise neighbour each time: chains 0, 1, ..., n - 1, 2 n - 2, ..., n.  An even chain is digitised
    from the hub (2 c leaves it), an odd one towards it (2 c + 1 leaves it)."""
    out = []
    for c in list(range(n)) + list(range(2 * n - 2, n - 1, -1)):
        out.extend([2 * c, 2 * c + 1] if c % 2 == 0 else [2 * c + 1, 2 * c])
    return out


@pytest.mark.parametrize("seed", PLANAR_SEEDS)
def test_planar_maps_have_the_faces_and_areas_of_the_union_find(twin, seed):
    """the definition and the twin on a random planar subdivision, against an answer that does not come from the rings:
    per face, det x the number of lattice triangles the union-find gave it"""
    m, info, want, want_skip = planar_case(seed)
    P.assert_planar_answer(want, info, what=seed)
    P.assert_planar_answer(want_skip, info, skip_face0=True, what=seed)
    for flags, ref in ((0, want), (SKIP0 | NOPTS, want_skip)):
        rc, got, _ = twin_rings(twin, m, flags)
        assert rc == 0
        D.assert_same_rings(got, ref, (seed, flags))
        P.assert_planar_answer(got, info, skip_face0=bool(flags & SKIP0), what=(seed, flags))


def test_planar_seeds_have_holes_trees_long_rings_wide_junctions_and_wide_areas():
    """what the seeds of the GPU test must contain, on the definition alone, so that test cannot run empty"""
    holes = trees = longest = degree = bits = 0
    for seed in PLANAR_GPU_SEEDS:
        m, info, want, _ = planar_case(seed)
        a2, face = D.area2_of(want["rings"]), want["rings"]["face"].tolist()
        holes += sum(1 for f, a in zip(face, a2) if f != 0 and a < 0)
        trees += sum(1 for a in a2 if a == 0)
        longest = max(longest, int(np.diff(want["ring_first"].astype(np.int64)).max()))
        ends = np.concatenate([m[0][m[1][:-1].astype(np.int64)], m[0][m[1][1:].astype(np.int64) - 1]])  # the chains' end points
        degree = max(degree, int(np.unique(ends, axis=0, return_counts=True)[1].max()))
        if info["full_range"]:
            bits = max(bits, max(abs(a) for a in a2).bit_length())
            assert m[0].max() > (1 << 46) - (1 << 40) and m[0].min() < -(1 << 46) + (1 << 40), seed
    assert holes >= 1 and trees >= 1 and longest > 256 and degree == 8 and bits > 64, (holes, trees, longest, degree, bits)
    assert sum(1 for s in PLANAR_GPU_SEEDS if planar_case(s)[1]["frame"]) in range(2, 7)
    assert sum(1 for s in PLANAR_GPU_SEEDS if planar_case(s)[1]["full_range"]) in range(2, 7)


def test_fan_is_one_ring_in_the_written_order(twin):
    """599 directions of length 2^47 on one point, neighbours one unit apart: the walk written out in fan_walk"""
    n = 300
    m, want = generated_case("fan-%d" % n)
    assert want["counts"] == dict(n_rings=1, n_halves=2 * (2 * n - 1), n_points=2 * (2 * n - 1), n_mixed=0, n_skipped=0)
    assert want["ring_half"].tolist() == fan_walk(n) and D.area2_of(want["rings"]) == [0]
    for flags in (0, NOPTS):
        rc, got, _ = twin_rings(twin, m, flags)
        assert rc == 0
        D.assert_same_rings(got, D.rings_ref(*m, points=not flags) if flags else want, flags)


def test_sliver_fan_orders_cross_products_of_one_unit(twin):
    """300 directions whose cross products are j - j' between two products of 2^94"""
    m, want = generated_case("sliver-fan-300")
    inc = [(int(a[0]) - int(b[0]), int(a[1]) - int(b[1])) for a, b in ((m[0][2 * c + 1 - c % 2], m[0][2 * c + c % 2]) for c in range(300))]
    assert all(0 < abs(p[0] * q[1] - p[1] * q[0]) < 300 for p, q in zip(inc, inc[1:])) and min(min(p) for p in inc) > 1 << 46
    assert float(inc[0][0]) * float(inc[1][1]) == float(inc[0][1]) * float(inc[1][0])  # (what a comparator in double would see)
    assert want["counts"]["n_rings"] == 1 and want["counts"]["n_halves"] == 600 and D.area2_of(want["rings"]) == [0]
    rc, got, _ = twin_rings(twin, m)
    assert rc == 0
    D.assert_same_rings(got, want)


def test_tie_fan_is_ordered_by_h(twin):
    """200 chains along one direction from each of two hubs, 300 spokes round them: h alone orders the ties; the first
    hub's ring mixes faces, the second's does not"""
    m, want = generated_case("tie-fan-200")
    assert want["counts"] == dict(n_rings=2, n_halves=2000, n_points=2000, n_mixed=1, n_skipped=0)
    assert sorted(want["rings"]["flags"].tolist()) == [0, 1] and want["rings"]["face"][want["rings"]["flags"] == 0].tolist() == [5]
    for flags in (0, SKIP0, NOPTS):
        rc, got, _ = twin_rings(twin, m, flags)
        assert rc == 0
        D.assert_same_rings(got, D.rings_ref(*m, skip_face0=bool(flags & SKIP0), points=not flags & NOPTS) if flags else want, flags)


@pytest.mark.parametrize("n", [64, 65, 32768, 32769])
def test_path_is_one_ring_within_the_round_budget(twin, n):
    """one ring of exactly 2 n half-chains.  The budget is the smallest `rounds` with 2^(rounds - 1) >= 2 n; a ring of
    2^k half-chains needs all k + 1 of them, the last one being the round in which no minimum changes"""
    m, want = generated_case("path-%d" % n)
    assert want["counts"] == dict(n_rings=1, n_halves=2 * n, n_points=2 * n, n_mixed=0, n_skipped=0)
    rc, got, rounds = twin_rings(twin, m)
    assert rc == 0  # (5 = RJ_E_INTERNAL: the budget ran out)
    D.assert_same_rings(got, want, n)
    budget = (2 * n - 1).bit_length() + 1
    assert rounds[0] <= budget and rounds[1] <= budget
    if 2 * n & (2 * n - 1) == 0:
        assert rounds[0] == budget == {128: 8, 65536: 17}[2 * n]


def check_shoelace(got):
    row = got["ring_row"].astype(np.int64)
    assert [P.shoelace(got["ring_xy"][row[k]:row[k + 1]]) for k in range(len(got["rings"]))] == D.area2_of(got["rings"])


def test_long_chains(twin):
    """chains of 100 003 and 50 000 points, 74 and 79 zero-length edges at a chain's end: every array against the
    definition, and the shoelace sum of every ring's points is its area2"""
    m, want = generated_case("long-chains")
    lengths = np.diff(m[1].astype(np.int64)).tolist()
    assert lengths == [100_003, 50_000, 100_083] and (m[0][100_003:100_003 + 75] == m[0][100_003]).all() and (m[0][-81:] == m[0][-1]).all()
    assert [(f, le) for f, le, *_ in D.ring_list(*m)[0]] == [(0, 1), (1, 0), (1, 4), (2, 5)]
    a2 = D.area2_of(want["rings"])
    assert a2[0] == -a2[1] and a2[2] == -a2[3] and a2[1] > 3 * a2[3] > 0 and want["counts"]["n_points"] == 2 * (100_002 + 49_999 + 100_082)
    assert P.shoelace(np.array([[0, 0], [-(1 << 46), 5], [(1 << 46) - 1, -(1 << 46)]])) == (1 << 92) - 5 * ((1 << 46) - 1)
    check_shoelace(want)
    rc, got, _ = twin_rings(twin, m)
    assert rc == 0
    D.assert_same_rings(got, want)


def check_face_order(got, skip_face0):
    """the rings ascend by ((uint32) face, leader): negative faces behind every non-negative one"""
    face, leader = got["rings"]["face"].astype(np.int64), got["rings"]["leader"].astype(np.int64)
    key = [((f & 0xFFFFFFFF) << 32) | le for f, le in zip(face.tolist(), leader.tolist())]
    assert key == sorted(key) and len(set(key)) == len(key)
    neg = np.flatnonzero(face < 0)
    assert len(neg) and (face[neg[0]:] < 0).all() and (face[:neg[0]] >= 0).all()
    assert bool((face == 0).any()) != skip_face0


def test_faces_outside_31_bits_sort_as_unsigned(twin):
    m, want = generated_case("odd-faces")
    assert set(P.ODD_FACES) <= set(m[2].tolist()) | set(m[3].tolist())
    assert want["rings"]["face"].tolist() == sorted(want["rings"]["face"].tolist(), key=lambda f: f & 0xFFFFFFFF)
    assert want["rings"]["face"][-1] == -1 and (want["rings"]["face"] == -(1 << 31)).any() and want["counts"]["n_rings"] == 28
    for flags in (0, SKIP0):
        ref = D.rings_ref(*m, skip_face0=True) if flags else want
        check_face_order(ref, bool(flags))
        rc, got, _ = twin_rings(twin, m, flags)
        assert rc == 0
        D.assert_same_rings(got, ref, flags)


FIELD = 530_000


def check_triangle_field(got, n):
    """the closed forms of P.triangle_field(n): every half-chain is a ring of its own of three points and area2 +-36;
    the rings of face f are the half-chains of column f - 1, contiguous and in leader order"""
    assert got["counts"] == dict(n_rings=2 * n, n_halves=2 * n, n_points=6 * n, n_mixed=0, n_skipped=0)
    h = np.arange(2 * n, dtype=np.int64)
    order = np.lexsort((h, (h >> 1) % 1000))
    assert np.array_equal(got["rings"]["leader"], order) and np.array_equal(got["ring_half"], order)
    assert np.array_equal(got["rings"]["face"], (order >> 1) % 1000 + 1) and not got["rings"]["flags"].any()
    assert np.array_equal(got["ring_first"], np.arange(2 * n + 1)) and np.array_equal(got["ring_row"], 3 * np.arange(2 * n + 1))
    ccw = ((order >> 1) % 3 == 2) == (order & 1).astype(bool)  # (a chain digitised clockwise and walked backwards is counter-clockwise)
    assert np.array_equal(got["rings"]["area2_lo"].view(np.int64), np.where(ccw, 36, -36))
    assert np.array_equal(got["rings"]["area2_hi"], np.where(ccw, 0, -1))


def test_triangle_field_on_the_twin_has_the_closed_forms(twin):
    """1 060 000 half-chains, more than the 1 048 576 threads of the device's largest grid"""
    rc, got, _ = twin_rings(twin, P.triangle_field(FIELD))
    assert rc == 0 and 2 * FIELD > 4096 * 256
    check_triangle_field(got, FIELD)
    # and on a field small enough for the definition
    m = P.triangle_field(2500)
    want = D.rings_ref(*m)
    check_triangle_field(want, 2500)
    rc, got, _ = twin_rings(twin, m)
    assert rc == 0
    D.assert_same_rings(got, want)
