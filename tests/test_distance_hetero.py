"""The two distance queries on the CPU over the inputs of tests/distance_cases.py: for every heterogeneous family of
tests/skewed_pairs.py, both bases and every point set the nearest twin with the filter and the prune equals the one
without, array for array, and a sample of 16 points equals the definition in Python integers, cross-multiplied, over all
edges -- and so does the within twin at three distances; the near-tie and the exact-tie fan, alone at full scale and at 72
centres, equal the definition in all eight variants, and no two of a centre's candidates are separable in double; every
new point set has its defining property, asserted from the integers; three mutations of a scratch copy of the header --
a filter that decides equal doubles, a carry dropped from w5_mul3, a prune one cell too eager -- each fail the same
checks that pass above.  The GPU side is tests/test_gpu_distance_hetero.py."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distance_cases as DC  # noqa: E402
import nearest_ref as NR  # noqa: E402
import skewed_pairs as S  # noqa: E402
import test_nearest as TN  # noqa: E402
import test_within as TW  # noqa: E402
from test_nearest import check_dist, tuples_of  # noqa: E402

SAMPLE = 16
STRIDE = 4   # the within twin runs on every fourth point of a set (three distances, two variants each: brute forces)
FAMILY_BASES = [(name, base) for name in S.NAMES for base in (0, 1)]
SCENES = [("tie", "single"), ("tie", "replicated"), ("equal", "single"), ("equal", "replicated")]


@pytest.fixture(scope="module")
def near():
    return TN.twin_lib()


@pytest.fixture(scope="module")
def wtwin():
    return TW.twin_lib()


# ---- the checks, as lists of what is wrong (empty for the header as it is, not empty for its mutants) -----------------------
def within_pair(W, seg, pts, md, variants=((0, 1, 1), (0, 0, 0))):
    """the within twin in these variants -> a function i -> the list of point i (of the first variant), or None where the
    variants differ in any array"""
    first = TW.call_twin(W, seg, pts, md, *variants[0])
    rc, counts, off, eid, rec, dist, _ = first
    for o in [first] + [TW.call_twin(W, seg, pts, md, *v, capacity=counts[0]) for v in variants[1:]]:
        assert o[0] == TW.OK
        if o[1] != counts or not (np.array_equal(o[2], off) and np.array_equal(o[3], eid) and np.array_equal(o[4], rec) and np.array_equal(o[5], dist)):
            return None
    return lambda i: tuples_of(rec[int(off[i]):int(off[i + 1])])


def all_lists(W, seg, pts, md, variant):
    row = within_pair(W, seg, pts, md, (variant,))
    return [row(i) for i in range(len(pts))]


def family_failures(L, W, name, base, only=None):
    """every disagreement of a family's sets: twin (1, 1) against twin (0, 0), the sample against the definition"""
    ctx, seg, sets = DC.family_sets(name, base)
    edges = [tuple(e) for e in seg.tolist()]
    bad = []
    for k in sets:
        if only and k not in only:
            continue
        pts = DC.points_of(ctx, base, sets, k)
        a, da = TN.run_twin(L, seg, pts, -1, 1, 1, 1)   # (from the last eid down: at a tie the answer arrives after its rival)
        b, db = TN.run_twin(L, seg, pts, -1, 0, 0, 0)
        if a != b or not np.array_equal(da, db):
            bad.append((k, "nearest: pruned and filtered against the full brute force"))
        sub = pts[::STRIDE]
        pick = np.unique(np.linspace(0, len(sub) - 1, SAMPLE).astype(np.int64))
        tables = {int(i): DC.exact_table(int(sub[i][0]), int(sub[i][1]), edges) for i in pick}
        want = [DC.nearest_of(tables[int(i)]) for i in pick]
        if [a[STRIDE * int(i)] for i in pick] != want:
            bad.append((k, "nearest: the definition"))
        check_dist(want, da[STRIDE * pick])
        if W is None:
            continue
        for md in (0, DC.median_up(da), DC.LARGE[name]) + (DC.KNOT_DIST if k == "knot" else ()):
            row = within_pair(W, seg, sub, md)
            if row is None:
                bad.append((k, "within %d: pruned and filtered against the full brute force" % md))
            elif [row(int(i)) for i in pick] != [DC.within_of(tables[int(i)], md) for i in pick]:
                bad.append((k, "within %d: the definition" % md))
    return bad


@functools.lru_cache(maxsize=None)
def scene(kind, how):
    rng = np.random.default_rng(50 + SCENES.index((kind, how)))
    return DC.single_scene(kind, rng) if how == "single" else DC.replicated_scene(kind, rng)


@functools.lru_cache(maxsize=None)
def scene_tables(kind, how):
    sc = scene(kind, how)
    edges = NR.edges_of(sc.pts, sc.row)
    return {tuple(p): DC.exact_table(int(p[0]), int(p[1]), edges) for p in sc.points.tolist()}


def fan_failures(L, kind, how, variants=TN.VARIANTS):
    """the variants of the nearest twin in which a centre's answer is not the definition's"""
    sc = scene(kind, how)
    seg = TN.seg_array(NR.edges_of(sc.pts, sc.row))
    tables = scene_tables(kind, how)
    want = [DC.nearest_of(tables[tuple(p)]) for p in sc.points.tolist()]
    return [v for v in variants if TN.run_twin(L, seg, sc.points, -1, *v)[0] != want]


# ---- the families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", FAMILY_BASES, ids=["%s-%d" % fb for fb in FAMILY_BASES])
def test_family_twins_agree_and_equal_the_definition(near, wtwin, name, base):
    assert family_failures(near, wtwin, name, base) == []


# ---- the fans --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,how", SCENES, ids=["%s-%s" % s for s in SCENES])
def test_fans_nearest_is_the_definition_in_every_variant(near, kind, how):
    sc = scene(kind, how)
    assert len(sc.points) >= 64 and len(sc.row) - 1 > len(sc.fans) * 64
    assert fan_failures(near, kind, how) == []
    seg = TN.seg_array(NR.edges_of(sc.pts, sc.row))
    got, dist = TN.run_twin(near, seg, sc.points)
    check_dist(got, dist)
    tables = scene_tables(kind, how)
    for i, p in enumerate(sc.points.tolist()):
        fan, own = sc.fans[i % len(sc.fans)], sc.fan_eids[i % len(sc.fans)]
        assert tuple(p) == tuple(fan.P) and got[i][0] in own
        table, mine = tables[tuple(p)], set(own.tolist())
        d2 = [NR.d2_of(*table[int(e)][:3]) for e in own]
        # the condition on the inputs: the candidates are the centre's own fan, and no two of them can be ordered in double
        far = max(d2)
        assert all(t[3] * far.denominator > far.numerator * t[4] for e, t in enumerate(table) if e not in mine)
        assert DC.inseparable(d2)
        if kind == "equal":
            assert all(v == fan.m ** 2 for v in d2) and got[i][0] == own.min()
        else:
            assert len(set(d2)) == len(d2) and NR.d2_of(*got[i][1:]) == min(d2)
        if how == "single" and i:
            break   # (the same point again)


@pytest.mark.parametrize("kind,how", SCENES, ids=["%s-%s" % s for s in SCENES])
def test_fans_within_at_the_common_distance(wtwin, kind, how):
    """equal: m - 1 lists none, m and m + 1 list the whole fan of every centre, equality on the wide branch; tie: the fan's
    distance lies strictly between h and h + 1, so floor lists none and ceil all"""
    sc = scene(kind, how)
    seg = TN.seg_array(NR.edges_of(sc.pts, sc.row))
    tables = scene_tables(kind, how)
    pts = sc.points if how == "replicated" else sc.points[:2]
    fan = sc.fans[0]   # (the replicated fans share h, or m)
    m = fan.m or fan.h + 1
    for md, full in ((m - 1, False), (m, True), (m + 1, True)):
        want = [DC.within_of(tables[tuple(p)], md) for p in pts.tolist()]
        for i, row in enumerate(want):
            assert [t[0] for t in row] == (sc.fan_eids[i % len(sc.fans)].tolist() if full else [])
        for v in TW.VARIANTS:
            assert all_lists(wtwin, seg, pts, md, v) == want, (md, v)


# ---- the generators keep their properties ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", FAMILY_BASES, ids=["%s-%d" % fb for fb in FAMILY_BASES])
def test_point_sets_have_their_properties(near, name, base):
    ctx, seg, sets = DC.family_sets(name, base)
    bm, qm = ctx.maps[base], ctx.maps[1 - base]
    b, n = sets["vertices"]
    assert b > 0 and b % 64 != 0 and n > 64 and b + n <= qm.n_points
    assert (b + n == qm.n_points) == (name == DC.REACHES_LAST)
    for k, p in sets.items():
        if k != "vertices":
            assert p.dtype == np.int64 and p.shape[1] == 2 and 64 < len(p) <= 4096 and p.min() >= DC.LO and p.max() <= DC.HI
    # shuffled: the other map's vertices, not in the map's order
    own = set(map(tuple, qm.pts.tolist()))
    assert all(tuple(v) in own for v in sets["shuffled"].tolist())
    assert not np.array_equal(sets["shuffled"], qm.pts[:len(sets["shuffled"])])
    # border: both extremes of the range, all four corners, every point on a side of the domain
    p = sets["border"]
    assert {(DC.LO, DC.LO), (DC.LO, DC.HI), (DC.HI, DC.LO), (DC.HI, DC.HI)} <= set(map(tuple, p.tolist()))
    assert (np.isin(p[:, 0], (DC.LO, DC.HI)) | np.isin(p[:, 1], (DC.LO, DC.HI))).all()
    # on_base: at distance 0 (vertices) or below one unit (rounded midpoints); some vertices are shared by several chains
    got, dist = TN.run_twin(near, seg, sets["on_base"])
    half = len(sets["on_base"]) - len(sets["on_base"]) // 2
    assert (dist[:half] == 0).all() and (dist < 1).all()
    # random: most points are far from every edge (farther than a cell of the boxes)
    assert (TN.run_twin(near, seg, sets["random"])[1] > DC.CELL).mean() > 0.5
    assert ("knot" in sets) == (name == "outlier")
    assert ("along_long_edges" in sets) == (len(DC.long_edges(bm)) > 0)
    assert name not in ("long_long", "short_chains_frame") or "along_long_edges" in sets
    assert "along_long_edges" in sets or base not in ctx.skew["frame"]
    if "knot" in sets:
        x0, y0, x1, y1 = DC.knot_box(ctx, bm)
        assert len(DC.knot_edges(ctx, bm)) > 800 and max(x1 - x0, y1 - y0) <= 24   # (21 quanta and the jitter)
        q = S.quant(sets["knot"])
        g = DC.KNOT_GROW
        assert ((q[:, 0] >= x0 - g) & (q[:, 0] <= x1 + g) & (q[:, 1] >= y0 - g) & (q[:, 1] <= y1 + g)).all()
        assert ((q[:, 0] >= x0) & (q[:, 0] <= x1) & (q[:, 1] >= y0) & (q[:, 1] <= y1)).mean() > 0.5
    if "along_long_edges" in sets:
        got, dist = TN.run_twin(near, seg, sets["along_long_edges"])
        long_ones = set(DC.long_edges(bm).tolist())
        share = np.mean([t[0] in long_ones for t in got])
        assert share >= 0.9, share
        assert (dist > 0).mean() > 0.9 and np.median(dist) <= 6


def test_on_base_meets_shared_vertices(wtwin):
    """at a lattice's junctions several chains share the vertex: the definition lists them all at max_dist 0 and the nearest
    is the smallest eid"""
    ctx, seg, sets = DC.family_sets("skew_lattice", 0)
    edges = [tuple(e) for e in seg.tolist()]
    lists = all_lists(wtwin, seg, sets["on_base"], 0, (0, 1, 1))
    junctions = [i for i, row in enumerate(lists) if len(row) >= 3]
    assert len(junctions) >= 5, len(junctions)
    for i in junctions[:5]:
        x, y = sets["on_base"][i].tolist()
        t = DC.exact_table(x, y, edges)
        assert DC.within_of(t, 0) == lists[i] and DC.nearest_of(t) == lists[i][0]


# ---- the new inputs bite -----------------------------------------------------------------------------------------------------
MUTATIONS = {
    # the filter decides doubles that it cannot order (equal ones among them)
    "keep_above_one": ("constexpr double kKeep = 1.0 - 0x1p-48;", "constexpr double kKeep = 1.0 + 0x1p-48;"),
    # the carry of a.w[1] b1 into w[3] of the 320-bit product
    "mul3_carry": ("t = (t >> 64) + (p20 >> 64) + (p11 >> 64) + (uint64_t) p21;", "t = (t >> 64) + (p20 >> 64) + (uint64_t) p21;"),
    # the prune one cell too eager: the gap is the difference of the cell numbers, not one less
    "gap_g": ("return g > 1 ? (uint32_t) (g - 1) : 0u;", "return g > 0 ? (uint32_t) g : 0u;"),
}


def mutant(tag, tmp_path):
    old, new = MUTATIONS[tag]
    text = open(os.path.join(TN.CSRC, "rj_nearest.h")).read()
    assert text.count(old) == 1
    with open(tmp_path / "rj_nearest.h", "w") as f:
        f.write(text.replace(old, new))
    return TN.twin_lib(str(tmp_path), "_hetero_" + tag)


def test_mutant_filter_is_caught_by_the_tie_fan(near, tmp_path):
    L = mutant("keep_above_one", tmp_path)
    for how in ("single", "replicated"):
        assert fan_failures(near, "tie", how) == []
        assert fan_failures(L, "tie", how), "the mutant survives the %s tie fan" % how


def test_mutant_carry_is_caught_by_the_fans(near, tmp_path):
    L = mutant("mul3_carry", tmp_path)
    caught = [(kind, how) for kind, how in SCENES if fan_failures(L, kind, how)]
    assert ("tie", "single") in caught or ("equal", "single") in caught, caught
    assert any(how == "replicated" for _, how in caught), caught


def test_mutant_prune_is_caught_by_a_family(near, tmp_path):
    L = mutant("gap_g", tmp_path)
    sets = ("random", "border")
    assert family_failures(near, None, "skew_lattice", 0, only=sets) == []
    bad = family_failures(L, None, "skew_lattice", 0, only=sets)
    assert bad, "the mutant survives the random and the border points of skew_lattice"
