"""Input families for the overlay where the four fixed pairs of tests/test_overlay_map.py say nothing (test
infrastructure): cuts that coincide along an edge, edges with tens of cuts, maps whose edge counts and chain ends sit on
the 64-edge wave boundaries of the device kernels, face ids next to 2^31 and coordinates at the corners of the scaled
range.  One function per family returning (ctx, gsize); preconditions(oracle, ctx, gsize) asserts FROM THE ORACLE'S
RECORDS ALONE that the pair has the property it is there for, so a generator change that loses the ties or the long
runs fails on the CPU.

Every family stays inside the predicate domain.  The reference computes intersection points with rational<__int128>
whose numerators reach about 2^(48 + 2 L) for edges of length 2^L; they wrap for edges longer than roughly 1/200 of
the scaled range, and this project reproduces that arithmetic "modulo 2^128" (rayjoin_amd/csrc/rj_predicates.h).  Seen
with the oracle: lattice_map(2, 1, 5) x lattice_map(10, 3, 6) has 53 brute-force pairs of which the grid finds 0,
lattice_map(3, 1) x lattice_map(40, 3) 312 against 4-5.  So many cuts per edge cannot be had from long edges: they
come from a fine map in a window of a few cells of a coarse one, under one hand-set Scaling, and preconditions()
asserts for every pair that no edge is longer than MAX_EDGE (1/256 of the scaled range) in x or in y."""
import numpy as np

from rayjoin_amd import maps, synth

import overlay_faces_ref as F
import overlay_ops_ref as R

MAX_EDGE = maps.INTERNAL_RANGE // 256
TIES_SEEDS = (0, 1, 2, 3)
BIG = (1 << 31) - 60
CORNER = ((1 << 46) - 1 - 40, -(1 << 46) + 40)


def _context(m0, m1, **what):
    """two scaled maps under ONE hand-set Scaling (the one of synth.US_BBOX: the areas in input units need one)"""
    ctx = maps.Context([None, None])
    ctx.scaling = maps.Scaling(synth.US_BBOX)
    ctx.set_map(0, m0)
    ctx.set_map(1, m1)
    ctx.hard = what
    return ctx


# ---- ties: integer chains on a tiny lattice ---------------------------------------------------------------------------------
def ties(seed, shift=(0, 0), face_base=0, family="ties"):
    """adversarial_chains(60, 9, 12, 21 + seed) x adversarial_chains(80, 5, 12, 40 + seed): steps of at most 3 units
    on a lattice of +-12: hundreds of cuts at shared vertices, many of them the same point on the same edge"""
    ms = []
    for im, args in enumerate(((60, 9, 12, 21 + seed), (80, 5, 12, 40 + seed))):
        pts, row, left, right = synth.adversarial_chains(*args)
        pts = pts + np.array(shift, dtype=np.int64)
        left, right = (np.where(f != 0, f + face_base, 0) for f in (left, right))
        ms.append(maps.ScaledMap(im, pts, row, left, right))
    return _context(ms[0], ms[1], family=family, seed=seed), 64


def ties_corner(seed=0):
    """the same chains next to the (+2^46 - 1, -2^46) corner of the scaled range: carries and borrows between the
    two limbs of the areas, negated products on the right side"""
    return ties(seed, shift=CORNER, family="ties_corner")


def big_ids(seed=0):
    """every nonzero face id f (below 50) replaced by 2^31 - 60 + f: the largest is 2^31 - 11"""
    return ties(seed, face_base=BIG, family="big_ids")


# ---- many cuts on one edge ---------------------------------------------------------------------------------------------------
MANY = {"a": (512, 48, 2, 3), "b": (600, 64, 1, 2)}  # G of map 0, (G, k) of map 1, window width in cells of map 0


def many_cuts(which="a"):
    """map 0 = lattice_map(G0, 1, 5) over US_BBOX, map 1 = a lattice of G1 x G1 cells in a window a few cells of map 0
    wide at 40 % of the box: every edge of map 0 that crosses the window is cut by tens of lines of map 1.  Map 0 is
    reduced to the chains within 4 cells of the window (the Python walk over all its uncut edges is the cost).  G0 is
    512 / 600: the one-segment chains of lattice_map(256, 1) reach 1/173 of the scaled range with their vertex jitter,
    those of G0 = 512 1/335 (the counts seen: 380 and 322 intersections, longest runs 27 and 46)"""
    G0, G1, k1, wide = MANY[which]
    x0, y0, x1, y1 = synth.US_BBOX
    cw, ch = (x1 - x0) / G0, (y1 - y0) / G0
    wx, wy = x0 + 0.4 * (x1 - x0), y0 + 0.4 * (y1 - y0)
    window = (wx, wy, wx + wide * cw, wy + wide * ch)
    g0, g1 = synth.lattice_map(G0, 1, 5), synth.lattice_map(G1, k1, 6, bbox=window)
    margin = 4
    lo = g0.points[g0.row_index[:-1].astype(np.int64)]
    hi = g0.points[g0.row_index[1:].astype(np.int64) - 1]
    near = ((np.minimum(lo[:, 0], hi[:, 0]) > window[0] - margin * cw) & (np.maximum(lo[:, 0], hi[:, 0]) < window[2] + margin * cw)
            & (np.minimum(lo[:, 1], hi[:, 1]) > window[1] - margin * ch) & (np.maximum(lo[:, 1], hi[:, 1]) < window[3] + margin * ch))
    g0 = keep_chains(g0, np.flatnonzero(near))
    sc = maps.Scaling(synth.US_BBOX)
    ctx = _context(scaled(sc, 0, g0), scaled(sc, 1, g1), family="many_cuts", which=which)
    ctx.scaling = sc
    return ctx, 2048


def scaled(sc, im, g):
    return maps.ScaledMap(im, sc.scale(g.points), g.row_index, g.chains[:, 3], g.chains[:, 4])


def keep_chains(g, which):
    """the planar graph of the chains `which` (ascending), points repacked"""
    row = g.row_index.astype(np.int64)
    idx = np.concatenate([np.arange(row[c], row[c + 1]) for c in which])
    new_row = np.r_[0, np.cumsum(row[which + 1] - row[which])]
    chains = g.chains[which].copy()
    chains[:, 0] = np.arange(len(which))
    chains[:, 1], chains[:, 2] = new_row[:-1], new_row[1:] - 1
    return maps.PlanarGraph(chains, new_row.astype(np.uint32), g.points[idx])


def trimmed(g, n_edges):
    """g cut down to n_edges edges: whole chains dropped from the end, then the last chain shortened"""
    row = g.row_index.astype(np.int64)
    edges_to = row - np.arange(len(row))  # edges before chain c
    nc = int(np.searchsorted(edges_to, n_edges, side="left"))  # chains 0 .. nc - 1 hold at least n_edges
    assert 0 < nc <= g.n_chains and edges_to[nc] >= n_edges
    g = keep_chains(g, np.arange(nc))
    cut = int(edges_to[nc] - n_edges)
    assert g.row_index[-1] - g.row_index[-2] - cut >= 2
    if cut:
        row = g.row_index.copy()
        row[-1] -= cut
        chains = g.chains.copy()
        chains[-1, 2] -= cut
        g = maps.PlanarGraph(chains, row, g.points[:int(row[-1])])
    return g


# ---- wave geometry -----------------------------------------------------------------------------------------------------------
def _window(frac=0.02, at=0.4):
    x0, y0, x1, y1 = synth.US_BBOX
    return (x0 + at * (x1 - x0), y0 + at * (y1 - y0), x0 + (at + frac) * (x1 - x0), y0 + (at + frac) * (y1 - y0))


def _ring(n, bbox, seed, face):
    """one closed chain of n edges around the centre of bbox (star-shaped, so simple), face on its left"""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = bbox
    ang = 2 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    r = 0.5 * (1.0 + 0.2 * np.cos(5 * ang + 1.0) + rng.uniform(-0.02, 0.02, n)) / 1.25
    pts = np.stack([0.5 * (x0 + x1) + r * np.cos(ang) * 0.5 * (x1 - x0), 0.5 * (y0 + y1) + r * np.sin(ang) * 0.5 * (y1 - y0)], 1)
    pts = np.concatenate([pts, pts[:1]])
    return maps.PlanarGraph(np.array([[0, 0, n, face, 0]], np.int64), np.array([0, n + 1], np.uint32), pts)


WAVES = ("63x65", "64x128", "321x40", "ring1000", "193x64")


def waves(which):
    """small maps in a window of 2 % of the box whose edge counts and chain ends sit on the device's 64-edge waves.
    ctx.hard holds what preconditions() asserts: n_edges of both maps, an edge 64 j - 1 a chain must end on, and for
    the ring that it stays uncut."""
    W = _window()
    L = synth.lattice_map
    want = dict(family="waves", which=which, uncut_ring=False, chain_end=None, single=None)
    if which == "63x65":      # 4 chains of 16 with the last one short; 12 chains of 6 less one chain and one edge
        g0, g1 = trimmed(L(1, 16, 91, bbox=W), 63), trimmed(L(2, 6, 92, bbox=W), 65)
        want.update(n_edges=(63, 65))
    elif which == "64x128":   # chains end on edges 15, 31, 47, 63; and 31, 63, 95, 127
        g0, g1 = L(1, 16, 93, bbox=W), L(1, 32, 94, bbox=W)
        want.update(n_edges=(64, 128), chain_end=63)
    elif which == "321x40":   # 64 * 5 + 1 edges in chains of 27; map 1 is ONE chain of 40 edges across the window
        g0 = trimmed(L(2, 27, 95, bbox=W), 321)
        g1 = keep_chains(L(1, 40, 96, bbox=(W[0] - 0.1 * (W[2] - W[0]), W[1] + 0.45 * (W[3] - W[1]), W[2] + 0.1 * (W[2] - W[0]), W[3])),
                         np.array([0]))
        want.update(n_edges=(321, 40), single=1)
    elif which == "ring1000":  # a closed ring of 1000 edges inside ONE face of map 1: no record, 16 waves without a reset
        g1 = L(2, 8, 97, bbox=W, vertex_jitter=0.1)
        cw, ch = (W[2] - W[0]) / 2, (W[3] - W[1]) / 2
        g0 = _ring(1000, (W[0] + 0.25 * cw, W[1] + 0.25 * ch, W[0] + 0.75 * cw, W[1] + 0.75 * ch), 98, face=7)
        want.update(n_edges=(1000, 96), uncut_ring=True, single=0)
    elif which == "193x64":   # 64 * 3 + 1 edges; map 1's chains of 8 edges end on 63 with a cut map 0 around it
        g0, g1 = trimmed(L(3, 9, 99, bbox=W), 193), trimmed(L(2, 8, 100, bbox=W), 64)
        want.update(n_edges=(193, 64), chain_end=63)
    else:
        raise KeyError(which)
    sc = maps.Scaling(synth.US_BBOX)
    ctx = _context(scaled(sc, 0, g0), scaled(sc, 1, g1), **want)
    return ctx, 256


# ---- every family, by name ---------------------------------------------------------------------------------------------------
FAMILIES = ([("ties-%d" % s, lambda s=s: ties(s)) for s in TIES_SEEDS] + [("ties_corner", ties_corner), ("big_ids", big_ids)]
            + [("many_cuts-%s" % w, lambda w=w: many_cuts(w)) for w in sorted(MANY)]
            + [("waves-%s" % w, lambda w=w: waves(w)) for w in WAVES])
NAMES = [n for n, _ in FAMILIES]


def family(name):
    return dict(FAMILIES)[name]()


def same_face_chains(ctx):
    """does a chain have the SAME nonzero face on both sides?  (The random faces of the tie families: about one chain in
    fifty.)  The calls without _op keep such a chain's pieces, adding +v and -v to one row; (intersection, pair)
    through the _op calls drops them (rayjoin_amd/csrc/rj_overlay_ops.h): only on the other pairs are the two the same"""
    return any(bool(((m.left == m.right) & (m.left != 0)).any()) for m in ctx.maps)


def assert_rows_without_op(ctx, old_rows, op_rows):
    """the rows of the call without _op against those of (intersection, pair): equal, or with same_face_chains() the
    same rows plus rows of area 0 that only such chains touch"""
    if not same_face_chains(ctx):
        assert old_rows == op_rows
        return
    old = {r[:2]: r[2] for r in old_rows}
    assert len(old) == len(old_rows) and all(old.get(r[:2]) == r[2] for r in op_rows)
    assert all(v == 0 for k, v in old.items() if k not in {r[:2] for r in op_rows})


def oracle_maps(oracle, ctx):
    return [oracle.Map(m.pts, m.row_index, m.left, m.right) for m in ctx.maps]


def run_lengths(xs, im):
    """lengths of the runs of records of one edge of map im"""
    eid = xs[im]["eid"][:, im]
    if not len(eid):
        return np.zeros(0, np.int64)
    return np.diff(np.flatnonzero(np.r_[True, eid[1:] != eid[:-1], True]))


def coincident(xs, im):
    """consecutive records of map im that are the same point on the same edge"""
    x = xs[im]
    if len(x) < 2:
        return 0
    return int(((x["eid"][1:, im] == x["eid"][:-1, im]) & (x["x_num"][1:] == x["x_num"][:-1]) & (x["y_num"][1:] == x["y_num"][:-1])).sum())


def mid_points(xs, im):
    """the mid-points the record stage locates: trunc((p + q) / 2) of consecutive records of one edge"""
    x = xs[im]
    if len(x) < 2:
        return np.zeros((0, 2), np.int64)
    same = x["eid"][1:, im] == x["eid"][:-1, im]

    def half(a):
        s = a[1:][same] + a[:-1][same]  # (|coordinate| <= 2^46: no overflow)
        return np.where(s >= 0, s // 2, -((-s) // 2))

    return np.stack([half(x["x_num"]), half(x["y_num"])], 1)


def preconditions(oracle, ctx, gsize):
    """-> (xs, pip, pairs by brute force): the oracle pipeline's records of the pair (as overlay_faces_ref.oracle_records)
    after asserting what the family is there for"""
    what = ctx.hard
    fam = what["family"]
    m = ctx.maps
    for x in m:
        assert x.pts.min() >= maps.INTERNAL_MIN and x.pts.max() <= maps.INTERNAL_MAX
        p1 = x.edge_p1().astype(np.int64)
        assert np.abs(x.pts[p1 + 1] - x.pts[p1]).max() <= MAX_EDGE, fam
        assert np.all(np.diff(x.row_index.astype(np.int64)) >= 2)
    om = oracle_maps(oracle, ctx)
    brute = oracle.lsi_brute(om[0], om[1])
    xs, pip = F.oracle_records(oracle, ctx, gsize)
    grid = oracle.lsi_grid(om[0], om[1], gsize)["eid"]
    assert np.array_equal(grid, brute), (fam, len(grid), len(brute))
    for im in range(2):  # the vertex faces and the mid-point faces do not hang on the grid
        assert np.array_equal(pip[im], om[1 - im].face_ids(oracle.pip_brute(om[1 - im], im, m[im].pts)))
        mids = mid_points(xs, im)
        if len(mids):
            assert np.array_equal(oracle.pip_grid(om[1 - im], 1 - im, mids, gsize), oracle.pip_brute(om[1 - im], im, mids)), (fam, im)
    if fam in ("ties", "ties_corner", "big_ids"):
        for im in range(2):
            assert coincident(xs, im) >= 100, (fam, im, coincident(xs, im))
            assert run_lengths(xs, im).max() >= 8
        assert len(brute) >= 500
        assert R.output_map(R.all_pieces(m, xs, pip), "union", "pair")["n_one_point"] >= 500
    if fam == "ties_corner":
        assert all(x.pts[:, 0].min() > (1 << 46) - 200 and x.pts[:, 1].max() < -(1 << 46) + 200 for x in m)
    if fam == "big_ids":
        for x in m:
            assert int(((x.left >= BIG) & (x.right >= BIG)).sum()) >= 1 and max(x.left.max(), x.right.max()) < 1 << 31
    if fam == "many_cuts":
        assert len(brute) >= 200 and run_lengths(xs, 0).max() >= 16, (len(brute), run_lengths(xs, 0).max())
    if fam == "waves":
        assert (m[0].n_edges, m[1].n_edges) == what["n_edges"]
        if what["chain_end"] is not None:
            j = what["chain_end"]
            assert j % 64 == 63 and any(j + 1 in (x.row_index[1:].astype(np.int64) - np.arange(1, x.n_chains + 1)).tolist() for x in m)
        if what["single"] is not None:
            assert m[what["single"]].n_chains == 1
        if what["uncut_ring"]:
            assert len(brute) == 0 and m[0].n_edges >= 15 * 64 and m[0].n_chains == 1
            assert np.all(pip[0] == pip[0][0]) and pip[0][0] != 0
        else:
            assert len(brute) >= 4
    return xs, pip, brute
