"""Raw ring sets for the polygon tests (tests/test_polygons.py, tests/test_gpu_polygons.py, tests/polygons_fuzz_more.py).
The definition of rayjoin_amd/csrc/rj_polygons.h is total: any ring records that pass the input check are valid, a planar
map is not needed.  So every generator here writes the three arrays of rj_map_rings directly -- rings as RING_DTYPE sorted
by ((uint32) face << 32) | leader, ring_row, ring_xy -- with area2 as the generator labels it (a two-point ring may be a
shell or a hole), and returns (rings, ring_row, ring_xy, info): info holds what the construction knows (the parents where it
gives them, the pieces the seed conditions of tests/test_polygons.py are asserted on).  Every generator is seeded or has
no randomness at all.

sliver_ceilings   ceiling edges whose height at a hole's top p is p.y + t / d with d near 2^45 and t in [-2, 5]: the two
                  products of candidate() are near 2^90 and differ by t; the order of two candidates is decided by the
                  fractional step of lower(); half of the edges fall (dy < 0): floor_div's negative branch
slope_fan         candidates of exactly equal height whose slopes differ by 1 / (dx_a dx_b) (Bezout neighbours), exact
                  duplicates and a collinear edge of double length (the slot decides), equal heights that are no integers
top_sweep         hole rings of 1 to 1000 points with the top at every lane position of the device's lane group, a
                  second point of equal y and smaller x, a decoy edge over every x but the top's
long_rings        a hole and a shell of 100 003 points: the top late in the ring, the winning edge deep in the ring
degenerate_records   walks of 40 steps that end at an orphan, rings without points of every kind and place, a one-point
                  ring, faces outside [0, 2^31)
carry_field       many polygons of area2 near 2^65 in three faces: the int128 prefix scan over several blocks
hole_field_answer the construction's polygons of polygons_cases.hole_field (any size)"""
import math
from fractions import Fraction

import numpy as np

import polygons_ref as PR
import rings_ref as D

LIM = 1 << 46
M64 = (1 << 64) - 1
NONE = PR.NONE
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def pack(items):
    """items [(face, leader, area2, [points])] -> (rings, ring_row, ring_xy, index): the records sorted by
    ((uint32) face << 32) | leader; index[k] = the ring that items[k] became"""
    keys = [((f & 0xFFFFFFFF) << 32) | le for f, le, _, _ in items]
    assert len(set(keys)) == len(keys) and all(0 <= le <= 0xFFFFFFFF for _, le, _, _ in items)
    order = sorted(range(len(items)), key=keys.__getitem__)
    rings = np.zeros(len(items), D.RING_DTYPE)
    index, row, pts = [0] * len(items), [0], []
    for r, k in enumerate(order):
        f, le, a2, p = items[k]
        rings[r] = (f, 0, le, 0, a2 & M64, a2 >> 64)
        index[k] = r
        pts.extend(p)
        row.append(len(pts))
    assert all(-LIM <= c < LIM for p in pts for c in p)
    return rings, np.array(row, np.uint32), np.array(pts, np.int64).reshape(-1, 2), index


def answer_from_parents(rings, parent):
    """the arrays and counts of rj_rings_polygons from the records and the parent of every ring (NONE: none): what
    polygons_ref derives from its walks, here from a construction's parents"""
    n = len(rings)
    parent = np.asarray(parent, np.uint32)
    face = rings["face"]
    a2 = D.area2_of(rings)
    r = np.arange(n, dtype=np.uint32)
    is_shell = parent == r
    shells = np.flatnonzero(is_shell)
    held = np.flatnonzero((parent != NONE) & ~is_shell)
    order = np.lexsort((np.concatenate([np.zeros(len(shells), np.int64), held.astype(np.int64) + 1]),
                        np.concatenate([shells, parent[held]]).astype(np.int64)))
    ring = np.concatenate([shells, held])[order].astype(np.uint32)
    starts = np.flatnonzero(is_shell[ring])
    first = np.concatenate([starts, [len(ring)]]).astype(np.uint32)
    members, bounds = ring.tolist(), first.tolist()
    totals = [sum(a2[m] for m in members[bounds[k]:bounds[k + 1]]) for k in range(len(shells))]
    polygons = np.zeros(len(shells), PR.POLYGON_DTYPE)
    polygons["face"], polygons["shell"], polygons["n_holes"] = face[shells], shells, np.diff(first.astype(np.int64)) - 1
    polygons["area2_lo"] = np.array([t & M64 for t in totals], np.uint64)
    polygons["area2_hi"] = np.array([t >> 64 for t in totals], np.int64)
    not0 = face != 0
    counts = dict(n_polygons=len(shells), n_members=len(ring), n_holes=len(held), n_orphans=int((not0 & (parent == NONE)).sum()),
                  n_face0=int((~not0).sum()))
    return dict(parent=parent, polygons=polygons, poly_first=first, poly_ring=ring, counts=counts)


def _parents(index, parent_item):
    """parent_item[k] = the item that is item k's parent (None: none) -> parent[] by ring"""
    parent = np.full(len(index), NONE, np.uint32)
    for k, p in enumerate(parent_item):
        if p is not None:
            parent[index[k]] = index[p]
    return parent


def _triangle(px, py):
    """a clockwise triangle with top (px, py): (points, area2)"""
    return [(px, py), (px + 1, py - 2), (px - 2, py - 3)], -7


# ---- slivers ---------------------------------------------------------------------------------------------------------
def sliver_edge(rng, px, py):
    """-> (u, v, t, d): a ceiling edge u -> v over p.x whose height there is p.y + t / d exactly: a = p.x - v.x and
    d = u.x - v.x coprime and near 2^45, dy a - e d = t with dy = t / a mod d (minus d half of the time) and e = p.y - v.y"""
    while True:
        a = int(rng.integers(1 << 40, 1 << 45))
        d = a + int(rng.integers(1 << 40, 1 << 45))
        if math.gcd(a, d) != 1:
            continue
        t = int(rng.integers(-2, 6))
        dy = t * pow(a, -1, d) % d
        if rng.random() < 0.5:
            dy -= d
        e, rest = divmod(dy * a - t, d)
        assert rest == 0
        v = (px - a, py - e)
        u = (v[0] + d, v[1] + dy)
        if all(-LIM <= c < LIM for c in u + v):
            return u, v, t, d


def sliver_ceilings(seed, n_holes=6, n_edges=80):
    """n_holes small triangles of face 1 close to each other, n_edges sliver edges over the top of each, every edge a
    two-point ring [u, v] of face 1, about 70 % of them labelled shell (area2 1) and the rest hole (area2 0): walks of
    several steps; leaders shuffled.  info: holes [(ring, p, [(u, v, t, d)])]"""
    rng = np.random.default_rng(seed)
    n = n_holes * (n_edges + 1)
    leaders = rng.permutation(n).tolist()
    items, holes = [], []
    for _ in range(n_holes):
        px, py = int(rng.integers(-(1 << 20), 1 << 20)), int(rng.integers(-(1 << 20), 1 << 20))
        pts, a2 = _triangle(px, py)
        edges = [sliver_edge(rng, px, py) for _ in range(n_edges)]
        holes.append((len(items), (px, py), edges))
        items.append((1, leaders[len(items)], a2, pts))
        for u, v, _, _ in edges:
            items.append((1, leaders[len(items)], 1 if rng.random() < 0.7 else 0, [u, v]))
    rings, row, xy, index = pack(items)
    return rings, row, xy, dict(holes=[(index[k], p, edges) for k, p, edges in holes])


# ---- slope fans --------------------------------------------------------------------------------------------------------
def bezout_neighbours(dx, dy, lo, hi):
    """every (dx', dy') with lo <= dx' < hi and dy dx' - dy' dx = +-1 (dx > 0 and dy coprime)"""
    out = []
    inv = pow(dy % dx, -1, dx)
    for s in (1, -1):
        x = s * inv % dx
        while x < hi:
            if x >= lo:
                assert (dy * x - s) % dx == 0
                out.append((x, (dy * x - s) // dx))
            x += dx
    return out


def bezout_chain(rng, n, sign, lo, hi, ok=lambda dx, dy: True):
    """n directions (dx, dy), lo <= dx < hi, dy of the given sign, consecutive ones Bezout neighbours: their slopes differ by
    1 / (dx_a dx_b), far below what a double resolves; ok(dx, dy) holds for each"""
    while True:
        dx = int(rng.integers(lo, hi))
        dy = sign * int(rng.integers(dx // 8, dx - dx // 8))
        if math.gcd(dx, dy) != 1 or not ok(dx, dy):
            continue
        chain = [(dx, dy)]
        while len(chain) < n:
            nxt = [c for c in bezout_neighbours(*chain[-1], lo, hi) if ok(*c) and c not in chain]
            if not nxt:
                break
            chain.append(nxt[int(rng.integers(0, len(nxt)))])
        if len(chain) == n:
            assert all(abs(a[1] * b[0] - b[1] * a[0]) == 1 for a, b in zip(chain, chain[1:])) and all(dy * sign > 0 for _, dy in chain)
            return chain


def slope_fan(seed, n_chain=12):
    """three holes, a face each (the fans reach over each other's rays).  Every fan edge is a two-point ring [u, v].
    A (face 1): top p, two chains (falling and rising) from the shared v = (p.x, p.y + 3): every edge has the height p.y + 3
      exactly, n = 0.  The steepest falling edge wins; it comes three times (the ring of the smallest slot wins) and once
      more with (2 dx, 2 dy): same height, same slope, the slot decides.
    B (face 2): a rising chain with even dx = 2 m and odd dy through the common point (p.x, p.y + 5 + 1/2): equal heights
      that are no integers, p.x strictly inside every edge; the winner comes twice.
    C (face 3): a chain (falling for even seeds) from V - (dx, dy) to V + (dx, dy), V = (p.x, p.y + 3): p.x strictly inside, the
      height an integer with n = dy dx not 0; the winner comes twice.
    The winners and their chain neighbours are shells; a fifth of the other edges are labelled hole.
    info: groups [dict(hole, p, height, edges [(item ring, u, v)], pairs [(a, b) positions in edges of chain neighbours], ties [rings of
    equal height and smallest slope], above)]"""
    rng = np.random.default_rng(seed)
    items, groups = [], []

    def add_group(face, p, height, edges, pairs):
        """edges [(u, v)] in chain order; the smallest slope, its copies and neighbours protected from the hole label"""
        slopes = [Fraction(u[1] - v[1], u[0] - v[0]) for u, v in edges]
        low = min(slopes)
        keep = {k for k, s in enumerate(slopes) if s == low}
        keep |= {b for a, b in pairs if a in keep} | {a for a, b in pairs if b in keep}
        pts, a2 = _triangle(*p)
        hole = len(items)
        items.append((face, 0, a2, pts))
        at = []
        for k, (u, v) in enumerate(edges):
            at.append(len(items))
            items.append((face, 0, 1 if k in keep or rng.random() < 0.8 else 0, [u, v]))
        groups.append(dict(hole=hole, p=p, height=height, edges=[(at[k], u, v) for k, (u, v) in enumerate(edges)], pairs=pairs,
                           ties=[at[k] for k, s in enumerate(slopes) if s == low]))

    def chain_pairs(lengths):
        out, base = [], 0
        for n in lengths:
            out += [(base + k, base + k + 1) for k in range(n - 1)]
            base += n
        return out

    # A: the far left of the range, so that v + 2 (dx, dy) stays inside it
    p = (-LIM + int(rng.integers(16, 1 << 20)), int(rng.integers(-(1 << 20), 1 << 20)))
    v = (p[0], p[1] + 3)
    falling, rising = bezout_chain(rng, n_chain, -1, 1 << 40, 1 << 45), bezout_chain(rng, n_chain, 1, 1 << 40, 1 << 45)
    edges = [((v[0] + dx, v[1] + dy), v) for dx, dy in falling + rising]
    wdx, wdy = min(falling, key=lambda c: Fraction(c[1], c[0]))
    edges += [((v[0] + wdx, v[1] + wdy), v)] * 2 + [((v[0] + 2 * wdx, v[1] + 2 * wdy), v)]
    add_group(1, p, Fraction(v[1]), edges, chain_pairs([n_chain, n_chain]))
    # B: through (p.x, w + 1/2)
    p = (int(rng.integers(-(1 << 20), 1 << 20)), int(rng.integers(-(1 << 20), 1 << 20)))
    w = p[1] + 5
    half = bezout_chain(rng, n_chain, 1, 1 << 39, 1 << 44, ok=lambda m, dy: dy % 2 == 1)
    edges = []
    for m, dy in half:
        v = (p[0] - m, w + (1 - dy) // 2)
        edges.append(((v[0] + 2 * m, v[1] + dy), v))
    edges.append(min(edges, key=lambda e: Fraction(e[0][1] - e[1][1], e[0][0] - e[1][0])))
    add_group(2, p, Fraction(2 * w + 1, 2), edges, chain_pairs([n_chain]))
    # C: through the integer point V, p.x strictly inside
    p = (int(rng.integers(-(1 << 20), 1 << 20)), int(rng.integers(-(1 << 20), 1 << 20)))
    V = (p[0], p[1] + 3)
    through = bezout_chain(rng, n_chain, -1 if seed % 2 == 0 else 1, 1 << 40, 1 << 45)
    edges = [((V[0] + dx, V[1] + dy), (V[0] - dx, V[1] - dy)) for dx, dy in through]
    edges.append(min(edges, key=lambda e: Fraction(e[0][1] - e[1][1], e[0][0] - e[1][0])))
    add_group(3, p, Fraction(V[1]), edges, chain_pairs([n_chain]))
    leaders = rng.permutation(len(items)).tolist()
    rings, row, xy, index = pack([(f, leaders[k], a2, pts) for k, (f, _, a2, pts) in enumerate(items)])
    for g in groups:
        g["hole"] = index[g["hole"]]
        g["edges"] = [(index[k], u, v) for k, u, v in g["edges"]]
        g["ties"] = sorted(index[k] for k in g["ties"])
        g["above"] = g["ties"][0]  # u is a ring's first point: the smallest slot is the smallest ring
    return rings, row, xy, dict(groups=groups)


# ---- tops ----------------------------------------------------------------------------------------------------------------
TOP_SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 1000)
TOP_AT_1000 = (0, 3, 7, 500, 501, 502, 506, 993, 999)


def top_sweep(seed=0):
    """hole rings of n points for n in TOP_SIZES, the top at every index (TOP_AT_1000 for 1000), a column of 64 units each,
    under one shell over the whole range of y; the tops at three levels, two of them 200 units from -2^46 and 2^46.  With
    the top (X, Y): a second point (X - 10, Y) at an index of another lane position (index mod 8), every other point in
    [X - 20, X - 1] x [Y - 50, Y - 1]; the decoy, a two-point shell (X, Y + 2) -> (X - 20, Y + 1), covers every x of the ring
    but X.  A ring whose top comes out as any other point has the decoy above it, not the shell.
    info: parent (every hole: the shell), holes [(ring, n, index of the top, index of the equal-y point or None)]"""
    rng = np.random.default_rng(seed)
    cases = [(n, t) for n in TOP_SIZES for t in (range(n) if n <= 17 else TOP_AT_1000)]
    x1 = 64 * len(cases) + 100
    items = [(1, 0, 2 * (x1 + 100) * (2 * LIM - 1), [(-100, -LIM), (x1, -LIM), (x1, LIM - 1), (-100, LIM - 1)])]
    parent_item, holes = [0], []
    for c, (n, t) in enumerate(cases):
        X, Y = 64 * c + 40, (-LIM + 200, int(rng.integers(-1000, 1000)), LIM - 200)[c % 3]
        pts = [(X - int(rng.integers(1, 21)), Y - int(rng.integers(1, 51))) for _ in range(n)]
        pts[t] = (X, Y)
        twin = None
        if n >= 2:
            twin = next(i for i in ((t + off) % n for off in range(1 + c % 5, n + 5)) if i != t and i % 8 != t % 8)
            pts[twin] = (X - 10, Y)
        holes.append((len(items), n, t, twin))
        items.append((1, 0, -1, pts))
        parent_item.append(0)
        items.append((1, 0, 1, [(X, Y + 2), (X - 20, Y + 1)]))
        parent_item.append(len(items) - 1)
    leaders = rng.permutation(len(items)).tolist()
    rings, row, xy, index = pack([(f, leaders[k], a2, pts) for k, (f, _, a2, pts) in enumerate(items)])
    return rings, row, xy, dict(parent=_parents(index, parent_item), holes=[(index[k], n, t, twin) for k, n, t, twin in holes])


LONG = 100_003


def long_rings():
    """ring by leader: 0 a hole of LONG points, point i at (LONG - i, 7919 i mod 1000) but for its top (12, 5000) at index
    LONG - 12; 1 a shell of LONG points that runs from x = LONG + 10 down to x = 12 at heights 20000 to 20006 and closes
    through (-50, -100000): the one edge over x = 12 starts at its point LONG - 3; 2 a decoy shell with a ceiling at 20010;
    3, 4 two-point shells at height 10000 over every x of the hole but 12 (a wrong top meets one of them).
    info: parent"""
    n = LONG
    hole = [(n - i, 7919 * i % 1000) for i in range(n)]
    hole[n - 12] = (12, 5000)
    shell = [(n + 10 - j, 20000 + 31 * j % 7) for j in range(n - 1)] + [(-50, -100000)]
    assert shell[n - 2][0] == 12 and shell[n - 3][0] == 13
    area2 = sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(shell, shell[1:] + shell[:1]))
    assert area2 > 0
    items = [(1, 0, -1, hole), (1, 1, area2, shell), (1, 2, 120, [(0, 20008), (30, 20008), (30, 20010), (0, 20010)]),
             (1, 3, 1, [(12, 10000), (-10, 10000)]), (1, 4, 1, [(n + 20, 10000), (13, 10000)])]
    rings, row, xy, index = pack(items)
    return rings, row, xy, dict(parent=_parents(index, [1, 1, 2, 3, 4]))


# ---- degenerate records ----------------------------------------------------------------------------------------------------
COLUMN = 40
DEGENERATE_FACES = ((1, 2), (-5, INT32_MIN), (INT32_MAX, -1))
DEGENERATE_COUNTS = dict(n_polygons=3, n_members=44, n_holes=41, n_orphans=44, n_face0=3)


def degenerate_records(faces):
    """faces (fa, fb).  A column of COLUMN clockwise squares of face fa, square j at [j, j + 4] x [10 j + 2, 10 j + 6] under
    the bottom edge of square j + 1, and no shell: COLUMN orphans, the walk of the lowest has COLUMN - 1 steps.  The same
    column of face fb 1000 units to the right inside a shell of face fb, and a one-point ring beside it: COLUMN + 1 holes.
    Rings without points for face 0, fa, fb and area2 0, 5, -5, their leaders 0, 255 and 2^32 - 1: the first, a middle
    and the last ring of their face (the rings with points have leaders 100 to 149); three of face 0, two shells, four orphans.
    info: parent, column (the rings of the orphan column, lowest first)"""
    fa, fb = faces
    items, parent_item = [], []

    def square(face, leader, x, j):
        x0, y0 = x + j, 10 * j + 2
        items.append((face, leader, -32, [(x0, y0), (x0, y0 + 4), (x0 + 4, y0 + 4), (x0 + 4, y0)]))

    order = np.random.default_rng(COLUMN).permutation(COLUMN).tolist()
    for j in range(COLUMN):
        square(fa, 100 + order[j], 0, j)
        parent_item.append(None)
    shell = len(items)
    items.append((fb, 149, 2 * 70 * 430, [(990, -10), (1060, -10), (1060, 420), (990, 420)]))
    parent_item.append(shell)
    for j in range(COLUMN):
        square(fb, 100 + order[j], 1000, j)
        parent_item.append(shell)
    items.append((fb, 148, 0, [(1050, 0)]))
    parent_item.append(shell)
    for face in (0, fa, fb):
        for a2, leader in ((0, 0), (5, 255), (-5, 0xFFFFFFFF)):
            items.append((face, leader, a2, []))
            parent_item.append(len(items) - 1 if face != 0 and a2 > 0 else None)
    rings, row, xy, index = pack(items)
    return rings, row, xy, dict(parent=_parents(index, parent_item), column=[index[j] for j in range(COLUMN)])


# ---- carries -----------------------------------------------------------------------------------------------------------------
def carry_field(n, salt=0):
    """n squares of side 2^32 (area2 2^65) at a pitch of 2^33 from (-2^46, -2^46), 2^14 to a row, faces 1, 2, 3 in turn,
    leaders 2 k; in each one clockwise hole of 2^32 - 2 by 2^32 - 3 units, area2 -2 (2^32 - 2)(2^32 - 3), leader 2 k + 1.
    salt != 0: the recorded area2 of shell k has the low word (k + 1) salt 0x9E3779B97F4A7C15 mod 2^64 added -- the
    definition takes area2 as it stands -- so that the low words of the prefix carry into the high ones at about every
    second member.  info: parent, areas (the members' area2 in member order)"""
    S, cols = 1 << 32, 1 << 14
    k = np.arange(n, dtype=np.int64)
    x0, y0 = -LIM + (k % cols) * (2 * S), -LIM + (k // cols) * (2 * S)
    assert n <= cols * cols and int(x0.max()) + S < LIM and int(y0.max()) + S < LIM
    corners = lambda xa, ya, xb, yb, cw: np.stack([np.stack(c, 1) for c in (((xa, ya), (xa, yb), (xb, yb), (xb, ya)) if cw else
                                                                            ((xa, ya), (xb, ya), (xb, yb), (xa, yb)))], 1)  # noqa: E731
    pts = np.stack([corners(x0, y0, x0 + S, y0 + S, False), corners(x0 + 1, y0 + 1, x0 + S - 1, y0 + S - 2, True)], 1)  # [n, 2, 4, 2]
    face = np.repeat(k % 3 + 1, 2)
    leader = np.arange(2 * n, dtype=np.int64)
    order = np.lexsort((leader, face))  # ring r is record order[r]: shell k is record 2 k, its hole 2 k + 1
    at = np.empty(2 * n, np.int64)
    at[order] = np.arange(2 * n)
    hole_a2 = -2 * (S - 2) * (S - 3)
    a2 = []
    for i in range(n):
        a2 += [(1 << 65) + ((i + 1) * salt * 0x9E3779B97F4A7C15 & M64), hole_a2]
    rings = np.zeros(2 * n, D.RING_DTYPE)
    rings["face"], rings["leader"] = face[order], leader[order]
    rings["area2_lo"] = np.array([a2[i] & M64 for i in order.tolist()], np.uint64)
    rings["area2_hi"] = np.array([a2[i] >> 64 for i in order.tolist()], np.int64)
    xy = pts.reshape(2 * n, 4, 2)[order].reshape(-1, 2)
    row = (4 * np.arange(2 * n + 1)).astype(np.uint32)
    parent = at[2 * (order // 2)].astype(np.uint32)
    members = np.lexsort((np.arange(2 * n), parent))  # shell, hole, shell, hole: a hole's ring follows its shell's
    return rings, row, np.ascontiguousarray(xy), dict(parent=parent, areas=[a2[int(order[m])] for m in members.tolist()])


# ---- the hole field ------------------------------------------------------------------------------------------------------------
def hole_field_answer(rings, n):
    """polygons_cases.hole_field with n holes: ring 0 the outside, 1 the shell of face 1, 2 .. n + 1 its holes, then the
    n shells of face 2 -> the construction's polygons"""
    assert len(rings) == 2 * n + 2 and rings["face"].tolist() == [0, 1] + [1] * n + [2] * n
    parent = np.concatenate([[NONE, 1], np.ones(n, np.int64), np.arange(n + 2, 2 * n + 2)]).astype(np.uint32)
    return answer_from_parents(rings, parent)
