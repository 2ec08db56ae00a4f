"""Inputs for the two distance queries (rj_nearest_query, rj_within_query) that the uniform lattices and ring maps of their
own suites never give (test infrastructure, not collected by pytest): point sets over the heterogeneous families of
tests/skewed_pairs.py, and two fans of edges around a point whose distances a double cannot order (tie_fan) or that are
equal as rationals with different limbs (equal_fan), alone at full scale and replicated at 72 centres inside a map of two
tree levels.  tests/test_distance_hetero.py holds the host twins to the Python definition on them and asserts each
generator's property from the integers alone; tests/test_gpu_distance_hetero.py holds the device to the twins.

Everything is in the library's scaled int64 coordinates, [-2^46, 2^46)."""
import collections
from fractions import Fraction

import numpy as np

from rayjoin_amd import maps, synth

import nearest_ref as NR
import skewed_pairs as S

LO, HI = maps.INTERNAL_MIN, maps.INTERNAL_MAX   # -2^46, 2^46 - 1
CELL = 1 << S.QUANT_SHIFT
N_POINTS = 1024            # points of a set at most (the twins are brute forces over up to 50 000 edges)
REACHES_LAST = "thin_band"  # the family whose `vertices` range ends at the query map's last vertex
KNOT_GROW = 1              # cells around the knot's quantised box that `knot` points may lie in
FILTER_KEEP = 1 - Fraction(1, 1 << 48)   # closer()'s kKeep: doubles nearer to each other than this go to the wide compare


# ---- point sets of a family ------------------------------------------------------------------------------------------------
def long_edges(m):
    """eids of the edges longer than 1/256 of the range (the frames, long_long's domain-long segments, outlier's coarse
    lattice)"""
    s = m.segments()
    return np.flatnonzero(np.maximum(np.abs(s[:, 2] - s[:, 0]), np.abs(s[:, 3] - s[:, 1])) > S.MAX_EDGE)


def knot_edges(ctx, m):
    """eids of the knot of an `outlier` map: the edges inside the knot's box (restated from skewed_pairs.outlier through
    the family's own `tiny` box) with the lattice's jitter around it"""
    t = ctx.skew["tiny"]
    w, side = t[2] - t[0], S.KNOT * (S.DOMAIN[2] - S.DOMAIN[0])
    x0, y0 = t[0] + 1.6 * w, t[1] + 0.5 * (t[3] - t[1])
    (sx0, sy0), (sx1, sy1) = ctx.scaling.scale(np.array([[x0 - side, y0 - side], [x0 + 2 * side, y0 + 2 * side]]))
    s = m.segments()
    inside = (s[:, [0, 2]].min(1) >= sx0) & (s[:, [0, 2]].max(1) <= sx1) & (s[:, [1, 3]].min(1) >= sy0) & (s[:, [1, 3]].max(1) <= sy1)
    return np.flatnonzero(inside)


def knot_box(ctx, m):
    """the knot's quantised box (x0, y0, x1, y1), cells inclusive"""
    s = S.quant(m.segments()[knot_edges(ctx, m)])
    return int(s[:, [0, 2]].min()), int(s[:, [1, 3]].min()), int(s[:, [0, 2]].max()), int(s[:, [1, 3]].max())


def vertex_range(name, n_query, n, rng):
    """(b, n) with b > 0 and b % 64 != 0; in REACHES_LAST it ends at the last vertex"""
    n = min(n, n_query - 130)
    b = n_query - n if name == REACHES_LAST else int(rng.integers(65, n_query - n - 1))
    if b % 64 == 0:
        b, n = b + 1, n - (name == REACHES_LAST)
    assert 0 < b and b % 64 and b + n <= n_query and n > 64
    return b, n


def along(seg, rng, per_edge):
    """points a few units to the left and right of the interiors of these edges, and past their ends"""
    out = []
    for ax, ay, bx, by in seg.tolist():
        dx, dy = bx - ax, by - ay
        ln = max(abs(dx), abs(dy))
        for _ in range(per_edge):
            t, off = int(rng.integers(ln // 50, ln - ln // 50)), int(rng.integers(1, 6)) * (1 if rng.integers(0, 2) else -1)
            x, y = ax + dx * t // ln, ay + dy * t // ln
            # the unit normal's larger component is the one across the edge's longer axis: `off` units that way
            out.append((x, y + off) if abs(dx) >= abs(dy) else (x + off, y))
        for sx, sy, ex, ey in ((ax, ay, -dx, -dy), (bx, by, dx, dy)):   # past the ends, along the edge and a little beside it
            for _ in range(max(1, per_edge // 16)):
                t = int(rng.integers(1, 1 << 20))
                out.append((sx + ex * t // ln + int(rng.integers(-5, 6)), sy + ey * t // ln + int(rng.integers(-5, 6))))
    return np.clip(np.array(out, np.int64), LO, HI)


def point_sets(ctx, base, rng, n=N_POINTS):
    """-> {name: int64[m, 2], m <= n} for the base map ctx.maps[base]; `vertices` is a range (b, m) of the other map's
    vertices instead"""
    name = ctx.skew["family"]
    bm, qm = ctx.maps[base], ctx.maps[1 - base]
    seg = bm.segments()
    sets = collections.OrderedDict()
    sets["vertices"] = vertex_range(name, qm.n_points, n, rng)
    sets["shuffled"] = qm.pts[rng.permutation(qm.n_points)[:n]]
    sets["random"] = rng.integers(LO, HI, size=(n, 2))   # as test_gpu_skewed.want_of: most are far from every edge of the dense part
    pick = rng.integers(0, len(seg), n // 2)
    sets["on_base"] = np.concatenate([bm.pts[rng.integers(0, bm.n_points, n - n // 2)],
                                      np.stack([(seg[pick, 0] + seg[pick, 2]) // 2, (seg[pick, 1] + seg[pick, 3]) // 2], 1)])
    side = rng.integers(LO, HI, size=(4, n // 8))
    sets["border"] = np.concatenate([np.array([(LO, LO), (LO, HI), (HI, LO), (HI, HI)], np.int64),
                                     np.stack([side[0], np.full(n // 8, LO)], 1), np.stack([side[1], np.full(n // 8, HI)], 1),
                                     np.stack([np.full(n // 8, LO), side[2]], 1), np.stack([np.full(n // 8, HI), side[3]], 1)])
    if name == "outlier":
        x0, y0, x1, y1 = knot_box(ctx, bm)
        g = KNOT_GROW
        sets["knot"] = np.stack([rng.integers((x0 - g) * CELL, (x1 + 1 + g) * CELL, n // 2), rng.integers((y0 - g) * CELL, (y1 + 1 + g) * CELL, n // 2)], 1) - S.COORD_OFFSET
    le = long_edges(bm)
    if len(le):   # (the framed maps, long_long, and outlier's coarse lattice)
        sets["along_long_edges"] = along(seg[le], rng, max(16, min(256, (n // 2) // len(le))))[:n]
    for k, p in sets.items():
        if k != "vertices":
            sets[k] = np.ascontiguousarray(p, np.int64)
            assert 0 < len(sets[k]) <= n and sets[k].min() >= LO and sets[k].max() <= HI
    return sets


def points_of(ctx, base, sets, name):
    """the coordinates of a set: the slice of the other map's vertices for `vertices`"""
    if name == "vertices":
        b, m = sets[name]
        return ctx.maps[1 - base].pts[b:b + m]
    return sets[name]


# ---- the fans --------------------------------------------------------------------------------------------------------------
Fan = collections.namedtuple("Fan", "P edges m h")   # m: the common distance of an equal fan; h: a tie fan's lies in (h, h + 1)


def d2_interior(P, e):
    """the squared distance of P from the LINE of e as a Fraction (the fans' edges all hold P over their interior)"""
    ax, ay, bx, by = e
    dx, dy, ex, ey = bx - ax, by - ay, P[0] - ax, P[1] - ay
    assert 0 < ex * dx + ey * dy < dx * dx + dy * dy
    return Fraction((dx * ey - dy * ex) ** 2, dx * dx + dy * dy)


def rotated(x, y, quarter):
    for _ in range(quarter % 4):
        x, y = -y, x
    return x, y


def inseparable(d2s):
    """the condition on a fan: no two of these exact squared distances are apart by the filter's margin once in double"""
    f = [Fraction(float(v)) for v in d2s]
    return min(f) >= max(f) * FILTER_KEEP


def tie_fan(rng, K=64, L_bits=(40, 45), h_bits=(30, 44), centre=None, h=None):
    """K >= 64 edges around P after nearest_cases.FAR_EDGE / NEAR_EDGE: edge k runs from (-L_k, h) to (L_k, h + 1) with
    L_k = L - k, turned by 90 degrees (k mod 4) times about the origin and moved to P, in a random order.  d^2 =
    L_k^2 (2 h + 1)^2 / (4 L_k^2 + 1) ascends with L_k: the nearest is the edge with the smallest L_k, by a relative margin of
    about 1 / (2 L^3), far below what a double can tell -- asserted here, as a condition on the inputs"""
    assert K >= 64
    L = int(rng.integers(1 << L_bits[0], 1 << L_bits[1]))
    h = h or int(rng.integers(1 << h_bits[0], 1 << h_bits[1]))
    room = HI - max(L, h + 1) - 1
    P = centre if centre is not None else (int(rng.integers(-room, room)), int(rng.integers(-room, room)))
    edges = []
    for k in range(K):
        a, b = rotated(-(L - k), h, k), rotated(L - k, h + 1, k)
        edges.append((P[0] + a[0], P[1] + a[1], P[0] + b[0], P[1] + b[1]))
    d2 = [d2_interior(P, e) for e in edges]
    assert all(d2[k + 1] < d2[k] for k in range(K - 1)) and inseparable(d2), "doubles must not be able to order the fan"
    order = rng.permutation(K)
    edges = [edges[int(k)] for k in order]
    assert all(LO <= v <= HI for e in edges for v in e)
    return Fan(P, edges, None, h)


# primitive Pythagorean triples whose hypotenuse divides 1105 = 5 13 17
TRIPLES = [(3, 4, 5), (5, 12, 13), (8, 15, 17), (16, 63, 65), (33, 56, 65), (13, 84, 85), (36, 77, 85), (21, 220, 221), (140, 171, 221)]
HYP = 1105


def equal_fan(rng, m_bits=43, len_bits=44, centre=None, m=None):
    """edges at EXACTLY the distance m = 1105 q from P: for every triple (a, b, c) and its rotations and reflections the
    line with the unit normal (a, b) / c at m from P (its foot m (a, b) / c is an integer point), and on it an edge
    foot - s1 k (-b, a) .. foot + s2 k (-b, a) with random k, s1, s2 > 0: the cross product is (s1 + s2) k c m and
    l = ((s1 + s2) k c)^2 -- equal as rationals, different in every limb; every ninth edge instead starts AT a foot and leads
    away from P (where = 1, num = m^2, den = 1: an end against interiors still takes the wide compare)"""
    m = m or HYP * int(rng.integers(1 << (m_bits - 12), 1 << (m_bits - 11)))
    assert m % HYP == 0
    half = 1 << len_bits
    room = HI - m - half - 1
    P = centre if centre is not None else (int(rng.integers(-room, room)), int(rng.integers(-room, room)))
    edges = []
    for a, b, c in TRIPLES:
        for nx, ny in ((a, b), (-a, b), (a, -b), (-a, -b), (b, a), (-b, a), (b, -a), (-b, -a)):
            fx, fy = P[0] + m // c * nx, P[1] + m // c * ny
            if len(edges) % 9 == 8:
                t = int(rng.integers(1, half // (2 * c)))
                edges.append((fx, fy, fx + t * nx, fy + t * ny))
                continue
            k = int(rng.integers(1, 1 << 12))
            s1, s2 = (int(v) for v in rng.integers(1, half // (2 * c * k), 2))
            e = (fx + s1 * k * ny, fy - s1 * k * nx, fx - s2 * k * ny, fy + s2 * k * nx)
            edges.append(e if rng.integers(0, 2) else e[2:] + e[:2])
    for e in edges:
        ax, ay, bx, by = e
        dot = (P[0] - ax) * (bx - ax) + (P[1] - ay) * (by - ay)
        d2 = d2_interior(P, e) if dot > 0 else Fraction((P[0] - ax) ** 2 + (P[1] - ay) ** 2)
        assert d2 == m * m and all(LO <= v <= HI for v in e)
    order = rng.permutation(len(edges))
    return Fan(P, [edges[int(k)] for k in order], m, None)


# ---- a fan inside a map ----------------------------------------------------------------------------------------------------
Scene = collections.namedtuple("Scene", "pts row points fans fan_eids")   # fan_eids[i]: the eids of fan i's edges, ascending
GRID = 9   # the domain in 9 x 9 cells: fans in the columns 0 .. 7 (72 centres), the decoy lattice in column 8


def decoy_lattice(box):
    """a lattice of 4 992 edges (78 leaf blocks of 64, a tree of two levels) in this part (fractions) of the domain, scaled"""
    g = synth.lattice_map(12, 16, 401, bbox=S.sub_bbox(*box))
    return maps.Scaling(synth.US_BBOX).scale(g.points), g.row_index.astype(np.int64)


def scene_of(rng, fans, points, box):
    """the fans' edges as two-point chains and the decoy lattice's chains in one map, the chains in a random order"""
    lp, lrow = decoy_lattice(box)
    chains = [(i, np.array(e, np.int64).reshape(2, 2)) for i, f in enumerate(fans) for e in f.edges]
    chains += [(-1, lp[lrow[c]:lrow[c + 1]]) for c in range(len(lrow) - 1)]
    pts, row, owner = [], [0], []
    for k in rng.permutation(len(chains)):
        i, c = chains[int(k)]
        pts.append(c)
        row.append(row[-1] + len(c))
        owner += [i] * (len(c) - 1)
    owner = np.array(owner)
    pts = np.concatenate(pts)
    assert pts.min() >= LO and pts.max() <= HI and len(owner) > 64 * 64
    return Scene(pts, np.array(row, np.uint32), np.array(points, np.int64).reshape(-1, 2), fans, [np.flatnonzero(owner == i) for i in range(len(fans))])


def single_scene(kind, rng, copies=70):
    """one fan at the issue's full scale, its centre `copies` times as the points (a full wave runs the wide compare in
    every lane), the decoys in the corner of the domain opposite the centre"""
    fan = tie_fan(rng) if kind == "tie" else equal_fan(rng)
    bx, by = (0.02 if fan.P[0] >= 0 else 0.93), (0.02 if fan.P[1] >= 0 else 0.93)
    return scene_of(rng, [fan], [fan.P] * copies, (bx, by, bx + 0.05, by + 0.05))


def replicated_scene(kind, rng):
    """a fan of its own draw at each of 72 centres, one per cell of the grid's columns 0 .. 7, small enough to stay inside
    its cell (half a cell is 2^42.8: L below 2^42.5, h and m below 2^41.6) -- so every centre's nearest edges are its own
    fan's -- and the decoys in column 8"""
    pitch = (HI - LO + 1) // GRID
    fans = []
    for i in range(GRID):
        for j in range(GRID - 1):
            c = (LO + j * pitch + pitch // 2 + int(rng.integers(-1000, 1000)), LO + i * pitch + pitch // 2 + int(rng.integers(-1000, 1000)))
            h, m = (fans[0].h, fans[0].m) if fans else (None, None)   # (one h or m for all centres: one max_dist lists every centre's fan)
            fans.append(tie_fan(rng, 64, (40, 42), (30, 41), centre=c, h=h) if kind == "tie" else equal_fan(rng, 41, 41, centre=c, m=m))
    for f in fans:
        assert all(abs(v - f.P[k % 2]) < pitch // 2 for e in f.edges for k, v in enumerate(e))
    x0 = (GRID - 1) / GRID
    return scene_of(rng, fans, [f.P for f in fans], (x0 + 0.02, 0.1, x0 + 0.09, 0.9))


# ---- what both test modules share ------------------------------------------------------------------------------------------
# the large max_dist of a family's within queries: far above the few units that `along_long_edges` points lie from their long
# edge, hundreds to thousands of edges for a point inside the dense part, and enough for some point of every set to reach
# an edge -- the `border` points are the farthest: 0.02 of the range (2^41.4) from the dense corners and 0.03 from
# rings_frame's frame, 0.004 from short_chains_frame's, 0.1 and 0.12 (2^43.9) from outlier's frame and coarse lattice, 2^45 from
# the ends of long_long's segments, 0.003 per axis (2^39.1) from thin_band's ticks
LARGE = dict(skew_lattice=1 << 42, skew_rings=1 << 42, skew_short_chains=1 << 42, rings_frame=1 << 42, short_chains_frame=1 << 40,
             outlier=1 << 44, long_long=3 << 44, thin_band=1 << 40)
assert sorted(LARGE) == sorted(S.NAMES)
KNOT_DIST = (1 << 10, 1 << 26)   # on outlier's `knot`: 2^10 units, and 2^10 cells of the boxes -- every point lists the whole knot
_sets = {}


def family_sets(name, base):
    """-> (ctx, the base map's segments, point_sets): one draw per family and base, shared by the CPU and the GPU module"""
    if (name, base) not in _sets:
        ctx = S.family(name)
        rng = np.random.default_rng(1000 + 2 * S.NAMES.index(name) + base)
        _sets[name, base] = (ctx, ctx.maps[base].segments(), point_sets(ctx, base, rng))
    return _sets[name, base]


def median_up(dist):
    """the median of the twin's nearest distances, rounded up to an integer max_dist"""
    d = np.sort(np.asarray(dist))
    return int(np.ceil(d[len(d) // 2]))


def exact_table(px, py, edges):
    """[(where, num, den, N, D)] of the point against every edge, N / D = d^2 in Python integers (nearest_ref.point_edge)"""
    out = []
    for e in edges:
        where, num, den = NR.point_edge(px, py, e)
        out.append((where, num, den, num * num if where == NR.INTERIOR else num, den))
    return out


def nearest_of(table, max_dist=-1):
    """the definition on a table, cross-multiplied: the smallest N / D, the smaller eid on a tie; MISS where none qualifies"""
    best, bn, bd, m2 = (NR.MISS, 0, 0, 0), None, None, max_dist * max_dist
    for eid, (where, num, den, N, D) in enumerate(table):
        if max_dist >= 0 and N > m2 * D:
            continue
        if bn is None or N * bd < bn * D:
            best, bn, bd = (eid, where, num, den), N, D
    return best


def within_of(table, max_dist):
    m2 = max_dist * max_dist
    return [(eid, where, num, den) for eid, (where, num, den, N, D) in enumerate(table) if N <= m2 * D]
