"""Chain maps for the polygon tests (tests/test_polygons.py, tests/test_gpu_polygons.py): each is (xy int64 [np, 2],
row_index uint32, left int32, right int32), turned into rings by rings_ref.rings_ref and then into polygons.  Where the
answer is known from the construction it comes with the map; the written answers are in tests/test_polygons.py."""
import numpy as np

import rings_cases as K
from rings_planar import SHEAR

LIM = 1 << 46
NONE = 0xFFFFFFFF
COLUMN_SIZES = (1, 2, 3, 64, 65, 1000)
LINEAR_MAPS = {"identity": ((1, 0), (0, 1)), "shear": SHEAR, "quarter-turn": ((0, -1), (1, 0)), "spiral": ((1, 1), (-1, 1)),
               "reflection": ((-1, 0), (0, -1))}  # (all of positive determinant: a counter-clockwise walk stays one)
SPAN_HOLES = 2000
SPAN_SHIFT = 36  # 2^(47 - s) strips of the one domain-wide edge + 2 n <= 2 (2 n + 1) edges first holds at 2^11 <= 4002


def box(x0, y0, x1, y1, inside, outside):
    """a closed chain counter-clockwise round the rectangle: `inside` on its left"""
    return ([(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)], inside, outside)


def closed(points, inside, outside):
    """a closed chain through `points` (counter-clockwise): `inside` on its left"""
    return (list(points) + [points[0]], inside, outside)


def multi_part():
    """face 1 in three parts: two disjoint squares, each with a hole (faces 2 and 3 inside), and an island of face 1 inside
    the first hole with a hole of its own (face 4)"""
    return K.chain_map([box(0, 0, 20, 20, 1, 0), box(5, 5, 15, 15, 2, 1), box(30, 0, 50, 20, 1, 0), box(35, 5, 45, 15, 3, 1),
                        box(7, 7, 13, 13, 1, 2), box(9, 9, 11, 11, 4, 1)])


def hole_column(k):
    """one shell of face 1 with k holes (face 2 inside) stacked so that the ray of hole j hits hole j + 1: hole j is
    [j, j + 4] x [10 j + 2, 10 j + 6], its top (j + 4, 10 j + 6) lies under the bottom edge of hole j + 1"""
    chains = [box(-10, -10, k + 20, 10 * k + 20, 1, 0)]
    chains += [box(j, 10 * j + 2, j + 4, 10 * j + 6, 2, 1) for j in range(k)]
    return K.chain_map(chains)


def _in_shell(holes):
    return K.chain_map([box(-100, -100, 100, 100, 1, 0)] + holes)


def below_hole_vertex():
    """the top (4, 4) of a square hole exactly below the vertex (4, 10) of a triangular hole: only the edge (8, 14) -> (4, 10)
    covers the ray"""
    return _in_shell([box(0, 0, 4, 4, 2, 1), closed([(4, 10), (8, 14), (0, 14)], 2, 1)])


def equal_heights():
    """two triangular holes that both start at (4, 10) and open to the right, above the top (4, 4): their lower edges have
    the same height at the ray, the flatter one is lower just right of it"""
    return _in_shell([box(0, 0, 4, 4, 2, 1), closed([(4, 10), (12, 10), (12, 12)], 2, 1), closed([(4, 10), (12, 14), (12, 18)], 2, 1)])


def neither_covers():
    """a triangular hole whose vertex (4, 10) points to the right, above the top (4, 4): neither of its edges covers the ray"""
    return _in_shell([box(0, 0, 4, 4, 2, 1), closed([(0, 8), (4, 10), (0, 12)], 2, 1)])


def below_vertical_edges():
    """above the top (4, 4): the left edge of one hole at x = 4 (its bottom edge covers the ray); above the top (-6, 4): the
    right edge of another at x = -6 (its bottom edge does not)"""
    return _in_shell([box(0, 0, 4, 4, 2, 1), box(4, 10, 8, 14, 2, 1), box(-10, 0, -6, 4, 2, 1), box(-10, 10, -6, 14, 2, 1)])


def repeated_top():
    """a hole whose top is two points of the ring (a zero-length edge), under a hole with a horizontal bottom edge"""
    return _in_shell([([(0, 0), (4, 0), (4, 4), (4, 4), (0, 4), (0, 0)], 2, 1), box(-20, 10, 20, 14, 2, 1)])


def domain_span(n=SPAN_HOLES):
    """a shell over the whole coordinate range, -2^46 to 2^46 - 1, above n holes of 4 units: the one long edge lies in
    2^(47 - s) strips"""
    chains = [box(-LIM, -LIM, LIM - 1, LIM - 1, 1, 0)] + [box(8 * j, 0, 8 * j + 4, 4, 2, 1) for j in range(n)]
    return K.chain_map(chains)


def touching_shells():
    """two squares of face 1 that touch at (0, 0) (the layout of rings_cases.crossing), each with a hole (faces 2 and 3)"""
    return K.chain_map([([(0, 0), (40, 0), (40, 40), (0, 40), (0, 0)], 1, 0), ([(0, 0), (-40, 0), (-40, -40), (0, -40), (0, 0)], 1, 0),
                        box(10, 10, 30, 30, 2, 1), box(-30, -30, -10, -10, 3, 1)])


def touching_holes():
    """two square holes of face 1 that touch at (10, 10), where both chains start: one ring of face 1 round both"""
    return K.chain_map([box(-100, -100, 100, 100, 1, 0), ([(10, 10), (0, 10), (0, 0), (10, 0), (10, 10)], 2, 1),
                        ([(10, 10), (20, 10), (20, 20), (10, 20), (10, 10)], 2, 1)])


def orphan():
    """a clockwise ring labelled 5 with nothing round it"""
    return K.chain_map([([(0, 0), (0, 4), (4, 4), (4, 0), (0, 0)], 5, 0)])


HAND = {"hole": K.square_with_hole, "dangling": K.dangling, "star": K.star, "multi-part": multi_part, "below-hole-vertex": below_hole_vertex,
        "equal-heights": equal_heights, "neither-covers": neither_covers, "below-vertical-edges": below_vertical_edges,
        "repeated-top": repeated_top, "touching-shells": touching_shells, "touching-holes": touching_holes, "orphan": orphan}
HAND.update({"column-%d" % k: (lambda k=k: hole_column(k)) for k in COLUMN_SIZES})


# ---- laminar families ------------------------------------------------------------------------------------------------
def _nest(rng, x0, y0, x1, y1, face, depth, parent, rects):
    """rectangles inside (x0, x1) x (y0, y1), a gap of at least one unit to its boundary and to each other: one per cell
    of a g x g grid, with probability 0.6, inset by 1 to 3 units; then the same inside each"""
    g = int(rng.integers(2, 4))
    cw, ch = (x1 - x0) // g, (y1 - y0) // g
    if depth >= 5 or cw < 8 or ch < 8:
        return
    for ix in range(g):
        for iy in range(g):
            if rng.random() > 0.6:
                continue
            a, b, c, d = (int(v) for v in rng.integers(1, 4, 4))
            r = (x0 + ix * cw + a, y0 + iy * ch + b, x0 + (ix + 1) * cw - c, y0 + (iy + 1) * ch - d)
            f = int(rng.choice([v for v in (1, 2, 3) if v != face]))
            rects.append((r, f, face, parent))
            _nest(rng, *r, f, depth + 1, len(rects) - 1, rects)


def laminar(seed, A=((1, 0), (0, 1)), size=320):
    """random nested rectangles on a lattice, depth at most 5, face ids from a pool of three that differ from the
    enclosing region's, under the linear map A; every boundary cut into one to three chains at lattice points, the chains
    shuffled, half of them reversed.  -> (map, info): info["rects"] = [(rect, face inside, face outside, enclosing
    rectangle or -1)], info["at"] = {image of a boundary point: rectangle}"""
    rng = np.random.default_rng(seed)
    rects = []
    _nest(rng, 0, 0, size, size, 0, 0, -1, rects)
    img = lambda p: (A[0][0] * p[0] + A[0][1] * p[1], A[1][0] * p[0] + A[1][1] * p[1])  # noqa: E731
    chains, at = [], {}
    for k, ((x0, y0, x1, y1), inside, outside, _) in enumerate(rects):
        loop = ([(x, y0) for x in range(x0, x1)] + [(x1, y) for y in range(y0, y1)] + [(x, y1) for x in range(x1, x0, -1)] +
                [(x0, y) for y in range(y1, y0, -1)])  # counter-clockwise, every lattice point of the boundary
        keep = sorted(set(rng.choice(len(loop), size=min(len(loop), 4 + int(rng.integers(0, 6))), replace=False).tolist()) |
                      {loop.index(c) for c in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))})
        pts = [img(loop[i]) for i in keep]
        for p in pts:
            at[p] = k
        cuts = sorted(rng.choice(len(pts), size=int(rng.integers(1, 4)), replace=False).tolist())
        for a, b in zip(cuts, cuts[1:] + [cuts[0] + len(pts)]):
            piece = [pts[i % len(pts)] for i in range(a, b + 1)]
            chains.append((piece[::-1], outside, inside) if rng.random() < 0.5 else (piece, inside, outside))
    order = rng.permutation(len(chains)).tolist()
    return K.chain_map([chains[i] for i in order]), dict(rects=rects, at=at)


def laminar_parents(info, rings, ring_row, ring_xy, area2):
    """the parent of every ring from the construction: a ring lies on one rectangle (found by its first point) -- the
    counter-clockwise one is the shell of the rectangle's inside, the clockwise one a hole of the enclosing rectangle's
    shell, or a ring of face 0"""
    on = [info["at"][tuple(int(v) for v in ring_xy[int(ring_row[r])])] for r in range(len(rings))]
    shell_of = {k: r for r, k in enumerate(on) if area2[r] > 0}
    want = []
    for r, k in enumerate(on):
        if area2[r] > 0:
            want.append(r)
        else:
            outer = info["rects"][k][3]
            want.append(shell_of[outer] if outer >= 0 else NONE)
    return np.array(want, np.uint32)


def hole_field(n_side=260, pitch=1 << 17):
    """n_side^2 square holes of one face (more than 2^16 for 260) in one shell, a strip of 2^16 units apart: the holes of a
    column share their buckets with the shell's long top edge only"""
    j = np.arange(n_side * n_side, dtype=np.int64)
    x0, y0 = (j % n_side) * pitch + 64, (j // n_side) * pitch + 64
    w = 1000
    corners = np.stack([np.stack([x0, y0], 1), np.stack([x0 + w, y0], 1), np.stack([x0 + w, y0 + w], 1), np.stack([x0, y0 + w], 1),
                        np.stack([x0, y0], 1)], 1)  # [n, 5, 2]
    L = n_side * pitch
    shell = np.array([[0, 0], [L, 0], [L, L], [0, L], [0, 0]], np.int64)
    xy = np.concatenate([shell, corners.reshape(-1, 2)])
    n = len(j)
    row = (np.arange(n + 2, dtype=np.uint32) * 5).astype(np.uint32)
    left = np.concatenate([[1], np.full(n, 2)]).astype(np.int32)
    right = np.concatenate([[0], np.full(n, 1)]).astype(np.int32)
    return xy, row, left, right
