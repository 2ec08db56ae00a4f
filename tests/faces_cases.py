"""Hand-built chain maps for the face tests (tests/test_faces.py, tests/test_gpu_faces.py) with the answers written out:
name -> (xy int64 [np, 2], row_index uint32, the answer).  The answer: left / right per chain, the counts of rj_map_faces
(n_conflicts 0: no labels go in), area2 per face, and, where the case is about it, `above` per ring (rings ascend by leader).
Face k is the k-th shell by its leader half-chain; 2 c is chain c forward, 2 c + 1 backward."""
import numpy as np

from rings_cases import chain_map

COUNTS = ("n_faces", "n_rings", "n_holes", "n_outer", "n_skipped", "n_dangling", "n_conflicts")


def _square(x0, y0, x1, y1, clockwise=False):
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return pts[::-1] if clockwise else pts


def _case(chains, left, right, counts, area2, above=None):
    xy, row, _, _ = chain_map([(pts, 0, 0) for pts in chains])
    return xy, row, dict(left=left, right=right, counts=dict(zip(COUNTS, counts + (0,))), area2=area2, above=above)


def triangle():
    return _case([[(0, 0), (4, 0), (0, 4), (0, 0)]], [1], [0], (1, 2, 0, 1, 0, 0), [16])


def square_in_square():
    """face 1 between the squares, face 2 inside the inner one (digitised clockwise: its right side)"""
    return _case([_square(0, 0, 10, 10), _square(2, 2, 6, 6, clockwise=True)], [1, 1], [0, 2], (2, 4, 1, 1, 0, 0), [168, 32])


def island_in_lake_in_island():
    """land (face 1) between chains 0 and 1, a lake (face 2) inside chain 1 with two islets (faces 3, 4), the lower one's top
    under the upper one: every half-chain is a ring of its own, ring = h.  above(ring 5, the lower islet's outside) = ring 7, the
    upper islet's outside -- a hole --, above(7) = ring 2, the lake's shell: a walk of length 2"""
    chains = [_square(0, 0, 40, 40), _square(5, 5, 35, 35), _square(10, 10, 20, 15), _square(12, 20, 28, 25)]
    return _case(chains, [1, 2, 3, 4], [0, 1, 2, 2], (4, 8, 3, 1, 0, 0), [1400, 1540, 100, 160], above=[None, None, None, 0, None, 7, None, 2])


def dangle_in_face():
    """a chain that hangs from the square's first point into its inside: both its sides are face 1, one ring with the square"""
    return _case([_square(0, 0, 10, 10), [(0, 0), (3, 4)]], [1, 1], [0, 1], (1, 2, 0, 1, 0, 1), [200])


def segment_in_face():
    """an isolated segment inside the square: a ring of area 0, a hole of face 1"""
    return _case([_square(0, 0, 10, 10), [(3, 3), (5, 4)]], [1, 1], [0, 1], (1, 3, 1, 1, 0, 1), [200], above=[None, None, 0])


def bridge_to_island():
    """an island joined to its shell by a bridge between their first points: face 1's boundary is ONE ring (the square, the
    bridge, the island's outside, the bridge back), no hole"""
    return _case([_square(0, 0, 10, 10), _square(4, 4, 6, 6), [(0, 0), (4, 4)]], [1, 2, 1], [0, 1, 1], (2, 3, 0, 1, 0, 1), [192, 8])


def top_under_shared_vertex():
    """a house whose roof's ridge (5, 14) is shared by two ceiling edges; the segment's top (5, 3) lies exactly under it: the
    half-open rule takes the edge on its right, (10, 10) -> (5, 14), alone"""
    return _case([[(0, 0), (10, 0), (10, 10), (5, 14), (0, 10), (0, 0)], [(4, 2), (5, 3)]], [1, 1], [0, 1], (1, 3, 1, 1, 0, 1), [240],
                 above=[None, None, 0])


def top_under_vertical_edge():
    """a square with a notch from its top; the segment's top (6, 2) lies under the notch's vertical edge x = 6: the ray stands
    at 6 + epsilon and meets (10, 10) -> (6, 10), not the notch's floor (6, 7) -> (3, 7)"""
    outer = [(0, 0), (10, 0), (10, 10), (6, 10), (6, 7), (3, 7), (3, 10), (0, 10), (0, 0)]
    return _case([outer, [(5, 1), (6, 2)]], [1, 1], [0, 1], (1, 3, 1, 1, 0, 1), [182], above=[None, None, 0])


def figure_eight():
    """two squares that share their first point, a junction of degree 4: their outsides are one ring"""
    return _case([_square(0, 0, 4, 4), [(0, 0), (-4, 0), (-4, -4), (0, -4), (0, 0)]], [1, 2], [0, 0], (2, 3, 0, 1, 0, 0), [32, 32])


def one_point_chain():
    return _case([[(0, 0), (4, 0), (0, 4), (0, 0)], [(1, 1)]], [1, 0], [0, 0], (1, 2, 0, 1, 1, 0), [16])


def empty_map():
    return np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), dict(left=[], right=[], counts=dict(zip(COUNTS, (0,) * 7)), area2=[], above=None)


def side_by_side():
    """a triangle under its hypotenuse y = x - 20 and a square above that line inside the triangle's box: the square's ray runs
    through the box of the triangle's edges and meets none; both outsides lie in face 0"""
    return _case([[(20, 0), (40, 0), (40, 40), (20, 0)], _square(22, 30, 25, 35)], [1, 2], [0, 0], (2, 4, 0, 2, 0, 0), [800, 30],
                 above=[None, None, None, None])


T = 1 << 46  # coordinates lie in [-T, T)


def corner_cell():
    """a square in a square inside [T - 2^15, T)^2: at shift 15 that cell's key is the largest 64-bit number, the one that
    fills the unused registration slots and that has no successor to search for.  The inner square's outside (ring 2) finds
    its ceiling edge in that very cell's run"""
    return _case([_square(T - 20, T - 20, T - 1, T - 1), _square(T - 15, T - 15, T - 10, T - 10, clockwise=True)], [1, 1], [0, 2],
                 (2, 4, 1, 1, 0, 0), [672, 50], above=[None, None, 0, None])


def corner_cell_alone():
    """one triangle in that cell: the map's first column is its last"""
    return _case([[(T - 10, T - 10), (T - 1, T - 10), (T - 10, T - 1), (T - 10, T - 10)]], [1], [0], (1, 2, 0, 1, 0, 0), [81])


def corner_cell_and_neighbour():
    """the triangle in the corner cell and a second one 40 000 units down and left, in another column and row at shift 15"""
    tri = lambda x, y: [(x, y), (x + 9, y), (x, y + 9), (x, y)]  # noqa: E731
    return _case([tri(T - 40010, T - 40010), tri(T - 10, T - 10)], [1, 2], [0, 0], (2, 4, 0, 2, 0, 0), [81, 81], above=[None] * 4)


def low_corner_cell():
    """the mirror: a square in a square in the cell of key 0"""
    return _case([_square(-T, -T, 19 - T, 19 - T), _square(5 - T, 5 - T, 10 - T, 10 - T, clockwise=True)], [1, 1], [0, 2], (2, 4, 1, 1, 0, 0),
                 [672, 50], above=[None, None, 0, None])


HAND = {"corner-cell": corner_cell, "corner-cell-alone": corner_cell_alone, "corner-cell-neighbour": corner_cell_and_neighbour,
        "low-corner-cell": low_corner_cell, "triangle": triangle, "square-in-square": square_in_square, "island-lake-island": island_in_lake_in_island, "dangle": dangle_in_face,
        "segment": segment_in_face, "bridge": bridge_to_island, "shared-vertex": top_under_shared_vertex, "vertical-edge": top_under_vertical_edge,
        "figure-eight": figure_eight, "one-point": one_point_chain, "empty": empty_map, "side-by-side": side_by_side}


def diamond_column(n, pitch=16, x=100):
    """n isolated unit squares standing on a corner, one above the other: (x, y), (x + 1, y + 1), (x, y + 2), (x - 1, y + 1) at
    y = pitch k, digitised clockwise.  Each is two rings, its inside (a shell) and its outside (a hole); the top (x, y + 2) of
    square k lies under the lowest corner of square k + 1, strictly inside the x-range of its lower right edge: above(outside k)
    = outside k + 1 -- a jumping depth of n -- and every outside ends in face 0.  All 4 n edges are ceiling edges of one
    column of the grid (their x lie in [x - 1, x + 1], far from a cell border at any shift).
    -> (xy, row_index); left[k] = 0, right[k] = k + 1"""
    k = np.arange(n, dtype=np.int64)
    y = pitch * k
    one = np.stack([np.stack([np.full(n, x), y], 1), np.stack([np.full(n, x - 1), y + 1], 1), np.stack([np.full(n, x), y + 2], 1),
                    np.stack([np.full(n, x + 1), y + 1], 1), np.stack([np.full(n, x), y], 1)], axis=1)  # [n, 5, 2], clockwise
    return one.reshape(-1, 2), (5 * np.arange(n + 1)).astype(np.uint32)
