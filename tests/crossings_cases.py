"""Hand-built chain maps for rj_map_crossings with the answers written out: the smallest shapes at which each rule of
rayjoin_amd/csrc/rj_crossings.h can go wrong (HAND), the shapes that try the grid (GRID), and the generators of the
random tests.  A case is (chains, records, n_zero_edges): chains a list of point lists, edge e = p - c of point p of
chain c, records [(eid0, eid1, kind)] ascending.  HAND cases are written in small lattice units and go through as_map,
which multiplies them out and adds a far edge (the last one, meeting nothing) so that the coordinates span 2^30: at
shift 15 the map has thousands of cells, at 47 one.  ABSOLUTE and GRID cases are used as they stand."""
import numpy as np

PROPER, TOUCH, OVERLAP, EQUAL = 1, 2, 3, 4
L = 1 << 46
UNIT = 1 << 18
FAR = 1 << 30
CELL = 1 << 15  # a cell at the smallest shift


def chain_arrays(chains):
    xy = [p for c in chains for p in c]
    row = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    return np.array(xy, np.int64).reshape(-1, 2), row


def as_map(chains, unit=UNIT, off=(0, 0)):
    """lattice units -> (xy, row_index): multiplied out, moved by off, one far edge behind everything"""
    moved = [[(x * unit + off[0], y * unit + off[1]) for x, y in c] for c in chains]
    return chain_arrays(moved + [[(FAR, FAR), (FAR + unit, FAR)]])


HAND = {
    "x": ([[(0, 0), (4, 4)], [(0, 4), (4, 0)]], [(0, 1, PROPER)], 0),
    "x-uneven": ([[(0, 0), (7, 3)], [(1, 5), (2, 0)]], [(0, 1, PROPER)], 0),
    "t": ([[(0, 0), (4, 0)], [(2, 0), (2, 3)]], [(0, 1, TOUCH)], 0),
    "t-end-of-second": ([[(2, 3), (2, 0)], [(0, 0), (4, 0)]], [(0, 1, TOUCH)], 0),
    "t-skew": ([[(0, 0), (6, 3)], [(4, 2), (1, 7)]], [(0, 1, TOUCH)], 0),
    "corner": ([[(0, 0), (2, 2)], [(2, 2), (4, 0)]], [], 0),
    "corner-collinear": ([[(0, 0), (2, 2)], [(2, 2), (5, 5)]], [], 0),
    "corner-collinear-reversed": ([[(2, 2), (0, 0)], [(2, 2), (5, 5)]], [], 0),
    "bend-in-chain": ([[(0, 0), (2, 2), (5, 5), (5, 0)]], [], 0),
    "junction": ([[(3, 3), (0, 0)], [(3, 3), (6, 0)], [(3, 3), (3, 7)], [(0, 6), (3, 3)]], [], 0),
    "overlap": ([[(0, 0), (4, 0)], [(2, 0), (6, 0)]], [(0, 1, OVERLAP)], 0),
    "overlap-skew-opposite": ([[(0, 0), (4, 2)], [(6, 3), (2, 1)]], [(0, 1, OVERLAP)], 0),
    "overlap-vertical": ([[(1, 0), (1, 4)], [(1, 6), (1, 3)]], [(0, 1, OVERLAP)], 0),
    "inside": ([[(0, 0), (6, 0)], [(2, 0), (4, 0)]], [(0, 1, OVERLAP)], 0),
    "inside-shared-end": ([[(0, 0), (6, 0)], [(0, 0), (3, 0)]], [(0, 1, OVERLAP)], 0),
    "equal-same": ([[(1, 1), (3, 2)], [(1, 1), (3, 2)]], [(0, 1, EQUAL)], 0),
    "equal-opposite": ([[(1, 1), (3, 2)], [(3, 2), (1, 1)]], [(0, 1, EQUAL)], 0),
    "fold": ([[(0, 0), (3, 1), (0, 0)]], [(0, 1, EQUAL)], 0),
    "fold-longer": ([[(0, 0), (3, 1), (1, 4), (3, 1), (0, 0)]], [(0, 3, EQUAL), (1, 2, EQUAL)], 0),
    "collinear-apart": ([[(0, 0), (1, 1)], [(2, 2), (3, 3)]], [], 0),
    "collinear-apart-vertical": ([[(2, 0), (2, 1)], [(2, 5), (2, 3)]], [], 0),
    "parallel": ([[(0, 0), (4, 0)], [(0, 1), (4, 1)]], [], 0),
    "parallel-skew": ([[(0, 0), (4, 2)], [(0, 1), (4, 3)]], [], 0),
    "boxes-meet-segments-do-not": ([[(0, 0), (4, 4)], [(3, 0), (4, 1)]], [], 0),
    "closed": ([[(0, 0), (4, 0), (2, 3), (0, 0)]], [], 0),
    "bowtie": ([[(0, 0), (4, 4), (4, 0), (0, 4), (0, 0)]], [(0, 2, PROPER)], 0),
    "vertex-on-neighbour": ([[(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], [(4, 2), (8, 2), (8, 6), (4, 2)]], [(1, 4, TOUCH), (1, 6, TOUCH)], 0),
    # e0 zero, e1 (0,0)-(4,4), e2 zero, e3 (4,4)-(8,0), e4 zero; e5 (0,4)-(4,0) crosses e1, is parallel to e3; e6 a zero
    # edge lying on that crossing
    "zero-edges": ([[(0, 0), (0, 0), (4, 4), (4, 4), (8, 0), (8, 0)], [(0, 4), (4, 0)], [(2, 2), (2, 2)]], [(1, 5, PROPER)], 4),
    "only-zero-edges": ([[(1, 1), (1, 1), (1, 1)], [(1, 1), (1, 1)]], [], 3),
    "one-point-chains": ([[(1, 1)], [(0, 0), (4, 4)], [(2, 2)], [(0, 4), (4, 0)], [(9, 9)]], [(0, 1, PROPER)], 0),
    "one-edge": ([[(0, 0), (1, 2)]], [], 0),
    # three through one point, one of them ending there
    "three-at-a-point": ([[(0, 0), (4, 4)], [(0, 4), (4, 0)], [(2, 2), (2, 6)]], [(0, 1, PROPER), (0, 2, TOUCH), (1, 2, TOUCH)], 0),
}

# ---- coordinates at the edge of the range, as they stand -----------------------------------------------------------------
# D runs from (-L, -L) to (L - 1, L - 2).  C = (L - 2, L - 3) lies one unit of cross product to the right of it
# ((2L - 1)(2L - 3) - (2L - 2)^2 = -1, two products of 2^94: their difference is 0 in double).  Up = (L - 5, L - 2) lies
# left of D, Down = (L - 2, L - 6) right of it: Up - C crosses D properly, Down - C does not meet it.
_D = [(-L, -L), (L - 1, L - 2)]
_C, _UP, _DOWN = (L - 2, L - 3), (L - 5, L - 2), (L - 2, L - 6)
ABSOLUTE = {
    "diagonal-proper": ([_D, [_UP, _C]], [(0, 1, PROPER)], 0),
    "diagonal-none": ([_D, [_DOWN, _C]], [], 0),
    "diagonal-both": ([[_UP, _C], _D, [_C, _DOWN]], [(0, 1, PROPER)], 0),
    # the point itself on the diagonal of slope 1: a touch; one unit off: nothing
    "diagonal-touch": ([[(-L, -L), (L - 1, L - 1)], [(L - 9, L - 9), (L - 9, L - 1)]], [(0, 1, TOUCH)], 0),
    "diagonal-miss": ([[(-L, -L), (L - 1, L - 1)], [(L - 9, L - 8), (L - 9, L - 1)]], [], 0),
    # touches at exactly -2^46 and at 2^46 - 1, in x and in y
    "touch-at-the-rim": ([[(-L, -L), (-L, L - 1)], [(-L, 0), (5, 7)], [(L - 1, -L), (L - 1, L - 1)], [(0, 0), (L - 1, 5)],
                          [(-L + 1, -L), (L - 2, -L)], [(9, -L), (9, -L + 4)], [(-L + 1, L - 1), (L - 2, L - 1)], [(-7, L - 1), (-9, L - 5)]],
                         [(0, 1, TOUCH), (2, 3, TOUCH), (4, 5, TOUCH), (6, 7, TOUCH)], 0),
    "empty": ([], [], 0),
    "points-only": ([[(1, 1)], [(2, 2)]], [], 0),
}


def absolute_map(name):
    chains, want, zero = ABSOLUTE[name]
    return chain_arrays(chains), want, zero


# ---- shapes that try the grid, as they stand (forced shift 15: a cell is 2^15 wide) ----------------------------------------
def star(n, centre=(CELL // 2, CELL // 2)):
    """n edges through one interior point, pairwise different directions, all inside one cell of every shift: every pair
    crosses properly, n (n - 1) / 2 records"""
    cx, cy = centre
    chains = [[(cx - (100 - k), cy - 300), (cx + (100 - k), cy + 300)] for k in range(n)]
    return chains, [(a, b, PROPER) for a in range(n) for b in range(a + 1, n)], 0


_X = 1100 * CELL + 100
_K = 3 * CELL
GRID = {
    # an edge over more than 1000 cells, crossed by a short one in its last cell
    "long-last-cell": ([[(10, 10), (_X + 50, 60)], [(_X, 0), (_X + 20, 200)]], [(0, 1, PROPER)], 0),
    "long-last-cell-negative": ([[(-10, -10), (-_X - 50, -60)], [(-_X, 0), (-_X - 20, -200)]], [(0, 1, PROPER)], 0),
    # two long edges that share thousands of cells and cross once
    "two-long": ([[(0, 0), (1 << 25, _K)], [(0, _K), (1 << 25, 0)]], [(0, 1, PROPER)], 0),
    "two-long-mixed-sign": ([[(-(1 << 24), -_K), (1 << 24, _K)], [(-(1 << 24), _K), (1 << 24, -_K)], [(-(1 << 24), 5), (1 << 24, 5)]],
                            [(0, 1, PROPER), (0, 2, PROPER), (1, 2, PROPER)], 0),
    # the crossing point on a cell corner, on a vertical and on a horizontal cell boundary
    "on-a-corner": ([[(_K - 8, _K - 8), (_K + 8, _K + 8)], [(_K - 8, _K + 8), (_K + 8, _K - 8)]], [(0, 1, PROPER)], 0),
    "on-a-corner-negative": ([[(-_K - 8, -_K - 8), (-_K + 8, -_K + 8)], [(-_K - 8, -_K + 8), (-_K + 8, -_K - 8)]], [(0, 1, PROPER)], 0),
    "on-a-boundary-x": ([[(_K - 8, _K - 3), (_K + 8, _K + 13)], [(_K - 8, _K + 13), (_K + 8, _K - 3)]], [(0, 1, PROPER)], 0),
    "on-a-boundary-y": ([[(_K - 3, _K - 8), (_K + 13, _K + 8)], [(_K + 13, _K - 8), (_K - 3, _K + 8)]], [(0, 1, PROPER)], 0),
    # a vertex exactly on a cell corner inside a long edge; an overlap along a cell boundary
    "touch-on-a-corner": ([[(0, _K), (8 * CELL, _K)], [(_K, _K), (_K + 5, 5 * CELL)]], [(0, 1, TOUCH)], 0),
    "overlap-on-a-boundary": ([[(_K, 0), (_K, 6 * CELL)], [(_K, 9 * CELL), (_K, 4 * CELL)], [(_K - 1, 0), (_K - 1, 6 * CELL)]], [(0, 1, OVERLAP)], 0),
    "all-negative": ([[(-9 * CELL, -9 * CELL), (-5 * CELL, -5 * CELL)], [(-9 * CELL, -5 * CELL), (-5 * CELL, -9 * CELL)],
                      [(-7 * CELL, -7 * CELL), (-7 * CELL, -2 * CELL)]], [(0, 1, PROPER), (0, 2, TOUCH), (1, 2, TOUCH)], 0),
    "across-zero": ([[(-CELL, -CELL), (CELL, CELL)], [(-CELL, CELL), (CELL, -CELL)], [(0, 0), (0, 0)], [(-5, 0), (5, 0)]],
                    [(0, 1, PROPER), (0, 3, PROPER), (1, 3, PROPER)], 1),
}
STAR_SIZES = (63, 64, 65, 128, 129, 200)


def grid_map(name):
    chains, want, zero = GRID[name]
    return chain_arrays(chains), want, zero


# ---- random maps -------------------------------------------------------------------------------------------------
def soup(seed):
    """50-400 edges in chains of 1-12 points on a small lattice (so that touches, overlaps and equal edges occur), a
    tenth of the points repeated (zero edges), multiplied out and moved into any of the four quadrants, one far edge
    behind everything"""
    rng = np.random.default_rng(1000 + seed)
    want = int(rng.integers(50, 401))
    side = int(rng.choice([6, 9, 14, 24]))
    chains, n = [], 0
    while n < want:
        k = int(rng.integers(1, 13))
        pts = [tuple(int(v) for v in rng.integers(0, side, 2))]
        for _ in range(k - 1):
            if rng.random() < 0.1:
                pts.append(pts[-1])
            else:
                step = rng.integers(-3, 4, 2)
                pts.append((int(np.clip(pts[-1][0] + step[0], 0, side - 1)), int(np.clip(pts[-1][1] + step[1], 0, side - 1))))
        chains.append(pts)
        n += k - 1
    unit = int(rng.choice([1, 1 << 12, 1 << 16]))
    off = (int(rng.choice([0, -side * unit, -(side // 2) * unit])), int(rng.choice([0, -side * unit, -(side // 2) * unit])))
    return as_map(chains, unit, off)


def throw_chains(m, seed):
    """a planar map (xy, row_index, ...) with 1-5 extra chains of 2-4 points thrown across its bounding box"""
    xy, row = np.asarray(m[0], np.int64).reshape(-1, 2), np.asarray(m[1], np.uint32)
    rng = np.random.default_rng(7000 + seed)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    new_xy, new_row = [xy], list(row)
    for _ in range(int(rng.integers(1, 6))):
        k = int(rng.integers(2, 5))
        pts = np.stack([rng.integers(int(lo[0]), int(hi[0]) + 1, k), rng.integers(int(lo[1]), int(hi[1]) + 1, k)], axis=1)
        new_xy.append(pts.astype(np.int64))
        new_row.append(new_row[-1] + k)
    return np.concatenate(new_xy), np.array(new_row, np.uint32)
