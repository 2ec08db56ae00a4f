"""Hand-built chain maps for rj_map_node with the answers written out: the smallest shapes at which each rule of
rayjoin_amd/csrc/rj_node.h can go wrong (HAND), and the generators of the larger tests: brick walls, random soups, one
long edge with many T-junctions.  A hand case is (chains, noded chains, written counts): chains a list of point lists,
used as they stand; the records are those of the crossings definition (tests/crossings_ref.py) on the map; the written
counts are (n_cuts, n_cut_edges, n_max_cuts, n_used, n_proper, n_equal)."""
import random

import numpy as np

L = 1 << 46


def chain_arrays(chains):
    xy = [p for c in chains for p in c]
    row = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    return np.array(xy, np.int64).reshape(-1, 2), row


HAND = {
    "t": ([[(0, 0), (4, 0)], [(2, 0), (2, 3)]],
          [[(0, 0), (2, 0), (4, 0)], [(2, 0), (2, 3)]], (1, 1, 1, 1, 0, 0)),
    # a vertex of three chains inside one edge: one cut
    "three-chains-one-vertex": ([[(0, 0), (6, 0)], [(3, 0), (3, 4)], [(3, 0), (1, 5)], [(5, 5), (3, 0)]],
                                [[(0, 0), (3, 0), (6, 0)], [(3, 0), (3, 4)], [(3, 0), (1, 5)], [(5, 5), (3, 0)]], (1, 1, 1, 3, 0, 0)),
    # the records (0, 1), (0, 2) name the cut at 7 before the cut at 2
    "two-cuts-reversed": ([[(0, 0), (10, 0)], [(7, 0), (7, 3)], [(2, 0), (2, 3)]],
                          [[(0, 0), (2, 0), (7, 0), (10, 0)], [(7, 0), (7, 3)], [(2, 0), (2, 3)]], (2, 1, 2, 2, 0, 0)),
    "vertical": ([[(1, 0), (1, 8)], [(1, 5), (4, 5)], [(-2, 2), (1, 2)]],
                 [[(1, 0), (1, 2), (1, 5), (1, 8)], [(1, 5), (4, 5)], [(-2, 2), (1, 2)]], (2, 1, 2, 2, 0, 0)),
    "vertical-downward": ([[(1, 8), (1, 0)], [(1, 5), (4, 5)], [(-2, 2), (1, 2)]],
                          [[(1, 8), (1, 5), (1, 2), (1, 0)], [(1, 5), (4, 5)], [(-2, 2), (1, 2)]], (2, 1, 2, 2, 0, 0)),
    "right-to-left": ([[(9, 1), (0, 1)], [(3, 1), (3, 4)], [(6, 1), (6, -2)]],
                      [[(9, 1), (6, 1), (3, 1), (0, 1)], [(3, 1), (3, 4)], [(6, 1), (6, -2)]], (2, 1, 2, 2, 0, 0)),
    # a skew edge walked right to left and downward, steeper than 1: x still orders its cuts
    "skew-right-to-left": ([[(3, 9), (0, 0)], [(1, 3), (5, 3)], [(2, 6), (-4, 6)]],
                           [[(3, 9), (2, 6), (1, 3), (0, 0)], [(1, 3), (5, 3)], [(2, 6), (-4, 6)]], (2, 1, 2, 2, 0, 0)),
    # the second edge of a chain is cut: the slots behind it move, the ones before it do not
    "second-edge-of-a-chain": ([[(0, 5), (0, 0), (8, 0), (8, 5)], [(4, 0), (4, 2)]],
                               [[(0, 5), (0, 0), (4, 0), (8, 0), (8, 5)], [(4, 0), (4, 2)]], (1, 1, 1, 1, 0, 0)),
    "partial-overlap": ([[(0, 0), (4, 0)], [(2, 0), (6, 0)]],
                        [[(0, 0), (2, 0), (4, 0)], [(2, 0), (4, 0), (6, 0)]], (2, 2, 1, 1, 0, 0)),
    "partial-overlap-opposite": ([[(0, 0), (4, 2)], [(6, 3), (2, 1)]],
                                 [[(0, 0), (2, 1), (4, 2)], [(6, 3), (4, 2), (2, 1)]], (2, 2, 1, 1, 0, 0)),
    "one-inside-another": ([[(0, 0), (6, 0)], [(4, 0), (2, 0)]],
                           [[(0, 0), (2, 0), (4, 0), (6, 0)], [(4, 0), (2, 0)]], (2, 1, 2, 1, 0, 0)),
    "inside-shared-end": ([[(0, 0), (6, 0)], [(0, 0), (3, 0)]],
                          [[(0, 0), (3, 0), (6, 0)], [(0, 0), (3, 0)]], (1, 1, 1, 1, 0, 0)),
    "equal-only": ([[(1, 1), (3, 2)], [(3, 2), (1, 1)]], [[(1, 1), (3, 2)], [(3, 2), (1, 1)]], (0, 0, 0, 0, 0, 1)),
    "proper-only": ([[(0, 0), (4, 4)], [(0, 4), (4, 0)]], [[(0, 0), (4, 4)], [(0, 4), (4, 0)]], (0, 0, 0, 0, 1, 0)),
    # the crossing point is a third chain's vertex: both edges are cut there and the crossing disappears
    "proper-at-a-vertex": ([[(0, 0), (4, 4)], [(0, 4), (4, 0)], [(2, 2), (2, 6)]],
                           [[(0, 0), (2, 2), (4, 4)], [(0, 4), (2, 2), (4, 0)], [(2, 2), (2, 6)]], (2, 2, 1, 2, 1, 0)),
    # e0 a zero edge, e1 is cut, a one-point chain, e2 the stem, e3 a zero edge on the cut point
    "zero-edge-and-one-point-chain": ([[(0, 0), (0, 0), (4, 0)], [(9, 9)], [(2, 0), (2, 3)], [(2, 0), (2, 0)]],
                                      [[(0, 0), (0, 0), (2, 0), (4, 0)], [(9, 9)], [(2, 0), (2, 3)], [(2, 0), (2, 0)]], (1, 1, 1, 1, 0, 0)),
    # the diagonal of the whole range, cut three units from its start and eight from its end: distances up to 2^47
    "rim": ([[(-L, -L), (L - 1, L - 1)], [(L - 9, L - 9), (L - 9, L - 1)], [(-L + 3, -L + 3), (0, -L)]],
            [[(-L, -L), (-L + 3, -L + 3), (L - 9, L - 9), (L - 1, L - 1)], [(L - 9, L - 9), (L - 9, L - 1)], [(-L + 3, -L + 3), (0, -L)]],
            (2, 1, 2, 2, 0, 0)),
    "rim-vertical": ([[(L - 1, L - 1), (L - 1, -L)], [(L - 1, -L + 1), (0, 0)], [(-L, L - 2), (L - 1, L - 2)]],
                     [[(L - 1, L - 1), (L - 1, L - 2), (L - 1, -L + 1), (L - 1, -L)], [(L - 1, -L + 1), (0, 0)], [(-L, L - 2), (L - 1, L - 2)]],
                     (2, 1, 2, 2, 0, 0)),
    # two squares side by side and a third on top, each missing its neighbours' corner vertices (closed chains)
    "three-squares": ([[(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], [(4, 0), (8, 0), (8, 4), (4, 4), (4, 0)], [(2, 4), (6, 4), (6, 8), (2, 8), (2, 4)]],
                      [[(0, 0), (4, 0), (4, 4), (2, 4), (0, 4), (0, 0)], [(4, 0), (8, 0), (8, 4), (6, 4), (4, 4), (4, 0)],
                       [(2, 4), (4, 4), (6, 4), (6, 8), (2, 8), (2, 4)]], (3, 3, 1, 6, 0, 1)),
    "no-crossing": ([[(0, 0), (4, 0), (4, 4)], [(4, 4), (0, 4), (0, 0)]], [[(0, 0), (4, 0), (4, 4)], [(4, 4), (0, 4), (0, 0)]], (0, 0, 0, 0, 0, 0)),
}
CLOSED = ("three-squares",)  # the hand cases that RJ_NODE_DROP_LAST takes


# ---- brick walls ------------------------------------------------------------------------------------------------------
# (columns, rows, brick width, brick height, shift of the odd rows) -> the written number of cuts
WALLS = {(5, 4, 10, 6, 5): 30, (4, 3, 9, 4, 2): 16, (3, 3, 8, 8, 0): 0}


def brick_rings(cols, rows, w, h, shift, unit=1):
    """-> (ring_row uint32, ring_xy int64 [4 n, 2], ring_face int32): cols x rows rectangles, counter-clockwise, four points
    each, face k + 1 for brick k; the odd rows moved right by shift -- every brick misses its neighbours' corners"""
    xy = []
    for r in range(rows):
        for c in range(cols):
            x0, y0 = c * w + (shift if r % 2 else 0), r * h
            xy += [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]
    n = cols * rows
    return np.arange(0, 4 * n + 1, 4, dtype=np.uint32), np.array(xy, np.int64) * unit, np.arange(1, n + 1, dtype=np.int32)


def closed_chains(ring_row, ring_xy):
    """rings -> closed chains: every ring's first point again at its end (what maps.closed_chains_of_rings does, written
    on its own)"""
    out, row = [], [0]
    for b, e in zip(ring_row[:-1], ring_row[1:]):
        out += [ring_xy[b:e], ring_xy[b:b + 1]]
        row.append(row[-1] + int(e - b) + 1)
    return np.concatenate(out).reshape(-1, 2), np.array(row, np.uint32)


def wall_map(key, unit=1):
    ring_row, ring_xy, _ = brick_rings(*key, unit=unit)
    return closed_chains(ring_row, ring_xy)


# ---- random soups -------------------------------------------------------------------------------------------------------
SOUP_SEEDS = tuple(range(40))


def soup(seed):
    """8 to 14 chains of 1 to 6 random points on a 7 x 7 lattice: touches, overlaps, equal and zero edges, several cuts on
    one edge; odd seeds multiplied out by 2^20 and moved across zero"""
    rng = random.Random(seed)
    chains = [[(rng.randrange(7), rng.randrange(7)) for _ in range(rng.randint(1, 6))] for _ in range(rng.randint(8, 14))]
    unit, off = ((1 << 20), -3 * (1 << 20)) if seed % 2 else (1, 0)
    return chain_arrays([[(x * unit + off, y * unit + off) for x, y in c] for c in chains])


def closed_soup(seed):
    """the soup's chains of two points or more, each closed by its first point: what RJ_NODE_DROP_LAST takes"""
    xy, row = soup(seed)
    chains = [xy[b:e].tolist() for b, e in zip(row[:-1], row[1:]) if e - b >= 2]
    return chain_arrays([[tuple(p) for p in c] + [tuple(c[0])] for c in chains])


# ---- one long edge ------------------------------------------------------------------------------------------------------
def long_edge(n, seed=7):
    """one edge from (0, 0) to (n + 1, 0), walked right to left, and n stems whose foot lies on it, at x = 1 .. n in
    scrambled order; every seventh x has a second stem, downward: the same cut twice.  -> (map, the noded first chain)"""
    rng = random.Random(seed)
    xs = list(range(1, n + 1))
    rng.shuffle(xs)
    chains = [[(n + 1, 0), (0, 0)]]
    for x in xs:
        chains.append([(x, 0), (x, 1 + x % 3)])
        if x % 7 == 0:
            chains.append([(x, -2), (x, 0)])
    return chain_arrays(chains), [(x, 0) for x in range(n + 1, -1, -1)]
