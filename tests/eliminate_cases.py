"""Hand-built labelled chain maps for rj_map_eliminate with the answers written out: the smallest shapes at which each
rule of rayjoin_amd/csrc/rj_eliminate.h can go wrong (HAND), the edges whose lengths sit at a square (SQRT_EDGES), and
the generators of the structural maps (chains of 1 .. 1 000 points, 300 two-point chains in a row).

A hand case is (map, tol, faces, n_mutual, n_dropped): map the four arrays of rings_cases.chain_map; faces a dict
label -> (target, best, flags, area2), written by hand; n_dropped the chains that RJ_ELIM_DROP leaves out.

Most maps come from grid_map: rectangles cut by the lines x = xs[i], y = ys[j], labels[j][i] the face of the cell with
its lower left corner at (xs[i], ys[j]) (row 0 is the bottom one), 0 outside; one two-point chain per cell edge whose
two sides differ, vertical ones walked up (left = the cell to the west), horizontal ones walked to the right (left = the
cell to the north)."""
import numpy as np

from rings_cases import chain_map

LIM = 1 << 46
HUGE = (1 << 128) - 1
SIDE = (1 << 47) - 1
SLIVER, ELIMINATED, ISLAND, NEGATIVE = 1, 2, 4, 8


def grid_chains(xs, ys, labels):
    W, H = len(xs) - 1, len(ys) - 1
    assert len(labels) == H and all(len(r) == W for r in labels)
    at = lambda i, j: labels[j][i] if 0 <= i < W and 0 <= j < H else 0  # noqa: E731
    chains = []
    for i in range(W + 1):
        for j in range(H):
            if at(i - 1, j) != at(i, j):
                chains.append(([(xs[i], ys[j]), (xs[i], ys[j + 1])], at(i - 1, j), at(i, j)))
    for j in range(H + 1):
        for i in range(W):
            if at(i, j) != at(i, j - 1):
                chains.append(([(xs[i], ys[j]), (xs[i + 1], ys[j])], at(i, j), at(i, j - 1)))
    return chains


def grid_map(xs, ys, labels, extra=()):
    return chain_map(grid_chains(xs, ys, labels) + list(extra))


def swapped_outside(chains, face):
    """the chains between `face` and face 0 with their two labels exchanged: inconsistent labels"""
    return [(p, ri, le) if {le, ri} == {face, 0} else (p, le, ri) for p, le, ri in chains]


LONGER = grid_map([0, 10, 11, 21], [0, 10, 20], [[1, 3, 2], [1, 2, 2]])  # 3: 10 against face 1, 10 + 1 against face 2
ROW3 = grid_map([0, 1, 2, 3, 103], [0, 10, 20, 30, 40], [[2, 3, 4, 5], [0, 3, 4, 5], [0, 0, 4, 5], [0, 0, 0, 5]])
HOLE = grid_map([0, 10, 11, 21], [0, 10, 11, 21], [[1, 1, 1], [1, 3, 1], [1, 1, 1]],
                extra=[([(2, 2), (5, 5), (8, 2)], 1, 1), ([(10, 10), (11, 11)], 3, 3)])  # a dangle in face 1, a diagonal inside the hole
TWO_PART = grid_map([0, 10, 11, 21, 22], [0, 10], [[1, 3, 2, 3]])
ZERO_LENGTH = grid_map([0, 1, 100, 110], [0, 10], [[3, 0, 5]], extra=[([(0, 0), (0, 0)], 3, 5)])
ZERO_AREA = grid_map([0, 1], [0, 10], [[3]], extra=[([(0, 0), (0, 0)], 3, 9)])
BIG = chain_map([([(-LIM, -LIM), (LIM - 1, -LIM), (LIM - 1, LIM - 1), (-LIM, -LIM)], 1, 0)])  # area2 = SIDE^2 = 2^94 - 2^48 + 1


def between(a, s, b):
    """a sliver s (1 x 10) between the squares a and b: both borders are 10 long"""
    return grid_map([0, 10, 11, 21], [0, 10], [[a, s, b]])


def mutual(top):
    """the strips 3 (100 x 1) and 4 (100 x top) on each other, face 1 at their short ends"""
    return grid_map([-500, 0, 100], [0, 1, 1 + top], [[1, 3], [1, 4]])


HAND = {
    "longer-border": (LONGER, 20, {1: (1, 1, 0, 400), 2: (2, 2, 0, 420), 3: (2, 2, SLIVER | ELIMINATED, 20)}, 0, 2),
    "below-tol": (LONGER, 19, {1: (1, 1, 0, 400), 2: (2, 2, 0, 420), 3: (3, 3, 0, 20)}, 0, 0),
    # (1, 3) against (2, 3): the smaller min
    "equal-borders": (between(1, 3, 2), 20, {1: (1, 1, 0, 200), 2: (2, 2, 0, 200), 3: (1, 1, SLIVER | ELIMINATED, 20)}, 0, 1),
    # (3, -5) against (3, 7): equal min, and -5 is 2^32 - 5: the smaller max is 7
    "equal-borders-negative-label": (between(-5, 3, 7), 20, {3: (7, 7, SLIVER | ELIMINATED, 20), 7: (7, 7, 0, 200), -5: (-5, -5, 0, 200)}, 0, 1),
    # (9, -5) against (7, 9): the smaller min is 7
    "equal-borders-sliver-in-the-middle": (between(-5, 9, 7), 20, {7: (7, 7, 0, 200), 9: (7, 7, SLIVER | ELIMINATED, 20), -5: (-5, -5, 0, 200)}, 0, 1),
    "mutual-larger-stays": (mutual(2), 400, {1: (1, 1, 0, 3000), 3: (4, 4, SLIVER | ELIMINATED, 200), 4: (4, 3, SLIVER, 400)}, 1, 1),
    "mutual-equal-area": (mutual(1), 200, {1: (1, 1, 0, 2000), 3: (3, 4, SLIVER, 200), 4: (3, 3, SLIVER | ELIMINATED, 200)}, 1, 1),
    # best: 2 -> 3 -> 4 -> 5 (borders of 10, 20, 30): face 2 is three steps from its root
    "row-of-three": (ROW3, 60, {2: (5, 3, SLIVER | ELIMINATED, 20), 3: (5, 4, SLIVER | ELIMINATED, 40), 4: (5, 5, SLIVER | ELIMINATED, 60),
                                5: (5, 5, 0, 8000)}, 0, 6),
    "row-of-three-tighter": (ROW3, 59, {2: (4, 3, SLIVER | ELIMINATED, 20), 3: (4, 4, SLIVER | ELIMINATED, 40), 4: (4, 4, 0, 60), 5: (5, 5, 0, 8000)}, 0, 3),
    "island": (grid_map([0, 1], [0, 10], [[7]]), 20, {7: (7, 7, SLIVER | ISLAND, 20)}, 0, 0),
    "touches-zero-and-one": (grid_map([0, 10, 11], [0, 10], [[1, 3]]), 20, {1: (1, 1, 0, 200), 3: (1, 1, SLIVER | ELIMINATED, 20)}, 0, 1),
    # the hole's ring goes; the two dangles came with left == right and stay
    "hole-and-dangles": (HOLE, 2, {1: (1, 1, 0, 880), 3: (1, 1, SLIVER | ELIMINATED, 2)}, 0, 4),
    "two-part-below": (TWO_PART, 39, {1: (1, 1, 0, 200), 2: (2, 2, 0, 200), 3: (3, 3, 0, 40)}, 0, 0),
    "two-part-at": (TWO_PART, 40, {1: (1, 1, 0, 200), 2: (2, 2, 0, 200), 3: (2, 2, SLIVER | ELIMINATED, 40)}, 0, 2),
    # face 4's outer border with its labels exchanged: -210 from it, -10 from the border with face 3
    "swapped-labels": (chain_map(swapped_outside(grid_chains([0, 1, 11], [0, 10], [[3, 4]]), 4)), 20,
                       {3: (4, 4, SLIVER | ELIMINATED, 20), 4: (4, 4, NEGATIVE, -220)}, 0, 1),
    "swapped-labels-huge": (chain_map(swapped_outside(grid_chains([0, 1, 11], [0, 10], [[3, 4]]), 4)), HUGE,
                            {3: (4, 4, SLIVER | ELIMINATED, 20), 4: (4, 4, NEGATIVE, -220)}, 0, 1),
    "zero-length-neighbour": (ZERO_LENGTH, 20, {3: (5, 5, SLIVER | ELIMINATED, 20), 5: (5, 5, 0, 200)}, 0, 1),
    # tol = 0: face 9 has no area at all
    "tol-zero": (ZERO_AREA, 0, {3: (3, 3, 0, 20), 9: (3, 3, SLIVER | ELIMINATED, 0)}, 0, 1),
    "tol-zero-nothing": (LONGER, 0, {1: (1, 1, 0, 400), 2: (2, 2, 0, 420), 3: (3, 3, 0, 20)}, 0, 0),
    # everything is a sliver: best(1) = 2 ((1, 2) and (1, 3) weigh 10: the smaller max), 2 and 3 choose each other
    "tol-huge": (LONGER, HUGE, {1: (2, 2, SLIVER | ELIMINATED, 400), 2: (2, 3, SLIVER, 420), 3: (2, 2, SLIVER | ELIMINATED, 20)}, 1, 4),
    # no face 0: the outside is face 2, its area is negative, it is never a sliver and always a target -- the map's one chain goes
    "all-dropped": (chain_map([([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], 1, 2)]), 1000,
                    {1: (2, 2, SLIVER | ELIMINATED, 200), 2: (2, 2, NEGATIVE, -200)}, 0, 1),
    "high-word-below": (BIG, SIDE * SIDE - 1, {1: (1, 1, 0, SIDE * SIDE)}, 0, 0),
    "high-word-at": (BIG, SIDE * SIDE, {1: (1, 1, SLIVER | ISLAND, SIDE * SIDE)}, 0, 0),
}

# ---- lengths at a square: (dx, dy, floor(sqrt(dx^2 + dy^2))) -------------------------------------------------------------
M = (1 << 23) - 1
K = 2 * M * M + 1  # 2^47 - 2^25 + 3; (K - 1)^2 + (2 M)^2 = K^2 - 1
SQRT_EDGES = [(K, 0, K), (K, 1, K), (K - 1, 2 * M, K - 1), (SIDE, 0, SIDE), (SIDE, 1, SIDE), (0, SIDE, SIDE), (3, 4, 5), (1, 1, 1), (0, 0, 0),
              (SIDE, SIDE, 199032864766428)]  # floor(sqrt(2) (2^47 - 1)): 2 SIDE^2 lies between its square and the next
assert (K - 1) ** 2 + (2 * M) ** 2 == K * K - 1 and 199032864766428 ** 2 <= 2 * SIDE * SIDE < 199032864766429 ** 2


def sqrt_map():
    """one two-point chain per edge of SQRT_EDGES, every one from the corner (-2^46, -2^46)"""
    return chain_map([([(-LIM, -LIM), (-LIM + dx, -LIM + dy)], k + 1, 0) for k, (dx, dy, _) in enumerate(SQRT_EDGES)])


# ---- structure: what a wave and a block can get wrong ---------------------------------------------------------------------
def lengths_map(lengths=(1, 2, 63, 64, 65, 66, 1000), seed=7, span=1 << 40):
    """chains of the given numbers of points, random points of 40 bits, the faces 1 .. 4 and 0 in turn"""
    rng = np.random.default_rng(seed)
    chains = []
    for k, n in enumerate(lengths):
        pts = rng.integers(-span, span, size=(n, 2))
        chains.append(([tuple(p) for p in pts.tolist()], 1 + k % 4, (k + 2) % 5))
    return chain_map(chains)


def two_point_row(n=300, seed=9):
    """n two-point chains in a row (many chains in one wave) between three chains of 70, 1 and 130 points: the labels
    cycle through 1 .. 7, so every face is the sum of many chains"""
    rng = np.random.default_rng(seed)
    chains = [([tuple(p) for p in rng.integers(-1000, 1000, size=(70, 2)).tolist()], 1, 2), ([(5, 5)], 3, 0)]
    for k in range(n):
        a = rng.integers(-(1 << 45), 1 << 45, size=(2, 2))
        chains.append(([tuple(p) for p in a.tolist()], 1 + k % 7, 1 + (k * 3 + 1) % 7))
    chains.append(([tuple(p) for p in rng.integers(-1000, 1000, size=(130, 2)).tolist()], 7, 0))
    return chain_map(chains)
