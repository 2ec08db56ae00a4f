"""Hand-built chain maps for rj_map_simplify with the answers written out: the smallest shapes at which each rule of
rayjoin_amd/csrc/rj_simplify.h can go wrong (HAND), and the generators of the larger tests: random maps of open and
closed chains on a small lattice (ties abound), one long chain, a run of collinear points, the staircase that loses
one point per round.  A hand case is (chains, tol, kept, (n_rounds, n_closed, n_pinned_extra)): chains a list of point
lists, used as they stand; kept the input points of the output, in order."""
import random

import numpy as np

L = 1 << 46
HUGE = (1 << 128) - 1
SIDE = (1 << 47) - 1
BIG = [[(-L, -L), (L - 1, -L), (L - 1, L - 1)]]  # the weight of its middle point is SIDE^2, just below 2^94
SQUARE = [[(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]]
SQUARE9 = [[(0, 0), (5, 0), (10, 0), (10, 5), (10, 10), (5, 10), (0, 10), (0, 5), (0, 0)]]


def chain_arrays(chains):
    xy = [p for c in chains for p in c]
    row = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    return np.array(xy, np.int64).reshape(-1, 2), row


def collinear(n):
    return [[(3 * i, -2 * i) for i in range(n)]]


def staircase(n):
    """x = i, y = i^2 for odd i and 0 for even i: every weight differs and only the least can go, one point per round"""
    return [[(i, i * i if i % 2 else 0) for i in range(n)]]


HAND = {
    # |cross((5, 1), (10, 0))| = 10
    "peak-below": ([[(0, 0), (5, 1), (10, 0)]], 9, [0, 1, 2], (0, 0, 0)),
    "peak-at": ([[(0, 0), (5, 1), (10, 0)]], 10, [0, 2], (1, 0, 0)),
    # m1 = 2 (the far corner); m2: 1 and 3 tie at 100, the lower index wins
    "square": (SQUARE, HUGE, [0, 1, 2, 4], (1, 1, 2)),
    "square-mid-zero": (SQUARE9, 0, [0, 2, 4, 6, 8], (1, 1, 2)),
    # m1 = 4, m2 = 2 (tie with 6); 1, 3, 5, 7 go first (weight 0 against 6's 25), then 6
    "square-mid-huge": (SQUARE9, HUGE, [0, 2, 4, 8], (2, 1, 2)),
    # a ring a -> b -> a: m1 = b, no m2 (every cross product is 0)
    "there-and-back": ([[(0, 0), (4, 0), (0, 0)]], HUGE, [0, 1, 2], (0, 1, 1)),
    # a ring of one place: no m1
    "ring-of-one-place": ([[(3, 3), (3, 3), (3, 3), (3, 3)]], HUGE, [0, 3], (2, 1, 0)),
    "line-then-off": ([[(i, 2 * i) for i in range(8)] + [(9, 9)]], 0, [0, 7, 8], (4, 0, 0)),
    "collinear-100": (collinear(100), 0, [0, 99], (9, 0, 0)),
    "staircase-200": (staircase(200), HUGE, [0, 199], (198, 0, 0)),
    # (2, 0), (4, 0) lie on the line through (0, 0) and (6, 0), but they end their chains
    "chain-boundary": ([[(0, 0), (2, 0)], [(4, 0), (6, 0)]], HUGE, [0, 1, 2, 3], (0, 0, 0)),
    "chain-boundary-closed": ([[(0, 0), (2, 0), (1, 1), (0, 0)], [(0, 0), (2, 0)], [(4, 0), (6, 0), (8, 0)]], 0, [0, 1, 2, 3, 4, 5, 6, 8],
                              (1, 1, 2)),
    "one-point-chains": ([[(0, 0), (1, 0), (2, 0)], [(5, 5)], [(7, 7)], [(3, 0), (4, 0), (5, 0)]], 0, [0, 2, 3, 4, 5, 7], (1, 0, 0)),
    "vertical-and-right-to-left": ([[(1, 0), (1, 4), (1, 9)], [(9, 1), (5, 1), (0, 1)]], 0, [0, 2, 3, 5], (1, 0, 0)),
    "negative-below": ([[(-10, -10), (-5, -9), (0, -10)]], 9, [0, 1, 2], (0, 0, 0)),
    "negative-at": ([[(-10, -10), (-5, -9), (0, -10)]], 10, [0, 2], (1, 0, 0)),
    # clockwise: the cross product is negative, the weight is not
    "clockwise": ([[(0, 0), (5, -1), (10, 0)], [(0, 0), (5, 1), (10, 0)]], 9, [0, 1, 2, 3, 4, 5], (0, 0, 0)),
    # SIDE^2 = 2^94 - 2^48 + 1: its high word decides
    "big-below": (BIG, SIDE * SIDE - 1, [0, 1, 2], (0, 0, 0)),
    "big-at": (BIG, SIDE * SIDE, [0, 2], (1, 0, 0)),
    "big-low-word-only": (BIG, (SIDE * SIDE) % (1 << 64), [0, 1, 2], (0, 0, 0)),
    "big-high-word-only": (BIG, (SIDE * SIDE >> 64) << 64, [0, 1, 2], (0, 0, 0)),
    "big-high-word-above": (BIG, ((SIDE * SIDE >> 64) + 1) << 64, [0, 2], (1, 0, 0)),
    # the weights of 1, 2, 3 are all 2; the hashes order them 2 < 1 < 3: 2 goes, then 1 (its weight is 2 again, as 3's
    # is, and its hash is lower); 3 then weighs 4
    "equal-weights": ([[(0, 0), (1, 1), (2, 0), (3, 1), (4, 0)]], 2, [0, 3, 4], (2, 0, 0)),
    # weights 5, 10, 5: 1 and 3 go together, 2 loses both neighbours and then weighs 20
    "both-neighbours-go": ([[(0, 0), (1, 0), (2, 5), (3, 0), (4, 0)]], 10, [0, 2, 4], (1, 0, 0)),
    # a spike a -> b -> a' inside a chain has weight 0; behind it a' follows a: both weigh 0, the lower hash (point 1) goes
    "spike": ([[(0, 0), (4, 0), (9, 3), (4, 0), (4, 7)]], 0, [0, 3, 4], (2, 0, 0)),
}

SEEDS = list(range(40))


def random_map(seed):
    """-> (xy, row_index): 3..9 chains of 1..400 points (most short), open and closed, on a lattice of 4..40 a side"""
    rng = random.Random(9000 + seed)
    side = rng.choice((4, 7, 12, 40))
    chains = []
    for _ in range(rng.randint(3, 9)):
        n = rng.choice((1, 2, 3, rng.randint(4, 12), rng.randint(13, 70), rng.randint(71, 400)))
        pts = [(rng.randint(-side, side), rng.randint(-side, side)) for _ in range(n)]
        if n >= 3 and rng.random() < 0.5:
            kind = rng.random()
            if kind < 0.15:
                pts = [pts[0]] * n  # a ring of one place
            elif kind < 0.3:
                pts = [pts[0] if i % 2 == 0 else pts[1] for i in range(n | 1)]  # a -> b -> a -> ...
            pts[-1] = pts[0]
        elif n >= 8 and rng.random() < 0.4:  # a collinear run inside
            k = rng.randint(0, n - 6)
            for i in range(5):
                pts[k + i] = (pts[k][0] + i, pts[k][1] - 2 * i)
        chains.append(pts)
    return chain_arrays(chains)


def tols(seed):
    return [0, HUGE] + [random.Random(seed).choice((1, 2, 5, 17, 60, 400, 3000))]


def long_chain(n, seed=7):
    """one chain of n points: a random walk with collinear stretches"""
    rng = random.Random(seed)
    pts, x, y = [], 0, 0
    while len(pts) < n:
        dx, dy = rng.randint(0, 3), rng.randint(-3, 3)
        for _ in range(rng.choice((1, 1, 1, 2, 6))):
            pts.append((x, y))
            x, y = x + dx, y + dy
    return chain_arrays([pts[:n]])
