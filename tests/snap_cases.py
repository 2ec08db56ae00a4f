"""Hand-built chain maps for rj_map_snap with the answers written out: the smallest shapes at which each rule of
rayjoin_amd/csrc/rj_snap.h can go wrong (HAND), and the generators of the larger tests: n records, stars through one
half-integer point, one long edge with crossings and T-junctions mixed, random segments, a fan of near-parallel long
edges.  A hand case is (chains, snapped chains, written counts, records): chains a list of point lists, used as they
stand; records None: those of the crossings definition (tests/crossings_ref.py) on the map, else the list to pass; the
written counts are a dict of the rj_snap_counts fields that the case is about."""
import random

from node_cases import L, chain_arrays  # noqa: F401

PROPER, TOUCH, OVERLAP, EQUAL = 1, 2, 3, 4

HAND = {
    "x": ([[(0, 0), (4, 4)], [(0, 4), (4, 0)]],
          [[(0, 0), (2, 2), (4, 4)], [(0, 4), (2, 2), (4, 0)]], dict(n_cuts=2, n_cut_edges=2, n_proper=1, n_exact=1, n_at_end=0), None),
    # the crossing point is (3/2, 3/2): halves go up
    "half": ([[(0, 0), (3, 3)], [(0, 3), (3, 0)]],
             [[(0, 0), (2, 2), (3, 3)], [(0, 3), (2, 2), (3, 0)]], dict(n_cuts=2, n_proper=1, n_exact=0), None),
    # ... whatever the direction of the edges
    "half-reversed": ([[(3, 3), (0, 0)], [(3, 0), (0, 3)]],
                      [[(3, 3), (2, 2), (0, 0)], [(3, 0), (2, 2), (0, 3)]], dict(n_cuts=2, n_proper=1, n_exact=0), None),
    "half-one-reversed": ([[(0, 0), (3, 3)], [(3, 0), (0, 3)]],
                          [[(0, 0), (2, 2), (3, 3)], [(3, 0), (2, 2), (0, 3)]], dict(n_cuts=2, n_proper=1, n_exact=0), None),
    # (-3/2, -3/2): up is toward zero
    "negative-half": ([[(0, 0), (-3, -3)], [(0, -3), (-3, 0)]],
                      [[(0, 0), (-1, -1), (-3, -3)], [(0, -3), (-1, -1), (-3, 0)]], dict(n_cuts=2, n_proper=1, n_exact=0), None),
    # y = 0.4, 0.5, 0.6 on a shallow edge, the last vertical walked downward
    "shallow-ties": ([[(0, 0), (10, 1)], [(4, -2), (4, 3)], [(5, -2), (5, 3)], [(6, 3), (6, -2)]],
                     [[(0, 0), (4, 0), (5, 1), (6, 1), (10, 1)], [(4, -2), (4, 0), (4, 3)], [(5, -2), (5, 1), (5, 3)], [(6, 3), (6, 1), (6, -2)]],
                     dict(n_cuts=6, n_max_cuts=3, n_proper=3, n_exact=0), None),
    # x = 0.4, 0.5, 0.6 on a steep edge: its major axis is y
    "steep": ([[(0, 0), (1, 10)], [(-2, 4), (3, 4)], [(-2, 5), (3, 5)], [(-2, 6), (3, 6)]],
              [[(0, 0), (0, 4), (1, 5), (1, 6), (1, 10)], [(-2, 4), (0, 4), (3, 4)], [(-2, 5), (1, 5), (3, 5)], [(-2, 6), (1, 6), (3, 6)]],
              dict(n_cuts=6, n_max_cuts=3, n_proper=3, n_exact=0), None),
    # one touch and two proper crossings on one edge: the vertex at 2, the rounded points 4 (from 7/2) and 6 (from 11/2)
    "mixed": ([[(0, 0), (8, 0)], [(2, 0), (2, 5)], [(5, -2), (6, 2)], [(3, -1), (4, 1)]],
              [[(0, 0), (2, 0), (4, 0), (6, 0), (8, 0)], [(2, 0), (2, 5)], [(5, -2), (6, 0), (6, 2)], [(3, -1), (4, 0), (4, 1)]],
              dict(n_cuts=5, n_max_cuts=3, n_used=1, n_proper=2, n_exact=0), None),
    # 13/3 goes to 4, 5 is exact; the second chain ends on the third: a touch as well
    "two-to-one-point": ([[(0, 0), (10, 0)], [(4, -1), (5, 2)], [(5, -2), (5, 3)]],
                         [[(0, 0), (4, 0), (5, 0), (10, 0)], [(4, -1), (4, 0), (5, 2)], [(5, -2), (5, 0), (5, 2), (5, 3)]],
                         dict(n_cuts=5, n_used=1, n_proper=2, n_exact=1), None),
    # two rounded points on one edge with the same major offset, 4, and the minor offsets 3 and 4
    "minor-tie": ([[(0, 0), (10, 9)], [(3, 0), (4, 4)], [(3, 0), (5, 6)]],
                  [[(0, 0), (4, 3), (4, 4), (10, 9)], [(3, 0), (4, 3), (4, 4)], [(3, 0), (4, 4), (5, 6)]], dict(n_cuts=4, n_max_cuts=2, n_proper=2), None),
    # ... and the edge walked from its other end: the offsets are taken from (10, 9)
    "minor-tie-reversed": ([[(10, 9), (0, 0)], [(3, 0), (4, 4)], [(3, 0), (5, 6)]],
                           [[(10, 9), (4, 4), (4, 3), (0, 0)], [(3, 0), (4, 3), (4, 4)], [(3, 0), (4, 4), (5, 6)]], dict(n_cuts=4, n_max_cuts=2, n_proper=2),
                           None),
    # products of 2^47 x 2^95: the wide division
    "extreme": ([[(-L, -L), (L - 1, L - 2)], [(-L, L - 1), (L - 1, -L)]],
                [[(-L, -L), (0, -1), (L - 1, L - 2)], [(-L, L - 1), (0, -1), (L - 1, -L)]], dict(n_cuts=2, n_proper=1), None),
    "extreme2": ([[(-L, -L + 1), (L - 1, L - 1)], [(-L + 3, L - 1), (L - 2, -L)]],
                 [[(-L, -L + 1), (0, 0), (L - 1, L - 1)], [(-L + 3, L - 1), (0, 0), (L - 2, -L)]], dict(n_cuts=2, n_proper=1), None),
    # the crossing (3, 9/10) is within half a unit of the second edge's first point: that edge is not cut, the other is
    "at-end": ([[(0, 0), (10, 3)], [(3, 1), (3, -4)]],
               [[(0, 0), (3, 1), (10, 3)], [(3, 1), (3, -4)]], dict(n_cuts=1, n_cut_edges=1, n_proper=1, n_at_end=1, n_exact=0), None),
    # a ring that crosses itself
    "bow-tie": ([[(0, 0), (4, 4), (4, 0), (0, 4), (0, 0)]],
                [[(0, 0), (2, 2), (4, 4), (4, 0), (2, 2), (0, 4), (0, 0)]], dict(n_cuts=2, n_cut_edges=2, n_proper=1, n_exact=1), None),
    # records of kind PROPER that do not fit: parallel edges (den == 0); a T (un == 0); edges far apart
    "stale-parallel": ([[(0, 0), (4, 0)], [(0, 2), (4, 2)]], [[(0, 0), (4, 0)], [(0, 2), (4, 2)]],
                       dict(n_cuts=0, n_proper=1, n_stale=1, n_exact=0, n_at_end=0), [(0, 1, PROPER)]),
    "stale-t": ([[(0, 0), (4, 0)], [(2, 0), (2, 3)]], [[(0, 0), (4, 0)], [(2, 0), (2, 3)]],
                dict(n_cuts=0, n_proper=1, n_stale=1, n_exact=0, n_at_end=0), [(0, 1, PROPER)]),
    "stale-apart": ([[(0, 0), (4, 4)], [(10, 4), (14, 0)]], [[(0, 0), (4, 4)], [(10, 4), (14, 0)]],
                    dict(n_cuts=0, n_proper=1, n_stale=1, n_exact=0, n_at_end=0), [(0, 1, PROPER)]),
    # a touch recorded as a proper crossing and a proper crossing recorded as a touch: neither cuts
    "wrong-kinds": ([[(0, 0), (4, 0)], [(2, 0), (2, 3)], [(5, 5), (9, 9)], [(5, 9), (9, 5)]],
                    [[(0, 0), (4, 0)], [(2, 0), (2, 3)], [(5, 5), (9, 9)], [(5, 9), (9, 5)]],
                    dict(n_cuts=0, n_used=1, n_proper=1, n_stale=1), [(0, 1, PROPER), (2, 3, TOUCH)]),
    "no-crossing": ([[(0, 0), (4, 0), (4, 4)], [(4, 4), (0, 4), (0, 0)]], [[(0, 0), (4, 0), (4, 4)], [(4, 4), (0, 4), (0, 0)]], dict(n_cuts=0), None),
}
CLOSED = ("bow-tie",)  # the hand cases that RJ_SNAP_DROP_LAST takes

TWO_SQUARES = [[(0, 0), (4, 0), (4, 4), (0, 4)], [(2, 2), (6, 2), (6, 6), (2, 6)]]  # rings; 3 bounded faces of area2 24, 8, 24
THREE_TRIANGLES = [[(0, 0), (9, 0), (4, 8)], [(3, -2), (12, 3), (5, 5)], [(1, 3), (10, -1), (8, 7)]]  # rings that cross each other


# ---- the device's grain -----------------------------------------------------------------------------------------------
RECORD_COUNTS = (63, 64, 65)


def comb(n):
    """one edge from (0, 0) to (3 n + 1, 1) and n verticals across it, at x = 3 k + 1: n records, all proper"""
    return chain_arrays([[(0, 0), (3 * n + 1, 1)]] + [[(3 * k + 1, -2), (3 * k + 1, 3)] for k in range(n)])


STARS = (65, 129)


def star(k):
    """k edges through the point (1/2, 1/2), every one from (i - 70, -100) to its mirror image: k (k - 1) / 2 proper
    crossings that all round to (1, 1) -- every edge gets k - 1 equal cuts, one of which stays"""
    return chain_arrays([[(i - 70, -100), (71 - i, 101)] for i in range(k)])


def long_mixed(n, seed=11):
    """one edge from (4 n + 4, 0) to (0, 0), walked right to left; n skew edges across it whose crossing points
    (4 k + 4/3, 0) round to (4 k + 1, 0), and n stems whose foot lies on it at (4 k + 3, 0), in scrambled order; every
    seventh crossing has a stem at its rounded point as well: one point from a vertex and from a rounded crossing.
    -> (map, the snapped first chain)"""
    rng = random.Random(seed)
    ks = list(range(n))
    rng.shuffle(ks)
    chains = [[(4 * n + 4, 0), (0, 0)]]
    for k in ks:
        chains.append([(4 * k + 1, -1), (4 * k + 2, 2)])
        chains.append([(4 * k + 3, 0), (4 * k + 3, 1 + k % 3)])
        if k % 7 == 0:
            chains.append([(4 * k + 1, 4), (4 * k + 1, 0)])
    want = [(4 * n + 4, 0)] + [(x, 0) for k in range(n - 1, -1, -1) for x in (4 * k + 3, 4 * k + 1)] + [(0, 0)]
    return chain_arrays(chains), want


# ---- random maps --------------------------------------------------------------------------------------------------------
SEGMENT_SEEDS = tuple(range(20))


def random_segments(seed, n=40, box=40):
    """n chains of one random edge each in a box of `box` units: mostly proper crossings, many per edge"""
    rng = random.Random(1000 + seed)
    chains = []
    while len(chains) < n:
        a, b = (rng.randrange(box), rng.randrange(box)), (rng.randrange(box), rng.randrange(box))
        if a != b:
            chains.append([a, b])
    return chain_arrays(chains)


def fan(n=30, seed=3):
    """n edges from x = 0 to x = 96 with end heights in 0..11: near-parallel long edges whose crossings keep making new
    ones -- the input on which the rounds converge slowly (seed 3: 14 cutting rounds by tests/snap_ref.py)"""
    rng = random.Random(seed)
    return chain_arrays([[(0, rng.randrange(12)), (96, rng.randrange(12))] for _ in range(n)])
