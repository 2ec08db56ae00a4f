"""Chain maps for the dissolve tests (tests/test_dissolve.py, tests/test_gpu_dissolve.py) with the answers written out by
hand or built from the construction itself, never from tests/dissolve_ref.py.

A case is a dict: map (xy, row_index, left, right), classes (None: identity, else the table), flags, and the answer:
chains [(points, left, right)] in output order, origin, chain_out (per input chain), counts (the ones stated), records
{label: (n_sides, area2)} or None where the construction does not state them, or unmapped = n for a refused call.

HAND           small maps, one rule each
constructed()  maps that cross a wave and a block: paths, loops, pairs of long chains, rings_planar.long_chains()"""
import functools

import numpy as np

import rings_planar as RP
from rings_cases import chain_map

KEEP_EQUAL = 1
NONE = 0xFFFFFFFF

# two squares side by side: face 1 = [0, 10] x [0, 10], face 2 = [10, 20] x [0, 10]
SQ_A = [(10, 0), (0, 0), (0, 10), (10, 10)]    # clockwise round face 1: (0, 1)
SQ_MID = [(10, 0), (10, 10)]                   # upwards: (1, 2)
SQ_B = [(10, 0), (20, 0), (20, 10), (10, 10)]  # counter-clockwise round face 2: (2, 0)
SQUARES = chain_map([(SQ_A, 0, 1), (SQ_MID, 1, 2), (SQ_B, 2, 0)])
TRIANGLE = [(0, 0), (10, 0), (0, 10), (0, 0)]
BOX = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]


def case(m, chains, origin, chain_out, classes=None, flags=0, records=None, **counts):
    return dict(map=m, classes=None if classes is None else np.array(classes, np.int32), flags=flags, chains=chains, origin=origin, chain_out=chain_out,
                counts=counts, records=records, unmapped=0)


HAND = {
    # the border goes, the two outlines become one closed chain read from chain 0's first point; chain 2 runs backwards in it
    "squares-equal": case(SQUARES, [(SQ_A[:-1] + SQ_B[::-1], 0, 7)], [0], [0, NONE, 1], classes=[0, 7, 7], records={7: (2, 400)},
                          n_kept=2, n_dropped=1, n_skipped=0, n_chains=1, n_points=7, n_closed=1, n_classes=1),
    # three half-chains start at (10, 0) and at (10, 10): nothing joins
    "squares-different": case(SQUARES, [(SQ_A, 0, 1), (SQ_MID, 1, 2), (SQ_B, 2, 0)], [0, 1, 2], [0, 2, 4], records={1: (2, 200), 2: (2, 200)},
                              n_kept=3, n_dropped=0, n_chains=3, n_points=10, n_closed=0, n_classes=2),
    # (10, 0) has degree 2 and a change of classes: no join; (20, 0) has degree 2 and none: a join
    "class-change": case(chain_map([([(0, 0), (10, 0)], 1, 0), ([(10, 0), (20, 0)], 2, 0), ([(20, 0), (30, 0)], 2, 0)]),
                         [([(0, 0), (10, 0)], 1, 0), ([(10, 0), (20, 0), (30, 0)], 2, 0)], [0, 1], [0, 2, 2], records={1: (1, 0), 2: (2, 0)},
                         n_kept=3, n_chains=2, n_points=5, n_closed=0, n_classes=2),
    # a stem with both classes 1 at the vertex between two chains of classes (1, 0): kept, it makes a junction ...
    "t-junction": case(chain_map([([(0, 0), (10, 0)], 1, 0), ([(10, 0), (20, 0)], 1, 0), ([(10, 0), (10, 10)], 1, 1)]),
                       [([(0, 0), (10, 0)], 1, 0), ([(10, 0), (20, 0)], 1, 0), ([(10, 0), (10, 10)], 1, 1)], [0, 1, 2], [0, 2, 4], flags=KEEP_EQUAL,
                       records={1: (4, 0)}, n_kept=3, n_dropped=0, n_chains=3, n_points=6, n_closed=0, n_classes=1),
    # ... dropped, it leaves a vertex of degree 2
    "t-junction-dissolved": case(chain_map([([(0, 0), (10, 0)], 1, 0), ([(10, 0), (20, 0)], 1, 0), ([(10, 0), (10, 10)], 1, 1)]),
                                 [([(0, 0), (10, 0), (20, 0)], 1, 0)], [0], [0, 0, NONE], records={1: (2, 0)},
                                 n_kept=2, n_dropped=1, n_chains=1, n_points=3, n_closed=0, n_classes=1),
    "closed-alone": case(chain_map([(TRIANGLE, 1, 0)]), [(TRIANGLE, 1, 0)], [0], [0], records={1: (1, 100)},
                         n_kept=1, n_chains=1, n_points=4, n_closed=1, n_classes=1),
    # bottom and right side counter-clockwise (1, 0), left side and top clockwise (0, 1): one loop, chain 1 backwards
    "loop-of-two": case(chain_map([([(0, 0), (10, 0), (10, 10)], 1, 0), ([(0, 0), (0, 10), (10, 10)], 0, 1)]),
                        [([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], 1, 0)], [0], [0, 1], records={1: (2, 200)},
                        n_kept=2, n_chains=1, n_points=5, n_closed=1, n_classes=1),
    # a dangle at the closed chain's own vertex goes with the borders: the chain is alone there, a closed walk ...
    "dangle": case(chain_map([(BOX, 1, 0), ([(0, 0), (5, 5)], 1, 1)]), [(BOX, 1, 0)], [0], [0, NONE], records={1: (1, 200)},
                   n_kept=1, n_dropped=1, n_chains=1, n_points=5, n_closed=1, n_classes=1),
    # ... kept, three half-chains start at (0, 0): the same points, but an open walk that ends where it began
    "dangle-kept": case(chain_map([(BOX, 1, 0), ([(0, 0), (5, 5)], 1, 1)]), [(BOX, 1, 0), ([(0, 0), (5, 5)], 1, 1)], [0, 1], [0, 2], flags=KEEP_EQUAL,
                        records={1: (3, 200)}, n_kept=2, n_dropped=0, n_chains=2, n_points=7, n_closed=0, n_classes=1),
    # a one-point chain and an all-equal chain at the vertices of the others: skipped, they make no junction and no class
    "skipped": case(chain_map([([(0, 0)], 5, 0), ([(1, 0), (1, 0), (1, 0)], 2, 0), ([(0, 0), (1, 0)], 1, 0), ([(1, 0), (2, 0)], 1, 0)]),
                    [([(0, 0), (1, 0), (2, 0)], 1, 0)], [2], [NONE, NONE, 0, 0], records={1: (2, 0)},
                    n_kept=2, n_dropped=0, n_skipped=2, n_chains=1, n_points=3, n_closed=0, n_classes=1),
    # face 1 erased into the outside: its outline goes, the border and the outline of face 2 close a loop from chain 1
    "face-to-zero": case(SQUARES, [(SQ_MID[:1] + SQ_B[::-1], 0, 3)], [1], [NONE, 0, 1], classes=[0, 0, 3], records={3: (2, 200)},
                         n_kept=2, n_dropped=1, n_chains=1, n_points=5, n_closed=1, n_classes=1),
    "all-dissolve": case(SQUARES, [], [], [NONE, NONE, NONE], classes=[0, 0, 0], records={},
                         n_kept=0, n_dropped=3, n_chains=0, n_points=0, n_closed=0, n_classes=0),
    # repeated points inside a chain stay; labels outside [0, 2^31) are classes like any other without a table
    "verbatim": case(chain_map([([(0, 0), (0, 0), (5, 0), (5, 0)], -1, -(1 << 31)), ([(9, 0), (5, 0)], -(1 << 31), -1)]),
                     [([(0, 0), (0, 0), (5, 0), (5, 0), (9, 0)], -1, -(1 << 31))], [0], [0, 1], records={-(1 << 31): (2, 0), -1: (2, 0)},
                     n_kept=2, n_chains=1, n_points=5, n_closed=0, n_classes=2),
}
# label 2 lies outside a table of two entries: chain 1's right side and chain 2's left side; so does every negative label
HAND["unmapped"] = dict(case(SQUARES, [], [], [], classes=[0, 7]), unmapped=2)
HAND["unmapped-negative"] = dict(case(chain_map([(TRIANGLE, -4, 1)]), [], [], [], classes=[0, 7, 7, 7, 7]), unmapped=1)


# ---- constructed maps --------------------------------------------------------------------------------------------------
PATH_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
LOOP_SIZES = (2, 3, 64, 65, 1000)
PAIR_SIZES = (2, 63, 64, 65, 66, 257, 1000)


def path_case(n):
    """rings_planar.path(n) under KEEP_EQUAL: one chain of n + 1 points from chain 0's first point"""
    V = [(k, (k * 37) % 11) for k in range(n + 1)]
    return case(RP.path(n), [(V, 0, 0)], [0], [int(k % 3 == 1) for k in range(n)], flags=KEEP_EQUAL, n_kept=n, n_chains=1, n_points=n + 1, n_closed=0)


def loop_case(n, seed=0):
    """n two-point chains round a polygon with face 1 inside, digitised at random, in shuffled file order: one closed chain
    from the first point of file chain 0 in that chain's direction"""
    rng = np.random.default_rng(seed + n)
    ang = 2.0 * np.pi * np.arange(n) / n
    P = [(int(round(1e6 * np.cos(a))), int(round(1e6 * np.sin(a)))) for a in ang]
    assert len(set(P)) == n
    back = rng.random(n) < 0.5
    order = rng.permutation(n).tolist()
    chains = [([P[(e + 1) % n], P[e]], 0, 1) if back[e] else ([P[e], P[(e + 1) % n]], 1, 0) for e in order]
    e0 = order[0]
    if back[e0]:
        pts, le, ri = [P[(e0 + 1 - k) % n] for k in range(n + 1)], 0, 1
    else:
        pts, le, ri = [P[(e0 + k) % n] for k in range(n + 1)], 1, 0
    where = {e: f for f, e in enumerate(order)}
    out = [0] * n
    for e in range(n):
        out[where[e]] = 1 if bool(back[e]) != bool(back[e0]) else 0
    return case(chain_map(chains), [(pts, le, ri)], [0], out, n_kept=n, n_dropped=0, n_chains=1, n_points=n + 1, n_closed=1, n_classes=1)


def pair_case(m):
    """two chains of m points that both START at (0, 0) and two that both END at (0, 100): each pair is one chain, its
    first member backwards in the first pair and its second member backwards in the second"""
    a = [(-k, (3 * k) % 5) for k in range(m)]
    b = [(k, (2 * k) % 7) for k in range(m)]
    c = [(-(m - 1 - k), 100 + (3 * (m - 1 - k)) % 5) for k in range(m)]
    d = [(m - 1 - k, 100 + (2 * (m - 1 - k)) % 7) for k in range(m)]
    chains = [(a, 1, 0), (b, 0, 1), (c, 1, 0), (d, 0, 1)]
    want = [(a[::-1] + b[1:], 0, 1), (c + d[::-1][1:], 1, 0)]
    return case(chain_map(chains), want, [0, 2], [1, 0, 2, 3], n_kept=4, n_chains=2, n_points=2 * (2 * m - 1), n_closed=0, n_classes=1)


def long_case(keep_equal):
    """rings_planar.long_chains(): dropped, the hanging chain leaves the outer chain alone at its vertex (a closed walk);
    kept, it makes a junction there.  The points come out as they went in"""
    m = RP.long_chains()
    xy, row, left, right = m
    keep = [0, 1, 2] if keep_equal else [0, 2]
    chains = [([tuple(p) for p in xy[row[c]:row[c + 1]].tolist()], int(left[c]), int(right[c])) for c in keep]
    out = [0, 2, 4] if keep_equal else [0, NONE, 2]
    return case(m, chains, keep, out, flags=KEEP_EQUAL if keep_equal else 0, n_kept=len(keep), n_dropped=3 - len(keep), n_chains=len(keep),
                n_points=sum(len(c[0]) for c in chains), n_closed=1 if keep_equal else 2, n_classes=2)


CONSTRUCTED = [("path", n) for n in PATH_SIZES] + [("loop", n) for n in LOOP_SIZES] + [("pair", m) for m in PAIR_SIZES] + [("long", 0), ("long", 1)]


@functools.lru_cache(maxsize=None)
def constructed(kind, n):
    """computed once, shared, never changed"""
    return {"path": path_case, "loop": loop_case, "pair": pair_case, "long": lambda k: long_case(bool(k))}[kind](n)
