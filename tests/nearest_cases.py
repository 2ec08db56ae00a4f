"""Hand cases of rj_nearest_query with the answers written out: (eid, where, num, den) per point, MISS = (0xFFFFFFFF, 0, 0, 0).
where 0 = interior (num = the signed cross product (B - A) x (P - A), den = |B - A|^2), 1 = first end, 2 = second end
(num = d^2, den = 1).  tests/test_nearest.py checks the definition (tests/nearest_ref.py) and the host twin against them,
tests/test_gpu_nearest.py the device."""
import collections
from fractions import Fraction

Case = collections.namedtuple("Case", "pts row points max_dist want")
MISS = (0xFFFFFFFF, 0, 0, 0)
M = (1 << 46) - 1  # the largest coordinate
C = 1 << 16        # a cell of the index's boxes


def chains(*cs):
    """chains of (x, y) points -> (pts, row)"""
    pts, row = [], [0]
    for c in cs:
        pts += list(c)
        row.append(len(pts))
    return pts, row


def case(cs, points, want, max_dist=-1):
    pts, row = chains(*cs)
    assert len(points) == len(want)
    return Case(pts, row, list(points), max_dist, list(want))


def vertical(x):
    """a vertical edge (x, -100) -> (x, 100) as a chain: for a point (px, py) with |py| < 100 the interior case with
    c = -200 (px - x) and den = 40 000"""
    return [(x, -100), (x, 100)]


# Two long edges at 2^46 scale whose distances to the origin differ by about 2^-136 relative: the lines through
# (-L, h) -> (L, h + 1) and (-(L - 1), -h - 1) -> (L - 1, -h) have d^2 = L^2 (2 h + 1)^2 / (4 L^2 + 1), with L - 1 for L in the
# second one, and x / (4 x + 1) ascends: the edge with L - 1 is the nearer one, by far less than a double can tell.
L_, H_ = 1 << 45, 1 << 44
FAR_EDGE = [(-L_, H_), (L_, H_ + 1)]                    # c = -L (2 h + 1), den = 4 L^2 + 1
NEAR_EDGE = [(-(L_ - 1), -H_ - 1), (L_ - 1, -H_)]         # c = (L - 1)(2 h + 1), den = 4 (L - 1)^2 + 1
FAR_REC = (0, -L_ * (2 * H_ + 1), 4 * L_ * L_ + 1)
NEAR_REC = (0, (L_ - 1) * (2 * H_ + 1), 4 * (L_ - 1) ** 2 + 1)
_d2_far, _d2_near = Fraction(FAR_REC[1] ** 2, FAR_REC[2]), Fraction(NEAR_REC[1] ** 2, NEAR_REC[2])
assert _d2_near < _d2_far and float(_d2_near) == float(_d2_far), "doubles must not be able to order the pair"
assert (_d2_far - _d2_near) / _d2_near < Fraction(1, 1 << 60)

HAND = {
    # ---- distance 0, shared vertices ----
    "on_edge": case([[(0, 0), (10, 0)]], [(5, 0)], [(0, 0, 0, 100)]),
    "vertex_of_two_chains": case([[(0, 0), (10, 0)], [(10, 0), (10, 10)]], [(10, 0)], [(0, 2, 0, 1)]),
    "vertex_of_three_chains": case([[(-10, 0), (0, 0)], [(0, 0), (0, 10)], [(0, 0), (10, -10)]], [(0, 0)], [(0, 2, 0, 1)]),
    # ---- ties ----
    # outside the corner of a chain: edge 0 ends there (where 2), edge 1 starts there (where 1): 3^2 + 4^2 both
    "interior_chain_vertex": case([[(0, 0), (10, 0), (10, 10)]], [(13, -4)], [(0, 2, 25, 1)]),
    "parallel_interiors": case([[(0, 10), (20, 10)], [(0, -10), (20, -10)]], [(10, 0)], [(0, 0, -200, 400)]),
    # the end (3, 4) of edge 0 and the interior of y = -5 are both 5 away
    "end_then_interior": case([[(3, 4), (10, 4)], [(-10, -5), (10, -5)]], [(0, 0)], [(0, 1, 25, 1)]),
    "interior_then_end": case([[(-10, -5), (10, -5)], [(3, 4), (10, 4)]], [(0, 0)], [(0, 0, 100, 400)]),
    # ---- degenerate and boundary projections ----
    "zero_length_edge": case([[(5, 5), (5, 5)], [(100, 100), (110, 100)]], [(8, 9), (5, 5)], [(0, 1, 25, 1), (0, 1, 0, 1)]),
    "dot_is_zero": case([[(0, 0), (10, 0)]], [(0, 7)], [(0, 1, 49, 1)]),
    "dot_is_l": case([[(0, 0), (10, 0)]], [(10, -3)], [(0, 2, 9, 1)]),
    # ---- the ends of the domain ----
    # (M, -M) against the diagonal: c = 2M 0 - 2M 2M, den = 8 M^2; (-M, M) is the first end of edge 1
    "extremes": case([[(-M, -M), (M, M)], [(-M, M), (-M + 10, M)]], [(M, -M), (-M, M), (M, M)],
                     [(0, 0, -4 * M * M, 8 * M * M), (1, 1, 0, 1), (0, 2, 0, 1)]),
    "extremes_far_end": case([[(-M - 1, -M - 1), (-M - 1, -M + 5)]], [(M, M)], [(0, 2, (2 * M + 1) ** 2 + (2 * M - 5) ** 2, 1)]),
    # ---- what doubles cannot order ----
    "near_tie_farther_first": case([FAR_EDGE, NEAR_EDGE], [(0, 0)], [(1,) + NEAR_REC]),
    "near_tie_nearer_first": case([NEAR_EDGE, FAR_EDGE], [(0, 0)], [(0,) + NEAR_REC]),
    # ---- max_dist ----
    "max_dist_equal": case([[(0, 0), (10, 0)]], [(5, 7)], [(0, 0, 70, 100)], max_dist=7),
    "max_dist_one_less": case([[(0, 0), (10, 0)]], [(5, 7)], [MISS], max_dist=6),
    "max_dist_zero_on_edge": case([[(0, 0), (10, 0)]], [(5, 0), (5, 1)], [(0, 0, 0, 100), MISS], max_dist=0),
    "max_dist_largest": case([[(0, 0), (10, 0)]], [(5, 7)], [(0, 0, 70, 100)], max_dist=1 << 48),
    "all_miss": case([[(0, 0), (10, 0), (10, 10)], [(50, 50), (60, 50)]], [(1000, 1000), (-1000, 5), (30, 30)], [MISS] * 3, max_dist=20),
    # ---- the borders of the index's cells (2^16 wide, aligned with the coordinates) ----
    # adjacent cells: edge 1 in cell 1; the point at the far end of cell 0 (x = 0) and at the near end (x = 2^16 - 1)
    "cells_adjacent": case([vertical(-40000), vertical(C)], [(0, 0), (C - 1, 0)], [(0, 0, -200 * 40000, 40000), (1, 0, 200, 40000)]),
    # two cells apart: edge 1 in cell 2, its box's gap from cell 0 is 1 larger than that of the decoy, edge 0, in cell -1.  From
    # the near end of cell 0 edge 1 is the nearer one (2^16 + 1 against 2^16 + 4); from the far end it is the decoy.
    "cells_two_apart_decoy": case([vertical(-5), vertical(2 * C)], [(C - 1, 0), (0, 0)],
                                  [(1, 0, 200 * (C + 1), 40000), (0, 0, -200 * 5, 40000)]),
    "cells_two_apart_y": case([[(-100, -5), (100, -5)], [(-100, 2 * C), (100, 2 * C)]], [(0, C - 1)], [(1, 0, -200 * (C + 1), 40000)]),
    # ---- a one-edge map ----
    "one_edge": case([[(-3, -3), (3, 3)]], [(0, 0), (3, -3), (10, 10), (-4, -3)], [(0, 0, 0, 72), (0, 0, -36, 72), (0, 2, 98, 1), (0, 1, 1, 1)]),
}
