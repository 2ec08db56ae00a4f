"""Hand cases of rj_within_query with the answers written out: per point the list of (eid, where, num, den), ascending in
eid, [] where no edge lies within max_dist.  where 0 = interior (num = the signed cross product (B - A) x (P - A), den =
|B - A|^2, d^2 = num^2 / den), 1 = first end, 2 = second end (num = d^2, den = 1).  tests/test_within.py checks the
definition (tests/within_ref.py) and the host twin against them, tests/test_gpu_within.py the device."""
import collections

from nearest_cases import C, M, chains, vertical

Case = collections.namedtuple("Case", "pts row points max_dist want")


def case(cs, points, max_dist, want):
    pts, row = chains(*cs)
    assert len(points) == len(want) and all(list(w) == sorted(w) for w in want)
    return Case(pts, row, list(points), max_dist, [list(w) for w in want])


FLOOR = [(0, 0), (10, 0)]   # the horizontal edge of most cases: for (px, py) over its interior c = 10 py, den = 100
THREE = [[(-10, 0), (0, 0)], [(0, 0), (0, 10)], [(0, 0), (10, -10)]]  # three chains that share the vertex (0, 0)
CORNER = [[(0, 0), (10, 0), (10, 10)]]  # a chain with the interior vertex (10, 0)
LONG = [(-M, 0), (M, 0)]    # for (1, M): c = 2 M M, den = 4 M M, d = M exactly, where doubles round c

HAND = {
    # ---- the distance itself: equality is in, one less is out ----
    # (5, 5) over the interior: d = 5; (13, 4) behind the second end: 3^2 + 4^2
    "three_four_five_in": case([FLOOR], [(5, 5), (13, 4)], 5, [[(0, 0, 50, 100)], [(0, 2, 25, 1)]]),
    "three_four_five_out": case([FLOOR], [(5, 5), (13, 4)], 4, [[], []]),
    # d^2 = 16 / 5, not an integer: between 1 and 4
    "non_integer_d2_out": case([[(0, 0), (1, 2)]], [(2, 0)], 1, [[]]),
    "non_integer_d2_in": case([[(0, 0), (1, 2)]], [(2, 0)], 2, [[(0, 0, -4, 5)]]),
    # ---- max_dist = 0 ----
    "zero_on_vertex_of_three_chains": case(THREE, [(0, 0)], 0, [[(0, 2, 0, 1), (1, 1, 0, 1), (2, 1, 0, 1)]]),
    "zero_on_interior_point": case([FLOOR], [(5, 0), (5, 1)], 0, [[(0, 0, 0, 100)], []]),
    # ---- the tie at an interior vertex of a chain: a pair list, not a nearest ----
    "chain_vertex_tie": case(CORNER, [(13, -4)], 5, [[(0, 2, 25, 1), (1, 1, 25, 1)]]),
    "chain_vertex_tie_out": case(CORNER, [(13, -4)], 4, [[]]),
    # ---- degenerate and boundary projections ----
    "zero_length_edge": case([[(5, 5), (5, 5)], [(100, 100), (110, 100)]], [(8, 9), (5, 5)], 5, [[(0, 1, 25, 1)], [(0, 1, 0, 1)]]),
    "dot_is_zero": case([FLOOR], [(0, 7)], 7, [[(0, 1, 49, 1)]]),
    "dot_is_l": case([FLOOR], [(10, -3)], 3, [[(0, 2, 9, 1)]]),
    # ---- the ends of the domain: with the largest max_dist every edge is listed ----
    "extremes_all": case([[(-M, -M), (M, M)], [(-M, M), (-M + 10, M)]], [(M, -M), (-M, M), (M, M)], 1 << 48,
                         [[(0, 0, -4 * M * M, 8 * M * M), (1, 2, (2 * M - 10) ** 2 + (2 * M) ** 2, 1)],
                          [(0, 0, 4 * M * M, 8 * M * M), (1, 1, 0, 1)],
                          [(0, 2, 0, 1), (1, 2, (2 * M - 10) ** 2, 1)]]),
    # ---- what a double cannot tell from equality: the filter must leave it to the exact test ----
    "large_equal": case([LONG], [(1, M)], M, [[(0, 0, 2 * M * M, 4 * M * M)]]),
    "large_one_less": case([LONG], [(1, M)], M - 1, [[]]),
    # ---- the borders of the index's cells (2^16 wide): the (g - 1)+ of the prune ----
    # one cell apart: the edge on the first column of cell 1, the points at the near end (d = 1) and the far end (d = 2^16) of cell 0
    "cells_one_apart_in": case([vertical(C)], [(C - 1, 0), (0, 0)], C, [[(0, 0, 200, 40000)], [(0, 0, 200 * C, 40000)]]),
    "cells_one_apart_out": case([vertical(C)], [(C - 1, 0), (0, 0)], C - 1, [[(0, 0, 200, 40000)], []]),
    # two cells apart: one whole cell lies between, but the distance from the near end is only 2^16 + 1
    "cells_two_apart_in": case([vertical(2 * C)], [(C - 1, 0), (0, 0)], C + 1, [[(0, 0, 200 * (C + 1), 40000)], []]),
    "cells_two_apart_out": case([vertical(2 * C)], [(C - 1, 0), (0, 0)], C, [[], []]),
    "cells_two_apart_y_in": case([[(-100, 2 * C), (100, 2 * C)]], [(0, C - 1)], C + 1, [[(0, 0, -200 * (C + 1), 40000)]]),
    "cells_two_apart_y_out": case([[(-100, 2 * C), (100, 2 * C)]], [(0, C - 1)], C, [[]]),
    # ---- the shape of the CSR ----
    # an empty list between two lists: equal consecutive offsets
    "empty_between": case([FLOOR], [(5, 1), (5, 100), (5, -1)], 2, [[(0, 0, 10, 100)], [], [(0, 0, -10, 100)]]),
    # the second point lists the smaller eid: the sort must keep the points apart
    "second_point_smaller_eid": case([FLOOR, [(100, 0), (110, 0)]], [(105, 1), (5, 1)], 2, [[(1, 0, 10, 100)], [(0, 0, 10, 100)]]),
    "one_edge": case([[(-3, -3), (3, 3)]], [(0, 0), (3, -3), (10, 10), (-4, -3)], 5, [[(0, 0, 0, 72)], [(0, 0, -36, 72)], [], [(0, 1, 1, 1)]]),
    "one_point": case([[(-10, 5), (10, 5)], [(-10, -7), (10, -7)], [(20, 0), (30, 0)]], [(0, 0)], 6, [[(0, 0, -100, 400)]]),
}
