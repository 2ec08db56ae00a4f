"""Hand cases of rj_window_query with the answers written out: per window the list of (eid, flags), ascending in eid, []
where no edge meets the window.  flags bit 0: the edge's first point lies in the window, bit 1: its second point does.
tests/test_window.py checks the definition (tests/window_ref.py) and the host twin against them,
tests/test_gpu_window.py the device."""
import collections

from nearest_cases import C, M, chains

Case = collections.namedtuple("Case", "pts row windows want")
LO = -M - 1  # the smallest coordinate
I64 = (1 << 63) - 1


def case(cs, windows, want):
    pts, row = chains(*cs)
    assert len(windows) == len(want) and all(list(w) == sorted(w) for w in want)
    return Case(pts, row, [tuple(w) for w in windows], [list(w) for w in want])


W = (0, 0, 10, 10)          # the window of most cases
FLOOR = [(0, 0), (10, 0)]
CORNER = [[(0, 0), (10, 0), (10, 10)]]  # a chain with the interior vertex (10, 0)
ENDS = [[(LO, LO), (LO + 10, LO)], [(M, M - 10), (M, M)]]  # an edge at either end of the domain

HAND = {
    # ---- touching counts; one unit away does not ----
    # x + y = 20 through the corner (10, 10) and nothing else of the window; x + y = 21 beside it
    "touches_corner": case([[(5, 15), (15, 5)]], [W], [[(0, 0)]]),
    "corner_one_unit_away": case([[(5, 16), (16, 5)]], [W], [[]]),
    # ---- the box test alone would list it: x + y = 28 passes outside the corner, the boxes overlap ----
    "diagonal_outside_corner": case([[(8, 20), (20, 8)]], [W], [[]]),
    # ---- through the window, both ends outside ----
    "through": case([[(-5, 3), (15, 7)]], [W], [[(0, 0)]]),
    # x + y = 18 cuts off the corner (10, 10) alone: the three other corners lie on one side
    "cuts_top_right_corner": case([[(5, 13), (13, 5)]], [W], [[(0, 0)]]),
    # ---- collinear with a side ----
    "collinear_overlaps_side": case([[(0, -5), (0, 15)]], [W], [[(0, 0)]]),  # (its box touches the window in x0 == hx only)
    "collinear_beyond_side": case([[(0, 11), (0, 20)]], [W], [[]]),
    "collinear_from_corner": case([[(0, 10), (0, 20)]], [W], [[(0, 1)]]),
    # ---- the flags ----
    "inside_leaving_and_outside": case([[(2, 2), (8, 8)], [(5, 5), (15, 5)], [(-5, 5), (5, 5)], [(20, 20), (30, 30)]], [W],
                                       [[(0, 3), (1, 1), (2, 2)]]),
    "zero_length_edge": case([[(5, 5), (5, 5)], [(11, 5), (11, 5)]], [W], [[(0, 3)]]),
    # ---- degenerate windows ----
    # a point window on a chain's interior vertex lists both edges; one unit off an edge lists none
    "point_window_on_vertex": case(CORNER, [(10, 0, 10, 0)], [[(0, 2), (1, 1)]]),
    "point_window_on_edge_and_off": case([FLOOR], [(5, 0, 5, 0), (5, 1, 5, 1)], [[(0, 0)], []]),
    "line_window": case([FLOOR], [(5, -3, 5, 3), (11, -3, 11, 3), (-4, 0, 20, 0)], [[(0, 0)], [], [(0, 3)]]),
    # ---- inside one 2^16 cell of the index, not touching; and beside a wide window, in the cell of its x0 ----
    "same_quantum_apart": case([[(10, 10), (20, 20)]], [(30, 30, 40, 40), (21, 10, 40, 19)], [[], []]),
    "same_cell_beside_wide_window": case([[(10, 0), (50, 20)]], [(100, -2 * C, 3 * C, 2 * C), (50, -2 * C, 3 * C, 2 * C)], [[], [(0, 2)]]),
    # ---- empty windows are no error ----
    "empty_window": case([FLOOR], [(10, 0, 0, 10), (0, 10, 10, 0), (10, 10, 0, 0), W], [[], [], [], [(0, 3)]]),
    # ---- coordinates outside the domain: cut to it; wholly beside it: nothing, also where an edge lies on the border ----
    "outside_domain": case(ENDS, [(-(1 << 50), -(1 << 50), 1 << 50, 1 << 50), (1 << 47, 0, 1 << 48, M), (1 << 50, M - 5, 1 << 47, M),
                                  (M - 3, M - 5, 1 << 50, M + 7), (-I64 - 1, -I64 - 1, I64, I64)],
                           [[(0, 3), (1, 3)], [], [], [(1, 2)], [(0, 3), (1, 3)]]),
    # ---- both ends of the domain ----
    "domain_ends": case(ENDS, [(LO, LO, LO, LO), (M, M, M, M), (-I64 - 1, -I64 - 1, LO, LO), (M, M, I64, I64), (LO, LO, M, M), (LO + 1, LO, M, M - 1)],
                        [[(0, 1)], [(1, 2)], [(0, 1)], [(1, 2)], [(0, 3), (1, 3)], [(0, 2), (1, 1)]]),
    # the long diagonal of the domain: products of 2^47 operands; the point window beside it by one unit misses
    "domain_diagonal": case([[(LO, LO), (M, M)]], [(5, 5, 5, 5), (5, 4, 5, 4), (M - 1, LO, M, LO + 1), (LO, M - 1, LO + 1, M)], [[(0, 0)], [], [], []]),
    # ---- the shape of the CSR: an empty list between two lists, the second window lists the smaller eid ----
    "empty_between": case([FLOOR, [(100, 0), (110, 0)]], [(105, -1, 106, 1), (50, -1, 60, 1), (-1, -1, 1, 1)], [[(1, 0)], [], [(0, 1)]]),
}
