"""The definition of rj_nearest_query in plain Python integers and fractions.Fraction: brute force over all edges.  What
tests/test_nearest.py holds the host twin to and tests/test_gpu_nearest.py the device.

A map here is (pts, row_index): int (x, y) pairs and the first point of every chain with the point count at the end; edge
e of chain c runs from point e + c to point e + c + 1, as in the library."""
from fractions import Fraction

MISS = 0xFFFFFFFF
INTERIOR, FIRST_END, SECOND_END = 0, 1, 2
MAX_DIST = 1 << 48


def edges_of(pts, row_index):
    """-> [(ax, ay, bx, by)] in eid order"""
    out = []
    for c in range(len(row_index) - 1):
        for p in range(int(row_index[c]), int(row_index[c + 1]) - 1):
            out.append((int(pts[p][0]), int(pts[p][1]), int(pts[p + 1][0]), int(pts[p + 1][1])))
    return out


def point_edge(px, py, edge):
    """-> (where, num, den): the case, and the record's integers (the SIGNED cross product and l in the interior, d^2 and 1
    at an end)"""
    ax, ay, bx, by = edge
    dx, dy, ex, ey = bx - ax, by - ay, px - ax, py - ay
    dot, l = ex * dx + ey * dy, dx * dx + dy * dy
    if dot <= 0:
        return FIRST_END, ex * ex + ey * ey, 1
    if dot >= l:
        return SECOND_END, (px - bx) ** 2 + (py - by) ** 2, 1
    return INTERIOR, dx * ey - dy * ex, l


def d2_of(where, num, den):
    """the squared distance as a Fraction"""
    return Fraction(num * num, den) if where == INTERIOR else Fraction(num)


def nearest(px, py, edges, max_dist=-1):
    """-> (eid, where, num, den); (MISS, 0, 0, 0) where no edge qualifies"""
    best, best_d2 = (MISS, 0, 0, 0), None
    for eid, edge in enumerate(edges):
        where, num, den = point_edge(px, py, edge)
        d2 = d2_of(where, num, den)
        if max_dist >= 0 and d2 > max_dist * max_dist:
            continue
        if best_d2 is None or d2 < best_d2:  # (ascending eids: a tie keeps the smaller one)
            best, best_d2 = (eid, where, num, den), d2
    return best


def nearest_all(points, edges, max_dist=-1):
    return [nearest(int(x), int(y), edges, max_dist) for x, y in points]
