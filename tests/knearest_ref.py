"""The definition of rj_knearest_query in plain Python integers and fractions.Fraction, on nearest_ref.point_edge: all edges
sorted by (d^2, eid), max_dist applied, cut at k.  What tests/test_knearest.py holds the host twin to (test
infrastructure, not collected by pytest)."""
from fractions import Fraction

import nearest_ref as NR

MAX_K = 32


def knearest(px, py, edges, k, max_dist=-1):
    """-> [(eid, where, num, den)]: the first min(k, qualifying edges) of the order (d^2, eid)"""
    assert 1 <= k <= MAX_K
    rows = []
    for eid, edge in enumerate(edges):
        where, num, den = NR.point_edge(px, py, edge)
        d2 = Fraction(num * num, den) if where == NR.INTERIOR else Fraction(num)
        if max_dist >= 0 and d2 > max_dist * max_dist:
            continue
        rows.append((d2, eid, where, num, den))
    rows.sort(key=lambda r: (r[0], r[1]))
    return [r[1:] for r in rows[:k]]


def knearest_all(points, edges, k, max_dist=-1):
    return [knearest(int(x), int(y), edges, k, max_dist) for x, y in points]
