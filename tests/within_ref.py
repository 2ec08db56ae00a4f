"""The definition of rj_within_query in plain Python integers and fractions.Fraction, on the functions of
tests/nearest_ref.py: brute force over all edges.  What tests/test_within.py holds the host twin to and
tests/test_gpu_within.py the device.

A map is what it is in nearest_ref: (pts, row_index), edges in eid order."""
import nearest_ref as NR

MAX_DIST = NR.MAX_DIST


def within(px, py, edges, max_dist):
    """-> [(eid, where, num, den)] of every edge with d^2 <= max_dist^2, ascending in eid"""
    assert 0 <= max_dist <= MAX_DIST
    out = []
    for eid, edge in enumerate(edges):
        where, num, den = NR.point_edge(px, py, edge)
        if NR.d2_of(where, num, den) <= max_dist * max_dist:
            out.append((eid, where, num, den))
    return out


def within_all(points, edges, max_dist):
    """-> one list per point"""
    return [within(int(x), int(y), edges, max_dist) for x, y in points]


def csr_of(lists):
    """per-point lists -> (offsets, flat list of tuples)"""
    offsets, flat = [0], []
    for row in lists:
        flat += row
        offsets.append(len(flat))
    return offsets, flat
