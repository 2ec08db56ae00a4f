"""The definition of rj_window_query in plain Python integers and fractions.Fraction: brute force over all edges, and not
by the header's method.  The closed segment A + t (B - A), t in [0, 1], is clipped against the four closed half-planes of
the window (Liang-Barsky with exact fractions): the edge belongs iff a t is left.  No clamp: Python integers do not
overflow, so this is also what the clamp must not change.  What tests/test_window.py holds the host twin to and
tests/test_gpu_window.py the device.

A map is what it is in nearest_ref: (pts, row_index), edges in eid order.  A window is (x0, y0, x1, y1)."""
from fractions import Fraction


def flags_of(edge, win):
    ax, ay, bx, by = edge
    x0, y0, x1, y1 = win
    return (1 if x0 <= ax <= x1 and y0 <= ay <= y1 else 0) | (2 if x0 <= bx <= x1 and y0 <= by <= y1 else 0)


def meets(edge, win):
    ax, ay, bx, by = edge
    x0, y0, x1, y1 = win
    if x0 > x1 or y0 > y1:
        return False
    t0, t1 = Fraction(0), Fraction(1)
    dx, dy = bx - ax, by - ay
    for p, q in ((-dx, ax - x0), (dx, x1 - ax), (-dy, ay - y0), (dy, y1 - ay)):  # p t <= q
        if p == 0:
            if q < 0:
                return False
        elif p < 0:
            t0 = max(t0, Fraction(q, p))
        else:
            t1 = min(t1, Fraction(q, p))
    return t0 <= t1


def window(win, edges):
    """-> [(eid, flags)] of every edge that shares a point with the window, ascending in eid"""
    win = tuple(int(v) for v in win)
    return [(eid, flags_of(e, win)) for eid, e in enumerate(edges) if meets(e, win)]


def window_all(windows, edges):
    """-> one list per window"""
    return [window(w, edges) for w in windows]


def csr_of(lists):
    """per-window lists -> (offsets, eids, flags)"""
    offsets, eids, flags = [0], [], []
    for row in lists:
        eids += [e for e, _ in row]
        flags += [f for _, f in row]
        offsets.append(len(eids))
    return offsets, eids, flags
