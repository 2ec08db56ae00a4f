"""Thinning the chains of a map by effective area (rj_map_simplify), by definition: plain Python integers, lists and one
`while` loop per round, nothing shared with rayjoin_amd/csrc/rj_simplify.h.  Where the header keeps linked points and a
work list, this rebuilds, in every round, the list of the live points of every chain and looks at all of them.

simplify_ref(xy, row_index, tol, flags=0) -> (out_xy [n, 2] int64, out_row uint32, origin uint32, counts) or raises
Invalid; tol a Python int in [0, 2^128).  counts a dict with the names of rj_simplify_counts."""
import numpy as np

COUNTS = ("n_points", "n_removed", "n_rounds", "n_closed", "n_pinned_extra", "n_max_round")
L = 1 << 46
HUGE = (1 << 128) - 1


class Invalid(ValueError):
    pass


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def tie(p):
    return (p * 2654435761) % (1 << 32)


def pins_of(pts, b, e):
    """the pinned points of the chain [b, e): its two ends and, where it is closed, m1 and m2 -> (set, closed, extra)"""
    pinned = {b, e - 1}
    if e - b < 3 or pts[b] != pts[e - 1]:
        return pinned, False, 0
    a, interior, extra = pts[b], range(b + 1, e - 1), 0
    far = [(pts[q][0] - a[0]) ** 2 + (pts[q][1] - a[1]) ** 2 for q in interior]
    if max(far) > 0:
        m1 = b + 1 + far.index(max(far))  # (index: the first of equal values)
        pinned.add(m1)
        extra += 1
        wide = [abs(cross(a, pts[m1], pts[q])) for q in interior]
        if max(wide) > 0:
            pinned.add(b + 1 + wide.index(max(wide)))
            extra += 1
    return pinned, True, extra


def simplify_ref(xy, row_index, tol, flags=0):
    pts = [(int(x), int(y)) for x, y in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    nc = max(0, len(row) - 1)
    if flags != 0 or not 0 <= tol <= HUGE:
        raise Invalid("flags or tol")
    if nc == 0:
        if pts:
            raise Invalid("points without chains")
        return np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.uint32), dict.fromkeys(COUNTS, 0)
    if row[0] != 0 or row[-1] != len(pts) or any(b >= e for b, e in zip(row, row[1:])):
        raise Invalid("row_index")
    if any(not -L <= v < L for p in pts for v in p):
        raise Invalid("coordinate")
    counts = dict.fromkeys(COUNTS, 0)
    pinned = set()
    for b, e in zip(row, row[1:]):
        s, closed, extra = pins_of(pts, b, e)
        pinned |= s
        counts["n_closed"] += closed
        counts["n_pinned_extra"] += extra
    live = [list(range(b, e)) for b, e in zip(row, row[1:])]
    while True:
        gone = set()
        for chain in live:
            key = {}  # the candidates of this chain and their keys
            for u, p, w in zip(chain, chain[1:], chain[2:]):
                if p not in pinned:
                    weight = abs(cross(pts[u], pts[p], pts[w]))
                    if weight <= tol:
                        key[p] = (weight, tie(p))
            for u, p, w in zip(chain, chain[1:], chain[2:]):
                if p in key and all(q not in key or key[p] < key[q] for q in (u, w)):
                    gone.add(p)
        if not gone:
            break
        counts["n_rounds"] += 1
        counts["n_max_round"] = max(counts["n_max_round"], len(gone))
        live = [[p for p in chain if p not in gone] for chain in live]
    origin = [p for chain in live for p in chain]
    out_row = np.cumsum([0] + [len(chain) for chain in live]).astype(np.uint32)
    counts.update(n_points=len(origin), n_removed=len(pts) - len(origin))
    return np.array([pts[p] for p in origin], np.int64).reshape(-1, 2), out_row, np.array(origin, np.uint32), counts
