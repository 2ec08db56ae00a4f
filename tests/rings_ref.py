"""Test-side restatement of the FACE RINGS of a chain map (test infrastructure): the definition of
rayjoin_amd/csrc/rj_rings.h in plain Python -- dictionaries, lists and Python integers, one junction at a time, one walk
per ring -- independent of the sorts, the pointer doubling and the scans the product uses, so the two check each other.

A chain map: xy[np, 2] (integers), row_index[nc + 1], left[nc], right[nc]; left is the face on the left of a chain
walked from its first point to its last, y up.

half-chains   h = 2 c is chain c forward (face left[c]), h = 2 c + 1 chain c backward (face right[c]), h ^ 1 the twin.  A
              chain whose points are all equal is skipped: in no ring, counted in n_skipped.
incidences    incidence h = the start vertex of h, with the direction to the first point of the chain (walking inward from
              that end) that differs from it.
junction      the incidences on one point, counter-clockwise from the positive x axis: half-plane 0 (dy > 0, or dy == 0
              and dx > 0) first; inside a half-plane a before b when a.dx b.dy - a.dy b.dx > 0; equal directions by h.
successor     h arrives at the junction of h ^ 1 = o_k of its order o_0 .. o_{d-1}: next(h) = o_{(k - 1) mod d}.
ring          a cycle of next.  leader = its smallest h, face = the leader's, MIXED when another half-chain's face differs,
              half-chains in walk order from the leader, points = every half-chain's points in its direction without the
              last, area2 = sum of cross(a, b) over consecutive points including the closing pair.
order         ascending by ((uint32) face << 32) | leader."""
import functools

import numpy as np

RING_DTYPE = np.dtype([("face", "<i4"), ("flags", "<u4"), ("leader", "<u4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
MIXED = 1
ARRAYS = ("rings", "ring_first", "ring_half", "ring_row", "ring_xy")
COUNTS = ("n_rings", "n_halves", "n_points", "n_mixed", "n_skipped")


def half_points(pts, row_index, h):
    """the points of half-chain h in its direction"""
    c = h >> 1
    p = pts[int(row_index[c]):int(row_index[c + 1])]
    return p[::-1] if h & 1 else p


def _half_plane(d):
    return 0 if (d[1] > 0 or (d[1] == 0 and d[0] > 0)) else 1


def _ccw(a, b):
    """a, b = (h, (dx, dy)): negative when a comes first"""
    (ha, da), (hb, db) = a, b
    pa, pb = _half_plane(da), _half_plane(db)
    if pa != pb:
        return pa - pb
    cr = da[0] * db[1] - da[1] * db[0]
    if cr != 0:
        return -1 if cr > 0 else 1
    return ha - hb


def successor(xy, row_index):
    """-> ({h: next(h)} over the half-chains that are not skipped, number of skipped chains, the points as tuples)"""
    pts = [(int(x), int(y)) for x, y in np.asarray(xy).reshape(-1, 2).tolist()]
    nc = len(row_index) - 1
    junctions, at, skipped = {}, {}, 0
    for c in range(nc):
        if len(set(half_points(pts, row_index, 2 * c))) == 1:
            skipped += 1
            continue
        for h in (2 * c, 2 * c + 1):
            p = half_points(pts, row_index, h)
            q = next(v for v in p if v != p[0])
            junctions.setdefault(p[0], []).append((h, (q[0] - p[0][0], q[1] - p[0][1])))
            at[h] = p[0]
    order = {v: [h for h, _ in sorted(inc, key=functools.cmp_to_key(_ccw))] for v, inc in junctions.items()}
    nxt = {}
    for h in at:
        o = order[at[h ^ 1]]
        nxt[h] = o[(o.index(h ^ 1) - 1) % len(o)]
    return nxt, skipped, pts


def ring_list(xy, row_index, left, right):
    """-> ([(face, leader, mixed, [half-chains], [points], area2)] in ring order, number of skipped chains)"""
    nxt, skipped, pts = successor(xy, row_index)
    face = lambda h: int(right[h >> 1]) if h & 1 else int(left[h >> 1])  # noqa: E731
    seen, out = set(), []
    for h0 in sorted(nxt):
        if h0 in seen:
            continue
        halves, h = [], h0
        while h not in seen:
            seen.add(h)
            halves.append(h)
            h = nxt[h]
        assert h == h0  # next is a permutation
        ring = []
        for h in halves:
            ring.extend(half_points(pts, row_index, h)[:-1])
        area2 = sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(ring, ring[1:] + ring[:1]))
        out.append((face(h0), h0, any(face(h) != face(h0) for h in halves), halves, ring, area2))
    out.sort(key=lambda r: ((r[0] & 0xFFFFFFFF) << 32) | r[1])
    return out, skipped


def rings_ref(xy, row_index, left, right, skip_face0=False, points=True):
    """the arrays and the counts of rj_map_rings: dict(rings, ring_first, ring_half, ring_row, ring_xy, counts);
    points=False (RJ_RINGS_NO_POINTS): ring_row and ring_xy are None"""
    rl, skipped = ring_list(xy, row_index, left, right)
    if skip_face0:
        rl = [r for r in rl if r[0] != 0]
    rings = np.zeros(len(rl), RING_DTYPE)
    first, rows, halves, xy_out = [0], [0], [], []
    for k, (face, leader, mixed, hs, ring, area2) in enumerate(rl):
        rings[k] = (face, MIXED if mixed else 0, leader, 0, area2 & ((1 << 64) - 1), area2 >> 64)
        halves.extend(hs)
        xy_out.extend(ring)
        first.append(len(halves))
        rows.append(len(xy_out))
    counts = dict(n_rings=len(rl), n_halves=len(halves), n_points=len(xy_out), n_mixed=sum(1 for r in rl if r[2]), n_skipped=skipped)
    return dict(rings=rings, ring_first=np.array(first, np.uint32), ring_half=np.array(halves, np.uint32),
                ring_row=np.array(rows, np.uint32) if points else None,
                ring_xy=np.array(xy_out, np.int64).reshape(-1, 2) if points else None, counts=counts)


def area2_of(rings):
    """the exact area2 of RING_DTYPE rows as Python ints"""
    return [(int(hi) << 64) | int(lo) for lo, hi in zip(rings["area2_lo"].tolist(), rings["area2_hi"].tolist())]


def assert_same_rings(got, want, what=""):
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for name in ARRAYS:
        a, b = got[name], want[name]
        if b is None:
            assert a is None, (what, name)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name)
