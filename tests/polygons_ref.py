"""Test-side restatement of the POLYGONS of a set of face rings (test infrastructure): the definition of
rayjoin_amd/csrc/rj_polygons.h in plain Python -- Python integers and Fractions, every hole against every ceiling edge of
its face, one walk along `above` per hole -- independent of the strips, the sorts, the pointer jumping and the scans the
product uses, so the two check each other.

Input: the output of rj_map_rings with points (rings as RING_DTYPE rows, ring_row, ring_xy).

kind      face == 0: none (n_face0).  face != 0: shell when area2 > 0, hole otherwise.
top       the largest (y, x) among a ring's points.
ceiling   a ring edge u -> v (a point and its successor, the last point's successor is the first) with v.x < u.x, of a
          ring whose face is not 0.
above(H)  hole H of face f with top p: among the ceiling edges of rings of face f with v.x <= p.x < u.x and their height at
          p.x strictly above p.y, the one with the smallest (height at p.x, slope, point slot of u); its ring.
parent    follow above until a shell; a walk that ends at a hole with nothing above it: an orphan (n_orphans).
polygons  one per shell, ascending by shell; members: the shell, then its holes ascending; area2 = the members' sum."""
from fractions import Fraction

import numpy as np

POLYGON_DTYPE = np.dtype([("face", "<i4"), ("shell", "<u4"), ("n_holes", "<u4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
COUNTS = ("n_polygons", "n_members", "n_holes", "n_orphans", "n_face0")
ARRAYS = ("parent", "polygons", "poly_first", "poly_ring")
NONE = 0xFFFFFFFF


def area2_of(rows):
    """the exact area2 of RING_DTYPE / POLYGON_DTYPE rows as Python ints"""
    return [(int(hi) << 64) | int(lo) for lo, hi in zip(rows["area2_lo"].tolist(), rows["area2_hi"].tolist())]


def above_of(rings, ring_row, ring_xy):
    """-> (kinds, above): kinds[r] in "none", "shell", "hole"; above[r] = the ring above hole r, or None"""
    n = len(rings)
    face = [int(f) for f in rings["face"].tolist()]
    a2 = area2_of(rings)
    row = [int(v) for v in ring_row.tolist()]
    pts = [(int(x), int(y)) for x, y in np.asarray(ring_xy).reshape(-1, 2).tolist()]
    kinds = ["none" if face[r] == 0 else ("shell" if a2[r] > 0 else "hole") for r in range(n)]
    ceilings = {}  # face -> [(ux, uy, vx, vy, slot of u, ring)]
    for r in range(n):
        if face[r] == 0:
            continue
        for i in range(row[r], row[r + 1]):
            u, v = pts[i], pts[i + 1 if i + 1 < row[r + 1] else row[r]]
            if v[0] < u[0]:
                ceilings.setdefault(face[r], []).append((u[0], u[1], v[0], v[1], i, r))
    above = [None] * n
    for r in range(n):
        if kinds[r] != "hole" or row[r] == row[r + 1]:
            continue
        py, px = max((y, x) for x, y in pts[row[r]:row[r + 1]])
        best = None
        for ux, uy, vx, vy, slot, ring in ceilings.get(face[r], ()):
            if not vx <= px < ux:
                continue
            slope = Fraction(uy - vy, ux - vx)
            height = vy + slope * (px - vx)
            if height <= py:
                continue
            cand = (height, slope, slot, ring)
            if best is None or cand < best:
                best = cand
        if best is not None:
            above[r] = best[3]
    return kinds, above


def polygons_ref(rings, ring_row, ring_xy):
    """the arrays and the counts of rj_rings_polygons: dict(parent, polygons, poly_first, poly_ring, counts)"""
    n = len(rings)
    kinds, above = above_of(rings, ring_row, ring_xy)
    a2 = area2_of(rings)
    parent = np.full(n, NONE, np.uint32)
    members = {}
    orphans = 0
    for r in range(n):
        if kinds[r] == "shell":
            parent[r] = r
            members.setdefault(r, [])
        elif kinds[r] == "hole":
            at, steps = r, 0
            while at is not None and kinds[at] != "shell":
                at = above[at]
                steps += 1
                assert steps <= n  # tops rise strictly along above
            if at is None:
                orphans += 1
            else:
                parent[r] = at
                members.setdefault(at, []).append(r)
    shells = sorted(members)
    polygons = np.zeros(len(shells), POLYGON_DTYPE)
    first, ring = [0], []
    for k, s in enumerate(shells):
        holes = sorted(members[s])
        total = a2[s] + sum(a2[h] for h in holes)
        polygons[k] = (int(rings["face"][s]), s, len(holes), 0, total & ((1 << 64) - 1), total >> 64)
        ring.extend([s] + holes)
        first.append(len(ring))
    counts = dict(n_polygons=len(shells), n_members=len(ring), n_holes=len(ring) - len(shells), n_orphans=orphans,
                  n_face0=sum(1 for k in kinds if k == "none"))
    return dict(parent=parent, polygons=polygons, poly_first=np.array(first, np.uint32), poly_ring=np.array(ring, np.uint32), counts=counts)


def assert_same_polygons(got, want, what=""):
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for name in ARRAYS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name)
