"""Test-side restatement of the FACES of a chain map (test infrastructure): the definition of rayjoin_amd/csrc/rj_faces.h in
plain Python -- Python integers and Fractions, one walk per ring, every hole against every ceiling edge of the map, one walk
along `above` per hole -- independent of the grid, the sorts, the pointer jumping and the scans the product uses, so the two
check each other.

rings     the cycles of rings_ref.successor (no face involved), ascending by leader (the smallest half-chain).
kind      shell when area2 > 0, hole otherwise.  top: the largest (y, x) among a ring's points.
ceiling   a directed edge u -> v of a ring's walk with v.x < u.x; its number is 2 e + (h & 1), e the map's edge number.
above(H)  hole H with top p: among the ceiling edges of ALL rings with v.x <= p.x < u.x and their height at p.x strictly above
          p.y, the one with the smallest (height at p.x, slope, number); its ring.
face      follow above until a shell; nothing above: face 0.  Face k (1-based) is the k-th shell by leader.
left[c]   the face of the ring of half-chain 2 c, right[c] of 2 c + 1; 0 for a skipped chain.
label     (with in_left / in_right) of face k: the given label of its shell's leader; face 0: 0.  n_conflicts: the
          half-chains that are not skipped whose given label differs from the label of their computed face."""
from fractions import Fraction

import numpy as np

import rings_ref as D

FACE_DTYPE = np.dtype([("leader", "<u4"), ("n_holes", "<u4"), ("label", "<i4"), ("_pad", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
COUNTS = ("n_faces", "n_rings", "n_holes", "n_outer", "n_skipped", "n_dangling", "n_conflicts")
NONE = 0xFFFFFFFF


def area2_of(rows):
    """the exact area2 of FACE_DTYPE rows as Python ints"""
    return [(int(hi) << 64) | int(lo) for lo, hi in zip(rows["area2_lo"].tolist(), rows["area2_hi"].tolist())]


def ring_walks(xy, row_index):
    """-> ([(leader, [half-chains], area2, top (x, y), [(ux, uy, vx, vy, number)] its ceiling edges)] ascending by leader,
    {h: ring}, number of skipped chains)"""
    nxt, skipped, pts = D.successor(xy, row_index)
    row = [int(v) for v in row_index]
    ring_of, out = {}, []
    for h0 in sorted(nxt):
        if h0 in ring_of:
            continue
        halves, h = [], h0
        while h not in ring_of:
            ring_of[h] = len(out)
            halves.append(h)
            h = nxt[h]
        assert h == h0
        walk, ceilings = [], []
        for h in halves:
            c = h >> 1
            b, e = row[c], row[c + 1]
            idx = list(range(e - 1, b - 1, -1)) if h & 1 else list(range(b, e))
            for i, j in zip(idx, idx[1:]):
                u, v = pts[i], pts[j]
                walk.append(u)
                if v[0] < u[0]:
                    ceilings.append((u[0], u[1], v[0], v[1], 2 * (min(i, j) - c) + (h & 1)))
        area2 = sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(walk, walk[1:] + walk[:1]))
        ty, tx = max((y, x) for x, y in walk)
        out.append((h0, halves, area2, (tx, ty), ceilings))
    return out, ring_of, skipped


def above_of(walks):
    """-> [the ring above ring r, or None (a shell, or nothing above)]"""
    edges = [(ux, uy, vx, vy, num, r) for r, w in enumerate(walks) for ux, uy, vx, vy, num in w[4]]
    above = [None] * len(walks)
    for r, (_, _, area2, (px, py), _) in enumerate(walks):
        if area2 > 0:
            continue
        best = None
        for ux, uy, vx, vy, num, ring in edges:
            if not vx <= px < ux:
                continue
            slope = Fraction(uy - vy, ux - vx)
            height = vy + slope * (px - vx)
            if height <= py:
                continue
            cand = (height, slope, num, ring)
            if best is None or cand < best:
                best = cand
        if best is not None:
            above[r] = best[3]
    return above


def faces_ref(xy, row_index, in_left=None, in_right=None):
    """the arrays and the counts of rj_map_faces: dict(left, right, faces, counts, above, ring_face)"""
    nc = len(row_index) - 1
    walks, ring_of, skipped = ring_walks(xy, row_index)
    above = above_of(walks)
    n = len(walks)
    shells = [r for r in range(n) if walks[r][2] > 0]
    number = {r: k + 1 for k, r in enumerate(shells)}
    shell_of = [None] * n
    for r in range(n):
        at, steps = r, 0
        while at is not None and walks[at][2] <= 0:
            at = above[at]
            steps += 1
            assert steps <= n  # tops rise strictly along above
        shell_of[r] = at
    ring_face = [0 if s is None else number[s] for s in shell_of]
    given = None
    if in_left is not None:
        given = lambda h: int(in_right[h >> 1]) if h & 1 else int(in_left[h >> 1])  # noqa: E731
    left, right = np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    dangling = conflicts = 0
    for c in range(nc):
        if 2 * c not in ring_of:
            continue
        left[c], right[c] = ring_face[ring_of[2 * c]], ring_face[ring_of[2 * c + 1]]
        dangling += int(left[c] == right[c])
        for h in (2 * c, 2 * c + 1):
            s = shell_of[ring_of[h]]
            if given is not None and given(h) != (0 if s is None else given(walks[s][0])):
                conflicts += 1
    faces = np.zeros(len(shells), FACE_DTYPE)
    for k, s in enumerate(shells):
        holes = [r for r in range(n) if shell_of[r] == s and r != s]
        total = walks[s][2] + sum(walks[r][2] for r in holes)
        faces[k] = (walks[s][0], len(holes), given(walks[s][0]) if given is not None else 0, 0, total & ((1 << 64) - 1), total >> 64)
    n_holes = sum(1 for r in range(n) if walks[r][2] <= 0 and shell_of[r] is not None)
    counts = dict(n_faces=len(shells), n_rings=n, n_holes=n_holes, n_outer=n - len(shells) - n_holes, n_skipped=skipped, n_dangling=dangling,
                  n_conflicts=conflicts)
    return dict(left=left, right=right, faces=faces, counts=counts, above=above, ring_face=ring_face)


def assert_same_faces(got, want, what=""):
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for name in ("left", "right", "faces"):
        a, b = got[name], want[name]
        if a is None:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name)
