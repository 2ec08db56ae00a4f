"""Hand-built ring sets for the rings-to-map tests (tests/test_ringmap.py, tests/test_gpu_ringmap.py) with the answers
written out: every case is (rings, dissolve, answer) -- rings = (ring_row uint32, ring_xy int64 [n, 2], ring_face int32),
answer = dict(chains=[(points, left, right)], counts...) as tests/ringmap_ref.py's arrays would hold them.  The answers of the
disjoint loops come from the construction (loops_answer): a simple loop that touches nothing is one closed chain, read from
the smaller end of its smallest edge towards the larger."""
import numpy as np

import rings_cases as K
import rings_planar as P
import rings_ref as D

LIM = 1 << 46
LOOP_SIZES = (3, 63, 64, 65, 257)
LONG_LOOP = 100_003


def ring_set(rings):
    """rings = [(face, points)] -> (ring_row, ring_xy, ring_face)"""
    row, xy, face = [0], [], []
    for f, pts in rings:
        xy.extend(pts)
        row.append(len(xy))
        face.append(f)
    return np.array(row, np.uint32), np.array(xy, np.int64).reshape(-1, 2), np.array(face, np.int32)


def answer(chains, **counts):
    """chains = [(points, left, right)] in chain order -> the arrays and the counts (those not named are 0; n_chains,
    n_points and n_edges follow from the chains)"""
    xy, row = [], [0]
    for pts, _, _ in chains:
        xy.extend(pts)
        row.append(len(xy))
    c = dict(n_chains=len(chains), n_points=len(xy), n_edges=len(xy) - len(chains), n_closed=0, n_zero_edges=0, n_conflicts=0, n_dissolved=0)
    c.update(counts)
    return dict(xy=np.array(xy, np.int64).reshape(-1, 2), row_index=np.array(row, np.uint32), left=np.array([c_[1] for c_ in chains], np.int32),
                right=np.array([c_[2] for c_ in chains], np.int32), counts=c)


# ---- two squares that share the side x = 2 ----------------------------------------------------------------------------
SQ_A, SQ_B = [(0, 0), (2, 0), (2, 2), (0, 2)], [(2, 0), (4, 0), (4, 2), (2, 2)]
ROUND_A, ROUND_B = [(2, 0), (0, 0), (0, 2), (2, 2)], [(2, 0), (4, 0), (4, 2), (2, 2)]


def two_squares(fa, fb, dissolve):
    """7 unique edges; (2, 0) and (2, 2) have three.  Half-edge 3 walks (2, 0) -> (0, 0), 6 the shared side upwards, 8
    (2, 0) -> (4, 0): the three chains start at (2, 0), the twins of their walks have the leaders 5, 7 and 10."""
    rings = ring_set([(fa, SQ_A), (fb, SQ_B)])
    if dissolve and fa == fb:  # the shared side goes: 6 edges, one loop, read from (0, 0) -> (0, 2) with the outside on the left
        return rings, True, answer([([(0, 0), (0, 2), (2, 2), (4, 2), (4, 0), (2, 0), (0, 0)], 0, fa)], n_closed=1, n_dissolved=1)
    return rings, dissolve, answer([(ROUND_A, 0, fa), ([(2, 0), (2, 2)], fa, fb), (ROUND_B, fb, 0)])


def square_with_hole():
    """face 1 between two squares (its hole clockwise), face 2 inside: two closed chains, each read from its lower left
    corner upwards (the smallest edge is the left side, lo below hi), the outer face on the left of that direction"""
    rings = ring_set([(1, [(0, 0), (10, 0), (10, 10), (0, 10)]), (1, [(3, 3), (3, 6), (6, 6), (6, 3)]), (2, [(3, 3), (6, 3), (6, 6), (3, 6)])])
    return rings, False, answer([([(0, 0), (0, 10), (10, 10), (10, 0), (0, 0)], 0, 1), ([(3, 3), (3, 6), (6, 6), (6, 3), (3, 3)], 1, 2)], n_closed=2)


def rect_rings():
    """the rings of the two-rectangle output map (5 chains): the map of test_overlay_map.py's pair comes back as 3 chains"""
    U = 1 << 20
    rg = D.rings_ref(*K.rect_output_map(U))
    s = lambda pts: [(x * U, y * U) for x, y in pts]  # noqa: E731
    return ((rg["ring_row"], rg["ring_xy"], rg["rings"]["face"].astype(np.int32)), False,
            answer([(s([(3, 2), (2, 2), (2, 4), (3, 4)]), 0, 1), (s([(3, 2), (3, 4)]), 1, 2), (s([(3, 2), (4, 2), (4, 4), (3, 4)]), 2, 0)]))


def two_point_ring(dissolve):
    """a dangling edge: forward and backward slot of one unique edge, face 5 on both sides"""
    rings = ring_set([(5, [(0, 0), (3, 1)])])
    return rings, dissolve, (answer([], n_dissolved=1) if dissolve else answer([([(0, 0), (3, 1)], 5, 5)]))


def tiny_rings():
    """an empty ring first, a one-point ring, an empty ring in the middle and at the end: one zero-length edge, no chain"""
    return ring_set([(1, []), (3, [(7, 7)]), (4, []), (2, [])]), False, answer([], n_zero_edges=1)


def tiny_rings_and_a_triangle():
    """the same round a triangle: the ring of a point slot is found across empty rings"""
    rings = ring_set([(1, []), (3, [(7, 7)]), (4, []), (6, [(0, 0), (6, 0), (0, 6)]), (2, [])])
    return rings, False, answer([([(0, 0), (0, 6), (6, 0), (0, 0)], 0, 6)], n_closed=1, n_zero_edges=1)


def ring_twice():
    """the triangle as face 1, then as face 2: every unique edge has two slots of one kind; the smaller slot names the face"""
    tri = [(0, 0), (6, 0), (0, 6)]
    return ring_set([(1, tri), (2, tri)]), False, answer([([(0, 0), (0, 6), (6, 0), (0, 0)], 0, 1)], n_closed=1, n_conflicts=3)


def label_change():
    """face 3 below the x axis with a vertex at (2, 0), and a two-point ring of face 1 along (0, 0) - (2, 0) (its backward slot is
    the second one of that edge: one conflict).  Every vertex has two edges; the faces change at (0, 0) and (2, 0): two chains.
    Half-edge 1 walks (0, 0) -> (0, -2) with (3, 0), 4 walks (0, 0) -> (2, 0) with (1, 3)."""
    rings = ring_set([(3, [(0, -2), (4, -2), (4, 0), (2, 0), (0, 0)]), (1, [(0, 0), (2, 0)])])
    return rings, False, answer([([(0, 0), (0, -2), (4, -2), (4, 0), (2, 0)], 3, 0), ([(0, 0), (2, 0)], 1, 3)], n_conflicts=1)


def touching_squares():
    """two squares that touch in (0, 0), where four edges meet: two open chains from (0, 0) back to (0, 0), none closed"""
    rings = ring_set([(1, [(0, 0), (4, 0), (4, 4), (0, 4)]), (2, [(0, 0), (-4, 0), (-4, -4), (0, -4)])])
    return rings, False, answer([([(0, 0), (-4, 0), (-4, -4), (0, -4), (0, 0)], 2, 0), ([(0, 0), (0, 4), (4, 4), (4, 0), (0, 0)], 0, 1)])


# ---- disjoint loops: the answer from the construction ---------------------------------------------------------------------
def loops_answer(loops):
    """loops = [(face, points)]: simple closed loops that touch nothing, the face on the left of the points' order"""
    chains = []
    for face, pts in loops:
        n = len(pts)
        lo, hi, k, fwd = min((min(pts[i], pts[(i + 1) % n]), max(pts[i], pts[(i + 1) % n]), i, pts[i] < pts[(i + 1) % n]) for i in range(n))
        if fwd:  # the ring walks lo -> hi: the chain follows the ring from slot k
            chain = [pts[(k + j) % n] for j in range(n + 1)]
        else:  # the ring walks hi -> lo: the chain runs against it from slot k + 1
            chain = [pts[(k + 1 - j) % n] for j in range(n + 1)]
        chains.append(((lo, hi), chain, face if fwd else 0, 0 if fwd else face))
    chains.sort()
    return answer([c[1:] for c in chains], n_closed=len(chains))


def circle(n, radius=float(1 << 40), centre=(0, 0)):
    """n distinct lattice points counter-clockwise on a circle"""
    ang = 2.0 * np.pi * np.arange(n) / n
    pts = np.stack([np.rint(radius * np.cos(ang)) + centre[0], np.rint(radius * np.sin(ang)) + centre[1]], axis=1).astype(np.int64)
    return [tuple(p) for p in pts.tolist()]


def loop(n, rotate, clockwise, face=4):
    """one loop of n edges given from point `rotate`, counter-clockwise (face inside) or clockwise (face outside)"""
    pts = circle(n)
    pts = pts[rotate:] + pts[:rotate]
    if clockwise:
        pts = pts[::-1]
    loops = [(face, pts)]
    return ring_set(loops), False, loops_answer(loops)


def odd_face_loops():
    """disjoint triangles with every face of rings_planar.ODD_FACES, every other one clockwise; a ring of face 0 gives an
    edge with 0 on both sides"""
    loops = []
    for k, f in enumerate(P.ODD_FACES + P.ODD_FACES):
        x = 100 * k
        tri = [(x, 0), (x + 60, 0), (x, 60)]
        loops.append((f, tri[::-1] if k % 2 else tri))
    return ring_set(loops), False, loops_answer(loops)


def domain_corners():
    """a square with its corners at the ends of the coordinate range, given from the upper right corner, and one inside it clockwise"""
    T = LIM - 1
    loops = [(9, [(T, T), (-LIM, T), (-LIM, -LIM), (T, -LIM)]), (9, [(T - 1, T - 1), (T - 1, -LIM + 1), (-LIM + 1, -LIM + 1), (-LIM + 1, T - 1)])]
    return ring_set(loops), False, loops_answer(loops)


HAND = {"squares-equal": lambda: two_squares(1, 1, False), "squares-equal-dissolve": lambda: two_squares(1, 1, True),
        "squares-different": lambda: two_squares(1, 2, False), "squares-different-dissolve": lambda: two_squares(1, 2, True),
        "hole": square_with_hole, "rect": rect_rings, "two-point": lambda: two_point_ring(False), "two-point-dissolve": lambda: two_point_ring(True),
        "tiny": tiny_rings, "tiny-and-triangle": tiny_rings_and_a_triangle, "twice": ring_twice, "label-change": label_change,
        "touching": touching_squares, "odd-faces": odd_face_loops, "corners": domain_corners}
for _n in LOOP_SIZES:
    for _cw in (False, True):
        HAND["loop-%d-%s" % (_n, "cw" if _cw else "ccw")] = (lambda n, cw: lambda: loop(n, (2 * n) // 3 + 1, cw))(_n, _cw)


def long_loops():
    """{name: case} of the 100 003-edge loops (the twin's and the device's: the Python definition takes a while on them)"""
    return {"loop-%d-%s" % (LONG_LOOP, "cw" if cw else "ccw"): loop(LONG_LOOP, 70_001, cw) for cw in (False, True)}


# ---- large ring sets for the device against the twin --------------------------------------------------------------------------
def triangle_rings(n, width=1000, pitch=10):
    """n disjoint triangles on a raster, every third one clockwise, faces column + 1: n closed loops of 3 edges"""
    c = np.arange(n, dtype=np.int64)
    x0, y0 = pitch * (c % width), pitch * (c // width)
    tri = np.stack([np.stack([x0, y0], 1), np.stack([x0 + 6, y0], 1), np.stack([x0, y0 + 6], 1)], axis=1)  # [n, 3, 2]
    back = (c % 3) == 2
    tri[back] = tri[back][:, ::-1]
    return (3 * np.arange(n + 1)).astype(np.uint32), tri.reshape(-1, 2), (c % width + 1).astype(np.int32)


def junction_rings(n):
    """n two-point rings from one hub to n different tips, faces k + 1: n dangling edges on one junction of degree n"""
    k = np.arange(n, dtype=np.int64)
    xy = np.zeros((n, 2, 2), np.int64)
    xy[:, 1, 0], xy[:, 1, 1] = 1 + k % 1000, 1 + k // 1000 + 2000 * (k % 1000)  # (distinct points, none on the hub)
    xy[1::2] = xy[1::2, ::-1]  # every other ring starts at its tip
    return (2 * np.arange(n + 1)).astype(np.uint32), xy.reshape(-1, 2), (k + 1).astype(np.int32)
