"""Hand-built chain maps for the face-ring tests (tests/test_rings.py, tests/test_gpu_rings.py): each is
(xy int64 [np, 2], row_index uint32, left int32, right int32).  The answers are written out in tests/test_rings.py."""
import numpy as np

NECKLACE_SIZES = (1, 2, 63, 64, 65, 129, 1000)


def chain_map(chains):
    """chains = [(points, left, right)] -> the four arrays"""
    xy, row, left, right = [], [0], [], []
    for pts, le, ri in chains:
        xy.extend(pts)
        row.append(len(xy))
        left.append(le)
        right.append(ri)
    return (np.array(xy, np.int64).reshape(-1, 2), np.array(row, np.uint32), np.array(left, np.int32), np.array(right, np.int32))


def rect_output_map(U=1 << 20):
    """the intersection's output map of the two-rectangle pair of tests/test_overlay_map.py, as written out there"""
    s = lambda pts: [(x * U, y * U) for x, y in pts]  # noqa: E731
    return chain_map([(s([(4, 2), (4, 4), (3, 4)]), 2, 0), (s([(3, 4), (2, 4)]), 1, 0), (s([(3, 2), (4, 2)]), 2, 0),
                      (s([(2, 4), (2, 2), (3, 2)]), 1, 0), (s([(3, 2), (3, 4)]), 1, 2)])


def square_with_hole():
    """face 1 between two squares, face 2 inside the inner one"""
    return chain_map([([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], 1, 0), ([(3, 3), (6, 3), (6, 6), (3, 6), (3, 3)], 2, 1)])


def dangling():
    """a square and a chain that hangs from its corner into the outside"""
    return chain_map([([(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], 1, 0), ([(0, 0), (-3, -3)], 0, 0)])


def crossing():
    """two squares that touch in one vertex of degree 4"""
    return chain_map([([(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], 1, 0), ([(0, 0), (-4, 0), (-4, -4), (0, -4), (0, 0)], 2, 0)])


def closed_chain():
    return chain_map([([(0, 0), (6, 0), (0, 6), (0, 0)], 7, 0)])


def zero_length_edges():
    """a triangle of three chains: the first starts, the last ends with a zero-length edge"""
    return chain_map([([(0, 0), (0, 0), (6, 0)], 1, 0), ([(6, 0), (0, 6)], 1, 0), ([(0, 6), (0, 0), (0, 0)], 1, 0)])


def one_point_chain():
    """the triangle and a chain whose points are all equal"""
    return chain_map([([(0, 0), (6, 0), (0, 6), (0, 0)], 7, 0), ([(9, 9), (9, 9)], 3, 4), ([(0, 6), (0, 6), (0, 6)], 7, 7)])


def star(spokes=40, radius=1000):
    """dangling spokes on one vertex, every other one digitised towards the hub"""
    chains = []
    for k in range(spokes):
        a = 2.0 * np.pi * k / spokes + 0.01
        tip = (int(round(radius * np.cos(a))), int(round(radius * np.sin(a))))
        chains.append(([(0, 0), tip] if k % 2 == 0 else [tip, (0, 0)], 0, 0))
    return chain_map(chains)


def necklace(n, seed=7, radius=1_000_000):
    """a convex 3n-gon, counter-clockwise, face 1 inside: n chains of three edges each, in shuffled file order, about
    half of them digitised backwards (left and right swapped to match).  -> (the map, twice the polygon's area)"""
    rng = np.random.default_rng(seed + n)
    m = 3 * n
    ang = 2.0 * np.pi * np.arange(m) / m
    V = [(int(round(radius * np.cos(a))), int(round(radius * np.sin(a)))) for a in ang]
    chains = []
    for i in rng.permutation(n).tolist():
        pts = [V[(3 * i + k) % m] for k in range(4)]
        chains.append((pts[::-1], 0, 1) if rng.random() < 0.5 else (pts, 1, 0))
    area2 = sum(V[k][0] * V[(k + 1) % m][1] - V[k][1] * V[(k + 1) % m][0] for k in range(m))
    return chain_map(chains), area2


HAND = {"rect": rect_output_map, "hole": square_with_hole, "dangling": dangling, "crossing": crossing, "closed": closed_chain,
        "zero-edge": zero_length_edges, "one-point": one_point_chain, "star": star}


def all_cases():
    """{name: map} of the hand cases and the necklaces"""
    out = {name: f() for name, f in HAND.items()}
    for n in NECKLACE_SIZES:
        out["necklace-%d" % n] = necklace(n)[0]
    return out
