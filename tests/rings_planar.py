"""Generated chain maps for the face-ring tests (tests/test_rings.py, tests/test_gpu_rings.py), each
(xy int64 [np, 2], row_index uint32, left int32, right int32) as tests/rings_cases.py builds them:

planar_grid_map   a random planar subdivision of a lattice whose faces and areas are known WITHOUT the rings (union-find
                  over the lattice's triangles), sheared or stretched over the whole coordinate range
fan, sliver_fan, tie_fan   one junction with thousands of incidences: directions one unit apart at full range, cross
                  products of one unit between 2^94 products, equal directions that only h orders
path              one ring of exactly 2 n half-chains (the round budget of the pointer doubling at its edge)
long_chains       chains of 100 003 and 50 000 points, runs of repeated points at chain ends
odd_faces         face ids outside [0, 2^31)
triangle_field    more than 2^20 half-chains
"""
import numpy as np

from rings_cases import chain_map

LIM = 1 << 46  # coordinates are in [-LIM, LIM)
SHEAR = ((3, 1), (-1, 2))
P_CHOICES = (0.2, 0.3, 0.35, 0.5, 0.62, 0.75, 0.9)


# ---- 1. random planar maps ------------------------------------------------------------------------------------------
def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def planar_grid_map(rng, W, H, p, frame, A, off):
    """Vertices: the integer points of the (W + 1) x (H + 1) lattice, mapped by v -> A v + off (A an integer matrix of
    positive determinant, so left stays left).  Candidate edges: every horizontal and vertical unit edge and one diagonal
    per cell, (i, j) - (i + 1, j + 1) or (i + 1, j) - (i, j + 1) at random: no two cross, a vertex has degree up to 8.
    Each is kept with probability p; with frame every edge of the lattice's border is kept.

    Faces, without the rings: a cell is two triangles (t = 0 holds its bottom edge, t = 1 its top edge), node
    1 + 2 (j W + i) + t, and node 0 is everything outside the lattice.  The two nodes across an edge that is NOT kept are
    joined (union-find).  The component of node 0 is face 0, the others get 1, 2, ... in shuffled order; an edge's left
    and right are the components of its two nodes.  A triangle has area 1/2 before A, so twice the area of face f != 0
    is det A times its triangle count.

    Chains: edges strung through vertices of degree exactly 2 (there the two faces cannot change), 1 to 12 edges per
    chain from a shuffled edge order, about half of them reversed with left and right swapped, a point repeated with
    probability 0.1 (zero-length edges).

    -> (map, info): info = dict(det, triangles {face: count}, max_degree, n_edges)"""
    diag = rng.integers(0, 2, size=(W, H))
    tri = lambda i, j, t: 1 + 2 * (j * W + i) + t  # noqa: E731
    side = lambda i, j, left_edge: tri(i, j, (1 if left_edge else 0) if diag[i, j] == 0 else (0 if left_edge else 1))  # noqa: E731
    cand = []  # (a, b, node on the left of a -> b, node on the right, on the border)
    for j in range(H + 1):
        for i in range(W):  # (i, j) -> (i + 1, j): above it the bottom edge of cell (i, j), below it the top edge of cell (i, j - 1)
            cand.append(((i, j), (i + 1, j), tri(i, j, 0) if j < H else 0, tri(i, j - 1, 1) if j > 0 else 0, j in (0, H)))
    for i in range(W + 1):
        for j in range(H):  # (i, j) -> (i, j + 1): on its left the right edge of cell (i - 1, j), on its right the left edge of cell (i, j)
            cand.append(((i, j), (i, j + 1), side(i - 1, j, False) if i > 0 else 0, side(i, j, True) if i < W else 0, i in (0, W)))
    for i in range(W):
        for j in range(H):
            if diag[i, j] == 0:  # direction (1, 1): the triangle with the top edge on its left
                cand.append(((i, j), (i + 1, j + 1), tri(i, j, 1), tri(i, j, 0), False))
            else:  # direction (-1, 1): the triangle with the bottom edge on its left
                cand.append(((i + 1, j), (i, j + 1), tri(i, j, 0), tri(i, j, 1), False))
    keep = rng.random(len(cand)) < p
    parent = list(range(1 + 2 * W * H))
    edges = []
    for k, (a, b, nl, nr, border) in enumerate(cand):
        if keep[k] or (frame and border):
            edges.append((a, b, nl, nr))
        else:
            ra, rb = _find(parent, nl), _find(parent, nr)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)  # (node 0 stays the root of its component)
    roots = sorted({_find(parent, n) for n in range(len(parent))} - {0})
    ids = {0: 0}
    for r, f in zip(roots, (rng.permutation(len(roots)) + 1).tolist()):
        ids[r] = f
    face_of_node = [ids[_find(parent, n)] for n in range(len(parent))]
    triangles = {}
    for n in range(1, len(parent)):
        triangles[face_of_node[n]] = triangles.get(face_of_node[n], 0) + 1
    # chains through vertices of degree 2
    at = {}
    for e, (a, b, _, _) in enumerate(edges):
        at.setdefault(a, []).append(e)
        at.setdefault(b, []).append(e)
    used = [False] * len(edges)

    def step(v, e):
        """edge e walked from v -> (the vertex it reaches, the face on its left, the face on its right)"""
        a, b, nl, nr = edges[e]
        return (b, face_of_node[nl], face_of_node[nr]) if v == a else (a, face_of_node[nr], face_of_node[nl])

    chains = []
    for e0 in rng.permutation(len(edges)).tolist():
        if used[e0]:
            continue
        want = int(rng.integers(1, 13))
        used[e0] = True
        v, le, ri = step(edges[e0][0], e0)
        pts, n = [edges[e0][0], v], 1
        for forward in (True, False):
            while n < want:
                end = pts[-1] if forward else pts[0]
                more = [e for e in at[end] if not used[e]]
                if len(at[end]) != 2 or len(more) != 1:
                    break
                used[more[0]] = True
                v, l2, r2 = step(end, more[0])
                if not forward:
                    l2, r2 = r2, l2  # (walked against the chain)
                assert (l2, r2) == (le, ri)
                pts = pts + [v] if forward else [v] + pts
                n += 1
        if rng.random() < 0.5:
            pts, le, ri = pts[::-1], ri, le
        out = []
        for q in pts:
            out.extend([q] * (2 if rng.random() < 0.1 else 1))
        chains.append(([(A[0][0] * x + A[0][1] * y + off[0], A[1][0] * x + A[1][1] * y + off[1]) for x, y in out], le, ri))
    det = A[0][0] * A[1][1] - A[0][1] * A[1][0]
    assert det > 0 and all(-LIM <= c < LIM for pts, _, _ in chains for q in pts for c in q)
    info = dict(det=det, triangles=triangles, max_degree=max((len(v) for v in at.values()), default=0), n_edges=len(edges))
    return chain_map(chains), info


def full_range_transform(rng, W, H):
    """an integer matrix and an offset that stretch the lattice [0, W] x [0, H] over nearly all of [-2^46, 2^46)^2:
    x = a i + b j spans [0, a W + b H], y = -c i + d j spans [-c W, d H], each just short of 2^47"""
    span = 2 * LIM - 8
    a, b = 3 * span // (4 * W) - int(rng.integers(0, 1000)), span // (4 * H) - int(rng.integers(0, 1000))
    c, d = span // (4 * W) - int(rng.integers(0, 1000)), 3 * span // (4 * H) - int(rng.integers(0, 1000))
    return ((a, b), (-c, d)), (-LIM + 2, -LIM + 2 + c * W)


def draw_planar(seed):
    """the draw of the planar tests: W, H in [2, 60), p from P_CHOICES, a frame and the full-range stretch for about half
    of the seeds each.  -> (map, info); info also holds W, H, p, frame, full_range"""
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(2, 60)), int(rng.integers(2, 60))
    p = float(rng.choice(P_CHOICES))
    frame, full = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    A, off = full_range_transform(rng, W, H) if full else (SHEAR, (int(rng.integers(-1000, 1000)), int(rng.integers(-1000, 1000))))
    m, info = planar_grid_map(rng, W, H, p, frame, A, off)
    info.update(W=W, H=H, p=p, frame=frame, full_range=full)
    return m, info


def face_sums(got):
    """{face: the sum of its rings' area2} as Python ints"""
    sums = {}
    lo, hi = got["rings"]["area2_lo"].tolist(), got["rings"]["area2_hi"].tolist()
    for f, a, b in zip(got["rings"]["face"].tolist(), lo, hi):
        sums[f] = sums.get(f, 0) + ((b << 64) | a)
    return sums


def assert_planar_answer(got, info, skip_face0=False, what=""):
    """the independent answer: no ring mixes faces, no chain is skipped, the faces that have a ring are the union-find's
    components, the rings of face f != 0 sum to det x (triangles of f) and those of face 0 to minus everything else"""
    assert got["counts"]["n_mixed"] == 0 and got["counts"]["n_skipped"] == 0, what
    want = {f: info["det"] * n for f, n in info["triangles"].items() if f != 0}
    if not skip_face0:
        want[0] = -sum(want.values())
    assert face_sums(got) == want, what


# ---- 2. one junction, many incidences -----------------------------------------------------------------------------------
def _spokes(hub, tips, faces=None):
    """dangling one-edge chains hub - tip, every other one digitised towards the hub"""
    return [([hub, t] if k % 2 == 0 else [t, hub], 0 if faces is None else faces[k][0], 0 if faces is None else faces[k][1])
            for k, t in enumerate(tips)]


def fan(n):
    """hub (-2^46, -2^46); n spokes to (2^46 - 1, 2^46 - 1 - k) and n - 1 to (2^46 - 1 - k, 2^46 - 1): 2 n - 1 directions of
    length 2^47, pairwise non-parallel, neighbours one unit apart; all faces 0.  One ring of 2 (2 n - 1) half-chains, area2 0."""
    T = LIM - 1
    return chain_map(_spokes((-LIM, -LIM), [(T, T - k) for k in range(n)] + [(T - k, T) for k in range(1, n)]))


def sliver_fan(n, seed=5):
    """hub (-2^46, -2^46), spokes (D - j, D - j - 1) from it, D = 2^47 - 1, j < n, in shuffled file order: the cross
    product of spokes j and j' is j - j', a few units between two products of 2^94 -- 0 for a comparator in double"""
    D = 2 * LIM - 1
    order = np.random.default_rng(seed).permutation(n).tolist()
    return chain_map(_spokes((-LIM, -LIM), [(-LIM + D - j, -LIM + D - j - 1) for j in order]))


def tie_fan(n, around=300, seed=11):
    """two hubs.  From each, n chains along the direction (1, 2) with different lengths (to (k + 1, 2 (k + 1)): only h
    orders them) in shuffled order, and `around` spokes in general position; the first hub's chains have faces drawn
    from {3, 7} (its ring mixes faces), the second hub's all have face 5."""
    rng = np.random.default_rng(seed)
    chains = []
    for hub, mixed in (((0, 0), True), ((1 << 30, -(1 << 29)), False)):
        tips = [(k + 1, 2 * (k + 1)) for k in range(n)]
        for k in range(around):
            a = 2.0 * np.pi * (k + 0.37) / around
            tips.append((int(round(1e6 * np.cos(a))) + k, int(round(1e6 * np.sin(a)))))
        tips = [(hub[0] + tips[i][0], hub[1] + tips[i][1]) for i in rng.permutation(len(tips)).tolist()]
        faces = [(int(rng.choice((3, 7))), int(rng.choice((3, 7)))) if mixed else (5, 5) for _ in tips]
        chains.extend(_spokes(hub, tips, faces))
    return chain_map(chains)


# ---- 3. the round budget -----------------------------------------------------------------------------------------------
def path(n):
    """n one-edge chains end to end that do not close, every third digitised backwards: one ring of exactly 2 n half-chains"""
    V = [(k, (k * 37) % 11) for k in range(n + 1)]
    return chain_map([([V[k + 1], V[k]] if k % 3 == 1 else [V[k], V[k + 1]], 0, 0) for k in range(n)])


# ---- 4. long chains ----------------------------------------------------------------------------------------------------
def long_chains(m=100_002, tail=50_000, run=75):
    """two concentric closed chains of m + 1 points (face 1 between them, face 2 inside; the inner one digitised clockwise),
    an open chain of `tail` points hanging from the outer chain's first point into face 0, `run` copies of its first point in
    front of the hanging chain and run + 5 copies of its last point behind the inner chain"""
    ang = 2.0 * np.pi * np.arange(m) / m
    R = float(1 << 40)
    outer = np.stack([np.rint(R * np.cos(ang)), np.rint(R * np.sin(ang))], axis=1).astype(np.int64)
    inner = np.stack([np.rint(0.5 * R * np.cos(ang)), np.rint(0.5 * R * np.sin(ang))], axis=1).astype(np.int64)
    outer, inner = [tuple(q) for q in outer.tolist()], [tuple(q) for q in inner.tolist()]
    hang = [outer[0]] * run + [(outer[0][0] + 1000 * k, 777 * (k % 2) + 3 * (k % 5)) for k in range(1, tail - run + 1)]
    inner_cw = (inner + inner[:1])[::-1] + inner[:1] * (run + 5)
    return chain_map([(outer + outer[:1], 1, 0), (hang, 0, 0), (inner_cw, 1, 2)])


def shoelace(xy):
    """twice the signed area of the closed polygon xy [n, 2], exactly (a Python int; coordinates below 2^46)"""
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    # x yn - xn y with 23-bit low limbs: every partial product and every partial sum over 2^14 terms stays below 2^63
    total = 0
    for (a, b), sign in (((x, yn), 1), ((xn, y), -1)):
        ah, al, bh, bl = a >> 23, a & 0x7FFFFF, b >> 23, b & 0x7FFFFF
        for s in range(0, len(a), 1 << 14):
            t = slice(s, s + (1 << 14))
            total += sign * ((int((ah[t] * bh[t]).sum()) << 46) + (int((ah[t] * bl[t] + al[t] * bh[t]).sum()) << 23) + int((al[t] * bl[t]).sum()))
    return total


# ---- 5. faces outside [0, 2^31) ------------------------------------------------------------------------------------------
ODD_FACES = (-1, -(1 << 31), (1 << 31) - 1, 5, -3, 0)


def odd_faces(n=14, seed=3):
    """n disjoint closed triangles whose left / right are drawn from ODD_FACES (the first six chains have every one of
    them on the left once), about a third digitised clockwise"""
    rng = np.random.default_rng(seed)
    chains = []
    for k in range(n):
        x = 100 * k
        pts = [(x, 0), (x + 60, 0), (x, 60), (x, 0)]
        le = ODD_FACES[k] if k < len(ODD_FACES) else int(rng.choice(ODD_FACES))
        chains.append((pts[::-1] if rng.random() < 0.33 else pts, le, int(rng.choice(ODD_FACES))))
    return chain_map(chains)


# ---- 6. more than 2^20 half-chains ----------------------------------------------------------------------------------------
def triangle_field(n, width=1000, pitch=10):
    """n closed three-edge chains on a raster `width` wide: chain c in column c % width, row c // width, every third one
    digitised clockwise, both faces column + 1 -- 2 n rings of one half-chain each, 2 n / width per face"""
    c = np.arange(n, dtype=np.int64)
    x0, y0 = pitch * (c % width), pitch * (c // width)
    tri = np.stack([np.stack([x0, y0], 1), np.stack([x0 + 6, y0], 1), np.stack([x0, y0 + 6], 1), np.stack([x0, y0], 1)], axis=1)  # [n, 4, 2]
    back = (c % 3) == 2
    tri[back] = tri[back][:, ::-1]
    face = (c % width + 1).astype(np.int32)
    return tri.reshape(-1, 2), (4 * np.arange(n + 1)).astype(np.uint32), face, face.copy()
