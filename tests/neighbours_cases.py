"""Hand-built labelled chain maps for rj_map_neighbours with the answers written out: the smallest shapes at which each
rule of rayjoin_amd/csrc/rj_neighbours.h can go wrong (HAND), the constructed maps whose keyed sums cross a wave and a
block with their answers from a formula (pair_row, hub), and a label-matrix generator whose answer comes from the
matrix alone, never from a chain (matrix_case).

A hand case is dict(map, pairs, faces, counts):  pairs {(f, g): (w, n_chains, n_nodes)} over the unordered pairs, written
once with n_nodes as RJ_NB_VERTEX gives it -- rook only, the pairs with n_chains == 0 are absent and every n_nodes is 0;
faces {label: (n_sides, area2, perimeter, outer)};  counts the flagged call's n_nodes, n_node_pairs_raw and
max_labels_at_node.  Most maps come from eliminate_cases.grid_map: one two-point chain per cell edge whose sides differ."""
import math

import numpy as np

import eliminate_cases as EC
from rings_cases import chain_map

SIDE = EC.SIDE
DIAGONAL = 199032864766428  # floor(sqrt(2) (2^47 - 1)), eliminate_cases.SQRT_EDGES

CHECKERBOARD = EC.grid_map([0, 10, 20], [0, 10, 20], [[1, 2], [3, 4]])
ISLAND = EC.grid_map([0, 1], [0, 10], [[7]])
# a closed chain inside face 1: its one node is where it starts
CLOSED_INSIDE = chain_map([([(0, 0), (30, 0), (30, 30), (0, 30), (0, 0)], 1, 0), ([(10, 10), (20, 10), (20, 20), (10, 20), (10, 10)], 2, 1)])
# one border in two chains: the vertex between them has degree 2 and still counts
PSEUDO_NODE = chain_map([([(0, 0), (0, 5)], 1, 2), ([(0, 5), (0, 10)], 1, 2)])
NO_FACE_0 = chain_map([([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], 1, 2)])
# label 4 lies on both sides of two chains that end where faces 1 and 2 meet: one label at that node, not three
REPEATED_LABEL = chain_map([([(0, 0), (0, 10)], 1, 2), ([(0, 0), (5, -5)], 4, 4), ([(0, 0), (-5, -5)], 4, 4), ([(0, 0), (0, -9)], 4, 1)])

HAND = {
    # the tables of the issue
    "longer": dict(map=EC.LONGER, pairs={(1, 2): (10, 1, 2), (1, 3): (10, 1, 2), (2, 3): (11, 2, 3)},
                   faces={1: (6, 400, 60, 40), 2: (8, 420, 62, 41), 3: (4, 20, 22, 1)}, counts=(12, 14, 3)),
    "checkerboard": dict(map=CHECKERBOARD, pairs={(1, 2): (10, 1, 2), (1, 3): (10, 1, 2), (2, 4): (10, 1, 2), (3, 4): (10, 1, 2), (1, 4): (0, 0, 1), (2, 3): (0, 0, 1)},
                         faces={f: (4, 200, 40, 20) for f in (1, 2, 3, 4)}, counts=(9, 20, 4)),
    # the bridge inside the hole and the dangle in face 1 have left == right: sides, no length
    "hole": dict(map=EC.HOLE, pairs={(1, 3): (4, 4, 4)}, faces={1: (18, 880, 88, 84), 3: (6, 2, 4, 0)}, counts=(18, 8, 2)),
    "two-part": dict(map=EC.TWO_PART, pairs={(1, 3): (10, 1, 2), (2, 3): (20, 2, 4)}, faces={1: (4, 200, 40, 30), 2: (4, 200, 40, 20), 3: (8, 40, 44, 14)},
                     counts=(10, 12, 2)),
    "zero-length": dict(map=EC.ZERO_LENGTH, pairs={(3, 5): (0, 1, 1)}, faces={3: (5, 20, 22, 22), 5: (5, 200, 40, 40)}, counts=(8, 2, 2)),
    "island": dict(map=ISLAND, pairs={}, faces={7: (4, 20, 22, 22)}, counts=(4, 0, 1)),
    "closed-inside": dict(map=CLOSED_INSIDE, pairs={(1, 2): (40, 1, 1)}, faces={1: (2, 1600, 160, 120), 2: (1, 200, 40, 0)}, counts=(2, 2, 2)),
    "pseudo-node": dict(map=PSEUDO_NODE, pairs={(1, 2): (10, 2, 3)}, faces={1: (2, 0, 10, 0), 2: (2, 0, 10, 0)}, counts=(3, 6, 2)),
    # 3 < 7 < -5 = 2^32 - 5: the entries of face 3 are 7, then -5
    "negative-labels": dict(map=EC.between(-5, 3, 7), pairs={(3, -5): (10, 1, 2), (3, 7): (10, 1, 2)},
                            faces={3: (4, 20, 22, 2), 7: (4, 200, 40, 30), -5: (4, 200, 40, 30)}, counts=(8, 8, 2)),
    "no-face-0": dict(map=NO_FACE_0, pairs={(1, 2): (40, 1, 1)}, faces={1: (1, 200, 40, 0), 2: (1, -200, 40, 0)}, counts=(1, 2, 2)),
    "repeated-label": dict(map=REPEATED_LABEL, pairs={(1, 2): (10, 1, 2), (1, 4): (9, 1, 2), (2, 4): (0, 0, 1)},
                           faces={1: (2, 0, 19, 0), 2: (1, 0, 10, 0), 4: (5, 0, 9, 0)}, counts=(5, 10, 3)),
    "big": dict(map=EC.BIG, pairs={}, faces={1: (1, SIDE * SIDE, 2 * SIDE + DIAGONAL, 2 * SIDE + DIAGONAL)}, counts=(1, 0, 1)),
}


def sqrt_answer():
    """eliminate_cases.sqrt_map: face k + 1 is one edge of SQRT_EDGES against face 0, every edge from one corner -- rook only no
    pair at all, flagged every two faces meet at that corner.  The edge (0, 0, 0) ends where it starts: 10 nodes."""
    n = len(EC.SQRT_EDGES)
    return dict(map=EC.sqrt_map(), pairs={(f, g): (0, 0, 1) for f in range(1, n + 1) for g in range(f + 1, n + 1)},
                faces={k + 1: (1, EC.LIM * (dx - dy), r, r) for k, (dx, dy, r) in enumerate(EC.SQRT_EDGES)},  # cross(c, c + d) with c = (-2^46, -2^46)
                counts=(n, n * (n - 1), n))


# ---- structure: what a wave and a block can get wrong ---------------------------------------------------------------------
PAIR_ROWS = (1, 63, 64, 65, 257, 1000)
HUBS = (2, 3, 63, 64, 65, 257)


def pair_row(n):
    """the faces 1 and 2 separated by n chains of length 1 end to end: one pair, summed over n chains"""
    m = chain_map([([(0, k), (0, k + 1)], 1, 2) for k in range(n)])
    return dict(map=m, pairs={(1, 2): (n, n, n + 1)}, faces={1: (n, 0, n, 0), 2: (n, 0, n, 0)}, counts=(n + 1, 2 * (n + 1), 2))


def hub(n):
    """n spokes from (0, 0), wedge k + 1 between spoke k (its right-hand border, walked outwards: the wedge is on the left) and
    spoke k + 1 mod n.  Every two wedges meet at the hub; neighbours in the cycle share a spoke and its tip."""
    tips = [(int(round(1e6 * math.cos(2 * math.pi * k / n))) + k, int(round(1e6 * math.sin(2 * math.pi * k / n)))) for k in range(n)]
    length = [math.isqrt(x * x + y * y) for x, y in tips]
    m = chain_map([([(0, 0), tips[k]], k + 1, (k - 1) % n + 1) for k in range(n)])
    pairs = {(f, g): (0, 0, 1) for f in range(1, n + 1) for g in range(f + 1, n + 1)}
    for k in range(n):  # spoke k separates wedge k + 1 from wedge k (mod n)
        f, g = sorted((k + 1, (k - 1) % n + 1))
        w, chains, nodes = pairs[(f, g)]
        pairs[(f, g)] = (w + length[k], chains + 1, nodes + 1)
    faces = {k + 1: (2, 0, length[k] + length[(k + 1) % n], 0) for k in range(n)}
    return dict(map=m, pairs=pairs, faces=faces, counts=(n + 1, n * (n - 1) + 2 * n, n))


LIMIT_HUB = 65537  # faces at one vertex: 65 537 x 65 536 = 2^32 + 2^16 directed pairs, the first hub that is refused


def limit_hub(n=LIMIT_HUB):
    """n two-point chains from (0, 0), face k + 1 on the left of chain k and 0 on its right: n labels at one node and one at
    every tip, so n_node_pairs_raw = n (n - 1).  Rook only the map has n faces and no pair."""
    k = np.arange(n, dtype=np.int64)
    xy = np.zeros((2 * n, 2), np.int64)
    xy[1::2, 0], xy[1::2, 1] = 1 + k % 1000, 1 + k // 1000
    return xy, (2 * np.arange(n + 1)).astype(np.uint32), (k + 1).astype(np.int32), np.zeros(n, np.int32)


# ---- the label matrix: an answer that never sees a chain ------------------------------------------------------------------
def matrix_case(seed):
    """a random W x H label matrix (up to 40 x 40) over a small alphabet with 0, random increasing xs / ys -> (map, pairs):
    w(f, g) = the cell sides between unequal nonzero neighbours, n_chains their number, n_nodes(f, g) = the lattice corners
    whose four cells are not all equal and hold both labels"""
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.integers(2, 41)), int(rng.integers(2, 41))
    alphabet = [0] + [int(v) for v in rng.choice(np.arange(1, 60), size=int(rng.integers(2, 9)), replace=False)]
    labels = [[int(rng.choice(alphabet)) for _ in range(W)] for _ in range(H)]
    xs = np.cumsum(rng.integers(1, 50, size=W + 1)).tolist()
    ys = np.cumsum(rng.integers(1, 50, size=H + 1)).tolist()
    at = lambda i, j: labels[j][i] if 0 <= i < W and 0 <= j < H else 0  # noqa: E731
    pairs = {}

    def border(f, g, length):
        if f != g and f != 0 and g != 0:
            w, chains, nodes = pairs.get((min(f, g), max(f, g)), (0, 0, 0))
            pairs[(min(f, g), max(f, g))] = (w + length, chains + 1, nodes)
    for j in range(H):
        for i in range(W):
            border(at(i, j), at(i + 1, j), ys[j + 1] - ys[j])
            border(at(i, j), at(i, j + 1), xs[i + 1] - xs[i])
    for j in range(H + 1):
        for i in range(W + 1):
            cells = (at(i - 1, j - 1), at(i, j - 1), at(i - 1, j), at(i, j))
            here = sorted(set(cells) - {0})
            if len(set(cells)) > 1:
                for a, f in enumerate(here):
                    for g in here[a + 1:]:
                        w, chains, nodes = pairs.get((f, g), (0, 0, 0))
                        pairs[(f, g)] = (w, chains, nodes + 1)
    return EC.grid_map(xs, ys, labels), pairs
