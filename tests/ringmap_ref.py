"""The chain map of a set of labelled rings (rj_rings_map) in plain Python: dicts, sorted lists and walks that follow next
one step at a time -- no sort by a comparator, no scan, no pointer doubling.  Independent of rayjoin_amd/csrc/rj_ringmap.h,
whose comment states the definition that both implement; tests/test_ringmap.py holds the header's host twin equal to this,
tests/test_gpu_ringmap.py the device.

Input: ring_row (CSR, n_rings + 1), ring_xy ([n_points, 2]), ring_face (one 32-bit label per ring, on the left of the walk).
Output: dict(xy [n_points, 2] int64, row_index uint32, left int32, right int32, counts)."""
import numpy as np

COUNTS = ("n_chains", "n_points", "n_edges", "n_closed", "n_zero_edges", "n_conflicts", "n_dissolved")
ARRAYS = ("xy", "row_index", "left", "right")


def unique_edges(ring_row, ring_xy, ring_face, dissolve=False):
    """-> ([(lo, hi, left, right)] of the kept edges in their order, n_zero_edges, n_conflicts, n_dissolved)"""
    xy = [(int(x), int(y)) for x, y in np.asarray(ring_xy).reshape(-1, 2).tolist()]
    row = [int(v) for v in ring_row]
    groups, n_zero = {}, 0
    for r in range(len(row) - 1):
        b, e = row[r], row[r + 1]
        for i in range(b, e):
            u, v = xy[i], xy[b if i + 1 == e else i + 1]
            if u == v:
                n_zero += 1
                continue
            lo, hi = (u, v) if u < v else (v, u)
            groups.setdefault((lo, hi), ([], []))[0 if u == lo else 1].append((i, int(ring_face[r])))
    edges, n_conflicts, n_dissolved = [], 0, 0
    for key in sorted(groups):
        fwd, back = groups[key]
        n_conflicts += len(fwd) > 1 or len(back) > 1
        left, right = (min(fwd)[1] if fwd else 0), (min(back)[1] if back else 0)
        if dissolve and left == right:
            n_dissolved += 1
            continue
        edges.append((key[0], key[1], left, right))
    return edges, n_zero, n_conflicts, n_dissolved


def chains_of(edges):
    """-> [(leader, [half-edges in walk order], closed)] ascending by leader, and the functions start(h), faces(h)"""
    def start(h):
        return edges[h >> 1][h & 1]

    def faces(h):
        _, _, le, ri = edges[h >> 1]
        return (ri, le) if h & 1 else (le, ri)

    nh = 2 * len(edges)
    out = {}
    for h in range(nh):
        out.setdefault(start(h), []).append(h)

    def nxt(h):
        o = out[start(h ^ 1)]
        if len(o) != 2:
            return None
        g = o[0] if o[1] == (h ^ 1) else o[1]
        return g if faces(g) == faces(h) else None

    def walk(h0):
        w, g = [h0], nxt(h0)
        while g is not None and g != h0:
            w.append(g)
            g = nxt(g)
        return w

    has_pred = {nxt(h) for h in range(nh)} - {None}
    seen, chains = [False] * nh, []
    for closed in (False, True):  # the open walks from their first half-edges, then what is left: cycles, smallest h first
        for h in range(nh):
            if seen[h] or (not closed and h in has_pred):
                continue
            w = walk(h)
            twin = [g ^ 1 for g in reversed(w)]
            for g in w + twin:
                seen[g] = True
            if closed:
                k = twin.index(min(twin))
                twin = twin[k:] + twin[:k]
            chains.append((w[0], w, closed) if w[0] < twin[0] else (twin[0], twin, closed))
    return sorted(chains), start, faces


def rings_map_ref(ring_row, ring_xy, ring_face, dissolve=False):
    edges, n_zero, n_conflicts, n_dissolved = unique_edges(ring_row, ring_xy, ring_face, dissolve)
    chains, start, faces = chains_of(edges)
    pts, row, left, right = [], [0], [], []
    for leader, w, _ in chains:
        pts += [start(g) for g in w] + [start(w[-1] ^ 1)]
        row.append(len(pts))
        left.append(faces(leader)[0])
        right.append(faces(leader)[1])
    counts = dict(n_chains=len(chains), n_points=len(pts), n_edges=len(edges), n_closed=sum(1 for c in chains if c[2]), n_zero_edges=n_zero,
                  n_conflicts=n_conflicts, n_dissolved=n_dissolved)
    return dict(xy=np.array(pts, np.int64).reshape(-1, 2), row_index=np.array(row, np.uint32), left=np.array(left, np.int32),
                right=np.array(right, np.int32), counts=counts)


def as_map(got):
    """-> (xy, row_index, left, right), the argument order of tests/rings_ref.py"""
    return got["xy"], got["row_index"], got["left"], got["right"]


def assert_same_map(got, want, what=""):
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for name in ARRAYS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)


def canonical_rings(ring_faces, ring_row, ring_xy, area2=None):
    """rings as a sorted list of (face, area2, the cyclic point sequence from its smallest rotation), consecutive repeated
    points removed (they come from zero-length edges): what a map and its round trip have in common"""
    row = [int(v) for v in ring_row]
    xy = [tuple(p) for p in np.asarray(ring_xy).reshape(-1, 2).tolist()]
    out = []
    for r in range(len(row) - 1):
        pts = xy[row[r]:row[r + 1]]
        pts = [p for k, p in enumerate(pts) if p != pts[k - 1] or len(pts) == 1]
        if len(pts) > 1:
            s = min(range(len(pts)), key=lambda k: pts[k:] + pts[:k])
            pts = pts[s:] + pts[:s]
        a2 = sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(pts, pts[1:] + pts[:1])) if area2 is None else area2[r]
        out.append((int(ring_faces[r]), a2, tuple(pts)))
    return sorted(out)


def canonical_rings_np(ring_faces, ring_row, ring_xy, area2):
    """canonical_rings for ring sets of hundreds of thousands of rings, in numpy: the same canonical form (no consecutive
    repeated points, read from the smallest rotation) as a sorted list of (face, area2, the points' int64 bytes).  A ring
    whose smallest point occurs once starts there -- that is its smallest rotation --, found for all rings at once; the few
    rings that pass their smallest point more than once go through the Python comparison of rotations."""
    row = np.asarray(ring_row, np.int64)
    xy = np.ascontiguousarray(ring_xy, np.int64).reshape(-1, 2)
    n_rings, lens = len(row) - 1, np.diff(row)
    ring = np.repeat(np.arange(n_rings), lens)
    at = np.arange(len(xy))
    before = np.where(at == row[ring], row[ring + 1] - 1, at - 1)  # the cyclic predecessor of every point slot
    keep = (xy != xy[before]).any(axis=1) | (lens[ring] == 1)
    xy, ring = xy[keep], ring[keep]
    lens = np.bincount(ring, minlength=n_rings)
    row = np.concatenate([[0], np.cumsum(lens)])
    order = np.lexsort((xy[:, 1], xy[:, 0], ring))  # per ring: its points ascending
    first = order[row[:-1][lens > 0]]  # a slot of the smallest point of every ring that has points
    start = np.zeros(n_rings, np.int64)
    start[lens > 0] = first - row[:-1][lens > 0]
    smallest = np.zeros((n_rings, 2), np.int64)
    smallest[lens > 0] = xy[first]
    times = np.bincount(ring, weights=(xy == smallest[ring]).all(axis=1), minlength=n_rings)
    at = np.arange(len(xy)) - row[ring]
    rotated = np.empty_like(xy)
    rotated[row[ring] + (at - start[ring]) % np.maximum(lens[ring], 1)] = xy
    out = []
    for r in range(n_rings):
        pts = rotated[row[r]:row[r + 1]]
        if times[r] > 1:
            p = [tuple(q) for q in pts.tolist()]
            s = min(range(len(p)), key=lambda k: p[k:] + p[:k])
            pts = np.array(p[s:] + p[:s], np.int64)
        out.append((int(ring_faces[r]), area2[r], pts.tobytes()))
    return sorted(out)
