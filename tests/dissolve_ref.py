"""Merging faces by class and re-joining chains (rj_map_dissolve), by definition: plain Python integers, dicts and lists,
nothing shared with rayjoin_amd/csrc/rj_dissolve.h.  Where the header sorts chain ends, this keeps a dict of the
half-chains that start at every point; where it doubles pointers, this follows next one step at a time.

dissolve_ref(xy, row_index, left, right, classes=None, flags=0) -> Result or raises Invalid (Unmapped, a kind of Invalid
that carries n_unmapped, for a nonzero label outside the class table).

The definition.  class(0) = 0; without a table class(f) = f, with one class(f) = table[f] for 0 < f < len(table), and
every other nonzero label is unmapped.  A chain whose points are all equal is skipped; of the others a chain is kept
unless its two classes are equal and KEEP_EQUAL is not set.  Half-chain h = 2 c walks chain c first -> last with classes
(L, R), h = 2 c + 1 last -> first with (R, L); it starts at the chain's first / last point.  h arrives at the start point
of h ^ 1; when exactly two kept half-chains start there, h ^ 1 and one other g, and g has the classes of h, next(h) = g;
otherwise h ends.  Walks are the maximal sequences under next; an open walk is read from its first half-chain, a closed
one from its smallest.  Of a walk and its twin walk (the twins in reverse order) the one with the smaller leader is an
output chain; chains ascend by leader.  Its points: each half-chain's points in its direction without the last, then
the last point of the last half-chain."""
import numpy as np

COUNTS = ("n_kept", "n_dropped", "n_skipped", "n_chains", "n_points", "n_closed", "n_classes", "n_unmapped")
KEEP_EQUAL = 1
NONE = 0xFFFFFFFF
LIM = 1 << 46


class Invalid(ValueError):
    pass


class Unmapped(Invalid):
    def __init__(self, n):
        super().__init__("%d unmapped chain sides" % n)
        self.n_unmapped = n


class Result:
    """classes: a list of dicts (label, n_sides, area2), ascending by unsigned label; left / right (int32), xy [n, 2] int64,
    row_index, origin (uint32 per output chain), chain_out (uint32 per INPUT chain); counts; walks: per output chain the
    list of its half-chains; closed: per output chain, is it a closed walk"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def unsigned(label):
    return label % (1 << 32)


def dissolve_ref(xy, row_index, left, right, classes=None, flags=0):
    pts = [(int(x), int(y)) for x, y in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    left, right = [int(v) for v in np.asarray(left).tolist()], [int(v) for v in np.asarray(right).tolist()]
    table = None if classes is None else [int(v) for v in np.asarray(classes).tolist()]
    nc = max(0, len(row) - 1)
    if flags & ~KEEP_EQUAL:
        raise Invalid("flags")
    if table is not None and len(table) == 0:
        raise Invalid("a table without labels")
    counts = dict.fromkeys(COUNTS, 0)
    if nc == 0:
        if pts:
            raise Invalid("points without chains")
        none = np.zeros(0, np.int32)
        return Result(classes=[], left=none, right=none, xy=np.zeros((0, 2), np.int64), row_index=np.zeros(1, np.uint32), origin=np.zeros(0, np.uint32),
                      chain_out=np.zeros(0, np.uint32), counts=counts, walks=[], closed=[])
    if nc > len(pts) or row[0] != 0 or row[-1] != len(pts) or any(b >= e for b, e in zip(row, row[1:])):
        raise Invalid("row_index")
    if any(not -LIM <= v < LIM for p in pts for v in p):
        raise Invalid("coordinate")

    unmapped = 0

    def cls(f):
        nonlocal unmapped
        if f == 0 or table is None:
            return f
        if 0 < f < len(table):
            return table[f]
        unmapped += 1
        return 0
    L, R = [cls(f) for f in left], [cls(f) for f in right]
    if unmapped:
        raise Unmapped(unmapped)
    chain = [pts[b:e] for b, e in zip(row, row[1:])]
    kept = []
    for c in range(nc):
        if all(p == chain[c][0] for p in chain[c]):
            counts["n_skipped"] += 1
        elif L[c] == R[c] and not flags & KEEP_EQUAL:
            counts["n_dropped"] += 1
        else:
            kept.append(c)
    counts["n_kept"] = len(kept)

    def points(h):
        return chain[h >> 1][::-1] if h & 1 else chain[h >> 1]

    def pair(h):
        return (R[h >> 1], L[h >> 1]) if h & 1 else (L[h >> 1], R[h >> 1])
    starting = {}
    for c in kept:
        for h in (2 * c, 2 * c + 1):
            starting.setdefault(points(h)[0], []).append(h)
    nxt = {}
    for c in kept:
        for h in (2 * c, 2 * c + 1):
            there = starting[points(h)[-1]]
            assert h ^ 1 in there
            others = [g for g in there if g != h ^ 1]
            nxt[h] = others[0] if len(there) == 2 and pair(others[0]) == pair(h) else None
    has_pred = {g for g in nxt.values() if g is not None}
    walk_of, walks = {}, []
    for h in sorted(nxt):  # the open walks from their first half-chains
        if h not in has_pred:
            w = [h]
            while nxt[w[-1]] is not None:
                w.append(nxt[w[-1]])
            walks.append((w, False))
            for g in w:
                walk_of[g] = len(walks) - 1
    for h in sorted(nxt):  # what is left lies on cycles: ascending h meets the smallest half-chain of each first
        if h not in walk_of:
            w = [h]
            while nxt[w[-1]] != h:
                w.append(nxt[w[-1]])
            walks.append((w, True))
            for g in w:
                walk_of[g] = len(walks) - 1
    out = sorted((w for w in walks if w[0][0] < walks[walk_of[w[0][0] ^ 1]][0][0]), key=lambda w: w[0][0])
    assert all([g ^ 1 for g in w[::-1]] == rotated(walks[walk_of[w[0] ^ 1]][0], w[-1] ^ 1) for w, _ in out)
    oxy, orow, oleft, oright, origin, chain_out = [], [0], [], [], [], [NONE] * nc
    for k, (w, closed) in enumerate(out):
        for h in w:
            oxy.extend(points(h)[:-1])
            chain_out[h >> 1] = (k << 1) | (h & 1)
        oxy.append(points(w[-1])[-1])
        orow.append(len(oxy))
        oleft.append(pair(w[0])[0])
        oright.append(pair(w[0])[1])
        origin.append(w[0] >> 1)
        counts["n_closed"] += closed
    counts["n_chains"], counts["n_points"] = len(out), len(oxy)
    assert len(oxy) == sum(len(chain[c]) - 1 for c in kept) + len(out) and all(chain_out[c] != NONE for c in kept)
    # the class records
    area2, sides = {}, {}
    for c in kept:
        s = sum(ax * by - ay * bx for (ax, ay), (bx, by) in zip(chain[c], chain[c][1:]))
        for k, sign in ((L[c], 1), (R[c], -1)):
            if k != 0:
                area2[k] = area2.get(k, 0) + sign * s
                sides[k] = sides.get(k, 0) + 1
    records = [dict(label=k, n_sides=sides[k], area2=area2[k]) for k in sorted(area2, key=unsigned)]
    counts["n_classes"] = len(records)
    return Result(classes=records, left=np.array(oleft, np.int32), right=np.array(oright, np.int32), xy=np.array(oxy, np.int64).reshape(-1, 2),
                  row_index=np.array(orow, np.uint32), origin=np.array(origin, np.uint32), chain_out=np.array(chain_out, np.uint32), counts=counts,
                  walks=[w for w, _ in out], closed=[c for _, c in out])


def rotated(w, first):
    """the closed walk w read from `first`; an open walk as it is"""
    k = w.index(first)
    return w[k:] + w[:k]


def canonical(xy, row_index, left, right):
    """a chain map up to digitisation: consecutive duplicate points removed, each chain in the smaller of its two directions
    (left / right swapped with it), closed chains rotated to their smallest point, the chains sorted -> a list of
    (points tuple, left, right)"""
    pts = [tuple(p) for p in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    out = []
    for c, (b, e) in enumerate(zip(row, row[1:])):
        p = [q for k, q in enumerate(pts[b:e]) if k == 0 or q != pts[b + k - 1]]
        le, ri = int(left[c]), int(right[c])
        both = []
        for q, a, z in ((p, le, ri), (p[::-1], ri, le)):
            if len(q) > 1 and q[0] == q[-1]:
                ring = q[:-1]
                k = ring.index(min(ring))
                q = ring[k:] + ring[:k] + [ring[k]]
            both.append((tuple(q), a, z))
        out.append(min(both))
    return sorted(out)
