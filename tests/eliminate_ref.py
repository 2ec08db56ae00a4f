"""Merging sliver faces into a neighbour (rj_map_eliminate), by definition: plain Python integers, dicts and math.isqrt,
nothing shared with rayjoin_amd/csrc/rj_eliminate.h.  Where the header sorts chain sides and sums by key, this keeps a
dict per face; where it jumps pointers, this follows them one step at a time and keeps the path.

eliminate_ref(xy, row_index, left, right, tol, flags=0) -> Result or raises Invalid; tol a Python int in [0, 2^128).

The definition.  A face is a label other than 0 that occurs in left or right; faces are numbered by ascending
(label mod 2^32), and "smaller" means that order.  Of chain c over its edges p_i -> p_i+1: S(c) = the sum of
cross(p_i, p_i+1), L(c) = the sum of isqrt(dx^2 + dy^2).  area2(f) = the sum of S(c) over left[c] == f minus the sum over
right[c] == f.  f is a sliver when 0 <= area2(f) <= tol; area2(f) < 0 is NEGATIVE and never a sliver.  f != g, both not 0,
are neighbours when some chain has {left, right} = {f, g}; w(f, g) = the sum of L(c) over those chains (0 still makes a
pair).  best(f) of a sliver = the neighbour with the largest w, ties to the smaller min(f, g), then the smaller
max(f, g); a sliver without a neighbour is an ISLAND and stays; every other face has no best.  best(f) = g and
best(g) = f is a mutual pair: the larger area2 stays as a root, a tie goes to the smaller label.  target(f) = the root
reached by following best; target(0) = 0.  One call is one round.  Output labels = the targets; under DROP a chain goes
exactly when its input labels differ and its output labels are equal."""
import math

import numpy as np

COUNTS = ("n_faces", "n_slivers", "n_eliminated", "n_islands", "n_mutual", "n_negative", "n_chains", "n_points", "n_dropped")
DROP = 1
SLIVER, ELIMINATED, ISLAND, NEGATIVE = 1, 2, 4, 8
LIM = 1 << 46
HUGE = (1 << 128) - 1


class Invalid(ValueError):
    pass


class Result:
    """faces: a list of dicts (label, target, best, flags, area2), ascending by unsigned label; left / right: the output
    labels (int32 arrays); xy / row_index / origin: the output map under DROP (None without); counts; S, L: the chain sums"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def unsigned(label):
    return label % (1 << 32)


def chain_sums(pts, row):
    S, L = [], []
    for b, e in zip(row, row[1:]):
        s = l = 0
        for (ax, ay), (bx, by) in zip(pts[b:e - 1], pts[b + 1:e]):
            s += ax * by - ay * bx
            l += math.isqrt((bx - ax) ** 2 + (by - ay) ** 2)
        S.append(s)
        L.append(l)
    return S, L


def eliminate_ref(xy, row_index, left, right, tol, flags=0):
    pts = [(int(x), int(y)) for x, y in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    left, right = [int(v) for v in np.asarray(left).tolist()], [int(v) for v in np.asarray(right).tolist()]
    nc = max(0, len(row) - 1)
    if flags & ~DROP or not 0 <= tol <= HUGE:
        raise Invalid("flags or tol")
    drop = bool(flags & DROP)
    if nc == 0:
        if pts:
            raise Invalid("points without chains")
        return Result(faces=[], left=np.zeros(0, np.int32), right=np.zeros(0, np.int32), xy=np.zeros((0, 2), np.int64) if drop else None,
                      row_index=np.zeros(1, np.uint32) if drop else None, origin=np.zeros(0, np.uint32) if drop else None,
                      counts=dict.fromkeys(COUNTS, 0), S=[], L=[])
    if row[0] != 0 or row[-1] != len(pts) or any(b >= e for b, e in zip(row, row[1:])):
        raise Invalid("row_index")
    if any(not -LIM <= v < LIM for p in pts for v in p):
        raise Invalid("coordinate")
    S, L = chain_sums(pts, row)
    labels = sorted({f for f in left + right if f != 0}, key=unsigned)
    area2 = dict.fromkeys(labels, 0)
    weight = {f: {} for f in labels}
    for c in range(nc):
        le, ri = left[c], right[c]
        if le != 0:
            area2[le] += S[c]
        if ri != 0:
            area2[ri] -= S[c]
        if le != ri and le != 0 and ri != 0:
            weight[le][ri] = weight[le].get(ri, 0) + L[c]
            weight[ri][le] = weight[ri].get(le, 0) + L[c]
    sliver = {f: 0 <= area2[f] <= tol for f in labels}
    best = {}
    for f in labels:
        if sliver[f] and weight[f]:
            # the largest w, then the smaller min, then the smaller max
            best[f] = min(weight[f], key=lambda g: (-weight[f][g], min(unsigned(f), unsigned(g)), max(unsigned(f), unsigned(g))))
    ptr, n_mutual = {}, 0
    for f in labels:
        g = best.get(f, f)
        if g != f and best.get(g) == f:
            n_mutual += unsigned(f) < unsigned(g)
            stays = area2[f] > area2[g] if area2[f] != area2[g] else unsigned(f) < unsigned(g)
            g = f if stays else g
        ptr[f] = g
    target = {0: 0}
    for f in labels:
        path, g = {f}, f
        while ptr[g] != g:
            g = ptr[g]
            assert g not in path, "a cycle survived"
            path.add(g)
        target[f] = g
    faces = []
    for f in labels:
        fl = (SLIVER if sliver[f] else 0) | (ELIMINATED if target[f] != f else 0) | (ISLAND if sliver[f] and not weight[f] else 0) | \
            (NEGATIVE if area2[f] < 0 else 0)
        faces.append(dict(label=f, target=target[f], best=best.get(f, f), flags=fl, area2=area2[f]))
    out_left, out_right = [target[f] for f in left], [target[f] for f in right]
    keep = [not (drop and left[c] != right[c] and out_left[c] == out_right[c]) for c in range(nc)]
    kept = [c for c in range(nc) if keep[c]]
    counts = dict(n_faces=len(labels), n_slivers=sum(sliver.values()), n_eliminated=sum(1 for f in labels if target[f] != f),
                  n_islands=sum(1 for f in labels if sliver[f] and not weight[f]), n_mutual=n_mutual,
                  n_negative=sum(1 for f in labels if area2[f] < 0), n_chains=len(kept), n_points=sum(row[c + 1] - row[c] for c in kept),
                  n_dropped=nc - len(kept))
    out = Result(faces=faces, left=np.array([out_left[c] for c in kept], np.int32), right=np.array([out_right[c] for c in kept], np.int32), xy=None,
                 row_index=None, origin=None, counts=counts, S=S, L=L)
    if drop:
        out.xy = np.array([p for c in kept for p in pts[row[c]:row[c + 1]]], np.int64).reshape(-1, 2)
        out.row_index = np.cumsum([0] + [row[c + 1] - row[c] for c in kept]).astype(np.uint32)
        out.origin = np.array(kept, np.uint32)
    return out


def rounds_ref(xy, row_index, left, right, tol, max_rounds=8):
    """the call repeated under DROP until a round eliminates nothing -> (the last Result, the counts of every round)"""
    per_round = []
    m = (xy, row_index, left, right)
    for _ in range(max_rounds):
        r = eliminate_ref(*m, tol, DROP)
        per_round.append(r.counts)
        m = (r.xy, r.row_index, r.left, r.right)
        if r.counts["n_eliminated"] == 0:
            break
    return r, per_round
