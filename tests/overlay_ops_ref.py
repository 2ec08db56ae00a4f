"""Test-side restatement of the overlay OPERATIONS (test infrastructure): the chains walked exactly as
overlay_map_ref.pieces walks them, but keeping EVERY piece with its label; `how` and `by` are applied afterwards, piece by
piece, with the definitions written as plain Python -- independent of the per-edge rule, the truth table and the masks
the product uses (rayjoin_amd/csrc/rj_overlay_ops.h), so the two formulations check each other.

A side of a piece of map im has the ordered pair (f0, f1) = (face of map 0, face of map 1): (chain's face, label) for
im == 0, (label, chain's face) for im == 1.  Its key is by(f0, f1) when how selects the pair and the key is not (0, 0),
else None.  A piece is kept when its two keys differ.  Faces: the keys of kept pieces, ascending by
((uint32)f0 << 32) | (uint32)f1, from 1."""
import numpy as np

HOWS = ("intersection", "union", "difference", "symmetric_difference", "identity")
BYS = ("pair", "map0", "map1")

SELECTED = {
    "intersection": lambda f0, f1: f0 != 0 and f1 != 0,
    "union": lambda f0, f1: f0 != 0 or f1 != 0,
    "difference": lambda f0, f1: f0 != 0 and f1 == 0,
    "symmetric_difference": lambda f0, f1: (f0 != 0) != (f1 != 0),
    "identity": lambda f0, f1: f0 != 0,
}
NAMED = {"pair": lambda f0, f1: (f0, f1), "map0": lambda f0, f1: (f0, 0), "map1": lambda f0, f1: (0, f1)}


def all_pieces(scaled_maps, xsects_sorted_pair, point_in_polygon_pair):
    """-> [(im, source chain, left face, right face, label, [points])] of EVERY piece, in the writer's order: map 0's
    chains in order, then map 1's; a chain's pieces from its first vertex to its last.  The label of a piece is the
    face, in the other map, of its last vertex, or the mid-point face of the cut it starts at when it holds no vertex."""
    out = []
    for im in range(2):
        m = scaled_maps[im]
        pts = [(int(x), int(y)) for x, y in m.pts.tolist()]
        pip = [int(v) for v in np.asarray(point_in_polygon_pair[im]).tolist()]
        grouped = {}
        for x in xsects_sorted_pair[im]:
            grouped.setdefault(int(x["eid"][im]), []).append((int(x["x_num"]), int(x["y_num"]), int(x["mid_point_polygon_id"])))
        for ic in range(m.n_chains):
            b, e = int(m.row_index[ic]), int(m.row_index[ic + 1])
            left, right = int(m.left[ic]), int(m.right[ic])
            cur, label = [], 0
            for pid in range(b, e):
                label = pip[pid]
                cur.append(pts[pid])
                if pid == e - 1:
                    break
                for x, y, mid in grouped.get(pid - ic, []):
                    cur.append((x, y))
                    out.append((im, ic, left, right, label, cur))
                    cur = [(x, y)]
                    label = mid  # (of the last cut of an edge: DONTKNOW, replaced by the next vertex's face before use)
            out.append((im, ic, left, right, label, cur))
    return out


def side_pairs(im, left, right, label):
    """((f0, f1) of the left side, (f0, f1) of the right side)"""
    return ((left, label), (right, label)) if im == 0 else ((label, left), (label, right))


def key_of(pair, how, by):
    if not SELECTED[how](*pair):
        return None
    k = NAMED[by](*pair)
    return None if k == (0, 0) else k


def kept_pieces(all_, how, by):
    """-> [(im, chain, left key or None, right key or None, unique points)] of the kept pieces"""
    out = []
    for im, ic, left, right, label, pts in all_:
        lp, rp = side_pairs(im, left, right, label)
        kl, kr = key_of(lp, how, by), key_of(rp, how, by)
        if kl == kr:
            continue
        uniq = [pts[0]]
        for p in pts[1:]:
            if p != uniq[-1]:
                uniq.append(p)
        out.append((im, ic, kl, kr, uniq))
    return out


def _sort_key(pair):
    return ((pair[0] & 0xFFFFFFFF) << 32) | (pair[1] & 0xFFFFFFFF)


def output_map(all_, how, by, drop_degenerate=False):
    """the arrays of rj_overlay_map_op, as overlay_map_ref.output_map returns them"""
    ps = kept_pieces(all_, how, by)
    face_pairs = sorted({k for _, _, kl, kr, _ in ps for k in (kl, kr) if k is not None}, key=_sort_key)
    ids = {p: i + 1 for i, p in enumerate(face_pairs)}
    xy, row, left, right, origin = [], [0], [], [], []
    one = 0
    for im, ic, kl, kr, pts in ps:
        if len(pts) < 2:
            one += 1
            if drop_degenerate:
                continue
        xy.extend(pts)
        row.append(len(xy))
        left.append(ids[kl] if kl is not None else 0)
        right.append(ids[kr] if kr is not None else 0)
        origin.append((im << 31) | ic)
    return dict(xy=np.array(xy, dtype=np.int64).reshape(-1, 2), row_index=np.array(row, dtype=np.uint32),
                left=np.array(left, dtype=np.int32), right=np.array(right, dtype=np.int32),
                face_pairs=np.array(face_pairs, dtype=np.int32).reshape(-1, 2), origin=np.array(origin, dtype=np.uint32),
                n_one_point=one)


def cross_sum(pts):
    return sum(pts[i][0] * pts[i + 1][1] - pts[i + 1][0] * pts[i][1] for i in range(len(pts) - 1))


def face_rows(all_, how, by):
    """[(f0, f1, area2)] of rj_overlay_faces_op: +cross on the left key, -cross on the right key of every kept piece"""
    table = {}
    for _, _, kl, kr, pts in kept_pieces(all_, how, by):
        a2 = cross_sum(pts)
        if kl is not None:
            table[kl] = table.get(kl, 0) + a2
        if kr is not None:
            table[kr] = table.get(kr, 0) - a2
    return sorted(((f0, f1, a) for (f0, f1), a in table.items()), key=lambda r: _sort_key(r[:2]))


def cut_boundary_area2(all_, im):
    """{face: twice its area} of map im's faces from map im's OWN pieces (cut points as vertices): what the rows of a
    face sum to under (union, pair) -- the other map's chains inside the face cancel"""
    total = {}
    for jm, _, left, right, _, pts in all_:
        if jm == im:
            a2 = cross_sum(pts)
            if left != 0:
                total[left] = total.get(left, 0) + a2
            if right != 0:
                total[right] = total.get(right, 0) - a2
    return total


# ---- numpy forms, for maps too large for a Python loop (tests/overlay_midsize_check.py) --------------------------------------
# SELECTED / NAMED once more, as array expressions (tests/test_overlay_hard.py holds both forms equal to the plain ones)
SELECTED_NP = {
    "intersection": lambda f0, f1: (f0 != 0) & (f1 != 0),
    "union": lambda f0, f1: (f0 != 0) | (f1 != 0),
    "difference": lambda f0, f1: (f0 != 0) & (f1 == 0),
    "symmetric_difference": lambda f0, f1: (f0 != 0) ^ (f1 != 0),
    "identity": lambda f0, f1: f0 != 0,
}
NAMED_NP = {"pair": lambda f0, f1: (f0, f1), "map0": lambda f0, f1: (f0, np.zeros_like(f1)), "map1": lambda f0, f1: (np.zeros_like(f0), f1)}


def _keys_np(f0, f1, how, by):
    """int64 sort key of a side, -1 where the side has no face in the result"""
    assert (f0 >= 0).all() and (f1 >= 0).all() and (f0 < 1 << 31).all() and (f1 < 1 << 31).all()
    n0, n1 = NAMED_NP[by](f0, f1)
    return np.where(SELECTED_NP[how](f0, f1) & ((n0 != 0) | (n1 != 0)), (n0 << 32) | n1, -1)


def walk_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair):
    """all_pieces() as arrays, per map: the emitted sequence -- per chain its vertices, each followed by the cuts of the
    edge it starts, every cut twice (the end of one piece, the start of the next) -- as X, Y, start (a piece begins
    here), and per piece its source chain, the chain's left and right face and the piece's label"""
    out = []
    for im in range(2):
        m = scaled_maps[im]
        xs = xsects_sorted_pair[im]
        n, npts, nc = len(xs), m.n_points, m.n_chains
        row = m.row_index.astype(np.int64)
        vf = np.asarray(point_in_polygon_pair[im]).astype(np.int64)
        chain_of_point = np.repeat(np.arange(nc, dtype=np.int64), np.diff(row))
        eid = xs["eid"][:, im].astype(np.int64) if n else np.zeros(0, np.int64)
        edges_to = row[1:] - 1 - np.arange(nc)  # edge e belongs to chain c when e < edges_to[c], first such c
        rec_chain = np.searchsorted(edges_to, eid, side="right")
        rec_p1 = eid + rec_chain
        k = np.arange(n, dtype=np.int64)
        before = np.searchsorted(eid, np.arange(npts, dtype=np.int64) - chain_of_point, side="left")  # records ahead of a vertex
        pos_v = np.arange(npts, dtype=np.int64) + 2 * before
        pos_end = rec_p1 + 1 + 2 * k
        total = npts + 2 * n
        X, Y = np.zeros(total, np.int64), np.zeros(total, np.int64)
        X[pos_v], Y[pos_v] = m.pts[:, 0], m.pts[:, 1]
        for off in (0, 1):
            X[pos_end + off], Y[pos_end + off] = xs["x_num"], xs["y_num"]
        start = np.zeros(total, bool)
        start[pos_v[row[:-1]]] = True
        start[pos_end + 1] = True
        n_pieces = n + nc
        assert int(start.sum()) == n_pieces
        piece = np.cumsum(start) - 1
        # the label of a piece is set where it ENDS: at record k (piece k + its chain) the face of the edge's first vertex,
        # or the mid-point face of the record before when that is a cut of the same edge; at a chain's end the last vertex's
        label = np.zeros(n_pieces, np.int64)
        if n:
            same_edge = np.r_[False, eid[1:] == eid[:-1]]
            mid_prev = np.r_[0, xs["mid_point_polygon_id"][:-1].astype(np.int64)]
            label[k + rec_chain] = np.where(same_edge, mid_prev, vf[rec_p1])
        label[np.searchsorted(eid, edges_to, side="left") + np.arange(nc)] = vf[row[1:] - 1]
        piece_chain = np.zeros(n_pieces, np.int64)
        piece_chain[piece[pos_v]] = chain_of_point
        piece_chain[k + rec_chain + 1] = rec_chain  # (a piece between two cuts of one edge holds no vertex)
        out.append(dict(X=X, Y=Y, start=start, piece=piece, label=label, chain=piece_chain,
                        left=m.left.astype(np.int64)[piece_chain], right=m.right.astype(np.int64)[piece_chain]))
    return out


def _side_keys_np(im, w, how, by):
    if im == 0:
        return _keys_np(w["left"], w["label"], how, by), _keys_np(w["right"], w["label"], how, by)
    return _keys_np(w["label"], w["left"], how, by), _keys_np(w["label"], w["right"], how, by)


def output_maps_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, how, by, walk=None):
    """-> (output_map(all_pieces(...), how, by), the same with drop_degenerate) with numpy: a piece is kept when its two
    side keys differ"""
    walk = walk or walk_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair)
    parts = []
    for im, w in enumerate(walk):
        kl, kr = _side_keys_np(im, w, how, by)
        keep = kl != kr
        X, Y, start, piece = w["X"], w["Y"], w["start"], w["piece"]
        if "dup" not in w:  # consecutive equal points of one piece: once
            w["dup"] = np.r_[False, (X[1:] == X[:-1]) & (Y[1:] == Y[:-1]) & ~start[1:]]
        out = keep[piece] & ~w["dup"]
        parts.append(dict(xy=np.stack([X[out], Y[out]], axis=1), lens=np.bincount(piece[out], minlength=len(keep))[keep], kl=kl[keep],
                          kr=kr[keep], origin=((im << 31) | w["chain"][keep]).astype(np.uint32)))
    xy, lens, kl, kr, origin = (np.concatenate([p[name] for p in parts]) for name in ("xy", "lens", "kl", "kr", "origin"))
    keys = np.unique(np.concatenate([kl, kr]))
    keys = keys[keys >= 0]
    ids = lambda kk: np.where(kk >= 0, np.searchsorted(keys, kk) + 1, 0).astype(np.int32)  # noqa: E731
    left, right = ids(kl), ids(kr)
    face_pairs = np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    one = int((lens < 2).sum())
    full = dict(xy=xy.reshape(-1, 2), row_index=np.r_[0, np.cumsum(lens)].astype(np.uint32), left=left, right=right,
                face_pairs=face_pairs, origin=origin, n_one_point=one)
    stay = lens >= 2  # the numbering is taken over ALL kept pieces, also those drop_degenerate leaves out
    dropped = dict(xy=xy[np.repeat(stay, lens)].reshape(-1, 2), row_index=np.r_[0, np.cumsum(lens[stay])].astype(np.uint32),
                   left=left[stay], right=right[stay], face_pairs=face_pairs, origin=origin[stay], n_one_point=one)
    return full, dropped


def output_map_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, how, by, drop_degenerate=False, walk=None):
    return output_maps_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, how, by, walk=walk)[1 if drop_degenerate else 0]


def piece_cross_sums_np(w):
    """per piece of one map's walk, sum of x[i] y[i+1] - x[i+1] y[i] over its points as Python ints (object array), exact:
    a coordinate is split into a signed high part and a 24-bit low part, so that with |coordinate| <= 2^46 every partial
    product is below 2^48 and the int64 sums of the three weights over a piece of fewer than 2^14 points cannot wrap"""
    X, Y, start = w["X"], w["Y"], w["start"]
    first = np.flatnonzero(start)
    assert np.diff(np.r_[first, len(X)]).max() < 1 << 14 and max(np.abs(X).max(), np.abs(Y).max()) <= 1 << 46
    inner = np.r_[~start[1:], False]  # point i and point i + 1 belong to one piece
    xh, xl, yh, yl = X >> 24, X & 0xFFFFFF, Y >> 24, Y & 0xFFFFFF
    nx = lambda a: np.r_[a[1:], 0]  # noqa: E731
    hh = np.where(inner, xh * nx(yh) - nx(xh) * yh, 0)
    mid = np.where(inner, xh * nx(yl) + xl * nx(yh) - nx(xh) * yl - nx(xl) * yh, 0)
    ll = np.where(inner, xl * nx(yl) - nx(xl) * yl, 0)
    hh, mid, ll = (np.add.reduceat(v, first).astype(object) for v in (hh, mid, ll))
    return hh * (1 << 48) + mid * (1 << 24) + ll


def face_rows_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, how, by, walk=None, sums=None, arrays=False):
    """face_rows(all_pieces(...), how, by) with numpy, exact (consecutive equal points add nothing to a cross sum, so
    they need not be removed).  walk / sums: walk_np() and its piece_cross_sums_np(), when the caller has them.
    arrays: -> (face0, face1 int32, area2 as uint64 low and int64 high limbs: two's complement, what the device stores)"""
    walk = walk or walk_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair)
    sums = sums or [piece_cross_sums_np(w) for w in walk]
    keys, vals = [], []
    for im, w in enumerate(walk):
        kl, kr = _side_keys_np(im, w, how, by)
        keep = kl != kr
        for kk, sign in ((kl, 1), (kr, -1)):
            has = keep & (kk >= 0)
            keys.append(kk[has])
            vals.append(sums[im][has] * sign)
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    if not len(keys):
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.int64)) if arrays else []
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    first = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    total = np.add.reduceat(vals, first)
    if arrays:
        return ((keys[first] >> 32).astype(np.int32), (keys[first] & 0xFFFFFFFF).astype(np.int32),
                (total & ((1 << 64) - 1)).astype(np.uint64), (total >> 64).astype(np.int64))
    return [(int(k) >> 32, int(k) & 0xFFFFFFFF, int(v)) for k, v in zip(keys[first].tolist(), total.tolist())]
