"""Test-side restatement of the overlay's output map in scaled integers (test infrastructure): the chains walked exactly
as overlay_ref.write_output_chain walks them (src/app/output_chain.h:84-143), points as Python int pairs, consecutive
equal points once -- independent of the per-edge rule the product uses (rayjoin_amd/csrc/rj_overlay_map.h), so the two
formulations check each other.

Face numbering (rj_overlay_map, include/rayjoin_amd.h): the ordered pairs (face of map 0, face of map 1) that a kept
piece has on a side, ascending by ((uint32)f0 << 32) | (uint32)f1, from 1; a side without a face is 0.  The numbering
is taken over ALL kept pieces, also those drop_degenerate leaves out."""
import numpy as np

from rayjoin_amd import maps


def pieces(scaled_maps, xsects_sorted_pair, point_in_polygon_pair):
    """-> [(im, source chain, left face, right face, other face, [points])] of every kept piece, in the writer's order"""
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
            cur = []
            other = [0]

            def flush():
                if cur and other[0] != 0 and (left != 0 or right != 0):
                    uniq = [cur[0]]
                    for p in cur[1:]:
                        if p != uniq[-1]:
                            uniq.append(p)
                    out.append((im, ic, left, right, other[0], uniq))
                del cur[:]

            for pid in range(b, e):
                other[0] = pip[pid]
                cur.append(pts[pid])
                if pid != e - 1:
                    lst = grouped.get(pid - ic)
                    if lst:
                        cur.append(lst[0][:2])
                        for k in range(len(lst) - 1):
                            flush()
                            other[0] = lst[k][2]
                            cur.append(lst[k][:2])
                            cur.append(lst[k + 1][:2])
                        flush()
                        cur.append(lst[-1][:2])
            flush()
    return out


def _key(pair):
    return ((pair[0] & 0xFFFFFFFF) << 32) | (pair[1] & 0xFFFFFFFF)


def ordered_pair(im, mine, other):
    return (mine, other) if im == 0 else (other, mine)


def output_map(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, drop_degenerate=False):
    """-> dict: xy (int64 [np, 2]), row_index (uint32 [nc + 1]), left, right (int32 [nc]: output face ids),
    face_pairs (int32 [nf, 2]), origin (uint32 [nc]: (im << 31) | source chain), pairs ([(left pair or None, right pair
    or None)] per chain), n_one_point (pieces with fewer than two points, before dropping)"""
    ps = pieces(scaled_maps, xsects_sorted_pair, point_in_polygon_pair)
    pair_set = set()
    for im, _, l, r, o, _ in ps:
        for mine in (l, r):
            if mine != 0:
                pair_set.add(ordered_pair(im, mine, o))
    face_pairs = sorted(pair_set, key=_key)
    ids = {p: i + 1 for i, p in enumerate(face_pairs)}
    xy, row, left, right, origin, pairs = [], [0], [], [], [], []
    one = 0
    for im, ic, l, r, o, pts in ps:
        if len(pts) < 2:
            one += 1
            if drop_degenerate:
                continue
        lp = ordered_pair(im, l, o) if l != 0 else None
        rp = ordered_pair(im, r, o) if r != 0 else None
        xy.extend(pts)
        row.append(len(xy))
        left.append(ids[lp] if lp else 0)
        right.append(ids[rp] if rp else 0)
        origin.append((im << 31) | ic)
        pairs.append((lp, rp))
    return dict(xy=np.array(xy, dtype=np.int64).reshape(-1, 2), row_index=np.array(row, dtype=np.uint32),
                left=np.array(left, dtype=np.int32), right=np.array(right, dtype=np.int32),
                face_pairs=np.array(face_pairs, dtype=np.int32).reshape(-1, 2), origin=np.array(origin, dtype=np.uint32),
                pairs=pairs, n_one_point=one)


def as_scaled_map(om, map_id=0):
    """the output map as an input map (needs drop_degenerate: an input chain has at least two points)"""
    return maps.ScaledMap(map_id, om["xy"], om["row_index"], om["left"].astype(np.int64), om["right"].astype(np.int64))


def output_map_np(scaled_maps, xsects_sorted_pair, point_in_polygon_pair, drop_degenerate=False):
    """output_map() for maps too large for a Python loop (the full-size check): the same walk written with numpy over
    the whole emitted sequence -- per chain its vertices, each followed by the cuts of the edge it starts, every cut
    twice (the end of one piece, the start of the next).  tests/test_overlay_map.py holds it equal to output_map()."""
    parts = []
    for im in range(2):
        m = scaled_maps[im]
        xs = xsects_sorted_pair[im]
        n, npts, nc = len(xs), m.n_points, m.n_chains
        row = m.row_index.astype(np.int64)
        vf = np.asarray(point_in_polygon_pair[im]).astype(np.int64)
        chain_of_point = np.repeat(np.arange(nc, dtype=np.int64), np.diff(row))
        eid = xs["eid"][:, im].astype(np.int64) if n else np.zeros(0, np.int64)
        # a record's chain: edge e of chain c starts at point e + c, and e + c < row[c + 1] - 1
        rec_chain = np.searchsorted(row[1:] - 1 - np.arange(nc), eid, side="right") if n else np.zeros(0, np.int64)
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
        piece = np.cumsum(start) - 1  # piece of every emitted point: records of the chain before it + chains before it
        n_pieces = n + nc
        # labels by the piece's END: at record k (piece k + chain), or with the chain
        label = np.zeros(n_pieces, np.int64)
        same_edge = np.zeros(n, bool)
        if n:
            same_edge[1:] = eid[1:] == eid[:-1]
            mid_prev = np.r_[0, xs["mid_point_polygon_id"][:-1].astype(np.int64)]
            label[k + rec_chain] = np.where(same_edge, mid_prev, vf[rec_p1])
        recs_to_chain_end = np.searchsorted(eid, row[1:] - 1 - np.arange(nc), side="left")
        label[recs_to_chain_end + np.arange(nc)] = vf[row[1:] - 1]
        piece_chain = np.zeros(n_pieces, np.int64)
        piece_chain[piece[pos_v]] = chain_of_point
        piece_chain[k + rec_chain + 1] = rec_chain  # (a piece between two cuts of one edge holds no vertex)
        left, right = m.left.astype(np.int64)[piece_chain], m.right.astype(np.int64)[piece_chain]
        keep = (label != 0) & ((left != 0) | (right != 0))
        dup = np.zeros(total, bool)
        dup[1:] = (X[1:] == X[:-1]) & (Y[1:] == Y[:-1]) & ~start[1:]
        out = keep[piece] & ~dup
        lens = np.bincount(piece[out], minlength=n_pieces)[keep]
        f0l, f1l = (left, label) if im == 0 else (label, left)
        f0r, f1r = (right, label) if im == 0 else (label, right)
        key = lambda a, b, mine: np.where(mine != 0, ((a & 0xFFFFFFFF) << 32) | (b & 0xFFFFFFFF), -1)  # noqa: E731
        parts.append(dict(xy=np.stack([X[out], Y[out]], axis=1), lens=lens, kl=key(f0l, f1l, left)[keep], kr=key(f0r, f1r, right)[keep],
                          origin=((im << 31) | piece_chain[keep]).astype(np.uint32)))
    xy = np.concatenate([p["xy"] for p in parts])
    lens = np.concatenate([p["lens"] for p in parts])
    kl, kr = np.concatenate([p["kl"] for p in parts]), np.concatenate([p["kr"] for p in parts])
    origin = np.concatenate([p["origin"] for p in parts])
    keys = np.unique(np.concatenate([kl, kr]))
    keys = keys[keys >= 0]
    ids = lambda kk: np.where(kk >= 0, np.searchsorted(keys, kk) + 1, 0).astype(np.int32)  # noqa: E731
    left, right = ids(kl), ids(kr)
    one = int((lens < 2).sum())
    if drop_degenerate:
        stay = lens >= 2
        xy = xy[np.repeat(stay, lens)]
        lens, left, right, origin = lens[stay], left[stay], right[stay], origin[stay]
    return dict(xy=xy.reshape(-1, 2), row_index=np.r_[0, np.cumsum(lens)].astype(np.uint32), left=left, right=right,
                face_pairs=np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2), origin=origin, n_one_point=one)
