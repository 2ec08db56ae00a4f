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
