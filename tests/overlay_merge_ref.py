"""Test-side restatement of RJ_OVM_MERGE_PIECES (test infrastructure): merge(M) from the arrays of an output map M alone,
straight from the definition in include/rayjoin_amd.h.  Chain k > 0 of M joins chain k - 1 when both have the same
origin, the same left and the same right face and the last point of chain k - 1 equals the first point of chain k; the
chains of merge(M) are the maximal runs of joined chains, a run's points are its chains' points in order without the
first point of every joining chain.  merge_ref is the plain-Python form, merge_np the numpy form for maps too large for
a Python loop (tests/test_overlay_merge.py holds the two equal)."""
import numpy as np


def joins(xy, row_index, left, right, origin, k):
    """does chain k join chain k - 1?"""
    if k == 0:
        return False
    a, b = int(row_index[k]) - 1, int(row_index[k])  # last point of chain k - 1, first point of chain k
    return (int(origin[k]) == int(origin[k - 1]) and int(left[k]) == int(left[k - 1]) and int(right[k]) == int(right[k - 1])
            and int(xy[a][0]) == int(xy[b][0]) and int(xy[a][1]) == int(xy[b][1]))


def merge_ref(xy, row_index, left, right, origin):
    """-> dict(xy, row_index, left, right, origin) of merge(M), dtypes as M's"""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    pts = xy.tolist()
    out_xy, out_row, out_left, out_right, out_origin = [], [0], [], [], []
    for k in range(len(left)):
        b, e = int(row_index[k]), int(row_index[k + 1])
        if joins(pts, row_index, left, right, origin, k):
            out_xy.extend(pts[b + 1:e])
            out_row[-1] = len(out_xy)
        else:
            out_xy.extend(pts[b:e])
            out_row.append(len(out_xy))
            out_left.append(int(left[k]))
            out_right.append(int(right[k]))
            out_origin.append(int(origin[k]))
    return dict(xy=np.array(out_xy, dtype=np.int64).reshape(-1, 2), row_index=np.array(out_row, dtype=np.uint32),
                left=np.array(out_left, dtype=np.int32), right=np.array(out_right, dtype=np.int32),
                origin=np.array(out_origin, dtype=np.uint32))


def merge_np(xy, row_index, left, right, origin):
    """merge_ref with numpy"""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    row = np.asarray(row_index).astype(np.int64)
    left, right, origin = np.asarray(left), np.asarray(right), np.asarray(origin)
    nc = len(left)
    if nc == 0:
        return dict(xy=xy[:0], row_index=np.zeros(1, np.uint32), left=left.astype(np.int32), right=right.astype(np.int32),
                    origin=origin.astype(np.uint32))
    assert (np.diff(row) >= 1).all()  # (a chain has a first and a last point)
    join = np.zeros(nc, bool)
    first, last = row[1:-1], row[1:-1] - 1  # of chains 1 .. nc - 1 and 0 .. nc - 2
    join[1:] = ((origin[1:] == origin[:-1]) & (left[1:] == left[:-1]) & (right[1:] == right[:-1])
                & (xy[first, 0] == xy[last, 0]) & (xy[first, 1] == xy[last, 1]))
    keep = np.ones(len(xy), bool)
    keep[row[:-1][join]] = False
    start = ~join  # (chain 0 starts a run)
    lens = np.add.reduceat(np.diff(row) - join, np.flatnonzero(start))
    return dict(xy=xy[keep], row_index=np.r_[0, np.cumsum(lens)].astype(np.uint32), left=left[start].astype(np.int32),
                right=right[start].astype(np.int32), origin=origin[start].astype(np.uint32))


MERGED = ("xy", "row_index", "left", "right", "origin")


def merged_map(om, np_form=False):
    """merge of an output-map dict (as overlay_ops_ref.output_map returns it): the five arrays merged, face_pairs as they are"""
    out = (merge_np if np_form else merge_ref)(*(om[name] for name in MERGED))
    out["face_pairs"] = om["face_pairs"]
    return out


def n_joins(om):
    return sum(1 for k in range(len(om["left"])) if joins(om["xy"].tolist(), om["row_index"], om["left"], om["right"], om["origin"], k))


def longest_run(om):
    """chains in the longest run of joined chains"""
    best = cur = 0
    pts = om["xy"].tolist()
    for k in range(len(om["left"])):
        cur = cur + 1 if joins(pts, om["row_index"], om["left"], om["right"], om["origin"], k) else 1
        best = max(best, cur)
    return best
