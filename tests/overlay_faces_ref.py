"""Test-side restatement of the overlay's face table (test infrastructure): the output map's pieces walked chain by chain
exactly as overlay_ref.write_output_chain walks them (src/app/output_chain.h:84-143), every kept piece's points summed
with Python ints -- independent of the per-edge rule the product uses (rayjoin_amd/csrc/rj_overlay.h), so the two
formulations check each other.

Table: {(face of map 0, face of map 1): twice the signed area in scaled units^2}, for every ordered pair of nonzero
faces that receives a contribution; rows() sorts it by ((uint32)f0 << 32) | (uint32)f1."""
import numpy as np


def face_table(scaled_maps, xsects_sorted_pair, point_in_polygon_pair):
    """scaled_maps[im]: maps.ScaledMap (int64 points, row_index, left, right); xsects_sorted_pair[im]: records ordered
    by (eid[im], distance) with mid_point_polygon_id; point_in_polygon_pair[im]: face, in the other map, of every
    vertex of map im.  -> dict {(f0, f1): area2}"""
    table = {}
    for im in range(2):
        m = scaled_maps[im]
        pts = [(int(x), int(y)) for x, y in m.pts.tolist()]
        pip = [int(v) for v in np.asarray(point_in_polygon_pair[im]).tolist()]
        grouped = {}
        for x in xsects_sorted_pair[im]:
            grouped.setdefault(int(x["eid"][im]), []).append(x)

        def cut(x):
            return (int(x["x_num"]), int(x["y_num"]))

        for ic in range(m.n_chains):
            b, e = int(m.row_index[ic]), int(m.row_index[ic + 1])
            left, right = int(m.left[ic]), int(m.right[ic])
            piece = {"points": [], "other": 0}

            def flush():
                p = piece["points"]
                o = piece["other"]
                if p and o != 0 and (left != 0 or right != 0):
                    a2 = sum(p[i][0] * p[i + 1][1] - p[i + 1][0] * p[i][1] for i in range(len(p) - 1))
                    for mine, sign in ((left, 1), (right, -1)):
                        if mine != 0:
                            key = (mine, o) if im == 0 else (o, mine)
                            table[key] = table.get(key, 0) + sign * a2
                piece["points"] = []

            for pid in range(b, e):
                piece["other"] = pip[pid]
                piece["points"].append(pts[pid])
                if pid != e - 1:
                    lst = grouped.get(pid - ic)
                    if lst:
                        piece["points"].append(cut(lst[0]))
                        for k in range(len(lst) - 1):
                            flush()
                            piece["other"] = int(lst[k]["mid_point_polygon_id"])
                            piece["points"].append(cut(lst[k]))
                            piece["points"].append(cut(lst[k + 1]))
                        flush()
                        piece["points"].append(cut(lst[-1]))
            flush()
    return table


def rows(table):
    """[(f0, f1, area2)] ascending by ((uint32)f0 << 32) | (uint32)f1"""
    return sorted(((f0, f1, a) for (f0, f1), a in table.items()),
                  key=lambda r: ((r[0] & 0xFFFFFFFF) << 32) | (r[1] & 0xFFFFFFFF))


def oracle_records(oracle, ctx, gsize=2048):
    """the oracle pipeline's per-map records and vertex faces (-mode=grid semantics, as overlay_ref.oracle_overlay)"""
    m = [oracle.Map(ctx.maps[i].pts, ctx.maps[i].row_index, ctx.maps[i].left, ctx.maps[i].right) for i in range(2)]
    pairs = oracle.lsi_grid(m[0], m[1], gsize)["eid"]
    pip = []
    for im in range(2):
        eids = oracle.pip_grid(m[1 - im], 1 - im, ctx.maps[im].pts, gsize)
        pip.append(m[1 - im].face_ids(eids))
    xs = [oracle.overlay_edge_xsects(m[0], m[1], im, pairs, gsize) for im in range(2)]
    return xs, pip


def oracle_face_rows(oracle, ctx, gsize=2048):
    xs, pip = oracle_records(oracle, ctx, gsize)
    return rows(face_table(ctx.maps, xs, pip)), xs, pip


def text(rows_, scaling):
    """polyover_exec -face_table's file: "f0 f1 area" per row, area = area2 / 2 * rrx * rry, %.17g"""
    k = 0.5 * float(scaling.rrx) * float(scaling.rry)
    return "".join("%d %d %.17g\n" % (f0, f1, float(a) * k) for f0, f1, a in rows_)


def shoelace2(scaled_map, face):
    """twice the area of one face of a map from its chains (left side +, right side -), Python ints"""
    m = scaled_map
    total = 0
    for ic in range(m.n_chains):
        sgn = (1 if int(m.left[ic]) == face else 0) - (1 if int(m.right[ic]) == face else 0)
        if sgn == 0:
            continue
        b, e = int(m.row_index[ic]), int(m.row_index[ic + 1])
        p = m.pts[b:e].tolist()
        total += sgn * sum(p[i][0] * p[i + 1][1] - p[i + 1][0] * p[i][1] for i in range(len(p) - 1))
    return total
