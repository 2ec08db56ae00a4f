"""The face adjacency table of a chain map (rj_map_neighbours), by definition: plain Python integers, dicts, sets and
math.isqrt, nothing shared with rayjoin_amd/csrc/rj_neighbours.h.  Where the header sorts chain sides, incidences and
directed keys and sums by key, this keeps a dict per face and a set per node.

neighbours_ref(xy, row_index, left, right, flags=0) -> Result or raises Invalid.

The definition.  A face is a label other than 0 that occurs in left or right; faces are numbered by ascending
(label mod 2^32).  Of chain c over its edges p_i -> p_i+1: S(c) = the sum of cross(p_i, p_i+1), L(c) = the sum of
isqrt(dx^2 + dy^2).  area2(f) = the sum of S(c) over left[c] == f minus the sum over right[c] == f; n_sides(f) = the chain
sides that carry f.  f != g, both not 0, are edge neighbours when some chain has {left, right} = {f, g}: w(f, g) = the sum
of L(c) over those chains, n_chains(f, g) their number (w = 0 still makes a pair).  perimeter(f) = the sum of L(c) over
the chains with left != right and one side f; outer(f) the part whose other side is 0.  Under VERTEX a node is a
distinct point that is the first or the last point of some chain; F(P) = the nonzero labels on either side of any chain
that ends at P; n_nodes(f, g) = the nodes P with f and g both in F(P); a pair with n_nodes > 0 and n_chains = 0 is a
vertex-only neighbour.  Without VERTEX no node is looked at.  The entries of a face ascend by the neighbour's unsigned
label; n_node_pairs_raw = the sum over nodes of m (m - 1), m = |F(P)|, and the call is refused from 2^32 on."""
import math

import numpy as np

COUNTS = ("n_faces", "n_entries", "n_edge_pairs", "n_vertex_pairs", "n_nodes", "n_node_pairs_raw", "max_labels_at_node")
VERTEX = 1
LIM = 1 << 46
RAW_LIMIT = 1 << 32


class Invalid(ValueError):
    pass


class Result:
    """faces: a list of dicts (label, n_sides, n_edge_nbrs, n_vertex_nbrs, area2, perimeter, outer), ascending by unsigned
    label; offsets: a list of n_faces + 1 ints; entries: a list of dicts (label, face, n_chains, n_nodes, w); counts"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def pairs(self):
        """{(f, g): (w, n_chains, n_nodes)} over the directed pairs, by label"""
        out = {}
        for k, f in enumerate(self.faces):
            for e in self.entries[self.offsets[k]:self.offsets[k + 1]]:
                out[(f["label"], e["label"])] = (e["w"], e["n_chains"], e["n_nodes"])
        return out


def unsigned(label):
    return label % (1 << 32)


def neighbours_ref(xy, row_index, left, right, flags=0):
    pts = [(int(x), int(y)) for x, y in np.asarray(xy, np.int64).reshape(-1, 2).tolist()]
    row = [int(v) for v in np.asarray(row_index).tolist()]
    left, right = [int(v) for v in np.asarray(left).tolist()], [int(v) for v in np.asarray(right).tolist()]
    nc = max(0, len(row) - 1)
    if flags & ~VERTEX:
        raise Invalid("flags")
    if nc == 0:
        if pts:
            raise Invalid("points without chains")
        return Result(faces=[], offsets=[0], entries=[], counts=dict.fromkeys(COUNTS, 0))
    if nc > len(pts) or row[0] != 0 or row[-1] != len(pts) or any(b >= e for b, e in zip(row, row[1:])):
        raise Invalid("row_index")
    if any(not -LIM <= v < LIM for p in pts for v in p):
        raise Invalid("coordinate")
    labels = sorted({f for f in left + right if f != 0}, key=unsigned)
    number = {f: k for k, f in enumerate(labels)}
    face = {f: dict(label=f, n_sides=0, n_edge_nbrs=0, n_vertex_nbrs=0, area2=0, perimeter=0, outer=0) for f in labels}
    pair = {f: {} for f in labels}  # pair[f][g] = [w, n_chains, n_nodes]
    for c in range(nc):
        s = length = 0
        for (ax, ay), (bx, by) in zip(pts[row[c]:row[c + 1] - 1], pts[row[c] + 1:row[c + 1]]):
            s += ax * by - ay * bx
            length += math.isqrt((bx - ax) ** 2 + (by - ay) ** 2)
        le, ri = left[c], right[c]
        for mine, other, sign in ((le, ri, 1), (ri, le, -1)):
            if mine == 0:
                continue
            face[mine]["n_sides"] += 1
            face[mine]["area2"] += sign * s
            if mine == other:
                continue
            face[mine]["perimeter"] += length
            if other == 0:
                face[mine]["outer"] += length
            else:
                p = pair[mine].setdefault(other, [0, 0, 0])
                p[0] += length
                p[1] += 1
    n_nodes = raw = most = 0
    if flags & VERTEX:
        at = {}
        for c in range(nc):
            for p in {pts[row[c]], pts[row[c + 1] - 1]}:
                at.setdefault(p, set()).update(f for f in (left[c], right[c]) if f != 0)
        n_nodes = len(at)
        for here in at.values():
            m = len(here)
            raw += m * (m - 1)
            most = max(most, m)
            for f in here:
                for g in here:
                    if f != g:
                        pair[f].setdefault(g, [0, 0, 0])[2] += 1
        if raw >= RAW_LIMIT:
            raise Invalid("n_node_pairs_raw")
    offsets, entries = [0], []
    for f in labels:
        for g in sorted(pair[f], key=unsigned):
            w, n_chains, nodes = pair[f][g]
            entries.append(dict(label=g, face=number[g], n_chains=n_chains, n_nodes=nodes, w=w))
            face[f]["n_edge_nbrs" if n_chains else "n_vertex_nbrs"] += 1
        offsets.append(len(entries))
    counts = dict(n_faces=len(labels), n_entries=len(entries), n_edge_pairs=sum(f["n_edge_nbrs"] for f in face.values()) // 2,
                  n_vertex_pairs=sum(f["n_vertex_nbrs"] for f in face.values()) // 2, n_nodes=n_nodes, n_node_pairs_raw=raw, max_labels_at_node=most)
    return Result(faces=[face[f] for f in labels], offsets=offsets, entries=entries, counts=counts)
