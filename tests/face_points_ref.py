"""The definition of rj_face_points (rayjoin_amd/csrc/rj_face_points.h) in plain Python, with Python ints for the sums: per
face the count, the sum, min, max and the first of the points whose label is the face, and under MEMBERS their numbers.
No wave, no limb, no atomics: what the host twin and the device are held against."""
import collections

COUNTS = ("n_faces", "n_members", "n_outside", "n_unmatched", "n_runs")
MEMBERS = 1
NO_POINT = 0xFFFFFFFF
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
MAX_POINTS = 1 << 32

Result = collections.namedtuple("Result", "faces offsets members counts")


class Invalid(Exception):
    """what the call refuses with RJ_E_INVALID"""


def unsigned(label):
    return int(label) & 0xFFFFFFFF


def check_universe(universe):
    u = [int(v) for v in universe]
    if any(v == 0 for v in u) or any(unsigned(a) >= unsigned(b) for a, b in zip(u, u[1:])):
        raise Invalid("the universe must ascend strictly by unsigned label and must not contain 0")
    return u


def face_points_ref(labels, values=None, stride=1, universe=None, flags=0):
    """labels: n ints.  values: a flat sequence, the value of point i at values[i * stride], or None.  universe: the labels
    of the faces, or None for the distinct nonzero labels among the points.  -> Result(faces = dicts of label, first,
    n_points, sum, min, max; offsets and members as lists under MEMBERS, else None; counts)"""
    labels = [int(v) for v in labels]
    n = len(labels)
    if flags & ~MEMBERS:
        raise Invalid("unknown flags")
    if n >= MAX_POINTS:
        raise Invalid("n < 2^32")
    if values is not None and stride < 1:
        raise Invalid("value_stride >= 1")
    names = check_universe(universe) if universe is not None else sorted({v for v in labels if v != 0}, key=unsigned)
    number = {v: k for k, v in enumerate(names)}
    points = [[] for _ in names]
    outside = unmatched = 0
    for i, v in enumerate(labels):
        if v == 0:
            outside += 1
        elif v in number:
            points[number[v]].append(i)
        else:
            unmatched += 1
    faces = []
    for v, mine in zip(names, points):
        vals = [int(values[i * stride]) for i in mine] if values is not None else []
        faces.append(dict(label=v, first=mine[0] if mine else NO_POINT, n_points=len(mine), sum=sum(vals), min=min(vals) if vals else INT64_MAX,
                          max=max(vals) if vals else INT64_MIN))
    n_members = sum(len(p) for p in points)
    counts = dict(n_faces=len(names), n_members=n_members, n_outside=outside, n_unmatched=unmatched,
                  n_runs=sum(1 for i in range(n) if i == 0 or labels[i] != labels[i - 1]))
    assert n_members + outside + unmatched == n
    offsets = members = None
    if flags & MEMBERS:
        offsets, members = [0], []
        for mine in points:
            members += mine
            offsets.append(len(members))
    return Result(faces, offsets, members, counts)
