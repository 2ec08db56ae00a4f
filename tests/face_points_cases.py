"""Inputs for the tests of rj_face_points: hand cases with the answers written out, and the generated point sets on which
the wave logic of the table pass can break -- one label throughout, every label different, labels that alternate, runs of
1 .. 130 points laid so that they start and end on every lane and straddle wave and block boundaries, one run over many
blocks, and Zipf-like draws in sorted, block-shuffled and fully shuffled order.  A case is a Case(labels int32, values flat
int64 or None, stride, universe int32 or None); nothing here is ever changed by a test."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "labels values stride universe")
INT64_MAX, INT64_MIN, INT32_MIN = 2 ** 63 - 1, -2 ** 63, -2 ** 31
NO_POINT = 0xFFFFFFFF
SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
LAYOUTS = ("one", "distinct", "alternate", "runs")
ORDERS = ("sorted", "blocks", "shuffled")
SWEEP_SEEDS = tuple(range(20))


def case(labels, values=None, stride=1, universe=None):
    return Case(np.asarray(labels, np.int32), None if values is None else np.asarray(values, np.int64).reshape(-1), int(stride),
                None if universe is None else np.asarray(universe, np.int32).reshape(-1))


def face(label, first, n_points, total, lo, hi):
    return dict(label=label, first=first, n_points=n_points, sum=total, min=lo, max=hi)


def empty(label):
    return face(label, NO_POINT, 0, 0, INT64_MAX, INT64_MIN)


def counts(n_faces, n_members, n_outside, n_unmatched, n_runs):
    return dict(n_faces=n_faces, n_members=n_members, n_outside=n_outside, n_unmatched=n_unmatched, n_runs=n_runs)


# name -> dict(case, faces, offsets, members, counts): the answers by hand
HAND = {
    # two faces and the outside; face 3 comes back behind another label
    "two-faces": dict(case=case([3, 3, 0, 7, 3], [10, 20, 30, 40, 50]),
                      faces=[face(3, 0, 3, 80, 10, 50), face(7, 3, 1, 40, 40, 40)], offsets=[0, 3, 4], members=[0, 1, 4, 3], counts=counts(2, 4, 1, 0, 4)),
    # the faces ascend as unsigned numbers: 1, then INT32_MIN = 0x80000000, -5 = 0xFFFFFFFB, -1 = 0xFFFFFFFF
    "unsigned-order": dict(case=case([-1, 1, INT32_MIN, -5, 1, -1], [1, 2, 3, 4, 5, 6]),
                           faces=[face(1, 1, 2, 7, 2, 5), face(INT32_MIN, 2, 1, 3, 3, 3), face(-5, 3, 1, 4, 4, 4), face(-1, 0, 2, 7, 1, 6)],
                           offsets=[0, 2, 3, 4, 6], members=[1, 4, 2, 3, 0, 5], counts=counts(4, 6, 0, 0, 6)),
    # the sum leaves 64 bits on both sides: 5 INT64_MAX + 3 INT64_MIN = 2^64 - 5 in face 9, 3 INT64_MIN in face 4, 5 INT64_MAX in face 5
    "wide-sum": dict(case=case([9] * 5 + [4] * 3 + [9] * 3 + [5] * 5, [INT64_MAX] * 5 + [INT64_MIN] * 3 + [INT64_MIN] * 3 + [INT64_MAX] * 5),
                     faces=[face(4, 5, 3, -3 * 2 ** 63, INT64_MIN, INT64_MIN), face(5, 11, 5, 5 * INT64_MAX, INT64_MAX, INT64_MAX),
                            face(9, 0, 8, 2 ** 64 - 5, INT64_MIN, INT64_MAX)],
                     offsets=[0, 3, 8, 16], members=[5, 6, 7, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 8, 9, 10], counts=counts(3, 16, 0, 0, 4)),
    # mixed signs that cancel, in one run and across runs
    "cancel": dict(case=case([2, 2, 2, 2, 6, 2, 6], [7, -7, 2 ** 40, -2 ** 40, -1, 0, 1]),
                   faces=[face(2, 0, 5, 0, -2 ** 40, 2 ** 40), face(6, 4, 2, 0, -1, 1)], offsets=[0, 5, 7], members=[0, 1, 2, 3, 5, 4, 6],
                   counts=counts(2, 7, 0, 0, 4)),
    # a universe with a face that gets no point (8), and a label that is not in it (9)
    "universe": dict(case=case([5, 5, 9, 0, 2], [1, 2, 3, 4, 5], universe=[2, 5, 8]),
                     faces=[face(2, 4, 1, 5, 5, 5), face(5, 0, 2, 3, 1, 2), empty(8)], offsets=[0, 1, 3, 3], members=[4, 0, 1], counts=counts(3, 3, 1, 1, 4)),
    # the x and the y of three points: the same array with stride 2, and from its second element on
    "stride-x": dict(case=case([1, 1, 4], [10, -1, 20, -2, 30, -3], stride=2),
                     faces=[face(1, 0, 2, 30, 10, 20), face(4, 2, 1, 30, 30, 30)], offsets=[0, 2, 3], members=[0, 1, 2], counts=counts(2, 3, 0, 0, 2)),
    "stride-3": dict(case=case([4, 1, 4], [5, 0, 0, 6, 0, 0, -8], stride=3),
                     faces=[face(1, 1, 1, 6, 6, 6), face(4, 0, 2, -3, -8, 5)], offsets=[0, 1, 3], members=[1, 0, 2], counts=counts(2, 3, 0, 0, 3)),
    # no values: every sum 0, min and max empty
    "no-values": dict(case=case([7, 7, 0, 7]), faces=[face(7, 0, 3, 0, INT64_MAX, INT64_MIN)], offsets=[0, 3], members=[0, 1, 3], counts=counts(1, 3, 1, 0, 3)),
    # points whose only label is 0: no face without a universe
    "all-outside": dict(case=case([0, 0, 0], [1, 2, 3]), faces=[], offsets=[0], members=[], counts=counts(0, 0, 3, 0, 1)),
    # an empty universe: every nonzero label is unmatched
    "empty-universe": dict(case=case([3, 0, 3, -1], [1, 2, 3, 4], universe=[]), faces=[], offsets=[0], members=[], counts=counts(0, 0, 1, 3, 4)),
    # no points: no face without a universe, every record empty with one
    "no-points": dict(case=case([], []), faces=[], offsets=[0], members=[], counts=counts(0, 0, 0, 0, 0)),
    "no-points-universe": dict(case=case([], [], universe=[1, -1]), faces=[empty(1), empty(-1)], offsets=[0, 0, 0], members=[], counts=counts(2, 0, 0, 0, 0)),
}
BAD_UNIVERSES = {"descending": [5, 2], "zero": [0, 3], "zero-last": [3, 0], "duplicate": [2, 5, 5, 9], "signed-order": [-1, 1]}


def values_for(rng, n, stride):
    """n values spread over [n * stride]: small ones, the whole range and the extremes, so that sums leave 64 bits"""
    v = rng.integers(-1000, 1000, n * stride)
    wide = rng.integers(INT64_MIN, INT64_MAX, n * stride, endpoint=True)
    pick = rng.integers(0, 8, n * stride)
    v = np.where(pick >= 5, wide, v)
    v = np.where(pick == 3, INT64_MAX, v)
    v = np.where(pick == 4, INT64_MIN, v)
    return v.astype(np.int64)


def run_lengths():
    """1 .. 130 three times over with a shift in between: the runs start and end on every lane of a wave"""
    return list(range(1, 131)) + [37] + list(range(130, 0, -1)) + [11] + list(range(1, 131))


def layout(kind, n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "one":
        labels = np.full(n, 12, np.int32)
    elif kind == "distinct":
        labels = (rng.permutation(n) + 1).astype(np.int32)
        labels[::3] *= -1  # (negative labels among them)
    elif kind == "alternate":
        labels = np.where(np.arange(n) % 2 == 0, 5, -3).astype(np.int32)
    elif kind == "runs":
        lengths = run_lengths()
        names = [0, 1, 2, -1, INT32_MIN, 40, -40, 7, 9, 1000, 77]
        labels = np.concatenate([np.full(m, names[(3 * r) % len(names)], np.int32) for r, m in enumerate(lengths)])
        n = len(labels)
    else:
        raise KeyError(kind)
    return case(labels, values_for(rng, n, 2), 2)


def big(kind):
    """70 000 points of one face, or of none: many waves and blocks on one face or on the outside counter"""
    rng = np.random.default_rng(7)
    n = 70000
    return case(np.full(n, 0 if kind == "outside" else -8, np.int32), values_for(rng, n, 1))


def sweep(seed, order):
    """n <= 3 000 points over up to 200 faces plus 0, drawn Zipf-like: a few faces and the outside take most points"""
    rng = np.random.default_rng(seed)
    n, nf = int(rng.integers(1, 3001)), int(rng.integers(1, 201))
    names = np.concatenate([[0], rng.choice(np.arange(-5000, 5000)[np.arange(-5000, 5000) != 0], nf, replace=False)]).astype(np.int32)
    weight = 1.0 / np.arange(1, nf + 2) ** 1.2
    labels = names[rng.choice(nf + 1, n, p=weight / weight.sum())]
    if order == "sorted":
        labels = np.sort(labels)
    elif order == "blocks":
        labels = np.sort(labels)
        cuts = np.sort(rng.choice(np.arange(1, n), min(n - 1, 40), replace=False)) if n > 1 else []
        pieces = np.split(labels, cuts)
        labels = np.concatenate([pieces[j] for j in rng.permutation(len(pieces))])
    stride = 1 + seed % 3
    return case(labels, values_for(rng, n, stride), stride)


def universe_for(c, seed=0):
    """a universe for a case that has none: its faces but one that occurs (so n_unmatched is not 0 where there are two or
    more), and three that get no point"""
    rng = np.random.default_rng(seed)
    mine = sorted({int(v) for v in c.labels if v != 0}, key=lambda v: v & 0xFFFFFFFF)
    if len(mine) >= 2:
        del mine[int(rng.integers(0, len(mine)))]
    extra = {123456, -123456, 2 ** 31 - 1} - set(mine) - {int(v) for v in c.labels}
    return np.array(sorted(set(mine) | extra, key=lambda v: v & 0xFFFFFFFF), np.int32)
