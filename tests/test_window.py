"""The edges of a map that meet each rectangle on the CPU: the plain-Python definition (tests/window_ref.py, a clip with
exact fractions) on the hand cases of tests/window_cases.py with the answers written out; the host twin of the device's
pipeline (tests/hosttwin/window_twin.cc compiling rayjoin_amd/csrc/rj_window.h) against that definition in both orders, with
and without the containment shortcut and the prune: the hand cases, 2 000 random (segment, window) pairs with coordinates up
to the domain's ends and differences down to 1, and random small maps; the clamp; the two box functions against the exact
predicate; the counting call, the overflow and the refusals; three mutations of a scratch copy of the header, each caught
by a named hand case; the twin as a stand-alone program under the host sanitizers.  The GPU side is
tests/test_gpu_window.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref as NR  # noqa: E402
import window_cases as WC  # noqa: E402
import window_ref as WR  # noqa: E402
from test_nearest import CXX, seg_array  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "window_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
HEADERS = ("rj_window.h", "rj_within.h", "rj_nearest.h", "rj_predicates.h")
VARIANTS = [(reverse, contained, prune) for reverse in (0, 1) for contained in (0, 1) for prune in (0, 1)]
OK, INVALID, OVERFLOW = 0, 1, 3
CANARY32, CANARY8, CANARY64 = 0x5B5B5B5B, 0x5B, 0x5B5B5B5B5B5B5B5B
LO, HI = -(1 << 46), (1 << 46) - 1
COUNTS = ("n_pairs", "n_windows_hit", "max_per_window")


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_window.h")] + [os.path.join(CSRC, h) for h in HEADERS[1:]]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libwindow_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(CXX + ["-fPIC", "-shared", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.window_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 5
    L.window_meets.argtypes = L.window_box.argtypes = [C.c_void_p, C.c_void_p]
    L.window_normalise.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def call_twin(L, seg, windows, reverse=0, contained=1, prune=1, capacity=None, flags=True, offsets=True):
    """the raw call with canaries behind every array -> (rc, counts, offsets, eid, flags, work); capacity None: the counting
    call first, then the exact capacity"""
    seg = np.ascontiguousarray(seg, dtype=np.int64).reshape(-1, 4)
    win = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 4)
    n = len(win)
    counts = np.zeros(3, np.uint64)
    if capacity is None:
        rc = L.window_twin(seg.ctypes.data, len(seg), win.ctypes.data, n, reverse, contained, prune, 0, None, None, None, counts.ctypes.data, None)
        assert rc == OK
        capacity = int(counts[0])
    off = np.full(n + 2, CANARY64, np.uint64)
    eid, flg = np.full(capacity + 1, CANARY32, np.uint32), np.full(capacity + 1, CANARY8, np.uint8)
    work = np.zeros(2, np.uint64)
    counts[:] = 77
    rc = L.window_twin(seg.ctypes.data, len(seg), win.ctypes.data, n, reverse, contained, prune, capacity, off.ctypes.data if offsets else None, eid.ctypes.data,
                       flg.ctypes.data if flags else None, counts.ctypes.data, work.ctypes.data)
    assert off[n + 1] == CANARY64 and eid[capacity] == CANARY32 and flg[capacity] == CANARY8
    return rc, [int(v) for v in counts], off[:n + 1], eid[:capacity], flg[:capacity], [int(v) for v in work]


def run_twin(L, seg, windows, reverse=0, contained=1, prune=1):
    """-> (per-window lists of (eid, flags), counts, work); offsets, eids and counts are checked for consistency"""
    rc, counts, off, eid, flg, work = call_twin(L, seg, windows, reverse, contained, prune)
    assert rc == OK
    n_pairs = counts[0]
    assert off[0] == 0 and off[-1] == n_pairs == len(eid) and (np.diff(off.astype(np.int64)) >= 0).all()
    flat = list(zip(eid.tolist(), flg.tolist()))
    lists = [flat[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    lens = [len(r) for r in lists]
    assert counts == [n_pairs, sum(v > 0 for v in lens), max(lens, default=0)]
    return lists, counts, work


def check_case(L, c, variants=VARIANTS):
    edges = NR.edges_of(c.pts, c.row)
    want = WR.window_all(c.windows, edges)
    for v in variants:
        got, _, _ = run_twin(L, seg_array(edges), c.windows, *v)
        assert got == want, v
    return want


# ---- the definition and the twin on the hand cases ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_definition_gives_the_written_answers(name):
    c = WC.HAND[name]
    assert WR.window_all(c.windows, NR.edges_of(c.pts, c.row)) == c.want


@pytest.mark.parametrize("name", sorted(WC.HAND))
def test_twin_gives_the_written_answers(twin, name):
    assert check_case(twin, WC.HAND[name]) == WC.HAND[name].want


def test_the_required_cases_are_there():
    assert {"touches_corner", "corner_one_unit_away", "diagonal_outside_corner", "through", "collinear_overlaps_side", "collinear_beyond_side",
            "point_window_on_vertex", "point_window_on_edge_and_off", "line_window", "same_quantum_apart", "empty_window", "outside_domain",
            "domain_ends"} <= set(WC.HAND)
    assert [len(w) for w in WC.HAND["point_window_on_vertex"].want] == [2]
    assert all(not w for w in WC.HAND["empty_window"].want[:3])


# ---- random pairs -------------------------------------------------------------------------------------------------------
def random_pair(rng):
    """a segment and a window near each other: at the domain's ends or anywhere, extents from 1 unit to the whole domain,
    so that touching, missing by one and crossing all happen"""
    span = 1 << rng.choice((0, 1, 2, 3, 8, 16, 17, 30, 46, 47))
    cx, cy = rng.choice(((LO, LO), (HI, HI), (LO, HI), (0, 0), (rng.randint(LO, HI), rng.randint(LO, HI))))
    near = lambda c: max(LO, min(HI, c + rng.randint(-span, span)))  # noqa: E731
    seg = (near(cx), near(cy), near(cx), near(cy))
    x0, x1 = sorted((near(cx), near(cx)))
    y0, y1 = sorted((near(cy), near(cy)))
    kind = rng.randrange(8)
    if kind == 0:  # a point window on the segment's first point or one unit off it
        x0 = x1 = seg[0] + rng.choice((0, 0, 1, -1))
        y0 = y1 = seg[1]
    elif kind == 1:  # a line window
        x1 = x0
    elif kind == 2:  # a corner on the segment's line, or one unit off: the midpoint where it is an integer point
        x1, y1 = (seg[0] + seg[2]) // 2, (seg[1] + seg[3]) // 2 + rng.choice((0, 1))
        x0, y0 = x1 - rng.randint(0, span), y1 - rng.randint(0, span)
    return seg, (x0, y0, x1, y1)


def test_random_pairs_against_the_definition(twin):
    rng = random.Random(7)
    hits = misses = through = 0
    for _ in range(2000):
        seg, win = random_pair(rng)
        want = WR.meets(seg, win)
        s, w = np.array(seg, np.int64), np.array(win, np.int64)
        got = twin.window_meets(s.ctypes.data, w.ctypes.data)
        assert (got >= 0) == want, (seg, win, got)
        if want:
            assert got == WR.flags_of(seg, win), (seg, win)
            hits += 1
            through += got == 0
        else:
            misses += 1
    assert hits > 400 and misses > 400 and through > 50, (hits, misses, through)


def random_map(rng, scale):
    half = 1 << scale
    step = max(1, half // 8)
    coord = (lambda: rng.randint(-7, 7) * step) if rng.random() < 0.5 else (lambda: rng.randint(-half, half - 1))
    chains = [[(coord(), coord()) for _ in range(rng.randint(2, 6))] for _ in range(rng.randint(1, 5))]
    windows = []
    for _ in range(10):
        x0, x1 = sorted((coord(), coord()))
        y0, y1 = sorted((coord(), coord()))
        windows.append((x0, y0, x1, y1))
    windows += [(p[0], p[1], p[0], p[1]) for ch in chains for p in ch][:4]
    windows += [(5, 5, 4, 6), (-(1 << 62), -(1 << 62), 1 << 62, 1 << 62)]
    return WC.case(chains, windows, [[]] * len(windows))


@pytest.mark.parametrize("scale", [4, 17, 30, 46])
def test_random_small_maps(twin, scale):
    rng = random.Random(300 + scale)
    pairs = 0
    for k in range(40):
        c = random_map(rng, scale)
        want = check_case(twin, c, VARIANTS if k % 5 == 0 else [(0, 1, 1), (1, 0, 1), (1, 1, 0)])
        assert len(want[-1]) == len(NR.edges_of(c.pts, c.row)) and not want[-2]
        pairs += sum(len(w) for w in want)
    assert pairs > 1000, pairs


# ---- the clamp ----------------------------------------------------------------------------------------------------------
def test_the_clamp_changes_no_result(twin):
    rng = random.Random(11)
    big = lambda: rng.choice((-(1 << 63), (1 << 63) - 1, LO, HI, LO - 1, HI + 1, rng.randint(-(1 << 63), (1 << 63) - 1), rng.randint(LO, HI)))  # noqa: E731
    live = dead = 0
    for _ in range(3000):
        win = (big(), big(), big(), big())
        w = np.array(win, np.int64)
        alive = twin.window_normalise(w.ctypes.data)
        meets_domain = win[0] <= win[2] and win[1] <= win[3] and win[2] >= LO and win[0] <= HI and win[3] >= LO and win[1] <= HI
        assert bool(alive) == meets_domain, win
        if alive:
            live += 1
            assert w.tolist() == [max(LO, min(HI, v)) for v in win] and w[0] <= w[2] and w[1] <= w[3]
            # no point of the domain is lost or gained: a segment anywhere in the domain meets both or neither
            for _ in range(3):
                seg = tuple(rng.choice((LO, HI, rng.randint(LO, HI))) for _ in range(4))
                assert WR.meets(seg, win) == WR.meets(seg, tuple(w.tolist())) and WR.flags_of(seg, win) == WR.flags_of(seg, tuple(w.tolist()))
        else:
            dead += 1
            assert w.tolist() == list(win)
    assert live > 300 and dead > 300, (live, dead)


# ---- the boxes ----------------------------------------------------------------------------------------------------------
def test_inside_implies_flags_3_and_no_overlap_implies_no_hit(twin):
    """for random windows and boxes in cells: every segment whose quantised box lies in a box that is `inside` has flags 3,
    and none whose box lies in a box that does not `overlap` meets the window"""
    rng = random.Random(19)
    q = lambda v: (v + (1 << 46)) >> 16  # noqa: E731
    inside = apart = 0
    for _ in range(3000):
        unit = 1 << rng.choice((16, 17, 20))
        cx, cy = rng.randint(LO + 8 * unit, HI - 8 * unit), rng.randint(LO + 8 * unit, HI - 8 * unit)
        near = lambda c: c + rng.randint(-4 * unit, 4 * unit)  # noqa: E731
        x0, x1 = sorted((near(cx), near(cx)))
        y0, y1 = sorted((near(cy), near(cy)))
        win = (x0, y0, x1, y1)
        short = lambda c: c + rng.randint(-unit, unit)  # noqa: E731  (a segment shorter than most windows: inside happens)
        seg = (near(cx), near(cy), near(cx), near(cy)) if rng.random() < 0.3 else (short(cx), short(cy), short(cx), short(cy))
        # a box of the index above the segment: its own box in cells, grown by a cell or two on some sides
        box = np.array([q(min(seg[0], seg[2])) - rng.randint(0, 1), q(min(seg[1], seg[3])) - rng.randint(0, 1), q(max(seg[0], seg[2])) + rng.randint(0, 1),
                        q(max(seg[1], seg[3])) + rng.randint(0, 1)], np.int32)
        r = twin.window_box(box.ctypes.data, np.array(win, np.int64).ctypes.data)
        assert r >= 0
        if r & 2:
            inside += 1
            assert r & 1 and WR.meets(seg, win) and WR.flags_of(seg, win) == 3, (seg, win, box)
        if not r & 1:
            apart += 1
            assert not WR.meets(seg, win), (seg, win, box)
    assert inside > 100 and apart > 300, (inside, apart)
    # the empty box (padding) neither overlaps nor lies inside, whatever the window
    pad = np.array([0x7FFFFFFF, 0x7FFFFFFF, -1, -1], np.int32)
    assert twin.window_box(pad.ctypes.data, np.array([LO, LO, HI, HI], np.int64).ctypes.data) == 0


def test_the_shortcut_and_the_prune_only_save_work(twin):
    from rayjoin_amd import maps, synth
    m = maps.Context([synth.lattice_map(12, 5, 3)]).load().maps[0]
    seg = m.segments()
    x0, y0, x1, y1 = (int(v) for v in (m.pts[:, 0].min(), m.pts[:, 1].min(), m.pts[:, 0].max(), m.pts[:, 1].max()))
    windows = [(x0, y0, (x0 + x1) // 2, (y0 + y1) // 2), (x0 - (1 << 17), y0 - (1 << 17), x1 + (1 << 17), y1 + (1 << 17))]
    full, _, work_full = run_twin(twin, seg, windows, contained=0, prune=0)
    fast, _, work_fast = run_twin(twin, seg, windows, contained=1, prune=1)
    assert full == fast and work_full == [2 * len(seg), 0]
    assert all(f == 3 for _, f in fast[1]) and len(fast[1]) == len(seg) and work_fast[1] >= len(seg) and work_fast[0] < len(seg) // 2


# ---- refusals, the counting call and the overflow -------------------------------------------------------------------------
def test_refusals_counting_call_and_overflow(twin):
    c = WC.HAND["inside_leaving_and_outside"]
    seg = seg_array(NR.edges_of(c.pts, c.row))
    win = np.array([WC.W, (100, 100, 200, 200), WC.W], np.int64)  # lists of 3, 0 and 3
    counts, out = np.full(3, 77, np.uint64), np.zeros(8, np.uint32)
    for nw, cap, cnt, eid, w in [(1 << 32, 8, counts, out, win), (3, 1 << 32, counts, out, win), (3, 8, None, out, win), (3, 8, counts, None, win),
                                 (3, 8, counts, out, None)]:
        assert twin.window_twin(seg.ctypes.data, len(seg), None if w is None else w.ctypes.data, nw, 0, 1, 1, cap, None, None if eid is None else eid.ctypes.data,
                                None, None if cnt is None else cnt.ctypes.data, None) == INVALID
        assert (counts == 77).all() and not out.any()
    for v in VARIANTS:
        rc, cnts, off, eid, flg, _ = call_twin(twin, seg, win, *v, capacity=0)
        assert rc == OK and cnts == [6, 2, 3] and off.tolist() == [0, 3, 3, 6]
        rc, cnts, off, eid, flg, _ = call_twin(twin, seg, win, *v, capacity=5)  # one short: true counts and offsets, nothing else
        assert rc == OVERFLOW and cnts == [6, 2, 3] and off.tolist() == [0, 3, 3, 6] and (eid == CANARY32).all() and (flg == CANARY8).all()
        rc, cnts, off, eid, flg, _ = call_twin(twin, seg, win, *v, capacity=6, flags=False, offsets=False)
        assert rc == OK and eid.tolist() == [0, 1, 2, 0, 1, 2] and (flg == CANARY8).all()
    rc, cnts, off, *_ = call_twin(twin, seg, np.zeros((0, 4), np.int64), capacity=4)  # no windows: zero counts, offsets[0] = 0
    assert rc == OK and cnts == [0, 0, 0] and off.tolist() == [0]


# ---- mutations of the header, each caught by a hand case -----------------------------------------------------------------
MUTATIONS = [
    # (tag, the text, its replacement, the hand case that catches it)
    ("box_test_strict", "return hx >= w.x0 && lx <= w.x1", "return hx > w.x0 && lx <= w.x1", "collinear_overlaps_side"),
    ("dropped_corner", "for (int k = 0; k < 4; k++) {", "for (int k = 0; k < 3; k++) {", "cuts_top_right_corner"),
    ("containment_not_strict", "bx0 > q.x0 && bx1 < q.x1 && by0 > q.y0", "bx0 >= q.x0 && bx1 < q.x1 && by0 > q.y0", "same_cell_beside_wide_window"),
]


@pytest.mark.parametrize("tag,old,new,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught(tag, old, new, name, tmp_path):
    text = open(os.path.join(CSRC, "rj_window.h")).read()
    assert text.count(old) == 1
    with open(tmp_path / "rj_window.h", "w") as f:
        f.write(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mut_" + tag)
    c = WC.HAND[name]
    seg = seg_array(NR.edges_of(c.pts, c.row))
    offsets, eids, flags = WR.csr_of(c.want)
    wrong = []
    for v in VARIANTS:
        rc, counts, off, eid, flg, _ = call_twin(L, seg, c.windows, *v, capacity=len(eids) + 2)
        n = min(counts[0], len(eid))
        if rc != OK or eid[:n].tolist() != eids or flg[:n].tolist() != flags or off.tolist() != offsets:
            wrong.append(v)
    assert wrong, "the mutant %s survives the hand case %s" % (tag, name)


# ---- the stand-alone twin under the host sanitizers ----------------------------------------------------------------------
def case_text(c):
    edges = NR.edges_of(c.pts, c.row)
    offsets, eids, flags = WR.csr_of(c.want)
    words = [len(edges), len(c.windows), len(eids)] + [v for e in edges for v in e] + [v for w in c.windows for v in w] + offsets
    for e, f in zip(eids, flags):
        words += [e, f]
    return " ".join(str(int(v)) for v in words)


def test_standalone_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "window_twin_san")
    subprocess.check_call(CXX[:1] + ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-DWINDOW_TWIN_MAIN", "-I", CSRC, "-o", exe, SRC])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(case_text(WC.HAND[k]) for k in sorted(WC.HAND)) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 failures" % len(WC.HAND) in r.stdout and "runtime error" not in r.stderr
