"""Merging faces by class and re-joining chains on the CPU: the plain-Python definition (tests/dissolve_ref.py) on the maps
of tests/dissolve_cases.py with the answers written out; the host twin of the device's per-element functions
(tests/hosttwin/dissolve_twin.cc compiling rayjoin_amd/csrc/rj_dissolve.h) against that definition, every array and every
count, with and without records, chain_origin and chain_out: the hand cases, the constructed maps that cross a wave and a
block, 12 generated planar maps under three class tables, odd labels; two independent answers on the planar maps (the class
areas from the generator's triangle counts, the map from the composition rings -> relabel -> rings_map in canonical form);
the properties (a second call changes nothing, no joinable vertex is left, the edges are preserved); the contract of the
call (sizing, exact capacity, each capacity one short with canaries, every refusal); three mutations of a scratch copy of
the header, each caught by a hand case; the twin as a stand-alone program under the host sanitizers.  The GPU side is
tests/test_gpu_dissolve.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dissolve_cases as DC  # noqa: E402
import dissolve_ref as DR  # noqa: E402
import ringmap_ref as MR  # noqa: E402
import rings_planar as RP  # noqa: E402
import rings_ref as RR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "dissolve_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
HEADER = os.path.join(CSRC, "rj_dissolve.h")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
CLASS_DTYPE = np.dtype([("label", "<i4"), ("n_sides", "<u4"), ("area2_lo", "<u8"), ("area2_hi", "<i8")])
CANARY32, CANARY64 = 0x5B5B5B5B, 0x5B5B5B5B5B5B5B5B
OK, INVALID, OVERFLOW = 0, 1, 3
SEEDS = tuple(range(12))
TABLES = ("identity", 2, 3)


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_dissolve.h")] + [os.path.join(CSRC, h) for h in ("rj_rings.h", "rj_ringmap.h", "rj_eliminate.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libdissolve_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.dissolve_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64,
                                C.c_uint64, C.c_uint64] + [C.c_void_p] * 8
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def arrays(m):
    return (np.ascontiguousarray(m[0], np.int64).reshape(-1, 2), np.ascontiguousarray(m[1], np.uint32), np.ascontiguousarray(m[2], np.int32),
            np.ascontiguousarray(m[3], np.int32))


def records_of(rows):
    """CLASS_DTYPE rows -> the dicts of dissolve_ref"""
    return [dict(label=int(r["label"]), n_sides=int(r["n_sides"]), area2=(int(r["area2_hi"]) << 64) | int(r["area2_lo"])) for r in rows]


def ptr(a):
    return a.ctypes.data if a is not None else None


def twin_dissolve(L, m, classes=None, flags=0, records=True, origin=True, chain_out=True, capacities=None):
    """-> (status, Result or None, counts).  capacities None: the sizing call, then the exact capacities; else (classes,
    chains, points).  Behind every capacity lie canaries that must survive; an overflow or a refusal leaves every output
    as it was."""
    xy, row, left, right = arrays(m)
    table = None if classes is None else np.ascontiguousarray(classes, np.int32)
    nc = max(0, len(row) - 1)
    counts = np.zeros(8, np.uint64)

    def call(caps, recs, ol, orr, oxy, orow, org, cout):
        return L.dissolve_twin(xy.ctypes.data, len(xy), row.ctypes.data, left.ctypes.data, right.ctypes.data, nc, ptr(table), 0 if table is None else len(table),
                               flags, caps[0], caps[1], caps[2], ptr(recs), ptr(ol), ptr(orr), ptr(oxy), ptr(orow), ptr(org), ptr(cout), counts.ctypes.data)

    def named():
        return dict(zip(DR.COUNTS, (int(v) for v in counts)))
    if capacities is None:
        rc = call((0, 0, 0), None, None, None, None, None, None, None)
        c = named()
        if rc not in (OK, OVERFLOW):
            return rc, None, c
        capacities = (c["n_classes"], c["n_chains"], c["n_points"])
    kc, cc, pc = capacities
    recs = np.zeros(kc + 2, CLASS_DTYPE) if records else None
    if records:
        recs.view(np.uint32)[:] = CANARY32
    ol, orr = np.full(cc + 2, CANARY32, np.uint32).view(np.int32), np.full(cc + 2, CANARY32, np.uint32).view(np.int32)
    oxy, orow = np.full((pc + 2, 2), CANARY64, np.int64), np.full(cc + 3, CANARY32, np.uint32)
    org = np.full(cc + 2, CANARY32, np.uint32) if origin else None
    cout = np.full(nc + 2, CANARY32, np.uint32) if chain_out else None
    rc = call(capacities, recs, ol, orr, oxy, orow, org, cout)
    c = named()
    if rc != OK:
        assert all((a.view(np.uint32) == CANARY32).all() for a in (recs, ol, orr, oxy, orow, org, cout) if a is not None)
        return rc, None, c
    nk, n, npts = c["n_classes"], c["n_chains"], c["n_points"]
    assert (ol.view(np.uint32)[n:] == CANARY32).all() and (orr.view(np.uint32)[n:] == CANARY32).all()
    assert recs is None or (recs.view(np.uint32)[6 * nk:] == CANARY32).all()
    assert (oxy[npts:] == CANARY64).all() and (orow[n + 1:] == CANARY32).all() and (org is None or (org[n:] == CANARY32).all())
    assert cout is None or (cout[nc:] == CANARY32).all()
    return rc, DR.Result(classes=records_of(recs[:nk]) if records else None, left=ol[:n].copy(), right=orr[:n].copy(), xy=oxy[:npts], row_index=orow[:n + 1],
                         origin=org[:n] if origin else None, chain_out=cout[:nc] if chain_out else None, counts=c), c


def same(got, want, records=True, origin=True, chain_out=True):
    """(status, Result, counts) of the twin or the device against dissolve_ref's Result"""
    rc, r, c = got
    assert rc == OK and c == want.counts, (rc, c, want.counts)
    assert np.array_equal(r.xy, want.xy) and np.array_equal(r.row_index, want.row_index)
    assert np.array_equal(r.left, want.left) and np.array_equal(r.right, want.right)
    assert not records or r.classes == want.classes
    assert not origin or np.array_equal(r.origin, want.origin)
    assert not chain_out or np.array_equal(r.chain_out, want.chain_out)


# ---- the inputs: computed once, shared, never changed ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planar(seed):
    return RP.draw_planar(seed)


def table_of(m, kind):
    """the class table of a map: None (identity) or 1 + f % kind with 0 staying 0"""
    if kind == "identity":
        return None
    f = np.arange(max(1, int(max(m[2].max(), m[3].max())) + 1), dtype=np.int64)
    t = (1 + f % kind).astype(np.int32)
    t[0] = 0
    return t


@functools.lru_cache(maxsize=None)
def input_of(kind, key):
    """-> (map, class table or None, flags)"""
    if kind == "hand":
        k = DC.HAND[key]
        return k["map"], k["classes"], k["flags"]
    if kind == "built":
        k = DC.constructed(*key)
        return k["map"], k["classes"], k["flags"]
    if kind == "odd":
        return RP.odd_faces(), None, key
    m = planar(key[0])[0]
    return m, table_of(m, key[1]), key[2]


@functools.lru_cache(maxsize=None)
def answer(kind, key):
    m, table, flags = input_of(kind, key)
    return DR.dissolve_ref(*m, table, flags)


HAND_OK = sorted(n for n in DC.HAND if not DC.HAND[n]["unmapped"])
SMALL = [("hand", n) for n in HAND_OK] + [("built", k) for k in DC.CONSTRUCTED] + [("odd", 0), ("odd", DR.KEEP_EQUAL)]
PLANAR = [("planar", (s, t, 0)) for s in SEEDS for t in TABLES] + [("planar", (s, "identity", DR.KEEP_EQUAL)) for s in SEEDS[:4]]
EVERY = SMALL + PLANAR


# ---- the definition against the written answers -------------------------------------------------------------------------
def check_written(k, r):
    want_xy = [p for pts, _, _ in k["chains"] for p in pts]
    assert r.xy.tolist() == [list(p) for p in want_xy]
    assert r.row_index.tolist() == np.cumsum([0] + [len(pts) for pts, _, _ in k["chains"]]).tolist()
    assert r.left.tolist() == [le for _, le, _ in k["chains"]] and r.right.tolist() == [ri for _, _, ri in k["chains"]]
    assert r.origin.tolist() == k["origin"] and r.chain_out.tolist() == k["chain_out"]
    assert all(r.counts[name] == v for name, v in k["counts"].items()) and r.counts["n_unmapped"] == 0
    if k["records"] is not None:
        assert [(f["label"], f["n_sides"], f["area2"]) for f in r.classes] == [(f,) + k["records"][f] for f in sorted(k["records"], key=DR.unsigned)]


@pytest.mark.parametrize("name", HAND_OK)
def test_definition_gives_the_written_answer(name):
    check_written(DC.HAND[name], answer("hand", name))


@pytest.mark.parametrize("key", DC.CONSTRUCTED, ids=str)
def test_definition_gives_the_constructed_answer(key):
    check_written(DC.constructed(*key), answer("built", key))


@pytest.mark.parametrize("name", ["unmapped", "unmapped-negative"])
def test_definition_counts_unmapped_labels(twin, name):
    k = DC.HAND[name]
    with pytest.raises(DR.Unmapped) as e:
        DR.dissolve_ref(*k["map"], k["classes"], 0)
    assert e.value.n_unmapped == k["unmapped"]
    n = len(k["map"][2])
    for caps in (None, (4, n, len(k["map"][0]) + n)):
        rc, _, c = twin_dissolve(twin, k["map"], k["classes"], 0, capacities=caps)  # (twin_dissolve checks that nothing was written)
        assert rc == INVALID and c == dict(dict.fromkeys(DR.COUNTS, 0), n_unmapped=k["unmapped"])


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_twin(twin, what):
    m, table, flags = input_of(*what)
    want = answer(*what)
    same(twin_dissolve(twin, m, table, flags), want)
    same(twin_dissolve(twin, m, table, flags, records=False, origin=False, chain_out=False), want, records=False, origin=False, chain_out=False)


# ---- independent answers on the generated maps ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_class_areas_are_the_generators(seed):
    """area2 of a class = det x the triangles of its faces, which the generator knows without any chain"""
    m, info = planar(seed)
    for t in TABLES:
        table, r = table_of(m, t), answer("planar", (seed, t, 0))
        want = {}
        for f, n in info["triangles"].items():
            k = f if table is None or f == 0 else int(table[f])
            if k != 0:
                want[k] = want.get(k, 0) + info["det"] * n
        assert {f["label"]: f["area2"] for f in r.classes} == want


@pytest.mark.parametrize("seed", SEEDS)
def test_the_composition_gives_the_same_map(seed):
    """rings -> relabel the rings -> rings_map with its dissolve flag: the route there was before, in canonical form.
    Compared where the composition reports no conflict: on these inputs that is everywhere, and none may be left out"""
    m, _ = planar(seed)
    rings = RR.rings_ref(*m)
    for t in TABLES:
        table, r = table_of(m, t), answer("planar", (seed, t, 0))
        face = rings["rings"]["face"].astype(np.int64)
        ring_class = face if table is None else np.where(face == 0, 0, table[np.clip(face, 0, len(table) - 1)])
        comp = MR.rings_map_ref(rings["ring_row"], rings["ring_xy"], ring_class.astype(np.int32), dissolve=True)
        assert comp["counts"]["n_conflicts"] == 0
        assert DR.canonical(r.xy, r.row_index, r.left, r.right) == DR.canonical(*MR.as_map(comp))


def test_generated_maps_are_worth_their_time():
    """some output chain joins chains of opposite digitisation, some closed one is a loop of two chains or more"""
    rs = [answer(*w) for w in PLANAR]
    assert any(len({h & 1 for h in w}) == 2 for r in rs for w in r.walks)
    assert any(closed and len(w) >= 2 for r in rs for w, closed in zip(r.walks, r.closed))
    assert all(r.counts["n_dropped"] > 0 for r in rs[1:3])


# ---- the properties ------------------------------------------------------------------------------------------------------
def joinable(r):
    """the vertices of degree exactly 2 of a result whose two chains have equal class pairs through it"""
    ends = {}
    for k in range(len(r.left)):
        b, e = int(r.row_index[k]), int(r.row_index[k + 1]) - 1
        ends.setdefault(tuple(r.xy[b]), []).append((k, (int(r.left[k]), int(r.right[k]))))   # leaves with (l, r)
        ends.setdefault(tuple(r.xy[e]), []).append((k, (int(r.right[k]), int(r.left[k]))))   # leaves backwards with (r, l)
    return [p for p, v in ends.items() if len(v) == 2 and v[0][0] != v[1][0] and v[0][1] == v[1][1][::-1]]


def properties(dissolve, what):
    """dissolve(map, table, flags) -> Result"""
    m, table, flags = input_of(*what)
    r = dissolve(m, table, flags)
    again = dissolve((r.xy, r.row_index, r.left, r.right), None, flags)
    assert again.counts["n_kept"] == again.counts["n_chains"] == r.counts["n_chains"] and again.counts["n_closed"] == r.counts["n_closed"]
    assert np.array_equal(again.xy, r.xy) and np.array_equal(again.row_index, r.row_index)
    assert np.array_equal(again.left, r.left) and np.array_equal(again.right, r.right)
    assert [(f["label"], f["area2"]) for f in again.classes] == [(f["label"], f["area2"]) for f in r.classes]  # (fewer sides carry them)
    assert joinable(r) == []
    row = m[1].astype(np.int64)
    kept = r.chain_out != DR.NONE
    assert r.counts["n_points"] - r.counts["n_chains"] == int((row[1:] - row[:-1] - 1)[kept].sum()) and int(kept.sum()) == r.counts["n_kept"]
    assert all(int(r.row_index[k + 1]) - int(r.row_index[k]) >= 2 for k in range(len(r.left)))


@pytest.mark.parametrize("what", EVERY, ids=str)
def test_properties(twin, what):
    def by_twin(m, table, flags):
        rc, r, _ = twin_dissolve(twin, m, table, flags)
        assert rc == OK
        return r
    properties(by_twin, what)
    properties(lambda m, table, flags: DR.dissolve_ref(*m, table, flags), what)


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_sizing_call_exact_capacity_and_one_short(twin):
    what = ("planar", (3, 3, 0))
    (m, table, flags), want = input_of(*what), answer(*what)
    c = want.counts
    assert c["n_classes"] == 3 and 0 < c["n_chains"] < c["n_kept"] and c["n_dropped"] > 0
    caps = (c["n_classes"], c["n_chains"], c["n_points"])
    rc, _, got = twin_dissolve(twin, m, table, flags, capacities=(0, 0, 0))
    assert rc == OVERFLOW and got == c
    same(twin_dissolve(twin, m, table, flags, capacities=caps), want)
    same(twin_dissolve(twin, m, table, flags, capacities=tuple(v + 3 for v in caps)), want)
    for k in range(3):
        short = tuple(v - (1 if j == k else 0) for j, v in enumerate(caps))
        rc, _, got = twin_dissolve(twin, m, table, flags, capacities=short)  # (twin_dissolve checks that nothing was written)
        assert (rc, got) == (OVERFLOW, c)
    same(twin_dissolve(twin, m, table, flags, records=False, capacities=(0,) + caps[1:]), want, records=False)  # no records: no class capacity


def test_no_chains(twin):
    empty = (np.zeros((0, 2), np.int64), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for flags in (0, DR.KEEP_EQUAL):
        rc, r, c = twin_dissolve(twin, empty, None, flags)
        assert rc == OK and c == dict.fromkeys(DR.COUNTS, 0) == DR.dissolve_ref(*empty, None, flags).counts and r.row_index.tolist() == [0]


def test_a_map_where_everything_dissolves(twin):
    """that fits capacities of 0, so the sizing call, whose arrays are null, succeeds and must write nothing"""
    k, want = DC.HAND["all-dissolve"], answer("hand", "all-dissolve")
    assert want.counts["n_chains"] == want.counts["n_points"] == 0 and want.row_index.tolist() == [0]
    xy, row, left, right = arrays(k["map"])
    counts = np.zeros(8, np.uint64)
    rc = twin.dissolve_twin(xy.ctypes.data, len(xy), row.ctypes.data, left.ctypes.data, right.ctypes.data, 3, k["classes"].ctypes.data, 3, 0, 0, 0, 0,
                            None, None, None, None, None, None, None, counts.ctypes.data)
    assert rc == OK and dict(zip(DR.COUNTS, (int(v) for v in counts))) == want.counts
    same(twin_dissolve(twin, k["map"], k["classes"], 0), want)


def refused(twin, m, table=None, flags=0):
    """the definition refuses it, and so does the twin"""
    with pytest.raises(DR.Invalid):
        DR.dissolve_ref(*m, table, flags)
    n = len(m[2])
    return twin_dissolve(twin, m, table, flags)[0] == INVALID and twin_dissolve(twin, m, table, flags, capacities=(2 * n, n, len(m[0]) + n))[0] == INVALID


def test_bad_input(twin):
    xy, row, left, right = DC.chain_map([([(0, 0), (1, 0)], 1, 0), ([(2, 0), (3, 0)], 1, 2), ([(4, 0), (5, 0)], 2, 0)])
    assert twin_dissolve(twin, (xy, row, left, right))[0] == OK
    for bad_row in ([1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 2, 6], [0, 4, 2, 6], [0, 2, 4, 7]):
        assert refused(twin, (xy, np.array(bad_row, np.uint32), left, right))
    for v in (1 << 46, -(1 << 46) - 1):
        bad = xy.copy()
        bad[3, 1] = v
        assert refused(twin, (bad, row, left, right))
    assert refused(twin, (xy, row, left, right), flags=2) and refused(twin, (xy, row, left, right), flags=1 << 31) and refused(twin, (xy, row, left, right), flags=3)
    assert refused(twin, (xy[:2], row, left, right))  # more chains than points
    assert refused(twin, (xy, np.zeros(1, np.uint32), left[:0], right[:0]))  # points without chains
    assert refused(twin, (xy, row, left, right), table=np.array([0, 1], np.int32))  # label 2 outside the table
    counts = np.zeros(8, np.uint64)
    one = np.zeros(1, np.int32)
    args = [None, None, None, None, None, None, None, counts.ctypes.data]
    for n_points, n_chains in ((1 << 32, 3), (1 << 31, 1 << 31), ((1 << 31) + 3, 3), (2, 3), (3, 0)):  # the size limits: refused before anything is read
        assert twin.dissolve_twin(None, n_points, None, None, None, n_chains, None, 0, 0, 0, 0, 0, *args) == INVALID
    assert twin.dissolve_twin(None, 0, None, None, None, 0, one.ctypes.data, 0, 0, 0, 0, 0, *args) == INVALID  # a table without labels


# ---- mutations of the header, each caught ------------------------------------------------------------------------------------
MUTATIONS = {
    # a change of classes at a vertex of degree 2 no longer ends a walk
    "ignore-classes": ("if (left_of(g, cl, cr) != left_of(h, cl, cr) || right_of(g, cl, cr) != right_of(h, cl, cr)) return kNone;", "", "class-change"),
    # a third half-chain above the other two is not looked for
    "third-at-vertex": ("if (k + 2 < nh && starts_at(order[k + 2], start, p)) return kNone;", "", "t-junction"),
    # a chain whose points are all equal counts as a chain
    "skip-nothing": ("*differs = *differs || px != x0 || py != y0;", "*differs = true;", "skipped"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_mutated_header_is_caught(name, tmp_path):
    old, new, case = MUTATIONS[name]
    text = open(HEADER).read()
    assert text.count(old) == 1
    (tmp_path / "rj_dissolve.h").write_text(text.replace(old, new))
    L = twin_lib(str(tmp_path), "_mutant_" + name)
    os.remove(os.path.join(BUILD, "libdissolve_twin_mutant_%s.so" % name))
    m, table, flags = input_of("hand", case)
    rc, r, _ = twin_dissolve(L, m, table, flags)
    want = answer("hand", case)
    assert rc == OK and not (np.array_equal(r.row_index, want.row_index) and np.array_equal(r.xy, want.xy))
    same(twin_dissolve(L, *input_of("hand", "loop-of-two")), answer("hand", "loop-of-two"))  # (the same program otherwise)


# ---- the stand-alone program under the host sanitizers ----------------------------------------------------------------------
def case_text(m, table, flags, want, status):
    xy, row, left, right = arrays(m)
    out = [len(xy), len(row) - 1, -1 if table is None else len(table), flags]
    out += xy.reshape(-1).tolist() + row.tolist() + left.tolist() + right.tolist() + ([] if table is None else np.asarray(table).tolist())
    if status != OK:
        return " ".join(str(v) for v in out + [status] + [want[n] for n in DR.COUNTS])
    out += [OK] + [want.counts[n] for n in DR.COUNTS]
    out += want.xy.reshape(-1).tolist() + want.row_index.tolist() + want.left.tolist() + want.right.tolist() + want.origin.tolist() + want.chain_out.tolist()
    for f in want.classes:
        out += [f["label"], f["n_sides"], f["area2"] & (2 ** 64 - 1), ((f["area2"] >> 64) + 2 ** 63) % 2 ** 64 - 2 ** 63]
    return " ".join(str(v) for v in out)


def test_stand_alone_twin_program_under_sanitizers(tmp_path):
    """the twin with its own main, built with -fsanitize=address,undefined and run as a program of its own (nothing is
    loaded into Python under a sanitizer) over the hand cases, the refused ones included, and the constructed maps"""
    exe = os.path.join(BUILD, "dissolve_twin_main_san")
    os.makedirs(BUILD, exist_ok=True)
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDISSOLVE_TWIN_MAIN",
                               "-I", CSRC, "-o", exe, SRC])
    lines = [case_text(*input_of(*w), answer(*w), OK) for w in SMALL]
    for name in ("unmapped", "unmapped-negative"):
        k = DC.HAND[name]
        lines.append(case_text(k["map"], k["classes"], 0, dict(dict.fromkeys(DR.COUNTS, 0), n_unmapped=k["unmapped"]), INVALID))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == len(lines) and "MISMATCH" not in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
