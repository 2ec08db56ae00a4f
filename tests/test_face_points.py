"""Per-face counts, sums and members of located points on the CPU: the plain-Python definition (tests/face_points_ref.py) on
the hand cases of tests/face_points_cases.py with the answers written out; the host twin of the device's per-element
functions (tests/hosttwin/face_points_twin.cc compiling rayjoin_amd/csrc/rj_face_points.h) against that definition, array
for array and count for count, with and without values, universe, RJ_FP_MEMBERS and the records: the hand cases, the
layouts on which the wave logic can break at every size, one run over many blocks, the Zipf-like sweep; the contract of the
call (sizing, exact capacity, each capacity one short with canaries, every refusal, n == 0); three mutations of a scratch
copy of the header, each caught by a hand case; the twin as a stand-alone program under the host sanitizers.  The GPU side
is tests/test_gpu_face_points.py."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import face_points_cases as FC  # noqa: E402
import face_points_ref as FR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hosttwin", "face_points_twin.cc")
CSRC = os.path.join(ROOT, "rayjoin_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "hosttwin", "_build")
FACE_DTYPE = np.dtype([("label", "<i4"), ("first", "<u4"), ("n_points", "<u8"), ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("min", "<i8"), ("max", "<i8")])
CANARY32, CANARY64 = 0x5B5B5B5B, 0x5B5B5B5B5B5B5B5B
OK, INVALID, OVERFLOW = 0, 1, 3
assert FACE_DTYPE.itemsize == 48


def stale(out, hdr_dir=CSRC):
    deps = [SRC, os.path.join(hdr_dir, "rj_face_points.h")] + [os.path.join(CSRC, h) for h in ("rj_rings.h", "rj_eliminate.h")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps)


def twin_lib(hdr_dir=CSRC, tag=""):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libface_points_twin%s.so" % tag)
    if stale(out, hdr_dir):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", hdr_dir, "-I", CSRC, "-o", out, SRC])
    L = C.CDLL(out)
    L.face_points_twin.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    return L


@pytest.fixture(scope="module")
def twin():
    return twin_lib()


def faces_of(rows):
    """FACE_DTYPE rows -> the dicts of face_points_ref"""
    return [dict(label=int(r["label"]), first=int(r["first"]), n_points=int(r["n_points"]), sum=(int(r["sum_hi"]) << 64) + int(r["sum_lo"]), min=int(r["min"]),
                 max=int(r["max"])) for r in rows]


def ptr(a):
    return a.ctypes.data if a is not None else None


def host_arrays(c):
    """labels with one entry behind them (a mutant of the header may look there), values, the universe as an array that
    exists even where it is empty"""
    labels = np.concatenate([c.labels, np.array([0x7EEEEEEE], np.int32)])
    universe = None if c.universe is None else np.concatenate([c.universe, np.zeros(1, np.int32)])
    return labels, c.values, universe


def twin_face_points(L, c, flags=0, records=True, capacities=None):
    """-> (status, Result or None, counts).  capacities None: the sizing call, then the exact capacities; else (faces,
    members).  Behind every capacity lie canaries that must survive; an overflow or a refusal leaves every output as it was."""
    labels, values, universe = host_arrays(c)
    n, nfl = len(c.labels), 0 if c.universe is None else len(c.universe)
    counts = np.zeros(len(FR.COUNTS), np.uint64)
    members_on = bool(flags & FR.MEMBERS)

    def call(caps, faces, offsets, members):
        return L.face_points_twin(labels.ctypes.data, n, ptr(values), c.stride, ptr(universe), nfl, flags, caps[0], caps[1], ptr(faces), ptr(offsets), ptr(members),
                                  counts.ctypes.data)

    def named():
        return dict(zip(FR.COUNTS, (int(v) for v in counts)))
    if capacities is None:
        rc = call((0, 0), None, None, None)
        k = named()
        if rc not in (OK, OVERFLOW):
            return rc, None, k
        capacities = (k["n_faces"], k["n_members"] if members_on else 0)
    fc, mc = capacities
    faces = np.zeros(fc + 2, FACE_DTYPE) if records else None
    if records:
        faces.view(np.uint32)[:] = CANARY32
    offsets, members = np.full(fc + 3, CANARY64, np.uint64), np.full(mc + 2, CANARY32, np.uint32)
    rc = call((fc if records or members_on else 0, mc), faces, offsets, members)
    k = named()
    if rc != OK:
        assert all((a.view(np.uint32) == CANARY32).all() for a in (faces, offsets, members) if a is not None)
        if rc == OVERFLOW and not records and not members_on and capacities[1] == 0:  # neither records nor members: the counts are all there is
            return OK, FR.Result(None, None, None, k), k
        return rc, None, k
    nf, nm = k["n_faces"], k["n_members"]
    assert faces is None or (faces.view(np.uint32)[12 * nf:] == CANARY32).all()
    if members_on:
        assert (offsets[nf + 1:] == CANARY64).all() and (members[nm:] == CANARY32).all()
    else:
        assert (offsets == CANARY64).all() and (members == CANARY32).all()  # without the flag neither array is touched
    return rc, FR.Result(faces=faces_of(faces[:nf]) if records else None, offsets=[int(v) for v in offsets[:nf + 1]] if members_on else None,
                         members=[int(v) for v in members[:nm]] if members_on else None, counts=k), k


def same(got, want, records=True):
    """(status, Result, counts) of the twin or the device against face_points_ref's Result"""
    rc, r, k = got
    assert rc == OK and k == want.counts, (rc, k, want.counts)
    assert r.offsets == want.offsets and r.members == want.members
    assert not records or r.faces == want.faces


# ---- the inputs: computed once, shared, never changed ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_of(kind, key):
    if kind == "hand":
        return FC.HAND[key]["case"]
    if kind == "layout":
        return FC.layout(*key)
    if kind == "big":
        return FC.big(key)
    return FC.sweep(*key)


def variant(c, values, universe):
    """the case without its values, or with a universe of its own where it has none"""
    return FC.Case(c.labels, c.values if values else None, c.stride, FC.universe_for(c) if universe and c.universe is None else c.universe)


@functools.lru_cache(maxsize=None)
def answer(kind, key, values, universe, flags):
    c = variant(case_of(kind, key), values, universe)
    return FR.face_points_ref(c.labels, c.values, c.stride, c.universe, flags)


VARIANTS = tuple(itertools.product((True, False), (False, True), (0, FR.MEMBERS)))  # values, universe, flags
HANDS = [("hand", n) for n in sorted(FC.HAND)]
LAYOUTS = [("layout", (kind, n)) for kind in FC.LAYOUTS[:3] for n in FC.SIZES] + [("layout", ("runs", 0))]
SMALL = HANDS + [("layout", (kind, n)) for kind in FC.LAYOUTS[:3] for n in (1, 65, 129)]
SWEEP = [("sweep", (s, o)) for s in FC.SWEEP_SEEDS for o in FC.ORDERS]
EVERY = HANDS + LAYOUTS + [("big", "face"), ("big", "outside")] + SWEEP


def check_all_variants(run, what):
    """run(case, flags, records) -> (status, Result, counts), held against the definition in every variant"""
    for values, universe, flags in VARIANTS:
        c = variant(case_of(*what), values, universe)
        want = answer(*what, values, universe, flags)
        same(run(c, flags, True), want)
        same(run(c, flags, False), want, records=False)


# ---- the definition against the written answers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.HAND))
def test_definition_gives_the_written_answer(name):
    k = FC.HAND[name]
    c = k["case"]
    r = FR.face_points_ref(c.labels, c.values, c.stride, c.universe, FR.MEMBERS)
    assert r.faces == k["faces"] and r.offsets == k["offsets"] and r.members == k["members"] and r.counts == k["counts"]
    plain = FR.face_points_ref(c.labels, c.values, c.stride, c.universe, 0)
    assert plain.faces == k["faces"] and plain.counts == k["counts"] and plain.offsets is None and plain.members is None
    assert [FR.unsigned(f["label"]) for f in r.faces] == sorted(FR.unsigned(f["label"]) for f in r.faces)


def test_the_wide_sum_leaves_64_bits_on_both_sides():
    sums = {f["label"]: f["sum"] for f in FC.HAND["wide-sum"]["faces"]}
    assert sums[9] == 2 ** 64 - 5 > FR.INT64_MAX and sums[5] > FR.INT64_MAX and sums[4] < FR.INT64_MIN


def test_the_runs_start_and_end_on_every_lane():
    """the "runs" layout: runs of every length 1 .. 130, a run start and a run end on each of the 64 lanes, runs that
    straddle a wave and runs that straddle a block of 256"""
    lengths = FC.run_lengths()
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    ends = np.cumsum(lengths) - 1
    assert set(lengths) >= set(range(1, 131))
    assert {int(s) % 64 for s in starts} == set(range(64)) == {int(e) % 64 for e in ends}
    assert any(s // 64 != e // 64 for s, e in zip(starts, ends)) and any(s // 256 != e // 256 for s, e in zip(starts, ends))
    labels = case_of("layout", ("runs", 0)).labels
    assert len(labels) == sum(lengths) and FR.face_points_ref(labels).counts["n_runs"] == len(lengths)  # (neighbouring runs differ)


def test_the_sweep_is_skewed():
    """the outside and the largest face take most points of a sorted draw"""
    r = answer("sweep", (3, "sorted"), True, False, 0)
    top = max(f["n_points"] for f in r.faces)
    assert r.counts["n_outside"] + top > sum(r.counts[k] for k in ("n_members", "n_outside")) // 2 and r.counts["n_faces"] > 10


# ---- the twin against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", EVERY, ids=str)
def test_twin(twin, what):
    check_all_variants(lambda c, flags, records: twin_face_points(twin, c, flags, records), what)


def test_twin_gives_the_written_answers(twin):
    for name, k in sorted(FC.HAND.items()):
        rc, r, counts = twin_face_points(twin, k["case"], FR.MEMBERS)
        assert rc == OK and r.faces == k["faces"] and r.offsets == k["offsets"] and r.members == k["members"] and counts == k["counts"], name


def check_members(r):
    """the members ascend inside every face, are a permutation of the member points, and start at `first`"""
    for k, f in enumerate(r.faces):
        mine = r.members[r.offsets[k]:r.offsets[k + 1]]
        assert mine == sorted(mine) and len(mine) == f["n_points"] and f["first"] == (mine[0] if mine else FR.NO_POINT)
    assert len(set(r.members)) == len(r.members) == r.counts["n_members"] == r.offsets[-1]


@pytest.mark.parametrize("what", [("layout", ("runs", 0)), ("sweep", (5, "shuffled")), ("sweep", (8, "blocks")), ("hand", "universe")], ids=str)
def test_members(twin, what):
    for universe in (False, True):
        c = variant(case_of(*what), True, universe)
        rc, r, _ = twin_face_points(twin, c, FR.MEMBERS)
        assert rc == OK
        check_members(r)
        index = {f["label"]: k for k, f in enumerate(r.faces)}
        assert sorted(r.members) == [i for i, v in enumerate(c.labels) if int(v) in index]


# ---- the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, FR.MEMBERS))
def test_sizing_call_exact_capacity_and_one_short(twin, flags):
    what = ("sweep", (4, "blocks"))
    c, want = case_of(*what), answer(*what, True, False, flags)
    k = want.counts
    assert k["n_faces"] > 3 and k["n_members"] > 3
    caps = (k["n_faces"], k["n_members"] if flags else 0)
    rc, _, got = twin_face_points(twin, c, flags, capacities=(0, 0))
    assert rc == OVERFLOW and got == k
    same(twin_face_points(twin, c, flags, capacities=caps), want)
    same(twin_face_points(twin, c, flags, capacities=(caps[0] + 3, caps[1] + 3 if flags else 0)), want)
    for j in range(2 if flags else 1):
        short = tuple(v - (1 if i == j else 0) for i, v in enumerate(caps))
        for records in (True, False) if flags else (True,):  # (without the flag and the records there is no capacity to be short of)
            rc, _, got = twin_face_points(twin, c, flags, records=records, capacities=short)  # (twin_face_points checks that nothing was written)
            assert (rc, got) == (OVERFLOW, k)


def test_no_points(twin):
    for name in ("no-points", "no-points-universe", "all-outside", "empty-universe"):
        k = FC.HAND[name]
        for flags in (0, FR.MEMBERS):
            rc, r, counts = twin_face_points(twin, k["case"], flags)
            assert rc == OK and counts == k["counts"] and r.faces == k["faces"] and r.offsets == (k["offsets"] if flags else None)
    counts = np.zeros(5, np.uint64)
    assert twin.face_points_twin(None, 0, None, 1, None, 0, FR.MEMBERS, 0, 0, None, None, None, counts.ctypes.data) == OK and not counts.any()


def raw(twin, c, flags=0, caps=(0, 0), faces=True, offsets=True, members=True, n=None, stride=None, nfl=None, counts=True, labels=True):
    """the call itself with whatever arguments: outputs that exist are large enough for the capacities"""
    lab, values, universe = host_arrays(c)
    out = [np.zeros(caps[0] + 1, FACE_DTYPE), np.zeros(caps[0] + 2, np.uint64), np.zeros(caps[1] + 1, np.uint32), np.zeros(5, np.uint64)]
    return twin.face_points_twin(lab.ctypes.data if labels else None, len(c.labels) if n is None else n, ptr(values), c.stride if stride is None else stride,
                                 ptr(universe), (0 if c.universe is None else len(c.universe)) if nfl is None else nfl, flags, caps[0], caps[1],
                                 ptr(out[0]) if faces else None, ptr(out[1]) if offsets else None, ptr(out[2]) if members else None, ptr(out[3]) if counts else None)


def test_refusals(twin):
    c = FC.HAND["two-faces"]["case"]
    assert raw(twin, c, caps=(2, 0)) == OK and raw(twin, c, FR.MEMBERS, caps=(2, 4)) == OK
    for flags in (2, 3, 1 << 31):
        assert raw(twin, c, flags, caps=(2, 4)) == INVALID  # an unknown flag bit
        with pytest.raises(FR.Invalid):
            FR.face_points_ref(c.labels, c.values, c.stride, None, flags)
    assert raw(twin, c, labels=False) == INVALID  # null labels with n > 0
    assert raw(twin, c, counts=False) == INVALID  # null counts
    assert raw(twin, c, caps=(2, 0), faces=False) == INVALID  # a capacity without its array
    assert raw(twin, c, FR.MEMBERS, caps=(2, 4), offsets=False) == INVALID
    assert raw(twin, c, FR.MEMBERS, caps=(2, 4), members=False) == INVALID
    assert raw(twin, c, FR.MEMBERS, caps=(2, 4), faces=False) == OK  # (no records: the offsets carry the face capacity)
    assert raw(twin, c, caps=(2, 4)) == INVALID  # member_capacity without the flag
    assert raw(twin, c, stride=0) == INVALID  # value_stride == 0 with values
    assert raw(twin, FC.Case(c.labels, None, 1, None), stride=0) == OVERFLOW  # (without values the stride is not looked at: the sizing call)
    assert raw(twin, c, n=1 << 32) == INVALID and raw(twin, c, n=(1 << 32) + 5, labels=False) == INVALID  # n >= 2^32: refused before anything is read
    with pytest.raises(FR.Invalid):
        FR.face_points_ref(c.labels, c.values, 0)


@pytest.mark.parametrize("name", sorted(FC.BAD_UNIVERSES))
def test_a_bad_universe_is_refused(twin, name):
    c = FC.HAND["two-faces"]["case"]
    bad = FC.Case(c.labels, c.values, c.stride, np.array(FC.BAD_UNIVERSES[name], np.int32))
    with pytest.raises(FR.Invalid):
        FR.face_points_ref(bad.labels, bad.values, bad.stride, bad.universe)
    for flags in (0, FR.MEMBERS):
        rc, _, counts = twin_face_points(twin, bad, flags)
        assert rc == INVALID and counts == dict.fromkeys(FR.COUNTS, 0)
        rc, _, counts = twin_face_points(twin, bad, flags, capacities=(8, 8 if flags else 0))  # (twin_face_points checks that nothing was written)
        assert rc == INVALID and counts == dict.fromkeys(FR.COUNTS, 0)


# ---- mutations of the header, each caught ------------------------------------------------------------------------------------
# name -> ([(old, new)], the hand cases that catch it, with a universe of the case's own or not).  Every header of the directory is
# copied to a scratch directory that comes first on the include path, so the twin compiles the mutated copy and the
# repository's stays as it is.
MUTATIONS = {
    # the high limb of a value taken as unsigned: every negative value adds 2^64 to the sum
    "high-limb-unsigned": ([("(uint64_t) (uint32_t) v, v >> 32, v, v}", "(uint64_t) (uint32_t) v, (int64_t) ((uint64_t) v >> 32), v, v}")], ("cancel", "wide-sum")),
    # the run head compared with the next point, not the one before: a run takes the label of the point behind its end
    "head-looks-ahead": ([("RJ_RHD bool is_head(uint64_t i, const int32_t* label) { return i == 0 || label[i] != label[i - 1]; }",
                           "RJ_RHD bool is_head(uint64_t i, const int32_t* label) { return i == 0 || label[i] != label[i + 1]; }")], ("two-faces", "cancel")),
    # a universe check that accepts equal neighbours
    "universe-accepts-equal": ([(">= eliminate::key_of(face_label[k]);", "> eliminate::key_of(face_label[k]);")], ()),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_mutated_header_is_caught(name, tmp_path):
    edits, cases = MUTATIONS[name]
    for h in os.listdir(CSRC):
        if h.endswith(".h"):
            text = open(os.path.join(CSRC, h)).read()
            for old, new in edits if h == "rj_face_points.h" else ():
                assert text.count(old) == 1, old
                text = text.replace(old, new)
            (tmp_path / h).write_text(text)
    L = twin_lib(str(tmp_path), "_mutant_" + name)
    os.remove(os.path.join(BUILD, "libface_points_twin_mutant_%s.so" % name))
    for case in cases:
        k = FC.HAND[case]
        rc, r, counts = twin_face_points(L, k["case"], FR.MEMBERS)
        assert rc == OK and not (r.faces == k["faces"] and r.members == k["members"] and counts == k["counts"])
    if name == "universe-accepts-equal":
        c = FC.HAND["two-faces"]["case"]
        dup = FC.Case(c.labels, c.values, c.stride, np.array(FC.BAD_UNIVERSES["duplicate"], np.int32))
        assert twin_face_points(L, dup)[0] == OK  # (the repository's header refuses it: test_a_bad_universe_is_refused)
    k = FC.HAND["no-values"]  # (the same program otherwise: one face, no values, no universe)
    rc, r, counts = twin_face_points(L, k["case"], 0)
    assert rc == OK and counts["n_faces"] == 1 and counts["n_outside"] == 1


# ---- the stand-alone program under the host sanitizers ----------------------------------------------------------------------
def low(v):
    return v & (2 ** 64 - 1)


def case_text(c, flags, want, status):
    nfl = 0 if c.universe is None else len(c.universe)
    out = [len(c.labels), c.stride, int(c.values is not None), int(c.universe is not None), nfl, flags]
    if c.values is not None:
        out.append(len(c.values))
    out += c.labels.tolist() + ([] if c.values is None else c.values.tolist()) + ([] if c.universe is None else c.universe.tolist())
    if status != OK:
        return " ".join(str(v) for v in out + [status] + [want[n] for n in FR.COUNTS])
    out += [OK] + [want.counts[n] for n in FR.COUNTS]
    for f in want.faces:
        out += [f["label"], f["first"], f["n_points"], low(f["sum"]), (low(f["sum"] >> 64) + 2 ** 63) % 2 ** 64 - 2 ** 63, f["min"], f["max"]]
    if flags & FR.MEMBERS:
        out += want.offsets + want.members
    return " ".join(str(v) for v in out)


def test_stand_alone_twin_program_under_sanitizers(tmp_path):
    """the twin with its own main, built with -fsanitize=address,undefined and run as a program of its own (nothing is
    loaded into Python under a sanitizer) over the small cases in every variant, and the bad universes"""
    exe = os.path.join(BUILD, "face_points_twin_main_san")
    os.makedirs(BUILD, exist_ok=True)
    if stale(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFACE_POINTS_TWIN_MAIN",
                               "-I", CSRC, "-o", exe, SRC])
    lines = []
    for what in SMALL + [("layout", ("runs", 0)), ("sweep", (2, "shuffled"))]:
        for values, universe, flags in VARIANTS:
            lines.append(case_text(variant(case_of(*what), values, universe), flags, answer(*what, values, universe, flags), OK))
    c = FC.HAND["two-faces"]["case"]
    none = dict.fromkeys(FR.COUNTS, 0)
    for bad in FC.BAD_UNIVERSES.values():
        lines.append(case_text(FC.Case(c.labels, c.values, c.stride, np.array(bad, np.int32)), FR.MEMBERS, none, INVALID))
    lines.append(case_text(c, 2, none, INVALID))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == len(lines) and "MISMATCH" not in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr
