#!/usr/bin/env python3
"""rj_face_points at FULL size (test infrastructure: not collected by pytest, run by hand on the GPU like
tests/neighbours_fullsize_check.py; profiles/face_points_fullsize.txt holds its output):

  --base NAME --query NAME [--scale S]   two stand-ins of rayjoin_amd.synth: the vertices of the query map are located in
                                         the base map (PIPLBVH.Query), and the face ids are summarised per face of the base
                                         map.  bench.py's pairs: USCounty x BlockGroup (29.7 M points), WaterBodiesLike x
                                         BlockGroup (2.44 M rings)

Three inputs per pair: the face ids in the order of the query (the points follow their chains: coherent), with the universe
of the base map's faces; the same without a universe; the same points fully shuffled (labels and values permuted together),
with the universe.  Each with and without values (the x of the points) and with and without RJ_FP_MEMBERS: one cold call,
then three warm ones -- the minimum of the three per stage (HIP events) and the counts.  Beside them two yardsticks:
what a Python user does today on the same data in the same process -- torch.bincount for the counts and index_add_ into an
int64 tensor for the sum, which WRAPS in int64 where this call's sum is exact in 128 bits -- as the minimum of three warm
runs between torch events; and the memory floor of the table pass, 4 n bytes of labels (+ 8 n of values) at the achievable
HBM rate of 6 300 GB/s.  Every result is verified on the host: the counts of all faces against np.bincount, the sums, min,
max and first of a sample of faces against Python ints, the members of the sample against np.nonzero."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--base", default="USCounty")
ap.add_argument("--query", default="BlockGroup")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--out", help="append the report to this file")
a = ap.parse_args()
STAGES = ("universe", "table", "records", "members", "all")
HBM_GBS = 6300.0
SAMPLE = 16
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_located = {}


def located(ids, universe):
    """-> the labels as unsigned keys, the faces' keys ascending, the face number of every point, whether it is a member,
    the points per face; computed once per input"""
    at = (id(ids), universe is None)
    if at not in _located:
        key = ids.view(np.uint32)
        names = universe.view(np.uint32) if universe is not None else np.unique(key[key != 0])
        slot = np.searchsorted(names, key)
        hit = (key != 0) & (slot < len(names)) & (names[np.minimum(slot, len(names) - 1)] == key) if len(names) else np.zeros(len(key), bool)
        _located[at] = (key, names, slot, hit, np.bincount(slot[hit], minlength=len(names)))
    return _located[at]


def verify(ids, x, universe, counts, rec, off, mem):
    """the device's output on the host: all counts, a sample of faces in full"""
    key, names, slot, hit, per_face = located(ids, universe)
    assert len(rec) == len(names) == counts["n_faces"] and np.array_equal(rec["label"].view(np.uint32), names)
    assert np.array_equal(rec["n_points"], per_face.astype(np.uint64))
    assert counts["n_members"] == int(hit.sum()) and counts["n_outside"] == int((key == 0).sum()) and counts["n_unmatched"] == len(key) - int(hit.sum()) - int((key == 0).sum())
    assert counts["n_runs"] == (1 + int((ids[1:] != ids[:-1]).sum()) if len(ids) else 0)
    if off is not None:
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(per_face)]).astype(np.uint64)) and len(mem) == counts["n_members"]
    rng = np.random.default_rng(5)
    picks = set(rng.choice(len(names), min(SAMPLE, len(names)), replace=False).tolist()) | {int(np.argmax(per_face))} if len(names) else set()
    for k in picks:
        mine = np.nonzero(hit & (slot == k))[0]
        r = rec[k]
        assert int(r["first"]) == (int(mine[0]) if len(mine) else 0xFFFFFFFF)
        if x is not None:
            vals = [int(v) for v in x[mine]]
            assert (int(r["sum_hi"]) << 64) + int(r["sum_lo"]) == sum(vals)
            assert (int(r["min"]), int(r["max"])) == ((min(vals), max(vals)) if vals else (2 ** 63 - 1, -2 ** 63))
        else:
            assert (int(r["sum_lo"]), int(r["sum_hi"]), int(r["min"]), int(r["max"])) == (0, 0, 2 ** 63 - 1, -2 ** 63)
        if off is not None:
            assert np.array_equal(mem[int(off[k]):int(off[k + 1])], mine.astype(np.uint32))
    return len(picks)


def run(h, what, labels_dev, n, values_dev, stride, universe_dev, n_universe, ids, x, universe):
    """every combination of values and members on one input -> {(values, members): the stage times}"""
    out = {}
    for with_values in (False, True):
        for members in (False, True):
            flags = _capi.RJ_FP_MEMBERS if members else 0
            kw = dict(value_dev=values_dev if with_values else None, value_stride=stride, face_label_dev=universe_dev, n_face_labels=n_universe, flags=flags)
            try:
                c = h.face_points(labels_dev, n, (0, 0), **kw)
            except _capi.FacePointsOverflow as e:
                c = e.counts
            caps = (c["n_faces"], c["n_members"] if members else 0)
            bufs = [h.alloc(48 * max(1, caps[0])), h.alloc(8 * (caps[0] + 1)), h.alloc(4 * max(1, caps[1]))]
            best, walls = None, []
            for k in range(4):
                t0 = time.perf_counter()
                counts = h.face_points(labels_dev, n, caps, faces_dev=bufs[0], offsets_dev=bufs[1], members_dev=bufs[2], **kw)
                walls.append((time.perf_counter() - t0) * 1e3)
                ms = [h.get_option("face_points_last_us%d" % s) / 1000.0 for s in range(5)]
                if k:
                    best = ms if best is None else [min(p, q) for p, q in zip(best, ms)]
            rec = bufs[0].to_host(_capi.FP_FACE_DTYPE, caps[0])
            off, mem = (bufs[1].to_host(np.uint64, caps[0] + 1), bufs[2].to_host(np.uint32, caps[1])) if members else (None, None)
            t0 = time.perf_counter()
            checked = verify(ids, x if with_values else None, universe, counts, rec, off, mem)
            floor = (4 + (8 if with_values else 0)) * n / (HBM_GBS * 1e9) * 1e3
            say("  %s, %s, %s" % (what, "values" if with_values else "no values", "RJ_FP_MEMBERS" if members else "no members"))
            say("    %s" % counts)
            say("    first call %.3f ms wall; three warm calls %s ms wall" % (walls[0], ", ".join("%.3f" % w for w in walls[1:])))
            say("    the minimum of three warm calls per stage: ms  " + "  ".join("%s %.3f" % (s, v) for s, v in zip(STAGES, best)))
            say("    the table pass against its memory floor (%d n bytes at %.0f GB/s): %.3f ms to %.3f ms (%.1f x)"
                % (12 if with_values else 4, HBM_GBS, best[1], floor, best[1] / floor if floor else 0.0))
            say("    equal to numpy on the host (%.1f s): the counts of all %d faces, %d faces in full" % (time.perf_counter() - t0, caps[0], checked))
            out[(with_values, members)] = best
            for b in bufs:
                b.free()
    return out


def torch_yardstick(what, ids, x, n_bins, ours):
    """torch.bincount and index_add_ on the same data in the same process: the minimum of three warm runs"""
    import torch
    dev = torch.device("cuda:0")
    t_ids, t_x = torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev)
    if int(ids.min()) < 0:
        say("  the torch yardstick on %s: not run -- torch.bincount takes no negative label" % what)
        return

    def timed(fn):
        best = None
        for k in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            if k:
                best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
        return best, r
    t_count, cnt = timed(lambda: torch.bincount(t_ids, minlength=n_bins))
    t_sum, tot = timed(lambda: torch.zeros(n_bins, dtype=torch.int64, device=dev).index_add_(0, t_ids, t_x))  # (an int32 index, as the ids are)
    want = np.bincount(ids, minlength=n_bins)
    assert np.array_equal(cnt.cpu().numpy(), want)
    say("  the torch yardstick on %s: torch.bincount %.3f ms; index_add_ of an int64 sum %.3f ms (that sum wraps in int64; no min, max, first, no empty"
        " faces by label, labels as array indices only); together %.3f ms" % (what, t_count, t_sum, t_count + t_sum))
    say("    against it: rj_face_points without values, all stages %.3f ms to bincount's %.3f ms (%.2f x); with values %.3f ms to bincount + index_add_'s"
        " %.3f ms (%.2f x)" % (ours[(False, False)][4], t_count, ours[(False, False)][4] / t_count, ours[(True, False)][4], t_count + t_sum,
                               ours[(True, False)][4] / (t_count + t_sum)))
    del t_ids, t_x, cnt, tot
    torch.cuda.empty_cache()


if not a.no_torch:  # (torch opens the device first, as in bench.py: behind the library's own first call it finds none)
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
ctx = maps.Context([synth.standin(a.base, a.scale), synth.standin(a.query, a.scale)]).load()
dctx = ops.DeviceContext(ctx).LoadToDevice()
h = dctx.handle
dctx.BuildIndex(0)
pip = ops.PIPLBVH(dctx)
n = ctx.maps[1].n_points
pip.Init(n)
pip.Query(1)
ids = pip.get_face_ids()
pts = np.ascontiguousarray(ctx.maps[1].pts, np.int64).reshape(-1, 2)
x = np.ascontiguousarray(pts[:, 0])
sides = np.concatenate([np.asarray(ctx.maps[0].left), np.asarray(ctx.maps[0].right)]).astype(np.int32).view(np.uint32)
universe = np.unique(sides[sides != 0]).view(np.int32)
u_dev = h.alloc(4 * max(1, len(universe))).from_host(universe)
say("%s x %s%s: %d points located in a base map of %d faces" % (a.base, a.query, "" if a.scale == 1.0 else " at scale %g" % a.scale, n, len(universe)))
ours = run(h, "query order, universe", pip.faces, n, h.map_points_dev(1), 2, u_dev, len(universe), ids, x, universe)
if not a.no_torch:
    torch_yardstick("the query order", ids, x, int(universe.max()) + 1, ours)
run(h, "query order, no universe", pip.faces, n, h.map_points_dev(1), 2, None, 0, ids, x, None)
perm = np.random.default_rng(11).permutation(n)
ids_s, x_s = np.ascontiguousarray(ids[perm]), np.ascontiguousarray(x[perm])
l_dev, v_dev = h.alloc(4 * max(1, n)).from_host(ids_s), h.alloc(8 * max(1, n)).from_host(x_s)
ours = run(h, "fully shuffled, universe", l_dev, n, v_dev, 1, u_dev, len(universe), ids_s, x_s, universe)
if not a.no_torch:
    torch_yardstick("the shuffled points", ids_s, x_s, int(universe.max()) + 1, ours)
for b in (u_dev, l_dev, v_dev):
    b.free()
dctx.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
