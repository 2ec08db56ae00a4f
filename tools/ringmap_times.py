"""rj_rings_map next to rj_map_rings on the same data (profiles/ringmap_times.txt): warm, the median of repeated calls, device
events on the handle's stream and the host clock round the call (which ends in its one synchronise).

  python tools/ringmap_times.py measure lattice|lakes        the two times, one JSON line
  rocprofv3 --kernel-trace --stats -d DIR -o rm --output-format csv -- python tools/ringmap_times.py profile lattice|lakes
  python tools/ringmap_times.py stages DIR/rm_kernel_trace.csv    the per-stage split of that trace (the calls of rj_rings_map
                                                                  are the dispatches behind the last kernel of rj_map_rings)

lattice: the rings of the merged intersection map of tests/test_overlay_map.py's lattice pair; lakes: the rings of
synth.ring_map(1 000 000, 10 000 000, seed=11, max_edges=20)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayjoin_amd import _capi, maps, ops, synth  # noqa: E402

mode, data = sys.argv[1], sys.argv[2]


def stages(path):
    import collections
    import csv
    import re
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[max(i for i, r in enumerate(rows) if "k_rg_" in r["Kernel_Name"]) + 1:]
    calls = sum(1 for r in rows if "k_rm_check" in r["Kernel_Name"])

    def stage(n):
        m = re.search(r"k_rm_\w+", n)
        if m:
            return m.group(0)
        short = re.sub(r"<.*", "", n).split("::")[-1]
        if "SegBefore" in n or "HalfBefore" in n:
            return ("sort1:" if "SegBefore" in n else "sort2/merge:") + short
        return ("scan Slots:" if "Slots" in n else "rocprim u32:") + short

    tot = collections.defaultdict(lambda: [0, 0])
    for r in rows:
        t = tot[stage(r["Kernel_Name"])]
        t[0] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        t[1] += 1
    allk = sum(v[0] for v in tot.values())
    print("calls", calls, "kernel time per call %.3f ms" % (allk / calls / 1e6), "launches per call %.0f" % (len(rows) / calls))
    for s, (d, c) in sorted(tot.items(), key=lambda kv: -kv[1][0]):
        print("  %-60s %9.1f us/call  %5.1f %%  %4.0f launches/call" % (s, d / calls / 1e3, 100.0 * d / allk, c / calls))


if mode == "stages":
    stages(data)
    sys.exit(0)
REPEAT = 9 if mode == "measure" else 3
out = {"data": data}


def timed(h, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        t = time.perf_counter()
        r = fn()
        t = time.perf_counter() - t
        e1.record(stream)
    e1.synchronize()
    return r, e0.elapsed_time(e1), 1e3 * t


if data == "lattice":
    from test_gpu_overlay_merge import DROP, MERGE, overlay_of, raw_map
    from test_overlay_map import pair
    gs, _ = pair("lattice")
    dctx, ov = overlay_of(maps.Context(gs).load(), None)
    h = ov.h
    om = raw_map(ov, None, DROP | MERGE)
    src = (om.xy, om.n_points, om.row_index, om.left, om.right, om.n_chains)
else:
    t = time.time()
    g = synth.ring_map(1_000_000, 10_000_000, seed=11, max_edges=20)
    ctx = maps.Context([g, None]).load()
    m = ctx.maps[0]
    out["generate_s"] = time.time() - t
    h = _capi.Handle(0)
    bufs = [h.alloc(16 * m.n_points).from_host(np.ascontiguousarray(m.pts, np.int64)), h.alloc(4 * (m.n_chains + 1)).from_host(m.row_index),
            h.alloc(4 * m.n_chains).from_host(m.left.astype(np.int32)), h.alloc(4 * m.n_chains).from_host(m.right.astype(np.int32))]
    src = (bufs[0], m.n_points, bufs[1], bufs[2], bufs[3], m.n_chains)
    ne = np.diff(m.row_index.astype(np.int64)) - 1
    out["source_edges_per_chain"] = [int(ne.min()), float(ne.mean()), int(ne.max())]

stream = torch.cuda.Stream()
h.set_stream(stream.cuda_stream)
out["source"] = dict(n_chains=int(src[5]), n_points=int(src[1]))
# rj_map_rings: sized once, then the filling call timed
r = ops.face_rings(h, *src)
out["rings"] = dict(r.counts)
caps_r = (r.n_rings, r.n_halves, r.n_points)
rb = (r.rings, r.ring_first, r.ring_half, r.ring_row, r.ring_xy)
ev, host = [], []
for k in range(3 + REPEAT):
    _, a, b = timed(h, stream, lambda: h.map_rings(*src, 0, caps_r, *rb))
    if k >= 3:
        ev.append(a)
        host.append(b)
out["map_rings_ms"] = dict(event_median=float(np.median(ev)), event_min=min(ev), event_max=max(ev), host_median=float(np.median(host)))
# rj_rings_map: the same
dm = r.Map(h)
out["map"] = dict(dm.counts)
caps_m = (dm.n_chains, dm.n_points)
args = (r.ring_row, r.ring_xy, r.n_points, r.rings, 32, r.n_rings, 0)
ev, host = [], []
for k in range(3 + REPEAT):
    _, a, b = timed(h, stream, lambda: h.rings_map(*args, caps_m, dm.xy, dm.row_index, dm.left, dm.right))
    if k >= 3:
        ev.append(a)
        host.append(b)
out["rings_map_ms"] = dict(event_median=float(np.median(ev)), event_min=min(ev), event_max=max(ev), host_median=float(np.median(host)))
out["rings_map_calls"] = 3 + REPEAT + 2
print(json.dumps(out))
