"""bench.py's plain run end to end (no --full): one GPU with --dump-outputs, and two ranks on the box's one GPU
(--rehearse-one-gpu, collectives over gloo), whose plain run still times the pipelined steps that are its headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--steps", "2", "--warmup", "1", "--scale", "0.12"]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + COMMON + list(extra), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_single_gpu_run_and_its_dump(tmp_path):
    d = tmp_path / "dump"
    one = _bench("--gpus", "1", "--dump-outputs", str(d))
    assert all(one.get(k) is not None for k in CONTRACT) and one["steps"] == 2 and one["n_gpus"] == 1
    assert one["higher_is_better"] is True and one["dtype"] == "int128+f64" and one["ms_per_step"] > 0
    assert "roofline" not in one and "cpu_baseline" not in one and "detail" not in one and "secondary" not in one
    f = {n: np.load(d / (n + ".npy")) for n in ("lsi_count", "lsi_pairs", "lsi_records", "lsi_pair_index",
                                                 "pip_point_index", "pip_closest_eids", "pip_face_ids")}
    assert all(a.dtype == np.float64 for a in f.values())
    n = one["intersections"]
    assert n > 1000 and f["lsi_count"].tolist() == [n] and f["lsi_pairs"].shape == (n, 2) and f["lsi_records"].shape == (n, 7)
    assert (f["lsi_records"][:, 4:6] == f["lsi_pairs"]).all() and (np.diff(f["lsi_pairs"][:, 0] * 2.0 ** 32 + f["lsi_pairs"][:, 1]) > 0).all()
    k = f["pip_point_index"].size
    assert k > 100000 and f["pip_closest_eids"].shape == f["pip_face_ids"].shape == (k,)
    assert (f["pip_closest_eids"] != 0xFFFFFFFF).sum() > k // 2
    # the same seeded inputs on a second run: the same results, file for file
    d2 = tmp_path / "dump2"
    _bench("--gpus", "1", "--dump-outputs", str(d2))
    assert all(np.array_equal(a, np.load(d2 / (name + ".npy"))) for name, a in f.items())


def test_plain_two_rank_run():
    one = _bench("--gpus", "1")
    two = _bench("--gpus", "2", "--rehearse-one-gpu", "--warmup", "5")
    assert all(two.get(k) is not None for k in CONTRACT) and two["n_gpus"] == 2
    assert two["intersections"] == one["intersections"] and "chain range x2" in two["config"]["sharding"]
    # (N > 1: once the schedule has settled the timed steps are the pipelined ones, and they are the line's ms_per_step)
    assert two["pipelined"] == two["config"]["schedule_settled_before_timing"]
    if two["pipelined"]:
        assert two["ms_per_step"] == two["ms_per_step_pipelined"]
