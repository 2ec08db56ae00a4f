"""bench.py's plain run and --dump-outputs, without a GPU: the dump is exact, in an order that does not depend on the
order the LSI queue was filled in, and within its size bound; the plain line carries the contract fields and nothing
that needs a run of its own."""
import importlib.util
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _queue(cap, rng):
    """a step's results as the device leaves them: pairs, their rj_xsect records (int64 x 6), closest eids, face ids"""
    pairs = torch.from_numpy(rng.integers(0, 2 ** 31, size=(cap, 2), dtype=np.int64).astype(np.int32))
    pairs[3, 0] = -1  # eid 0xFFFFFFFF: the sort key must not overflow
    p64 = pairs.to(torch.int64) & 0xFFFFFFFF
    rec = torch.zeros((cap, 6), dtype=torch.int64)
    rec[:, 0] = torch.arange(cap) * 7 - (1 << 46)
    rec[:, 1] = 1
    rec[:, 2] = (1 << 46) - 1 - torch.arange(cap)
    rec[:, 3] = 1
    rec[:, 4] = p64[:, 0] | (p64[:, 1] << 32)
    rec[:, 5] = 0xFFFFFFFF   # mid_point_polygon_id = -1
    closest = torch.from_numpy(rng.integers(-1, 1 << 24, size=6000).astype(np.int32))
    return pairs, rec, closest, closest * 3


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_exact_sorted_and_independent_of_queue_order(tmp_path):
    b = _bench_module()
    rng = np.random.default_rng(1)
    cap, n, n_pts = 900, 600, 5000
    pairs, rec, closest, faces = _queue(cap, rng)
    b.dump_outputs(str(tmp_path / "a"), torch, n, cap, pairs, rec, closest, faces, n_pts)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    pairs2, rec2 = pairs.clone(), rec.clone()
    pairs2[:n], rec2[:n] = pairs[:n][perm], rec[:n][perm]
    b.dump_outputs(str(tmp_path / "b"), torch, n, cap, pairs2, rec2, closest, faces, n_pts)
    a, bb = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"lsi_count", "lsi_pairs", "lsi_records", "lsi_pair_index", "pip_point_index", "pip_closest_eids", "pip_face_ids"}
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], bb[k]), k
    pr, r = a["lsi_pairs"], a["lsi_records"]
    assert a["lsi_count"].tolist() == [n] and pr.shape == (n, 2) and r.shape == (n, 7)
    assert (np.diff(pr[:, 0] * 2.0 ** 32 + pr[:, 1]) > 0).all() and pr.max() == 0xFFFFFFFF
    assert (r[:, 4:6] == pr).all() and (r[:, 1] == 1).all() and (r[:, 6] == -1).all()
    want = {(int(p[0]) & 0xFFFFFFFF, int(p[1]) & 0xFFFFFFFF): int(x) for p, x in zip(pairs[:n].tolist(), rec[:n, 0].tolist())}
    assert all(want[(int(p[0]), int(p[1]))] == int(x) for p, x in zip(pr, r[:, 0]))   # 47-bit coordinates, exact
    idx = a["pip_point_index"].astype(np.int64)
    assert np.array_equal(idx, np.arange(n_pts))
    c = closest[:n_pts].numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(a["pip_closest_eids"], c) and np.array_equal(a["pip_face_ids"], faces[:n_pts].numpy())


def test_dump_samples_large_outputs_with_a_fixed_seed(tmp_path):
    b = _bench_module()
    b.DUMP_MAX_PAIRS, b.DUMP_POINTS = 128, 1000
    rng = np.random.default_rng(3)
    pairs, rec, closest, faces = _queue(900, rng)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), torch, 800, 900, pairs, rec, closest, faces, 5000)
    a, bb = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], bb[k]) for k in a)
    assert a["lsi_pairs"].shape == (128, 2) and a["pip_closest_eids"].shape == (1000,)
    assert (np.diff(a["lsi_pair_index"]) > 0).all() and (np.diff(a["pip_point_index"]) > 0).all()


def test_dump_stays_under_64_mb():
    b = _bench_module()
    worst = 8 * (1 + (2 + 7 + 1) * b.DUMP_MAX_PAIRS + 3 * b.DUMP_POINTS)
    assert worst <= 64 << 20


def test_plain_line_is_the_headline_alone(capsys):
    """a plain run prints the compact line and writes no --detail file; --full is off by default"""
    b = _bench_module()
    out = {"metric": "LSI+PIP query throughput, A |><| B", "value": 2.0, "unit": "M query segments/s", "n_gpus": 1, "steps": 3,
           "warmup": 1, "ms_per_step": 0.5, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "int128+f64", "data": "synthetic", "config": {"workload": "w", "sharding": "single GPU"}, "intersections": 7}
    b.emit(out, [], None)
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 1
    h = json.loads(lines[0])
    assert {k: h[k] for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")} == \
        {k: out[k] for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")}
    assert "detail" not in h and "roofline" not in h and "cpu_baseline" not in h
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'ap.add_argument("--full", action="store_true"' in src and '"--dump-outputs"' in src


def _args(b, monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + list(argv))
    return b.parse()


def test_only_the_headline_writes_the_dump(monkeypatch, tmp_path):
    """--full --dump-outputs on the default workload: the four secondary pairs run after the headline and must not
    overwrite its files -- run_pairs hands the dump directory to the headline's call alone"""
    b = _bench_module()
    calls = []

    def fake(args, env, base, query, steps, warmup, headline, with_cpu, full=True, dump_dir=None):
        calls.append((base, query, headline, full, dump_dir))
        return {"metric": "x, %s |><| %s" % (base, query)}

    monkeypatch.setattr(b, "run_workload", fake)
    env = (torch, None, torch.device("cpu"), 1, 0, 0)
    d = str(tmp_path / "dump")
    out, sec = b.run_pairs(_args(b, monkeypatch, "--full", "--dump-outputs", d), env)
    assert calls[0] == ("USCounty", "BlockGroup", True, True, d)
    assert [c[:2] for c in calls[1:]] == list(b.SECONDARY) and len(sec) == len(b.SECONDARY)
    assert all(c[2] is False and c[4] is None for c in calls[1:])
    calls.clear()
    out, sec = b.run_pairs(_args(b, monkeypatch, "--dump-outputs", d), env)   # plain: the headline alone
    assert calls == [("USCounty", "BlockGroup", True, False, d)] and sec == []


def test_flags_of_full_say_so_in_a_plain_run(monkeypatch, capsys):
    b = _bench_module()
    _args(b, monkeypatch, "--detail", "somewhere.json", "--no-secondary")
    assert "--detail, --no-secondary act only with --full" in capsys.readouterr().err
    _args(b, monkeypatch, "--full", "--detail", "somewhere.json", "--no-secondary")
    _args(b, monkeypatch)
    assert capsys.readouterr().err == ""
