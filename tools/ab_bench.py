#!/usr/bin/env python3
"""A/B of two builds of the library on ONE box (box-to-box spread is 2-3 %, more than most kernel changes): bench.py's
headline step, alternately with each .so (RAYJOIN_AMD_LIB), `rounds` times; prints the medians side by side.
usage (on the GPU box): tools/ab_bench.py rayjoin_amd/variants/librj_base.so rayjoin_amd/librayjoin_amd.so [rounds] [extra bench flags ...]
Flags of this tool, taken out of the extra ones: --env-a NAME=VALUE / --env-b NAME=VALUE set an environment variable for the runs
of one side only -- ONE library under two defaults, e.g. the same .so twice with --env-a RJ_POINTS_SPLIT=0 --env-b RJ_POINTS_SPLIT=1."""
import json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libs = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
extra = sys.argv[4:]
side_env = [{}, {}]
for i, flag in enumerate(("--env-a", "--env-b")):
    while flag in extra:
        k = extra.index(flag)
        name, value = extra[k + 1].split("=", 1)
        side_env[i][name] = value
        del extra[k:k + 2]
keys = {"step": lambda d: d["ms_per_step"], "pipelined": lambda d: d.get("ms_per_step_pipelined"),
        "dom_in_step": lambda d: d["roofline"]["kernel_ms"], "dom_alone": lambda d: d["roofline"].get("kernel_ms_alone"),
        "other_in_step": lambda d: d["roofline_other"]["kernel_ms"], "lsi_wall": lambda d: d["lsi_ms"], "pip_wall": lambda d: d["pip_ms"]}
res = [{k: [] for k in keys}, {k: [] for k in keys}]
detail = os.path.join(tempfile.mkdtemp(), "detail.json")  # (bench.py --full: stdout holds the compact line, the record goes here)
for r in range(rounds):
    for i, lib in enumerate(libs):
        env = dict(os.environ, RAYJOIN_AMD_LIB=lib, **side_env[i])
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "5", "--no-secondary", "--no-cpu-baseline", "--detail", detail] + extra,
                             env=env, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            print("run failed:", out.stderr[-2000:]); sys.exit(1)
        d = json.load(open(detail))["headline"]
        for k, f in keys.items():
            v = f(d)
            if v is not None:
                res[i][k].append(v)
        print("round %d %s: step %.4f pipelined %s %s in step %.4f" % (r, "AB"[i], d["ms_per_step"], d.get("ms_per_step_pipelined"), d["roofline"]["kernel"], d["roofline"]["kernel_ms"]), flush=True)
print(json.dumps({"A": libs[0], "B": libs[1], "env_A": side_env[0], "env_B": side_env[1], "rounds": rounds,
                  "median": {k: [round(statistics.median(res[i][k]), 4) if res[i][k] else None for i in (0, 1)] for k in keys}}))
