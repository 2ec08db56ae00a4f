"""The option surface of include/rayjoin_amd.h against the library: every option, report and debug knob the header's
option block lists is read from the header itself, so the document and rj_api.hip's option table cannot drift apart."""
import json
import os
import re
import subprocess
import sys

import pytest

from rayjoin_amd import _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rayjoin_amd.h")

# a valid value other than the default for every debug knob (the header lists the names, rj_api.hip the ranges)
DEBUG_VALUES = {"chunk_groups": 5, "group_lanes": 16, "max_blocks": 1000, "lsi_share_blocks": 300, "pip_share_blocks": 400,
                "stack_cap": 100, "walk_stack": 50, "strip_shift": 16, "lazy_columns_min": 12345, "run_cap": 32, "pack_solo": 40,
                "pack_spread": 7}
# the environment defaults: variable -> (option, value set, what a new handle must read)
ENV = {"RJ_LEAF_ORDER": ("leaf_order", "abc", 0), "RJ_LSI_SEGMENTS": ("lsi_segments", "3", 2),
       "RJ_WALK_POINTS": ("pip_walk_points", "4", 2), "RJ_POINTS_SPLIT": ("lsi_points_split", "1", 1),
       "RJ_LEAF_YSORT": ("leaf_ysort", "0", 0), "RJ_PIP_COLUMNS": ("pip_columns", "7", -1)}


def _header():
    """(settable options -> documented values, default first; report names expanded over their suffixes; debug knobs)"""
    src = open(HDR).read()
    start = src.index("/* ---- options ----")
    mid = src.index("rj_get_option reads any of these", start)
    end = src.index("*/", mid)
    settable = {m.group(1): [int(v) for v in m.group(2).split(" / ")]
                for m in re.finditer(r'^ \* "(\w+)"\s+(-?\d+(?: / -?\d+)*)\s{2,}', src[start:mid], re.M)}
    reports = []
    for name, suffix in re.findall(r'"([a-z_]+?)((?:0/1/2|0/1)?)"', src[mid:end]):
        if name not in settable:
            reports += [name + d for d in suffix.split("/")] if suffix else [name]
    dbg = src.index("/* Experiment knobs")
    debug = re.findall(r'"(\w+)"', src[dbg:src.index("*/", dbg)])
    return settable, reports, debug


def _refused(fn, *args):
    with pytest.raises(_capi.RayJoinError) as e:
        fn(*args)
    assert e.value.code == _capi.RJ_E_INVALID


def test_header_lists_the_option_surface():
    settable, reports, debug = _header()
    assert len(settable) == 14 and settable["pip_walk_points"] == [2, 1] and settable["own_stream"] == [1]
    assert "leaf_slots0" in reports and "leaf_slots1" in reports and "pip_schedule_us2" in reports and "comm_ranks" in reports
    assert set(debug) == set(DEBUG_VALUES)
    for var, (name, _, _) in ENV.items():
        assert name in settable and var in open(HDR).read()


def test_options_accept_their_documented_values_and_refuse_others():
    settable, _, _ = _header()
    h = _capi.Handle(0)
    try:
        for name, values in settable.items():
            if name == "own_stream":  # (set only: back to the handle's private stream)
                h.set_option(name, 1)
                _refused(h.get_option, name)
                continue
            for v in values[1:] + values[:1]:  # (ends on the default)
                h.set_option(name, v)
                assert h.get_option(name) == v, (name, v)
            if name == "stats":  # (any value but 0 is 1)
                h.set_option(name, 7)
                assert h.get_option(name) == 1
                h.set_option(name, values[0])
                continue
            for bad in {min(values) - 1, max(values) + 1}:
                _refused(h.set_option, name, bad)
                assert h.get_option(name) == values[0], (name, bad)
        for name, bad in (("pip_walk_points", 4), ("lsi_segments", 3), ("pip_walk", 3)):
            _refused(h.set_option, name, bad)
    finally:
        h.close()


def test_reports_and_debug_knobs_read_back():
    _, reports, debug = _header()
    h = _capi.Handle(0)
    try:
        for name in reports:
            h.get_option(name)
        for name in debug:
            h.set_debug_option(name, DEBUG_VALUES[name])
            assert h.get_debug_option(name) == DEBUG_VALUES[name], name
        for name, bad in (("group_lanes", 5), ("run_cap", 1), ("strip_shift", 14), ("max_blocks", 0)):
            _refused(h.set_debug_option, name, bad)
            assert h.get_debug_option(name) == DEBUG_VALUES[name], name
    finally:
        h.close()


def test_unknown_names_are_refused():
    h = _capi.Handle(0)
    try:
        for name in ("no_such_option", "chunk_groups", "leaf_slots"):
            _refused(h.set_option, name, 0)
        for name in ("no_such_option", "chunk_groups", "leaf_slots", "leaf_slots2", "leaf_slots01", "pip_schedule_us3",
                     "pip_rest_", "own_stream"):
            _refused(h.get_option, name)
        for name in ("no_such_option", "pip_walk", "query_key_strips"):
            _refused(h.set_debug_option, name, 0)
            _refused(h.get_debug_option, name)
    finally:
        h.close()


def test_environment_defaults():
    """One child process with the six variables set: atoi, then the option's own test; a refused value keeps the default."""
    code = ("import json\nfrom rayjoin_amd import _capi\nh = _capi.Handle(0)\n"
            "print(json.dumps({n: h.get_option(n) for n in %r}))\nh.close()\n" % [o for o, _, _ in ENV.values()])
    env = dict(os.environ, **{var: v for var, (_, v, _) in ENV.items()})
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {o: want for o, _, want in ENV.values()}
