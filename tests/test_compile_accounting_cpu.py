"""What the query compiler accounts per kernel class, without a GPU: `layout_bytes` and `algorithmic_bytes` (Compiler::run and
compute_layout_bytes in compile.cpp) with the `launches` and `queries` they were summed over, as vq_profile_json reports them.  The launch log of
tests/test_launch_plan_cpu.py does not show these figures.  The two batches of tests/native/launch_plan_driver.py run over the stubbed device
layer with VQ_LAUNCH_PLAN_PROFILE set, a process per leg (the routing knobs are read once per process); every section's profile is compared with
tests/golden/compile_accounting.json.  That file was recorded with the same stub and driver on the commit BEFORE Compiler::run was cut into
phases (468f5e5), twice with identical outcome: it is the behaviour to keep, never to be regenerated from the code under test.  No field
differed between the two recordings.  Left out all the same: `ms` (a device time; the stub's events report 0.0) and `gathered_bytes` (counted by
the kernels, 0 under the stub), which say nothing about the compiler, and `scan`, a constant of the kernel class."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
DRIVER = os.path.join(HERE, "native", "launch_plan_driver.py")
GOLDEN = os.path.join(HERE, "golden", "compile_accounting.json")
STUB_LIB = os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so")

FIELDS = ("launches", "queries", "layout_bytes", "algorithmic_bytes")
PREPASS = {"VQ_LAUNCH_PLAN_BATCH": "prepass", "VQ_STUB_DICT_SCAN": "1"}
LEGS = [{}, {"VQ_PROBE_MIN_DOCS": "0"}, dict(PREPASS), dict(PREPASS, VQ_PROBE_MIN_DOCS="0")]
# knobs of the launch-plan legs that must not leak in from the caller's environment
DROP = {"VQ_PROBE_MIN_DOCS", "VQ_LAUNCH_PLAN_BATCH", "VQ_STUB_DICT_SCAN", "VQ_UNION_OR", "VQ_NO_UNION_COV", "VQ_NO_UNION", "VQ_NO_RICH", "VQ_NO_WIDE", "VQ_PROBE_NO_ARR",
        "VQ_NO_PROBE_OR", "VQ_FORCE_GENERIC"}


def leg_id(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items())) or "shipped defaults"


def accounting(lib, env, tmp_dir):
    """one run of the driver with profiling on -> per section {"section": name, "kernels": {kernel: {field: value for FIELDS}}}"""
    log_path, prof_path = os.path.join(str(tmp_dir), "launches.jsonl"), os.path.join(str(tmp_dir), "profile.jsonl")
    for p in (log_path, prof_path):
        if os.path.exists(p):
            os.remove(p)
    full = {k: v for k, v in os.environ.items() if k not in DROP}
    full.update(env, VQ_LIB=lib, VQ_STUB_NOOP_LAUNCH="1", VQ_HOST_THREADS="4", VQ_STUB_LAUNCH_LOG=log_path, VQ_LAUNCH_PLAN_PROFILE=prof_path)
    r = subprocess.run([sys.executable, DRIVER], capture_output=True, text=True, timeout=600, env=full)
    assert r.returncode == 0 and "LAUNCH_PLAN_DRIVER_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    out = []
    with open(prof_path) as f:
        for line in f:
            rec = json.loads(line)
            out.append({"section": rec["section"], "kernels": {name: {k: v[k] for k in FIELDS} for name, v in sorted(rec["profile"]["kernels"].items())}})
    return out


@pytest.fixture(scope="module")
def stub_lib():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return STUB_LIB


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_holds_bytes_for_every_scan_class(golden):
    """what the recording is worth: three sections per leg; with the probe threshold at 0 every scan class of the first batch has queries with
    non-zero layout and algorithmic bytes"""
    assert sorted(golden) == sorted(leg_id(e) for e in LEGS)
    assert all(len(sections) == 3 for sections in golden.values())
    for sec in golden[leg_id({"VQ_PROBE_MIN_DOCS": "0"})]:
        scans = {k: v for k, v in sec["kernels"].items() if k.startswith("k_scan_") or k == "k_tile_scan"}
        assert set(scans) == {"k_scan_simple<2>", "k_scan_simple<2> (AND)", "k_scan_simple<2,rich>", "k_scan_probe (AND / OR)", "k_scan_union", "k_scan_wide", "k_tile_scan"}, sorted(scans)
        for name, v in scans.items():
            assert v["queries"] > 0 and v["layout_bytes"] > 0 and v["algorithmic_bytes"] > 0, (name, v)


@pytest.mark.parametrize("env", LEGS, ids=leg_id)
def test_compile_accounting_matches_the_recorded_one(stub_lib, golden, env, tmp_path):
    got = accounting(stub_lib, env, tmp_path)
    want = golden[leg_id(env)]
    assert [s["section"] for s in got] == [s["section"] for s in want]
    for g, w in zip(got, want):
        assert sorted(g["kernels"]) == sorted(w["kernels"]), (g["section"], sorted(g["kernels"]), sorted(w["kernels"]))
        for name in w["kernels"]:
            assert g["kernels"][name] == w["kernels"][name], (g["section"], name, g["kernels"][name], w["kernels"][name])
