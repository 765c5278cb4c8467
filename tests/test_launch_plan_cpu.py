"""The launch plan without a GPU: which scan kernel every query of a batch goes to, with which tables and launch parameters, in which order
(CompiledQuery::kclass; plan_layout, pack_upload and launch_scans behind run_partial in exec.cpp).  The host side runs over the stubbed device layer, whose launchers
write down what they are given (tests/native/hip_stub.cpp, VQ_STUB_LAUNCH_LOG; tests/native/launch_plan_driver.py); the records are compared
with tests/golden/launch_plan.json.  That file was recorded with the same stub and driver on the commit BEFORE routing moved into one
function (3ee56ad), twice with identical outcome — it is the behaviour to keep, never to be regenerated from the code under test.
The legs of the second batch (PREPASS_LEGS: the pre-pass loop of compile_batch) were recorded in the same way on the commit before run_partial
was split into phases (ea9e1d2)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
DRIVER = os.path.join(HERE, "native", "launch_plan_driver.py")
GOLDEN = os.path.join(HERE, "golden", "launch_plan.json")
STUB_LIB = os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so")

# The routing knobs are read once per process: every leg is a process of its own.  The corpus (262144 docs) lies below the shipped probe
# threshold of 40 M docs, so the knobs that shape the probe routes are also run with the threshold at 0, where those routes are taken.
KNOBS = [{"VQ_UNION_OR": "1", "VQ_NO_UNION_COV": "1"}, {"VQ_NO_UNION": "1"}, {"VQ_NO_RICH": "1"}, {"VQ_NO_WIDE": "1"}, {"VQ_PROBE_NO_ARR": "1"}, {"VQ_NO_PROBE_OR": "1"}]
LEGS = [{"VQ_PROBE_MIN_DOCS": "0"}, {}] + KNOBS[:2] + [{"VQ_FORCE_GENERIC": "1"}] + KNOBS[2:] + [dict(k, VQ_PROBE_MIN_DOCS="0") for k in KNOBS]
# The driver's second batch, which goes round the pre-pass loop (dictionary scan, union job, count pre-pass, the compilations between them)
PREPASS = {"VQ_LAUNCH_PLAN_BATCH": "prepass", "VQ_STUB_DICT_SCAN": "1"}
PREPASS_LEGS = [dict(PREPASS), dict(PREPASS, VQ_PROBE_MIN_DOCS="0")]


def leg_id(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items())) or "shipped defaults"


def record(lib, env, log_path):
    """one run of the driver -> its records (dicts, in launch order)"""
    if os.path.exists(log_path):
        os.remove(log_path)
    drop = {k for leg in LEGS + PREPASS_LEGS for k in leg}
    full = {k: v for k, v in os.environ.items() if k not in drop}
    full.update(env, VQ_LIB=lib, VQ_STUB_NOOP_LAUNCH="1", VQ_HOST_THREADS="4", VQ_STUB_LAUNCH_LOG=str(log_path))
    r = subprocess.run([sys.executable, DRIVER], capture_output=True, text=True, timeout=600, env=full)
    assert r.returncode == 0 and "LAUNCH_PLAN_DRIVER_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    with open(log_path) as f:
        return [json.loads(line) for line in f]


@pytest.fixture(scope="module")
def stub_lib():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return STUB_LIB


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_batch_reaches_every_scan_class(golden):
    """what the recording is worth: with the probe threshold at 0 every scan launcher but k_scan_leaf_f32 occurs, every probe shape included"""
    recs = golden[leg_id({"VQ_PROBE_MIN_DOCS": "0"})]
    assert {r["launch"] for r in recs if "launch" in r} >= {"k_scan_simple", "k_scan_probe", "k_scan_union", "k_scan_wide", "k_tile_scan", "k_merge_spans", "k_finalize", "k_facet_select"}
    assert {r["args"][0] for r in recs if r.get("launch") == "k_scan_probe"} == set(range(9))
    assert {tuple(r["args"][:1]) for r in recs if r.get("launch") == "k_scan_simple"} == {(0,), (1,)}  # plain and rich
    assert sum("section" in r for r in recs) == 3  # unsharded, two shards
    assert sorted(golden) == sorted(leg_id(e) for e in LEGS + PREPASS_LEGS)


@pytest.mark.parametrize("env", PREPASS_LEGS, ids=leg_id)
def test_the_prepass_batch_goes_round_the_prepass_loop(golden, env):
    """what the second recording is worth: in each of its three sections a dictionary scan, a union job and a count pre-pass (k_tile_scan with
    the fixed cand_cap of 256) come before the first scan launch, and the scans serve all five requests"""
    recs = golden[leg_id(env)]
    starts = [i for i, r in enumerate(recs) if "section" in r]
    assert len(starts) == 3  # unsharded, two shards
    for b, e in zip(starts, starts[1:] + [len(recs)]):
        launches = recs[b + 1:e]
        first_scan = next(i for i, r in enumerate(launches) if r["launch"].startswith("k_scan_") or (r["launch"] == "k_tile_scan" and r["args"][4] != 256))
        before = launches[:first_scan]
        assert {"k_dict_scan", "k_union"} <= {r["launch"] for r in before}
        assert any(r["launch"] == "k_tile_scan" and r["args"][4] == 256 for r in before)
        merge = next(i for i, r in enumerate(launches) if r["launch"] == "k_merge_spans")
        assert merge > first_scan and launches[merge]["args"] == [5]
        assert sorted(q for r in launches[first_scan:merge] for q in r["qmap"]) == list(range(5))


@pytest.mark.parametrize("env", LEGS + PREPASS_LEGS, ids=leg_id)
def test_launch_plan_matches_the_recorded_one(stub_lib, golden, env, tmp_path):
    got = record(stub_lib, env, tmp_path / "launches.jsonl")
    want = golden[leg_id(env)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want), (len(got), len(want), got[len(want):], want[len(got):])
