"""The second scan stream of a step changes no launch: over the stubbed device layer (tests/native/hip_stub.cpp, whose launchers write down what they
are given and ignore the stream) the launch log of steps that are cut in two — launcher calls, their order, their arguments, span and query
tables — is the same with every chunk on one stream (VQ_STEP_SCAN_STREAMS=1) and with the shipped default, and the recorded launch plan
(tests/golden/launch_plan.json) is met with the knob either way.

Run as a program this file is the driver of one such run (the knob is read once per process)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import veloci_amd
    from veloci_amd import _lib, synth
    from veloci_amd.dist import shard_step_begin, shard_step_end
    import test_gpu_step_scan_streams as G

    assert "host_" in _lib.lib_path() and os.environ.get("VQ_STUB_NOOP_LAUNCH") == "1" and os.environ.get("VQ_SHARD_CHUNKS") == "2"
    spec = synth.SynthSpec(num_docs=G.N, num_terms=2000, triples=4, extra_probe_dfs=tuple(G.DFS.values()), background_terms=0, with_t2t=True, with_facets=True, with_boost=True,
                           with_phrase=True, cat_values=16, tag_values=64)
    data, meta = synth.generate(spec, device="cpu")
    idx = veloci_amd.Index(data, device=0)
    failing = 0
    for case in ("mix", "second_chunk_empty"):
        with open(os.environ["VQ_STUB_LAUNCH_LOG"], "a") as f:
            f.write(json.dumps({"section": case}) + "\n")
        pending = None
        for reqs in G.case_steps(case, meta)[:3]:  # two steps in flight, as the benchmark drives them
            h = shard_step_begin(idx, veloci_amd.RequestBatch([veloci_amd.Request(r) for r in reqs]))
            if pending is not None:
                failing += int((shard_step_end(pending, G.STRIDE)[4] != 0).sum())
            pending = h
        failing += int((shard_step_end(pending, G.STRIDE)[4] != 0).sum())
    print("STEP_STREAMS_DRIVER_OK " + json.dumps({"failing": failing}))
    sys.exit(0)

from test_launch_plan_cpu import LEGS, golden, leg_id, record, stub_lib  # noqa: E402,F401  (the host-stub build, the recorded plan and how a leg is run)


def step_log(lib, knob, path):
    env = {k: v for k, v in os.environ.items() if k not in ("VQ_STEP_SCAN_STREAMS", "VQ_STEP_FIN_WAIT")}
    env.update(knob, VQ_LIB=lib, VQ_STUB_NOOP_LAUNCH="1", VQ_HOST_THREADS="4", VQ_STUB_LAUNCH_LOG=str(path), VQ_SHARD_CHUNKS="2", VQ_PROBE_MIN_DOCS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "STEP_STREAMS_DRIVER_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert json.loads(r.stdout.split("STEP_STREAMS_DRIVER_OK ")[1])["failing"] == 256
    with open(path) as f:
        return [json.loads(line) for line in f]


def test_the_launch_log_of_two_chunk_steps_does_not_depend_on_the_knob(stub_lib, tmp_path):
    two = step_log(stub_lib, {}, tmp_path / "two.jsonl")
    one = step_log(stub_lib, {"VQ_STEP_SCAN_STREAMS": "1"}, tmp_path / "one.jsonl")
    for i, (a, b) in enumerate(zip(two, one)):
        assert a == b, (i, a, b)
    assert len(two) == len(one)
    names = [r.get("launch") for r in two]
    # what the log is worth: 3 steps of 2 chunks and 3 steps of which one has an empty second chunk — a span merge and a finalize per chunk that
    # compiled, several scan kernels in front of a chunk's merge
    assert names.count("k_merge_spans") == names.count("k_finalize") and names.count("k_merge_spans") >= 6 + 5
    assert {"k_scan_probe", "k_scan_simple", "k_tile_scan", "k_facet_select"} <= set(names)
    assert names.index("k_merge_spans") > 2


@pytest.mark.parametrize("knob", [{}, {"VQ_STEP_SCAN_STREAMS": "1"}], ids=["two scan streams", "VQ_STEP_SCAN_STREAMS=1"])
def test_the_recorded_launch_plan_is_met_with_the_knob_either_way(stub_lib, golden, knob, tmp_path):
    leg = LEGS[0]
    got = record(stub_lib, dict(leg, **knob), tmp_path / "launches.jsonl")
    want = golden[leg_id(leg)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)
