"""A step that is cut in two runs its chunks on two scan streams (step_scan_stream in shard_step.cpp), and on an index that answers alone the next
step's scans no longer wait for this step's finalize.  Steps of 512 requests (the smallest a step is cut in two at, VQ_SHARD_CHUNKS=2), four of them
driven as the benchmark drives them (step i + 1 begun before step i is ended), on a 262 144-doc corpus with the probe kernels on:
every step's num_hits, counts, ids and scores equal vq_search_batch_flat's of the same requests bit for bit, and equal what the same steps give
with every chunk on one stream (VQ_STEP_SCAN_STREAMS=1: the knob is read once, so that run is a child process, one for all cases).

Run as a program (`python test_gpu_step_scan_streams.py OUT.npz`) this file is that child: it drives every case and writes the outputs down."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 262_144
STEP = 512
STEPS = 4
STRIDE = 10
CASES = ("headline", "mix", "second_chunk_empty", "one_failing", "neighbours")
# operand kinds by density at this size: bitmap images (d*), 16-bit arrays (a*), a tile-packed cover (c), a plain id list (s)
DFS = {"d1": N // 4, "d2": N // 8, "d3": N // 10, "a1": N // 32, "a2": N // 50, "a3": N // 128, "c": N // 512, "s": 24}
MISSING = {"search_req": {"search": {"path": "nosuchfield", "terms": ["x"]}}, "top": 10}


def build_index():
    import veloci_amd
    from veloci_amd import synth
    spec = synth.SynthSpec(num_docs=N, num_terms=2000, triples=4, extra_probe_dfs=tuple(DFS.values()), background_terms=20, with_t2t=True, with_facets=True, with_boost=True,
                           with_phrase=True, cat_values=16, tag_values=64)
    data, meta = synth.generate(spec)
    return veloci_amd.Index(data, device=0), meta


def case_steps(case, meta):
    """-> STEPS lists of STEP requests"""
    from veloci_amd import synth
    t = dict(zip(DFS, meta.extra_probes))
    tris = [list(x) for x in meta.triples]
    A, O, S = synth.req_and, synth.req_or, synth.req_single
    # the headline's shape: a 3-term AND on the probe kernel; operands of every kind, so that the steps differ from each other
    ands = [A(x) for x in tris] + [A([t["c"], t["d1"], t["d2"]]), A([t["c"], t["d1"], t["a1"]]), A([t["c"], t["a1"], t["a2"]]), A([t["c"], t["d2"], t["d3"]])]
    mix = ands + [O(tris[0]), O([t["c"], t["d1"]]), O([t["a1"], t["a2"], t["s"]]), S(t["d1"]), S(t["s"]), S(t["c"]), A([t["s"], t["d1"]]),
                  O([t[k] for k in ("d1", "d2", "a1", "a2", "c", "s")]), synth.req_and_phrase_locality(tris[1]),
                  S(t["d2"], facets=[{"field": "cat"}]), A([t["c"], t["d1"]], facets=[{"field": "cat"}, {"field": "tags[]", "top": 5}]),
                  dict(O([t["d1"], t["a2"]]), filter={"or": {"queries": [{"search": {"path": "body", "terms": [t[k]]}} for k in ("d2", "a1")]}},
                       facets=[{"field": "cat"}, {"field": "tags[]", "top": 5}])]  # (the generic kernel)
    pool = ands if case in ("headline", "neighbours") else mix
    steps = [[pool[(i * 7 + s * 3 + i // len(pool)) % len(pool)] for i in range(STEP)] for s in range(STEPS)]
    if case == "second_chunk_empty":  # nothing of the step's second chunk compiles: no launch, ev_done never recorded
        steps[1] = steps[1][:STEP // 2] + [MISSING] * (STEP // 2)
        steps[3] = [MISSING] * (STEP // 2) + steps[3][STEP // 2:]  # (and once the first chunk)
    if case == "one_failing":  # its status rides along, nothing throws
        steps[0][5] = MISSING
        steps[2][STEP // 2 - 1] = MISSING
    return steps


def suggest_requests(meta):
    heads = sorted({x[:2] for x in meta.extra_probes + [y for tri in meta.triples for y in tri]})[:6]
    return [{"path": "body", "terms": [h], "starts_with": True, "top": 10} for h in heads]


def drive(idx, meta, case):
    """the case's steps, two in flight -> [(num_hits, counts, ids, scores, status)] per step; `neighbours`: a flat batch and a suggest batch are
    issued while step 1 is in flight and before step 2 begins -> {"flat": ..., "suggest": json}"""
    import veloci_amd
    from veloci_amd.dist import shard_step_begin, shard_step_end
    batches = [veloci_amd.RequestBatch([veloci_amd.Request(r) for r in reqs]) for reqs in case_steps(case, meta)]
    outs, extra, pending = [], {}, None
    for s, b in enumerate(batches):
        if case == "neighbours" and s == 2:  # between two steps: step 1 is in flight (a flat batch takes workspace 0, which a step of even number holds)
            extra["flat"] = veloci_amd.search_batch_flat(batches[3].split(4)[1], idx, stride=STRIDE)
            extra["suggest"] = json.dumps(veloci_amd.suggest_batch(suggest_requests(meta), idx))
        h = shard_step_begin(idx, b)
        if pending is not None:
            outs.append(shard_step_end(pending, STRIDE))
        pending = h
    outs.append(shard_step_end(pending, STRIDE))
    return outs, extra


def pack(store, case, outs, extra):
    for s, o in enumerate(outs):
        for name, a in zip(("num_hits", "counts", "ids", "scores", "status"), o):
            store["%s/%d/%s" % (case, s, name)] = a.view(np.uint32) if a.dtype == np.float32 else a
    if "flat" in extra:
        for name, a in zip(("num_hits", "counts", "ids", "scores", "status"), extra["flat"]):
            store["%s/flat/%s" % (case, name)] = a.view(np.uint32) if a.dtype == np.float32 else a
        store["%s/suggest" % case] = np.frombuffer(extra["suggest"].encode(), np.uint8)


def run_all():
    idx, meta = build_index()
    store = {}
    for case in CASES:
        pack(store, case, *drive(idx, meta, case))
    return idx, meta, store


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.setdefault("VQ_PROBE_MIN_DOCS", "0")
    assert os.environ.get("VQ_STEP_SCAN_STREAMS") == "1" and os.environ.get("VQ_SHARD_CHUNKS") == "2"
    np.savez(sys.argv[1], **run_all()[2])
    print("STEP_SCAN_STREAMS_CHILD_OK")
    sys.exit(0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(index, meta, this process's outputs on two scan streams, the child's on one, the flat reference per case and step) — computed once"""
    import veloci_amd
    assert os.environ.get("VQ_PROBE_MIN_DOCS") == "0" and os.environ.get("VQ_STEP_SCAN_STREAMS") in (None, "2")
    keep = os.environ.get("VQ_SHARD_CHUNKS")
    os.environ["VQ_SHARD_CHUNKS"] = "2"  # (read at every step)
    try:
        idx, meta, two = run_all()
    finally:
        if keep is None:
            del os.environ["VQ_SHARD_CHUNKS"]
        else:
            os.environ["VQ_SHARD_CHUNKS"] = keep
    out = str(tmp_path_factory.mktemp("one_stream") / "one.npz")
    env = dict(os.environ, VQ_STEP_SCAN_STREAMS="1", VQ_SHARD_CHUNKS="2", VQ_PROBE_MIN_DOCS="0")
    env.pop("VQ_STEP_FIN_WAIT", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "STEP_SCAN_STREAMS_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    one = dict(np.load(out))
    flat = {}
    for case in CASES:
        for s, reqs in enumerate(case_steps(case, meta)):
            o = veloci_amd.search_batch_flat(reqs, idx, stride=STRIDE)
            for name, a in zip(("num_hits", "counts", "ids", "scores", "status"), o):
                flat["%s/%d/%s" % (case, s, name)] = a.view(np.uint32) if a.dtype == np.float32 else a
    return idx, meta, two, one, flat


def same(case, two, other, what):
    keys = [k for k in two if k.startswith(case + "/") and k.split("/")[1].isdigit()]
    assert len(keys) == STEPS * 5
    for k in keys:
        assert k in other and two[k].dtype == other[k].dtype and np.array_equal(two[k], other[k]), (what, k, np.flatnonzero((two[k] != other[k]).reshape(len(two[k]), -1).any(axis=1))[:8])


@pytest.mark.parametrize("case", CASES)
def test_steps_on_two_scan_streams_equal_the_flat_batch_and_one_stream(runs, case):
    idx, meta, two, one, flat = runs
    same(case, two, flat, "against vq_search_batch_flat")
    same(case, two, one, "against VQ_STEP_SCAN_STREAMS=1")
    status = np.stack([two["%s/%d/status" % (case, s)] for s in range(STEPS)])
    hits = np.stack([two["%s/%d/num_hits" % (case, s)] for s in range(STEPS)])
    failing = np.zeros((STEPS, STEP), bool)
    if case == "second_chunk_empty":
        failing[1, STEP // 2:] = failing[3, :STEP // 2] = True
    if case == "one_failing":
        failing[0, 5] = failing[2, STEP // 2 - 1] = True
    assert np.array_equal(status != 0, failing), np.argwhere((status != 0) != failing)[:8]
    assert (hits[~failing] > 0).mean() > 0.5 and not hits[failing].any()  # (the steps did find something: a few of the ANDs are empty by design of the lists)
    # the steps differ from each other: a step that read its neighbour's workspace would show
    assert any(not np.array_equal(two["%s/0/ids" % case], two["%s/%d/ids" % (case, s)]) for s in range(1, STEPS))


def test_a_flat_batch_and_a_suggest_batch_between_two_steps(runs):
    """they run on the index's scan stream and on the pre-passes' stream while a step is in flight, the next one begins behind them: the same answers as on an idle index"""
    import veloci_amd
    idx, meta, two, one, flat = runs
    reqs = case_steps("neighbours", meta)[3][STEP // 4:STEP // 2]
    alone = veloci_amd.search_batch_flat(reqs, idx, stride=STRIDE)
    for name, a in zip(("num_hits", "counts", "ids", "scores", "status"), alone):
        a = a.view(np.uint32) if a.dtype == np.float32 else a
        assert np.array_equal(two["neighbours/flat/" + name], a) and np.array_equal(one["neighbours/flat/" + name], a), name
    assert not alone[4].any() and (alone[0] > 0).mean() > 0.5
    sug = json.dumps(veloci_amd.suggest_batch(suggest_requests(meta), idx))
    assert any(json.loads(sug)) and bytes(two["neighbours/suggest"]).decode() == sug and bytes(one["neighbours/suggest"]).decode() == sug
