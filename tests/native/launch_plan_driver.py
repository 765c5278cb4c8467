"""Driver of the host-stub build for the launch plan (run by tests/test_launch_plan_cpu.py with VQ_LIB=<host-stub library>, VQ_STUB_NOOP_LAUNCH=1 and
VQ_STUB_LAUNCH_LOG=<file>): one batch that reaches every scan class — on an unsharded index and on the two halves of a two-shard one — goes
through compile, routing, table packing and the launch calls over a "device" whose launches do nothing but write down what they were given
(tests/native/hip_stub.cpp).  The routing knobs are read once per process, so every environment leg is a run of its own.
With VQ_LAUNCH_PLAN_BATCH=prepass (and VQ_STUB_DICT_SCAN=1: the stub answers prefix probes with a plain loop) a second batch runs instead, on the
same corpus: requests that go round the pre-pass loop of compile_batch (exec.cpp; the runners it calls are in prepass.cpp) — dictionary scan, union job, count pre-pass — beside plain
ones that are compiled once.
With VQ_LAUNCH_PLAN_PROFILE=<file> (tests/test_compile_accounting_cpu.py) profiling is on, and every section's profile_json() is appended to
that file: what the compiler accounted per kernel class, which the launch log does not show."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))

import veloci_amd  # noqa: E402
from veloci_amd import _lib, synth  # noqa: E402

assert "host_" in _lib.lib_path(), _lib.lib_path()
assert os.environ.get("VQ_STUB_NOOP_LAUNCH") == "1"
LOG = os.environ["VQ_STUB_LAUNCH_LOG"]

N = 262_144  # two shards of 131072 docs: the pure routes need 65536
# operand kinds by density (index.cpp): a bitmap image from 1/64, a 16-bit array below 1/16, a tile-packed cover image from 1/4096, else a plain id list
DFS = {"d1": N // 4, "d2": N // 8, "d3": N // 10, "a1": N // 32, "a2": N // 50, "a3": N // 128, "c": N // 512, "s": 24}
spec = synth.SynthSpec(num_docs=N, num_terms=2000, triples=1, extra_probe_dfs=tuple(DFS.values()), background_terms=0, with_t2t=True, with_facets=True, with_boost=True,
                       with_phrase=True, cat_values=16, tag_values=64)


def requests(meta):
    t = dict(zip(DFS, meta.extra_probes))
    tri = list(meta.triples[0])
    A, O, S = synth.req_and, synth.req_or, synth.req_single
    reqs = [S(t["d1"]), S(t["s"]), S(t["c"], top=40),
            A([t["c"], t["d1"]]), A([t["c"], t["a1"]]),                                                      # kProbeAnd1
            A([t["c"], t["d1"], t["d2"]]), A([t["c"], t["d1"], t["a1"]]), A([t["c"], t["a1"], t["a2"]]),      # kProbeAnd2A0..2
            A([t["c"], t["d1"], t["d2"], t["d3"]]), A([t["c"], t["d1"], t["d2"], t["a1"]]),                   # kProbeAnd3A0..3
            A([t["c"], t["d1"], t["a1"], t["a2"]]), A([t["c"], t["a1"], t["a2"], t["a3"]], top=100),
            A([t["s"], t["d1"]]), A([t["s"], t["a1"], t["d2"]]), A(tri),                                      # an id-list cover: k_scan_simple (AND)
            O([t["c"], t["d1"]]), O([t["c"], t["d1"], t["d2"]]), O([t["s"], t["d1"]]), O([t["a1"], t["a2"], t["s"]]), O(tri, top=50),
            synth.req_and_phrase_locality(tri),                                                               # rich
            O([t[k] for k in ("d1", "d2", "a1", "a2", "c", "s")]),                                            # wide
            A([t[k] for k in DFS]),
            dict(O([t["d1"], t["a2"]]), filter={"or": {"queries": [{"search": {"path": "body", "terms": [t[k]]}} for k in ("d2", "a1")]}},
                 facets=[{"field": "cat"}, {"field": "tags[]", "top": 5}]),                                   # k_tile_scan
            S(t["d2"], facets=[{"field": "cat"}]),
            {"search_req": {"search": {"path": "nosuchfield", "terms": ["x"]}}, "top": 10}]                   # declined
    return reqs


def prepass_requests(meta):
    """a prefix leaf over every term of the dictionary (more than VQ_UNION_MIN of them have postings: a union job), alone and inside an AND; an AND
    of ORs whose summation order follows run-time result sizes (count pre-pass); two plain requests that never come back for a second pass"""
    t = dict(zip(DFS, meta.extra_probes))
    tri = list(meta.triples[0])
    leaf = lambda term, **more: {"search": dict({"path": "body", "terms": [term]}, **more)}
    either = lambda *terms: {"or": {"queries": [leaf(x) for x in terms]}}
    prefix = leaf("", starts_with=True)
    return [synth.req_single(t["d1"]),
            {"search_req": prefix, "top": 10},
            {"search_req": {"and": {"queries": [prefix, leaf(t["d1"])]}}, "top": 10},
            {"search_req": {"and": {"queries": [either(tri[0], tri[1]), either(t["d2"], t["a1"]), leaf(t["a3"])]}}, "top": 10},
            synth.req_and([t["c"], t["d1"]])]


def mark(what):
    with open(LOG, "a") as f:
        f.write(json.dumps({"section": what}) + "\n")


declined = []
data, meta = synth.generate(spec, device="cpu")
PREPASS = os.environ.get("VQ_LAUNCH_PLAN_BATCH") == "prepass"
PROFILE = os.environ.get("VQ_LAUNCH_PLAN_PROFILE")
if PREPASS:
    assert os.environ.get("VQ_STUB_DICT_SCAN") == "1"
reqs = prepass_requests(meta) if PREPASS else requests(meta)
for lo, hi in ((0, N), (0, N // 2), (N // 2, N)):
    idx = veloci_amd.Index(data, device=0, doc_lo=lo, doc_hi=hi)
    mark("docs [%d, %d)" % (lo, hi))
    if PROFILE:
        idx.profile_enable()
    if PREPASS and hi - lo != N:
        idx.set_allreduce(lambda values: None)  # the sums over the shards: the other shard adds nothing
    if hi - lo == N:
        res = veloci_amd.search_batch(reqs, idx, raise_on_error=False)
    else:
        res = veloci_amd.PartialBatch(idx, [veloci_amd.Request(r) for r in reqs]).merge(None, 1, raise_on_error=False)
    declined.append([i for i, r in enumerate(res) if isinstance(r, Exception)])
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(json.dumps({"section": "docs [%d, %d)" % (lo, hi), "profile": idx.profile_json()}) + "\n")
    del idx
assert all(d == ([] if PREPASS else [len(reqs) - 1]) for d in declined), declined
print("LAUNCH_PLAN_DRIVER_OK " + json.dumps({"requests": len(reqs), "declined": declined}))
