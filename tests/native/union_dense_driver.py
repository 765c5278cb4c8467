"""Driver of the stubbed-device builds for the dense union route (run by tests/test_union_dense_cpu.py with VQ_LIB=<host-stub or sanitizer
library>, VQ_STUB_NOOP_LAUNCH=1, VQ_STUB_DICT_SCAN=1 and a slab budget of 0 MB: one slab group per job): prefix leaves that match more than 4096
dictionary terms go through run_union_jobs' host side — list tables, groups, uploads, the launch calls, the read-back — over a "device" whose
launches do nothing, so every merged list comes back empty.  Prints one summary line; any sanitizer report aborts the process."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import veloci_amd  # noqa: E402
import widecorpus  # noqa: E402
from veloci_amd import _lib  # noqa: E402

assert "host_" in _lib.lib_path(), _lib.lib_path()
assert os.environ.get("VQ_STUB_NOOP_LAUNCH") == "1" and os.environ.get("VQ_STUB_DICT_SCAN") == "1"
data, terms = widecorpus.build(num_terms=3000, num_docs=100_000)
leaf = lambda t, **kw: {"search": dict({"path": "body", "terms": [t], "starts_with": True}, **kw)}
reqs = [{"search_req": leaf("zq"), "top": 10},                                     # 4097 lists
        {"search_req": leaf("z"), "top": 10},                                      # 8193
        {"search_req": leaf("z", boost=-2.0), "top": 10},                          # a job of its own
        # (every leaf here is wide: k_union's host side sizes its output by counts read back from the device, which a stubbed launch never wrote)
        {"search_req": {"and": {"queries": [leaf("zq"), leaf("z")]}}, "top": 10},
        {"search_req": {"or": {"queries": [leaf("z"), leaf("zq", boost=1.5)]}}, "top": 10}]
stats = {"searched": 0, "batches": 0, "dense_launches": 0}
for lo, hi in ((0, None), (25_000, 100_000), (0, 10)):  # unsharded, a doc-range shard, a shard of 10 docs
    idx = veloci_amd.Index(data, device=0, doc_lo=lo, doc_hi=hi)
    idx.profile_enable()
    for r in (reqs if hi is None else reqs[:3]):
        if hi is None:
            veloci_amd.search(r, idx)
        else:
            veloci_amd.PartialBatch(idx, [veloci_amd.Request(r)]).merge(None, 1, raise_on_error=True)
        stats["searched"] += 1
    if hi is None:
        assert len(veloci_amd.search_batch(reqs, idx)) == len(reqs)
        stats["batches"] += 1
    prof = idx.profile_json()["kernels"]
    names = ("k_union_dense_scatter", "k_union_dense_count", "k_union_dense_write")
    assert len({prof[k]["launches"] for k in names}) == 1, prof
    stats["dense_launches"] += prof[names[0]]["launches"]
    # nothing was scattered: every merged list is its 8 sentinel entries (64 B) behind the bytes of the slab and of the block offsets
    w = prof["k_union_dense_write"]
    assert w["layout_bytes"] - w["algorithmic_bytes"] == 4 * (w["algorithmic_bytes"] - 64 * w["queries"]) // (4 * 2048), (lo, hi, w)
    del idx
print("UNION_DENSE_DRIVER_OK " + json.dumps(stats))
