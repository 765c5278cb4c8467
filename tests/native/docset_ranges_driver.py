"""Driver of tests/test_docset_ranges_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: the doc sets from numeric ranges over
the stubbed device layer (tests/native/hip_stub_docset_ranges.cpp answers the launchers with host loops) — parsing, column resolution, the move of
the bounds to key intervals, the routing, the passes over the clause table, the 1:n bitmaps, the sum over the shards and the error paths —
against numpy (tests/docsetrangecases.py), on a whole index and on an unaligned shard."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsetrangecases as RC  # noqa: E402


def main():
    whole = veloci_amd.Index(RC.index_data())
    shard = veloci_amd.Index(RC.index_data(*RC.SHARD), doc_lo=RC.SHARD[0], doc_hi=RC.SHARD[1])
    other = veloci_amd.Index(RC.index_data())
    bare = veloci_amd.Index(RC.index_data(*RC.SHARD), doc_lo=RC.SHARD[0], doc_hi=RC.SHARD[1])  # a shard without the hook
    RC.check_misuse(veloci_amd, whole, other, bare)
    state = {"calls": 0}
    shard.set_allreduce(RC.counting_hook(state))
    whole.set_allreduce(RC.counting_hook({"local": -1, "len": -1}))  # never called: an unsharded index needs no sum
    stats = {"cases": 0, "probe": 0}
    expect_calls = 0
    os.environ.pop("VQ_NO_RANGE_PROBE", None)
    for idx, (lo, hi) in ((whole, (0, RC.N)), (shard, RC.SHARD)):
        sets = {name: (None if ids is None else veloci_amd.DocSet(idx, ids)) for name, ids in RC.withins().items()}
        for case in RC.cases():
            route = RC.check_case(veloci_amd, idx, lo, hi, state, case, sets, os.environ)
            stats["probe"] += route
            stats["cases"] += 1
            expect_calls += (1 + route) if idx is shard else 0  # a probe-route case runs once more on the stream route
        # a range set as an operand of the algebra
        L, W = RC.clause_lists(), RC.withins()
        a, b = RC.expected(L["both"], None, lo, hi), RC.expected(L["1n"], None, lo, hi)
        for op, want in (("and", np.intersect1d(a, b)), ("or", np.union1d(a, b)), ("minus", np.setdiff1d(a, b))):
            state["local"], state["len"] = int(((a >= lo) & (a < hi)).sum()), int(a.size)
            da = veloci_amd.DocSet.from_range(idx, "full", gte=-100.0, lt=100.25)
            state["local"], state["len"] = int(((b >= lo) & (b < hi)).sum()), int(b.size)
            db = veloci_amd.DocSet.from_ranges(idx, L["1n"])
            state["local"], state["len"] = int(((want >= lo) & (want < hi)).sum()), int(want.size)
            got = veloci_amd.DocSet.combine(idx, op, [da, db])
            assert "error" not in state, state["error"]
            RC.docsetref.check(got, want, RC.N, lo, hi)
            assert got.range_route == -1 and da.range_route == 0
        assert W["none"] is None
    assert state["calls"] == expect_calls + 9, (state["calls"], expect_calls, stats)  # the shard alone: once per set made there
    stats["hook_calls"] = state["calls"]
    print("DOCSET_RANGES_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
