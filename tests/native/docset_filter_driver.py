"""Driver of tests/test_docset_filter_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: doc sets from a filter over the
stubbed device layer (tests/native/hip_stub_docset_filter.cpp answers the launcher with a host loop) — the filter-only compilation, the staged
program, the shared image tail, the length on a shard — against the numpy restatement of tests/countref.py and tests/docsetref.py, on the whole
index and on an unaligned shard, and the error paths."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
from veloci_amd import DocSet  # noqa: E402
import countcorpus as CC  # noqa: E402
import docsetfiltercases as FC  # noqa: E402
import docsetref  # noqa: E402


def main():
    Lib = veloci_amd.lib()
    L, _ = FC.corpus()
    data = CC.index_data(L)
    whole, shard = veloci_amd.Index(data), veloci_amd.Index(data, doc_lo=FC.SHARD[0], doc_hi=FC.SHARD[1])
    total = {"n": None, "calls": 0}

    def hook(arr):  # the sum over the shards: what numpy says the whole set holds
        assert arr.size == 1
        arr[0] = total["n"]
        total["calls"] += 1

    stats = {"sets": 0, "within": 0}
    cases = [c for c in FC.leaf_cases() if not c[0].startswith("prefix")] + FC.tree_cases()
    # every tree compiles as the filter of a request (what the device test relies on)
    for name, flt in FC.leaf_cases() + FC.tree_cases():
        r = veloci_amd.Request({"search_req": FC.leaf("all"), "filter": flt})
        rc = Lib.vq_debug_compile(whole.h, r.h)
        assert rc == (4 if name.startswith("prefix") else 0), (name, rc)  # (a prefix leaf waits for its dictionary scan, which this call does not run: no decline of the tree)
    for idx in (whole, shard):
        sharded = idx is shard
        # a shard without the hook declines, naming what it needs
        if sharded:
            try:
                DocSet.from_filter(idx, FC.leaf("d0"))
                raise AssertionError("a shard without an all-reduce hook made a set from a filter")
            except veloci_amd.VelociError as e:
                assert e.code == 4 and "vq_index_set_allreduce" in str(e), (e.code, str(e))
            idx.set_allreduce(hook)
        wants = []
        for name, flt in cases:
            want = FC.expected(flt)
            total["n"] = len(want)
            ds = DocSet.from_filter(idx, flt)
            docsetref.check(ds, want, FC.N, idx.doc_lo, idx.doc_hi)
            ds.close()
            wants.append(want)
            stats["sets"] += 1
        FC.assert_not_vacuous(wants, idx.doc_lo, idx.doc_hi)
        for name, ids in FC.within_cases():
            want = FC.expected(FC.WITHIN_FILTER, within=ids)
            total["n"] = len(np.unique(ids))
            within = DocSet(idx, ids) if not sharded else None
            if sharded:  # (vq_docset_create counts the whole array itself: no hook call)
                before = total["calls"]
                within = DocSet(idx, ids)
                assert total["calls"] == before
            total["n"] = len(want)
            ds = DocSet.from_filter(idx, FC.WITHIN_FILTER, within=within)
            within.close()  # the new set does not need it
            docsetref.check(ds, want, FC.N, idx.doc_lo, idx.doc_hi)
            # the result is an ordinary set: the `within` of another call
            again = FC.expected(FC.leaf("d5"), within=want)
            total["n"] = len(again)
            ds2 = DocSet.from_filter(idx, json.dumps(FC.leaf("d5")), within=ds)
            ds.close()
            docsetref.check(ds2, again, FC.N, idx.doc_lo, idx.doc_hi)
            ds2.close()
            stats["within"] += 1
    assert total["calls"] > 0
    # misuse: a set of another index, text that is no JSON, an unknown path (the search's own error), no tree at all
    other = DocSet(whole, [1, 2, 3])
    for bad, code, text in ((lambda: DocSet.from_filter(shard, FC.leaf("d0"), within=other), 6, "another index"),
                            (lambda: DocSet.from_filter(whole, '{"search": '), 7, "JsonError"),
                            (lambda: DocSet.from_filter(whole, {"search": {"path": "nofield", "terms": ["x"]}}), None, "nofield")):
        try:
            bad()
            raise AssertionError("accepted: " + text)
        except veloci_amd.VelociError as e:
            assert (code is None or e.code == code) and text in str(e), (e.code, str(e))
    try:
        veloci_amd.search({"search_req": FC.leaf("all"), "filter": {"search": {"path": "nofield", "terms": ["x"]}}}, whole)
        raise AssertionError("the search accepted an unknown path")
    except veloci_amd.VelociError as e:
        want_code, want_text = e.code, str(e)
    try:
        DocSet.from_filter(whole, {"search": {"path": "nofield", "terms": ["x"]}})
    except veloci_amd.VelociError as e:
        assert (e.code, str(e)) == (want_code, want_text), (e.code, str(e), want_code, want_text)
    print("DOCSET_FILTER_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
