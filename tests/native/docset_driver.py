"""Driver of tests/test_docset_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: the creation path of a doc set over the
stubbed device layer (tests/native/hip_stub_docset.cpp answers the launchers with host loops) — buffer sizes, the layout arithmetic, the shard
masking — against the numpy restatement of tests/docsetref.py, the error paths, and what the request compiler makes of an attached set."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsetref as R  # noqa: E402


def main():
    L = veloci_amd.lib()
    data = R.small_data()
    lists = R.id_lists()
    stats = {"sets": 0, "dense": 0, "tiled": 0}
    indexes = [veloci_amd.Index(data), veloci_amd.Index(data, doc_lo=R.SHARD[0], doc_hi=R.SHARD[1])]
    for idx in indexes:
        for name, ids in lists.items():
            ds = veloci_amd.DocSet(idx, ids)
            want = R.check(ds, ids, R.NUM_ANCHORS, idx.doc_lo, idx.doc_hi)
            stats["sets"] += 1
            stats["dense"] += want["bitmap"] is not None
            stats["tiled"] += want["tile_dir"] is not None
            if want["bitmap"] is not None and idx.doc_lo:  # no bit outside the shard; rank entries count from the bitmap base
                bits = np.unpackbits(ds.part(1).view(np.uint8), bitorder="little")
                docs = np.flatnonzero(bits) + want["base"]
                assert docs.min() >= idx.doc_lo and docs.max() < idx.doc_hi and want["base"] < idx.doc_lo
                assert ds.part(2)[(idx.doc_lo - want["base"]) // 512] == 0
            ds.close()
        # the same ids as a list, as int32, with a foreign id: refused, with the number of such ids in the message
        for bad in ([5, R.NUM_ANCHORS, 7, R.NUM_ANCHORS + 9], np.array([R.NUM_ANCHORS], np.uint32), [0xFFFFFFFF]):
            try:
                veloci_amd.DocSet(idx, bad)
                raise AssertionError("an id beyond the index's anchors was accepted")
            except veloci_amd.VelociError as e:
                n_bad = sum(1 for x in np.asarray(bad).tolist() if x >= R.NUM_ANCHORS)
                assert e.code == 6 and ("doc set: %d of the %d ids" % (n_bad, len(bad))) in str(e), (e.code, str(e))
        for bad in ([-1], [1 << 32], [1.5]):
            try:
                veloci_amd.DocSet(idx, bad)
                raise AssertionError("ids outside u32 were accepted")
            except ValueError:
                pass
    # the compiler: a request with a set is a request with a filter
    a, b = indexes
    req = {"search_req": {"search": {"path": "body", "terms": ["alpha"]}}}
    own = dict(req, filter={"search": {"path": "body", "terms": ["beta"]}})
    for spec in (req, own):
        r = veloci_amd.Request(spec)
        before = r.to_json()
        plain = L.vq_debug_compile(a.h, r.h)
        ds = veloci_amd.DocSet(a, [1, 2, 3])
        r.set_docset(ds)
        assert r.to_json() == before
        ds.close()  # the request keeps the set
        assert L.vq_debug_compile(a.h, r.h) == plain == 0, (L.vq_debug_compile(a.h, r.h), plain, L.vq_last_error())
        assert L.vq_debug_compile(b.h, r.h) == 6  # InvalidArgument: the set belongs to index a
        r.set_docset(None)
        assert L.vq_debug_compile(b.h, r.h) == 0
        stats["compiled"] = stats.get("compiled", 0) + 1
    # an empty set compiles too (a filter leaf without lists)
    r = veloci_amd.Request(req, docset=veloci_amd.DocSet(a, []))
    assert L.vq_debug_compile(a.h, r.h) == 0
    # a 3-term AND under a set asks for the count pre-pass, as under any filter (the operands' sizes inside a Set filter are not known statically)
    and3 = {"search_req": {"and": {"queries": [{"search": {"path": "body", "terms": [t]}} for t in ("alpha", "beta", "alpha")]}}}
    plain, under_set = veloci_amd.Request(and3), veloci_amd.Request(and3, docset=veloci_amd.DocSet(a, [1, 2]))
    assert L.vq_debug_compile(a.h, plain.h) == 0
    assert L.vq_debug_compile(a.h, under_set.h) == -2
    print("DOCSET_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
