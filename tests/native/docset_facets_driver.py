"""Driver of tests/test_docset_facets_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: the facet counts of a doc set over
the stubbed device layer (tests/native/hip_stub_docset_facets.cpp answers the launchers with host loops) — field resolution, the layout of the
call's device area, the counting mode per facet, the device / host ranking split, the sum over the shards, the rendering and the error paths —
against numpy (tests/docsetfacetcases.py), on a whole index and on an unaligned shard."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsetfacetcases as FC  # noqa: E402


def main():
    whole = veloci_amd.Index(FC.index_data())
    shard = veloci_amd.Index(FC.index_data(*FC.SHARD), doc_lo=FC.SHARD[0], doc_hi=FC.SHARD[1])
    other = veloci_amd.Index(FC.index_data())
    FC.check_misuse(veloci_amd, whole, other, shard)
    names = list(FC.id_sets()) + ["~" + FC.COMPLEMENT_OF]
    stats = {"pairs": 0, "entries": 0}
    state = {"calls": 0}
    shard.set_allreduce(FC.summing_hook(state, *FC.SHARD))
    whole.set_allreduce(FC.summing_hook({"len": -1}, 0, FC.N))  # never called: an unsharded index needs no sum
    for idx, (lo, hi) in ((whole, (0, FC.N)), (shard, FC.SHARD)):
        before = state["calls"]
        stats["pairs"] += FC.check_histograms(veloci_amd, idx, lo, hi, state, names, os.environ)
        stats["entries"] += FC.check_tops(veloci_amd, idx, state)
        if idx is whole:
            assert state["calls"] == before, state
    # the shard: one call of the hook per facet call on a set that is not empty (2 per pair, len(TOPS) + 1 of the tops), one per complement
    non_empty = len(names) - 1
    assert state["calls"] == 2 * non_empty * len(FC.HISTOGRAM_FIELDS) + len(FC.TOPS) + 1 + 1, state["calls"]
    stats["hook_calls"] = state["calls"]
    print("DOCSET_FACETS_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
