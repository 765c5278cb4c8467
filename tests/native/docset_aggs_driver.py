"""Driver of tests/test_docset_aggs_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: the numeric aggregations of a doc set
over the stubbed device layer (tests/native/hip_stub_docset_aggs.cpp answers the launchers with host loops) — parsing, column resolution, the
edges' move to keys, the state area, the rounding of the exact sum, the sum over three shards with the min / max agreement and the error paths —
against the yardstick of tests/docsetaggcases.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsetaggcases as AC  # noqa: E402


def main():
    whole = veloci_amd.Index(AC.index_data())
    other = veloci_amd.Index(AC.index_data())
    bare = veloci_amd.Index(AC.index_data(*AC.SHARD), doc_lo=AC.SHARD[0], doc_hi=AC.SHARD[1])  # a shard without the hook
    AC.check_misuse(veloci_amd, whole, other, bare)

    def never(values):
        raise AssertionError("an unsharded index called the hook")

    whole.set_allreduce(never)
    stats = {"cases": 0, "one_to_n": 0}
    made = {name: veloci_amd.DocSet(whole, ids) for name, ids in AC.sets().items()}
    for case in AC.cases():
        AC.check_case(made[case[1]], case)
        stats["cases"] += 1
        stats["one_to_n"] += "[]" in case[2]
    # several aggregations in one call: one field twice, 1:n mixed with anchor-keyed; request order
    E, S = AC.edge_lists(), AC.sets()
    mix = [("full", "quarter"), ("m[].v", "one"), ("full", "none"), ("sparse", "1023"), ("m[].v", "quarter"), ("crafted", "none")]
    for name in ("w-dense", "w-ids200", "n5"):
        got = made[name].aggregate([AC.spec(f, E[e]) for f, e in mix])
        assert len(got) == len(mix)
        for g, (f, e) in zip(got, mix):
            assert AC.same(g, AC.expected(f, S[name], E[e])), (name, f, e, g)
    st = made["big"].stats("crafted")
    assert st["sum"] == 1.0 and st["mean"] == 1.0 / 3.0 and made["only-nan"].stats("crafted")["mean"] is None
    assert made["w-dense"].histogram("sparse", E["quarter"]) == AC.expected("sparse", S["w-dense"], E["quarter"])["buckets"]
    # three shards as three threads of this process
    hook = AC.SumHook(3)
    shards = [veloci_amd.Index(AC.shard_index_data(lo, hi), doc_lo=lo, doc_hi=hi) for lo, hi in AC.THREE]
    for rank, s in enumerate(shards):
        s.set_allreduce(hook.of(rank))
    stats["hook_calls"] = AC.check_shards(veloci_amd, shards, hook)
    stats["hook_sizes"] = sorted(set(hook.sizes))
    print("DOCSET_AGGS_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
