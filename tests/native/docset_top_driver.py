"""Driver of tests/test_docset_top_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: a doc set ordered by a column over the
stubbed device layer (tests/native/hip_stub_docset_top.cpp answers the launchers with host loops) — spec parsing, column resolution, the scratch
area, the kernel sequence, the final order, skip and top, three shards with merge, pack and unpack, and the error paths — against the yardstick of
tests/docsettopcases.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsettopcases as TC  # noqa: E402


def main():
    for name in ("VQ_TOP_MAX_GRID", "VQ_TOP_FORCE_SELECT"):
        os.environ.pop(name, None)
    whole = veloci_amd.Index(TC.index_data())
    other = veloci_amd.Index(TC.index_data())
    TC.check_misuse(veloci_amd, whole, other)

    def never(values):
        raise AssertionError("a doc set ordered by a column called the hook")

    whole.set_allreduce(never)
    made = {name: veloci_amd.DocSet(whole, ids) for name, ids in TC.sets().items()}
    stats = {"cases": 0, "strided": 0, "forced": 0}
    cases = TC.cases()
    first = {}
    for case in cases:
        first[case] = TC.check_case(made[case[0]], case).pack()
        stats["cases"] += 1
    # every case of the small sets and every extra page again on a grid of three workgroups and with the select forced: the same rows
    extra = {e + (w,) for e in TC.extra_pages() for w in (True, False)}
    again = [c for c in cases if TC.sets()[c[0]].size <= 200 or c in extra]
    for knob, key in (("VQ_TOP_MAX_GRID", "strided"), ("VQ_TOP_FORCE_SELECT", "forced")):
        os.environ[knob] = str(TC.GRID) if knob == "VQ_TOP_MAX_GRID" else "1"
        try:
            for case in again:
                assert TC.check_case(made[case[0]], case).pack() == first[case], (knob, case)
                stats[key] += 1
        finally:
            del os.environ[knob]
    shards = [veloci_amd.Index(TC.shard_index_data(lo, hi), doc_lo=lo, doc_hi=hi) for lo, hi in TC.THREE]
    stats["merges"] = TC.check_shards(veloci_amd, shards)
    print("DOCSET_TOP_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
