"""Driver of the host-stub build for the batched highlight (run by tests/test_highlight_batch_cpu.py with VQ_LIB=<host-stub library> and
VQ_STUB_DICT_SCAN=1).  The stubbed launchers answer exact, distance-0 prefix and regex probes and the two text-rank kernels on the host in
the kernels' own formats, so the fixed parts without a Levenshtein distance go through the whole host side of vq_highlight_batch — the store
check, slots, rounds, the page's snippets — against vq_highlight_json one by one and the CPU oracle; failing parts, n == 0 and the counters
as well.  With VQ_NO_HIGHLIGHT_RANK=1 the same answers must come from the host route.  Prints one summary line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import veloci_amd  # noqa: E402
import highlightcorpus as HC  # noqa: E402
from oracle import binding as O  # noqa: E402
from veloci_amd import _lib  # noqa: E402

assert "host_stub" in _lib.lib_path(), _lib.lib_path()
assert os.environ.get("VQ_STUB_DICT_SCAN") == "1"


def counters(idx):
    a, b = C.c_uint64(), C.c_uint64()
    _lib.lib().vq_index_highlight_rank_counts(idx.h, C.byref(a), C.byref(b))
    _lib.lib().vq_index_highlight_rank_counts(idx.h, None, None)
    return a.value, b.value


def main():
    data, _ = HC.build()
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    good = [p for p in HC.fixed_parts() if not p.get("levenshtein_distance")]
    parts = good[:5] + [HC.FAILING[0]] + good[5:] + HC.FAILING[1:] + good[:3]
    got = veloci_amd.highlight_batch(parts, idx, raise_on_error=False)
    assert len(got) == len(parts)
    failed = entries = 0
    for k, (p, g) in enumerate(zip(parts, got)):
        try:
            single = HC.bits(veloci_amd.highlight(p, idx))
        except veloci_amd.VelociError as e:
            assert isinstance(g, veloci_amd.VelociError) and g.code == e.code, (k, p, g, e.code, str(e))
            try:
                ora.highlight_json(HC.as_text(p))
                raise AssertionError("the oracle answers a part the product fails: %r" % (p,))
            except O.OracleError:
                pass
            failed += 1
            continue
        assert not isinstance(g, veloci_amd.VelociError), (k, p, g.code, str(g))
        assert HC.bits(g) == single, (k, p, HC.bits(g)[:6], single[:6])
        assert single == HC.bits(ora.highlight_json(HC.as_text(p))), (k, p)
        entries += len(g)
    assert failed >= len(HC.FAILING)
    assert veloci_amd.highlight_batch([], idx) == []
    try:
        veloci_amd.highlight_batch(parts, idx)
        raise AssertionError("a failing part did not raise")
    except veloci_amd.VelociError as e:
        assert str(e).startswith("JsonError"), str(e)
    d0, s0 = counters(idx)
    assert len(veloci_amd.highlight_batch([HC.FREQUENT], idx)[0]) == 10
    d1, s1 = counters(idx)
    everything = dict(HC.FREQUENT)
    del everything["top"]
    matched = len(veloci_amd.highlight(everything, idx))
    print("HIGHLIGHT_BATCH_DRIVER_OK " + json.dumps({"parts": len(parts), "failed": failed, "entries": entries, "device_parts": d1, "snippets_built": s1,
                                                      "frequent_device_parts": d1 - d0, "frequent_snippets": s1 - s0, "frequent_matched": matched,
                                                      "no_rank": os.environ.get("VQ_NO_HIGHLIGHT_RANK") == "1"}))


if __name__ == "__main__":
    main()
