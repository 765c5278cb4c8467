"""Driver of the host-stub build for the batched suggest (run by tests/test_suggest_batch_cpu.py with VQ_LIB=<host-stub library> and
VQ_STUB_DICT_SCAN=1).  Exact-term suggests, which need no dictionary scan, failing requests and n == 0 through vq_suggest_batch against
vq_suggest_json one by one and the CPU oracle; and, because the stubbed launchers answer prefix probes of distance 0 on the host in the
kernels' own formats, prefix parts with `top` through the whole host side of the top-n route as well.  Prints one summary line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import veloci_amd  # noqa: E402
import suggestcorpus as SC  # noqa: E402
from oracle import binding as O  # noqa: E402
from veloci_amd import _lib  # noqa: E402

assert "host_stub" in _lib.lib_path(), _lib.lib_path()
assert os.environ.get("VQ_STUB_DICT_SCAN") == "1"


def main():
    data, terms = SC.build()
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    P = SC.part
    exact = [P("a", t, **kw) for t in ("foo", "FOO", "Foo", "bar", "ab", "nothere") for kw in ({}, {"top": 1}, {"ignore_case": False}, {"boost": 2.0, "top": 5, "skip": 1})]
    exact += [{"suggest": [P("a", "foo"), P("b", "foo"), P("a", "foo")], "top": 2}, {"suggest": [P("a", "Bar", top=3), P("b", "ab")], "skip": 1}]
    # distance 0 only (what the stub's scan loop answers), 16-bit image only
    prefix = [P("a", t, starts_with=True, top=top, skip=skip, boost=boost) for t in ("w", "qa", "qb", "qc", "zz", "fo", "wa") for top, skip, boost in
              ((1, None, None), (10, None, None), (10, 3, -1.0), (200, None, None), (1848, None, None), (1849, None, None), (None, None, None), (0, 4, 0.0))]
    prefix += [P("a", t, starts_with=True, top=0) for t in ("zza", "fo")]  # (top + skip == 0: fewer than 200 matches, the reference panics beyond)
    prefix += [{"suggest": [P("a", "w", starts_with=True, top=10), P("a", "zz", starts_with=True, top=10), P("a", "foo")], "top": 10},
               {"suggest": [P("a", "w", starts_with=True, top=10)] * 2, "top": 5},
               P("a", "w", starts_with=True, top=10, token_value={"path": "a", "boost_fun": "Multiply", "param": 0})]
    reqs = exact[:3] + [SC.FAILING[0]] + exact[3:] + SC.FAILING[1:] + prefix + [SC.FAILING[2]] + exact[:2]
    got = veloci_amd.suggest_batch(reqs, idx, raise_on_error=False)
    assert len(got) == len(reqs)
    failed = 0
    for k, (r, g) in enumerate(zip(reqs, got)):
        try:
            single = SC.bits(veloci_amd.suggest(r, idx))
        except veloci_amd.VelociError as e:
            assert isinstance(g, veloci_amd.VelociError) and g.code == e.code, (k, r, g, e.code)
            failed += 1
            continue
        assert not isinstance(g, veloci_amd.VelociError), (k, r, g.code)
        assert SC.bits(g) == single, (k, r, SC.bits(g)[:8], single[:8])
        assert single == SC.bits(ora.suggest_json(SC.as_text(r))), (k, r)
    assert failed == len(SC.FAILING) + 1
    assert veloci_amd.suggest_batch([], idx) == []
    try:
        veloci_amd.suggest_batch(reqs, idx)
        raise AssertionError("a failing request did not raise")
    except veloci_amd.VelociError as e:
        assert str(e).startswith("JsonError"), str(e)
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _lib.lib().vq_index_suggest_topn_probes(idx.h, None, C.byref(c))
    assert len(veloci_amd.suggest_batch([P("a", "w", starts_with=True, top=10)], idx)[0]) == 10  # the 2500-match prefix alone
    _lib.lib().vq_index_suggest_topn_probes(idx.h, C.byref(a), C.byref(b))
    print("SUGGEST_BATCH_DRIVER_OK " + json.dumps({"requests": len(reqs), "failed": failed, "entries": sum(len(g) for g in got if isinstance(g, list)),
                                                    "topn_probes": a.value, "records": b.value, "records_w_top10": b.value - c.value, "no_topn": os.environ.get("VQ_NO_SUGGEST_TOPN") == "1"}))


if __name__ == "__main__":
    main()
