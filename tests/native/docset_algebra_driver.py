"""Driver of tests/test_docset_algebra_cpu.py, run with VQ_LIB=<libveloci_host_stub.so> and VQ_STUB_DICT_SCAN=1: the doc set algebra over the stubbed
device layer (tests/native/hip_stub_docset_algebra.cpp answers the launchers with host loops) — the routing, the rounds over the operand table, the
temporary bitmap of the word route, the shard masking and the sharded length — against numpy (tests/docsetalgebracases.py for the ids,
tests/docsetref.py for the image), on a whole index and on an unaligned shard, under both routes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
import docsetalgebracases as AC  # noqa: E402
import docsetref as R  # noqa: E402

PARTS = (0, 1, 2, 3, 4)


def main():
    data = R.small_data()
    total = {"n": None, "calls": 0}

    def hook(values):
        assert values.size == 1
        total["calls"] += 1
        values[0] = total["n"]

    whole = veloci_amd.Index(data)
    shard = veloci_amd.Index(data, doc_lo=R.SHARD[0], doc_hi=R.SHARD[1])
    stats = {"cases": 0, "probe": 0, "word": 0, "forced": 0, "on_shard": 0}
    # a shard without the hook declines, naming it
    one = veloci_amd.DocSet(shard, [70_500])
    try:
        ~one
        raise AssertionError("a shard without the hook combined")
    except veloci_amd.VelociError as e:
        assert e.code == 4 and "vq_index_set_allreduce" in str(e), (e.code, str(e))
    shard.set_allreduce(hook)
    for idx in (whole, shard):
        lo, hi = idx.doc_lo, idx.doc_hi
        made = {}

        def operand(o):
            key = o if isinstance(o, str) else id(o)
            if key not in made:
                made[key] = veloci_amd.DocSet(idx, AC.ids_of(o))
            return made[key]

        for name, op, operands in AC.image_cases():
            want = AC.expected(op, operands)
            total["n"] = len(want)
            sets = [operand(o) for o in operands]
            ds = veloci_amd.DocSet.combine(idx, op, sets)
            image = R.check(ds, want, AC.N, lo, hi)
            route = AC.expected_route(op, operands, lo, hi)
            assert ds.route == route, (name, ds.route, route)
            if image["bitmap"] is not None:  # no bit outside the doc range
                docs = np.flatnonzero(np.unpackbits(ds.part(1).view(np.uint8), bitorder="little")) + image["base"]
                assert docs.min() >= lo and docs.max() < hi
            stats["cases"] += 1
            stats["on_shard"] += (1 + route) * (idx is shard)
            stats["probe" if route else "word"] += 1
            if route:  # the same case through the word route: the same image
                os.environ["VQ_NO_SETOP_PROBE"] = "1"
                try:
                    forced = veloci_amd.DocSet.combine(idx, op, sets)
                finally:
                    del os.environ["VQ_NO_SETOP_PROBE"]
                assert forced.route == 0, name
                for which in PARTS:
                    assert np.array_equal(forced.part(which), ds.part(which)), (name, which)
                assert len(forced) == len(ds) and forced.device_bytes == ds.device_bytes
                stats["forced"] += 1
                forced.close()
            ds.close()
        # operators, composition, export
        a, b, c = operand("dense"), operand("sparse"), operand("medium")
        want = np.setdiff1d(np.union1d(AC.ids_of("dense"), AC.ids_of("sparse")), AC.ids_of("medium"))
        total["n"] = len(np.union1d(AC.ids_of("dense"), AC.ids_of("sparse")))
        ab = a | b
        total["n"] = len(want)
        R.check(ab - c, want, AC.N, lo, hi)
        R.check(ab.minus(c), want, AC.N, lo, hi)
        total["n"] = AC.N - len(AC.ids_of("sparse"))
        nb = ~b
        total["n"] = len(AC.ids_of("sparse"))
        R.check(~nb, AC.ids_of("sparse"), AC.N, lo, hi)
        assert a.route == -1 and nb.route == 0
        ids = b.ids()
        few = np.full(8, 0xABABABAB, np.uint32)
        assert int(veloci_amd.lib().vq_docset_ids(b._handle(), few.ctypes.data, 5, 0)) == len(ids) and np.array_equal(few[:5], ids[:5]) and few[5] == 0xABABABAB
        closed = veloci_amd.DocSet(idx, [1])
        closed.close()
        try:
            a & closed
            raise AssertionError("a closed operand was accepted")
        except ValueError:
            pass
    assert total["calls"] == stats["on_shard"] + 5, total  # one u64 per set combined on the shard (5: the operator lines), none on the whole index
    print("DOCSET_ALGEBRA_DRIVER_OK " + json.dumps(stats))


if __name__ == "__main__":
    main()
