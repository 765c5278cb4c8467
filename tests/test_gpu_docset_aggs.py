"""Numeric aggregations of a doc set on the device (DocSet.aggregate / stats / histogram, vq_docset_aggregate, k_docset_agg_ids / k_docset_agg_values):
a. every case of tests/docsetaggcases.py on the whole index against the yardstick, field for field and bit for bit (the sum against math.fsum),
   once more with the wave pre-reduction of the sum switched off (VQ_NO_AGG_PREREDUCE=1) and once more on a grid of three workgroups per
   aggregation (VQ_AGG_MAX_GRID=3: every workgroup strides over its share in many rounds): the same bits;
b. bucket i against len(ds & DocSet.from_range(gte=e(i-1), lt=e(i))) for columns keyed by doc; two consecutive calls give identical results;
   several aggregations in one call, one field twice and 1:n mixed with anchor-keyed;
c. misuse, every refusal with its code, a shard without the hook included;
d. three shards in one process under one generic barrier-style sum hook, called from three threads: every rank ends with the whole index's answer
   bit for bit, a set that is empty on one rank and one that is empty everywhere included;
e. eight threads on one shared set."""
import os
import threading

import pytest

import docsetaggcases as AC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import veloci_amd
    os.environ.pop("VQ_NO_AGG_PREREDUCE", None)
    os.environ.pop("VQ_AGG_MAX_GRID", None)
    whole = veloci_amd.Index(AC.index_data(), device=0)

    def never(values):
        raise AssertionError("an unsharded index called the hook")

    whole.set_allreduce(never)
    return {"whole": whole, "sets": {name: veloci_amd.DocSet(whole, ids) for name, ids in AC.sets().items()}}


# ------------------------------------------------------------------------------------------ a: every case against the yardstick
@pytest.mark.parametrize("name", list(AC.sets()))
def test_every_case_equals_the_yardstick_bit_for_bit(built, name):
    cases = [c for c in AC.cases() if c[1] == name]
    assert len(cases) >= len(AC.ANCHOR_FIELDS) + 1
    ds = built["sets"][name]
    first = [AC.check_case(ds, c) for c in cases]
    os.environ["VQ_NO_AGG_PREREDUCE"] = "1"
    try:
        again = [AC.check_case(ds, c) for c in cases]
    finally:
        del os.environ["VQ_NO_AGG_PREREDUCE"]
    assert all(AC.same(a, b) for a, b in zip(first, again))
    os.environ["VQ_AGG_MAX_GRID"] = "3"
    try:
        strided = [AC.check_case(ds, c) for c in cases]
    finally:
        del os.environ["VQ_AGG_MAX_GRID"]
    assert all(AC.same(a, b) for a, b in zip(first, strided))


# ------------------------------------------------------------------------------------------ b: buckets, repetition, several in one call
IDENTITY = [("w-dense", "sparse", "quarter"), ("w-ids200", "full", "one-key"), ("l-every", "full", "tiny"), ("l-every", "full", "1e39"), ("l-medium", "late", "quarter"),
            ("l-every", "crafted", "minus-1e39")]


@pytest.mark.parametrize("name,field,edges", IDENTITY)
def test_a_bucket_is_the_length_of_the_set_under_the_range(built, name, field, edges):
    import veloci_amd
    idx, ds, e = built["whole"], built["sets"][name], AC.edge_lists()[edges]
    got = ds.histogram(field, e)
    assert len(got) == len(e) + 1 and sum(got) == ds.stats(field)["count"]
    for i, count in enumerate(got):
        bounds = {}
        if i > 0:
            bounds["gte"] = e[i - 1]
        if i < len(e):
            bounds["lt"] = e[i]
        clause = AC.to_json([dict(bounds, field=field)])
        under = ds & veloci_amd.DocSet.from_ranges(idx, clause)
        assert len(under) == count, (name, field, i, bounds, len(under), count)
        under.close()


def test_two_consecutive_calls_and_several_aggregations_in_one(built):
    E, S = AC.edge_lists(), AC.sets()
    mix = [("full", "quarter"), ("m[].v", "one"), ("full", "none"), ("sparse", "1023"), ("m[].v", "quarter"), ("crafted", "none"), ("full", "quarter"), ("late", "tiny")]
    specs = AC.to_json([AC.spec(f, E[e]) for f, e in mix])
    for name in ("w-dense", "w-ids200", "l-every", "n5", "w-empty"):
        ds = built["sets"][name]
        a, b = ds.aggregate(specs), ds.aggregate(specs)
        assert len(a) == len(b) == len(mix) and all(AC.same(x, y) for x, y in zip(a, b)), name
        for got, (f, e) in zip(a, mix):
            assert AC.same(got, AC.expected(f, S[name], E[e])), (name, f, e, got)
        assert AC.same(a[0], a[6])
    st = built["sets"]["big"].stats("crafted")
    assert st["sum"] == 1.0 and st["mean"] == 1.0 / 3.0 and st["min"] == -2.0 ** 100 and built["sets"]["only-nan"].stats("crafted")["mean"] is None


# ------------------------------------------------------------------------------------------ c: misuse
def test_misuse_is_refused_with_its_code(built):
    import veloci_amd
    other = veloci_amd.Index(AC.index_data(), device=0)
    bare = veloci_amd.Index(AC.index_data(*AC.SHARD), device=0, doc_lo=AC.SHARD[0], doc_hi=AC.SHARD[1])  # a shard without the hook
    AC.check_misuse(veloci_amd, built["whole"], other, bare)
    ds = veloci_amd.DocSet(built["whole"], [1, 2, 3])
    ds.close()
    with pytest.raises(ValueError):
        ds.stats("full")


# ------------------------------------------------------------------------------------------ d: shards
def test_three_shards_under_one_sum_hook_end_with_the_whole_index_answer():
    import veloci_amd
    hook = AC.SumHook(3)
    shards = [veloci_amd.Index(AC.shard_index_data(lo, hi), device=0, doc_lo=lo, doc_hi=hi) for lo, hi in AC.THREE]
    for rank, s in enumerate(shards):
        s.set_allreduce(hook.of(rank))
    calls = AC.check_shards(veloci_amd, shards, hook)
    assert calls == 5 * (len(AC.SHARD_SETS) - 1) and sorted(set(hook.sizes))[-1] == 512 * len(AC.SHARD_SPECS)
    for s in shards:
        s.set_allreduce(None)


# ------------------------------------------------------------------------------------------ e: threads
def test_eight_threads_on_one_shared_set(built):
    E, S = AC.edge_lists(), AC.sets()
    work = [("w-dense", "full", "quarter"), ("w-dense", "m[].v", "one"), ("w-ids200", "m[].v", "quarter"), ("w-dense", "crafted", "none")]
    want = {w: AC.expected(w[1], S[w[0]], E[w[2]]) for w in work}
    failures = []

    def run(t):
        try:
            for k in range(4):
                w = work[(t + k) % len(work)]
                got = built["sets"][w[0]].aggregate(AC.to_json([AC.spec(w[1], E[w[2]])]))[0]
                if not AC.same(got, want[w]):
                    failures.append((t, w, got))
        except Exception as e:  # noqa: BLE001 - reported below
            failures.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
