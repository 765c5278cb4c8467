"""Doc sets ordered by a column on the device (DocSet.top_by, vq_docset_top_by, k_top_fold / k_top_keys / k_top_pick / k_top_hist / k_top_tiecount /
k_top_emit):
a. every case of tests/docsettopcases.py on the whole index against the yardstick — docs and kinds element for element, values bit for bit, the
   counters number for number —, once more on a grid of three workgroups per kernel (VQ_TOP_MAX_GRID=3: many strided rounds, tie runs over
   several chunks) and once more with the select forced (VQ_TOP_FORCE_SELECT=1): the same rows;
b. for columns keyed by doc the counters equal ds.stats(field); pages (10, 0), (10, 10), (10, 20) concatenated give page (30, 0); two consecutive
   calls are identical; on `flat` the docs are ds.ids()[skip:skip + top];
c. misuse, every refusal with its code;
d. the three doc ranges of docsetaggcases.THREE as three indexes in one process without any hook: the merged parts equal the whole index's rows
   bit for bit, packed parts merge to the same, parts with different `top` are refused;
e. eight threads on one shared set."""
import os
import threading

import numpy as np
import pytest

import docsettopcases as TC

pytestmark = pytest.mark.gpu

KNOBS = ("VQ_TOP_MAX_GRID", "VQ_TOP_FORCE_SELECT")


@pytest.fixture(scope="module")
def built():
    import veloci_amd
    for name in KNOBS:
        os.environ.pop(name, None)
    whole = veloci_amd.Index(TC.index_data(), device=0)

    def never(values):
        raise AssertionError("a doc set ordered by a column called the hook")

    whole.set_allreduce(never)
    return {"whole": whole, "sets": {name: veloci_amd.DocSet(whole, ids) for name, ids in TC.sets().items()}}


# ------------------------------------------------------------------------------------------ a: every case against the yardstick
@pytest.mark.parametrize("name", TC.SET_NAMES)
def test_every_case_equals_the_yardstick_bit_for_bit(built, name):
    cases = [c for c in TC.cases() if c[0] == name]
    assert len(cases) >= 4 * len(TC.FIELDS) * 4
    ds = built["sets"][name]
    first = [TC.check_case(ds, c).pack() for c in cases]
    for knob, value in (("VQ_TOP_MAX_GRID", str(TC.GRID)), ("VQ_TOP_FORCE_SELECT", "1")):
        os.environ[knob] = value
        try:
            again = [TC.check_case(ds, c).pack() for c in cases]
        finally:
            del os.environ[knob]
        assert again == first, knob


# ------------------------------------------------------------------------------------------ b: counters, pages, repetition, pure doc order
@pytest.mark.parametrize("name", ("l-every", "w-dense", "w-ids200", "n5", "late-ends", "only-nan", "w-empty"))
def test_counters_pages_repetition_and_the_flat_column(built, name):
    ds = built["sets"][name]
    ids = ds.ids()
    for field in TC.ANCHOR_FIELDS:
        st = ds.stats(field)
        for descending in (False, True):
            whole = ds.top_by(field, top=30, descending=descending)
            assert whole.counters == {k: st[k] for k in ("docs", "count", "nan", "missing")}, (name, field)
            parts = [ds.top_by(field, top=10, skip=skip, descending=descending) for skip in (0, 10, 20)]
            assert np.array_equal(np.concatenate([p.docs for p in parts]), whole.docs) and np.array_equal(np.concatenate([p.kinds for p in parts]), whole.kinds)
            assert np.array_equal(np.concatenate([p.values for p in parts]).view(np.uint32), whole.values.view(np.uint32))
            again = ds.top_by(field, top=30, descending=descending)
            assert again.pack() == whole.pack()
    for top, skip in ((10, 0), (7, 3), (100, 150), (65_536, 0), (36, 65_500), (0, 0)):
        for descending in (False, True):
            got = ds.top_by("flat", top=top, skip=skip, descending=descending)
            assert np.array_equal(got.docs, ids[skip:skip + top]) and (got.values == np.float32(2.5)).all() and not got.kinds.any(), (name, top, skip)


# ------------------------------------------------------------------------------------------ c: misuse
def test_misuse_is_refused_with_its_code(built):
    import veloci_amd
    other = veloci_amd.Index(TC.index_data(), device=0)
    TC.check_misuse(veloci_amd, built["whole"], other)


# ------------------------------------------------------------------------------------------ d: shards
def test_three_shards_without_a_hook_merge_to_the_whole_index_rows():
    import veloci_amd
    shards = [veloci_amd.Index(TC.shard_index_data(lo, hi), device=0, doc_lo=lo, doc_hi=hi) for lo, hi in TC.THREE]
    assert TC.check_shards(veloci_amd, shards) == 3 * len(TC.shard_cases())


# ------------------------------------------------------------------------------------------ e: threads
def test_eight_threads_on_one_shared_set(built):
    S = TC.sets()
    work = [("w-dense", "stars", 10, 16_000, False, True), ("w-dense", "m[].v", 25, 5, True, True), ("w-ids200", "m[].v", 7, 60, False, False),
            ("w-dense", "sparse", 40, 26_000, True, True), ("l-every", "lowbyte", 300, 700, False, True)]
    want = {w: TC.expected(w[1], S[w[0]], w[2], w[3], w[4], w[5]) for w in work}
    failures = []

    def run(t):
        try:
            for k in range(5):
                w = work[(t + k) % len(work)]
                got = built["sets"][w[0]].top_by(w[1], top=w[2], skip=w[3], descending=w[4], with_missing=w[5])
                if not TC.same(got, want[w]):
                    failures.append((t, w, got.rows()[:5]))
        except Exception as e:  # noqa: BLE001 - reported below
            failures.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
