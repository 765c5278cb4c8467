"""Doc sets from numeric ranges on the device (DocSet.from_ranges, vq_docset_from_ranges, k_range_bits / k_range_probe / k_range_scatter):
a. every case of tests/docsetrangecases.py on a whole index and on an unaligned shard: the image element for element against numpy's comparison
   in float64, len and local_len, the route; each probe-route case once more under VQ_NO_RANGE_PROBE=1 with identical ids;
b. the shard's hook receives exactly one u64 per call, numpy's local count; the whole index never calls it;
c. searches with and without a `filter` of their own under a range set and under DocSet(index, <numpy's ids>): ids and score bits equal; a range
   set as a `combine` operand and as the `within` of from_filter against numpy's algebra;
d. misuse, every refusal with its code, a shard without the hook included; e. eight threads on one index with a shared `within`."""
import os
import threading

import numpy as np
import pytest

import docsetrangecases as RC
import docsetref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import veloci_amd
    state = {"calls": 0}
    whole = veloci_amd.Index(RC.index_data(), device=0)
    shard = veloci_amd.Index(RC.index_data(*RC.SHARD), device=0, doc_lo=RC.SHARD[0], doc_hi=RC.SHARD[1])
    shard.set_allreduce(RC.counting_hook(state))
    whole.set_allreduce(RC.counting_hook({"local": -1, "len": -1}))  # never called: an unsharded index needs no sum
    out = {"whole": (whole, 0, RC.N), "shard": (shard, *RC.SHARD), "state": state}
    for where in ("whole", "shard"):
        out[where + "-sets"] = {name: (None if ids is None else veloci_amd.DocSet(out[where][0], ids)) for name, ids in RC.withins().items()}
    os.environ.pop("VQ_NO_RANGE_PROBE", None)
    return out


# ------------------------------------------------------------------------------------------ a, b: the images, the routes, the hook
@pytest.mark.parametrize("where", ["whole", "shard"])
@pytest.mark.parametrize("within", list(RC.withins()))
def test_images_equal_numpy_on_both_routes(built, where, within):
    import veloci_amd
    idx, lo, hi = built[where]
    state = built["state"]
    cases = [c for c in RC.cases() if c[2] == within]
    assert len(cases) >= len(RC.UNDER_WITHINS)
    before, routes = state["calls"], []
    for case in cases:
        routes.append(RC.check_case(veloci_amd, idx, lo, hi, state, case, built[where + "-sets"], os.environ))
    # check_case holds the hook to one call per set made on the shard and to none on the whole index; the hook holds the one u64 against numpy's count
    assert state["calls"] - before == (len(cases) + sum(routes) if where == "shard" else 0)
    one_to_n = sum(any("[]" in c["field"] for c in RC.clause_lists()[case[1]]) for case in cases)
    assert sum(routes) == (len(cases) - one_to_n if within in ("ids200", "empty", "edges") else 0)


def test_from_range_is_from_ranges_with_one_clause(built):
    import veloci_amd
    idx, lo, hi = built["whole"]
    for kwargs in ({"gte": 10.0}, {"gt": -3.5, "lte": 7.75}, {"lt": -250.25, "missing": True}, {}):
        a = veloci_amd.DocSet.from_range(idx, "sparse", **kwargs)
        want = RC.expected([dict(kwargs, field="sparse")], None, lo, hi)
        docsetref.check(a, want, RC.N, lo, hi)
        t = a.ids_tensor()
        assert t.is_cuda and np.array_equal(t.cpu().numpy().astype(np.int64), want)
        w = veloci_amd.DocSet.from_range(idx, "full", lt=0.0, within=a)
        docsetref.check(w, RC.expected([dict(kwargs, field="sparse"), {"field": "full", "lt": 0.0}], None, lo, hi), RC.N, lo, hi)


# ------------------------------------------------------------------------------------------ c: composition and search
SEARCHES = [
    {"search_req": {"search": {"path": "body", "terms": ["alpha"]}}},
    {"search_req": {"or": {"queries": [{"search": {"path": "body", "terms": ["alpha"]}}, {"search": {"path": "body", "terms": ["beta"]}}]}}},
    {"search_req": {"search": {"path": "body", "terms": ["alpha"]}}, "boost": [{"path": "full", "boost_fun": "Add", "param": 1.0}]},
    {"search_req": {"or": {"queries": [{"search": {"path": "body", "terms": ["alpha"]}}, {"search": {"path": "body", "terms": ["beta"]}}]}},
     "filter": {"search": {"path": "body", "terms": ["alpha"]}}},
    {"search_req": {"search": {"path": "body", "terms": ["beta"]}}, "filter": {"or": {"queries": [{"search": {"path": "body", "terms": ["alpha"]}}, {"search": {"path": "body", "terms": ["beta"]}}]}}},
]
SEARCHED_UNDER = ("no-bounds", "gte", "missing-interval", "1n-missing", "clauses-9", "upside-down")


def test_searches_under_a_range_set_equal_searches_under_its_ids(built):
    import veloci_amd
    idx, lo, hi = built["whole"]
    hits = 0
    for name in SEARCHED_UNDER:
        clauses = RC.clause_lists()[name]
        want = RC.expected(clauses, None, lo, hi)
        by_range, by_ids = veloci_amd.DocSet.from_ranges(idx, clauses), veloci_amd.DocSet(idx, want)
        for req in SEARCHES:
            a, b = veloci_amd.search(req, idx, docset=by_range), veloci_amd.search(req, idx, docset=by_ids)
            assert a.num_hits == b.num_hits and np.array_equal(a.ids, b.ids), (name, req, a.ids, b.ids)
            assert np.array_equal(np.asarray(a.scores, np.float32).view(np.uint32), np.asarray(b.scores, np.float32).view(np.uint32)), (name, req)
            assert np.isin(a.ids, want).all()
            hits += int(a.num_hits)
    assert hits > 10  # the sets hold docs of the two terms: the searches found something to compare


@pytest.mark.parametrize("where", ["whole", "shard"])
def test_a_range_set_composes_with_the_algebra_and_with_from_filter(built, where):
    import veloci_amd
    idx, lo, hi = built[where]
    state, L = built["state"], RC.clause_lists()

    def made(make, want):
        state["local"], state["len"] = int(((want >= lo) & (want < hi)).sum()), int(want.size)
        ds = make()
        assert "error" not in state, state["error"]
        docsetref.check(ds, want, RC.N, lo, hi)
        return ds

    a_ids, b_ids, r_ids = RC.expected(L["both"], None, lo, hi), RC.expected(L["1n"], None, lo, hi), RC.expected(L["rare"], None, lo, hi)
    a = made(lambda: veloci_amd.DocSet.from_ranges(idx, L["both"]), a_ids)
    b = made(lambda: veloci_amd.DocSet.from_ranges(idx, L["1n"]), b_ids)
    r = made(lambda: veloci_amd.DocSet.from_ranges(idx, L["rare"]), r_ids)
    both = made(lambda: a & b, np.intersect1d(a_ids, b_ids))
    made(lambda: a | r, np.union1d(a_ids, r_ids))
    made(lambda: a - b, np.setdiff1d(a_ids, b_ids))
    made(lambda: ~a, np.setdiff1d(np.arange(RC.N), a_ids))
    few = made(lambda: r & a, np.intersect1d(r_ids, a_ids))
    assert few.route == 1 and both.route == 0 and both.range_route == -1 and a.route == -1  # the algebra's own routes: a range set is an ordinary operand
    # the docs of the two terms: alpha 1, 70 500, 149 000; beta 2, 100 000
    term_docs = np.array([1, 2, 70_500, 100_000, 149_000])
    leaf = {"or": {"queries": [{"search": {"path": "body", "terms": ["alpha"]}}, {"search": {"path": "body", "terms": ["beta"]}}]}}
    everything = made(lambda: veloci_amd.DocSet.from_ranges(idx, L["no-bounds"]), RC.expected(L["no-bounds"], None, lo, hi))
    made(lambda: veloci_amd.DocSet.from_filter(idx, leaf, within=everything), np.intersect1d(term_docs, RC.expected(L["no-bounds"], None, lo, hi)))
    made(lambda: veloci_amd.DocSet.from_filter(idx, leaf, within=a), np.intersect1d(term_docs, a_ids))


# ------------------------------------------------------------------------------------------ d: misuse
def test_misuse_is_refused_with_its_code(built):
    import veloci_amd
    other = veloci_amd.Index(RC.index_data(), device=0)
    bare = veloci_amd.Index(RC.index_data(*RC.SHARD), device=0, doc_lo=RC.SHARD[0], doc_hi=RC.SHARD[1])  # a shard without the hook
    RC.check_misuse(veloci_amd, built["whole"][0], other, bare)
    ds = veloci_amd.DocSet(built["whole"][0], [1, 2, 3])
    ds.close()
    with pytest.raises(ValueError):
        veloci_amd.DocSet.from_range(built["whole"][0], "full", gte=1.0, within=ds)


# ------------------------------------------------------------------------------------------ e: threads
def test_eight_threads_on_one_index_with_a_shared_within(built):
    import veloci_amd
    idx, lo, hi = built["whole"]
    sets, L, W = built["whole-sets"], RC.clause_lists(), RC.withins()
    work = [("gte", "none"), ("clauses-17", "ids200"), ("1n-and-columns", "dense"), ("missing-interval", "ids200"), ("late-missing", "dense"), ("rare", "none"),
            ("1n", "ids200"), ("lt-f32-0.1", "edges")]
    want = {w: RC.expected(L[w[0]], W[w[1]], lo, hi) for w in work}
    failures = []

    def run(t):
        try:
            for k in range(6):
                name, within = work[(t + k) % len(work)]
                ds = veloci_amd.DocSet.from_ranges(idx, RC.to_json(L[name]), within=sets[within])
                if not (np.array_equal(ds.ids(), want[(name, within)]) and len(ds) == want[(name, within)].size):
                    failures.append((t, name, within))
                ds.close()
        except Exception as e:  # noqa: BLE001 - reported below
            failures.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
