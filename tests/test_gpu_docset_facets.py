"""Facet counts of a doc set on the device (DocSet.facets, vq_docset_facets, k_docset_facet_count):
a. the histograms alone (`top: null`: every non-zero counter) against numpy (tests/docsetfacetcases.py), on a whole index and on a shard whose
   hook holds the shard's local counters against numpy before it answers with the sum, each pair once more under VQ_NO_DOCSET_FACET_LDS=1;
b. `top` 0, 1, 10, 1024, 1025 and null with crowds of ties at the cuts;
c. against the CPU oracle through the equivalence the doc-set tests use: the oracle's answer to a search under the `acl` leaf g_k (a filter tree, a
   combined set) with facets equals the facets of the set — strings, counts, order and num_hits; one mini-indexer corpus with an n-step field;
d. the library's own search with facets under the `acl` leaf over two shards against the per-shard `facets` with the hook;
e. misuse; f. eight threads on one shared set."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import docsetfacetcases as FC

pytestmark = pytest.mark.gpu

ACL_SIZES = (0, 300, 9_000, 99_999, 100_001, 130_000)
FACETS = [{"field": "cat"}, {"field": "tags[]", "top": 5}, {"field": "tags[]", "top": None}]


@pytest.fixture(scope="module")
def built():
    import veloci_amd
    state = {"calls": 0}
    whole = veloci_amd.Index(FC.index_data(), device=0)
    shard = veloci_amd.Index(FC.index_data(*FC.SHARD), device=0, doc_lo=FC.SHARD[0], doc_hi=FC.SHARD[1])
    shard.set_allreduce(FC.summing_hook(state, *FC.SHARD))
    return {"whole": (whole, 0, FC.N), "shard": (shard, *FC.SHARD), "state": state}


def facet_list(ds, facets):
    """vq_docset_facets read entry by entry: (num_hits, [(field, [(value, count)])]) — a field asked twice keeps both entries"""
    L = ds.L
    text = json.dumps(facets).encode()
    h = C.c_void_p()
    from veloci_amd import _lib
    _lib.check(L.vq_docset_facets(ds.index.h, ds._handle(), text, len(text), C.byref(h)))
    try:
        assert L.vq_result_len(h) == 0
        out = [(L.vq_result_facet_field(h, f).decode(), [(L.vq_result_facet_value(h, f, i).decode(), int(L.vq_result_facet_count(h, f, i))) for i in range(L.vq_result_facet_len(h, f))])
               for f in range(L.vq_result_num_facets(h))]
        doc = json.loads(L.vq_result_to_json(h).decode())  # the JSON rendering works unchanged on the result
        assert doc["num_hits"] == L.vq_result_num_hits(h) and doc["data"] == []
        return int(L.vq_result_num_hits(h)), out
    finally:
        L.vq_result_free(h)


# ------------------------------------------------------------------------------------------ a: the histograms alone
@pytest.mark.parametrize("where", ["whole", "shard"])
@pytest.mark.parametrize("name", list(FC.id_sets()) + ["~" + FC.COMPLEMENT_OF])
def test_histograms_equal_numpy_in_both_modes(built, where, name):
    import veloci_amd
    idx, lo, hi = built[where]
    before = built["state"]["calls"]
    assert FC.check_histograms(veloci_amd, idx, lo, hi, built["state"], [name], os.environ) == len(FC.HISTOGRAM_FIELDS)
    if where == "whole":
        assert built["state"]["calls"] == before  # an unsharded index never calls the hook
    elif name != "n0":
        assert built["state"]["calls"] > before  # ... a shard does, also for a set with no id inside it


# ------------------------------------------------------------------------------------------ b: top
@pytest.mark.parametrize("where", ["whole", "shard"])
def test_top_with_ties_at_the_cut(built, where):
    import veloci_amd
    assert FC.check_tops(veloci_amd, built[where][0], built["state"]) > 2000


# ------------------------------------------------------------------------------------------ c: against the oracle
@pytest.fixture(scope="module")
def corpus():
    """the 300 000-doc synthetic corpus of test_gpu_docset.py with its `acl` field: row k of acl.textindex.text_id_to_anchor is set k"""
    import veloci_amd
    from veloci_amd import synth
    from oracle import binding as O
    spec = synth.SynthSpec(num_docs=300_000, num_terms=5000, triples=2, extra_probe_dfs=(1000, 30_000, 300_000), background_terms=40)
    data, meta = synth.generate(spec)
    rng = np.random.default_rng(77)
    rows = [np.sort(rng.choice(data.num_anchors, size=size, replace=False)) for size in ACL_SIZES]
    acl_off = np.zeros(len(rows) + 1, np.uint64)
    acl_off[1:] = np.cumsum([len(r) for r in rows])
    acl_vals = np.concatenate(rows).astype(np.uint32)
    data.add_fst("acl.textindex", [b"g%d" % k for k in range(len(rows))])
    data.add_token_to_anchor_score("acl.textindex.to_anchor_id_score", acl_off, acl_vals, rng.integers(1, 200, size=len(acl_vals)).astype(np.uint32), None)
    data.add_key_value_store("acl.textindex.text_id_to_anchor", acl_off, acl_vals)
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    return {"data": data, "meta": meta, "idx": idx, "ora": ora, "rows": rows}


def acl_leaf(k):
    return {"search": {"path": "acl", "terms": ["g%d" % k]}}


def oracle_facets(ora, search_req, facets=FACETS):
    want = ora.search_json(json.dumps({"search_req": search_req, "facets": facets, "top": 1}))
    return want.num_hits, list(want.facets)


def test_every_acl_row_equals_the_oracles_search_under_its_leaf(corpus):
    import veloci_amd
    for k, row in enumerate(corpus["rows"]):
        ds = veloci_amd.DocSet(corpus["idx"], row)
        got = facet_list(ds, FACETS)
        want = oracle_facets(corpus["ora"], acl_leaf(k))
        assert got[0] == want[0] == len(row)
        assert [f for f, _ in got[1]] == ["cat", "tags[]", "tags[]"]
        if len(row) == 0:  # the empty set: every requested field with an empty list
            assert all(e == [] for _, e in got[1]) and all(e == [] for _, e in want[1])
            continue
        assert got[1] == want[1], (k, [(f, e[:6]) for f, e in got[1]], [(f, e[:6]) for f, e in want[1]])
        assert veloci_amd.DocSet(corpus["idx"], row).facets(FACETS) == {"cat": want[1][0][1], "tags[]": want[1][2][1]}


def test_a_set_from_a_filter_and_a_combined_set_equal_the_oracle(corpus):
    """A filter leaf selects the anchors of the TEXTS its tokens stand in, a search leaf the docs its postings hold: on `acl` (one text per row) the
    two are the same docs, so from_filter(tree over acl leaves) is held against the oracle's search with search_req = tree.  On the tokenized
    identity column `body` they are not (a filter leaf over a body term selects next to nothing, in the oracle as in the library), so the and / or
    tree over body terms is held against the oracle's search through the docs that search returns, staged as a set."""
    import veloci_amd
    idx, meta = corpus["idx"], corpus["meta"]
    tree = {"and": {"queries": [{"or": {"queries": [acl_leaf(1), acl_leaf(3)]}}, {"or": {"queries": [acl_leaf(2), acl_leaf(4)]}}]}}
    ds = veloci_amd.DocSet.from_filter(idx, tree)
    want = oracle_facets(corpus["ora"], tree)
    rows = corpus["rows"]
    assert want[0] == np.intersect1d(np.union1d(rows[1], rows[3]), np.union1d(rows[2], rows[4])).size > 10_000 and facet_list(ds, FACETS) == want
    a, b, c = meta.triples[0]
    d = meta.triples[1][0]
    leaf = lambda t: {"search": {"path": "body", "terms": [t]}}
    tree = {"and": {"queries": [{"or": {"queries": [leaf(a), leaf(b)]}}, {"or": {"queries": [leaf(c), leaf(d)]}}]}}
    hits = corpus["ora"].search_json(json.dumps({"search_req": tree, "top": 100_000}))
    want = oracle_facets(corpus["ora"], tree)
    assert want[0] == hits.num_hits == len(hits.ids) > 1000
    assert facet_list(veloci_amd.DocSet(idx, hits.ids), FACETS) == want
    # (a | b) - c of three acl rows: numpy's ids, staged as a set of their own, and the oracle's count over those very docs
    sets = [veloci_amd.DocSet(idx, corpus["rows"][k]) for k in (2, 3, 1)]
    combined = (sets[0] | sets[1]) - sets[2]
    ids = np.setdiff1d(np.union1d(corpus["rows"][2], corpus["rows"][3]), corpus["rows"][1])
    assert np.array_equal(combined.ids(), ids)
    got = facet_list(combined, FACETS)
    assert got == facet_list(veloci_amd.DocSet(idx, ids), FACETS) and got[0] == ids.size
    data = corpus["data"]
    kb, off, vals = data.key_value_stores["tags[].textindex.anchor_to_text_id"]
    rows_of = np.concatenate([vals[int(off[i - kb]):int(off[i - kb + 1])] for i in ids[:2000]])
    first = veloci_amd.DocSet(idx, ids[:2000]).facets([{"field": "tags[]", "top": None}])["tags[]"]
    counts = np.bincount(rows_of, minlength=65536)
    assert [c for _, c in first] == sorted((int(x) for x in counts[counts > 0]), reverse=True)


def test_an_n_step_field_of_a_mini_indexer_corpus_equals_the_oracle():
    """`tags[]` indexed without `facet: true` has no anchor_to_text_id store: the facet's source is the composed store"""
    import veloci_amd
    from veloci_amd import mini_indexer
    from oracle import binding as O
    rng = np.random.default_rng(3)
    words = ["red", "green", "blue", "cyan", "pink", "grey", "gold"]
    docs = [{"title": "doc %s" % ("even" if i % 2 == 0 else "odd"), "tags": [words[j] for j in rng.choice(7, size=rng.integers(0, 4), replace=False)]} for i in range(400)]
    data, _ = mini_indexer.build_index(docs, {"title": {"fulltext": {"tokenize": True}}, "tags[]": {"fulltext": {"tokenize": False}}})
    assert "tags[].textindex.anchor_to_text_id" not in data.key_value_stores and "tags[].parent_to_value_id" in data.key_value_stores
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    facets = [{"field": "tags[]", "top": None}, {"field": "tags[]", "top": 2}]
    for term in ("even", "odd", "doc"):
        search_req = {"search": {"path": "title", "terms": [term]}}
        want = oracle_facets(ora, search_req, facets)
        hits = ora.search_json(json.dumps({"search_req": search_req, "top": 1000}))
        ds = veloci_amd.DocSet(idx, hits.ids)  # the docs the oracle's search counts over
        assert want[0] == len(hits.ids) >= 200 and facet_list(ds, facets) == want, (term, facet_list(ds, facets), want)


# ------------------------------------------------------------------------------------------ d: product against product over two shards
def test_two_shards_with_the_hook_equal_the_sharded_search_under_the_acl_leaf(corpus):
    import veloci_amd
    from veloci_amd.dist import search_shards_local
    data = corpus["data"]
    cut = data.num_anchors // 3 + 11
    shards = [veloci_amd.Index(data, device=0, doc_lo=0, doc_hi=cut), veloci_amd.Index(data, device=0, doc_lo=cut, doc_hi=data.num_anchors)]
    facets = [{"field": "cat"}, {"field": "tags[]", "top": 5}]
    ks = (1, 2, 4)
    reqs = [{"search_req": acl_leaf(k), "facets": facets, "top": 1} for k in ks]
    merged = search_shards_local(shards, reqs)
    barrier, slots, total = threading.Barrier(2), [None, None], [None]

    def hook(rank):
        def add(values):
            slots[rank] = values.copy()
            barrier.wait()
            if rank == 0:
                total[0] = slots[0] + slots[1]
            barrier.wait()
            values[:] = total[0]
            barrier.wait()
        return add

    got, errs = [None, None], []

    def run(rank):
        try:
            shards[rank].set_allreduce(hook(rank))
            got[rank] = [veloci_amd.DocSet(shards[rank], corpus["rows"][k]).facet_result(facets) for k in ks]  # every rank calls in the same order
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i, k in enumerate(ks):
        for rank in (0, 1):  # every rank holds the summed answer
            assert got[rank][i].num_hits == merged[i].num_hits == len(corpus["rows"][k])
            assert got[rank][i].facets == merged[i].facets, (k, rank)
    for s in shards:
        s.set_allreduce(None)


# ------------------------------------------------------------------------------------------ e: misuse
def test_misuse(built):
    import veloci_amd
    other = veloci_amd.Index(FC.index_data(), device=0)
    bare = veloci_amd.Index(FC.index_data(*FC.SHARD), device=0, doc_lo=FC.SHARD[0], doc_hi=FC.SHARD[1])  # a shard without the hook
    FC.check_misuse(veloci_amd, built["whole"][0], other, bare)
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.DocSet(bare, [70_500]).facets([{"field": "hot"}])
    assert e.value.code == 4 and "vq_index_set_allreduce" in str(e.value)


# ------------------------------------------------------------------------------------------ f: threads
def test_eight_threads_on_one_shared_set(built):
    import veloci_amd
    idx = built["whole"][0]
    ids = FC.id_sets()["n4097"]
    ds = veloci_amd.DocSet(idx, ids)
    asked = [("zipf[]", 10), ("csr[]", None), ("hot", None), ("big[]", None), ("fit", 1024)]
    alone = ds.facets(json.loads(FC.json_of(asked)))
    assert alone == {f: FC.expected(f, ids, t) for f, t in asked}
    out, errs = [None] * 8, []

    def run(i):
        try:
            out[i] = [ds.facets(FC.json_of(asked)) for _ in range(5)]
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert all(g == alone for gs in out for g in gs)
