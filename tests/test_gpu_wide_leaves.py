"""Leaves that match more than 4096 dictionary terms (prefix, fuzzy and regex leaves on a large dictionary): the dense union route
(veloci_amd/csrc/union_dense.hip) against the CPU oracle, bit-exact scores.  The oracle's time for one such leaf grows quadratically
with the number of matched terms, so the bulk runs on a 40 000-term corpus (about 11 k lists per first letter) and only two requests
on the 300 000-term one; oracle answers are cached per request."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
UNION = ("k_union<count>", "k_union<write>")
DENSE = ("k_union_dense_scatter", "k_union_dense_count", "k_union_dense_write")


class Corpus:
    def __init__(self, data, terms):
        import veloci_amd
        from oracle import binding as O
        self.data, self.terms = data, terms
        self.idx = veloci_amd.Index(data, device=0)
        self.ora = O.OracleIndex(data.num_anchors)
        data.load_into(self.ora)
        self.cache = {}

    def want(self, req):
        js = json.dumps(req)
        if js not in self.cache:
            self.cache[js] = self.ora.search_json(js)
        return self.cache[js]

    def check(self, req):
        import veloci_amd
        from parity import assert_same
        got = veloci_amd.search(req, self.idx)
        assert_same(req, got, self.want(req))
        return got

    def lists(self, prefix):
        return sum(1 for t in self.terms if t.startswith(prefix.encode()))


@pytest.fixture(scope="module")
def wide():
    import widecorpus
    return Corpus(*widecorpus.build(num_terms=40_000, num_docs=1_000_000))


def part(term, **kw):
    p = {"path": "body", "terms": [term], "starts_with": True}
    p.update(kw)
    return p


def leaf(term, **kw):
    return {"search": part(term, **kw)}


def launches(idx):
    return {k: v["launches"] for k, v in idx.profile_json()["kernels"].items()}


def test_single_wide_leaves(wide):
    assert min(wide.lists(c) for c in "abcd") > 2 * 4096 and 64 < wide.lists("ab") < 4096
    wide.idx.profile_enable()
    r = wide.check({"search_req": leaf("a"), "top": 10})
    assert r.num_hits > 100_000
    prof = launches(wide.idx)
    wide.idx.profile_enable(False)
    assert all(prof.get(k, 0) == 1 for k in DENSE) and not any(prof.get(k, 0) for k in UNION), prof
    wide.check({"search_req": leaf("a"), "top": 20, "skip": 5})
    wide.check({"search_req": leaf("a", ignore_case=False), "top": 10})
    wide.check({"search_req": leaf("A", ignore_case=False), "top": 10})  # nothing matches
    wide.check({"search_req": leaf("b", boost=1.5), "top": 10})
    r = wide.check({"search_req": leaf("b", boost=-2.0), "top": 10})  # negative values in the slab
    assert r.num_hits > 100_000 and (r.scores < 0).all()
    r = wide.check({"search_req": leaf("ab", levenshtein_distance=1), "top": 10})  # every term with a prefix within distance 1 of "ab"
    assert r.num_hits > 200_000
    r = wide.check({"search_req": {"search": {"path": "body", "terms": [".*[a-g]"], "is_regex": True}}, "top": 10})
    assert sum(1 for t in wide.terms if t[-1:] in b"abcdefg") > 4096 and r.num_hits > 100_000
    r = wide.check({"search_req": leaf("c"), "top": 10, "facets": [{"field": "cat", "top": 5}]})
    assert r.facets and len(r.facets["cat"]) == 5


def test_wide_leaves_in_trees_and_as_side_inputs(wide):
    import veloci_amd
    from parity import assert_same
    reqs = [{"search_req": {"and": {"queries": [leaf("a"), leaf("b")]}}, "top": 30},
            {"search_req": {"or": {"queries": [leaf("a"), leaf("b")]}}, "top": 30},
            {"search_req": {"and": {"queries": [leaf("a"), leaf("ab")]}}, "top": 30},  # wide AND narrow (k_union)
            {"search_req": {"or": {"queries": [leaf("d"), leaf("ab")]}}, "top": 30},
            # three run-time-sized operands: the summation order follows the merged lengths
            {"search_req": {"and": {"queries": [leaf("a"), leaf("ab", levenshtein_distance=1), leaf("c")]}}, "top": 30},
            {"search_req": leaf("ab"), "filter": leaf("a"), "top": 30},
            {"search_req": leaf("a"), "filter": leaf("ab"), "top": 30},
            {"search_req": leaf("ab"), "filter": leaf("c"), "top": 30},
            {"search_req": leaf("ab"), "boost_term": [part("a", boost=3.0)], "top": 30},
            {"search_req": leaf("a"), "boost_term": [part("b", boost=2.0)], "top": 30},
            {"search_req": leaf("a", boost=1.5), "top": 15, "skip": 3}]
    singles = [wide.check(r) for r in reqs]
    assert all(s.num_hits > 0 for s in singles)
    # one batch: the leaf "a" appears in seven requests and is merged once (one union job per leaf_union_key)
    wide.idx.profile_enable()
    batch = veloci_amd.search_batch(reqs + reqs[:2], wide.idx)
    prof = wide.idx.profile_json()
    wide.idx.profile_enable(False)
    for r, g, s in zip(reqs + reqs[:2], batch, singles + singles[:2]):
        assert_same(r, g, wide.want(r))
        assert g.ids.tolist() == s.ids.tolist() and np.array_equal(g.scores.view(np.uint32), s.scores.view(np.uint32))
    # 20 wide leaves in the batch, far fewer union jobs
    assert 4 <= prof["kernels"]["k_union_dense_scatter"]["queries"] <= 10, prof["kernels"]["k_union_dense_scatter"]
    # the same wide leaf twice in one batch: one union job
    wide.idx.profile_enable()
    twice = veloci_amd.search_batch([reqs[-1], dict(reqs[-1], top=40)], wide.idx)
    prof = wide.idx.profile_json()
    wide.idx.profile_enable(False)
    assert prof["kernels"]["k_union_dense_scatter"]["queries"] == 1 and prof["kernels"]["k_union_dense_scatter"]["launches"] == 1, prof["kernels"]
    assert_same(reqs[-1], twice[0], wide.want(reqs[-1]))
    assert_same(dict(reqs[-1], top=40), twice[1], wide.want(dict(reqs[-1], top=40)))


def test_boundary_4096_lists_stay_on_k_union_4097_take_the_dense_route(wide):
    assert wide.lists("zr") == 4096 and wide.lists("zq") == 4097
    idx = wide.idx
    idx.profile_enable()
    try:
        wide.check({"search_req": leaf("zr"), "top": 10})
        prof = launches(idx)
        assert all(prof.get(k, 0) > 0 for k in UNION) and not any(prof.get(k, 0) for k in DENSE), prof
        wide.check({"search_req": leaf("zq"), "top": 10})
        prof = idx.profile_json()["kernels"]
        assert all(prof[k]["launches"] == 1 for k in DENSE) and not any(k in prof and prof[k]["launches"] for k in UNION), prof
        # byte accounting: 6 B + one 4-byte atomic per posting and the slab's clear; 4 B per doc; 4 B per doc and 8 B per entry
        ta = wide.data.token_to_anchor_score["body.textindex.to_anchor_id_score"][0]
        ids = [i for i, t in enumerate(wide.terms) if t.startswith(b"zq")]
        postings = int(sum(int(ta[i + 1]) - int(ta[i]) for i in ids))
        slab = (wide.data.num_anchors + 2047) // 2048 * 2048 * 4
        assert prof["k_union_dense_scatter"]["layout_bytes"] == slab + 10 * postings and prof["k_union_dense_scatter"]["algorithmic_bytes"] == 6 * postings
        assert prof["k_union_dense_count"]["algorithmic_bytes"] == slab
        entries = (prof["k_union_dense_write"]["algorithmic_bytes"] - slab) // 8 - 8
        assert 0.9 * postings < entries <= postings, (entries, postings)
        wide.check({"search_req": {"and": {"queries": [leaf("zr"), leaf("zq", levenshtein_distance=1)]}}, "top": 10})
        wide.check({"search_req": {"or": {"queries": [leaf("zr"), leaf("zq")]}}, "top": 10})
    finally:
        idx.profile_enable(False)


def _over_shards(parts, reqs):
    """Doc-range shards of one index on one GPU, run in threads; the sums some requests need over all shards (merged list lengths: the
    AND summation order) go through vq_index_set_allreduce; partials gathered and merged."""
    import veloci_amd
    from veloci_amd.dist import exchange_local
    n = len(parts)
    barrier = threading.Barrier(n, timeout=300)
    slots, totals, pbs, errs = [None] * n, [None], [None] * n, []

    def make_hook(rank):
        def hook(values):
            slots[rank] = values.copy()
            barrier.wait()
            if rank == 0:
                totals[0] = np.sum(np.stack(slots), axis=0, dtype=np.uint64)
            barrier.wait()
            values[:] = totals[0]
            barrier.wait()
        return hook

    parsed = [veloci_amd.Request(r) for r in reqs]

    def run(rank):
        try:
            parts[rank].set_allreduce(make_hook(rank))
            pbs[rank] = veloci_amd.PartialBatch(parts[rank], parsed)
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    g = exchange_local(pbs)
    res = pbs[0].merge(g.data_ptr(), n, raise_on_error=True)
    for pb in pbs[1:]:
        pb.merge(None, 1, raise_on_error=False)
    return res


def test_wide_leaves_over_doc_range_shards(wide):
    import veloci_amd
    from parity import assert_same
    from veloci_amd.dist import search_shards_local
    N = wide.data.num_anchors
    plain = [{"search_req": leaf("a"), "top": 10},
             {"search_req": leaf("a"), "top": 20, "skip": 5},
             {"search_req": leaf("b", boost=-2.0), "top": 10},
             {"search_req": leaf("b", boost=1.5), "top": 10},
             {"search_req": leaf("ab", levenshtein_distance=1), "top": 10},
             {"search_req": leaf("c"), "top": 10, "facets": [{"field": "cat", "top": 5}]},
             {"search_req": {"or": {"queries": [leaf("a"), leaf("b")]}}, "top": 30},
             {"search_req": {"or": {"queries": [leaf("d"), leaf("ab")]}}, "top": 30},
             {"search_req": leaf("zq"), "top": 10}]
    summed = [{"search_req": {"and": {"queries": [leaf("a"), leaf("b")]}}, "top": 30},
              {"search_req": {"and": {"queries": [leaf("a"), leaf("ab")]}}, "top": 30},
              {"search_req": {"and": {"queries": [leaf("a"), leaf("ab", levenshtein_distance=1), leaf("c")]}}, "top": 30},
              {"search_req": leaf("ab"), "filter": leaf("a"), "top": 30},
              {"search_req": leaf("a"), "filter": leaf("ab"), "top": 30},
              {"search_req": leaf("ab"), "boost_term": [part("a", boost=3.0)], "top": 30}]
    for cuts in ((0, N // 4, N), (0, 10, N // 4, N)):  # ¼ and ¾ of the docs; then with a shard of 10 docs in front (few or no postings in range)
        parts = [veloci_amd.Index(wide.data, device=0, doc_lo=cuts[i], doc_hi=cuts[i + 1]) for i in range(len(cuts) - 1)]
        for r, g in zip(plain, search_shards_local(parts, plain)):
            assert_same(r, g, wide.want(r))
        for r, g in zip(plain + summed, _over_shards(parts, plain + summed)):
            assert_same(r, g, wide.want(r))
        for p in parts:
            p.close()


def test_contention_and_degenerate_shapes():
    import widecorpus
    rng = np.random.default_rng(23)
    # 1000 docs, 6000 non-empty lists under one prefix: every slab word is hit by hundreds of atomics
    lists = {"q%05d" % i: rng.choice(1000, size=int(rng.integers(20, 200)), replace=False) for i in range(6000)}
    lists.update({"n%03d" % i: rng.choice(1000, size=50, replace=False) for i in range(100)})
    c = Corpus(*widecorpus.crafted(1000, lists))
    r = c.check({"search_req": leaf("q"), "top": 10})
    assert r.num_hits == 1000  # the union is every doc
    c.check({"search_req": leaf("q", boost=-0.5), "top": 1000})
    c.check({"search_req": {"and": {"queries": [leaf("q"), leaf("n")]}}, "top": 20, "facets": [{"field": "cat", "top": 3}]})
    # 5000 lists of one posting each (and a few longer ones), distinct docs, docs up to the range's last
    docs = rng.permutation(300_000)
    lists = {"s%05d" % i: docs[i:i + 1] for i in range(5000)}
    lists["s99999"] = np.array([299_999])
    lists.update({"t%03d" % i: docs[5000 + 40 * i:5000 + 40 * (i + 1)] for i in range(200)})
    c = Corpus(*widecorpus.crafted(300_000, lists))
    r = c.check({"search_req": leaf("s"), "top": 10})
    assert 5000 <= r.num_hits <= 5001
    c.check({"search_req": leaf("s"), "top": 100, "skip": 4950})
    c.check({"search_req": {"or": {"queries": [leaf("s"), leaf("t")]}}, "top": 10})
    # all one-posting lists on the same doc; and one doc per list in list order (every doc of a 4100-doc index, one list each)
    c = Corpus(*widecorpus.crafted(5000, {"u%05d" % i: np.array([4999]) for i in range(4200)}))
    assert c.check({"search_req": leaf("u"), "top": 10}).num_hits == 1
    c = Corpus(*widecorpus.crafted(4100, {"v%05d" % i: np.array([i]) for i in range(4100)}))
    assert c.check({"search_req": leaf("v"), "top": 10}).num_hits == 4100


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import veloci_amd, widecorpus
data, terms = widecorpus.build(num_terms=300_000, num_docs=1_000_000, planted=False)
idx = veloci_amd.Index(data, device=0)
leaf = lambda t: {"search": {"path": "body", "terms": [t], "starts_with": True}}
reqs = [{"search_req": leaf("b"), "top": 50}, {"search_req": leaf("c"), "top": 50}, {"search_req": {"and": {"queries": [leaf("b"), leaf("c")]}}, "top": 50}]
idx.profile_enable()
out = [{"num_hits": int(g.num_hits), "ids": g.ids.tolist(), "scores": g.scores.view(np.uint32).tolist()} for g in veloci_amd.search_batch(reqs, idx)]
prof = idx.profile_json()["kernels"]
print("WIDE_CHILD " + json.dumps({"results": out, "dense_launches": prof["k_union_dense_scatter"]["launches"], "dense_jobs": prof["k_union_dense_scatter"]["queries"]}))
"""


def test_scale_80k_lists_and_slab_groups():
    import widecorpus
    c = Corpus(*widecorpus.build(num_terms=300_000, num_docs=1_000_000, planted=False))
    assert c.lists("a") > 70_000 and 64 < c.lists("ab") < 4096
    # the two oracle calls this corpus gets
    r = c.check({"search_req": leaf("a"), "top": 10})
    assert r.num_hits > 500_000
    c.check({"search_req": {"and": {"queries": [leaf("a"), leaf("ab")]}}, "top": 10})
    # two further wide leaves in one batch: a slab budget of 4 MB (a slab of 1 M docs: one group per job) against the default (one group).  The
    # budget is read once per process: children, one after the other
    outs = []
    for env in ({"VQ_UNION_DENSE_SLAB_MB": "4"}, {}):
        p = subprocess.run([sys.executable, "-c", CHILD, HERE], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "WIDE_CHILD " in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
        outs.append(json.loads(p.stdout.split("WIDE_CHILD ", 1)[1]))
    assert outs[0]["results"] == outs[1]["results"] and all(r["num_hits"] > 100_000 for r in outs[0]["results"])
    assert outs[0]["dense_jobs"] == outs[1]["dense_jobs"] == 2 and outs[0]["dense_launches"] == 2 and outs[1]["dense_launches"] == 1, outs


def test_dense_route_on_every_materialised_leaf_that_has_a_test():
    """VQ_UNION_DENSE_MIN=1 (read once per process: a child): every union job of the existing fuzzy / prefix parity tests goes through the dense
    kernels and must still equal the oracle."""
    select = "fuzzy or starts_with or leaf_top or bench_jmdict or config4_real_shape or unicode or random_requests_on_reference or 1n_boost"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_parity.py"), os.path.join(HERE, "test_gpu_unicode_fuzzy.py"), "-m", "gpu", "-q", "-x", "-k", select],
                       env=dict(os.environ, VQ_UNION_DENSE_MIN="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
