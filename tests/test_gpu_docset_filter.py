"""Doc sets from a filter tree on the device (DocSet.from_filter, vq_docset_from_filter, k_filter_bits): the image element for element against the
numpy restatements (tests/countref.py for the ids, tests/docsetref.py for the image) on a whole index and on an unaligned shard; leaves numpy does
not restate (fuzzy, regex) against the oracle; searches under such a set against the oracle's answer to the same request with the tree as its
`filter`, bit for bit through every entry point; two shards on one GPU; misuse and lifetime.

The equivalence rule: the ids of from_filter(F, within=S) are exactly the ids the compiler's filter of a request with `filter: F` and doc set S
selects."""
import json
import threading

import numpy as np
import pytest

import countcorpus as CC
import docsetfiltercases as FC
import docsetref

pytestmark = pytest.mark.gpu

N = FC.N
IMAGE_CASES = FC.leaf_cases() + FC.tree_cases()


@pytest.fixture(scope="module")
def env():
    import veloci_amd
    from oracle import binding as O
    L, info = FC.corpus()
    data = CC.index_data(L)
    total = {"n": None}

    def numpy_total(values):  # the shard's all-reduce hook: what numpy says the whole set holds
        assert values.size == 1
        values[0] = total["n"]

    whole = veloci_amd.Index(data, device=0)
    shard = veloci_amd.Index(data, device=0, doc_lo=FC.SHARD[0], doc_hi=FC.SHARD[1])
    shard.set_allreduce(numpy_total)
    ora = data.load_into(O.OracleIndex(N))
    return {"L": L, "info": info, "data": data, "whole": whole, "shard": shard, "total": total, "ora": ora, "want": {}}


def wanted(env, req):
    """the oracle's answer, computed once per request and shared by the tests"""
    key = json.dumps(req, sort_keys=True)
    if key not in env["want"]:
        env["want"][key] = env["ora"].search_json(key)
    return env["want"][key]


def make(env, which, flt, within=None, want=None):
    """from_filter on the whole index or the shard; on the shard the hook answers with the size of `want`"""
    import veloci_amd
    env["total"]["n"] = None if want is None else len(want)
    return veloci_amd.DocSet.from_filter(env[which], flt, within=within)


# ------------------------------------------------------------------------------------------ 1: the image
def test_the_expected_sets_cover_every_kind_of_image():
    for lo, hi in ((0, N), FC.SHARD):
        seen = FC.assert_not_vacuous([FC.expected(f) for _, f in IMAGE_CASES], lo, hi)
        print(lo, hi, seen)
    L, _ = FC.corpus()
    assert FC.kinds(L["d0"]) == (True, True, False) and FC.kinds(L["pmid"]) == (False, True, False) and FC.kinds(L["pedge"]) == (False, False, False)
    assert FC.kinds(L["fempty"]) == (False, False, True)


@pytest.mark.parametrize("which", ["whole", "shard"])
@pytest.mark.parametrize("name", [n for n, _ in IMAGE_CASES])
def test_image_of_a_filter(env, name, which):
    flt = dict(IMAGE_CASES)[name]
    want = FC.expected(flt)
    idx = env[which]
    ds = make(env, which, flt, want=want)
    docsetref.check(ds, want, N, idx.doc_lo, idx.doc_hi)
    if which == "shard" and ds.part(1).size:  # no bit outside the shard
        docs = np.flatnonzero(np.unpackbits(ds.part(1).view(np.uint8), bitorder="little")) + (idx.doc_lo & ~65535)
        assert docs.min() >= idx.doc_lo and docs.max() < idx.doc_hi


@pytest.mark.parametrize("which", ["whole", "shard"])
@pytest.mark.parametrize("name", [n for n, _ in FC.within_cases()])
def test_image_of_a_filter_within_a_set(env, name, which):
    import veloci_amd
    ids = dict(FC.within_cases())[name]
    idx = env[which]
    want = FC.expected(FC.WITHIN_FILTER, within=ids)
    assert len(want) == len(np.intersect1d(np.intersect1d(env["L"]["d3"], env["L"]["d4"]), ids))
    within = veloci_amd.DocSet(idx, ids)
    docsetref.check(make(env, which, FC.WITHIN_FILTER, within=within, want=want), want, N, idx.doc_lo, idx.doc_hi)
    if name == "within-f100001":  # the set's bitmap image is what the kernel copies
        assert within.part(1).size
    if name == "within-fsmall":   # ... a tile directory and no bitmap
        assert within.part(3).size and not within.part(1).size


# ------------------------------------------------------------------------------------------ 2: leaves the numpy restatement refuses
@pytest.mark.parametrize("name,flt", [("fuzzy", CC.leaf("t1a", levenshtein_distance=1)), ("regex", CC.leaf("d[0-3]", is_regex=True))])
def test_fuzzy_and_regex_leaves_against_the_oracle(env, name, flt):
    w = wanted(env, {"search_req": CC.leaf("all"), "filter": flt, "top": N})
    want = np.sort(np.asarray(w.ids, np.int64))
    assert w.num_hits == len(want) > 900
    for which in ("whole", "shard"):
        idx = env[which]
        ds = make(env, which, flt, want=want)
        assert len(ds) == len(want)
        assert np.array_equal(ds.ids(), want[(want >= idx.doc_lo) & (want < idx.doc_hi)])


# ------------------------------------------------------------------------------------------ 3: search equivalence
def test_near_tie_cases_under_a_set_from_their_filter(env):
    import veloci_amd
    from parity import assert_same
    cases = [c for c in CC.near_tie_cases(env["L"], env["info"]) if c["filter"]]
    assert {c["filter"] for c in cases} >= {"f100000", "f100001"} and len(cases) >= 30
    sets = {f: veloci_amd.DocSet.from_filter(env["whole"], CC.leaf(f)) for f in ("f099999", "f100000", "f100001")}
    assert [len(sets[f]) for f in sorted(sets)] == [99_999, 100_000, 100_001]  # the two sides of the Set / Vec line and the line itself
    hits = 0
    for c in cases:
        req = {k: v for k, v in c["request"].items() if k != "filter"}
        got = veloci_amd.search(req, env["whole"], docset=sets[c["filter"]])
        assert_same(c["request"], got, wanted(env, c["request"]))
        hits += got.num_hits
    assert hits > 5000


def tree_requests():
    """[(request with its filter, request without it, the filter)] for count_requests()' filter-tree and depth3"""
    out = []
    for name, req, _ in CC.count_requests():
        if name in ("filter-tree", "depth3"):
            out.append((req, {k: v for k, v in req.items() if k != "filter"}, req["filter"]))
    assert len(out) == 2
    return out


def test_tree_filters_through_every_entry_point(env):
    import veloci_amd
    from parity import assert_same
    idx = env["whole"]
    reqs, sets = [], []
    for full, bare, flt in tree_requests():
        ds = veloci_amd.DocSet.from_filter(idx, flt)
        w = wanted(env, full)
        assert w.num_hits > 0
        assert_same(full, veloci_amd.search(bare, idx, docset=ds), w)
        reqs += [bare, full]
        sets += [ds, None]
    for full, g in zip([f for f, _, _ in tree_requests() for _ in (0, 1)], veloci_amd.search_batch(reqs, idx, docsets=sets)):
        assert_same(full, g, wanted(env, full))
    num_hits, counts, ids, scores, status = veloci_amd.search_batch_flat(reqs, idx, stride=16, docsets=sets)
    assert not status.any(), status
    for i, full in enumerate([f for f, _, _ in tree_requests() for _ in (0, 1)]):
        w = wanted(env, full)
        n = int(counts[i])
        assert int(num_hits[i]) == w.num_hits and n == len(w.ids) and ids[i, :n].tolist() == list(w.ids), (i, full)
        assert np.array_equal(scores[i, :n].view(np.uint32), np.asarray(w.scores, np.float32).view(np.uint32)), (i, full)


# ------------------------------------------------------------------------------------------ 4: two shards on one GPU
def summing_hooks():
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

    return barrier, hook


def on_both(shards, body):
    """body(rank) on a thread per shard, each with its summing hook; -> [result of rank 0, of rank 1]"""
    barrier, hook = summing_hooks()
    out, errs = [None, None], []

    def run(rank):
        try:
            shards[rank].set_allreduce(hook(rank))
            out[rank] = body(rank)
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    return out  # (the hooks stay: taking one off waits for the index's batches in flight, and body may have left one)


def test_two_shards(env):
    import veloci_amd
    from veloci_amd.dist import exchange_local, search_shards_local
    from parity import assert_same
    cut = N // 3 + 11
    shards = [veloci_amd.Index(env["data"], device=0, doc_lo=0, doc_hi=cut), veloci_amd.Index(env["data"], device=0, doc_lo=cut, doc_hi=N)]
    # without a sum over the shards a shard declines
    for s in shards:
        with pytest.raises(veloci_amd.VelociError) as e:
            veloci_amd.DocSet.from_filter(s, CC.leaf("d0"))
        assert e.value.code == 4 and "vq_index_set_allreduce" in str(e.value)
    trees = tree_requests()
    filters = [flt for _, _, flt in trees]
    per_shard = on_both(shards, lambda rank: [veloci_amd.DocSet.from_filter(shards[rank], f) for f in filters])
    for s in shards:
        s.set_allreduce(None)
    for k, flt in enumerate(filters):
        want = FC.expected(flt)
        assert len(per_shard[0][k]) == len(per_shard[1][k]) == len(want)
        assert per_shard[0][k].local_len + per_shard[1][k].local_len == len(want)
        assert np.array_equal(np.concatenate([per_shard[0][k].ids(), per_shard[1][k].ids()]), want)
    # requests whose compilation needs no sums over the shards: the shards one after the other
    plain = [(dict(search_req=sr, top=10, filter=flt), dict(search_req=sr, top=10), k)
             for k, flt in enumerate(filters) for sr in (CC.leaf("d0"), CC.AND(CC.leaf("d3"), CC.leaf("d4")), CC.OR(CC.leaf("d0"), CC.leaf("pmid")))]
    got = search_shards_local(shards, [bare for _, bare, _ in plain], docsets=[[per_shard[s][k] for _, _, k in plain] for s in (0, 1)])
    for (full, _, _), g in zip(plain, got):
        assert wanted(env, full).num_hits > 0
        assert_same(full, g, wanted(env, full))
    # the ANDs of three operands measure their operands inside the set first, summed over the shards: the shards side by side
    pbs = on_both(shards, lambda rank: veloci_amd.PartialBatch(shards[rank], [veloci_amd.Request(bare, docset=per_shard[rank][k]) for k, (_, bare, _) in enumerate(trees)]))
    g = exchange_local(pbs)
    got = pbs[0].merge(g.data_ptr(), 2)
    pbs[1].merge(None, 1)
    for s in shards:
        s.set_allreduce(None)
    for (full, _, _), res in zip(trees, got):
        assert_same(full, res, wanted(env, full))


# ------------------------------------------------------------------------------------------ 5: misuse and lifetime
def test_misuse(env):
    import veloci_amd
    other = veloci_amd.DocSet(env["whole"], [1, 2, 3])
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.DocSet.from_filter(env["shard"], CC.leaf("d0"), within=other)
    assert e.value.code == 6 and e.value.kind == "InvalidArgument"
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.DocSet.from_filter(env["whole"], '{"search": {"path": "body", ')
    assert e.value.code == 7
    nopath = {"search": {"path": "nofield", "terms": ["x"]}}
    with pytest.raises(veloci_amd.VelociError) as of_search:
        veloci_amd.search({"search_req": CC.leaf("all"), "filter": nopath}, env["whole"])
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.DocSet.from_filter(env["whole"], nopath)
    assert (e.value.code, str(e.value)) == (of_search.value.code, str(of_search.value))


def test_a_set_outlives_its_within_and_its_request(env):
    import veloci_amd
    from parity import assert_same
    idx = env["whole"]
    f1, f2 = CC.OR(CC.AND(CC.leaf("f100000"), CC.leaf("d5")), CC.leaf("fsmall")), CC.AND(CC.leaf("d3"), CC.leaf("d4"))
    within = veloci_amd.DocSet.from_filter(idx, f1)
    ds = veloci_amd.DocSet.from_filter(idx, f2, within=within)
    within.close()
    del within
    both = veloci_amd.DocSet.from_filter(idx, CC.AND(f1, f2))
    want = FC.expected(CC.AND(f1, f2))
    assert len(want) > 1000
    for which in (0, 1, 2, 3, 4):  # every part: two ways to the same set
        assert np.array_equal(ds.part(which), both.part(which)), which
    docsetref.check(ds, want, N, 0, N)
    full = {"search_req": CC.AND(CC.leaf("d0"), CC.leaf("d1")), "top": 10, "filter": CC.AND(f1, f2)}
    bare = {k: v for k, v in full.items() if k != "filter"}
    r = veloci_amd.Request(bare, docset=ds)
    assert_same(full, veloci_amd.search(r, idx), wanted(env, full))
    del r
    docsetref.check(ds, want, N, 0, N)
    assert_same(full, veloci_amd.search(bare, idx, docset=ds), wanted(env, full))
    r = veloci_amd.Request(bare, docset=ds)
    ds.close()  # the request keeps the set
    assert_same(full, veloci_amd.search(r, idx), wanted(env, full))
