"""Doc sets on the device: the staged image element for element against a numpy restatement (tests/docsetref.py), on a whole index and on a
doc-range shard; searches restricted by a doc set against the CPU oracle's answer to the same request with the equivalent `filter` leaf — a field
`acl` whose text_id_to_anchor rows are the sets — bit for bit through every entry point (single, batch, flat batch, partial + merge over two
shards, the sharded step inside the library); lifetime and misuse."""
import json
import threading

import numpy as np
import pytest

import docsetref as R

pytestmark = pytest.mark.gpu

SET_SIZES = (0, 300, 9_000, 99_999, 100_001, 130_000)  # 99 999 / 100 001: the two sides of the reference's FilterResult::Set / Vec line


@pytest.fixture(scope="module")
def small():
    import veloci_amd
    data = R.small_data()
    return veloci_amd.Index(data, device=0), veloci_amd.Index(data, device=0, doc_lo=R.SHARD[0], doc_hi=R.SHARD[1])


@pytest.fixture(scope="module")
def lists():
    return R.id_lists()


# ------------------------------------------------------------------------------------------ 1, 2: the image
@pytest.mark.parametrize("name", ["empty", "one", "last", "every", "edges", "repeated", "sparse", "medium", "dense"])
def test_image_on_a_whole_index(small, lists, name):
    import veloci_amd
    idx = small[0]
    want = R.check(veloci_amd.DocSet(idx, lists[name]), lists[name], R.NUM_ANCHORS, 0, R.NUM_ANCHORS)
    assert (want["bitmap"] is not None) == (name in ("every", "medium", "dense")), name  # 64 x unique ids >= 200 003: the index's own rule
    assert (want["tile_dir"] is not None) == (name not in ("empty", "one", "last", "edges")), name


def test_image_from_a_device_tensor(small, lists):
    import torch
    import veloci_amd
    idx = small[0]
    ids = lists["dense"]
    for dtype in (torch.int32, torch.uint32):
        t = torch.from_numpy(ids.astype(np.int32)).to("cuda:0").view(dtype)
        R.check(veloci_amd.DocSet(idx, t), ids, R.NUM_ANCHORS, 0, R.NUM_ANCHORS)
    t = torch.from_numpy(ids.astype(np.int32)).to("cuda:0")
    for cut in (1, 2, 3):  # a view that starts 4, 8, 12 bytes behind a 16-byte boundary, with 1 to 3 ids behind the last whole vector
        R.check(veloci_amd.DocSet(idx, t[cut:len(ids) - 2 * cut]), ids[cut:len(ids) - 2 * cut], R.NUM_ANCHORS, 0, R.NUM_ANCHORS)
    R.check(veloci_amd.DocSet(idx, t[:2]), ids[:2], R.NUM_ANCHORS, 0, R.NUM_ANCHORS)  # shorter than one vector
    with pytest.raises(ValueError):
        veloci_amd.DocSet(idx, t[::2])
    with pytest.raises(ValueError):
        veloci_amd.DocSet(idx, t.to(torch.int64))


def test_ids_beyond_the_index_are_refused(small):
    import veloci_amd
    for idx in small:
        for bad, n_bad in (([5, R.NUM_ANCHORS, 7, R.NUM_ANCHORS + 9], 2), (np.arange(R.NUM_ANCHORS - 3, R.NUM_ANCHORS + 600), 600), ([0xFFFFFFFF], 1)):
            with pytest.raises(veloci_amd.VelociError) as e:
                veloci_amd.DocSet(idx, bad)
            assert e.value.code == 6 and e.value.kind == "InvalidArgument" and ("doc set: %d of the %d ids" % (n_bad, len(bad))) in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["empty", "one", "last", "every", "edges", "repeated", "sparse", "medium", "dense"])
def test_image_on_a_shard(small, lists, name):
    import veloci_amd
    idx = small[1]
    lo, hi = R.SHARD
    ds = veloci_amd.DocSet(idx, lists[name])
    want = R.check(ds, lists[name], R.NUM_ANCHORS, lo, hi)
    ids = np.unique(lists[name])
    assert len(ds) == ids.size and ds.local_len == int(((ids >= lo) & (ids < hi)).sum())  # len: the whole set; local: the shard's ids only
    assert want["base"] == 65536 < lo
    if want["bitmap"] is not None:
        docs = np.flatnonzero(np.unpackbits(ds.part(1).view(np.uint8), bitorder="little")) + want["base"]
        assert docs.min() >= lo and docs.max() < hi and np.array_equal(docs, ds.ids())  # no bit outside [doc_lo, doc_hi)
        rank = ds.part(2)
        assert rank[0] == 0 and rank[(lo - want["base"]) // 512] == 0 and rank[-1] == ds.local_len  # counted from the bitmap base, as the index's own lists


# ------------------------------------------------------------------------------------------ 3: search parity through the equivalence
@pytest.fixture(scope="module")
def corpus():
    import veloci_amd
    from veloci_amd import synth
    from oracle import binding as O
    spec = synth.SynthSpec(num_docs=300_000, num_terms=5000, triples=2, extra_probe_dfs=(1000, 30_000, 300_000), background_terms=40)
    data, meta = synth.generate(spec)
    rng = np.random.default_rng(77)
    offsets, anchors = data.token_to_anchor_score["body.textindex.to_anchor_id_score"][:2]
    a, b, c = meta.triples[0]
    tc = data.term_id("body.textindex", c)
    of_c = anchors[int(offsets[tc]):int(offsets[tc + 1])].astype(np.int64)
    rows = []
    for size in SET_SIZES:
        row = rng.choice(data.num_anchors, size=size, replace=False)
        if size == 300:  # half of the small set from the rarest probe term's docs: the restricted searches keep some hits
            row = np.unique(np.concatenate([rng.choice(of_c, size=150, replace=False), row]))[:300]
        rows.append(np.sort(row))
    assert [len(r) for r in rows] == list(SET_SIZES)
    acl_off = np.zeros(len(rows) + 1, np.uint64)
    acl_off[1:] = np.cumsum([len(r) for r in rows])
    acl_vals = np.concatenate(rows).astype(np.uint32)
    data.add_fst("acl.textindex", [b"g%d" % k for k in range(len(rows))])
    data.add_token_to_anchor_score("acl.textindex.to_anchor_id_score", acl_off, acl_vals, rng.integers(1, 200, size=len(acl_vals)).astype(np.uint32), None)
    data.add_key_value_store("acl.textindex.text_id_to_anchor", acl_off, acl_vals)
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    # every set handed over shuffled and with some ids twice
    shuffled = [rng.permutation(np.concatenate([r, r[: len(r) // 7]])) for r in rows]
    sets = [veloci_amd.DocSet(idx, s) for s in shuffled]
    for ds, r in zip(sets, rows):
        assert len(ds) == ds.local_len == len(r)
    return {"data": data, "meta": meta, "idx": idx, "ora": ora, "rows": rows, "shuffled": shuffled, "sets": sets, "want": {}}


def acl_leaf(k):
    return {"search": {"path": "acl", "terms": ["g%d" % k]}}


def requests(meta):
    from veloci_amd import synth
    a, b, c = meta.triples[0]
    d, e, f = meta.triples[1]
    leaf = lambda t, **kw: {"search": dict({"path": "body", "terms": [t]}, **kw)}
    sub = lambda ts: {"or": {"queries": [leaf(t) for t in ts]}}
    return [
        synth.req_single(meta.extra_probes[1]),
        synth.req_and([a, b, c]),  # the summation order follows the operands' sizes INSIDE a Set filter, their own sizes under a Vec filter
        synth.req_and([d, e, f], top=25),
        synth.req_or([a, b, c], top=20),
        {"search_req": {"and": {"queries": [sub([a, b]), sub([c, d])]}}, "top": 10},
        {"search_req": leaf(a, levenshtein_distance=1), "top": 10},
        synth.req_and([a, b], boost=[{"path": "pop", "boost_fun": "Multiply", "param": 1.0}]),
        synth.req_and_phrase_locality([a, b, c]),
        dict(synth.req_or([a, b]), text_locality=True, phrase_boosts=[{"search1": {"path": "body", "terms": [a]}, "search2": {"path": "body", "terms": [b]}}]),
        synth.req_and([a, b], facets=[{"field": "cat"}, {"field": "tags[]", "top": 5}]),
        synth.req_or([a, b, c], top=10, skip=10),
        synth.req_or([a, b, c], top=20, filter={"or": {"queries": [leaf(t) for t in meta.background[:20]]}}),
    ]


def oracle_form(req, k):
    """the request with the set as the reference would take it: one more filter leaf"""
    own = req.get("filter")
    return dict(req, filter=acl_leaf(k) if own is None else {"and": {"queries": [own, acl_leaf(k)]}})


def wanted(corpus, req, k):
    """the oracle's answer, computed once per (request, set) and shared by the tests"""
    key = (json.dumps(req, sort_keys=True), k)
    if key not in corpus["want"]:
        corpus["want"][key] = corpus["ora"].search_json(json.dumps(req if k is None else oracle_form(req, k)))
    return corpus["want"][key]


def test_search_with_a_doc_set_equals_the_oracle_with_the_filter_leaf(corpus):
    import veloci_amd
    from parity import assert_same
    hits = 0
    for k, ds in enumerate(corpus["sets"]):
        for req in requests(corpus["meta"]):
            got = veloci_amd.search(req, corpus["idx"], docset=ds)
            assert_same(oracle_form(req, k), got, wanted(corpus, req, k))
            hits += got.num_hits
            if k == 0:
                assert got.num_hits == 0 and len(got.ids) == 0  # the empty set: the empty row's path
    assert hits > 10_000
    # ... and the product's own filter-leaf form takes the same path as the doc-set form (the empty row included)
    for k in (0, 1, 3, 4):
        for req in requests(corpus["meta"])[:4]:
            assert_same(oracle_form(req, k), veloci_amd.search(oracle_form(req, k), corpus["idx"]), wanted(corpus, req, k))


def test_batch_with_mixed_sets_and_none(corpus):
    import veloci_amd
    from parity import assert_same
    reqs, ks = [], []
    for i, req in enumerate(requests(corpus["meta"]) * 3):
        reqs.append(req)
        ks.append([0, 1, None, 2, 3, 4, None, 5][(i * 3 + i // 12) % 8])
    got = veloci_amd.search_batch(reqs, corpus["idx"], docsets=[None if k is None else corpus["sets"][k] for k in ks])
    assert len(set(ks)) == 7
    for req, k, g in zip(reqs, ks, got):
        assert_same(req if k is None else oracle_form(req, k), g, wanted(corpus, req, k))


def test_flat_batch_with_sets(corpus):
    import veloci_amd
    reqs, ks = [], []
    for i, req in enumerate(requests(corpus["meta"]) * 2):
        reqs.append({key: v for key, v in req.items() if key != "facets"})
        ks.append([5, None, 4, 3, 1, 2, 0][i % 7])
    stride = 32
    num_hits, counts, ids, scores, status = veloci_amd.search_batch_flat(reqs, corpus["idx"], stride=stride, docsets=[None if k is None else corpus["sets"][k] for k in ks])
    assert not status.any(), status
    for i, (req, k) in enumerate(zip(reqs, ks)):
        w = wanted(corpus, req, k)
        n = int(counts[i])
        assert int(num_hits[i]) == w.num_hits and n == len(w.ids) and ids[i, :n].tolist() == list(w.ids), (i, k, req)
        assert np.array_equal(scores[i, :n].view(np.uint32), np.asarray(w.scores, np.float32).view(np.uint32)), (i, k, req)


def needs_sums_over_shards(req):
    """an AND of three operands under a filter: the operands' sizes inside the filter are measured first and summed over the shards"""
    return "and" in req["search_req"] and len(req["search_req"]["and"]["queries"]) > 2


@pytest.fixture(scope="module")
def two_shards(corpus):
    import veloci_amd
    data = corpus["data"]
    cut = data.num_anchors // 3 + 11
    shards = [veloci_amd.Index(data, device=0, doc_lo=0, doc_hi=cut), veloci_amd.Index(data, device=0, doc_lo=cut, doc_hi=data.num_anchors)]
    return shards, [[veloci_amd.DocSet(s, ids) for ids in corpus["shuffled"]] for s in shards]


def test_two_shards_with_sets(corpus, two_shards):
    import veloci_amd
    from veloci_amd.dist import exchange_local, search_shards_local
    from parity import assert_same
    shards, per_shard = two_shards
    for s in shards:
        s.set_allreduce(None)
    for k, row in enumerate(corpus["rows"]):
        assert [len(per_shard[s][k]) for s in (0, 1)] == [len(row)] * 2 and sum(per_shard[s][k].local_len for s in (0, 1)) == len(row)
    every = [(req, k) for k in (None, 0, 1, 2, 3, 4, 5) for req in requests(corpus["meta"])]
    plain = [(req, k) for req, k in every if k is None or not needs_sums_over_shards(req)]
    summed = [(req, k) for req, k in every if k is not None and needs_sums_over_shards(req)]
    assert len(plain) >= 50 and len(summed) >= 18
    got = search_shards_local(shards, [req for req, _ in plain], docsets=[[None if k is None else per_shard[s][k] for _, k in plain] for s in (0, 1)])
    for (req, k), g in zip(plain, got):
        assert_same(req if k is None else oracle_form(req, k), g, wanted(corpus, req, k))
    # Without a sum over the shards a shard declines the ANDs of three operands under a set, as it declines them under the filter leaf ...
    for form in (veloci_amd.Request(summed[0][0], docset=per_shard[0][1]), veloci_amd.Request(oracle_form(summed[0][0], 1))):
        with pytest.raises(veloci_amd.VelociError) as e:
            veloci_amd.search(form, shards[0])
        assert e.value.code == 4 and "vq_index_set_allreduce" in str(e.value)
    # ... and with one (the shards run side by side and add up their counts) they answer like the oracle
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

    pbs, errs = [None, None], []

    def run(rank):
        try:
            shards[rank].set_allreduce(hook(rank))
            pbs[rank] = veloci_amd.PartialBatch(shards[rank], [veloci_amd.Request(req, docset=per_shard[rank][k]) for req, k in summed])
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    g = exchange_local(pbs)
    got = pbs[0].merge(g.data_ptr(), 2)
    pbs[1].merge(None, 1)
    for (req, k), res in zip(summed, got):
        assert_same(oracle_form(req, k), res, wanted(corpus, req, k))
    for s in shards:
        s.set_allreduce(None)


def test_sharded_step_inside_the_library_with_sets(corpus, two_shards):
    """vq_shard_step_begin / _end over the two shards, one thread each, the exchange handed in through vq_comm_init_custom: every request under
    every set and without one in ONE step; each rank attaches the sets it built on its own shard.  The request objects are dropped before the
    step ends: the step keeps the sets alive."""
    import veloci_amd
    from veloci_amd.dist import LocalExchange, shard_step_begin, shard_step_end
    shards, per_shard = two_shards
    every = [(req, k) for k in (None, 0, 1, 2, 3, 4, 5) for req in requests(corpus["meta"])]
    ex = LocalExchange(shards)
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

    outs, errs = [None, None], []

    def run(rank):
        try:
            shards[rank].set_allreduce(hook(rank))
            sets = [veloci_amd.DocSet(shards[rank], corpus["shuffled"][k]) if k is not None else None for _, k in every]  # handles of this step's own
            batch = veloci_amd.RequestBatch([req for req, _ in every], docsets=sets)
            for ds in sets:
                if ds is not None:
                    ds.close()
            step = shard_step_begin(shards[rank], batch)
            outs[rank] = shard_step_end(step, 32)
        except Exception as ex_:  # noqa: BLE001
            errs.append(repr(ex_))
            barrier.abort()
            ex.barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for rank in (0, 1):  # every rank holds the merged result
        num_hits, counts, ids, scores, status = outs[rank]
        assert not status.any(), status
        for i, (req, k) in enumerate(every):
            w = wanted(corpus, req, k)
            n = int(counts[i])
            assert int(num_hits[i]) == w.num_hits and n == len(w.ids) and ids[i, :n].tolist() == list(w.ids), (rank, i, k, req)
            assert np.array_equal(scores[i, :n].view(np.uint32), np.asarray(w.scores, np.float32).view(np.uint32)), (rank, i, k, req)
    for s in shards:
        veloci_amd.lib().vq_comm_destroy(s.h)
        s.set_allreduce(None)


# ------------------------------------------------------------------------------------------ 4: lifetime and misuse
def test_a_request_keeps_its_set_and_a_set_keeps_to_its_index(corpus, small):
    import veloci_amd
    from parity import assert_same
    idx = corpus["idx"]
    req = requests(corpus["meta"])[3]
    r = veloci_amd.Request(req)
    before = r.to_json()
    ds = veloci_amd.DocSet(idx, corpus["shuffled"][2])
    r.set_docset(ds)
    assert r.to_json() == before and json.loads(before)["filter"] is None
    ds.close()
    with pytest.raises(ValueError):
        len(ds)
    for _ in range(2):
        assert_same(oracle_form(req, 2), veloci_amd.search(r, idx), wanted(corpus, req, 2))
    # a set of another index: that request alone fails
    other = veloci_amd.DocSet(small[0], [1, 2, 3])
    got = veloci_amd.search_batch([req, req, req], idx, raise_on_error=False, docsets=[corpus["sets"][1], other, None])
    assert isinstance(got[1], veloci_amd.VelociError) and got[1].code == 6
    assert_same(oracle_form(req, 1), got[0], wanted(corpus, req, 1))
    assert_same(req, got[2], wanted(corpus, req, None))
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.search(req, idx, docset=other)
    assert e.value.code == 6 and "another index" in str(e.value)
    r.set_docset(None)  # detached: the plain request again
    assert_same(req, veloci_amd.search(r, idx), wanted(corpus, req, None))
