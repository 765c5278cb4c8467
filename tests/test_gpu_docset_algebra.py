"""Doc set algebra on the device (DocSet.combine and the operators, vq_docset_combine, k_setop_words / k_setop_probe / k_setop_clear): every case of
tests/docsetalgebracases.py on a whole index and on an unaligned shard, the image element for element against numpy's set operations restated by
tests/docsetref.py; both routes on the same inputs; sets that differ in one id at word, shard and index borders; operand lists longer than the
kernels' table; results as operands, as `within` and under searches through every entry point, held against DocSet(index, <numpy's ids>); the
export to a device tensor; misuse, lifetime and concurrent callers."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import countcorpus as CC
import docsetalgebracases as AC
import docsetfiltercases as FC
import docsetref as R

pytestmark = pytest.mark.gpu

N = AC.N
PARTS = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def env():
    import veloci_amd
    data = R.small_data()
    total = {"n": None, "calls": 0}

    def numpy_total(values):  # the shard's all-reduce hook: what numpy says the whole set holds
        assert values.size == 1
        total["calls"] += 1
        values[0] = total["n"]

    whole = veloci_amd.Index(data, device=0)
    shard = veloci_amd.Index(data, device=0, doc_lo=R.SHARD[0], doc_hi=R.SHARD[1])
    bare = veloci_amd.Index(data, device=0, doc_lo=R.SHARD[0], doc_hi=R.SHARD[1])  # a shard without the hook
    shard.set_allreduce(numpy_total)
    return {"whole": whole, "shard": shard, "bare": bare, "total": total, "sets": {"whole": {}, "shard": {}}, "keep": []}


def operand(env, which, o):
    """the DocSet of a case's operand on that index, made once"""
    import veloci_amd
    key = o if isinstance(o, str) else id(o)
    if not isinstance(o, str):
        env["keep"].append(o)  # (ids are keyed by identity: the arrays stay alive)
    sets = env["sets"][which]
    if key not in sets:
        sets[key] = veloci_amd.DocSet(env[which], AC.ids_of(o))
    return sets[key]


def combine(env, which, op, sets, want, no_probe=False):
    import veloci_amd
    env["total"]["n"] = len(want)
    if no_probe:
        os.environ["VQ_NO_SETOP_PROBE"] = "1"
    try:
        return veloci_amd.DocSet.combine(env[which], op, sets)
    finally:
        os.environ.pop("VQ_NO_SETOP_PROBE", None)


def run_cases(env, which, cases):
    idx = env[which]
    lo, hi = idx.doc_lo, idx.doc_hi
    routes = {0: 0, 1: 0}
    for name, op, operands in cases:
        want = AC.expected(op, operands)
        sets = [operand(env, which, o) for o in operands]
        ds = combine(env, which, op, sets, want)
        try:
            image = R.check(ds, want, N, lo, hi)
        except AssertionError as e:
            raise AssertionError("%s on %s: %s" % (name, which, e)) from e
        if image["bitmap"] is not None:  # no bit outside the doc range
            docs = np.flatnonzero(np.unpackbits(ds.part(1).view(np.uint8), bitorder="little")) + image["base"]
            assert docs.min() >= lo and docs.max() < hi, name
        route = AC.expected_route(op, operands, lo, hi)
        assert ds.route == route, (name, which, ds.route, route)
        routes[route] += 1
        if route:  # the same operands through the word route: the same image, part for part
            forced = combine(env, which, op, sets, want, no_probe=True)
            assert forced.route == 0, name
            for part in PARTS:
                assert np.array_equal(forced.part(part), ds.part(part)), (name, which, part)
            assert len(forced) == len(ds) and forced.local_len == ds.local_len and forced.device_bytes == ds.device_bytes, name
            forced.close()
        ds.close()
    return routes


# ------------------------------------------------------------------------------------------ 1, 2: the image, the routes
# (that the cases cover every kind of image and both routes is asserted without a GPU: tests/test_docset_algebra_cpu.py)
@pytest.mark.parametrize("which", ["whole", "shard"])
@pytest.mark.parametrize("op", AC.OPS)
def test_image_of_every_ordered_pair(env, op, which):
    routes = run_cases(env, which, [c for c in AC.pair_cases() if c[1] == op])
    print(routes)
    assert routes[0] + routes[1] == 81 and routes[0] > 0 and (routes[1] > 0) == (op != "or")


@pytest.mark.parametrize("which", ["whole", "shard"])
def test_image_of_the_complements(env, which):
    import veloci_amd
    idx = env[which]
    assert run_cases(env, which, AC.not_cases()) == {0: 9, 1: 0}
    none = combine(env, which, "not", [operand(env, which, "every")], [])
    assert len(none) == 0 and none.local_len == 0 and none.ids().size == 0
    env["total"]["n"] = N
    everything = ~operand(env, which, "empty")
    assert everything.local_len == idx.doc_hi - idx.doc_lo and len(everything) == N
    assert int(everything.ids()[-1]) == idx.doc_hi - 1 < N  # N is no multiple of 32: the tail bits of the last word stay clear
    for name in ("sparse", "dense", "edges"):
        a = operand(env, which, name)
        env["total"]["n"] = N - len(a)
        inverse = ~a
        env["total"]["n"] = len(a)
        back = ~inverse
        for part in PARTS:
            assert np.array_equal(back.part(part), a.part(part)), (name, part)
        assert len(back) == len(a) and back.device_bytes == a.device_bytes
    assert operand(env, which, "dense").route == -1
    assert isinstance(everything, veloci_amd.DocSet)


@pytest.mark.parametrize("which", ["whole", "shard"])
def test_sets_that_differ_in_one_id(env, which):
    routes = run_cases(env, which, AC.edge_cases())
    assert routes[0] and routes[1]


@pytest.mark.parametrize("which", ["whole", "shard"])
def test_more_operands_than_a_launch_takes(env, which):
    routes = run_cases(env, which, AC.nary_cases())
    assert routes[0] >= 8 and routes[1] >= 6, routes


def test_a_shard_without_the_hook_declines_and_a_whole_index_never_calls_it(env):
    import veloci_amd
    a = veloci_amd.DocSet(env["bare"], [70_500, 70_501])
    for op, sets in (("and", [a, a]), ("or", [a]), ("minus", [a, a]), ("not", [a])):
        with pytest.raises(veloci_amd.VelociError) as e:
            veloci_amd.DocSet.combine(env["bare"], op, sets)
        assert e.value.code == 4 and "vq_index_set_allreduce" in str(e.value)
    calls = []
    env["whole"].set_allreduce(lambda values: calls.append(1))
    try:
        R.check(operand(env, "whole", "sparse") | operand(env, "whole", "dense"), AC.expected("or", ["sparse", "dense"]), N, 0, N)
    finally:
        env["whole"].set_allreduce(None)
    assert not calls
    before = env["total"]["calls"]
    combine(env, "shard", "or", [operand(env, "shard", "sparse")], AC.ids_of("sparse"))
    assert env["total"]["calls"] == before + 1  # one u64 per combine on a shard


# ------------------------------------------------------------------------------------------ 3: composition
@pytest.mark.parametrize("which", ["whole", "shard"])
def test_results_compose(env, which):
    idx = env[which]
    lo, hi = idx.doc_lo, idx.doc_hi
    a, b, c = (operand(env, which, n) for n in ("medium", "repeated", "dense"))
    ab_ids = AC.expected("or", ["medium", "repeated"])
    want = np.setdiff1d(ab_ids, AC.ids_of("dense"))
    env["total"]["n"] = len(ab_ids)
    ab = a | b
    env["total"]["n"] = len(want)
    R.check(ab - c, want, N, lo, hi)
    R.check(ab.minus(c), want, N, lo, hi)
    # a probe-route result as the operand of a word-route combine and the other way round
    small = combine(env, which, "and", [operand(env, which, "sparse"), c], AC.expected("and", ["sparse", "dense"]))
    assert small.route == 1
    want = np.union1d(AC.expected("and", ["sparse", "dense"]), AC.ids_of("medium"))
    env["total"]["n"] = len(want)
    R.check(small | a, want, N, lo, hi)
    want = np.intersect1d(ab_ids, AC.expected("and", ["sparse", "dense"]))
    env["total"]["n"] = len(want)
    R.check(ab & small, want, N, lo, hi)


# ------------------------------------------------------------------------------------------ 4: search
@pytest.fixture(scope="module")
def corpus():
    import veloci_amd
    L, info = FC.corpus()
    data = CC.index_data(L)
    return {"L": L, "data": data, "idx": veloci_amd.Index(data, device=0)}


def set_recipes():
    """[(ids numpy expects, recipe(index) -> DocSet)]"""
    import veloci_amd
    L, _ = FC.corpus()
    d0, d5, d3, pmid = (FC.expected(CC.leaf(t)) for t in ("d0", "d5", "d3", "pmid"))
    extra = np.asarray(L["fsmall"], np.int64)
    return [
        (np.setdiff1d(d0, d5), lambda idx: veloci_amd.DocSet.from_filter(idx, CC.leaf("d0")) - veloci_amd.DocSet.from_filter(idx, CC.leaf("d5"))),
        (np.setdiff1d(np.union1d(d3, extra), pmid),
         lambda idx: (veloci_amd.DocSet.from_filter(idx, CC.leaf("d3")) | veloci_amd.DocSet(idx, extra)) & ~veloci_amd.DocSet.from_filter(idx, CC.leaf("pmid"))),
    ]


def search_requests():
    return [dict(search_req=sr, top=10) for sr in (CC.leaf("d1"), CC.AND(CC.leaf("d0"), CC.leaf("d1")), CC.OR(CC.leaf("d0"), CC.leaf("pmid")),
                                                    CC.AND(CC.leaf("d0"), CC.leaf("d1"), CC.leaf("d2")))]


def test_search_under_a_combined_set_equals_search_under_its_ids(corpus):
    import veloci_amd
    from parity import assert_same
    idx = corpus["idx"]
    reqs = search_requests()
    hits = 0
    for want, recipe in set_recipes():
        assert len(want) > 1000
        ds, base = recipe(idx), veloci_amd.DocSet(idx, want)
        R.check(ds, want, FC.N, 0, FC.N)
        baseline = [veloci_amd.search(r, idx, docset=base) for r in reqs]
        for r, w in zip(reqs, baseline):
            assert_same(r, veloci_amd.search(r, idx, docset=ds), w)
            hits += w.num_hits
        for r, g, w in zip(reqs, veloci_amd.search_batch(reqs, idx, docsets=[ds] * len(reqs)), baseline):
            assert_same(r, g, w)
        num_hits, counts, ids, scores, status = veloci_amd.search_batch_flat(reqs, idx, stride=16, docsets=[ds] * len(reqs))
        assert not status.any(), status
        for i, w in enumerate(baseline):
            n = int(counts[i])
            assert int(num_hits[i]) == w.num_hits and n == len(w.ids) and ids[i, :n].tolist() == w.ids.tolist(), i
            assert np.array_equal(scores[i, :n].view(np.uint32), w.scores.view(np.uint32)), i
        # as the `within` of from_filter
        inside = veloci_amd.DocSet.from_filter(idx, FC.WITHIN_FILTER, within=ds)
        R.check(inside, FC.expected(FC.WITHIN_FILTER, within=want), FC.N, 0, FC.N)
    assert hits > 1000
    assert veloci_amd.DocSet.from_filter(idx, CC.leaf("d0")).route == -1 and ds.route in (0, 1)  # no combine made the first, one made the second


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


def test_two_shards(corpus):
    import veloci_amd
    from veloci_amd.dist import search_shards_local
    from parity import assert_same
    data, idx = corpus["data"], corpus["idx"]
    cut = FC.N // 3 + 11
    shards = [veloci_amd.Index(data, device=0, doc_lo=0, doc_hi=cut), veloci_amd.Index(data, device=0, doc_lo=cut, doc_hi=FC.N)]
    recipes = set_recipes()
    barrier, hook = summing_hooks()
    per_shard, errs = [None, None], []

    def run(rank):
        try:
            shards[rank].set_allreduce(hook(rank))
            per_shard[rank] = [recipe(shards[rank]) for _, recipe in recipes]
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for s in shards:
        s.set_allreduce(None)
    reqs = search_requests()[:3]  # (no sums over the shards: the shards one after the other)
    for k, (want, _) in enumerate(recipes):
        assert len(per_shard[0][k]) == len(per_shard[1][k]) == len(want)
        assert np.array_equal(np.concatenate([per_shard[0][k].ids(), per_shard[1][k].ids()]), want)
        base = veloci_amd.DocSet(idx, want)
        got = search_shards_local(shards, reqs, docsets=[[per_shard[s][k]] * len(reqs) for s in (0, 1)])
        for r, g in zip(reqs, got):
            w = veloci_amd.search(r, idx, docset=base)
            assert w.num_hits > 0
            assert_same(r, g, w)


# ------------------------------------------------------------------------------------------ 5: export
@pytest.mark.parametrize("which", ["whole", "shard"])
def test_ids_as_a_device_tensor(env, which):
    import torch
    import veloci_amd
    idx = env[which]
    want = AC.expected("minus", ["dense", "medium"])
    ds = combine(env, which, "minus", [operand(env, which, "dense"), operand(env, which, "medium")], want)
    t = ds.ids_tensor()
    assert t.dtype == torch.int32 and t.is_cuda and t.device.index == idx.device and t.numel() == ds.local_len > 1000
    assert np.array_equal(t.cpu().numpy().view(np.uint32), ds.ids())
    again = veloci_amd.DocSet(idx, t)  # the way back in
    assert len(again) == ds.local_len
    for part in PARTS:
        assert np.array_equal(again.part(part), ds.part(part)), part
    assert combine(env, which, "and", [operand(env, which, "empty")], []).ids_tensor().numel() == 0
    L = veloci_amd.lib()
    few = np.full(8, 0xABABABAB, np.uint32)
    assert int(L.vq_docset_ids(ds._handle(), few.ctypes.data, 5, 0)) == ds.local_len
    assert np.array_equal(few[:5], ds.ids()[:5]) and few[5] == 0xABABABAB
    buf = torch.full((8,), -1, dtype=torch.int32, device=t.device)
    torch.cuda.synchronize()
    assert int(L.vq_docset_ids(ds._handle(), buf.data_ptr(), 5, 1)) == ds.local_len
    assert buf.cpu().tolist() == ds.ids()[:5].astype(np.int64).tolist() + [-1, -1, -1]


# ------------------------------------------------------------------------------------------ 6: misuse and lifetime
def test_misuse(env):
    import veloci_amd
    L = veloci_amd.lib()
    a, b = operand(env, "whole", "sparse"), operand(env, "whole", "dense")
    out = C.c_void_p()
    two = (C.c_void_p * 2)(a._handle(), b._handle())
    holed = (C.c_void_p * 2)(a._handle(), None)
    for op, sets, n in ((0, two, 0), (0, None, 0), (1, holed, 2), (4, two, 2), (-1, two, 2), (3, two, 2)):
        assert L.vq_docset_combine(env["whole"].h, op, sets, n, C.byref(out)) == 6 and not out.value, (op, n)
    assert L.vq_docset_combine(None, 0, two, 2, C.byref(out)) == 6 and L.vq_docset_combine(env["whole"].h, 0, two, 2, None) == 6
    with pytest.raises(veloci_amd.VelociError) as e:  # an operand of another index
        veloci_amd.DocSet.combine(env["shard"], "and", [operand(env, "shard", "dense"), a])
    assert e.value.code == 6 and e.value.kind == "InvalidArgument"
    with pytest.raises(ValueError):
        veloci_amd.DocSet.combine(env["whole"], "xor", [a, b])
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.DocSet.combine(env["whole"], "and", [])
    assert e.value.code == 6
    closed = veloci_amd.DocSet(env["whole"], [1, 2])
    closed.close()
    with pytest.raises(ValueError):
        a & closed
    assert L.vq_debug_docset_route(None) == -1 and L.vq_docset_ids(None, None, 0, 0) == 0


def test_a_result_outlives_its_operands(env):
    import veloci_amd
    idx = env["whole"]
    x, y = veloci_amd.DocSet(idx, AC.ids_of("dense")), veloci_amd.DocSet(idx, AC.ids_of("repeated"))
    both, either = y & x, x | y
    x.close()
    y.close()
    del x, y
    R.check(both, AC.expected("and", ["repeated", "dense"]), N, 0, N)
    R.check(either, AC.expected("or", ["dense", "repeated"]), N, 0, N)
    R.check(either - both, np.setdiff1d(AC.expected("or", ["dense", "repeated"]), AC.expected("and", ["repeated", "dense"])), N, 0, N)


def test_eight_threads_on_shared_operands(env):
    import veloci_amd
    idx = env["whole"]
    names = ("dense", "medium", "sparse", "repeated")
    sets = {n: operand(env, "whole", n) for n in names}
    jobs = [("and", ["dense", "medium"]), ("and", ["sparse", "dense"]), ("or", ["sparse", "medium"]), ("minus", ["dense", "medium", "sparse"]),
            ("minus", ["repeated", "dense"]), ("not", ["sparse"]), ("or", ["dense", "repeated", "sparse"]), ("and", ["repeated", "medium", "dense"])]
    want = [R.image(AC.expected(op, operands), N, 0, N) for op, operands in jobs]
    errs = []

    def run(k):
        try:
            op, operands = jobs[k]
            for _ in range(4):
                ds = veloci_amd.DocSet.combine(idx, op, [sets[n] for n in operands])
                assert len(ds) == want[k]["len"] and np.array_equal(ds.part(4), want[k]["padded"]), k
                assert (want[k]["bitmap"] is None and ds.part(1).size == 0) or np.array_equal(ds.part(1), want[k]["bitmap"]), k
                ds.close()
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
