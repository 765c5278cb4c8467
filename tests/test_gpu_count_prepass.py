"""The count pre-pass (k_tile_scan in count mode) on the device: every number it measures against a numpy restatement (tests/countref.py, pinned
on the oracle by tests/test_count_ref_cpu.py), read through vq_debug_node_counts, and the three decisions the compiler takes from those numbers —
the summation order of an AND, the label of an AND inside an OR, the Set / Vec line of the filter — at operand sizes one apart, bit for bit
against the CPU oracle through every entry point.  All comparisons are integer equality.

The corpus is tests/countcorpus.py's: 201 608 docs (six tiles of 32768 and one of 5000), lists from numpy; tests/test_count_ref_cpu.py checks that
the lists have the shapes they were built for and that every near-tie case changes the oracle's answer when one doc moves.  Which request is
compiled with which bitmap width and how many spans is read from the entry point, not assumed: the tests assert that 64, 128 and 256 words and
several spans occurred."""
import json
import threading

import numpy as np
import pytest

import countcorpus as CC
import countref

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4
SET_TERMS = ("fsmall", "f100000", "f100001", "fempty")
COUNT_KERNEL = "k_tile_scan<count pre-pass>"
CUT = CC.N // 2 + 1000  # where the two shards meet: no tile boundary of any width


@pytest.fixture(scope="module")
def world():
    import veloci_amd
    L, info = CC.build_lists()
    data = CC.index_data(L)
    from oracle import binding as O
    ora = data.load_into(O.OracleIndex(CC.N))
    idx = veloci_amd.Index(data, device=0)
    idx.profile_enable(True)
    rng = np.random.default_rng(5)
    shuffled = {t: rng.permutation(np.concatenate([L[t], L[t][: len(L[t]) // 9]])) for t in SET_TERMS}  # any order, some ids twice
    sets = {t: veloci_amd.DocSet(idx, shuffled[t]) for t in SET_TERMS}
    assert CUT % 2048 != 0 and L["s0only"].max() < CUT <= L["s1only"].min()
    return {"L": L, "info": info, "lists": {"body": L}, "data": data, "ora": ora, "idx": idx, "sets": sets, "shuffled": shuffled, "alone": {}, "want": {}, "values": {},
            "cases": CC.near_tie_cases(L, info)}


@pytest.fixture(scope="module")
def shards(world):
    import veloci_amd
    two = [veloci_amd.Index(world["data"], device=0, doc_lo=0, doc_hi=CUT), veloci_amd.Index(world["data"], device=0, doc_lo=CUT, doc_hi=CC.N)]
    return two, [{t: veloci_amd.DocSet(s, world["shuffled"][t]) for t in SET_TERMS} for s in two]


def on_both_shards(two, body, unhook=True):
    """body(rank) on a thread per shard, the shards' sums wired to each other (vq_index_set_allreduce) -> [result of rank 0, of rank 1].
    unhook=False leaves the hooks in place: vq_index_set_allreduce waits until no batch of the index holds a workspace, so a caller whose body
    returns partials that are still to be merged takes the hooks off itself, after the merge."""
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

    out, errs = [None, None], []

    def run(rank):
        try:
            two[rank].set_allreduce(hook(rank))
            out[rank] = body(rank)
        except Exception as ex:  # noqa: BLE001
            errs.append(repr(ex))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(rank,)) for rank in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if unhook or errs:
        for s in two:
            s.set_allreduce(None)
    assert not errs, errs
    return out


# ------------------------------------------------------------------------------------------------------------------------ the counts
def matched_lists(part, L):
    """posting lists with entries that the leaf matches"""
    term = part["terms"][0]
    return sum(1 for t, d in L.items() if len(d) and (t.startswith(term) if part.get("starts_with") else t == term))


def expected_measured(req, L, filtered):
    """The node ids the compiler has measured (compile.cpp: apply_counts and the AND branch of compile_node_inner): the operands of every AND of
    three or more operands whose result size is not known before the request runs — and those of the ANDs of two as well when some OR needs the
    label of such an AND (its own operand, or the first operand of an OR below it).  Known: a leaf of at most one posting list, or one
    materialised first (more than 4 lists, or more than one beside an AND of three), in a request without a filter."""
    def wide(node):
        if "search" in node:
            return False
        kind = "and" if "and" in node else "or"
        return (kind == "and" and len(node[kind]["queries"]) >= 3) or any(wide(q) for q in node[kind]["queries"])

    has_wide = wide(req["search_req"])
    out, maybe, counter, label_wanted = set(), set(), [0], [False]

    def leaf_known(part):
        n = matched_lists(part, L)
        materialised = n > 4 or (n > 1 and has_wide)
        return (materialised or n <= 1) and not filtered

    def walk(node):
        """-> (node id of the result, size known, label known)"""
        my = counter[0]
        counter[0] += 1
        if "search" in node:
            return my, leaf_known(node["search"]), True
        kind = "and" if "and" in node else "or"
        ch = [walk(q) for q in node[kind]["queries"]]
        if len(ch) == 0:
            return my, True, False
        if len(ch) == 1:
            return ch[0]
        if kind == "or":
            label_wanted[0] = label_wanted[0] or not all(lab for _, _, lab in ch)
            return my, False, ch[0][2]
        (out if len(ch) >= 3 else maybe).update(i for i, known, _ in ch if not known)
        return my, False, all(known for _, known, _ in ch) and all(lab for _, _, lab in ch)

    walk(req["search_req"])
    return out | maybe if label_wanted[0] else out


def check_counts(world, name, req, docset, got, lo=0, hi=None):
    """one request's numbers from the entry point against the reference (restricted to [lo, hi) for a shard's own numbers)"""
    L = world["L"]
    ids = L[docset] if docset is not None else None
    ref, fsize = countref.node_counts(req, world["lists"], docset=ids, lo=lo, hi=hi)
    filtered = fsize is not None
    if name.startswith("plain"):
        assert got["status"] == -1 and got["nodes"] == [] and got["n_spans"] == 0 and got["tile_words"] == 0, (name, got)
        return
    assert got["status"] == 0, (name, got)
    assert got["has_filter"] == filtered and got["filter_count"] == (fsize or 0), (name, got["filter_count"], fsize)
    measured = [n for n, _, _ in got["nodes"]]
    assert set(measured) == expected_measured(req, L, filtered) and len(set(measured)) == len(measured), (name, measured)
    for node, hits, inside in got["nodes"]:
        assert hits == ref[node][0], (name, node, hits, ref[node])
        assert inside == (ref[node][1] if filtered else 0), (name, node, inside, ref[node])
    assert got["tile_words"] in (64, 128, 256) and got["n_spans"] >= 1, (name, got)


def alone(world, k):
    """the numbers of count request k sent alone (computed once)"""
    import veloci_amd
    if k not in world["alone"]:
        name, req, docset = CC.count_requests()[k]
        world["alone"][k] = veloci_amd.debug_node_counts([req], world["idx"], docsets=[world["sets"][docset] if docset else None])[0]
    return world["alone"][k]


def test_every_shape_alone_equals_the_reference(world):
    reqs = CC.count_requests()
    widths, spans, filters = set(), set(), set()
    for k, (name, req, docset) in enumerate(reqs):
        world["idx"].profile_json(reset=True)
        got = alone(world, k)
        kernels = world["idx"].profile_json(reset=True)["kernels"]
        check_counts(world, name, req, docset, got)
        assert not any(kn.startswith("k_scan") or (kn.startswith("k_tile_scan") and kn != COUNT_KERNEL) for kn in kernels), (name, sorted(kernels))  # no result scan
        if got["status"] == 0:
            assert kernels[COUNT_KERNEL]["launches"] == 1 and kernels[COUNT_KERNEL]["queries"] == 1, (name, kernels)
            widths.add(got["tile_words"])
            spans.add(got["n_spans"])
            filters.add(got["filter_count"])
            assert any(h for _, h, _ in got["nodes"]) or name in ("filter-empty",), name
        else:
            assert COUNT_KERNEL not in kernels, name
    assert widths == {64, 128, 256}, widths       # every bitmap width of the count query
    assert len(spans) >= 2 and max(spans) >= 2, spans  # several spans, and more than one span count
    assert {0, 99_999, 100_000, 100_001} <= filters, filters  # the empty filter and both sides of the Set / Vec line, exactly


def test_a_batch_gives_every_request_the_numbers_it_gets_alone(world):
    """counted and uncounted requests interleaved in one call: every query finds its own counters"""
    import veloci_amd
    reqs = CC.count_requests()
    plain = [k for k, r in enumerate(reqs) if r[0].startswith("plain")]
    counted = [k for k, r in enumerate(reqs) if not r[0].startswith("plain")]
    order = []
    for i, k in enumerate(reversed(counted)):  # c p c c p c c p c ... : an uncounted one behind every second counted one, and one in front
        if i % 2 == 1 or i == 0:
            order.append(plain[(i // 2) % len(plain)])
        order.append(k)
    order += counted[:5]  # (some requests twice)
    assert len(order) > len(reqs) and order[0] in plain and order[1] in counted
    got = veloci_amd.debug_node_counts([reqs[k][1] for k in order], world["idx"], docsets=[world["sets"][reqs[k][2]] if reqs[k][2] else None for k in order])
    for k, g in zip(order, got):
        assert g == alone(world, k), (reqs[k][0], g, alone(world, k))


def test_the_near_tie_requests_are_counted_as_their_builder_says(world):
    """the sizes the decisions of T1 - T5 rest on, as the kernel counts them: one apart"""
    import veloci_amd
    cases = world["cases"]
    got = veloci_amd.debug_node_counts([{k: v for k, v in c["request"].items() if not (c["docset"] and k == "filter")} for c in cases], world["idx"],
                                       docsets=[world["sets"][c["docset"]] if c["docset"] else None for c in cases])
    for c, g in zip(cases, got):
        if c["name"].startswith("T2-plain"):  # without a filter the unions are materialised first and their lengths are the sizes: nothing to count
            assert g["status"] == -1, (c["name"], g)
            continue
        assert g["status"] == 0 and g["has_filter"] == (c["filter"] is not None), (c["name"], g)
        assert g["filter_count"] == {None: 0, "f100000": 100_000, "f100001": 100_001}[c["filter"]], c["name"]
        ids = [node for node, sub in countref.sub_requests(c["request"]) if any(sub is op for op in c["operands"])]
        by_node = {n: (h, i) for n, h, i in g["nodes"]}
        which = 1 if c["filter"] == "f100000" else 0
        # (T3's leaf operand is not measured: without a filter its size is its list's length)
        measured = [(i, s) for i, s in zip(ids, c["sizes"]) if i in by_node]
        assert len(measured) >= 2 and [by_node[i][which] for i, _ in measured] == [s for _, s in measured], (c["name"], g["nodes"], c["sizes"])


def test_the_limit_of_measured_operands(world):
    """127 measured operands use 255 counters, all the candidate area holds; 128 are declined before anything is launched"""
    import veloci_amd
    idx = world["idx"]
    req = CC.limit_request(127)
    idx.profile_json(reset=True)
    got = veloci_amd.debug_node_counts([req], idx)[0]
    assert got["status"] == 0 and [n for n, _, _ in got["nodes"]] and sorted(n for n, _, _ in got["nodes"]) == list(range(1, 128)), got
    ref, fsize = countref.node_counts(req, world["lists"])
    assert got["filter_count"] == fsize == 100_000
    for node, hits, inside in got["nodes"]:
        assert (hits, inside) == ref[node], (node, hits, inside, ref[node])
    assert sum(1 for _, h, _ in got["nodes"] if h) >= 45 and idx.profile_json(reset=True)["kernels"][COUNT_KERNEL]["launches"] == 1
    over = veloci_amd.debug_node_counts([CC.limit_request(128)], idx)[0]
    assert over["status"] == UNSUPPORTED and over["nodes"] == [] and over["n_spans"] == 0, over
    assert COUNT_KERNEL not in idx.profile_json(reset=True)["kernels"]
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.search(CC.limit_request(128), idx)
    assert e.value.code == UNSUPPORTED and "127" in str(e.value)
    # ... and beside it in a batch the 127 are counted as alone
    both = veloci_amd.debug_node_counts([CC.limit_request(128), req, CC.count_requests()[0][1]], idx)
    assert both[0]["status"] == UNSUPPORTED and both[1] == got and both[2] == alone(world, 0)


def test_two_shards_count_their_own_docs_and_sum_to_the_whole(world, shards):
    import veloci_amd
    two, per_shard = shards
    reqs = [r for r in CC.count_requests() if not r[0].startswith("plain")] + [("T4-label", world["cases"][-1]["request"], None)]
    whole = veloci_amd.debug_node_counts([r[1] for r in reqs], world["idx"], docsets=[world["sets"][r[2]] if r[2] else None for r in reqs])

    def body(rank):
        sets = [per_shard[rank][r[2]] if r[2] else None for r in reqs]
        local = veloci_amd.debug_node_counts([r[1] for r in reqs], two[rank], summed=False, docsets=sets)
        return local, veloci_amd.debug_node_counts([r[1] for r in reqs], two[rank], summed=True, docsets=sets)

    (local0, summed0), (local1, summed1) = on_both_shards(two, body)
    zero_somewhere = 0
    for k, (name, req, docset) in enumerate(reqs):
        check_counts(world, name, req, docset, local0[k], lo=0, hi=CUT)
        check_counts(world, name, req, docset, local1[k], lo=CUT, hi=CC.N)
        w = whole[k]
        assert [n for n, _, _ in local0[k]["nodes"]] == [n for n, _, _ in local1[k]["nodes"]] == [n for n, _, _ in w["nodes"]], name
        assert [(n, a + c, b + d) for (n, a, b), (_, c, d) in zip(local0[k]["nodes"], local1[k]["nodes"])] == w["nodes"], name
        assert local0[k]["filter_count"] + local1[k]["filter_count"] == w["filter_count"], name
        for s in (summed0[k], summed1[k]):  # after the sum over the shards: the unsharded numbers, on every rank
            assert s["status"] == 0 and s["nodes"] == w["nodes"] and s["filter_count"] == w["filter_count"] and s["has_filter"] == w["has_filter"], (name, s, w)
        zero_somewhere += any(a == 0 and c > 0 or c == 0 and a > 0 for (_, a, _), (_, c, _) in zip(local0[k]["nodes"], local1[k]["nodes"]))
    assert zero_somewhere >= 2  # lists that lie in one shard only


# ------------------------------------------------------------------------------------------------------------------------ the decisions
def product_form(world, case, sets=None):
    """(request, doc set) as the product takes the case: T5 hands the filter's ids over as a doc set"""
    sets = world["sets"] if sets is None else sets
    if case["docset"]:
        return {k: v for k, v in case["request"].items() if k != "filter"}, sets[case["docset"]]
    return case["request"], None


def wanted(world, case):
    if case["name"] not in world["want"]:
        w = world["ora"].search_json(json.dumps(case["request"]))
        assert 0 < w.num_hits == len(w.ids) < 1024  # every hit is returned: every hit's score bits are compared
        world["want"][case["name"]] = w
    return world["want"][case["name"]]


def test_every_near_tie_case_depends_on_the_order(world):
    """numpy precondition: the reference's summation order and the one a count off by one would select give different f32 bits for some hit
    (T4, the label: test_count_ref_cpu.py shows the oracle's answer change by a factor when the sizes swap)"""
    shares = []
    for case in world["cases"]:
        if case["label"]:
            continue
        hits, differ, expected = CC.order_precondition(world["ora"], case, world["values"])
        assert hits == wanted(world, case).num_hits and differ >= 1, (case["name"], hits, differ)
        shares.append(differ / hits)
    assert len(shares) == 37 and min(shares) >= 0.1, shares


def test_single_requests_equal_the_oracle(world):
    import veloci_amd
    from parity import assert_same
    for case in world["cases"]:
        req, ds = product_form(world, case)
        assert_same(case["request"], veloci_amd.search(req, world["idx"], docset=ds), wanted(world, case))


def test_batch_equals_the_oracle(world):
    import veloci_amd
    from parity import assert_same
    forms = [product_form(world, c) for c in world["cases"]]
    for case, got in zip(world["cases"], veloci_amd.search_batch([f[0] for f in forms], world["idx"], docsets=[f[1] for f in forms])):
        assert_same(case["request"], got, wanted(world, case))


def check_flat(world, out, where):
    num_hits, counts, ids, scores, status = out
    assert not status.any(), (where, status)
    for i, case in enumerate(world["cases"]):
        w = wanted(world, case)
        n = int(counts[i])
        assert int(num_hits[i]) == w.num_hits and n == len(w.ids) and ids[i, :n].tolist() == list(w.ids), (where, case["name"])
        assert np.array_equal(scores[i, :n].view(np.uint32), np.asarray(w.scores, np.float32).view(np.uint32)), (where, case["name"])


def test_flat_batch_equals_the_oracle(world):
    import veloci_amd
    forms = [product_form(world, c) for c in world["cases"]]
    check_flat(world, veloci_amd.search_batch_flat([f[0] for f in forms], world["idx"], stride=CC.ALL, docsets=[f[1] for f in forms]), "flat")


def test_partial_and_merge_over_two_shards_equal_the_oracle(world, shards):
    """every shard counts its own docs, the sums over the shards (the all-reduce hook) decide on both alike"""
    import veloci_amd
    from veloci_amd.dist import exchange_local
    from parity import assert_same
    two, per_shard = shards

    def body(rank):
        forms = [product_form(world, c, per_shard[rank]) for c in world["cases"]]
        return veloci_amd.PartialBatch(two[rank], [veloci_amd.Request(r, docset=d) for r, d in forms])

    pbs = on_both_shards(two, body, unhook=False)
    g = exchange_local(pbs)
    got = pbs[0].merge(g.data_ptr(), 2)
    flat = pbs[1].merge_flat(g.data_ptr(), 2, stride=CC.ALL)  # (every rank merges the same gathered buffer)
    for s in two:
        s.set_allreduce(None)
    for case, res in zip(world["cases"], got):
        assert_same(case["request"], res, wanted(world, case))
    check_flat(world, flat, "merge_flat")
