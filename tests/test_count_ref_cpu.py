"""The reference of the count pre-pass tests (tests/countref.py) pinned on the CPU oracle, and the teeth of the near-tie requests
(tests/countcorpus.py), without a GPU.

A node's size is the oracle's num_hits for that sub-tree sent as a request of its own, its size inside the filter the num_hits of the same request
with the filter attached, the filter's size the num_hits of the filter sent as a search.  Every near-tie case must matter: its sizes are what
its builder says, the reference's summation order and the one a count off by one selects give different f32 bits for some hit (the oracle's
own scores are the sums in the expected order), and after one doc has moved so that the two closest sizes swap the oracle answers differently."""
import json

import numpy as np
import pytest

import countcorpus as CC
import countref


@pytest.fixture(scope="module")
def corpus():
    L, info = CC.build_lists()
    return {"L": L, "info": info, "ora": CC.oracle_index(L), "lists": {"body": L}, "values": {}, "moved": {}}


def hits_of(ora, search_req, flt=None):
    req = {"search_req": search_req, "top": 1}
    if flt is not None:
        req["filter"] = flt
    return ora.search_json(json.dumps(req)).num_hits


def oracle_filter(req, docset):
    """the request's filter as the reference would take the doc set: one more filter leaf"""
    own = req.get("filter")
    if docset is None:
        return own
    return CC.leaf(docset) if own is None else CC.AND(own, CC.leaf(docset))


def test_lists_have_the_shapes_they_were_built_for(corpus):
    L, info = corpus["L"], corpus["info"]
    assert [len(L[t]) for t in ("f099999", "f100000", "f100001", "fempty")] == [99_999, 100_000, 100_001, 0]
    assert 0 in L["f100000"] and CC.N - 1 in L["f100000"] and set(CC.EDGES) <= set(L["pedge"].tolist())
    for b in CC.EDGE_BASES:
        assert {b + 2047, b + 2048, b + 4095, b + 4096, b + 8191, b + 8192, b + 32767, b + 32768} <= set(CC.EDGES)
    per_tile = np.bincount(L["pfull"] // CC.TILE, minlength=7)
    assert per_tile[2] == CC.TILE and per_tile[4] == 1
    for r in (1, 2, 3):  # at every bitmap width the first entry of a tile (from doc 8192 on) sits at list index r mod 4
        d = L["pal%d" % r]
        for w in (2048, 4096, 8192):
            first = np.searchsorted(d, np.arange(8192, CC.N, w))
            assert (first % 4 == r).all() and (d[first] < np.arange(8192, CC.N, w) + w).all(), (r, w)
    assert sorted(len(L[t]) % 4 for t in ("pal0", "pal1", "pal2")) == [1, 2, 3]  # lists that end 1, 2, 3 entries past a multiple of 4
    assert len(L["pmid"]) * 64 < CC.N <= len(L["pal0"]) * 64 and len(L["fsmall"]) * 64 < CC.N <= len(L["d0"]) * 64  # without / with a bitmap image
    assert len(np.union1d(np.union1d(L["ua0"], L["ua1"]), L["ua2"])) < len(L["ua0"]) + len(L["ua1"]) + len(L["ua2"])  # the lists of a leaf overlap


def test_reference_counts_equal_the_oracle(corpus):
    ora, lists = corpus["ora"], corpus["lists"]
    checked = 0
    for name, req, docset in CC.count_requests():
        ids = corpus["L"][docset] if docset is not None else None
        counts, fsize = countref.node_counts(req, lists, docset=ids)
        flt = oracle_filter(req, docset)
        assert (fsize is None) == (flt is None), name
        if flt is not None:
            assert fsize == hits_of(ora, flt), name
        for node, sub in countref.sub_requests(req):
            assert counts[node][0] == hits_of(ora, sub), (name, node)
            if flt is not None:
                assert counts[node][1] == hits_of(ora, sub, flt), (name, node)
            checked += 1
        # a doc range cuts every number in two
        cut = CC.N // 2 + 1000
        lo_part, lo_f = countref.node_counts(req, lists, docset=ids, hi=cut)
        hi_part, hi_f = countref.node_counts(req, lists, docset=ids, lo=cut)
        for node, (h, inside) in counts.items():
            assert lo_part[node][0] + hi_part[node][0] == h and (inside is None or lo_part[node][1] + hi_part[node][1] == inside), (name, node)
        assert fsize is None or lo_f + hi_f == fsize
    assert checked >= 90


def test_near_tie_cases_have_teeth(corpus):
    L, info, ora, lists = corpus["L"], corpus["info"], corpus["ora"], corpus["lists"]
    cases = CC.near_tie_cases(L, info)
    assert {c["name"].split("-")[0] for c in cases} == {"T1", "T2", "T3", "T4", "T5"} and len(cases) == 39
    for case in cases:
        req, name = case["request"], case["name"]
        # the sizes the reference compares: inside the filter up to 100 000 ids, the operands' own beyond
        counts, fsize = countref.node_counts(req, lists)
        use_inside = fsize is not None and fsize <= CC.SET_LINE
        assert fsize in (None, 100_000, 100_001) and use_inside == (case["filter"] == "f100000"), name
        and_node = 1 if case["label"] else 0
        ids = [node for node, sub in countref.sub_requests(req) if any(sub is op for op in case["operands"])]
        assert len(ids) == len(case["operands"]) and ids[0] == and_node + 1, name
        assert [counts[i][1 if use_inside else 0] for i in ids] == case["sizes"], (name, [counts[i] for i in ids])
        want = ora.search_json(json.dumps(req))
        assert 0 < want.num_hits == len(want.ids) < 1024, name  # every hit is returned
        got = dict(zip(np.asarray(want.ids).tolist(), np.asarray(want.scores, np.float32).view(np.uint32).tolist()))
        if not case["label"]:
            hits, differ, expected = CC.order_precondition(ora, case, corpus["values"])
            assert hits == want.num_hits and differ >= 1, (name, hits, differ)
            assert differ * 10 >= hits, (name, hits, differ)  # (about a quarter of the hits is usual)
            assert {d: int(np.float32(s).view(np.uint32)) for d, s in expected.items()} == got, name  # the oracle sums in the expected order
        if case["move"] is None:
            continue
        key = tuple(case["move"])
        if key not in corpus["moved"]:
            corpus["moved"][key] = CC.oracle_index(CC.moved(L, case["move"]))
        after = corpus["moved"][key].search_json(json.dumps(req))
        new = dict(zip(np.asarray(after.ids).tolist(), np.asarray(after.scores, np.float32).tolist()))
        common = sorted(set(got) & set(new))
        assert len(common) >= want.num_hits - 1, name  # the moved doc is no hit of the AND: the hit set stays
        old_scores = np.array([got[d] for d in common], np.uint32).view(np.float32)
        new_scores = np.array([new[d] for d in common], np.float32)
        changed = old_scores.view(np.uint32) != new_scores.view(np.uint32)
        assert changed.any(), name
        if case["label"]:  # another slot structure: max of two operands against (their sum) x 4 — no rounding matter
            ratio = np.maximum(old_scores, new_scores)[changed] / np.minimum(old_scores, new_scores)[changed]
            assert changed.sum() * 4 >= len(common) and ratio.min() > 1.5, (name, int(changed.sum()), float(ratio.min()))
    assert len(corpus["moved"]) == 5
