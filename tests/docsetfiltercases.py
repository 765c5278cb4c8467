"""The cases of the doc-set-from-a-filter tests (tests/test_gpu_docset_filter.py on the device, tests/native/docset_filter_driver.py over the stubbed
device layer): the corpus of tests/countcorpus.py plus one list `all` with every doc, the filter trees, and the numpy answers of tests/countref.py
they are held against.  Everything here is computed once per process and never changed."""
import functools

import numpy as np

import countcorpus as CC
import countref

N = CC.N
SHARD = (70_001, 150_000)  # not aligned to 65536, 16384 or 32
leaf, prefix, AND, OR = CC.leaf, CC.prefix, CC.AND, CC.OR


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (lists with `all`, info)"""
    L, info = CC.build_lists()
    L = dict(L)
    L["all"] = np.arange(N, dtype=np.int64)
    return L, info


def _request(name):
    return {n: r for n, r, _ in CC.count_requests()}[name]


def leaf_cases():
    """[(name, filter)]: single leaves over exact terms and prefixes"""
    terms = ("pedge", "pfull", "pmid", "d0", "d5", "pal0", "pal1", "pal2", "pal3", "fsmall", "fempty", "nosuch")
    return [(t, leaf(t)) for t in terms] + [("prefix-ua", prefix("ua")), ("prefix-uw", prefix("uw"))]


def tree_cases():
    return [("depth3", _request("depth3")["search_req"]), ("and16", _request("and16")["search_req"]), ("filter-tree", _request("filter-tree")["filter"]),
            ("or-pedge-fempty", OR(leaf("pedge"), leaf("fempty"))), ("and-d5-fempty", AND(leaf("d5"), leaf("fempty")))]


WITHIN_FILTER = AND(leaf("d3"), leaf("d4"))


def within_cases():
    """[(name, ids of the set to search within)]: each goes with WITHIN_FILTER"""
    L, _ = corpus()
    return [("within-fsmall", L["fsmall"]), ("within-f100001", L["f100001"]), ("within-empty", np.zeros(0, np.int64))]


def expected(flt, within=None):
    """all ids the filter (and-ed with the set `within`) selects: sorted unique int64"""
    L, _ = corpus()
    return countref.filter_docs({"filter": flt}, {"body": L}, docset=within)


def kinds(ids, lo=0, hi=N):
    """(dense, tiled, empty) of the image a set of these ids gets on [lo, hi): the rules of tests/docsetref.py"""
    local = ids[(ids >= lo) & (ids < hi)]
    span = hi - lo
    return span >= 65536 and local.size * 64 >= span, span >= 65536 and local.size * 4096 >= span, local.size == 0


def assert_not_vacuous(expected_sets, lo=0, hi=N):
    """the expected sets hold a dense one, a tiled one that is not dense, one with neither part, and an empty one"""
    seen = {"dense": 0, "tiled": 0, "plain": 0, "empty": 0}
    for ids in expected_sets:
        dense, tiled, empty = kinds(ids, lo, hi)
        seen["dense"] += dense
        seen["tiled"] += tiled and not dense
        seen["plain"] += not tiled and not empty
        seen["empty"] += empty
    assert all(seen.values()), seen
    return seen
