"""Facet counts of a doc set (DocSet.facets, vq_docset_facets): the index, the sets and the requests tests/test_gpu_docset_facets.py runs on the
device and tests/native/docset_facets_driver.py over the stubbed device layer, with a numpy restatement of what each must answer (np.bincount over
the CSR / direct arrays, then the ranking rule: count descending, value id ascending, zero counts dropped).  No GPU is needed to import or check
this file.  The index has docsetref.NUM_ANCHORS anchors and is built from raw stores, whole and on the shard docsetref.SHARD (stores cut to the
shard's anchors, key_base = doc_lo)."""
import numpy as np

import docsetref

N = docsetref.NUM_ANCHORS
SHARD = docsetref.SHARD
RANGES = ((0, N), SHARD)
LDS_VALUES = 4096  # kDocsetFacetLdsValues (veloci_amd/csrc/kernels.hpp): the longest histogram the LDS mode takes
MAX_TOP = 1024     # kMaxTopK: the most entries the selection kernels rank; beyond it the host ranks
LONG_ROW_ANCHOR, TRIPLE_ANCHOR, BEYOND_ANCHOR = 100_003, 100_004, 100_005  # inside the shard


class Field:
    """one facet field: `rows` (offsets, values) over the anchors [0, keys), `terms` values of the dictionary, how the index holds it"""

    def __init__(self, name, offsets, values, terms, keys=N, composed=None):
        self.name, self.offsets, self.values, self.terms, self.keys, self.composed = name, np.asarray(offsets, np.int64), np.asarray(values, np.int64), terms, keys, composed
        self.direct = composed is None and "[]" not in name and int(np.diff(self.offsets).max(initial=0)) <= 1

    def num_values(self, lo=0, hi=N):
        """max(dictionary size, largest value id of the range's rows + 1): the histogram's length on an index of [lo, hi)"""
        a, b = min(lo, self.keys), min(hi, self.keys)
        part = self.values[self.offsets[a]:self.offsets[b]]
        return max(self.terms, int(part.max()) + 1 if part.size and b > a else 0)

    def counts(self, ids, lo=0, hi=N):
        """the histogram of the ids inside [lo, hi) (np.bincount over the rows' values), as long as the index of that range makes it"""
        ids = np.asarray(ids, np.int64)
        rows = ids[(ids >= lo) & (ids < hi) & (ids < self.keys)]
        start, length = self.offsets[rows], self.offsets[rows + 1] - self.offsets[rows]
        at = np.repeat(start - np.concatenate([[0], np.cumsum(length)[:-1]]), length) + np.arange(int(length.sum()))
        nv = self.num_values(lo, hi)
        vals = self.values[at]
        return np.bincount(vals[vals < nv], minlength=nv).astype(np.int64)

    def term(self, v):
        return "%s%06d" % (self.name[:3], v) if v < self.terms else ""

    def ranked(self, counts, top):
        """[(text, count)]: count descending, value id ascending, zero counts dropped, the first `top` (None: all)"""
        nz = np.flatnonzero(counts)
        order = nz[np.lexsort((nz, -counts[nz]))]
        if top is not None:
            order = order[:top]
        return [(self.term(int(v)), int(counts[v])) for v in order]


def _csr(lengths, values):
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    assert off[-1] == len(values)
    return off, np.asarray(values, np.int64)


_FIELDS = None


def fields():
    """name -> Field; built once"""
    global _FIELDS
    if _FIELDS is not None:
        return _FIELDS
    rng = np.random.default_rng(23)
    out = {}
    # a scalar field with fewer keys than anchors and rows without a value: a direct store with 0xFFFFFFFF entries
    keys = 150_010
    has = rng.random(keys) < 0.8
    out["direct"] = Field("direct", *_csr(has.astype(np.int64), rng.integers(0, 37, size=int(has.sum()))), terms=37, keys=keys)
    # rows of 0-3 values, one row of 5 000 values, one row with the same value three times
    lengths = rng.integers(0, 4, size=N)
    lengths[LONG_ROW_ANCHOR], lengths[TRIPLE_ANCHOR] = 5000, 3
    off, vals = _csr(lengths, rng.integers(0, 1000, size=int(lengths.sum())))
    vals[off[TRIPLE_ANCHOR]:off[TRIPLE_ANCHOR] + 3] = 777
    out["csr[]"] = Field("csr[]", off, vals, terms=1000)
    # histograms of exactly the LDS bound and of one more counter
    out["fit"] = Field("fit", *_csr(np.ones(N, np.int64), np.concatenate([np.arange(LDS_VALUES), rng.integers(0, LDS_VALUES, size=N - LDS_VALUES)])), terms=LDS_VALUES)
    lengths = rng.integers(1, 3, size=N)
    out["over[]"] = Field("over[]", *_csr(lengths, np.concatenate([np.arange(LDS_VALUES + 1), rng.integers(0, LDS_VALUES + 1, size=int(lengths.sum()) - LDS_VALUES - 1)])),
                          terms=LDS_VALUES + 1)
    # 65 536 values, Zipf
    lengths = rng.integers(1, 4, size=N)
    zipf = np.minimum(rng.zipf(1.3, size=int(lengths.sum())) - 1, 65535)
    out["zipf[]"] = Field("zipf[]", *_csr(lengths, zipf), terms=65536)
    # every doc holds the same value: one hot counter, count = the set's size
    out["hot"] = Field("hot", *_csr(np.ones(N, np.int64), np.full(N, 3)), terms=5)
    # value ids beyond the dictionary render as ""; the largest lies inside the shard
    vals = rng.integers(0, 13, size=N)
    vals[BEYOND_ANCHOR] = 14
    out["beyond"] = Field("beyond", *_csr(np.ones(N, np.int64), vals), terms=10)
    # 200 000 values: `top: null` is ranked on the host
    has = rng.random(N) < 0.25
    out["big[]"] = Field("big[]", *_csr(has.astype(np.int64) * 2, rng.integers(0, 200_000, size=2 * int(has.sum()))), terms=200_000)
    # an n-step field: anchor -> value ids (comp[].parent_to_value_id) -> text ids (comp[].textindex.parent_to_value_id), composed on first use
    n_val = 50_000
    lengths = (rng.random(N) < 0.2).astype(np.int64) * rng.integers(1, 4, size=N)
    a_off, a_vals = _csr(lengths, rng.integers(0, n_val, size=int(lengths.sum())))
    text_of = rng.integers(0, 300, size=n_val)
    out["comp[]"] = Field("comp[]", a_off, text_of[a_vals], terms=300, composed=(a_off, a_vals, text_of))
    _FIELDS = out
    return out


def index_data(lo=0, hi=N):
    """the IndexData of the doc range [lo, hi): every anchor-keyed store cut to the range's anchors with key_base = lo"""
    import veloci_amd
    data = docsetref.small_data()
    for f in fields().values():
        data.add_fst(f.name + ".textindex", [f.term(v).encode() for v in range(f.terms)])
        a, b = min(lo, f.keys), min(hi, f.keys)
        if f.composed is not None:
            a_off, a_vals, text_of = f.composed
            data.add_key_value_store(f.name + ".parent_to_value_id", a_off[a:b + 1] - a_off[a], a_vals[a_off[a]:a_off[b]], key_base=a)
            data.add_key_value_store(f.name + ".textindex.parent_to_value_id", np.arange(len(text_of) + 1), text_of)
            continue
        store = ".textindex.anchor_to_text_id" if "[]" in f.name else ".textindex.parent_to_value_id"
        data.add_key_value_store(f.name + store, f.offsets[a:b + 1] - f.offsets[a], f.values[f.offsets[a]:f.offsets[b]], key_base=a)
    assert isinstance(data, veloci_amd.IndexData)
    return data


SET_SIZES = (0, 1, 3, 4, 5, 64, 65, 4097)


def id_sets():
    """name -> ids (numpy int64, sorted, unique): the sizes around a 16-byte vector and a wave, every anchor, ids outside the shard only; the sets
    of three ids and more hold the long row, the row with the repeated value and the value beyond the dictionary"""
    rng = np.random.default_rng(41)
    special = np.array([LONG_ROW_ANCHOR, TRIPLE_ANCHOR, BEYOND_ANCHOR])
    out = {}
    for size in SET_SIZES:
        ids = rng.choice(N, size=size, replace=False)
        if size >= 3:
            ids[:3] = special
            while np.unique(ids).size < size:
                ids = np.concatenate([np.unique(ids), rng.choice(N, size=size - np.unique(ids).size, replace=False)])
        out["n%d" % size] = np.unique(ids).astype(np.int64)
        assert out["n%d" % size].size == size
    out["every"] = np.arange(N, dtype=np.int64)
    outside = np.concatenate([np.arange(0, SHARD[0], 7), np.arange(SHARD[1], N, 5)])
    out["outside"] = outside.astype(np.int64)
    return out


COMPLEMENT_OF = "n4097"  # ~DocSet of this set is one more case
HISTOGRAM_FIELDS = ("direct", "csr[]", "fit", "over[]", "zipf[]", "hot", "beyond", "big[]", "comp[]")
TOPS = (0, 1, 10, 1024, 1025, None)


def tie_set():
    """ids whose zipf[] counts tie in crowds at the cuts of TOPS: the docs whose values all lie in the tail of the Zipf law (every row holds a value),
    so thousands of values are counted once or twice behind the one hot value the law's clipping makes"""
    f = fields()["zipf[]"]
    return np.flatnonzero(np.minimum.reduceat(f.values, f.offsets[:-1]) >= 2000)


def expected(field, ids, top):
    """what DocSet(ids).facets([{"field": field, "top": top}]) holds for `field`: on the whole index, and on a shard after its sum over the shards"""
    f = fields()[field]
    return f.ranked(f.counts(ids), top)


def summing_hook(state, lo, hi):
    """the hook of a shard [lo, hi) that stands for all the others: state["call"] = [(field, ids)] of the call under way.  It holds what the shard
    hands over against numpy's LOCAL histograms (the kernel's whole output on the shard) and answers with the histograms of the whole corpus"""
    def hook(values):
        state["calls"] = state.get("calls", 0) + 1
        try:
            if state.get("len") is not None:  # the length of a set the algebra makes: one u64
                assert values.size == 1
                values[0] = state["len"]
                return
            F = fields()
            local = np.concatenate([F[f].counts(ids, lo, hi) for f, ids in state["call"]])
            assert values.size == local.size, (values.size, local.size)
            assert np.array_equal(values, local.astype(np.uint64)), np.flatnonzero(values != local.astype(np.uint64))[:5]
            whole = []
            for f, ids in state["call"]:
                w, n = F[f].counts(ids), F[f].num_values(lo, hi)
                assert not w[n:].any()
                whole.append(w[:n])
            values[:] = np.concatenate(whole).astype(np.uint64)
        except Exception as e:  # noqa: BLE001 - kept for the caller: the library only learns that the sum failed
            state["error"] = repr(e)
            raise
    return hook


def facets_of(ds, state, field_tops, ids):
    """ds.facets(...) with the hook told what is under way; -> {field: [(value, count)]}"""
    state["call"] = [(f, ids) for f, _ in field_tops]
    got = ds.facets([{"field": f, "top": t} for f, t in field_tops])
    assert "error" not in state, state["error"]
    return got


def check_histograms(veloci_amd, idx, lo, hi, state, names, env):
    """every (set, field) pair of `names` x HISTOGRAM_FIELDS with top: null — the kernel's whole output — value for value, count for count, order
    included, then once more under VQ_NO_DOCSET_FACET_LDS=1: the two agree with each other.  -> pairs checked"""
    S = id_sets()
    pairs = 0
    for name in names:
        ids = S[name[1:]] if name.startswith("~") else S[name]
        ds = veloci_amd.DocSet(idx, ids)
        if name.startswith("~"):
            state["len"] = N - ids.size
            ds, ids = ~ds, np.setdiff1d(np.arange(N), ids)
            state["len"] = None
        local = int(((ids >= lo) & (ids < hi)).sum())
        assert len(ds) == ids.size and ds.local_len == local
        for field in HISTOGRAM_FIELDS:
            want = expected(field, ids, None)
            got = facets_of(ds, state, [(field, None)], ids)
            assert list(got) == [field] and got[field] == want, (name, field, got[field][:5], want[:5])
            env["VQ_NO_DOCSET_FACET_LDS"] = "1"
            try:
                forced = facets_of(ds, state, [(field, None)], ids)
            finally:
                del env["VQ_NO_DOCSET_FACET_LDS"]
            assert forced == got, (name, field)
            pairs += 1
        res = ds.facet_result([])
        assert res.facets is None and res.num_hits == ids.size and len(res.ids) == 0
        ds.close()
    return pairs


def check_tops(veloci_amd, idx, state):
    """every top of TOPS on the 65 536-value field over the set whose counts tie at the cuts, alone and as one call with several fields (request
    order, a field asked twice); -> entries compared"""
    ids = tie_set()
    ds = veloci_amd.DocSet(idx, ids)
    n = 0
    for top in TOPS:
        want = expected("zipf[]", ids, top)
        got = facets_of(ds, state, [("zipf[]", top)], ids)
        assert got == {"zipf[]": want}, (top, got["zipf[]"][:12], want[:12])
        assert len(want) == (min(top, len(expected("zipf[]", ids, None))) if top is not None else len(want))
        n += len(want)
    several = [("hot", None), ("zipf[]", 1025), ("csr[]", 10), ("direct", 1), ("big[]", None), ("zipf[]", 1025)]
    state["call"] = [(f, ids) for f, _ in several]
    res = ds.facet_result(json_of(several))
    assert "error" not in state, state["error"]
    assert res.num_hits == ids.size and len(res.ids) == 0 and len(res.scores) == 0
    assert list(res.facets) == ["hot", "zipf[]", "csr[]", "direct", "big[]"]  # request order (the dict keeps the first place of a field asked twice)
    for f, t in several:
        assert res.facets[f] == expected(f, ids, t), f
    ds.close()
    return n


def json_of(field_tops):
    import json
    return json.dumps([{"field": f, "top": t} for f, t in field_tops])


def check_misuse(veloci_amd, idx, other_idx, shard_without_hook):
    """a set of another index, an unknown field, malformed JSON, a shard without the hook: the codes and the texts"""
    ds = veloci_amd.DocSet(idx, [1, 2, 70_500])
    foreign = veloci_amd.DocSet(other_idx, [1, 2, 70_500])
    L = veloci_amd.lib()

    def raw(index, d, text):
        import ctypes as C
        out = C.c_void_p()
        rc = L.vq_docset_facets(index.h if index is not None else None, d._handle() if d is not None else None, text, len(text) if text is not None else 0,
                                C.byref(out))
        if rc == 0:
            L.vq_result_free(out)
        return rc, L.vq_last_error().decode()

    rc, msg = raw(idx, foreign, b'[{"field": "hot"}]')
    assert rc == 6 and "another index" in msg, (rc, msg)
    for field in ("nosuch", "nosuch[]", "body"):  # unknown fields, a field without a facet store: the search's own code and text
        rc, msg = raw(idx, ds, json_of([(field, 3)]).encode())
        req = {"search_req": {"search": {"path": "body", "terms": ["alpha"]}}, "facets": [{"field": field, "top": 3}]}
        try:
            veloci_amd.search(req, idx)
            raise AssertionError("the search accepted the facet field " + field)
        except veloci_amd.VelociError as err:
            assert (rc, msg) == (err.code, str(err)), (field, rc, msg, err.code, str(err))
    rc, msg = raw(idx, ds, b'[{"field": "nosuch"}]')
    assert rc == 3 and msg == "Did not found path in indices nosuch.textindex.parent_to_value_id", (rc, msg)
    for text, part in ((b'[{"field": "hot"', "JsonError"), (b'{"field": "hot"}', "facets: expected a sequence"), (b'[{"top": 3}]', "missing field `field`"), (b'[3]', "FacetRequest: expected an object")):
        rc, msg = raw(idx, ds, text)
        assert rc == 7 and part in msg, (text, rc, msg)
    for args in ((None, ds, b"[]"), (idx, None, b"[]"), (idx, ds, None)):
        rc, msg = raw(*args)
        assert rc == 6 and "null argument" in msg, (rc, msg)
    rc, msg = raw(idx, ds, b"null")  # Request.facets is an Option: null is no facet
    assert rc == 0
    on_shard = veloci_amd.DocSet(shard_without_hook, [70_500])
    rc, msg = raw(shard_without_hook, on_shard, b'[{"field": "hot"}]')
    assert rc == 4 and "vq_index_set_allreduce" in msg, (rc, msg)
    rc, msg = raw(shard_without_hook, on_shard, b"[]")  # nothing to sum
    assert rc == 0
    for d in (ds, foreign, on_shard):
        d.close()
    try:
        ds.facets([{"field": "hot"}])
        raise AssertionError("a closed set was accepted")
    except ValueError:
        pass


def mode(field, lo=0, hi=N, forced=False):
    """"lds" or "cache": the rule of docset_facets.cpp"""
    return "lds" if not forced and fields()[field].num_values(lo, hi) <= LDS_VALUES else "cache"


def host_ranked(field, top, lo=0, hi=N):
    nv = fields()[field].num_values(lo, hi)
    return (nv if top is None else min(top, nv)) > MAX_TOP


def assert_not_vacuous():
    """the cases reach both counting modes, a host-ranked facet, a direct and a CSR store, a composed store, an empty set, a value beyond the
    dictionary, the long row, ties at the cuts; -> what was seen"""
    F, S = fields(), id_sets()
    seen = {"modes": sorted({mode(n, lo, hi) for n in HISTOGRAM_FIELDS for lo, hi in RANGES}),
            "host_ranked": [n for n in HISTOGRAM_FIELDS if host_ranked(n, None)],
            "direct": [n for n in HISTOGRAM_FIELDS if F[n].direct], "csr": [n for n in HISTOGRAM_FIELDS if not F[n].direct and F[n].composed is None],
            "composed": [n for n in HISTOGRAM_FIELDS if F[n].composed is not None], "empty_sets": [n for n, ids in S.items() if ids.size == 0]}
    assert seen["modes"] == ["cache", "lds"] and seen["host_ranked"] and seen["direct"] and seen["csr"] and seen["composed"] and seen["empty_sets"], seen
    assert F["fit"].num_values() == LDS_VALUES and F["over[]"].num_values() == LDS_VALUES + 1 and mode("fit") == "lds" and mode("over[]") == "cache"
    for lo, hi in RANGES:
        assert F["beyond"].num_values(lo, hi) == 15 > F["beyond"].terms  # the same histogram on the shard: its sum over the shards lines up
    assert ("", 1) in expected("beyond", S["n3"], None)
    assert F["direct"].keys < N and int((np.diff(F["direct"].offsets) == 0).sum()) > 1000
    off = F["csr[]"].offsets
    assert off[LONG_ROW_ANCHOR + 1] - off[LONG_ROW_ANCHOR] == 5000 and list(F["csr[]"].values[off[TRIPLE_ANCHOR]:off[TRIPLE_ANCHOR + 1]]) == [777] * 3
    assert expected("hot", S["n4097"], None) == [("hot000003", 4097)]
    assert S["outside"].size > 10_000 and not ((S["outside"] >= SHARD[0]) & (S["outside"] < SHARD[1])).any()
    assert len(expected("big[]", S["every"], None)) > MAX_TOP
    counts = F["zipf[]"].counts(tie_set())
    ranked = np.sort(counts[counts > 0])[::-1]
    seen["ties_at"] = []
    for top in (1, 10, 1024, 1025):
        if ranked.size > top and ranked[top - 1] == ranked[top]:
            seen["ties_at"].append(top)
    assert {10, 1024, 1025} <= set(seen["ties_at"]), seen  # many values tie at the cut: the order among them is by value id
    return seen
