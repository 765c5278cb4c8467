"""Doc sets from numeric ranges (DocSet.from_ranges, vq_docset_from_ranges): the columns, the clause lists and the `within` sets that
tests/test_gpu_docset_ranges.py runs on the device and tests/native/docset_ranges_driver.py over the stubbed device layer, with the ids numpy
expects of each.  The yardstick compares in float64: a stored float32 is widened and held against the bound as the JSON number parses.  No GPU is
needed to import or check this file.  The index has docsetref.NUM_ANCHORS anchors, whole and on the shard docsetref.SHARD.

A column is defined over all anchors; the index of the doc range [lo, hi) holds its cut with key_base = lo.  `late` is the exception: it is one
column of 50 001 keys from key_base = lo + 1003 on (3 mod 4 on the whole index, 0 mod 4 on the shard, whose doc_lo is 1 mod 4), begins and ends inside the range, and the docs outside it have no
value — on every shard alike, so the length of a set is a sum over shards of one definition."""
import json

import numpy as np

import docsetalgebracases
import docsetref

N = docsetref.NUM_ANCHORS
SHARD = docsetref.SHARD
RANGES = ((0, N), SHARD)
LATE_SHIFT, LATE_KEYS = 1003, 50_001
M_VALUES = 260_001
F32_01 = float(np.float32(0.1))  # 0.10000000149011612: what a stored float32(0.1) is
FLT_MAX = float(np.finfo(np.float32).max)
SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 0.1, 16777216.0, 16777218.0, FLT_MAX, -FLT_MAX]
CLAUSE_TABLE = 8  # kRangeClauseTable (veloci_amd/csrc/kernels.hpp): the clauses one pass takes

_COLUMNS = None


def _grid(rng, n):
    """a quarter-step grid in [-1000, 1000]: bounds equal to stored values occur"""
    return (rng.integers(-4000, 4001, size=n) / 4.0).astype(np.float32)


def _seed_specials(vals, positions):
    for k, at in enumerate(positions):
        vals[at:at + len(SPECIALS)] = np.array(SPECIALS, np.float32)
    return vals


def columns():
    """name -> dict(values f32 [N], present bool [N]) for the anchor-keyed columns; "m[].v": values / present over the value ids, `anchor` (the
    first entry of the value's value_id_to_anchor row, -1: an empty row) and the table itself (offsets, entries)"""
    global _COLUMNS
    if _COLUMNS is not None:
        return _COLUMNS
    rng = np.random.default_rng(67)
    spots = (40, SHARD[0] + 5, 100_000, SHARD[1] - 40, 180_000)  # before, inside and behind the shard
    out = {}
    out["full"] = {"values": _seed_specials(_grid(rng, N), spots), "present": np.ones(N, bool)}
    # about a third present, in runs of 1 .. 90 docs that start anywhere: they cross 32-row and 64-row boundaries
    present = np.zeros(N, bool)
    at = 0
    while at < N:
        run = int(rng.integers(1, 91))
        if rng.random() < 1 / 3:
            present[at:at + run] = True
        at += run
    present[[0, 31, 32, N - 1, SHARD[0], SHARD[1] - 1]] = True
    present[[SHARD[0] - 1, SHARD[1]]] = False
    for s in spots:
        present[s:s + len(SPECIALS)] = True
    out["sparse"] = {"values": _seed_specials(_grid(rng, N), spots), "present": present}
    out["late"] = {"values": _seed_specials(_grid(rng, N), (2000, SHARD[0] + 2000, 100_000)), "present": np.ones(N, bool)}
    # 40 values in all, 12 of them inside the shard: a result that carries neither bitmap nor tile directory on either range
    rare = np.zeros(N, bool)
    inside = np.arange(SHARD[0], SHARD[1])
    outside = np.concatenate([np.arange(0, SHARD[0]), np.arange(SHARD[1], N)])
    rare[rng.choice(inside, size=12, replace=False)] = True
    rare[rng.choice(outside, size=28, replace=False)] = True
    out["rare"] = {"values": (np.arange(N) % 97).astype(np.float32), "present": rare}
    # 1:n: anchors carry 0 to 5 values; the values' ids are scattered over the value id space, the ids left over are empty rows; one row in 50 holds
    # a second entry, which counts for nothing
    lengths = rng.choice(6, size=N, p=[0.3, 0.35, 0.2, 0.1, 0.04, 0.01])
    owners = rng.permutation(np.repeat(np.arange(N), lengths))[:M_VALUES - 2000]
    anchor = np.full(M_VALUES, -1, np.int64)
    anchor[rng.permutation(M_VALUES)[:owners.size]] = owners
    second = (anchor >= 0) & (rng.random(M_VALUES) < 0.02)
    row_len = (anchor >= 0).astype(np.int64) + second
    offsets = np.zeros(M_VALUES + 1, np.int64)
    offsets[1:] = np.cumsum(row_len)
    entries = np.zeros(int(offsets[-1]), np.int64)
    entries[offsets[:-1][anchor >= 0]] = anchor[anchor >= 0]
    entries[offsets[:-1][second] + 1] = rng.integers(0, N, size=int(second.sum()))
    m_vals = _grid(rng, M_VALUES)
    m_vals[rng.choice(M_VALUES, size=500, replace=False)] = np.nan
    out["m[].v"] = {"values": m_vals, "present": rng.random(M_VALUES) < 0.85, "anchor": anchor, "offsets": offsets, "entries": entries}
    _COLUMNS = out
    return out


def view(field, lo, hi):
    """(values f32 [N], has-a-value bool [N]) of an anchor-keyed column as the index of [lo, hi) and its fellow shards hold it"""
    c = columns()[field]
    if field != "late":
        return c["values"], c["present"]
    has = np.zeros(N, bool)
    has[lo + LATE_SHIFT:lo + LATE_SHIFT + LATE_KEYS] = True
    return c["values"], has


def index_data(lo=0, hi=N):
    """the IndexData of the doc range [lo, hi): the two-term text field of docsetref.small_data() (searches can run) and the columns"""
    data = docsetref.small_data()
    C = columns()
    for name in ("full", "sparse", "rare"):
        present = None if name == "full" else C[name]["present"][lo:hi]
        data.add_boost(name + ".boost_valid_to_value", C[name]["values"][lo:hi], present, key_base=lo)
    first = lo + LATE_SHIFT
    assert lo < first and first + LATE_KEYS < hi and first % 4 == (3 if lo == 0 else 0)
    data.add_boost("late.boost_valid_to_value", C["late"]["values"][first:first + LATE_KEYS], None, key_base=first)
    m = C["m[].v"]
    data.add_boost("m[].v.boost_valid_to_value", m["values"], m["present"], key_base=0)
    data.add_key_value_store("m[].v.value_id_to_anchor", m["offsets"], m["entries"])
    data.add_boost("orphan[].v.boost_valid_to_value", m["values"][:100], None, key_base=0)  # a 1:n column without its value_id_to_anchor store
    return data


def _inside(v64, clause):
    ok = ~np.isnan(v64)
    with np.errstate(invalid="ignore"):
        if "gte" in clause:
            ok &= v64 >= clause["gte"]
        if "gt" in clause:
            ok &= v64 > clause["gt"]
        if "lte" in clause:
            ok &= v64 <= clause["lte"]
        if "lt" in clause:
            ok &= v64 < clause["lt"]
    return ok


def clause_mask(clause, lo, hi):
    """bool [N]: the docs that satisfy the clause on the index of [lo, hi), compared in float64"""
    field, missing = clause["field"], bool(clause.get("missing", False))
    if "[]" in field:
        m = columns()[field]
        owned = m["present"] & (m["anchor"] >= 0)
        inside = owned & _inside(m["values"].astype(np.float64), clause)
        has = np.bincount(m["anchor"][owned], minlength=N) > 0
        hit = np.bincount(m["anchor"][inside], minlength=N) > 0
        return hit | (~has if missing else False)
    values, has = view(field, lo, hi)
    return np.where(has, _inside(values.astype(np.float64), clause), missing)


def expected(clauses, within, lo, hi):
    """the ids of the whole set (numpy int64, sorted): every clause holds, and `within` (None, or ids) does"""
    mask = np.ones(N, bool)
    for c in clauses:
        mask &= clause_mask(c, lo, hi)
    if within is not None:
        w = np.zeros(N, bool)
        w[np.asarray(within, np.int64)] = True
        mask &= w
    return np.flatnonzero(mask)


def to_json(clauses):
    """JSON text of a clause list; JSON has no infinity, a bound beyond the floats stands for it"""
    return json.dumps(clauses).replace("-Infinity", "-1e999").replace("Infinity", "1e999")


def withins():
    """name -> ids (None: no `within`): a dense set (carries a bitmap: the stream route), 200 ids (none: the probe route), the empty set, the ids at
    the borders of a word, of the shard and of the index"""
    L = docsetref.id_lists()
    return {"none": None, "dense": np.unique(L["dense"]), "ids200": np.unique(L["sparse"]), "empty": np.zeros(0, np.int64),
            "edges": np.array(docsetalgebracases.EDGE_POSITIONS, np.int64)}


def _c(field, missing=None, **bounds):
    out = {"field": field}
    out.update(bounds)
    if missing is not None:
        out["missing"] = missing
    return out


def _many(n):
    """n clauses over the anchor-keyed columns, each of which lets most docs pass and every one of which removes some"""
    out = []
    for k in range(n):
        field = ("full", "sparse", "late")[k % 3]
        if k % 2:
            out.append(_c(field, missing=field != "full", lt=990.0 - 7.25 * k))
        else:
            out.append(_c(field, missing=field != "full", gte=-990.0 + 6.5 * k))
    return out


def clause_lists():
    """name -> clause list"""
    out = {
        # each of the four bounds alone, both-sided intervals; 10 and -250.25 are stored values: inclusive against exclusive
        "gte": [_c("full", gte=10.0)], "gt": [_c("full", gt=10.0)], "lte": [_c("full", lte=-250.25)], "lt": [_c("full", lt=-250.25)],
        "both": [_c("full", gte=-100.0, lt=100.25)], "both-open-closed": [_c("sparse", gt=-3.5, lte=7.75)], "between-the-grid": [_c("full", gt=10.01, lt=10.24)],
        # 0.1 against float32(0.1), in both directions
        "lte-0.1": [_c("full", gt=0.05, lte=0.1)], "gte-0.1": [_c("full", gte=0.1, lt=0.25)], "lte-f32-0.1": [_c("full", gt=0.05, lte=F32_01)],
        "lt-f32-0.1": [_c("full", gt=0.05, lt=F32_01)],
        # the zeros are equal; the denormals are values
        "gte-0": [_c("full", gte=0.0, lt=0.25)], "gt-0": [_c("full", gt=0.0, lt=0.25)], "lte-minus-0": [_c("full", gt=-0.25, lte=-0.0)], "lt-0": [_c("full", gt=-0.25, lt=0.0)],
        "gte-minus-0": [_c("sparse", gte=-0.0, lte=0.0)],
        "above-1e-50": [_c("full", gt=1e-50, lt=0.25)], "below-minus-1e-50": [_c("full", lt=-1e-50, gt=-0.25)], "the-denormal": [_c("full", gte=1e-50, lte=2e-45)],
        "around-zero": [_c("full", gte=-1e-50, lte=1e-50)],
        # the infinities are values; a bound no float32 equals; the largest float
        "gte-inf": [_c("full", gte=np.inf)], "gt-flt-max": [_c("full", gt=FLT_MAX)], "lte-minus-inf": [_c("sparse", lte=-np.inf)], "finite": [_c("full", gt=-np.inf, lt=np.inf)],
        "gt-inf": [_c("full", gt=np.inf)], "beyond-floats": [_c("full", gte=1e300)], "lte-1e300": [_c("full", lte=1e300, gte=FLT_MAX)],
        "above-2^24": [_c("full", gt=16777216.0, lt=16777218.0)], "gte-2^24+1": [_c("full", gte=16777217.0, lt=2e7)], "lte-2^24+1": [_c("full", gte=1e7, lte=16777217.0)],
        # a lower bound above the upper one; no bounds; missing
        "upside-down": [_c("full", gte=5.0, lte=4.0)], "upside-down-missing": [_c("sparse", missing=True, gte=5.0, lte=4.0)], "no-bounds": [_c("full")], "everything": [_c("rare", missing=True)],
        "no-bounds-sparse": [_c("sparse")], "missing-alone": [_c("sparse", missing=True)], "missing-interval": [_c("sparse", missing=True, gte=0.0, lt=500.0)],
        "not-missing-interval": [_c("sparse", missing=False, gte=0.0, lt=500.0)],
        # a column that begins and ends inside the range, at 3 mod 4; a column of 40 values
        "late": [_c("late", gte=-500.0, lte=500.0)], "late-missing": [_c("late", missing=True, gt=900.0)], "late-no-bounds": [_c("late")],
        "rare": [_c("rare", gte=0.0)], "rare-some": [_c("rare", gte=10.0, lt=60.0)],
        # several clauses
        "two-on-one-field": [_c("full", gte=-100.0), _c("full", lt=100.25)], "three-fields": [_c("full", gte=-500.0), _c("sparse", missing=True, lt=0.0), _c("late", missing=True, gte=-900.0)],
        "and-rare": [_c("full", lt=900.0), _c("rare", gte=0.0)], "clauses-8": _many(8), "clauses-9": _many(9), "clauses-16": _many(16), "clauses-17": _many(17),
        # 1:n: any present value of the doc inside the interval
        "1n": [_c("m[].v", gte=0.0, lt=50.0)], "1n-missing": [_c("m[].v", missing=True, gte=900.0)], "1n-no-bounds": [_c("m[].v")], "1n-missing-alone": [_c("m[].v", missing=True, gte=5.0, lte=4.0)],
        "1n-and-columns": [_c("full", gte=-800.0), _c("m[].v", lt=0.0), _c("sparse", missing=True, gte=-900.0)], "1n-twice": [_c("m[].v", lt=-500.0), _c("m[].v", gt=500.0)],
        "1n-second-pass": _many(8) + [_c("m[].v", missing=True, lt=800.0)],
    }
    return out


# the clause lists that run under every `within`; all others run without one
UNDER_WITHINS = ("gte", "lt-f32-0.1", "no-bounds", "missing-interval", "late-missing", "rare", "clauses-9", "clauses-17", "upside-down", "1n", "1n-and-columns")


def cases():
    """[(name, clause list name, within name)]"""
    out = [(name, name, "none") for name in clause_lists()]
    out += [("%s-in-%s" % (name, w), name, w) for name in UNDER_WITHINS for w in withins() if w != "none"]
    return out


def expected_route(clauses, within, lo, hi, forced=False):
    """the routing rule of docset_ranges.cpp: the probe route (1) when `within` carries no bitmap and every clause is anchor-keyed"""
    if forced or within is None or any("[]" in c["field"] for c in clauses):
        return 0
    return int(docsetref.image(within, N, lo, hi)["bitmap"] is None)


def counting_hook(state):
    """the hook of a shard that stands for all the others: it is handed one u64, the shard's local count (state["local"], numpy's), and answers
    with the whole set's length (state["len"])"""
    def hook(values):
        state["calls"] = state.get("calls", 0) + 1
        try:
            assert values.size == 1, values.size
            assert int(values[0]) == state["local"], (int(values[0]), state["local"])
            values[0] = state["len"]
        except Exception as e:  # noqa: BLE001 - kept for the caller: the library only learns that the sum failed
            state["error"] = repr(e)
            raise
    return hook


def check_case(veloci_amd, idx, lo, hi, state, case, within_sets, env):
    """one case on the index of [lo, hi): the image element for element, len and local_len, the route; a probe-route case once more under
    VQ_NO_RANGE_PROBE=1 with identical ids.  within_sets: name -> DocSet of `idx`.  -> the route taken"""
    name, list_name, within_name = case
    clauses, w_ids = clause_lists()[list_name], withins()[within_name]
    want = expected(clauses, w_ids, lo, hi)
    state["local"], state["len"] = int(((want >= lo) & (want < hi)).sum()), int(want.size)
    calls = state.get("calls", 0)
    ds = veloci_amd.DocSet.from_ranges(idx, to_json(clauses), within=within_sets[within_name])
    assert "error" not in state, (name, state["error"])
    assert state.get("calls", 0) == calls + (1 if (lo, hi) != (0, N) else 0), name  # one u64 per call on a shard, none on the whole index
    image = docsetref.check(ds, want, N, lo, hi)
    assert len(ds) == want.size and ds.local_len == image["local_len"] == state["local"], name
    route = expected_route(clauses, w_ids, lo, hi)
    assert ds.range_route == route and ds.route == -1, (name, ds.range_route, route)
    if route == 1:
        env["VQ_NO_RANGE_PROBE"] = "1"
        try:
            again = veloci_amd.DocSet.from_ranges(idx, to_json(clauses), within=within_sets[within_name])
        finally:
            del env["VQ_NO_RANGE_PROBE"]
        assert again.range_route == 0 and np.array_equal(again.ids(), ds.ids()) and len(again) == len(ds), name
        again.close()
    ds.close()
    return route


def check_misuse(veloci_amd, idx, other_idx, shard_without_hook):
    """every refusal with its code: 7 VQ_ERR_JSON, 6 VQ_ERR_INVALID_ARGUMENT, 3 the search's ERR_INDEX_NOT_FOUND, 4 VQ_ERR_UNSUPPORTED"""
    import ctypes as C
    L = veloci_amd.lib()

    def raw(index, text, within=None):
        out = C.c_void_p()
        rc = L.vq_docset_from_ranges(index.h if index is not None else None, text, len(text) if text is not None else 0, within._handle() if within is not None else None,
                                     C.byref(out))
        if rc == 0:
            L.vq_docset_free(out)
        return rc, L.vq_last_error().decode()

    for text in (b'[{"field": "full", "gte": 1', b'{"field": "full"}', b'[{"field": "full", "gte": "10"}]', b'[{"field": "full", "lt": true}]', b'[{"field": "full", "missing": 1}]',
                 b'[{"field": 7}]', b'[3]', b'[{"field": "full", "gte": 1, "gte": 2}]'):
        rc, msg = raw(idx, text)
        assert rc == 7 and "JsonError" in msg, (text, rc, msg)
    for text, part in ((b"[]", "empty"), (b'[{"gte": 1}]', "without `field`"), (b'[{"field": "full", "gt": 1, "gte": 1}]', "`gt` and `gte`"),
                       (b'[{"field": "full", "lt": 1, "lte": 1}]', "`lt` and `lte`"), (b'[{"field": "full", "ge": 1}]', "unknown key"),
                       (b'[{"field": "body.textindex.token_values", "gte": 1}]', "term ids")):
        rc, msg = raw(idx, text)
        assert rc == 6 and part in msg, (text, rc, msg)
    foreign = veloci_amd.DocSet(other_idx, [1, 2, 70_500])
    rc, msg = raw(idx, b'[{"field": "full"}]', foreign)
    assert rc == 6 and "another index" in msg, (rc, msg)
    foreign.close()
    for args in ((None, b'[{"field": "full"}]'), (idx, None)):
        rc, msg = raw(*args)
        assert rc == 6 and "null argument" in msg, (rc, msg)
    rc, msg = raw(idx, b'[{"field": "nosuch", "gte": 1}]')
    assert rc == 3 and msg == "Did not found path in indices nosuch.boost_valid_to_value", (rc, msg)
    try:  # the search's own code and text for a boost on that column
        veloci_amd.search({"search_req": {"search": {"path": "body", "terms": ["alpha"]}}, "boost": [{"path": "nosuch", "boost_fun": "Add", "param": 1.0}]}, idx)
        raise AssertionError("the search accepted the boost column")
    except veloci_amd.VelociError as err:
        assert (rc, msg) == (err.code, str(err)), (rc, msg, err.code, str(err))
    rc, msg = raw(idx, b'[{"field": "orphan[].v", "gte": 1}]')
    assert rc == 3 and msg == "Did not found path in indices orphan[].v.value_id_to_anchor", (rc, msg)
    rc, msg = raw(shard_without_hook, b'[{"field": "full", "gte": 1}]')
    assert rc == 4 and "vq_index_set_allreduce" in msg, (rc, msg)
    rc, msg = raw(idx, b'[{"field": "full", "gte": null, "lt": 3, "missing": null}]')  # a null bound is an absent one
    assert rc == 0, (rc, msg)
    try:
        veloci_amd.DocSet.from_range(idx, "full", gte=float("inf"))
        raise AssertionError("an infinite Python float went into JSON")
    except ValueError:
        pass


def _kind(ids, lo, hi):
    return docsetalgebracases.kind(ids, lo, hi)


def assert_not_vacuous():
    """the expected sets reach every image kind, an empty and a full result, both routes, answers that differ between an inclusive and an exclusive
    bound, selected docs in the first and the last word and at both shard edges; later passes remove docs; -> what was seen"""
    L, W, C = clause_lists(), withins(), columns()
    seen = {"kinds": {}, "routes": set(), "cases": len(cases())}
    full = False
    for k, (lo, hi) in enumerate(RANGES):
        kinds = seen["kinds"].setdefault(k, {})
        for name, list_name, w in cases():
            want = expected(L[list_name], W[w], lo, hi)
            kind = _kind(want, lo, hi)
            kinds[kind] = kinds.get(kind, 0) + 1
            seen["routes"].add(expected_route(L[list_name], W[w], lo, hi))
            full = full or want.size == N
        assert set(kinds) == {"plain", "tiled", "dense", "empty"}, (lo, hi, kinds)
        assert _kind(expected(L["rare"], None, lo, hi), lo, hi) == "plain" and _kind(W["dense"], lo, hi) == "dense" and _kind(W["ids200"], lo, hi) != "dense"
        assert expected_route(L["gte"], W["ids200"], lo, hi) == 1 and expected_route(L["gte"], W["dense"], lo, hi) == 0 and expected_route(L["1n"], W["ids200"], lo, hi) == 0
        assert expected_route(L["gte"], W["empty"], lo, hi) == 1 and expected_route(L["gte"], W["edges"], lo, hi) == 1
        # inclusive against exclusive on a stored value; 0.1 against float32(0.1)
        for a, b in (("gte", "gt"), ("lte", "lt"), ("gte-0", "gt-0"), ("lte-minus-0", "lt-0"), ("lte-f32-0.1", "lt-f32-0.1"), ("gte-0.1", "lte-0.1"), ("gte-inf", "gt-inf"),
                     ("gte-2^24+1", "above-2^24")):
            ia, ib = expected(L[a], None, lo, hi), expected(L[b], None, lo, hi)
            assert ia.size and not np.array_equal(ia, ib), (a, b, ia.size, ib.size)
        assert expected(L["lte-0.1"], None, lo, hi).size == 0 and expected(L["above-2^24"], None, lo, hi).size == 0 and expected(L["gt-inf"], None, lo, hi).size == 0
        assert expected(L["gte-0"], None, lo, hi).size > expected(L["gt-0"], None, lo, hi).size == expected(L["above-1e-50"], None, lo, hi).size > expected(L["gte-0.1"], None, lo, hi).size > 0
        for name in ("the-denormal", "gte-inf", "gt-flt-max", "beyond-floats", "lte-minus-inf", "lte-1e300"):
            assert 0 < expected(L[name], None, lo, hi).size <= 2 * 5, name
        assert np.array_equal(expected(L["gt-flt-max"], None, lo, hi), expected(L["gte-inf"], None, lo, hi))
        assert np.array_equal(expected(L["around-zero"], None, lo, hi), np.flatnonzero(C["full"]["values"] == 0))
        # the docs at the edges: of the first and the last word, of the shard
        nan_docs = np.flatnonzero(np.isnan(C["sparse"]["values"]) & C["sparse"]["present"])
        for list_name in ("no-bounds", "no-bounds-sparse", "missing-alone", "upside-down-missing"):  # the last: the docs without a value, nothing else
            want = expected(L[list_name], None, lo, hi)
            edges, beside = np.isin([0, 31, N - 1, SHARD[0], SHARD[1] - 1], want), np.isin([SHARD[0] - 1, SHARD[1]], want)
            assert (edges.all() if list_name != "upside-down-missing" else not edges.any() and beside.all()), (list_name, edges, beside)
        assert expected(L["missing-alone"], None, lo, hi).size == N - nan_docs.size > expected(L["no-bounds-sparse"], None, lo, hi).size
        # a second and a third pass remove docs the earlier passes kept
        for fewer, more in (("clauses-8", "clauses-9"), ("clauses-16", "clauses-17"), ("clauses-8", "1n-second-pass")):
            assert 0 < expected(L[more], None, lo, hi).size < expected(L[fewer], None, lo, hi).size, (fewer, more)
        assert len(L["clauses-9"]) == CLAUSE_TABLE + 1 and len(L["clauses-17"]) == 2 * CLAUSE_TABLE + 1
        # `late` begins and ends inside the range; NaN is present and satisfies nothing
        late = expected(L["late-no-bounds"], None, lo, hi)
        assert lo < late[0] == lo + LATE_SHIFT and late[-1] == lo + LATE_SHIFT + LATE_KEYS - 1 < hi and late.size == LATE_KEYS - (1 if lo == 0 else 2), (late[0], late[-1], late.size)
        assert nan_docs.size and not np.isin(nan_docs, expected(L["no-bounds-sparse"], None, lo, hi)).any() and not np.isin(nan_docs, expected(L["missing-alone"], None, lo, hi)).any()
    m = C["m[].v"]
    per_anchor = np.bincount(m["anchor"][m["anchor"] >= 0], minlength=N)
    assert m["values"].size == M_VALUES and per_anchor.max() == 5 and per_anchor.min() == 0 and int((m["anchor"] < 0).sum()) >= 2000
    assert (np.diff(m["anchor"][m["anchor"] >= 0]) < 0).sum() > 100_000 and int((np.diff(m["offsets"]) == 2).sum()) > 1000  # not monotone; rows with a second entry
    assert expected(L["1n-missing-alone"], None, 0, N).size > 50_000 and expected(L["1n-twice"], None, 0, N).size > 1000
    assert full and seen["routes"] == {0, 1}, seen
    seen["routes"] = sorted(seen["routes"])
    return seen
