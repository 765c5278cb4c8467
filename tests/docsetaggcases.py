"""Numeric aggregations of a doc set (DocSet.aggregate / stats / histogram, vq_docset_aggregate): the columns, the sets, the edge lists and the
yardsticks that tests/test_gpu_docset_aggs.py runs on the device and tests/native/docset_aggs_driver.py over the stubbed device layer.  No GPU is
needed to import or check this file.

The columns are those of docsetrangecases (`full`, `sparse`, `late`, `rare`, `m[].v`, `orphan[]`, unchanged) and one more, `crafted`, whose values
are chosen for the sum: 2^100 and -2^100 around a 1.0, values that cancel, FLT_MAX many times beside a denormal, NaNs alone, docs without a value,
the infinities.  The sets are the `within` sets of docsetrangecases, the id lists of docsetalgebracases and small crafted ones.

The yardstick: counters and buckets by comparison in float64 in numpy, min / max by numpy with the NaNs removed, the sum by math.fsum of the finite
values (fsum returns the correctly rounded float64 of the exact sum) with the rule for the infinities spelled out."""
import json
import math
import struct
import threading

import numpy as np

import docsetalgebracases
import docsetrangecases as RC
import docsetref

N = docsetref.NUM_ANCHORS
SHARD = docsetref.SHARD
THREE = ((0, SHARD[0]), SHARD, (SHARD[1], N))  # the three doc ranges of the shard tests
MAX_EDGES = 1023  # kAggMaxEdges (veloci_amd/csrc/kernels.hpp)
FLT_MAX = RC.FLT_MAX
ANCHOR_FIELDS = ("full", "sparse", "late", "rare", "crafted")
SHARD_FIELDS = ("full", "sparse", "rare", "crafted", "m[].v")  # (`late` is one column per index in docsetrangecases, not a cut of one over all anchors)

# `crafted`: where the chosen values sit (one block in each of the three doc ranges where the block's point is a sum over ranks)
BIG = (5_000, 100_001, 160_000)  # 2^100, 1.0, -2^100: exact sum 1.0; float64 summation in this order gives 0.0
CANCEL = (6_000, 6_001, 90_000, 90_001, 170_000, 170_001)  # 3.25, -3.25, 1e-40, -1e-40, FLT_MAX, -FLT_MAX: exactly 0
MANY_MAX = (7_000, 300)  # FLT_MAX 300 times from here on, then one 1e-45
ONLY_NAN = (8_000, 10)
ONLY_MISSING = (9_000, 10)
INFS = (10_000, 10_001, 10_002)  # +inf, -inf, 2.0
POS_INF = (10_100, 10_101)  # +inf, 3.0
NEG_INF = (120_000, 120_001)  # -inf, 3.0

_CRAFTED = None


def crafted():
    """-> dict(values f32 [N], present bool [N])"""
    global _CRAFTED
    if _CRAFTED is not None:
        return _CRAFTED
    rng = np.random.default_rng(71)
    vals = (rng.integers(-2_000_000, 2_000_001, size=N) / 1024.0).astype(np.float32) * np.float32(0.37)  # fractions that do not sum exactly in float64
    present = np.ones(N, bool)
    vals[list(BIG)] = np.array([2.0 ** 100, 1.0, -2.0 ** 100], np.float32)
    vals[list(CANCEL)] = np.array([3.25, -3.25, 1e-40, -1e-40, FLT_MAX, -FLT_MAX], np.float32)
    vals[MANY_MAX[0]:MANY_MAX[0] + MANY_MAX[1]] = np.float32(FLT_MAX)
    vals[MANY_MAX[0] + MANY_MAX[1]] = np.float32(1e-45)
    vals[ONLY_NAN[0]:ONLY_NAN[0] + ONLY_NAN[1]] = np.nan
    present[ONLY_MISSING[0]:ONLY_MISSING[0] + ONLY_MISSING[1]] = False
    vals[list(INFS)] = np.array([np.inf, -np.inf, 2.0], np.float32)
    vals[list(POS_INF)] = np.array([np.inf, 3.0], np.float32)
    vals[list(NEG_INF)] = np.array([-np.inf, 3.0], np.float32)
    _CRAFTED = {"values": vals, "present": present}
    return _CRAFTED


def index_data(lo=0, hi=N):
    """docsetrangecases.index_data of the doc range, unchanged, and the `crafted` column"""
    data = RC.index_data(lo, hi)
    c = crafted()
    data.add_boost("crafted.boost_valid_to_value", c["values"][lo:hi], c["present"][lo:hi], key_base=lo)
    return data


def shard_index_data(lo, hi):
    """one of THREE: the cut of every column of SHARD_FIELDS (docsetrangecases.index_data asks for a doc range `late` fits into)"""
    data = docsetref.small_data()
    C = dict(RC.columns(), crafted=crafted())
    for name in ("full", "sparse", "rare", "crafted"):
        present = None if name == "full" else C[name]["present"][lo:hi]
        data.add_boost(name + ".boost_valid_to_value", C[name]["values"][lo:hi], present, key_base=lo)
    m = C["m[].v"]
    data.add_boost("m[].v.boost_valid_to_value", m["values"], m["present"], key_base=0)
    data.add_key_value_store("m[].v.value_id_to_anchor", m["offsets"], m["entries"])
    return data


def sets():
    """name -> ids (numpy int64, sorted, unique)"""
    W, L = RC.withins(), docsetalgebracases.LISTS
    out = {"w-" + k: np.unique(v) for k, v in W.items() if v is not None}  # dense (bitmap), ids200 (tiled), empty, edges
    out.update({"l-" + k: np.unique(np.asarray(L[k], np.int64)) for k in ("every", "medium", "repeated", "one", "last", "edges")})
    for n in (1, 3, 4, 5):  # the 16-byte vector edge; the specials of `full` and `sparse` begin at 100 000
        out["n%d" % n] = np.arange(100_000, 100_000 + n)
    out["range-ends"] = np.array([0, SHARD[0] - 1, SHARD[0], SHARD[1] - 1, SHARD[1], N - 1])
    out["late-ends"] = np.unique([base + RC.LATE_SHIFT + d for base in (0, SHARD[0]) for d in (-1, 0, RC.LATE_KEYS - 1, RC.LATE_KEYS)])
    out["big"] = np.array(BIG)
    out["cancel"] = np.array(CANCEL)
    out["many-max"] = np.arange(MANY_MAX[0], MANY_MAX[0] + MANY_MAX[1] + 1)
    out["only-nan"] = np.arange(ONLY_NAN[0], ONLY_NAN[0] + ONLY_NAN[1])
    out["only-missing"] = np.arange(ONLY_MISSING[0], ONLY_MISSING[0] + ONLY_MISSING[1])
    out["infs"] = np.array(INFS)
    out["pos-inf"] = np.array(POS_INF)
    out["neg-inf"] = np.array(NEG_INF)
    out["outside-shard"] = np.array([5, 6_000, 9_003, SHARD[0] - 1, SHARD[1], 170_000, N - 1])  # empty on the middle rank
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


def edge_lists():
    """name -> edges (None: no `edges`).  The declined lists are in check_misuse"""
    return {
        "none": None,
        "one": [0.0],  # with -0 present: both zeros lie in the upper bucket
        "quarter": [-500.25, -3.5, 0.0, 7.75, 250.0, 999.75],  # stored quarter-step values
        "0.1": [0.1], "f32-0.1": [RC.F32_01],  # a stored float32(0.1) is >= 0.1 and >= itself, and not >= the next double
        "one-key": [0.1, RC.F32_01],  # two edges on one f32 key: the bucket between them is empty
        "1e39": [1e39],  # beyond the floats: only +inf is at or above it
        "minus-1e39": [-1e39, 0.0],
        "1023": [float(x) for x in np.linspace(-1000.0, 1000.0, MAX_EDGES)],
        "tiny": [-1e-50, 0.0, 1e-50, 2e-45],  # around the zeros and the denormals
    }


def kind(ids):
    return docsetalgebracases.kind(ids, 0, N)


def cases():
    """[(name, set, field, edge list)]: every set under every field without edges; the edge lists on the sets that have something to show"""
    S = sets()
    out = [("%s/%s" % (s, f), s, f, "none") for s in S for f in ANCHOR_FIELDS + ("m[].v",)]
    for e in edge_lists():
        if e == "none":
            continue
        for s, f in (("l-every", "full"), ("w-dense", "sparse"), ("w-ids200", "full"), ("n5", "full"), ("l-medium", "m[].v"), ("w-empty", "full"), ("l-every", "crafted")):
            out.append(("%s/%s/%s" % (s, f, e), s, f, e))
    return out


def spec(field, edges):
    return {"field": field} if edges is None else {"field": field, "edges": list(edges)}


def to_json(specs):
    return json.dumps(specs).replace("-Infinity", "-1e999").replace("Infinity", "1e999")


def _values_of(field, ids, lo=0):
    """-> (f32 values the aggregation sees, docs of the set without a value)"""
    ids = np.asarray(ids, np.int64)
    if "[]" in field:
        m = RC.columns()[field]
        member = np.zeros(N, bool)
        member[ids] = True
        owned = m["present"] & (m["anchor"] >= 0)
        sel = owned.copy()
        sel[owned] = member[m["anchor"][owned]]
        return m["values"][sel], int(ids.size - np.unique(m["anchor"][sel]).size)
    values, has = (crafted()["values"], crafted()["present"]) if field == "crafted" else RC.view(field, lo, N)
    h = has[ids]
    return values[ids][h], int((~h).sum())


def exact_sum(x64):
    """x64: the counted values (float64, no NaN): the infinity rule, else math.fsum"""
    pos, neg = bool((x64 == np.inf).any()), bool((x64 == -np.inf).any())
    if pos and neg:
        return math.nan
    if pos or neg:
        return math.inf if pos else -math.inf
    return math.fsum(x64[np.isfinite(x64)].tolist())


def expected(field, ids, edges):
    """the dict DocSet.aggregate answers on the whole index"""
    v, missing = _values_of(field, ids)
    nan = np.isnan(v)
    x = v[~nan].astype(np.float64)
    out = {"docs": int(np.asarray(ids).size), "count": int(x.size), "missing": missing, "nan": int(nan.sum()), "min": None, "max": None, "sum": 0.0}
    if x.size:
        out["min"], out["max"] = float(x.min()) + 0.0, float(x.max()) + 0.0  # (-0.0 + 0.0 is +0.0: a zero is reported as +0.0)
        out["sum"] = exact_sum(x)
    if edges is not None:
        e = np.asarray(edges, np.float64)
        which = (x[:, None] >= e[None, :]).sum(axis=1) if x.size * e.size < 5_000_000 else np.searchsorted(e, x, side="right")
        out["buckets"] = np.bincount(which.astype(np.int64), minlength=e.size + 1).tolist()
    return out


def _bits(x):
    return None if x is None else struct.pack("<d", x) if not math.isnan(x) else b"nan"


def same(got, want):
    """field for field, the floats bit for bit (every NaN is one)"""
    if set(got) != set(want):
        return False
    return all((_bits(got[k]) == _bits(want[k])) if k in ("min", "max", "sum") else got[k] == want[k] for k in want)


def check_case(ds, case):
    """one case on DocSet `ds` (of the case's set, on the whole index) against the yardstick"""
    name, s, field, e = case
    edges = edge_lists()[e]
    want = expected(field, sets()[s], edges)
    got = ds.aggregate(to_json([spec(field, edges)]))[0]
    assert same(got, want), (name, got, want)
    if "[]" not in field:
        assert got["docs"] == got["missing"] + got["nan"] + got["count"], (name, got)
    if edges is not None:
        assert sum(got["buckets"]) == got["count"] and len(got["buckets"]) == len(edges) + 1, (name, got)
    return got


class SumHook:
    """the hook of n ranks that run as threads of one process: a barrier-style sum that knows nothing of what it sums"""

    def __init__(self, n):
        self.n, self.barrier, self.slots, self.total, self.calls, self.sizes = n, threading.Barrier(n), [None] * n, None, [0] * n, []

    def of(self, rank):
        def add(values):
            self.calls[rank] += 1
            self.slots[rank] = values.copy()
            self.barrier.wait()
            if rank == 0:
                assert len({s.size for s in self.slots}) == 1, [s.size for s in self.slots]
                self.total = np.sum(self.slots, axis=0, dtype=np.uint64)
                self.sizes.append(int(values.size))
            self.barrier.wait()
            values[:] = self.total
            self.barrier.wait()
        return add

    def run(self, work):
        """work(rank) on n threads -> their results; the first exception of any is raised here"""
        got, errs = [None] * self.n, []

        def one(rank):
            try:
                got[rank] = work(rank)
            except Exception as ex:  # noqa: BLE001 - raised below
                errs.append(ex)
                self.barrier.abort()

        threads = [threading.Thread(target=one, args=(r,)) for r in range(self.n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        real = [e for e in errs if not isinstance(e, threading.BrokenBarrierError)] or errs
        if real:
            raise real[0]
        return got


SHARD_SPECS = [("full", "quarter"), ("crafted", "none"), ("m[].v", "quarter"), ("sparse", "one"), ("rare", "none"), ("crafted", "1e39"), ("full", "none")]
SHARD_SETS = ("l-every", "w-dense", "w-ids200", "big", "cancel", "many-max", "infs", "neg-inf", "only-nan", "only-missing", "outside-shard", "range-ends", "l-one", "w-empty")


def check_shards(veloci_amd, shards, hook):
    """shards: the three indexes of THREE with hook.of(rank) set.  Every rank ends with the whole index's answer, bit for bit -> hook calls per rank"""
    S, E = sets(), edge_lists()
    specs = [spec(f, E[e]) for f, e in SHARD_SPECS]
    want = {s: [expected(f, S[s], E[e]) for f, e in SHARD_SPECS] for s in SHARD_SETS}
    text = to_json(specs)

    def work(rank):
        out = {}
        for s in SHARD_SETS:  # every rank makes the same calls in the same order
            ds = veloci_amd.DocSet(shards[rank], S[s])
            out[s] = (ds.aggregate(text), ds.local_len)
            ds.close()
        return out

    before = list(hook.calls)
    got = hook.run(work)
    for s in SHARD_SETS:
        for rank in range(3):
            for g, w, (f, e) in zip(got[rank][s][0], want[s], SHARD_SPECS):
                assert same(g, w), (s, rank, f, e, g, w)
    assert got[1]["outside-shard"][1] == 0 and got[0]["outside-shard"][1] > 0 and got[0]["w-empty"][1] == 0  # a set that is empty on one rank; on all
    calls = [hook.calls[r] - before[r] for r in range(3)]
    # one call for counters, buckets and limbs, four for min and max; none for the set that is empty everywhere
    assert calls == [5 * (len(SHARD_SETS) - 1)] * 3, calls
    return calls[0]


def check_misuse(veloci_amd, idx, other_idx, shard_without_hook):
    """every refusal with its code: 7 VQ_ERR_JSON, 6 VQ_ERR_INVALID_ARGUMENT, 3 the search's ERR_INDEX_NOT_FOUND, 4 VQ_ERR_UNSUPPORTED"""
    import ctypes as C
    L = veloci_amd.lib()
    ds = veloci_amd.DocSet(idx, [1, 2, 70_500])

    def raw(index, docset, text):
        out = C.c_void_p()
        rc = L.vq_docset_aggregate(index.h if index is not None else None, docset._handle() if docset is not None else None, text, len(text) if text is not None else 0,
                                   C.byref(out))
        if rc == 0:
            L.vq_docset_aggs_free(out)
        return rc, L.vq_last_error().decode()

    for text in (b'[{"field": "full"', b'{"field": "full"}', b'[{"field": "full", "edges": ["1"]}]', b'[{"field": "full", "edges": [1, true]}]', b'[{"field": "full", "edges": 3}]',
                 b'[{"field": 7}]', b'[3]'):
        rc, msg = raw(idx, ds, text)
        assert rc == 7 and "JsonError" in msg, (text, rc, msg)
    too_many = json.dumps([{"field": "full", "edges": list(range(MAX_EDGES + 1))}]).encode()
    for text, part in ((b"[]", "empty"), (b'[{"edges": [1]}]', "without `field`"), (b'[{"field": "full", "edge": [1]}]', "unknown key"), (too_many, "more than 1023 edges"),
                       (b'[{"field": "full", "edges": [2, 1]}]', "strictly ascend"), (b'[{"field": "full", "edges": [1, 1]}]', "strictly ascend"),
                       (b'[{"field": "body.textindex.token_values"}]', "term ids")):
        rc, msg = raw(idx, ds, text)
        assert rc == 6 and part in msg, (text[:60], rc, msg)
    rc, msg = raw(idx, ds, json.dumps([{"field": "full", "edges": list(range(MAX_EDGES))}]).encode())
    assert rc == 0, (rc, msg)
    foreign = veloci_amd.DocSet(other_idx, [1, 2, 70_500])
    rc, msg = raw(idx, foreign, b'[{"field": "full"}]')
    assert rc == 6 and "another index" in msg, (rc, msg)
    foreign.close()
    for args in ((None, ds, b'[{"field": "full"}]'), (idx, None, b'[{"field": "full"}]'), (idx, ds, None)):
        rc, msg = raw(*args)
        assert rc == 6 and "null argument" in msg, (rc, msg)
    rc, msg = raw(idx, ds, b'[{"field": "nosuch"}]')
    assert rc == 3 and msg == "Did not found path in indices nosuch.boost_valid_to_value", (rc, msg)
    rc, msg = raw(idx, ds, b'[{"field": "orphan[].v"}]')
    assert rc == 3 and msg == "Did not found path in indices orphan[].v.value_id_to_anchor", (rc, msg)
    for text in (b'[{"field": "nosuch"}]', b'[{"field": "orphan[].v"}]', b'[{"field": "body.textindex.token_values"}]'):  # from_ranges' own errors
        out = C.c_void_p()
        rc2 = L.vq_docset_from_ranges(idx.h, text, len(text), None, C.byref(out))
        msg2 = L.vq_last_error().decode()
        rc, msg = raw(idx, ds, text)
        assert rc == rc2 and msg.split(": ", 1)[-1] == msg2.split(": ", 1)[-1], (rc, msg, rc2, msg2)
    on_shard = veloci_amd.DocSet(shard_without_hook, [70_500])
    rc, msg = raw(shard_without_hook, on_shard, b'[{"field": "full"}]')
    assert rc == 4 and "vq_index_set_allreduce" in msg, (rc, msg)
    on_shard.close()
    rc, msg = raw(idx, ds, b'[{"field": "full", "edges": null}, {"field": "full", "edges": []}]')  # null: no edges; an empty list: one bucket
    assert rc == 0, (rc, msg)
    got = ds.aggregate([{"field": "full", "edges": []}])[0]
    assert got["buckets"] == [got["count"]] and ds.histogram("full", []) == [got["count"]]
    ds.close()


def assert_not_vacuous():
    """every image kind occurs among the sets; the exact sum differs from float64 summation somewhere; missing and nan are counted somewhere;
    a histogram has every bucket filled; the crafted sets are what their names say; -> what was seen"""
    S, E = sets(), edge_lists()
    kinds = {}
    for name, ids in S.items():
        kinds.setdefault(kind(ids), []).append(name)
    assert set(kinds) == {"plain", "tiled", "dense", "empty"}, kinds
    seen = {"kinds": {k: len(v) for k, v in kinds.items()}, "cases": len(cases()), "inexact": 0, "missing": 0, "nan": 0, "full-histograms": 0, "1n-missing": 0}
    for name, s, field, e in cases():
        want = expected(field, S[s], E[e])
        v, _ = _values_of(field, S[s])
        x = v[~np.isnan(v)].astype(np.float64)
        if x.size and np.isfinite(want["sum"]) and float(np.sum(x)) != want["sum"]:
            seen["inexact"] += 1
        seen["missing"] += want["missing"] > 0
        seen["nan"] += want["nan"] > 0
        seen["1n-missing"] += "[]" in field and want["missing"] > 0
        if "buckets" in want:
            assert sum(want["buckets"]) == want["count"], name
            seen["full-histograms"] += all(b > 0 for b in want["buckets"]) and len(want["buckets"]) > 2
        if "[]" not in field:
            assert want["docs"] == want["missing"] + want["nan"] + want["count"], name
    assert seen["inexact"] and seen["missing"] and seen["nan"] and seen["full-histograms"] and seen["1n-missing"], seen
    big = expected("crafted", S["big"], None)
    assert big["sum"] == 1.0 and float(np.sum(crafted()["values"][S["big"]].astype(np.float64))) == 0.0 and big["max"] == 2.0 ** 100
    cancel = expected("crafted", S["cancel"], None)
    assert cancel["sum"] == 0.0 and cancel["count"] == 6 and cancel["min"] == -FLT_MAX
    many = expected("crafted", S["many-max"], None)
    assert many["sum"] == math.fsum([FLT_MAX] * 300 + [float(np.float32(1e-45))]) > 300 * FLT_MAX * (1 - 1e-15) and many["min"] == float(np.float32(1e-45))
    assert expected("crafted", S["only-nan"], None) == {"docs": 10, "count": 0, "missing": 0, "nan": 10, "min": None, "max": None, "sum": 0.0}
    assert expected("crafted", S["only-missing"], None) == {"docs": 10, "count": 0, "missing": 10, "nan": 0, "min": None, "max": None, "sum": 0.0}
    assert math.isnan(expected("crafted", S["infs"], None)["sum"]) and expected("crafted", S["pos-inf"], None)["sum"] == math.inf
    assert expected("crafted", S["neg-inf"], None)["sum"] == -math.inf and expected("crafted", S["neg-inf"], None)["max"] == 3.0
    # the zeros: -0 is in the set and the minimum of {0, -0} is reported as +0.0; 0.1 against float32(0.1); two edges on one key
    n4 = expected("full", S["n4"], E["one"])
    assert n4["buckets"] == [1, 3] and n4["min"] == -math.inf  # 0.0, -0.0, +inf at or above 0; -inf below
    zeros = expected("full", np.array([100_000, 100_001]), E["tiny"])
    assert zeros["buckets"] == [0, 0, 2, 0, 0] and struct.pack("<d", zeros["min"]) == struct.pack("<d", 0.0) == struct.pack("<d", zeros["max"])
    a, b, c = (expected("full", S["l-every"], E[k])["buckets"] for k in ("0.1", "f32-0.1", "one-key"))
    assert a == b and c == [a[0], 0, a[1]] and a[1] > 0
    assert expected("full", S["l-every"], E["1e39"])["buckets"][1] == 5  # the five seeded +inf
    late = expected("late", S["late-ends"], None)
    assert late["missing"] > 0 and late["count"] > 0
    assert len(E["1023"]) == MAX_EDGES and all(x < y for x, y in zip(E["1023"], E["1023"][1:]))
    # the shard sets: the big three lie on three ranks, one set is empty on the middle rank only
    for (lo, hi), at in zip(THREE, BIG):
        assert lo <= at < hi
    out = S["outside-shard"]
    assert not ((out >= SHARD[0]) & (out < SHARD[1])).any() and (out < SHARD[0]).any() and (out >= SHARD[1]).any()
    return seen
