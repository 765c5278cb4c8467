"""Doc sets ordered by a column (DocSet.top_by, vq_docset_top_by): the columns, the sets, the pages and the yardstick that
tests/test_gpu_docset_top.py runs on the device and tests/native/docset_top_driver.py over the stubbed device layer.  No GPU is needed to import or
check this file.

The index is docsetaggcases.index_data() (its columns `full`, `sparse`, `late`, `rare`, `crafted`, `m[].v`, unchanged) and three more columns:
`stars` (values 1..5: every key has about 40 000 ties), `flat` (one value everywhere: the order is pure doc id) and `lowbyte` (values whose bit
patterns differ only in the lowest byte, so the last radix pass alone decides, and a few docs that differ from them only in the top byte).

The yardstick: per doc a kind (0 number, 1 NaN, 2 no value) and a float64 value (negated for descending), ordered by
np.lexsort((doc, value, kind)).  It compares floats — -0 equals +0, so ties fall to the doc id — and never forms an integer key of a float."""
import numpy as np

import docsetaggcases as AC
import docsetrangecases as RC

N = AC.N
SHARD = AC.SHARD
THREE = AC.THREE
MAX_ROWS = 65_536  # kTopMaxRows (veloci_amd/csrc/kernels.hpp)
SET_NAMES = ("l-every", "w-dense", "w-ids200", "w-empty", "n1", "n3", "n4", "n5", "range-ends", "late-ends", "only-nan", "only-missing", "infs", "cancel", "outside-shard")
NEW_FIELDS = ("stars", "flat", "lowbyte")
ANCHOR_FIELDS = AC.ANCHOR_FIELDS + NEW_FIELDS
FIELDS = ANCHOR_FIELDS + ("m[].v",)
SHARD_FIELDS = AC.SHARD_FIELDS + NEW_FIELDS  # (`late` is one column per index, not a cut of one over all anchors)
LOW_BASE = 0x42280000  # 42.0: `lowbyte` holds the patterns LOW_BASE + 0 .. 255
TOP_BYTE_DOCS = {50: 0x41280011, 100_020: 0x43280011, 100_021: 0x41280011, 160_500: 0x43280011}  # LOW_BASE + 0x11 with another top byte
GRID = 3  # the grid cap the strided runs use (VQ_TOP_MAX_GRID)

_NEW = None
_SETS = None
_ORDER = {}
_SORTED = {}


def new_columns():
    """name -> f32 [N]; every doc has a value"""
    global _NEW
    if _NEW is None:
        rng = np.random.default_rng(83)
        low = (LOW_BASE + rng.integers(0, 256, size=N)).astype(np.uint32)
        for doc, bits in TOP_BYTE_DOCS.items():
            low[doc] = bits
        _NEW = {"stars": rng.integers(1, 6, size=N).astype(np.float32), "flat": np.full(N, 2.5, np.float32), "lowbyte": low.view(np.float32)}
    return _NEW


def index_data(lo=0, hi=N):
    data = AC.index_data(lo, hi)
    for name, vals in new_columns().items():
        data.add_boost(name + ".boost_valid_to_value", vals[lo:hi], None, key_base=lo)
    return data


def shard_index_data(lo, hi):
    data = AC.shard_index_data(lo, hi)
    for name, vals in new_columns().items():
        data.add_boost(name + ".boost_valid_to_value", vals[lo:hi], None, key_base=lo)
    return data


def sets():
    global _SETS
    if _SETS is None:
        S = AC.sets()
        _SETS = {k: S[k] for k in SET_NAMES}
    return _SETS


def _per_doc(field, descending, lo=0):
    """-> (kind u8 [N], value f64 [N]) of every doc of the index as the order sees it"""
    key = (field, bool(descending), lo)
    if key in _ORDER:
        return _ORDER[key]
    if "[]" in field:
        m = RC.columns()[field]
        owned = m["present"] & (m["anchor"] >= 0)
        nan = np.isnan(m["values"])
        num = owned & ~nan
        val = np.full(N, np.inf if not descending else -np.inf)
        (np.maximum if descending else np.minimum).at(val, m["anchor"][num], m["values"][num].astype(np.float64))
        has_num = np.bincount(m["anchor"][num], minlength=N) > 0
        has_any = np.bincount(m["anchor"][owned], minlength=N) > 0
        kind = np.where(has_num, 0, np.where(has_any, 1, 2)).astype(np.uint8)
    else:
        if field in NEW_FIELDS:
            values, has = new_columns()[field], np.ones(N, bool)
        elif field == "crafted":
            values, has = AC.crafted()["values"], AC.crafted()["present"]
        else:
            values, has = RC.view(field, lo, N)
        val = values.astype(np.float64)
        kind = np.where(~has, 2, np.where(np.isnan(val), 1, 0)).astype(np.uint8)
    val = np.where(kind == 0, val, 0.0)
    _ORDER[key] = (kind, val)
    return _ORDER[key]


def ordered(field, ids, descending, lo=0):
    """the whole set in the order -> (docs i64, values f32, kinds u8), the values as the result reports them"""
    ids = np.asarray(ids, np.int64)
    memo = (field, bool(descending), lo, int(ids.size), int(ids.sum()), int(ids[:1].sum()), int(ids[-1:].sum()))  # (the sets are few and differ in these)
    if memo in _SORTED:
        return _SORTED[memo]
    kind, val = _per_doc(field, descending, lo)
    k, v = kind[ids], val[ids]
    order = np.lexsort((ids, -v if descending else v, k))
    docs, k, v = ids[order], k[order], v[order]
    out = (v + 0.0).astype(np.float32)  # (-0.0 + 0.0 is +0.0: a zero is reported as +0.0)
    out[k == 1] = np.nan
    _SORTED[memo] = (docs, out, k)
    return _SORTED[memo]


def expected(field, ids, top, skip, descending=False, with_missing=True, lo=0):
    """-> dict(docs u32, values f32, kinds u8, counters) of DocSet.top_by on the whole index"""
    docs, values, kinds = ordered(field, ids, descending, lo)
    counters = {"docs": int(docs.size), "count": int((kinds == 0).sum()), "nan": int((kinds == 1).sum()), "missing": int((kinds == 2).sum())}
    if not with_missing:
        keep = kinds == 0
        docs, values, kinds = docs[keep], values[keep], kinds[keep]
    return {"docs": docs[skip:skip + top].astype(np.uint32), "values": values[skip:skip + top], "kinds": kinds[skip:skip + top], "counters": counters}


def same(got, want):
    """docs and kinds element for element, values bit for bit, counters number for number; `got`: a TopByResult or a dict like `want`"""
    g = got if isinstance(got, dict) else {"docs": got.docs, "values": got.values, "kinds": got.kinds, "counters": got.counters}
    return (g["docs"].dtype == np.uint32 and g["values"].dtype == np.float32 and g["kinds"].dtype == np.uint8 and np.array_equal(g["docs"], want["docs"])
            and np.array_equal(g["kinds"], want["kinds"]) and np.array_equal(g["values"].view(np.uint32), want["values"].view(np.uint32)) and g["counters"] == want["counters"])


def pages(name, n):
    """the (top, skip) pages of a set of n ids.  A page whose top + skip exceeds MAX_ROWS is a refusal, not a page (check_misuse holds the code):
    for the two sets of more than 65 536 ids the pages measured from n are left to the smaller sets, and `l-every` runs the two pages at the bound"""
    out = [(1, 0), (10, 0), (10, 5), (n, 0), (max(n - 1, 0), 0), (n + 7, 0), (5, n), (0, 0), (7, max(n - 3, 0))]
    if name == "l-every":
        out += [(MAX_ROWS, 0), (36, 65_500)]
    return [(t, s) for t, s in dict.fromkeys(out) if t + s <= MAX_ROWS]


def _class_starts(field, ids, descending):
    """row numbers where the numbers end and where the NaN docs end"""
    _, _, kinds = ordered(field, ids, descending)
    return int((kinds == 0).sum()), int((kinds <= 1).sum())


def extra_pages():
    """[(set, field, top, skip, descending)]: pages cut inside a tie run of `stars` and at its end, pages that reach into the NaN rows and the
    missing rows, pages on `late`"""
    S = sets()
    out = []
    for s in ("l-every", "w-dense", "w-ids200"):
        for descending in (False, True):
            _, values, _ = ordered("stars", S[s], descending)
            first = int((values == values[0]).sum())  # the length of the first tie run
            second = int((values == values[first]).sum())
            for end in (first, first + second):
                for top, skip in ((10, end - 10), (10, end - 5), (end, 0), (3, end - 1)):  # at the run's end, across it, the whole run, from its last row on
                    if skip >= 0 and top + skip <= MAX_ROWS:
                        out.append((s, "stars", top, skip, descending))
            out.append((s, "stars", 10, first // 2, descending))
    for s, f in (("w-dense", "sparse"), ("w-ids200", "sparse"), ("w-dense", "m[].v"), ("only-nan", "crafted"), ("only-missing", "crafted"), ("n5", "sparse"), ("infs", "crafted"),
                 ("late-ends", "late"), ("w-dense", "late"), ("w-ids200", "late"), ("l-every", "late"), ("w-dense", "rare")):
        for descending in (False, True):
            numbers, not_missing = _class_starts(f, S[s], descending)
            for at in {numbers, not_missing}:
                for top, skip in ((10, at - 5), (4, at - 4), (6, at), (3, at + 2), (at + 2, 0)):
                    if skip >= 0 and top + skip <= MAX_ROWS:
                        out.append((s, f, top, skip, descending))
    return list(dict.fromkeys(out))


def cases():
    """[(set, field, top, skip, descending, with_missing)]"""
    S = sets()
    out = []
    for s in SET_NAMES:
        for f in FIELDS:
            for top, skip in pages(s, int(S[s].size)):
                for descending in (False, True):
                    for with_missing in (True, False):
                        out.append((s, f, top, skip, descending, with_missing))
    for s, f, top, skip, descending in extra_pages():
        for with_missing in (True, False):
            out.append((s, f, top, skip, descending, with_missing))
    return list(dict.fromkeys(out))


def check_case(ds, case):
    s, f, top, skip, descending, with_missing = case
    want = expected(f, sets()[s], top, skip, descending, with_missing)
    got = ds.top_by(f, top=top, skip=skip, descending=descending, with_missing=with_missing)
    assert same(got, want), (case, got.rows()[:12], got.counters, list(zip(want["docs"].tolist(), want["values"].tolist(), want["kinds"].tolist()))[:12], want["counters"])
    assert not got.partial and len(got) == want["docs"].size
    return got


def chunk_of(n, grid=GRID):
    """position in the set's ids -> the tie chunk that holds it under a grid cap (top_grid and vpc of kernels.hpp / docset_top.hip, restated)"""
    nvec = (n + 3) // 4
    g = max(1, min((nvec + 63) // 64, grid))
    vpc = (nvec + g - 1) // g
    return lambda pos: pos // (vpc * 4)


def _bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def assert_not_vacuous():
    """what the cases reach, from the yardstick alone -> dict of counts; every condition the issue names is asserted"""
    S = sets()
    kinds = {AC.kind(ids) for ids in S.values()}
    assert kinds == {"plain", "tiled", "dense", "empty"}, kinds
    seen = {"cases": 0, "cut-inside-run": 0, "cut-at-run-end": 0, "run-over-chunks": 0, "threshold-nan": 0, "threshold-missing": 0, "lowest-byte": 0, "short-pages": 0,
            "select": 0, "all-winners": 0}
    for s, f, top, skip, descending, with_missing in cases():
        seen["cases"] += 1
        ids = S[s]
        docs, values, k = ordered(f, ids, descending)
        if not with_missing:
            docs, values, k = docs[k == 0], values[k == 0], k[k == 0]
        rows = top + skip
        assert rows <= MAX_ROWS
        seen["short-pages"] += skip + top > docs.size
        seen["select" if ids.size > rows else "all-winners"] += 1
        if not 0 < rows < docs.size:
            continue
        last, nxt = rows - 1, rows  # the last row taken and the first one left
        tie = k[last] == k[nxt] and (k[last] != 0 or values[last] == values[nxt])
        if tie:
            seen["cut-inside-run"] += 1
            run = docs[(k == k[last]) & ((values == values[last]) | (k != 0))]
            where = chunk_of(int(ids.size))(np.searchsorted(ids, run))
            seen["run-over-chunks"] += int(np.unique(where).size > 1)
        elif last > 0 and k[last - 1] == k[last] and (k[last] != 0 or values[last - 1] == values[last]):
            seen["cut-at-run-end"] += 1
        seen["threshold-nan"] += int(k[last] == 1 and with_missing)
        seen["threshold-missing"] += int(k[last] == 2 and with_missing)
        if f == "lowbyte" and k[last] == 0 and k[nxt] == 0 and values[last] != values[nxt]:
            a, b = _bits(values[last]), _bits(values[nxt])
            seen["lowest-byte"] += int((a ^ b) < 256)
    for name in ("cut-inside-run", "cut-at-run-end", "run-over-chunks", "threshold-nan", "threshold-missing", "lowest-byte", "short-pages", "select", "all-winners"):
        assert seen[name] > 0, (name, seen)
    # both zeros tied: the order between +0 and -0 is the doc id's, in both directions, and both come back as +0.0
    for descending in (False, True):
        docs, values, _ = ordered("full", S["n4"], descending)
        at = int(np.flatnonzero(docs == 100_000)[0])
        assert docs[at + 1] == 100_001 and _bits(values[at]) == _bits(values[at + 1]) == 0
    full = RC.columns()["full"]["values"]
    assert _bits(full[100_000]) == 0 and _bits(full[100_001]) == 0x80000000 and np.isposinf(full[100_002]) and np.isneginf(full[100_003])  # both infinities in n4
    docs, values, _ = ordered("full", S["n4"], False)
    assert docs.tolist() == [100_003, 100_000, 100_001, 100_002] and np.isneginf(values[0]) and np.isposinf(values[-1])
    # a denormal: 1e-40 and -1e-40 around the zero of `cancel`; the smallest one in l-every
    docs, values, _ = ordered("crafted", S["cancel"], False)
    assert docs.tolist() == [170_001, 6_001, 90_001, 90_000, 6_000, 170_000] and 0 < float(values[3]) < 1.2e-38
    assert _bits(full[100_005]) == 1 and 100_005 in S["l-every"]
    # a 1:n doc with several values: its minimum ascending, its maximum descending
    m = RC.columns()["m[].v"]
    owned = m["present"] & (m["anchor"] >= 0) & ~np.isnan(m["values"])
    per = np.bincount(m["anchor"][owned], minlength=N)
    several = np.flatnonzero(per >= 3)
    assert several.size > 100
    doc = int(several[several >= 100][0])
    mine = m["values"][owned & (m["anchor"] == doc)].astype(np.float64)
    assert _per_doc("m[].v", False)[1][doc] == mine.min() and _per_doc("m[].v", True)[1][doc] == mine.max() and mine.min() < mine.max()
    seen["1n-several"] = int(several.size)
    # the top-byte docs of `lowbyte` sort before and behind everything else, in both directions
    docs, _, _ = ordered("lowbyte", S["l-every"], False)
    assert set(docs[:2].tolist()) == {50, 100_021} and set(docs[-2:].tolist()) == {100_020, 160_500}
    low = new_columns()["lowbyte"].view(np.uint32)
    rest = np.ones(N, bool)
    rest[list(TOP_BYTE_DOCS)] = False
    assert ((low[rest] ^ LOW_BASE) < 256).all() and np.unique(low[rest]).size == 256
    # `late`: docs below key_base and behind the last key are missing
    _, _, k = ordered("late", S["late-ends"], False)
    assert (k == 2).sum() > 0 and (k == 0).sum() > 0
    # the shard sets
    out = S["outside-shard"]
    assert not ((out >= SHARD[0]) & (out < SHARD[1])).any() and (out < SHARD[0]).any() and (out >= SHARD[1]).any()
    seen["kinds"] = sorted(kinds)
    return seen


SHARD_SETS = ("l-every", "w-dense", "w-ids200", "n5", "range-ends", "only-nan", "only-missing", "infs", "cancel", "outside-shard", "w-empty")
SHARD_PAGES = ((10, 0), (10, 5), (7, 40_000), (0, 0), (300, 0))


def shard_cases():
    """[(set, field, top, skip, descending, with_missing)] of the three-shard runs"""
    out = []
    for s in SHARD_SETS:
        for f in SHARD_FIELDS:
            for k, (top, skip) in enumerate(SHARD_PAGES):
                out.append((s, f, top, skip, bool(k % 2), k != 2))
                if k == 1:
                    out.append((s, f, top, skip, False, False))
    return out


def check_shards(veloci_amd, shards):
    """shards: the three indexes of THREE, no hook set.  The merged parts equal the whole index's rows bit for bit; packed, unpacked and merged
    parts equal the direct merge; parts with different `top` are refused -> the number of merges"""
    S = sets()
    made = {s: [veloci_amd.DocSet(idx, S[s]) for idx in shards] for s in SHARD_SETS}
    assert made["outside-shard"][1].local_len == 0 and made["outside-shard"][0].local_len > 0 and made["w-empty"][0].local_len == 0
    merges = 0
    for s, f, top, skip, descending, with_missing in shard_cases():
        kw = dict(top=top, skip=skip, descending=descending, with_missing=with_missing)
        parts = [ds.top_by(f, **kw) for ds in made[s]]
        assert all(p.partial for p in parts)
        assert sum(p.counters["docs"] for p in parts) == S[s].size and [p.counters["docs"] for p in parts] == [ds.local_len for ds in made[s]]
        want = expected(f, S[s], top, skip, descending, with_missing)
        direct = veloci_amd.merge_top_by(parts)
        assert same(direct, want) and not direct.partial, (s, f, kw, direct.rows()[:8], direct.counters, want["counters"])
        packed = veloci_amd.merge_top_by([p.pack() for p in parts])
        assert same(packed, want) and packed.pack() == direct.pack()
        from veloci_amd import dist
        assert same(dist.top_by_shards_local(shards, made[s], f, **kw), want)
        merges += 3
    a = made["l-every"][0].top_by("full", top=10)
    for other in (dict(top=11), dict(top=10, skip=1), dict(top=10, descending=True), dict(top=10, with_missing=False)):
        b = made["l-every"][1].top_by("full", **other)
        try:
            veloci_amd.merge_top_by([a, b])
        except veloci_amd.VelociError as e:
            assert e.code == 6 and "differ" in str(e), (other, e)
        else:
            raise AssertionError("parts that differ in %r were merged" % (other,))
    try:
        veloci_amd.merge_top_by([a, made["l-every"][1].top_by("sparse", top=10)])
    except veloci_amd.VelociError as e:
        assert e.code == 6 and "`field`" in str(e)
    else:
        raise AssertionError("parts of two fields were merged")
    for group in made.values():
        for ds in group:
            ds.close()
    return merges


def check_misuse(veloci_amd, idx, other_idx):
    """every refusal with its code: 7 VQ_ERR_JSON, 6 VQ_ERR_INVALID_ARGUMENT, 3 the search's ERR_INDEX_NOT_FOUND, 4 VQ_ERR_UNSUPPORTED"""
    import ctypes as C
    L = veloci_amd.lib()
    ds = veloci_amd.DocSet(idx, [1, 2, 70_500])

    def raw(index, docset, text):
        out = C.c_void_p()
        rc = L.vq_docset_top_by(index.h if index is not None else None, docset._handle() if docset is not None else None, text, len(text) if text is not None else 0, C.byref(out))
        if rc == 0:
            L.vq_docset_top_free(out)
        return rc, L.vq_last_error().decode()

    for text in (b'{"field": "full"', b'[{"field": "full"}]', b'{"field": "full", "top": "3"}', b'{"field": "full", "skip": "0"}', b'{"field": "full", "descending": 1}',
                 b'{"field": "full", "with_missing": "yes"}', b'{"field": 7}', b'3'):
        rc, msg = raw(idx, ds, text)
        assert rc == 7 and "JsonError" in msg, (text, rc, msg)
    for text, part in ((b'{"top": 3}', "without `field`"), (b'{"field": "full", "order": "desc"}', "unknown key"), (b'{"field": "full", "top": -1}', "unsigned"),
                       (b'{"field": "full", "skip": 1.5}', "unsigned"), (b'{"field": "body.textindex.token_values"}', "term ids")):
        rc, msg = raw(idx, ds, text)
        assert rc == 6 and part in msg, (text, rc, msg)
    for text in (b'{"field": "full", "top": 65537}', b'{"field": "full", "top": 1, "skip": 65536}', b'{"field": "full", "top": 4294967295, "skip": 4294967295}'):
        rc, msg = raw(idx, ds, text)
        assert rc == 4 and "65536" in msg, (text, rc, msg)
    for text in (b'{"field": "full", "top": 65536}', b'{"field": "full", "top": 0, "skip": 65536}', b'{"field": "full", "top": null, "skip": null}'):
        rc, msg = raw(idx, ds, text)
        assert rc == 0, (text, rc, msg)
    foreign = veloci_amd.DocSet(other_idx, [1, 2, 70_500])
    rc, msg = raw(idx, foreign, b'{"field": "full"}')
    assert rc == 6 and "another index" in msg, (rc, msg)
    foreign.close()
    for args in ((None, ds, b'{"field": "full"}'), (idx, None, b'{"field": "full"}'), (idx, ds, None)):
        rc, msg = raw(*args)
        assert rc == 6 and "null argument" in msg, (rc, msg)
    rc, msg = raw(idx, ds, b'{"field": "nosuch"}')
    assert rc == 3 and msg == "Did not found path in indices nosuch.boost_valid_to_value", (rc, msg)
    rc, msg = raw(idx, ds, b'{"field": "orphan[].v"}')
    assert rc == 3 and msg == "Did not found path in indices orphan[].v.value_id_to_anchor", (rc, msg)
    for field in ("nosuch", "orphan[].v", "body.textindex.token_values"):  # as vq_docset_aggregate answers them
        out = C.c_void_p()
        text = ('[{"field": "%s"}]' % field).encode()
        rc2 = L.vq_docset_aggregate(idx.h, ds._handle(), text, len(text), C.byref(out))
        msg2 = L.vq_last_error().decode()
        rc, msg = raw(idx, ds, ('{"field": "%s"}' % field).encode())
        assert rc == rc2 and msg.split(": ", 1)[-1] == msg2.split(": ", 1)[-1], (rc, msg, rc2, msg2)
    # malformed images and merges
    good = ds.top_by("full", top=2).pack()
    for image in (good[:-1], good + b"\0", good[:63], b"", b"\1" + good[1:], good[:20] + b"\xff\xff\xff\x7f" + good[24:]):
        try:
            veloci_amd.merge_top_by([image])
        except veloci_amd.VelociError as e:
            assert e.code == 6, (len(image), e)
        else:
            raise AssertionError("a malformed image of %d bytes was taken" % len(image))
    try:
        veloci_amd.merge_top_by([])
    except veloci_amd.VelociError as e:
        assert e.code == 6 and "no part" in str(e)
    else:
        raise AssertionError("a merge of nothing was answered")
    whole = veloci_amd.merge_top_by([good])  # one whole result: a copy
    assert whole.pack() == good and not whole.partial
    ds.close()
    try:
        ds.top_by("full")
    except ValueError:
        pass
    else:
        raise AssertionError("a closed set was ordered")
