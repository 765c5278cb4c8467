"""Crafted inputs for k_merge_spans and k_finalize run alone (vq_debug_merge_spans / vq_debug_finalize, tests/test_gpu_merge_kernels.py).

One builder per case.  A merge builder returns a list of calls, a call being a list of jobs `(table, top_k)` with `table` a u64 array of
shape (n_spans, top_k) as the scans leave it: a set of keys per span, zeros behind.  A finalize builder returns a list of calls
`{"top_k": [...], "keys": [shard][job] -> u64[top_k], "hits": [shard][job], "stride_pad": bytes}` whose shard lists are what the merge emits:
sorted descending, zeros behind.  The expected output always comes from mergeref.py.

Every builder asserts, here on the CPU, the property its case is built for.  For the merge that property is mostly WHICH ROUTE the kernel
takes, and the builders cannot see the kernel: `route()` below restates the kernel's rule (veloci_amd/csrc/kernels.hip, k_merge_spans —
bound route for 1 <= top_k <= 64 and more than 256 slots; bound = the top_k-th largest of the maxima over the 64 subsets "flat index
mod 64", floor 1; more than 2048 keys at or above it: back to rounds of (2048 - top_k) / top_k spans) and is used only to SELECT inputs.
When the kernel's rule changes, these asserts must be revisited with it: they would go on passing while the cases stop reaching the
branches they are named after.  The same holds for finalize's prune inside the shard loop (kept keys + top_k > 2048)."""
import numpy as np

from mergeref import make_key, merge_ref

K_BLOCK = 64
CAND_CAP = 2048
MAX_TOP_K = 1024


# ------------------------------------------------------------------------------------------------ helpers
def random_keys(rng, n):
    """n unique non-zero keys: positive f32 scores (with repeats: 1/8 of the keys share a score with another) and unique doc ids"""
    docs = rng.choice(0xFFFFFFFF, size=n, replace=False).astype(np.uint64)
    scores = (rng.random(n) * 50.0).astype(np.float32)
    if n >= 8:
        scores[: n // 8] = scores[n // 8: 2 * (n // 8)]
    keys = make_key(scores, docs)
    assert len(np.unique(keys)) == n and keys.min() > 0
    return keys


def spans_of(keys, n_spans, top_k, rng=None):
    """keys dealt into spans of top_k slots, the same number each (the rest zeros behind the span's keys), shuffled first when rng is given"""
    keys = np.asarray(keys, np.uint64)
    if rng is not None:
        keys = rng.permutation(keys)
    per = -(-len(keys) // n_spans)
    assert per <= top_k
    table = np.zeros((n_spans, top_k), np.uint64)
    for s in range(n_spans):
        part = keys[s * per:(s + 1) * per]
        table[s, :len(part)] = part
    return table


def route(table, top_k):
    """The kernel's rule restated -> {"route": "bound" | "fallback" | "rounds", "slots", "per_round", and on the bound routes "bound", "kept"}"""
    flat = np.asarray(table, np.uint64).ravel()
    info = {"slots": len(flat), "per_round": (CAND_CAP - top_k) // top_k}
    if not (1 <= top_k <= K_BLOCK and len(flat) > 4 * K_BLOCK):
        return dict(info, route="rounds")
    maxima = np.zeros(K_BLOCK, np.uint64)
    np.maximum.at(maxima, np.arange(len(flat)) % K_BLOCK, flat)
    bound = max(int(np.sort(maxima)[::-1][top_k - 1]), 1)
    kept = int(np.count_nonzero(flat >= np.uint64(bound)))
    return dict(info, route="bound" if kept <= CAND_CAP else "fallback", bound=bound, kept=kept)


def check_table(table, top_k):
    table = np.asarray(table, np.uint64)
    assert table.ndim == 2 and table.shape[1] == top_k and table.shape[0] >= 1 and 1 <= top_k <= MAX_TOP_K
    nz = table[table != 0]
    assert len(np.unique(nz)) == len(nz), "keys are unique"
    for row in table:  # zeros only behind a span's keys
        n = int(np.count_nonzero(row))
        assert np.all(row[:n] != 0) and np.all(row[n:] == 0)
    return table


# ------------------------------------------------------------------------------------------------ merge cases
def merge_bound_ordinary():
    rng = np.random.default_rng(101)
    jobs = []
    for top_k, n_spans in ((10, 30), (64, 40)):
        table = spans_of(random_keys(rng, n_spans * top_k), n_spans, top_k)
        r = route(table, top_k)
        assert r["slots"] > 256 and r["route"] == "bound" and top_k <= r["kept"] <= CAND_CAP, r
        jobs.append((table, top_k))
    # the bound is the window's last key: the 10 best keys in 10 different subsets, so exactly top_k keys reach the bound
    top_k, n_spans = 10, 30
    keys = np.sort(random_keys(rng, 300))[::-1]
    flat = np.zeros(300, np.uint64)
    flat[:10] = keys[:10]            # flat index i lies in subset i
    flat[10:] = rng.permutation(keys[10:])
    table = flat.reshape(n_spans, top_k)
    r = route(table, top_k)
    assert r["route"] == "bound" and r["kept"] == top_k and r["bound"] == int(keys[top_k - 1]), r
    jobs.append((table, top_k))
    return [jobs]


def merge_bound_top1():
    rng = np.random.default_rng(102)
    jobs = []
    for n_spans in (257, 5000):
        table = spans_of(random_keys(rng, n_spans), n_spans, 1)
        r = route(table, 1)
        assert r["route"] == "bound" and r["kept"] == 1, r
        jobs.append((table, 1))
    return [jobs]


def merge_rounds_by_size():
    rng = np.random.default_rng(103)
    jobs = []
    for top_k, n_spans in ((64, 4), (1, 256)):
        table = spans_of(random_keys(rng, n_spans * top_k), n_spans, top_k)
        r = route(table, top_k)
        assert r["slots"] == 256 and r["route"] == "rounds", r  # exactly 256 slots: not above the bound route's floor
        jobs.append((table, top_k))
    return [jobs]


def merge_rounds_by_top_k():
    rng = np.random.default_rng(104)
    jobs = []
    for top_k, n_spans, per_round in ((65, 40, 30), (682, 5, 2), (683, 5, 1), (1024, 5, 1)):
        table = spans_of(random_keys(rng, n_spans * top_k), n_spans, top_k)
        r = route(table, top_k)
        assert top_k > K_BLOCK and r["route"] == "rounds" and r["per_round"] == per_round and n_spans > per_round, r  # more than one round
        jobs.append((table, top_k))
    return [jobs]


def merge_few_hits_per_span():
    """300 spans of 8 hits under top_k 64: subset j is position j of every span, 56 subsets are empty, the bound falls to 1"""
    rng = np.random.default_rng(105)
    table = spans_of(random_keys(rng, 2400), 300, 64)
    assert all(np.count_nonzero(row) == 8 for row in table)
    r = route(table, 64)
    assert r["route"] == "fallback" and r["bound"] == 1 and r["kept"] == 2400 > CAND_CAP, r
    return [[(table, 64)]]


def merge_one_subset_hoards_the_small_keys():
    rng = np.random.default_rng(106)
    keys = np.sort(random_keys(rng, 40 * 64))
    table = np.zeros((40, 64), np.uint64)
    table[:, 63] = rng.permutation(keys[:40])                      # position 63 of every span: the 40 smallest keys
    table[:, :63] = rng.permutation(keys[40:]).reshape(40, 63)
    r = route(table, 64)
    assert r["route"] == "fallback" and r["bound"] == int(keys[39]) and r["kept"] == 40 * 64 - 39 > CAND_CAP, r
    return [[(table, 64)]]


def _edge_table(rng, kept):
    """64 spans of 64 keys of which exactly `kept` reach the bound: the kept-th largest key is the only key of subset 63 at or above
    itself, every other subset holds a larger one"""
    keys = np.sort(random_keys(rng, 4096))[::-1]
    big, bound, small = keys[:kept - 1], keys[kept - 1], rng.permutation(keys[kept:])
    table = np.zeros((64, 64), np.uint64)
    table[0, 63] = bound
    table[1:, 63] = small[:63]
    table[:, :63] = rng.permutation(np.concatenate([big, small[63:]])).reshape(64, 63)
    r = route(table, 64)
    assert r["bound"] == int(bound) and r["kept"] == kept, r
    return table, r


def merge_edge_of_the_buffer():
    rng = np.random.default_rng(107)
    fits, r_fits = _edge_table(rng, CAND_CAP)
    over, r_over = _edge_table(rng, CAND_CAP + 1)
    assert r_fits["kept"] == 2048 and r_fits["route"] == "bound" and r_over["kept"] == 2049 and r_over["route"] == "fallback"
    return [[(fits, 64)], [(over, 64)]]


def merge_short_and_empty():
    rng = np.random.default_rng(108)
    jobs = [(np.zeros((30, 10), np.uint64), 10), (np.zeros((3, 65), np.uint64), 65)]  # every span empty, on either route
    assert route(*jobs[0])["route"] == "bound" and route(*jobs[0])["kept"] == 0 and route(*jobs[1])["route"] == "rounds"
    lone = np.zeros((501, 10), np.uint64)  # one span with 3 keys among 500 empty ones
    lone[250, :3] = random_keys(rng, 3)
    r = route(lone, 10)
    assert r["route"] == "bound" and r["bound"] == 1 and r["kept"] == 3, r
    jobs.append((lone, 10))
    jobs.append((random_keys(rng, 1).reshape(1, 1), 1))
    jobs.append((random_keys(rng, 1024).reshape(1, 1024), 1024))
    jobs.append((spans_of(random_keys(rng, 700), 1, 1024), 1024))  # a lone span that is not full
    return [jobs]


def merge_equal_scores():
    """3000 keys of one score: the window is the largest ids.  Under top_k 64 the ids descend along the flat table, so the 64 best lie one
    in each subset and the bound is the window's last key; under top_k 300 the rounds route ranks them"""
    rng = np.random.default_rng(109)
    ids = np.sort(rng.choice(0xFFFFFFFF, size=3000, replace=False))[::-1]
    keys = make_key(np.full(3000, 7.25, np.float32), ids)
    flat = np.zeros(47 * 64, np.uint64)
    flat[:3000] = keys
    t64 = flat.reshape(47, 64)
    r = route(t64, 64)
    assert r["route"] == "bound" and r["kept"] == 64 and r["bound"] == int(keys[63]), r
    t300 = spans_of(keys, 10, 300, rng)
    assert route(t300, 300)["route"] == "rounds"
    for table, top_k in ((t64, 64), (t300, 300)):
        want = merge_ref(table, top_k)
        assert np.array_equal(want & np.uint64(0xFFFFFFFF), ids[:top_k].astype(np.uint64)) and len(np.unique(want >> np.uint64(32))) == 1
    return [[(t64, 64), (t300, 300)]]


DOMAIN_SCORES = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-45, 1.0, 2.5, np.inf], np.float32)  # 1e-45: the smallest denormal


def domain_keys(rng, n_docs=40):
    """every score of DOMAIN_SCORES on the docs 0, 0xFFFFFFFE and n_docs - 2 random ones"""
    bits = DOMAIN_SCORES.view(np.uint32)
    assert bits[5] == 1 and bits[4] == 0 and bits[3] == 0x80000000 and 0x80000000 < bits[2] < 0x80800000
    docs = np.concatenate([[0, 0xFFFFFFFE], 1 + rng.choice(0xFFFFFFFD, size=n_docs - 2, replace=False)]).astype(np.uint64)
    keys = make_key(np.repeat(DOMAIN_SCORES, n_docs), np.tile(docs, len(DOMAIN_SCORES)))
    assert len(np.unique(keys)) == len(keys) and keys.min() > 0
    return keys


def merge_key_domain():
    rng = np.random.default_rng(110)
    keys = domain_keys(rng)  # 360 keys
    jobs = []
    for top_k, n_spans in ((50, 36), (300, 4)):
        table = spans_of(keys, n_spans, top_k, rng)
        want = merge_ref(table, top_k)
        assert make_key(np.float32(np.inf), 0) in want and want[0] == make_key(np.float32(np.inf), 0xFFFFFFFE)  # (score > 0, doc 0) is in the window
        jobs.append((table, top_k))
    assert route(*jobs[0])["route"] == "bound" and route(*jobs[1])["route"] == "rounds"
    # all 360 keys wanted: negatives, both zeros and doc 0 are all in the window
    table = spans_of(keys, 3, 360, rng)
    assert np.count_nonzero(merge_ref(table, 360)) == 360
    jobs.append((table, 360))
    return [jobs]


def merge_mixed_launch():
    """one job from each case above in ONE launch: different top_k, keys_base and part_keys_off that are prefixes"""
    jobs = [b()[0][0] for b in (merge_bound_ordinary, merge_bound_top1, merge_rounds_by_size, merge_rounds_by_top_k, merge_few_hits_per_span,
                                merge_one_subset_hoards_the_small_keys, merge_short_and_empty, merge_equal_scores, merge_key_domain)]
    jobs.insert(6, merge_edge_of_the_buffer()[1][0])  # the twin that overflows
    assert len(jobs) == 10 and len({top_k for _, top_k in jobs}) >= 3
    in_off, out_off = merge_offsets(jobs)
    assert in_off[0] == 0 and out_off[0] == 0 and all(in_off[j + 1] - in_off[j] == jobs[j][0].size for j in range(len(jobs)))
    assert all(out_off[j + 1] - out_off[j] == jobs[j][1] for j in range(len(jobs)))
    return [jobs]


def merge_offsets(jobs):
    """-> (prefix of n_spans * top_k, prefix of top_k), each with a closing entry: where job j's input and output lie"""
    return (np.concatenate([[0], np.cumsum([t.size for t, _ in jobs])]).astype(np.int64),
            np.concatenate([[0], np.cumsum([k for _, k in jobs])]).astype(np.int64))


MERGE_CASES = {
    "bound_ordinary": merge_bound_ordinary,
    "bound_top_k_1": merge_bound_top1,
    "rounds_by_size": merge_rounds_by_size,
    "rounds_by_top_k": merge_rounds_by_top_k,
    "few_hits_per_span": merge_few_hits_per_span,
    "one_subset_hoards_the_small_keys": merge_one_subset_hoards_the_small_keys,
    "edge_of_the_buffer": merge_edge_of_the_buffer,
    "short_and_empty": merge_short_and_empty,
    "equal_scores": merge_equal_scores,
    "key_domain": merge_key_domain,
    "mixed_launch": merge_mixed_launch,
}


# ------------------------------------------------------------------------------------------------ finalize cases
def shard_list(keys, top_k):
    """what the merge emits for one shard and job: the keys (at most top_k) sorted descending, zeros behind"""
    assert len(keys) <= top_k
    return merge_ref(keys, top_k)


def finalize_call(top_k, keys, hits, stride_pad=0):
    top_k = [int(k) for k in top_k]
    assert len(keys) == len(hits) >= 1 and stride_pad % 8 == 0
    for sk, sh in zip(keys, hits):
        assert len(sk) == len(sh) == len(top_k)
        for lst, k in zip(sk, top_k):
            lst = np.asarray(lst, np.uint64)
            n = int(np.count_nonzero(lst))
            assert lst.shape == (k,) and np.all(lst[:n] != 0) and np.all(lst[n:] == 0) and np.all(np.diff(lst[:n].astype(object)) < 0), "sorted descending, zeros behind"
    for j in range(len(top_k)):  # unique inside a job (jobs may share keys: they are different queries)
        mine = np.concatenate([np.asarray(sk[j], np.uint64) for sk in keys])
        mine = mine[mine != 0]
        assert len(np.unique(mine)) == len(mine)
    return {"top_k": top_k, "keys": keys, "hits": [[int(h) for h in sh] for sh in hits], "stride_pad": stride_pad}


def random_shards(rng, num_shards, top_k, fill=None):
    """one job: per shard fill[s] (default top_k) random keys, unique over the shards -> [shard] -> u64[top_k]"""
    fill = [top_k] * num_shards if fill is None else list(fill)
    keys = random_keys(rng, max(sum(fill), 1))
    out, at = [], 0
    for f in fill:
        out.append(shard_list(keys[at:at + f], top_k))
        at += f
    return out


def one_job(rng, num_shards, top_k, fill=None, hits=None, stride_pad=0):
    lists = random_shards(rng, num_shards, top_k, fill)
    hits = [int(np.count_nonzero(l)) + 5 * s for s, l in enumerate(lists)] if hits is None else hits
    return finalize_call([top_k], [[l] for l in lists], [[h] for h in hits], stride_pad)


def mid_loop_prunes(call):
    """does k_finalize prune inside its shard loop for some job of the call (kept keys + top_k above the buffer when a shard is appended)"""
    def job(k):
        n, pruned = 0, False
        for _ in call["keys"]:
            if n + k > CAND_CAP:
                n, pruned = min(n, k), True
            n += k
        return pruned
    return any(job(k) for k in call["top_k"])


def finalize_no_mid_loop_prune():
    rng = np.random.default_rng(201)
    calls = [one_job(rng, s, k) for s in (1, 2) for k in (1, 10, 1024)]
    for c in calls:
        assert len(c["keys"]) * c["top_k"][0] <= CAND_CAP and not mid_loop_prunes(c)
    return calls


def finalize_mid_loop_prune():
    rng = np.random.default_rng(202)
    calls = [one_job(rng, s, k) for s, k in ((3, 683), (3, 1024), (8, 300), (16, 1024), (64, 64))]
    for c in calls:
        assert len(c["keys"]) * c["top_k"][0] > CAND_CAP and mid_loop_prunes(c)
    return calls


def finalize_winners_in_the_last_shard_only():
    rng = np.random.default_rng(203)
    keys = np.sort(random_keys(rng, 8 * 300))
    calls = []
    for last_wins in (True, False):
        last, rest = (keys[-300:], keys[:-300]) if last_wins else (keys[:300], keys[300:])
        rest = rng.permutation(rest)
        lists = [shard_list(rest[s * 300:(s + 1) * 300], 300) for s in range(7)] + [shard_list(last, 300)]
        assert (lists[7][299] > max(l[0] for l in lists[:7])) if last_wins else (lists[7][0] < min(l[299] for l in lists[:7]))
        c = finalize_call([300], [[l] for l in lists], [[300]] * 8)
        assert mid_loop_prunes(c)
        calls.append(c)
    return calls


def finalize_short_shards():
    rng = np.random.default_rng(204)
    calls = [one_job(rng, 8, 300, fill=(300, 0, 17, 300, 1, 299, 0, 300)),   # some shards short, the window full, a mid-loop prune
             one_job(rng, 3, 10, fill=(10, 3, 0)),
             one_job(rng, 8, 300, fill=(40, 0, 17, 100, 1, 0, 0, 60)),       # fewer keys in all than top_k: out_n < top_k
             one_job(rng, 2, 1024, fill=(1000, 23)),
             one_job(rng, 8, 300, fill=[0] * 8, hits=[0] * 8),               # every shard empty: out_n 0
             one_job(rng, 1, 1, fill=[0], hits=[0])]
    assert sum(np.count_nonzero(s[0]) for s in calls[2]["keys"]) == 218 < 300 and sum(np.count_nonzero(s[0]) for s in calls[3]["keys"]) == 1023
    assert all(not np.any(s[0]) for s in calls[4]["keys"])
    return calls


def finalize_hits():
    rng = np.random.default_rng(205)
    big = [(1 << 31) + 12345, (1 << 32) + 7, 0, (1 << 33) - 1, 3, 0xFFFFFFFF, 1 << 32, 0]
    assert sum(big) > (1 << 33) and sum(big) < (1 << 64)
    calls = [one_job(rng, 8, 10, hits=big), one_job(rng, 2, 10, hits=[0, 0]), one_job(rng, 3, 64, hits=[0, (1 << 40) + 1, 0])]
    return calls


def finalize_key_domain_and_equal_scores():
    rng = np.random.default_rng(206)
    dom = rng.permutation(domain_keys(rng))  # 360 keys dealt over 8 shards of 45
    ids = rng.choice(0xFFFFFFFF, size=2400, replace=False)
    equal = make_key(np.full(2400, 0.5, np.float32), ids)
    calls = []
    for top_k in (45, 360):
        lists = [shard_list(dom[s * 45:(s + 1) * 45], top_k) for s in range(8)]
        calls.append(finalize_call([top_k], [[l] for l in lists], [[45]] * 8))
    assert mid_loop_prunes(calls[1]) and not mid_loop_prunes(calls[0])
    lists = [shard_list(equal[s * 300:(s + 1) * 300], 300) for s in range(8)]
    calls.append(finalize_call([300], [[l] for l in lists], [[300]] * 8))
    want = merge_ref(equal, 300)
    assert np.array_equal(want & np.uint64(0xFFFFFFFF), np.sort(ids)[::-1][:300].astype(np.uint64))  # the window is the largest ids
    return calls


def finalize_stride():
    """the 8 x 300 case with the partials 0 and 256 bytes apart beyond their size: the same answer"""
    calls = []
    for pad in (0, 256):
        calls.append(one_job(np.random.default_rng(207), 8, 300, stride_pad=pad))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(calls[0]["keys"], calls[1]["keys"])) and calls[0]["hits"] == calls[1]["hits"]
    assert [c["stride_pad"] for c in calls] == [0, 256]
    return calls


def finalize_mixed_launch():
    rng = np.random.default_rng(208)
    top_k = [1, 10, 64, 300, 683, 1024]
    per_job = [random_shards(rng, 8, k, fill=[max(k - 3 * s, 0) if j % 2 else k for s in range(8)]) for j, k in enumerate(top_k)]
    keys = [[per_job[j][s] for j in range(len(top_k))] for s in range(8)]
    hits = [[1000 * s + j + ((1 << 32) if s == 3 else 0) for j in range(len(top_k))] for s in range(8)]
    c = finalize_call(top_k, keys, hits)
    assert mid_loop_prunes(c)
    return [c]


FINALIZE_CASES = {
    "no_mid_loop_prune": finalize_no_mid_loop_prune,
    "mid_loop_prune": finalize_mid_loop_prune,
    "winners_in_the_last_shard_only": finalize_winners_in_the_last_shard_only,
    "short_shards": finalize_short_shards,
    "hits": finalize_hits,
    "key_domain_and_equal_scores": finalize_key_domain_and_equal_scores,
    "stride": finalize_stride,
    "mixed_launch": finalize_mixed_launch,
}


def chained_case():
    """two queries (top_k 64 on the bound route, 300 on rounds) over 8 "shards": per shard and query a span table for the merge, whose output
    is finalize's input -> (merge jobs shard-major, top_k per query, raw tables [query][shard])"""
    rng = np.random.default_rng(301)
    top_k = [64, 300]
    n_spans = [40, 9]
    raw = []
    for k, ns in zip(top_k, n_spans):
        keys = random_keys(rng, 8 * ns * k)
        raw.append([check_table(spans_of(keys[s * ns * k:(s + 1) * ns * k], ns, k), k) for s in range(8)])
    assert route(raw[0][0], 64)["route"] == "bound" and route(raw[1][0], 300)["route"] == "rounds"
    jobs = [(raw[q][s], top_k[q]) for s in range(8) for q in range(2)]
    return jobs, top_k, raw


# ------------------------------------------------------------------------------------------------ the entry points through ctypes
def _p(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def call_merge(L, jobs):
    """vq_debug_merge_spans over the jobs of one call -> (return code, [job] -> u64[top_k])"""
    span_keys = np.ascontiguousarray(np.concatenate([np.asarray(t, np.uint64).ravel() for t, _ in jobs]))
    n_spans = np.array([t.shape[0] for t, _ in jobs], np.uint32)
    top_k = np.array([k for _, k in jobs], np.uint32)
    out = np.zeros(int(top_k.sum()), np.uint64)
    rc = L.vq_debug_merge_spans(_p(span_keys), _p(n_spans), _p(top_k), len(jobs), _p(out))
    off = merge_offsets(jobs)[1]
    return rc, [out[off[j]:off[j + 1]] for j in range(len(jobs))]


def call_finalize(L, call):
    """vq_debug_finalize over one call -> (return code, [job] -> (ids[top_k], score bits[top_k], n, hits))"""
    top_k = np.array(call["top_k"], np.uint32)
    shard_keys = np.ascontiguousarray(np.concatenate([np.asarray(l, np.uint64) for sk in call["keys"] for l in sk]))
    shard_hits = np.array(call["hits"], np.uint64).ravel()
    total = int(top_k.sum())
    ids, bits, n, hits = np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(len(top_k), np.uint32), np.zeros(len(top_k), np.uint64)
    rc = L.vq_debug_finalize(_p(shard_keys), _p(shard_hits), len(call["keys"]), call["stride_pad"], _p(top_k), len(top_k), _p(ids), _p(bits), _p(n), _p(hits))
    off = np.concatenate([[0], np.cumsum(top_k)]).astype(np.int64)
    return rc, [(ids[off[j]:off[j + 1]], bits[off[j]:off[j + 1]], int(n[j]), int(hits[j])) for j in range(len(top_k))]
