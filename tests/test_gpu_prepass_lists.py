"""The pre-pass kernels, list by list: k_union (one and two levels) and the dense union, the text-locality kernels (k_loc_gather, the segmented
sorts, k_loc_expand, k_loc_compact), k_range_hits and k_b1n_map run alone through the vq_debug_*_lists entry points on crafted indexes, and every
entry of every list they build — docs, f32 bit patterns, length, the 8 sentinel entries, the scalars the compiler consumes — is compared with the
plain restatements of tests/prepass_ref.py.  No tolerance: each value is one IEEE division, one multiplication and comparisons.  The shapes are
the smallest at which the kernels' boundaries exist (64 lanes, the 16-entry window, the 64-entry flush, 256-thread blocks, job slices)."""
import numpy as np
import pytest

import prepass_ref as R
import prepasscorpus as P

pytestmark = pytest.mark.gpu

SENT = 0xFFFFFFFF
UNION_K = ("k_union<count>", "k_union<write>")
DENSE_K = ("k_union_dense_scatter", "k_union_dense_count", "k_union_dense_write")


def launches(idx):
    return {k: v["launches"] for k, v in idx.profile_json(reset=True)["kernels"].items()}


def open_index(data, **kw):
    import veloci_amd
    idx = veloci_amd.Index(data, device=0, **kw)
    idx.profile_enable(True)
    return idx


def check_list(tag, got_docs, got_bits, want_docs, want_bits):
    n = len(want_docs)
    assert len(got_docs) - P.PAD == n, (tag, len(got_docs) - P.PAD, n)
    bad = np.flatnonzero((got_docs[:n] != want_docs) | (got_bits[:n] != want_bits))
    assert len(bad) == 0, (tag, "first wrong entries", [(int(i), int(got_docs[i]), int(want_docs[i]), hex(int(got_bits[i])), hex(int(want_bits[i]))) for i in bad[:5]])
    assert (got_docs[n:] == SENT).all() and (got_bits[n:] == 0).all(), (tag, "sentinels", got_docs[n:], got_bits[n:])


# ================================================================================================================================ union
N_DOCS = 40_000
SHARD = (10_000, 10_000 + 3 * 2048 + 100)  # not a multiple of the dense route's 2048-doc blocks
PALETTE = np.array([1, 2, 199, 2047, 2048, 65504], np.uint32)
LENS = (1, 15, 16, 17, 31, 32, 33, 100)


class UnionCorpus:
    def __init__(self):
        rng = np.random.default_rng(21)
        self.rng = rng
        self.lists = []
        self.refs = {}

        def scores(n):
            s = rng.integers(1, 200, size=n).astype(np.uint32)
            pick = rng.random(n) < 0.3
            s[pick] = PALETTE[rng.integers(0, len(PALETTE), size=int(pick.sum()))]
            return s

        def add(docs, sc=None):
            docs = np.unique(np.asarray(docs, np.uint32))
            self.lists.append((docs, scores(len(docs)) if sc is None else np.asarray(sc, np.uint32)))
            return len(self.lists) - 1

        def rand(n, lo=0, hi=N_DOCS):
            return lo + rng.choice(hi - lo, size=n, replace=False)

        self.len_tok = [add(rand(n, 0, 5000) if n == 1 else rand(n)) for n in LENS]
        self.pool = [add(rand(LENS[k % len(LENS)])) for k in range(200)]
        self.tiny = [add(rand(1 + k % 3)) for k in range(4096)]
        self.big = [add(rand(1000)) for _ in range(64)]
        self.four = [add(rand(4)) for _ in range(64)]
        same = rand(300)
        # every list holds the same docs; the scores are neighbouring f16 values (1024 .. 1087 are exact and one ulp apart)
        self.same = [add(same, 1024 + (7 * l + np.arange(300)) % 64) for l in range(64)]
        self.m32a, self.m32b = add(30_000 + np.arange(32)), add(30_100 + np.arange(32))
        self.m33, self.m95 = add(30_200 + np.arange(33)), add(30_300 + np.arange(95))
        self.low = add(rand(50, 0, 5000))
        # doc 0, the last doc of the index, the first and last doc of SHARD and their neighbours
        self.edge = add(np.concatenate([[0, 1, 2, 5, SHARD[0] - 1, SHARD[0], SHARD[1] - 1, SHARD[1], N_DOCS - 1], rand(800)]))
        self.data = P.postings_data(N_DOCS, self.lists)
        self.postings = self.data.token_to_anchor_score[P.POSTINGS]

    def term_scores(self, n, negative=False):
        s = self.rng.uniform(0.25, 4.0, size=n).astype(np.float32)
        return -s if negative else s

    def groups(self):
        """name -> jobs [(tokens, term scores)] of one call"""
        if hasattr(self, "_groups"):
            return self._groups
        ts = self.term_scores
        job = lambda toks, **kw: (list(toks), ts(len(toks), **kw))
        ones = lambda toks: (list(toks), np.ones(len(toks), np.float32))
        g = {
            # window refills: lists of 1 .. 100 postings alone, two of them, all eight
            "lens": [job([t]) for t in self.len_tok] + [job([self.len_tok[0], self.len_tok[3]]), job(self.len_tok)],
            # lanes of one wave: 2, 63, 64 lists
            "one_level": [job(self.pool[:2]), job(self.pool[:63]), job(self.pool[:64])],
            # 65, 128, 129 lists: a second level over 2 / 2 / 3 level-1 lists
            "two_levels": [job(self.pool[:65]), job(self.pool[:128]), job(self.pool[:129])],
            # 64 x 64 lists of 1 - 3 postings
            "tiny4096": [job(self.tiny)],
            # output lengths 64, 65, 127 (n mod 64 = 0, 1, 63) and 32: the 64-entry flush and its tail
            "flush": [job([self.m32a, self.m32b]), job([self.m32a, self.m33]), job([self.m32a, self.m95]), job([self.m32a])],
            # 500 spans; 2 spans over a 4-entry pivot; every span boundary doc held by all 64 lanes
            "spans": [job(self.big), job(self.four), job(self.same), ones(self.same)],
            # negative term scores (the max is the least negative); the list with doc 0 and the last doc
            "values": [job(self.pool[:10], negative=True), job(self.same, negative=True), job([self.edge]), job([self.edge, self.len_tok[7]], negative=True)],
            # three jobs of different shapes in one call
            "three_shapes": [job([self.len_tok[2]]), job(self.pool[:70]), job(self.big)],
            # (shard) lists and one whole job without postings in the range
            "shard": [job([t]) for t in self.len_tok] + [job([self.low]), job(self.pool[:64]), job(self.pool[:129]), job([self.edge]), job(self.big), job([self.low, self.edge])],
        }
        self._groups = g
        return g

    def ref(self, name, lo=0, hi=None):
        key = (name, lo, hi)
        if key not in self.refs:
            self.refs[key] = [R.union(self.postings, t, s, lo, hi) for t, s in self.groups()[name]]
        return self.refs[key]


@pytest.fixture(scope="module")
def ucorpus():
    return UnionCorpus()


@pytest.fixture(scope="module")
def uindex(ucorpus):
    return open_index(ucorpus.data)


@pytest.fixture(scope="module")
def ushard(ucorpus):
    return open_index(ucorpus.data, doc_lo=SHARD[0], doc_hi=SHARD[1])


def check_union(idx, corpus, name, lo=0, hi=None):
    jobs = corpus.groups()[name]
    want = corpus.ref(name, lo, hi)
    levels = 2 if any(len(t) > 64 for t, _ in jobs) else 1
    results = {}
    for route in (1, 2, 0):
        launches(idx)
        rc, got = P.run_union(idx, jobs, route)
        assert rc == 0, (name, route, rc)
        seen = launches(idx)
        if route == 2:
            assert all(seen.get(k, 0) >= 1 for k in DENSE_K) and not any(k in seen for k in UNION_K), (name, route, seen)
        else:  # (no job here has more than 4096 lists: the shipped rule keeps them all on k_union)
            assert all(seen.get(k, 0) == levels for k in UNION_K) and not any(k in seen for k in DENSE_K), (name, route, seen)
        for j, ((docs, bits, max_bits), (wd, wv, wmax)) in enumerate(zip(got, want)):
            check_list((name, "route", route, "job", j), docs, bits, wd, wv.view(np.uint32))
            assert max_bits == int(np.float32(wmax).view(np.uint32)), (name, route, j, hex(max_bits), wmax)
        results[route] = got
    for j in range(len(jobs)):  # k_union and the dense route agree entry for entry
        assert np.array_equal(results[1][j][0], results[2][j][0]) and np.array_equal(results[1][j][1], results[2][j][1]) and results[1][j][2] == results[2][j][2], (name, j)
    return want


@pytest.mark.parametrize("name", ["lens", "one_level", "two_levels", "tiny4096", "flush", "spans", "values", "three_shapes"])
def test_union_lists_match_the_reference_on_both_routes(ucorpus, uindex, name):
    """k_union<count/write> (kernels.hip: the quantile span bounds `pd[len * s / n_spans]`, the 16-entry window refill `pos - wbase >= kUnionWindow`,
    the 64-entry flush `(n & 63u) == 63u` and its tail, the sentinels of the last span, the level-2 pass over f32 lists) and
    k_union_dense_scatter / count / offsets / write (union_dense.hip) forced by `route`: whole lists against the reference and against each other."""
    want = check_union(uindex, ucorpus, name)
    if name == "flush":
        assert [len(d) for d, _, _ in want] == [64, 65, 127, 32]
    if name == "spans":  # (run_union_level: spans = min(total / 128, 4096, longest list))
        assert len(want[2][0]) == 300 and len(want[3][0]) == 300
    if name == "values":
        assert want[2][0][0] == 0 and want[2][0][-1] == N_DOCS - 1 and (want[0][1] < 0).all() and want[0][2] < 0


def test_union_lists_of_a_doc_range_shard(ucorpus, ushard):
    """The same kernels on a shard [10000, 16244): lists and one whole job without postings in the range (k_union: `pos >= end` from the start, a task
    whose pivot is empty; dense: a job whose scatter has nothing to write), a range that is no multiple of the dense route's 2048-doc blocks
    (k_union_dense_write: the last block's `doc0 + i` stays below the range), the first and the last doc of the range hit."""
    want = check_union(ushard, ucorpus, "shard", *SHARD)
    lens = [len(d) for d, _, _ in want]
    assert lens[0] == 0 and lens[8] == 0 and want[8][2] == 0.0  # the 1-posting list and the job of `low` lie outside
    assert want[11][0][0] == SHARD[0] and want[11][0][-1] == SHARD[1] - 1
    assert 0 < lens[9] < len(ucorpus.ref("one_level")[2][0])


def test_debug_entry_points_refuse_bad_arguments(ucorpus, uindex):
    """vq_debug_*_lists: -2 for an unknown path, a job without lists, a token beyond the store, an unknown route, an output area that is too small,
    anchors that do not ascend"""
    ok = [([ucorpus.m32a], np.ones(1, np.float32))]
    assert P.run_union(uindex, ok, 1)[0] == 0
    assert P.run_union(uindex, ok, 1, path="nope.textindex.to_anchor_id_score")[0] == -2
    assert P.run_union(uindex, ok, 3)[0] == -2
    assert P.run_union(uindex, [([], np.zeros(0, np.float32))], 1)[0] == -2
    assert P.run_union(uindex, [([len(ucorpus.lists)], np.ones(1, np.float32))], 1)[0] == -2
    assert P.run_union(uindex, ok, 1, cap=32 + P.PAD - 1)[0] == -2
    assert P.run_union(uindex, ok, 1, cap=32 + P.PAD)[0] == 0
    assert P.run_union(uindex, [(ucorpus.tiny + [ucorpus.low], np.ones(4097, np.float32))], 1)[0] == -2  # more than two levels of k_union take
    assert P.run_range_hits(uindex, [([ucorpus.edge], [5, 5])])[0] == -2
    assert P.run_range_hits(uindex, [([ucorpus.edge], [7, 5])])[0] == -2
    assert P.run_locality(uindex, [("body.textindex.tokens_to_text_id", "body.textindex.text_id_to_anchor", [0])])[0] == -2
    assert P.run_boost1n(uindex, [("a.value_id_to_parent", "b.value_id_to_anchor", "b.boost_valid_to_value", [0])])[0] == -2


def test_union_above_4096_lists_takes_the_dense_route_as_shipped(ucorpus, uindex):
    """run_union_jobs' shipped rule (route 0): 4097 lists go to the dense kernels, the 4096 of `tiny4096` (above) stay on k_union"""
    toks = ucorpus.tiny + [ucorpus.low]
    ts = ucorpus.term_scores(len(toks))
    launches(uindex)
    rc, got = P.run_union(uindex, [(toks, ts)], 0)
    seen = launches(uindex)
    assert rc == 0 and all(seen.get(k, 0) >= 1 for k in DENSE_K) and not any(k in seen for k in UNION_K), seen
    wd, wv, wmax = R.union(ucorpus.postings, toks, ts)
    check_list("4097 lists", got[0][0], got[0][1], wd, wv.view(np.uint32))
    assert got[0][2] == int(np.float32(wmax).view(np.uint32))


# ================================================================================================================================ range hits
def anchors_around(rng, docs, n):
    """n ascending anchors: doc 0 and the last doc of the index, docs of the lists, their right neighbours (adjacent anchors; anchors no list holds)"""
    if n == 1:
        return [int(docs[len(docs) // 2])]
    pick = rng.choice(docs, size=min(len(docs), n), replace=False).astype(np.int64)
    cand = np.unique(np.concatenate([pick, pick[: n // 3] + 1]))
    cand = cand[(cand > 0) & (cand < N_DOCS - 1)]
    cand = rng.permutation(cand)[: n - 2]
    out = np.unique(np.concatenate([[0, N_DOCS - 1], cand]))
    assert len(out) == n, (len(out), n)
    return out.astype(np.uint32).tolist()


def check_range(idx, corpus, jobs):
    launches(idx)
    rc, got = P.run_range_hits(idx, jobs)
    assert rc == 0
    seen = launches(idx)
    assert seen.get("k_range_hits", 0) == 1, seen
    for j, ((tokens, anchors), counts) in enumerate(zip(jobs, got)):
        want = R.range_hits(corpus.postings, tokens, anchors)
        assert np.array_equal(counts, want), (j, len(tokens), np.flatnonzero(counts != want)[:8], counts[:8], want[:8])


def test_range_hits_one_list_path(ucorpus, uindex):
    """k_range_hits, `J.n_lists == 1u`: a lane per anchor, 1 / 63 / 64 / 65 / 130 anchors (`an[j - 1u]` read across the block edge at j = 64), anchors 0
    and the last doc, adjacent anchors (between-count 0), anchors the list does not hold; five jobs in one call (the `block_begin` search) and the
    longest alone.  (An anchor held several times by ONE list cannot be staged: the loader takes ascending unique lists only; the many-lists test
    has anchors held by several lists.)"""
    rng = np.random.default_rng(5)
    docs = ucorpus.lists[ucorpus.edge][0]
    jobs = [([ucorpus.edge], anchors_around(rng, docs, n)) for n in (1, 63, 64, 65, 130)]
    a = jobs[3][1]
    assert any(y == x + 1 for x, y in zip(a, a[1:])) and any(x not in set(docs.tolist()) for x in a)
    check_range(uindex, ucorpus, jobs)
    check_range(uindex, ucorpus, jobs[4:])


def test_range_hits_many_lists_path(ucorpus, uindex):
    """k_range_hits, a workgroup per anchor: 2 / 64 / 65 / 200 lists (`i += 64u` lane striding, the shfl_u64 wave reduction), anchors held by several lists"""
    rng = np.random.default_rng(6)
    jobs = []
    for k in (2, 64, 65, 200):
        docs = np.unique(np.concatenate([ucorpus.lists[t][0] for t in ucorpus.pool[:k]]))
        jobs.append((ucorpus.pool[:k], anchors_around(rng, docs, 70 if k > 2 else 10)))
    # an anchor that all 64 lists of `same` hold
    jobs.append((ucorpus.same, [0] + sorted(ucorpus.lists[ucorpus.same[0]][0][[1, 2, 150, 299]].tolist())))
    check_range(uindex, ucorpus, jobs)


def test_range_hits_both_paths_and_an_empty_job_in_one_call(ucorpus, uindex):
    """k_range_hits' `jobs[mid].block_begin <= blockIdx.x` search over jobs of 3 blocks (one list, 130 anchors), none (no lists; no anchors) and one block per anchor"""
    rng = np.random.default_rng(7)
    docs = ucorpus.lists[ucorpus.edge][0]
    pool_docs = np.unique(np.concatenate([ucorpus.lists[t][0] for t in ucorpus.pool[:65]]))
    jobs = [([ucorpus.edge], anchors_around(rng, docs, 130)), ([], [3, 9, 27]), (ucorpus.pool[:65], anchors_around(rng, pool_docs, 5)), ([ucorpus.big[0]], []),
            ([ucorpus.big[1]], anchors_around(rng, ucorpus.lists[ucorpus.big[1]][0], 1)), (ucorpus.big[:3], anchors_around(rng, ucorpus.lists[ucorpus.big[2]][0], 64))]
    check_range(uindex, ucorpus, jobs)


# ================================================================================================================================ text locality
N_ANCHORS = 6000
F_T2T, F_T2A = "f[].textindex.tokens_to_text_id", "f[].textindex.text_id_to_anchor"
G_T2T, G_T2A = "g[].textindex.tokens_to_text_id", "g[].textindex.text_id_to_anchor"
F_KEY_BASE = 10


class LocalityCorpus:
    def __init__(self):
        self.t2t = {F_T2T: P.KVBuilder(), G_T2T: P.KVBuilder()}
        self.f_rows, self.g_rows = [], []  # text_id_to_anchor rows; f's first key is F_KEY_BASE
        self.jobs = {}

        def f_text(anchors):
            self.f_rows.append(anchors)
            return F_KEY_BASE + len(self.f_rows) - 1

        def g_text(anchors):
            self.g_rows.append(anchors)
            return len(self.g_rows) - 1

        def f_job(name, counts):
            self.jobs[name] = (F_T2T, F_T2A, P.rows_for_counts(self.t2t[F_T2T], counts))

        # ---- "runs": the sorted slice of this job, by position (it is the first job of its calls: positions are thread indexes of k_loc_expand)
        runs = [(3, 2), (f_text([90]), 1), (f_text([100]), 2), (f_text([100, 101, 102]), 3), (f_text(list(range(200, 210))), 64), (f_text([301, 300, 300]), 185),
                (f_text([400]), 300), (f_text([]), 2)]
        z = f_text([500, 501])
        runs.append((z, 2))
        ends = np.cumsum([c for _, c in runs]) - 1
        assert ends[5] == 256 and ends[5] - 185 + 1 < 256  # a run that starts in block 0 and ends on the first thread of block 1
        assert ends[6] - 300 + 1 < 512 <= ends[6]          # a run across blocks 1 and 2
        f_job("runs", dict(runs))
        self.runs_len = int(ends[-1]) + 1
        # ---- "next": its slice starts with the text the slice of "runs" ends with (3 times here, twice there); texts beyond the last key
        nxt = {z: 3, f_text([510]): 2, f_text([500, 511]): 4}
        # ---- "straddle": after the sort by (anchor, value), pairs 63 and 64 are anchor 2000 with 2*2*2 and 2*3*3: the first is kept
        st = {f_text([1000 + i]): 2 for i in range(63)}
        st[f_text([2000])] = 3
        st[f_text([2000])] = 2
        st.update({f_text([2001 + i]): 2 for i in range(10)})
        # ---- pairs per job: n texts twice, one anchor each; 0: texts that do not repeat
        pairs = {n: {f_text([3000 + 200 * k + i]): 2 for i in range(n)} for k, n in enumerate((1, 63, 64, 65, 129))}
        pairs[0] = {f_text([2990 + i]): 1 for i in range(5)}
        # ---- gather rows of 0 .. 1000 entries, each gathered twice
        rowlen = {n: [f_text([(4200 + 7 * i + n) % N_ANCHORS]) for i in range(n)] for n in (0, 1, 255, 256, 257, 1000)}
        last_key = F_KEY_BASE + len(self.f_rows) - 1
        nxt[last_key + 1] = 2
        nxt[last_key + 50] = 3
        f_job("next", nxt)
        f_job("straddle", st)
        for n, counts in pairs.items():
            f_job("pairs%d" % n, counts)
        for n, texts in rowlen.items():
            tok = self.t2t[F_T2T].add(texts)
            self.jobs["row%d" % n] = (F_T2T, F_T2A, [tok, tok])
        self.jobs["f_empty"] = (F_T2T, F_T2A, [])
        self.jobs["f_unknown_tokens"] = (F_T2T, F_T2A, [10 ** 6, 10 ** 6])
        # ---- the second field: its own tables
        g1 = {g_text([5000 + i, 5500 + i]): 2 + i % 3 for i in range(40)}
        g2 = {g_text([5100, 5600 - i]): 2 for i in range(3)}
        for name, counts in (("g1", g1), ("g2", g2)):
            self.jobs[name] = (G_T2T, G_T2A, P.rows_for_counts(self.t2t[G_T2T], counts))
        self.jobs["g_empty"] = (G_T2T, G_T2A, [])

        from veloci_amd.index import IndexData, csr_from_lists
        data = IndexData(N_ANCHORS)
        for path, b in self.t2t.items():
            data.add_key_value_store(path, *b.store())
        data.add_key_value_store(F_T2A, *csr_from_lists(self.f_rows), key_base=F_KEY_BASE)
        data.add_key_value_store(G_T2A, *csr_from_lists(self.g_rows))
        self.data = data
        self.refs = {}

    def ref(self, name, lo=0, hi=None):
        key = (name, lo, hi)
        if key not in self.refs:
            t2t, t2a, tokens = self.jobs[name]
            self.refs[key] = R.locality(self.data.key_value_stores[t2t], self.data.key_value_stores[t2a], tokens, lo, hi)
        return self.refs[key]


@pytest.fixture(scope="module")
def lcorpus():
    return LocalityCorpus()


@pytest.fixture(scope="module")
def lindex(lcorpus):
    return open_index(lcorpus.data)


def check_locality(idx, corpus, names, lo=0, hi=None):
    launches(idx)
    rc, got = P.run_locality(idx, [corpus.jobs[n] for n in names])
    assert rc == 0
    seen = launches(idx)
    assert seen.get("k_locality", 0) == 1, seen
    for name, (docs, bits) in zip(names, got):
        wd, wv = corpus.ref(name, lo, hi)
        check_list(("locality", name, lo, hi), docs, bits, wd, wv.view(np.uint32))


ALL_17 = ["pairs0", "pairs1", "g1", "pairs63", "f_empty", "pairs64", "row0", "row1", "pairs65", "g2", "row255", "row256", "pairs129", "row257", "row1000", "straddle", "g_empty"]


def test_locality_runs_across_blocks_and_job_slices(lcorpus, lindex):
    """k_loc_expand: the `jobs[mid].seg_begin <= i` job search, the end of a run (`ids[i + 1] == t` only inside the slice) and its start (lower bound inside
    [seg_begin, i]): runs of c = 1 (dropped), 2, 3, 64, one of 185 that ends on the first thread of the second 256-thread block, one of 300 across the
    next block edge, a run that ends its job's slice while the next slice starts with the same text; text ids below the text_id_to_anchor key base,
    beyond its last key, with an empty row.  k_loc_compact: the smaller of two values of one anchor.  One job and two jobs per call."""
    wd, wv = lcorpus.ref("runs")
    assert dict(zip(wd.tolist(), wv.tolist()))[100] == 8.0 and 90 not in wd and set(wv.tolist()) == {8.0, 18.0, 2.0 * 64 * 64, 2.0 * 185 * 185, 2.0 * 300 * 300}
    assert dict(zip(*[x.tolist() for x in lcorpus.ref("next")])) == {500: 18.0, 501: 18.0, 510: 8.0, 511: 32.0}
    check_locality(lindex, lcorpus, ["runs"])
    check_locality(lindex, lcorpus, ["runs", "next"])


def test_locality_pairs_rows_and_17_jobs_over_two_tables(lcorpus, lindex):
    """k_loc_gather rows of 0 / 1 / 255 / 256 / 257 / 1000 entries; k_loc_compact rounds of 64 pairs: 0 (len 0, sentinels written), 1, 63, 64, 65, 129 pairs,
    and one anchor at pair positions 63 and 64 (`sorted[i - 1]` across the round: the smaller value is kept once); 17 jobs in one call over two
    tokens_to_text_id tables (two gather launches), an empty job between two others and an empty job last"""
    assert [len(lcorpus.ref("pairs%d" % n)[0]) for n in (0, 1, 63, 64, 65, 129)] == [0, 1, 63, 64, 65, 129]
    assert [len(lcorpus.ref("row%d" % n)[0]) for n in (0, 1, 255, 256, 257, 1000)] == [0, 1, 255, 256, 257, 1000]
    wd, wv = lcorpus.ref("straddle")
    assert wd[63] == 2000 and wv[63] == 8.0 and wd[64] == 2001 and len(wd) == 74
    assert len(ALL_17) == 17
    check_locality(lindex, lcorpus, ALL_17)
    check_locality(lindex, lcorpus, ["pairs0", "f_unknown_tokens"])  # entries gathered, no pair: the lists are empty but written


def test_locality_without_any_entry_launches_nothing(lcorpus, lindex):
    """run_locality_jobs' early return: no job gathers anything, no kernel runs, every list is empty"""
    launches(lindex)
    rc, got = P.run_locality(lindex, [lcorpus.jobs["f_empty"], lcorpus.jobs["row0"]])
    assert rc == 0 and [len(d) - P.PAD for d, _ in got] == [0, 0] and "k_locality" not in launches(lindex)


def test_locality_lists_of_two_doc_range_shards(lcorpus):
    """text_id_to_anchor rows cut to the shard by the loader (d_row_start / d_row_len): each half's lists are the reference restricted to its range"""
    names = ["runs", "next", "straddle", "pairs129", "row1000", "g1", "g2"]
    whole = sum(len(lcorpus.ref(n)[0]) for n in names)
    halves = 0
    for lo, hi in ((0, 3100), (3100, N_ANCHORS)):
        idx = open_index(lcorpus.data, doc_lo=lo, doc_hi=hi)
        check_locality(idx, lcorpus, names, lo, hi)
        halves += sum(len(lcorpus.ref(n, lo, hi)[0]) for n in names)
        idx.close()
    assert halves == whole and 0 < len(lcorpus.ref("row1000", 0, 3100)[0]) < 1000


# ================================================================================================================================ 1:n boost lists
TO_PARENT, TO_ANCHOR = "tags[].name.textindex.value_id_to_parent", "tags[].rank.value_id_to_anchor"
RANK, PRIO = "tags[].rank.boost_valid_to_value", "tags[].prio.boost_valid_to_value"
A_BASE, A_END = 3, 3400   # value ids value_id_to_anchor knows
B_BASE, B_END = 5, 3390   # value ids the boost columns know
B1N_SHARD = (150, 2999)


def b1n_anchor_row(v):
    if 100 <= v < 3000:
        return [] if v % 4 == 3 else ([v, v + 7] if v % 10 == 0 else [v])
    if 3000 <= v < 3100:
        return [10 + v - 3000]   # low anchors: a step down behind any id below 3000
    if 3200 <= v < 3300:
        return [2998]            # the anchor of value id 2998
    if 3300 <= v < 3400:
        return [v + 1000]
    return [v]


class Boost1nCorpus:
    def __init__(self):
        from veloci_amd.index import IndexData, csr_from_lists
        rng = np.random.default_rng(31)
        self.parent = P.KVBuilder(key_base=2)
        self.jobs = {}
        ids = np.arange(B_BASE, B_END)
        present = np.where((ids >= 100) & (ids < 3000) & (ids % 4 == 1), 0, 1).astype(np.uint8)  # `rank`: ids 4k + 1 below 3000 have no value

        def job(name, vids, col=RANK):
            vids = rng.permutation(np.asarray(vids, np.int64))
            cuts = sorted(rng.integers(0, len(vids) + 1, size=2).tolist())
            texts = [self.parent.add(part) for part in (vids[:cuts[0]], vids[cuts[0]:cuts[1]], vids[cuts[1]:])]
            self.jobs[name] = (TO_PARENT, TO_ANCHOR, col, [0, 10 ** 6] + texts)  # (text ids outside value_id_to_parent are skipped)

        evens = lambda n, first=100: list(range(first, first + 2 * n, 2))
        odds = lambda n, first=101: list(range(first, first + 2 * n, 2))
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
            job("n%d" % n, rng.choice(np.arange(100, 3000), size=n, replace=False))
        job("all_kept", evens(300))
        job("none_kept", odds(300))
        job("kept_63_64", odds(63) + [226, 228] + odds(40, 229))          # sorted positions 63 and 64 are the only boosted ids
        job("kept_255_256", odds(255) + [610, 612] + odds(43, 613))       # the last of one 256-round, the first of the next
        job("down_63_64", evens(64) + list(range(3000, 3020)))            # anchors 100 .. 226, then 10 ..: one step down, across positions 63 / 64
        job("down_255_256", evens(256) + list(range(3000, 3010)))
        job("equal_63_64", evens(63) + [2998, 3200] + list(range(3300, 3310)))    # anchor 2998 at positions 63 and 64
        job("equal_255_256", evens(255) + [2998, 3200] + list(range(3300, 3305)))
        job("ascending", evens(150))
        job("outside", [0, 1, 2, 3, 4, 50, 60, 3389, 3390, 3395, 3399, 3400, 5000])
        job("duplicates", [200, 204, 208, 204])
        job("prio_n257", rng.choice(np.arange(100, 3000), size=257, replace=False), PRIO)
        job("prio_odds", odds(300), PRIO)
        data = IndexData(N_ANCHORS)
        data.add_key_value_store(TO_PARENT, *self.parent.store(), key_base=2)
        data.add_key_value_store(TO_ANCHOR, *csr_from_lists([b1n_anchor_row(v) for v in range(A_BASE, A_END)]), key_base=A_BASE)
        data.add_boost(RANK, (ids * 0.25 + 1).astype(np.float32), present=present, key_base=B_BASE)
        data.add_boost(PRIO, (-ids).astype(np.float32), key_base=B_BASE)
        self.data = data
        self.refs = {}

    def ref(self, name, lo=0, hi=None):
        key = (name, lo, hi)
        if key not in self.refs:
            tp, ta, col, texts = self.jobs[name]
            self.refs[key] = R.boost1n(self.data.key_value_stores[tp], self.data.key_value_stores[ta], self.data.boost[col], texts, lo, hi)
        return self.refs[key]


@pytest.fixture(scope="module")
def bcorpus():
    return Boost1nCorpus()


def check_boost1n(idx, corpus, names, lo=0, hi=None):
    launches(idx)
    rc, got = P.run_boost1n(idx, [corpus.jobs[n] for n in names])
    assert rc == 0
    seen = launches(idx)
    assert seen.get("k_boost1n", 0) == 1, seen
    for name, (docs, bits, total, ascending, several) in zip(names, got):
        wd, wb, wtotal, wasc, wsev = corpus.ref(name, lo, hi)
        check_list(("boost1n", name, lo, hi), docs, bits, wd, wb)
        assert (total, ascending, several) == (wtotal, wasc, wsev), (name, (total, ascending, several), (wtotal, wasc, wsev))


def test_boost1n_lists_flags_and_keep_patterns(bcorpus):
    """k_b1n_map: rounds of 4 x 64 value ids (0 .. 1000 ids per job), the compaction `written + popc(ms & below)` with all / no / only positions 63, 64 /
    only positions 255, 256 kept, the pair in front handed from ballot to ballot and round to round (`before = below ? got : prev`): a step down and
    an equal pair exactly across positions 63 / 64 and 255 / 256 set `flags` bit 0 / bit 1, a strictly ascending list sets neither; value ids
    outside either key range; a boost column with and without a `present` bitmap; every job of the file in one call (a workgroup per job)."""
    r = bcorpus.ref
    assert r("n0")[2] == 0 and len(r("n0")[0]) == 0 and 0 < r("n1000")[2] < 1000
    assert r("all_kept")[2] == 300 and r("none_kept")[2] == 0 and r("kept_63_64")[2] == 2 and r("kept_255_256")[2] == 2
    assert r("down_63_64")[2:] == (84, False, False) and r("down_255_256")[2:] == (266, False, False)
    assert r("equal_63_64")[2:] == (75, True, True) and r("equal_255_256")[2:] == (262, True, True)
    assert r("ascending")[2:] == (150, True, False) and r("duplicates")[2:] == (4, True, True)
    assert r("outside")[0].tolist() == [50, 60, 4389] and r("prio_odds")[2] == 150
    idx = open_index(bcorpus.data)
    check_boost1n(idx, bcorpus, sorted(bcorpus.jobs))
    check_boost1n(idx, bcorpus, ["n0"])
    check_boost1n(idx, bcorpus, ["down_63_64", "n0", "equal_255_256"])
    idx.close()


def test_boost1n_lists_of_a_doc_range_shard(bcorpus):
    """k_b1n_map's `in_shard` compaction: a shard keeps a strict subset in value-id order (len < total) while total and the flags speak of the whole list"""
    lo, hi = B1N_SHARD
    wd, _, total, _, _ = bcorpus.ref("all_kept", lo, hi)
    assert 0 < len(wd) < total and len(bcorpus.ref("down_63_64", lo, hi)[0]) < 84
    idx = open_index(bcorpus.data, doc_lo=lo, doc_hi=hi)
    check_boost1n(idx, bcorpus, sorted(bcorpus.jobs), lo, hi)
    idx.close()
