"""vq_highlight_batch: n highlight parts as one device batch.  A part with `snippet` and its own `top` has its texts ranked and cut to the page
on the device (k_text_best / k_text_select, veloci_amd/csrc/text_rank.hip) and only the page's snippets built.  Every result — snippets byte
for byte, f32 scores bit for bit, text ids, order, error code — must equal vq_highlight_json's for the same part and the CPU oracle's; the two
kernels alone are driven over crafted CSRs against a numpy restatement (max per text, then a sort by (-score, text))."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import highlightcorpus as HC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = int(os.environ.get("VQ_TEST_SEED", "4711"))
SPLIT = 4096  # kTextRankSplit (kernels.hpp)


class Corpus:
    def __init__(self, data):
        import veloci_amd
        from oracle import binding as O
        self.data = data
        self.idx = veloci_amd.Index(data, device=0)
        self.ora = O.OracleIndex(data.num_anchors)
        data.load_into(self.ora)
        self.O = O
        self.want_cache = {}

    def counters(self):
        from veloci_amd import _lib
        a, b = C.c_uint64(), C.c_uint64()
        _lib.lib().vq_index_highlight_rank_counts(self.idx.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def want(self, part):
        """the oracle's answer, computed once per part text: the bits, or the error's code"""
        js = HC.as_text(part)
        if js not in self.want_cache:
            try:
                self.want_cache[js] = HC.bits(self.ora.highlight_json(js))
            except self.O.OracleError as e:
                self.want_cache[js] = ("error", e.code)
        return self.want_cache[js]

    def check(self, parts):
        """batch == single == oracle, part by part; -> the batch's answers"""
        import veloci_amd
        got = veloci_amd.highlight_batch(parts, self.idx, raise_on_error=False)
        assert len(got) == len(parts)
        for k, (p, g) in enumerate(zip(parts, got)):
            try:
                single = HC.bits(veloci_amd.highlight(p, self.idx))
            except veloci_amd.VelociError as e:
                assert isinstance(g, veloci_amd.VelociError) and g.code == e.code, (k, p, g, e.code, str(e))
                assert isinstance(self.want(p), tuple), (k, p, self.want(p))
                continue
            assert not isinstance(g, veloci_amd.VelociError), (k, p, g.code)
            assert HC.bits(g) == single, (k, p, HC.bits(g)[:6], single[:6])
            assert single == self.want(p), (k, p, single[:6], self.want(p)[:6])
        return got


@pytest.fixture(scope="module")
def corpus():
    data, info = HC.build()
    assert len(info["title"]["terms"]) > 300 and "tags[]" in info and "sub[].text" in info
    return Corpus(data)


@pytest.fixture(scope="module")
def reference_corpus():
    import refcases
    data, docs, info = refcases.build("test_all")
    return Corpus(data)


def test_fixed_parts_batch_equals_single_equals_oracle(corpus):
    parts = HC.fixed_parts()
    d0, s0 = corpus.counters()
    got = corpus.check(parts)
    d1, s1 = corpus.counters()
    assert d1 - d0 >= 30 and s1 > s0, (d0, d1, s0, s1)
    assert sum(len(g) for g in got if isinstance(g, list)) > 1000
    tie = got[parts.index(HC.part("title", "tieword", top=10))]
    assert len(tie) == 10 and len({s for _, s, _ in tie}) == 1 and [i for _, _, i in tie] == sorted(i for _, _, i in tie)


def test_frequent_token_prefix_builds_the_page_only(corpus):
    import veloci_amd
    everything = dict(HC.FREQUENT)
    del everything["top"]
    matched = veloci_amd.highlight(everything, corpus.idx)
    assert len(matched) > 300  # the single call ranks (and builds a snippet for) every one of them
    d0, s0 = corpus.counters()
    got = veloci_amd.highlight_batch([HC.FREQUENT], corpus.idx)[0]
    d1, s1 = corpus.counters()
    assert HC.bits(got) == HC.bits(matched)[:10]
    assert d1 - d0 == 1 and s1 - s0 <= 10, (d1 - d0, s1 - s0)


def test_reference_highlight_parts(reference_corpus):
    import test_reference_integration as TRI
    parts = TRI.highlight_parts()
    got = reference_corpus.check(parts)
    assert sum(1 for g in got if isinstance(g, list)) > 150
    with_top = [dict(p, top=top, skip=skip) for p in parts[::3] for top, skip in ((1, 0), (3, 1))]
    d0, _ = reference_corpus.counters()
    reference_corpus.check(with_top)
    assert reference_corpus.counters()[0] > d0


def test_random_parts(corpus):
    parts = HC.random_parts(200, SEED)
    d0, _ = corpus.counters()
    got = corpus.check(parts)
    assert corpus.counters()[0] - d0 > 40
    assert sum(1 for g in got if isinstance(g, list) and g) > 80


@pytest.mark.parametrize("n", [0, 1, 2, 17, 300])
def test_batch_sizes_with_duplicates(corpus, n):
    pool = HC.fixed_parts()
    parts = [pool[(7 * k) % len(pool)] for k in range(n)]  # 300 over a pool of about 50: every part several times
    got = corpus.check(parts)
    assert len(got) == n


def test_failing_parts_fail_alone(corpus):
    import veloci_amd
    good = [HC.FREQUENT, HC.part("tags[]", "nice", top=10)]
    parts = [good[0]]
    for f in HC.FAILING:
        parts += [f, good[len(parts) % 2]]
    got = corpus.check(parts)
    bad = [k for k, g in enumerate(got) if isinstance(g, veloci_amd.VelociError)]
    assert bad == [1, 3, 5, 7, 9], bad
    assert len({got[k].code for k in bad}) >= 3, [got[k].code for k in bad]  # JSON, unknown field, invalid request
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.highlight_batch(parts, corpus.idx)
    assert e.value.code == got[1].code and str(e.value).startswith("JsonError"), str(e.value)


def test_host_route_parts_inside_a_device_batch(corpus):
    parts = [HC.FREQUENT] + HC.HOST_ROUTE + [HC.FREQUENT]
    d0, _ = corpus.counters()
    got = corpus.check(parts)
    assert corpus.counters()[0] - d0 == 2  # boost -1, boost 0 and the part without top stay on the host route
    assert len(got[0]) == len(got[-1]) == 10 and len(got[2]) == 10 and len(got[3]) > 50  # (boost 0: every score ties; no top: every text)


def test_field_that_fails_the_store_check_stays_on_the_host_route(corpus):
    import veloci_amd
    broken = [p for p in HC.BROKEN if p["path"] == "broken"]
    whole = [p for p in HC.BROKEN if p["path"] == "whole"]
    d0, _ = corpus.counters()
    got = corpus.check(broken)
    assert corpus.counters()[0] == d0
    assert isinstance(got[0], veloci_amd.VelociError) and isinstance(got[1], list) and len(got[1]) == 1  # text 3 has no snippet; `beta` reaches text 2 alone
    got = corpus.check(whole)  # the same relation with every row in place, an identity column: staged on first use, the device route
    assert corpus.counters()[0] - d0 == len(whole)
    assert [len(g) for g in got] == [2, 1, 1]


CHILD = r"""
import ctypes as C, json, sys
import veloci_amd
from veloci_amd import _lib
import highlightcorpus as HC
parts = json.load(open(sys.argv[1]))
data, _ = HC.build()
idx = veloci_amd.Index(data, device=0)
got = veloci_amd.highlight_batch(parts, idx, raise_on_error=False)
a, b = C.c_uint64(), C.c_uint64()
_lib.lib().vq_index_highlight_rank_counts(idx.h, C.byref(a), C.byref(b))
print("HOST_ROUTE " + json.dumps({"device_parts": a.value, "snippets_built": b.value,
                                  "answers": [None if isinstance(g, veloci_amd.VelociError) else HC.bits(g) for g in got]}))
"""


def test_knob_keeps_every_part_on_the_host_route(corpus, tmp_path):
    import veloci_amd as V
    parts = HC.fixed_parts() + HC.FAILING
    got = V.highlight_batch(parts, corpus.idx, raise_on_error=False)
    path = tmp_path / "parts.json"
    path.write_text(json.dumps(parts))
    env = dict(os.environ, VQ_NO_HIGHLIGHT_RANK="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    child = subprocess.run([sys.executable, "-c", CHILD, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0 and "HOST_ROUTE " in child.stdout, child.stdout[-2000:] + child.stderr[-3000:]
    host = json.loads(child.stdout.split("HOST_ROUTE ", 1)[1])
    assert host["device_parts"] == 0 and host["snippets_built"] > 0, (host["device_parts"], host["snippets_built"])
    assert host["answers"] == [None if isinstance(g, V.VelociError) else [list(x) for x in HC.bits(g)] for g in got]


# ------------------------------------------------------------------------------------------------ the kernels alone
def device_rank(rows, scores, num_texts, top_n):
    """rows: lists of text ids; scores: one f32 per row -> ([(text, bits)], touched) or the return code"""
    from veloci_amd import _lib
    L = _lib.lib()
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    vals = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32), np.uint32)
    bits = np.ascontiguousarray(np.asarray(scores, np.float32).view(np.uint32))
    out_t, out_b = np.zeros(max(top_n, 1), np.uint32), np.zeros(max(top_n, 1), np.uint32)
    n, touched = C.c_uint32(), C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.vq_debug_text_rank(p(off), p(vals), p(bits), len(rows), num_texts, top_n, p(out_t), p(out_b), C.byref(n), C.byref(touched))
    if rc != 0:
        return rc
    return list(zip(out_t[:n.value].tolist(), out_b[:n.value].tolist())), touched.value


def numpy_rank(rows, scores, num_texts, top_n):
    best = np.zeros(num_texts, np.float32)
    for r, s in zip(rows, scores):
        if len(r):
            np.maximum.at(best, np.asarray(r, np.int64), np.float32(s))
    texts = np.nonzero(best)[0]
    order = np.lexsort((texts, -best[texts].astype(np.float64)))
    picked = texts[order][:top_n]
    return list(zip(picked.tolist(), best[picked].view(np.uint32).tolist())), len(texts)


def score_sets(rng, n):
    one = np.float32(7.5).view(np.uint32)
    yield "all equal", np.full(n, 7.5, np.float32)
    yield "lowest mantissa byte", (one + rng.integers(0, 256, size=n).astype(np.uint32)).view(np.float32)
    yield "top byte", ((rng.integers(1, 0x7F, size=n).astype(np.uint32) << 24) | np.uint32(0x00345678)).view(np.float32)
    yield "random over 8", np.asarray([0.5, 1.0, 1.5, 2.0, 3.25, 10.0, 10.000001, 400.0], np.float32)[rng.integers(0, 8, size=n)]


def crafted_rows(rng, num_texts):
    """rows of lengths 0, 1, 63, 64, 65 and one of at least three split lengths; texts repeat inside a row and across rows"""
    rows = [rng.integers(0, num_texts, size=k).tolist() for k in (0, 1, 63, 64, 65, 7, 300)]
    rows.append(rng.integers(0, num_texts, size=3 * SPLIT + 5).tolist())
    rows.append([int(rows[2][0])] * 3 + [int(rows[3][1])])  # the same text three times in one row, and texts of other rows again
    rows.append([num_texts - 1, 0])
    return rows


@pytest.mark.parametrize("num_texts", [1, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_text_rank_kernels_on_crafted_rows(num_texts):
    rng = np.random.default_rng(SEED + num_texts)
    rows = crafted_rows(rng, num_texts)
    ran = 0
    for name, scores in score_sets(rng, len(rows)):
        assert np.isfinite(scores).all() and (scores > 0).all()
        _, touched = numpy_rank(rows, scores, num_texts, 1)
        for top_n in sorted({1, 10, max(touched - 1, 1), touched, min(touched + 1, 1024), 1024}):
            if not 1 <= top_n <= 1024:
                continue
            want = numpy_rank(rows, scores, num_texts, top_n)
            got = device_rank(rows, scores, num_texts, top_n)
            assert got == want, (num_texts, name, top_n, got if isinstance(got, int) else (got[1], want[1], [k for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:5]))
            ran += 1
    assert ran >= 12


def test_text_rank_kernels_sparse_rows_and_ties_across_the_cut():
    """few touched texts among many, every score equal: the page is the touched texts with the smallest ids, whatever piece of the array they lie in"""
    rng = np.random.default_rng(SEED)
    num_texts = 4099
    texts = rng.choice(num_texts, size=1500, replace=False)
    rows = [texts[:700].tolist(), texts[700:].tolist(), []]
    for top_n in (1, 10, 699, 1024):
        for scores in ([2.0, 2.0, 1.0], [1.0, 2.0, 3.0], [2.0, 1.0, 1.0]):
            assert device_rank(rows, scores, num_texts, top_n) == numpy_rank(rows, scores, num_texts, top_n), (top_n, scores)
    assert device_rank([[], []], [1.0, 2.0], 100, 10) == ([], 0)  # nothing touched


def test_text_rank_refuses_arguments_outside_its_range():
    ok = ([[0, 1, 2]], [1.0], 8)
    assert device_rank(*ok, 1) == ([(0, np.float32(1.0).view(np.uint32).item())], 3)
    assert device_rank(*ok, 0) == -2 and device_rank(*ok, 1025) == -2
    assert device_rank([[0, 8]], [1.0], 8, 1) == -2           # a text id outside num_texts
    assert device_rank([[0]], [1.0], 0, 1) == -2
    assert device_rank([[0]], [1.0], (128 << 20) // 4 + 1, 1) == -2  # beyond the workspace budget
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert device_rank([[0]], [bad], 8, 1) == -2, bad
