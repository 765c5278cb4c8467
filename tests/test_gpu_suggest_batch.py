"""vq_suggest_batch: n suggest requests as one device batch, the leaf top-n loop of a part with its own `top` run on the device (k_dict_topn,
veloci_amd/csrc/dict_topn.hip).  Every result — texts, f32 scores bit for bit, term ids, order — must equal vq_suggest_json's for the same
request and the CPU oracle's; the kernel alone is driven over crafted streams against the reference's loop (search_field.rs:322-333 +
sort.rs:25-34) written out here."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import suggestcorpus as SC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = int(os.environ.get("VQ_TEST_SEED", "4711"))


class Corpus:
    def __init__(self):
        import veloci_amd
        from oracle import binding as O
        self.data, self.terms = SC.build()
        self.idx = veloci_amd.Index(self.data, device=0)
        self.ora = O.OracleIndex(self.data.num_anchors)
        self.data.load_into(self.ora)
        self.O = O
        self.want_cache = {}

    def counters(self):
        from veloci_amd import _lib
        a, b = C.c_uint64(), C.c_uint64()
        _lib.lib().vq_index_suggest_topn_probes(self.idx.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def want(self, req):
        """the oracle's answer, computed once per request text: the bits, or the error's code"""
        js = SC.as_text(req)
        if js not in self.want_cache:
            try:
                self.want_cache[js] = SC.bits(self.ora.suggest_json(js))
            except self.O.OracleError as e:
                self.want_cache[js] = ("error", e.code)
        return self.want_cache[js]

    def check(self, reqs):
        """batch == single == oracle, request by request; -> the batch's answers"""
        import veloci_amd
        got = veloci_amd.suggest_batch(reqs, self.idx, raise_on_error=False)
        assert len(got) == len(reqs)
        for k, (r, g) in enumerate(zip(reqs, got)):
            try:
                single = SC.bits(veloci_amd.suggest(r, self.idx))
            except veloci_amd.VelociError as e:
                assert isinstance(g, veloci_amd.VelociError) and g.code == e.code, (k, r, g, e.code, str(e))
                assert isinstance(self.want(r), tuple), (k, r, self.want(r))
                continue
            assert not isinstance(g, veloci_amd.VelociError), (k, r, g.code)
            assert SC.bits(g) == single, (k, r, SC.bits(g)[:12], single[:12])
            assert single == self.want(r), (k, r, single[:12], self.want(r)[:12])
        return got


@pytest.fixture(scope="module")
def corpus():
    c = Corpus()
    a = c.terms["a"]
    assert [SC.count_prefix(a, h) for h, _ in SC.PLANTED] == [n for _, n in SC.PLANTED]
    assert SC.count_prefix(a, "w") == SC.N_W and SC.count_prefix(a, "zz") == SC.N_ZZ and len(a) >= 3000 and len(c.terms["b"]) >= 2500
    return c


def test_fixed_requests_batch_equals_single_equals_oracle(corpus):
    reqs = SC.fixed_requests()
    before = corpus.counters()
    got = corpus.check(reqs)
    after = corpus.counters()
    assert after[0] > before[0]
    assert sum(len(g) for g in got) > 1000
    # the planted prefixes with top 1: all of them answer one entry
    for head, _ in SC.PLANTED:
        assert len(got[reqs.index(SC.part("b", head, starts_with=True, top=1, skip=0))]) == 1


@pytest.mark.parametrize("n", [0, 1, 2, 17, 300])
def test_batch_sizes(corpus, n):
    pool = SC.fixed_requests()
    got = corpus.check([pool[(7 * k) % len(pool)] for k in range(n)])
    assert len(got) == n


def test_top_0_over_200_or_more_matches_batch_equals_single(corpus):
    """top + skip == 0 on a prefix with 200 or more matches: the reference panics there, so the oracle is left out; such a part is on the full
    route, keeps nothing, and the batch must answer what the single call answers, also beside parts that keep something."""
    import veloci_amd
    P = SC.part
    bare = [P("a", head, starts_with=True, top=0, skip=skip) for head in ("w", "zz", "qa", "qb", "qc") for skip in (None, 0)]
    beside = [{"suggest": [P("a", "w", starts_with=True, top=0), P("a", "zz", starts_with=True, top=10)], "top": 10},
              {"suggest": [P("b", "w", starts_with=True, top=0, skip=0), P("a", "w", starts_with=True, top=10), P("a", "w", starts_with=True, top=0)], "top": 5, "skip": 1}]
    reqs = bare + beside
    got = veloci_amd.suggest_batch(reqs, corpus.idx)
    for r, g in zip(reqs, got):
        assert SC.bits(g) == SC.bits(veloci_amd.suggest(r, corpus.idx)), r
    assert all(len(g) == 0 for g in got[:len(bare)]) and [len(g) for g in got[len(bare):]] == [10, 5]


def test_failing_requests_fail_alone(corpus):
    import veloci_amd
    good = [SC.part("a", "w", starts_with=True, top=10), {"suggest": [SC.part("b", "zz", starts_with=True, top=3)], "top": 3}]
    reqs = [good[0]]
    for f in SC.FAILING:
        reqs += [f, good[len(reqs) % 2]]
    got = corpus.check(reqs)
    bad = [k for k, g in enumerate(got) if isinstance(g, veloci_amd.VelociError)]
    assert bad == [1, 3, 5, 7], bad
    assert len({got[k].code for k in bad}) >= 3, [got[k].code for k in bad]  # JSON, unknown field, invalid request
    with pytest.raises(veloci_amd.VelociError) as e:
        veloci_amd.suggest_batch(reqs, corpus.idx)
    assert e.value.code == got[1].code and str(e.value).startswith("JsonError"), str(e.value)


def test_random_batch_takes_the_topn_route_and_copies_less_back(corpus, tmp_path):
    reqs = SC.random_requests(300, SEED, corpus.terms)
    p0, r0 = corpus.counters()
    got = corpus.check(reqs)
    p1, r1 = corpus.counters()
    print("top-n probes", p1 - p0, "records copied back", r1 - r0)
    assert p1 - p0 > 0
    # one request, the 2500-match prefix with top 10: at most top + skip + 200 records come back (the loop's buffer), not the match set
    import veloci_amd
    one = SC.part("a", "w", starts_with=True, top=10)
    assert len(veloci_amd.suggest_batch([one], corpus.idx)[0]) == 10
    p2, r2 = corpus.counters()
    assert p2 - p1 == 1 and r2 - r1 <= 210, (p2 - p1, r2 - r1)
    # VQ_NO_SUGGEST_TOPN=1 in a child process: the same answers, no top-n probe
    path = tmp_path / "reqs.json"
    path.write_text(json.dumps(reqs))
    env = dict(os.environ, VQ_NO_SUGGEST_TOPN="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    child = subprocess.run([sys.executable, "-c", CHILD, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0 and "FULL_ROUTE " in child.stdout, child.stdout[-2000:] + child.stderr[-3000:]
    full = json.loads(child.stdout.split("FULL_ROUTE ", 1)[1])
    assert full["topn_probes"] == 0 and full["records"] > 0, (full["topn_probes"], full["records"])
    import veloci_amd as V
    mine = [None if isinstance(g, V.VelociError) else [list(x) for x in SC.bits(g)] for g in got]
    assert full["answers"] == mine


CHILD = r"""
import ctypes as C, json, sys
import veloci_amd
from veloci_amd import _lib
import suggestcorpus as SC
reqs = json.load(open(sys.argv[1]))
data, terms = SC.build()
idx = veloci_amd.Index(data, device=0)
got = veloci_amd.suggest_batch(reqs, idx, raise_on_error=False)
a, b = C.c_uint64(), C.c_uint64()
_lib.lib().vq_index_suggest_topn_probes(idx.h, C.byref(a), C.byref(b))
print("FULL_ROUTE " + json.dumps({"topn_probes": a.value, "records": b.value,
                                  "answers": [None if isinstance(g, veloci_amd.VelociError) else SC.bits(g) for g in got]}))
"""


# ------------------------------------------------------------------------------------------------ the kernel alone
def class_scores():
    from oracle import binding as O
    return np.array([O.default_score_for_distance(c >> 1, bool(c & 1)) for c in range(512)], np.float32)


def reference_loop(terms, classes, top_n, score):
    """search_field.rs:322-333 + sort.rs:25-34: the buffer as the reference leaves it, in buffer order (comparator: score desc, id desc)"""
    buf, worst = [], -np.inf
    for t, c in zip(terms.tolist(), classes.tolist()):
        s = float(score[c])
        if s < worst:
            continue
        if buf and len(buf) == top_n + 200:
            buf.sort(key=lambda e: (-e[0], -e[1]))
            del buf[top_n:]
            worst = buf[-1][0]
        buf.append((s, t, c))
    return [(t, c) for _, t, c in buf]


def device_loop(terms, classes, top_n):
    from veloci_amd import _lib
    L = _lib.lib()
    terms = np.ascontiguousarray(terms, np.uint32)
    classes = np.ascontiguousarray(classes, np.uint32)
    out_t, out_c, out_n = np.zeros(top_n + 200, np.uint32), np.zeros(top_n + 200, np.uint32), C.c_uint32()
    rc = L.vq_debug_dict_topn(terms.ctypes.data_as(C.c_void_p), classes.ctypes.data_as(C.c_void_p), len(terms), top_n, out_t.ctypes.data_as(C.c_void_p),
                              out_c.ctypes.data_as(C.c_void_p), C.byref(out_n))
    assert rc == 0, rc
    return list(zip(out_t[:out_n.value].tolist(), out_c[:out_n.value].tolist()))


def ids(rng, n):
    return np.cumsum(rng.integers(1, 9, size=n)).astype(np.uint32)  # ascending term ids with gaps


def sequences(rng, n):
    """class sequences of n matches; scores of the classes used here: 0/1 best (10.0), then falling with the class (2 and 3 tie)"""
    ramp = np.linspace(0, 1, n) if n else np.zeros(0)
    yield "all equal", np.full(n, 6, np.uint32)
    yield "improving", (2 * np.floor((1 - ramp) * 255)).astype(np.uint32)   # everything passes: a cut every 200 pushes
    yield "worsening", (2 * np.floor(ramp * 255)).astype(np.uint32)         # after the first cut everything is skipped
    yield "alternating", np.where(np.arange(n) % 2 == 0, 4, 9).astype(np.uint32)
    yield "random over 8", rng.integers(0, 8, size=n).astype(np.uint32)
    yield "random over 300", rng.integers(0, 300, size=n).astype(np.uint32)


@pytest.mark.parametrize("top_n", [1, 10, 56, 1848])
def test_topn_kernel_on_crafted_streams(top_n):
    score = class_scores()
    assert score[0] == score[1] == 10.0 and score[2] == score[3] and (np.diff(score[2::2]) < 0).all()
    rng = np.random.default_rng(SEED + top_n)
    ran = 0
    for n in [0, 1, 63, 64, 65, top_n + 199, top_n + 200, top_n + 201, top_n + 264, top_n + 265, 20000 if top_n != 56 else 7777]:
        t = ids(rng, n)
        for name, cls in sequences(rng, n):
            want = reference_loop(t, cls, top_n, score)
            got = device_loop(t, cls, top_n)
            assert got == want, (top_n, n, name, len(got), len(want), [k for k, (a, b) in enumerate(zip(got, want)) if a != b][:5])
            ran += 1
    assert ran == 66


@pytest.mark.parametrize("lane", [0, 63, 29])
def test_topn_kernel_cut_inside_a_step(lane):
    """The second cut is fired by the match at `lane` of a 64-match step; behind it, in the same step, sit matches that passed the old worst
    score and that the new one rejects (and better ones that it keeps)."""
    top_n, good, better = 10, 6, 2
    score = class_scores()
    assert score[better] > score[good] > score[40]
    first = [good] * 211                      # fills the buffer (210) and fires the first cut at index 210: worst = score[good]
    fire_at = 448 + lane                      # index of the match that fires the second cut
    body = [better] * 12 + [good] * 187       # 199 pushes behind the 11 kept: the buffer is full again, 12 better entries in it
    pad = [40] * (fire_at - len(first) - len(body))  # below worst: skipped, they only move the step boundary
    cls = first + pad + body
    assert len(cls) == fire_at and len(pad) > 0
    cls += [good]                              # fires the cut: worst becomes score[better]; pushed all the same
    cls += [good, better, good, good, better, 0, good, 40, 1] * 30  # the lanes behind it: `good` is now rejected
    cls = np.asarray(cls, np.uint32)
    t = ids(np.random.default_rng(lane), len(cls))
    want = reference_loop(t, cls, top_n, score)
    got = device_loop(t, cls, top_n)
    assert got == want, [k for k, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert sum(1 for _, c in want if c == good) == 1  # only the match that fired the cut


def test_topn_kernel_refuses_what_it_cannot_hold():
    from veloci_amd import _lib
    L = _lib.lib()
    z = np.zeros(4, np.uint32)
    out = np.zeros(4096, np.uint32)
    n = C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.vq_debug_dict_topn(p(z), p(z), 4, 0, p(out), p(out), C.byref(n)) == -2
    assert L.vq_debug_dict_topn(p(z), p(z), 4, 1849, p(out), p(out), C.byref(n)) == -2
    assert L.vq_debug_dict_topn(p(z), p(np.full(4, 512, np.uint32)), 4, 10, p(out), p(out), C.byref(n)) == -2
