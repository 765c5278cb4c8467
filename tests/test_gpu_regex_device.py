"""Regex leaves scanned on the device (k_dict_regex, veloci_amd/csrc/dict_regex.hip): a DFA compiled on the host from the pattern and the
dictionary's alphabet, walked by one lane per term.  Results — ids and scores bit for bit — against the CPU oracle on an ASCII corpus (its regex
is byte-wise) and, on every corpus, against the host route (std::wregex over every term) taken from a child process with VQ_NO_REGEX_DEVICE=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LONG = "m" * 4999 + "z"  # 5000 code points: beyond the kernel's staging buffer, walked from HBM


def _add_field(data, field, lists, seed):
    """a second text field beside widecorpus.crafted's `body`"""
    rng = np.random.default_rng(seed)
    terms = sorted(t.encode() for t in lists)
    per = [np.sort(np.asarray(lists[t.decode()], np.int64)) for t in terms]
    offsets = np.zeros(len(terms) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in per])
    anchors = np.concatenate(per).astype(np.uint32)
    data.add_fst(field + ".textindex", terms)
    data.add_token_to_anchor_score(field + ".textindex.to_anchor_id_score", offsets, anchors, rng.integers(1, 200, size=len(anchors)).astype(np.uint32), None)
    data.add_key_value_store(field + ".textindex.text_id_to_anchor", offsets, anchors)


def build_corpus(name):
    """ascii: 2 x 2048 + 37 terms (k_dict_regex: a block boundary and a partial last round) of 1..40 code points and one of 5000
    astral: a small dictionary with code points above U+FFFF (the u32 image)          latin: Latin-1 and Greek terms"""
    import widecorpus
    rng = np.random.default_rng({"ascii": 41, "astral": 42, "latin": 43}[name])
    docs = 6000
    if name == "ascii":
        words = {"foo", "foobar", "barbazx", "bazfoo", "abde", "abcde", "bcdxe", "ab", "abc", "a", "Ab", "ABDE", "q", "qqz", LONG, "m" * 35 + "z", "x9", "42", "7up"}
        alpha = np.frombuffer(b"abcdefgmoqrxzABFZ0159", np.uint8)
        while len(words) < 2 * 2048 + 37:
            words.add(bytes(alpha[rng.integers(0, len(alpha), size=int(rng.integers(1, 41)))]).decode())
        lists = {w: rng.choice(docs, size=int(rng.integers(1, 5)), replace=False) for w in sorted(words)}
        data, terms = widecorpus.crafted(docs, lists)
        _add_field(data, "title", {"red%02d" % i: rng.choice(docs, size=3, replace=False) for i in range(40)}, 9)
        ids = {t: i for i, t in enumerate(terms)}
        pairs = sorted((ids[a.encode()], ids[b.encode()]) for a, b in (("foo", "foobar"), ("ab", "abc"), ("abde", "abcde")))
        offs = np.arange(len(pairs) + 1, dtype=np.uint64) * 2
        data.add_phrase_pair_to_anchor("body.textindex.phrase_pair_to_anchor", [p[0] for p in pairs], [p[1] for p in pairs], offs,
                                       np.sort(rng.choice(docs, size=(len(pairs), 2), replace=False), axis=1).ravel())
        return data, terms
    if name == "astral":
        words = ["a", "ab", "x\U0001F600y", "\U0001F600", "\U00010400\U00010428", "\U00010428", "\U00010400", "éa", "東京", "z\U0010FFFF", "\U0001F601\U0001F600\U0001F601",
                 "q" * 3000 + "\U0001F600", "K", "k"] + ["w%03d%s" % (i, chr(0x1F600 + i % 16)) for i in range(300)]
    else:
        base = ["Éclair", "éclair", "ECLAIR", "straße", "STRASSE", "ΑΘΗΝΑ", "αθηνα", "Αθήνα", "σοφός", "ΣΟΦΟΣ", "σοφόσ", "µm", "μm", "ÿ", "Ÿ", "K", "k", "K", "ß", "ǆ", "ǅ", "é", "É",
                "año", "AÑO", "ano", "line\nbreak", " x", "naïve", "NAÏVE", "ωμέγα", "ΩΜΈΓΑ"]
        greek = [chr(c) for c in range(0x3B1, 0x3CA)] + [chr(c) for c in range(0x391, 0x3A2)] + list("éèàüöäßñçÉÈÀÜÖÄÑÇab")
        words = set(base)
        while len(words) < 700:
            words.add("".join(greek[int(k)] for k in rng.integers(0, len(greek), size=int(rng.integers(1, 12)))))
        words = sorted(words)
    return widecorpus.crafted(docs, {w: rng.choice(docs, size=int(rng.integers(1, 5)), replace=False) for w in words})


def rx(pattern, path="body", **kw):
    return dict({"path": path, "terms": [pattern], "is_regex": True}, **kw)


def variants(patterns):
    """every pattern with starts_with off and on, ignore_case true, false and absent in turn"""
    out = []
    for i, p in enumerate(patterns):
        for sw in (False, True):
            kw = {"starts_with": True} if sw else {}
            ic = (None, True, False)[(i + sw) % 3]
            if ic is not None:
                kw["ignore_case"] = ic
            out.append({"search_req": {"search": rx(p, **kw)}, "top": 10})
    # ... and all six combinations for three of them
    for p in patterns[:3]:
        for sw in (False, True):
            for ic in (None, True, False):
                kw = dict({"starts_with": True} if sw else {}, **({} if ic is None else {"ignore_case": ic}))
                out.append({"search_req": {"search": rx(p, **kw)}, "top": 10, "skip": 2})
    return out


PATTERNS = {
    # every operator; one pattern that matches nothing (`#` is in no term), one that matches everything, some whose start state accepts (`x*`, `a|`, `(ab)?`)
    "ascii": ["ab.*", "(foo|ba[rz])+x?", "[a-c]{2,3}d.*e", "a|", "x*", "(ab)?", "q{2,}?z", "[^a-m]+", r"\d+[a-z]?", "zz#", "(?:ab|cd){1,2}e??", "m+z", "m{30,}z", ".", r"\w{39,}", "AB.E",
              "[A-Z][a-z]*", ".*", "b{2}", "(a|b)(c|d)+?", r"f\S\So?", "[0-9]{2}", "a.c"],
    "astral": ["\U0001F600", ".*\U0001F600.*", "\U00010400.?", "[\U00010400-\U0001044f]+", "w\\d+.", "w0[0-4]\\d[\U0001F600-\U0001F603]", "q+.", ".", "..", "k", "[^a-z]+", "z\U0010FFFF|東.",
               r"\W+", r"\S{1,3}", "x.y"],
    "latin": ["é.*", "É.*", ".*σ", ".*ς", "[α-ω]+", "[Α-Ω]+", "αθ.να", "µm|km", "μ.", r"\w+", r"\W+", "k", "[k]", "ÿ", "straße", "line.break", r"line\sbreak", "ǆ", "[éèà]{2,}", "(σ|ς)+.?",
              "añ?o", ".{11}", "[^α-ω]"],
}
DECLINED = ["^ab", "ab$", r"\bab", "(a)\\1b?", "ab(?=c)", "[[:digit:]]+"]


def as_json(res):
    return {"num_hits": int(res.num_hits), "ids": res.ids.tolist(), "scores": res.scores.view(np.uint32).tolist()}


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import veloci_amd
import test_gpu_regex_device as T
name, path = sys.argv[2], sys.argv[3]
reqs = json.load(open(path))
data, terms = T.build_corpus(name)
idx = veloci_amd.Index(data, device=0)
idx.profile_enable()
out = [T.as_json(r) for r in veloci_amd.search_batch(reqs, idx)]
assert "k_dict_regex" not in idx.profile_json()["kernels"] or idx.profile_json(False)["kernels"]["k_dict_regex"]["launches"] == 0
print("HOST_ROUTE " + json.dumps(out))
"""


def host_route(name, reqs, tmp_path):
    """the same requests in one child process that keeps every regex leaf on the host route"""
    path = tmp_path / ("reqs_%s.json" % name)
    path.write_text(json.dumps(reqs))
    env = dict(os.environ, VQ_NO_REGEX_DEVICE="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, "-c", CHILD, HERE, name, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "HOST_ROUTE " in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.split("HOST_ROUTE ", 1)[1])


class Corpus:
    def __init__(self, name, oracle=False):
        import veloci_amd
        self.name = name
        self.data, self.terms = build_corpus(name)
        self.idx = veloci_amd.Index(self.data, device=0)
        self.ora = None
        if oracle:
            from oracle import binding as O
            self.ora = O.OracleIndex(self.data.num_anchors)
            self.data.load_into(self.ora)
        self.cache = {}

    def want(self, req):
        js = json.dumps(req)
        if js not in self.cache:
            self.cache[js] = self.ora.search_json(js)
        return self.cache[js]

    def regex_launches(self):
        k = self.idx.profile_json()["kernels"].get("k_dict_regex")
        return (k["launches"], k["queries"]) if k else (0, 0)


@pytest.fixture(scope="module")
def ascii_corpus():
    c = Corpus("ascii", oracle=True)
    assert len(c.terms) == 2 * 2048 + 37 and max(len(t) for t in c.terms) == 5000
    return c


def leaves_of(req):
    return [req["search_req"]["search"]]


def check_against_host(c, reqs, tmp_path, declined=()):
    import veloci_amd
    for r in reqs:
        route = c.idx.regex_route(leaves_of(r)[0])
        assert route["device"] != (r in declined), (r, route)
    got = [as_json(g) for g in veloci_amd.search_batch(reqs, c.idx)]
    host = host_route(c.name, reqs, tmp_path)
    for r, g, h in zip(reqs, got, host):
        assert g == h, (json.dumps(r), g, h)
    return got


def test_every_operator_equals_the_oracle_and_the_host_route(ascii_corpus, tmp_path):
    import veloci_amd
    from parity import assert_same
    c = ascii_corpus
    reqs = variants(PATTERNS["ascii"])
    got = check_against_host(c, reqs, tmp_path)
    for r in reqs:
        assert_same(r, veloci_amd.search(r, c.idx), c.want(r))
    hits = {r["search_req"]["search"]["terms"][0]: g["num_hits"] for r, g in zip(reqs, got) if "starts_with" not in r["search_req"]["search"]}
    assert hits["zz#"] == 0 and hits[".*"] == hits["x*"] == hits["a|"] == hits["(ab)?"] > 4000 and hits["m{30,}z"] >= 2 and hits["ab.*"] > 0, hits


@pytest.mark.parametrize("name", ["astral", "latin"])
def test_non_ascii_dictionaries_equal_the_host_route(name, tmp_path):
    c = Corpus(name)
    d = c.idx.regex_route(rx("."))
    assert d["device"] and d["classes"] >= 1
    got = check_against_host(c, variants(PATTERNS[name]), tmp_path)
    assert sum(1 for g in got if g["num_hits"] > 0) > len(got) // 2
    c.idx.close()


def test_profile_one_launch_per_device_leaf_none_for_a_declined_one_and_the_lds_budget(ascii_corpus, tmp_path):
    import veloci_amd
    from parity import assert_same
    c = ascii_corpus
    c.idx.profile_enable()
    try:
        r = {"search_req": {"search": rx("ab.*")}, "top": 10}
        assert_same(r, veloci_amd.search(r, c.idx), c.want(r))
        assert c.regex_launches() == (1, 1)  # (the parent commit has no such kernel)
        declined = [{"search_req": {"search": rx(p)}, "top": 10} for p in DECLINED]
        check_against_host(c, declined, tmp_path, declined=declined)
        assert c.regex_launches() == (0, 0)
        # the table budget: `.*a.{8}` is 512 states, and every further single-letter alternative behind it adds 256 states and a class; the first
        # pattern of the series that leaves the device route does so for the LDS budget (68 KiB), one class behind the last one that stays
        letters = "bcdefgmoqrxzABFZ0159"
        under = over = None
        for k in range(1, len(letters) + 1):
            p = rx(".*a.{8}(?:%s)" % "|".join(letters[:k]))
            route = c.idx.regex_route(p)
            if not route["device"]:
                over = (p, route)
                break
            under = (p, route)
        assert under and over, (under, over)
        print("LDS budget: device", under[1], "host", over[1]["reason"])
        assert "LDS table budget" in over[1]["reason"] and under[1]["states"] <= 4096
        assert 60 * 1024 < 2 * under[1]["states"] * under[1]["classes"] + 256 <= 68 * 1024
        pair = [{"search_req": {"search": under[0]}, "top": 10}, {"search_req": {"search": over[0]}, "top": 10}]
        c.idx.profile_json()
        got = [as_json(g) for g in veloci_amd.search_batch(pair, c.idx)]
        assert c.regex_launches() == (1, 1)  # the one under the budget ran on the device, the one over it did not
        assert got == host_route(c.name, pair, tmp_path)
    finally:
        c.idx.profile_enable(False)


def test_one_batch_of_many_regex_leaves(ascii_corpus):
    import veloci_amd
    from parity import assert_same
    c = ascii_corpus
    pats = ["ab.*", "(foo|ba[rz])+x?", "[a-c]{2,3}d.*e", "q{2,}?z", "[^a-m]+", r"\d+[a-z]?", "(?:ab|cd){1,2}e??", "m+z", "m{30,}z", r"\w{39,}", "AB.E", "b{2}", "(a|b)(c|d)+?",
            r"f\S\So?", "[0-9]{2}", "a.c", "zz#", "fo+.*"]
    L = [rx(p) for p in pats]  # 18 distinct leaves on `body`: more than the 16 probes a k_dict_scan block groups
    leaf = lambda p: {"search": p}
    reqs = [{"search_req": leaf(p), "top": 10} for p in L]
    reqs += [{"search_req": leaf(rx(p, path="title")), "top": 10} for p in ("red0[1-3]", "red.*5", "r.d1\\d")]  # a second dictionary
    reqs += [{"search_req": leaf(L[0]), "top": 3 + k} for k in range(5)]  # the same leaf five times
    reqs += [{"search_req": leaf({"path": "body", "terms": ["abcde"], "levenshtein_distance": 1}), "top": 10},
             {"search_req": leaf({"path": "body", "terms": ["fo"], "starts_with": True}), "top": 10},
             {"search_req": {"and": {"queries": [leaf({"path": "body", "terms": ["ab"], "starts_with": True}), leaf(L[4])]}}, "top": 10},
             {"search_req": {"or": {"queries": [leaf({"path": "body", "terms": ["bazfo"], "levenshtein_distance": 1}), leaf(L[1])]}}, "top": 10}]
    reqs += [{"search_req": {"and": {"queries": [leaf(L[4]), leaf(L[5])]}}, "top": 10},
             {"search_req": {"or": {"queries": [leaf(L[0]), leaf(L[7]), leaf(L[16])]}}, "top": 10},
             {"search_req": {"and": {"queries": [leaf(L[4]), {"or": {"queries": [leaf(L[2]), leaf(L[12])]}}]}}, "top": 10},
             {"search_req": leaf(L[4]), "filter": leaf(L[5]), "top": 10},
             {"search_req": leaf(L[0]), "boost_term": [dict(L[17], boost=3.0)], "top": 10},
             {"search_req": leaf(L[17]), "phrase_boosts": [{"search1": L[17], "search2": L[1]}], "top": 10},
             {"search_req": leaf(dict(L[4], top=5)), "top": 10},
             {"search_req": leaf(L[1]), "explain": True, "top": 5},
             {"search_req": leaf(L[0]), "why_found": True, "top": 5},
             {"search_req": leaf(L[12]), "top": 10, "skip": 3}]
    assert len(reqs) == 40
    singles = [veloci_amd.search(r, c.idx) for r in reqs]
    c.idx.profile_enable()
    try:
        batch = veloci_amd.search_batch(reqs, c.idx)
        launches, probes = c.regex_launches()
    finally:
        c.idx.profile_enable(False)
    assert probes == 18 + 3 and launches == 1, (launches, probes)  # one probe per distinct leaf; one timed bracket around the launches of the batch
    for r, g, s in zip(reqs, batch, singles):
        assert as_json(g) == as_json(s), json.dumps(r)
        assert_same(r, g, c.want(r))
        if r.get("why_found"):
            assert {k: sorted(v) for k, v in g.why_found_terms.items()} == {k: sorted(v) for k, v in s.why_found_terms.items()} and g.why_found_terms
        if r.get("explain"):
            assert g.explain == s.explain and g.explain


def test_leaf_of_more_than_4096_terms_takes_the_dense_union_and_shards_agree():
    import veloci_amd
    import widecorpus
    from oracle import binding as O
    from parity import assert_same
    from veloci_amd.dist import search_shards_local
    data, terms = widecorpus.build(num_terms=20_000, num_docs=200_000, planted=False)
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    assert sum(1 for t in terms if t[-1:] in b"abcdefg") > 4096
    reqs = [{"search_req": {"search": rx(".*[a-g]")}, "top": 10}, {"search_req": {"search": rx("[ab].*q[a-m]+")}, "top": 10, "skip": 4}]
    want = [ora.search_json(json.dumps(r)) for r in reqs]
    idx.profile_enable()
    got = veloci_amd.search_batch(reqs, idx)
    prof = idx.profile_json()["kernels"]
    assert prof["k_dict_regex"]["launches"] == 1 and prof["k_dict_regex"]["queries"] == 2 and prof["k_union_dense_scatter"]["launches"] >= 1, prof
    for r, g, w in zip(reqs, got, want):
        assert_same(r, g, w)
    # two doc-range shards of the same corpus
    N = data.num_anchors
    parts = [veloci_amd.Index(data, device=0, doc_lo=0, doc_hi=N // 3), veloci_amd.Index(data, device=0, doc_lo=N // 3, doc_hi=N)]
    for r, g, w in zip(reqs, search_shards_local(parts, reqs), want):
        assert_same(r, g, w)
    for p in parts + [idx]:
        p.close()
