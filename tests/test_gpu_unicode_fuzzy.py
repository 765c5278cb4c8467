"""Fuzzy / prefix leaves and suggest (K9, k_dict_scan) on a dictionary with code points above U+FFFF and on query terms longer than 64 code
points: product == oracle (search_field.rs:85-95 builds its automaton over the chars of a term of any length).  A hand-built corpus with two
fields: `wide` (emoji with modifiers and ZWJ sequences, Deseret and Adlam case pairs, CJK Extension B, mathematical alphanumerics, a term with
U+F389, ASCII and accented words, terms of 31-300 code points with near-duplicates at 1-4 edits) and `bmp` (below U+10000 only)."""
import json
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ASTRAL = ["🎉", "🎉🎉", "party🎉", "🎊", "👍", "👍🏽", "👍🏿", "👨‍👩‍👧", "👩🏽‍💻", "❤️", "😀x", "x😀", "😀😁", "😁😀",
          "𐐔𐐯𐑅𐐨𐑉𐐯𐐻", "𐐼𐐯𐑅𐐨𐑉𐐯𐐻", "𐐔𐐆𐐝", "𐐼𐐮𐑅",            # Deseret (U+10400 .. : capital -> U+10428 ..)
          "𞤀𞤣𞤤𞤢𞤥", "𞤢𞤣𞤤𞤢𞤥", "𞤐𞤫𞤲", "𞤲𞤫𞤲",                # Adlam (U+1E900 .. : capital -> U+1E922 ..)
          "𠮷", "𠮷野家", "𠮷野", "𡈽", "𡈽𠮷",                    # CJK Extension B
          "𝐇𝐞𝐥𝐥𝐨", "𝐇𝐞𝐥𝐥𝐨𝐬", "𝓗𝓮𝓵𝓵𝓸", "𝕳𝖊𝖑𝖑𝖔",          # mathematical alphanumerics
          "\uf389", "\uf389abc", "x\uf389", "🎉abc"]             # U+F389: what U+1F389 (🎉) would alias to in 16 bits
PLAIN = ["hello", "Hello", "héllo", "help", "straße", "Straße", "über", "Über", "party", "parties", "theme", "there", "привет", "東京", "a", "ab"]
ALPHA_ASTRAL = "ab𝐚𝐛😀😁𐐔𐐼𞤀𞤢𠮷é"
ALPHA_BMP = "abcdeéüxyz東"


def _long(rng, n, alpha):
    return "".join(rng.choice(alpha) for _ in range(n))


def _edit(rng, w, k, alpha):
    """k random edits (insert, delete, substitute, adjacent transposition)"""
    s = list(w)
    for _ in range(k):
        op = rng.randint(0, 3)
        if op == 0 and len(s) > 1:
            del s[rng.randrange(len(s))]
        elif op == 1:
            s.insert(rng.randint(0, len(s)), rng.choice(alpha))
        elif op == 2 and s:
            s[rng.randrange(len(s))] = rng.choice(alpha)
        elif op == 3 and len(s) > 1:
            i = rng.randrange(len(s) - 1)
            s[i], s[i + 1] = s[i + 1], s[i]
    return "".join(s)


def _words(seed):
    rng = random.Random(seed)
    wide, bmp = set(ASTRAL) | set(PLAIN), set(PLAIN) | {"\uf389", "\uf389abc", "x\uf389"}
    long_wide, long_bmp = [], []
    for n in (31, 32, 33, 63, 64, 65, 100, 150, 200, 300):
        for _ in range(2):
            long_wide.append(_long(rng, n, ALPHA_ASTRAL))
            long_bmp.append(_long(rng, n, ALPHA_BMP))
    for base, out, alpha in ((long_wide, wide, ALPHA_ASTRAL), (long_bmp, bmp, ALPHA_BMP)):
        for w in base:
            out.add(w)
            out.add(w.upper())
            for k in (1, 1, 2, 3, 4):
                out.add(_edit(rng, w, k, alpha))
            i = rng.randrange(len(w) - 1)  # one adjacent transposition
            out.add(w[:i] + w[i + 1] + w[i] + w[i + 2:])
    for w in ASTRAL:
        for k in (1, 2):
            wide.add(_edit(rng, w, k, ALPHA_ASTRAL))
        if len(w) > 1:
            wide.add(w[1] + w[0] + w[2:])  # transposition of two astral characters
    for w in PLAIN:
        bmp.add(_edit(rng, w, 1, ALPHA_BMP))
    wide.discard("")
    bmp.discard("")
    return sorted(wide, key=lambda t: t.encode()), sorted(bmp, key=lambda t: t.encode()), long_wide, long_bmp


def build(num_docs=5000, seed=11):
    from veloci_amd.index import IndexData
    wide, bmp, long_wide, long_bmp = _words(seed)
    data = IndexData(num_docs)
    nrng = np.random.default_rng(seed)
    for field, terms in (("wide", wide), ("bmp", bmp)):
        lens = nrng.integers(1, 60, size=len(terms))
        offsets = np.zeros(len(terms) + 1, np.uint64)
        offsets[1:] = np.cumsum(lens)
        anchors = np.zeros(int(offsets[-1]), np.uint32)
        scores = np.zeros(int(offsets[-1]), np.uint32)
        for t in range(len(terms)):
            o, n = int(offsets[t]), int(lens[t])
            anchors[o:o + n] = np.sort(nrng.choice(num_docs, size=n, replace=False))
            scores[o:o + n] = nrng.integers(1, 200, size=n)
        path = field + ".textindex"
        data.add_fst(path, [t.encode() for t in terms])
        data.add_token_to_anchor_score(path + ".to_anchor_id_score", offsets, anchors, scores, None)
        data.add_key_value_store(path + ".text_id_to_anchor", offsets, anchors)
        # phrase pairs of neighbouring terms, on every doc both lists hold
        keys = [(t, t + 1) for t in range(0, len(terms) - 1, 3)]
        pairs = [np.intersect1d(anchors[int(offsets[a]):int(offsets[a + 1])], anchors[int(offsets[b]):int(offsets[b + 1])]) for a, b in keys]
        po = np.zeros(len(keys) + 1, np.uint64)
        po[1:] = np.cumsum([len(p) for p in pairs])
        data.add_phrase_pair_to_anchor(path + ".phrase_pair_to_anchor", [k[0] for k in keys], [k[1] for k in keys], po,
                                       np.concatenate(pairs).astype(np.uint32))
    return data, {"wide": wide, "bmp": bmp, "long_wide": long_wide, "long_bmp": long_bmp}


@pytest.fixture(scope="module")
def uni():
    import veloci_amd
    from oracle import binding as O
    data, info = build()
    idx = veloci_amd.Index(data, device=0)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    return data, info, idx, ora


def _part(path, term, **kw):
    p = {"path": path, "terms": [term]}
    p.update(kw)
    return p


def _probes(info):
    """query terms: astral, U+1F389 / U+F389, long (<= 64 and > 64 code points, some edited), plain"""
    rng = random.Random(5)
    wide = ["🎉", "🎉abc", "party🎉", "👍🏽", "👍🏾", "👨‍👩‍👦", "𐐔𐐯𐑅𐐨𐑉𐐯𐐻", "𐐼𐐯𐑅𐐨𐑉𐐯𐑂", "𐐔𐐆", "𞤀𞤣𞤤𞤢", "𞤢𞤣𞤤𞤢𞤥", "𠮷野", "𠮷", "𝐇𝐞𝐥𝐥𝐨",
            "𝐇𝐥𝐞𝐥𝐨", "\uf389", "hello", "héllo", "Straße", "😁😀"]
    for w in info["long_wide"][::3]:
        wide += [w, _edit(rng, w, 2, ALPHA_ASTRAL)]
    bmp = ["🎉", "🎉abc", "\uf389abc", "𠮷", "hello", "Über", "a😀b"]
    for w in info["long_bmp"][::3]:
        bmp += [w, _edit(rng, w, 2, ALPHA_BMP), w[:70] + "😀"]
    return [("wide", t) for t in wide] + [("bmp", t) for t in bmp]


def check(uni, req):
    import veloci_amd
    from parity import assert_same
    _, _, idx, ora = uni
    got = veloci_amd.search(req, idx)
    assert_same(req, got, ora.search_json(json.dumps(req)))
    return got


def check_batch(uni, reqs, index=None):
    import veloci_amd
    from parity import assert_same
    _, _, idx, ora = uni
    got = veloci_amd.search_batch(reqs, index or idx)
    hits = 0
    for r, g in zip(reqs, got):
        assert_same(r, g, ora.search_json(json.dumps(r)))
        hits += g.num_hits
    return hits


def test_fuzzy_distances_and_case(uni):
    _, info, _, _ = uni
    reqs = []
    for path, t in _probes(info):
        for lev in range(6):
            for ic in (None, True, False):
                p = _part(path, t, levenshtein_distance=lev)
                if ic is not None:
                    p["ignore_case"] = ic
                reqs.append({"search_req": {"search": p}, "top": 20})
    assert check_batch(uni, reqs) > 1000


def test_starts_with(uni):
    _, info, _, _ = uni
    reqs = []
    for path, t in _probes(info) + [("wide", "𐐔"), ("wide", "𞤢"), ("wide", "😀"), ("wide", "𝐇"), ("bmp", "😀")]:
        for lev in (None, 1, 2):
            for ic in (None, True, False):
                p = _part(path, t, starts_with=True)
                if lev is not None:
                    p["levenshtein_distance"] = lev
                if ic is not None:
                    p["ignore_case"] = ic
                reqs.append({"search_req": {"search": p}, "top": 20})
    assert check_batch(uni, reqs) > 1000


def test_leaf_top_trees_filters_boosts_and_phrases(uni):
    _, info, _, _ = uni
    lw, lb = info["long_wide"], info["long_bmp"]
    f = lambda path, t, **kw: {"search": _part(path, t, **kw)}
    for path, t, kw in (("wide", "🎉", {"starts_with": True}), ("wide", lw[12], {"levenshtein_distance": 3}), ("bmp", lb[14], {"levenshtein_distance": 4}),
                        ("wide", "𐐼𐐯𐑅𐐨𐑉𐐯𐐻", {"levenshtein_distance": 2})):
        for top in (1, 3, 10):
            check(uni, {"search_req": {"search": _part(path, t, top=top, **kw)}, "top": 10})
    reqs = [
        {"search_req": {"or": {"queries": [f("wide", "🎉", levenshtein_distance=1), f("wide", lw[13], levenshtein_distance=2), f("bmp", lb[12], levenshtein_distance=3),
                                           f("bmp", "hello")]}}, "top": 30},
        {"search_req": {"and": {"queries": [f("wide", "𝐇𝐞𝐥𝐥𝐨", levenshtein_distance=2), f("wide", "😀", starts_with=True, levenshtein_distance=1)]}}, "top": 30},
        {"search_req": f("wide", lw[15], levenshtein_distance=2), "filter": f("wide", "𐐔", starts_with=True, levenshtein_distance=1), "top": 30},
        {"search_req": f("bmp", "he", starts_with=True), "filter": f("bmp", lb[16], levenshtein_distance=2, ignore_case=True), "top": 30},
        {"search_req": f("wide", "party", starts_with=True), "boost_term": [_part("wide", "🎉abc", levenshtein_distance=1, boost=3.0),
                                                                              _part("wide", lw[18], levenshtein_distance=2, boost=2.0)], "top": 30},
        {"search_req": f("wide", "𠮷", starts_with=True),
         "phrase_boosts": [{"search1": _part("wide", "𠮷野", levenshtein_distance=1), "search2": _part("wide", "𠮷野家", levenshtein_distance=1)},
                           {"search1": _part("wide", lw[12], levenshtein_distance=2), "search2": _part("wide", lw[13], levenshtein_distance=2)}], "top": 30},
    ]
    for r in reqs:
        check(uni, r)


def test_matches_are_astral_long_and_never_the_f389_alias(uni):
    """the hits come from astral terms and from terms of more than 64 code points; U+1F389 never matches U+F389 (a 16-bit cast would)"""
    import veloci_amd
    _, info, idx, ora = uni

    def terms_of(req):
        got = veloci_amd.suggest(req, idx)
        want = ora.suggest_json(json.dumps(req))
        assert [(t, np.float32(s).view(np.uint32)) for t, s, _ in got] == [(t, np.float32(s).view(np.uint32)) for t, s, _ in want], req
        return [t for t, _, _ in got]

    party = terms_of(_part("wide", "🎉", starts_with=True, top=100))
    assert "🎉" in party and "🎉🎉" in party and "🎉abc" in party
    assert not any("\uf389" in t for t in party), party
    for path in ("wide", "bmp"):
        for req in (_part(path, "🎉", levenshtein_distance=0, starts_with=True, top=100), _part(path, "🎉abc", levenshtein_distance=0, starts_with=True, top=100),
                    _part(path, "x🎉", levenshtein_distance=0, starts_with=True, top=100)):
            assert not any("\uf389" in t for t in terms_of(req)), req
    assert terms_of(_part("bmp", "\uf389abc", levenshtein_distance=0, starts_with=True, top=100)) == ["\uf389abc"]
    # (suggest answers lower-cased texts)
    deseret = terms_of(_part("wide", "𐐔𐐯𐑅𐐨𐑉𐐯𐐻", levenshtein_distance=1, top=100))
    assert "𐐼𐐯𐑅𐐨𐑉𐐯𐐻" in deseret and len(deseret) >= 2
    adlam = terms_of(_part("wide", "𞤀𞤣𞤤𞤢𞤥", levenshtein_distance=1, ignore_case=False, top=100))
    assert "𞤢𞤣𞤤𞤢𞤥" in adlam
    for w in info["long_wide"][12:] + info["long_bmp"][12:]:
        assert len(w) > 64
        path = "wide" if w in info["long_wide"] else "bmp"
        got = terms_of(_part(path, w, levenshtein_distance=4, top=100))
        assert w.lower() in got and len(got) >= 2 and all(len(t) > 60 for t in got), (w, got)
    got = terms_of(_part("wide", info["long_wide"][14][:80], starts_with=True, levenshtein_distance=2, top=100))
    assert info["long_wide"][14].lower() in got


def test_suggest(uni):
    import veloci_amd
    _, info, idx, ora = uni
    reqs = [_part(path, t, starts_with=True, top=10) for path, t in _probes(info)[:20]]
    reqs += [_part(path, t, levenshtein_distance=2, top=10) for path, t in _probes(info)]
    reqs.append({"suggest": [_part("wide", "𐐔", starts_with=True), _part("bmp", "he", starts_with=True), _part("wide", info["long_wide"][16], levenshtein_distance=3)],
                 "top": 15})
    n = 0
    for r in reqs:
        got = veloci_amd.suggest(r, idx)
        want = ora.suggest_json(json.dumps(r))
        assert [(t, np.float32(s).view(np.uint32)) for t, s, _ in got] == [(t, np.float32(s).view(np.uint32)) for t, s, _ in want], r
        n += len(got)
    assert n > 100


def test_batches_mix_both_image_widths(uni):
    """one batch holds probes of the 32-bit `wide` image, the 16-bit `bmp` image, inline and pooled, short and long"""
    _, info, _, _ = uni
    reqs = []
    for path, t in _probes(info):
        reqs.append({"search_req": {"search": _part(path, t, levenshtein_distance=2)}, "top": 10})
        reqs.append({"search_req": {"search": _part(path, t[:3], starts_with=True)}, "top": 10})
    random.Random(2).shuffle(reqs)
    assert check_batch(uni, reqs) > 500


def test_two_shards_merge_equals_unsharded(uni):
    import veloci_amd
    from parity import assert_same
    from veloci_amd.dist import exchange_local
    data, info, _, ora = uni
    N = data.num_anchors
    cut = N // 3
    s0 = veloci_amd.Index(data, device=0, doc_lo=0, doc_hi=cut)
    s1 = veloci_amd.Index(data, device=0, doc_lo=cut, doc_hi=N)
    reqs = []
    for path, t in _probes(info):
        reqs.append({"search_req": {"search": _part(path, t, levenshtein_distance=3, ignore_case=True)}, "top": 15})
        reqs.append({"search_req": {"search": _part(path, t[:2], starts_with=True, levenshtein_distance=1)}, "top": 15})
    p0 = veloci_amd.PartialBatch(s0, reqs)
    p1 = veloci_amd.PartialBatch(s1, reqs)
    g = exchange_local([p0, p1])
    res = p0.merge(g.data_ptr(), 2)
    p1.merge(None, 1)
    hits = 0
    for r, got in zip(reqs, res):
        assert_same(r, got, ora.search_json(json.dumps(r)))
        hits += got.num_hits
    assert hits > 500


def test_seeded_random_batch(uni):
    """>= 500 probes: random astral and long strings, and dictionary terms, with random edits, distances, prefix and case flags"""
    _, info, _, _ = uni
    rng = random.Random(20261016)
    reqs = []
    for i in range(600):
        path = "wide" if i % 3 else "bmp"
        terms = info[path]
        r = rng.random()
        if r < 0.35:
            t = _edit(rng, rng.choice(terms), rng.randint(0, 4), ALPHA_ASTRAL if path == "wide" else ALPHA_BMP)
        elif r < 0.7:
            t = _edit(rng, _long(rng, rng.randint(60, 260), ALPHA_ASTRAL), rng.randint(0, 3), ALPHA_ASTRAL)
            if rng.random() < 0.5:  # one of the long terms, a few edits away
                t = _edit(rng, rng.choice(info["long_wide" if path == "wide" else "long_bmp"]), rng.randint(0, 4), ALPHA_ASTRAL)
        else:
            t = _long(rng, rng.randint(1, 8), ALPHA_ASTRAL)
        p = _part(path, t or "a", levenshtein_distance=rng.randint(0, 5))
        if rng.random() < 0.4:
            p["starts_with"] = True
            if rng.random() < 0.5:
                p["terms"] = [p["terms"][0][:max(1, len(p["terms"][0]) // 2)]]
        if rng.random() < 0.6:
            p["ignore_case"] = rng.random() < 0.5
        reqs.append({"search_req": {"search": p}, "top": 10})
    assert check_batch(uni, reqs) > 1000
