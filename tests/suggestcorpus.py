"""Two small dictionaries and suggest requests for the batched suggest (vq_suggest_batch): shared by tests/test_gpu_suggest_batch.py and the
host-stub driver tests/native/suggest_batch_driver.py.  Built straight through IndexData.add_fst with one posting per term.

field `a` (16-bit image) and field `b` (one term above U+FFFF: the 32-bit image, so its probes take the wide scan), about 3000 terms each, of
1-20 letters so that scores differ by length; many terms in both fields; case variants whose texts merge; planted prefixes:
  qa / qb / qc   exactly 201 / 202 / 203 matches: with top 1 no cut of the top-n loop, a cut at the last push, a cut and one more push
  w              about 2500 matches of 2-20 letters: several cuts, the worst score rises
  zz             400 matches of one length: every score ties, the survivors are decided by id order alone
`a` also has a token_values boost column."""
import json
import struct

import numpy as np

PLANTED = (("qa", 201), ("qb", 202), ("qc", 203))
N_W = 2500
N_ZZ = 400
LETTERS = "abcdeilnorst"  # (none of q, w, z: the planted prefixes keep their counts)


def _words(rng, n, lo, hi, head=""):
    out = set()
    while len(out) < n:
        out.add(head + "".join(LETTERS[int(k)] for k in rng.integers(0, len(LETTERS), size=int(rng.integers(lo, hi + 1)))))
    return out


def field_terms(seed, astral):
    rng = np.random.default_rng(seed)
    words = _words(rng, 250, 1, 20)
    words |= {"Foo", "foo", "FOO", "fOo", "Bar", "bar", "BAR", "foobar", "Foobar", "FOOBAR", "a", "A", "ab", "AB", "Ab"}
    for head, n in PLANTED:
        words |= _words(rng, n, 0, 14, head)
    words |= _words(rng, N_W, 1, 19, "w")
    words |= _words(rng, N_ZZ, 6, 6, "zz")
    if astral:
        words.add("x\U0001F600y")
    return sorted(w.encode() for w in words)


def build():
    """-> (IndexData, {"a": [terms as bytes], "b": [...]})"""
    from veloci_amd.index import IndexData
    shared = field_terms(7, False)
    rng = np.random.default_rng(8)
    keep = rng.random(len(shared)) < 0.9  # `b`: most of a's terms, some of its own, one above U+FFFF
    terms = {"a": shared, "b": sorted(set(t for t, k in zip(shared, keep) if k) | set(field_terms(9, True)[::10]))}
    docs = 64
    data = IndexData(docs)
    for f, ts in terms.items():
        offsets = np.arange(len(ts) + 1, dtype=np.uint64)
        anchors = (np.arange(len(ts)) % docs).astype(np.uint32)
        data.add_fst(f + ".textindex", ts)
        data.add_token_to_anchor_score(f + ".textindex.to_anchor_id_score", offsets, anchors, np.full(len(ts), 10, np.uint32), None)
        data.add_key_value_store(f + ".textindex.text_id_to_anchor", offsets, anchors)
    vals = (np.arange(len(terms["a"])) % 7 + 1).astype(np.float32)
    present = (np.arange(len(terms["a"])) % 3 != 0).astype(np.uint8)
    data.add_boost("a.textindex.token_values.boost_valid_to_value", vals, present)
    return data, terms


def count_prefix(terms, prefix):
    return sum(1 for t in terms if t.decode().lower().startswith(prefix))


def part(field, term, **kw):
    return dict({"path": field, "terms": [term]}, **{k: v for k, v in kw.items() if v is not None})


def fixed_requests():
    """every ingredient once, by hand"""
    P = part
    reqs = []
    for top in (1, 10, 200, 1848, 1849):  # 1849: just beyond the kernel's buffer, the full route
        for term in ("w", "qa", "qb", "qc", "zz", "f", "wa"):
            reqs.append(P("a", term, starts_with=True, top=top))
    for head, _ in PLANTED:  # top 1: no cut / a cut at the last push / a cut and one more push; and with skip
        reqs.append(P("b", head, starts_with=True, top=1, skip=0))
        reqs.append(P("a", head, starts_with=True, top=1, skip=1))
    reqs += [
        P("a", "w", starts_with=True, top=10, skip=5000),          # skip beyond the result
        P("a", "zza", starts_with=True, top=0),                    # top 0: nothing to keep (full route).  Fewer than 200 matches: with top + skip == 0
                                                                   # the reference's cut truncates to nothing and then reads the last element (it panics);
                                                                   # 200 and more: test_gpu_suggest_batch.py holds the batch against the single call alone
        P("a", "w", starts_with=True, top=0, skip=7),              # top + skip >= 1 with top 0
        P("a", "wa", starts_with=True),                            # no top: nothing to cut
        P("a", "w", starts_with=True, top=10, boost=2.5),
        P("a", "w", starts_with=True, top=10, boost=-1.0),         # reverses the final order
        P("a", "w", starts_with=True, top=10, boost=0.0),          # every score ties in the final sort
        P("a", "wa", starts_with=True, top=10, levenshtein_distance=1),
        P("b", "was", starts_with=True, top=10, levenshtein_distance=2),
        P("a", "foo", levenshtein_distance=1, top=10),             # fuzzy, no prefix
        P("a", "foobar", levenshtein_distance=2, top=3, skip=1),
        P("a", "FOO", starts_with=True, top=10, ignore_case=True),
        P("a", "FOO", starts_with=True, top=10, ignore_case=False),
        P("a", "Fo", starts_with=True, top=10),
        P("a", "fo+.*", is_regex=True, top=10),
        P("b", "ba[rz]", is_regex=True),
        P("a", "foo"),                                             # exact
        P("a", "foo", top=1, ignore_case=False),
        P("a", "w", starts_with=True, top=10, token_value={"path": "a", "boost_fun": "Multiply", "param": 0}),
        P("a", "zz", starts_with=True, top=5, token_value={"path": "a", "boost_fun": "Log10", "param": 1}),
        P("b", "x", starts_with=True, top=10),                     # reaches the term above U+FFFF
    ]
    w10 = P("a", "w", starts_with=True, top=10)
    multi = [
        {"suggest": [w10], "top": 10},
        {"suggest": [w10, P("b", "w", starts_with=True, top=10)], "top": 10, "skip": 0},
        {"suggest": [w10, w10], "top": 5},                                               # parts repeat
        {"suggest": [P("a", "f", starts_with=True, top=10, skip=2), P("b", "f", starts_with=True, top=10, skip=2), P("a", "foo", levenshtein_distance=1, top=10)], "top": 10, "skip": 3},
        {"suggest": [P("a", "zz", starts_with=True, top=10), P("b", "zz", starts_with=True, top=200), P("a", "qa", starts_with=True)], "top": 20},
        {"suggest": [P("a", "Fo", starts_with=True, top=10), P("b", "fO", starts_with=True, top=10)]},   # texts merge across case and fields
        {"suggest": [w10], "top": 10}, {"suggest": [w10], "top": 10},                                      # the same request three times
        {"suggest": [P("a", "w", starts_with=True, top=11)], "top": 10},                                   # equal but for the part's top
    ]
    return reqs + multi


FAILING = ['{"path": "a", "terms": ["w"', {"path": "nope", "terms": ["w"], "starts_with": True, "top": 10}, {"path": "a", "terms": [], "top": 10},
           {"path": "a", "terms": ["(w"], "is_regex": True, "top": 10}]


def random_requests(n, seed, terms):
    """n seeded requests over the same ingredients, in the reference generator's shape (starts_with, levenshtein_distance 0-2, top / skip)"""
    rng = np.random.default_rng(seed)
    pool = ["w", "wa", "q", "qa", "qb", "qc", "z", "zz", "zza", "f", "fo", "foo", "Foo", "FOO", "a", "b", "ba", "x"]
    for f in ("a", "b"):
        ts = terms[f]
        for k in rng.integers(0, len(ts), size=40):
            t = ts[int(k)].decode()
            pool.append(t[:int(rng.integers(1, 6))])
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]  # noqa: E731

    def one_part():
        kind = pick(["prefix", "fuzzy", "exact", "regex"], [0.8, 0.1, 0.06, 0.04])
        p = {"path": pick(["a", "b"]), "terms": [pick(pool)]}
        if kind == "regex":
            p["terms"] = [pick(["w[ab].*", "fo+", "zz[a-c].*", "q[abc]a.*"])]
            p["is_regex"] = True
        elif kind == "prefix":
            p["starts_with"] = True
            lev = pick([None, 0, 1, 2], [0.4, 0.3, 0.2, 0.1])
            if lev is not None:
                p["levenshtein_distance"] = lev
        elif kind == "fuzzy":
            p["levenshtein_distance"] = pick([1, 2])
        top = pick([None, 0, 1, 10, 200, 1848, 1849], [0.1, 0.05, 0.15, 0.45, 0.15, 0.05, 0.05])
        if top is not None:
            p["top"] = top
        skip = pick([None, 0, 3, 500], [0.5, 0.2, 0.2, 0.1])
        if skip is not None:
            p["skip"] = skip
        if top == 0 and not skip:  # top + skip == 0: only where fewer than 200 terms match (the reference panics beyond)
            p["terms"] = ["fo+"] if kind == "regex" else [pick(["zza", "foo", "qaa"])]
        boost = pick([None, 2.5, -1.0, 0.0], [0.7, 0.1, 0.1, 0.1])
        if boost is not None:
            p["boost"] = boost
        ic = pick([None, True, False], [0.6, 0.2, 0.2])
        if ic is not None:
            p["ignore_case"] = ic
        if p["path"] == "a" and rng.random() < 0.1:
            p["token_value"] = {"path": "a", "boost_fun": pick(["Multiply", "Add", "Log10"]), "param": 1}
        return p

    out = []
    for _ in range(n):
        k = int(pick([1, 2, 3], [0.5, 0.25, 0.25]))
        parts = [one_part() for _ in range(k)]
        if k == 1 and rng.random() < 0.5:
            out.append(parts[0])
        else:
            req = {"suggest": parts}
            if rng.random() < 0.8:
                req["top"] = pick([1, 10, 50])
            if rng.random() < 0.3:
                req["skip"] = pick([0, 2, 30])
            out.append(req)
    return out


def bits(rows):
    """[(text, score, id)] with the score as its f32 bits"""
    return [(t, struct.unpack("<I", struct.pack("<f", s))[0], i) for t, s, i in rows]


def as_text(req):
    return req if isinstance(req, str) else json.dumps(req)
