"""A small corpus and highlight parts for the batched highlight (vq_highlight_batch): shared by tests/test_gpu_highlight_batch.py and the
host-stub driver tests/native/highlight_batch_driver.py.  About 400 documents through mini_indexer.build_index:

  title        tokenized root field, 1-20 words (a text of w words has 2 w - 1 tokens: the separators count).  `the` is in more than 300 texts;
               pr / pre / pref / prefix / prefixes / prefixation share a prefix and score by length; 30 texts hold `tieword` and nothing else
               that starts with `tie`, so a search for it ties on all of them; a few texts are one word (their own only token: no token rows)
  tags[]       short texts, many of one word; `zeal`, `zebra`, `zen` occur only as one-word texts
  sub[].text   nested texts
  code         not tokenized
and two fields built by hand: `broken`, whose text_id_to_token_ids lacks the row of a text that tokens_to_text_id lists (it fails the store
check of the device route), and `whole`, consistent and declared an identity column (its table is staged on the first batched highlight)."""
import json
import struct

import numpy as np

LETTERS = "abcdeilnors"  # (none of p, t, z: the planted words keep their counts)
FAMILY = ("pr", "pre", "pref", "prefix", "prefixes", "prefixation")
N_DOCS = 400
INDICES = {"*GLOBAL*": {"features": ["All"]}, "code": {"features": ["All"], "fulltext": {"tokenize": False}}}  # (All: text_id_to_token_ids is written)


def _word(rng):
    return "".join(LETTERS[int(k)] for k in rng.integers(0, len(LETTERS), size=int(rng.integers(2, 9))))


def documents():
    rng = np.random.default_rng(20)
    vocab = sorted({_word(rng) for _ in range(300)})
    docs = []
    for d in range(N_DOCS):
        n = int(rng.integers(1, 21)) if d % 40 else 1
        words = [vocab[int(k)] for k in rng.integers(0, len(vocab), size=n)]
        if n > 1:
            if d % 4 == 1:
                words[int(rng.integers(0, n))] = FAMILY[(d // 4) % len(FAMILY)]
            if d % 10 != 9:  # nine texts in ten
                words[int(rng.integers(0, n))] = "the" if d % 3 else "The"
            if d % 13 == 2 and n > 3:
                words[0] = "prefix"
                words[-1] = "pre"
            if d < 120 and d % 4 == 3:  # 30 texts
                words.append("tieword")
        sep = [" ", ", ", " - ", ". "]
        title = words[0]
        for w in words[1:]:
            title += sep[int(rng.integers(0, len(sep)))] + w
        tags = [vocab[int(k)] for k in rng.integers(0, 40, size=int(rng.integers(0, 4)))]
        if d % 7 == 0:
            tags.append("nice day for the " + vocab[d % 50])
        if d % 11 == 0:
            tags.append(("zeal", "zebra", "zen")[d % 3])
        if d % 9 == 0:
            tags.append("prefix " + vocab[d % 17])
        sub = [{"text": " ".join(vocab[int(k)] for k in rng.integers(0, 60, size=int(rng.integers(1, 8)))) + (" the end" if (d + j) % 2 else "")} for j in range(d % 3)]
        docs.append({"title": title, "tags": tags, "sub": sub, "code": "abc%d" % (d % 50)})
    return docs


def _add_hand_field(data, field, terms, token_rows, text_rows, identity):
    """a field by hand: sorted terms, tokens_to_text_id rows (token id -> text ids), text_id_to_token_ids rows (text id -> token ids)"""
    from veloci_amd.index import csr_from_lists
    assert terms == sorted(terms)
    n = len(terms)
    data.add_fst(field + ".textindex", [t.encode() for t in terms])
    data.set_column_meta(field, identity, True)
    offsets = np.arange(n + 1, dtype=np.uint64)
    anchors = np.arange(n, dtype=np.uint32)
    data.add_token_to_anchor_score(field + ".textindex.to_anchor_id_score", offsets, anchors, np.full(n, 10, np.uint32), None)
    data.add_key_value_store(field + ".textindex.text_id_to_anchor", offsets, anchors)
    data.add_key_value_store(field + ".textindex.tokens_to_text_id", *csr_from_lists([token_rows.get(t, []) for t in range(n)]))
    data.add_key_value_store(field + ".textindex.text_id_to_token_ids", *csr_from_lists([text_rows.get(t, []) for t in range(n)]))


def build():
    """-> (IndexData, info) as mini_indexer.build_index returns them, with the two hand-made fields added"""
    from veloci_amd import mini_indexer
    entries = [{"text": "the", "value": 2.0}, {"text": "prefix", "value": 3.0}, {"text": "pre", "value": 0.5}]
    data, info = mini_indexer.build_index(documents(), INDICES, token_values=(entries, "title"))
    terms = [" ", "alpha", "alpha beta", "alpha gamma", "beta", "gamma"]
    token_rows = {0: [2, 3], 1: [2, 3], 4: [2], 5: [3]}
    _add_hand_field(data, "broken", terms, token_rows, {2: [1, 0, 4]}, False)           # text 3 has no token row
    _add_hand_field(data, "whole", terms, token_rows, {2: [1, 0, 4], 3: [1, 0, 5]}, True)
    return data, info


def part(path, term, **kw):
    p = {"path": path, "terms": [term], "snippet": True}
    p.update({k: v for k, v in kw.items() if v is not None})
    return {k: v for k, v in p.items() if not (k == "snippet" and v == "absent")}


FREQUENT = part("title", "th", starts_with=True, top=10, skip=0)  # `the` / `The`: more than 300 texts, ten returned
HOST_ROUTE = [part("title", "pr", starts_with=True, top=10, boost=-1.0), part("title", "pr", starts_with=True, top=10, boost=0.0), part("title", "pr", starts_with=True)]
FAILING = ['{"path": "title", "terms": ["the"', part("nosuchfield", "the", top=10), part("code", "abc7", top=10), part("title", "the", top=10, snippet="absent"),
           part("tags[]", "ze", starts_with=True, top=10)]
BROKEN = [part("broken", "alpha", top=10), part("broken", "beta", top=10), part("broken", "a", starts_with=True, top=10), part("whole", "alpha", top=10),
          part("whole", "a", starts_with=True, top=1, skip=1), part("whole", "gamma", top=10)]


def fixed_parts():
    """every ingredient once, by hand"""
    P = part
    parts = [FREQUENT]
    for top in (1, 10, 1024, 1025):
        parts += [P("title", "the", top=top), P("title", "t", starts_with=True, top=top), P("title", "pr", starts_with=True, top=top, skip=0)]
    parts += [
        P("title", "pr", starts_with=True, top=5, skip=3),
        P("title", "pr", starts_with=True, top=1000, skip=24),                       # top + skip == 1024
        P("title", "pr", starts_with=True, top=1000, skip=25),                       # ... and just beyond: the host route
        P("title", "pr", starts_with=True, top=0, skip=2),
        P("title", "th", starts_with=True, top=10, skip=5000),                       # skip beyond the result
        P("title", "prefix", levenshtein_distance=1, top=10),
        P("title", "prefix", levenshtein_distance=2, starts_with=True, top=20),
        P("title", "pre.*", is_regex=True, top=10),
        P("title", "tie[a-z]+", is_regex=True, top=7),
        P("title", "tieword", top=10),                                               # 30 texts tie: the first ten by text id
        P("title", "tieword", top=10, skip=25),
        P("title", "pr", starts_with=True, top=10, boost=2.5),
        P("title", "THE", top=10, ignore_case=True),
        P("title", "The", top=10, ignore_case=False),
        P("title", "pr", starts_with=True, top=10, snippet_info={"num_words_around_snippet": 2, "snippet_start_tag": "<em>", "snippet_end_tag": "</em>", "snippet_connector": " [..] "}),
        P("title", "the", top=10, snippet_info={"max_snippets": 0}),
        P("title", "the", top=3, snippet_info={"num_words_around_snippet": 0, "max_snippets": 1}),
        P("title", "pr", starts_with=True, top=10, token_value={"path": "title", "boost_fun": "Multiply", "param": 0}),
        P("title", "pr", starts_with=True, top=10, token_value={"path": "title", "boost_fun": "Log10", "param": 0}),   # log10(0.5) < 0: a score below 0, the host route
        P("title", "nothere", top=10),
        P("title", "Prefix,", top=10),                                               # normalize_text rewrites the term
        P("tags[]", "nice", top=10), P("tags[]", "prefix", top=10), P("tags[]", "d", starts_with=True, top=10), P("tags[]", "the", top=1),
        P("sub[].text", "the", top=10), P("sub[].text", "end", top=10, skip=2), P("sub[].text", "e", starts_with=True, top=10),
    ]
    return parts + HOST_ROUTE + BROKEN


def random_parts(n, seed):
    rng = np.random.default_rng(seed)
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]  # noqa: E731
    pool = ["the", "The", "th", "t", "pr", "pre", "prefix", "prefixes", "tieword", "tie", "nice", "day", "end", "e", "a", "d", "s", "zeal", "ze", "nothere"]
    pool += [_word(rng)[:int(rng.integers(1, 4))] for _ in range(20)]
    out = []
    for _ in range(n):
        kind = pick(["prefix", "fuzzy", "exact", "regex"], [0.6, 0.15, 0.2, 0.05])
        p = {"path": pick(["title", "tags[]", "sub[].text", "whole", "broken"], [0.6, 0.15, 0.15, 0.05, 0.05]), "terms": [pick(pool)]}
        if p["path"] in ("whole", "broken"):
            p["terms"] = [pick(["alpha", "a", "beta", "gamma", "g"])]
        if kind == "regex":
            p["terms"] = [pick(["pre.*", "t[hi]e.*", "[a-c].*"])]
            p["is_regex"] = True
        elif kind == "prefix":
            p["starts_with"] = True
            if rng.random() < 0.3:
                p["levenshtein_distance"] = pick([0, 1])
        elif kind == "fuzzy":
            p["levenshtein_distance"] = pick([1, 2])
        if rng.random() < 0.93:
            p["snippet"] = True
        top = pick([None, 0, 1, 10, 200, 1024, 1025], [0.1, 0.05, 0.15, 0.45, 0.1, 0.1, 0.05])
        if top is not None:
            p["top"] = top
        skip = pick([None, 0, 3, 50], [0.5, 0.2, 0.2, 0.1])
        if skip is not None:
            p["skip"] = skip
        if top == 0 and not skip and p["path"] not in ("whole", "broken"):  # top + skip == 0: only where fewer than 200 terms match (the reference panics beyond)
            p["terms"] = ["tie[a-z]+"] if kind == "regex" else ["tieword"]
        boost = pick([None, 2.5, -1.0, 0.0], [0.8, 0.1, 0.05, 0.05])
        if boost is not None:
            p["boost"] = boost
        if rng.random() < 0.2:
            p["snippet_info"] = pick([{"num_words_around_snippet": 1}, {"max_snippets": 1, "num_words_around_snippet": 2}, {"snippet_connector": " ~ "}, {"max_snippets": 0}])
        if p["path"] == "title" and rng.random() < 0.1:
            p["token_value"] = {"path": "title", "boost_fun": pick(["Multiply", "Add", "Log10"]), "param": 1}
        out.append(p)
    return out


def bits(rows):
    """[(text, score, id)] with the score as its f32 bits"""
    return [(t, struct.unpack("<I", struct.pack("<f", s))[0], i) for t, s, i in rows]


def as_text(p):
    return p if isinstance(p, str) else json.dumps(p)
