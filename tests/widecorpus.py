"""Corpora for leaves that match very many dictionary terms (the dense union route): a vectorised numpy builder, straight through
IndexData.add_fst / add_token_to_anchor_score (synth.generate loops over its background terms in Python).

build(): T unique random 8-letter lowercase terms whose first letter is drawn from "abcd", every term with a list of 1-40 distinct
docs out of N and scores 1-199; two planted prefixes with exactly 4096 ("zr") and exactly 4097 ("zq") terms; a `cat` facet column;
the text_id_to_anchor store wordcorpus has.  crafted(): a corpus from explicit (term, docs) lists, for the degenerate shapes."""
import numpy as np

PLANTED = (("zr", 4096), ("zq", 4097))
CAT_VALUES = 16


def _planted(prefix, n):
    i = np.arange(n, dtype=np.int64) * 7919  # distinct six-letter tails (base 26)
    tails = np.stack([(i // 26 ** k) % 26 for k in range(5, -1, -1)], axis=1).astype(np.uint8) + ord("a")
    head = np.tile(np.frombuffer(prefix.encode(), np.uint8), (n, 1))
    return np.ascontiguousarray(np.concatenate([head, tails], axis=1)).view("S8").ravel()


def _finish(num_docs, terms, term_of_posting, docs, scores, seed):
    """terms: sorted unique bytes; postings as parallel arrays (any order, (term, doc) pairs may repeat: the first is kept)"""
    from veloci_amd.index import IndexData
    key = term_of_posting.astype(np.uint64) * np.uint64(num_docs) + docs.astype(np.uint64)
    key, first = np.unique(key, return_index=True)  # ascending (term, doc), distinct docs inside a list
    t = (key // np.uint64(num_docs)).astype(np.int64)
    lens = np.bincount(t, minlength=len(terms)).astype(np.uint64)
    offsets = np.zeros(len(terms) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    anchors = (key % np.uint64(num_docs)).astype(np.uint32)
    data = IndexData(num_docs)
    data.add_fst("body.textindex", terms)
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", offsets, anchors, scores[first].astype(np.uint32), None)
    data.add_key_value_store("body.textindex.text_id_to_anchor", offsets, anchors)
    data.add_fst("cat.textindex", ["cat%02d" % i for i in range(CAT_VALUES)])
    cat = np.random.default_rng(seed ^ 0xCA7).integers(0, CAT_VALUES, size=num_docs).astype(np.uint32)
    data.add_key_value_store("cat.textindex.parent_to_value_id", np.arange(num_docs + 1, dtype=np.uint64), cat)
    return data


def build(num_terms=40_000, num_docs=1_000_000, seed=11, planted=True):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 26, size=(num_terms + num_terms // 8 + 64, 8)).astype(np.uint8) + ord("a")
    raw[:, 0] = np.frombuffer(b"abcd", np.uint8)[rng.integers(0, 4, size=len(raw))]
    words = np.unique(np.ascontiguousarray(raw).view("S8").ravel())
    assert len(words) >= num_terms
    words = words[np.sort(rng.choice(len(words), size=num_terms, replace=False))]
    if planted:
        words = np.unique(np.concatenate([words] + [_planted(p, n) for p, n in PLANTED]))
        assert len(words) == num_terms + sum(n for _, n in PLANTED)
    lens = rng.integers(1, 41, size=len(words))
    term_of_posting = np.repeat(np.arange(len(words), dtype=np.int64), lens)
    docs = rng.integers(0, num_docs, size=len(term_of_posting))
    scores = rng.integers(1, 200, size=len(term_of_posting))
    terms = [bytes(w) for w in words.tolist()]  # (8 letters each: bytewise sorted, as np.unique left them)
    return _finish(num_docs, terms, term_of_posting, docs, scores, seed), terms


def crafted(num_docs, lists, seed=5):
    """lists: {term (str): array of docs}; scores 1-199 drawn here"""
    rng = np.random.default_rng(seed)
    terms = sorted(t.encode() for t in lists)
    per = [np.asarray(lists[t.decode()], np.int64) for t in terms]
    term_of_posting = np.repeat(np.arange(len(terms), dtype=np.int64), [len(p) for p in per])
    docs = np.concatenate(per)
    return _finish(num_docs, terms, term_of_posting, docs, rng.integers(1, 200, size=len(docs)), seed), terms
