"""The plain references of tests/prepass_ref.py, pinned against the CPU oracle: what the GPU tests (tests/test_gpu_prepass_lists.py) compare the
pre-pass kernels with is itself what the reference implementation computes for a whole request."""
import json

import numpy as np

import prepass_ref as R


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_union_reference_matches_the_oracle_on_a_prefix_leaf():
    """resolve_token_to_anchor (search_field.rs:419-464): a `starts_with` leaf over 300 terms of mixed lengths under one prefix; the oracle's
    (id, score bits) of ALL hits equal the union reference with term scores default_score_for_distance(Levenshtein distance of term and prefix
    = the extra letters, prefix_matches = true) — what the product's host code (term_lookup.cpp scoring_distance) hands k_union."""
    import widecorpus
    from oracle import binding as O
    rng = np.random.default_rng(17)
    num_docs, prefix = 2000, "pre"
    tails = {""}
    while len(tails) < 300:
        tails.add("".join(rng.choice(list("abcdefgh"), size=int(rng.integers(1, 9)))))
    lists = {prefix + t: rng.choice(num_docs, size=int(rng.integers(1, 60)), replace=False) for t in tails}
    lists.update({"other%03d" % i: rng.choice(num_docs, size=20, replace=False) for i in range(30)})  # terms the prefix does not match
    data, terms = widecorpus.crafted(num_docs, lists)
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    got = ora.search_json(json.dumps({"search_req": {"search": {"path": "body", "terms": [prefix], "starts_with": True}}, "top": num_docs + 1}))
    tokens = [i for i, t in enumerate(terms) if t.startswith(prefix.encode())]
    assert len(tokens) == 300 and len({len(terms[i]) for i in tokens}) == 9
    scores = [O.default_score_for_distance(len(terms[i]) - len(prefix), True) for i in tokens]
    docs, vals, max_value = R.union(data.token_to_anchor_score["body.textindex.to_anchor_id_score"], tokens, scores)
    assert got.num_hits == len(docs) == len(got.ids) and len(docs) > num_docs // 2
    assert sorted(zip(got.ids.tolist(), _bits(got.scores).tolist())) == list(zip(docs.tolist(), _bits(vals).tolist()))
    assert _bits([max_value])[0] == _bits(got.scores).max() == _bits(got.scores)[0]  # (positive floats order like their bit patterns; hits come best first)


def test_locality_reference_matches_the_oracle_on_a_repeated_text_field():
    """boost.rs:34-87 on a 1:n text field whose texts repeat across documents: a request with `text_locality` against the same request without.  A doc
    outside the reference's list keeps its score bit for bit; a doc inside has f32(score) * f32(2 * c * c), the smallest such factor of its texts
    — the oracle multiplies the hit's score by the boost value in one f32 multiplication (boost.rs:25-31 apply_boost_from_iter)."""
    from veloci_amd import mini_indexer
    from oracle import binding as O
    rng = np.random.default_rng(9)
    words = ["alpha", "alpine", "beta", "betal", "gamma", "delta", "omega", "river"]
    phrases = [" ".join(rng.choice(words, int(rng.integers(2, 5)))) for _ in range(40)]  # texts repeat across documents
    docs = [{"lines": [{"text": str(rng.choice(phrases))} for _ in range(int(rng.integers(1, 4)))]} for _ in range(400)]
    data, _ = mini_indexer.build_index(docs, {"lines[].text": {"fulltext": {"tokenize": True}}})
    ora = O.OracleIndex(data.num_anchors)
    data.load_into(ora)
    path = "lines[].text.textindex"
    t2t, t2a = data.key_value_stores[path + ".tokens_to_text_id"], data.key_value_stores[path + ".text_id_to_anchor"]
    leaf = lambda t: {"search": {"path": "lines[].text", "terms": [t]}}
    boosted = 0
    for terms in (("alpha", "beta"), ("gamma", "delta", "river"), ("omega", "alpine")):
        req = {"search_req": {"or": {"queries": [leaf(t) for t in terms]}}, "top": 1000}
        plain = ora.search_json(json.dumps(req))
        local = ora.search_json(json.dumps(dict(req, text_locality=True)))
        assert plain.num_hits == local.num_hits == len(plain.ids) > 50
        ldocs, lvals = R.locality(t2t, t2a, [data.term_id(path, t) for t in terms])
        factor = dict(zip(ldocs.tolist(), lvals.tolist()))
        assert len(factor) > 10 and set(factor) <= set(plain.ids.tolist())
        before = dict(zip(plain.ids.tolist(), plain.scores.tolist()))
        for doc, score in zip(local.ids.tolist(), local.scores):
            want = np.float32(before[doc]) * np.float32(factor[doc]) if doc in factor else np.float32(before[doc])
            assert _bits([score])[0] == _bits([want])[0], (terms, doc, score, before[doc], factor.get(doc))
        boosted += len(factor)
    assert boosted > 100
