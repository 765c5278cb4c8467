"""The crafted corpus and the requests of tests/test_gpu_col_boost.py's whole-search checks: 131 072 docs — the smallest size at which a whole
index and each of two doc-range shards still has the 65 536 docs the rich k_scan_simple route asks for — with every kind of boost column.

Field `body` (identity column): four terms ta .. td with 9000 / 5000 / 3000 / 2000 postings and 250 planted common docs (an AND of two has a
few hundred hits, few enough to compare every hit's score) and two more (te, tf) for the shapes of more than four leaves; integer posting
scores below 2048 (exact in f16).  A token_value per term.  Filters go through `items[].text`: on an identity column like `body` a filter's ids
are the matched term ids (search_field.rs:474-481), which selects nothing here.
Boost columns: `pop` in [1, 1e5); `frac` in (0, 1) — negative logarithms; `zero` — a third of the rows 0.0, so that `v + 0 == 0` and the factor
is -inf; `gap` — about half the rows missing from the `present` bitmap; `items[].rank` — a 1:n column, 0-3 values on one doc in four, joined to
the leaf field `items[].text` (built by veloci_amd.mini_indexer, which knows the relations a 1:n boost walks).

No request here can score a hit NaN: no logarithm of a negative value, no 0 * -inf (a `zero` boost never follows a score that can be 0, and is
never followed by a multiplication with 0).  How a NaN ranks is not pinned; tests/test_gpu_col_boost.py's hook tests cover NaN values."""
import json

import numpy as np

NUM_DOCS = 131072
SEED = 90210
LISTS = {"ta": 9000, "tb": 5000, "tc": 3000, "td": 2000, "te": 2500, "tf": 3500}
PLANTED = 250
ITEM_WORDS = ["alpha", "alpine", "alps", "beta", "bet", "gamma"]
RARE_ITEM_WORDS = ["zeta", "zebra"]  # few enough docs for a window of 1024 to hold every hit


def build():
    """-> IndexData"""
    from veloci_amd import mini_indexer
    rng = np.random.default_rng(SEED)
    # the 1:n field first: the indexer makes the IndexData, the hand-made stores join it under their own paths
    docs = [{} for _ in range(NUM_DOCS)]
    for d in rng.choice(NUM_DOCS, NUM_DOCS // 4, replace=False):
        items = []
        for _ in range(int(rng.integers(0, 4))):
            word = str(rng.choice(RARE_ITEM_WORDS)) if rng.random() < 0.02 else str(rng.choice(ITEM_WORDS))
            it = {"text": word}
            if rng.random() < 0.85:
                it["rank"] = int(rng.integers(1, 9))
            items.append(it)
        if items:
            docs[int(d)]["items"] = items
    data, _ = mini_indexer.build_index(docs, {"*GLOBAL*": {"features": ["All"]}, "items[].text": {}, "items[].rank": {"boost": {"boost_type": "f32"}}})
    assert data.num_anchors == NUM_DOCS

    terms = sorted(LISTS)
    planted = rng.choice(NUM_DOCS, PLANTED, replace=False)
    offsets, anchors, scores = [0], [], []
    for t in terms:
        own = rng.choice(NUM_DOCS, LISTS[t], replace=False)
        docs_t = np.unique(np.concatenate([own, planted]) if t in ("ta", "tb", "tc", "td") else own).astype(np.uint32)
        anchors.append(docs_t)
        scores.append(rng.integers(1, 2048, len(docs_t)).astype(np.uint32))
        offsets.append(offsets[-1] + len(docs_t))
    anchors, scores = np.concatenate(anchors), np.concatenate(scores)
    data.add_fst("body.textindex", terms)
    data.set_column_meta("body", True, True)
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", offsets, anchors, scores, None)
    data.add_key_value_store("body.textindex.tokens_to_text_id", offsets, anchors)
    data.add_boost("body.textindex.token_values.boost_valid_to_value", rng.uniform(2.0, 500.0, len(terms)).astype(np.float32))

    data.add_boost("pop.boost_valid_to_value", (1.0 + rng.random(NUM_DOCS) * (1e5 - 1.0)).astype(np.float32))
    frac = rng.random(NUM_DOCS).astype(np.float32)
    frac[(frac <= 0) | (frac >= 1)] = np.float32(0.25)
    data.add_boost("frac.boost_valid_to_value", frac)
    data.add_boost("zero.boost_valid_to_value", rng.choice(np.array([0.0, 0.0, 0.0, 2.0, 3.0, 5.0, 10.0, 100.0, 7.5], np.float32), NUM_DOCS))
    data.add_boost("gap.boost_valid_to_value", rng.uniform(1.0, 1000.0, NUM_DOCS).astype(np.float32), present=(rng.random(NUM_DOCS) < 0.5).astype(np.uint8))
    return data


def leaf(term, **kw):
    return {"search": dict({"path": "body", "terms": [term]}, **kw)}


def tree(kind, *kids):
    return {kind: {"queries": [leaf(k) if isinstance(k, str) else k for k in kids]}}


def boost(path, fun, param=None, **kw):
    b = {"path": path, "boost_fun": fun}
    if param is not None:
        b["param"] = param
    b.update(kw)
    return b


RICH, TILE = "k_scan_simple<2,rich>", "k_tile_scan"
ITEM_FILTER = {"search": {"path": "items[].text", "terms": ["alpha"]}}  # about one doc in ten


def requests(skip_score):
    """-> [(name, request, kernel that answers it on an index or shard of 65 536 docs and more)].  skip_score: the unboosted score of some hit
    of AND(ta, tb), for the skip_when_score requests."""
    and2, or2 = tree("and", "ta", "tb"), tree("or", "tc", "td")
    and_of_ors = tree("and", tree("or", "ta", "td"), tree("or", "tb", "tc"))
    or5 = tree("or", "ta", "tb", "tc", "td", "te")
    and_of_or3 = tree("and", tree("or", "ta", "tb", "tc"), tree("or", "td", "te", "tf"))
    out = []

    def add(name, search_req, boosts, kernel=RICH, top=1024, **extra):
        r = {"search_req": search_req, "top": top, "boost": boosts}
        r.update(extra)
        out.append((name, r, kernel))

    logs = [("pop", "Log10", 1.0), ("pop", "Log2", 0.0), ("frac", "Log10", 0.0), ("frac", "Log2", 0.5), ("zero", "Log10", 0.0), ("zero", "Log2", 0.0), ("gap", "Log10", 1.0),
            ("gap", "Log2", None)]
    for col, fun, param in logs:  # every column under both logarithms: AND (every hit compared), AND of ORs, and the best ten of a leaf and an OR
        b = [boost(col, fun, param)]
        add(f"and {col} {fun}", and2, b)
        add(f"and-of-ors {col} {fun}", and_of_ors, b)
        add(f"leaf {col} {fun}", leaf("td"), b, top=10)
        add(f"or {col} {fun}", or2, b, top=10)
    for fun in ("Multiply", "Add", "Replace"):
        add(f"and pop {fun}", and2, [boost("pop", fun, 1.0)])
    add("leaf skip window", leaf("tc"), [boost("pop", "Log10", 1.0)], top=10, skip=25)
    add("or deep window", or2, [boost("frac", "Log10", 0.0)], top=1000, skip=24)
    # two boosts in sequence: the second sees the first's result (negative scores, -inf, a row that is missing)
    add("frac Log10 then pop Log2", and2, [boost("frac", "Log10", 0.0), boost("pop", "Log2", 1.0)])
    add("gap Log10 then zero Log10", and2, [boost("gap", "Log10", 1.0), boost("zero", "Log10", 0.0)])
    add("zero Log2 then pop Add", and_of_ors, [boost("zero", "Log2", 0.0), boost("pop", "Add", 0.0)])
    add("pop Log2 then gap Replace then frac Log10", and2, [boost("pop", "Log2", 1.0), boost("gap", "Replace", 1.0), boost("frac", "Log10", 0.0)])
    # expression and skip_when_score
    add("expression", and2, [boost("pop", "Log10", 1.0, expression="$SCORE / 1000")])
    add("expression only", and2, [{"path": "frac", "expression": "10 * $SCORE"}, boost("pop", "Log2", 0.0)])
    add("skip_when_score", and2, [boost("pop", "Log10", 1.0, skip_when_score=[skip_score])])
    add("skip_when_score of 3 and expression", and2, [boost("frac", "Log2", 0.0, skip_when_score=[1.0, skip_score, 2.5], expression="$SCORE - 0.5"), boost("pop", "Log10", 1.0)])
    # a token_value boost (host arithmetic, libm) under a column boost (device arithmetic)
    add("token_value and column", tree("and", leaf("ta", token_value={"path": "body", "boost_fun": "Log10", "param": 1.0}), "tb"), [boost("pop", "Log10", 1.0)])
    add("token_value Log2 leaf", leaf("td", token_value={"path": "body", "boost_fun": "Log2", "param": 0.0}), [boost("frac", "Log2", 0.0)], top=10)
    # a filter
    add("filter", and2, [boost("pop", "Log10", 1.0)], filter=ITEM_FILTER)
    add("filter or", or2, [boost("gap", "Log2", 1.0), boost("frac", "Log10", 0.0)], top=10, filter=ITEM_FILTER)
    # shapes the rich route declines (more than four leaves): k_tile_scan
    for col, fun, param in logs[:5] + logs[6:7]:
        add(f"or5 {col} {fun}", or5, [boost(col, fun, param)], kernel=TILE, top=10)
        add(f"and-of-or3 {col} {fun}", and_of_or3, [boost(col, fun, param)], kernel=TILE)
    add("or5 window", or5, [boost("pop", "Log10", 1.0), boost("gap", "Log2", 1.0)], kernel=TILE, top=1000, skip=24)
    add("and-of-or3 sequence", and_of_or3, [boost("frac", "Log10", 0.0, expression="$SCORE * 3"), boost("zero", "Log10", 0.0, skip_when_score=[0.0])], kernel=TILE)
    add("and-of-or3 filter", and_of_or3, [boost("pop", "Log2", 1.0)], kernel=TILE, filter=ITEM_FILTER)
    return out


def explain_requests():
    """explain: true (single requests and batches only: the sharded path declines explain).  No `zero` column: its -inf factor is not a JSON number."""
    and2 = tree("and", "ta", "tb")
    out = []
    for boosts in ([boost("pop", "Log10", 1.0)], [boost("frac", "Log10", 0.0)], [boost("gap", "Log10", 1.0), boost("pop", "Log2", 0.0)],
                   [boost("pop", "Log10", 0.0, expression="$SCORE / 7"), boost("frac", "Log10", 0.5)]):
        out.append({"search_req": and2, "top": 1024, "boost": boosts, "explain": True})
        out.append({"search_req": leaf("td"), "top": 10, "skip": 3, "boost": boosts, "explain": True})
        out.append({"search_req": tree("or", "tc", "td"), "top": 10, "boost": boosts, "explain": True})
    return out


def one_to_n_requests():
    """the 1:n boost op: leaves on items[].text, the boost on items[].rank (rank >= 1 and param >= 0: no -inf, no NaN)"""
    out = []
    for fun, param in (("Log10", 1.0), ("Log2", 1.0), ("Log10", 0.0), ("Log2", 0.0)):
        b = [{"path": "items[].rank", "boost_fun": fun, "param": param}]
        item = lambda term, **kw: {"search": dict({"path": "items[].text", "terms": [term]}, **kw)}
        out.append({"search_req": item("zeta"), "top": 1024, "boost": b})
        out.append({"search_req": item("ze", starts_with=True), "top": 1024, "boost": b})
        out.append({"search_req": item("alp", starts_with=True), "top": 10, "boost": b})
        out.append({"search_req": {"or": {"queries": [item("zebra"), leaf("td")]}}, "top": 10, "boost": b + [boost("pop", "Log10", 1.0)]})
        out.append({"search_req": {"and": {"queries": [item("al", starts_with=True), leaf("ta")]}}, "top": 1024, "boost": b})
    return out


def dumps(req):
    return json.dumps(req)
