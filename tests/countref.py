"""What the count pre-pass measures, restated with numpy sets: the request's search_req walked in the compiler's preorder (the root is node 0,
an operand follows its predecessor's whole sub-tree), every node evaluated as a sorted array of doc ids.  A leaf is the union of the posting lists
of the dictionary terms it matches (the term itself, or every term with that prefix for `starts_with`; an unknown term matches nothing), an
`and` / `or` node the intersection / union of its operands (no operands: empty).  The request's `filter` — a leaf or a tree, evaluated the same
way — and its doc set are intersected into THE filter.  `lo` / `hi` restrict every result to a doc range (a shard).

node_counts -> ({node id: (hits, hits inside the filter)}, filter size or None).  Pinned against the oracle by tests/test_count_ref_cpu.py.

Not covered, and refused: leaves with other matching rules (levenshtein, regex), and an `or` with two plain leaves of the same term — the compiler
fuses those into one leaf and numbers the members together, which is no preorder."""
import numpy as np

EMPTY = np.zeros(0, np.int64)


def leaf_docs(part, lists):
    """lists: {path: {term (str): ascending doc ids}}"""
    assert not part.get("levenshtein_distance") and not part.get("is_regex"), part
    assert len(part["terms"]) == 1, part
    term, of_path = part["terms"][0], lists[part["path"]]
    if part.get("starts_with"):
        hit = [d for t, d in of_path.items() if t.startswith(term)]
    else:
        hit = [of_path[term]] if term in of_path else []
    return np.unique(np.concatenate([np.asarray(d, np.int64) for d in hit])) if hit else EMPTY


def node_docs(node, lists, visit=None):
    """the docs of a search_req / filter node; visit(docs) is called once per node, in preorder"""
    slot = None
    if visit is not None:
        slot = visit()
    if "search" in node:
        docs = leaf_docs(node["search"], lists)
    else:
        kind = "and" if "and" in node else "or"
        queries = node[kind]["queries"]
        if kind == "or":
            plain = [q["search"]["terms"][0] for q in queries if "search" in q]
            assert len(plain) == len(set(plain)), "an or with two leaves of one term is fused by the compiler: not numbered in preorder"
        docs = None
        for q in queries:
            d = node_docs(q, lists, visit)
            docs = d if docs is None else (np.intersect1d(docs, d) if kind == "and" else np.union1d(docs, d))
        if docs is None:
            docs = EMPTY
    if slot is not None:
        slot.append(docs)
    return docs


def filter_docs(request, lists, docset=None):
    """the ids of the request's filter (its `filter` and-ed with the doc set), or None without one"""
    f = node_docs(request["filter"], lists) if request.get("filter") is not None else None
    if docset is not None:
        ds = np.unique(np.asarray(docset, np.int64))
        f = ds if f is None else np.intersect1d(f, ds)
    return f


def node_counts(request, lists, docset=None, lo=0, hi=None):
    """-> ({node id: (hits, hits inside the filter)}, filter size); without a filter the second number of every pair and the size are None"""
    cut = (lambda d: d[(d >= lo) & (d < (np.iinfo(np.int64).max if hi is None else hi))])
    f = filter_docs(request, lists, docset)
    slots = []

    def visit():
        slots.append([])
        return slots[-1]

    node_docs(request["search_req"], lists, visit)
    out = {}
    for k, (docs,) in enumerate(slots):
        docs = cut(docs)
        out[k] = (len(docs), None if f is None else len(np.intersect1d(docs, f)))
    return out, (None if f is None else len(cut(f)))


def sub_requests(request):
    """[(node id, the node as a request of its own)] in preorder: what test_count_ref_cpu.py sends to the oracle"""
    out = []

    def walk(node):
        out.append((len(out), node))
        if "search" not in node:
            for q in node["and" if "and" in node else "or"]["queries"]:
                walk(q)

    walk(request["search_req"])
    return out
