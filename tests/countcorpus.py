"""The crafted corpus of the count pre-pass tests (tests/test_count_ref_cpu.py on the oracle alone, tests/test_gpu_count_prepass.py on the device):
201 608 docs — six tiles of 32768 and a seventh of 5000, as tests/test_gpu_probe_score_class.py — with posting lists built from numpy, no
column meta (so a `filter` leaf over `body` resolves through body.textindex.text_id_to_anchor, whose rows are the posting lists), and the requests
over it: the count shapes (doc positions, list kinds, trees, filters) and the near-tie cases T1 - T5, whose operand sizes lie one apart.

A near-tie case names its AND's operands, the operand the reference finds shortest and the one a count off by one would find (`alt`), and how to
`move` one doc so that the two closest sizes swap."""
import itertools

import numpy as np

TILE = 32768
N = 6 * TILE + 5000
POSTINGS = "body.textindex.to_anchor_id_score"
SET_LINE = 100_000  # a filter of up to this many ids is a FilterResult::Set: the operands' sizes inside it decide
ALL = 1000          # `top` of the near-tie requests: above every hit set here

EDGE_BASES = (0, TILE, 3 * TILE)
EDGES = sorted({0, N - 1} | {b + o for b in EDGE_BASES for o in (2047, 2048, 4095, 4096, 8191, 8192, 32767, 32768)})


def leaf(term, **kw):
    return {"search": dict({"path": "body", "terms": [term]}, **kw)}


def prefix(term):
    return leaf(term, starts_with=True)


def AND(*qs):
    return {"and": {"queries": list(qs)}}


def OR(*qs):
    return {"or": {"queries": list(qs)}}


def build_lists():
    """-> ({term: ascending unique doc ids (int64)}, info): info names the special docs"""
    rng = np.random.default_rng(20250611)
    L = {}
    special = np.array(EDGES, np.int64)
    pool = rng.permutation(np.setdiff1d(np.arange(N, dtype=np.int64), special))
    in_f = special[::2]  # every other edge doc lies in the filter — 0 among them; N - 1 is added below
    in_f = np.union1d(in_f, [N - 1])
    n_rand = SET_LINE - len(in_f)
    f_rand, rest = pool[:n_rand], pool[n_rand:]
    F = np.union1d(in_f, f_rand)
    assert len(F) == SET_LINE and 0 in F and N - 1 in F
    f_drop, x_vec = int(f_rand[0]), int(rest[0])  # in no other list: the docs by which the 99 999 / 100 001 filters differ
    cur = {"in": 1, "out": 1}

    def take(where, k):
        src = f_rand if where == "in" else rest
        out = src[cur[where]:cur[where] + k]
        cur[where] += k
        assert len(out) == k
        return out

    def put(name, *parts):
        docs = np.unique(np.concatenate([np.asarray(p, np.int64) for p in parts])) if parts else np.zeros(0, np.int64)
        assert name not in L
        L[name] = docs

    # ---- filters
    put("f100000", F)
    put("f099999", np.setdiff1d(F, [f_drop]))
    put("f100001", F, [x_vec])
    put("fempty")
    # ---- T1 / T5: three leaves whose sizes inside F are 600, 601, 602 and whose own sizes are 902, 901, 900; t1d ties with t1a inside F
    c1 = take("in", 400)
    put("t1a", c1, take("in", 200), take("out", 302))
    put("t1b", c1, take("in", 201), take("out", 300))
    put("t1c", c1, take("in", 202), take("out", 298))
    put("t1d", c1, take("in", 200), take("out", 310))
    # ---- T2: prefix families of two lists; union sizes 500, 501, 502, sums of the list lengths 750, 651, 602 (all docs inside F)
    c2 = take("in", 300)
    pa, pb, pc = take("in", 200), take("in", 201), take("in", 202)
    put("xa0", c2[:200], pa), put("xa1", c2[100:], pa[:150])
    put("xb0", c2[:200], pb), put("xb1", c2[100:], pb[:50])
    put("xc0", c2[:200], pc), put("xc1", c2[100:])
    # ---- T3: |t3a u t3b| = 501, |t3c n t3d| = 500, |t3e| = 502
    c3, s3 = take("in", 300), take("in", 200)
    put("t3a", c3[:150], take("out", 100)), put("t3b", c3[150:], take("out", 101))
    put("t3c", c3, s3, take("out", 100)), put("t3d", c3, s3, take("out", 150))
    put("t3e", c3, take("out", 202))
    # ---- T4: sizes inside F 600 and 601
    c4 = take("in", 300)
    put("l4a", c4, take("in", 300), take("out", 50))
    put("l4b", c4, take("in", 301), take("out", 40))
    # ---- doc positions and list kinds (count shapes)
    put("fsmall", c1[:40], c3[:40], take("in", 120), take("out", 100))  # a filter without a bitmap image
    put("pedge", special)                                                # tiny; every edge doc
    put("pfull", np.arange(2 * TILE, 3 * TILE), [4 * TILE + 777, 0, N - 1])  # a tile with every doc, a tile with exactly one
    every8 = np.arange(8192, N, 8)
    put("pal0", every8)
    for r in (1, 2, 3):  # r entries in front: the first entry of every later tile sits at list index r mod 4
        put("pal%d" % r, np.arange(1, r + 1), every8 + r)
    put("pmid", rng.choice(N, 1000, replace=False))  # a tile directory, no bitmap image
    for k, size in enumerate((20_000, 35_000, 50_000, 64_000, 90_000, 120_000)):
        put("d%d" % k, rng.choice(N, size, replace=False), special[k::3])
    put("ua0", L["d0"][:3000], special[:5]), put("ua1", L["d0"][2000:6000]), put("ua2", L["d0"][5000:5500], L["d1"][:700])
    for k in range(6):  # more than four lists: the leaf is materialised first
        put("uw%d" % k, L["d2"][k * 900:k * 900 + 1500], special[k::6])
    put("s0only", L["d3"][L["d3"] < 90_000][:5000]), put("s1only", L["d4"][L["d4"] >= 120_000][:5000])  # each inside one shard of the two-shard tests
    info = {"F": F, "f_drop": f_drop, "x_vec": x_vec}
    return L, info


def scores_of(term_index, docs):
    """integer scores below 2048 (exact in f16)"""
    return (1 + (docs * 7919 + term_index * 104729) % 1999).astype(np.uint32)


def index_data(L):
    from veloci_amd.index import IndexData, csr_from_lists
    terms = sorted(L)
    data = IndexData(N)
    data.add_fst("body.textindex", terms)
    off, docs = csr_from_lists([L[t] for t in terms])
    scores = np.concatenate([scores_of(k, L[t]) for k, t in enumerate(terms)])
    data.add_token_to_anchor_score(POSTINGS, off, docs, scores, None)
    data.add_key_value_store("body.textindex.text_id_to_anchor", off, docs)
    return data


def oracle_index(L):
    from oracle import binding as O
    return index_data(L).load_into(O.OracleIndex(N))


def moved(L, moves):
    """a copy of the lists with (term, doc, +1 / -1) applied: the doc added to / taken out of the term's list"""
    out = dict(L)
    for term, doc, sign in moves:
        assert (doc in out[term]) == (sign < 0), (term, doc, sign)
        out[term] = np.union1d(out[term], [doc]) if sign > 0 else np.setdiff1d(out[term], [doc])
    return out


# ---------------------------------------------------------------------------------------------------------------- the near-tie cases
def and_order(n, shortest):
    """summation order of an AND of n operands whose `shortest` is taken out and added last (swap_remove)"""
    order = list(range(n))
    order[shortest] = order[n - 1]
    order.pop()
    return order + [shortest]


def only_in(L, term, others, inside=None, outside=None):
    """a doc of `term` that is in none of `others` (and inside / outside the given set)"""
    d = L[term]
    for o in others:
        d = np.setdiff1d(d, L[o])
    if inside is not None:
        d = np.intersect1d(d, inside)
    if outside is not None:
        d = np.setdiff1d(d, outside)
    return int(d[0])


def near_tie_cases(L, info):
    """-> [case]: name, request (filter-leaf form, what the oracle takes), docset (None, or the filter term whose ids the product gets as a doc set
    instead of the `filter`), operands (the AND's operands as sub-trees), sizes (the numbers the reference compares), shortest / alt (operand
    indices), path (where the AND sits: "root" or "or0"), move (the doc moves after which alt IS the shortest)"""
    F = info["F"]
    cases = []

    def add(name, operands, sizes, flt=None, docset=False, move=None, wrap=None):
        lo = min(sizes)
        shortest = sizes.index(lo)
        others = sorted(s for i, s in enumerate(sizes) if i != shortest)
        assert others[0] - lo <= 1, (name, sizes)  # the two smallest sizes: one apart, or equal (the first wins)
        alt = min((i for i in range(len(sizes)) if i != shortest), key=lambda i: (sizes[i], i))
        node = AND(*operands)
        req = {"search_req": wrap(node) if wrap else node, "top": ALL}
        if flt:
            req["filter"] = leaf(flt)
        cases.append({"name": name, "request": req, "docset": flt if docset else None, "operands": list(operands), "sizes": list(sizes), "shortest": shortest, "alt": alt,
                      "filter": flt, "move": move, "label": wrap is not None})

    t1 = {"t1a": (600, 902), "t1b": (601, 901), "t1c": (602, 900), "t1d": (600, 910)}
    for flt, which, tag in (("f100000", 0, "set"), ("f100001", 1, "vec")):
        for docset in (False, True):
            kind = "T5" if docset else "T1"
            for perm in itertools.permutations(("t1a", "t1b", "t1c")):
                lo2 = sorted(perm, key=lambda t: t1[t][which])[:2]  # the two closest: a doc of the second smallest moves to the smallest
                doc = only_in(L, lo2[1], [t for t in t1 if t != lo2[1]], inside=F if which == 0 else None, outside=None if which == 0 else F)
                add("%s-%s-%s" % (kind, tag, "".join(t[-1] for t in perm)), [leaf(t) for t in perm], [t1[t][which] for t in perm], flt, docset,
                    move=[(lo2[1], doc, -1), (lo2[0], doc, +1)])
            if which == 0:  # two equal smallest sizes: the first minimal operand wins, whichever it is
                for perm in (("t1d", "t1c", "t1a"), ("t1c", "t1a", "t1d")):
                    add("%s-set-tie-%s" % (kind, "".join(t[-1] for t in perm)), [leaf(t) for t in perm], [t1[t][0] for t in perm], flt, docset)
    # T2: the sizes of the unions decide (500, 501, 502), not the sums of the list lengths (750, 651, 602)
    doc = only_in(L, "xb0", ["xa0", "xa1", "xb1", "xc0", "xc1"])
    for flt in (None, "f100000"):
        for perm in (("xa", "xb", "xc"), ("xc", "xa", "xb"), ("xb", "xc", "xa")):
            sizes = [{"xa": 500, "xb": 501, "xc": 502}[p] for p in perm]
            add("T2-%s-%s" % ("set" if flt else "plain", "".join(p[-1] for p in perm)), [prefix(p) for p in perm], sizes, flt,
                move=[("xb0", doc, -1), ("xa0", doc, +1)])
    # T3: sub-tree operands
    doc = only_in(L, "t3a", ["t3b", "t3c", "t3d", "t3e"])
    subs = {"or": (OR(leaf("t3a"), leaf("t3b")), 501), "and": (AND(leaf("t3c"), leaf("t3d")), 500), "e": (leaf("t3e"), 502)}
    for perm in (("or", "and", "e"), ("e", "or", "and"), ("and", "e", "or")):
        add("T3-" + "-".join(perm), [subs[p][0] for p in perm], [subs[p][1] for p in perm], move=[("t3a", doc, -1), ("t3c", doc, +1), ("t3d", doc, +1)])
    # T4: the label of a two-operand AND inside an OR is its LONGER operand's; a' carries the first operand's term
    doc = only_in(L, "l4b", ["l4a"], inside=F)
    for first, second, sizes in (("l4a", "l4b", [600, 601]), ("l4b", "l4a", [601, 600])):
        add("T4-%s%s" % (first[-1], second[-1]), [leaf(first), leaf(second)], sizes, "f100000", move=[("l4b", doc, -1), ("l4a", doc, +1)],
            wrap=lambda node, first=first: OR(node, leaf(first)))
    return cases


def operand_values(ora, case, cache):
    """{doc: f32 score} per operand of the case's AND: the oracle's answer to the operand as a request of its own (under the case's filter)"""
    import json
    out = []
    for op in case["operands"]:
        req = {"search_req": op, "top": 5000}
        if case["filter"]:
            req["filter"] = leaf(case["filter"])
        key = json.dumps(req, sort_keys=True)
        if key not in cache:
            w = ora.search_json(key)
            assert w.num_hits == len(w.ids)
            cache[key] = dict(zip(np.asarray(w.ids).tolist(), np.asarray(w.scores, np.float32).tolist()))
        out.append(cache[key])
    return out


def summed(values, order, docs):
    """f32 sums of the operands' scores in `order`, per doc"""
    acc = np.array([values[order[0]][d] for d in docs], np.float32)
    for k in order[1:]:
        acc = acc + np.array([values[k][d] for d in docs], np.float32)
    return acc


def order_precondition(ora, case, cache):
    """A three-operand case: the reference's summation order and the order a count off by one would select give different f32 score bits for
    some hit.  -> (hits, hits whose bits differ, the expected scores per doc)"""
    values = operand_values(ora, case, cache)
    docs = sorted(set.intersection(*[set(v) for v in values]))
    n = len(values)
    want = summed(values, and_order(n, case["shortest"]), docs)
    other = summed(values, and_order(n, case["alt"]), docs)
    differ = int((want.view(np.uint32) != other.view(np.uint32)).sum())
    return len(docs), differ, dict(zip(docs, want.tolist()))


# ---------------------------------------------------------------------------------------------------------------- the count shapes
def count_requests():
    """-> [(name, request, docset)]: docset None, or the term whose ids are attached as a doc set.  Every request either measures nodes or is
    marked by its name ("plain-...") as one that needs no count pre-pass."""
    big = "f100000"
    R = []

    def add(name, search_req, flt=None, docset=None):
        req = {"search_req": search_req, "top": 10}
        if flt is not None:
            req["filter"] = flt
        R.append((name, req, docset))

    add("and3-set", AND(leaf("t1a"), leaf("t1b"), leaf("t1c")), leaf(big))
    add("and3-positions", AND(leaf("pedge"), leaf("pfull"), leaf("d5")), leaf(big))
    add("and3-tiny-lists", AND(leaf("pedge"), leaf("pmid"), leaf("fsmall")), leaf("fsmall"))
    add("and4-alignment", AND(leaf("pal1"), leaf("pal2"), leaf("pal3"), leaf("pal0")), leaf("d5"))
    add("and3-dense", AND(leaf("d3"), leaf("d4"), leaf("d5")), leaf("f100001"))
    add("and-or-and-leaf", AND(OR(leaf("d0"), leaf("pmid")), AND(leaf("d4"), leaf("d5")), leaf("d3")))
    add("depth3", AND(OR(AND(leaf("d3"), leaf("d4"), leaf("pfull")), leaf("pedge")), OR(leaf("d1"), AND(leaf("d2"), leaf("d5"))), leaf("d5")), leaf(big))
    add("and16", AND(*[leaf(t) for t in ("d5", "d4", "d3", "d2", "d1", "d0", "pfull", "pal0", "pal1", "pal2", "pal3", "f100000", "f100001", "f099999", "d5", "d4")]), leaf("d5"))
    add("union-leaf-materialised", AND(prefix("ua"), leaf("d0"), prefix("uw")), leaf(big))
    add("unknown-term", AND(leaf("nosuch"), leaf("d0"), leaf("d1")), leaf(big))
    add("label-2-lists", OR(AND(prefix("ua"), leaf("d0")), leaf("d1")))          # no AND of three: the leaf's lists are OR-ed by the presence program
    add("label-filter", OR(AND(leaf("l4a"), leaf("l4b")), leaf("l4a")), leaf(big))
    add("filter-tree", AND(leaf("d3"), leaf("d4"), leaf("pfull")), OR(AND(leaf(big), leaf("d5")), leaf("fsmall")))
    add("filter-empty", AND(leaf("d3"), leaf("d4"), leaf("d5")), leaf("fempty"))
    for f in ("f099999", "f100000", "f100001"):
        add("filter-" + f, AND(leaf("d3"), leaf("pedge"), leaf("d5")), leaf(f))
    add("docset-small", AND(leaf("d3"), leaf("d4"), leaf("d5")), None, "fsmall")
    add("docset-bitmap", AND(leaf("d3"), leaf("pedge"), leaf("d5")), None, "f100000")
    add("docset-and-filter", AND(leaf("d3"), leaf("d4"), leaf("pfull")), leaf("d5"), "f100001")
    add("docset-empty", AND(leaf("d3"), leaf("d4"), leaf("d5")), None, "fempty")
    add("one-shard-lists", AND(leaf("s0only"), leaf("d5"), leaf("s1only")), leaf(big))
    add("one-shard-list", AND(leaf("s0only"), leaf("d5"), leaf("d3")), leaf("f100001"))
    add("plain-leaf", leaf("d0"))
    add("plain-and3", AND(leaf("d0"), leaf("d1"), leaf("d2")))   # single lists, no filter: every size is a list length
    add("plain-or", OR(leaf("d0"), leaf("pmid")), leaf(big))
    return R


def limit_request(measured):
    """an AND tree whose every node but the root is measured: levels of (sub-tree, 3 known leaves, 4 unknown ones) under a filter"""
    assert measured >= 16
    known, unknown = [leaf(t) for t in ("d0", "d1", "d2")], [leaf("nosuch%d" % k) for k in range(4)]
    levels, last = divmod(measured, 8)
    if last < 3:
        levels, last = levels - 1, last + 8
    node = AND(*(known + unknown + known + unknown)[:last])
    for _ in range(levels):
        node = AND(node, *known, *unknown)
    return {"search_req": node, "filter": leaf("f100000"), "top": 10}
