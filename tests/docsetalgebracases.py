"""Doc set algebra (DocSet.combine, vq_docset_combine): the cases tests/test_gpu_docset_algebra.py runs on the device and
tests/native/docset_algebra_driver.py over the stubbed device layer, with the ids numpy expects of each.  No GPU is needed to import or check this
file.  Operands are the nine lists of docsetref.id_lists() on docsetref.NUM_ANCHORS anchors, on the whole index and on the shard docsetref.SHARD;
a case is (name, op, [operand, ...]) where an operand is the name of one of the nine lists or an id array of its own."""
import numpy as np

import docsetref

N = docsetref.NUM_ANCHORS
SHARD = docsetref.SHARD
RANGES = ((0, N), SHARD)
LISTS = docsetref.id_lists()
NAMES = list(LISTS)
OPS = ("and", "or", "minus")
EDGE_POSITIONS = (0, 31, 32, SHARD[0] - 1, SHARD[0], SHARD[1] - 1, SHARD[1], N - 1)


def ids_of(operand):
    return np.unique(np.asarray(LISTS[operand] if isinstance(operand, str) else operand, np.int64))


def expected(op, operands):
    """the ids of the whole result (numpy int64, sorted)"""
    sets = [ids_of(o) for o in operands]
    if op == "not":
        assert len(sets) == 1
        return np.setdiff1d(np.arange(N), sets[0])
    out = sets[0]
    for s in sets[1:]:
        out = {"and": np.intersect1d, "or": np.union1d, "minus": np.setdiff1d}[op](out, s)
    return out


def kind(ids, lo, hi):
    """the image a set of these ids carries on [lo, hi): "dense" (bitmap), "tiled" (tile directory only), "plain" (neither), "empty" (no local id)"""
    want = docsetref.image(ids, N, lo, hi)
    if want["bitmap"] is not None:
        return "dense"
    if want["tile_dir"] is not None:
        return "tiled"
    return "plain" if want["local_len"] else "empty"


_KIND_OF_LIST = {}


def has_bitmap(operand, lo, hi):
    if not isinstance(operand, str):
        return kind(ids_of(operand), lo, hi) == "dense"
    if (operand, lo, hi) not in _KIND_OF_LIST:
        _KIND_OF_LIST[(operand, lo, hi)] = kind(ids_of(operand), lo, hi)
    return _KIND_OF_LIST[(operand, lo, hi)] == "dense"


def expected_route(op, operands, lo, hi):
    """the routing rule: the probe route (1) for an AND with a bitmap-less operand and a MINUS whose minuend has none, else the word route (0)"""
    if op == "and":
        return int(any(not has_bitmap(o, lo, hi) for o in operands))
    if op == "minus":
        return int(not has_bitmap(operands[0], lo, hi))
    return 0


def pair_cases():
    """all 81 ordered pairs of the nine lists under and, or, minus"""
    return [("%s-%s-%s" % (a, op, b), op, [a, b]) for op in OPS for a in NAMES for b in NAMES]


def not_cases():
    return [("not-" + a, "not", [a]) for a in NAMES]


def edge_cases():
    """pairs of sets that differ in exactly one id, at the borders of a word, of the shard and of the index, on a base with a bitmap and on one without"""
    out = []
    for base_name in ("dense", "sparse"):
        for p in EDGE_POSITIONS:
            without = np.setdiff1d(ids_of(base_name), [p])
            with_p = np.union1d(without, [p])
            for op in OPS:
                out.append(("edge-%s-%d-%s" % (base_name, p, op), op, [with_p, without]))
            out.append(("edge-%s-%d-minus-reversed" % (base_name, p), "minus", [without, with_p]))
    return out


def nary_operands(seed=11):
    rng = np.random.default_rng(seed)
    holes = rng.permutation(N)[:7000].reshape(70, 100)
    nearly_all = [np.setdiff1d(np.arange(N), h) for h in holes]  # 70 sets, each `every` minus a different 100 ids
    small = [rng.choice(N, size=50, replace=False) for _ in range(70)]  # 70 sets of 50 random ids
    mixed = [small[k] if k % 2 else rng.choice(N, size=6000, replace=False) for k in range(70)]  # 35 without a bitmap, 35 with one
    a = rng.choice(N, size=2000, replace=False)
    three = [a, np.union1d(a[:1000], rng.choice(N, size=500, replace=False)), np.union1d(a[500:700], rng.choice(N, size=100, replace=False))]
    return {"nearly_all": nearly_all, "small": small, "mixed": mixed, "three": three, "holes": holes}


def nary_cases():
    o = nary_operands()
    cases = [
        ("and-70", "and", o["nearly_all"]),
        ("or-70", "or", o["small"]),
        ("or-70-mixed", "or", o["mixed"]),
        ("minus-70", "minus", ["every"] + o["mixed"]),
        ("minus-70-from-dense", "minus", ["dense"] + o["mixed"]),
        ("and-71-sparse-leader", "and", o["nearly_all"][:35] + ["sparse"] + o["nearly_all"][35:]),  # the probe route in rounds
        ("minus-70-sparse-minuend", "minus", ["repeated"] + o["mixed"]),
        ("mix-and", "and", ["sparse", "medium", "dense"]),
        ("mix-minus", "minus", ["dense", "sparse", "medium"]),
        ("mix-or", "or", ["one", "sparse", "dense"]),
        ("and-three-sparse", "and", [o["three"][0], o["three"][2], o["three"][1]]),  # the leader: the 300-id set in the middle
    ]
    for name in ("dense", "sparse", "empty"):
        cases += [("single-%s-%s" % (op, name), op, [name]) for op in OPS]
    return cases


def image_cases():
    return pair_cases() + not_cases() + edge_cases() + nary_cases()


OPERAND_KINDS = {  # list -> (whole index, shard)
    "medium": ("dense", "dense"), "dense": ("dense", "dense"), "every": ("dense", "dense"), "repeated": ("tiled", "tiled"), "sparse": ("tiled", "tiled"),
    "one": ("plain", "plain"), "edges": ("plain", "empty"), "empty": ("empty", "empty"), "last": ("plain", "empty"),
}


def assert_not_vacuous():
    """the expected results of the pairs cover every kind of image under every operation on both doc ranges, both routes are taken, the operands are
    of the kinds the routes depend on; -> {(op, range index): {kind: cases}}"""
    seen = {}
    for k, (lo, hi) in enumerate(RANGES):
        for name, kinds in OPERAND_KINDS.items():
            assert kind(ids_of(name), lo, hi) == kinds[k], (name, lo, hi, kind(ids_of(name), lo, hi))
        for _, op, operands in pair_cases():
            got = seen.setdefault((op, k), {})
            what = kind(expected(op, operands), lo, hi)
            got[what] = got.get(what, 0) + 1
        for op in OPS:
            assert set(seen[(op, k)]) == {"dense", "tiled", "plain", "empty"}, (op, lo, hi, seen[(op, k)])
            routes = {expected_route(op, operands, lo, hi) for _, o, operands in pair_cases() if o == op}
            assert routes == ({0} if op == "or" else {0, 1}), (op, routes)
        both = expected("and", ["sparse", "dense"])
        assert int(((both >= lo) & (both < hi)).sum()) == (83, 37)[k]
    o = nary_operands()
    assert len(expected("and", o["nearly_all"])) == N - 7000 and len(expected("and", o["three"])) == 200
    assert min(range(3), key=lambda i: len(ids_of(o["three"][i]))) == 2 and not any(has_bitmap(x, lo, hi) for x in o["three"] for lo, hi in RANGES)
    assert sum(has_bitmap(x, lo, hi) for x in o["mixed"] for lo, hi in RANGES) == 70 and not any(has_bitmap(x, lo, hi) for x in o["small"] for lo, hi in RANGES)
    names = [n for n, _, _ in image_cases()]
    assert len(names) == len(set(names)) == 243 + 9 + 64 + 20
    return seen
