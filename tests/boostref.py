"""A plain high-precision restatement of the column boost (add_boost / apply_boost, boost.rs:283-377, 470-504) and of the two logarithms it
takes.  Nothing of the product or the oracle runs here.

Logarithms: log10 / log2 of an f32, correctly rounded to f32 from numpy.longdouble (x87 extended, 64-bit mantissa).  The long-double result
carries an error of about 2^-63 relative, so an input is *usable* only when that result lies farther than 2^-58 (relative) from the midpoint of
two neighbouring f32 values — then no error of that size can change the rounding.  tests/golden/log_vectors.json (tests/gen_log_vectors.py,
mpmath at 200 bits) anchors the route; tests/test_boost_ref_cpu.py holds the two together and asserts that no committed input is unusable.

The boost: `v + param` in f32, the five functions, the optional expression added after, the `|skip - score| < 1e-5f` rule in f32, key_base /
num_keys / present — in numpy float32 steps, one IEEE rounding per operation (numpy never fuses a multiply with an add)."""
import json
import os

import numpy as np

F = np.float32
LD = np.longdouble
assert np.finfo(LD).nmant == 63, "boostref needs the 80-bit long double (64-bit mantissa) of x86"

HERE = os.path.dirname(os.path.abspath(__file__))
FUNS = ("Log2", "Log10", "Multiply", "Add", "Replace")  # BoostFunction, boost_request.rs:22-33 (the order of the product's BoostFun)
FUN_CODE = {None: -1, "Log2": 0, "Log10": 1, "Multiply": 2, "Add": 3, "Replace": 4}
MIDPOINT_MARGIN = LD(2.0) ** -58
MAX_DROP_FRACTION = 0.001


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(F)


def same(got, want):
    """element-wise: NaN results compare as "is NaN", everything else by bit pattern"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return np.where(np.isnan(want), np.isnan(got), bits(got) == bits(want))


def log_f32(fun, x):
    """fun "Log10" / "Log2" of the f32 array x -> (the correctly rounded f32 results, usable mask).  log(+-0) = -inf, log(x < 0) = NaN,
    log(+inf) = +inf, log(NaN) = NaN: exact, always usable."""
    x = np.ascontiguousarray(x, F)
    out = np.empty(len(x), F)
    usable = np.ones(len(x), bool)
    pos = (x > 0) & np.isfinite(x)
    out[x == 0] = -np.inf
    out[x < 0] = np.nan
    out[np.isnan(x)] = np.nan
    out[x == np.inf] = np.inf
    xl = x[pos].astype(LD)  # exact
    out[pos], usable[pos] = round_to_f32(np.log10(xl) if fun == "Log10" else np.log2(xl))
    return out, usable


def round_to_f32(y):
    """long-double values y (finite, well inside the f32 range) -> (y rounded to f32, True where y lies farther than MIDPOINT_MARGIN * |y| from
    both rounding midpoints around that f32)"""
    y = np.asarray(y, LD)
    r = y.astype(F)  # one rounding, to nearest even (the C conversion)
    rl = r.astype(LD)
    mid_up, mid_down = (rl + np.nextafter(r, F(np.inf)).astype(LD)) / 2, (rl + np.nextafter(r, F(-np.inf)).astype(LD)) / 2  # exact
    margin = MIDPOINT_MARGIN * np.abs(y)
    return r, (np.abs(y - mid_up) > margin) & (np.abs(y - mid_down) > margin)


def parse_expression(expression):
    """"x op y" (expression.rs:26-95): x / y = "$SCORE" (the boost value) or a float, op one of / * + -  ->  (left, op, right), an operand
    None for $SCORE, else its f32"""
    left, op, right = expression.split(" ")
    assert op in "/*+-" and len(op) == 1
    operand = lambda s: None if s == "$SCORE" else F(s)
    return operand(left), op, operand(right)


def apply_col_boost(fun, param, expression, skip, values, present_words, key_base, docs, scores):
    """The boost of one column applied to scores[i] for doc docs[i].  fun: one of FUNS or None; param: f32; expression: text or None; skip: the
    skip_when_score values; the column: `values` (f32, one per key from key_base on) and `present_words` (None: every row present; else bit
    r & 31 of word r >> 5 set for a present row r).
    -> (scores after the boost, log10 factor, usable): the factor is the f32 log10(v + param) of every doc with a present row (0.0 without one),
    usable is False where a logarithm this element depends on lies too close to a rounding midpoint to be called."""
    values = np.ascontiguousarray(values, F)
    docs = np.ascontiguousarray(docs, np.uint32).astype(np.int64)
    scores = np.ascontiguousarray(scores, F)
    param = F(param)
    n = len(docs)
    row = docs - int(key_base)
    has_row = (row >= 0) & (row < len(values))
    r = np.where(has_row, row, 0)
    if present_words is not None and len(values):
        words = np.ascontiguousarray(present_words, np.uint32)
        has_row &= ((words[r >> 5] >> (r & 31).astype(np.uint32)) & np.uint32(1)) == 1
    v = values[r] if len(values) else np.zeros(n, F)
    with np.errstate(all="ignore"):
        skipped = np.zeros(n, bool)
        for s in skip or ():
            skipped |= np.abs(F(s) - scores) < F(0.00001)  # NaN compares false: not skipped
        vp = v + param
        log10_vp, ok10 = log_f32("Log10", vp)
        usable = np.ones(n, bool)
        if fun == "Log10":
            boosted, usable = scores * log10_vp, ok10
        elif fun == "Log2":
            log2_vp, usable = log_f32("Log2", vp)
            boosted = scores * log2_vp
        elif fun == "Multiply":
            boosted = scores * vp
        elif fun == "Add":
            boosted = scores + vp
        elif fun == "Replace":
            boosted = vp.copy()
        else:
            assert fun is None
            boosted = scores.copy()
        if expression is not None:
            left, op, right = parse_expression(expression)
            a = v if left is None else np.full(n, left, F)
            b = v if right is None else np.full(n, right, F)
            e = a / b if op == "/" else a * b if op == "*" else a + b if op == "+" else a - b
            boosted = boosted + e
    applied = has_row & ~skipped
    out = np.where(applied, boosted, scores).astype(F)
    factor = np.where(has_row, log10_vp, F(0.0)).astype(F)
    return out, factor, np.where(applied, usable, True) & np.where(has_row, ok10, True)


# ---------------------------------------------------------------------------------------------- the inputs of the logarithm tests
POWERS_OF_TEN = [F(10 ** k) for k in range(11)]  # 1 .. 1e10: every power of ten that is exact in f32 (5^11 needs more than 24 bits)
RANDOM_SEED, RANDOM_COUNT = 20261, 20000
PARAMS = (0.0, 1.0, 0.5, -1.0)


def load_anchors():
    """tests/golden/log_vectors.json -> (inputs f32, exact log10 f32, exact log2 f32)"""
    with open(os.path.join(HERE, "golden", "log_vectors.json")) as f:
        doc = json.load(f)
    return tuple(from_bits(np.array([int(h, 16) for h in doc[k]], np.uint32)) for k in ("x_bits", "log10_bits", "log2_bits"))


def structured_inputs():
    """finite positive inputs where a logarithm goes wrong first: around 1, the exact powers, the ends of the range"""
    one = F(1.0)
    out = [one, np.nextafter(one, F(2.0)), np.nextafter(one, F(0.0))]
    out += POWERS_OF_TEN
    out += [F(np.ldexp(1.0, k)) for k in range(-149, 128)]  # every power of two, denormals included
    out += [from_bits(np.array([b], np.uint32))[0] for b in (1, 2, 3, 0x00400000, 0x007FFFFF, 0x00800000, 0x00800001)]  # denormals, FLT_MIN
    out += [np.finfo(F).max, np.nextafter(np.finfo(F).max, F(0.0))]
    return np.array(out, F)


def special_inputs():
    """+0 and -0 (-inf), negative values (NaN), +inf, NaN"""
    return np.array([0.0, -0.0, -1.5, -np.finfo(F).tiny, -np.inf, np.inf, np.nan], F)


def random_inputs():
    rng = np.random.default_rng(RANDOM_SEED)
    return from_bits(rng.integers(1, 0x7F800000, RANDOM_COUNT, dtype=np.uint32))  # every positive finite f32 is equally likely


def integer_inputs():
    return np.arange(1, 4097, dtype=F)  # (taken with each of PARAMS)


def log_inputs():
    """every input the logarithm tests take, as direct arguments of the logarithm (the integers already with each param added in f32)"""
    ints = integer_inputs()
    return np.concatenate([structured_inputs(), special_inputs()] + [ints + F(p) for p in PARAMS] + [random_inputs(), load_anchors()[0]])


# ---------------------------------------------------------------------------------------------- the elements of the boost tests
COLUMN = np.array([0.5, 1.0, 3.0, 99999.0, 1e-3, 0.0, -2.0, 1e30, 1e-10, 7.25, -0.0, 2.0, 1e5, 0.1, 1023.0, 6e-39], F)  # (6e-39: a denormal)
KEY_BASE, NUM_KEYS = 1000, 96  # the column is COLUMN six times over
SKIPS = ([], [0.5], [20.6, 0.0], [20.6, 0.0, -5.0], [20.6, 0.0, -5.0, 0.5])
EXPRESSIONS = (None, "$SCORE / 3", "$SCORE * 2.5", "$SCORE + 0.1", "$SCORE - 7", "10 / $SCORE", "3 * $SCORE", "1.5 + $SCORE", "100 - $SCORE", "$SCORE * $SCORE", "2 / 3",
               "$SCORE / $SCORE")


def boost_column():
    """-> (values, present words with rows 3, 31, 32 and 63 — the word boundaries — cleared)"""
    present = np.full(NUM_KEYS // 32, 0xFFFFFFFF, np.uint32)
    for row in (3, 31, 32, 63):
        present[row >> 5] &= ~np.uint32(1 << (row & 31))
    return np.tile(COLUMN, NUM_KEYS // len(COLUMN)), present


def boost_elements():
    """-> (docs, scores): every interesting doc (below the column, at both its ends, one past it, the last u32, every row) with every
    interesting score (positive, negative, -0, huge, tiny, infinite, exactly on a skip value and 0.99e-5 / 1.01e-5 to either side of it, as
    far as f32 has such a value)"""
    docs = np.array([0, KEY_BASE - 1, KEY_BASE, KEY_BASE + NUM_KEYS - 1, KEY_BASE + NUM_KEYS, 0xFFFFFFFF] + [KEY_BASE + r for r in range(NUM_KEYS)], np.uint32)
    near = []
    for s in (0.0, 0.5, 20.6, -5.0):
        near += [F(s), F(s) + F(0.99e-5), F(s) + F(1.01e-5), F(s) - F(0.99e-5), F(s) - F(1.01e-5)]
    scores = np.array([1.0, -1.0, -0.0, 3e38, -3e38, 1e-30, 12.34, 1e6, np.inf, -np.inf] + near, F)
    return np.repeat(docs, len(scores)), np.tile(scores, len(docs))


def ulp_distance(a, b):
    """distance in f32 steps between finite a and b (element-wise, over the ordered integers behind the bit patterns)"""
    def key(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
