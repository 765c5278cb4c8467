"""The yardsticks of tests/test_gpu_col_boost.py, checked without a GPU: tests/boostref.py's long-double logarithms against the mpmath anchors
(tests/golden/log_vectors.json), its midpoint rule on every committed input, the exact cases, the boost restatement on hand-computed values;
the oracle's "f64" log mode against boostref and beside its "libm" mode; and vq_debug_col_boost's argument handling on the stubbed device
layer, up to the point where it declines for want of a device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boostref as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def test_long_double_route_equals_the_mpmath_anchors():
    x, want10, want2 = B.load_anchors()
    assert len(x) == 2048 and np.all(x > 0) and np.all(np.isfinite(x))
    for fun, want in (("Log10", want10), ("Log2", want2)):
        got, usable = B.log_f32(fun, x)
        assert usable.all(), (fun, x[~usable])
        bad = ~B.same(got, want)
        assert not bad.any(), (fun, x[bad][:8], got[bad][:8], want[bad][:8])


def test_no_committed_input_is_dropped_by_the_midpoint_rule():
    x = B.log_inputs()
    assert len(x) > 30000
    for fun in ("Log10", "Log2"):
        _, usable = B.log_f32(fun, x)
        dropped = int((~usable).sum())
        print(fun, "inputs", len(x), "dropped", dropped)
        assert dropped <= B.MAX_DROP_FRACTION * len(x)
        assert dropped == 0, (fun, x[~usable])  # (pick other seeds rather than live with a drop)


def test_midpoint_rule_refuses_a_result_it_cannot_call():
    # the rule itself, on long-double values placed by hand around 1 + 2^-24, the midpoint between 1.0f and its upper neighbour
    mid = np.longdouble(1.0) + np.longdouble(2.0) ** -24
    offsets = [0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -56, -2.0 ** -56, 2.0 ** -30]
    r, usable = B.round_to_f32(np.array([mid + np.longdouble(o) for o in offsets]))
    assert usable.tolist() == [False, False, False, True, True, True]
    up = np.nextafter(F(1.0), F(2.0))
    assert r[3] == up and r[5] == up and r[4] == F(1.0)


def test_exact_cases():
    got, usable = B.log_f32("Log10", np.array(B.POWERS_OF_TEN, F))
    assert usable.all() and got.tolist() == [float(k) for k in range(11)]
    ks = np.arange(-149, 128)
    got, usable = B.log_f32("Log2", np.ldexp(1.0, ks).astype(F))
    assert usable.all() and got.tolist() == [float(k) for k in ks]
    for fun in ("Log10", "Log2"):
        got, usable = B.log_f32(fun, B.special_inputs())  # +0, -0, -1.5, -FLT_MIN, -inf, +inf, NaN
        assert usable.all()
        assert got[0] == -np.inf and got[1] == -np.inf and np.isnan(got[2:5]).all() and got[5] == np.inf and np.isnan(got[6])
        one = B.log_f32(fun, np.array([1.0], F))[0]
        assert B.bits(one)[0] == 0  # +0, not -0


def test_boost_restatement_on_hand_computed_values():
    values = np.array([10.0, 100.0, 0.5, 8.0], F)
    docs = np.array([4, 5, 6, 7, 8, 9], np.uint32)  # key_base 5: doc 4 is below the column, doc 9 one past it
    scores = np.full(6, 3.0, F)
    out, factor, usable = B.apply_col_boost("Log10", 0.0, None, [], values, None, 5, docs, scores)
    assert usable.all() and out.tolist() == [3.0, 3.0, 6.0, float(F(3.0) * F(np.log10(0.5))), float(F(3.0) * F(np.log10(8.0))), 3.0]
    assert factor.tolist()[:3] == [0.0, 1.0, 2.0] and factor[5] == 0.0
    present = np.array([0b1011], np.uint32)  # row 2 missing
    out, factor, _ = B.apply_col_boost("Log2", 0.0, None, [], values, present, 5, docs, scores)
    assert out.tolist() == [3.0, float(F(3.0) * F(np.log2(10.0))), float(F(3.0) * F(np.log2(100.0))), 3.0, 9.0, 3.0] and factor[3] == 0.0
    # function first, the expression (on the value, not value + param) added after; skip within 1e-5 of the incoming score
    out, _, _ = B.apply_col_boost("Multiply", 1.0, "$SCORE / 4", [2.0, 3.0], values, None, 5, docs, np.array([1.0, 1.0, 3.0, 3.000011, 2.000009, 1.0], F))
    assert out.tolist() == [1.0, float(F(11.0) + F(2.5)), 3.0, float(F(3.000011) * F(1.5) + F(0.125)), float(F(2.000009)), 1.0]
    out, _, _ = B.apply_col_boost("Add", -1.0, "2 - $SCORE", None, values, None, 5, docs, scores)
    assert out.tolist() == [3.0, 3.0 + 9.0 - 8.0, 3.0 + 99.0 - 98.0, 3.0 - 0.5 + 1.5, 3.0 + 7.0 - 6.0, 3.0]
    out, _, _ = B.apply_col_boost("Replace", 0.5, "$SCORE * $SCORE", None, values, None, 5, docs, scores)
    assert out.tolist() == [3.0, 110.5, 10100.5, 1.25, 72.5, 3.0]
    out, _, _ = B.apply_col_boost(None, 0.0, "1 + 1", None, values, None, 5, docs, scores)
    assert out.tolist() == [3.0, 5.0, 5.0, 5.0, 5.0, 3.0]


def test_boost_elements_fall_on_both_sides_of_the_skip_window_and_of_the_column():
    """what the GPU test feeds the hook: scores 0.99e-5 from a skip value are inside the f32 window and 1.01e-5 outside, docs lie on both sides
    of both ends of the column, and the cleared rows sit on the word boundaries"""
    (values, present), (docs, scores) = B.boost_column(), B.boost_elements()
    assert len(values) == B.NUM_KEYS == 32 * len(present) and [r for r in range(B.NUM_KEYS) if not (present[r >> 5] >> (r & 31)) & 1] == [3, 31, 32, 63]
    assert {B.KEY_BASE - 1, B.KEY_BASE, B.KEY_BASE + B.NUM_KEYS - 1, B.KEY_BASE + B.NUM_KEYS} <= set(docs.tolist())
    at = docs == B.KEY_BASE + 2  # value 3.0
    out, _, _ = B.apply_col_boost("Replace", 0.0, None, [0.0, 0.5], values, None, B.KEY_BASE, docs[at], scores[at])
    skipped = {float(s) for s, o in zip(scores[at], out) if B.bits(o) != B.bits(F(3.0))}
    d = F(0.99e-5)
    assert skipped == {0.0, float(F(1e-30)), float(d), float(-d), 0.5, float(F(0.5) + d), float(F(0.5) - d)}, skipped
    off = {float(F(1.01e-5)), float(F(0.5) + F(1.01e-5)), float(F(0.5) - F(1.01e-5))}
    assert off <= set(scores[at].tolist()) and not (off & skipped)
    out, factor, _ = B.apply_col_boost("Replace", 0.0, None, None, values, present, B.KEY_BASE, docs, np.full(len(docs), 12345.0, F))  # (no value is 12345)
    untouched = sorted(set(docs[B.bits(out) == B.bits(F(12345.0))].tolist()))
    assert untouched == [0, B.KEY_BASE - 1] + [B.KEY_BASE + r for r in (3, 31, 32, 63)] + [B.KEY_BASE + B.NUM_KEYS, 0xFFFFFFFF]


def test_oracle_f64_log_is_the_exact_log_and_libm_stays_within_its_documented_error():
    from oracle import binding as O
    x = B.log_inputs()
    seen_difference = False
    for fun, libm_bound in (("Log10", 2), ("Log2", 1)):
        want, usable = B.log_f32(fun, x)
        got = O.boost_log(fun, x, "f64")
        bad = usable & ~B.same(got, want)
        assert not bad.any(), (fun, x[bad][:8], got[bad][:8], want[bad][:8])
        libm = O.boost_log(fun, x, "libm")
        fin = np.isfinite(want)
        assert B.same(libm[~fin], want[~fin]).all()
        d = B.ulp_distance(libm[fin], want[fin])
        print(fun, "libm differs from the exact f32 on", int((d != 0).sum()), "of", int(fin.sum()), "inputs, by at most", int(d.max()), "ulp")
        assert d.max() <= libm_bound
        seen_difference = seen_difference or bool((d != 0).any())
    assert seen_difference  # the two modes are two definitions: this libm is not correctly rounded everywhere


def _tiny_index(values, tv_values=None):
    """one term `aaa` in every doc (posting score 100), the column `pop` with one value per doc; optionally a token_value of the term"""
    from veloci_amd.index import IndexData
    n = len(values)
    data = IndexData(n)
    data.add_fst("body.textindex", ["aaa"])
    data.set_column_meta("body", True, True)
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", [0, n], np.arange(n), np.full(n, 100, np.uint32))
    data.add_key_value_store("body.textindex.tokens_to_text_id", [0, n], np.arange(n))
    data.add_boost("pop.boost_valid_to_value", values)
    if tv_values is not None:
        data.add_boost("body.textindex.token_values.boost_valid_to_value", tv_values)
    return data


def test_oracle_log_mode_reaches_the_boost_stage_and_its_explain_record_only():
    from oracle import binding as O
    x, _, _ = B.load_anchors()
    x = x[(x > F(1e-30)) & (x < F(1e30))]  # (finite, non-zero logs: the records are read back through JSON)
    data = _tiny_index(x, tv_values=np.array([1234.5], F))
    ora = data.load_into(O.OracleIndex(data.num_anchors))
    with pytest.raises(KeyError):
        ora.set_boost_log("exact")
    results = {}
    for mode in (None, "libm", "f64"):
        if mode:
            ora.set_boost_log(mode)
        for fun in ("Log10", "Log2"):
            req = {"search_req": {"search": {"path": "body", "terms": ["aaa"]}}, "top": len(x), "explain": True, "boost": [{"path": "pop", "boost_fun": fun, "param": 0.0}]}
            results[mode, fun] = ora.search_json(json.dumps(req))
        tv = {"search_req": {"search": {"path": "body", "terms": ["aaa"], "token_value": {"path": "body", "boost_fun": "Log10", "param": 0.0}}}, "top": 5}
        results[mode, "tv"] = ora.search_json(json.dumps(tv))
    for fun in ("Log10", "Log2"):  # the default is libm
        assert results[None, fun].explain_json == results["libm", fun].explain_json and np.array_equal(B.bits(results[None, fun].scores), B.bits(results["libm", fun].scores))
    # token_value boosts are host arithmetic in the product: libm in both modes
    assert np.array_equal(B.bits(results["libm", "tv"].scores), B.bits(results["f64", "tv"].scores)) and results["f64", "tv"].scores[0] != 0
    base = results["f64", "tv"].scores[0] / np.log10(F(1234.5))  # (about the leaf's score; only used to see that the boost did apply)
    assert 0.5 < base < 200
    for fun in ("Log10", "Log2"):
        want, usable = B.log_f32(fun, x)
        assert usable.all()
        r = results["f64", fun]
        assert r.num_hits == len(x) and len(r.ids) == len(x)
        leaf = None
        for doc, score, records in zip(r.ids, r.scores, r.explain):
            boosts = [F(rec["Boost"]) for rec in records if "Boost" in rec]
            if leaf is None:  # every doc has the same leaf score: recover it from any other function-free record
                leaf = [F(rec["TermToAnchor"]["final_score"]) for rec in records if "TermToAnchor" in rec][0]
            if fun == "Log10":  # the factor record, then the score after the boost
                assert len(boosts) == 2 and B.bits(boosts[0]) == B.bits(want[doc]), (x[doc], boosts, want[doc])
            else:
                assert len(boosts) == 1
            assert B.bits(boosts[-1]) == B.bits(F(leaf * want[doc])) == B.bits(score), (fun, x[doc], boosts, leaf, want[doc], score)
        assert results["libm", fun].explain_json != r.explain_json  # (some anchor's libm logarithm is not the exact one)


_HOOK_SCRIPT = r"""
import ctypes as C, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.vq_last_error.restype = C.c_char_p
vp, u32 = C.c_void_p, C.c_uint32
f = L.vq_debug_col_boost
f.restype = C.c_int
f.argtypes = [C.c_int, C.c_float, C.c_char_p, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp]
values = np.arange(1, 65, dtype=np.float32)
present = np.array([0xFFFFFFFF, 0x7FFFFFFF], np.uint32)
docs = np.arange(0, 70, dtype=np.uint32)
scores = np.ones(70, np.float32)
out, fac = np.zeros(70, np.float32), np.zeros(70, np.float32)
skip = np.array([1, 2, 3, 4, 5], np.float32)
p = lambda a: a.ctypes.data_as(vp)
def call(fun=1, param=1.0, expr=None, n_skip=0, num_keys=64, pres=present, key_base=3, d=docs, n=70, o=out):
    return f(fun, param, expr, p(skip), n_skip, p(values), num_keys, None if pres is None else p(pres), key_base, None if d is None else p(d), p(scores), n, None if o is None else p(o), p(fac))
# what the parse and the argument checks take ends at the launcher: no device
assert call() == -1 and call(fun=-1, pres=None) == -1 and call(fun=4, expr=b"$SCORE * 2.5", n_skip=4) == -1 and call(fun=0, expr=b"10 / $SCORE", n_skip=1) == -1
# what they refuse never gets there
assert call(fun=5) == -2 and call(fun=-2) == -2 and call(n=0) == -2 and call(d=None) == -2 and call(o=None) == -2 and call(key_base=0xFFFFFFF0) == -2
assert call(n_skip=5) == -2 and b"skip_when_score" in L.vq_last_error()
assert call(expr=b"$SCORE ^ 2") == -2 and b"expression" in L.vq_last_error()
assert call(expr=b"$SCORE *") == -2
print("COL_BOOST_HOOK_OK")
"""


def test_hook_argument_handling_up_to_the_decline_on_the_stubbed_device():
    csrc = os.path.join(ROOT, "veloci_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    so = os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so")
    r = subprocess.run([sys.executable, "-c", _HOOK_SCRIPT, so], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "COL_BOOST_HOOK_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]


def test_every_layer_names_the_hook():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "veloci_amd/csrc/capi_debug.cpp", "tests/native/hip_stub_col_boost.cpp"):
        assert "debug_col_boost" in open(os.path.join(ROOT, rel)).read(), rel
