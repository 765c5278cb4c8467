"""Log-boost scores pinned bit for bit.  Two questions, kept apart:

1. Is the device's logarithm right?  vq_debug_col_boost runs the scans' own boost functions alone; their results are held against
   tests/boostref.py (exact logarithms from long double, anchored by mpmath vectors) element for element, NaN values included — and the device
   factor against the host's libm, which may differ by its documented error and no more.
2. Is everything around it right?  Whole searches on a crafted corpus (tests/boostcorpus.py) against the oracle in its "f64" log mode, which
   takes the logarithm of a column boost the way the device does: ids, every score bit and every explain record must be the same — alone, in
   a batch and over two doc-range shards, on the rich k_scan_simple route and on k_tile_scan.

Requests whose final scores could be NaN (0 * -inf, the logarithm of a negative value) are kept out of the searches: how a NaN ranks is not
defined here.  The hook tests cover NaN values."""
import ctypes as C
import json

import numpy as np
import pytest

import boostref as B

pytestmark = pytest.mark.gpu
F = np.float32


def run_hook(fun, param, expression, skip, values, present_words, key_base, docs, scores):
    import veloci_amd
    L = veloci_amd.lib()
    values, docs, scores = np.ascontiguousarray(values, F), np.ascontiguousarray(docs, np.uint32), np.ascontiguousarray(scores, F)
    skip = np.ascontiguousarray(skip if skip else [], F)
    out, factor = np.full(len(docs), 12345.0, F), np.full(len(docs), 12345.0, F)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.vq_debug_col_boost(B.FUN_CODE[fun], float(param), expression.encode() if expression is not None else None, p(skip), len(skip), p(values), len(values),
                              p(None if present_words is None else np.ascontiguousarray(present_words, np.uint32)), key_base, p(docs), p(scores), len(docs), p(out), p(factor))
    assert rc == 0, (rc, L.vq_last_error())
    return out, factor


def check_hook(fun, param, expression, skip, values, present_words, key_base, docs, scores, what):
    """-> (elements compared, elements the midpoint rule dropped)"""
    got, got_factor = run_hook(fun, param, expression, skip, values, present_words, key_base, docs, scores)
    want, want_factor, usable = B.apply_col_boost(fun, param, expression, skip, values, present_words, key_base, docs, scores)
    for name, g, w in (("score", got, want), ("log10 factor", got_factor, want_factor)):
        bad = np.flatnonzero(usable & ~B.same(g, w))
        rows = np.asarray(docs, np.int64)[bad[:8]] - key_base
        assert len(bad) == 0, (what, name, len(bad), "docs", np.asarray(docs)[bad[:8]].tolist(), "values", [float(values[r]) if 0 <= r < len(values) else None for r in rows],
                               "scores in", np.asarray(scores, F)[bad[:8]].tolist(), "got", g[bad[:8]].tolist(), "want", w[bad[:8]].tolist())
    return int(usable.sum()), int((~usable).sum())


def test_log_vectors_through_the_device_boost_are_the_exact_logs():
    """score 1.0 * log(v + param): the result is the device's logarithm itself.  Every committed vector, by bit pattern (NaN as NaN)."""
    direct = np.concatenate([B.structured_inputs(), B.special_inputs(), B.random_inputs(), B.load_anchors()[0]])
    ints = B.integer_inputs()
    compared = dropped = 0
    for fun in ("Log10", "Log2"):
        for values, param in [(direct, 0.0)] + [(ints, p) for p in B.PARAMS]:
            c, d = check_hook(fun, param, None, None, values, None, 0, np.arange(len(values)), np.ones(len(values), F), (fun, param))
            compared, dropped = compared + c, dropped + d
    print("vector elements compared", compared, "dropped by the midpoint rule", dropped, "device results that are not the exact f32 logarithm: 0")
    assert dropped == 0 and compared == 2 * (len(direct) + len(B.PARAMS) * len(ints))


def test_device_log_against_the_hosts_libm_stays_within_its_documented_error():
    """|device - libm| <= 2 ulp for log10, <= 1 ulp for log2: glibc's documented errors for log10f / log2f (the device side is exact, see above).
    libm is reached through the oracle's "libm" logarithm, the very call its boost stage makes."""
    from oracle import binding as O
    x = B.log_inputs()
    for fun, bound in (("Log10", 2), ("Log2", 1)):
        got, _ = run_hook(fun, 0.0, None, None, x, None, 0, np.arange(len(x)), np.ones(len(x), F))
        libm = O.boost_log(fun, x, "libm")
        fin = np.isfinite(libm)
        assert B.same(got[~fin], libm[~fin]).all()
        d = B.ulp_distance(got[fin], libm[fin])
        print(fun, "largest device-to-libm difference", int(d.max()), "ulp;", int((d != 0).sum()), "of", int(fin.sum()), "inputs differ")
        assert d.max() <= bound, (fun, x[fin][d > bound][:8])


def test_every_function_expression_skip_and_row_against_the_restatement():
    """Every function with and without each operator, both operand kinds on both sides; scores positive, negative, +-0, huge, infinite, on and
    just off a skip value (1 - 4 skip values); docs below, at both ends of and one past the column; rows 31, 32, 63 (word boundaries) and 3
    cleared in `present`.  NaN and infinite results included."""
    (values, present), (docs, scores) = B.boost_column(), B.boost_elements()
    calls = 0
    for fi, fun in enumerate((None,) + B.FUNS):
        for ei, expression in enumerate(B.EXPRESSIONS):
            for words in (None, present):
                skip = B.SKIPS[(fi + ei + (words is not None)) % len(B.SKIPS)]
                for param in (0.0, 1.0) if expression is None else (0.5,):
                    check_hook(fun, param, expression, skip, values, words, B.KEY_BASE, docs, scores, (fun, param, expression, skip, words is not None))
                    calls += 1
        for skip in B.SKIPS:  # every number of skip values under every function
            check_hook(fun, -1.0, None, skip, values, present, B.KEY_BASE, docs, scores, (fun, skip))
            calls += 1
    assert calls == 6 * (2 * (len(B.EXPRESSIONS) - 1) + 4 + len(B.SKIPS))


def test_hook_refuses_what_the_request_parser_refuses():
    import veloci_amd
    L = veloci_amd.lib()
    one = np.ones(4, F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    docs = np.arange(4, dtype=np.uint32)
    call = lambda fun, expr, n_skip, n: L.vq_debug_col_boost(fun, 0.0, expr, p(np.ones(5, F)), n_skip, p(one), 4, None, 0, p(docs), p(one), n, p(one.copy()), p(one.copy()))
    assert call(1, None, 0, 4) == 0
    assert call(1, None, 5, 4) == -2 and call(1, b"$SCORE % 2", 0, 4) == -2 and call(9, None, 0, 4) == -2 and call(1, None, 0, 0) == -2


# ------------------------------------------------------------------------------------------------------------ whole searches
@pytest.fixture(scope="module")
def crafted():
    import veloci_amd
    import boostcorpus as BC
    from oracle import binding as O
    data = BC.build()
    ora = data.load_into(O.OracleIndex(data.num_anchors))
    ora.set_boost_log("f64")
    idx = veloci_amd.Index(data, device=0)
    idx.profile_enable(True)
    base = ora.search_json(json.dumps({"search_req": BC.tree("and", "ta", "tb"), "top": 1024}))
    assert 300 <= base.num_hits <= 1024
    reqs = BC.requests(float(base.scores[len(base.scores) // 3]))
    wants = [ora.search_json(json.dumps(r)) for _, r, _ in reqs]  # computed once, shared by the three routes
    return data, idx, ora, reqs, wants


def scan_kernels(idx):
    return {k for k in idx.profile_json(reset=True)["kernels"] if k.startswith("k_scan") or k == "k_tile_scan"}


def test_corpus_reaches_what_it_is_meant_to_reach(crafted):
    """the yardstick's side: negative scores, -inf factors, missing rows, a skip that fires, windows that hold every hit, no NaN anywhere"""
    import boostcorpus as BC
    _, _, ora, reqs, wants = crafted
    by_name = {name: (r, w) for (name, r, _), w in zip(reqs, wants)}
    for name, (r, w) in by_name.items():
        assert w.num_hits > 0 and len(w.ids) > 0 and not np.isnan(w.scores).any(), name
    assert by_name["and frac Log10"][1].scores.max() < 0 and by_name["and pop Log10"][1].num_hits == len(by_name["and pop Log10"][1].ids)
    # the reference's top-n loop drops a hit below -FLT_MAX (sort.rs:5-22): the hits a `zero` row sends to -inf leave the window
    zero = by_name["and zero Log10"][1]
    assert 0 < len(zero.ids) < zero.num_hits <= 1024 and np.isfinite(zero.scores).all()
    assert np.isinf(by_name["and-of-or3 sequence"][1].scores).any()  # (+inf: a negative score times -inf)
    plain, skipping = by_name["and pop Log10"][1], by_name["skip_when_score"][1]
    assert sorted(plain.ids.tolist()) == sorted(skipping.ids.tolist()) and plain.ids.tolist() != skipping.ids.tolist()
    gap, unboosted = by_name["and gap Log10"][1], ora.search_json(json.dumps({"search_req": by_name["and gap Log10"][0]["search_req"], "top": 1024}))
    same_score = len(set(zip(gap.ids.tolist(), B.bits(gap.scores).tolist())) & set(zip(unboosted.ids.tolist(), B.bits(unboosted.scores).tolist())))
    assert len(gap.ids) // 4 < same_score < 3 * len(gap.ids) // 4  # about half the hits have no `gap` row and keep their score
    assert {k for _, _, k in reqs} == {BC.RICH, BC.TILE}


def test_single_requests_bit_for_bit_on_both_routes(crafted):
    import veloci_amd
    from parity import assert_same
    _, idx, _, reqs, wants = crafted
    answered = {}
    for (name, r, kernel), w in zip(reqs, wants):
        idx.profile_json(reset=True)
        assert_same(r, veloci_amd.search(r, idx), w, exact_scores=True)
        answered[name] = scan_kernels(idx)
    elsewhere = {name: sorted(answered[name]) for name, _, kernel in reqs if answered[name] != {kernel}}
    assert not elsewhere, elsewhere  # (both routes occur: test_corpus_reaches_what_it_is_meant_to_reach)


def test_batch_bit_for_bit(crafted):
    import veloci_amd
    import boostcorpus as BC
    from parity import assert_same
    _, idx, _, reqs, wants = crafted
    idx.profile_json(reset=True)
    for (name, r, _), g, w in zip(reqs, veloci_amd.search_batch([r for _, r, _ in reqs], idx), wants):
        assert_same(r, g, w, exact_scores=True)
    assert scan_kernels(idx) == {BC.RICH, BC.TILE}


def test_two_shards_bit_for_bit(crafted):
    """two doc ranges of 65 536 docs: every boost column is cut at the shard's first doc (key_base on the device) and the rich route still applies"""
    import test_gpu_parity as P
    from parity import assert_same
    data, _, _, reqs, wants = crafted
    got = P._search_batch_over_shards(data, [r for _, r, _ in reqs], 2)
    for (name, r, _), g, w in zip(reqs, got, wants):
        assert not isinstance(g, Exception), (name, str(g))
        assert_same(r, g, w, exact_scores=True)


def test_explain_records_character_for_character(crafted):
    """k_explain recomputes every quoted value, the Log10 factor among them: the JSON must equal the oracle's (floats as %.9g of the f32)"""
    import veloci_amd
    import boostcorpus as BC
    from parity import assert_same
    _, idx, ora, _, _ = crafted
    reqs = BC.explain_requests()
    wants = [ora.search_json(json.dumps(r)) for r in reqs]
    for r, w in zip(reqs, wants):
        g = veloci_amd.search(r, idx)
        assert_same(r, g, w, exact_scores=True)
        assert g.explain_json == w.explain_json, json.dumps(r)
        assert len(g.explain) == len(g.ids) > 0 and sum(1 for rec in g.explain if rec and any("Boost" in e for e in rec)) > len(g.ids) // 4, json.dumps(r)
    for r, g, w in zip(reqs, veloci_amd.search_batch(reqs, idx), wants):
        assert_same(r, g, w, exact_scores=True)
        assert g.explain_json == w.explain_json, json.dumps(r)
    ora.set_boost_log("libm")  # the records are what the log mode is about: under libm some factor differs
    try:
        assert any(ora.search_json(json.dumps(r)).explain_json != w.explain_json for r, w in zip(reqs, wants))
    finally:
        ora.set_boost_log("f64")


def test_1n_boost_op_bit_for_bit(crafted):
    """the 1:n boost (OP_BOOST1N: the leaf's hits joined to the values of items[].rank) under both logarithms: alone, in a batch, over two shards"""
    import veloci_amd
    import boostcorpus as BC
    import test_gpu_parity as P
    from parity import assert_same
    data, idx, ora, _, _ = crafted
    reqs = BC.one_to_n_requests()
    wants = [ora.search_json(json.dumps(r)) for r in reqs]
    assert all(w.num_hits > 0 and not np.isnan(w.scores).any() for w in wants)
    unboosted = ora.search_json(json.dumps({k: v for k, v in reqs[0].items() if k != "boost"}))
    assert unboosted.ids.tolist() != wants[0].ids.tolist() or not np.array_equal(unboosted.scores, wants[0].scores)  # (the boost does apply)
    idx.profile_json(reset=True)
    for r, w in zip(reqs, wants):
        assert_same(r, veloci_amd.search(r, idx), w, exact_scores=True)
    assert scan_kernels(idx) == {BC.TILE}  # (the op lives in the interpreter of k_tile_scan)
    for r, g, w in zip(reqs, veloci_amd.search_batch(reqs, idx), wants):
        assert_same(r, g, w, exact_scores=True)
    for r, g, w in zip(reqs, P._search_batch_over_shards(data, reqs, 2), wants):
        assert not isinstance(g, Exception), (str(g), json.dumps(r))
        assert_same(r, g, w, exact_scores=True)


def test_benchmark_shape_bit_for_bit():
    """synth.req_and_of_ors, the third shape of the benchmark mix (AND of ORs, a Log10 `pop` boost, a phrase pair, text locality), on the
    synthetic corpus of the parity tests"""
    import veloci_amd
    from veloci_amd import synth
    from oracle import binding as O
    from parity import assert_same
    spec = synth.SynthSpec(num_docs=300_000, num_terms=5000, triples=2, extra_probe_dfs=(1000, 30_000, 300_000), background_terms=40)
    data, meta = synth.generate(spec)
    idx = veloci_amd.Index(data, device=0)
    ora = data.load_into(O.OracleIndex(data.num_anchors))
    ora.set_boost_log("f64")
    (a, b, c), (d, e, f) = meta.triples[0], meta.triples[1]
    reqs = [synth.req_and_of_ors([a, b], [c, d]), synth.req_and_of_ors([a, d], [b, e], top=1000), synth.req_and_of_ors([c, f], [e, b], top=100)]
    wants = [ora.search_json(json.dumps(r)) for r in reqs]
    assert all(w.num_hits > 0 for w in wants)
    for r, w in zip(reqs, wants):
        assert_same(r, veloci_amd.search(r, idx), w, exact_scores=True)
    for r, g, w in zip(reqs, veloci_amd.search_batch(reqs, idx), wants):
        assert_same(r, g, w, exact_scores=True)
