"""The plain restatement of the two merges (mergeref.py) and the crafted cases (mergecases.py) without a GPU: every builder's property asserts
hold, the restatement equals a brute-force Python sort, the order_f32 / unorder_f32 restatements round-trip, and vq_debug_merge_spans /
vq_debug_finalize refuse bad arguments (-2) before they touch a device."""
import os
import struct

import numpy as np
import pytest

import mergecases as M
from mergeref import finalize_ref, make_key, merge_ref, order_f32, unorder_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(M.MERGE_CASES))
def test_merge_builders_hold_their_properties(name):
    calls = M.MERGE_CASES[name]()
    assert calls
    for jobs in calls:
        assert jobs
        for table, top_k in jobs:
            M.check_table(table, top_k)
            assert table.size <= 1 << 17  # a call moves well under a megabyte


@pytest.mark.parametrize("name", sorted(M.FINALIZE_CASES))
def test_finalize_builders_hold_their_properties(name):
    calls = M.FINALIZE_CASES[name]()
    assert calls
    for c in calls:
        assert sum(c["top_k"]) * len(c["keys"]) <= 1 << 17
        M.finalize_call(c["top_k"], c["keys"], c["hits"], c["stride_pad"])  # (its asserts: sorted lists, unique keys per job)
    jobs, top_k, raw = M.chained_case()
    assert len(jobs) == 16 and [k for _, k in jobs[:2]] == top_k and len(raw) == 2


def test_every_row_of_the_issue_tables_is_a_case():
    assert sorted(M.MERGE_CASES) == sorted(["bound_ordinary", "bound_top_k_1", "rounds_by_size", "rounds_by_top_k", "few_hits_per_span", "one_subset_hoards_the_small_keys",
                                            "edge_of_the_buffer", "short_and_empty", "equal_scores", "key_domain", "mixed_launch"])
    assert sorted(M.FINALIZE_CASES) == sorted(["no_mid_loop_prune", "mid_loop_prune", "winners_in_the_last_shard_only", "short_shards", "hits", "key_domain_and_equal_scores",
                                               "stride", "mixed_launch"])
    shapes = lambda calls: sorted((len(c["keys"]), c["top_k"][0]) for c in calls)  # noqa: E731
    assert shapes(M.finalize_no_mid_loop_prune()) == [(1, 1), (1, 10), (1, 1024), (2, 1), (2, 10), (2, 1024)]
    assert shapes(M.finalize_mid_loop_prune()) == [(3, 683), (3, 1024), (8, 300), (16, 1024), (64, 64)]
    assert M.finalize_mixed_launch()[0]["top_k"] == [1, 10, 64, 300, 683, 1024] and len(M.finalize_mixed_launch()[0]["keys"]) == 8
    # the constants the route rule is restated with are the kernel's
    dev = open(os.path.join(ROOT, "veloci_amd", "csrc", "device_types.hpp")).read()
    assert "constexpr int kBlock = 64;" in dev and "constexpr int kCandCap = 2048;" in dev and "constexpr int kMaxTopK = 1024;" in dev
    assert (M.K_BLOCK, M.CAND_CAP, M.MAX_TOP_K) == (64, 2048, 1024)


def brute_top_k(keys, top_k):
    best = sorted((int(k) for k in keys if int(k) != 0), reverse=True)[:top_k]
    return best + [0] * (top_k - len(best))


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def brute_unorder(word):
    return word & 0x7FFFFFFF if word & 0x80000000 else ~word & 0xFFFFFFFF


def test_restatement_equals_a_brute_force_sort():
    rng = np.random.default_rng(5)
    tables = [(np.array([[5, 9, 0], [7, 0, 0], [1 << 63, 3, 2]], np.uint64), 4),
              (np.array([[0, 0], [0, 0]], np.uint64), 3),
              (np.concatenate([M.domain_keys(rng, 4), np.zeros(5, np.uint64)]).reshape(-1, 1), 30)]
    for table, top_k in tables:
        for k in (1, top_k, 64):
            want = brute_top_k(table.ravel(), k)
            assert [int(x) for x in merge_ref(table, k)] == want
            shards = [table[i::2].ravel() for i in range(2)]
            ids, bits, n, hits = finalize_ref(shards, [(1 << 63) + 5, (1 << 63) + 6], k)
            real = [x for x in want if x]
            assert n == len(real) and hits == 11  # the u64 sum wraps
            assert [int(x) for x in ids] == [x & 0xFFFFFFFF for x in real] and [int(x) for x in bits] == [brute_unorder(x >> 32) for x in real]
    assert finalize_ref([np.zeros(3, np.uint64)], [1 << 33, 1 << 33, 5][:1], 3)[2:] == (0, 1 << 33)


def test_order_restatements_round_trip_the_special_values():
    specials = [float("-inf"), -3.5, -1e-40, -0.0, 0.0, 1e-45, 1.0, 2.5, float("inf"), -1e-45, 3.4028234663852886e38, -3.4028234663852886e38]
    vals = np.array(specials, np.float32)
    assert np.array_equal(vals[:9].view(np.uint32), M.DOMAIN_SCORES.view(np.uint32))
    bits = vals.view(np.uint32)
    assert [int(b) for b in bits] == [f32_bits(x) for x in specials]
    words = order_f32(bits)
    assert np.array_equal(unorder_f32(words), bits)
    for b, w in zip(bits, words):  # the definition, in Python integers
        b = int(b)
        assert int(w) == ((~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000) and brute_unorder(int(w)) == b
    # the words order like the floats, -0.0 directly below +0.0
    order = np.argsort(words, kind="stable")
    assert np.all(np.diff(vals[order].astype(np.float64)) >= 0) and int(words[3]) + 1 == int(words[4])
    assert np.all(words != 0)  # only the NaN 0xFFFFFFFF maps to the empty slot's high word
    assert int(make_key(np.float32(1.0), 0)) == (0xBF800000 << 32) and int(make_key(np.float32(-0.0), 0xFFFFFFFE)) == (0x7FFFFFFF << 32) | 0xFFFFFFFE


def test_entry_points_refuse_bad_arguments_before_the_device():
    """-2 from the C ABI's own checks: the same on a machine with a GPU, on one without, and over the stubbed device layer"""
    import ctypes as C
    import veloci_amd
    L = veloci_amd.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    keys, out = np.ones(4096, np.uint64), np.zeros(4096, np.uint64)
    u = lambda *v: np.array(v, np.uint32)  # noqa: E731
    merge = lambda sk, ns, tk, nj, o: L.vq_debug_merge_spans(sk, ns, tk, nj, o)  # noqa: E731
    assert merge(None, p(u(1)), p(u(1)), 1, p(out)) == -2
    assert merge(p(keys), None, p(u(1)), 1, p(out)) == -2
    assert merge(p(keys), p(u(1)), None, 1, p(out)) == -2
    assert merge(p(keys), p(u(1)), p(u(1)), 1, None) == -2
    assert merge(p(keys), p(u(1)), p(u(1)), 0, p(out)) == -2
    assert merge(p(keys), p(u(1)), p(u(0)), 1, p(out)) == -2
    assert merge(p(keys), p(u(1)), p(u(1025)), 1, p(out)) == -2
    assert merge(p(keys), p(u(0)), p(u(4)), 1, p(out)) == -2
    assert merge(p(keys), p(u(2, 0)), p(u(4, 4)), 2, p(out)) == -2
    assert merge(p(keys), p(u(16384, 1)), p(u(1024, 1)), 2, p(out)) == -2      # 2^24 + 1 keys
    assert merge(p(keys), p(u(0xFFFFFFFF)), p(u(1024)), 1, p(out)) == -2
    hits, o32, n = np.zeros(8, np.uint64), np.zeros(4096, np.uint32), np.zeros(8, np.uint32)
    fin = lambda sk, sh, s, pad, tk, nj, a, b, c, d: L.vq_debug_finalize(sk, sh, s, pad, tk, nj, a, b, c, d)  # noqa: E731
    good = (p(keys), p(hits), 2, 0, p(u(4)), 1, p(o32), p(o32), p(n), p(hits))
    for at in (0, 1, 4, 6, 7, 8, 9):
        assert fin(*[None if i == at else a for i, a in enumerate(good)]) == -2, at
    for at, bad in ((2, 0), (5, 0), (3, 4), (3, 12), (3, 257), (4, p(u(0))), (4, p(u(1025))), (2, 16385), (2, 0xFFFFFFFF)):
        args = list(good)
        args[at] = bad
        if at == 2 and bad > 2:
            args[4] = p(u(1024))  # 16385 shards of 1024 keys: above 2^24
        assert fin(*args) == -2, (at, bad)
