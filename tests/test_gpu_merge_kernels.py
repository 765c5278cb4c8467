"""k_merge_spans and k_finalize run alone (vq_debug_merge_spans / vq_debug_finalize) on the crafted tables of mergecases.py, element for element
against the plain top-k of mergeref.py.  The keys are integers: every comparison is exact.  Which branch a case reaches (bound route, its
fallback, rounds, finalize's prune inside the shard loop) is asserted by its builder on the CPU."""
import numpy as np
import pytest

import mergecases as M
from mergeref import finalize_ref, merge_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import veloci_amd
    return veloci_amd.lib()


@pytest.mark.parametrize("name", sorted(M.MERGE_CASES))
def test_merge_spans_equals_the_plain_top_k(L, name):
    for c, jobs in enumerate(M.MERGE_CASES[name]()):
        rc, outs = M.call_merge(L, jobs)
        assert rc == 0, (name, c, rc)
        for j, ((table, top_k), got) in enumerate(zip(jobs, outs)):
            want = merge_ref(table, top_k)
            assert np.array_equal(got, want), (name, c, j, top_k, table.shape, M.route(table, top_k), int(np.argmax(got != want)))


def check_finalize(got, shard_lists, shard_hits, top_k, where):
    ids, bits, n, hits = got
    w_ids, w_bits, w_n, w_hits = finalize_ref(shard_lists, shard_hits, top_k)
    assert n == w_n and hits == w_hits, (where, n, w_n, hits, w_hits)
    assert np.array_equal(ids[:n], w_ids) and np.array_equal(bits[:n], w_bits), where  # (entries behind out_n are not compared)


@pytest.mark.parametrize("name", sorted(M.FINALIZE_CASES))
def test_finalize_equals_the_plain_top_k(L, name):
    answers = []
    for c, call in enumerate(M.FINALIZE_CASES[name]()):
        rc, outs = M.call_finalize(L, call)
        assert rc == 0, (name, c, rc)
        for j, top_k in enumerate(call["top_k"]):
            check_finalize(outs[j], [sk[j] for sk in call["keys"]], [sh[j] for sh in call["hits"]], top_k, (name, c, j, top_k, len(call["keys"])))
        answers.append(outs)
    if name == "stride":  # the same partials further apart: the same answer
        (a,), (b,) = answers
        assert a[2:] == b[2:] and np.array_equal(a[0][:a[2]], b[0][:b[2]]) and np.array_equal(a[1][:a[2]], b[1][:b[2]])


def test_merge_output_feeds_finalize(L):
    """8 "shards" x 2 queries: each shard's span tables through k_merge_spans (one launch of 16 jobs), the 8 partial key lists through
    k_finalize, against the plain top-k of the raw span tables"""
    jobs, top_k, raw = M.chained_case()
    rc, parts = M.call_merge(L, jobs)
    assert rc == 0
    keys = [[parts[s * 2 + q] for q in range(2)] for s in range(8)]
    hits = [[int(np.count_nonzero(raw[q][s])) + (1 << 30) * s for q in range(2)] for s in range(8)]
    rc, outs = M.call_finalize(L, M.finalize_call(top_k, keys, hits))  # (finalize_call asserts the merge's lists sorted, zeros behind)
    assert rc == 0
    for q in range(2):
        check_finalize(outs[q], [raw[q][s] for s in range(8)], [h[q] for h in hits], top_k[q], ("chained", q))
