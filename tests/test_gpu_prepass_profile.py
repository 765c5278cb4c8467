"""The device work of the pre-pass runners, not only their results: one call per vq_debug_* entry point on the corpora of test_gpu_prepass_lists.py
(union on the two-level and on the dense route, text locality over two tables, range hits with both paths, 1:n boost lists), and after each the
profile's `launches`, `layout_bytes`, `algorithmic_bytes` and `queries` of every kernel against tests/golden/prepass_profile.json.  That file was
recorded on an MI355X by tools/record_prepass_profile.py from the commit BEFORE the runners moved to prepass.cpp and onto the staging arena, through
the same calls (prepass_profile_calls.profile_calls).  All four fields are integers computed on the host: the comparison is exact."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def test_prepass_runners_launch_and_book_what_they_did_before_the_staging_arena(golden_dir):
    from prepass_profile_calls import profile_calls
    with open(os.path.join(golden_dir, "prepass_profile.json")) as f:
        want = json.load(f)
    got = profile_calls()
    assert sorted(got) == sorted(want)
    for call in sorted(want):
        assert sorted(got[call]) == sorted(want[call]), (call, sorted(got[call]), sorted(want[call]))
        for kernel, fields in want[call].items():
            assert got[call][kernel] == fields, (call, kernel, got[call][kernel], fields)
    # the calls reach what they are meant to pin
    assert want["union_two_levels"]["k_union<count>"]["launches"] == 2 and "k_union_dense_write" in want["union_dense"]
    assert "k_locality" in want["locality_two_tables"] and "k_boost1n" in want["boost1n"] and "k_range_hits" in want["range_hits_both_paths"]
