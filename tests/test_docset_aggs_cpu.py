"""Numeric aggregations of a doc set (vq_docset_aggregate, DocSet.aggregate / stats / histogram) without a GPU: the assertion that the shared cases
are not vacuous, the whole host path over the stubbed device layer against the yardstick (tests/native/docset_aggs_driver.py,
tests/docsetaggcases.py), the same host code and the rounding of the exact sum under ASan + UBSan as a program of its own
(tests/native/docset_aggs_check.cpp), the compiler's resource report of docset_aggs.hip, and the places that must name the new entry point."""
import json
import os
import subprocess
import sys

import pytest

import docsetaggcases as AC
import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_the_cases_reach_every_image_kind_an_inexact_sum_missing_nan_and_a_full_histogram():
    seen = AC.assert_not_vacuous()
    print(seen)
    assert set(seen["kinds"]) == {"plain", "tiled", "dense", "empty"} and seen["inexact"] and seen["missing"] and seen["nan"] and seen["full-histograms"]
    header = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "constexpr uint32_t kAggMaxEdges = %d;" % AC.MAX_EDGES in header


def test_aggregations_on_the_stubbed_device_equal_the_yardstick():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    env.pop("VQ_NO_AGG_PREREDUCE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_aggs_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_AGGS_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_AGGS_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats["cases"] == len(AC.cases()) and stats["one_to_n"] > 20, stats
    # per call and rank one sum of the whole state, then four rounds of 512 digit slots per aggregation
    assert stats["hook_calls"] == 5 * (len(AC.SHARD_SETS) - 1) and stats["hook_sizes"][-1] == 512 * len(AC.SHARD_SPECS) and len(stats["hook_sizes"]) == 2, stats


def test_aggregations_and_the_rounding_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_aggs.cpp") for s in stubs) and "docset_aggs.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_aggs_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_AGGS_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_AGGS_CHECK_OK ", 1)[1])
    print(stats)
    # seven sets of five aggregations on the whole index and on each of two shards; five hook calls per call and rank but for the empty set
    assert stats["rounding"] >= 15 and stats["aggs"] == 3 * 7 * 5 and stats["hook_calls"] == 2 * 5 * 6, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_the_aggregation_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_aggs.hip", tmp_path).items() if "k_docset_agg" in k}
    print(rows)
    assert len(rows) == 4 and sum("k_docset_agg_ids" in k for k in rows) == 2 and sum("k_docset_agg_values" in k for k in rows) == 2, sorted(rows)
    for k, v in rows.items():  # the line the other doc-set kernels are held to
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (k, v)
        # edge keys and bucket histogram (1024 u32 each), 18 u64 limbs, 8 u32 counters and keys: DESIGN.md
        assert v["LDS Size [bytes/block]"] == 2 * 4 * (AC.MAX_EDGES + 1) + 18 * 8 + 8 * 4, (k, v)


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "vq_docset_aggregate" in text, rel
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "veloci_amd/csrc/capi.cpp"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in ("vq_docset_aggs_len", "vq_docset_aggs_get", "vq_docset_aggs_free", "vq_debug_docset_aggregate_ms"):
            assert name in text, (rel, name)
    py = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for name in ("def aggregate(self, specs)", "def stats(self, field)", "def histogram(self, field, edges)"):
        assert name in py, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =", 1)[1].split("\n", 1)[0].split()
    assert "docset_aggs.hip" in srcs and "docset_aggs.cpp" in srcs and "docset_aggs.cpp" in mk.split("HOST_SRCS =", 1)[1].split("\n", 1)[0].split()
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    for name in ("launch_docset_agg_ids", "launch_docset_agg_values", "kAggMaxEdges"):
        assert name in kernels, name
    # the column resolution is shared with from_ranges, not copied
    ranges, aggs = open(os.path.join(CSRC, "docset_ranges.cpp")).read(), open(os.path.join(CSRC, "docset_aggs.cpp")).read()
    assert ranges.count("resolve_range_column(") == 2 and "resolve_range_column(" in aggs and "BOOST_VALID_TO_VALUE" not in aggs
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("k_docset_agg_ids", "k_docset_agg_values", "kAggMaxEdges", "VQ_NO_AGG_PREREDUCE", "docset_aggs.hip", "agg_limbs_to_double"):
        assert name in design, name
    knobs = design.split("8a", 1)[1] if "8a" in design else ""
    assert "VQ_NO_AGG_PREREDUCE" in knobs
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ds.stats(" in readme and "ds.histogram(" in readme
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "DocSet.aggregate" in integration and "digit" in integration
