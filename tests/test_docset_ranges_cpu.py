"""Doc sets from numeric ranges (vq_docset_from_ranges, DocSet.from_ranges) without a GPU: the whole host path over the stubbed device layer against
numpy (tests/native/docset_ranges_driver.py, tests/docsetrangecases.py), the same host code under ASan + UBSan as a program of its own
(tests/native/docset_ranges_check.cpp), the compiler's resource report of docset_ranges.hip, the places that must name the new entry point, and
the assertion that the shared cases are not vacuous."""
import json
import os
import subprocess
import sys

import pytest

import docsetrangecases as RC
import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_the_cases_reach_every_image_kind_both_routes_and_the_edges():
    seen = RC.assert_not_vacuous()
    print(seen)
    assert seen["routes"] == [0, 1] and all(set(k) == {"plain", "tiled", "dense", "empty"} for k in seen["kinds"].values())
    header = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "constexpr uint32_t kRangeClauseTable = %d;" % RC.CLAUSE_TABLE in header  # the pass length the 9- and 17-clause cases straddle is the builder's


def test_ranges_on_the_stubbed_device_equal_numpy():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    env.pop("VQ_NO_RANGE_PROBE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_ranges_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_RANGES_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_RANGES_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats["cases"] == 2 * len(RC.cases()) and stats["probe"] >= 40 and stats["hook_calls"] > len(RC.cases()), stats


def test_ranges_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_ranges.cpp") for s in stubs) and "docset_ranges.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_ranges_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_RANGES_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_RANGES_CHECK_OK ", 1)[1])
    print(stats)
    # per index every list under no `within`, a dense one, a short one and the empty one; the lists without a 1:n clause take the probe route under the
    # last two and run once more on the stream route
    lists, with_1n = stats["lists"], 5
    assert lists == 41 and stats["probe"] == 2 * 2 * (lists - with_1n) and stats["sets"] == 2 * 4 * lists + stats["probe"], stats
    assert stats["hook_calls"] == stats["sets"] // 2 and stats["ids"] > 1_000_000, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_the_range_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_ranges.hip", tmp_path).items() if "k_range" in k}
    print(rows)
    assert len(rows) == 3 and all(any(name in k for k in rows) for name in ("k_range_bits", "k_range_probe", "k_range_scatter")), sorted(rows)
    for k, v in rows.items():  # the line the other doc-set kernels are held to
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "vq_docset_from_ranges" in text, rel
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "veloci_amd/csrc/capi.cpp"):
        assert "vq_debug_docset_range_route" in open(os.path.join(ROOT, rel)).read(), rel
    py = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for name in ("def from_ranges(cls, index, ranges, within=None)", "def from_range(cls, index, field, gte=None, gt=None, lte=None, lt=None, missing=False, within=None)"):
        assert name in py, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =", 1)[1].split("\n", 1)[0].split()
    assert "docset_ranges.hip" in srcs and "docset_ranges.cpp" in srcs and "docset_ranges.cpp" in mk.split("HOST_SRCS =", 1)[1].split("\n", 1)[0].split()
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    for name in ("launch_range_bits", "launch_range_probe", "launch_range_scatter"):
        assert name in kernels, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("k_range_bits", "k_range_probe", "k_range_scatter", "kRangeClauseTable", "VQ_NO_RANGE_PROBE", "docset_ranges.hip"):
        assert name in design, name
    knobs = design.split("8a", 1)[1] if "8a" in design else ""
    assert "VQ_NO_RANGE_PROBE" in knobs
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "DocSet.from_range" in readme
    assert "DocSet.from_ranges" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
