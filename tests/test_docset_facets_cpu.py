"""Facet counts of a doc set (vq_docset_facets, DocSet.facets) without a GPU: the whole host path over the stubbed device layer against numpy
(tests/native/docset_facets_driver.py, tests/docsetfacetcases.py), the same host code under ASan + UBSan as a program of its own
(tests/native/docset_facets_check.cpp), the compiler's resource report of docset_facets.hip, the places that must name the new entry point, and
the assertion that the shared cases are not vacuous."""
import json
import os
import subprocess
import sys

import pytest

import docsetfacetcases as FC
import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_the_cases_reach_both_modes_every_store_kind_and_the_host_ranking():
    seen = FC.assert_not_vacuous()
    print(seen)
    assert seen["modes"] == ["cache", "lds"] and seen["composed"] == ["comp[]"] and seen["empty_sets"] == ["n0"]
    header = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "constexpr uint32_t kDocsetFacetLdsValues = %d;" % FC.LDS_VALUES in header  # the bound the cases straddle is the builder's


def test_facets_on_the_stubbed_device_equal_numpy():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    env.pop("VQ_NO_DOCSET_FACET_LDS", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_facets_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_FACETS_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_FACETS_DRIVER_OK ", 1)[1])
    print(stats)
    sets = len(FC.id_sets()) + 1
    assert stats["pairs"] == 2 * sets * len(FC.HISTOGRAM_FIELDS) and stats["entries"] > 4000 and stats["hook_calls"] > 100, stats


def test_facets_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_facets.cpp") for s in stubs) and "docset_facets.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_facets_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_FACETS_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_FACETS_CHECK_OK ", 1)[1])
    print(stats)
    assert stats["calls"] == 52 and stats["hook_calls"] == 16 and stats["entries"] > 10_000, stats  # per index 4 sets x 3 requests and the empty set, in both modes


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_the_count_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_facets.hip", tmp_path).items() if "k_docset_facet" in k}
    print(rows)
    assert len(rows) == 1 and "k_docset_facet_count" in next(iter(rows)), sorted(rows)
    for k, v in rows.items():  # the line the other doc-set kernels are held to; the LDS is the histogram of the LDS mode
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (k, v)
        assert v["LDS Size [bytes/block]"] == 4 * FC.LDS_VALUES, (k, v)


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp", "DESIGN.md"):
        assert "vq_docset_facets" in open(os.path.join(ROOT, rel)).read(), rel
    py = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for name in ("def facets(self, facets)", "def facet_result(self, facets)"):
        assert name in py, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =", 1)[1].split("\n", 1)[0].split()
    assert "docset_facets.hip" in srcs and "docset_facets.cpp" in srcs and "docset_facets.cpp" in mk.split("HOST_SRCS =", 1)[1].split("\n", 1)[0].split()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("k_docset_facet_count", "kDocsetFacetLdsValues", "VQ_NO_DOCSET_FACET_LDS", "docset_facets.hip"):
        assert name in design, name
    knobs = design.split("8a", 1)[1] if "8a" in design else ""
    assert "VQ_NO_DOCSET_FACET_LDS" in knobs
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "DocSet.facets" in readme or ".facets(" in readme
    compile_cpp = open(os.path.join(CSRC, "compile.cpp")).read()
    assert compile_cpp.count("is not staged as an anchor-keyed CSR") == 1 and compile_cpp.count("resolve_facet(idx, fr)") == 1  # one resolution for both callers
    assert "resolve_facet(idx, fr)" in open(os.path.join(CSRC, "docset_facets.cpp")).read()
