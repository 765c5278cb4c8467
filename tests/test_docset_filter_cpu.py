"""Doc sets from a filter (vq_docset_from_filter) without a GPU: the whole host path over the stubbed device layer against the numpy restatements
(tests/native/docset_filter_driver.py, tests/docsetfiltercases.py), the same host code under ASan + UBSan as a program of its own
(tests/native/docset_filter_check.cpp), the compiler's resource report of docset_filter.hip, and the places that must name the new entry point."""
import json
import os
import subprocess
import sys

import pytest

import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_sets_from_filters_on_the_stubbed_device_equal_the_restatement():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_filter_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_FILTER_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_FILTER_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats == {"sets": 34, "within": 6}, stats  # 12 exact-term leaves + 5 trees, 3 sets to search within: on the whole index and on the shard


def test_sets_from_filters_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_filter.cpp") for s in stubs) and "docset.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_filter_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_FILTER_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_FILTER_CHECK_OK ", 1)[1])
    assert stats == {"sets": 45, "orders": 12}, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_filter_kernel_compiles_for_gfx950_at_four_waves_per_simd(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_filter.hip", tmp_path).items() if "k_filter_bits" in k}
    print(rows)
    assert len(rows) == 1, sorted(rows)
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 128, (k, v)


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp"):
        assert "vq_docset_from_filter" in open(os.path.join(ROOT, rel)).read(), rel
    assert "def from_filter(cls, index, filter, within=None)" in open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "docset_filter.hip" in mk.split("SRCS =", 1)[1].split("\n", 1)[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_filter_bits" in design and "from_filter" in open(os.path.join(ROOT, "README.md")).read()
