"""Doc sets (vq_docset_*) without a GPU: the creation path over the stubbed device layer against the numpy restatement
(tests/native/docset_driver.py, tests/docsetref.py), the same host code under ASan + UBSan as a program of its own (tests/native/docset_check.cpp),
the compiler's resource report of docset.hip, and the places that must name the new entry points."""
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
NAMES = ("vq_docset_create", "vq_docset_len", "vq_docset_local_len", "vq_docset_device_bytes", "vq_debug_docset_part", "vq_docset_free", "vq_request_set_docset")


def test_creation_path_on_the_stubbed_device_equals_the_restatement():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats["sets"] == 18 and stats["dense"] >= 5 and stats["tiled"] > stats["dense"] and stats["compiled"] == 2, stats


def test_doc_sets_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset.cpp") for s in stubs) and "docset.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_CHECK_OK ", 1)[1])
    assert stats == {"sets": 10, "compiled": 2}, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_docset_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset.hip", tmp_path).items() if "k_docset_" in k}
    print(rows)
    assert len(rows) == 7, sorted(rows)
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] <= 64, (k, v)


def test_every_layer_names_the_entry_points():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in NAMES:
            assert name in text, (rel, name)
    search = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for text in ("class DocSet:", "def search(request, index, docset=None)", "def search_batch(requests, index, raise_on_error=True, docsets=None)",
                 "def search_batch_flat(batch, index, stride=10, docsets=None)", "def set_docset(self, docset)"):
        assert text in search, text
    assert "def search_shards_local(shards, requests, docsets=None)" in open(os.path.join(ROOT, "veloci_amd", "dist.py")).read()
    assert "docset.hip" in open(os.path.join(CSRC, "Makefile")).read() and "k_docset_mark" in open(os.path.join(ROOT, "DESIGN.md")).read()
