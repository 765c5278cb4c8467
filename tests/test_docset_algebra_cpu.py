"""Doc set algebra (vq_docset_combine, vq_docset_ids, vq_debug_docset_route) without a GPU: the whole host path over the stubbed device layer against
numpy (tests/native/docset_algebra_driver.py, tests/docsetalgebracases.py), the same host code under ASan + UBSan as a program of its own
(tests/native/docset_algebra_check.cpp), the compiler's resource report of docset_algebra.hip, the places that must name the new entry points,
and the assertion that the shared cases are not vacuous."""
import json
import os
import subprocess
import sys

import pytest

import docsetalgebracases as AC
import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
ENTRY_POINTS = ("vq_docset_combine", "vq_docset_ids", "vq_debug_docset_route")


def test_the_cases_cover_every_image_kind_and_both_routes():
    seen = AC.assert_not_vacuous()
    print(seen)
    assert len(seen) == 6


def test_combined_sets_on_the_stubbed_device_equal_numpy():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    env.pop("VQ_NO_SETOP_PROBE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_algebra_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_ALGEBRA_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_ALGEBRA_DRIVER_OK ", 1)[1])
    print(stats)
    n = len(AC.image_cases())
    assert stats["cases"] == 2 * n and stats["probe"] + stats["word"] == 2 * n and stats["forced"] == stats["probe"] > 100 and stats["word"] > 100, stats


def test_combined_sets_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_algebra.cpp") for s in stubs) and "docset_algebra.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_algebra_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_ALGEBRA_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_ALGEBRA_CHECK_OK ", 1)[1])
    print(stats)
    assert stats == {"sets": 74, "probe": 18, "word": 38}, stats  # per index 9 probe-route cases (each once more through the word route) and 19 word-route cases


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_setop_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_algebra.hip", tmp_path).items() if "k_setop_" in k}
    print(rows)
    assert len(rows) == 3 and all(any(name in k for k in rows) for name in ("k_setop_words", "k_setop_probe", "k_setop_clear")), sorted(rows)
    for k, v in rows.items():  # the line docset.hip's kernels are held to
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (k, v)


def test_every_layer_names_the_entry_points():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in ENTRY_POINTS:
            assert name in text, (rel, name)
    header = open(os.path.join(ROOT, "include", "veloci_amd.h")).read()
    assert "enum { VQ_DOCSET_AND = 0, VQ_DOCSET_OR = 1, VQ_DOCSET_MINUS = 2, VQ_DOCSET_NOT = 3 };" in header
    py = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for name in ("def combine(cls, index, op, sets)", "def all_of(cls, index, sets)", "def any_of(cls, index, sets)", "def minus(self, *others)", "def ids_tensor(self)",
                 "def __and__", "def __or__", "def __sub__", "def __invert__", "def route(self)"):
        assert name in py, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =", 1)[1].split("\n", 1)[0].split()
    assert "docset_algebra.hip" in srcs and "docset_algebra.cpp" in srcs and "docset_algebra.cpp" in mk.split("HOST_SRCS =", 1)[1].split("\n", 1)[0].split()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("k_setop_words", "k_setop_probe", "VQ_NO_SETOP_PROBE", "vq_docset_combine"):
        assert name in design, name
    assert "DocSet.combine" in open(os.path.join(ROOT, "README.md")).read()
