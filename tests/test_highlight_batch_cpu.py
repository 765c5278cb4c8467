"""The batched highlight (vq_highlight_batch) without a GPU: the host side over the stubbed device layer (tests/native/highlight_batch_driver.py),
the same under ASan + UBSan as a program of its own (tests/native/highlight_batch_check.cpp), the compiler's resource report of text_rank.hip,
and the places that must name the new entry points."""
import json
import os
import re
import subprocess
import sys

import pytest

import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def run_driver(extra_env):
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4", **extra_env)
    if "VQ_NO_HIGHLIGHT_RANK" not in extra_env:
        env.pop("VQ_NO_HIGHLIGHT_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "highlight_batch_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "HIGHLIGHT_BATCH_DRIVER_OK " in r.stdout, tail
    return json.loads(r.stdout.split("HIGHLIGHT_BATCH_DRIVER_OK ", 1)[1])


def test_batch_on_the_stubbed_device_equals_the_single_parts_and_the_oracle():
    stats = run_driver({})
    print(stats)
    assert stats["parts"] >= 50 and stats["failed"] >= 7 and stats["entries"] > 1500, stats
    assert stats["device_parts"] >= 60, stats  # (the batch runs twice: once collecting errors, once raising)
    # the frequent-token prefix with top 10: more than 300 texts hold a matched token, ten snippets are built
    assert stats["frequent_matched"] > 300 and stats["frequent_device_parts"] == 1 and stats["frequent_snippets"] <= 10, stats
    host = run_driver({"VQ_NO_HIGHLIGHT_RANK": "1"})  # the knob: the same answers (the driver checks them), every part on the host route
    assert host["no_rank"] and host["device_parts"] == 0 and host["entries"] == stats["entries"] and host["frequent_snippets"] == host["frequent_matched"], (host, stats)


def test_highlight_batch_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_text_rank.cpp") for s in stubs) and "exec.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "highlight_batch_check", host_srcs, stubs))
    assert r.returncode == 0 and "HIGHLIGHT_BATCH_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("HIGHLIGHT_BATCH_CHECK_OK ", 1)[1])
    print(stats)
    assert stats["good"] == 24 and stats["failing"] == 10 and stats["device_parts"] >= 12, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_text_rank_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("text_rank.hip", tmp_path).items() if re.search(r"k_text_best|k_text_select", k)}
    print(rows)
    assert len(rows) == 2 and sum(1 for k in rows if "k_text_best" in k) == 1, sorted(rows)
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
    v = next(v for k, v in rows.items() if "k_text_select" in k)
    assert v["VGPRs"] <= 128, v  # 1024 threads per workgroup: 16 waves on one CU, four per SIMD


def test_every_layer_names_the_entry_points():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in ("vq_highlight_batch", "vq_index_highlight_rank_counts", "vq_debug_text_rank"):
            assert name in text, (rel, name)
    assert "def highlight_batch(parts, index, raise_on_error=True)" in open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    assert "VQ_NO_HIGHLIGHT_RANK" in open(os.path.join(ROOT, "DESIGN.md")).read()
