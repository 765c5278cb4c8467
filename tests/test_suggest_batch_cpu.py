"""The batched suggest (vq_suggest_batch) without a GPU: the host side over the stubbed device layer (tests/native/suggest_batch_driver.py), the
same under ASan + UBSan as a program of its own (tests/native/suggest_batch_check.cpp), the compiler's resource report of dict_topn.hip, and
the places that must name the new entry point."""
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
    if "VQ_NO_SUGGEST_TOPN" not in extra_env:
        env.pop("VQ_NO_SUGGEST_TOPN", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "suggest_batch_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "SUGGEST_BATCH_DRIVER_OK " in r.stdout, tail
    return json.loads(r.stdout.split("SUGGEST_BATCH_DRIVER_OK ", 1)[1])


def test_batch_on_the_stubbed_device_equals_the_single_requests_and_the_oracle():
    stats = run_driver({})
    print(stats)
    assert stats["requests"] >= 90 and stats["failed"] == 5 and stats["entries"] > 2000, stats
    # 7 prefixes x (top 1, 10, 10+3, 200, 1848, 0+4) + the multi-part requests' parts; the 2500-match prefix with top 10 brings back the loop's
    # buffer (at most top + 200 entries), not its matches
    assert stats["topn_probes"] >= 42 and stats["records_w_top10"] <= 210, stats
    full = run_driver({"VQ_NO_SUGGEST_TOPN": "1"})  # the knob: the same answers (the driver checks them), every part on the full route
    assert full["no_topn"] and full["topn_probes"] == 0 and full["entries"] == stats["entries"] and full["records_w_top10"] == 2500, (full, stats)


def test_suggest_batch_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_dict_topn.cpp") for s in stubs) and "exec.cpp" in host_srcs and "prepass.cpp" in host_srcs
    env = dict(os.environ)
    env.pop("VQ_NO_SUGGEST_TOPN", None)
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "suggest_batch_check", host_srcs, stubs), env=env)
    assert r.returncode == 0 and "SUGGEST_BATCH_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("SUGGEST_BATCH_CHECK_OK ", 1)[1])
    print(stats)
    assert stats["good"] == 18 and stats["failing"] == 8 and stats["topn_probes"] >= 8, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_topn_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("dict_topn.hip", tmp_path).items() if re.search(r"k_dict_topn|k_topn_", k)}
    print(rows)
    assert len(rows) == 4 and sum(1 for k in rows if "k_dict_topn" in k) == 1, sorted(rows)
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
    v = next(v for k, v in rows.items() if "k_dict_topn" in k)
    assert v["LDS Size [bytes/block]"] == 0 and v["VGPRs"] <= 64, v  # the buffer is dynamic LDS (16 KiB at most); one wave per block


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in ("vq_suggest_batch", "vq_index_suggest_topn_probes", "vq_debug_dict_topn"):
            assert name in text, (rel, name)
    assert "def suggest_batch(requests, index, raise_on_error=True)" in open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    assert "VQ_NO_SUGGEST_TOPN" in open(os.path.join(ROOT, "DESIGN.md")).read()
