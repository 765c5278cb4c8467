"""The dense union route (veloci_amd/csrc/union_dense.hip, run_union_jobs in prepass.cpp) without a GPU: the compiler's resource report of its
kernels, and the host side of wide leaves over the stubbed device layer, plain and under ASan + UBSan (tests/native/union_dense_driver.py)."""
import json
import os
import subprocess
import sys

import pytest

import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
DRIVER = os.path.join(HERE, "native", "union_dense_driver.py")
STUB_ENV = {"VQ_STUB_NOOP_LAUNCH": "1", "VQ_STUB_DICT_SCAN": "1", "VQ_UNION_DENSE_SLAB_MB": "0", "VQ_HOST_THREADS": "4"}


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_dense_union_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("union_dense.hip", tmp_path).items() if "k_union_dense" in k}
    print(rows)
    assert len(rows) == 4, sorted(rows)  # scatter, count, offsets, write
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)  # streaming kernels: nothing here may cost waves


def _run_driver(so, extra_env):
    env = dict(os.environ, VQ_LIB=so, **STUB_ENV, **extra_env)
    r = subprocess.run([sys.executable, DRIVER], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "UNION_DENSE_DRIVER_OK" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    stats = json.loads(r.stdout.split("UNION_DENSE_DRIVER_OK ", 1)[1])
    # 5 requests and their batch unsharded, 3 requests on each of two shards.  One slab group per job (budget 0 MB), so one launch per job:
    # 1 + 1 + 1 + 2 + 2 for the single requests, 4 for the batch (zq, z, z boosted, zq boosted), 3 per shard
    assert stats["searched"] == 11 and stats["batches"] == 1 and stats["dense_launches"] == 7 + 4 + 3 + 3, stats
    return stats


def test_wide_leaves_through_the_host_side_on_the_stubbed_device():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _run_driver(os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), {})


def test_wide_leaves_through_the_host_side_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    libstdcxx = subprocess.run(["g++", "-print-file-name=libstdc++.so.6"], capture_output=True, text=True).stdout.strip()
    assert os.path.sep in libasan
    _run_driver(os.path.join(ROOT, "veloci_amd", "_host_asan", "libveloci_host_asan.so"),
                {"LD_PRELOAD": libasan + " " + libstdcxx, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
