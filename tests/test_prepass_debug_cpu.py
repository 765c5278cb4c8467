"""The vq_debug_*_lists entry points (the pre-pass drivers alone, tests/test_gpu_prepass_lists.py) without a GPU: their argument handling, the host
side of the four drivers and the copy of the lists under ASan + UBSan as a program of its own (tests/native/prepass_debug_check.cpp) over the
stubbed device layer, and the places that must name the new entry points."""
import json
import os

import sanitized

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
NAMES = ("vq_debug_union_lists", "vq_debug_locality_lists", "vq_debug_range_hits", "vq_debug_boost1n_lists")


def test_prepass_debug_entry_points_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert "prepass.cpp" in host_srcs and "capi.cpp" in host_srcs and "capi_debug.cpp" in host_srcs and stubs
    env = {k: v for k, v in os.environ.items() if k not in ("VQ_UNION_DENSE_MIN", "VQ_STUB_LAUNCH_LOG")}
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "prepass_debug_check", host_srcs, stubs), env=env)
    assert r.returncode == 0 and "PREPASS_DEBUG_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("PREPASS_DEBUG_CHECK_OK ", 1)[1])
    assert stats == {"ok": 7, "refused": 18}, stats


def test_every_layer_names_the_entry_points():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi_debug.cpp", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in NAMES:
            assert name in text, (rel, name)
