"""vq_debug_node_counts (the count pre-pass alone, tests/test_gpu_count_prepass.py) without a GPU: its argument handling, the batch's compilation
passes in front of the count pre-pass, the packing of the count queries and the copy-out under ASan + UBSan as a program of its own
(tests/native/count_debug_check.cpp) over the stubbed device layer, and the places that must name the entry point."""
import json
import os
import re

import sanitized

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "vq_debug_node_counts"


def test_count_debug_entry_point_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert "exec.cpp" in host_srcs and "capi.cpp" in host_srcs and stubs
    env = {k: v for k, v in os.environ.items() if k not in ("VQ_STUB_LAUNCH_LOG",)}
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "count_debug_check", host_srcs, stubs), env=env)
    assert r.returncode == 0 and "COUNT_DEBUG_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("COUNT_DEBUG_CHECK_OK ", 1)[1])
    assert stats == {"ok": 9, "refused": 10}, stats


def test_every_layer_names_the_entry_point():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "veloci_amd/search.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, rel)).read(), rel
    # the entry point runs the batch's own passes: one definition of the count query's launch, reached from the batch and from the entry point
    exec_cpp = open(os.path.join(ROOT, "veloci_amd", "csrc", "exec.cpp")).read()
    assert len(re.findall(r"\brun_count_queries\(", exec_cpp)) == 2 and len(re.findall(r"\bmeasure_counts\(", exec_cpp)) == 3
    assert len(re.findall(r"\bcompile_before_counts\(", exec_cpp)) == 3
