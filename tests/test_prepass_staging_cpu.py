"""The staging helpers of the pre-pass runners (veloci_amd/csrc/staging.hpp) without a GPU, under ASan + UBSan as a program of its own
(tests/native/staging_check.cpp) over the stubbed device layer: the typed arena (every section on a 256-byte boundary, none overlapping, the
committed size, round trips and their sub-ranges, zero inside its own section, no copy for an empty section, no section after commit), the row
cutter of the gather stage against a plain loop, the padded list length; and where the runners must not lay a buffer out by hand any more."""
import json
import os
import re

import sanitized

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_staging_helpers_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert "prepass.cpp" in host_srcs and "exec.cpp" in host_srcs and any(s.endswith("hip_stub.cpp") for s in stubs)
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "staging_check", host_srcs, stubs))
    assert r.returncode == 0 and "STAGING_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("STAGING_CHECK_OK ", 1)[1])
    # 4 orders x 4 rotations of the element sizes (1, 4, 8, 24 bytes), 5 sections (0, 1, 255, 256, 257 elements) each; 19 pieces of the rows cut
    assert stats == {"arenas": 16, "sections": 80, "row_pieces": 19}, stats


def test_runners_lay_no_buffer_out_by_hand():
    """prepass.cpp and the two runners that stayed in exec.cpp: no `al` lambda, no cast of a meta buffer plus an offset, no restated padding rule"""
    prepass = open(os.path.join(CSRC, "prepass.cpp")).read()
    exec_cpp = open(os.path.join(CSRC, "exec.cpp")).read()
    stayed = "".join(re.search(r"^(?:static )?void %s\(.*?^}$" % fn, exec_cpp, re.M | re.S).group(0) for fn in ("run_count_queries", "run_text_rank"))
    assert "StageArena" in stayed and "auto al = " not in prepass + stayed and not re.search(r"align_up\([^;]*, 256\)", prepass + stayed)
    assert not re.search(r"reinterpret_cast<[^>]*>\(\w+ \+ ", prepass + stayed)
    for name, text in (("prepass.cpp", prepass), ("exec.cpp", exec_cpp), ("compile.cpp", open(os.path.join(CSRC, "compile.cpp")).read()),
                       ("term_lookup.cpp", open(os.path.join(CSRC, "term_lookup.cpp")).read()),  # (these two were part of compile.cpp)
                       ("text_requests.cpp", open(os.path.join(CSRC, "text_requests.cpp")).read()), ("capi.cpp", open(os.path.join(CSRC, "capi.cpp")).read()),
                       ("capi_debug.cpp", open(os.path.join(CSRC, "capi_debug.cpp")).read()), ("shard_step.cpp", open(os.path.join(CSRC, "shard_step.cpp")).read())):  # (part of capi.cpp)
        assert "+ 8 + 3) / 4 * 4" not in text, name
    for fn in ("run_fuzzy_probes", "run_union_jobs", "run_range_jobs", "run_locality_jobs", "run_boost1n_jobs"):
        assert re.search(r"^void %s\(" % fn, prepass, re.M) and not re.search(r"^void %s\(" % fn, exec_cpp, re.M), fn
