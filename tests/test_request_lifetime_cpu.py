"""Who keeps a request alive, without a GPU: a partial batch or a step that a caller holds shares its requests with their handles, so the handles
may be freed — or given another doc set — as soon as the call that took them has returned (include/veloci_amd.h).  Steps with deep requests,
partial batches and a doc set changed mid-step, each against the same run with the handles freed at the end, under ASan + UBSan as a program of
its own (tests/native/request_lifetime_check.cpp) over the stubbed device layer."""
import json
import os

import sanitized

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_handles_freed_while_batches_and_steps_are_alive_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert "capi.cpp" in host_srcs and "shard_step.cpp" in host_srcs and "exec.cpp" in host_srcs and stubs
    env = {k: v for k, v in os.environ.items() if k not in ("VQ_STUB_LAUNCH_LOG", "VQ_SHARD_CHUNKS")}
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "request_lifetime_check", host_srcs, stubs), env=env)
    assert r.returncode == 0 and "REQUEST_LIFETIME_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("REQUEST_LIFETIME_CHECK_OK ", 1)[1])
    # per run two steps, one partial batch and the step whose doc set changes, and after the early frees one more step with the new set;
    # freed early: the 6 + 3 request handles of the steps and the partial batch, the first doc set's handle
    assert stats == {"steps": 7, "partial_batches": 2, "handles_freed_early": 10}, stats


def test_the_header_states_the_rule():
    header = open(os.path.join(ROOT, "include", "veloci_amd.h")).read()
    assert header.count("as soon as the call returns") >= 3
    assert "as soon as the call returns" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
