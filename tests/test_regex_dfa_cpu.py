"""Regex leaves on the device route (veloci_amd/csrc/regex_dfa.cpp, dict_regex.hip, run_fuzzy_probes in prepass.cpp) without a GPU: the pattern -> DFA
compiler against std::wregex under ASan + UBSan (tests/native/regex_dfa_check.cpp, a program of its own), the compiler's resource report of
k_dict_regex, and the whole host side over the stubbed device layer against the host route (tests/native/regex_route_driver.py)."""
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


def test_dfa_agrees_with_std_wregex_under_asan_and_ubsan(tmp_path):
    exe = sanitized.build(tmp_path, "regex_dfa_check", [os.path.join(HERE, "native", "regex_dfa_check.cpp"), os.path.join(CSRC, "regex_dfa.cpp")], flags=["-O1", "-Wall"])
    # 700 patterns per alphabet (ASCII, Latin-1 + Greek, one above U+FFFF) x 200 terms x ignore_case x starts_with
    r, tail = sanitized.run(exe, ["700", "200"], timeout=900)
    assert "REGEX_DFA_CHECK " in r.stdout, tail
    stats = json.loads(r.stdout.split("REGEX_DFA_CHECK ", 1)[1])
    print(stats)
    assert stats["patterns"] >= 2000 and stats["terms_per_pattern"] >= 200 and stats["compared"] == stats["patterns"] * 200 * 4, stats
    assert stats["disagreements"] == 0 and stats["declined"] == 0 and stats["invalid"] == 0 and stats["every_operator"], tail
    assert stats["accepted"] > stats["compared"] // 20 and stats["compared"] - stats["accepted"] > stats["compared"] // 20, stats  # both answers occur
    assert stats["outside"] >= 12 and stats["outside_not_declined"] == 0, tail
    assert r.returncode == 0, tail


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_regex_kernel_compiles_for_gfx950_without_scratch_and_leaves_two_blocks_per_cu(tmp_path):
    rows = {k: v for k, v in KR.resource_report("dict_regex.hip", tmp_path).items() if "k_dict_regex" in k}
    print(rows)
    assert len(rows) == 4, sorted(rows)  # u16 / u32 image x small / full table budget
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] <= 80 * 1024, (k, v)
    assert sum(1 for v in rows.values() if v["LDS Size [bytes/block]"] <= 20 * 1024) == 2, rows  # the small-table form: eight blocks per CU


def test_regex_parts_on_the_stubbed_device_equal_the_host_route():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_NOOP_LAUNCH="1", VQ_STUB_DICT_SCAN="1",
               VQ_HOST_THREADS="4")
    env.pop("VQ_NO_REGEX_DEVICE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "regex_route_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "REGEX_ROUTE_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("REGEX_ROUTE_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats["parts"] >= 60 and stats["declined"] >= 8 and stats["invalid"] >= 4 and stats["regex_launches"] == 2, stats
