"""The vq_debug_*_lists entry points (the pre-pass drivers alone, tests/test_gpu_prepass_lists.py) without a GPU: their argument handling, the host
side of the four drivers and the copy of the lists under ASan + UBSan as a program of its own (tests/native/prepass_debug_check.cpp) over the
stubbed device layer, and the places that must name the new entry points."""
import glob
import json
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
NAMES = ("vq_debug_union_lists", "vq_debug_locality_lists", "vq_debug_range_hits", "vq_debug_boost1n_lists")


def test_prepass_debug_entry_points_under_asan_and_ubsan(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    host_srcs = re.search(r"^HOST_SRCS = (.*)$", mk, re.M).group(1).split()
    stubs = sorted(glob.glob(os.path.join(HERE, "native", "hip_stub*.cpp")))
    exe = str(tmp_path / "prepass_debug_check")
    objs, jobs = [], []
    for src in [os.path.join(CSRC, s) for s in host_srcs] + stubs + [os.path.join(HERE, "native", "prepass_debug_check.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        jobs.append((src, subprocess.Popen(["g++", "-std=c++17", "-O0", "-g1", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
                                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for src, p in jobs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src, err[-3000:])
    # the sanitizers' runtimes are linked statically: the program then runs in whatever environment the suite runs in, with no library order to keep
    r = subprocess.run(["g++", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-o", exe, *objs], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("VQ_UNION_DENSE_MIN", "VQ_STUB_LAUNCH_LOG")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
    assert r.returncode == 0 and "PREPASS_DEBUG_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("PREPASS_DEBUG_CHECK_OK ", 1)[1])
    assert stats == {"ok": 7, "refused": 18}, stats


def test_every_layer_names_the_entry_points():
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in NAMES:
            assert name in text, (rel, name)
