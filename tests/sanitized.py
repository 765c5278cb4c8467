"""The build recipe of the stand-alone check programs (tests/native/*_check.cpp): sources compiled side by side with g++ under ASan + UBSan, the
sanitizers' runtimes linked statically, the program run and its stderr scanned for their reports.  The tests keep their own assertions on what
goes into the program and on what it prints."""
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
HOST_FLAGS = ["-O0", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]


def host_sources():
    """-> (HOST_SRCS of csrc/Makefile, the files of the stubbed device layer)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HOST_SRCS = (.*)$", mk, re.M).group(1).split(), sorted(glob.glob(os.path.join(HERE, "native", "hip_stub*.cpp")))


def build(tmp_path, name, sources, flags=HOST_FLAGS):
    """-> the program `name` under tmp_path, from `sources` (paths)"""
    exe = str(tmp_path / name)
    objs, jobs = [], []
    for src in sources:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        jobs.append((src, subprocess.Popen(["g++", "-std=c++17", "-g1", "-pthread", *flags, *SANITIZE, "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for src, p in jobs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src, err[-3000:])
    # the sanitizers' runtimes are linked statically: the program then runs in whatever environment the suite runs in, with no library order to keep
    r = subprocess.run(["g++", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-o", exe, *objs], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def build_host_check(tmp_path, check, host_srcs, stubs):
    """-> the program of tests/native/<check>.cpp over the library's host sources and the stubbed device layer"""
    return build(tmp_path, check, [os.path.join(CSRC, s) for s in host_srcs] + list(stubs) + [os.path.join(HERE, "native", check + ".cpp")])


def run(exe, args=(), env=None, timeout=600):
    """-> (the finished process, the end of its output); no sanitizer may have reported anything"""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ) if env is None else env)
    tail = r.stdout[-3000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
    return r, tail
