"""The probe kernels' 16-bit array images without a GPU: the host side stages crafted lists over the stubbed device layer
(tests/native/hip_stub.cpp) and tests/native/arr16_class_driver.py reads every list's image and pivot back (vq_debug_arr16_list) — sorted tiles,
pads 0xFFFF, no real entry 0xFFFF, the class bit exactly where raw <= pivot, the pivot by the quantile rule."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
DRIVER = os.path.join(HERE, "native", "arr16_class_driver.py")
STUB_LIB = os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so")


def test_array_entries_carry_the_score_class():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=STUB_LIB, VQ_STUB_NOOP_LAUNCH="1", VQ_HOST_THREADS="4")
    r = subprocess.run([sys.executable, DRIVER], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ARR16_CLASS_DRIVER_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
