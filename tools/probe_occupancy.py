"""LDS bytes and resident one-wave workgroups per CU of every probe scan kernel, as the runtime grants them (hipOccupancyMaxActiveBlocksPerMultiprocessor),
over a sweep of the array operands' LDS slot — the steps show the LDS allocation granule.  usage: python tools/probe_occupancy.py [cand_cap]  (GPU box)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (the HIP runtime of the process: see veloci_amd/_lib.py)
import veloci_amd  # noqa: E402

L = veloci_amd.lib()
f = L.vq_debug_probe_occupancy
f.restype = C.c_uint32
f.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)]
cand_cap = int(sys.argv[1]) if len(sys.argv) > 1 else 32
SHAPES = [("k_scan_probe_1 <1,0>", 0, 1, 0), ("k_scan_probe_1 <1,1>", 0, 1, 1), ("k_scan_probe_2_0", 1, 2, 0), ("k_scan_probe_2_1", 2, 2, 1), ("k_scan_probe_2_2", 3, 2, 2),
          ("k_scan_probe_3_0", 4, 3, 0), ("k_scan_probe_3_1", 5, 3, 1), ("k_scan_probe_3_2", 6, 3, 2), ("k_scan_probe_3_3", 7, 3, 3), ("k_scan_probe_or <1,0>", 8, 1, 0),
          ("k_scan_probe_or <2,0>", 8, 2, 0)]
for name, shape, nd, na in SHAPES:
    row = []
    for gran in ([0] if na == 0 else [64, 128, 136, 140, 144, 148, 152, 160, 176, 192, 224, 256]):
        lds = C.c_uint32(0)
        wgs = f(shape, nd, na, gran * 4, cand_cap, C.byref(lds))
        row.append("%s%d B -> %d" % ("" if na == 0 else "%d granules: " % gran, lds.value, wgs))
    print("%-24s %s" % (name, "; ".join(row)))
