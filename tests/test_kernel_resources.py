"""The compiler's own resource report of the probe kernels (scan_probe.hip, cross-compiled for gfx950; no GPU needed): a kernel is charged the
registers of the largest body it contains and gets its waves per SIMD from that — 512 registers per SIMD lane, so 128 is the line for four
waves, 168 what three leave.  All nine AND bodies in one kernel once cost the headline shape a wave per SIMD without anybody looking."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def resource_report(src, tmp_path):
    """-> {kernel name: {field: int}} from -Rpass-analysis=kernel-resource-usage, compiled with the Makefile's own flags"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-x", "hip", *flags, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "out.o")],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        k, _, v = m.group(1).strip().partition(":")
        if k == "Function Name":
            cur = rows.setdefault(v.strip(), {})
        elif cur is not None and v.strip().lstrip("-").isdigit():
            cur[k.strip()] = int(v)
    return rows


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_probe_kernels_keep_their_register_budget(tmp_path):
    rows = {k: v for k, v in resource_report("scan_probe.hip", tmp_path).items() if "k_scan_probe" in k}
    print(rows)
    ands = {k: v for k, v in rows.items() if "k_scan_probe_or" not in k}
    low = {k: v for k, v in ands.items() if re.search(r"k_scan_probe_(1|2_\d)E", k)}  # ND <= 2
    assert len(low) == 4 and len(ands) == 8 and len(rows) == 9, sorted(rows)
    for k, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 168, (k, v)  # what the one-kernel form took: three waves per SIMD
    for k, v in low.items():
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 128 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)  # four waves per SIMD
