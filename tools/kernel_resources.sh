#!/bin/bash
# Per-kernel register / scratch / LDS / occupancy report from the compiler (no GPU needed).
# Every .hip file of the library (SRCS of the Makefile), compiled with the Makefile's flags.  usage: tools/kernel_resources.sh [file.hip ...]
cd "$(dirname "$0")/../veloci_amd/csrc"
FLAGS=$(sed -n 's/^CXXFLAGS ?= //p' Makefile)
FILES=${*:-$(sed -n 's/^SRCS = //p' Makefile | tr ' ' '\n' | grep '\.hip$')}
OUT=$(mktemp -d)
for f in $FILES; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -x hip $FLAGS -Rpass-analysis=kernel-resource-usage -c $f -o $OUT/${f%.hip}.o 2>&1
done |
python3 -c '
import re, sys
cur = None
rows = {}
for line in sys.stdin:
    m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = t.split(":", 1)[1].strip(); rows[cur] = {}
    elif cur and ":" in t:
        k, v = t.split(":", 1); rows[cur][k.strip()] = v.strip()
for name, r in rows.items():
    print("%-70s VGPR %-4s AGPR %-3s SGPR %-4s spilled SGPR %-5s scratch %-6s occupancy %-3s LDS %s" % (name[:70], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("SGPRs Spill"), r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]")))
'
rm -rf "$OUT"
