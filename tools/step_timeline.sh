# GPU-side timeline of the headline's steps: start, end, queue and gaps of the vq:: kernels (rocprofv3 --kernel-trace, a run of its own: no counters).
# usage: bash tools/step_timeline.sh  (GPU box, from the repository root; VQ_LIB and the library's knobs are passed on to the benchmark)
# A negative "after the previous end" is an overlap: the kernel started while an earlier one was still running (two scan streams).
export TMPDIR=/tmp
S=$(mktemp -d /tmp/step_timeline.XXXXXX)
timeout -k 10 400 rocprofv3 --kernel-trace --kernel-include-regex "vq::" --output-format csv -d $S -o p -- python3 bench.py --steps 6 --warmup 2 --no-cpu --no-extra --no-latency --no-parity > gpurun_out/tl.json 2> gpurun_out/tl.err || exit 1
f=$(find $S -name "*kernel_trace.csv" | head -1)
python3 - "$f" <<'PY'
import csv, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
rows = [r for r in rows if "vq::" in r["Kernel_Name"]][-40:]
t0 = int(rows[0]["Start_Timestamp"])
prev_end = None
for r in rows:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    gap = (s - prev_end) / 1e3 if prev_end is not None else 0.0
    print(f"{r['Kernel_Name'].split('(')[0][4:]:22s} [{(s - t0) / 1e3:9.1f} .. {(e - t0) / 1e3:9.1f}] us, start {gap:+9.1f} us after the previous end, ran {(e - s) / 1e3:9.1f} us, queue {r.get('Queue_Id', '?')}")
    prev_end = max(prev_end or 0, e)
PY
rm -rf $S
