# Counter evidence for the per-shape probe kernels on the plain headline run: kernel trace (registers, LDS, duration per kernel), the SQ cycle and
# instruction sets, FETCH_SIZE and WRITE_SIZE — each counter set in a pass of its own (never --pmc together with a trace domain other than
# --kernel-trace).  Every pass runs under its own time limit and the first failure ends the script.  Per-kernel means under $PROFILE_OUT/<tag>/
# (default build/profiles/<tag>/: build/ is kept out of git; copy what is to be judged into profiles/).
# usage: tools/profile_probe_shapes.sh <tag> <library .so under veloci_amd/> [bench args...]
tag=$1; lib=$2; shift 2
O=${PROFILE_OUT:-build/profiles}/$tag; mkdir -p $O
B="bench.py --steps 4 --warmup 2 --no-cpu --no-extra --no-latency --no-parity $*"
echo "== $tag ($lib): $B" > $O/log.txt
pass() {  # name, rocprofv3 arguments...
    name=$1; shift
    S=/tmp/pps_${tag}_$name; rm -rf $S
    VQ_LIB=veloci_amd/$lib timeout -k 10 300 rocprofv3 --kernel-trace --kernel-include-regex "vq::" --output-format csv "$@" -d $S -o p -- python3 $B > $O/bench_$name.json 2> $O/bench_$name.err
    rc=$?
    echo "pass $name rc=$rc" >> $O/log.txt
    if [ $rc -ne 0 ]; then tail -5 $O/bench_$name.err >> $O/log.txt; cat $O/log.txt; exit $rc; fi
}
pass stats --stats
python3 tools/kernel_trace_summary.py /tmp/pps_${tag}_stats $O/kernel_trace.csv
pmc() {
    name=$1; shift
    pass $name --pmc "$@"
    python3 tools/pmc_summary.py /tmp/pps_${tag}_$name $O/pmc_$name.csv > /dev/null
}
pmc sq_cycles SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT
pmc sq_insts SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_WAVES
pmc fetch FETCH_SIZE
pmc write WRITE_SIZE
cat $O/log.txt
