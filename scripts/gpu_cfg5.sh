#!/bin/bash
# config 5 on one GPU: bench with the CPU baseline (--full), kernel trace, MFMA-busy counters of the setup; outputs under
# $OUT_DIR (default out/ in the repository root)
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=${OUT_DIR:-out}
mkdir -p $O
python bench.py --config cfg5 --steps 5 --warmup 2 --full > $O/bench_cfg5.json 2> $O/bench_cfg5.err
echo "bench cfg5 exit $?"; tail -3 $O/bench_cfg5.err; cat $O/bench_cfg5.json
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_cfg5 -- python3 bench.py --config cfg5 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_cfg5_rocprof.json 2> $O/prof_cfg5.err
echo "rocprof exit $?"
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_cfg5_mfma -- python3 bench.py --config cfg5s --steps 1 --warmup 0 --no-cpu-baseline > $O/pmc_cfg5_mfma.json 2> $O/pmc_cfg5_mfma.err
echo "pmc exit $?"
find $O/prof_cfg5 $O/pmc_cfg5_mfma -name "*.csv" | head
