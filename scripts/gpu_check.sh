#!/bin/bash
# One GPU-box pass: parity tests, bench (--full: roofline + cpu_baseline), kernel trace, PMC traffic passes.  Outputs under
# $OUT_DIR (default out/ in the repository root).
set -x
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=${OUT_DIR:-out}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $O/pytest_gpu.log
python bench.py --full > $O/bench_cfg4.json 2> $O/bench_cfg4.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_cfg4 -- python3 bench.py --no-cpu-baseline > $O/bench_cfg4_rocprof.json 2> $O/prof_cfg4.err
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 bench.py --no-cpu-baseline --steps 1 --warmup 0 > $O/pmc_fetch.json 2> $O/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 bench.py --no-cpu-baseline --steps 1 --warmup 0 > $O/pmc_write.json 2> $O/pmc_write.err
ls -la $O $O/*/* | tail -40
tail -3 $O/pytest_gpu.log
cat $O/bench_cfg4.json
