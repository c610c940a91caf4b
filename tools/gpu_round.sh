#!/bin/bash
# One box session for a round's record: the default bench line (with secondaries), the same command's
# headline under rocprofv3 --kernel-trace --stats, the PMC passes of the headline kernel, then the GPU
# parity suite and smoke().  Every GPU step under its own limit; the first failure ends the script.
# Usage: TAG=r06a [SKIP_TESTS=1] [SKIP_PMC=1] bash tools/gpu_round.sh
set -e
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
T=${TAG:-round}
OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT/$T
timeout -k 10 420 python3 -u bench.py --full > $OUT/$T/bench.json 2> $OUT/$T/bench.err || { tail -20 $OUT/$T/bench.err; exit 1; }
tail -c 600 $OUT/$T/bench.json; echo
timeout -s KILL 180 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$T/trace -o run -- python3 bench.py --no-secondary --no-cpu-baseline > $OUT/$T/bench_prof.json 2> $OUT/$T/bench_prof.err || { echo "rocprof failed"; tail -5 $OUT/$T/bench_prof.err; exit 1; }
find $OUT/$T/trace -name "*kernel_stats.csv" -exec cp {} $OUT/$T/c2_v1_bench_kernel_stats.csv \;
head -4 $OUT/$T/c2_v1_bench_kernel_stats.csv
if [ -z "$SKIP_PMC" ]; then TAG=$T/pmc bash tools/pmc_passes.sh > /dev/null || exit 1; cat gpurun_out/$T/pmc/summary.txt | head -30; fi
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/$T/pytest_gpu.log 2>&1 || { tail -30 $OUT/$T/pytest_gpu.log; exit 1; }
  tail -2 $OUT/$T/pytest_gpu.log
  timeout -k 10 180 python3 -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/$T/smoke.log 2>&1
  tail -1 $OUT/$T/smoke.log
fi
