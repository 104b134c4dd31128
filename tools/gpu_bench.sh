# bench + rocprof kernel stats for one workload (each step time-limited)
set -o pipefail
cd $GRAFT_REPO_ROOT
export OSE_SKIP_BUILD=1
WL=${1:-url}
mkdir -p gpurun_out
LOG=${OSE_BENCH_OUT:-$PWD/bench_out}/bench_$WL.log
mkdir -p $(dirname $LOG)
timeout -k 10 400 python bench.py --full --workload $WL --steps 20 --warmup 5 > $LOG 2>&1 || { echo "bench failed"; tail -30 $LOG; exit 1; }
grep '"metric"' $LOG
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $GRAFT_REPO_ROOT/gpurun_out/prof_$WL -o $WL --output-format csv -- python3 $GRAFT_REPO_ROOT/bench.py --workload $WL --steps 10 --warmup 2 --no-cpu-baseline > $GRAFT_REPO_ROOT/gpurun_out/prof_$WL.log 2>&1 || { echo "rocprof failed"; tail -30 $GRAFT_REPO_ROOT/gpurun_out/prof_$WL.log; exit 1; }
f=$(find $GRAFT_REPO_ROOT/gpurun_out/prof_$WL -name "*kernel_stats.csv" | head -1)
head -12 "$f"
