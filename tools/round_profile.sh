# Round profile: rocprofv3 kernel trace + separate PMC passes for the default bench workload, summaries under $OUT/<tag>_*
# (default OUT: prof_out/ in the repository; copy what is to be kept into profiles/).  usage, on the GPU machine:
#   bash tools/round_profile.sh r02h
# The program stands directly behind `--` (python3 itself: no env / shell hop under the profiler), PMC passes are their own runs.
set -e
TAG=${1:-r02}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)          # absolute: the passes run from /tmp
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o t -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench_trace.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_fetch -o f -- python3 $R/bench.py --full --no-cpu-baseline --no-accuracy --steps 5 --warmup 1 > $OUT/${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_write -o w -- python3 $R/bench.py --full --no-cpu-baseline --no-accuracy --steps 5 --warmup 1 > $OUT/${TAG}_write.log 2>&1
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA --output-format csv -d $OUT/${TAG}_sq -o s -- python3 $R/bench.py --full --no-cpu-baseline --no-accuracy --steps 4 --warmup 1 > $OUT/${TAG}_sq.log 2>&1
cd $R
python tools/prof_summary.py kernel-stats $OUT/${TAG}_trace $OUT/${TAG}_kernel_stats.md > /dev/null
python tools/prof_summary.py pmc $OUT/${TAG}_fetch $OUT/${TAG}_write $OUT/${TAG}_pmc.json 1048576 1 > /dev/null
python tools/pmc_kernel.py $OUT/${TAG}_sq m2l > $OUT/${TAG}_pmc_sq_m2l.txt
python tools/pmc_kernel.py $OUT/${TAG}_sq near_spmv >> $OUT/${TAG}_pmc_sq_m2l.txt
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
tail -c 600 $OUT/${TAG}_bench.json
head -16 $OUT/${TAG}_kernel_stats.md
cat $OUT/${TAG}_pmc_sq_m2l.txt
