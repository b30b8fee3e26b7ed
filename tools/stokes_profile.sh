# The three rocprofv3 passes of tools/round_profile.sh for `bench.py --workload stokes_rbc` (config 4), under $OUT (default prof_out/).
# usage: bash tools/stokes_profile.sh r02h [stokes_rbc_traction]      (second argument: the workload, default stokes_rbc)
set -e
TAG=${1:-r02}
WL=${2:-stokes_rbc}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)          # absolute: the passes run from /tmp
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stokes_trace -o t -- python3 $R/bench.py --full --workload $WL --no-cpu-baseline --no-accuracy > $OUT/${TAG}_stokes_trace.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_stokes_fetch -o f -- python3 $R/bench.py --full --workload $WL --no-cpu-baseline --no-accuracy --steps 5 --warmup 1 > $OUT/${TAG}_stokes_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_stokes_write -o w -- python3 $R/bench.py --full --workload $WL --no-cpu-baseline --no-accuracy --steps 5 --warmup 1 > $OUT/${TAG}_stokes_write.log 2>&1
cd $R
python tools/prof_summary.py kernel-stats $OUT/${TAG}_stokes_trace $OUT/${TAG}_stokes_kernel_stats.md | head -12
python tools/prof_summary.py pmc $OUT/${TAG}_stokes_fetch $OUT/${TAG}_stokes_write $OUT/${TAG}_stokes_pmc.json 524288 1 | tail -5
python bench.py --full --workload $WL > $OUT/${TAG}_bench_stokes.json 2> $OUT/${TAG}_bench_stokes.err
tail -c 400 $OUT/${TAG}_bench_stokes.json
