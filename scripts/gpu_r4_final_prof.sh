# round 4, second session: the profile set of scripts/gpu_r4_prof.sh on the final code, then the bench line
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
set -x
bash $ROOT/scripts/gpu_r4_prof.sh || exit 1
cd $ROOT && mkdir -p $OUT
timeout -k 10 500 python bench.py --full > $OUT/r04_bench.json 2> $OUT/r04_bench.err || { tail -20 $OUT/r04_bench.err; exit 1; }
tail -c 600 $OUT/r04_bench.json
