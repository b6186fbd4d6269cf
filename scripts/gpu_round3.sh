# Round-3 measurement set (everything DESIGN.md / BASELINE.md quote).  usage: bash scripts/gpu_round3.sh [TAG]
# -> $OUT (default out/): <TAG>_bench.json, <TAG>_kernel_stats.csv, <TAG>_pmc_kernels.json, <TAG>_stargaps_kernel_stats.csv,
#    <TAG>_stargaps_pmc_kernels.json, <TAG>_gloo2.json
TAG=${1:-r03}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
set -x
cd $ROOT
mkdir -p $OUT
timeout -k 10 1000 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -30 $OUT/${TAG}_bench.err; exit 1; }
cut -c1-600 $OUT/${TAG}_bench.json
cd /tmp && export TMPDIR=/tmp
R=$ROOT
rm -rf $OUT/prof_$TAG
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o b -- python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $OUT/prof_$TAG.log 2>&1 || { tail -30 $OUT/prof_$TAG.log; exit 1; }
cp $(find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_kernel_stats.csv
find $OUT/prof_$TAG -name "*kernel_trace*" -size +20M -delete
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_${TAG}_$c
  timeout -k 10 400 rocprofv3 --pmc $c --kernel-include-regex "k_rank_scan|k_msd_|k_tie_simple|k_copy_rows|k_row_count" --output-format csv -d $OUT/pmc_${TAG}_$c -o s -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $OUT/pmc_$TAG.log 2>&1 || { tail -5 $OUT/pmc_$TAG.log; exit 1; }
  cp $(find $OUT/pmc_${TAG}_$c -name "*counter_collection.csv" | head -1) $OUT/${TAG}_pmc_${c}_counter_collection.csv
done
python3 $R/scripts/pmc_summary.py $OUT/${TAG}_pmc_FETCH_SIZE_counter_collection.csv $OUT/${TAG}_pmc_WRITE_SIZE_counter_collection.csv > $OUT/${TAG}_pmc_kernels.json
# similar rows with gaps (span_scan.hip): kernel stats and the FETCH / WRITE passes of its kernels
rm -rf $OUT/prof_${TAG}_star
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_star -o s -- python3 $R/scripts/gpu_stargaps.py 2 0 > $OUT/prof_${TAG}_star.log 2>&1 || { tail -30 $OUT/prof_${TAG}_star.log; exit 1; }
cp $(find $OUT/prof_${TAG}_star -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_stargaps_kernel_stats.csv
find $OUT/prof_${TAG}_star -name "*kernel_trace*" -size +20M -delete
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_${TAG}_star_$c
  timeout -k 10 400 rocprofv3 --pmc $c --kernel-include-regex "k_sp_|k_pp_" --output-format csv -d $OUT/pmc_${TAG}_star_$c -o s -- python3 $R/scripts/gpu_stargaps.py 1 0 > $OUT/pmc_${TAG}_star.log 2>&1 || { tail -5 $OUT/pmc_${TAG}_star.log; exit 1; }
  cp $(find $OUT/pmc_${TAG}_star_$c -name "*counter_collection.csv" | head -1) $OUT/${TAG}_star_pmc_${c}_counter_collection.csv
done
python3 $R/scripts/pmc_summary.py --star $OUT/${TAG}_star_pmc_FETCH_SIZE_counter_collection.csv $OUT/${TAG}_star_pmc_WRITE_SIZE_counter_collection.csv > $OUT/${TAG}_stargaps_pmc_kernels.json
cd $R
# two ranks sharing this GPU over gloo: the multi-process code path of bench.py (partitioned index, collectives, failure agreement)
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 3 --warmup 1 --backend gloo --cols-per-gpu 500000 > $OUT/${TAG}_gloo2.json 2> $OUT/${TAG}_gloo2.err || { tail -20 $OUT/${TAG}_gloo2.err; exit 1; }
cut -c1-500 $OUT/${TAG}_gloo2.json
