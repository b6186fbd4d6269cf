set -x
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
cd /tmp && export TMPDIR=/tmp
rm -rf "$OUT"/pmc_fetch "$OUT"/pmc_write
mkdir -p "$OUT"
# --full: k_scan_stream and k_apply_groups0 run only in the other workloads
timeout -k 10 500 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "k_rank_scan|k_scan_stream|k_apply_groups0" --output-format csv -d "$OUT"/pmc_fetch -o f -- python3 "$ROOT"/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$OUT"/pmc_fetch.log 2>&1 || { tail -20 "$OUT"/pmc_fetch.log; exit 1; }
timeout -k 10 500 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "k_rank_scan|k_scan_stream|k_apply_groups0" --output-format csv -d "$OUT"/pmc_write -o w -- python3 "$ROOT"/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$OUT"/pmc_write.log 2>&1 || { tail -20 "$OUT"/pmc_write.log; exit 1; }
ls -R "$OUT"/pmc_fetch | head; head -5 "$OUT"/pmc_fetch/*counter_collection.csv
