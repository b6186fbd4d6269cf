set -x
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
cd "$ROOT"
mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full > "$OUT"/bench_full.log 2>&1 || { tail -30 "$OUT"/bench_full.log; exit 1; }
tail -2 "$OUT"/bench_full.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_r1 -o r1 -- python3 "$ROOT"/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT"/prof_r1.log 2>&1 || { tail -30 "$OUT"/prof_r1.log; exit 1; }
tail -2 "$OUT"/prof_r1.log
find "$OUT"/prof_r1 -name "*stats*" | head; find "$OUT"/prof_r1 -name "*kernel_trace*" -size +20M -delete
