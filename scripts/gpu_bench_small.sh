set -x
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
cd "$ROOT"
mkdir -p "$OUT"
python __graft_entry__.py smoke > "$OUT"/smoke.log 2>&1 || { tail -30 "$OUT"/smoke.log; exit 1; }
tail -3 "$OUT"/smoke.log
timeout -k 10 300 python bench.py --full --rows 1000 --cols-per-gpu 20000 --steps 2 --warmup 1 --cpu-sample-cols 5000 > "$OUT"/bench_small.log 2>&1 || { tail -30 "$OUT"/bench_small.log; exit 1; }
tail -3 "$OUT"/bench_small.log
timeout -k 10 600 python bench.py --full --rows 1000 --cols-per-gpu 200000 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT"/bench_200k.log 2>&1 || { tail -30 "$OUT"/bench_200k.log; exit 1; }
tail -3 "$OUT"/bench_200k.log
