# round 4, second session: the whole GPU suite, smoke, the bench line
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=${OUT:-$ROOT/out}
set -x
cd $ROOT && mkdir -p $OUT
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $OUT/r4h_tests.log 2>&1 || { tail -40 $OUT/r4h_tests.log; exit 1; }
tail -3 $OUT/r4h_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout -k 10 400 python bench.py --full > $OUT/r4h_bench.json 2> $OUT/r4h_bench.err || { tail -20 $OUT/r4h_bench.err; exit 1; }
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "r4h_bench.json")).read().strip().splitlines()[-1])
print("C3 ms/step", round(d["ms_per_step"], 2), "boundary", d.get("boundary_ms"), "latency", d.get("latency_ms"))
for w in d["other_workloads"]:
    print(w["workload"][:60], round(w["ms_per_step"], 2), {k: v for k, v in w["stages_ms"].items() if v > 0.3}, "dp_kind", w.get("dp_kind"))
PY
