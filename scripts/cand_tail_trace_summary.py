"""The tail of the rank-order scan in a rocprofv3 --kernel-trace csv of bench.py (profiles/cand_tail_summary.txt): for every traced
step the spans the parts of the tail are judged on, their average, shortest and longest, the averages of the tail's kernels, and
the last traced step from the lean scan's start to k_count_unfilled's end in launch order.  The first two traced steps (bench.py's
warm-up) are left out of the figures.
  part 1: start of the region sort (k_cand_sort_compact / k_cand_region) to the start of k_tie_big
  part 2: start of the runs' first kernel (k_runs / k_cand_lcp) to the end of their last (k_runs_long / k_cand_runs_long)
  part 3: end of the lean scan to the start of the region sort
  tail:   end of the lean scan to the end of k_count_unfilled
usage: python3 scripts/cand_tail_trace_summary.py TAG kernel_trace.csv"""
import csv
import re
import sys

tag, path = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(path)))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["Kernel_Name"] = re.sub(r"^void ", "", r["Kernel_Name"])          # (templates are listed with their return type)
    r["q"] = r.get("Queue_Id", "?")
rows.sort(key=lambda r: r["s"])


def is_(r, *names):
    return any(re.match(n + r"\b", r["Kernel_Name"]) for n in names)


steps, cur = [], None
for r in rows:
    if is_(r, "k_rank_scan_lean"):
        cur = [r]
    elif cur is not None:
        cur.append(r)
        if is_(r, "k_count_unfilled"):
            steps.append(cur)
            cur = None


def first(step, *names):
    return next((r for r in step if is_(r, *names)), None)


def last(step, *names):
    return next((r for r in reversed(step) if is_(r, *names)), None)


spans = {"part1": [], "part2": [], "part3": [], "tail": []}
for st in steps:
    scan, sort, big = st[0], first(st, "k_cand_sort_compact", "k_cand_region"), first(st, "k_tie_big")
    r0, r1 = first(st, "k_runs", "k_cand_lcp"), last(st, "k_runs_long", "k_cand_runs_long", "k_runs", "k_cand_runs")
    if sort and big:
        spans["part1"].append((big["s"] - sort["s"]) / 1e3)
        spans["part3"].append((sort["s"] - scan["e"]) / 1e3)
    if r0 and r1:
        spans["part2"].append((r1["e"] - r0["s"]) / 1e3)
    spans["tail"].append((st[-1]["e"] - scan["e"]) / 1e3)
print(f"{tag}: {len(steps)} traced steps; averages and spreads without the first two (warm-up)")
skip = 2 if len(steps) > 4 else 0
steps = steps[skip:]
for k, d in spans.items():
    d = d[skip:]
    if d:
        print(f"{tag:10s} {k:6s} average {sum(d) / len(d):7.1f} us  min {min(d):7.1f}  max {max(d):7.1f}  in step order " + " ".join("%.0f" % x for x in d))
for name in ("k_rank_scan_lean", "k_tie_pairs", "k_tie_simple", "k_cand_counts", "k_cand_sort_compact", "k_cand_region", "k_tie_groups", "k_tie_big",
             "k_runs", "k_cand_lcp", "k_cand_runs", "k_runs_long", "k_cand_runs_long", "k_count_unfilled"):
    d = [(r["e"] - r["s"]) / 1e3 for st in steps for r in st if is_(r, name)]
    if d:
        print(f"{tag:10s} {name:20s} launches {len(d):3d}  average {sum(d) / len(d):7.1f} us  min {min(d):7.1f}  max {max(d):7.1f}")
if steps:
    st, t0 = steps[-1], steps[-1][0]["s"]
    print(f"## {tag}: last traced step (us from the lean scan's start): start end duration queue kernel")
    for r in st:
        print(f"{(r['s'] - t0) / 1e3:8.0f} {(r['e'] - t0) / 1e3:8.0f} {(r['e'] - r['s']) / 1e3:7.0f} q{r['q']} {r['Kernel_Name'][:48]}")
