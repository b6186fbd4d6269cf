"""The four streaming kernels of the C3 step from a rocprofv3 --kernel-trace csv of bench.py: the averages of the sort passes and the
lean scan over the traced steps, with their shortest and longest launch (profiles/scan_rows_ahead_summary.txt).
usage: python3 scripts/scan_trace_summary.py TAG kernel_trace.csv"""
import csv
import re
import sys

tag, path = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(path)))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["Kernel_Name"] = re.sub(r"^void ", "", r["Kernel_Name"])          # (templates are listed with their return type)
rows.sort(key=lambda r: r["s"])
for name in ("k_msd_pack_split", "k_msd_split", "k_msd_finish", "k_msd_finish_big", "k_rank_scan_lean", "k_tie_pairs"):
    d = [(r["e"] - r["s"]) / 1e3 for r in rows if re.match(name + r"\b", r["Kernel_Name"])]
    if d:
        print(f"{tag:10s} {name:20s} launches {len(d):3d}  average {sum(d) / len(d):7.1f} us  min {min(d):7.1f}  max {max(d):7.1f}"
              + ("  in launch order " + " ".join("%.0f" % x for x in d) if len(d) <= 12 else ""))
