"""The front of the C3 step from a rocprofv3 --kernel-trace csv of bench.py: the averages of the front's kernels over the traced
steps, and the last traced step from the previous step's k_count_unfilled to pass 1 of the sort in launch order
(profiles/front_of_step_summary.txt).  usage: python3 scripts/front_trace_summary.py TAG kernel_trace.csv"""
import csv
import re
import sys

tag, path = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(path)))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["Kernel_Name"] = re.sub(r"^void ", "", r["Kernel_Name"])          # (templates are listed with their return type)
rows.sort(key=lambda r: r["s"])
queues = {q: i for i, q in enumerate(sorted({r["Queue_Id"] for r in rows}))}
for name in ("k_row_count_fast", "k_row_count", "k_row_offsets", "k_sample_keys", "k_sample_twins", "k_count_equal_neighbours",
             "k_msd_pack_split"):
    d = [(r["e"] - r["s"]) / 1e3 for r in rows if re.match(name + r"\b", r["Kernel_Name"])]
    if d:
        print(f"{tag:10s} {name:28s} launches {len(d):3d}  average {sum(d) / len(d):7.1f} us  min {min(d):7.1f}  max {max(d):7.1f}"
              + ("  in launch order " + " ".join("%.0f" % x for x in d) if len(d) <= 8 else ""))
ends = [k for k, r in enumerate(rows) if r["Kernel_Name"].startswith("k_count_unfilled")]
pass1 = [k for k, r in enumerate(rows) if r["Kernel_Name"].startswith("k_msd_pack_split")]
if len(ends) >= 1 and pass1:
    last = pass1[-1]
    before = [k for k in ends if k < last]
    if before:
        k0 = before[-1]
        t0 = rows[k0]["e"]
        print(f"{tag}: last traced step, the previous k_count_unfilled's end to pass 1's start: {(rows[last]['s'] - t0) / 1e3:.0f} us, "
              f"{last - k0 - 1} launches between them; start end duration queue kernel (us from that end)")
        for r in rows[k0:last + 1]:
            print(f"{(r['s'] - t0) / 1e3:8.0f} {(r['e'] - t0) / 1e3:8.0f} {(r['e'] - r['s']) / 1e3:6.0f} q{queues[r['Queue_Id']]} {r['Kernel_Name'][:56]}")
