"""Per-launch sums of the counters in a rocprofv3 --pmc csv, kernel by kernel (counter unit of WRITE_SIZE: KiB), as the lines of
profiles/msd_cursors_summary.txt.
usage: python3 scripts/pmc_write_size.py TAG counter_collection.csv"""
import collections
import csv
import sys

tag, path = sys.argv[1], sys.argv[2]
acc = collections.defaultdict(float)
launches = collections.defaultdict(set)
for r in csv.DictReader(open(path)):
    k = (r["Kernel_Name"].split("(")[0].replace("void ", ""), r["Counter_Name"])
    acc[k] += float(r["Counter_Value"])
    launches[k].add(r["Dispatch_Id"])
for k, v in sorted(acc.items()):
    n = len(launches[k])
    print(f"{tag:10s} {k[0]:32s} {k[1]:12s} launches {n:2d}  per launch {v / n:14.1f} KiB = {v / n * 1024 / 1e9:7.3f} GB", flush=True)
