"""The alignment path (CIGAR) of each aligned read on one MI355X: fbg_pindex_chains_cigar beside fbg_pindex_chains_align
for the same reads, csrc/pindex_align.hip.

The star_gaps graph of scripts/gpu_rows_bench.py; reads cut from the gap-stripped rows as in scripts/gpu_align_bench.py
(two substitutions per read, every second read with a symbol deleted and every other second one with a symbol inserted),
at one read length per tier of the column history: --lds-read (150) symbols, whose history stays in LDS, and
--scratch-read (600), whose history goes to device memory in batches of option path_batch_kib.  Minimum seed length 12,
cap 64, unbounded band, pad 16, no window limit.  One warm-up and --repeats (5) timed rounds of seeds -> chains ->
chains_align -> chains_cigar; device times lie between hipEvents inside the library.  One JSON line per read length:
  align_ms         fbg_pindex_chains_align [median, min, max]
  cigar_ms         fbg_pindex_chains_cigar: the sizes, the pass with its history, the trace and the compaction
  cigar_over_align median cigar_ms / median align_ms
  chains_call_wall_ms   host time of the whole chains(align=True, cigar=True) call, the copies of the arrays included
  paths, ops, columns, history_bytes, batches    fbg_pindex_cigar_stats
  columns_per_s    columns / median cigar_ms
  runs_hist        reads by runs, 0 .. 9 and more
Usage: python scripts/gpu_cigar_bench.py [--patterns 200000] [--long-patterns 50000] [--rows 1000] [--star-cols 200000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_locate_bench import sample_patterns, star_msa  # noqa: E402
from gpu_seeds_bench import mmm, warm  # noqa: E402

CAP, L, PAD = 64, 12, 16
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def edited_reads(rng, msa, count, read):
    """gpu_align_bench.edited_reads at a read length of choice."""
    data, _ = sample_patterns(rng, msa, count, length=read + 1, mutated=0.0)
    w = data.reshape(count, read + 1).copy()
    rows = np.arange(count)
    for at in (rng.integers(0, read // 2, count), rng.integers(read // 2, read, count)):
        w[rows, at] = ACGT[(np.searchsorted(ACGT, w[rows, at]) + rng.integers(1, 4, count)) % 4]
    idx = np.arange(read)[None, :]
    at = rng.integers(1, read - 1, count)[:, None]
    deleted = np.take_along_axis(w, idx + (idx >= at), axis=1)
    inserted = np.take_along_axis(w, idx - (idx > at), axis=1)
    inserted[rows, at[:, 0]] = ACGT[rng.integers(0, 4, count)]
    out = np.where((rows % 2 == 0)[:, None], deleted, inserted)
    return np.ascontiguousarray(out).ravel(), np.arange(count + 1, dtype=np.uint64) * read


def run(eng, pix, msa, count, read, a, rng):
    pats = edited_reads(rng, msa, count, read)
    pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, rows=True)
    pix.chains(align=True, pad=PAD, cigar=True)
    t = {k: [] for k in ("align_ms", "cigar_ms", "chains_call_wall_ms")}
    for _ in range(a.repeats):
        pix.seeds(pats, min_length=L, max_per_seed=CAP)
        t0 = time.perf_counter()
        ch = pix.chains(align=True, pad=PAD, cigar=True)
        wall = (time.perf_counter() - t0) * 1e3
        t["align_ms"].append(ch.align_ms)
        t["cigar_ms"].append(ch.cigar_ms)
        t["chains_call_wall_ms"].append(wall)
    st = pix.cigar_stats()
    runs = np.diff(ch.cigar_off.astype(np.int64))
    out = {"workload": "star_gaps", "rows": int(msa.shape[0]), "reads": int(count), "read_len": read, "pad": PAD, "min_length": L,
           "cap": CAP, "aligned": pix.align_stats()["aligned"], **st, "path_batch_kib": eng.get_option("path_batch_kib"),
           "runs_hist": np.bincount(np.minimum(runs, 9), minlength=10).tolist()}
    out.update({k: mmm(v) for k, v in t.items()})
    out["cigar_over_align"] = round(float(np.median(t["cigar_ms"]) / np.median(t["align_ms"])), 3)
    out["columns_per_s"] = round(st["columns"] / (np.median(t["cigar_ms"]) / 1e3)) if st["columns"] else 0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=200_000)
    ap.add_argument("--long-patterns", type=int, default=50_000)
    ap.add_argument("--lds-read", type=int, default=150)
    ap.add_argument("--scratch-read", type=int, default=600)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2031)
    with F.Engine(0) as eng:
        msa = star_msa(rng, a.rows, a.star_cols)
        b = eng.minmax_dp(eng.elastic_f(msa))
        eng.msa_load_host(msa)
        with eng.pattern_index_of_segmentation(b, rows=True) as pix:
            run(eng, pix, msa, a.patterns, a.lds_read, a, rng)
            run(eng, pix, msa, a.long_patterns, a.scratch_read, a, rng)


if __name__ == "__main__":
    main()
