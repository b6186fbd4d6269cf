"""The edit distance of each read to a row that carries its chain on one MI355X: fbg_pindex_chains_align beside the
calls it follows, csrc/pindex_align.hip.

The star_gaps graph of scripts/gpu_rows_bench.py (and with --c3 its c3 graph); reads of 150 symbols cut from the
gap-stripped rows, every read with two substitutions, every second one with a symbol deleted and every other second one
with a symbol inserted; minimum seed length 12, cap 64, unbounded band, pad 16, no window limit.  One warm-up and
--repeats (5) timed rounds of seeds -> chains -> chains_rows -> chains_align; device times lie between hipEvents inside
the library.  One JSON line per graph:
  search_ms, chain_ms, chains_rows_ms   fbg_pindex_seeds, fbg_pindex_chains, fbg_pindex_chains_rows [median, min, max]
  align_ms                              fbg_pindex_chains_align: the row choice, the windows and the two passes
  aligned, unsupported, too_long, too_wide, cells, table_bytes    fbg_pindex_align_stats
  cells_per_s                           cells / median align_ms (a cell is one (read symbol, window symbol) pair; both
                                        passes and everything before them are in the time)
  edits_hist                            reads by edits, 0 .. 5 and more
Usage: python scripts/gpu_align_bench.py [--patterns 200000] [--rows 1000] [--star-cols 200000] [--c3] [--c3-cols 100000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_locate_bench import c3_msa, sample_patterns, star_msa  # noqa: E402
from gpu_seeds_bench import mmm, warm  # noqa: E402

CAP, L, READ, PAD = 64, 12, 150, 16
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def edited_reads(rng, msa, count):
    """count reads of READ symbols: windows of READ + 1 symbols of the rows, two symbols replaced by other ones, then in
    even reads one symbol deleted, in odd reads one inserted and the last dropped."""
    data, _ = sample_patterns(rng, msa, count, length=READ + 1, mutated=0.0)
    w = data.reshape(count, READ + 1).copy()
    rows = np.arange(count)
    for at in (rng.integers(0, READ // 2, count), rng.integers(READ // 2, READ, count)):
        w[rows, at] = ACGT[(np.searchsorted(ACGT, w[rows, at]) + rng.integers(1, 4, count)) % 4]
    idx = np.arange(READ)[None, :]
    at = rng.integers(1, READ - 1, count)[:, None]
    deleted = np.take_along_axis(w, idx + (idx >= at), axis=1)
    inserted = np.take_along_axis(w, idx - (idx > at), axis=1)
    inserted[rows, at[:, 0]] = ACGT[rng.integers(0, 4, count)]
    out = np.where((rows % 2 == 0)[:, None], deleted, inserted)
    return np.ascontiguousarray(out).ravel(), np.arange(count + 1, dtype=np.uint64) * READ


def run(eng, name, msa, a, rng):
    b = eng.minmax_dp(eng.elastic_f(msa))
    pats = edited_reads(rng, msa, a.patterns)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b, rows=True) as pix:
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, rows=True)
        pix.chains(rows=True, align=True, pad=PAD)
        t = {k: [] for k in ("search_ms", "chain_ms", "chains_rows_ms", "align_ms")}
        for _ in range(a.repeats):
            res = pix.seeds(pats, min_length=L, max_per_seed=CAP)
            ch = pix.chains(rows=True, align=True, pad=PAD)
            t["search_ms"].append(res.search_ms)
            t["chain_ms"].append(ch.device_ms)
            t["chains_rows_ms"].append(ch.rows_ms)
            t["align_ms"].append(ch.align_ms)
        st = pix.align_stats()
        e = ch.edits[ch.edits != 0xffffffff]
        out = {"workload": name, "blocks": len(b), "rows": int(msa.shape[0]), "reads": int(a.patterns), "read_len": READ, "pad": PAD,
               "min_length": L, "cap": CAP, "chained": int((np.diff(ch.chain_off.astype(np.int64)) > 0).sum()), **st,
               "edits_hist": np.bincount(np.minimum(e, 5), minlength=6).tolist()}
        out.update({k: mmm(v) for k, v in t.items()})
        out["cells_per_s"] = round(st["cells"] / (np.median(t["align_ms"]) / 1e3)) if st["cells"] else 0
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=200_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--c3", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2030)
    with F.Engine(0) as eng:
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)
        if a.c3:
            run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)


if __name__ == "__main__":
    main()
