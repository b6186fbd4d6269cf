"""Chaining along one MSA row on one MI355X: fbg_pindex_chains_by_row beside fbg_pindex_chains + fbg_pindex_chains_rows on
the same seeds, and what fbg_pindex_chains_align aligns after either, csrc/pindex_byrow.hip.

The star_gaps graph and the edited reads of scripts/gpu_align_bench.py (reads of 150 symbols cut from the gap-stripped
rows, two substitutions and one deleted or inserted symbol each; minimum seed length 12, cap 64, unbounded band, pad
16).  One warm-up and --repeats (5) timed rounds of seeds -> chains -> chains_rows -> chains_align -> chains_by_row ->
chains_rows -> chains_align; device times lie between hipEvents inside the library.  One JSON line per graph:
  search_ms                             fbg_pindex_seeds [median, min, max]
  chain_ms, chains_rows_ms, align_ms    fbg_pindex_chains, fbg_pindex_chains_rows and fbg_pindex_chains_align after it
  by_row_ms, by_row_rows_ms, by_row_align_ms   fbg_pindex_chains_by_row, and the two calls after it
  aligned, unsupported                  fbg_pindex_align_stats after the plain call; by_row_aligned, by_row_unsupported after
                                        fbg_pindex_chains_by_row
  reads_lds ... max_places              fbg_pindex_chains_by_row_stats
  same_score                            reads whose by-row score is the plain chain's
Usage: python scripts/gpu_byrow_bench.py [--patterns 200000] [--rows 1000] [--star-cols 200000] [--c3] [--c3-cols 100000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_align_bench import CAP, L, PAD, READ, edited_reads  # noqa: E402
from gpu_locate_bench import c3_msa, star_msa  # noqa: E402
from gpu_seeds_bench import mmm, warm  # noqa: E402


def run(eng, name, msa, a, rng):
    b = eng.minmax_dp(eng.elastic_f(msa))
    pats = edited_reads(rng, msa, a.patterns)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b, rows=True) as pix:
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, rows=True)
        pix.chains(rows=True, align=True, pad=PAD)
        pix.chains(rows=True, align=True, pad=PAD, by_row=True)
        keys = ("search_ms", "chain_ms", "chains_rows_ms", "align_ms", "by_row_ms", "by_row_rows_ms", "by_row_align_ms")
        t = {k: [] for k in keys}
        for _ in range(a.repeats):
            res = pix.seeds(pats, min_length=L, max_per_seed=CAP)
            ch = pix.chains(rows=True, align=True, pad=PAD)
            plain = pix.align_stats()
            br = pix.chains(rows=True, align=True, pad=PAD, by_row=True)
            mine = pix.align_stats()
            for k, v in zip(keys, (res.search_ms, ch.device_ms, ch.rows_ms, ch.align_ms, br.device_ms, br.rows_ms, br.align_ms)):
                t[k].append(v)
        out = {"workload": name, "blocks": len(b), "rows": int(msa.shape[0]), "reads": int(a.patterns), "read_len": READ, "pad": PAD,
               "min_length": L, "cap": CAP, "chained": int((np.diff(ch.chain_off.astype(np.int64)) > 0).sum()),
               "aligned": plain["aligned"], "unsupported": plain["unsupported"],
               "by_row_chained": int((np.diff(br.chain_off.astype(np.int64)) > 0).sum()), "by_row_aligned": mine["aligned"],
               "by_row_unsupported": mine["unsupported"], "same_score": int((br.score == ch.score).sum()), **pix.by_row_stats()}
        out.update({k: mmm(v) for k, v in t.items()})
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
