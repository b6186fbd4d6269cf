"""Co-linear chaining of a read's seeds on one MI355X: fbg_pindex_chains (start columns, binning, the three tiers of
k_pc_chain, trace, scan, trace) beside the calls it saves the caller, csrc/pindex_chain.hip.

The two graphs of scripts/gpu_locate_bench.py, built through fbg_pindex_build_segmentation (chaining needs the MSA
columns), and the two read batches of scripts/gpu_seeds_bench.py (10^6 reads of 100 symbols: "one_in_ten" with one
substitution in 10 % of the reads, "two_each" with two in every read).  Minimum lengths 1 and 12, cap 64, unbounded band.
Every row is one warm-up and --repeats (5) timed rounds of seeds -> places fetch -> chains; device times lie between
hipEvents inside the library.  One JSON line per row:
  search_ms   fbg_pindex_seeds                                  [median, min, max]
  fetch_ms    fbg_pindex_seeds_fetch + fbg_pindex_seeds_places: what a caller who chains on the host has to copy
  chain_ms    fbg_pindex_chains
  anchors, reads_small / reads_wave / reads_spill               fbg_pindex_chain_stats
  chained, entries                                              reads with a chain, chain entries in all
--seeds-only prints, per graph and batch, --repeats values of fbg_pindex_seeds' search_ms (L = 12, cap 64, after one
warm-up) and nothing the chain calls added: the figure a parent commit is compared on.  The package binds every entry
point it lists when it loads the library, so this tree's package does not load a parent's library: for the parent's
figures copy this file into scripts/ of a built checkout of the parent and run it there with --seeds-only, the two in
alternating processes.
Usage: python scripts/gpu_chains_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--seeds-only]
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
from gpu_seeds_bench import mmm, two_substitutions, warm  # noqa: E402

CAP = 64


def rows(pix, name, batch, pats, n_pat, repeats):
    for L in (1, 12):
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True)
        s_ms, f_ms, c_ms = [], [], []
        for _ in range(repeats):
            res = pix.seeds(pats, min_length=L, max_per_seed=CAP, chain=True)
            s_ms.append(res.search_ms)
            f_ms.append(res.fetch_ms)
            c_ms.append(res.chains.device_ms)
        st = pix.chain_stats()
        print(json.dumps({
            "workload": name, "batch": batch, "text_len": pix.text_length(), "reads": int(n_pat), "read_len": 100,
            "min_length": L, "cap": CAP, "seeds": len(res), "start_places": int(res.occ.start_off[-1]),
            "search_ms": mmm(s_ms), "fetch_ms": mmm(f_ms), "chain_ms": mmm(c_ms), "anchors": st["anchors"],
            "reads_small": st["reads_small"], "reads_wave": st["reads_wave"], "reads_spill": st["reads_spill"],
            "chained": int((np.diff(res.chains.chain_off.astype(np.int64)) > 0).sum()), "entries": int(res.chains.chain_off[-1]),
        }), flush=True)


def seeds_only(pix, name, batch, pats, n_pat, repeats):
    pix.seeds(warm(pats), min_length=12, max_per_seed=CAP)
    ms = [round(pix.seeds(pats, min_length=12, max_per_seed=CAP).search_ms, 3) for _ in range(repeats)]
    print(json.dumps({"workload": name, "batch": batch, "text_len": pix.text_length(), "reads": int(n_pat),
                      "seeds_search_ms": ms}), flush=True)


def run(eng, name, msa, a, rng):
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    pats = sample_patterns(rng, msa, a.patterns)
    two = two_substitutions(np.random.default_rng(2028), sample_patterns(np.random.default_rng(2029), msa, a.patterns, mutated=0.0))
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b) as pix:
        for batch, p in (("one_in_ten", pats), ("two_each", two)):
            (seeds_only if a.seeds_only else rows)(pix, name, batch, p, a.patterns, a.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seeds-only", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
