"""The second-best chain and the mapping quality on one MI355X: fbg_pindex_chains_mapq (start columns, the span and mask
kernels, the binning, the three tiers of k_pc_chain, trace, scan, trace, the final kernel) beside fbg_pindex_chains on
the same seeds, csrc/pindex_mapq.hip.

The graphs, read batches, minimum lengths, cap and band of scripts/gpu_chains_bench.py.  Every row is one warm-up and
--repeats (5) timed rounds of seeds -> chains -> mapq (margin --margin, default 0); device times lie between hipEvents
inside the library.  One JSON line per row:
  chain_ms    fbg_pindex_chains                                  [median, min, max]
  mapq_ms     fbg_pindex_chains_mapq
  ratio       median mapq_ms / median chain_ms
  reads_with_second, anchors_kept, anchors_excluded, mapq0, mapq60   fbg_pindex_mapq_stats
  second_entries                                                 entries of the secondary chains in all
The mapq call repeats the chain call's sort, its host look at the tier sizes and its DP on the kept anchors, and adds
linear kernels: a ratio well above 2 is a reason to look at the mask and span kernels.  The chain call's figure on a parent
commit comes from scripts/gpu_chains_bench.py in a built checkout of that commit (chain_ms of the same rows).
Usage: python scripts/gpu_mapq_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--margin 0]
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


def rows(pix, name, batch, pats, n_pat, repeats, margin):
    for L in (1, 12):
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, mapq=True, mapq_margin=margin)
        c_ms, q_ms = [], []
        for _ in range(repeats):
            res = pix.seeds(pats, min_length=L, max_per_seed=CAP, chain=True, mapq=True, mapq_margin=margin)
            c_ms.append(res.chains.device_ms)
            q_ms.append(res.chains.mapq_ms)
        st = pix.mapq_stats()
        print(json.dumps({
            "workload": name, "batch": batch, "text_len": pix.text_length(), "reads": int(n_pat), "read_len": 100,
            "min_length": L, "cap": CAP, "margin": margin, "seeds": len(res), "start_places": int(res.occ.start_off[-1]),
            "chain_ms": mmm(c_ms), "mapq_ms": mmm(q_ms), "ratio": round(float(np.median(q_ms) / max(np.median(c_ms), 1e-9)), 3),
            "runs": repeats, **st, "second_entries": int(res.chains.second_off[-1]),
        }), flush=True)


def run(eng, name, msa, a, rng):
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    pats = sample_patterns(rng, msa, a.patterns)
    two = two_substitutions(np.random.default_rng(2028), sample_patterns(np.random.default_rng(2029), msa, a.patterns, mutated=0.0))
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b) as pix:
        for batch, p in (("one_in_ten", pats), ("two_each", two)):
            rows(pix, name, batch, p, a.patterns, a.repeats, a.margin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--margin", type=int, default=0)
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
