"""Paired reads, a seedless mate rescued by alignment, on one MI355X: fbg_pindex_pairs_align (the row choice, the fragment
ends, the windows and their start search, the scan, the gather, the bit-vector recurrence over every window, the pick)
beside fbg_pindex_chains_pairs and fbg_pindex_chains_align in the same run, csrc/pindex_pairs_align.hip.

The input of scripts/gpu_pairs_bench.py: a star phylogeny at 1 % with gap runs, --rows x --cols, and --pairs (100,000)
pairs of 100-symbol mates from fragments of 300 .. 500 gap-stripped symbols of a row, the second mate
reverse-complemented.  Here the second given read of every pair gets a substitution every 6 symbols, so no stretch of it
reaches min_length 12 and it has no seed where it comes from.  In a text of some 4 x 10^8 symbols a 12-mer also occurs by
chance, so most damaged reads still get a short chain somewhere else (damaged_with_chain counts them), and the default
selection, reads without a chain, would pass them over: the call is given a mask of the damaged reads, both strands, and
aligns each in the window of --insert symbols that its mate's chain opens.  One seeds call, a warm-up, then --repeats (5)
timed rounds; device times lie between hipEvents inside the library.  One JSON line:
  chain_ms, pairs_ms   fbg_pindex_chains, fbg_pindex_chains_pairs without adopt          [median, min, max]
  align_ms             fbg_pindex_chains_align (pad 16) on the same chains
  pair_align_ms        fbg_pindex_pairs_align
  align_gcells_s, pair_align_gcells_s   cells of either call over its median time, in 10^9 cells per second
  pairs_with_chain_candidate   pairs that fbg_pindex_chains_pairs found a candidate for
  damaged_with_chain, edits_median   damaged virtual reads with a chain of their own; the median edits of the accepted reads
  stats                stats[] of the new call
Both align calls run the same recurrence: a rate of the new call far below the align call's points at the new prepare and
gather work, not at the recurrence.  (The align call's windows are a read and two pads long, the new call's an insert long:
its reads stay in registers over many more columns.)
Usage: python scripts/gpu_pair_align_bench.py [--pairs 100000] [--rows 1000] [--cols 200000] [--insert 0,600]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_locate_bench import star_msa  # noqa: E402
from gpu_pairs_bench import CAP, MIN_LENGTH, READ, sample_pairs  # noqa: E402
from gpu_seeds_bench import mmm  # noqa: E402

EVERY = 6


def damage(rng, data):
    """A substitution at every EVERY-th symbol, from the third on, of the second given read of every pair."""
    reads = data.reshape(-1, READ)
    at = np.arange(2, READ, EVERY)
    old = reads[1::2][:, at]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    new = letters[rng.integers(0, 4, old.shape)]
    clash = new == old
    new[clash] = letters[(np.searchsorted(letters, old[clash]) + 1) % 4]
    reads[1::2, at] = new
    return reads.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--insert", default="0,600")
    a = ap.parse_args()
    ins = tuple(int(x) for x in a.insert.split(","))
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2030)
    with F.Engine(0) as eng:
        msa = star_msa(rng, a.rows, a.cols)
        b = eng.minmax_dp(eng.elastic_f(msa))
        data, off = sample_pairs(rng, msa, a.pairs)
        pats = (damage(rng, data.copy()), off)
        eng.msa_load_host(msa)
        with eng.pattern_index_of_segmentation(b, rows=True) as pix:
            sd = pix.seeds(pats, min_length=MIN_LENGTH, max_per_seed=CAP, strands=True)
            n = 2 * a.pairs
            select = np.zeros(2 * n, dtype=np.uint8)
            select[1:n:2] = select[n + 1::2] = 1
            pix.chains(pairs=ins, align=True, pair_align=True, pair_select=select)
            c_ms, p_ms, g_ms, m_ms = [], [], [], []
            for _ in range(a.repeats):
                ch = pix.chains(pairs=ins, align=True, pair_align=True, pair_select=select)
                c_ms.append(ch.device_ms)
                p_ms.append(ch.pairs_ms)
                g_ms.append(ch.align_ms)
                m_ms.append(ch.mate_ms)
            cells = pix.align_stats()["cells"]
            rate = lambda c, ms: round(c / max(float(np.median(ms)), 1e-9) / 1e6, 2)      # noqa: E731
            print(json.dumps({
                "workload": "star_gaps", "rows": a.rows, "cols": a.cols, "text_len": pix.text_length(), "pairs": a.pairs,
                "reads": 2 * a.pairs, "read_len": READ, "every": EVERY, "min_length": MIN_LENGTH, "cap": CAP, "insert": list(ins),
                "seeds": len(sd), "chain_ms": mmm(c_ms), "pairs_ms": mmm(p_ms), "align_ms": mmm(g_ms), "pair_align_ms": mmm(m_ms),
                "align_cells": cells, "align_gcells_s": rate(cells, g_ms), "pair_align_gcells_s": rate(ch.mate_stats["cells"], m_ms),
                "pairs_with_chain_candidate": int((ch.pair_which != 0xff).sum()), "runs": a.repeats,
                "damaged_with_chain": int((np.diff(ch.chain_off.astype(np.int64))[select != 0] > 0).sum()),
                "edits_median": int(np.median(ch.mate_edits[ch.mate_insert != 0xffffffff])) if ch.mate_stats["pairs"] else None,
                "stats": ch.mate_stats,
            }), flush=True)


if __name__ == "__main__":
    main()
