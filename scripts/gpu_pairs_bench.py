"""Paired reads on one MI355X: fbg_pindex_chains_pairs (start columns, the span and window kernels, the binning, the three
tiers of k_pc_chain, trace, scan, trace, the rescue spans, the pick; with adopt also the two adopt kernels and one more
trace, scan, trace) beside fbg_pindex_chains on the same seeds, csrc/pindex_pairs.hip.

A star phylogeny at 1 % with gap runs (scripts/gpu_locate_bench.py, star_msa), --rows x --cols.  --pairs (100,000) pairs
of 100-symbol mates from fragments of 300 .. 500 gap-stripped symbols of a row, one mate in ten with a substitution, the
second mate reverse-complemented: 2 x --pairs given reads, twice as many virtual ones.  One seeds call (min_length 12, cap
64, both strands), a warm-up, then --repeats (5) timed rounds of chains -> pairs -> chains -> pairs with adopt; device times
lie between hipEvents inside the library.  One JSON line:
  chain_ms        fbg_pindex_chains                                  [median, min, max]
  pairs_ms        fbg_pindex_chains_pairs without adopt
  adopt_ms        fbg_pindex_chains_pairs with adopt
  ratio, ratio_adopt   the medians over the median chain_ms
  which0 .. rescue_differs   stats[] of the call
The pairs call repeats the chain call's sort, its host look at the tier sizes and its DP on the kept places, and adds
linear kernels: a ratio well above 2 is a reason to look at the window and span kernels.
Usage: python scripts/gpu_pairs_bench.py [--pairs 100000] [--rows 1000] [--cols 200000] [--insert 0,600]
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
from gpu_seeds_bench import mmm  # noqa: E402

CAP, MIN_LENGTH, READ = 64, 12, 100
COMP = np.arange(256, dtype=np.uint8)
for x, y in zip(b"ACGT", b"TGCA"):
    COMP[x] = y


def sample_pairs(rng, msa, count):
    """(uint8 data, uint64 offsets) of 2 x count reads: per pair the first READ symbols of a fragment of 300 .. 500
    symbols of a row's gap-stripped text, and the reverse complement of its last READ."""
    rows = [r[r != ord("-")] for r in msa]
    rows = [r for r in rows if len(r) >= 500]
    base = np.cumsum([0] + [len(r) for r in rows])
    flat = np.concatenate(rows)
    ri = rng.integers(0, len(rows), count)
    frag = rng.integers(300, 501, count)
    st = (rng.random(count) * (base[ri + 1] - base[ri] - frag + 1)).astype(np.int64) + base[ri]
    first = flat[st[:, None] + np.arange(READ)[None, :]]
    last = COMP[flat[(st + frag - READ)[:, None] + np.arange(READ)[None, :]]][:, ::-1]
    data = np.stack((first, last), axis=1)
    data[1::2] = data[1::2, ::-1]                     # every other pair gives its reverse mate first
    data = data.reshape(2 * count, READ).copy()
    mut = np.nonzero(rng.random(2 * count) < 0.10)[0]
    data[mut, rng.integers(0, READ, len(mut))] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(mut))]
    return np.ascontiguousarray(data).ravel(), np.arange(2 * count + 1, dtype=np.uint64) * READ


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
        pats = sample_pairs(rng, msa, a.pairs)
        eng.msa_load_host(msa)
        with eng.pattern_index_of_segmentation(b) as pix:
            sd = pix.seeds(pats, min_length=MIN_LENGTH, max_per_seed=CAP, strands=True)
            pix.chains(pairs=ins, adopt_pairs=True)
            c_ms, p_ms, a_ms = [], [], []
            for _ in range(a.repeats):
                plain = pix.chains(pairs=ins)
                c_ms.append(plain.device_ms)
                p_ms.append(plain.pairs_ms)
                a_ms.append(pix.chains(pairs=ins, adopt_pairs=True).pairs_ms)
            med = max(float(np.median(c_ms)), 1e-9)
            print(json.dumps({
                "workload": "star_gaps", "rows": a.rows, "cols": a.cols, "text_len": pix.text_length(), "pairs": a.pairs,
                "reads": 2 * a.pairs, "read_len": READ, "min_length": MIN_LENGTH, "cap": CAP, "insert": list(ins), "seeds": len(sd),
                "start_places": int(sd.occ.start_off[-1]), "chain_ms": mmm(c_ms), "pairs_ms": mmm(p_ms), "adopt_ms": mmm(a_ms),
                "ratio": round(float(np.median(p_ms)) / med, 3), "ratio_adopt": round(float(np.median(a_ms)) / med, 3),
                "runs": a.repeats, **plain.pair_stats, "rescue_entries": int(plain.rescue_off[-1]),
            }), flush=True)


if __name__ == "__main__":
    main()
