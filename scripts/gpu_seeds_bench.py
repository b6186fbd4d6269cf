"""Maximal exact-match seeds on one MI355X: fbg_pindex_seeds (two walks, scan, sizes), fbg_pindex_seeds_fetch and
fbg_pindex_seeds_places, csrc/locate.hip.

The two graphs and the 10^6 reads of 100 symbols of scripts/gpu_locate_bench.py (same generators, same seed; 10 % of the
reads carry one substitution: batch "one_in_ten"), and a second batch in which every read carries two substitutions
("two_each").  Minimum lengths 1 and 12, caps 0 and 64.  Every row is one warm-up call and --repeats (5) timed calls;
device times lie between hipEvents inside the library (search_ms: fbg_pindex_seeds; fetch_ms: the per-seed copies and the
expansion kernels).  One JSON line per row:
  seeds                 reported seeds;  seeded: reads with one or more;  restarted: seeds found after a restart
  search_ms / fetch_ms  [median, min, max]
  reads_per_s           from the median search_ms
  places                ends + starts reported
  call_ms               host wall time of PatternIndex.seeds (three calls, copies and host arrays), median
--baseline prints, per graph and batch, --repeats values of fbg_pindex_locate's search_ms and of
fbg_pindex_occurrences' search_ms (cap 0) instead (after one warm-up each): the figures a parent commit is compared on.
This mode calls nothing the seeds calls added, but the package binds every entry point it lists when it loads the
library, so this tree's package does not load a parent's library: for the parent's figures copy this file into
scripts/ of a built checkout of the parent and run it there (it imports the package of the tree it lies in).
Usage: python scripts/gpu_seeds_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--baseline]
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

from gpu_locate_bench import c3_msa, sample_patterns, star_msa  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def mmm(xs):
    return [round(float(np.median(xs)), 3), round(float(min(xs)), 3), round(float(max(xs)), 3)]


def two_substitutions(rng, pats, length=100):
    """Every read of the batch with two symbols replaced by other ones, at two different positions."""
    data = pats[0].reshape(-1, length).copy()
    n = len(data)
    a = rng.integers(0, length, n)
    b = (a + rng.integers(1, length, n)) % length
    for at in (a, b):
        old = data[np.arange(n), at]
        new = ACGT[rng.integers(0, 4, n)]
        same = new == old
        new[same] = ACGT[(np.searchsorted(ACGT, old[same]) + 1) % 4]
        data[np.arange(n), at] = new
    return np.ascontiguousarray(data).ravel(), pats[1]


def warm(pats):
    return pats[0][:pats[1][1000]], pats[1][:1001]


def rows(pix, name, batch, pats, n_pat, repeats):
    for L in (1, 12):
        for cap in (0, 64):
            pix.seeds(warm(pats), min_length=L, max_per_seed=cap)
            s_ms, f_ms, c_ms = [], [], []
            for _ in range(repeats):
                t0 = time.perf_counter()
                res = pix.seeds(pats, min_length=L, max_per_seed=cap)
                c_ms.append((time.perf_counter() - t0) * 1e3)
                s_ms.append(res.search_ms)
                f_ms.append(res.fetch_ms)
            print(json.dumps({
                "workload": name, "batch": batch, "text_len": pix.text_length(), "reads": int(n_pat), "read_len": 100,
                "min_length": L, "cap": cap, "seeds": len(res), "seeded": int((np.diff(res.seed_off.astype(np.int64)) > 0).sum()),
                "restarted": int((res.occ.restarts > 0).sum()), "search_ms": mmm(s_ms), "fetch_ms": mmm(f_ms),
                "reads_per_s": round(n_pat / (np.median(s_ms) / 1e3)),
                "places": int(res.occ.end_off[-1] + res.occ.start_off[-1]), "call_ms": round(float(np.median(c_ms)), 1),
            }), flush=True)


def baseline(pix, name, batch, pats, n_pat, repeats):
    pix.locate(warm(pats))
    loc = []
    for _ in range(repeats):
        pix.locate(pats)
        loc.append(round(pix.stats()["search_ms"], 3))
    pix.occurrences(warm(pats), max_per_pattern=0)
    occ = [round(pix.occurrences(pats, max_per_pattern=0).search_ms, 3) for _ in range(repeats)]
    print(json.dumps({"workload": name, "batch": batch, "text_len": pix.text_length(), "reads": int(n_pat),
                      "locate_search_ms": loc, "occurrences_search_ms": occ}), flush=True)


def run(eng, name, msa, a, rng):
    import founderblockgraphs_amd as F
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(eng, msa, b, packed=True)
    pats = sample_patterns(rng, msa, a.patterns)
    two = two_substitutions(np.random.default_rng(2028), sample_patterns(np.random.default_rng(2029), msa, a.patterns, mutated=0.0))
    with eng.pattern_index(labels, edges) as pix:
        for batch, p in (("one_in_ten", pats), ("two_each", two)):
            (baseline if a.baseline else rows)(pix, name, batch, p, a.patterns, a.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
