"""Where patterns occur, on one MI355X: fbg_pindex_occurrences (search + sizes) and fbg_pindex_occurrences_fetch (the
expansion of SA ranges into places), csrc/locate.hip.

The two graphs and the 10^6 patterns of 100 symbols of scripts/gpu_locate_bench.py (same generators, same seed), with
caps of 1 and 64 places per pattern and list; then 10^5 patterns of 12 symbols, whose ranges are long, with caps of 64
and 1024.  Every row is one warm-up call and --repeats (5) timed calls; device times lie between hipEvents inside the
library (search_ms: length sort + walk + sizes + scans, fetch_ms: the two expansion kernels), without the copies.  One
JSON line per row:
  search_ms / fetch_ms  [median, min, max]
  places                ends + starts reported; places_per_s from the median fetch_ms
  found, restarted      patterns found, and found after one or more restarts
  call_ms               host wall time of PatternIndex.occurrences (both calls, copies and host arrays), median
--locate-only prints, per graph, --repeats values of fbg_pindex_locate's search_ms instead (after one warm-up): the
figure the parent commit is compared on.
Usage: python scripts/gpu_occurrences_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000]
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


def mmm(xs):
    return [round(float(np.median(xs)), 3), round(float(min(xs)), 3), round(float(max(xs)), 3)]


def rows(pix, name, pats, n_pat, length, caps, repeats):
    for cap in caps:
        pix.occurrences((pats[0][:pats[1][1000]], pats[1][:1001]), max_per_pattern=cap)      # warm-up
        s_ms, f_ms, c_ms = [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pix.occurrences(pats, max_per_pattern=cap)
            c_ms.append((time.perf_counter() - t0) * 1e3)
            s_ms.append(res.search_ms)
            f_ms.append(res.fetch_ms)
        places = int(res.end_off[-1] + res.start_off[-1])
        found = res.count > 0
        print(json.dumps({
            "workload": name, "text_len": pix.text_length(), "patterns": int(n_pat), "pattern_len": length, "cap": cap,
            "search_ms": mmm(s_ms), "fetch_ms": mmm(f_ms), "places": places,
            "places_per_s": round(places / (np.median(f_ms) / 1e3)) if places else 0,
            "end_total": int(res.end_total.sum()), "start_total": int(res.start_total.sum()),
            "found": int(found.sum()), "restarted": int((found & (res.restarts > 0)).sum()),
            "call_ms": round(float(np.median(c_ms)), 1),
        }), flush=True)


def run(eng, name, msa, a, rng):
    import founderblockgraphs_amd as F
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(eng, msa, b, packed=True)
    pats = sample_patterns(rng, msa, a.patterns)
    short = sample_patterns(np.random.default_rng(2027), msa, a.patterns // 10, length=12)    # rng: as gpu_locate_bench.py
    with eng.pattern_index(labels, edges) as pix:
        if a.locate_only:
            pix.locate((pats[0][:pats[1][1000]], pats[1][:1001]))
            ms = []
            for _ in range(a.repeats):
                pix.locate(pats)
                ms.append(round(pix.stats()["search_ms"], 3))
            print(json.dumps({"workload": name, "text_len": pix.text_length(), "patterns": a.patterns, "locate_search_ms": ms}),
                  flush=True)
            return
        rows(pix, name, pats, a.patterns, 100, (1, 64), a.repeats)
        rows(pix, name, short, a.patterns // 10, 12, (64, 1024), a.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--locate-only", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
