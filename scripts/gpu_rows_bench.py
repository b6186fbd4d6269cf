"""The MSA rows that carry a start place and a chain on one MI355X: fbg_pindex_build_segmentation_rows,
fbg_pindex_seeds_rows and fbg_pindex_chains_rows beside the calls they follow, csrc/pindex_rows.hip.

The two graphs and the two read batches of scripts/gpu_chains_bench.py (10^6 reads of 100 symbols: "one_in_ten" with one
substitution in 10 % of the reads, "two_each" with two in every read), minimum length 12, cap 64, unbounded band.
Per graph one JSON line for the build: one warm-up and --repeats (5) builds with and without the row table,
  build_ms, rows_build_ms   fbg_pindex_stats' build_ms (the host's clock around the call, which ends synchronised)
                            [median, min, max]
  index_bytes, table_bytes  fbg_pindex_stats and fbg_pindex_rows_stats
and per batch one line, one warm-up and --repeats timed rounds of seeds -> chains -> seeds_rows -> chains_rows; device
times lie between hipEvents inside the library:
  search_ms        fbg_pindex_seeds          chain_ms         fbg_pindex_chains
  seeds_rows_ms    fbg_pindex_seeds_rows     chains_rows_ms   fbg_pindex_chains_rows
  start_places, places_unsupported, chained, chains_unsupported
--grouping measures the lane grouping on an MSA of 16 rows (the c3 generator, the one_in_ten batch): seeds_rows_ms and
chains_rows_ms with 16 lanes per place / chain (the default up to 16 rows) and, under option rows_wave, with a wave each.
--parent-compare prints, per graph, --repeats values of the plain build's build_ms and, per batch, of fbg_pindex_seeds'
search_ms (after one warm-up each) and uses nothing this feature added: the figures a parent commit is compared on.
The package binds every entry point it lists when it loads the library, so this tree's package does not load a
parent's library: for the parent's figures copy this file into scripts/ of a built checkout of the parent and run it
there with --parent-compare, the two in alternating processes.
Usage: python scripts/gpu_rows_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--parent-compare | --grouping]
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

CAP, L = 64, 12


def builds(eng, b, repeats, rows):
    """build_ms of one warm-up (dropped) and `repeats` builds; the last index's byte counts."""
    ms, sizes = [], {}
    for k in range(repeats + 1):
        with (eng.pattern_index_of_segmentation(b, rows=True) if rows else eng.pattern_index_of_segmentation(b)) as pix:
            st = pix.stats()
            sizes = {"index_bytes": st["index_bytes"], "text_len": pix.text_length()}
            if rows:
                sizes["table_bytes"] = pix.rows_stats()["table_bytes"]
            if k:
                ms.append(st["build_ms"])
    return ms, sizes


def batch_rows(pix, name, batch, pats, n_pat, repeats):
    pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, rows=True)
    t = {k: [] for k in ("search_ms", "chain_ms", "seeds_rows_ms", "chains_rows_ms")}
    for _ in range(repeats):
        res = pix.seeds(pats, min_length=L, max_per_seed=CAP, chain=True, rows=True)
        t["search_ms"].append(res.search_ms)
        t["chain_ms"].append(res.chains.device_ms)
        t["seeds_rows_ms"].append(res.rows_ms)
        t["chains_rows_ms"].append(res.chains.rows_ms)
    st = pix.rows_stats()
    out = {"workload": name, "batch": batch, "reads": int(n_pat), "read_len": 100, "min_length": L, "cap": CAP, "rows": st["rows"],
           "seeds": len(res), "start_places": int(res.occ.start_off[-1]), "places_unsupported": st["places_unsupported"],
           "chained": int((np.diff(res.chains.chain_off.astype(np.int64)) > 0).sum()), "chains_unsupported": st["chains_unsupported"]}
    out.update({k: mmm(v) for k, v in t.items()})
    print(json.dumps(out), flush=True)


def batch_parent(pix, name, batch, pats, n_pat, repeats):
    pix.seeds(warm(pats), min_length=L, max_per_seed=CAP)
    ms = [round(pix.seeds(pats, min_length=L, max_per_seed=CAP).search_ms, 3) for _ in range(repeats)]
    print(json.dumps({"workload": name, "batch": batch, "reads": int(n_pat), "seeds_search_ms": ms}), flush=True)


def run(eng, name, msa, a, rng):
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    pats = sample_patterns(rng, msa, a.patterns)
    two = two_substitutions(np.random.default_rng(2028), sample_patterns(np.random.default_rng(2029), msa, a.patterns, mutated=0.0))
    eng.msa_load_host(msa)
    plain, sizes = builds(eng, b, a.repeats, False)
    if a.parent_compare:
        print(json.dumps({"workload": name, "blocks": len(b), "plain_build_ms": [round(x, 3) for x in plain], **sizes}), flush=True)
        pix = eng.pattern_index_of_segmentation(b)
    else:
        with_rows, rsizes = builds(eng, b, a.repeats, True)
        print(json.dumps({"workload": name, "blocks": len(b), "build_ms": mmm(plain), "rows_build_ms": mmm(with_rows), **rsizes}),
              flush=True)
        pix = eng.pattern_index_of_segmentation(b, rows=True)
    with pix:
        for batch, p in (("one_in_ten", pats), ("two_each", two)):
            (batch_parent if a.parent_compare else batch_rows)(pix, name, batch, p, a.patterns, a.repeats)


def grouping(eng, a, rng):
    msa = c3_msa(rng, 16, a.c3_cols)
    b = eng.minmax_dp(eng.elastic_f(msa))
    pats = sample_patterns(rng, msa, a.patterns)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b, rows=True) as pix:
        for wave in (0, 1, 0, 1):
            eng.set_option("rows_wave", wave)
            pix.seeds(warm(pats), min_length=L, max_per_seed=CAP, chain=True, rows=True)
            p_ms, c_ms = [], []
            for _ in range(a.repeats):
                res = pix.seeds(pats, min_length=L, max_per_seed=CAP, chain=True, rows=True)
                p_ms.append(res.rows_ms)
                c_ms.append(res.chains.rows_ms)
            print(json.dumps({"workload": "c3_16_rows", "lanes": 64 if wave else 16, "reads": int(a.patterns),
                              "start_places": int(res.occ.start_off[-1]), "seeds_rows_ms": mmm(p_ms), "chains_rows_ms": mmm(c_ms)}),
                  flush=True)
        eng.set_option("rows_wave", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-compare", action="store_true")
    ap.add_argument("--grouping", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        if a.grouping:
            return grouping(eng, a, rng)
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
