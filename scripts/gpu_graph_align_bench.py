"""The edit distance of each read to a path of the graph around its chain on one MI355X: fbg_pindex_chains_align_graph
beside the row alignment it follows, csrc/pindex_graph.hip.

The star_gaps graph and the edited reads of scripts/gpu_align_bench.py (150 symbols, two substitutions and one inserted
or deleted symbol each: three planted edits), 20,000 of them by default: on 1000 similar rows a block holds about 900
nodes and a read costs 900 times the cells of its row alignment; minimum seed length 12, cap 64, unbounded band, pad 16,
no cell limit.
The reads are chained by row and aligned against their rows; the graph alignment then takes the reads that alignment
left with more than the planted edits and the reads without a row, which is the intended use of its select mask.  One
warm-up and --repeats (5) timed rounds of seeds -> chains_by_row -> chains_align -> chains_align_graph; device times lie
between hipEvents inside the library.  One JSON line per graph:
  search_ms, chain_ms, align_ms, graph_ms   fbg_pindex_seeds, _chains_by_row, _chains_align, _chains_align_graph
                                            [median, min, max]
  selected                                  the reads the mask names
  aligned .. batches                        fbg_pindex_align_graph_stats
  graph_cells_per_s, align_cells_per_s      cells / median time of either call on the same run (a graph cell is one
                                            (read symbol, label symbol of the window's nodes) pair)
  improved                                  selected reads with graph edits below their row edits
Usage: python scripts/gpu_graph_align_bench.py [--patterns 20000] [--rows 1000] [--star-cols 200000] [--c3] [--c3-cols 100000]
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

PLANTED, NONE = 3, 0xffffffff


def run(eng, name, msa, a, rng):
    b = eng.minmax_dp(eng.elastic_f(msa))
    pats = edited_reads(rng, msa, a.patterns)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b, rows=True) as pix:
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP)
        pix.chains(by_row=True, align=True, pad=PAD, graph=True, graph_pad=PAD)
        t = {k: [] for k in ("search_ms", "chain_ms", "align_ms", "graph_ms")}
        for _ in range(a.repeats):
            res = pix.seeds(pats, min_length=L, max_per_seed=CAP)
            ch = pix.chains(by_row=True, align=True, pad=PAD)
            sel = (ch.edits == NONE) | (ch.edits > PLANTED)
            gr = pix.chains(by_row=True, align=True, pad=PAD, graph=True, graph_pad=PAD, select=sel)
            t["search_ms"].append(res.search_ms)
            t["chain_ms"].append(gr.device_ms)
            t["align_ms"].append(gr.align_ms)
            t["graph_ms"].append(gr.graph_ms)
        st, at = pix.graph_align_stats(), pix.align_stats()
        both = sel & (gr.graph_edits != NONE) & (gr.edits != NONE)
        out = {"workload": name, "blocks": len(b), "rows": int(msa.shape[0]), "reads": int(a.patterns), "read_len": READ, "pad": PAD,
               "min_length": L, "cap": CAP, "selected": int(sel.sum()), **st, "align_cells": at["cells"],
               "improved": int((gr.graph_edits[both] < gr.edits[both]).sum()), "graph_batch_kib": eng.get_option("graph_batch_kib")}
        out.update({k: mmm(v) for k, v in t.items()})
        out["graph_cells_per_s"] = round(st["cells"] / (np.median(t["graph_ms"]) / 1e3)) if st["cells"] else 0
        out["align_cells_per_s"] = round(at["cells"] / (np.median(t["align_ms"]) / 1e3)) if at["cells"] else 0
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=20_000)
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
