"""The alignment path of each read against the stretch of the graph its path spells on one MI355X:
fbg_pindex_chains_graph_cigar beside the graph alignment it follows, csrc/pindex_gcigar.hip.

The workload and the read selection of scripts/gpu_graph_align_bench.py: the star_gaps graph, 20,000 edited reads of 150
symbols (three planted edits), chained by row and aligned against their rows; the graph alignment takes the reads that
alignment left with more than the planted edits and the reads without a row, and the CIGAR is traced for the reads it
aligned.  One warm-up and --repeats (5) timed rounds of seeds -> chains_by_row -> chains_align -> chains_align_graph ->
chains_graph_cigar; device times lie between hipEvents inside the library.  One JSON line per graph:
  graph_ms, graph_cigar_ms                  fbg_pindex_chains_align_graph, _chains_graph_cigar [median, min, max]
  selected                                  the reads the mask names
  paths .. batches                          fbg_pindex_graph_cigar_stats
  cigar_cells                               the sum of L * N over the traced reads, the work of the trace
  graph_cells                               cells of fbg_pindex_align_graph_stats, the work of the graph call
  cigar_share                               median graph_cigar_ms / median graph_ms
  with_indel                                traced reads whose path holds an I or a D
Usage: python scripts/gpu_graph_cigar_bench.py [--patterns 20000] [--rows 1000] [--star-cols 200000] [--c3] [--c3-cols 100000]
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
from gpu_graph_align_bench import NONE, PLANTED  # noqa: E402
from gpu_locate_bench import c3_msa, star_msa  # noqa: E402
from gpu_seeds_bench import mmm, warm  # noqa: E402


def run(eng, name, msa, a, rng):
    b = eng.minmax_dp(eng.elastic_f(msa))
    pats = edited_reads(rng, msa, a.patterns)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b, rows=True) as pix:
        pix.seeds(warm(pats), min_length=L, max_per_seed=CAP)
        pix.chains(by_row=True, align=True, pad=PAD, graph=True, graph_pad=PAD, graph_cigar=True)
        t = {k: [] for k in ("graph_ms", "graph_cigar_ms")}
        for _ in range(a.repeats):
            pix.seeds(pats, min_length=L, max_per_seed=CAP)
            ch = pix.chains(by_row=True, align=True, pad=PAD)
            sel = (ch.edits == NONE) | (ch.edits > PLANTED)
            gr = pix.chains(by_row=True, align=True, pad=PAD, graph=True, graph_pad=PAD, select=sel, graph_cigar=True)
            t["graph_ms"].append(gr.graph_ms)
            t["graph_cigar_ms"].append(gr.graph_cigar_ms)
        st, gs = pix.graph_cigar_stats(), pix.graph_align_stats()
        code, length = gr.graph_cigar_ops & 15, (gr.graph_cigar_ops >> 4).astype(np.int64)
        read_of = np.repeat(np.arange(len(gr.graph_cigar_off) - 1), np.diff(gr.graph_cigar_off.astype(np.int64)))
        cols = np.bincount(read_of, weights=np.where((code == 2) | (code == 7) | (code == 8), length, 0), minlength=len(pats))
        out = {"workload": name, "blocks": len(b), "rows": int(msa.shape[0]), "reads": int(a.patterns), "read_len": READ, "pad": PAD,
               "min_length": L, "cap": CAP, "selected": int(sel.sum()), **st, "cigar_cells": int(cols.sum()) * READ, "graph_cells": gs["cells"],
               "with_indel": int(len(np.unique(read_of[(code == 1) | (code == 2)]))), "path_batch_kib": eng.get_option("path_batch_kib")}
        out.update({k: mmm(v) for k, v in t.items()})
        out["cigar_share"] = round(float(np.median(t["graph_cigar_ms"]) / np.median(t["graph_ms"])), 5) if np.median(t["graph_ms"]) else 0
        assert int(cols.sum()) == st["columns"]
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
