"""Pattern index of a founder graph on one MI355X: build and batched search (fbg_pindex_*, csrc/locate.hip).

Two MSAs are segmented (elastic min-max-length) on the GPU and turned into their founder graphs:
  c3     the BASELINE C3 generator (iid ACGT, "ACGT"[splitmix64 >> 62] via fbg_msa_synthetic's formula is not needed
         here: numpy iid bytes), 1000 rows x --c3-cols columns (default a 100,000-column prefix of C3)
  star   a star phylogeny: 1000 noisy copies (p = 0.01) of one ancestor, 2 % gap cells in runs of 8, --star-cols
Then 10^6 patterns of length 100 are sampled from gap-stripped rows, 10 % of them with one substitution, and searched
in one fbg_pindex_locate call (one warm-up call first).  One JSON line per run:
  text_len (N + 1), index_bytes (occ lines + counts + B / E + tables), build_ms (host wall time of fbg_pindex_build
  with its uploads), search_ms (device time: length sort + search kernel), search_call_ms (host wall time of the
  call including copies), patterns_per_s and chars_per_s (from search_ms), occ_lines_per_char.
Usage: python scripts/gpu_locate_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def c3_msa(rng, m, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, n), dtype=np.uint8)]


def star_msa(rng, m, n, p=0.01, gap_frac=0.02, run=8):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = np.tile(acgt[rng.integers(0, 4, n, dtype=np.uint8)], (m, 1))
    mut = rng.random((m, n), dtype=np.float32) < p
    a[mut] = acgt[rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)]
    start = rng.random((m, n), dtype=np.float32) < gap_frac / run
    gap = start.copy()
    for k in range(1, run):
        gap[:, k:] |= start[:, :-k]
    a[gap] = ord("-")
    return a


def sample_patterns(rng, msa, count, length=100, mutated=0.10):
    rows = [r[r != ord("-")] for r in msa]
    rows = [r for r in rows if len(r) >= length]
    base = np.cumsum([0] + [len(r) for r in rows])
    flat = np.concatenate(rows)
    ri = rng.integers(0, len(rows), count)
    st = (rng.random(count) * (base[ri + 1] - base[ri] - length + 1)).astype(np.int64) + base[ri]
    pats = flat[st[:, None] + np.arange(length)[None, :]]
    mut = np.nonzero(rng.random(count) < mutated)[0]
    pats[mut, rng.integers(0, length, len(mut))] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(mut))]
    off = np.arange(count + 1, dtype=np.uint64) * length
    return np.ascontiguousarray(pats).ravel(), off


def run(eng, name, msa, n_pat, rng):
    import founderblockgraphs_amd as F
    t0 = time.perf_counter()
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(eng, msa, b, packed=True)
    t_graph = time.perf_counter() - t0
    data, off = sample_patterns(rng, msa, n_pat)
    with eng.pattern_index(labels, edges) as pix:
        st_build = pix.stats()
        pix.locate((data[:off[1000]], off[:1001]))               # warm-up: code objects, rocPRIM
        t1 = time.perf_counter()
        count, pos = pix.locate((data, off))
        call_ms = (time.perf_counter() - t1) * 1e3
        st = pix.stats()
        out = {
            "workload": name, "rows": int(msa.shape[0]), "cols": int(msa.shape[1]), "blocks": int(len(b)),
            "nodes": int(len(labels[1]) - 1), "edges": int(len(edges)), "text_len": pix.text_length(),
            "index_bytes": st_build["index_bytes"], "index_bytes_per_symbol": round(st_build["index_bytes"] / pix.text_length(), 3),
            "build_ms": round(st_build["build_ms"], 2), "patterns": int(n_pat), "pattern_len": 100,
            "search_ms": round(st["search_ms"], 3), "search_call_ms": round(call_ms, 2),
            "patterns_per_s": round(n_pat / (st["search_ms"] / 1e3)), "chars_per_s": round(len(data) / (st["search_ms"] / 1e3)),
            "occ_lines_per_char": round(st["occ_lines"] / len(data), 3),
            "found": int((count > 0).sum()), "mean_pos": round(float(pos.mean()), 2), "graph_s": round(t_graph, 2),
        }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a.patterns, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a.patterns, rng)


if __name__ == "__main__":
    main()
