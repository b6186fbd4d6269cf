"""Semi-repeat-free check of a founder graph on one MI355X (fbg_pindex_validate, csrc/pindex_validate.hip).

The two graphs of scripts/gpu_locate_bench.py (c3: iid ACGT, 1000 rows x --c3-cols; star: 1000 noisy copies of one
ancestor with 2 % gap cells in runs of 8, --star-cols), each in two segmentations:
  dp      the project's own elastic min-max-length segmentation (what founderblockgraph writes)
  random  the same number of blocks at random boundaries (a graph with INVALID nodes: the early exit at work)
Per graph one JSON line: nodes, edges, text_len, the node counts per status, slots_scanned (SA slots read),
wave_nodes (ranges of more than 16 slots, one wave each), table_bytes (what the build keeps for validation),
validate_ms (device time of the validation kernels: median of --runs calls after one warm-up call) with its
min / max, and validate_call_ms (host wall time of the median call, copies included).
Usage: python scripts/gpu_validate_bench.py [--c3-cols 100000] [--star-cols 200000] [--runs 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_locate_bench import c3_msa, star_msa  # noqa: E402


def run(eng, name, msa, runs, rng):
    import founderblockgraphs_amd as F
    f = eng.elastic_f(msa)
    b_dp = eng.minmax_dp(f)
    n = msa.shape[1]
    cuts = np.sort(rng.choice(np.arange(0, n - 1), size=len(b_dp) - 1, replace=False))
    b_rand = np.concatenate([cuts, [n]]).astype(np.uint64)
    for seg, b in (("dp", b_dp), ("random", b_rand)):
        labels, edges, blocks = F.graph_from_segmentation(eng, msa, b, packed=True, with_blocks=True)
        with eng.pattern_index(labels, edges) as pix:
            pix.validate(blocks)                                   # warm-up: code objects
            ms, call = [], []
            for _ in range(runs):
                t0 = time.perf_counter()
                r = pix.validate(blocks)
                call.append((time.perf_counter() - t0) * 1e3)
                ms.append(r.device_ms)
            k = int(np.argsort(ms)[len(ms) // 2])
            tb = ctypes.c_uint64(0)
            pix._L.fbg_pindex_validate_stats(pix._h, None, None, ctypes.byref(tb))
            c = r.counts()
            out = {
                "workload": name, "segmentation": seg, "rows": int(msa.shape[0]), "cols": int(n), "blocks": int(len(b)),
                "nodes": int(len(labels[1]) - 1), "edges": int(len(edges)), "text_len": pix.text_length(),
                "checked": c["valid"] + c["invalid"], **c, "bad_cuts": int(len(r.bad_cuts)),
                "slots_scanned": int(r.slots_scanned), "wave_nodes": int(r.wave_nodes), "table_bytes": int(tb.value),
                "validate_ms": round(ms[k], 3), "validate_ms_min": round(min(ms), 3), "validate_ms_max": round(max(ms), 3),
                "validate_call_ms": round(call[k], 2),
            }
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a.runs, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a.runs, rng)


if __name__ == "__main__":
    main()
