"""MSA rows and columns of reported places, on one MI355X: fbg_pindex_occurrences_msa (k_po_expand_msa) beside
fbg_pindex_occurrences_fetch (k_po_expand) on the same search, csrc/locate.hip.

The two graphs and the batches of scripts/gpu_occurrences_bench.py (same generators, same seeds), the index built by
fbg_pindex_build_segmentation.  Every row is one warm-up and --repeats (5) timed rounds of search, fetch and coordinates;
device times lie between hipEvents inside the library, without the copies.  One JSON line per row:
  fetch_ms / msa_ms   [median, min, max] of the two expansions; ratio = median msa_ms / median fetch_ms
  places              ends + starts reported
  map_bytes, gapped_nodes, sample_columns   fbg_pindex_msa_stats
--paths-only prints instead, per graph, one line with build_ms of fbg_pindex_build_segmentation, --repeats values of
fbg_pindex_locate's search_ms and of fbg_segmentation_repair's device_ms: the figures two checkouts are compared on, run
in alternating processes (it uses no call this commit adds).
Usage: python scripts/gpu_msa_coords_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--paths-only]
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
from gpu_occurrences_bench import mmm  # noqa: E402


def rows(pix, name, pats, n_pat, length, caps, repeats):
    st = pix.msa_stats()
    for cap in caps:
        pix.occurrences((pats[0][:pats[1][1000]], pats[1][:1001]), max_per_pattern=cap, msa=True)      # warm-up
        f_ms, m_ms = [], []
        for _ in range(repeats):
            res = pix.occurrences(pats, max_per_pattern=cap, msa=True)
            f_ms.append(res.fetch_ms)
            m_ms.append(res.msa_ms)
        places = int(res.end_off[-1] + res.start_off[-1])
        print(json.dumps({
            "workload": name, "text_len": pix.text_length(), "patterns": int(n_pat), "pattern_len": length, "cap": cap,
            "fetch_ms": mmm(f_ms), "msa_ms": mmm(m_ms), "ratio": round(float(np.median(m_ms) / max(np.median(f_ms), 1e-9)), 3),
            "places": places, "sentinels": int((res.end_row == 0xffffffff).sum() + (res.start_row == 0xffffffff).sum()), **st,
        }), flush=True)


def run(eng, name, msa, a, rng):
    f = eng.elastic_f(msa)
    b = eng.minmax_dp(f)
    pats = sample_patterns(rng, msa, a.patterns)
    short = sample_patterns(np.random.default_rng(2027), msa, a.patterns // 10, length=12)
    eng.msa_load_host(msa)
    with eng.pattern_index_of_segmentation(b) as pix:
        if a.paths_only:
            out = {"workload": name, "text_len": pix.text_length(), "blocks": len(b), "build_ms": round(pix.stats()["build_ms"], 3)}
            pix.locate((pats[0][:pats[1][1000]], pats[1][:1001]))
            ms = []
            for _ in range(a.repeats):
                pix.locate(pats)
                ms.append(round(pix.stats()["search_ms"], 3))
            out["locate_search_ms"] = ms
        else:
            rows(pix, name, pats, a.patterns, 100, (1, 64), a.repeats)
            rows(pix, name, short, a.patterns // 10, 12, (64, 1024), a.repeats)
            return
    # the repair loop on every second boundary of the segmentation (blocks twice as wide, some of them invalid)
    rep = []
    for _ in range(a.repeats + 1):
        t = {}
        eng.repair_segmentation(np.concatenate((b[:-1][1::2], b[-1:])), timing=t)
        rep.append(round(t["device_ms"], 3))
    out["repair_device_ms"] = rep[1:]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths-only", action="store_true")
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
