"""Seeds and chains on both strands on one MI355X: PatternIndex.seeds(strands=True) + chains() (fbg_pindex_seeds_strands
with k_px_revcomp, fbg_pindex_chains over the 2n virtual reads, fbg_pindex_chain_strands with k_pc_strand) beside the
route a caller had before: reverse complement of every read with numpy on the host, one seeds() call on the 2n
concatenated reads, chains(), and the strand pick with numpy.  csrc/locate.hip.

The graphs of scripts/gpu_locate_bench.py, built through fbg_pindex_build_segmentation, and a batch of reads of 100
symbols sampled from the rows, one substitution in 10 % of them, every second read reverse-complemented.  Minimum
length 12, cap 64, unbounded band.  Both routes are checked to pick the same strand and score for every read.  Every
row is one warm-up and --repeats (5) rounds, the two routes in turns; one JSON line per graph:
  device_ms / host_route_device_ms   seeds + chains (+ strand pick on the device route): device time between hipEvents
                                     inside the library                               [median, min, max]
  wall_ms / host_route_wall_ms       host clock around the whole route, the fetches and, on the host route, the numpy
                                     passes (host_prepare_ms, host_pick_ms) included
  strand_ms                          fbg_pindex_chain_strands (k_pc_strand)
  revcomp_ms                         k_px_revcomp alone, as the device time of a stranded seeds call that reports nothing
                                     (min_length 2^32: upload, k_px_revcomp, length sort) less that of the same plain call
                                     on the 2n reads (upload, length sort): a difference of two medians
  forward / reverse / none           reads by outcome
Usage: python scripts/gpu_strands_bench.py [--patterns 1000000] [--c3-cols 100000] [--star-cols 200000] [--only c3|star_gaps]
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
from gpu_seeds_bench import mmm, warm  # noqa: E402

CAP, L = 64, 12


def host_revcomp(table, data, off):
    """(data, off) of the 2n virtual reads: the given reads, then rc of each, for reads of any lengths."""
    o = off.astype(np.int64)
    total = int(o[-1] - o[0])
    read = np.repeat(np.arange(len(o) - 1), np.diff(o))
    src = o[read] + o[read + 1] - 1 - (np.arange(total) + o[0])
    return np.concatenate((data[o[0]:o[-1]], table[data[src]])), np.concatenate((o - o[0], o[1:] - o[0] + total)).astype(np.uint64)


def device_route(pix, pats):
    t0 = time.perf_counter()
    sd = pix.seeds(pats, min_length=L, max_per_seed=CAP, chain=True, strands=True)
    wall = (time.perf_counter() - t0) * 1e3
    ch = sd.chains
    return dict(strand=ch.strand, score=ch.best_score, wall=wall, device=sd.search_ms + ch.device_ms + ch.strand_ms, pick=ch.strand_ms,
                counts=ch.strand_counts, seeds=len(sd))


def host_route(pix, table, pats):
    n = len(pats[1]) - 1
    t0 = time.perf_counter()
    both = host_revcomp(table, *pats)
    t1 = time.perf_counter()
    sd = pix.seeds(both, min_length=L, max_per_seed=CAP, chain=True)
    t2 = time.perf_counter()
    ch = sd.chains
    ln = np.diff(ch.chain_off.astype(np.int64))
    t = ch.score[n:] > ch.score[:n]
    strand = np.where(np.where(t, ln[n:], ln[:n]) > 0, t.astype(np.uint8), np.uint8(0xff))
    score = np.maximum(ch.score[:n], ch.score[n:])
    t3 = time.perf_counter()
    return dict(strand=strand, score=score, wall=(t3 - t0) * 1e3, device=sd.search_ms + ch.device_ms, prepare=(t1 - t0) * 1e3,
                pick=(t3 - t2) * 1e3, seeds=len(sd))


def run(eng, name, msa, a, rng):
    import founderblockgraphs_amd as F
    table = F.complement_table()
    b = eng.minmax_dp(eng.elastic_f(msa))
    data, off = sample_patterns(rng, msa, a.patterns)
    rows = data.reshape(-1, 100)
    rows[1::2] = table[rows[1::2, ::-1]]
    pats = (np.ascontiguousarray(rows).ravel(), off)
    eng.msa_load_host(msa)
    none = 1 << 32
    with eng.pattern_index_of_segmentation(b) as pix:
        device_route(pix, warm(pats))
        host_route(pix, table, warm(pats))
        dev, hst, rc_ms, plain_ms = [], [], [], []
        both = host_revcomp(table, *pats)
        for _ in range(a.repeats):
            dev.append(device_route(pix, pats))
            hst.append(host_route(pix, table, pats))
            rc_ms.append(pix.seeds(pats, min_length=none, strands=True).search_ms)
            plain_ms.append(pix.seeds(both, min_length=none).search_ms)
        d, h = dev[-1], hst[-1]
        assert np.array_equal(d["strand"], h["strand"]) and np.array_equal(d["score"], h["score"]) and d["seeds"] == h["seeds"]
        print(json.dumps({
            "workload": name, "text_len": pix.text_length(), "reads": int(a.patterns), "read_len": 100, "min_length": L, "cap": CAP,
            "seeds": d["seeds"], **d["counts"],
            "device_ms": mmm([x["device"] for x in dev]), "wall_ms": mmm([x["wall"] for x in dev]),
            "strand_ms": mmm([x["pick"] for x in dev]),
            "host_route_device_ms": mmm([x["device"] for x in hst]), "host_route_wall_ms": mmm([x["wall"] for x in hst]),
            "host_prepare_ms": mmm([x["prepare"] for x in hst]), "host_pick_ms": mmm([x["pick"] for x in hst]),
            "revcomp_ms": round(float(np.median(rc_ms) - np.median(plain_ms)), 3),
            "stranded_front_ms": mmm(rc_ms), "plain_front_ms": mmm(plain_ms),
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--c3-cols", type=int, default=100_000)
    ap.add_argument("--star-cols", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("c3", "star_gaps"))
    a = ap.parse_args()
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(2026)
    with F.Engine(0) as eng:
        if a.only != "star_gaps":
            run(eng, "c3", c3_msa(rng, a.rows, a.c3_cols), a, rng)
        if a.only != "c3":
            run(eng, "star_gaps", star_msa(rng, a.rows, a.star_cols), a, rng)


if __name__ == "__main__":
    main()
