"""The second-best chain of every read and the mapping quality: the definitions of include/fbg_hip.h
(fbg_pindex_chains_mapq), statement by statement, on top of chain_model.

Inputs are what PatternIndex.seeds(msa=True) returns (seed_off, q_start, length, start_off, start_col), the lengths of
the (virtual) reads, and the primary chains as a chaining call reports them (chain_off, score, anchor_place,
anchor_seed): the model does not care whether fbg_pindex_chains or fbg_pindex_chains_by_row made them.  Python integers
throughout: nothing wraps.  The model is the checker of the kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import chain_model as CM

NONE = CM.NONE
U64_MAX = 2 ** 64 - 1


def span_of(anchors):
    """(lo, hi) of a chain given as [(g, t, q, k, c)] in read order, hi exclusive; None for an empty chain."""
    if not anchors:
        return None
    return anchors[0][4], anchors[-1][4] + anchors[-1][3]


def excluded(c, k, span, margin):
    """[c, c + k) meets [lo - margin, hi + margin)."""
    lo, hi = span
    return c + k + margin > lo and c < hi + margin


def kept_anchors(anchors, span, margin):
    """The anchors of a read that the widened span of its primary chain leaves; none without a primary chain."""
    if span is None:
        return []
    return [a for a in anchors if not excluded(a[4], a[3], span, margin)]


def secondary_of(anchors, span, band, margin):
    """(score, chain as a list of anchors, number of kept anchors) of the secondary chain: chain_model's chain on the kept
    anchors."""
    kept = kept_anchors(anchors, span, margin)
    score, idx = CM.chain_of(kept, band)
    return score, [kept[j] for j in idx], len(kept)


def mapq_of(s1, s2, L, primary):
    """60 * (s1 - min(s2, s1)) // L; 0 for an empty primary chain or an empty read."""
    if not primary or L == 0:
        return 0
    return (60 * (s1 - min(s2, s1))) // L


def mapq_stranded_of(s1, second, twin_score, L, primary):
    return mapq_of(s1, max(second, twin_score), L, primary)


def solve(seed_off, q_start, length, start_off, start_col, read_len, chain_off, score, anchor_place, anchor_seed, band, margin,
          stranded=False, cache=None):
    """-> a namespace of second_off, second, second_lo, second_hi, mapq, second_place, second_seed (NumPy arrays of the
    dtypes the engine returns), mapq_stranded (stranded: the reads are 2k virtual reads, the twin of v is v +- k), and
    the statistics of fbg_pindex_mapq_stats.  cache: a dict that keeps the secondary of (read, span, band, margin)
    between calls on the same seeds."""
    n = len(seed_off) - 1
    off, second, lo2, hi2, mq, place, seed = [0], [], [], [], [], [], []
    stats = dict(reads_with_second=0, anchors_kept=0, anchors_excluded=0, mapq0=0, mapq60=0)
    for r in range(n):
        a, b = int(chain_off[r]), int(chain_off[r + 1])
        prim = [(int(g), int(t), int(q_start[t]), int(length[t]), int(start_col[g])) for g, t in zip(anchor_place[a:b], anchor_seed[a:b])]
        span = span_of(prim)
        key = (r, span, band, margin)
        if cache is not None and key in cache:
            sc, sec, n_kept, n_all = cache[key]
        else:
            an = CM.read_anchors(seed_off, q_start, length, start_off, start_col, r) if span is not None else []
            sc, sec, n_kept = secondary_of(an, span, band, margin)
            n_all = len(an)
            if cache is not None:
                cache[key] = (sc, sec, n_kept, n_all)
        second.append(sc)
        s2 = span_of(sec)
        lo2.append(NONE if s2 is None else s2[0])
        hi2.append(NONE if s2 is None else s2[1])
        place += [x[0] for x in sec]
        seed += [x[1] for x in sec]
        off.append(len(place))
        q = mapq_of(int(score[r]), sc, int(read_len[r]), span is not None)
        mq.append(q)
        if span is not None:
            stats["anchors_kept"] += n_kept
            stats["anchors_excluded"] += n_all - n_kept
            stats["reads_with_second"] += sc > 0
            stats["mapq0"] += q == 0
            stats["mapq60"] += q == 60
    out = SimpleNamespace(second_off=np.array(off, dtype=np.uint64), second=np.array(second, dtype=np.uint32),
                          second_lo=np.array(lo2, dtype=np.uint32), second_hi=np.array(hi2, dtype=np.uint32),
                          mapq=np.array(mq, dtype=np.uint8), second_place=np.array(place, dtype=np.uint32),
                          second_seed=np.array(seed, dtype=np.uint32), stats=stats, mapq_stranded=None)
    if stranded:
        k = n // 2
        out.mapq_stranded = np.array([mapq_stranded_of(int(score[v]), second[v], int(score[v + k if v < k else v - k]), int(read_len[v]),
                                                       int(chain_off[v + 1]) > int(chain_off[v])) for v in range(n)], dtype=np.uint8)
    return out
