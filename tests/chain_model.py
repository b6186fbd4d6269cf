"""Co-linear chaining of a read's seeds: the literal O(A^2) dynamic programme of include/fbg_hip.h (fbg_pindex_chains).

Inputs are what PatternIndex.seeds(msa=True) returns: seed_off (reads -> seeds), q_start and length per seed, start_off
(seeds -> capped start places) and start_col per place.  An anchor is a start place g with start_col[g] != NONE; i
precedes j iff seed(i) < seed(j), c_j >= c_i + k_i and |(c_j - c_i) - (q_j - q_i)| <= band (band None: unbounded);
best[j] = k_j + max(0, max over predecessors); ties go to the smallest g, for the predecessor and for the chain's end.
Signed 64-bit and Python integers throughout: nothing wraps.  The model is the checker of the kernels; nothing here is
used by the product."""
import itertools

import numpy as np

NONE = 0xffffffff


def precedes(ti, ci, qi, ki, tj, cj, qj, band):
    return ti < tj and cj >= ci + ki and (band is None or abs((cj - ci) - (qj - qi)) <= band)


def read_anchors(seed_off, q_start, length, start_off, start_col, r):
    """[(g, t, q, k, c)] of read r in g order."""
    out = []
    for t in range(int(seed_off[r]), int(seed_off[r + 1])):
        for g in range(int(start_off[t]), int(start_off[t + 1])):
            if int(start_col[g]) != NONE:
                out.append((g, t, int(q_start[t]), int(length[t]), int(start_col[g])))
    return out


def chain_of(anchors, band):
    """(score, [index into anchors] in ascending order) of one read's anchors [(g, t, q, k, c)] given in g order.  The
    scan over the earlier anchors is one NumPy expression per anchor; argmax returns the first maximum, the smallest g."""
    if not anchors:
        return 0, []
    _, t, q, k, c = (np.array(col, dtype=np.int64) for col in zip(*anchors))
    best, pred = np.zeros(len(anchors), dtype=np.int64), [None] * len(anchors)
    for j in range(len(anchors)):
        ok = (t[:j] < t[j]) & (c[j] >= c[:j] + k[:j])
        if band is not None:
            ok &= np.abs((c[j] - c[:j]) - (q[j] - q[:j])) <= band
        cand = np.where(ok, best[:j], 0)
        m = int(cand.max()) if j else 0
        if m > 0:
            pred[j] = int(np.argmax(cand))
        best[j] = k[j] + m
    end = int(np.argmax(best))
    out, j = [], end
    while j is not None:
        out.append(j)
        j = pred[j]
    return int(best[end]), out[::-1]


def solve(seed_off, q_start, length, start_off, start_col, band):
    """Per read (anchors, score, chain as indices into anchors): the part of chains() that does not depend on min_score."""
    out = []
    for r in range(len(seed_off) - 1):
        an = read_anchors(seed_off, q_start, length, start_off, start_col, r)
        out.append((an,) + chain_of(an, band))
    return out


def assemble(solved, min_score):
    off, score, place, seed = [0], [], [], []
    for an, sc, idx in solved:
        score.append(sc)
        if sc >= min_score:
            place += [an[j][0] for j in idx]
            seed += [an[j][1] for j in idx]
        off.append(len(place))
    return (np.array(off, dtype=np.uint64), np.array(score, dtype=np.uint32), np.array(place, dtype=np.uint32),
            np.array(seed, dtype=np.uint32))


def chains(seed_off, q_start, length, start_off, start_col, band, min_score):
    """-> (chain_off uint64[n + 1], score uint32[n], anchor_place uint32[], anchor_seed uint32[])."""
    return assemble(solve(seed_off, q_start, length, start_off, start_col, band), min_score)


def brute_force(anchors, band):
    """Every non-empty subset of the anchors in g order whose neighbours precede one another -> (best score, the valid
    chains of that score as index tuples).  Exponential: for up to about 10 anchors."""
    top, at = 0, []
    for size in range(1, len(anchors) + 1):
        for sub in itertools.combinations(range(len(anchors)), size):
            ok = all(precedes(anchors[a][1], anchors[a][4], anchors[a][2], anchors[a][3], anchors[b][1], anchors[b][4],
                              anchors[b][2], band) for a, b in zip(sub, sub[1:]))
            if not ok:
                continue
            sc = sum(anchors[j][3] for j in sub)
            if sc > top:
                top, at = sc, [sub]
            elif sc == top:
                at.append(sub)
    return top, at
