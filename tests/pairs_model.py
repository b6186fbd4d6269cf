"""Paired reads: the definitions of include/fbg_hip.h (fbg_pindex_chains_pairs), statement by statement, on top of
chain_model and mapq_model.span_of.

Inputs are what PatternIndex.seeds(msa=True, strands=True) returns for n given reads, n even (seed_off, q_start, length,
start_off, start_col over the 2n virtual reads), and the primary chains as a chaining call reports them (chain_off, score,
anchor_place, anchor_seed): the model does not care whether fbg_pindex_chains or fbg_pindex_chains_by_row made them.
Python integers throughout: nothing wraps.  The model is the checker of the kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import chain_model as CM
from mapq_model import U64_MAX, span_of

NONE = CM.NONE
NO_PAIR = 0xff
STATS = ("which0", "which1", "which2", "which3", "none", "places_kept", "places_excluded", "rescue_differs")


def twin(v, n):
    return v + n if v < n else v - n


def partner(v, n):
    """The twin of v's mate."""
    return (v ^ 1) + n if v < n else (v - n) ^ 1


def window_of(span, forward, max_insert):
    """The window that the primary span of v = partner(w) opens for w; forward: v < n.  None: empty."""
    if span is None:
        return None
    lo, hi = span
    if forward:
        return lo, min(lo + max_insert, U64_MAX)
    return max(hi - max_insert, 0), hi


def in_window(c, k, W):
    return W is not None and c >= W[0] and c + k <= W[1]


def kept_anchors(anchors, W):
    return [a for a in anchors if in_window(a[4], a[3], W)]


def rescue_of(anchors, W, band):
    """(score, chain as a list of anchors, number of kept anchors): chain_model's chain on the kept places alone."""
    kept = kept_anchors(anchors, W)
    score, idx = CM.chain_of(kept, band)
    return score, [kept[j] for j in idx], len(kept)


def candidates(p, n):
    """[(forward virtual read, reverse virtual read, forward is the rescue, reverse is the rescue)] of pair p, in order."""
    a, b = 2 * p, 2 * p + 1
    return [(a, b + n, False, True), (a, b + n, True, False), (b, a + n, False, True), (b, a + n, True, False)]


def valid(sf, sr, min_insert, max_insert):
    """The four conditions on the spans of F and R (None: an empty chain), one by one."""
    both = sf is not None and sr is not None
    return (both, both and sf[0] <= sr[0], both and sf[1] <= sr[1], both and min_insert <= sr[1] - sf[0] <= max_insert)


def pick_of(cands, min_insert, max_insert):
    """cands: [(span F, score F, span R, score R)] in candidate order -> (which, pair_score, t_lo, t_hi)."""
    best = None
    for i, (sf, xf, sr, xr) in enumerate(cands):
        if all(valid(sf, sr, min_insert, max_insert)) and (best is None or xf + xr > best[1]):
            best = (i, xf + xr, sf[0], sr[1])
    return best if best is not None else (NO_PAIR, 0, NONE, NONE)


def solve(seed_off, q_start, length, start_off, start_col, chain_off, score, anchor_place, anchor_seed, band, min_insert, max_insert,
          cache=None):
    """-> a namespace of which, pair_score, t_lo, t_hi (per pair), rescue_off, rescue_score, rescue_lo, rescue_hi,
    rescue_place, rescue_seed (per virtual read), stats (a dict over STATS), kept (places kept per virtual read) and what
    adopt leaves: chain_off, score, anchor_place, anchor_seed, and chosen (per pair None or (F, R, F is rescue, R is
    rescue)).  cache: a dict that keeps the anchors of a read between calls on the same seeds."""
    V = len(seed_off) - 1
    n, P = V // 2, V // 4
    assert V % 4 == 0 and min_insert <= max_insert
    prim, pspan = [], []
    for v in range(V):
        a, b = int(chain_off[v]), int(chain_off[v + 1])
        ch = [(int(g), int(t), int(q_start[t]), int(length[t]), int(start_col[g])) for g, t in zip(anchor_place[a:b], anchor_seed[a:b])]
        prim.append(ch)
        pspan.append(span_of(ch))
    stats = dict.fromkeys(STATS, 0)
    resc, rscore, rspan, kept = [], [], [], []
    for w in range(V):
        if cache is not None and w in cache:
            an = cache[w]
        else:
            an = CM.read_anchors(seed_off, q_start, length, start_off, start_col, w)
            if cache is not None:
                cache[w] = an
        v = partner(w, n)
        sc, ch, nk = rescue_of(an, window_of(pspan[v], v < n, max_insert), band)
        resc.append(ch)
        rscore.append(sc)
        rspan.append(span_of(ch))
        kept.append(nk)
        stats["places_kept"] += nk
        stats["places_excluded"] += len(an) - nk
    which, pscore, tlo, thi, chosen = [], [], [], [], []
    for p in range(P):
        cs = candidates(p, n)
        got = pick_of([(rspan[f] if fr else pspan[f], rscore[f] if fr else int(score[f]),
                        rspan[r] if rr else pspan[r], rscore[r] if rr else int(score[r])) for f, r, fr, rr in cs], min_insert, max_insert)
        which.append(got[0])
        pscore.append(got[1])
        tlo.append(got[2])
        thi.append(got[3])
        if got[0] == NO_PAIR:
            stats["none"] += 1
            chosen.append(None)
        else:
            stats["which%d" % got[0]] += 1
            f, r, fr, rr = cs[got[0]]
            chosen.append((f, r, fr, rr))
            w = f if fr else r
            stats["rescue_differs"] += rscore[w] != int(score[w])
    # adopt: the chosen reads get the chosen chains, their twins the empty chain; a pair without a candidate keeps all four
    new = [(prim[v], int(score[v])) for v in range(V)]
    for c in chosen:
        if c is None:
            continue
        f, r, fr, rr = c
        new[f] = (resc[f], rscore[f]) if fr else new[f]
        new[r] = (resc[r], rscore[r]) if rr else new[r]
        new[twin(f, n)] = new[twin(r, n)] = ([], 0)
    u32, u64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint64))
    csr = lambda chains: u64(np.concatenate(([0], np.cumsum([len(c) for c in chains]))))      # noqa: E731
    flat = lambda chains, j: u32([a[j] for c in chains for a in c])      # noqa: E731
    newc = [c for c, _ in new]
    return SimpleNamespace(
        which=np.array(which, dtype=np.uint8), pair_score=u32(pscore), t_lo=u32(tlo), t_hi=u32(thi),
        rescue_off=csr(resc), rescue_score=u32(rscore), rescue_lo=u32([NONE if s is None else s[0] for s in rspan]),
        rescue_hi=u32([NONE if s is None else s[1] for s in rspan]), rescue_place=flat(resc, 0), rescue_seed=flat(resc, 1),
        stats=stats, kept=kept, chosen=chosen, chain_off=csr(newc), score=u32([s for _, s in new]), anchor_place=flat(newc, 0),
        anchor_seed=flat(newc, 1))
