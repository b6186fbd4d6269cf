"""Paired reads, a mate rescued by alignment in the insert window: the definitions of include/fbg_hip.h
(fbg_pindex_pairs_align), statement by statement, on top of rows_model.Model (the row texts G_r and p(r, block)),
align_model.align and pairs_model.partner / twin.

Inputs are the 2n virtual reads, the current chains (chain_off, score, anchor_place, anchor_seed: the model does not care
which chaining call made them), per virtual read the rows that carry its chain (rows_model.chain_rows), q_start per seed and
the start places (start_src, start_dst, start_offset).  Python integers throughout: nothing wraps.  The model is the checker
of the kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import align_model as AM
from pairs_model import partner

NONE = AM.NONE
NO_PAIR = 0xff
MAX_READ = AM.MAX_READ
CLAMP = 1 << 33
STATS = ("selected", "aligned", "no_row", "empty", "too_long", "too_wide", "rejected_edits", "rejected_insert", "cells", "pairs")


def fragment(rm, r, anchors, L):
    """anchors: (node, offset in the node, q_start) of every anchor of a chain on row r, L the read length -> (fs, fe): the
    fragment ends projected along the first and the last anchor's diagonal."""
    (u1, o1, q1), (u2, o2, q2) = anchors[0], anchors[-1]
    x1, x2 = rm.p[r][rm.block_of[u1]] + o1, rm.p[r][rm.block_of[u2]] + o2
    return max(0, x1 - q1), min(len(rm.G[r]), x2 + L - q2)


def window_of(fs, fe, glen, forward, max_insert):
    """(w0, w1) of the window that an anchored v opens for partner(v); forward: v < n."""
    max_insert = min(max_insert, CLAMP)
    if forward:
        return fs, min(glen, fs + max_insert)
    return max(0, fe - max_insert), fe


def candidates(p, n):
    """[(chained read v, aligned read w)] of pair p in candidate order; v < n for the even ones."""
    a, b = 2 * p, 2 * p + 1
    return [(a, b + n), (b + n, a), (b, a + n), (a + n, b)]


def solve(rm, vreads, chain_off, score, anchor_place, anchor_seed, chain_sets, q_start, start_src, start_dst, start_offset,
          min_insert, max_insert, max_edits=NONE, max_window=0, select=None, max_read=MAX_READ, align=AM.align):
    """-> a namespace of row, edits, t_start, t_end, insert (uint32[2n]), which (uint8[n / 2]), pair_score, t_lo, t_hi
    (uint32[n / 2]), stats (a dict over STATS), and for the tests frag (per virtual read None or (r, fs, fe)), windows (per
    virtual read None or (w0, w1)) and status (per virtual read None or a name of STATS[1:6])."""
    V = len(chain_off) - 1
    n, P = V // 2, V // 4
    assert V % 4 == 0 and min_insert <= max_insert
    anchored = [int(chain_off[v + 1]) > int(chain_off[v]) for v in range(V)]
    frag = [None] * V
    for v in range(V):
        if not anchored[v] or not chain_sets[v]:
            continue
        r = chain_sets[v][0]
        an = []
        for g, t in zip(anchor_place[int(chain_off[v]):int(chain_off[v + 1])], anchor_seed[int(chain_off[v]):int(chain_off[v + 1])]):
            u, o = rm.node_and_offset(int(start_src[g]), int(start_dst[g]), int(start_offset[g]))
            an.append((u, o, int(q_start[t])))
        frag[v] = (r,) + fragment(rm, r, an, len(vreads[v]))
    out = np.full((5, V), NONE, dtype=np.uint32)
    st = dict.fromkeys(STATS, 0)
    windows, status = [None] * V, [None] * V
    for w in range(V):
        v = partner(w, n)
        if not anchored[v] or not (bool(select[w]) if select is not None else not anchored[w]):
            continue
        st["selected"] += 1
        if frag[v] is None:
            status[w] = "no_row"
        else:
            r, fs, fe = frag[v]
            P_w = bytes(vreads[w])
            w0, w1 = windows[w] = window_of(fs, fe, len(rm.G[r]), v < n, int(max_insert))
            out[0, w] = r
            if len(P_w) == 0 or w1 == w0:
                status[w] = "empty"
            elif len(P_w) > max_read:
                status[w] = "too_long"
            elif max_window and w1 - w0 > max_window:
                status[w] = "too_wide"
            else:
                status[w] = "aligned"
                e, s, t = align(P_w, rm.G[r][w0:w1])
                out[1:4, w] = e, w0 + s, w0 + t
                st["cells"] += len(P_w) * (w1 - w0)
        st[status[w]] += 1
    which, pscore, tlo, thi = [], [], [], []
    for p in range(P):
        best = None
        for i, (v, w) in enumerate(candidates(p, n)):
            if status[w] != "aligned":
                continue
            r, fs, fe = frag[v]
            e, ts, te = (int(x) for x in out[1:4, w])
            insert = te - fs if v < n else fe - ts
            assert 0 <= insert <= min(int(max_insert), CLAMP)
            if e > max_edits:
                st["rejected_edits"] += 1
            elif insert < min_insert:
                st["rejected_insert"] += 1
            else:
                out[4, w] = insert
                sc = int(score[v]) + len(vreads[w]) - e
                if best is None or sc > best[1]:
                    best = (i, sc) + ((fs, te) if v < n else (ts, fe))
        st["pairs"] += best is not None
        best = best if best is not None else (NO_PAIR, 0, NONE, NONE)
        which.append(best[0])
        pscore.append(best[1])
        tlo.append(best[2])
        thi.append(best[3])
    u32 = lambda x: np.array(x, dtype=np.uint32)      # noqa: E731
    return SimpleNamespace(row=out[0], edits=out[1], t_start=out[2], t_end=out[3], insert=out[4], which=np.array(which, dtype=np.uint8),
                           pair_score=u32(pscore), t_lo=u32(tlo), t_hi=u32(thi), stats=st, frag=frag, windows=windows, status=status)
