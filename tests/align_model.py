"""The edit distance of each read to a row that carries its chain (include/fbg_hip.h, fbg_pindex_chains_align),
restated on byte strings.

rows_model.Model gives G_r, p(r, j) and node_of; the chains and the places come from elsewhere (the engine, or the other
models on the CPU).  For a (virtual) read with text P of L symbols and a non-empty chain:
  r        the smallest row that supports every anchor of the chain (rows_model); none -> all four results NONE;
  d_i      x_i - q_i with x_i = p(r, block(u_i)) + o_i for every anchor;
  W        G_r[w0 : w1), w0 = max(0, min d_i - pad), w1 = min(|G_r|, max d_i + L + pad);
  D        D(0, j) = 0, D(i, 0) = i, D(i, j) = min(D(i-1, j-1) + [P[i-1] != W[j-1]], D(i-1, j) + 1, D(i, j-1) + 1);
  edits    min_j D(L, j); t_end = w0 + the smallest such j;
  t_start  t_end - j' for the smallest j' that attains the minimum of D'(L, j') over the reversed read against
           W[0 : e) reversed with D'(0, j) = j: the largest start s with lev(P, G_r[s : t_end)) == edits.
L > max_read, and then w1 - w0 > max_window (0: no limit), keep the row and set the three other results to NONE.
Both DPs are written out cell by cell (last_row; windows of many cells go through last_row_by_rows, the same recurrence
a row at a time, which the CPU tests compare with it); brute() is the check of the end and start rules over all substrings of the
window.  The model is the checker of the kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

NONE = 0xffffffff
MAX_READ = 1024          # what fbg_pindex_align_stats reports; the GPU tests compare


def last_row(P, W, first_row):
    """D(L, j) for j = 0 .. |W| of the recurrence with D(0, j) = first_row(j) and D(i, 0) = i."""
    prev = [first_row(j) for j in range(len(W) + 1)]
    for i in range(1, len(P) + 1):
        cur = [i] + [0] * len(W)
        for j in range(1, len(W) + 1):
            cur[j] = min(prev[j - 1] + (P[i - 1] != W[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev


def last_row_by_rows(P, W, first_row):
    """last_row a whole row at a time, for the long reads of the tier tests: cur[j] = min over k <= j of
    (min(diagonal, vertical) at k) + (j - k), which a running minimum of the values less their index gives.  The CPU
    tests compare it with last_row on every small input."""
    Wn = np.frombuffer(bytes(W), dtype=np.uint8)
    idx = np.arange(len(W) + 1, dtype=np.int64)
    prev = np.array([first_row(j) for j in range(len(W) + 1)], dtype=np.int64)
    for i in range(1, len(P) + 1):
        base = np.empty(len(W) + 1, dtype=np.int64)
        base[0] = i
        base[1:] = np.minimum(prev[:-1] + (Wn != P[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(base - idx) + idx
    return prev.tolist()


LITERAL_CELLS = 1 << 14      # windows of more cells than this go by rows


def smallest_min(row):
    best = min(row)
    return best, row.index(best)


def align(P, W):
    """-> (edits, s, e): P against the text W, ends of W free; W[s : e) by the two passes of the definition."""
    P, W = bytes(P), bytes(W)
    dp = last_row if len(P) * len(W) <= LITERAL_CELLS else last_row_by_rows
    edits, e = smallest_min(dp(P, W, lambda j: 0))
    back, j = smallest_min(dp(P[::-1], W[:e][::-1], lambda j: j))
    assert back == edits, (back, edits)
    return edits, e - j, e


def lev(a, b):
    return last_row(a, b, lambda j: j)[-1]


def brute(P, W):
    """The same by the definition's words: the minimum of lev over all substrings, the smallest end among those that
    attain it, then the largest start for that end."""
    P, W = bytes(P), bytes(W)
    d = {}
    for s in range(len(W) + 1):          # one DP per start: its last row holds lev(P, W[s : s + j]) for every j
        for j, v in enumerate(last_row(P, W[s:], lambda j: j)):
            d[(s, s + j)] = v
    edits = min(d.values())
    e = min(e for (s, e), v in d.items() if v == edits)
    s = max(s for (s, e2), v in d.items() if e2 == e and v == edits)
    return edits, s, e


def window(rm, r, anchors, L, pad):
    """anchors: (node, offset in the node, q_start) of every anchor -> (w0, w1) on row r."""
    diag = [rm.p[r][rm.block_of[u]] + o - q for u, o, q in anchors]
    return max(0, min(diag) - pad), min(len(rm.G[r]), max(diag) + L + pad)


def chains_align(rm, vreads, chain_off, anchor_place, anchor_seed, chain_sets, q_start, start_src, start_dst, start_offset,
                 pad=16, max_window=0, max_read=MAX_READ, check=None):
    """-> row, edits, t_start, t_end (uint32[n]), stats (the dict of PatternIndex.align_stats without table_bytes), and the
    windows (w0, w1) per read (None where there is no row).  chain_sets: per read the rows that carry its chain
    (rows_model.chain_rows).  check: called with (P, W, (edits, s, e)) for every aligned read."""
    n = len(chain_off) - 1
    out = np.full((4, n), NONE, dtype=np.uint32)
    st = dict(aligned=0, unsupported=0, too_long=0, too_wide=0, cells=0, max_read=max_read)
    wins = [None] * n
    for R in range(n):
        a, b = int(chain_off[R]), int(chain_off[R + 1])
        if a == b:
            continue
        if not chain_sets[R]:
            st["unsupported"] += 1
            continue
        r = chain_sets[R][0]
        out[0, R] = r
        P = bytes(vreads[R])
        anchors = []
        for g, t in zip(anchor_place[a:b], anchor_seed[a:b]):
            u, o = rm.node_and_offset(int(start_src[g]), int(start_dst[g]), int(start_offset[g]))
            anchors.append((u, o, int(q_start[t])))
        w0, w1 = window(rm, r, anchors, len(P), int(pad))
        wins[R] = (w0, w1)
        assert w0 < w1
        if len(P) > max_read:
            st["too_long"] += 1
            continue
        if max_window and w1 - w0 > max_window:
            st["too_wide"] += 1
            continue
        W = rm.G[r][w0:w1]
        res = align(P, W)
        if check:
            check(P, W, res)
        out[1:, R] = res[0], w0 + res[1], w0 + res[2]
        st["aligned"] += 1
        st["cells"] += len(P) * len(W)
    return out[0], out[1], out[2], out[3], st, wins


def of_cpu(c, pad=16, max_window=0, max_read=MAX_READ, check=None):
    """The model on what test_rows.cpu() made of an input."""
    row, edits, ts, te, st, wins = chains_align(c.rm, c.vreads, c.chain_off, c.anchor_place, c.anchor_seed, c.chain_sets, c.q_start,
                                                c.start_src, c.start_dst, c.start_offset, pad, max_window, max_read, check)
    return SimpleNamespace(row=row, edits=edits, t_start=ts, t_end=te, stats=st, windows=wins)


def best_edits(edits, strand):
    """Per given read the edits of the strand that Chains.strand picked, NONE where the strand is 0xff."""
    k = len(strand)
    return np.array([NONE if s == 0xff else int(edits[int(s) * k + R]) for R, s in enumerate(strand)], dtype=np.uint32)
