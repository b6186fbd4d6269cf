"""Plain restatement of the row-chunk mode, --heuristic-subset=ROWNUM (fbg.cpp:3400-3433, 3467-3500), for the tests.

  1. f of every chunk of `rows` consecutive rows, max-merged (oracle compute_f with f_init);
  2. the min-max-length DP on the merged f (oracle minmax_dp);
  3. the repair loop: the graph of the segmentation in output_efg's numbering (per block a dict label -> id by first
     row, a set of (previous id, id)), validate_model.naive_validate, bad_cuts, drop the flagged boundaries, again
     until none is flagged.
Nothing here is used by the product.
"""
import numpy as np

import validate_model as VM
from oracle import pyoracle as O


def segmentation_graph(msa, boundaries):
    """(labels, edges, blocks): labels a list of bytes in node order, edges a sorted list of distinct (u, v), blocks
    the block (from 0) of every node.  A row that is all gaps in a block has no node there and no edge across."""
    msa = np.ascontiguousarray(msa, dtype=np.uint8)
    m, n = msa.shape
    labels, blocks, edges = [], [], set()
    prev = [None] * m
    x0 = 0
    for j, b in enumerate(int(x) for x in boundaries):
        x1 = min(b + 1, n)
        ids, cur = {}, [None] * m
        for i in range(m):
            lab = msa[i, x0:x1].tobytes().replace(b"-", b"")
            if not lab:
                continue
            if lab not in ids:
                ids[lab] = len(labels)
                labels.append(lab)
                blocks.append(j)
            cur[i] = ids[lab]
            if prev[i] is not None:
                edges.add((prev[i], cur[i]))
        prev = cur
        x0 = b + 1
    return labels, sorted(edges), np.array(blocks, dtype=np.int64)


def chunked_f(msa, rows, ignore="", disable_tricks=False):
    msa = np.ascontiguousarray(msa, dtype=np.uint8)
    f = np.zeros(msa.shape[1], dtype=np.uint64)
    for r in range(0, msa.shape[0], rows):
        f = O.compute_f(msa[r:r + rows], ignore, disable_tricks, f_init=f)
    return f


def cuts_of(msa, boundaries, ignore=""):
    """(bad_cuts, status, graph) of one validation round."""
    labels, edges, blocks = segmentation_graph(msa, boundaries)
    status, _ = VM.naive_validate(labels, edges, blocks, ignore.encode() if isinstance(ignore, str) else ignore)
    return VM.bad_cuts(status, blocks), status, (labels, edges, blocks)


def repair(msa, boundaries, ignore=""):
    """-> (final boundaries, rounds, removed per round)."""
    b = [int(x) for x in boundaries]
    removed = []
    while True:
        cuts, _, _ = cuts_of(msa, b, ignore)
        if not cuts:
            return np.array(b, dtype=np.uint64), len(removed), removed
        removed.append(len(cuts))
        drop = set(cuts)
        b = [x for k, x in enumerate(b) if k not in drop]


def heuristic(msa, rows, ignore="", disable_tricks=False):
    """-> (initial boundaries, final boundaries, rounds, removed per round, merged f)."""
    f = chunked_f(msa, rows, ignore, disable_tricks)
    b0 = O.minmax_dp(f)[2]
    b1, rounds, removed = repair(msa, b0, ignore)
    return b0, b1, rounds, removed, f
