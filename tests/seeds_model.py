"""Plain Python restatement of fbg_pindex_seeds (include/fbg_hip.h): a read cut greedily into the maximal pieces the
search of the index accepts.

    i = 0
    while i < |P|:
        k = search(P[i:]).pos             rule 4 of locate_model.Index.locate
        if k == 0:  i += 1                P[i] cannot be matched from the full range: skipped
        else:       seed (i, k); i += k   the failing symbol, if any, starts the next search

Seeds of fewer than L symbols are consumed but not reported.  Everything else a seed carries is what
occ_model.Index.occurrences reports for the pattern P[i : i + k] with the same cap.  The model is the checker of the
kernels; nothing here is used by the product."""
from types import SimpleNamespace

import locate_model as M


def cuts(index, pattern):
    """[(i, k)] of every seed of the pattern, short ones included."""
    P = M.as_bytes(pattern)
    out, i = [], 0
    while i < len(P):
        k = index.locate(P[i:])[1]
        if k == 0:
            i += 1
        else:
            out.append((i, k))
            i += k
    return out


def seeds(index, pattern, L=1, cap=None):
    """-> a list of namespace(q_start, length, occ) in ascending q_start; occ = index.occurrences(P[i : i + k], cap)
    (index: an occ_model.Index)."""
    if L < 1:
        raise ValueError("the minimum length is 1 or more")
    P = M.as_bytes(pattern)
    return [SimpleNamespace(q_start=i, length=k, occ=index.occurrences(P[i:i + k], cap)) for i, k in cuts(index, P) if k >= L]
