"""Chaining along one MSA row (include/fbg_hip.h, fbg_pindex_chains_by_row), restated on the other models.

For a (virtual) read R, with the anchors of chain_model (start places g with a column) and rows(g) of rows_model:
  chain(R, r)     chain_model.chain_of on the anchors g of R with r in rows(g): the same columns, `precedes`, band and
                  ties to the smallest g; nothing is chained in row coordinates;
  rowscore(R, r)  its score, 0 without such an anchor;
  score[R]        max over r of rowscore(R, r);
  row[R]          the smallest r that attains score[R], NONE where score[R] == 0;
  n_best_rows[R]  the number of rows that attain score[R], 0 where score[R] == 0;
  the chain       of R is chain(R, row[R]), empty where score[R] < min_score or score[R] == 0.
A read with more start places than max_places is not chained: score 0, no row, an empty chain.

by_row() groups a read's rows by the set of anchors they support and runs chain_of once per distinct set; brute_by_row()
goes row by row with chain_model.brute_force.  The model is the checker of the kernels; nothing here is used by the
product."""
from types import SimpleNamespace

import numpy as np

import chain_model as CM
import rows_model as RM

NONE = 0xffffffff


def places_per_read(c):
    return np.diff(c.start_off[c.seed_off.astype(np.int64)].astype(np.int64))


def by_row(c, band, min_score, max_places=1024):
    """c: what test_rows.cpu() / test_mapping_scale.cpu() hold of an input (seed_off, q_start, length, start_off,
    start_col, sets, rm) -> chain_off, score, row, n_best_rows, anchor_place, anchor_seed, col2 (start_col under the mask
    of the chosen rows), the rows of every chain (chain_n_rows, chain_first_row, row_bits, chain_sets) and the counts
    too_many, no_row and anchors_kept of fbg_pindex_chains_by_row_stats."""
    n = len(c.seed_off) - 1
    places = places_per_read(c)
    off, score, row, nbest, place, seed = [0], [], [], [], [], []
    col2 = np.full(len(c.start_col), NONE, dtype=np.uint32)
    too_many = no_row = 0
    for R in range(n):
        an = CM.read_anchors(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, R) if places[R] <= max_places else []
        too_many += places[R] > max_places
        of_row = {}
        for i, a in enumerate(an):
            for r in c.sets[a[0]]:
                of_row.setdefault(r, []).append(i)
        solved = {}                                   # support vector -> (score, chain as indices into an)
        for r, vec in of_row.items():
            if tuple(vec) not in solved:
                sc, idx = CM.chain_of([an[i] for i in vec], band)
                solved[tuple(vec)] = (sc, [vec[j] for j in idx])
        top = max((solved[tuple(v)][0] for v in of_row.values()), default=0)
        best = sorted(r for r, v in of_row.items() if solved[tuple(v)][0] == top) if top else []
        no_row += bool(an) and top == 0
        score.append(top)
        row.append(best[0] if best else NONE)
        nbest.append(len(best))
        if best:
            for i in of_row[best[0]]:
                col2[an[i][0]] = an[i][4]
            if top >= min_score:
                idx = solved[tuple(of_row[best[0]])][1]
                place += [an[j][0] for j in idx]
                seed += [an[j][1] for j in idx]
        off.append(len(place))
    out = SimpleNamespace(chain_off=np.array(off, dtype=np.uint64), score=np.array(score, dtype=np.uint32),
                          row=np.array(row, dtype=np.uint32), n_best_rows=np.array(nbest, dtype=np.uint32),
                          anchor_place=np.array(place, dtype=np.uint32), anchor_seed=np.array(seed, dtype=np.uint32), col2=col2,
                          too_many=int(too_many), no_row=int(no_row), anchors_kept=int((col2 != NONE).sum()), places=places,
                          max_places=max_places)
    out.chain_n_rows, out.chain_first_row, out.row_bits, out.chain_sets = RM.chain_rows(c.rm.m, c.sets, out.chain_off, out.anchor_place)
    return out


def stats(m, lds_max, byrow_lds=0):
    """The dict of PatternIndex.by_row_stats() for the model m, the compiled lds_max and option byrow_lds."""
    lim = 0 if byrow_lds < 0 else lds_max if byrow_lds == 0 else min(byrow_lds, lds_max)
    lim = min(lim, m.max_places)
    p = m.places
    return dict(reads_lds=int(((p > 0) & (p <= lim)).sum()), reads_device=int(((p > lim) & (p <= m.max_places)).sum()),
                reads_too_many=m.too_many, reads_no_row=m.no_row, anchors_kept=m.anchors_kept, lds_max=lds_max,
                max_places=m.max_places)


def as_cpu(c, m):
    """c with the chains of the model m in place of the plain ones: what rows_model, align_model and cigar_model take."""
    out = SimpleNamespace(**vars(c))
    for f in ("chain_off", "score", "anchor_place", "anchor_seed", "chain_n_rows", "chain_first_row", "row_bits", "chain_sets"):
        setattr(out, f, getattr(m, f))
    return out


def brute_by_row(c, R, band):
    """Row by row: (score, row, n_best_rows, the chain of that row as places g) of read R, each row's best chains by
    chain_model.brute_force over the anchors it supports, the representative with the smallest g from the end on."""
    an = CM.read_anchors(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, R)
    per_row = []
    for r in range(c.rm.m):
        mine = [a for a in an if r in c.sets[a[0]]]
        top, at = CM.brute_force(mine, band)
        per_row.append((top, [mine[j][0] for j in min(at, key=lambda sub: sub[::-1])] if at else []))
    top = max((t for t, _ in per_row), default=0)
    if top == 0:
        return 0, NONE, 0, []
    best = [r for r, (t, _) in enumerate(per_row) if t == top]
    return top, best[0], len(best), per_row[best[0]][1]
