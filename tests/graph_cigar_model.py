"""The alignment path of each read against the stretch of the graph its path spells (include/fbg_hip.h,
fbg_pindex_chains_graph_cigar), composed from the two models it is defined by.

For a read that graph_align_model aligns, with text P of L symbols:
  T        graph_align_model.spell(g, path, start_offset, end_offset): the labels of the path back to back, from
           start_offset in the first node up to end_offset in the last; N = |T|;
  runs     cigar_model.path(P, T), whose E(0, 0) must be the modelled edits, merged by cigar_model.runs_of;
  stats    as cigar_model.of_align counts them: paths, ops, columns (the sum of N), history_bytes and batches.
gaf_fields gives the twelve columns and two tags of a GAF record from the same values.  The model is the checker of the
kernels and of the tool; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import cigar_model as CG
import graph_align_model as GM

NONE = GM.NONE


def of_graph(g, c, m, batch_kib=1 << 20, check=None):
    """The model on a graph (g), what test_rows.cpu() made of an input (c) and graph_align_model.of_cpu of it (m) -> off
    (uint64[n + 1]), ops (uint32), runs (per read [(code, length)]), strings, texts (T per read, None without an
    alignment), hist (history bytes per traced read), stats (the dict of PatternIndex.graph_cigar_stats).  check: called
    with (R, P, T, edits, op string) for every aligned read."""
    n = len(c.vreads)
    off, ops, runs, hist, texts = [0], [], [], [], []
    st = dict(paths=0, ops=0, columns=0, history_bytes=0, batches=0)
    for R in range(n):
        r, T = [], None
        if m.edits[R] != NONE:
            P = bytes(c.vreads[R])
            T = GM.spell(g, m.paths[R], int(m.start_offset[R]), int(m.end_offset[R]))
            s, e = CG.path(P, T)
            assert e == int(m.edits[R]), (R, e, int(m.edits[R]))
            assert len(T) <= len(P) + e
            if check:
                check(R, P, T, e, s)
            r = CG.runs_of(s)
            CG.consequences(r, len(P), len(T), e)
            st["paths"] += 1
            st["columns"] += len(T)
            hist.append(CG.history_bytes(len(P), len(T)))
        runs.append(r)
        texts.append(T)
        ops += CG.encode(r)
        off.append(len(ops))
    st["ops"] = len(ops)
    st["history_bytes"] = sum(hist)
    st["batches"] = CG.batches(hist, max(int(batch_kib), 1) << 10)
    return SimpleNamespace(hist=hist, off=np.array(off, dtype=np.uint64), ops=np.array(ops, dtype=np.uint32), runs=runs, stats=st,
                           strings=[CG.string_of(r) for r in runs], texts=texts)


def gaf_fields(g, m, gc, v, k, L, reverse, ids):
    """The fields of the GAF record of virtual read v, pattern k of L symbols; ids: the S id of every node, as bytes."""
    path = m.paths[v]
    plen = sum(len(g.labels[u]) for u in path)
    count = {code: 0 for code in CG.LETTER}
    for code, length in gc.runs[v]:
        count[code] += length
    return [b"read%d" % k, b"%d" % L, b"0", b"%d" % L, b"-" if reverse else b"+", b"".join(b">" + ids[u] for u in path), b"%d" % plen,
            b"%d" % m.start_offset[v], b"%d" % (plen - len(g.labels[path[-1]]) + int(m.end_offset[v])), b"%d" % count[CG.EQ],
            b"%d" % sum(count.values()), b"255", b"NM:i:%d" % m.edits[v], b"cg:Z:" + gc.strings[v].encode()]
