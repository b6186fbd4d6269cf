"""fbg_pindex_chains_align_graph on the inputs of tests/test_mapping_scale.py: `founders` (200 rows of 12 founders, about
8,000 virtual reads) after plain and after by-row chains, and 17 and 128 rows with the whole graph as the window.

Every array is compared with tests/graph_align_model.py in its numpy form (a column at a time for every node of a block
at once; tests/test_align_graph.py compares that form with the cell form on every small input).  Model time on the
`founders` input: about 12 s for the 1,318 reads whose plain chain no row carries and about 42 s for all 4,205 reads with
a by-row chain, so every read is selected and no subset is drawn."""
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import byrow_model as BM  # noqa: E402
import graph_align_model as GM  # noqa: E402
import test_align_graph as TG  # noqa: E402
import test_mapping_scale as MS  # noqa: E402
import test_rows as TR  # noqa: E402

NONE = GM.NONE
HUGE = 1 << 40
FEWER_EDITS_ON_THE_GRAPH = 193               # founders: reads with graph_edits < the edits of their by-row alignment


@functools.lru_cache(maxsize=None)
def graph(name):
    c = MS.cpu(name)
    return GM.Graph(*c.graph, len(c.b))


@functools.lru_cache(maxsize=None)
def by_row(name):
    c = MS.cpu(name)
    return BM.as_cpu(c, BM.by_row(c, c.band, 0))


@functools.lru_cache(maxsize=None)
def unsupported(name):
    """The virtual reads whose plain chain no row carries."""
    c = MS.cpu(name)
    ln = np.diff(c.chain_off.astype(np.int64))
    return tuple(int(ln[R] > 0 and not c.chain_sets[R]) for R in range(len(c.vreads)))


@functools.lru_cache(maxsize=None)
def model(name, chains, pad=16):
    c = MS.cpu(name) if chains == "plain" else by_row(name)
    return GM.of_cpu(graph(name), c, pad, 0, unsupported(name) if chains == "plain" and name == "founders" else None, rows_only=True)


@functools.lru_cache(maxsize=None)
def row_alignment(name):
    with mock.patch.object(AM, "LITERAL_CELLS", 0):           # the model's DPs a row at a time in numpy
        return AM.of_cpu(by_row(name), 16, 0)


def test_founders_input_is_what_the_graph_alignment_needs():
    c, g = MS.cpu("founders"), graph("founders")
    assert max(g.first[j + 1] - g.first[j] for j in range(g.nb)) >= 12 and sum(unsupported("founders")) > 1000
    assert sum(len(p) >= 2 for p in g.preds) > 100


def run(engine, name, chains, pad, select=None):
    c = MS.cpu(name) if chains == "plain" else by_row(name)
    g, m = graph(name), model(name, chains, pad)
    with TR.build(engine, c.A, c.b) as pix:
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=True, rows=True)
        ch = pix.chains(band=c.band, by_row=chains != "plain", graph=True, graph_pad=pad, select=select)
        assert np.array_equal(ch.chain_off, c.chain_off) and np.array_equal(ch.anchor_place, c.anchor_place)
        TG.same_python(ch, m, (name, chains))
        assert pix.graph_align_stats() == TG.stats_of(m, g)
        assert np.array_equal(ch.best_graph_edits, GM.best_edits(m.edits, ch.strand))
    return c, g, m, ch


@pytest.mark.gpu
def test_founders_after_plain_chains(engine):
    """The reads whose chain no row carries: the row alignment has nothing for them, the graph spells a path for each."""
    c, g, m, ch = run(engine, "founders", "plain", 16, unsupported("founders"))
    sel = np.array(unsupported("founders"), dtype=bool)
    assert m.stats["aligned"] == int(sel.sum()) and (m.edits[sel] != NONE).all() and (m.edits[~sel] == NONE).all()
    assert (m.n_path[sel] >= 1).all() and int((m.edits[sel] == 0).sum()) > 0


@pytest.mark.gpu
def test_founders_after_by_row_chains(engine):
    """Every read, and beside the row alignment of the same chains: never more edits on the graph where the row's window
    lies inside the graph's, and fewer for the reads that recombine rows or carry another row's private symbol."""
    c, g, m, ch = run(engine, "founders", "by_row", 16)
    am = row_alignment("founders")
    assert TG.inequality(g, c, m, am) > 3000
    both = (m.edits != NONE) & (am.edits != NONE)
    assert int(both.sum()) == am.stats["aligned"] == m.stats["aligned"]
    assert int((m.edits[both] < am.edits[both]).sum()) == FEWER_EDITS_ON_THE_GRAPH
    assert int((ch.graph_edits[both] < am.edits[both]).sum()) == FEWER_EDITS_ON_THE_GRAPH


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [17, 128])
def test_the_whole_graph_as_the_window(engine, rows):
    c, g, m, ch = run(engine, f"m{rows}", "plain", HUGE)
    assert all(w == (0, g.nb - 1) for w in m.windows if w) and m.stats["aligned"] > 100
    assert m.stats["nodes"] == m.stats["aligned"] * len(g.labels)
