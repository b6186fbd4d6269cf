"""The edit distance of each read to a path of the graph around its chain: fbg_pindex_chains_align_graph, _fetch,
fbg_pindex_align_graph_stats and PatternIndex.chains(graph=True) / .graph_align_stats() (include/fbg_hip.h,
csrc/pindex_graph.hip).

The checker is tests/graph_align_model.py: the window in blocks, the recurrence over the DAG cell by cell with the
row-wise minimum on entering a node, the walk back through the merges, and a brute force over every path and substring
of tiny graphs.  The inputs are those of tests/test_rows.py (with its CPU pipeline of seeds, chains and row sets, and
byrow_model for the chains along one row) and three of this file's own: two predecessor columns that cross at a word
boundary, a node with 130 predecessors, and reads at the word and tier boundaries on a two-haplotype graph.  On the CPU
the tests assert that the inputs hold what they are meant to hold; on the GPU every array is compared exactly."""
import ctypes
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import byrow_model as BM  # noqa: E402
import graph_align_model as GM  # noqa: E402
import test_rows as TR  # noqa: E402

CALLS = ("fbg_pindex_chains_align_graph", "fbg_pindex_chains_align_graph_fetch", "fbg_pindex_align_graph_stats")
NONE = GM.NONE
HUGE = 1 << 40
PADS = (16, 0, HUGE)
LENGTHS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, GM.MAX_READ, GM.MAX_READ + 1)


# ---- this file's inputs ------------------------------------------------------------------------------------------------

def rnd(rng, k):
    return "".join(rng.choice(list("ACGT"), k))


def merge_parts():
    rng = np.random.default_rng(6364)
    U, V, T = rnd(rng, 64), rnd(rng, 40), rnd(rng, 20)
    return U, V, T, [rnd(rng, 12) for _ in range(4)]


def merge_input():
    """Block 0 holds a = Ra U, b = Rb U v0, d = Rd T, e = Re T; block 1 holds c = V[1:] for every row.  The read
    U[1:] V (63 + 40 symbols) has F_a(63) = 0 < F_b(63) and F_b(64) = 0 < F_a(64); the read U V has the same one row later.
    The read T[-10:] c[:10] comes into c through d and through e alike."""
    U, V, T, (Ra, Rb, Rd, Re) = merge_parts()
    heads = [Ra + U, Rb + U + V[0], Rd + T + "G" * 45, Re + T + "C" * 45]
    heads[2], heads[3] = "G" * 45 + Rd + T, "C" * 45 + Re + T
    width = max(len(h) for h in heads)
    rows = [h + "-" * (width - len(h)) + V[1:] for h in heads]
    c = V[1:]
    reads = [U[1:] + V, U + V, T[-10:] + c[:10], Ra[-4:] + U + "T" + V[1:20]]
    return TR.msa_of(rows), [width - 1, width + len(c) - 1], [r.encode() for r in reads], 8, 8, None, 0


def fan_input():
    """130 rows with labels of their own in block 0 and one label for all in block 1: a node with 130 predecessors."""
    rng = np.random.default_rng(130)
    tail = rnd(rng, 24)
    heads = ["".join("ACGT"[(r >> (2 * k)) & 3] for k in range(4)) + "TTGACCAT" for r in range(130)]
    assert len(set(heads)) == 130
    rows = [h + tail for h in heads]
    reads = [heads[r][2:] + tail[:12] for r in (0, 77, 129)] + [heads[5][:6] + "A" + heads[5][6:] + tail[:9], tail[3:20]]
    return TR.msa_of(rows), [11, 35], [r.encode() for r in reads], 6, 4, None, 0


def length_haps():
    rng = np.random.default_rng(1100)
    h0 = list(rnd(rng, 1100))
    h1 = list(h0)
    for x in range(17, 1100, 29):
        h1[x] = "ACGT"[("ACGT".index(h1[x]) + 1) % 4]
    return "".join(h0), "".join(h1)


def length_input():
    """Two haplotypes of 1100 symbols that differ every 29 columns, in blocks of 100, and two rows that change between them
    at every boundary: two nodes per block, and every node of a block joined to every node of the next.  Per length of
    LENGTHS one read: cut from haplotype 0 (even index) or recombinant, haplotype 0 up to a block boundary inside the
    read and haplotype 1 after it (odd index); two substitutions planted where there is room."""
    h0, h1 = length_haps()
    reads = []
    for k, L in enumerate(LENGTHS):
        a = 1100 - L if L >= 1000 else 37 + 53 * k
        cut = (a + L // 2) // 100 * 100
        cut += 100 if cut <= a else 0
        src = h0 if k % 2 == 0 else h0[:cut] + h1[cut:]
        P = bytearray(src[a:a + L].encode())
        for x in ((L // 3, (2 * L) // 3) if L >= 60 else ()):
            P[x] = b"ACGT"[(b"ACGT".index(P[x]) + 2) % 4]
        reads.append(bytes(P))
    mixed = ["".join((h0, h1)[(j + t) % 2][100 * j:100 * j + 100] for j in range(11)) for t in (0, 1)]      # every edge between two blocks
    return TR.msa_of([h0, h1] + mixed), list(range(99, 1100, 100)), reads, 12, 4, None, 0


OWN = {"graph_merge": merge_input, "graph_fan": fan_input, "graph_lengths": length_input}
NAMES = list(TR.INPUTS) + ["graph_merge", "graph_fan"]
LONG = ("tiers", "graph_lengths")                # reads of about a thousand symbols: the model goes a column at a time


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False, by_row=False):
    """test_rows.cpu() on an input of either file; by_row: with the chains of byrow_model in place of the plain ones."""
    with mock.patch.dict(TR.INPUTS, OWN):
        c = TR.cpu(name, strands)
    if by_row:
        c = BM.as_cpu(c, BM.by_row(c, c.band, c.min_score))
    return c


@functools.lru_cache(maxsize=None)
def graph(name):
    with mock.patch.dict(TR.INPUTS, OWN):
        A, b = TR.INPUTS[name]()[:2]
    return GM.Graph.of(A, b)


@functools.lru_cache(maxsize=None)
def model(name, strands=False, by_row=False, pad=16, max_cells=0, select=None, batch_kib=1 << 20):
    return GM.of_cpu(graph(name), cpu(name, strands, by_row), pad, max_cells, select, batch_kib=batch_kib)


def stats_of(m, g):
    return dict(m.stats, table_bytes=g.table_bytes())


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_graph_align_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    for words in ("graph_batch_kib", "no CIGAR over the path", "no affine gaps", "no\n * pruning inside it"):
        assert words in header, words


def random_case(rng):
    """A tiny layered graph from rows that pick one of up to three labels per block, and a read cut from a row's text or a
    recombination of two with up to two edits: at most 4 blocks, 3 nodes per block, labels of at most 6 symbols."""
    nb, m = int(rng.integers(2, 5)), int(rng.integers(4, 7))
    al = "AC" if rng.integers(0, 3) else "ACGT"
    rows, b, x = [""] * m, [], 0
    for j in range(nb):
        w = int(rng.integers(1, 5))
        variants = list(dict.fromkeys(rnd2(rng, al, w) for _ in range(3)))
        for r in range(m):
            rows[r] += variants[int(rng.integers(0, len(variants)))]
        x += w
        b.append(x - 1)
    g = GM.Graph.of(TR.msa_of(rows), b)
    text = "".join(rows[int(rng.integers(0, m))][:b[nb // 2 - 1] + 1 if nb > 1 else 0]) + rows[int(rng.integers(0, m))][b[nb // 2 - 1] + 1:]
    s = int(rng.integers(0, len(text)))
    P = bytearray(text[s:s + int(rng.integers(1, 8))].encode())
    for _ in range(int(rng.integers(0, 3))):
        k, op = int(rng.integers(0, len(P))), int(rng.integers(0, 3))
        if op == 0:
            P[k] = ord(rng.choice(list(al)))
        elif op == 1 and len(P) > 1:
            del P[k]
        else:
            P.insert(k, ord(rng.choice(list(al))))
    return g, bytes(P)


def rnd2(rng, al, k):
    return "".join(rng.choice(list(al), k))


def fits(g, jl, jh):
    nodes = range(g.first[jl], g.first[jh + 1])
    return jh - jl < 4 and all(g.first[j + 1] - g.first[j] <= 3 for j in range(jl, jh + 1)) and all(len(g.labels[v]) <= 6 for v in nodes)


def both_forms(g, jl, jh, P):
    """The model cell by cell and a column at a time -> (edits, end, start, path) of the first, equal to the second."""
    res = []
    for step in (GM.step_cells, GM.step_rows):
        edits, end, last = GM.forward(g, jl, jh, P, step)
        start, path = GM.trace(g, jl, P, last, edits, end, step)
        res.append((edits, end, start, path, {v: [int(x) for x in c] for v, c in last.items()}))
    edits, end, last = GM.forward_blocks(g, jl, jh, P)
    start, path = GM.trace(g, jl, P, last, edits, end, GM.step_rows)
    res.append((edits, end, start, path, {v: [int(x) for x in c] for v, c in last.items()}))
    assert res[0] == res[1] == res[2]
    return res[0][:4]


def consequences(g, jl, jh, P, res):
    """What follows from the definition: a path of the graph inside the window, whose replay gives edits <= L."""
    edits, end, start, path = res
    assert path[0] == start[0] and path[-1] == end[0] and 0 <= edits <= len(P)
    assert all(jl <= g.block_of[v] <= jh for v in path)
    assert all((u, v) in set(g.edges) for u, v in zip(path, path[1:]))
    assert 0 <= start[1] <= len(g.labels[start[0]]) and 0 <= end[1] <= len(g.labels[end[0]])
    assert GM.lev(P, GM.spell(g, path, start[1], end[1])) == edits


def test_definition_against_brute_force_on_tiny_graphs():
    rng = np.random.default_rng(2500)
    merged = ties = 0
    for it in range(300):
        g, P = random_case(rng)
        jl, jh = 0, g.nb - 1
        assert fits(g, jl, jh)
        merged += any(len(p) >= 2 for p in g.preds)
        res = both_forms(g, jl, jh, P)
        assert res == GM.brute(g, jl, jh, P), (it, g.labels, g.edges, P)
        consequences(g, jl, jh, P, res)
        steps = []
        edits, end, last = GM.forward(g, jl, jh, P)
        GM.trace(g, jl, P, last, edits, end, steps=steps)
        ties += any(len(ok) >= 2 for _, ok in steps)
    assert merged >= 250 and ties >= 10, (merged, ties)


SMALL = [n for n in NAMES if n != "tiers"]


@pytest.mark.parametrize("name", SMALL)
def test_model_forms_agree_and_keep_the_consequences(name):
    """Every input, plain and stranded, after plain and after by-row chains, at every pad: the two forms of the column
    step, the consequences, and the brute force wherever the window is tiny enough."""
    g = graph(name)
    brutes = 0
    for strands in (False, True):
        for by_row in (False, True):
            c = cpu(name, strands, by_row)
            for pad in PADS:
                seen = []

                def check(R, P, jl, jh, res):
                    nonlocal brutes
                    if len(P) * sum(len(g.labels[v]) for v in range(g.first[jl], g.first[jh + 1])) <= GM.LITERAL_CELLS:
                        assert both_forms(g, jl, jh, P) == res
                    consequences(g, jl, jh, P, res)
                    if fits(g, jl, jh) and len(P) <= 12:
                        assert res == GM.brute(g, jl, jh, P), (name, R)
                        brutes += 1
                    seen.append(R)
                m = GM.of_cpu(g, c, pad, check=check)
                assert len(seen) == m.stats["aligned"]
                assert (m.edits[m.edits != NONE] <= np.array([len(c.vreads[R]) for R in np.flatnonzero(m.edits != NONE)])).all()
    if name == "bounds":
        assert brutes > 0


@pytest.mark.parametrize("name", SMALL)
def test_graph_edits_are_at_most_the_row_edits(name):
    """A read that the by-row alignment aligns at the same pad, whose row has a node in every block of the window and
    whose row window lies inside those blocks, has graph_edits <= edits."""
    g = graph(name)
    checked = 0
    for strands in (False, True):
        c = cpu(name, strands, True)
        for pad in (16, 0):
            m, am = GM.of_cpu(g, c, pad), AM.of_cpu(c, pad)
            checked += inequality(g, c, m, am)
    assert checked > 0 or name in ("m1",)


def inequality(g, c, m, am):
    checked = 0
    for R in range(len(c.vreads)):
        if am.edits[R] == NONE or m.edits[R] == NONE:
            continue
        r, (jl, jh), (w0, w1) = int(am.row[R]), m.windows[R], am.windows[R]
        if any(c.rm.node_of[r][j] is None for j in range(jl, jh + 1)):
            continue
        end = c.rm.p[r][jh + 1] if jh + 1 < g.nb else len(c.rm.G[r])
        if c.rm.p[r][jl] <= w0 and w1 <= end:
            assert m.edits[R] <= am.edits[R], R
            checked += 1
    return checked


def test_recombinant_input_is_what_it_claims():
    """Both spliced reads lie on the graph with no edit, along three nodes that no row carries, and get no row alignment
    after plain chains."""
    c, g, m = cpu("recombinant"), graph("recombinant"), model("recombinant")
    am = AM.of_cpu(c, 16)
    n = len(c.reads)
    for R in (n - 2, n - 1):
        assert m.edits[R] == 0 and m.n_path[R] == 3 and am.edits[R] == NONE and am.row[R] == NONE
        path = m.paths[R]
        assert not any(all(c.rm.node_of[r][g.block_of[v]] == v for v in path) for r in range(c.rm.m))
        assert GM.spell(g, path, int(m.start_offset[R]), int(m.end_offset[R])) == c.reads[R]
    assert (m.edits[:n - 2] == 0).all()


def test_merge_input_is_what_it_claims():
    c, g = cpu("graph_merge"), graph("graph_merge")
    U, V, T, _ = merge_parts()
    a, b, d, e, cnode = 0, 1, 2, 3, 4
    assert g.preds[cnode] == [a, b, d, e] and g.labels[cnode] == V[1:].encode()
    for R, row in ((0, 63), (1, 64)):
        edits, end, last = GM.forward(g, 0, 1, c.reads[R])
        Fa, Fb = last[a], last[b]
        assert Fa[row] < Fb[row] and Fb[row + 1] < Fa[row + 1], (R, Fa[row - 1:row + 3], Fb[row - 1:row + 3])
        assert all(Fa[i] < Fb[i] for i in range(row - 8, row + 1)) and all(Fb[i] < Fa[i] for i in range(row + 1, len(c.reads[R]) + 1))
        assert edits == 0 and end == (cnode, len(c.reads[R]) - row - 1)
    m = model("graph_merge")
    assert m.edits.tolist() == [0, 0, 0, 1] and (m.n_path == 2).all()
    assert m.paths[0] == [b, cnode] and m.paths[1] == [b, cnode] and m.paths[3] == [a, cnode]
    steps = []
    edits, end, last = GM.forward(g, 0, 1, c.reads[2])
    start, path = GM.trace(g, 0, c.reads[2], last, edits, end, steps=steps)
    assert steps == [(cnode, [d, e])] and path == [d, cnode] == m.paths[2]


def test_fan_input_is_what_it_claims():
    c, g, m = cpu("graph_fan"), graph("graph_fan"), model("graph_fan")
    assert len(g.preds[130]) == 130 and g.first == [0, 130, 131]
    assert m.edits.tolist() == [0, 0, 0, 1, 0] and [p[0] for p in m.paths[:4]] == [0, 64, 128, 5]      # 16 rows share the six symbols and m.paths[4] == [130]
    assert all(w == (0, 1) for w in m.windows[:4]) and m.stats["merges"] >= 4 * 130


def test_bounds_and_gaps_inputs_are_what_they_claim():
    g, m = graph("bounds"), model("bounds")
    ones = [j for j in range(g.nb) if g.minlen[j] == 1]
    assert len(ones) == 12
    assert any({g.block_of[v] for v in p} >= set(ones) for p in m.paths)            # a path through the twelve blocks
    c, g = cpu("gaps"), graph("gaps")
    r = 2                                                                         # the row with an all-gap middle block
    assert c.rm.node_of[r][1] is None and (c.rm.node_of[r][0], c.rm.node_of[r][2]) not in g.edges
    assert all(g.block_of[v] == g.block_of[u] + 1 for u, v in g.edges)


def test_lengths_input_is_what_it_claims():
    c, g, m = cpu("graph_lengths"), graph("graph_lengths"), model("graph_lengths")
    assert [len(r) for r in c.reads] == list(LENGTHS) and all(g.first[j + 1] - g.first[j] == 2 for j in range(g.nb))
    assert m.stats["too_long"] == 1 and m.edits[-1] == NONE and m.edits[0] == NONE            # no seed in one symbol
    assert m.edits[1:-1].tolist() == [2] * 10
    for k in range(1, len(LENGTHS) - 1):
        assert m.n_path[k] >= 2 and m.stats["merges"] > 0
        if k % 2:                                                                 # recombinant: nodes of both haplotypes
            assert {(v - g.first[g.block_of[v]]) for v in m.paths[k]} == {0, 1}, k


# ---- GPU ----------------------------------------------------------------------------------------------------------

def c_graph(pix, n, pad=16, max_cells=0, select=None, want=(1,) * 6):
    """The C ABI: -> the six arrays, path_off, path_nodes, device_ms."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    arr = [np.full(n + 1, 7, dtype=np.uint32) for _ in range(6)]
    ms, total = ctypes.c_double(0), ctypes.c_uint64(99)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
    rc = L.fbg_pindex_chains_align_graph(pix._h, pad, max_cells, None if sel is None else sel.ctypes.data_as(_lib.u8p),
                                         *[a.ctypes.data_as(_lib.u32p) if w else None for a, w in zip(arr, want)], ctypes.byref(total),
                                         ctypes.byref(ms))
    assert rc == 0, (rc, pix._eng._chk)
    assert all(a[n] == 7 for a in arr)                 # nothing past the n entries
    off = np.full(n + 2, 7, dtype=np.uint64)
    nodes = np.full(total.value + 1, 7, dtype=np.uint32)
    assert L.fbg_pindex_chains_align_graph_fetch(pix._h, off.ctypes.data_as(_lib.u64p), nodes.ctypes.data_as(_lib.u32p)) == 0
    assert off[n + 1] == 7 and nodes[total.value] == 7 and off[n] == total.value
    return [a[:n] for a in arr], off[:n + 1], nodes[:total.value], ms.value


def same(got, off, nodes, m, what):
    for f, a in zip(GM.FIELDS, got):
        want = getattr(m, f)
        assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want), (what, f, a.tolist(), want.tolist())
    assert off.dtype == m.path_off.dtype and np.array_equal(off, m.path_off), (what, "path_off")
    assert nodes.dtype == m.path_nodes.dtype and np.array_equal(nodes, m.path_nodes), (what, "path_nodes", nodes.tolist(), m.path_nodes.tolist())


def same_python(ch, m, what):
    got = (ch.graph_edits, ch.graph_start[:, 0], ch.graph_start[:, 1], ch.graph_end[:, 0], ch.graph_end[:, 1],
           np.diff(ch.graph_path_off.astype(np.int64)).astype(np.uint32))
    same(got, ch.graph_path_off, ch.graph_path_nodes, m, what)
    for R in range(len(m.paths)):
        assert ch.graph_path(R).tolist() == m.paths[R]


def seeded(pix, c, strands):
    return pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=strands, rows=True)


def chained(pix, c, by_row, **kw):
    return pix.chains(band=c.band, min_score=c.min_score, by_row=by_row, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("by_row", [False, True])
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_input_through_both_interfaces(engine, name, strands, by_row):
    """Every input after plain and after by-row chains, at pads 16, 0, 2^40 and 2^64 - 1, with a cell limit at the median
    of the input's cells, with every other read selected and with none; `tiers` at pad 16 only."""
    c, g = cpu(name, strands, by_row), graph(name)
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.graph_align_stats() == dict.fromkeys(pix.GRAPH_STATS, 0)
        seeded(pix, c, strands)
        ch = chained(pix, c, by_row)
        assert np.array_equal(ch.chain_off, c.chain_off) and np.array_equal(ch.anchor_place, c.anchor_place)
        assert ch.graph_edits is None and ch.graph_path_off is None and ch.best_graph_edits is None
        for pad in PADS if name not in LONG else PADS[:1]:
            m = model(name, strands, by_row, pad)
            got, off, nodes, ms = c_graph(pix, n, pad)
            same(got, off, nodes, m, (name, pad, "C"))
            assert pix.graph_align_stats() == stats_of(m, g), (name, pad)
            assert ms > 0 or m.stats["aligned"] == 0
            ch = chained(pix, c, by_row, graph=True, graph_pad=pad)
            same_python(ch, m, (name, pad, "python"))
            if strands:
                assert np.array_equal(ch.best_graph_edits, GM.best_edits(m.edits, ch.strand)) and ch.best_graph_edits.dtype == np.uint32
            else:
                assert ch.best_graph_edits is None
        if name in LONG:
            return
        got, off, nodes, _ = c_graph(pix, n, 0xffffffffffffffff)
        same(got, off, nodes, model(name, strands, by_row, HUGE), (name, "2^64 - 1"))
        full = model(name, strands, by_row)
        cells = sorted(x for x in full.cells if x)
        if cells:
            limit = cells[len(cells) // 2]
            m = model(name, strands, by_row, 16, limit)
            assert m.stats["too_wide"] > 0 or cells[-1] == limit
            got, off, nodes, _ = c_graph(pix, n, 16, limit)
            same(got, off, nodes, m, (name, "max_cells"))
            assert pix.graph_align_stats() == stats_of(m, g)
        for sel in (tuple(R % 2 for R in range(n)), (0,) * n):
            m = model(name, strands, by_row, 16, 0, sel)
            got, off, nodes, _ = c_graph(pix, n, 16, 0, sel)
            same(got, off, nodes, m, (name, "select"))
            assert pix.graph_align_stats() == stats_of(m, g)
            same_python(chained(pix, c, by_row, graph=True, select=sel), m, (name, "select", "python"))


@pytest.mark.gpu
def test_word_and_tier_boundaries(engine):
    """Reads of 1 .. max_read + 1 symbols on the two-haplotype graph, every other one recombinant: every register tier
    and the LDS tier with merges and trace steps across nodes, and the skip; then each length alone."""
    c, g, m = cpu("graph_lengths"), graph("graph_lengths"), model("graph_lengths")
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        ch = chained(pix, c, False, graph=True)
        same_python(ch, m, "lengths")
        assert pix.graph_align_stats() == stats_of(m, g)
        for R, P in enumerate(c.reads):
            pix.seeds([P], min_length=c.L, max_per_seed=c.cap, msa=True)
            one = pix.chains(graph=True)
            assert int(one.graph_edits[0]) == int(m.edits[R]) and one.graph_path(0).tolist() == m.paths[R], len(P)
            assert one.graph_start[0].tolist() == [int(m.start_node[R]), int(m.start_offset[R])]
            assert one.graph_end[0].tolist() == [int(m.end_node[R]), int(m.end_offset[R])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chains", "graph_lengths", "graph_fan"])
def test_one_read_per_batch_gives_the_same_arrays(engine, name):
    from conftest import fbg_options
    c, g = cpu(name), graph(name)
    n = len(c.vreads)
    m, one = model(name), model(name, batch_kib=1)
    assert m.stats["batches"] == 1 and dict(m.stats, batches=0) == dict(one.stats, batches=0)
    assert 1 < one.stats["batches"] <= one.stats["aligned"]
    if name == "graph_fan":
        assert one.stats["batches"] == one.stats["aligned"]              # 131 nodes: the columns of one read exceed the KiB
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        chained(pix, c, False)
        got, off, nodes, _ = c_graph(pix, n)
        same(got, off, nodes, m, (name, "default"))
        assert pix.graph_align_stats() == stats_of(m, g)
        with fbg_options(engine, {"graph_batch_kib": 1}):
            got, off, nodes, _ = c_graph(pix, n)
            same(got, off, nodes, one, (name, "one KiB"))
            assert pix.graph_align_stats() == stats_of(one, g)


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    dummy = [np.zeros(4096, dtype=np.uint32) for _ in range(6)]
    call = lambda h: L.fbg_pindex_chains_align_graph(h, 16, 0, None, *[u32(a) for a in dummy], None, None)      # noqa: E731
    fetch = lambda h: L.fbg_pindex_chains_align_graph_fetch(h, None, None)      # noqa: E731
    c, g, m = cpu("chains"), graph("chains"), model("chains")
    mb = model("chains", False, True)
    n = len(c.reads)
    assert call(None) == _lib.FBG_ERR_INVALID and fetch(None) == _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_align_graph_stats(None, *[None] * 10) == _lib.FBG_ERR_INVALID
    with TR.build(engine, c.A, c.b, rows=False) as plain, TR.build(engine, c.A, c.b) as pix:
        # no row table
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(plain._h) == _lib.FBG_ERR_INVALID and fetch(plain._h) == _lib.FBG_ERR_INVALID
        for f in (lambda: plain.chains(graph=True), plain.graph_align_stats):
            with pytest.raises(FbgError) as ei:
                f()
            assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
        # no seeds call yet; seeds without chains; chains without the call
        assert call(pix._h) == _lib.FBG_ERR_INVALID
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True)
        assert call(pix._h) == _lib.FBG_ERR_INVALID and fetch(pix._h) == _lib.FBG_ERR_INVALID
        # no reads; reads without seeds
        pix.seeds([], msa=True, chain=True)
        assert call(pix._h) == 0 and fetch(pix._h) == 0
        e = pix.chains(graph=True)
        assert len(e.graph_edits) == 0 and e.graph_edits.dtype == np.uint32 and e.graph_path_off.tolist() == [0]
        pix.seeds([b"NN", b""], msa=True, chain=True)
        got, off, nodes, _ = c_graph(pix, 2)
        assert all(a.tolist() == [NONE, NONE] for a in got[:5]) and got[5].tolist() == [0, 0] and off.tolist() == [0, 0, 0]
        assert pix.graph_align_stats() == dict.fromkeys(pix.GRAPH_STATS, 0)
        # repeated calls, with and without the optional arrays; the row alignment and its paths untouched, and the reverse
        seeded(pix, c, False)
        ch = chained(pix, c, False, rows=True, align=True, cigar=True)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID           # before the call
        before = (pix.align_stats(), pix.cigar_stats(), pix.rows_stats(), pix.chain_stats())

        def row_state():
            arr = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
            coff, ops = np.zeros(n + 1, dtype=np.uint64), np.zeros(len(ch.cigar_ops) + 1, dtype=np.uint32)
            assert L.fbg_pindex_chains_cigar_fetch(pix._h, coff.ctypes.data_as(_lib.u64p), u32(ops)) == 0
            return [a.tolist() for a in (coff, ops)]
        paths = row_state()
        assert paths[0] == ch.cigar_off.tolist()
        for want in ((1,) * 6, (0, 1, 0, 0, 0, 0), (0,) * 6, (1,) * 6):
            got, off, nodes, _ = c_graph(pix, n, want=want)
            for f, a, w in zip(GM.FIELDS, got, want):
                assert np.array_equal(a, getattr(m, f)) if w else (a == 7).all(), (f, want)
            assert np.array_equal(off, m.path_off) and np.array_equal(nodes, m.path_nodes)
            assert pix.graph_align_stats() == stats_of(m, g)
        assert (pix.align_stats(), pix.cigar_stats(), pix.rows_stats(), pix.chain_stats()) == before and row_state() == paths
        arr = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
        assert L.fbg_pindex_chains_align(pix._h, 16, 0, *[u32(a) for a in arr], None) == 0
        assert L.fbg_pindex_chains_cigar(pix._h, None, None, None) == 0
        assert np.array_equal(arr[1], ch.edits) and row_state() == paths
        off, nodes = np.zeros(n + 1, dtype=np.uint64), np.zeros(len(m.path_nodes) + 1, dtype=np.uint32)
        assert L.fbg_pindex_chains_align_graph_fetch(pix._h, off.ctypes.data_as(_lib.u64p), u32(nodes)) == 0
        assert np.array_equal(off, m.path_off) and np.array_equal(nodes[:-1], m.path_nodes)      # the graph result outlives them
        # a locate and an occurrences call overwrite the reads on the device
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        got, off, nodes, _ = c_graph(pix, n)
        same(got, off, nodes, m, "after locate")
        # a failed call leaves the stats
        assert call(None) == _lib.FBG_ERR_INVALID and pix.graph_align_stats() == stats_of(m, g)
        # a chaining call of either kind invalidates the result and the fetch
        chained(pix, c, True)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID
        got, off, nodes, _ = c_graph(pix, n)
        same(got, off, nodes, mb, "by row")
        chained(pix, c, False)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID
        same(*c_graph(pix, n)[:3], m, "plain again")
        # and so does a seeds call, which also takes the chains away
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID and call(pix._h) == _lib.FBG_ERR_INVALID


# ---- the tool ------------------------------------------------------------------------------------------------------------

def test_tool_graph_align_needs_its_prerequisites():
    import subprocess
    import test_chains as TC
    assert os.path.exists(TC.LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([TC.LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--graph-align" in p.stderr
    base = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0]]
    for extra in (["--chain=2", "--graph-align"], ["--rows", "--graph-align=4"], ["--graph-align"]):
        p = subprocess.run([TC.LOCATE] + base + extra, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--graph-align needs --chain and --rows" in p.stderr and b"usage:" in p.stderr
    p = subprocess.run([TC.LOCATE] + base + ["--chain", "--rows", "--graph-align=x"], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--graph-align takes a pad" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", ["recombinant", "chains"])
def test_tool_prints_the_graph_alignments(engine, name, strands, tmp_path):
    """fbg_locate --graph-align adds one H line after the lines of every chain, formatted here from the model on the tool's
    chains (unbounded band, no minimum score); every other byte of the output is what it is without the flag."""
    import chain_model as CM
    import test_chains as TC
    from types import SimpleNamespace
    from oracle import pyoracle as O
    c, g = cpu(name, strands), graph(name)
    off, _, place, seed = CM.chains(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, None, 0)
    c2 = SimpleNamespace(**dict(vars(c), chain_off=off, anchor_place=place, anchor_seed=seed))
    xgfa, fasta = str(tmp_path / "g.xgfa"), str(tmp_path / "g.fasta")
    O.write_xgfa(c.A, c.b, xgfa)
    with open(fasta, "wb") as fh:
        for r, row in enumerate(c.A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))
    ids = [ln.split(b"\t")[1] for ln in open(xgfa, "rb").read().splitlines() if ln.startswith(b"S\t")]
    assert len(ids) == len(g.labels)
    keep = [R for R, r in enumerate(c.reads) if r]                  # the tool reads whitespace-separated tokens
    data = b"".join(c.reads[R] + b"\n" for R in keep)
    n = len(c.reads)
    v_of = (lambda i: keep[i // 2] + (i % 2) * n) if strands else (lambda i: keep[i])
    args = ["--graph=" + xgfa, "--msa=" + fasta, "--seeds=%d" % c.L, "--occurrences=%d" % c.cap, "--chain", "--rows"] + \
        (["--strands"] if strands else [])
    for more in ([], ["--align"]):
        plain = TC.TL.run_locate(args + more, data)
        assert plain.returncode == 0 and b"\nH\t" not in plain.stdout, plain.stderr
        for flag, pad in (("--graph-align", 16), ("--graph-align=0", 0)):
            m = GM.of_cpu(g, c2, pad)
            got = TC.TL.run_locate(args + more + [flag], data)
            assert got.returncode == 0, got.stderr
            want, i, wait = [], 0, None
            for ln in plain.stdout.splitlines(keepends=True):
                want.append(ln)
                if ln.startswith(b"C\t"):
                    wait = [int(ln.split(b"\t")[2]) + len(more), v_of(i)]
                    i += 1
                if wait is not None:
                    if wait[0] == 0:
                        v = wait[1]
                        want.append(b"H\t*\n" if m.edits[v] == NONE else b"H\t%d\t%s\t%d\t%s\t%d\t%s\n" % (
                            m.edits[v], ids[m.start_node[v]], m.start_offset[v], ids[m.end_node[v]], m.end_offset[v],
                            b"".join(b">" + ids[u] for u in m.paths[v])))
                        wait = None
                    else:
                        wait[0] -= 1
            assert wait is None and i == len(keep) * (2 if strands else 1)
            assert got.stdout == b"".join(want)
            assert b"".join(ln for ln in got.stdout.splitlines(keepends=True) if not ln.startswith(b"H\t")) == plain.stdout
        assert (m.edits != NONE).any() and ((m.edits == NONE).any() or name != "chains")
    if name == "recombinant":
        R = len(c.reads) - 1
        assert m.edits[R] == 0 and b"H\t0\t" in got.stdout and got.stdout.count(b">") >= 3
