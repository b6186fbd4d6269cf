"""Graph alignment, graph CIGAR and the GAF writer on long edited reads, a wide graph, many reads and many batches:
fbg_pindex_chains_align_graph (csrc/pindex_graph.hip), fbg_pindex_chains_graph_cigar (k_pj_sizes, k_pj_gather of
csrc/pindex_gcigar.hip and pg_trace of csrc/pindex_align.hip on PjState) and fbg_locate --graph-cigar --gaf, between the toy
inputs of test_align_graph.py and test_graph_cigar.py and the workload of scripts/gpu_graph_cigar_bench.py.

The checkers are tests/graph_align_model.py (a column at a time in numpy), tests/graph_cigar_model.py and tests/cigar_model.py
(a row at a time in numpy: LITERAL_CELLS is lowered for the length of a call); every comparison with the engine is exact and
every model result is computed once per process.  The inputs, and what each adds:

  long_edits  of test_align_scale.py: the MSA and segmentation of `founders` (200 rows, 140 blocks, 1,437 nodes, up to 17
              nodes a block, labels of 1 to 18 symbols) and reads of 64 .. 1025 symbols with planted X, I, D and foreign
              bytes (0 and N).  This file runs K = 6 of every REPS = 12 of them and the two tail reads (see below): 176
              reads, 352 virtual reads, all 29 lengths.  test_align_graph_scale.py has the wide graph with reads of at most
              120 symbols, test_align_graph.py and test_graph_cigar.py have reads above two words on a graph of two rows,
              two nodes a block and a dozen reads.  Here every word count 1 .. 16 (each register tier, the LDS-state tier,
              the device-history tier of the trace) meets blocks of 17 nodes, paths of 5 to 99 nodes and hundreds of other
              reads; N (from a path, not a window) lies on both sides of L; the batches of graph_batch_kib and of
              path_batch_kib hold several reads, reads without history and unaligned reads between them; k_pj_sizes runs
              two workgroups, k_pj_gather on labels that are all shorter than a wave, most reads starting inside a label.
              A path of one node cannot occur: the shortest read has 64 symbols and the longest label 18.
  bytes       of test_align_scale.py: bytes 0x80 .. 0xFE and lower case, on the graph calls for the first time (a signed
              comparison or an alphabet assumption in pindex_graph.hip would show).
  founders, m17, m128   of test_align_graph_scale.py, with its models: 8,042 virtual reads (32 workgroups of k_pj_sizes),
              thousands of them without a result between the aligned ones, through k_pj_sizes, k_pj_gather and the scans
              over n + 1.

Time.  With all 350 reads of long_edits the graph model takes 34 s after plain and 27 s after by-row chains and the cigar
models 4 s and 3 s; on an MI355X test_long_edits_in_batches then takes 16.9 s (plain) and 14.6 s (by-row) of GPU-side time,
above the target of 10 s a test: one read a batch (graph_batch_kib = 1) runs the reads one wave after the other, 4.6 s of
device time for the 301 aligned reads of K = 7 where the default takes 59 ms, and the batches of 1024 KiB take 1.5 s a call.
With K = 7 the plain case took 10.07 s; with K = 6, the largest that meets the target, test_long_edits_in_batches takes
8.7 s (plain) and 7.5 s (by-row).  Every other GPU test of this file takes about a second or less beside its models
(pytest --durations with the models computed by an earlier test: test_long_edits 0.09 s a case, the C calls 0.14 s, each
founders case under 1.5 s, m17 and m128 under 1 s with their models, the selection 3.8 s with its model, large-small-large
0.25 s, bytes 0.02 s, the tool 1.1 s).  The models of the K = 6 reads take about 13 s and 11 s (graph) and 2 s each (cigar) on the CPU, every other aligned
read selected 7 s; founders 42 s and 12 s, shared with test_align_graph_scale.py in a run of the whole suite; the CPU tests
of this file alone about 75 s.  Pad 0 is left to test_graph_cigar.py for that reason.

With K = 6 the counts of the whole input that the CPU tests ask for (400 and 350 aligned reads, 200 with device history)
are asked for in proportion, K / REPS of them; every other condition is asked of the reads of this file as it stands."""
import collections
import functools
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import byrow_model as BM  # noqa: E402
import chain_model as CM  # noqa: E402
import cigar_model as CG  # noqa: E402
import graph_align_model as GM  # noqa: E402
import graph_cigar_model as JM  # noqa: E402
import test_align_graph as TG  # noqa: E402
import test_align_graph_scale as GS  # noqa: E402
import test_align_scale as AS  # noqa: E402
import test_chains as TC  # noqa: E402
import test_mapping_scale as TM  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options  # noqa: E402
from test_graph_cigar import c_gcigar, same, same_chains  # noqa: E402

NONE = GM.NONE
HUGE = GS.HUGE
CHAINS = ("plain", "by_row")
BUDGET_SHARED, BUDGET_EACH = AS.BUDGET_SHARED, AS.BUDGET_EACH      # path_batch_kib and graph_batch_kib alike
SCALE = (("founders", "plain", 16), ("founders", "by_row", 16), ("m17", "plain", HUGE), ("m128", "plain", HUGE))
K = 6                          # of every REPS = 12 reads of test_align_scale.long_edits_input, and its two tail reads


# ---- the inputs and the models, each once -----------------------------------------------------------------------------------

def cached(f):
    """functools.lru_cache on the arguments with the defaults filled in: f(x) and f(x, default) are one entry."""
    sig, inner = inspect.signature(f), functools.lru_cache(maxsize=None)(f)

    @functools.wraps(f)
    def call(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        return inner(*bound.args)
    return call


def kept():
    """The reads of long_edits that this file runs."""
    cycled = AS.REPS * len(AS.LENGTHS)
    return [j for j in range(cycled + len(AS.TAIL_LENGTHS)) if j >= cycled or j % AS.REPS < K]


def subset(c, given):
    """What test_mapping_scale.cpu() would hold of the reads `given` of c alone, taken from c: the seeds, places and
    chains of their virtual reads with the indices between them renumbered.  origin: the virtual reads of c they were."""
    n = len(c.reads)
    v = list(given) + [n + R for R in given]
    so, po, co = (x.astype(np.int64) for x in (c.seed_off, c.start_off, c.chain_off))
    pieces = lambda lo, hi: np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)  # noqa: E731
    seeds, anchors = pieces(so[v], so[np.array(v) + 1]), pieces(co[v], co[np.array(v) + 1])
    places = pieces(po[so[v]], po[so[np.array(v) + 1]])                # the places of a read's seeds lie one after the other
    new_seed, new_place = np.full(len(c.q_start), -1, dtype=np.int64), np.full(len(c.start_col), -1, dtype=np.int64)
    new_seed[seeds], new_place[places] = np.arange(len(seeds)), np.arange(len(places))
    offsets = lambda counts: np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)      # noqa: E731
    out = SimpleNamespace(**{k: x for k, x in vars(c).items() if k not in ("solved", "places_per_read", "seed_of_place", "palindromes")})
    out.origin, out.reads, out.truth, out.vreads = v, [c.reads[R] for R in given], [c.truth[R] for R in given], [c.vreads[R] for R in v]
    out.seed_off, out.start_off, out.chain_off = offsets(np.diff(so)[v]), offsets(np.diff(po)[seeds]), offsets(np.diff(co)[v])
    for f in ("q_start", "length", "count", "restarts", "end_total", "start_total"):
        setattr(out, f, getattr(c, f)[seeds])
    for f in ("start_src", "start_dst", "start_offset", "start_row", "start_col", "n_rows", "first_row"):
        setattr(out, f, getattr(c, f)[places])
    out.sets = [c.sets[x] for x in places]
    place, seed = new_place[c.anchor_place[anchors].astype(np.int64)], new_seed[c.anchor_seed[anchors].astype(np.int64)]
    assert (place >= 0).all() and (seed >= 0).all()                    # a chain's anchors are its own read's
    out.anchor_place, out.anchor_seed = place.astype(np.uint32), seed.astype(np.uint32)
    for f in ("score", "chain_n_rows", "chain_first_row", "row_bits"):
        setattr(out, f, getattr(c, f)[v])
    out.chain_sets = [c.chain_sets[R] for R in v]
    out.strand, out.best_score = c.strand[list(given)], c.best_score[list(given)]
    s = out.strand.tolist()
    out.strand_counts = dict(forward=s.count(0), reverse=s.count(1), none=s.count(TM.STRAND_NONE))
    return out


@cached
def cpu(name, chains="plain"):
    if name == "bytes":
        return AS.bytes_cpu()
    if name != "long_edits":
        return TM.cpu(name) if chains == "plain" else GS.by_row(name)
    if chains == "plain":
        return subset(AS.cpu(name), kept())
    c = cpu(name)
    return BM.as_cpu(c, BM.by_row(c, c.band, 0))


@cached
def graph(name):
    if name == "bytes":
        c = AS.bytes_cpu()
        return GM.Graph.of(c.A, c.b)
    if name == "long_edits":
        c = AS.cpu(name)
        return GM.Graph(*c.graph, len(c.b))
    return GS.graph(name)


@cached
def model(name, chains="plain", pad=16, select=None):
    if name in ("long_edits", "bytes"):
        return GM.of_cpu(graph(name), cpu(name, chains), pad, 0, select, rows_only=True)
    assert select is None
    return GS.model(name, chains, pad)                 # founders after plain chains: the reads of GS.unsupported


@cached
def gcigar(name, chains="plain", pad=16, select=None):
    with AS.by_rows(CG):
        return JM.of_graph(graph(name), cpu(name, chains), model(name, chains, pad, select))


@cached
def row_alignment():
    """test_align_scale.aligned("long_edits"), the row alignment after plain chains, for the reads of this file."""
    am, v = AS.aligned("long_edits"), cpu("long_edits").origin
    return SimpleNamespace(edits=am.edits[v], row=am.row[v], windows=[am.windows[R] for R in v])


def history(c, m, gc):
    """Bytes of device history per virtual read (0: none, or no alignment)."""
    return [CG.history_bytes(len(c.vreads[R]), len(gc.texts[R])) if m.edits[R] != NONE else 0 for R in range(len(c.vreads))]


def graph_batches(g, c, m, kib):
    """The batches of the graph call under graph_batch_kib = kib: graph_align_model.batches_of on the scratch of every
    aligned read, the nodes of its window times two columns of its word count."""
    sizes = [0] * len(c.vreads)
    for R, w in enumerate(m.windows):
        if m.edits[R] != NONE:
            sizes[R] = (g.first[w[1] + 1] - g.first[w[0]]) * 2 * AS.words(len(c.vreads[R]))
    return GM.batches_of(sizes, kib)


def with_letter(gc, R, code):
    return any(k == code for k, _ in gc.runs[R])


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

FLOOR = {"plain": 400, "by_row": 350, "history": 200}      # of the whole input; this file's share of it is K / REPS


def floor(what):
    return FLOOR[what] * K // AS.REPS


@pytest.mark.parametrize("chains", CHAINS)
def test_long_edits_is_what_the_graph_calls_need(chains):
    """gcigar() runs graph_cigar_model.of_graph over the whole input, which asserts lev(P, T) == edits and N <= L + edits
    for every aligned read."""
    c, g, m, gc = cpu("long_edits", chains), graph("long_edits"), model("long_edits", chains), gcigar("long_edits", chains)
    n, nv = len(c.reads), len(c.vreads)
    ok = [R for R in range(nv) if m.edits[R] != NONE]
    L = {R: len(c.vreads[R]) for R in ok}
    N = {R: len(gc.texts[R]) for R in ok}
    assert nv == 2 * n and len(ok) == m.stats["aligned"] == gc.stats["paths"] >= floor(chains) and m.stats["too_long"] >= 1
    assert max(g.first[j + 1] - g.first[j] for j in range(g.nb)) == 17 and len(g.labels) > 1400
    assert max(len(x) for x in g.labels) < 64                                # every label shorter than a wave
    # every word count: a read, an I, a D
    per = collections.Counter(AS.words(L[R]) for R in ok)
    with_i = {AS.words(L[R]) for R in ok if with_letter(gc, R, CG.I)}
    with_d = {AS.words(L[R]) for R in ok if with_letter(gc, R, CG.D)}
    every = set(range(1, 17))
    assert all(per[w] >= 1 for w in every) and with_i == every and with_d == every, (per, with_i, with_d)
    # paths of few nodes and of many; N on either side of L; starts inside a label, ends at a label's end
    # (a path of one node cannot occur here: the shortest read has 64 symbols and the longest label 18; that case is
    # test_graph_cigar.test_gather_edges_occur_in_the_inputs')
    assert max(len(m.paths[R]) for R in ok) >= 64 and 2 <= min(len(m.paths[R]) for R in ok) <= 8
    longer, shorter = sum(N[R] > L[R] for R in ok), sum(N[R] < L[R] for R in ok)
    assert longer > 0 and shorter > 0
    assert all(N[R] <= L[R] + int(m.edits[R]) for R in ok)
    heavy = [R for R in ok if AS.words(L[R]) >= 5 and 4 * int(m.edits[R]) > L[R]]
    assert heavy
    inside = sum(m.start_offset[R] > 0 for R in ok)
    full = sum(int(m.end_offset[R]) == len(g.labels[m.paths[R][-1]]) for R in ok)
    assert inside > 0 and full > 0 and any(m.start_offset[R] == 0 for R in ok)
    # both strands; the bytes that no label holds
    reverse = sum(R >= n for R in ok)
    zero, enn = sum(0 in c.vreads[R] for R in ok), sum(ord("N") in c.vreads[R] for R in ok)
    assert reverse > 0 and len(ok) - reverse > 0 and zero > 0 and enn > 0
    # the histories in device memory and the batches of the trace
    hist = history(c, m, gc)
    assert [hist[R] for R in ok] == gc.hist and gc.stats["history_bytes"] == sum(hist) and gc.stats["batches"] == 1
    long_reads = [R for R, h in enumerate(hist) if h]
    assert len(long_reads) >= floor("history")
    shared, each = AS.batch_ranges(hist, BUDGET_SHARED << 10), AS.batch_ranges(hist, BUDGET_EACH << 10)
    assert len(shared) == CG.batches(gc.hist, BUDGET_SHARED << 10) >= 10
    several = [b for b in shared if len(b) >= 2]
    assert len(several) >= 2
    assert len(each) == CG.batches(gc.hist, BUDGET_EACH << 10) == len(long_reads) and min(h for h in hist if h) > BUDGET_EACH << 10
    between = sum(any(hist[R] == 0 for R in range(b[0], b[-1])) for b in several)
    unaligned_between = sum(any(m.edits[R] == NONE for R in range(b[0], b[-1])) for b in several)
    assert between > 0 and unaligned_between > 0
    # the batches of the graph call
    gb = {kib: graph_batches(g, c, m, kib) for kib in (1 << 20, BUDGET_SHARED, BUDGET_EACH)}
    assert gb[1 << 20] == m.stats["batches"] == 1 and 1 < gb[BUDGET_SHARED] < len(ok) and gb[BUDGET_SHARED] < gb[BUDGET_EACH] <= len(ok)
    print("long_edits", chains, dict(virtual_reads=nv, with_a_chain=int((np.diff(c.chain_off.astype(np.int64)) > 0).sum()), aligned=len(ok),
                                     too_long=m.stats["too_long"], per_word_count=[per[w] for w in range(1, 17)],
                                     path_nodes=(min(len(m.paths[R]) for R in ok), max(len(m.paths[R]) for R in ok)),
                                     N_above_L=longer, N_below_L=shorter, N_minus_L=(min(N[R] - L[R] for R in ok), max(N[R] - L[R] for R in ok)),
                                     most_edits=max(int(m.edits[R]) for R in ok), heavy=len(heavy), start_inside=inside, end_at_label_end=full,
                                     reverse=reverse, zero_byte=zero, N_byte=enn, runs=gc.stats["ops"], history_reads=len(long_reads),
                                     history_bytes=(min(h for h in hist if h), max(hist), sum(hist)),
                                     path_batches={BUDGET_SHARED: len(shared), BUDGET_EACH: len(each)}, several=len(several),
                                     graph_batches=gb))


def test_the_filter_gives_what_the_pipeline_gives_on_the_reads_alone():
    """subset() against test_mapping_scale.cpu() on a few reads as an input of their own (every 40th read of this file's),
    and the whole input filtered to all of its reads against itself."""
    from unittest import mock
    c = cpu("long_edits")
    given = list(range(0, len(c.reads), 40))
    with mock.patch.dict(TM.INPUTS, {"some_of_long_edits": lambda: (c.A, [c.reads[R] for R in given], [c.truth[R] for R in given], c.high)}):
        alone = TM.cpu("some_of_long_edits")
    full = AS.cpu("long_edits")
    for got, want in ((subset(c, given), alone), (subset(full, range(len(full.reads))), full)):
        assert got.reads == want.reads and got.vreads == want.vreads and got.truth == want.truth
        for f in TR.SEED_FIELDS + TR.PLACE_FIELDS + TR.CHAIN_FIELDS + ("count", "restarts", "end_total", "start_total", "n_rows", "first_row",
                                                                    "chain_n_rows", "chain_first_row", "row_bits", "strand", "best_score"):
            a, b = getattr(got, f), getattr(want, f)
            assert a.dtype == b.dtype and np.array_equal(a, b), f
        assert got.sets == want.sets and got.chain_sets == want.chain_sets and got.strand_counts == want.strand_counts
    assert len(alone.q_start) > 20 and len(alone.anchor_place) > 10


def planted_stretch(t):
    """The symbols [a, end) of the row a read of long_edits was cut from that its planted edits lay it on."""
    row, a, L, strand, planted, plan = t
    return a, a + L - sum(k == "I" for _, k in plan) + sum(len(k) for _, k in plan if k in ("D", "DD"))


@pytest.mark.parametrize("chains", CHAINS)
def test_long_edits_graph_edits_against_the_rows_and_the_planted_edits(chains):
    """The ground truth outside the graph models.  A row is a path of the graph, so (a) wherever the row alignment's window
    lies inside the blocks of the graph's window and the row has a node in each of them, graph_edits <= the row's edits
    (test_align_graph.inequality, against the row alignment of the plain chains: either side is a minimum over its own
    window, whichever chains made the window); (b) where the chain is on the strand the read was cut from and the stretch
    of its row that the planted edits lay it on is inside the graph's window, graph_edits <= the planted cost (X, I, D one
    each, a deletion of two symbols two, the foreign byte one).  At least 20 reads are judged in (b) among those whose row
    alignment found the row they were cut from."""
    c, g, m, am = cpu("long_edits", chains), graph("long_edits"), model("long_edits", chains), row_alignment()
    n = len(c.reads)
    checked = TG.inequality(g, c, m, am)
    assert checked >= 20
    judged = true_row = exact = 0
    for R, t in enumerate(c.truth):
        row, a, L, strand, planted, plan = t
        v = strand * n + R
        if int(c.strand[R]) != strand or m.edits[v] == NONE:
            continue
        jl, jh = m.windows[v]
        if any(c.rm.node_of[row][j] is None for j in range(jl, jh + 1)):
            continue
        x0, x1 = planted_stretch(t)
        end = c.rm.p[row][jh + 1] if jh + 1 < g.nb else len(c.rm.G[row])
        if not (c.rm.p[row][jl] <= x0 and x1 <= end):
            continue
        judged += 1
        true_row += am.edits[v] != NONE and int(am.row[v]) == row
        exact += int(m.edits[v]) == planted
        assert int(m.edits[v]) <= planted, (R, int(m.edits[v]), plan)
    print("long_edits", chains, "ground truth", dict(reads=n, graph_at_most_row=checked, judged=judged, of_them_true_row=true_row,
                                                     edits_equal_planted=exact))
    assert true_row >= 20


def test_bytes_input_is_what_it_claims_on_the_graph():
    c, g, m, gc = cpu("bytes"), graph("bytes"), model("bytes"), gcigar("bytes")
    assert min(min(r) for r in c.reads) >= 0x61 and max(max(r) for r in c.reads) >= 0xf0
    assert all(any(x >= 0x80 for x in r) and any(x < 0x80 for x in r) for r in c.reads)
    assert gc.strings == ["17=1X17=1I17=1D17=", "32=1X32=1I32=1D32=", "82=1X82=1I82=1D82="]
    assert m.edits.tolist() == [3, 3, 3] and [len(p) for p in m.paths] == [2, 4, 8] and {len(x) for x in g.labels} == {50}
    print("bytes on the graph", gc.strings, m.paths)


@pytest.mark.parametrize("name,chains,pad", SCALE)
def test_scale_inputs_have_what_the_graph_cigar_needs(name, chains, pad):
    c, m, gc = cpu(name, chains), model(name, chains, pad), gcigar(name, chains, pad)
    nv = len(c.vreads)
    indel = sum(any(k in (CG.I, CG.D) for k, _ in r) for r in gc.runs)
    zero_between = sum(gc.off[R] == gc.off[R + 1] and 0 < gc.off[R] < gc.off[-1] for R in range(nv))
    assert gc.stats["paths"] == m.stats["aligned"] > 100 and gc.stats["history_bytes"] == 0 and gc.stats["batches"] == 0
    if name == "founders":
        assert nv > 8000                                             # k_pj_sizes: 32 workgroups
        if chains == "by_row":
            assert gc.stats["paths"] > 1000 and indel > 100 and zero_between > 100
        else:
            assert zero_between > 1000 and nv - gc.stats["paths"] > 6000
    print(name, chains, dict(virtual_reads=nv, paths=gc.stats["paths"], runs=gc.stats["ops"], columns=gc.stats["columns"], with_indel=indel,
                             zero_between=zero_between))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def traced(pix, c, chains, pad=16, select=None):
    return pix.chains(band=c.band, min_score=0, by_row=chains != "plain", graph=True, graph_pad=pad, select=select, graph_cigar=True)


def arrays(ch):
    out = [ch.graph_edits, ch.graph_start, ch.graph_end, ch.graph_path_off, ch.graph_path_nodes, ch.graph_cigar_off, ch.graph_cigar_ops]
    return [a.tolist() for a in out] + ([ch.best_graph_edits.tolist()] if ch.best_graph_edits is not None else [])


def check(pix, ch, c, g, m, gc, what, graph_batches=None, path_batches=None):
    """The arrays and statistics of a chains(graph=True, graph_cigar=True) call against the models."""
    assert np.array_equal(ch.chain_off, c.chain_off) and np.array_equal(ch.anchor_place, c.anchor_place), what
    TG.same_python(ch, m, what)
    want = TG.stats_of(m, g) if graph_batches is None else dict(TG.stats_of(m, g), batches=graph_batches)
    assert pix.graph_align_stats() == want, (what, pix.graph_align_stats(), want)
    if ch.strand is not None:
        want = GM.best_edits(m.edits, ch.strand)
        assert ch.best_graph_edits.dtype == want.dtype and np.array_equal(ch.best_graph_edits, want), what
    else:
        assert ch.best_graph_edits is None
    same(ch.graph_cigar_off, ch.graph_cigar_ops, gc, what)
    assert np.diff(ch.graph_cigar_off.astype(np.int64)).tolist() == [len(r) for r in gc.runs], what
    want = gc.stats if path_batches is None else dict(gc.stats, batches=path_batches)
    assert pix.graph_cigar_stats() == want, (what, pix.graph_cigar_stats(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("chains", CHAINS)
def test_long_edits(engine, chains, strands):
    """Stranded, and plain with the virtual reads given as reads."""
    c, g, m, gc = cpu("long_edits", chains), graph("long_edits"), model("long_edits", chains), gcigar("long_edits", chains)
    with TR.build(engine, c.A, c.b) as pix:
        sd = TM.call(pix, c) if strands else TM.call(pix, c, reads=c.vreads, strands=False)
        TR.same_as_cpu(sd, cpu("long_edits"), "long_edits")
        ch = traced(pix, c, chains)
        assert (ch.strand is not None) == strands
        if strands and chains == "plain":
            assert np.array_equal(ch.strand, c.strand)
        check(pix, ch, c, g, m, gc, ("long_edits", chains, strands))
        same_chains(ch, gc, ("long_edits", chains, strands))
        assert pix.graph_cigar_stats()["history_bytes"] == sum(history(c, m, gc)) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("chains", CHAINS)
def test_long_edits_in_batches(engine, chains):
    """The budgets of test_long_edits_is_what_the_graph_calls_need for the graph call, for the trace and for both: the same
    arrays, the models' numbers of batches, and the options as they were afterwards."""
    c, g, m, gc = cpu("long_edits", chains), graph("long_edits"), model("long_edits", chains), gcigar("long_edits", chains)
    defaults = {k: engine.get_option(k) for k in ("graph_batch_kib", "path_batch_kib")}
    assert defaults == {"graph_batch_kib": 1 << 20, "path_batch_kib": 1 << 20}
    gb = {kib: graph_batches(g, c, m, kib) for kib in (BUDGET_SHARED, BUDGET_EACH)}
    pb = {kib: CG.batches(gc.hist, kib << 10) for kib in (BUDGET_SHARED, BUDGET_EACH)}
    assert 1 < gb[BUDGET_SHARED] < gb[BUDGET_EACH] and 10 <= pb[BUDGET_SHARED] < pb[BUDGET_EACH]
    with TR.build(engine, c.A, c.b) as pix:
        TM.call(pix, c)
        whole = traced(pix, c, chains)
        check(pix, whole, c, g, m, gc, "default")
        assert m.stats["batches"] == gc.stats["batches"] == 1
        want = arrays(whole)
        ms = {"default": (round(whole.graph_ms, 1), round(whole.graph_cigar_ms, 1))}
        for kib in (BUDGET_SHARED, BUDGET_EACH, BUDGET_SHARED):
            with fbg_options(engine, {"graph_batch_kib": kib}):
                ch = traced(pix, c, chains)
                check(pix, ch, c, g, m, gc, ("graph_batch_kib", kib), graph_batches=gb[kib])
            assert arrays(ch) == want, ("graph_batch_kib", kib)
            ms["graph_batch_kib", kib] = round(ch.graph_ms, 1)
        for kib in (BUDGET_SHARED, BUDGET_EACH, BUDGET_SHARED):
            with fbg_options(engine, {"path_batch_kib": kib}):
                ch = traced(pix, c, chains)
                check(pix, ch, c, g, m, gc, ("path_batch_kib", kib), path_batches=pb[kib])
            assert arrays(ch) == want, ("path_batch_kib", kib)
            ms["path_batch_kib", kib] = round(ch.graph_cigar_ms, 1)
        with fbg_options(engine, {"graph_batch_kib": BUDGET_SHARED, "path_batch_kib": BUDGET_SHARED}):
            ch = traced(pix, c, chains)
            check(pix, ch, c, g, m, gc, "both", graph_batches=gb[BUDGET_SHARED], path_batches=pb[BUDGET_SHARED])
        assert arrays(ch) == want, "both"
        assert {k: engine.get_option(k) for k in defaults} == defaults
        check(pix, traced(pix, c, chains), c, g, m, gc, "default again")
    print("long_edits", chains, "device ms of the graph call and of the trace", ms)


@pytest.mark.gpu
def test_long_edits_through_the_c_calls(engine):
    c, g, m, gc = cpu("long_edits"), graph("long_edits"), model("long_edits"), gcigar("long_edits")
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        TM.call(pix, c)
        got, poff, nodes, ms = TG.c_graph(pix, n)                              # guard words behind every array
        TG.same(got, poff, nodes, m, "C graph")
        assert ms > 0 and pix.graph_align_stats() == TG.stats_of(m, g)
        n_ops, total, off, ops, ms = c_gcigar(pix, n)
        same(off, ops, gc, "C graph cigar")
        assert n_ops.tolist() == [len(r) for r in gc.runs] and total == gc.stats["ops"] and ms > 0 and pix.graph_cigar_stats() == gc.stats
        ch = traced(pix, c, "plain")
        py = (ch.graph_edits, ch.graph_start[:, 0], ch.graph_start[:, 1], ch.graph_end[:, 0], ch.graph_end[:, 1], np.diff(ch.graph_path_off.astype(np.int64)))
        for f, a, b in zip(GM.FIELDS, got, py):
            assert np.array_equal(a, b), f
        assert np.array_equal(ch.graph_path_off, poff) and np.array_equal(ch.graph_path_nodes, nodes)
        assert np.array_equal(ch.graph_cigar_off, off) and np.array_equal(ch.graph_cigar_ops, ops)


@cached
def every_other_aligned():
    m = model("long_edits")
    ok = np.flatnonzero(m.edits != NONE)
    sel = np.zeros(len(m.edits), dtype=np.uint8)
    sel[ok[::2]] = 1
    return tuple(int(x) for x in sel)


@pytest.mark.gpu
def test_long_edits_with_every_other_aligned_read_selected(engine):
    c, g, full, fc = cpu("long_edits"), graph("long_edits"), model("long_edits"), gcigar("long_edits")
    sel = every_other_aligned()
    m, gc = model("long_edits", "plain", 16, sel), gcigar("long_edits", "plain", 16, sel)
    on = np.array(sel, dtype=bool)
    assert m.stats["aligned"] == int(on.sum()) == (full.stats["aligned"] + 1) // 2 and m.stats["not_selected"] == int((full.edits[~on] != NONE).sum()) \
        + full.stats["too_long"]
    assert 0 < gc.stats["history_bytes"] < fc.stats["history_bytes"]
    with TR.build(engine, c.A, c.b) as pix:
        TM.call(pix, c)
        whole = traced(pix, c, "plain")
        ch = traced(pix, c, "plain", select=sel)
        check(pix, ch, c, g, m, gc, "select")
        # the reads left out: no path, no runs
        assert (ch.graph_edits[~on] == NONE).all() and (np.diff(ch.graph_path_off.astype(np.int64))[~on] == 0).all()
        assert (np.diff(ch.graph_cigar_off.astype(np.int64))[~on] == 0).all()
        # the others: the rows of the whole call
        for f in ("graph_edits", "graph_start", "graph_end"):
            assert np.array_equal(getattr(ch, f)[on], getattr(whole, f)[on]), f
        for R in np.flatnonzero(on).tolist():
            assert ch.graph_path(R).tolist() == whole.graph_path(R).tolist() and ch.graph_cigar(R) == whole.graph_cigar(R) != "", R


@pytest.mark.gpu
@pytest.mark.parametrize("name,chains,pad", SCALE)
def test_scale_inputs(engine, name, chains, pad):
    """What test_align_graph_scale.run does, with the graph CIGAR: founders after plain chains (the reads whose chain no
    row carries) and after by-row chains, 17 and 128 rows with the whole graph as the window."""
    c, g, m, gc = cpu(name, chains), graph(name), model(name, chains, pad), gcigar(name, chains, pad)
    select = GS.unsupported(name) if chains == "plain" and name == "founders" else None
    with TR.build(engine, c.A, c.b) as pix:
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=True, rows=True)
        ch = traced(pix, c, chains, pad, select)
        check(pix, ch, c, g, m, gc, (name, chains))
        assert gc.stats["history_bytes"] == 0 and gc.stats["paths"] == m.stats["aligned"] > 100


@cached
def three_reads():
    """Three reads of long_edits (one with a history in device memory, a short one with a D, one without an alignment on
    either strand) as an input of their own -> (c, graph model, cigar model) after by-row chains."""
    c, m, gc = cpu("long_edits", "by_row"), model("long_edits", "by_row"), gcigar("long_edits", "by_row")
    n, hist = len(c.reads), history(c, m, gc)
    with_history = next(R for R in range(n) if hist[R])
    short = next(R for R in range(n) if m.edits[R] != NONE and len(c.reads[R]) <= 256 and with_letter(gc, R, CG.D))
    unaligned = next(R for R in range(n) if m.edits[R] == NONE and m.edits[n + R] == NONE)      # every such read is one too long
    given = sorted((with_history, short, unaligned))
    small = subset(cpu("long_edits"), given)
    small = BM.as_cpu(small, BM.by_row(small, small.band, 0))
    sm = GM.of_cpu(graph("long_edits"), small, 16, 0, None, rows_only=True)
    with AS.by_rows(CG):
        sg = JM.of_graph(graph("long_edits"), small, sm)
    # per read the models do not depend on the batch
    v = given + [n + R for R in given]
    assert sm.edits.tolist() == m.edits[v].tolist() and sm.paths == [m.paths[R] for R in v] and sg.runs == [gc.runs[R] for R in v]
    assert sg.stats["history_bytes"] > 0 and sg.stats["paths"] >= 2 and (sm.edits == NONE).sum() >= 2
    return small, sm, sg


@pytest.mark.gpu
def test_one_index_large_then_small_then_large(engine):
    """The founders batch, three reads of long_edits, a locate and an occurrences call (they overwrite the reads on the
    device), the three reads' chains again from the saved reads, the founders batch again: every array is a fresh index's and
    the model's, and the statistics follow each call.  A launch or a buffer sized by an earlier call's N or n would show."""
    f, g, fm, fg = cpu("founders", "by_row"), graph("founders"), model("founders", "by_row"), gcigar("founders", "by_row")
    c, m, gc = three_reads()
    assert np.array_equal(f.A, c.A) and f.b == c.b
    patterns = [r for r in f.vreads[:1500] if r] + [b"ACGT" * 400]
    with TR.build(engine, c.A, c.b) as fresh:
        TM.call(fresh, c)
        ch = traced(fresh, c, "by_row")
        check(fresh, ch, c, g, m, gc, "fresh")
        small = arrays(ch)
    with TR.build(engine, f.A, f.b) as pix:
        TM.call(pix, f)
        first = traced(pix, f, "by_row")                        # the first call of a fresh index
        check(pix, first, f, g, fm, fg, "first")
        large = arrays(first)
        TM.call(pix, c)
        ch = traced(pix, c, "by_row")
        check(pix, ch, c, g, m, gc, "small")
        assert arrays(ch) == small
        count = pix.locate(patterns)[0]
        assert (count > 0).sum() > 500
        pix.occurrences(patterns[:200], max_per_pattern=8)
        ch = traced(pix, c, "by_row")                           # the saved reads, shorter than the buffers
        check(pix, ch, c, g, m, gc, "small again")
        assert arrays(ch) == small
        TM.call(pix, f)
        again = traced(pix, f, "by_row")
        check(pix, again, f, g, fm, fg, "again")
        assert arrays(again) == large


@pytest.mark.gpu
def test_bytes_are_compared_as_they_are(engine):
    c, g, m, gc = cpu("bytes"), graph("bytes"), model("bytes"), gcigar("bytes")
    with TR.build(engine, c.A, c.b) as pix:
        sd = TG.seeded(pix, c, False)
        for f in TR.SEED_FIELDS:
            assert np.array_equal(getattr(sd, f), getattr(c, f)), f
        ch = TG.chained(pix, c, False, graph=True, graph_cigar=True)
        check(pix, ch, c, g, m, gc, "bytes")
        same_chains(ch, gc, "bytes")
        assert [ch.graph_cigar(R) for R in range(3)] == ["17=1X17=1I17=1D17=", "32=1X32=1I32=1D32=", "82=1X82=1I82=1D82="]
        assert ch.graph_edits.tolist() == [3, 3, 3]


# ---- the tool ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_tool_writes_gaf_for_long_edits(engine, tmp_path):
    """fbg_locate --strands --graph-align --graph-cigar --gaf=FILE on the reads of long_edits without a zero byte (the tool
    reads whitespace-separated tokens): stdout is the --graph-align output with the runs as eighth field, the file the
    model's records in the order of the H lines."""
    from oracle import pyoracle as O
    c, g = cpu("long_edits"), graph("long_edits")
    off, _, place, seed = CM.chains(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, None, 0)      # the tool's defaults
    assert np.array_equal(off, c.chain_off) and np.array_equal(place, c.anchor_place) and np.array_equal(seed, c.anchor_seed)
    m, gc = model("long_edits"), gcigar("long_edits")
    xgfa, fasta, gaf = str(tmp_path / "g.xgfa"), str(tmp_path / "g.fasta"), str(tmp_path / "g.gaf")
    O.write_xgfa(c.A, c.b, xgfa)
    with open(fasta, "wb") as fh:
        for r, row in enumerate(c.A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))
    ids = [ln.split(b"\t")[1] for ln in open(xgfa, "rb").read().splitlines() if ln.startswith(b"S\t")]
    assert len(ids) == len(g.labels)
    n = len(c.reads)
    keep = [R for R, r in enumerate(c.reads) if 0 not in r]
    assert len(keep) < n and any(ord("N") in c.reads[R] for R in keep)
    data = b"".join(c.reads[R] + b"\n" for R in keep)
    args = ["--graph=" + xgfa, "--msa=" + fasta, "--seeds=%d" % c.L, "--occurrences=%d" % c.cap, "--chain", "--rows", "--strands", "--graph-align"]
    base = TC.TL.run_locate(args, data)
    assert base.returncode == 0, base.stderr
    want, records, i = [], [], 0
    for ln in base.stdout.splitlines(keepends=True):
        if ln.startswith(b"H\t"):
            v = keep[i // 2] + (i % 2) * n
            if ln != b"H\t*\n":
                assert m.edits[v] != NONE and gc.strings[v]
                ln = ln[:-1] + b"\t" + gc.strings[v].encode() + b"\n"
                assert len(ln.split(b"\t")) == 8
                records.append(JM.gaf_fields(g, m, gc, v, i // 2, len(c.vreads[v]), v >= n, ids))
            else:
                assert m.edits[v] == NONE and gc.strings[v] == ""
            i += 1
        want.append(ln)
    assert i == 2 * len(keep)
    got = TC.TL.run_locate(args + ["--graph-cigar", "--gaf=" + gaf], data)
    assert got.returncode == 0, got.stderr
    assert got.stdout == b"".join(want)
    assert open(gaf, "rb").read() == b"".join(b"\t".join(r) + b"\n" for r in records)
    assert len(records) > 100 and any(r[4] == b"-" for r in records) and any(r[4] == b"+" for r in records)
    assert any(r[5].count(b">") > 32 for r in records)
