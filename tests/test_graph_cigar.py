"""The alignment path (CIGAR) of each read against the stretch of the graph its path spells, and the GAF writer:
fbg_pindex_chains_graph_cigar, _graph_cigar_fetch, fbg_pindex_graph_cigar_stats, PatternIndex.chains(graph=True,
graph_cigar=True) / .graph_cigar_stats() and fbg_locate --graph-cigar / --gaf (include/fbg_hip.h, csrc/pindex_gcigar.hip).

The checker is tests/graph_cigar_model.py, which composes graph_align_model (the path and its two offsets) and cigar_model
(the walk).  The inputs are those of tests/test_align_graph.py and one of this file's own, graph_indels: reads on the
two-haplotype graph with a deletion, an insertion and a substitution each, placed in runs of equal symbols so that every
read has several optimal alignments and the walk's preferences decide.  On the CPU the tests assert that the inputs hold
what they are meant to hold; on the GPU every array is compared exactly."""
import collections
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import chain_model as CM  # noqa: E402
import cigar_model as CG  # noqa: E402
import graph_align_model as GM  # noqa: E402
import graph_cigar_model as JM  # noqa: E402
import test_align_graph as TG  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402

LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_chains_graph_cigar", "fbg_pindex_chains_graph_cigar_fetch", "fbg_pindex_graph_cigar_stats")
NONE = GM.NONE
ZERO_STATS = dict(paths=0, ops=0, columns=0, history_bytes=0, batches=0)
INDEL_LENGTHS = (64, 65, 128, 129, 192, 193, 256, 257, 320)


# ---- this file's input ------------------------------------------------------------------------------------------------

def indel_input():
    """On the MSA of test_align_graph.length_input: read k of INDEL_LENGTHS[k] symbols starts at 31 + 67 k, is cut from
    haplotype 0 (even k) or recombinant at a block boundary inside it (odd k), and carries three edits: the first of two
    equal neighbours from a quarter on is deleted, the first of two equal neighbours from the half on is doubled, and the
    symbol at three quarters is rotated by two."""
    A, b, _, L0, cap, band, min_score = TG.length_input()
    h0, h1 = TG.length_haps()
    reads = []
    for k, L in enumerate(INDEL_LENGTHS):
        a = 31 + 67 * k
        cut = (a + L // 2) // 100 * 100
        cut += 100 if cut <= a else 0
        src = h0 if k % 2 == 0 else h0[:cut] + h1[cut:]
        s = list(src[a:a + L + 1])
        x = next(i for i in range(L // 4, len(s) - 1) if s[i] == s[i + 1])
        del s[x]
        y = next(i for i in range(L // 2, len(s) - 1) if s[i] == s[i + 1])
        s.insert(y, s[y])
        s[3 * L // 4] = "ACGT"[("ACGT".index(s[3 * L // 4]) + 2) % 4]
        reads.append("".join(s[:L]).encode())
    return A, b, reads, L0, cap, band, min_score


OWN = {"graph_indels": indel_input}
NAMES = TG.NAMES + ["graph_indels"]
SMALL = [n for n in NAMES if n != "tiers"]


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False, by_row=False):
    """test_align_graph.cpu() on an input of any of the files (this file's input goes into its table for the length of
    the call, as its own go into test_rows')."""
    with mock.patch.dict(TG.OWN, OWN):
        return TG.cpu(name, strands, by_row)


@functools.lru_cache(maxsize=None)
def graph(name):
    with mock.patch.dict(TG.OWN, OWN):
        return TG.graph(name)


@functools.lru_cache(maxsize=None)
def aligned(name, strands=False, by_row=False, pad=16, select=None):
    return GM.of_cpu(graph(name), cpu(name, strands, by_row), pad, 0, select)


@functools.lru_cache(maxsize=None)
def model(name, strands=False, by_row=False, pad=16, select=None, batch_kib=1 << 20):
    return JM.of_graph(graph(name), cpu(name, strands, by_row), aligned(name, strands, by_row, pad, select), batch_kib)


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_graph_cigar_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    for words in ("N <= L + edits", "path_batch_kib", "never\n * D"):
        assert words in header, words


def test_python_refuses_graph_cigar_without_graph():
    from founderblockgraphs_amd.api import Chains, PatternIndex
    with pytest.raises(ValueError):
        PatternIndex.chains(object.__new__(PatternIndex), graph_cigar=True)
    ch = Chains(np.zeros(1, dtype=np.uint64), None, None, None, 0, 0)
    assert ch.graph_cigar_off is None and ch.graph_cigar_ops is None and ch.graph_cigar_ms is None
    for f in (ch.graph_cigar, ch.graph_cigar_runs):
        with pytest.raises(ValueError):
            f(0)


@pytest.mark.parametrize("name", SMALL)
def test_model_agrees_with_the_brute_force_and_keeps_the_consequences(name):
    """Every input, plain and stranded, after plain and after by-row chains, at pads 16 and 0: of_graph asserts
    lev(P, T) == edits, N <= L + edits and the consequences for every aligned read; here also the two forms of the DP on the
    small ones, the enumeration of every optimal alignment where it is small enough, and no runs without an alignment."""
    g = graph(name)
    brutes = 0
    for strands in (False, True):
        for by_row in (False, True):
            c = cpu(name, strands, by_row)
            for pad in (16, 0):
                m = aligned(name, strands, by_row, pad)
                seen = []

                def check(R, P, T, edits, ops):
                    nonlocal brutes
                    if len(P) * len(T) <= CG.LITERAL_CELLS:
                        assert np.array_equal(np.array(CG.suffix_dp(P, T)), CG.suffix_dp_by_rows(P, T))
                    if (len(P) <= 8 and len(T) <= 12) or (edits <= 3 and len(P) <= 64):
                        assert ops == CG.brute_path(P, T, edits)[0], (name, R)
                        brutes += 1
                    seen.append(R)
                gc = JM.of_graph(g, c, m, check=check)
                assert len(seen) == m.stats["aligned"] == gc.stats["paths"]
                assert len(gc.off) == len(c.vreads) + 1 and gc.off[-1] == len(gc.ops) == gc.stats["ops"]
                for R in range(len(c.vreads)):
                    assert (m.edits[R] == NONE) == (gc.off[R] == gc.off[R + 1]), R
    assert brutes > 0 or name in ("m1",)


def test_indel_input_is_what_it_claims():
    """All nine reads are aligned with three edits, one D, one I and one X each, each has several optimal alignments, and
    the model's is the smallest of them; paths of one to four nodes, reads of one to five words, two with device history."""
    c, g, m, gc = cpu("graph_indels"), graph("graph_indels"), aligned("graph_indels"), model("graph_indels")
    assert [len(r) for r in c.reads] == list(INDEL_LENGTHS)
    assert m.edits.tolist() == [3] * 9 and m.stats["aligned"] == 9
    assert gc.strings[0] == "18=1D17=1I12=1X15="
    seen = collections.Counter()
    for R, P in enumerate(c.reads):
        count = {code: sum(n for k, n in gc.runs[R] if k == code) for code in CG.LETTER}
        assert (count[CG.D], count[CG.I], count[CG.X]) == (1, 1, 1), (R, gc.strings[R])
        want, ways = CG.brute_path(P, gc.texts[R], 3)
        assert 6 <= ways <= 12 and "".join(CG.LETTER[k] * n for k, n in gc.runs[R]) == want, (R, ways)
        seen.update(k for k, _ in gc.runs[R])
    assert set(seen) == {CG.I, CG.D, CG.EQ, CG.X}
    assert {int(x) for x in m.n_path} == {1, 2, 3, 4}
    assert sorted({(len(P) + 63) // 64 for P in c.reads}) == [1, 2, 3, 4, 5]
    assert gc.hist == [0] * 7 + [20560, 25600] and gc.stats["history_bytes"] == 46160 and gc.stats["batches"] == 1
    assert model("graph_indels", batch_kib=1).stats == dict(gc.stats, batches=2)
    # the existing inputs barely test the preferences: no I or D on the length reads
    lengths = model("graph_lengths")
    assert {k for r in lengths.runs for k, _ in r} == {CG.EQ, CG.X}


def test_gather_edges_occur_in_the_inputs():
    """What the gather kernel has to get right occurs: a path of one node and of many, a start at offset 0 and inside a
    label, an end offset equal to the label's length, labels shorter than 64 symbols and labels whose length is no multiple
    of 64.  (An empty T, start_offset == end_offset in one node, needs edits == L, which no read with a seed has: the seed
    alone matches.)"""
    one = many = first = inside = full = short = ragged = 0
    for name in SMALL:
        g = graph(name)
        for strands in (False, True):
            m, gc = aligned(name, strands), model(name, strands)
            for R, path in enumerate(m.paths):
                if m.edits[R] == NONE:
                    continue
                one += len(path) == 1
                many += len(path) >= 3
                first += m.start_offset[R] == 0
                inside += m.start_offset[R] > 0
                assert gc.texts[R]
                full += int(m.end_offset[R]) == len(g.labels[path[-1]])
                short += any(len(g.labels[v]) < 64 for v in path)
                ragged += any(len(g.labels[v]) > 64 and len(g.labels[v]) % 64 for v in path)
    assert min(one, many, first, inside, full, short, ragged) > 0, (one, many, first, inside, full, short, ragged)


def test_tool_graph_cigar_and_gaf_need_their_prerequisites(tmp_path):
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--graph-cigar" in p.stderr and b"--gaf=FILE" in p.stderr
    base = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2", "--rows"]
    gaf = str(tmp_path / "out.gaf")
    for extra, words in ((["--graph-cigar"], b"--graph-cigar needs --graph-align"),
                         (["--graph-cigar", "--align", "--cigar"], b"--graph-cigar needs --graph-align"),
                         (["--graph-align", "--gaf=" + gaf], b"--gaf needs --graph-cigar"),
                         (["--gaf=" + gaf], b"--gaf needs --graph-cigar")):
        p = subprocess.run([LOCATE] + base + extra, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and words in p.stderr and b"usage:" in p.stderr, extra
        assert not os.path.exists(gaf)
    # a file that cannot be written fails before the graph is read, let alone searched
    p = subprocess.run([LOCATE, "--graph=" + str(tmp_path / "no.xgfa"), "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2",
                        "--rows", "--graph-align", "--graph-cigar", "--gaf=" + str(tmp_path / "no" / "such" / "out.gaf")],
                       input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"cannot write" in p.stderr and b"no.xgfa" not in p.stderr


def test_gaf_fields_follow_from_the_model():
    """Every field of the record against the values it is defined by, on this file's input and on `chains`, whose reverse
    virtual reads are aligned too."""
    records = reverse = 0
    for name in ("graph_indels", "chains"):
        c, g, m, gc = cpu(name, True), graph(name), aligned(name, True), model(name, True)
        ids = [b"%d" % (v + 1) for v in range(len(g.labels))]
        n = len(c.reads)
        for v in range(2 * n):
            if m.edits[v] == NONE:
                continue
            k, L = v % n, len(c.vreads[v])
            f = JM.gaf_fields(g, m, gc, v, k, L, v >= n, ids)
            assert len(f) == 14 and f[0] == b"read%d" % k and f[1] == f[3] == b"%d" % L and f[2] == b"0"
            assert f[4] == (b"-" if v >= n else b"+")
            assert f[5].split(b">")[1:] == [ids[u] for u in m.paths[v]] and f[5].startswith(b">")
            spelled = b"".join(g.labels[u] for u in m.paths[v])
            assert int(f[6]) == len(spelled) and spelled[int(f[7]):int(f[8])] == gc.texts[v]
            ops = "".join(CG.LETTER[code] * length for code, length in gc.runs[v])
            assert int(f[9]) == ops.count("=") and int(f[10]) == len(ops) and f[11] == b"255"
            assert f[12] == b"NM:i:%d" % (len(ops) - ops.count("=")) == b"NM:i:%d" % m.edits[v]
            assert f[13] == b"cg:Z:" + gc.strings[v].encode()
            records += 1
            reverse += v >= n
    assert records >= 9 and reverse > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------

def c_gcigar(pix, n, want=(1, 1)):
    """fbg_pindex_chains_graph_cigar and _fetch through the C calls -> n_ops, total, off, ops, ms; nothing past the arrays."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    n_ops = np.full(n + 1, 7, dtype=np.uint32)
    total, ms = ctypes.c_uint64(99), ctypes.c_double(0)
    rc = L.fbg_pindex_chains_graph_cigar(pix._h, n_ops.ctypes.data_as(_lib.u32p) if want[0] else None,
                                         ctypes.byref(total) if want[1] else None, ctypes.byref(ms))
    assert rc == 0, rc
    assert n_ops[n] == 7
    off = np.full(n + 2, 7, dtype=np.uint64)
    assert L.fbg_pindex_chains_graph_cigar_fetch(pix._h, off.ctypes.data_as(_lib.u64p), None) == 0
    assert off[n + 1] == 7
    t = int(off[n])
    ops = np.full(t + 1, 7, dtype=np.uint32)
    off2 = np.zeros(n + 1, dtype=np.uint64)
    assert L.fbg_pindex_chains_graph_cigar_fetch(pix._h, off2.ctypes.data_as(_lib.u64p), ops.ctypes.data_as(_lib.u32p)) == 0
    assert ops[t] == 7 and np.array_equal(off2, off[:n + 1])
    if want[1]:
        assert total.value == t
    if want[0]:
        assert np.array_equal(n_ops[:n].astype(np.uint64), np.diff(off[:n + 1]))
    else:
        assert (n_ops == 7).all()
    return n_ops[:n], t, off[:n + 1], ops[:t], ms.value


def same(off, ops, gc, what):
    assert off.dtype == gc.off.dtype and ops.dtype == gc.ops.dtype, what
    assert np.array_equal(off, gc.off), (what, off.tolist(), gc.off.tolist())
    assert np.array_equal(ops, gc.ops), (what, [hex(x) for x in ops], [hex(x) for x in gc.ops])


def same_chains(ch, gc, what):
    same(ch.graph_cigar_off, ch.graph_cigar_ops, gc, what)
    for R in range(len(gc.runs)):
        assert ch.graph_cigar(R) == gc.strings[R], (what, R)
        runs = ch.graph_cigar_runs(R)
        assert runs.dtype == np.int64 and runs.shape == (len(gc.runs[R]), 2) and runs.tolist() == [list(r) for r in gc.runs[R]]


@pytest.mark.gpu
@pytest.mark.parametrize("by_row", [False, True])
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_input_through_both_interfaces(engine, name, strands, by_row):
    """Every input after plain and after by-row chains, at pads 16 and 0 (the long inputs at 16 only), through the C calls
    and through Python; a plain chains(graph=True) has no CIGAR fields."""
    c = cpu(name, strands, by_row)
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.graph_cigar_stats() == ZERO_STATS
        TG.seeded(pix, c, strands)
        TG.chained(pix, c, by_row)
        for pad in (16, 0) if name not in TG.LONG else (16,):
            m, gc = aligned(name, strands, by_row, pad), model(name, strands, by_row, pad)
            got, off, nodes, _ = TG.c_graph(pix, n, pad)
            TG.same(got, off, nodes, m, (name, pad, "graph"))
            n_ops, total, off, ops, ms = c_gcigar(pix, n)
            same(off, ops, gc, (name, pad, "C"))
            assert total == gc.stats["ops"] and pix.graph_cigar_stats() == gc.stats, (name, pad, pix.graph_cigar_stats(), gc.stats)
            assert ms > 0 or gc.stats["paths"] == 0
            ch = TG.chained(pix, c, by_row, graph=True, graph_pad=pad, graph_cigar=True)
            TG.same_python(ch, m, (name, pad, "python graph"))
            same_chains(ch, gc, (name, pad, "python"))
            assert pix.graph_cigar_stats() == gc.stats and ch.graph_cigar_ms >= 0
            plain = TG.chained(pix, c, by_row, graph=True, graph_pad=pad)
            assert plain.graph_cigar_off is None and plain.graph_cigar_ops is None and plain.graph_cigar_ms is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["graph_lengths", "graph_indels"])
def test_word_and_tier_boundaries(engine, name):
    """The reads of every word count together and then each alone, so that a launch sized by another read's N shows; 256
    symbols is the last read whose history stays in LDS, and the read of max_read + 1 symbols has no runs."""
    c, m, gc = cpu(name), aligned(name), model(name)
    with TR.build(engine, c.A, c.b) as pix:
        TG.seeded(pix, c, False)
        ch = TG.chained(pix, c, False, graph=True, graph_cigar=True)
        same_chains(ch, gc, name)
        assert pix.graph_cigar_stats() == gc.stats and gc.stats["history_bytes"] > 0
        if name == "graph_lengths":
            assert len(c.reads[-1]) == GM.MAX_READ + 1 and ch.graph_cigar(len(c.reads) - 1) == "" and m.edits[-2] != NONE
        for R, P in enumerate(c.reads):
            pix.seeds([P], min_length=c.L, max_per_seed=c.cap, msa=True)
            one = pix.chains(graph=True, graph_cigar=True)
            assert one.graph_cigar(0) == gc.strings[R] and one.graph_cigar_off.tolist() == [0, len(gc.runs[R])], len(P)
            st = pix.graph_cigar_stats()
            hist = CG.history_bytes(len(P), len(gc.texts[R])) if m.edits[R] != NONE else 0
            assert st["history_bytes"] == hist and (hist > 0) == (256 < len(P) <= GM.MAX_READ and m.edits[R] != NONE), len(P)
            assert st["batches"] == (1 if hist else 0) and st["paths"] == (0 if m.edits[R] == NONE else 1)
            assert st["columns"] == (len(gc.texts[R]) if m.edits[R] != NONE else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["graph_lengths", "graph_indels"])
def test_one_read_per_batch_gives_the_same_arrays(engine, name):
    from conftest import fbg_options
    c, gc, one = cpu(name), model(name), model(name, batch_kib=1)
    n = len(c.reads)
    long_reads = sum(1 for h in gc.hist if h)
    assert gc.stats["batches"] == 1 and one.stats == dict(gc.stats, batches=long_reads) and long_reads >= 2
    with TR.build(engine, c.A, c.b) as pix:
        TG.seeded(pix, c, False)
        TG.chained(pix, c, False)
        TG.c_graph(pix, n)
        same(*c_gcigar(pix, n)[2:4], gc, (name, "default"))
        assert pix.graph_cigar_stats() == gc.stats
        with fbg_options(engine, {"path_batch_kib": 1}):
            same(*c_gcigar(pix, n)[2:4], one, (name, "one KiB"))
            assert pix.graph_cigar_stats() == one.stats
        assert engine.get_option("path_batch_kib") == 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chains", "graph_indels"])
def test_unselected_reads_have_no_runs(engine, name):
    c = cpu(name)
    n = len(c.reads)
    with TR.build(engine, c.A, c.b) as pix:
        TG.seeded(pix, c, False)
        TG.chained(pix, c, False)
        for sel in (tuple(R % 2 for R in range(n)), tuple(1 - R % 2 for R in range(n)), (0,) * n):
            m, gc = aligned(name, select=sel), model(name, select=sel)
            TG.c_graph(pix, n, 16, 0, sel)
            n_ops, _, off, ops, _ = c_gcigar(pix, n)
            same(off, ops, gc, (name, sel))
            assert pix.graph_cigar_stats() == gc.stats
            assert all(n_ops[R] == 0 for R in range(n) if not sel[R]) and (any(n_ops) or not any(sel))
            same_chains(TG.chained(pix, c, False, graph=True, select=sel, graph_cigar=True), gc, (name, sel, "python"))


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    big32, big64 = np.zeros(1 << 16, dtype=np.uint32), np.zeros(4096, dtype=np.uint64)
    call = lambda h: L.fbg_pindex_chains_graph_cigar(h, u32(big32), None, None)      # noqa: E731
    fetch = lambda h: L.fbg_pindex_chains_graph_cigar_fetch(h, u64(big64), u32(big32))      # noqa: E731
    c, m, gc = cpu("chains"), aligned("chains"), model("chains")
    mb, gb = aligned("chains", False, True), model("chains", False, True)
    n = len(c.reads)
    # a NULL index
    assert call(None) == fetch(None) == L.fbg_pindex_graph_cigar_stats(None, *[None] * 5) == _lib.FBG_ERR_INVALID
    with TR.build(engine, c.A, c.b, rows=False) as plain, TR.build(engine, c.A, c.b) as pix:
        # no row table
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(plain._h) == fetch(plain._h) == _lib.FBG_ERR_INVALID
        with pytest.raises(FbgError) as ei:
            plain.graph_cigar_stats()
        assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
        # no seeds call yet; seeds without chains; chains without a graph call, even with a row alignment and its CIGAR
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        TG.seeded(pix, c, False)
        rows = TG.chained(pix, c, False, align=True, cigar=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        assert pix.graph_cigar_stats() == ZERO_STATS
        # a graph call, and a fetch before the call
        TG.c_graph(pix, n)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID
        assert call(pix._h) == 0 and fetch(pix._h) == 0
        # no reads
        pix.seeds([], msa=True, chain=True)
        assert call(pix._h) == _lib.FBG_ERR_INVALID
        e = pix.chains(graph=True, graph_cigar=True)
        assert e.graph_cigar_off.tolist() == [0] and len(e.graph_cigar_ops) == 0 and e.graph_cigar_ops.dtype == np.uint32
        assert call(pix._h) == 0 and fetch(pix._h) == 0 and pix.graph_cigar_stats() == ZERO_STATS
        # reads without seeds: every chain empty, nothing of the graph call on the device
        pix.seeds([b"NN", b""], msa=True, chain=True)
        TG.c_graph(pix, 2)
        n_ops, total, off, ops, _ = c_gcigar(pix, 2)
        assert n_ops.tolist() == [0, 0] and total == 0 and off.tolist() == [0, 0, 0] and pix.graph_cigar_stats() == ZERO_STATS
        # repeated calls, with and without the optional pointers; the graph alignment, the row alignment and the row CIGAR
        # as they were
        TG.seeded(pix, c, False)
        rows = TG.chained(pix, c, False, align=True, cigar=True)
        TG.same(*TG.c_graph(pix, n)[:3], m, "graph")

        def state():
            coff, cops = np.zeros(n + 1, dtype=np.uint64), np.zeros(len(rows.cigar_ops) + 1, dtype=np.uint32)
            assert L.fbg_pindex_chains_cigar_fetch(pix._h, u64(coff), u32(cops)) == 0
            poff, nodes = np.zeros(n + 1, dtype=np.uint64), np.zeros(len(m.path_nodes) + 1, dtype=np.uint32)
            assert L.fbg_pindex_chains_align_graph_fetch(pix._h, u64(poff), u32(nodes)) == 0
            return ([a.tolist() for a in (coff, cops, poff, nodes)], pix.align_stats(), pix.cigar_stats(), pix.graph_align_stats(),
                    pix.rows_stats(), pix.chain_stats())
        before = state()
        assert before[0][0] == rows.cigar_off.tolist() and before[0][2] == m.path_off.tolist() and before[0][3][:-1] == m.path_nodes.tolist()
        for want in ((1, 1), (0, 1), (0, 0), (1, 0), (1, 1)):
            _, _, off, ops, _ = c_gcigar(pix, n, want)
            same(off, ops, gc, want)
            assert pix.graph_cigar_stats() == gc.stats
        assert L.fbg_pindex_chains_graph_cigar(pix._h, None, None, None) == 0 and L.fbg_pindex_chains_graph_cigar_fetch(pix._h, None, None) == 0
        assert state() == before
        # and the reverse: a new row alignment and row CIGAR leave the graph CIGAR
        arr = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
        assert L.fbg_pindex_chains_align(pix._h, 16, 0, *[u32(a) for a in arr], None) == 0
        assert L.fbg_pindex_chains_cigar(pix._h, None, None, None) == 0
        off, ops = np.zeros(n + 1, dtype=np.uint64), np.zeros(len(gc.ops) + 1, dtype=np.uint32)
        assert L.fbg_pindex_chains_graph_cigar_fetch(pix._h, u64(off), u32(ops)) == 0
        same(off, ops[:-1], gc, "after the row calls")
        assert state() == before
        # a locate and an occurrences call overwrite the reads on the device
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        same(*c_gcigar(pix, n)[2:4], gc, "after locate")
        # a failed call leaves the stats
        assert call(None) == _lib.FBG_ERR_INVALID and pix.graph_cigar_stats() == gc.stats
        # a new graph call starts over: no CIGAR yet, then that call's
        m0, g0 = aligned("chains", False, False, 0), model("chains", False, False, 0)
        TG.same(*TG.c_graph(pix, n, 0)[:3], m0, "pad 0")
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID
        same(*c_gcigar(pix, n)[2:4], g0, "pad 0")
        assert pix.graph_cigar_stats() == g0.stats
        # a chaining call of either kind invalidates the graph alignment and its CIGAR; so does a seeds call
        stats = pix.graph_cigar_stats()
        TG.chained(pix, c, True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID and pix.graph_cigar_stats() == stats
        TG.same(*TG.c_graph(pix, n)[:3], mb, "by row")
        same(*c_gcigar(pix, n)[2:4], gb, "by row")
        TG.chained(pix, c, False)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        TG.c_graph(pix, n)
        assert call(pix._h) == 0 and fetch(pix._h) == 0
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID


# ---- the tool ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", ["chains", "graph_indels"])
def test_tool_prints_the_paths_and_writes_gaf(engine, name, strands, tmp_path):
    """fbg_locate --graph-align --graph-cigar: the --graph-align output (which test_align_graph compares with the model)
    with the runs, formatted here from the model on the tool's chains, as the eighth field of every H line that has
    numbers; --gaf=FILE leaves stdout alone and writes the model's records in the order of those lines."""
    from oracle import pyoracle as O
    c, g = cpu(name, strands), graph(name)
    off, _, place, seed = CM.chains(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, None, 0)
    c2 = SimpleNamespace(**dict(vars(c), chain_off=off, anchor_place=place, anchor_seed=seed))
    xgfa, fasta, gaf = str(tmp_path / "g.xgfa"), str(tmp_path / "g.fasta"), str(tmp_path / "g.gaf")
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
    k_of = (lambda i: i // 2) if strands else (lambda i: i)
    args = ["--graph=" + xgfa, "--msa=" + fasta, "--seeds=%d" % c.L, "--occurrences=%d" % c.cap, "--chain", "--rows"] + \
        (["--strands"] if strands else [])
    for flag, pad in (("--graph-align", 16), ("--graph-align=0", 0)):
        m = GM.of_cpu(g, c2, pad)
        gc = JM.of_graph(g, c2, m)
        base = TC.TL.run_locate(args + [flag], data)
        assert base.returncode == 0, base.stderr
        got = TC.TL.run_locate(args + [flag, "--graph-cigar"], data)
        assert got.returncode == 0, got.stderr
        want, records, i = [], [], 0
        for ln in base.stdout.splitlines(keepends=True):
            if ln.startswith(b"H\t"):
                v = v_of(i)
                if ln != b"H\t*\n":
                    assert m.edits[v] != NONE and gc.strings[v]
                    ln = ln[:-1] + b"\t" + gc.strings[v].encode() + b"\n"
                    assert len(ln.split(b"\t")) == 8
                    records.append(b"\t".join(JM.gaf_fields(g, m, gc, v, k_of(i), len(c.vreads[v]), v >= n, ids)) + b"\n")
                else:
                    assert m.edits[v] == NONE and gc.strings[v] == ""
                i += 1
            want.append(ln)
        assert i == len(keep) * (2 if strands else 1) and records
        assert got.stdout == b"".join(want)
        both = TC.TL.run_locate(args + [flag, "--graph-cigar", "--gaf=" + gaf], data)
        assert both.returncode == 0 and both.stdout == got.stdout, both.stderr
        assert open(gaf, "rb").read() == b"".join(records)
    if strands and name == "chains":
        assert any(r.split(b"\t")[4] == b"-" for r in records)
