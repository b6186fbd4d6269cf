"""The edit distance of each read to a row that carries its chain: fbg_pindex_chains_align, fbg_pindex_align_stats,
PatternIndex.chains(align=True) / .align_stats() and fbg_locate --align (include/fbg_hip.h, csrc/pindex_align.hip).

The checker is tests/align_model.py: the window from the row's text and the chain's diagonals, the two DPs of the
definition cell by cell, and a brute-force minimum over all substrings of the window.  The inputs are those of
tests/test_rows.py (with its CPU pipeline of seeds, chains and row sets) and three of this file's own: reads with a
substitution, an insertion and a deletion and a periodic row; reads at the word and tier boundaries of the kernel; the
example graph of the tool.  On the CPU the tests assert that the inputs hold what they are meant to hold; on the GPU
every array is compared exactly."""
import ctypes
import functools
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402

LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_chains_align", "fbg_pindex_align_stats")
NONE = AM.NONE
TABLE = TR.TABLE
HUGE = 1 << 40                    # a pad larger than any row
PADS = (16, 0, HUGE)
BOUNDARY_LENGTHS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, AM.MAX_READ, AM.MAX_READ + 1)


# ---- this file's inputs (cpu() below hands them to the pipeline of test_rows) ----------------------------------------

def edits_input():
    """Three rows, the third periodic in its middle and with a gap.  Reads: cut from a row; with one substitution, one
    inserted symbol, one deleted symbol (seeds on either side of the edit); cut from the periodic stretch, exact and with
    a period deleted; with a foreign symbol at the end and at the start (ties between ends, between starts); whole rows;
    four periods alone (many ends).  The periodic stretch lies inside one block, so no path of the graph skips a period."""
    rng = np.random.default_rng(1759)
    base = "".join(rng.choice(list("ACGT"), 96))
    r1 = list(base)
    for x in (13, 41, 77):
        r1[x] = "ACGT"[("ACGT".index(r1[x]) + 1) % 4]
    r2 = base[:30] + "AC" * 10 + "--" + base[52:]
    rows = [base, "".join(r1), r2]
    G = [r.replace("-", "").encode() for r in rows]
    sub = bytearray(G[0][10:60])
    sub[25] = ord("ACGT"[("ACGT".index(chr(sub[25])) + 2) % 4])
    reads = [G[0][8:50],                                   # 0: exact
             bytes(sub),                                   # 1: substitution
             G[0][20:45] + b"T" + G[0][45:75],             # 2: insertion into the read
             G[0][5:30] + G[0][31:70],                     # 3: deletion from the read
             G[2][22:58],                                  # 4: the periodic stretch, exact
             G[2][18:38] + G[2][40:64],                    # 5: a period deleted
             G[1][40:70] + b"N",                           # 6: several ends
             b"N" + G[1][40:70],                           # 7: several starts
             G[2][60:] + b"NN"] + G + [b"ACACACAC"]        # 8: runs past the row's end; 9 .. 11: whole rows; 12: periods
    return TR.msa_of(rows), [15, 29, 51, 63, 79, 95], reads, 6, 8, None, 0


def boundary_row():
    rng = np.random.default_rng(40)
    return "".join(rng.choice(list("ACGT"), AM.MAX_READ + 64)).encode()


def other(c):
    return b"ACGT"["ACGT".index(chr(c)) ^ 1]


def boundary_input():
    """One row of max_read + 64 symbols in blocks of 100 columns, and per length of BOUNDARY_LENGTHS one read cut from it
    with two substitutions planted where there is room (the 129 read at position 63, the 257 read at position 64).  The
    reads of max_read and max_read + 1 symbols are suffixes of the row: their best end is the window's last symbol."""
    g = boundary_row()
    reads = []
    for k, L in enumerate(BOUNDARY_LENGTHS):
        a = len(g) - L if L >= AM.MAX_READ else 7 + 11 * k
        P = bytearray(g[a:a + L])
        at = {129: (63, 100), 257: (64, 200)}.get(L, (L // 3, (2 * L) // 3) if L >= 60 else ())
        for x in at:
            P[x] = other(P[x])
        reads.append(bytes(P))
    return TR.msa_of([g]), list(range(99, len(g), 100)) + [len(g) - 1], reads, 1, 4, None, 0


TOOL_DATA = b"AGCGACTAGATAC AGCAGTT CGACTAX T XX GACTAGTTTCA AGXTTAC AGCGTCTCGTTAC\n"


def tool_input():
    """The example graph of xGFAspec.md as a segmentation of golden/msa.fasta, with the reads of test_rows' tool test."""
    from fasta_util import read_fasta
    A, _ = read_fasta(TC.GOLDEN[0])
    return A, [1, 5, 8, 14], TOOL_DATA.split(), 3, 4, 2, 0


OWN = {"align_edits": edits_input, "align_boundary": boundary_input, "align_tool": tool_input}
NAMES = list(TR.INPUTS) + ["align_edits", "align_boundary"]


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False):
    """test_rows.cpu() on an input of either file.  test_rows looks an input up by name in its own table, so this file's
    inputs are in that table for the length of the call and no longer; the results are kept here and in its caches."""
    with mock.patch.dict(TR.INPUTS, OWN):
        return TR.cpu(name, strands)
SMALL = [n for n in NAMES if n not in ("tiers", "align_boundary")]      # every window small enough for the literal DP


@functools.lru_cache(maxsize=None)
def model(name, strands=False, pad=16, max_window=0):
    return AM.of_cpu(cpu(name, strands), pad, max_window)


def stats_of(m, c):
    return dict(m.stats, table_bytes=4 * len(c.b) * c.rm.m)


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_align_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    assert "#define FBG_ALIGN_NONE 0xffffffffu" in header and _lib.ALIGN_NONE == NONE


def test_end_and_start_rules_against_brute_force():
    """Random reads and texts over two and four symbols, half of them reads cut from the text with up to three edits."""
    rng = np.random.default_rng(300)
    ties = 0
    for it in range(300):
        al = b"AC" if it % 3 else b"ACGT"
        W = bytes(rng.choice(list(al), int(rng.integers(1, 12))))
        L = int(rng.integers(1, 9))
        if it % 2 and len(W) >= L:
            s = int(rng.integers(0, len(W) - L + 1))
            P = bytearray(W[s:s + L])
            for _ in range(int(rng.integers(0, 4))):
                k, op = int(rng.integers(0, len(P))), int(rng.integers(0, 3))
                if op == 0:
                    P[k] = int(rng.choice(list(al)))
                elif op == 1 and len(P) > 1:
                    del P[k]
                else:
                    P.insert(k, int(rng.choice(list(al))))
            P = bytes(P)
        else:
            P = bytes(rng.choice(list(al), L))
        got = AM.align(P, W)
        assert got == AM.brute(P, W), (P, W)
        assert AM.last_row(P, W, lambda j: 0) == AM.last_row_by_rows(P, W, lambda j: 0)
        assert AM.last_row(P, W, lambda j: j) == AM.last_row_by_rows(P, W, lambda j: j)
        ties += AM.last_row(P, W, lambda j: 0).count(got[0]) > 1
    assert ties > 50


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_brute_force_and_the_bound(name):
    """Every input, plain and on both strands, at every pad: the two passes against the minimum over all substrings
    (windows of up to 48 symbols; the row-at-a-time DP on every window), and edits <= L - max k."""
    for strands in (False, True):
        c = cpu(name, strands)
        for pad in PADS:
            seen = []

            def check(P, W, res):
                if len(W) <= 48:
                    assert res == AM.brute(P, W), (name, P, W)
                for first in (lambda j: 0, lambda j: j):
                    assert AM.last_row(P, W, first) == AM.last_row_by_rows(P, W, first)
                seen.append(1)
            m = AM.of_cpu(c, pad, check=check)
            assert len(seen) == m.stats["aligned"]
            bound(c, m)


def bound(c, m):
    for R in range(len(c.vreads)):
        ks = c.length[c.anchor_seed[int(c.chain_off[R]):int(c.chain_off[R + 1])]]
        if m.edits[R] != NONE:
            assert int(m.edits[R]) <= len(c.vreads[R]) - int(ks.max()), R
            assert m.row[R] != NONE and m.t_start[R] <= m.t_end[R]
        else:
            assert m.t_start[R] == NONE and m.t_end[R] == NONE


def test_long_inputs_keep_the_bound():
    for name in ("tiers", "align_boundary"):
        bound(cpu(name), model(name))


def ends_and_starts(c, m, R):
    """How many ends attain edits, and how many starts for the chosen end."""
    w0, w1 = m.windows[R]
    P, W = c.vreads[R], c.rm.G[int(m.row[R])][w0:w1]
    e = int(m.t_end[R]) - w0
    return (AM.last_row(P, W, lambda j: 0).count(int(m.edits[R])),
            AM.last_row(P[::-1], W[:e][::-1], lambda j: j).count(int(m.edits[R])))


def test_edits_input_is_what_it_claims():
    c, m = cpu("align_edits"), model("align_edits")
    G = c.rm.G
    assert (m.row[:4] == 0).all() and m.edits[:4].tolist() == [0, 1, 1, 1]
    assert (m.t_start[0], m.t_end[0]) == (8, 50) and (m.t_start[1], m.t_end[1]) == (10, 60)
    assert (m.t_start[2], m.t_end[2]) == (20, 75) and (m.t_start[3], m.t_end[3]) == (5, 70)
    for R in (1, 2, 3):                                                   # the edit lies between two anchors
        assert c.chain_off[R + 1] - c.chain_off[R] >= 2
    assert m.row[4] == 2 and m.edits[4] == 0 and m.row[5] == 2 and (m.edits[5], m.t_start[5], m.t_end[5]) == (2, 18, 64)
    # ties: the periods alone, the foreign symbol at either end
    e12, s12 = ends_and_starts(c, m, 12)
    e6, s6 = ends_and_starts(c, m, 6)
    e7, s7 = ends_and_starts(c, m, 7)
    assert e12 >= 4 and e6 >= 2 and s7 >= 2, (e12, s12, e6, s6, e7, s7)
    assert m.row[12] == 2 and (m.edits[12], m.t_start[12], m.t_end[12]) == (0, 30, 38)      # the first of the periodic ends
    assert (m.edits[6], m.t_start[6], m.t_end[6]) == (1, 40, 70)          # the smallest end: the symbol is inserted
    assert (m.edits[7], m.t_start[7], m.t_end[7]) == (1, 40, 70)          # the largest start
    # the window runs into both ends of the row: whole rows, and the read past the row's end
    for R in (9, 10, 11):
        r = int(m.row[R])
        assert m.edits[R] == 0 and m.windows[R] == (0, len(G[r])) and (m.t_start[R], m.t_end[R]) == (0, len(G[r]))
    assert m.edits[8] == 2 and m.t_end[8] == len(G[int(m.row[8])]) == m.windows[8][1]
    z, h = model("align_edits", pad=0), model("align_edits", pad=HUGE)
    assert np.array_equal(z.edits[:4], m.edits[:4]) and z.stats["cells"] < m.stats["cells"] < h.stats["cells"]
    assert all(h.windows[R] == (0, len(G[int(h.row[R])])) for R in range(len(c.reads)) if h.windows[R])
    assert z.windows[1] == (10, 60) and z.windows[0] == (8, 50)
    # clamped at one end only
    assert any(w and w[0] == 0 and w[1] < len(G[int(m.row[R])]) for R, w in enumerate(m.windows))
    assert any(w and w[0] > 0 and w[1] == len(G[int(m.row[R])]) for R, w in enumerate(m.windows))
    # a window that max_window skips keeps its row
    w = model("align_edits", max_window=70)
    skipped = [R for R in range(len(c.reads)) if w.windows[R] and w.windows[R][1] - w.windows[R][0] > 70]
    assert skipped and w.stats["too_wide"] == len(skipped) and 0 < w.stats["aligned"] == m.stats["aligned"] - len(skipped)
    for R in skipped:
        assert w.row[R] == m.row[R] != NONE and w.edits[R] == w.t_start[R] == w.t_end[R] == NONE
    assert c.rm.m <= 16


def test_inputs_of_test_rows_hold_what_the_align_tests_need():
    # a recombinant chain: not empty, and no row
    c, m = cpu("recombinant"), model("recombinant")
    n = len(c.reads)
    for R in (n - 2, n - 1):
        assert c.chain_off[R + 1] > c.chain_off[R] and m.row[R] == m.edits[R] == m.t_start[R] == m.t_end[R] == NONE
    assert m.stats["unsupported"] == 2 and (m.edits[:n - 2] == 0).all()
    # a window across cells of the row without a node
    c, m = cpu("gaps"), model("gaps")
    across = 0
    for R, w in enumerate(m.windows):
        if w and m.edits[R] != NONE:
            r = int(m.row[R])
            across += any(c.rm.node_of[r][j] is None and w[0] < c.rm.p[r][j] < w[1] for j in range(len(c.b)))
    assert across > 0
    # a window across the one-column blocks
    c, m = cpu("bounds"), model("bounds")
    assert any(w and m.edits[R] == 0 and sum(w[0] <= c.rm.p[int(m.row[R])][j] < w[1] for j in range(1, 13)) == 12
               for R, w in enumerate(m.windows))
    # a chain emptied by min_score; a read with edits across two rows' pieces; a reverse virtual read
    c, m = cpu("chains"), model("chains")
    lens = np.diff(c.chain_off.astype(np.int64))
    assert ((lens == 0) & (c.score > 0) & (m.row == NONE)).any()
    assert ((m.edits != NONE) & (m.edits > 0)).any()
    s, ms = cpu("chains", True), model("chains", True)
    n = len(c.reads)
    assert ms.edits[2 * n - 1] == 0 and ms.edits[n - 1] == NONE          # the read given as its reverse complement
    assert np.array_equal(ms.edits[:n], m.edits)
    strand = np.array([STM.pick(int(s.score[R]), int(s.score[n + R]), lens2(s)[R] > 0, lens2(s)[n + R] > 0)[0] for R in range(n)])
    be = AM.best_edits(ms.edits, strand)
    assert strand[n - 1] == 1 and be[n - 1] == 0 and (strand == 0xff).any() and (be[strand == 0xff] == NONE).all()
    # a chosen row of 64 or more
    m = model("m129")
    assert ((m.row != NONE) & (m.row >= 64)).any() and ((m.row != NONE) & (m.row < 64)).any()
    # the boundary reads
    c, m = cpu("align_boundary"), model("align_boundary")
    g = c.rm.G[0]
    assert [len(r) for r in c.reads] == list(BOUNDARY_LENGTHS) and len(g) == AM.MAX_READ + 64
    assert m.stats["too_long"] == 1 and m.row[-1] == 0 and m.edits[-1] == NONE
    assert m.edits[:-1].tolist() == [0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]
    assert m.t_end[-2] == len(g) == m.windows[-2][1] and m.t_start[-2] == 64
    assert c.reads[5][63] != g[7 + 55 + 63] and c.reads[9][64] != g[7 + 99 + 64]


def lens2(s):
    return np.diff(s.chain_off.astype(np.int64))


def test_tool_align_needs_its_prerequisites():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--align" in p.stderr
    base = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0]]
    for extra in (["--chain=2", "--align"], ["--rows", "--align=4"], ["--align"]):
        p = subprocess.run([LOCATE] + base + extra, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--align needs --chain and --rows" in p.stderr and b"usage:" in p.stderr
    p = subprocess.run([LOCATE] + base + ["--chain", "--rows", "--align=x"], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--align takes a pad" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

FIELDS = ("row", "edits", "t_start", "t_end")


def c_align(pix, n, pad=16, max_window=0, want=(1, 1, 1, 1)):
    from founderblockgraphs_amd import _lib
    arr = [np.full(n + 1, 7, dtype=np.uint32) for _ in range(4)]
    ms = ctypes.c_double(0)
    rc = _lib.lib().fbg_pindex_chains_align(pix._h, pad, max_window, *[a.ctypes.data_as(_lib.u32p) if w else None for a, w in zip(arr, want)],
                                            ctypes.byref(ms))
    assert rc == 0, rc
    assert all(a[n] == 7 for a in arr)                 # nothing past the n entries
    return [a[:n] for a in arr], ms.value


def same(got, m, what):
    for f, g in zip(FIELDS, got):
        want = getattr(m, f)
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), (what, f, g.tolist(), want.tolist())


def seeded(pix, c, strands, **kw):
    sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band, min_score=c.min_score,
                   strands=strands, rows=True, **kw)
    return sd


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_input_through_both_interfaces(engine, name, strands):
    """Every input at pads 16, 0, 2^40 and 2^64 - 1 and with a window limit of 30; the `tiers` input, whose reads of
    about a thousand symbols make the model slow, at pads 16 and 2^64 - 1 only and without the window limit."""
    c = cpu(name, strands)
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.align_stats()["table_bytes"] == 0 and pix.align_stats()["max_read"] == AM.MAX_READ
        sd = seeded(pix, c, strands)
        TR.same_as_cpu(sd, c, name)
        assert sd.chains.edits is None and sd.chains.align_row is None and sd.chains.best_edits is None
        for pad in PADS if name != "tiers" else PADS[:1]:
            m = model(name, strands, pad)
            got, ms = c_align(pix, n, pad)
            same(got, m, (name, pad, "C"))
            assert pix.align_stats() == stats_of(m, c), (name, pad)
            assert ms > 0 or m.stats["aligned"] + m.stats["unsupported"] == 0
            ch = pix.chains(band=c.band, min_score=c.min_score, align=True, pad=pad)
            same((ch.align_row, ch.edits, ch.t_start, ch.t_end), m, (name, pad, "python"))
            if strands:
                assert np.array_equal(ch.best_edits, AM.best_edits(m.edits, ch.strand)) and ch.best_edits.dtype == np.uint32
            else:
                assert ch.best_edits is None
        # pads beyond the clamp, and a window limit
        got, _ = c_align(pix, n, 0xffffffffffffffff)
        same(got, model(name, strands, HUGE), (name, "2^64 - 1"))
        if name != "tiers":
            m = model(name, strands, 16, 30)
            got, _ = c_align(pix, n, 16, 30)
            same(got, m, (name, "max_window"))
            assert pix.align_stats() == stats_of(m, c)


@pytest.mark.gpu
def test_word_and_tier_boundaries(engine):
    """Reads of 1 .. max_read + 1 symbols against one row: every register tier, the LDS tier, the skip."""
    c, m = cpu("align_boundary"), model("align_boundary")
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.align_stats()["max_read"] == AM.MAX_READ == BOUNDARY_LENGTHS[-2]
        seeded(pix, c, False)
        ch = pix.chains(align=True)
        same((ch.align_row, ch.edits, ch.t_start, ch.t_end), m, "boundary")
        st = pix.align_stats()
        assert (st["aligned"], st["too_long"], st["too_wide"], st["unsupported"]) == (len(c.reads) - 1, 1, 0, 0)
        assert ch.edits[-1] == NONE and ch.align_row[-1] == 0 and ch.t_end[-2] == AM.MAX_READ + 64
        # each length alone: a call whose only read is of that tier
        for R, P in enumerate(c.reads):
            pix.seeds([P], min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
            one = pix.chains(align=True)
            assert [int(getattr(one, f)[0]) for f in ("align_row", "edits", "t_start", "t_end")] == \
                   [int(getattr(m, f)[R]) for f in FIELDS], len(P)


@pytest.mark.gpu
def test_a_wave_per_chain_agrees_with_sixteen_lanes(engine):
    from conftest import fbg_options
    c, m = cpu("align_edits"), model("align_edits")
    with fbg_options(engine, {"rows_wave": 1}), TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        same(c_align(pix, len(c.reads))[0], m, "rows_wave")


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    dummy = [np.zeros(4096, dtype=np.uint32) for _ in range(4)]
    call = lambda h: L.fbg_pindex_chains_align(h, 16, 0, *[u32(a) for a in dummy], None)      # noqa: E731
    c, m = cpu("chains"), model("chains")
    n = len(c.reads)
    # a NULL index
    assert call(None) == _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_align_stats(None, *[None] * 7) == _lib.FBG_ERR_INVALID
    with TR.build(engine, c.A, c.b, rows=False) as plain, TR.build(engine, c.A, c.b) as pix:
        # no row table
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(plain._h) == _lib.FBG_ERR_INVALID
        for f in (lambda: plain.chains(align=True), plain.align_stats):
            with pytest.raises(FbgError) as ei:
                f()
            assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
        # no seeds call yet; seeds without chains
        assert call(pix._h) == _lib.FBG_ERR_INVALID
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True)
        assert call(pix._h) == _lib.FBG_ERR_INVALID
        assert pix.align_stats()["aligned"] == 0
        # no reads
        pix.seeds([], msa=True, chain=True)
        assert call(pix._h) == 0
        e = pix.chains(align=True)
        assert len(e.edits) == 0 and e.edits.dtype == np.uint32
        # reads without seeds: every chain empty
        pix.seeds([b"NN", b""], msa=True, chain=True)
        got, _ = c_align(pix, 2)
        assert all(g.tolist() == [NONE, NONE] for g in got)
        assert pix.align_stats() == dict(aligned=0, unsupported=0, too_long=0, too_wide=0, cells=0, max_read=AM.MAX_READ, table_bytes=0)
        # repeated calls, with and without the optional arrays; every other state as it was
        sd = seeded(pix, c, False)
        ch = sd.chains
        k = len(sd.q_start)

        def state():
            nr, fr = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            bits = np.zeros(n * pix.rows_stats()["words_per_set"], dtype=np.uint64)
            assert L.fbg_pindex_chains_rows(pix._h, u32(nr), u32(fr), bits.ctypes.data_as(_lib.u64p), None) == 0
            pl, se = np.zeros(len(ch.anchor_place) + 1, dtype=np.uint32), np.zeros(len(ch.anchor_place) + 1, dtype=np.uint32)
            assert L.fbg_pindex_chains_fetch(pix._h, u32(pl), u32(se), None) == 0
            return (TC.seeds_state(pix, k), [a.tolist() for a in (nr, fr, bits, pl, se)], pix.stats(), pix.chain_stats(), pix.rows_stats())
        before = state()
        assert before[1][0] == c.chain_n_rows.tolist() and before[1][3][:-1] == c.anchor_place.tolist()
        for want in ((1, 1, 1, 1), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 1, 1)):
            got, _ = c_align(pix, n, want=want)
            for f, g, w in zip(FIELDS, got, want):
                assert np.array_equal(g, getattr(m, f)) if w else (g == 7).all(), (f, want)
            assert pix.align_stats() == stats_of(m, c)
        assert state() == before
        # a locate and an occurrences call overwrite the reads on the device
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        mid = state()                                      # the two searches moved fbg_pindex_stats, and nothing else
        assert mid[:2] == before[:2] and mid[3:] == before[3:]
        same(c_align(pix, n)[0], m, "after locate")
        assert state() == mid
        # a failed call leaves the stats
        assert L.fbg_pindex_chains_align(None, 16, 0, None, None, None, None, None) == _lib.FBG_ERR_INVALID
        assert pix.align_stats() == stats_of(m, c)
        # a new seeds call invalidates the chains, and with them the alignment
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap)
        assert call(pix._h) == _lib.FBG_ERR_INVALID


def tool_lines(plain, m, n, strands):
    """The output with --rows and without --align, and after the A lines of the i-th chain the G line of its read."""
    out, i, wait = [], 0, None
    lines = plain.splitlines(keepends=True)
    for at, ln in enumerate(lines):
        out.append(ln)
        if ln.startswith(b"C\t"):
            v = (i // 2 + (i % 2) * n) if strands else i
            i += 1
            wait = [int(ln.split(b"\t")[2]), v]
        if wait is not None:
            if wait[0] == 0:
                v = wait[1]
                out.append(b"G\t*\n" if m.edits[v] == NONE else b"G\t%d\t%d\t%d\t%d\n" % (m.row[v], m.edits[v], m.t_start[v], m.t_end[v]))
                wait = None
            else:
                wait[0] -= 1
    assert wait is None
    return b"".join(out), i


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
def test_tool_prints_the_alignments(engine, strands):
    """fbg_locate --align adds one G line per chain, formatted here from the model; every other byte of the output is
    what it is without --align (which test_rows and test_chains compare with the engine line by line)."""
    c = cpu("align_tool", strands)
    args = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2", "--rows"] + (["--strands"] if strands else [])
    plain = TC.TL.run_locate(args, TOOL_DATA)
    assert plain.returncode == 0 and b"\nG\t" not in plain.stdout, plain.stderr
    for flag, pad in (("--align", 16), ("--align=0", 0), ("--align=3", 3)):
        m = model("align_tool", strands, pad)
        got = TC.TL.run_locate(args + [flag], TOOL_DATA)
        assert got.returncode == 0, got.stderr
        want, chains = tool_lines(plain.stdout, m, len(c.reads), strands)
        assert chains == len(c.vreads)
        assert got.stdout == want
        assert b"".join(ln for ln in got.stdout.splitlines(keepends=True) if not ln.startswith(b"G\t")) == plain.stdout
    assert (m.edits == NONE).any() and (m.edits != NONE).any()
    with TR.build(engine, c.A, c.b) as pix:                     # the engine agrees with the pipeline the model ran on
        TR.same_as_cpu(seeded(pix, c, strands), c, "tool")
