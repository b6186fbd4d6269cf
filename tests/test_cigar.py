"""The alignment path (CIGAR) of each aligned read: fbg_pindex_chains_cigar, _cigar_fetch, fbg_pindex_cigar_stats,
PatternIndex.chains(align=True, cigar=True) / .cigar_stats() and fbg_locate --cigar (include/fbg_hip.h, csrc/pindex_align.hip).

The checker is tests/cigar_model.py: the suffix DP of the definition as a full matrix, the walk, and an enumeration of
every optimal alignment.  The inputs are those of tests/test_align.py (and through it of tests/test_rows.py), with the
alignments of tests/align_model.py, and one of this file's own: substitutions directly beside an insertion and beside a
deletion.  On the CPU the tests assert that the inputs hold what they are meant to hold; on the GPU every array is
compared exactly."""
import collections
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
import cigar_model as GM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_align as TA  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402

LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_chains_cigar", "fbg_pindex_chains_cigar_fetch", "fbg_pindex_cigar_stats")
NONE = AM.NONE
PADS = TA.PADS
ZERO_STATS = dict(paths=0, ops=0, columns=0, history_bytes=0, batches=0)


# ---- this file's input ------------------------------------------------------------------------------------------------

def adjacent_input():
    """Two rows of 96 symbols without gaps, the second with three symbols changed outside the reads.  Reads cut from the first row: a
    substitution directly before an inserted symbol; a substitution directly before a deleted symbol; two substitutions,
    an insertion and a deletion with equal stretches between them (2 * edits + 1 runs); the reverse complement of the
    second read, whose reverse virtual read is that read again."""
    rng = np.random.default_rng(2207)
    base = "".join(rng.choice(list("ACGT"), 96))
    r1 = list(base)
    for x in (1, 84, 92):
        r1[x] = "ACGT"[("ACGT".index(r1[x]) + 1) % 4]
    rows = [base, "".join(r1)]
    g = base.encode()
    sub = lambda x: bytes([next(ch for ch in b"ACGT" if ch not in g[x - 1:x + 2])])      # noqa: E731
    reads = [g[10:35] + sub(35) + b"N" + g[36:70],
             g[5:30] + sub(30) + g[32:66],
             g[8:20] + sub(20) + g[21:33] + b"N" + g[33:45] + g[46:60] + sub(60) + g[61:80]]
    reads.append(STM.revcomp(reads[1], TR.TABLE))
    return TR.msa_of(rows), [15, 29, 51, 63, 79, 95], reads, 6, 8, None, 0


OWN = {"cigar_adjacent": adjacent_input}
NAMES = TA.NAMES + ["cigar_adjacent"]


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False):
    """test_align.cpu() on an input of any of the three files (this file's input goes into test_rows' table for the
    length of the call, as test_align's do)."""
    if name in OWN:
        with mock.patch.dict(TR.INPUTS, OWN):
            return TR.cpu(name, strands)
    return TA.cpu(name, strands)


@functools.lru_cache(maxsize=None)
def aligned(name, strands=False, pad=16, max_window=0):
    return AM.of_cpu(cpu(name, strands), pad, max_window) if name in OWN else TA.model(name, strands, pad, max_window)


@functools.lru_cache(maxsize=None)
def model(name, strands=False, pad=16, max_window=0):
    return GM.of_align(cpu(name, strands), aligned(name, strands, pad, max_window))


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_cigar_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    for name, code in (("I", GM.I), ("D", GM.D), ("EQ", GM.EQ), ("X", GM.X)):
        assert f"#define FBG_CIGAR_{name} {code}u" in header
    assert _lib.CIGAR_OPS == GM.LETTER
    assert "path_batch_kib" in header


def test_python_refuses_cigar_without_align():
    from founderblockgraphs_amd.api import PatternIndex
    with pytest.raises(ValueError):
        PatternIndex.chains(object.__new__(PatternIndex), cigar=True)


def random_case(rng, it):
    """A read of up to 8 symbols and a text of up to 12 over two or four symbols; every second read is cut from the text
    and edited, every fourth with a symbol deleted between matches (random reads alone never show a D)."""
    al = b"AC" if it % 3 == 0 else b"ACGT"
    W = bytes(rng.choice(list(al), int(rng.integers(1, 13))).tolist())
    L = int(rng.integers(1, 9))
    if it % 2 and len(W) >= L:
        s = int(rng.integers(0, len(W) - L + 1))
        P = bytearray(W[s:s + L])
        if it % 4 == 3 and len(W) - s >= 7:
            P = bytearray(W[s:s + 3] + W[s + 4:s + 8])
        for _ in range(int(rng.integers(0, 4 if it % 4 == 1 else 2))):
            k, op = int(rng.integers(0, len(P))), int(rng.integers(0, 3))
            if op == 0:
                P[k] = int(rng.choice(list(al)))
            elif op == 1 and len(P) > 1:
                del P[k]
            elif len(P) < 8:
                P.insert(k, int(rng.choice(list(al))))
        return bytes(P), W
    return bytes(rng.choice(list(al), L).tolist()), W


def test_walk_against_every_optimal_alignment():
    """Random reads and texts over two and four symbols, half of them reads cut from the text with up to three planted
    edits; T is the stretch that align_model.align picks, as in the product.  The model's walk is the smallest optimal
    alignment, the two forms of the DP agree, and the consequences of the definition hold; all four ops occur, and so do
    inputs with several optimal alignments."""
    rng = np.random.default_rng(411)
    seen, several = collections.Counter(), 0
    for it in range(400):
        P, W = random_case(rng, it)
        edits, s, e = AM.align(P, W)
        T = W[s:e]
        E = GM.suffix_dp(P, T)
        assert np.array_equal(np.array(E), GM.suffix_dp_by_rows(P, T)), (P, T)
        ops = GM.walk(P, T, E)
        assert E[0][0] == edits
        want, count = GM.brute_path(P, T, edits)
        assert ops == want, (P, T, ops, want)
        GM.consequences(GM.runs_of(ops), len(P), len(T), edits)
        seen.update(set(ops))
        several += count > 1
    assert all(seen[ch] >= 10 for ch in "=XID") and several > 50, (seen, several)


@pytest.mark.parametrize("name", NAMES)
def test_consequences_on_every_input(name):
    """Every input, plain and on both strands, at every pad: of_align asserts the consequences of the definition for every
    aligned read; here also the two forms of the DP on the small ones, the brute force where it is small enough, and that
    reads without an alignment have no runs."""
    for strands in (False, True):
        c = cpu(name, strands)
        for pad in PADS:
            m = aligned(name, strands, pad)
            seen = []

            def check(P, T, edits, ops):
                if len(P) * len(T) <= GM.LITERAL_CELLS:
                    assert np.array_equal(np.array(GM.suffix_dp(P, T)), GM.suffix_dp_by_rows(P, T))
                if len(P) <= 8 and len(T) <= 12:
                    assert ops == GM.brute_path(P, T, edits)[0]
                seen.append(1)
            g = GM.of_align(c, m, check)
            assert len(seen) == m.stats["aligned"] == g.stats["paths"]
            assert len(g.off) == len(c.vreads) + 1 and g.off[-1] == len(g.ops) == g.stats["ops"]
            for R in range(len(c.vreads)):
                assert (m.edits[R] == NONE) == (g.off[R] == g.off[R + 1]), R


def test_inputs_hold_what_they_claim():
    c, m, g = cpu("align_edits"), aligned("align_edits"), model("align_edits")
    assert g.strings[:4] == ["42=", "25=1X24=", "25=1I30=", "26=1D38="]
    # a period deleted: the D run may stand at several places of the periodic stretch, and the rule picks the first at
    # which the diagonal no longer keeps the distance
    assert g.strings[5] == "30=2D14=" and m.edits[5] == 2
    P, T = bytes(c.vreads[5]), c.rm.G[2][18:64]
    every = GM.brute_paths(P, T, 2)
    assert len(every) > 1 and min(every, key=lambda s: [GM.RANK[ch] for ch in s]) == "=" * 30 + "DD" + "=" * 14
    assert len({s.index("D") for s in every if "DD" in s}) > 1
    assert g.strings[6] == "30=1I" and g.strings[7] == "1I30=" and g.strings[8] == "34=2I" and g.strings[12] == "8="
    assert g.stats == dict(paths=13, ops=sum(len(r) for r in g.runs), columns=int((m.t_end - m.t_start).sum()), history_bytes=0, batches=0)
    # this file's input: X beside I, X beside D, and as many runs as a path can have
    c, m, g = cpu("cigar_adjacent"), aligned("cigar_adjacent"), model("cigar_adjacent")
    assert g.strings[:3] == ["25=1X1I34=", "25=1X1D34=", "12=1X12=1I12=1D14=1X19="], g.strings
    assert m.edits[:3].tolist() == [2, 2, 4] and len(g.runs[2]) == 2 * 4 + 1
    assert m.edits[3] > 10 and len(g.runs[3]) > 10          # the other strand's text on a chance seed: a path of many runs
    # a reverse virtual read with a path that is not one run
    s, ms, gs = cpu("cigar_adjacent", True), aligned("cigar_adjacent", True), model("cigar_adjacent", True)
    n = len(c.reads)
    assert s.vreads[n + 3] == c.reads[1] and gs.strings[n + 3] == g.strings[1] and gs.strings[:n] == g.strings
    assert ms.edits[n + 3] == 2
    # the boundary reads: the history of the reads of more than 4 words alone goes to device memory
    c, m, g = cpu("align_boundary"), aligned("align_boundary"), model("align_boundary")
    N = (m.t_end - m.t_start).tolist()
    assert g.stats["history_bytes"] == 5 * N[9] * 16 + 16 * N[10] * 16 and g.stats["batches"] == 1
    assert g.strings[0] == "1=" and g.strings[3] == "21=1X21=1X21=" and g.strings[-1] == ""
    assert all(len(r) == 5 for r in g.runs[1:-1])
    gs = model("align_boundary", True)
    assert {k for r in gs.runs for k, _ in r} == {GM.I, GM.D, GM.EQ, GM.X}      # reverse reads against a random row
    # reads that a window limit skips
    w = aligned("align_edits", max_window=30)
    gw = model("align_edits", max_window=30)
    assert w.stats["too_wide"] > 0 and gw.stats["paths"] == w.stats["aligned"] < 13


def test_tool_cigar_needs_align():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--cigar" in p.stderr
    base = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2", "--rows"]
    for extra in (["--cigar"], ["--cigar", "--strands"]):
        p = subprocess.run([LOCATE] + base + extra, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--cigar needs --align" in p.stderr and b"usage:" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

def c_cigar(pix, n, want=(1, 1)):
    """fbg_pindex_chains_cigar and _fetch through the C calls -> n_ops, total, off, ops, ms; nothing past the arrays."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    n_ops = np.full(n + 1, 7, dtype=np.uint32)
    total, ms = ctypes.c_uint64(99), ctypes.c_double(0)
    rc = L.fbg_pindex_chains_cigar(pix._h, n_ops.ctypes.data_as(_lib.u32p) if want[0] else None,
                                   ctypes.byref(total) if want[1] else None, ctypes.byref(ms))
    assert rc == 0, rc
    assert n_ops[n] == 7
    off = np.full(n + 2, 7, dtype=np.uint64)
    assert L.fbg_pindex_chains_cigar_fetch(pix._h, off.ctypes.data_as(_lib.u64p), None) == 0
    assert off[n + 1] == 7
    t = int(off[n])
    ops = np.full(t + 1, 7, dtype=np.uint32)
    off2 = np.zeros(n + 1, dtype=np.uint64)
    assert L.fbg_pindex_chains_cigar_fetch(pix._h, off2.ctypes.data_as(_lib.u64p), ops.ctypes.data_as(_lib.u32p)) == 0
    assert ops[t] == 7 and np.array_equal(off2, off[:n + 1])
    if want[1]:
        assert total.value == t
    if want[0]:
        assert np.array_equal(n_ops[:n].astype(np.uint64), np.diff(off[:n + 1]))
    else:
        assert (n_ops == 7).all()
    return n_ops[:n], t, off[:n + 1], ops[:t], ms.value


def same(off, ops, g, what):
    assert off.dtype == g.off.dtype and ops.dtype == g.ops.dtype, what
    assert np.array_equal(off, g.off), (what, off.tolist(), g.off.tolist())
    assert np.array_equal(ops, g.ops), (what, [hex(x) for x in ops], [hex(x) for x in g.ops])


def same_chains(ch, g, what):
    same(ch.cigar_off, ch.cigar_ops, g, what)
    for R in range(len(g.runs)):
        assert ch.cigar(R) == g.strings[R], (what, R)
        runs = ch.cigar_runs(R)
        assert runs.dtype == np.int64 and runs.shape == (len(g.runs[R]), 2) and runs.tolist() == [list(r) for r in g.runs[R]]


def seeded(pix, c, strands):
    return pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band, min_score=c.min_score,
                     strands=strands, rows=True)


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_input_through_both_interfaces(engine, name, strands):
    """Every input at pads 16, 0 and 2^40 (`tiers` at 16 only) through the C calls and through Python, and after an
    align call with a window limit of 30, whose skipped reads have no runs."""
    c = cpu(name, strands)
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.cigar_stats() == ZERO_STATS
        sd = seeded(pix, c, strands)
        assert sd.chains.cigar_off is None and sd.chains.cigar_ops is None and sd.chains.cigar_ms is None
        for pad in PADS if name != "tiers" else PADS[:1]:
            m, g = aligned(name, strands, pad), model(name, strands, pad)
            TA.same(TA.c_align(pix, n, pad)[0], m, (name, pad, "align"))
            n_ops, total, off, ops, ms = c_cigar(pix, n)
            same(off, ops, g, (name, pad, "C"))
            assert total == g.stats["ops"] and pix.cigar_stats() == g.stats, (name, pad, pix.cigar_stats(), g.stats)
            assert ms > 0 or g.stats["paths"] == 0
            ch = pix.chains(band=c.band, min_score=c.min_score, align=True, pad=pad, cigar=True)
            TA.same((ch.align_row, ch.edits, ch.t_start, ch.t_end), m, (name, pad, "python align"))
            same_chains(ch, g, (name, pad, "python"))
            assert pix.cigar_stats() == g.stats and pix.align_stats() == TA.stats_of(m, c)
            plain = pix.chains(band=c.band, min_score=c.min_score, align=True, pad=pad)
            assert plain.cigar_off is None and plain.cigar_ops is None and plain.cigar_ms is None
        if name != "tiers":
            m, g = aligned(name, strands, 16, 30), model(name, strands, 16, 30)
            TA.same(TA.c_align(pix, n, 16, 30)[0], m, (name, "max_window"))
            _, _, off, ops, _ = c_cigar(pix, n)
            same(off, ops, g, (name, "max_window"))
            assert pix.cigar_stats() == g.stats
            for R in range(n):
                if m.edits[R] == NONE:
                    assert off[R] == off[R + 1]


@pytest.mark.gpu
def test_word_and_tier_boundaries(engine):
    """Reads of 1 .. max_read + 1 symbols against one row, together and each alone: 256 is the last read whose history
    stays in LDS, 257 the first whose history goes to device memory, and the read of max_read + 1 symbols is skipped."""
    c, m, g = cpu("align_boundary"), aligned("align_boundary"), model("align_boundary")
    assert [len(r) for r in c.reads] == list(TA.BOUNDARY_LENGTHS)
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        ch = pix.chains(align=True, cigar=True)
        same_chains(ch, g, "boundary")
        st = pix.cigar_stats()
        assert st == g.stats and st["paths"] == len(c.reads) - 1
        assert st["history_bytes"] == sum(GM.history_bytes(len(P), int(m.t_end[R] - m.t_start[R]))
                                          for R, P in enumerate(c.reads) if m.edits[R] != NONE and len(P) > 256) > 0
        assert ch.cigar(len(c.reads) - 1) == ""
        for R, P in enumerate(c.reads):
            pix.seeds([P], min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
            one = pix.chains(align=True, cigar=True)
            assert one.cigar(0) == g.strings[R] and one.cigar_off.tolist() == [0, len(g.runs[R])], len(P)
            st = pix.cigar_stats()
            hist = GM.history_bytes(len(P), int(m.t_end[R] - m.t_start[R])) if m.edits[R] != NONE else 0
            assert st["history_bytes"] == hist and (hist > 0) == (256 < len(P) <= AM.MAX_READ), len(P)
            assert st["batches"] == (1 if hist else 0) and st["paths"] == (0 if len(P) > AM.MAX_READ else 1)


@pytest.mark.gpu
def test_batches(engine):
    """A budget of 1 KiB makes every read of more than 256 symbols a batch of its own, one of 100 KiB only the longest, one
    of 300 KiB puts several into a batch (cigar_model.batches); the arrays are those of the default budget, which takes one
    batch.  No read of `tiers` that is aligned has
    more than 256 symbols (its long read has no carrying row), so that input has no batch under any budget."""
    from conftest import fbg_options
    for name, strands in (("align_boundary", False), ("align_boundary", True), ("tiers", False)):
        c, m, g = cpu(name, strands), aligned(name, strands), model(name, strands)
        long_reads = sum(1 for R, P in enumerate(c.vreads) if m.edits[R] != NONE and len(P) > 256)
        with TR.build(engine, c.A, c.b) as pix:
            seeded(pix, c, strands)
            ch = pix.chains(band=c.band, min_score=c.min_score, align=True, cigar=True)
            same_chains(ch, g, (name, "default"))
            assert pix.cigar_stats() == g.stats and g.stats["batches"] <= 1
            for kib in (1, 100, 300):
                with fbg_options(engine, {"path_batch_kib": kib}):
                    ch = pix.chains(band=c.band, min_score=c.min_score, align=True, cigar=True)
                    same_chains(ch, g, (name, kib))
                    st = pix.cigar_stats()
                assert st == dict(g.stats, batches=st["batches"])
                if name == "tiers":
                    assert long_reads == 0 and st["batches"] == 0
                else:
                    assert st["batches"] == GM.batches(g.hist, kib << 10) and long_reads >= 2
                    if kib == 1:
                        assert st["batches"] == long_reads > 1
        assert GM.batches(model("align_boundary").hist, 100 << 10) == 2 and GM.batches(model("align_boundary", True).hist, 300 << 10) == 2
        assert engine.get_option("path_batch_kib") == 1 << 20


@pytest.mark.gpu
def test_a_wave_per_chain_gives_the_same_paths(engine):
    from conftest import fbg_options
    c, g = cpu("align_edits"), model("align_edits")
    with fbg_options(engine, {"rows_wave": 1}), TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        TA.c_align(pix, len(c.reads))
        _, _, off, ops, _ = c_cigar(pix, len(c.reads))
        same(off, ops, g, "rows_wave")


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    big32, big64 = np.zeros(1 << 16, dtype=np.uint32), np.zeros(4096, dtype=np.uint64)
    call = lambda h: L.fbg_pindex_chains_cigar(h, u32(big32), None, None)      # noqa: E731
    fetch = lambda h: L.fbg_pindex_chains_cigar_fetch(h, u64(big64), u32(big32))      # noqa: E731
    c, m, g = cpu("chains"), aligned("chains"), model("chains")
    n = len(c.reads)
    # a NULL index
    assert call(None) == fetch(None) == L.fbg_pindex_cigar_stats(None, *[None] * 5) == _lib.FBG_ERR_INVALID
    with TR.build(engine, c.A, c.b, rows=False) as plain, TR.build(engine, c.A, c.b) as pix:
        # no row table
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(plain._h) == fetch(plain._h) == _lib.FBG_ERR_INVALID
        with pytest.raises(FbgError) as ei:
            plain.cigar_stats()
        assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
        # no seeds call yet; seeds without chains; chains without an align call
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID
        assert pix.cigar_stats() == ZERO_STATS
        # an align call, and a fetch before the cigar call
        TA.c_align(pix, n)
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID
        assert call(pix._h) == 0 and fetch(pix._h) == 0
        # no reads
        pix.seeds([], msa=True, chain=True)
        assert call(pix._h) == _lib.FBG_ERR_INVALID
        e = pix.chains(align=True, cigar=True)
        assert e.cigar_off.tolist() == [0] and len(e.cigar_ops) == 0 and e.cigar_ops.dtype == np.uint32
        assert call(pix._h) == 0 and fetch(pix._h) == 0 and pix.cigar_stats() == ZERO_STATS
        # reads without seeds: every chain empty
        pix.seeds([b"NN", b""], msa=True, chain=True)
        TA.c_align(pix, 2)
        n_ops, total, off, ops, _ = c_cigar(pix, 2)
        assert n_ops.tolist() == [0, 0] and total == 0 and off.tolist() == [0, 0, 0] and pix.cigar_stats() == ZERO_STATS
        # repeated calls, with and without the optional pointers; every other state as it was
        sd = seeded(pix, c, False)
        ch = sd.chains
        k = len(sd.q_start)
        TA.same(TA.c_align(pix, n)[0], m, "align")

        def state():
            nr, fr = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            bits = np.zeros(n * pix.rows_stats()["words_per_set"], dtype=np.uint64)
            assert L.fbg_pindex_chains_rows(pix._h, u32(nr), u32(fr), u64(bits), None) == 0
            pl, se = np.zeros(len(ch.anchor_place) + 1, dtype=np.uint32), np.zeros(len(ch.anchor_place) + 1, dtype=np.uint32)
            assert L.fbg_pindex_chains_fetch(pix._h, u32(pl), u32(se), None) == 0
            return (TC.seeds_state(pix, k), [a.tolist() for a in (nr, fr, bits, pl, se)], pix.stats(), pix.chain_stats(), pix.rows_stats(),
                    pix.align_stats())
        before = state()
        for want in ((1, 1), (0, 1), (0, 0), (1, 0), (1, 1)):
            _, _, off, ops, _ = c_cigar(pix, n, want)
            same(off, ops, g, want)
            assert pix.cigar_stats() == g.stats
        assert L.fbg_pindex_chains_cigar(pix._h, None, None, None) == 0 and L.fbg_pindex_chains_cigar_fetch(pix._h, None, None) == 0
        assert state() == before
        # the four align arrays come from the align call alone, and a new one starts over: it returns them again, has no
        # paths yet, and the paths follow
        TA.same(TA.c_align(pix, n)[0], m, "align again")
        assert fetch(pix._h) == _lib.FBG_ERR_INVALID          # the new align call has no paths yet
        same(*c_cigar(pix, n)[2:4], g, "again")
        # a locate and an occurrences call overwrite the reads on the device
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        mid = state()
        assert mid[:2] == before[:2] and mid[3:] == before[3:]
        same(*c_cigar(pix, n)[2:4], g, "after locate")
        assert state() == mid
        # a failed call leaves the stats
        assert call(None) == _lib.FBG_ERR_INVALID and pix.cigar_stats() == g.stats
        # a new align call with another pad changes the paths to that call's
        m0, g0 = aligned("chains", False, 0), model("chains", False, 0)
        TA.same(TA.c_align(pix, n, 0)[0], m0, "pad 0")
        same(*c_cigar(pix, n)[2:4], g0, "pad 0")
        assert pix.cigar_stats() == g0.stats
        # a new chains call invalidates the alignment and its paths; so does a new seeds call
        stats = pix.cigar_stats()
        pix.chains(band=c.band, min_score=c.min_score)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID and pix.cigar_stats() == stats
        TA.c_align(pix, n)
        assert call(pix._h) == 0 and fetch(pix._h) == 0
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        assert call(pix._h) == fetch(pix._h) == _lib.FBG_ERR_INVALID


def with_cigar(stdout, g, n, strands):
    """The --align output with the sixth field added to every G line that has numbers."""
    out, i = [], 0
    for ln in stdout.splitlines(keepends=True):
        if ln.startswith(b"G\t"):
            v = (i // 2 + (i % 2) * n) if strands else i
            i += 1
            if ln != b"G\t*\n":
                assert g.strings[v]
                ln = ln[:-1] + b"\t" + g.strings[v].encode() + b"\n"
            else:
                assert g.strings[v] == ""
        out.append(ln)
    return b"".join(out), i


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
def test_tool_prints_the_paths(engine, strands):
    """fbg_locate --align --cigar: the --align output (which test_align compares with the model) with the path, formatted
    here from the model, as the sixth field of every G line that has numbers; without --cigar no byte changes."""
    c = TA.cpu("align_tool", strands)
    args = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2", "--rows"] + (["--strands"] if strands else [])
    plain = TC.TL.run_locate(args, TA.TOOL_DATA)
    assert plain.returncode == 0, plain.stderr
    for flag, pad in (("--align", 16), ("--align=0", 0)):
        m = TA.model("align_tool", strands, pad)
        g = GM.of_align(c, m)
        base = TC.TL.run_locate(args + [flag], TA.TOOL_DATA)
        assert base.returncode == 0, base.stderr
        want_base, chains = TA.tool_lines(plain.stdout, m, len(c.reads), strands)
        assert base.stdout == want_base and chains == len(c.vreads)          # byte for byte the output of --align
        got = TC.TL.run_locate(args + [flag, "--cigar"], TA.TOOL_DATA)
        assert got.returncode == 0, got.stderr
        want, lines = with_cigar(base.stdout, g, len(c.reads), strands)
        assert lines == len(c.vreads) and got.stdout == want
    assert any(g.strings) and not all(g.strings)
