"""Alignment and alignment paths on long edited reads, many rows, many blocks and many reads in one call:
fbg_pindex_chains_align (k_pa_prefix, k_pa_prepare, k_pa_gather, k_pa_edit) and fbg_pindex_chains_cigar (k_pg_sizes,
k_pg_path<NW>, k_pg_compact and the host's batch loop) of csrc/pindex_align.hip, between the toy inputs of test_align.py and
test_cigar.py and the workload of the benchmarks.

The checkers are tests/align_model.py and tests/cigar_model.py on the CPU pipeline of test_mapping_scale.cpu(); every
comparison with the engine is exact.  The DPs of the models go a row at a time in numpy here (LITERAL_CELLS is lowered
for the length of a call; test_align.py and test_cigar.py compare that form with the literal one).  The inputs:

  founders, repeats, m16, m17, m128   those of test_mapping_scale.py: the breadth (200 rows, about 140 blocks, more than
             8000 virtual reads, the row counts beside the lane switch).  None aligns a read of more than 120 symbols.
  long_edits the MSA and segmentation of `founders`; reads of 64 .. 1025 symbols cut from random rows with substitutions,
             deleted and inserted symbols planted at the word boundaries of the forward pass (read positions 64 k) and
             of the history pass (L - 64 k), a share with a zero byte or an N, every third on the reverse strand.
  bytes      3 rows x 400 columns over the bytes 0x80 .. 0xFE and lower-case letters, reads of 70, 130 and 330 symbols
             with a substitution, an inserted and a deleted symbol each.

A planted edit at read position p: the read symbol p is replaced (X) or is an extra symbol (I), or the text symbol
behind p read symbols is left out (D, or two of them).  An I of a path is counted at the index i of its read symbol and a
D at the number i of read symbols before it; the kernel's trace is then at a = L - i, and a - 1 leaves a word where
(L - i) % 64 is 1.

What a read of one word cannot show: a D with i in {1, L - 1}.  A path "1=1D.." costs no less than the path that starts
one text symbol later with X or =, and the start rule takes the largest start; a path "..1D1=" costs no less than the
one that ends one symbol earlier, and the end rule takes the smallest end.  So the D cases at (L - i) % 64 in {0, 1, 63}
are asserted for the reads of 2 to 4 and of 5 to 16 words, and asserted absent for the reads of one word."""
import collections
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import cigar_model as GM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_align as TA  # noqa: E402
import test_cigar as TG  # noqa: E402
import test_mapping_scale as TM  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options  # noqa: E402

NONE = AM.NONE
TABLE = TM.TABLE
HUGE = TA.HUGE
SCALE = ("founders", "repeats", "m16", "m17", "m128")
LENGTHS = (64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 320, 321, 383, 384, 385, 448, 512, 513, 640, 704, 768, 832,
           896, 960, 1023, 1024, 1025)
REPS = 12
TAIL_LENGTHS = (180, 330)             # reads across the private symbols near the end of founders' row EARLY: no other row carries them
EDIT_AT = (63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321)
KINDS = ("X", "D", "I", "DD")
COST = {"X": 1, "D": 1, "I": 1, "DD": 2}
MAX_EDITS, EDIT_GAP = 3, 26          # per read; symbols between two planted edits (seeds of 12 on both sides of each)
BUDGET_SHARED, BUDGET_EACH = 1024, 1  # path_batch_kib: several history reads a batch; less than any history, so one a batch
GROUPS = ((1, 1), (2, 4), (5, 16))    # word counts: one word, the register tier, the LDS-state tier


# ---- the inputs ---------------------------------------------------------------------------------------------------------

def foreign(g, x):
    """A symbol that differs from the text around position x, so an X or I planted there can be nothing cheaper."""
    return next(ch for ch in b"ACGT" if ch not in g[max(x - 1, 0):x + 2])


def edit_positions(rng, L):
    """A few of the read positions p and L - p, p in EDIT_AT, inside (20, L - 20) and EDIT_GAP apart, in random order."""
    cand = sorted({x for p in EDIT_AT for x in (p, L - p) if 20 < x < L - 20})
    at = []
    for x in rng.permutation(cand).tolist():
        if len(at) < MAX_EDITS and all(abs(x - y) >= EDIT_GAP for y in at):
            at.append(x)
    return sorted(at)


def edited(g, a, L, at, kind):
    """-> (L symbols of g from offset a on with an edit at every read position of `at`, the kinds cycling from `kind` on,
    [(position, kind)])."""
    out, src, plan = bytearray(), a, []
    for pos in at:
        take = pos - len(out)
        out += g[src:src + take]
        src += take
        k = KINDS[kind % len(KINDS)]
        kind += 1
        plan.append((pos, k))
        if k == "X":
            out.append(foreign(g, src))
            src += 1
        elif k == "I":
            out.append(foreign(g, src))
        else:
            src += len(k)
    out += g[src:src + L - len(out)]
    assert len(out) == L
    return bytes(out), plan


def long_edits_input():
    """truth[R]: (row, offset, L, strand, planted edit operations, [(position, kind)])."""
    A = TM.founders_msa()[0]
    G = TM.stripped(A)
    rng = np.random.default_rng(77)
    reads, truth, kind = [], [], 0
    for j in range(REPS * len(LENGTHS) + len(TAIL_LENGTHS)):
        if j < REPS * len(LENGTHS):
            L = LENGTHS[j % len(LENGTHS)]
            r = int(rng.integers(0, len(G)))
            a = int(rng.integers(0, len(G[r]) - L - 2 * MAX_EDITS))
        else:                                # the tail of the row that ends early, up to four symbols before its end
            L, r = TAIL_LENGTHS[j - REPS * len(LENGTHS)], TM.EARLY
            a = len(G[r]) - L - 4
        at = edit_positions(rng, L)
        s, plan = edited(G[r], a, L, at, kind)
        kind += len(at)
        planted = sum(COST[k] for _, k in plan)
        if j % 4 == 3:                       # a byte that no row holds: 0 or N; in a read of one word at either end
            ends = (0, L - 1)[(j // 4) % 2]
            free = [x for x in range(13, L - 13) if all(abs(x - p) > 13 for p in at)]
            x = ends if L <= 64 else free[int(rng.integers(0, len(free)))]
            s = s[:x] + (b"\0", b"N")[(j // 8) % 2] + s[x + 1:]
            plan = plan + [(x, "byte")]
            planted += 1
        strand = int(j % 3 == 2)
        reads.append(STM.revcomp(s, TABLE) if strand else s)
        truth.append((r, a, L, strand, planted, plan))
    return A, reads, truth, 80


HIGH = bytes(range(0x80, 0xff)) + b"abcdefghijklmnopqrstuvwxyz"
BYTE_LENGTHS = (70, 130, 330)


def bytes_input():
    """An input of test_rows' form: three unrelated random rows over HIGH (every place has one row); per length of
    BYTE_LENGTHS a read cut from a row of its own, with a substitution, an inserted and a deleted symbol."""
    rng = np.random.default_rng(909)
    rows = [bytes(rng.choice(list(HIGH), 400).tolist()) for _ in range(3)]
    reads = []
    for k, L in enumerate(BYTE_LENGTHS):
        a, base = 5 + 20 * k, rows[k]
        P = bytearray(base[a:a + L + 1])
        x, i, d = L // 4, L // 2, (3 * L) // 4
        del P[d]                                                             # a deleted symbol
        P.insert(i, next(ch for ch in HIGH if ch not in base[a + i - 1:a + i + 2]))      # an inserted symbol
        P[x] = next(ch for ch in HIGH if ch not in base[a + x - 1:a + x + 2])            # a substitution
        reads.append(bytes(P[:L]))
    return TR.msa_of(rows), [49, 99, 149, 199, 249, 299, 349, 399], reads, 12, 8, None, 0


OWN = {"long_edits": long_edits_input}


@functools.lru_cache(maxsize=None)
def cpu(name):
    """test_mapping_scale.cpu() on one of its inputs or on `long_edits`, which is in its table for the length of the call."""
    with mock.patch.dict(TM.INPUTS, OWN):
        return TM.cpu(name)


@functools.lru_cache(maxsize=None)
def bytes_cpu():
    with mock.patch.dict(TR.INPUTS, {"bytes": bytes_input}):
        return TR.cpu("bytes")


def by_rows(model):
    return mock.patch.object(model, "LITERAL_CELLS", 0)


@functools.lru_cache(maxsize=None)
def aligned(name, pad=16, max_window=0):
    with by_rows(AM):
        return AM.of_cpu(bytes_cpu() if name == "bytes" else cpu(name), pad, max_window)


@functools.lru_cache(maxsize=None)
def paths(name, pad=16, max_window=0):
    with by_rows(GM):
        return GM.of_align(bytes_cpu() if name == "bytes" else cpu(name), aligned(name, pad, max_window))


def words(L):
    return (L + 63) // 64


def history(c, m):
    """Bytes of device history per virtual read (0: none)."""
    return [GM.history_bytes(len(c.vreads[R]), int(m.t_end[R] - m.t_start[R])) if m.edits[R] != NONE else 0 for R in range(len(c.vreads))]


def batch_ranges(hist, budget):
    """cigar_model.batches with the reads of every batch: [[R, ...]] of the reads with a history, by the same rule."""
    out, room = [], None
    for R, h in enumerate(hist):
        if h == 0:
            continue
        if room is None or h > room:
            out.append([])
            room = budget
        out[-1].append(R)
        room = max(room - h, 0)
    return out


def indel_cells(runs):
    """-> ([i of every inserted read symbol], [i = read symbols before every D run])."""
    i, ins, dels = 0, [], []
    for code, n in runs:
        if code == GM.I:
            ins += range(i, i + n)
        if code == GM.D:
            dels.append(i)
        else:
            i += n
    return ins, dels


BESIDE = (0, 1, 63)


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_long_edits_input_is_what_it_claims():
    c, m, g = cpu("long_edits"), aligned("long_edits"), paths("long_edits")
    n, nv = len(c.reads), len(c.vreads)
    ok = [R for R in range(nv) if m.edits[R] != NONE]
    L = {R: len(c.vreads[R]) for R in ok}
    N = {R: int(m.t_end[R] - m.t_start[R]) for R in ok}
    assert sorted({len(r) for r in c.reads[:-len(TAIL_LENGTHS)]}) == list(LENGTHS) and n == REPS * len(LENGTHS) + len(TAIL_LENGTHS)
    # every word count: reads, an I, a D
    per = collections.Counter(words(L[R]) for R in ok)
    with_i = {words(L[R]) for R in ok if any(k == GM.I for k, _ in g.runs[R])}
    with_d = {words(L[R]) for R in ok if any(k == GM.D for k, _ in g.runs[R])}
    every = set(range(1, 17))
    assert all(per[w] >= 2 for w in every) and with_i == every and with_d == every, (per, with_i, with_d)
    assert any(L[R] == AM.MAX_READ for R in ok) and m.stats["too_long"] >= 1
    # an I and a D beside a word boundary of the history pass (counted from the read's end) and of the forward pass
    hits = collections.Counter()
    for R in ok:
        grp = next(k for k, (lo, hi) in enumerate(GROUPS) if lo <= words(L[R]) <= hi)
        ins, dels = indel_cells(g.runs[R])
        for op, cells in (("I", ins), ("D", dels)):
            hits[grp, op, "end"] += sum((L[R] - i) % 64 in BESIDE for i in cells)
            hits[grp, op, "start"] += sum(i % 64 in BESIDE for i in cells)
            for i in cells:
                hits[grp, op, "end", (L[R] - i) % 64] += 1
    for grp in range(len(GROUPS)):
        for side in ("end", "start"):
            assert hits[grp, "I", side] > 0, (grp, side)
            assert (hits[grp, "D", side] > 0) == (grp > 0), (grp, side)          # one word: see the head of this file
    for grp in (1, 2):                                # each of the three residues on its own, where a - 1 leaves a word
        assert all(hits[grp, op, "end", k] > 0 for op in "ID" for k in BESIDE), hits
    # N on either side of L; many runs; many edits; rows of every word of the row sets
    assert any(N[R] > L[R] for R in ok) and any(N[R] < L[R] for R in ok)
    assert any(words(L[R]) == 16 and N[R] >= L[R] + 2 for R in ok)
    most_runs = max(len(g.runs[R]) for R in ok)
    assert most_runs > 100
    heavy = [R for R in ok if words(L[R]) >= 5 and 4 * int(m.edits[R]) > L[R]]
    assert heavy
    rows = {int(m.row[R]) for R in ok}
    assert any(64 <= r < 128 for r in rows) and any(r >= 128 for r in rows)
    # the row that ends early: a window up to its last symbol, behind which the row has cells without a node
    end = len(c.rm.G[TM.EARLY])
    tails = [R for R in ok if m.row[R] == TM.EARLY and m.windows[R][1] == end]
    assert tails and any(k in (GM.I, GM.D) for R in tails for k, _ in g.runs[R]) and len(c.rm.G[0]) > end + 100
    # the histories in device memory and their batches
    hist = history(c, m)
    assert [h for R, h in enumerate(hist) if m.edits[R] != NONE] == g.hist
    long_reads = [R for R, h in enumerate(hist) if h]
    assert len(long_reads) >= 40 and g.stats["history_bytes"] == sum(hist)
    shared, each = batch_ranges(hist, BUDGET_SHARED << 10), batch_ranges(hist, BUDGET_EACH << 10)
    assert len(shared) == GM.batches(g.hist, BUDGET_SHARED << 10) >= 3 and sum(len(b) >= 2 for b in shared) >= 2
    assert len(each) == GM.batches(g.hist, BUDGET_EACH << 10) == len(long_reads) and max(hist) > BUDGET_EACH << 10
    assert g.stats["batches"] == 1
    between = sum(any(hist[R] == 0 for R in range(b[0], b[-1])) for b in shared)
    unaligned_between = sum(any(m.edits[R] == NONE for R in range(b[0], b[-1])) for b in shared)
    assert between > 0 and unaligned_between > 0
    print("long_edits", dict(virtual_reads=nv, aligned=m.stats["aligned"], too_long=m.stats["too_long"], unsupported=m.stats["unsupported"],
                             cells=m.stats["cells"], per_word_count=[per[w] for w in range(1, 17)], widest_N=max(N.values()),
                             most_edits=max(int(m.edits[R]) for R in ok), most_runs=most_runs, runs=g.stats["ops"], heavy=len(heavy),
                             history_reads=len(long_reads), history_bytes=(min(h for h in hist if h), max(hist), sum(hist)),
                             batches={BUDGET_SHARED: len(shared), BUDGET_EACH: len(each)}, rows=len(rows),
                             rows_from_64=sum(m.row[R] >= 64 for R in ok)))
    print("long_edits indels beside a word boundary", {k: v for k, v in sorted(hits.items()) if len(k) == 3})


def test_long_edits_against_the_planted_edits():
    """The ground truth outside the models: where the strand is the one the read was cut from and the model's row is the
    row it was cut from, the planted edits are one alignment to that row inside the window, so edits is at most their
    number (two for a two-symbol deletion, one for the foreign byte), and t_start lies within that many symbols of the
    offset the read was cut at (an alignment of at most e edits starts within e symbols of the diagonal)."""
    c, m = cpu("long_edits"), aligned("long_edits")
    n = len(c.reads)
    judged = exact = 0
    for R, (row, a, L, strand, planted, plan) in enumerate(c.truth):
        v = strand * n + R
        if int(c.strand[R]) != strand or m.edits[v] == NONE or int(m.row[v]) != row:
            continue
        judged += 1
        exact += int(m.edits[v]) == planted
        assert int(m.edits[v]) <= planted, (R, int(m.edits[v]), plan)
        assert abs(int(m.t_start[v]) - a) <= planted, (R, int(m.t_start[v]), a, plan)      # v is the read as it was cut
    print("long_edits ground truth", dict(reads=n, judged=judged, edits_equal_planted=exact))
    assert judged >= 20


@pytest.mark.parametrize("name", SCALE)
def test_scale_inputs_have_what_the_align_tests_need(name):
    c, m, g = cpu(name), aligned(name), paths(name)
    ok = m.edits != NONE
    assert ok.sum() > 100 and m.stats["unsupported"] > 0 and (m.edits[ok] > 0).sum() > 10
    zero_between = sum(g.off[R] == g.off[R + 1] and 0 < g.off[R] < g.off[-1] for R in range(len(c.vreads)))
    assert zero_between > 100                                       # reads without runs between others
    if name == "founders":
        assert len(c.vreads) + 1 > 8000 and len(c.b) > 100 and c.rm.m > 64
        assert ((m.row != NONE) & (m.row >= 64) & (m.row < 128)).any() and ((m.row != NONE) & (m.row >= 128)).any()
        assert any(w and w[0] == 0 for w in m.windows) and any(w and w[1] == len(c.rm.G[int(m.row[R])]) for R, w in enumerate(m.windows))
        indel = sum(any(k in (GM.I, GM.D) for k, _ in r) for r in g.runs)
        assert indel > 100
        w = aligned(name, 16, founders_window())
        assert w.stats["too_wide"] > 0 and w.stats["aligned"] > 0
    if name in ("m17", "m128"):
        h = aligned(name, HUGE)
        assert all(w == (0, len(c.rm.G[int(h.row[R])])) for R, w in enumerate(h.windows) if w)          # both clamps
    print(name, dict(virtual_reads=len(c.vreads), aligned=m.stats["aligned"], unsupported=m.stats["unsupported"], too_long=m.stats["too_long"],
                     cells=m.stats["cells"], runs=g.stats["ops"], zero_between=zero_between))


def founders_window():
    """The median window length of the model at pad 16."""
    m = aligned("founders")
    return int(np.median([w[1] - w[0] for w in m.windows if w]))


def test_bytes_input_is_what_it_claims():
    c, m, g = bytes_cpu(), aligned("bytes"), paths("bytes")
    assert [len(r) for r in c.reads] == list(BYTE_LENGTHS) and min(min(r) for r in c.reads) >= 0x61 and max(max(r) for r in c.reads) >= 0xf0
    assert sum(max(r) >= 0x80 for r in c.A.tolist()) == 3
    for R in range(len(c.reads)):
        assert m.edits[R] == 3 and m.row[R] == R, (R, g.strings[R])
        assert {k for k, _ in g.runs[R]} == {GM.EQ, GM.X, GM.I, GM.D}, g.strings[R]
    print("bytes", g.strings)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

ALIGN = ("align_row", "edits", "t_start", "t_end")


def traced(pix, c, pad=16, max_window=0):
    return pix.chains(band=c.band, min_score=c.min_score, rows=True, align=True, pad=pad, max_window=max_window, cigar=True)


def arrays(ch):
    return [getattr(ch, f).tolist() for f in ALIGN + ("cigar_off", "cigar_ops")] + ([ch.best_edits.tolist()] if ch.best_edits is not None else [])


def check(pix, ch, c, m, g, what, batches=None):
    """The arrays and statistics of a chains(align=True, cigar=True) call against the models."""
    TA.same([getattr(ch, f) for f in ALIGN], m, what)
    if ch.strand is not None:
        assert np.array_equal(ch.strand, c.strand), what
        want = AM.best_edits(m.edits, c.strand)
        assert ch.best_edits.dtype == want.dtype and np.array_equal(ch.best_edits, want), what
    else:
        assert ch.best_edits is None
    assert pix.align_stats() == TA.stats_of(m, c), (what, pix.align_stats(), m.stats)
    TG.same(ch.cigar_off, ch.cigar_ops, g, what)
    assert np.diff(ch.cigar_off.astype(np.int64)).tolist() == [len(r) for r in g.runs], what
    want = g.stats if batches is None else dict(g.stats, batches=batches)
    assert pix.cigar_stats() == want, (what, pix.cigar_stats(), want)


def run(engine, name, cases, options=None):
    """One index of the input and a stranded call; then every (pad, max_window) of `cases` against the models."""
    c = cpu(name)
    out = []
    with fbg_options(engine, options or {}), TR.build(engine, c.A, c.b) as pix:
        sd = TM.call(pix, c)
        TR.same_as_cpu(sd, c, name)
        for pad, mw in cases:
            ch = traced(pix, c, pad, mw)
            check(pix, ch, c, aligned(name, pad, mw), paths(name, pad, mw), (name, pad, mw))
            out.append(arrays(ch))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [16, 0])
@pytest.mark.parametrize("name", SCALE)
def test_scale_inputs(engine, name, pad):
    run(engine, name, [(pad, 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m17", "m128"])
def test_whole_rows_as_windows(engine, name):
    run(engine, name, [(HUGE, 0)])


@pytest.mark.gpu
def test_founders_with_a_window_limit(engine):
    mw = founders_window()
    m = aligned("founders", 16, mw)
    assert m.stats["too_wide"] > 0 and m.stats["aligned"] > 0
    run(engine, "founders", [(16, mw)])


@pytest.mark.gpu
def test_a_wave_per_chain_on_sixteen_rows(engine):
    assert run(engine, "m16", [(16, 0), (0, 0)], {"rows_wave": 1}) == run(engine, "m16", [(16, 0), (0, 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [16, 0])
@pytest.mark.parametrize("strands", [False, True])
def test_long_edits(engine, strands, pad):
    """Plain (the virtual reads given as reads) and stranded."""
    c, m, g = cpu("long_edits"), aligned("long_edits", pad), paths("long_edits", pad)
    with TR.build(engine, c.A, c.b) as pix:
        sd = TM.call(pix, c) if strands else TM.call(pix, c, reads=c.vreads, strands=False)
        TR.same_as_cpu(sd, c, "long_edits")
        ch = traced(pix, c, pad)
        assert (ch.strand is not None) == strands
        check(pix, ch, c, m, g, ("long_edits", strands, pad))
        assert pix.cigar_stats()["history_bytes"] == sum(history(c, m)) > 0


@pytest.mark.gpu
def test_long_edits_in_batches(engine):
    """The budgets of test_long_edits_input_is_what_it_claims: the same arrays, the model's number of batches."""
    c, m, g = cpu("long_edits"), aligned("long_edits"), paths("long_edits")
    with TR.build(engine, c.A, c.b) as pix:
        TM.call(pix, c)
        whole = traced(pix, c)
        check(pix, whole, c, m, g, "default")
        assert g.stats["batches"] == 1
        for kib in (BUDGET_SHARED, BUDGET_EACH, BUDGET_SHARED):
            with fbg_options(engine, {"path_batch_kib": kib}):
                ch = traced(pix, c)
                check(pix, ch, c, m, g, kib, batches=GM.batches(g.hist, kib << 10))
            assert arrays(ch) == arrays(whole)
        assert GM.batches(g.hist, BUDGET_SHARED << 10) >= 3 and GM.batches(g.hist, BUDGET_EACH << 10) >= 40


@pytest.mark.gpu
def test_long_edits_through_the_c_calls(engine):
    c, m, g = cpu("long_edits"), aligned("long_edits"), paths("long_edits")
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        TM.call(pix, c)
        got, ms = TA.c_align(pix, n)
        TA.same(got, m, "C align")
        assert ms > 0 and pix.align_stats() == TA.stats_of(m, c)
        n_ops, total, off, ops, ms = TG.c_cigar(pix, n)
        TG.same(off, ops, g, "C cigar")
        assert n_ops.tolist() == [len(r) for r in g.runs] and total == g.stats["ops"] and ms > 0 and pix.cigar_stats() == g.stats
        ch = traced(pix, c)
        for f, a in zip(ALIGN, got):
            assert np.array_equal(getattr(ch, f), a), f
        assert np.array_equal(ch.cigar_off, off) and np.array_equal(ch.cigar_ops, ops)


def subset(c, m, g, given):
    """The models' results for the stranded call on the reads `given` of c: per read they do not depend on the batch."""
    n = len(c.reads)
    v = list(given) + [n + R for R in given]
    out = [getattr(m, f)[v].tolist() for f in TA.FIELDS]
    runs = [g.runs[R] for R in v]
    ops = [x for r in runs for x in GM.encode(r)]
    out += [np.cumsum([0] + [len(r) for r in runs]).tolist(), ops]
    out.append(AM.best_edits(m.edits[v], c.strand[list(given)]).tolist())
    hist = [history(c, m)[R] for R in v]
    stats = dict(paths=sum(m.edits[R] != NONE for R in v), ops=len(ops), columns=sum(int(m.t_end[R] - m.t_start[R]) for R in v if m.edits[R] != NONE),
                 history_bytes=sum(hist), batches=int(any(hist)))
    return out, stats


@pytest.mark.gpu
def test_one_index_large_then_small_then_large(engine):
    """The founders batch, three reads of long_edits (one with a history in device memory), a locate and an occurrences
    call (they overwrite the reads on the device), the three reads' chains again from the saved reads, the founders
    batch again: every array is a fresh index's and the model's."""
    f, fm, fg = cpu("founders"), aligned("founders"), paths("founders")
    c, m, g = cpu("long_edits"), aligned("long_edits"), paths("long_edits")
    assert np.array_equal(f.A, c.A) and f.b == c.b
    n, hist = len(c.reads), history(c, m)
    with_history = next(R for R in range(n) if hist[R] and c.strand[R] == 0)
    short = next(R for R in range(n) if m.edits[R] != NONE and len(c.reads[R]) <= 256 and any(k == GM.D for k, _ in g.runs[R]))
    unaligned = next(R for R in range(n) if m.edits[R] == NONE and m.edits[n + R] == NONE)
    given = sorted((with_history, short, unaligned))
    three = [c.reads[R] for R in given]
    want, want_stats = subset(c, m, g, given)
    assert want_stats["history_bytes"] > 0 and want_stats["paths"] >= 2
    patterns = [r for r in f.vreads[:1500] if r] + [b"ACGT" * 400]
    with TR.build(engine, c.A, c.b) as fresh:
        TM.call(fresh, c, reads=three)
        small = arrays(traced(fresh, c))
        assert small == want and fresh.cigar_stats() == want_stats
    with TR.build(engine, f.A, f.b) as pix:
        TM.call(pix, f)
        first = traced(pix, f)                                  # the first call of a fresh index
        check(pix, first, f, fm, fg, "first")
        large = arrays(first)
        TM.call(pix, c, reads=three)
        assert arrays(traced(pix, c)) == small and pix.cigar_stats() == want_stats
        count = pix.locate(patterns)[0]
        assert (count > 0).sum() > 500
        pix.occurrences(patterns[:200], max_per_pattern=8)
        assert arrays(traced(pix, c)) == small and pix.cigar_stats() == want_stats      # the saved reads, shorter than the buffers
        TM.call(pix, f)
        again = traced(pix, f)
        check(pix, again, f, fm, fg, "again")
        assert arrays(again) == large


@pytest.mark.gpu
def test_bytes_are_compared_as_they_are(engine):
    c, m, g = bytes_cpu(), aligned("bytes"), paths("bytes")
    with TR.build(engine, c.A, c.b) as pix:
        sd = TA.seeded(pix, c, False)
        TR.same_as_cpu(sd, c, "bytes")
        ch = traced(pix, c)
        check(pix, ch, c, m, g, "bytes")
        TG.same_chains(ch, g, "bytes")
        assert m.edits.tolist() == [3, 3, 3]
