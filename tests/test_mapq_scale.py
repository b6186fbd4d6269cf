"""The second-best chain and the mapping quality (fbg_pindex_chains_mapq, fbg_pindex_mapq_strands, fbg_pindex_mapq_stats;
k_pq_span, k_pq_mask, k_pq_final of csrc/pindex_mapq.hip and the chain kernels in the mapq state's own chain state) on
one seeded input with duplicated loci, thousands of workgroups of start places and a ground truth outside the model,
between the toy inputs of test_mapq.py and a workload.  The helpers are those of test_mapping_scale.py; its cpu() runs
here with max_per_seed 64 and band 8.  Every call is stranded with min_length 12; every GPU comparison is exact.

The input `duplications`: 50 rows x 3460 columns, copies of twelve founders with private substitutions (1.2 % of the
cells).  Rows and long reads are fewer than a first sketch of 200 rows and 300 long reads had: the models' time on the
CPU is quadratic in the places of a read, and rows_model and byrow_model are linear in the rows.
  * A 600-column segment of the founders at [100, 700) is planted at [1420, 2020) with one column in 50 diverged and at
    [2160, 2760) with one in 20 (a diverged column has another symbol in every founder, gaps stay gaps; one column per
    stride, so the blocks of the copies stay short).  The loci are more than 100 columns apart.
  * The first 200 columns of the segment, and 100 columns before each of the three loci, are alike in all rows and free
    of private substitutions.  A start place is an edge: a seed inside a node has as many places as the node has edges in
    and out, and a block with one diverse column has a dozen nodes.  Only between one-node blocks does a seed have the two
    or three places per locus that leave a read of several seeds in the small tier (32 places); the short reads are cut
    there.  Without the stretch the small tier had no secondary of more than two anchors.
  * Two arrays of 30 copies of the 16-symbol UNIT at [820, 1300) and [2880, 3360), the first the same in all rows, the
    second with a substitution in four rows.  Their 12-mers have more than a thousand places (30 copies x the edges of the
    nodes), the cap keeps 64 in a few columns, and the reads cut there chain poorly: they are in the input for the capped
    seeds and the long offset ranges, not for their chains.
  * Reads, 926 in all, each simulated one with its truth (row, offset, length, strand): 600 from simulate() with 8 empty
    and all-N reads in between; 20 per array with an N at every 13th symbol, half of them 300 to 520 symbols across and
    inside the array; 150 long reads of 150 to 550 symbols (four in five at least 400: the spill tier) from the three loci
    and up to 40 symbols past their ends, an N at every 13th symbol, strands alternating; 100 short ones of 40 to 100
    symbols made the same way inside the conserved stretch; 16 reads of 38 symbols, 30 symbols left out, and 38 more, so
    that the band keeps the two pieces in two chains 30 columns apart: the reads on which margin 0 and margin 50 differ (the
    loci and the capped arrays give none); 12 reads of a piece and its reverse complement, where the twin strand competes.

What the CPU tests assert of the models, at margin 0 unless said (measured):
  (a) virtual reads with a secondary of at least 3 anchors in the small tier: 78; of at least 8 in the wave tier: 105, in
      the spill tier: 43 (at least 40 each); the longest secondary has 34 anchors;
  (b) among virtual reads with a primary chain, mapq 0 with second == score: 184; 0 < second < score: 309; mapq 60: 338
      (at least 100 each); mapq_stranded < mapq: 47 (at least 20);
  (c) 1852 virtual reads, 7413 seeds, 194 638 start places (hundreds of workgroups of k_pq_mask); the mask keeps 103 116 of them,
      53 % (20 % to 80 %); half the virtual reads have no seed and lie between reads that have seeds and places; 1800
      seeds are capped.  A seed without a place does not occur at max_per_seed 64 (a reported seed has an occurrence):
      that case of the offset search stays with test_mapq.test_state_rules;
  (d) margin 0 and margin 50 give different secondaries for 21 reads (at least 10);
  (e) for every simulated read none of whose seeds on its true strand was capped (count > max_per_seed): if mapq > 0 on the true strand, [lo - margin, hi + margin) of
      the primary chain meets the true columns of the read.  538 reads are judged, 523 of them with mapq > 0, at margins 0
      and 50, without a violation;
  (f) none of these reads has mapq_stranded 0 on its true strand and a positive one on the other.
Recorded, not required: mapq of the true strands in steps of ten: 203, 142, 56, 58, 17, 76, 338; 14 simulated reads lie
inside the segment or its first copy where the two have the same text, 8 of them get mapq 0 (the others carry a private
substitution or an N that tells the loci apart).  A min_score of 120 empties 795 primary chains.

The by-row calls run with option byrow_max = 512: 767 virtual reads are chained along a row, 170 have more places and
come out empty (no secondary, quality 0), and for a few reads the secondary beats the chain of the chosen row.

Margins 0 and 50 put 60 and 2 anchors exactly above the widened span (c == hi + margin) and none exactly below it
(c + k + margin == lo): a chain takes in what abuts it.  The plain parity test therefore also runs at margin EDGE = 1308,
the distance of the first copy from the segment less the seed length, where 224 anchors lie on the lower and 604 on the
upper edge (on_the_edge, asserted on the CPU).

Which test fails for an error in pindex_mapq.hip (each tried once on a scratch build, never committed): `>=` for `>`
at the lower end of the widened span in k_pq_mask fails the plain parity at margin EDGE (secondaries) and the by-row
parity (one anchor in anchors_kept); `<=` for `<` at the upper end fails the plain parity, the batch and the one-index
test (60 anchors at margin 0); a wrong read from po_find at a read without seeds masks a read's places with
its neighbour's span, and every second virtual read is such a neighbour (parity, and the batch test, where the neighbours
differ between the runs: all five tests failed); a counter that loses waves shows in mapq_stats() over hundreds of workgroups of places and several
of reads (anchors_kept 25 651 for 103 116); the twin index off by one gives the 47 reads of (b) and the 12 inverted reads another competitor
(mapq_stranded, best_mapq, and (f) on the engine's output)."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import byrow_model as BM  # noqa: E402
import mapq_model as QM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains_by_row as TB  # noqa: E402
import test_mapping_scale as MS  # noqa: E402
import test_mapq as TQ  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options, random_msa  # noqa: E402

GAP = MS.GAP
NONE = QM.NONE
U64 = QM.U64_MAX
TABLE, UNIT = MS.TABLE, MS.UNIT
ROWS, BASE = 50, 2500                       # the MSA before the arrays are inserted
SEGMENT, COPIES_AT, DIVERGED = (100, 700), (940, 1680), (0.02, 0.05)
FLANK, CONSERVED = 100, 200                 # columns before a locus and at its start that are alike in all rows
ARRAYS_AT, ARRAY_COPIES = (820, 2400), 30   # columns of the base MSA before which the two arrays are inserted
CAP, BAND = 64, 8                           # of every call; the band is below the period of the arrays
MARGINS = (0, 50)
EDGE = COPIES_AT[0] + len(UNIT) * ARRAY_COPIES - SEGMENT[0] - 12      # the margin at which the seeds of the other locus abut: see on_the_edge
HIGH = 120                                  # a min_score that empties a share of the chains
N_RANDOM, N_TANDEM, N_LONG, N_SHORT, N_INVERTED = 600, 20, 150, 100, 12
N_DELETION = 16
BYROW_MAX = 512                             # option byrow_max of the by-row calls: the model's cost is quadratic in it


# ---- the input ----------------------------------------------------------------------------------------------------------

def diverge(rng, F, x0, x1, share):
    """One column in every 1 / share of the columns [x0, x1) gets another symbol in every founder (one shift per column);
    gaps stay gaps."""
    w = int(round(1 / share))
    at = np.arange(x0, x1, w) + rng.integers(0, w, len(range(x0, x1, w)))
    for x, d in zip(at.tolist(), rng.integers(1, 4, len(at)).tolist()):
        sym = F[:, x] != GAP
        F[sym, x] = MS.ALPHA[(np.searchsorted(MS.ALPHA, F[sym, x]) + d) % 4]
    return at


@functools.lru_cache(maxsize=None)
def duplications_msa():
    """-> (A, loci, diverged): loci[name] = (first column, column after the last) in A of 'segment', 'copy1', 'copy2',
    'array1', 'array2'; diverged[name] = the diverged columns of 'copy1' and 'copy2', counted from the copy's first."""
    rng = np.random.default_rng(2031)
    F = random_msa(rng, 12, BASE, gap_p=0.004, gap_run=5, similar=0.93)
    s0, s1 = SEGMENT
    same = np.random.default_rng(2032)
    F[:, s0:s0 + CONSERVED] = random_msa(same, 12, CONSERVED, similar=1.0)
    diverged = {}
    for name, at, share in zip(("copy1", "copy2"), COPIES_AT, DIVERGED):
        F[:, at:at + s1 - s0] = F[:, s0:s1]
        diverged[name] = diverge(rng, F, at, at + s1 - s0, share) - at
    for at in (s0,) + COPIES_AT:                                         # the flank before a locus: its own, alike in all rows
        F[:, at - FLANK:at] = random_msa(same, 12, FLANK, similar=1.0)
    pick = rng.integers(0, 12, ROWS)
    pick[:12] = np.arange(12)
    A = MS.copies(rng, F, pick, private=0.012)
    for at in (s0,) + COPIES_AT:                                         # no private substitutions in flank and stretch
        A[:, at - FLANK:at + CONSERVED] = F[pick][:, at - FLANK:at + CONSERVED]
    width = len(UNIT) * ARRAY_COPIES
    rep = [np.tile(np.frombuffer(UNIT * ARRAY_COPIES, dtype=np.uint8), (ROWS, 1)) for _ in range(2)]
    for r, x in ((5, 40), (20, 41), (21, 200), (ROWS - 1, 333)):          # the second array: a substitution in a few rows
        rep[1][r, x] = ord("A") if rep[1][r, x] != ord("A") else ord("C")
    a0, a1 = ARRAYS_AT
    A = np.hstack([A[:, :a0], rep[0], A[:, a0:a1], rep[1], A[:, a1:]])
    shift = lambda x: x + width * (x >= a0) + width * (x >= a1)      # noqa: E731
    loci = dict(segment=(shift(s0), shift(s0) + s1 - s0), array1=(a0, a0 + width), array2=(a1 + width, a1 + 2 * width))
    for name, at in zip(("copy1", "copy2"), COPIES_AT):
        loci[name] = (shift(at), shift(at) + s1 - s0)
    return A, loci, diverged


def with_n(G, r, a, ln, strand):
    """ln symbols of row r from offset a on with an N at every 13th, as test_mapping_scale.repeats_input makes them."""
    s = bytearray(G[r][a:a + ln])
    s[12::13] = b"N" * len(s[12::13])
    return (STM.revcomp(bytes(s), TABLE) if strand else bytes(s)), (r, a, ln, strand)


@functools.lru_cache(maxsize=None)
def duplications():
    """-> (A, reads, truth, kind): kind[R] is 'random', 'array1', 'array2', 'long' or 'short'."""
    A, loci, _ = duplications_msa()
    G = MS.stripped(A)
    rng = np.random.default_rng(47)
    reads, truth = MS.simulate(rng, A, N_RANDOM, every=75)
    kind = ["random"] * len(reads)
    at = lambda r, x: int((A[r, :x] != GAP).sum())      # noqa: E731          offset of column x in the text of row r

    def add(what, r, a, ln, strand):
        a = max(0, min(a, len(G[r]) - ln))
        s, t = with_n(G, r, a, ln, strand)
        reads.append(s)
        truth.append(t)
        kind.append(what)

    j = 0
    for name in ("array1", "array2"):
        x0, x1 = loci[name]
        for i in range(N_TANDEM):
            ln = int(rng.integers(300, 520)) if i % 2 else int(rng.integers(80, 200))       # spill tier; room beside it
            r = (5, 20, 21, ROWS - 1, 33, 48)[i % 6]
            # the long ones across an end of the array or inside it, the shorter ones inside: room for a second chain beside
            shift = int(rng.integers(-60, x1 - x0 - ln + 60)) if i % 2 else int(rng.integers(0, x1 - x0 - ln + 1))
            add(name, r, at(r, x0) + shift, ln, j % 2)
            j += 1
    for what, count, lo, hi in (("long", N_LONG, 150, 550), ("short", N_SHORT, 40, 100)):
        for i in range(count):
            x0, x1 = loci[("segment", "copy1", "copy2")[i % 3]]
            ln = int(rng.integers(400 if what == "long" and i % 5 else lo, hi + 1))      # four long reads in five: the spill tier
            r = int(rng.integers(0, ROWS))
            if what == "short":                                                      # well inside the conserved stretch
                first = int(rng.integers(x0 + 5, x0 + CONSERVED - 70 - ln + 1))
            else:
                first = int(rng.integers(x0 - 40, max(x1 + 40 - ln, x0 - 39)))       # column of the first symbol, about
            add(what, r, at(r, max(first, 0)), ln, j % 2)
            j += 1
    for i in range(N_DELETION):                  # 38 symbols, 30 left out, 38 more: the band keeps the pieces in two chains
        r = int(rng.integers(0, ROWS))
        a = at(r, (loci["segment"][1] + 4, loci["copy1"][1] + 4, loci["copy2"][1] + 4)[i % 3]) + 2 * (i // 3)
        s = bytearray(G[r][a:a + 38] + b"N" + G[r][a + 69:a + 107])
        s[12::13] = b"N" * len(s[12::13])
        reads.append(STM.revcomp(bytes(s), TABLE) if i % 2 else bytes(s))
        truth.append(None)
        kind.append("deletion")
    for r in range(0, ROWS, ROWS // N_INVERTED)[:N_INVERTED]:                # a piece and its reverse complement: one read, both strands
        piece = G[r][at(r, loci["array2"][1] + 20) + r // 4:][:30]
        reads.append(piece + STM.revcomp(piece, TABLE))
        truth.append(None)
        kind.append("inverted")
    return A, reads, truth, kind


def duplications_input():
    return duplications()[:3] + (HIGH,)


@functools.lru_cache(maxsize=None)
def cpu():
    c = MS.cpu("duplications", cap=CAP, band=BAND, source=duplications_input)
    c.kind = duplications()[3]
    c.lens = [len(r) for r in c.vreads]
    _, c.loci, c.diverged = duplications_msa()
    return c


# ---- the models ---------------------------------------------------------------------------------------------------------

CACHE = {}                                  # mapq_model's secondaries by (read, span, band, margin): one for every margin


def emptied(ch, min_score):
    """The chains ch with those below min_score empty: what a chaining call with that min_score reports."""
    keep = ch.score >= min_score
    ln = np.diff(ch.chain_off.astype(np.int64)) * keep
    of = np.repeat(keep, np.diff(ch.chain_off.astype(np.int64)))
    return SimpleNamespace(chain_off=np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64), score=ch.score,
                           anchor_place=ch.anchor_place[of], anchor_seed=ch.anchor_seed[of])


@functools.lru_cache(maxsize=None)
def primary(by_row, min_score):
    """The primary chains of the model: chain_model's, or byrow_model's for reads of up to BYROW_MAX start places."""
    if min_score:
        return emptied(primary(by_row, 0), min_score)
    c = cpu()
    return BM.by_row(c, BAND, 0, BYROW_MAX) if by_row else c


@functools.lru_cache(maxsize=None)
def model(margin, by_row=False, min_score=0):
    c, ch = cpu(), primary(by_row, min_score)
    return QM.solve(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, c.lens, ch.chain_off, ch.score, ch.anchor_place,
                    ch.anchor_seed, BAND, margin, True, CACHE)


def tiers(c):
    """(small, wave, spill): which virtual reads the chain kernels take in each tier, by their start places."""
    p = c.places_per_read
    return (p > 0) & (p <= MS.PC_SMALL), (p > MS.PC_SMALL) & (p <= MS.PC_LDS), p > MS.PC_LDS


def span_of(s, chain_off, place, seed, v):
    """(lo, hi) of the chain of virtual read v in the columns of the seeds s, None for an empty one."""
    o0, o1 = int(chain_off[v]), int(chain_off[v + 1])
    if o1 == o0:
        return None
    return int(s.start_col[place[o0]]), int(s.start_col[place[o1 - 1]]) + int(s.length[seed[o1 - 1]])


def check_truth(c, s, ch, margin):
    """Conditions (e) and (f) of the module's docstring on the chains ch (chain_off, anchor_place, anchor_seed, mapq,
    mapq_stranded) of a call with that margin, over the seeds s (seed_off, length, start_col) -> (reads judged, of these
    with mapq > 0).  c supplies what no call returns: the truth, the columns of the rows and the capped seeds."""
    n = len(c.reads)
    judged = positive = 0
    for R, t in enumerate(c.truth):
        if t is None:
            continue
        row, a, ln, strand = t
        v, w = strand * n + R, (1 - strand) * n + R
        if (c.count[int(s.seed_off[v]):int(s.seed_off[v + 1])] > c.cap).any():
            continue
        judged += 1
        if ch.mapq[v] > 0:
            positive += 1
            lo, hi = span_of(s, ch.chain_off, ch.anchor_place, ch.anchor_seed, v)
            t0, t1 = int(c.cols[row][a]), int(c.cols[row][a + ln - 1]) + 1
            assert lo - margin < t1 and t0 < hi + margin, (R, t, (lo, hi), (t0, t1), margin)
        assert not (ch.mapq_stranded[v] == 0 and ch.mapq_stranded[w] > 0), (R, t, margin)
    return judged, positive


def as_chains(c, m):
    """The model m with the primary chains of c: the fields check_truth reads of a Chains object."""
    return SimpleNamespace(chain_off=c.chain_off, anchor_place=c.anchor_place, anchor_seed=c.anchor_seed, mapq=m.mapq,
                           mapq_stranded=m.mapq_stranded)


def on_the_edge(c, margin):
    """(anchors with c + k + margin == lo, anchors with c == hi + margin) over the reads with a primary chain: the last
    anchors kept below and the first kept above the widened span.  The first copy lies 1320 columns after the segment, so
    at margin EDGE = 1320 - 12 a read's first seed at the segment ends where the widened span of its chain at the copy
    begins, and its last seed at the copy begins where the widened span of its chain at the segment ends."""
    read = np.repeat(np.arange(len(c.vreads)), np.diff(c.seed_off.astype(np.int64)))[c.seed_of_place]
    spans = [span_of(c, c.chain_off, c.anchor_place, c.anchor_seed, v) or (-1, -1) for v in range(len(c.vreads))]
    lo, hi = (np.array(x, dtype=np.int64)[read] for x in zip(*spans))
    col, k = c.start_col.astype(np.int64), c.length.astype(np.int64)[c.seed_of_place]
    has = (lo >= 0) & (c.start_col != NONE)
    return int((has & (col + k + margin == lo)).sum()), int((has & (col == hi + margin)).sum())


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_input_is_what_it_claims():
    """(a) to (d) of the docstring, on the models alone."""
    c, m = cpu(), model(0)
    A = c.A
    n = len(c.reads)
    assert A.shape == (ROWS, BASE + 2 * len(UNIT) * ARRAY_COPIES) and BAND < len(UNIT)
    x0, x1 = c.loci["segment"]
    for name, share in zip(("copy1", "copy2"), DIVERGED):
        y0, y1 = c.loci[name]
        differs = (A[:, x0:x1] != A[:, y0:y1]).mean(axis=0) > 0.5             # in every row but for gaps and private symbols
        assert differs.sum() == len(c.diverged[name]) == round(share * (x1 - x0)) and (np.flatnonzero(differs) == c.diverged[name]).all()
    loci = sorted(c.loci.values())
    assert all(b[0] - a[1] >= 100 for a, b in zip(loci, loci[1:]))
    for name in ("array1", "array2"):
        y0, y1 = c.loci[name]
        assert (A[0, y0:y1].tobytes() == UNIT * ARRAY_COPIES) and ((A[:, y0:y1] != A[0, y0:y1]).sum() == 0) == (name == "array1")
    assert MS.oracle_boundaries(A) == c.b
    # (c) the sizes, and reads without seeds between reads that have seeds and places
    seeds, places = np.diff(c.seed_off.astype(np.int64)), c.places_per_read
    assert len(c.vreads) > 1500 and len(c.start_col) > 100000
    between = (seeds[1:-1] == 0) & (places[:-2] > 0) & (places[2:] > 0)
    assert between.sum() > 50 and (seeds == 0).sum() > n // 4 and (c.start_total > CAP).sum() > 1000 and (c.start_total <= CAP).sum() > 1000
    assert sum(len(r) == 0 for r in c.reads) >= 2 and sum(len(r) > 0 and set(r) == {ord("N")} for r in c.reads) >= 2
    st = m.stats
    share = st["anchors_kept"] / (st["anchors_kept"] + st["anchors_excluded"])
    assert 0.2 <= share <= 0.8, st
    # (a) secondaries of several anchors in every tier
    sl = np.diff(m.second_off.astype(np.int64))
    got = [int((t & (sl >= need)).sum()) for t, need in zip(tiers(c), (3, 8, 8))]
    assert min(got) >= 40, got
    assert MS.model_chain_stats(c) == dict(anchors=int((c.start_col != NONE).sum()), reads_small=int(tiers(c)[0].sum()),
                                           reads_wave=int(tiers(c)[1].sum()), reads_spill=int(tiers(c)[2].sum()))
    # (b) the classes of the quality
    prim = np.diff(c.chain_off.astype(np.int64)) > 0
    equal = prim & (m.mapq == 0) & (m.second == c.score)
    less = prim & (m.second > 0) & (m.second < c.score)
    sure = prim & (m.mapq == 60)
    below = prim & (m.mapq_stranded < m.mapq)
    classes = [int(x.sum()) for x in (equal, less, sure, below)]
    assert min(classes[:3]) >= 100 and classes[3] >= 20, classes
    assert (m.second <= c.score).all() and not m.second[~prim].any()
    # (d) the margin matters
    m50 = model(50)
    differ = sum(tuple(m.second_place[int(m.second_off[v]):int(m.second_off[v + 1])]) !=
                 tuple(m50.second_place[int(m50.second_off[v]):int(m50.second_off[v + 1])]) for v in range(2 * n))
    assert differ >= 10, differ
    # a margin at which many anchors lie on either end of the widened span, where margins 0 and 50 have next to none
    assert min(on_the_edge(c, EDGE)) >= 20, on_the_edge(c, EDGE)
    print("anchors on the edge (below, above) at margins 0, 50, EDGE:", [on_the_edge(c, x) for x in MARGINS + (EDGE,)])
    # margins that exclude everything; a min_score that empties a share of the primary chains
    for margin in (A.shape[1], U64):
        assert not model(margin).second.any() and model(margin).stats["anchors_kept"] == 0
    high = primary(False, HIGH)
    gone = prim & (np.diff(high.chain_off.astype(np.int64)) == 0)
    assert 100 < gone.sum() < prim.sum() - 100
    print("duplications:", dict(reads=n, seeds=len(c.q_start), places=len(c.start_col), stats=st, with_anchors=got, longest=int(sl.max()),
                                classes=classes, differ=differ, emptied_by_high=int(gone.sum())))


def test_by_row_chains_are_another_primary():
    """The by-row chains differ from the plain ones on this input, reads of more than BYROW_MAX places come out empty, and
    some secondaries then beat the chain of the chosen row."""
    c, b, m = cpu(), primary(True, 0), model(0, by_row=True)
    many = c.places_per_read > BYROW_MAX
    assert b.too_many == many.sum() > tiers(c)[2].sum() > 0 and not b.score[many].any() and (b.score > 0).sum() > 500
    lower = int(((b.score < c.score) & (b.score > 0)).sum())
    above = int((m.second > b.score).sum())
    assert lower > 0 and above > 0 and not m.mapq[m.second > b.score].any()
    print("by row:", dict(chained=int((b.score > 0).sum()), too_many=b.too_many, below_the_plain_score=lower, second_above_score=above))


@pytest.mark.parametrize("margin", MARGINS)
def test_models_agree_with_the_truth(margin):
    """(e) and (f) on the models; recorded: the histogram of mapq and the exact repeats that get quality 0."""
    c, m = cpu(), model(margin)
    n = len(c.reads)
    judged, positive = check_truth(c, c, as_chains(c, m), margin)
    assert judged > 300 and positive > 200, (judged, positive)
    true = [t[3] * n + R for R, t in enumerate(c.truth) if t is not None]
    hist = np.bincount(m.mapq[true] // 10, minlength=7).tolist()
    # reads cut inside the segment or its first copy from columns in which that copy has not diverged: one text, two loci
    lost = set(c.diverged["copy1"].tolist())
    exact = zero = 0
    for R, t in enumerate(c.truth):
        if t is None:
            continue
        row, a, ln, strand = t
        t0, t1 = int(c.cols[row][a]), int(c.cols[row][a + ln - 1]) + 1
        for x0, x1 in (c.loci["segment"], c.loci["copy1"]):
            if x0 <= t0 and t1 <= x1 and not lost & set(range(t0 - x0, t1 - x0)):
                exact += 1
                zero += int(m.mapq[strand * n + R] == 0)
    print("margin", margin, dict(judged=judged, positive=positive, mapq_by_tens=hist, exact=exact, exact_with_mapq0=zero))


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def seeded(pix, c):
    """The stranded seeds call of the input with a plain chaining call; the seeds, places and chains are the models'."""
    sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=CAP, msa=True, chain=True, band=BAND, strands=True, rows=True)
    assert sd.strands and sd.reads == len(c.reads)
    TR.same_as_cpu(sd, c, "duplications")
    assert np.array_equal(sd.occ.start_total, c.start_total)
    return sd


def check(pix, ch, m, c, what):
    """Every array of a mapq call against the model m, and the statistics."""
    TQ.same(ch, m, what)
    assert ch.mapq_stranded.dtype == np.uint8 and np.array_equal(ch.mapq_stranded, m.mapq_stranded), what
    n = len(c.reads)
    want = [0 if s == STM.NONE else int(m.mapq_stranded[s * n + R]) for R, s in enumerate(ch.strand.tolist())]
    assert ch.best_mapq.dtype == np.uint8 and ch.best_mapq.tolist() == want, what
    assert pix.mapq_stats() == m.stats, (what, pix.mapq_stats(), m.stats)
    empty = np.diff(ch.chain_off.astype(np.int64)) == 0
    assert not ch.second_score[empty].any() and not ch.mapq[empty].any() and (ch.second_lo[empty] == NONE).all(), what


def margins(c):
    return MARGINS + (c.A.shape[1], U64)


def build(engine, c):
    assert MS.engine_boundaries(engine, c.A) == c.b                   # the engine's segmentation is the oracle's
    return TR.build(engine, c.A, c.b)


@pytest.mark.gpu
def test_parity_after_the_plain_call(engine):
    c = cpu()
    tier_counts = MS.model_chain_stats(c)
    with build(engine, c) as pix:
        seeded(pix, c)
        for min_score in (0, HIGH):
            want = primary(False, min_score)
            for margin in margins(c) + ((EDGE,) if min_score == 0 else ()):
                ch = pix.chains(band=BAND, min_score=min_score, mapq=True, mapq_margin=margin)
                for f in TR.CHAIN_FIELDS:
                    assert np.array_equal(getattr(ch, f), getattr(want, f)), (min_score, margin, f)
                check(pix, ch, model(margin, False, min_score), c, (min_score, margin))
                assert (ch.second_score <= ch.score).all()
                st = pix.chain_stats()
                assert {k: st[k] for k in tier_counts} == tier_counts and (st["small_max"], st["lds_max"]) == (MS.PC_SMALL, MS.PC_LDS)
                if margin in (c.A.shape[1], U64):
                    assert not ch.second_score.any() and ch.second_off[-1] == 0 and pix.mapq_stats()["anchors_kept"] == 0
        # an empty primary chain: no secondary, quality 0, whatever the read's anchors would chain to
        gone = (np.diff(c.chain_off.astype(np.int64)) > 0) & (np.diff(ch.chain_off.astype(np.int64)) == 0)
        assert gone.sum() > 100 and not ch.mapq_stranded[gone].any()
        # through seeds(chain=True, mapq=True): the same object
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=CAP, msa=True, chain=True, band=BAND, strands=True, mapq=True, mapq_margin=50)
        check(pix, sd.chains, model(50), c, "seeds")


@pytest.mark.gpu
def test_parity_after_the_by_row_call(engine):
    c, want = cpu(), primary(True, 0)
    above = 0
    with fbg_options(engine, {"byrow_max": BYROW_MAX}), build(engine, c) as pix:
        seeded(pix, c)
        for min_score in (0, HIGH):
            for margin in margins(c):
                ch = pix.chains(band=BAND, min_score=min_score, by_row=True, mapq=True, mapq_margin=margin)
                if min_score == 0:
                    TB.same(TB.of_chains(ch), want, margin)
                    TB.check_stats(pix, want)
                check(pix, ch, model(margin, True, min_score), c, ("by row", min_score, margin))
                assert not ch.mapq[ch.second_score > ch.score].any()
                above = max(above, int((ch.second_score > ch.score).sum()))
    assert above > 0                                                  # test_by_row_chains_are_another_primary has the count


@pytest.mark.gpu
def test_truth_on_what_the_engine_returns(engine):
    c = cpu()
    with build(engine, c) as pix:
        sd = seeded(pix, c)
        s = SimpleNamespace(seed_off=sd.seed_off, length=sd.length, start_col=sd.occ.start_col)
        for margin in MARGINS:
            ch = pix.chains(band=BAND, mapq=True, mapq_margin=margin)
            judged, positive = check_truth(c, s, ch, margin)
            assert judged > 300 and positive > 200, (margin, judged, positive)


def per_read(sd, v):
    """What must not depend on the batch a virtual read is in: scores, spans, qualities, and the anchors of both chains
    counted from the read's first start place and first seed."""
    ch = sd.chains
    base = np.array([int(sd.occ.start_off[int(sd.seed_off[v])]), int(sd.seed_off[v])])
    return ((int(ch.score[v]), int(ch.second_score[v]), int(ch.second_lo[v]), int(ch.second_hi[v]), int(ch.mapq[v]),
             int(ch.mapq_stranded[v])), (ch.of(v) - base).tolist(), (ch.second(v) - base).tolist())


def same_reads(part, whole, first, count, n, what):
    """The `count` given reads of the call `part` are reads first .. first + count of the call `whole` of n given reads."""
    assert part.reads == count and whole.reads == n
    for j in range(count):
        for strand in (0, 1):
            assert per_read(part, strand * count + j) == per_read(whole, strand * n + first + j), (what, first + j, strand)
        assert part.chains.best_mapq[j] == whole.chains.best_mapq[first + j] and part.chains.strand[j] == whole.chains.strand[first + j]


def mapq_call(pix, c, reads, margin):
    return pix.seeds(reads, min_length=c.L, max_per_seed=CAP, msa=True, chain=True, band=BAND, strands=True, mapq=True, mapq_margin=margin)


@pytest.mark.gpu
def test_a_read_is_independent_of_its_batch(engine):
    c, m = cpu(), model(50)
    n = len(c.reads)
    cuts = [0, 97, 97 + 610, n]                                       # three batches of unequal size
    sl = np.diff(m.second_off.astype(np.int64))
    alone = []                                                        # two reads of every tier with a secondary, then two more
    for t, need in zip(tiers(c), (3, 8, 8)):
        alone += (np.flatnonzero(t & (sl >= need)) % n).tolist()[:2]
    alone += [R for R in (np.flatnonzero(tiers(c)[1] & (sl >= 8)) % n).tolist() if R not in alone][-2:]
    assert len(set(alone)) == 8
    with build(engine, c) as pix:
        parts = [mapq_call(pix, c, c.reads[a:b], 50) for a, b in zip(cuts, cuts[1:])]
        singles = [mapq_call(pix, c, [c.reads[R]], 50) for R in alone]
        whole = mapq_call(pix, c, c.reads, 50)
        check(pix, whole.chains, m, c, "whole")
        for part, a, b in zip(parts, cuts, cuts[1:]):
            same_reads(part, whole, a, b - a, n, "batch")
        for one, R in zip(singles, alone):
            same_reads(one, whole, R, 1, n, "alone")
        st = pix.chain_stats()
        assert min(st["reads_small"], st["reads_wave"], st["reads_spill"]) > 0


@pytest.mark.gpu
def test_one_index_across_the_large_batch_and_a_small_one(engine):
    """The large batch, three reads, the large batch with another margin: the chain buffers of the mapq state are sized by
    the large call, hold three reads' worth, and are filled again.  Nothing of an earlier call may show."""
    c = cpu()
    n = len(c.reads)
    three = [int(np.flatnonzero(t & (model(0).second > 0))[0]) % n for t in tiers(c)]
    with build(engine, c) as pix:
        first = mapq_call(pix, c, c.reads, 0)
        check(pix, first.chains, model(0), c, "first")
        small = mapq_call(pix, c, [c.reads[R] for R in three], 0)
        for j, R in enumerate(three):
            for strand in (0, 1):
                assert per_read(small, strand * 3 + j) == per_read(first, strand * n + R), (R, strand)
        st = pix.mapq_stats()
        assert st["reads_with_second"] == sum(int(small.chains.second_score[v] > 0) for v in range(6)) >= 3
        again = mapq_call(pix, c, c.reads, 50)
        check(pix, again.chains, model(50), c, "again")
        assert not np.array_equal(again.chains.second_place, first.chains.second_place)
