"""Paired reads at scale (fbg_pindex_chains_pairs; k_pp_span, k_pp_mask, k_pp_pick, k_pp_adopt_read, k_pp_adopt_pred of
csrc/pindex_pairs.hip and the chain kernels in the pairs state's own chain state) on one seeded input with duplicated loci,
hundreds of workgroups of start places and a ground truth outside the model, between the toy inputs of test_pairs.py and a
workload.  The checker is tests/pairs_model.py on the seeds, places and primary chains of test_mapping_scale.cpu(); every
call is stranded with min_length 12, max_per_seed 64 and band 8, as in test_mapq_scale.py, whose MSA this is
(duplications_msa(): 50 rows x 3460 columns, a 600-column segment with two diverged copies, a private flank before each of
the three loci, two tandem arrays).  Every GPU comparison is exact.

The input: 744 interleaved pairs (12 workgroups of k_pp_span over 2976 virtual reads, 3 of k_pp_pick with a last wave of 40
lanes), 7134 seeds, 158 473 start places (620 workgroups of k_pp_mask).  A fragment is (row, first symbol, extent): mate 1
its first symbols, mate 2 the reverse complement of its last ones, the mates given in either order (every second couple of
a group the other way round).  A mate carries an N at every 13th symbol and 0 to 2 substitutions; one short mate in four has
no N in its second half, so that the seeds of a chain differ in length (without these every seed had 12 symbols, and a hi
made from the first seed's length went unnoticed).  The groups:
  ordinary 340   fragments of 150 .. 400 symbols anywhere (one in an array is drawn once more), mates of 50 .. 90;
  flank 40, exact 80   the forward mate in the private flank of a locus, the reverse one in its conserved stretch, between
                 two diverged columns of the first copy (TIE): segment and first copy have one text there, and the primary
                 of that mate lies at another copy for 41 of the 120.  The exact ones have 51-symbol mates without
                 substitutions on fragments of EXACT = 240 columns (40) and of 241 (40): their end seeds lie on the ends;
  reverse 140    the forward mate in the conserved stretch (TIE), the reverse one in the diverse part of the locus: the
                 reverse mate's primary is right and the forward one needs the rescue (candidates 1 and 3);
  long 16, array 8   mates of 400 .. 519 symbols on fragments of up to 700, in the loci and across the arrays: the spill tier;
  over 60        fragments 13 or more symbols longer than max_insert: the window's end cuts the far mate, the chosen
                 candidate takes the shortened rescue chain (rescue_differs);
  first 16       fragments that begin in columns 0 .. 11;
  nocol 30       ordinary, one mate ending in a piece across the separator of two edge strings: a seed whose place has no
                 witness column (gapped columns do not make such a place; a pattern across '#' does, as in test_chains.py);
  degenerate 14  after every 49 others, between ordinary pairs: an empty mate, an all-N mate, a mate inside the first array
                 (every seed of it keeps 64 of more than a thousand places: the cap takes places, never the last one of a
                 reported seed), two identical mates, a mate and its own reverse complement.  Two long pairs follow each.

What test_input_is_what_it_claims asserts of the model at NATURAL = (100, 720) unless said, measured (floor):
  virtual reads with 3 or more seeds 1299 (600); rescue chains whose first and last seed differ in length 226 (100);
  which0 .. which3 and none: 307, 46, 309, 42, 40 (150 for 0 and 2, 20 for the others); rescue_differs 71 (35);
  flank pairs whose conserved mate's primary lies at another copy 41 (20);
  reads by tier: 735 small, 740 wave, 21 spill (10 each); reads whose rescue run has kept and excluded places: 702 wave
  (300), 21 spill (10); adopted rescue chains of the spill tier 13 (5);
  windows clamped at 0: 230 (100); fragments from the first 12 columns that end before column 720: 16;
  anchors on the edges (c == W.lo kept, c == W.lo - 1, c + k == W.hi kept, c + k == W.hi + 1): 153, 171, 191, 127 at NATURAL,
  and 307, 224, 491, 340 (100 each) at ABUT = (240, 240), where the exact group abuts by construction: a fragment of 240
  gap-free columns has its last seed end at lo(F) + 240 and its first begin at hi(R) - 240, one of 241 lies one column out;
  all 40 fragments of 240 columns are proper there and none of 241;
  places without a column 209 (90), counted neither as kept nor as excluded: kept 73 126 + excluded 85 138 + 209 = all;
  reads without seeds between reads with places 716 (300); pairs where two valid candidates tie at the best score and the
  smaller number wins 532 (250); winners other than candidate 0: 397 (190);
  HIGH = 48 empties 514 of 1496 primary chains (250 .. all but 250), 248 of them in pairs then without a candidate (100);
  NARROW = (260, 720) leaves 376 proper pairs of 704 with the same windows (30 % .. 70 %): the insert condition alone.
By row (byrow_max 512): 1442 reads chained along a row, 44 with more places come out empty; rescue_differs 190.

The ground truth (test_model_finds_the_fragments, and test_truth_on_what_the_engine_returns on the engine's arrays): of 730 simulated pairs 656 are
judged: [t_lo, t_hi) meets the fragment's columns.  Excused, 74 (10 %, at most 20 %): 47 where the cap took a mate's true
place (a seed of more than 64 places and no seed with a place at its true column: all of them touch an array; the rule
"no capped seed" of test_mapq_scale would excuse 380, since seeds inside nodes of many edges pass 64 places), 11 without a
candidate, 16 whose text stands at another copy or array as well and that were found there (checked: the interval meets
the same columns of that copy).  194 chosen candidates use a rescue chain in other columns than that read's primary (90).

Which GPU tests fail for an error in pindex_pairs.hip (each tried once on a scratch build, never committed; "all six" are
both parity cases, every stage, the batches, the one index and the tool; the truth test is too coarse for any of them):
  `>` for `>=` at W.lo in k_pp_mask: all six (a pair becomes proper: none 39 for 40); `<` for `<=` at W.hi: all six;
  the clamp at 0 replaced by hi - min(hi, max_insert) + 1: all six; `>=` for `>` in the score comparison of k_pp_pick: all
  six (which 1 for 0, 3 for 2); hi(F) <= hi(R) dropped: all six; the counters added by wave 0 of a workgroup only: both
  parity cases, every stage, the batches and the one index (none 8 for 40, places_kept 18 068 for 73 126; the tool prints no
  counters); PP_TWIN leaving the score: all six (score of the adopted chains; the twins' score 0 in test_every_stage_on_adopted_chains); the PP_KEEP
  branch removed: both parity cases, at min_score HIGH with adopt (the emptied chains come back); k_pp_span taking k of the
  chain's first seed: all six, none before the mates without N in their second half were added.

Time: the CPU tests 17 s, the models of all parity runs 16 s and of the stages on the adopted chains 9 s more, once per
process."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import byrow_model as BM  # noqa: E402
import cigar_model as CG  # noqa: E402
import graph_align_model as GM  # noqa: E402
import graph_cigar_model as JM  # noqa: E402
import heuristic_model as HM  # noqa: E402
import mapq_model as QM  # noqa: E402
import pairs_model as PM  # noqa: E402
import rows_model as RM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
import test_mapping_scale as MS  # noqa: E402
import test_mapq_scale as QS  # noqa: E402
import test_pairs as TP  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options  # noqa: E402

GAP, NONE, U64, TABLE = MS.GAP, QM.NONE, QM.U64_MAX, MS.TABLE
CAP, BAND, BYROW_MAX = QS.CAP, QS.BAND, QS.BYROW_MAX
FLANK, CONSERVED = QS.FLANK, QS.CONSERVED
LOCI = ("segment", "copy1", "copy2")
N_ORDINARY, N_FLANK, N_EXACT, N_REVERSE, N_LONG, N_ARRAY, N_FIRST, N_NOCOL, N_OVER = 340, 120, 80, 140, 16, 8, 16, 30, 60
EVERY = 50                                  # a degenerate pair after every EVERY - 1 others
EXACT = 240                                 # columns of the planted group of fragments: half of N_EXACT; the other half has one more
SHORT, LONG_MATE, LONGEST = (150, 400), (400, 520), 700       # symbols of a fragment, of a long mate, of the longest fragment
TIE = (74, 147)                             # columns of the conserved stretch between two diverged columns of the first copy: one text, two loci
HIGH = 48                                   # a min_score that empties a share of the primary chains
# the insert bounds of the parity runs, and what each is for
NATURAL = (100, 720)                        # the fragments: 150 .. 700 symbols, a few columns more across gaps, less what the ends do not seed
NARROW = (260, 720)                         # rejects the shorter half of the ordinary fragments on the insert condition alone
ABUT = (EXACT, EXACT)                       # min_insert == max_insert: the planted group; its anchors lie on the window's edges
INSERTS = (NATURAL, NARROW, ABUT, (0, U64), (0, 0))        # (0, 2^64 - 1): the saturated window end; (0, 0): no window holds a seed


# ---- the input ----------------------------------------------------------------------------------------------------------

def rc(s):
    return STM.revcomp(bytes(s), TABLE)


def mate(rng, text, rev, subs, tail=False):
    """`text` (its reverse complement if rev) with an N at every 13th symbol and `subs` substitutions elsewhere.  tail: no
    N in the second half, so that the mate ends in one longer seed and the seeds of a chain differ in length."""
    s = bytearray(rc(text) if rev else text)
    stop = 13 * (len(s) // 26) if tail else len(s)
    s[12:stop:13] = b"N" * len(s[12:stop:13])
    for _ in range(subs):
        at = int(rng.integers(0, len(s)))
        if s[at] != ord("N"):
            s[at] = rng.choice([x for x in b"ACGT" if x != s[at]])
    return bytes(s)


@functools.lru_cache(maxsize=None)
def fragments():
    """-> (A, reads, truth, frag, kind): reads 2p and 2p + 1 are the mates of pair p, truth[R] = (row, offset, length, strand)
    of a simulated mate in the gap-stripped row, frag[p] = (row, first symbol, extent in symbols) or None for a degenerate
    pair, kind[p] its group."""
    A, loci, _ = QS.duplications_msa()
    G = MS.stripped(A)
    rng = np.random.default_rng(61)
    at = lambda r, x: int((A[r, :x] != GAP).sum())      # noqa: E731          offset of column x in the text of row r
    labels, edges, _ = HM.segmentation_graph(A, MS.oracle_boundaries(A))
    S = [labels[u] + labels[v] for u, v in edges]
    specs = []                                                        # (kind, row, first symbol, extent, l1, l2, most substitutions, flip)

    def add(kind, i, r, a, f, l1, l2, subs=2):
        a = max(0, min(a, len(G[r]) - f))
        specs.append((kind, r, a, f, min(l1, f), min(l2, f), subs, (i // 2) % 2))

    short = lambda: int(rng.integers(50, 91))      # noqa: E731
    for i in range(N_ORDINARY + N_NOCOL):
        r, f = int(rng.integers(0, len(G))), int(rng.integers(SHORT[0], SHORT[1] + 1))
        a = int(rng.integers(0, len(G[r]) - f + 1))
        if any(a < y1 and y0 < a + f for y0, y1 in (loci["array1"], loci["array2"])):      # in an array: once more, so that fewer are
            a = int(rng.integers(0, len(G[r]) - f + 1))
        add("ordinary" if i < N_ORDINARY else "nocol", i, r, a, f, short(), short())
    for i in range(N_FLANK):                      # the forward mate in the private flank, the reverse one in the conserved stretch
        x0 = loci[LOCI[i % 3]][0]
        r = int(rng.integers(0, len(G)))
        if i < N_EXACT:                           # EXACT columns, or one more; no substitutions: the end seeds lie on the fragment's ends
            f, l1, l2, s = EXACT + i % 2, 51, 51, int(rng.integers(0, TIE[1] - (EXACT + 1 - FLANK) + 1))
        else:
            l1, l2 = int(rng.integers(40, 61)), int(rng.integers(40, 61))
            s = int(rng.integers(0, FLANK - l1 + 1))
            f = FLANK - s + int(rng.integers(TIE[0] + l2, TIE[1] + 1))
        add("exact" if i < N_EXACT else "flank", i, r, at(r, x0 - FLANK + s), f, l1, l2, 0 if i < N_EXACT else 2)
    for i in range(N_REVERSE):                    # the forward mate in the conserved stretch, the reverse one in the diverse part
        x0, x1 = loci[LOCI[i % 3]]
        r, l1, l2 = int(rng.integers(0, len(G))), int(rng.integers(40, 61)), short()
        s = int(rng.integers(TIE[0], TIE[1] - l1 + 1))
        e = int(rng.integers(CONSERVED + l2, min(s + SHORT[1], x1 - x0) + 1))
        add("reverse", i, r, at(r, x0 + s), at(r, x0 + e) - at(r, x0 + s), l1, l2)
    for i in range(N_LONG + N_ARRAY):             # long mates in the loci and across the arrays
        r, l1, l2 = int(rng.integers(0, len(G))), int(rng.integers(*LONG_MATE)), int(rng.integers(*LONG_MATE))
        f = int(rng.integers(max(l1, l2) + 40, LONGEST + 1))
        if i < N_LONG:
            x0, x1 = loci[LOCI[i % 3]]
            first = int(rng.integers(x0 - 60, max(x1 + 60 - f, x0 - 59)))
        else:
            y0, y1 = loci[("array1", "array2")[i % 2]]
            first = int(rng.integers(y0 - 150, y1 + 150 - f + 1))
        add("long" if i < N_LONG else "array", i, r, at(r, max(first, 0)), f, l1, l2)
    for i in range(N_OVER):                       # a few dozen symbols longer than max_insert: the window's end cuts the far mate
        r, l1, l2 = int(rng.integers(0, len(G))), short(), short()
        f = NATURAL[1] + int(rng.integers(13, min(l1, l2) - 12))
        a = int(rng.integers(0, len(G[r]) - f + 1))
        while any(a < y1 + 20 and y0 - 20 < a + f for y0, y1 in (loci["array1"], loci["array2"])):      # beside the arrays
            a = int(rng.integers(0, len(G[r]) - f + 1))
        add("over", i, r, a, f, l1, l2)
    for i in range(N_FIRST):                      # fragments that begin in the first columns: the clamp at 0
        add("first", i, int(rng.integers(0, len(G))), i % 12, int(rng.integers(SHORT[0], SHORT[1] + 1)), short(), short())
    # the order: the long pairs two by two behind a degenerate pair, everything else shuffled
    longs = [s for s in specs if s[0] in ("long", "array")]
    rest = [s for s in specs if s[0] not in ("long", "array")]
    rest = [rest[j] for j in rng.permutation(len(rest)).tolist()]
    reads, truth, frag, kind = [], [], [], []

    def simulated(spec):
        what, r, a, f, l1, l2, subs, flip = spec
        t1, t2 = G[r][a:a + l1], G[r][a + f - l2:a + f]
        tails = [what not in ("exact", "long", "array") and int(rng.integers(0, 4)) == 0 for _ in range(2)]      # one short mate in four
        m1 = mate(rng, t1, 0, int(rng.integers(0, subs + 1)), tails[0])
        m2 = mate(rng, t2, 1, int(rng.integers(0, subs + 1)), tails[1])
        if what == "nocol":                       # a piece across the separator of two edge strings: a seed whose place has no column
            e = int(rng.integers(0, len(S) - 1))
            m1 = m1 + b"N" + S[e + 1][-6:] + b"#" + S[e][:6]
        two = [(m1, (r, a, l1, 0)), (m2, (r, a + f - l2, l2, 1))]
        return two[::-1] if flip else two

    def put(two, f, what):
        for s, t in two:
            reads.append(s)
            truth.append(t)
        frag.append(f)
        kind.append(what)

    d = 0
    while rest or longs:
        if len(frag) % EVERY == EVERY - 1:
            (x, tx), (y, ty) = simulated(rest[d % len(rest)])     # an ordinary pair's mates, used again
            a1 = loci["array1"][0]
            two = [[(b"", None), (y, ty)], [(x, tx), (b"N" * 30, None)], [(mate(rng, G[7][at(7, a1) + 20 + d:][:64], 0, 0), None), (y, ty)],
                   [(x, tx), (x, tx)], [(x, tx), (rc(x), None)]][d % 5]
            put(two, None, ("empty", "all_n", "capped", "identical", "own_rc")[d % 5])
            d += 1
            for s in longs[:2]:
                put(simulated(s), s[1:4], s[0])
            longs = longs[2:]
        elif rest:
            s = rest.pop()
            put(simulated(s), s[1:4], s[0])
        else:
            s = longs.pop()
            put(simulated(s), s[1:4], s[0])
    return A, reads, truth, frag, kind


def pairs_input():
    return fragments()[:3] + (HIGH,)


@functools.lru_cache(maxsize=None)
def cpu():
    c = MS.cpu("pairs", cap=CAP, band=BAND, source=pairs_input)
    _, _, _, c.frag, c.kind = fragments()
    c.lens = [len(r) for r in c.vreads]
    c.loci = QS.duplications_msa()[1]
    return c


# ---- the models ---------------------------------------------------------------------------------------------------------

CACHE = {}                                  # pairs_model's anchors by virtual read


@functools.lru_cache(maxsize=None)
def primary(by_row=False, min_score=0):
    """The primary chains of the model: chain_model's, or byrow_model's for reads of up to BYROW_MAX start places."""
    if min_score:
        return QS.emptied(primary(by_row, 0), min_score)
    c = cpu()
    return BM.by_row(c, BAND, 0, BYROW_MAX) if by_row else c


@functools.lru_cache(maxsize=None)
def model(ins=NATURAL, by_row=False, min_score=0):
    c, ch = cpu(), primary(by_row, min_score)
    return PM.solve(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, ch.chain_off, ch.score, ch.anchor_place, ch.anchor_seed,
                    BAND, ins[0], ins[1], CACHE)


def spans(c, ch):
    """(lo, hi) per virtual read of the chains ch over the seeds of c, None for an empty chain."""
    return [QS.span_of(c, ch.chain_off, ch.anchor_place, ch.anchor_seed, v) for v in range(len(ch.chain_off) - 1)]


def windows(c, ch, max_insert):
    """Per virtual read w the window that the primary chain of partner(w) opens, None where that chain is empty."""
    n = len(c.reads)
    sp = spans(c, ch)
    return [PM.window_of(sp[PM.partner(w, n)], PM.partner(w, n) < n, max_insert) for w in range(2 * n)]


def on_the_edges(c, ch, max_insert):
    """Anchors with c == W.lo kept, c == W.lo - 1 (dropped), c + k == W.hi kept and c + k == W.hi + 1 (dropped), as `seen`
    counts reads in test_pairs.test_model_agrees_with_brute_force; then the windows whose lower end is clamped at 0."""
    n = len(c.reads)
    W = windows(c, ch, max_insert)
    sp = spans(c, ch)
    read = np.repeat(np.arange(2 * n), np.diff(c.seed_off.astype(np.int64)))[c.seed_of_place]
    open_ = np.array([w is not None for w in W])[read] & (c.start_col != NONE)
    lo = np.array([w[0] if w else 0 for w in W], dtype=np.int64)[read]
    hi = np.array([min(w[1], 1 << 62) if w else 0 for w in W], dtype=np.int64)[read]          # above every c + k
    col = c.start_col.astype(np.int64)
    end = col + c.length[c.seed_of_place].astype(np.int64)
    kept = open_ & (col >= lo) & (end <= hi)
    clamp = sum(1 for w in range(2 * n) if W[w] is not None and PM.partner(w, n) >= n and sp[PM.partner(w, n)][1] < max_insert < U64)
    return dict(lo_kept=int((kept & (col == lo)).sum()), lo_dropped=int((open_ & (col + 1 == lo)).sum()),
                hi_kept=int((kept & (end == hi)).sum()), hi_dropped=int((open_ & (end == hi + 1)).sum()), clamp=clamp)


def candidates(c, ch, m, p, ins):
    """[(valid, score)] of the four candidates of pair p: primary chains ch, rescue chains of the model or call m."""
    n = len(c.reads)
    out = []
    for f, r, fr, rr in PM.candidates(p, n):
        rs = lambda v: None if m.rescue_lo[v] == NONE else (int(m.rescue_lo[v]), int(m.rescue_hi[v]))      # noqa: E731
        ps = lambda v: QS.span_of(c, ch.chain_off, ch.anchor_place, ch.anchor_seed, v)      # noqa: E731
        sf, sr = (rs(f) if fr else ps(f)), (rs(r) if rr else ps(r))
        score = int(m.rescue_score[f] if fr else ch.score[f]) + int(m.rescue_score[r] if rr else ch.score[r])
        out.append((PM.valid(sf, sr, *ins), score))
    return out


def true_columns(c, p):
    row, a, f = c.frag[p]
    return int(c.cols[row][a]), int(c.cols[row][a + f - 1]) + 1


def cut_away(c, s, R):
    """The cap took the true place of given read R: a seed on the strand it was cut from has more than CAP start places, and
    none of its seeds has a start place at the column that seed was cut from.  s: seed_off, q_start, start_off, start_col and
    start_total of the model or of the engine."""
    row, a, ln, strand = c.truth[R]
    v = strand * len(c.reads) + R
    t0, t1 = int(s.seed_off[v]), int(s.seed_off[v + 1])
    if not (s.start_total[t0:t1] > c.cap).any():
        return False
    for t in range(t0, t1):
        q = int(s.q_start[t])
        if q < ln and (s.start_col[int(s.start_off[t]):int(s.start_off[t + 1])] == c.cols[row][a + q]).any():
            return False
    return True


def elsewhere(c, p):
    """Where else the text of pair p stands: the same columns of the other loci for a fragment with fewer than a seed's
    symbols outside its locus, both arrays for a pair whose mates both touch an array (one unit, sixty periods)."""
    t0, t1 = true_columns(c, p)
    out = []
    for x0, x1 in map(c.loci.get, LOCI):
        if x0 - MS.MIN_LENGTH < t0 and t1 < x1 + MS.MIN_LENGTH:
            out += [(t0 - x0 + y0, t1 - x0 + y0) for y0, _ in map(c.loci.get, LOCI) if y0 != x0]
    arrays = [c.loci["array1"], c.loci["array2"]]
    ends = [(int(c.cols[r][a]), int(c.cols[r][a + ln - 1]) + 1) for r, a, ln, _ in c.truth[2 * p:2 * p + 2]]
    if all(any(lo < y1 and y0 < hi for y0, y1 in arrays) for lo, hi in ends):
        out += arrays
    return out


def check_truth(c, s, m, ch):
    """The ground truth: for every simulated pair none of whose mates has a capped seed on its true strand and that got a
    candidate, [t_lo, t_hi) meets the fragment's columns.  s: the seeds (seed_off), m: the model or the engine's arrays (which,
    t_lo, t_hi, rescue_off, rescue_place, chosen), ch: the primary chains -> (simulated, judged, excused for a capped seed,
    excused without a candidate, rescued wrong primaries)."""
    simulated = judged = cap = none = copy = 0
    for p, f in enumerate(c.frag):
        if f is None:
            continue
        simulated += 1
        t0, t1 = true_columns(c, p)
        meets = lambda lo, hi: int(m.t_lo[p]) < hi and lo < int(m.t_hi[p])      # noqa: E731
        if cut_away(c, s, 2 * p) or cut_away(c, s, 2 * p + 1):
            cap += 1
        elif m.which[p] == PM.NO_PAIR:
            none += 1
        elif not meets(t0, t1) and any(meets(lo, hi) for lo, hi in elsewhere(c, p)):
            copy += 1
        else:
            judged += 1
            assert meets(t0, t1), (p, c.kind[p], f, (t0, t1), (int(m.t_lo[p]), int(m.t_hi[p])))
    wrong = TP.rescued_wrong_primaries(m, c.start_col, ch.chain_off, ch.anchor_place)
    return simulated, judged, cap, none, copy, wrong


def facts():
    """Everything test_input_is_what_it_claims asserts, measured on the models."""
    c, m = cpu(), model()
    n, P = len(c.reads), len(c.reads) // 2
    seeds, places = np.diff(c.seed_off.astype(np.int64)), c.places_per_read
    out = dict(pairs=P, virtual_reads=2 * n, seeds=len(c.q_start), places=len(c.start_col), no_column=int((c.start_col == NONE).sum()))
    out["several_seeds"] = int((seeds >= 3).sum())
    ends = [(int(c.length[m.rescue_seed[int(a)]]), int(c.length[m.rescue_seed[int(b) - 1]])) for a, b in zip(m.rescue_off, m.rescue_off[1:]) if b > a]
    out["rescue_chains_first_and_last_seed_differ"] = sum(x != y for x, y in ends)
    out["between"] = int(((seeds[1:-1] == 0) & (places[:-2] > 0) & (places[2:] > 0)).sum())
    out["stats"] = dict(m.stats)
    # the pairs of the flank group: the primary of the mate in the conserved stretch at another copy
    sp = spans(c, c)
    flank = wrong = 0
    for p, k in enumerate(c.kind):
        if k in ("flank", "exact"):
            R = 2 * p + [t[3] for t in c.truth[2 * p:2 * p + 2]].index(1)          # the reverse mate, in the conserved stretch
            t0, t1 = true_columns(c, p)
            v = n + R
            flank += 1
            wrong += sp[v] is not None and not (sp[v][0] < t1 and t0 < sp[v][1])
    out["flank"], out["flank_primary_elsewhere"] = flank, wrong
    # the tiers of the rescue runs: kept and excluded places in wave and spill reads, adopted spill rescue chains
    small, wave, spill = QS.tiers(c)
    kept = np.array(m.kept)
    out["tiers"] = [int(x.sum()) for x in (small, wave, spill)]
    out["wave_kept_and_excluded"] = int((wave & (kept > 0) & (kept < places)).sum())
    out["spill_kept_and_excluded"] = int((spill & (kept > 0) & (kept < places)).sum())
    out["spill_rescue_adopted"] = sum(1 for ch in m.chosen if ch is not None and spill[ch[0] if ch[2] else ch[1]])
    out["long_mates"] = sum(len(r) >= 400 for r in c.reads)
    # ties and winners
    tie = other = 0
    for p in range(P):
        cs = candidates(c, c, m, p, NATURAL)
        ok = [sc for v, sc in cs if all(v)]
        if ok:
            best = [i for i, (v, sc) in enumerate(cs) if all(v) and sc == max(ok)]
            assert best[0] == m.which[p]
            tie += len(best) > 1
            other += best[0] != 0
    out["tie_smaller_wins"], out["winner_not_0"] = tie, other
    out["edges"] = {ins: on_the_edges(c, c, ins[1]) for ins in (NATURAL, ABUT)}
    # the degenerate pairs and what HIGH empties
    out["degenerate"] = sum(f is None for f in c.frag)
    prim = np.diff(c.chain_off.astype(np.int64)) > 0
    gone = prim & (np.diff(primary(False, HIGH).chain_off.astype(np.int64)) == 0)
    mh = model(NATURAL, False, HIGH)
    out["emptied_by_high"], out["primaries"] = int(gone.sum()), int(prim.sum())
    out["emptied_in_pairs_without_candidate"] = int(sum(gone[v] for p in np.flatnonzero(mh.which == PM.NO_PAIR).tolist()
                                                        for v in (2 * p, 2 * p + 1, 2 * p + n, 2 * p + 1 + n)))
    out["narrow"] = dict(model(NARROW).stats)
    return out


def with_chains(c, m):
    """c with the chains m (chain_off, score, anchor_place, anchor_seed), their rows and their strands: what the models of
    the later stages take."""
    out = SimpleNamespace(**vars(c))
    for f in TR.CHAIN_FIELDS:
        setattr(out, f, getattr(m, f))
    out.chain_n_rows, out.chain_first_row, out.row_bits, out.chain_sets = RM.chain_rows(c.rm.m, c.sets, m.chain_off, m.anchor_place)
    out.strand, out.best_score = TP.strands_of(m, len(c.reads))
    return out


@functools.lru_cache(maxsize=None)
def selection():
    """At most 64 virtual reads for the graph calls: reads that adopt a rescue chain in other columns than their primary
    (and two adopted rescue chains of the spill tier), twins that lose a chain, reads of pairs without a candidate that have one."""
    c, m = cpu(), model()
    n = len(c.reads)
    spill = QS.tiers(c)[2]
    full = np.diff(c.chain_off.astype(np.int64)) > 0
    rescued, twins, kept, spilled = [], [], [], []
    for p, ch in enumerate(m.chosen):
        if ch is None:
            kept += [v for v in (2 * p, 2 * p + 1, 2 * p + n, 2 * p + 1 + n) if full[v]]
            continue
        f, r, fr, rr = ch
        w = f if fr else r
        a, b, a0, b0 = int(m.rescue_off[w]), int(m.rescue_off[w + 1]), int(c.chain_off[w]), int(c.chain_off[w + 1])
        if m.rescue_place[a:b].tolist() != c.anchor_place[a0:b0].tolist():
            rescued.append(w)
        if spill[w]:
            spilled.append(w)
        twins += [v for v in (PM.twin(f, n), PM.twin(r, n)) if full[v]]
    big = ([w for w in rescued if spill[w]] + [w for w in spilled if w not in rescued])[:2]
    short = lambda vs: [v for v in vs if c.lens[v] <= 100]      # noqa: E731
    chosen = big + short(rescued)[:30] + short(twins)[:14] + short(kept)[:14]
    sel = np.zeros(2 * n, dtype=np.uint8)
    sel[chosen] = 1
    return tuple(int(x) for x in sel), len(big), len(short(rescued)[:30]), len(short(twins)[:14]), len(short(kept)[:14])


@functools.lru_cache(maxsize=None)
def adopted():
    """The models of every later stage on the adopted chains of model(): the chains with rows and strands, the row
    alignment and its CIGAR, the second-best chains and qualities, the graph alignment and its CIGAR of selection()."""
    from unittest import mock
    c = with_chains(cpu(), model())
    with mock.patch.object(AM, "LITERAL_CELLS", 0):
        am = AM.of_cpu(c)
    with mock.patch.object(CG, "LITERAL_CELLS", 0):
        cg = CG.of_align(c, am)
        qm = QM.solve(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, c.lens, c.chain_off, c.score, c.anchor_place,
                      c.anchor_seed, BAND, 0, True, {})
        g = GM.Graph(*c.graph, len(c.b))
        gm = GM.of_cpu(g, c, 16, 0, selection()[0], rows_only=True)
        gc = JM.of_graph(g, c, gm)
    return SimpleNamespace(c=c, am=am, cg=cg, qm=qm, g=g, gm=gm, gc=gc)


def batch_cuts(c):
    """Three batches of unequal size: [0, a, b, n] in given reads, a degenerate pair before and a spill-tier pair behind a and b."""
    n = len(c.reads)
    spill = QS.tiers(c)[2]
    at = [2 * (p + 1) for p in range(len(c.frag) - 1) if c.frag[p] is None and c.kind[p + 1] in ("long", "array")
          and any(spill[v] for v in (2 * p + 2, 2 * p + 3, 2 * p + 2 + n, 2 * p + 3 + n))]
    return [0, at[0], at[4], n]


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_input_is_what_it_claims():
    """Everything the docstring counts, on the models alone; each floor about half of the measured figure."""
    c, m, f = cpu(), model(), facts()
    print("pairs_scale:", f)
    A, n = c.A, len(c.reads)
    assert A.shape == (QS.ROWS, QS.BASE + 2 * len(QS.UNIT) * QS.ARRAY_COPIES) and MS.oracle_boundaries(A) == c.b
    # the sizes: k_pp_pick three workgroups and a partial last wave, k_pp_span ten, k_pp_mask hundreds
    assert f["pairs"] >= 600 and f["pairs"] % 64 and f["pairs"] > 2 * 256 and f["virtual_reads"] > 9 * 256 and f["places"] >= 50000
    assert f["several_seeds"] >= 600 and f["stats"]["rescue_differs"] >= 35 and f["rescue_chains_first_and_last_seed_differ"] >= 100
    for R, t in enumerate(c.truth):               # a simulated mate is its row's text with N and substitutions: at most 2 + a 13th
        if t is not None and c.kind[R // 2] != "nocol":
            row, a, ln, strand = t
            text = c.rm.G[row][a:a + ln]
            got = rc(c.reads[R]) if strand else c.reads[R]
            assert len(got) == ln and sum(x != y for x, y in zip(got, text)) <= 2 + (ln + 1) // 13
    # one mate in the conserved stretch, the other in the private flank; the primary of the first at another copy
    assert f["flank"] == N_FLANK and f["flank_primary_elsewhere"] >= 20
    for p, k in enumerate(c.kind):
        if k in ("flank", "exact"):
            cols = sorted((int(c.cols[r][a]), int(c.cols[r][a + ln - 1]) + 1) for r, a, ln, _ in c.truth[2 * p:2 * p + 2])
            x0 = min(x for x, _ in map(c.loci.get, LOCI) if x > cols[0][0])
            assert x0 - FLANK <= cols[0][0] and cols[0][1] <= x0 <= cols[1][0] and cols[1][1] <= x0 + CONSERVED
            if k == "exact":
                assert cols[1][1] - cols[0][0] in (EXACT, EXACT + 1)
    # long mates; kept and excluded places in rescue runs of the wave and the spill tier; an adopted spill-tier rescue chain
    assert f["long_mates"] == 2 * (N_LONG + N_ARRAY) and min(f["tiers"]) >= 10
    assert f["wave_kept_and_excluded"] >= 300 and f["spill_kept_and_excluded"] >= 10 and f["spill_rescue_adopted"] >= 5
    assert MS.model_chain_stats(c)["reads_spill"] == f["tiers"][2]
    # the clamp at 0, the edges of the windows (at ABUT by construction), places without a column
    assert f["edges"][NATURAL]["clamp"] >= 100
    assert sum(c.frag[p] is not None and c.frag[p][1] < 12 and true_columns(c, p)[1] < NATURAL[1] for p in range(n // 2)) >= N_FIRST
    for what in ("lo_kept", "lo_dropped", "hi_kept", "hi_dropped"):
        assert f["edges"][ABUT][what] >= 100, (what, f["edges"])
    assert f["no_column"] >= 90
    assert m.stats["places_kept"] + m.stats["places_excluded"] == f["places"] - f["no_column"]
    # degenerate pairs between ordinary ones; reads without seeds between reads with places; ties; every candidate
    assert f["degenerate"] >= 12 and {"empty", "all_n", "capped", "identical", "own_rc"} <= set(c.kind)
    assert all(c.frag[p - 1] is not None and c.frag[p + 1] is not None for p in range(n // 2) if c.frag[p] is None)
    for p, k in enumerate(c.kind):
        if k == "capped":                         # every seed of that mate kept CAP of its places
            v = 2 * p + [t is None for t in c.truth[2 * p:2 * p + 2]].index(True)
            t0, t1 = int(c.seed_off[v]), int(c.seed_off[v + 1])
            assert t1 > t0 and (c.start_total[t0:t1] > CAP).all() and (np.diff(c.start_off.astype(np.int64))[t0:t1] == CAP).all()
    assert f["between"] >= 300 and f["tie_smaller_wins"] >= 250 and f["winner_not_0"] >= 190
    st = m.stats
    assert min(st["which0"], st["which2"]) >= 150 and min(st["which1"], st["which3"], st["none"]) >= 20, st
    # HIGH empties a share of the primary chains, some of them in pairs that then have no candidate
    assert 250 <= f["emptied_by_high"] <= f["primaries"] - 250 and f["emptied_in_pairs_without_candidate"] >= 100
    # NARROW rejects about half of the pairs of NATURAL, with the same windows: on the insert condition alone
    proper, narrow = f["pairs"] - st["none"], f["pairs"] - f["narrow"]["none"]
    assert 0.3 * proper <= narrow <= 0.7 * proper and f["narrow"]["places_kept"] == st["places_kept"]
    # the other bounds: nothing at (0, 0); at (0, 2^64 - 1) every window of a forward chain is open above
    assert (model((0, 0)).which == PM.NO_PAIR).all() and model((0, 0)).rescue_off[-1] == 0
    assert model((0, U64)).stats["places_kept"] > st["places_kept"]
    exact = [p for p, k in enumerate(c.kind) if k == "exact"]
    wide = np.array([true_columns(c, p)[1] - true_columns(c, p)[0] for p in exact])
    got = model(ABUT).which[exact] != PM.NO_PAIR
    print("ABUT: proper among the fragments of EXACT columns", int(got[wide == EXACT].sum()), "of", int((wide == EXACT).sum()))
    assert got[wide == EXACT].sum() >= 30 and not got[wide == EXACT + 1].any()      # not the fragments of one column more
    # the batches of test_a_pair_is_independent_of_its_batch and the selection of test_every_stage_on_adopted_chains
    cuts = batch_cuts(c)
    assert len({b - a for a, b in zip(cuts, cuts[1:])}) == 3 and all(x % 2 == 0 for x in cuts)
    sel = selection()
    assert sum(sel[0]) <= 64 and sel[1] == 2 and min(sel[2:]) >= 10, sel[1:]


def test_by_row_chains_are_another_primary():
    c, b = cpu(), primary(True)
    many = c.places_per_read > BYROW_MAX
    assert b.too_many == many.sum() > 0 and not b.score[many].any() and (b.score > 0).sum() > 500
    m = model(NATURAL, True)
    assert not np.array_equal(b.anchor_place, c.anchor_place) and (m.which != PM.NO_PAIR).sum() > 300
    print("by row:", dict(chained=int((b.score > 0).sum()), too_many=b.too_many, stats=m.stats))


def test_model_finds_the_fragments():
    """The ground truth, at NATURAL: see check_truth.  744 pairs, 730 simulated, 652 judged; excused: 48 whose true place the
    cap cut away, 13 without a candidate, 17 whose text stands at another copy as well and that were found there."""
    c, m = cpu(), model()
    simulated, judged, cap, none, copy, wrong = check_truth(c, c, m, c)
    print("truth:", dict(simulated=simulated, judged=judged, cut_away=cap, no_candidate=none, at_a_copy=copy, rescued_wrong_primaries=wrong))
    assert simulated == sum(f is not None for f in c.frag) and judged + cap + none + copy == simulated
    assert 5 * (cap + none + copy) <= simulated and wrong >= 90


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def pairs_call(pix, ins, by_row=False, min_score=0, adopt=False, **kw):
    return pix.chains(band=BAND, min_score=min_score, by_row=by_row, pairs=ins, adopt_pairs=adopt, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("by_row", [False, True])
def test_parity_plain_and_by_row(engine, by_row):
    c = cpu()
    with fbg_options(engine, {"byrow_max": BYROW_MAX}), QS.build(engine, c) as pix:
        QS.seeded(pix, c)
        for min_score in (0, HIGH):
            want = primary(by_row, min_score)
            ch0 = pix.chains(band=BAND, min_score=min_score, by_row=by_row)
            TP.same_adopted(ch0, want, (by_row, min_score, "primary"))
            for ins in INSERTS:
                what = (by_row, min_score, ins)
                m = model(ins, by_row, min_score)
                ch = pairs_call(pix, ins, by_row, min_score)
                TP.same(ch, m, what)
                TP.same_adopted(ch, want, what)                       # without adopt the chains are the primaries, bit for bit
                ad = pairs_call(pix, ins, by_row, min_score, adopt=True)
                TP.same(ad, m, what + ("adopt",))
                TP.same_adopted(ad, m, what + ("adopt",))
                if ins == (0, 0):
                    assert (ch.pair_which == PM.NO_PAIR).all() and ch.rescue_off[-1] == 0
            st = pix.chain_stats()
            assert min(st["reads_small"], st["reads_wave"], st["reads_spill"]) > 0


def as_model(ch):
    """The arrays of a pairs call under the names of the model."""
    out = SimpleNamespace(**{g: getattr(ch, f) for f, g in TP.FIELDS})
    out.chosen = [ch.pair(p) for p in range(len(ch.pair_which))]
    return out


@pytest.mark.gpu
def test_truth_on_what_the_engine_returns(engine):
    c = cpu()
    with QS.build(engine, c) as pix:
        sd = QS.seeded(pix, c)
        s = SimpleNamespace(seed_off=sd.seed_off, q_start=sd.q_start, start_off=sd.occ.start_off, start_col=sd.occ.start_col,
                            start_total=sd.occ.start_total)
        ch0 = pix.chains(band=BAND)
        ch = pairs_call(pix, NATURAL)
        simulated, judged, cap, none, copy, wrong = check_truth(c, s, as_model(ch), ch0)
        assert 5 * (cap + none + copy) <= simulated and judged + cap + none + copy == simulated and wrong >= 90


@pytest.mark.gpu
def test_every_stage_on_adopted_chains(engine):
    import ctypes
    import test_align_scale as AS
    import test_graph_cigar_scale as GS
    from founderblockgraphs_amd import _lib
    L, INVALID = _lib.lib(), _lib.FBG_ERR_INVALID
    u32, u64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    c, m, a = cpu(), model(), adopted()
    n, V = len(c.reads), 2 * len(c.reads)
    sel = np.array(selection()[0], dtype=np.uint8)
    every = dict(rows=True, align=True, cigar=True, mapq=True, graph=True, graph_cigar=True, select=sel)
    with QS.build(engine, c) as pix:
        sd = QS.seeded(pix, c)
        pix.chains(band=BAND, **every)                                # every stage is current, on the primary chains
        code, out, stats = TP.c_pairs(pix, V, NATURAL, adopt=True, nseeds=len(sd.q_start))
        assert code == 0 and dict(zip(PM.STATS, stats.tolist())) == m.stats
        assert np.array_equal(out[-2], m.chain_off) and np.array_equal(out[-1], m.score)
        # every stage made from the chains is stale, with px_need's message
        big = [np.zeros(len(sd.q_start) + len(sd.occ.start_col) + V + 2, dtype=np.uint32) for _ in range(2)]
        wide, total = np.zeros(V + 1, dtype=np.uint64), ctypes.c_uint64(0)
        for stale in (lambda: L.fbg_pindex_chains_cigar(pix._h, None, ctypes.byref(total), None),
                      lambda: L.fbg_pindex_chains_cigar_fetch(pix._h, u64(wide), u32(big[0])),
                      lambda: L.fbg_pindex_chains_mapq_fetch(pix._h, u32(big[0]), u32(big[1]), None),
                      lambda: L.fbg_pindex_mapq_strands(pix._h, big[0].ctypes.data_as(_lib.u8p), None),
                      lambda: L.fbg_pindex_chains_align_graph_fetch(pix._h, u64(wide), u32(big[0])),
                      lambda: L.fbg_pindex_chains_graph_cigar(pix._h, None, ctypes.byref(total), None),
                      lambda: L.fbg_pindex_chains_graph_cigar_fetch(pix._h, u64(wide), u32(big[0]))):
            assert stale() == INVALID and "no current" in TP.engine_error(engine)
        assert pix.mapq_stats() == dict.fromkeys(pix.mapq_stats(), 0)
        # run again, every stage equals its model on the model's adopted chains
        ch = pairs_call(pix, NATURAL, adopt=True, **every)
        TP.same(ch, m, "adopt")
        TP.same_adopted(ch, m, "adopt")
        assert np.array_equal(ch.strand, a.c.strand) and np.array_equal(ch.best_score, a.c.best_score)
        for got, want, f in ((ch.n_rows, a.c.chain_n_rows, "n_rows"), (ch.first_row, a.c.chain_first_row, "first_row"), (ch.row_bits, a.c.row_bits, "bits")):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), f
        AS.check(pix, ch, a.c, a.am, a.cg, "adopted")
        QS.check(pix, ch, a.qm, a.c, "adopted")
        GS.check(pix, ch, a.c, a.g, a.gm, a.gc, "adopted")
        assert a.gm.stats["aligned"] >= 30 and a.am.stats["aligned"] >= 500
        # the twin of every chosen read is empty with score 0, and every given read of a proper pair has its candidate's strand
        for p, chosen in enumerate(m.chosen):
            if chosen is not None:
                f, r = chosen[:2]
                for v in (PM.twin(f, n), PM.twin(r, n)):
                    assert ch.chain_off[v] == ch.chain_off[v + 1] and ch.score[v] == 0, (p, v)
                assert ch.strand[f % n] == f // n and ch.strand[r % n] == r // n, p


def pair_view(sd, ch, p):
    """What must not depend on the batch pair p arrives in: its result, and per virtual read the rescue chain and the chain
    of the call, anchors counted from the read's first start place and first seed."""
    n = sd.reads
    out = [(int(ch.pair_which[p]), int(ch.pair_score[p]), int(ch.pair_lo[p]), int(ch.pair_hi[p])), ch.pair(p) and ch.pair(p)[2:]]
    for v in (2 * p, 2 * p + 1, 2 * p + n, 2 * p + 1 + n):
        base = np.array([int(sd.occ.start_off[int(sd.seed_off[v])]), int(sd.seed_off[v])])
        out.append((int(ch.rescue_score[v]), int(ch.rescue_lo[v]), int(ch.rescue_hi[v]), (ch.rescue(v) - base).tolist(), int(ch.score[v]),
                    (ch.of(v) - base).tolist()))
    return out


def seeds_call(pix, c, reads):
    return pix.seeds(reads, min_length=c.L, max_per_seed=CAP, msa=True, strands=True)


@pytest.mark.gpu
def test_a_pair_is_independent_of_its_batch(engine):
    c, m = cpu(), model()
    n = len(c.reads)
    cuts = batch_cuts(c)
    with QS.build(engine, c) as pix:
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            sd = seeds_call(pix, c, c.reads[a:b])
            parts.append((sd, pairs_call(pix, NATURAL, adopt=True)))
        sd = seeds_call(pix, c, c.reads)
        whole = pairs_call(pix, NATURAL, adopt=True)
        TP.same(whole, m, "whole")
        TP.same_adopted(whole, m, "whole")
        for (part_sd, part), a, b in zip(parts, cuts, cuts[1:]):
            assert part_sd.reads == b - a
            for p in range((b - a) // 2):
                assert pair_view(part_sd, part, p) == pair_view(sd, whole, a // 2 + p), (a, p)
        total = {k: sum(part.pair_stats[k] for _, part in parts) for k in PM.STATS}
        assert total == whole.pair_stats == m.stats


@pytest.mark.gpu
def test_one_index_across_a_large_call_and_small_ones(engine):
    """The whole batch, one pair, a batch without places, the whole batch again: the buffers of the pairs state are sized by
    the large call and reused; nothing of an earlier call may show."""
    c, m = cpu(), model()
    p = next(p for p, ch in enumerate(m.chosen) if ch is not None and ch[2] + ch[3] and c.kind[p] == "flank")
    with QS.build(engine, c) as pix:
        seeds_call(pix, c, c.reads)
        first = pairs_call(pix, NATURAL)
        TP.same(first, m, "first")
        TP.same_adopted(first, cpu(), "first")
        ad = pairs_call(pix, NATURAL, adopt=True)                      # 1. the whole batch, adopting
        TP.same(ad, m, "whole")
        TP.same_adopted(ad, m, "whole")
        sd = seeds_call(pix, c, c.reads[2 * p:2 * p + 2])             # 2. one pair: four virtual reads
        ch0 = pix.chains(band=BAND)
        small = pairs_call(pix, NATURAL, adopt=True)
        sm = TP.model_of(sd, ch0, BAND, NATURAL)
        TP.same(small, sm, "small")
        TP.same_adopted(small, sm, "small")
        assert small.pair_which[0] == m.which[p] and small.pair_stats["none"] == 0
        seeds_call(pix, c, [b"", b"NNN", b"N" * 30, b""])              # 3. a batch without places
        for adopt in (False, True):
            e = pairs_call(pix, NATURAL, adopt=adopt)
            assert e.pair_which.tolist() == [PM.NO_PAIR] * 2 and e.rescue_off.tolist() == [0] * 9 and e.chain_off.tolist() == [0] * 9
            assert e.pair_stats == dict(dict.fromkeys(PM.STATS, 0), none=2)
        seeds_call(pix, c, c.reads)                                   # 4. the whole batch again, without adopt
        again = pairs_call(pix, NATURAL)
        TP.same(again, m, "again")
        for f, _ in TP.FIELDS:
            assert np.array_equal(getattr(again, f), getattr(first, f)), f
        TP.same_adopted(again, first, "again")
        assert again.pair_stats == first.pair_stats


@pytest.mark.gpu
def test_tool_prints_the_pairs_of_the_whole_read_set(engine, tmp_path):
    """One fbg_locate --pairs run over every pair without an empty mate (the tool reads tokens)."""
    from oracle import pyoracle as O
    c, m = cpu(), model()
    keep = [p for p in range(len(c.reads) // 2) if c.reads[2 * p] and c.reads[2 * p + 1]]
    reads = [c.reads[2 * p + j] for p in keep for j in (0, 1)]
    k = len(reads)
    assert len(c.reads) // 2 - 5 <= len(keep) < len(c.reads) // 2
    graph, fasta = str(tmp_path / "g.xgfa"), str(tmp_path / "g.fasta")
    O.write_xgfa(c.A, c.b, graph)
    with open(fasta, "wb") as fh:
        for r, row in enumerate(c.A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))
    args = ["--graph=" + graph, "--msa=" + fasta, "--seeds=%d" % c.L, "--occurrences=%d" % CAP, "--chain=%d" % BAND, "--strands",
            "--pairs=%d,%d" % NATURAL]
    got = TC.TL.run_locate(args, b"".join(r + b"\n" for r in reads))
    assert got.returncode == 0, got.stderr
    with QS.build(engine, c) as pix:
        sd = seeds_call(pix, c, reads)
        tm = TP.model_of(sd, pix.chains(band=BAND), BAND, NATURAL)
    for f in ("which", "pair_score", "t_lo", "t_hi"):             # a pair does not depend on its batch: the model of the whole set
        assert np.array_equal(getattr(tm, f), getattr(m, f)[keep]), f
    lines = got.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith(b"Z\t")] == TP.z_lines(tm)
    assert [ln for ln in lines if ln[:2] in (b"C\t", b"A\t", b"T\t")] == TP.chain_lines(sd, tm, k)
