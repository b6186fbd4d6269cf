"""Mate rescue by alignment at scale (fbg_pindex_pairs_align; k_pl_frag, k_pl_window, k_pl_pick of csrc/pindex_pairs_align.hip and
k_pa_gather / k_pa_edit through pa_windows) on two seeded inputs with a ground truth outside the model, between the toy
inputs of test_pair_align.py and a workload.  The checker is tests/pair_align_model.py on the whole CPU pipeline of the
models: test_mapping_scale.cpu(source=...) for seeds, places, chains and rows, byrow_model and pairs_model where the chains
are by row or adopted, then pair_align_model.solve with the row-at-a-time alignment of test_pair_align (one memo by read and
window).  No array of the engine enters a model, and every GPU comparison is exact: nine arrays and ten counters.

Input A: 1192 interleaved pairs on the `founders` MSA of test_mapping_scale.py (200 rows x 1500 columns, about 140 blocks,
row EARLY = 77 ends 200 columns early), min_length 12, max_per_seed 32, band 8, both strands.  V = 4768 virtual reads: 19
workgroups of k_pl_frag and k_pl_window with a last one of 160 (161) lanes, 5 of k_pl_pick with a last one of 168 lanes and
a last wave of 40.  A pair is cut from a fragment (row, first symbol, extent) of a row's gap-stripped text: mate 1 its first
symbols, mate 2 the reverse complement of its last ones; the pair is built for a candidate number 0 .. 3 (which mate is
damaged, which is given first), the numbers in turn.  A damaged mate has a substitution at every 6th symbol, drawn again
until seeds_model finds no seed of 12 on either strand; every third of the plain ones also has 1 .. 3 inserted or deleted
symbols.  The partner has no N and, one in four, one substitution.  The groups:
  plain 620      fragments of 150 .. 400 symbols, mates of 50 .. 120;
  tiers 49       four pairs (one per candidate number) for a damaged mate of 64, 65, 128, 129, 192, 193, 256, 257, 320, 512,
                 1023 and 1024 symbols and one of 1025: the register tiers of 1 .. 4 words, the LDS tier, too_long; run at
                 their own max_insert TIERS;
  first 24, last 24   fragments that begin in symbols 0 .. 11 and that end in the last 12 of a row (row 77 and three rows
                 that copy its founder among them);
  pre 16, post 16   a chained forward mate that begins in symbols 0 .. 2 with 3 .. 8 random symbols before it (x_1 - q_1 < 0),
                 a chained reverse mate that ends with its row with 3 .. 8 symbols behind it (x_last + L - q_last > |G_r|).
                 Behind a row's last symbol a seed runs on by one symbol whatever the letter (the restart of the search at
                 the last node), and no row spells such a seed: the symbols behind begin with an N;
  early 12       the chained mate over a private symbol of row 77, which no other row carries: a forward one whose window
                 runs into that row's end, a reverse one that ends with the row and goes on: fe is clamped at a |G_r| that
                 k_pl_frag makes without a last node;
  high 60        rows that copy founder 10 (rows >= 64), every second chained mate over a private symbol of a row >= 128;
  block 48       a forward chained mate that begins at p(r, j), one symbol before it, one after it, j >= 1;
  abut 40, abut1 40   extent max_insert of NATURAL, and one more; mates of 60 symbols, the partner exact;
  over 40        fragments 13 .. 40 symbols longer than max_insert: the window cuts the damaged mate (0.38 edits per symbol
                 against 0.19 of the plain group);
  both 60        no mate damaged: 20 exact, 20 with a substitution in symbols 3 .. 10 of one mate (its chain scores less:
                 the other candidate wins), 20 with both mates a piece and its reverse complement (they chain on either
                 strand: three and four valid candidates);
  chance 40      a damaged mate with 16 symbols of another place over a stretch: a seed and a chain elsewhere.  The default
                 selection passes it over, the mask of the damaged reads takes it;
  no_row 40      the partner with an N at every 13th symbol, as in test_pairs_scale: every seed picks its place on its own;
  shift 40       the partner with 1 .. 3 symbols inserted or deleted in its middle third: its last anchor lies off its first
                 one's diagonal.  Added after the planted error "fe from the first anchor's record" changed nothing;
  degenerate 23  after every 49 others: an empty mate, an all-N mate of 30, two identical mates, a mate and its own reverse
                 complement, a mate from another row's far end.
Input B: 150 pairs on test_mapq_scale.duplications_msa() (max_per_seed 64): the forward mate exact in the private flank of
the segment or of its first copy, the reverse mate damaged, cut from the conserved stretch TIE whose text stands at both
loci (all 150 do); only the window says which.

What test_inputs_are_what_they_claim asserts of the models, default selection at NATURAL = (100, 448) unless said,
measured (floor):
  damaged mates with inserted or deleted symbols 207 (a third of the plain group); aligned reads with t_end - t_start != L
  401 (200); aligned reads of 1, 2, 3, 4 words and of the LDS tier 226, 559, 8, 7, 15 (113, 280, 4, 3, 7); at TIERS every
  tier length has 2 .. 5 aligned reads, 38 in all (1 each, 19), and the read of 1025 symbols is too_long;
  forward windows cut short by the row's end 57 (28), reverse windows from 0: 44 (22); fragments clamped at 0: 15 (7), at
  |G_r| 19 (9), 3 of them on row 77 (2); windows on row 77, whose last cell has no node, 7 (3);
  windows with row >= 64: 198 (100), >= 128: 94 (47); forward windows that begin at a p(r, j), one before, one after: 58,
  28, 56 (14 each); chains whose ends lie on different diagonals 15 (7);
  all-ones mask: selected 1482, aligned 1020 (the condition: 1000), no_row 455 = 31 % (at most 40 %); pairs with three or
  four valid candidates 15 (7); ties at the best score that the smaller number wins 11 (5); winners that are not the
  smallest valid number 54 (27);
  damaged mask: which 0 .. 3: 200, 191, 207, 186 (the condition: 100 each); chance reads with a chain 40 (all), whose
  result differs between the default selection and the mask 29 (14);
  the quarter mask selects 786 reads whose partner has no chain (390): of the 1167 it marks, selected counts 381;
  all-N mates with edits == L and t_start == t_end == w0: 5 (2);
  NARROW = (275, 448) keeps 454 of 801 accepted reads: 43 % rejected on the insert alone (30 % .. 70 %);
  the median edits of the accepted reads 15 = MEDIAN_EDITS; at that bound 122 rejected_edits under the quarter mask (60);
  ABUT = (448, 448) with max_edits 10, the substitutions of an abut mate: 32 of the 40 fragments of 448 symbols are accepted
  (16), the 18 forward-window ones all with t_end == w1 (8).  The issue expected none of the fragments of 449 to be accepted
  at min_insert == max_insert.  By the header's definition that does not hold: a window that cuts one symbol off a mate still
  holds an alignment that ends on its last column, with one more edit (23 of 27 accepted ones) or as many (4; never fewer,
  never two more: asserted).  With the bound 3 of the 40 pass (at most a quarter of the other kind), without it 27;
  every one of the ten counters is non-zero in some run; nothing is aligned at (0, 0); at (0, 2^64 - 1) every window runs to
  its row's end or from 0.

The ground truth (test_model_finds_the_fragments, and test_truth_on_what_the_engine_returns on the engine's arrays, which
must give the same counts): under the damaged mask at NATURAL, [t_start, t_end) of mate_row in MSA columns meets the columns
the mate was cut from; for B inside the partner's locus.  After chains by row, where every chain has a row: A 1109
simulated, 1007 judged, 93 fragments over max_insert (tiers, over, abut1), 9 without a row (more than byrow_max places), 0
not accepted, 0 found a second time; B 150 of 150 judged; excused 102 of 1259 = 8 % (at most 25 %).  After plain chains
every judged pair is right as well (A 711, B 150), but 305 partners of A have no carrying row: a seed inside a node takes its
smallest place on its own, as 29 % of the chains of the founders' single reads do, so the 25 % are asserted by row.

The GPU tests: test_parity in three modes (plain chains, by_row with byrow_max 512, adopt_pairs) over RUNS: NATURAL under
the four selections, PLUS and MINUS (|W| % 64 of 1 and 63), NARROW, ABUT with and without its bound, (0, 2^64 - 1), (0, 0),
TIERS, max_edits 0, 15 and none, pair_max_window at 0, max_insert and max_insert - 1, through Python and through the C call
with its guard entries; the chains are compared with the model's first.  The batches of 64 pairs (V = 256: the second
workgroup of k_pl_window holds the lane of wlen[V] alone), 128 pairs, one pair and the rest; one index across the whole set,
one pair, no places, nothing selected, chains(align=True), the whole set again, then the widest windows and the narrowest;
one fbg_locate --pair-align run over the 1187 pairs without an empty mate.

Planted errors.  The errors of the issue were to be tried on scratch builds on the GPU; that run was not made (see the
commit message).  They are made instead in kernels_restated(), the three kernels once more lane by lane with their unsigned
arithmetic, which without an error equals the model on every run it is tried on, as the kernels do on the GPU; an error that
changes a compared array or counter there fails the exact comparison of every GPU test that makes such a run (parity in
each mode; the batches at NATURAL, max_edits 15, all ones; the one index at NATURAL; the tool at NATURAL, max_edits 15, on
adopted chains).
test_planted_errors_change_what_the_parity_tests_compare keeps that asserted.  Entries that differ, at NATURAL with the
default selection unless said:
  k_pl_pick `sc >= best`: which 2, all ones 11 (and t_hi 2): parity, the one index, the batches (which 9); not the tool;
  `got <= min_insert`: NARROW 1 read, ABUT all 78 pairs (pairs 0 for 78), ABUT with the bound 35: parity only;
  `e >= max_edits`: max_edits 15 under the quarter mask 15 reads (rejected_edits 137 for 122), ABUT with the bound 35:
  parity, the batches (55 reads) and the tool (50);
  L_w taken from v: pair_score of 681 pairs: parity, the batches, the one index, the tool ("all four" below);
  the insert of odd candidates as te - fs: insert 387, pairs 731 for 760: all four;
  pl_partner without the ^ 1: row 832, edits 828, which 462, selected 1175 for 1222: all four;
  k_pl_frag fe from the first anchor: insert 5, t_hi 5 (4 in the batches and the tool): all four; nothing before the shift group;
  glen without the last label's length: insert 17, t_hi 17, cells 33 291 071 for 33 295 537: all four;
  the reverse window opened at fs: edits 376, insert 388, which 144, pairs 619 for 760: all four;
  counters of k_pl_window by wave 0 only: selected 311 for 1222, aligned 199 for 815: parity, the batches, the one index
  (the tool prints no counters);
  counters of k_pl_pick by wave 0 only: pairs 212 for 760, rejected_insert 1 for 14: parity, the batches, the one index.
The truth test counts pairs and is too coarse for most of them.

Time: the CPU tests 21 s (test_inputs_are_what_they_claim 15 s: it runs the models of a dozen runs).  On the GPU, each with
its models, beside its nearest sibling of test_pairs_scale.py in the same session: test_parity[adopt] 6.2 s (it runs first
and makes the inputs, the plain chains and the memo of alignments), [by_row] 1.8 s, [plain] 0.2 s, against 6.6 s and 4.5 s of
test_parity_plain_and_by_row; the truth on the engine's arrays 0.5 s against 0.06 s (two indexes, A and B, each after plain
chains and by row: the condition on the excused share spans both inputs, so it stays one test); the batches 0.08 s against
0.11 s; the one index 0.07 s against 0.08 s; the tool 1.6 s (two runs, with and without the flag) against 0.9 s."""
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
import heuristic_model as HM  # noqa: E402
import occ_model as OM  # noqa: E402
import pair_align_model as PA  # noqa: E402
import pairs_model as PM  # noqa: E402
import rows_model as RM  # noqa: E402
import seeds_model as SDM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
import test_mapping_scale as MS  # noqa: E402
import test_mapq_scale as QS  # noqa: E402
import test_pair_align as TA  # noqa: E402
import test_pairs as TP  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options  # noqa: E402

GAP, NONE, U64, TABLE = MS.GAP, PA.NONE, 0xffffffffffffffff, MS.TABLE
L, BAND, BYROW_MAX = MS.MIN_LENGTH, 8, 512          # min_length and band of every call; option byrow_max of the by-row calls
CAP_A, CAP_B = 32, QS.CAP                            # max_per_seed on the founders and on the duplications
EARLY = MS.EARLY
TIE, FLANK = (74, 147), QS.FLANK                     # the conserved stretch that segment and first copy share; the private flank before a locus
EVERY, EVERY_SUB = 50, 6                             # a degenerate pair after every EVERY - 1 others; a substitution at every 6th symbol
TIER_LENGTHS = (64, 65, 128, 129, 192, 193, 256, 257, 320, 512, 1023, 1024)      # of a damaged mate: 1 .. 4 words, LDS; then one of 1025
ABUT_MATE = 60                                       # symbols of both mates of the abut group: ten substitutions in the damaged one
N_PLAIN, N_FIRST, N_LAST, N_PRE, N_POST, N_EARLY = 620, 24, 24, 16, 16, 12          # pairs of each group of input A
N_HIGH, N_BLOCK, N_ABUT, N_OVER, N_BOTH, N_CHANCE, N_NOROW = 60, 48, 80, 40, 60, 40, 40
N_SHIFT = 40                                         # partners with symbols inserted or deleted in their middle third
N_B = 150
# the insert bounds of the parity runs, in symbols of the partner's row, and what each is for
NATURAL = (100, 448)                                 # holds the plain fragments (150 .. 400 symbols); 448 = 7 * 64: |W| % 64 == 0 in pa_chunk
PLUS, MINUS = (100, 449), (100, 447)                 # |W| % 64 of 1 and of 63
NARROW = (275, 448)                                  # rejects the shorter half of the plain fragments on the insert alone
ABUT = (448, 448)                                    # min_insert == max_insert: the alignment ends on the window's last column or is rejected
WIDE = (0, U64)                                      # clamped at 2^33: every window reaches the row's end (or its start)
NOTHING = (0, 0)                                     # every window is empty
TIERS = (0, 1152)                                    # holds the fragments of the tiers group (up to 1135 symbols)
ABUT_EDITS = len(range(EVERY_SUB // 3, ABUT_MATE, EVERY_SUB))      # the substitutions of an abut mate: one symbol cut away costs one more
MEDIAN_EDITS = 15                                    # near the median edits of the accepted reads at NATURAL (measured: see the docstring)
MODES = {"plain": dict(), "by_row": dict(by_row=True), "adopt": dict(adopt_pairs=True)}
# (insert, max_edits, max_window, selection) of the parity runs of every mode
RUNS = ((NATURAL, NONE, 0, None), (NATURAL, NONE, 0, "ones"), (NATURAL, NONE, 0, "damaged"), (NATURAL, MEDIAN_EDITS, 0, "quarter"),
        (PLUS, 0, 0, None), (MINUS, NONE, MINUS[1], None), (NARROW, NONE, 0, None), (ABUT, NONE, 0, None), (ABUT, ABUT_EDITS, 0, "damaged"),
        (WIDE, NONE, 0, None), (NOTHING, NONE, 0, "ones"), (TIERS, NONE, 0, None), (NATURAL, NONE, NATURAL[1] - 1, None),
        (NATURAL, NONE, NATURAL[1], None))


# ---- the inputs ---------------------------------------------------------------------------------------------------------

def rc(s):
    return STM.revcomp(bytes(s), TABLE)


@functools.lru_cache(maxsize=None)
def host(which):
    """The MSA of an input with what the construction asks of it: the row texts, the index for the seeds of a mate, p(r, j)."""
    A = MS.founders_msa()[0] if which == "a" else QS.duplications_msa()[0]
    b = MS.oracle_boundaries(A)
    labels, edges, _ = HM.segmentation_graph(A, b)
    return SimpleNamespace(A=A, b=b, G=MS.stripped(A), index=OM.Index(labels, edges), rm=RM.Model(A, b))


def n_seeds(h, read):
    """Seeds of L symbols of a read, on both strands (seeds_model.cuts: the seeds without their places)."""
    return sum(k >= L for P in (bytes(read), rc(read)) if P for _, k in SDM.cuts(h.index, P))


def letters(rng, k):
    return bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))


def damage(rng, h, text, indels=0, splice=None):
    """`text` with a substitution at every 6th symbol from the third on, then `indels` inserted or deleted symbols, drawn
    again until seeds_model finds no seed of L on either strand; None after forty draws.  splice: 16 symbols put over a
    stretch of the result instead, and a seed is then required: the chance group."""
    for _ in range(40):
        out = bytearray(text)
        for at in range(EVERY_SUB // 3, len(out), EVERY_SUB):
            out[at] = rng.choice([c for c in b"ACGT" if c != out[at]])
        for _ in range(indels):
            at = int(rng.integers(1, len(out) - 1))
            if rng.integers(0, 2):
                out.insert(at, int(rng.choice(list(b"ACGT"))))
            else:
                del out[at]
        if splice is not None:
            at = int(rng.integers(4, len(out) - len(splice) - 4))
            out[at:at + len(splice)] = splice
        if (n_seeds(h, out) == 0) == (splice is None):
            return bytes(out)
    return None


def pair_of(rng, h, kind, r, a, f, l1, l2, cand, indels=0, subs=1, pre=0, post=0, npat=False, splice=None, shift=0):
    """-> None or a namespace: the pair of a fragment (row r, first symbol a, extent f), mate 1 its first l1 symbols and
    mate 2 the reverse complement of its last l2.  cand: the candidate number the pair is built for: the reverse mate is
    damaged for 0 and 2, the forward one for 1 and 3, and the mates change places for 2 and 3; None: no mate is damaged.
    The other mate has no N and at most `subs` substitutions (npat: an N at every 13th symbol instead), `pre` random symbols
    before a forward one, `post` behind a reverse one (before it is complemented), `shift` symbols inserted or deleted in
    its middle third: its first and its last anchor then lie on different diagonals."""
    G = h.G[r]
    if a < 0 or a + f > len(G) or max(l1, l2) > f or min(l1, l2) < 1:
        return None
    text = [G[a:a + l1], G[a + f - l2:a + f]]
    dam = None if cand is None else int(cand in (0, 2))
    made = [0, 0]
    mates = []
    for k in (0, 1):
        if k == dam:
            s = damage(rng, h, text[k], indels, splice)
            if s is None:
                return None
            made[k] = len(range(EVERY_SUB // 3, len(text[k]), EVERY_SUB)) + indels
        else:
            s = bytearray(text[k])
            if npat:
                s[12::13] = b"N" * len(s[12::13])
            elif subs and rng.integers(0, 4) == 0:
                at = int(rng.integers(0, len(s)))
                s[at] = rng.choice([c for c in b"ACGT" if c != s[at]])
                made[k] = 1
            if shift:
                grow = int(rng.integers(0, 2))
                for _ in range(shift):
                    at = int(rng.integers(len(s) // 3, 2 * len(s) // 3))
                    if grow:
                        s.insert(at, int(rng.choice(list(b"ACGT"))))
                    else:
                        del s[at]
                made[k] = shift
            if k == 0 and pre:
                s = bytearray(letters(rng, pre)) + s
            if k == 1 and post:      # an N first: behind a row's last symbol a seed runs on by any letter (the restart of the search at
                s = s + bytearray(b"N" + letters(rng, post - 1))       # the last node), and no row spells such a seed
            s = bytes(s)
            if n_seeds(h, s) == 0:
                return None
        mates.append(s)
    reads, truth = [mates[0], rc(mates[1])], [(r, a, l1, 0), (r, a + f - l2, l2, 1)]
    swap = cand is not None and cand >= 2
    if swap:
        reads, truth, made = reads[::-1], truth[::-1], made[::-1]
    return SimpleNamespace(kind=kind, reads=reads, truth=truth, frag=(r, a, f), cand=cand, bad=None if dam is None else dam ^ swap, made=made)


def private_sites(A, pick, founder, rows):
    """(row, column) where a row of `rows` has a symbol that no other row copying `founder` has there."""
    mine = np.flatnonzero(pick == founder)
    out = []
    for r in rows:
        others = [q for q in mine.tolist() if q != r]
        for x in np.flatnonzero((A[others] != A[r]).all(axis=0) & (A[r] != GAP)).tolist():
            out.append((r, x))
    return out


def fill(rng, count, draw):
    out = []
    for i in range(100 * count):
        if len(out) == count:
            return out
        p = draw(len(out), i)
        if p is not None:
            out.append(p)
    raise AssertionError("the construction does not find its pairs")


@functools.lru_cache(maxsize=None)
def fragments_a():
    """Input A -> (A, reads, pairs): reads 2p and 2p + 1 are the mates of pairs[p] (see pair_of; a degenerate pair has no fragment)."""
    h = host("a")
    A, pick, _ = MS.founders_msa()
    G, rm = h.G, h.rm
    m = len(G)
    rng = np.random.default_rng(71)
    at = lambda r, x: int((A[r, :x] != GAP).sum())      # noqa: E731          offset of column x in the text of row r
    row = lambda: int(rng.integers(0, m))      # noqa: E731
    mate = lambda: int(rng.integers(50, 121))      # noqa: E731
    extent = lambda: int(rng.integers(150, 401))      # noqa: E731
    sib = [r for r in range(m) if pick[r] == pick[EARLY] and r != EARLY][:3]
    out = []

    def plain(i, _):
        r, f = row(), extent()
        return pair_of(rng, h, "plain", r, int(rng.integers(0, len(G[r]) - f + 1)), f, mate(), mate(), i % 4,
                       indels=int(rng.integers(1, 4)) if i % 3 == 0 else 0)
    out += fill(rng, N_PLAIN, plain)

    def tier(i, _):      # the damaged mate of a tier's length, 20 .. 50 symbols, a partner of 60
        k = TIER_LENGTHS[i // 4] if i < 4 * len(TIER_LENGTHS) else 1025
        r, f = row(), k + 60 + int(rng.integers(20, 51))
        if len(G[r]) < f:
            return None
        cand = i % 4
        return pair_of(rng, h, "tiers", r, int(rng.integers(0, len(G[r]) - f + 1)), f, *((60, k) if cand in (0, 2) else (k, 60)), cand)
    out += fill(rng, 4 * len(TIER_LENGTHS) + 1, tier)

    def first(i, _):
        return pair_of(rng, h, "first", row(), i % 12, extent(), mate(), mate(), i % 4)
    out += fill(rng, N_FIRST, first)

    def last(i, j):      # among them the row that ends early and three rows that copy its founder
        r, f = ([EARLY] + sib)[i % 6] if i % 6 < 4 else row(), extent()
        return pair_of(rng, h, "last", r, len(G[r]) - (i + j) % 12 - f, f, mate(), mate(), i % 4)
    out += fill(rng, N_LAST, last)

    def pre(i, j):       # x_1 - q_1 < 0: random symbols before a forward mate that begins in symbols 0 .. 2
        return pair_of(rng, h, "pre", row(), (i + j) % 3, extent(), mate(), mate(), (0, 2)[i % 2], pre=3 + i % 6)
    out += fill(rng, N_PRE, pre)

    def post(i, j):      # x_last + L - q_last > |G_r|: random symbols past the row's end
        r, f = sib[i % 6] if i % 6 < 3 else row(), extent()
        return pair_of(rng, h, "post", r, len(G[r]) - f, f, mate(), int(rng.integers(30, 46)), (1, 3)[i % 2], subs=0, post=3 + (i + j) % 6)
    out += fill(rng, N_POST, post)

    site = [at(EARLY, x) for _, x in private_sites(A, pick, pick[EARLY], [EARLY])][-2:]      # the two last private symbols of the row that ends early

    def early(i, j):     # the chained mate over a private symbol of the row that ends early: no other row carries it
        end = len(G[EARLY])
        if i % 2 == 0:   # a forward chained mate over both symbols: the window runs into the row's end
            l1 = int(rng.integers(70, 81))
            a = int(rng.integers(site[1] - l1 + 14, site[0] - 13))
            return pair_of(rng, h, "early", EARLY, a, int(rng.integers(150, end - a + 1)), l1, mate(), (0, 2)[(i // 2) % 2], subs=0)
        l2 = end - site[1] + int(rng.integers(14, 30))          # a reverse chained mate from before the last symbol to the row's end, and past it
        f = l2 + int(rng.integers(60, 200))
        return pair_of(rng, h, "early", EARLY, end - f, f, mate(), l2, (1, 3)[(i // 2) % 2], subs=0, post=3 + (i + j) % 6)
    out += fill(rng, N_EARLY, early)

    ten = np.flatnonzero(pick == 10).tolist()
    sites = private_sites(A, pick, 10, [r for r in ten if r >= 128])

    def high(i, j):      # rows that copy founder 10; every second one over a private symbol of a row >= 128: no smaller row carries it
        cand, lc, lo = i % 4, mate(), mate()
        f = extent()
        if i % 2:
            r, x = sites[(i // 2 + j) % len(sites)]
            s = at(r, x) - int(rng.integers(14, lc - 14))       # the chained mate begins here: the symbol well inside it
        else:
            r = ten[(i // 2 + j) % len(ten)]
            s = int(rng.integers(0, len(G[r]) - f))
        a = s if cand in (0, 2) else s + lc - f                   # the chained mate is the forward one for 0 and 2
        return pair_of(rng, h, "high", r, a, f, *((lc, lo) if cand in (0, 2) else (lo, lc)), cand, subs=0)
    out += fill(rng, N_HIGH, high)

    def block(i, _):     # a forward chained mate that begins at p(r, j), one symbol before it, one after it
        r, f = int(rng.integers(0, 10)), extent()
        j = int(rng.integers(1, len(h.b)))
        return pair_of(rng, h, "block", r, rm.p[r][j] + i % 3 - 1, f, mate(), mate(), (0, 2)[(i // 3) % 2], subs=0)
    out += fill(rng, N_BLOCK, block)

    def abut(i, _):      # extent max_insert, and one more; both mates exact apart from the damage
        r, f = int(rng.integers(0, 10)), NATURAL[1] + i % 2
        return pair_of(rng, h, "abut" if i % 2 == 0 else "abut1", r, int(rng.integers(0, len(G[r]) - f + 1)), f, ABUT_MATE, ABUT_MATE,
                       (i // 2) % 4, subs=0)
    out += fill(rng, N_ABUT, abut)

    def over(i, _):
        r, f = row(), NATURAL[1] + int(rng.integers(13, 41))
        return pair_of(rng, h, "over", r, int(rng.integers(0, len(G[r]) - f + 1)), f, mate(), mate(), i % 4)
    out += fill(rng, N_OVER, over)

    def both(i, _):      # both mates chain: exact; one with a substitution in its first symbols; both a piece and its reverse complement
        r, f = row(), extent()
        a = int(rng.integers(0, len(G[r]) - f + 1))
        p = pair_of(rng, h, "both", r, a, f, mate(), mate(), None, subs=0)
        if p is not None and i % 3 == 1:
            k = (i // 3) % 2
            s = bytearray(p.reads[k])
            q = int(rng.integers(3, 11))
            s[q] = rng.choice([c for c in b"ACGT" if c != s[q]])
            p.reads[k], p.kind = bytes(s), "both_sub"
        if p is not None and i % 3 == 2:
            k1, k2 = int(rng.integers(25, 31)), int(rng.integers(25, 31))
            x, y = G[r][a:a + k1], G[r][a + f - k2:a + f]
            p.reads, p.truth, p.kind = [x + rc(x), y + rc(y)], [None, None], "both_inv"
        if p is not None and (i // 2) % 2:
            p.reads, p.truth = p.reads[::-1], p.truth[::-1]
        return p
    out += fill(rng, N_BOTH, both)

    def chance(i, _):    # a damaged mate with 16 symbols of another place: a seed and a chain elsewhere
        r, f, q = row(), extent(), row()
        far = int(rng.integers(0, len(G[q]) - 16))
        a = int(rng.integers(0, len(G[r]) - f + 1))
        if abs(far - a) < 600:
            return None
        p = pair_of(rng, h, "chance", r, a, f, mate(), mate(), i % 4, splice=G[q][far:far + 16])
        return p
    out += fill(rng, N_CHANCE, chance)

    def norow(i, _):     # the N pattern of test_pairs_scale in the partner: every seed picks its smallest place on its own
        r, f = row(), extent()
        return pair_of(rng, h, "no_row", r, int(rng.integers(0, len(G[r]) - f + 1)), f, mate(), mate(), i % 4, npat=True)
    out += fill(rng, N_NOROW, norow)

    def shifted(i, _):   # the partner's last anchor off its first one's diagonal: fe is not fs + L
        r, f = row(), extent()
        return pair_of(rng, h, "shift", r, int(rng.integers(0, len(G[r]) - f + 1)), f, int(rng.integers(70, 121)), int(rng.integers(70, 121)), i % 4,
                       subs=0, shift=1 + i % 3)
    out += fill(rng, N_SHIFT, shifted)

    out = [out[j] for j in rng.permutation(len(out)).tolist()]
    pairs, d = [], 0
    while out:
        if len(pairs) % EVERY == EVERY - 1:
            r, f = row(), extent()
            p = pair_of(rng, h, "plain", r, int(rng.integers(0, len(G[r]) - f + 1)), f, mate(), mate(), None, subs=0)
            if p is None:
                continue
            x, y = p.reads
            q = (r + 100) % m
            two = [[b"", y], [x, b"N" * 30], [x, x], [x, rc(x)], [x, rc(G[q][-40:])]][d % 5]
            pairs.append(SimpleNamespace(kind=("empty", "all_n", "identical", "own_rc", "far")[d % 5], reads=two, truth=[None, None], frag=None,
                                         cand=None, bad=None, made=[0, 0]))
            d += 1
        else:
            pairs.append(out.pop())
    return A, [s for p in pairs for s in p.reads], pairs


@functools.lru_cache(maxsize=None)
def fragments_b():
    """Input B: the forward mate exact in the private flank of the segment or of its first copy, the reverse mate damaged, cut
    from the conserved stretch TIE whose text stands at both loci."""
    h = host("b")
    A, loci, _ = QS.duplications_msa()
    rng = np.random.default_rng(72)
    at = lambda r, x: int((A[r, :x] != GAP).sum())      # noqa: E731

    def draw(i, _):
        x0 = loci[("segment", "copy1")[i % 2]][0]
        r, l1, l2 = int(rng.integers(0, len(A))), int(rng.integers(40, 61)), int(rng.integers(40, 61))
        s, e = int(rng.integers(0, FLANK - l1 + 1)), int(rng.integers(TIE[0] + l2, TIE[1] + 1))
        a = at(r, x0 - FLANK + s)
        return pair_of(rng, h, ("segment", "copy1")[i % 2], r, a, at(r, x0 + e) - a, l1, l2, (0, 2)[(i // 2) % 2], subs=0)
    pairs = fill(rng, N_B, draw)
    return A, [s for p in pairs for s in p.reads], pairs


def tool_pairs():
    """The pairs of input A without an empty mate: fbg_locate reads tokens."""
    return [p for p in fragments_a()[2] if p.reads[0] and p.reads[1]]


SOURCES = {"a": lambda: fragments_a()[2], "b": lambda: fragments_b()[2], "tool": tool_pairs}


@functools.lru_cache(maxsize=None)
def cpu(which="a"):
    """The whole CPU pipeline of an input up to the plain chains, by test_mapping_scale.cpu, and what the tests ask of the pairs."""
    pairs = SOURCES[which]()
    A = host("b" if which == "b" else "a").A
    c = MS.cpu("pair_align_" + which, cap=CAP_B if which == "b" else CAP_A, band=BAND,
               source=lambda: (A, [s for p in pairs for s in p.reads], [t for p in pairs for t in p.truth], 0))
    c.which, c.pairs = which, pairs
    c.loci = QS.duplications_msa()[1] if which == "b" else None
    n = len(c.reads)
    c.bad = [2 * p + x.bad for p, x in enumerate(c.pairs) if x.bad is not None]            # the damaged given reads
    c.damaged = np.zeros(2 * n, dtype=np.uint8)
    c.damaged[c.bad] = 1
    c.damaged[[v + n for v in c.bad]] = 1
    return c


def selection(c, name):
    """None; all ones; the damaged reads on both strands; a seeded quarter of the virtual reads."""
    V = 2 * len(c.reads)
    if name is None:
        return None
    if name == "ones":
        return np.ones(V, dtype=np.uint8)
    if name == "damaged":
        return c.damaged
    return (np.random.default_rng(73).random(V) < 0.25).astype(np.uint8)


# ---- the models ---------------------------------------------------------------------------------------------------------

ALIGN = TA.cached(TA.fast_align)            # one memo of alignments by (read, window) for every run of every mode
CACHE = {}                                  # pairs_model's anchors by virtual read, per input


@functools.lru_cache(maxsize=None)
def chains(which, mode, ins):
    """The chains the rescue runs on: chain_model's, byrow_model's, or the chains pairs_model adopts at these insert bounds;
    with the rows that carry them."""
    c = cpu(which)
    if mode == "plain":
        return c
    if mode == "by_row":
        return BM.by_row(c, BAND, 0, BYROW_MAX)
    m = PM.solve(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, c.chain_off, c.score, c.anchor_place, c.anchor_seed, BAND,
                 ins[0], ins[1], CACHE.setdefault(which, {}))
    m.chain_sets = RM.chain_rows(c.rm.m, c.sets, m.chain_off, m.anchor_place)[3]
    return m


@functools.lru_cache(maxsize=None)
def model(which="a", mode="plain", ins=NATURAL, max_edits=NONE, max_window=0, sel=None):
    c = cpu(which)
    ch = chains(which, mode, ins if mode == "adopt" else None)
    return PA.solve(c.rm, c.vreads, ch.chain_off, ch.score, ch.anchor_place, ch.anchor_seed, ch.chain_sets, c.q_start, c.start_src,
                    c.start_dst, c.start_offset, ins[0], ins[1], max_edits, max_window, selection(c, sel), align=ALIGN)


def raw_ends(c, ch, v, r, first_only=False):
    """x_1 - q_1 and x_last + L - q_last of the chain of v on row r, before the clamps (first_only: both from the first anchor)."""
    rm = c.rm
    o0, o1 = int(ch.chain_off[v]), int(ch.chain_off[v + 1])
    x = []
    for o in (o0, o0 if first_only else o1 - 1):
        g, t = int(ch.anchor_place[o]), int(ch.anchor_seed[o])
        u, off = rm.node_and_offset(int(c.start_src[g]), int(c.start_dst[g]), int(c.start_offset[g]))
        x.append(rm.p[r][rm.block_of[u]] + off - int(c.q_start[t]))
    return x[0], x[1] + len(c.vreads[v])


def valid_candidates(c, ch, m, p):
    """[(i, score)] of the valid candidates of pair p."""
    n = len(c.reads)
    return [(i, int(ch.score[v]) + len(c.vreads[w]) - int(m.edits[w])) for i, (v, w) in enumerate(PA.candidates(p, n))
            if int(m.insert[w]) != NONE]


def facts():
    """Everything test_inputs_are_what_they_claim asserts of input A, measured on the models."""
    c = cpu()
    n, P = len(c.reads), len(c.pairs)
    rm = c.rm
    m = model()
    out = dict(pairs=P, virtual_reads=2 * n, kinds={k: sum(p.kind == k for p in c.pairs) for k in sorted({p.kind for p in c.pairs})})
    out["tier_lengths"] = {k: sum(p.kind == "tiers" and len(p.reads[p.bad]) == k for p in c.pairs) for k in TIER_LENGTHS + (1025,)}
    out["tier_directions"] = sorted({p.cand for p in c.pairs if p.kind == "tiers"})
    out["with_indels"] = sum(p.bad is not None and p.made[p.bad] > len(range(EVERY_SUB // 3, p.truth[p.bad][2], EVERY_SUB)) for p in c.pairs)
    # the windows of the default run at NATURAL
    f = dict(forward_cut_by_row_end=0, reverse_from_0=0, clamp_fs=0, clamp_fe=0, last_cell_without_node=0, clamp_fe_without_node=0, row64=0, row128=0,
             at_block=0, before_block=0, after_block=0, indel_span=0, off_diagonal=0, words={1: 0, 2: 0, 3: 0, 4: 0}, lds=0)
    starts = [set(rm.p[r][1:]) for r in range(rm.m)]
    for w in range(2 * n):
        if m.windows[w] is None:
            continue
        v = PM.partner(w, n)
        r, fs, fe = m.frag[v]
        w0, w1 = m.windows[w]
        glen = len(rm.G[r])
        x1, x2 = raw_ends(c, c, v, r)
        nonode = rm.node_of[r][-1] is None
        f["forward_cut_by_row_end"] += v < n and fs + NATURAL[1] > glen
        f["reverse_from_0"] += v >= n and fe < NATURAL[1]
        f["clamp_fs"] += x1 < 0
        f["off_diagonal"] += x2 - x1 != len(c.vreads[v])
        f["clamp_fe"] += x2 > glen
        f["last_cell_without_node"] += nonode
        f["clamp_fe_without_node"] += nonode and x2 > glen
        f["row64"] += r >= 64
        f["row128"] += r >= 128
        if v < n:
            f["at_block"] += w0 in starts[r]
            f["before_block"] += w0 + 1 in starts[r]
            f["after_block"] += w0 - 1 in starts[r] and w0 > 0
        if m.status[w] == "aligned":
            k = len(c.vreads[w])
            f["indel_span"] += int(m.t_end[w]) - int(m.t_start[w]) != k
            if k <= 256:
                f["words"][(k + 63) // 64] += 1
            else:
                f["lds"] += 1
    out["windows"] = f
    return out


def accepted(m):
    return m.insert != NONE


def pair_facts():
    """What the picks, the selections and the other runs are asserted to hold, measured on the models of input A."""
    c = cpu()
    n, P = len(c.reads), len(c.pairs)
    default, ones, dm = model(), model(sel="ones"), model(sel="damaged")
    out = {}
    three = tie = other = 0
    for p in range(P):
        ok = valid_candidates(c, c, ones, p)
        if ok:
            top = max(sc for _, sc in ok)
            best = [i for i, sc in ok if sc == top]
            assert best[0] == ones.which[p] and top == ones.pair_score[p]
            three += len(ok) >= 3
            tie += len(best) > 1
            other += best[0] != ok[0][0]
        else:
            assert ones.which[p] == PA.NO_PAIR
    out["three_valid"], out["tie_smaller_wins"], out["winner_not_smallest_valid"] = three, tie, other
    out["which_damaged"] = [int((dm.which == i).sum()) for i in range(4)]
    chance = [2 * p + x.bad + s * n for p, x in enumerate(c.pairs) if x.kind == "chance" for s in (0, 1)]
    out["chance_with_chain"] = sum(int(c.chain_off[v + 1]) > int(c.chain_off[v]) for v in chance)
    out["chance_differs"] = sum(int(default.edits[v]) != int(dm.edits[v]) for v in chance)
    out["all_n"] = sum(len(c.vreads[w]) == 30 and set(c.vreads[w]) == {ord("N")} and default.status[w] == "aligned" and int(default.edits[w]) == 30
                       and int(default.t_start[w]) == int(default.t_end[w]) == default.windows[w][0] for w in range(2 * n))
    out["median_edits"] = float(np.median(default.edits[accepted(default)]))
    narrow = model(ins=NARROW)
    out["narrow"] = (int(accepted(narrow).sum()), int(accepted(default).sum()), narrow.stats["rejected_insert"])
    quarter = selection(c, "quarter")
    out["quarter_partner_unchained"] = sum(bool(quarter[w]) and int(c.chain_off[PM.partner(w, n) + 1]) == int(c.chain_off[PM.partner(w, n)])
                                           for w in range(2 * n))
    # the abut group at min_insert == max_insert, with the edit bound of its substitutions and without
    uncut = model(ins=PLUS, max_edits=0)           # max_insert + 1 holds the longer fragments: the edits of a mate that is not cut
    for name, m in (("abut_bounded", model(ins=ABUT, max_edits=ABUT_EDITS, sel="damaged")), ("abut_unbounded", model(ins=ABUT))):
        got = dict(abut=0, abut1=0, abut_on_last_column=0, abut_forward=0, abut1_edits_over=0, abut1_cut_costs_one=0)
        for p, x in enumerate(c.pairs):
            if x.kind in ("abut", "abut1"):
                for w in (2 * p + x.bad, 2 * p + x.bad + n):
                    if int(m.insert[w]) != NONE:
                        got[x.kind] += 1
                        assert int(m.insert[w]) == ABUT[1]
                        if x.kind == "abut" and PM.partner(w, n) < n:
                            got["abut_forward"] += 1
                            got["abut_on_last_column"] += int(m.t_end[w]) == m.windows[w][1]
                        got["abut1_edits_over"] += x.kind == "abut1" and int(m.edits[w]) > ABUT_EDITS
                        got["abut1_cut_costs_one"] += x.kind == "abut1" and int(m.edits[w]) == int(uncut.edits[w]) + 1
                        assert x.kind == "abut" or int(uncut.edits[w]) <= int(m.edits[w]) <= int(uncut.edits[w]) + 1
        out[name] = got
    bound = model(max_edits=MEDIAN_EDITS, sel="quarter")
    out["rejected_edits_at_median"] = bound.stats["rejected_edits"]
    over = [2 * p + x.bad + s * n for p, x in enumerate(c.pairs) if x.kind == "over" for s in (0, 1)]
    plain = [2 * p + x.bad + s * n for p, x in enumerate(c.pairs) if x.kind == "plain" for s in (0, 1)]
    mean = lambda vs: float(np.mean([int(default.edits[v]) / len(c.vreads[v]) for v in vs if default.status[v] == "aligned"]))      # noqa: E731
    out["edits_per_symbol_over_and_plain"] = (round(mean(over), 3), round(mean(plain), 3))
    seen = dict.fromkeys(PA.STATS, 0)
    for run in RUNS:
        for k, x in model("a", "plain", *run).stats.items():
            seen[k] = max(seen[k], x)
    out["largest_counters"] = seen
    out["ones"] = dict(ones.stats)
    return out


def cut_columns(c, x):
    """The MSA columns the damaged mate of pair x was cut from."""
    row, a, ln, _ = x.truth[x.bad]
    return int(c.cols[row][a]), int(c.cols[row][a + ln - 1]) + 1


def at_both_loci(c, x):
    """Input B: the text the damaged mate was cut from stands in the same row at the same columns of the other locus."""
    row = x.truth[x.bad][0]
    t0, t1 = cut_columns(c, x)
    x0, y0 = c.loci[x.kind][0], c.loci["copy1" if x.kind == "segment" else "segment"][0]
    return c.A[row, t0:t1].tobytes() == c.A[row, t0 - x0 + y0:t1 - x0 + y0].tobytes()


def check_truth(c, res, ins=NATURAL):
    """The ground truth: for every simulated pair with a damaged mate that the run accepted, [t_start, t_end) of the mate's
    row, in MSA columns, meets the columns the mate was cut from.  res: row, edits, t_start, t_end, insert per virtual read, of
    the model or of the engine, from a run that selects the damaged reads.  Excused, in this order: a fragment longer than
    max_insert; a partner without a carrying row (or without a chain); a mate that was not accepted; an interval elsewhere
    in the window with no more edits than the damage made (checked: the text stands there as well as at its place)
    -> the counts."""
    n = len(c.reads)
    out = dict(simulated=0, judged=0, over=0, no_row=0, not_accepted=0, second=0, both_loci=0)
    for p, x in enumerate(c.pairs):
        if x.bad is None:
            continue
        out["simulated"] += 1
        w = 2 * p + x.bad + n * x.truth[x.bad][3]            # the strand the mate was cut from
        if x.frag[2] > ins[1]:
            out["over"] += 1
        elif int(res.row[w]) == NONE:
            out["no_row"] += 1
        elif int(res.insert[w]) == NONE:
            out["not_accepted"] += 1
        else:
            r = int(res.row[w])
            lo, hi = int(c.cols[r][int(res.t_start[w])]), int(c.cols[r][int(res.t_end[w]) - 1]) + 1
            t0, t1 = cut_columns(c, x)
            if not (lo < t1 and t0 < hi) and int(res.edits[w]) <= x.made[x.bad]:
                out["second"] += 1
                continue
            assert lo < t1 and t0 < hi, (c.which, p, x.kind, x.frag, (t0, t1), (lo, hi), int(res.edits[w]), x.made)
            out["judged"] += 1
            if c.which == "b":
                # the window holds one locus: the mate lies at its partner's, not at the other copy
                x0, x1 = c.loci[x.kind]
                assert x0 - FLANK <= lo and hi <= x1, (p, x.kind, (lo, hi))
                out["both_loci"] += at_both_loci(c, x)
    return out


def truth_holds(a, b):
    """The conditions of the ground truth on the counts of inputs A and B."""
    excused = sum(t[k] for t in (a, b) for k in ("over", "no_row", "not_accepted", "second"))
    simulated = a["simulated"] + b["simulated"]
    assert all(t["judged"] + t["over"] + t["no_row"] + t["not_accepted"] + t["second"] == t["simulated"] for t in (a, b))
    assert 4 * excused <= simulated, (a, b)
    assert b["both_loci"] >= min(100, 2 * b["simulated"] // 3), b


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_inputs_are_what_they_claim():
    """Everything the docstring counts, on the models alone; each floor about half of the measured figure."""
    c, f, g = cpu(), facts(), pair_facts()
    print("pair_align_scale:", f, g)
    n, P, V = len(c.reads), len(c.pairs), 2 * len(c.reads)
    m = model()
    assert c.A.shape == (200, 1500) and len(c.b) > 100 and len(c.rm.G[EARLY]) == 1280 and c.rm.node_of[EARLY][-1] is None
    # the launch shapes: a partial last workgroup and a partial last wave in every kernel, 17 workgroups or more of k_pl_window
    assert f["pairs"] == P and V == 4 * P and V % 256 and P % 64 and V >= 4096 and (V + 1 + 255) // 256 >= 17 and (P + 255) // 256 >= 4
    assert 1000 <= P <= 1250
    # the groups
    k = f["kinds"]
    assert (k["plain"], k["tiers"], k["first"], k["last"], k["pre"], k["post"], k["early"]) == (N_PLAIN, 4 * len(TIER_LENGTHS) + 1, N_FIRST, N_LAST,
                                                                                              N_PRE, N_POST, N_EARLY)
    assert (k["high"], k["block"], k["abut"], k["abut1"], k["over"], k["chance"], k["no_row"]) == (N_HIGH, N_BLOCK, N_ABUT // 2, N_ABUT // 2,
                                                                                                   N_OVER, N_CHANCE, N_NOROW)
    assert k["shift"] == N_SHIFT
    assert k["both"] + k["both_sub"] + k["both_inv"] == N_BOTH
    assert min(k[d] for d in ("empty", "all_n", "identical", "own_rc", "far")) >= 4
    assert all(c.pairs[p].frag is None for p in range(EVERY - 1, P, EVERY)) and sum(x.frag is None for x in c.pairs) == P // EVERY
    assert all(f["tier_lengths"][x] >= 3 for x in TIER_LENGTHS) and f["tier_lengths"][1025] == 1 and f["tier_directions"] == [0, 1, 2, 3]
    per_cand = [sum(x.cand == i for x in c.pairs) for i in range(4)]
    assert max(per_cand) - min(per_cand) <= 40, per_cand           # spread evenly over the four candidate numbers
    assert 3 * f["with_indels"] >= N_PLAIN and f["windows"]["indel_span"] >= 200
    # a damaged mate, other than the chance group's, has no seed and no chain on either strand; the chance group's have both
    for p, x in enumerate(c.pairs):
        if x.bad is not None:
            R = 2 * p + x.bad
            seeds = [int(c.seed_off[v + 1]) - int(c.seed_off[v]) for v in (R, R + n)]
            chained = [int(c.chain_off[v + 1]) - int(c.chain_off[v]) for v in (R, R + n)]
            assert (sum(seeds) > 0) == (x.kind == "chance") and (sum(chained) > 0 or x.kind != "chance"), (p, x.kind, seeds, chained)
            text = c.rm.G[x.truth[x.bad][0]][x.truth[x.bad][1]:][:x.truth[x.bad][2]]
            assert AM.lev(rc(c.reads[R]) if x.truth[x.bad][3] else c.reads[R], text) <= x.made[x.bad] + (16 if x.kind == "chance" else 0)
    # the ends of the rows, the high rows, the block starts, the tiers: on the windows of the default run at NATURAL
    w = f["windows"]
    assert w["forward_cut_by_row_end"] >= 28 and w["reverse_from_0"] >= 22 and w["clamp_fs"] >= 7 and w["clamp_fe"] >= 9, w
    assert w["last_cell_without_node"] >= 3 and w["clamp_fe_without_node"] >= 2 and w["off_diagonal"] >= FLOOR["off_diagonal"], w
    assert w["row64"] >= 100 and w["row128"] >= 47 and min(w["at_block"], w["before_block"], w["after_block"]) >= 14, w
    assert w["words"][1] >= 113 and w["words"][2] >= 280 and w["words"][3] >= 4 and w["words"][4] >= 3 and w["lds"] >= 7, w
    t = model(ins=TIERS, sel="damaged")
    got = {x: 0 for x in TIER_LENGTHS}
    for p, x in enumerate(c.pairs):
        if x.kind == "tiers":
            for v in (2 * p + x.bad, 2 * p + x.bad + n):
                if t.status[v] == "aligned":
                    got[len(c.vreads[v])] += 1
    print("tiers aligned at their own max_insert:", got, t.stats)
    assert all(x >= 1 for x in got.values()) and sum(got.values()) >= 19 and t.stats["too_long"] == 1, got
    # the picks under the all-ones mask; the selections
    assert g["three_valid"] >= FLOOR["three_valid"] and g["tie_smaller_wins"] >= FLOOR["tie"] and g["winner_not_smallest_valid"] >= FLOOR["other"], g
    assert min(g["which_damaged"]) >= 100, g
    assert g["chance_with_chain"] >= N_CHANCE and g["chance_differs"] >= FLOOR["chance"] and g["all_n"] >= 2, g
    assert g["quarter_partner_unchained"] >= 390
    # the conditions that keep the tests from turning hollow
    ones = g["ones"]
    assert 5 * ones["no_row"] <= 2 * ones["selected"] and ones["aligned"] >= 1000, ones
    assert all(x > 0 for x in g["largest_counters"].values()), g["largest_counters"]
    # NARROW rejects about half on the insert alone; the bound on the edits is near the median and rejects
    narrow, natural, rejected = g["narrow"]
    assert 0.3 * natural <= natural - narrow <= 0.7 * natural and natural - narrow <= rejected, g["narrow"]
    assert abs(g["median_edits"] - MEDIAN_EDITS) <= 2 and g["rejected_edits_at_median"] >= FLOOR["rejected_edits"], g
    assert g["edits_per_symbol_over_and_plain"][0] > g["edits_per_symbol_over_and_plain"][1]
    # at min_insert == max_insert and the edits of the damage, a fragment of max_insert symbols is accepted, none of one more
    ab, un = g["abut_bounded"], g["abut_unbounded"]
    # (a window that cuts one symbol off a mate still holds an alignment that ends on its last column, of one more edit or,
    # for a few, of as many: pair_facts asserts that; so the bound, which only a few mates of one symbol more pass)
    assert ab["abut"] >= FLOOR["abut"] and ab["abut_on_last_column"] == ab["abut_forward"] >= FLOOR["abut"] // 2, ab
    assert ab["abut1"] <= ab["abut"] // 4 and un["abut1"] > ab["abut1"] and 4 * un["abut1_cut_costs_one"] >= 3 * un["abut1"], (ab, un)
    # nothing at (0, 0); every window to the row's end at (0, 2^64 - 1)
    z = model(ins=NOTHING, sel="ones")
    assert z.stats["aligned"] == 0 and z.stats["empty"] == z.stats["selected"] - z.stats["no_row"] > 0 and (z.which == PA.NO_PAIR).all()
    wide = model(ins=WIDE)
    for v in range(V):
        if wide.windows[v] is not None:
            r, fs, fe = wide.frag[PM.partner(v, n)]
            assert wide.windows[v] == ((fs, len(c.rm.G[r])) if PM.partner(v, n) < n else (0, fe))
    # input B: two loci, one text
    b = cpu("b")
    assert len(b.pairs) == N_B and sum(at_both_loci(b, x) for x in b.pairs) >= 100
    for p, x in enumerate(b.pairs):
        R = 2 * p + x.bad
        assert b.seed_off[R] == b.seed_off[R + 1] and b.seed_off[R + len(b.reads)] == b.seed_off[R + len(b.reads) + 1]


FLOOR = dict(three_valid=7, tie=5, other=27, chance=14, rejected_edits=60, abut=16, off_diagonal=7)      # about half of what is measured


SMALL = (0, 128)                                     # windows of 128 symbols: with a read of up to 128 at most 2^14 cells, align_model's literal form


def test_model_row_form_agrees_with_the_literal_form():
    """fast_align, the DP a row at a time, against align_model.align cell by cell, on reads and windows of the inputs."""
    rng = np.random.default_rng(74)
    done = 0
    for which in ("a", "b"):
        c, m = cpu(which), model(which, ins=SMALL, sel="damaged")
        n = len(c.reads)
        ws = [w for w in range(2 * n) if m.status[w] == "aligned" and len(c.vreads[w]) * (m.windows[w][1] - m.windows[w][0]) <= AM.LITERAL_CELLS]
        for w in rng.permutation(ws)[:150].tolist():
            r = m.frag[PM.partner(w, n)][0]
            W = c.rm.G[r][m.windows[w][0]:m.windows[w][1]]
            assert len(c.vreads[w]) * len(W) <= 1 << 14 and TA.fast_align(c.vreads[w], W) == AM.align(c.vreads[w], W), (which, w)
            done += 1
    assert done >= 200, done


@functools.lru_cache(maxsize=None)
def truth_of_the_models():
    return {(which, mode): check_truth(cpu(which), model(which, mode, sel="damaged")) for which in ("a", "b") for mode in ("plain", "by_row")}


def test_model_finds_the_fragments():
    """The ground truth at NATURAL under the damaged mask.  Every judged pair is right after plain chains and after chains by
    row; the share of excused pairs is asserted on the chains by row, each of which has a row (after plain chains a quarter
    of the partners have none: see the docstring)."""
    t = truth_of_the_models()
    print("truth:", t)
    truth_holds(t["a", "by_row"], t["b", "by_row"])
    assert t["a", "plain"]["judged"] >= 500 and t["b", "plain"]["judged"] >= 100


# ---- planted errors, on the CPU -----------------------------------------------------------------------------------------

PLANTS = ("k_pl_pick: sc >= best for sc > best", "k_pl_pick: got <= min_insert for <", "k_pl_pick: e >= max_edits for >",
          "k_pl_pick: L_w taken from v", "k_pl_pick: the insert of odd candidates as te - fs", "pl_partner without the ^ 1 for v >= n",
          "k_pl_frag: fe from the first anchor's record",
          "k_pl_frag: glen without the last label's length", "k_pl_window: the reverse window opened at fs, clamped to the row",
          "k_pl_window: the counters added by wave 0 of a workgroup only", "k_pl_pick: the counters added by wave 0 of a workgroup only")
# the runs the planted errors are tried on: one set of windows (max_insert 448), every selection, both edit bounds, min_insert == max_insert
PLANT_RUNS = tuple(r for r in RUNS if r[0][1] == NATURAL[1] and r[2] == 0)
FIELDS = ("row", "edits", "t_start", "t_end", "insert", "which", "pair_score", "t_lo", "t_hi")


def kernels_restated(c, ch, run, plant=0):
    """k_pl_frag, k_pl_window and k_pl_pick of csrc/pindex_pairs_align.hip once more, lane by lane and with the kernels' own
    unsigned arithmetic, apart from pair_align_model: with plant == 0 it must equal the model; plant = 1 .. 11 makes the
    error PLANTS[plant - 1].  A lane is virtual read w (pair p) and sits in wave (w % 256) // 64 of its workgroup."""
    ins, max_edits, max_window, sel = run
    select, rm = selection(c, sel), c.rm
    n = len(c.reads)
    V, P, mi = 2 * n, n // 2, min(ins[1], PA.CLAMP)
    partner = lambda w: (w ^ 1) + n if w < n else (w - n if plant == 6 else (w - n) ^ 1)      # noqa: E731
    anchored = np.diff(ch.chain_off.astype(np.int64)) > 0
    frag = [(None, 0, 0, 0)] * V
    for v in range(V):
        if anchored[v] and ch.chain_sets[v]:
            r = ch.chain_sets[v][0]
            x1, x2 = raw_ends(c, ch, v, r, first_only=plant == 7)
            glen = rm.p[r][-1] if plant == 8 else len(rm.G[r])
            frag[v] = (r, max(0, x1), min(glen, max(0, x2)), glen)
    out = np.full((5, V), NONE, dtype=np.uint32)
    st = dict.fromkeys(PA.STATS, 0)
    for w in range(V):
        v = partner(w)
        if not anchored[v] or not (bool(select[w]) if select is not None else not anchored[w]):
            continue
        counts = plant != 10 or w % 256 < 64
        st["selected"] += counts
        r, fs, fe, glen = frag[v]
        if r is None:
            st["no_row"] += counts
            continue
        w0, w1 = (fs, min(glen, fs + mi)) if v < n or plant == 9 else (max(0, fe - mi), fe)
        assert 0 <= w0 <= w1 <= len(rm.G[r])                          # every planted window lies in its row
        k = len(c.vreads[w])
        kind = "empty" if k == 0 or w1 == w0 else "too_long" if k > PA.MAX_READ else "too_wide" if max_window and w1 - w0 > max_window else "aligned"
        st[kind] += counts
        out[0, w] = r
        if kind == "aligned":
            e, a, b = ALIGN(c.vreads[w], rm.G[r][w0:w1])
            out[1:4, w] = e, w0 + a, w0 + b
            st["cells"] += counts * k * (w1 - w0)
    which, score, lo, hi = [], [], [], []
    for p in range(P):
        counts = plant != 11 or p % 256 < 64
        best = None
        for i, (v, w) in enumerate(PA.candidates(p, n)):
            if int(out[1, w]) == NONE:
                continue
            _, fs, fe, _ = frag[v]
            e, ts, te = (int(x) for x in out[1:4, w])
            got = (te - fs if i % 2 == 0 or plant == 5 else fe - ts) & 0xffffffff
            if (e >= max_edits) if plant == 3 else (e > max_edits):
                st["rejected_edits"] += counts
            elif (got <= ins[0]) if plant == 2 else (got < ins[0]):
                st["rejected_insert"] += counts
            else:
                out[4, w] = got
                sc = (int(ch.score[v]) + len(c.vreads[v if plant == 4 else w]) - e) & U64
                if best is None or ((sc >= best[1]) if plant == 1 else (sc > best[1])):
                    best = (i, sc) + ((ts, fe) if i % 2 else (fs, te))
        st["pairs"] += counts and best is not None
        best = best if best is not None else (PA.NO_PAIR, 0, NONE, NONE)
        which.append(best[0])
        score.append(best[1] & 0xffffffff)
        lo.append(best[2])
        hi.append(best[3])
    u32 = lambda x: np.array(x, dtype=np.uint32)      # noqa: E731
    return SimpleNamespace(row=out[0], edits=out[1], t_start=out[2], t_end=out[3], insert=out[4], which=np.array(which, dtype=np.uint8),
                           pair_score=u32(score), t_lo=u32(lo), t_hi=u32(hi), stats={k: int(x) for k, x in st.items()})


def differences(got, m):
    """What an exact comparison of a call with the model m would report: per field the entries that differ, and the counters."""
    out = {f: int((getattr(got, f) != getattr(m, f)).sum()) for f in FIELDS}
    out.update({k: (got.stats[k], m.stats[k]) for k in PA.STATS if got.stats[k] != m.stats[k]})
    return {k: x for k, x in out.items() if x}


def test_planted_errors_change_what_the_parity_tests_compare():
    """Each error of PLANTS, made in a restatement of the three kernels, changes an array or a counter that the GPU tests
    compare exactly, on the runs they make; without an error the restatement is the model, entry by entry."""
    c = cpu()
    for run in PLANT_RUNS:
        assert differences(kernels_restated(c, c, run), model("a", "plain", *run)) == {}, run
    for k, name in enumerate(PLANTS, 1):
        seen = {run: differences(kernels_restated(c, c, run, k), model("a", "plain", *run)) for run in PLANT_RUNS}
        print("planted:", name, {(r[0], r[1], r[3]): d for r, d in seen.items() if d})
        assert sum(bool(d) for d in seen.values()) >= 1, name
        # the runs of the batch test, of the one-index test and of the truth test among them, where the error is not about one bound
        if k not in (1, 2, 3):
            assert all(seen[r] for r in PLANT_RUNS if r[0] == NATURAL), (name, seen)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def seeded(pix, c, reads=None):
    """The stranded seeds call of an input; for the whole input the seeds, places and plain chains are the models'."""
    sd = pix.seeds(c.reads if reads is None else reads, min_length=L, max_per_seed=c.cap, msa=True, chain=True, band=BAND, strands=True,
                   rows=True)
    if reads is None:
        assert sd.strands and sd.reads == len(c.reads)
        TR.same_as_cpu(sd, c, c.name)
    return sd


def rescue(pix, c, run, mode="plain", select=None, **kw):
    ins, max_edits, max_window, sel = run
    return pix.chains(band=BAND, pairs=ins, pair_align=True, pair_max_edits=max_edits, pair_max_window=max_window,
                      pair_select=selection(c, sel) if select is None else select, **MODES[mode], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity(engine, mode):
    c = cpu()
    V = 2 * len(c.reads)
    with fbg_options(engine, {"byrow_max": BYROW_MAX}), QS.build(engine, c) as pix:
        seeded(pix, c)
        for run in RUNS:
            want = chains("a", mode, run[0] if mode == "adopt" else None)
            ch = rescue(pix, c, run, mode)
            TP.same_adopted(ch, want, (mode, run, "the chains"))          # first the chains: a mismatch there is not the rescue's
            m = model("a", mode, *run)
            TA.same(ch, m, (mode, run, "python"))
            TA.same_c(TA.c_call(pix, V, run[0], run[1], run[2], selection(c, run[3])), m, (mode, run, "c"))


def as_result(ch):
    return SimpleNamespace(**{g: getattr(ch, f) for f, g in TA.READ_FIELDS + TA.PAIR_FIELDS})


@pytest.mark.gpu
def test_truth_on_what_the_engine_returns(engine):
    got = {}
    for which in ("a", "b"):
        c = cpu(which)
        with fbg_options(engine, {"byrow_max": BYROW_MAX}), QS.build(engine, c) as pix:
            seeded(pix, c)
            for mode in ("plain", "by_row"):
                got[which, mode] = check_truth(c, as_result(rescue(pix, c, (NATURAL, NONE, 0, "damaged"), mode)))
    truth_holds(got["a", "by_row"], got["b", "by_row"])
    assert got == truth_of_the_models()


def pair_view(ch, p, n):
    """What must not depend on the batch pair p arrives in: its pick and the results of its four virtual reads."""
    reads = [2 * p, 2 * p + 1, 2 * p + n, 2 * p + 1 + n]
    return [int(getattr(ch, f)[p]) for f, _ in TA.PAIR_FIELDS] + [int(getattr(ch, f)[v]) for f, _ in TA.READ_FIELDS for v in reads]


def batch_cuts(n):
    """In given reads: 64 pairs (V = 256: the second workgroup of k_pl_window holds the lane of wlen[V] alone), 128 pairs, one pair, the rest."""
    return [0, 128, 384, 386, n]


@pytest.mark.gpu
def test_a_pair_is_independent_of_its_batch(engine):
    c = cpu()
    n = len(c.reads)
    run = (NATURAL, MEDIAN_EDITS, 0, "ones")
    m = model("a", "plain", *run)
    cuts = batch_cuts(n)
    with QS.build(engine, c) as pix:
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            seeded(pix, c, c.reads[a:b])
            parts.append(rescue(pix, c, run, select=np.ones(2 * (b - a), dtype=np.uint8)))
        seeded(pix, c)
        whole = rescue(pix, c, run)
        TA.same(whole, m, "whole")
        for part, a, b in zip(parts, cuts, cuts[1:]):
            assert len(part.mate_which) == (b - a) // 2
            for p in range((b - a) // 2):
                assert pair_view(part, p, b - a) == pair_view(whole, a // 2 + p, n), (a, p)
        total = {k: sum(part.mate_stats[k] for part in parts) for k in PA.STATS}
        assert total == whole.mate_stats == m.stats


@pytest.mark.gpu
def test_one_index_across_large_and_small_calls(engine):
    """The buffers of the rescue state are sized by the large call and reused, the windows' by every call from its scan;
    nothing of an earlier call may show, and the alignment call that shares the prefix table and pa_windows goes between."""
    c = cpu()
    n = len(c.reads)
    run = (NATURAL, NONE, 0, None)
    m = model("a", "plain", *run)
    p = next(p for p in range(len(c.pairs)) if m.which[p] != PA.NO_PAIR and c.pairs[p].kind == "plain")
    inv = [s for x in c.pairs if x.kind == "both_inv" for s in x.reads][:8]
    with QS.build(engine, c) as pix:
        seeded(pix, c)
        first = rescue(pix, c, run)                                   # 1. the whole set
        TA.same(first, m, "first")
        seeded(pix, c, c.reads[2 * p:2 * p + 2])                      # 2. one pair
        one = rescue(pix, c, run)
        assert pair_view(one, 0, 2) == pair_view(first, p, n) and one.mate_stats["pairs"] == 1
        seeded(pix, c, [b"", b"NNN", b"N" * 30, b""])                 # 3. a batch without places: every output at its fill value
        e = rescue(pix, c, run, select=np.ones(8, dtype=np.uint8))
        assert e.mate_which.tolist() == [PA.NO_PAIR] * 2 and e.mate_score.tolist() == [0, 0]
        assert e.mate_lo.tolist() == e.mate_hi.tolist() == [NONE] * 2
        assert all(getattr(e, f).tolist() == [NONE] * 8 for f, _ in TA.READ_FIELDS) and e.mate_stats == dict.fromkeys(PA.STATS, 0)
        seeded(pix, c, inv)                                           # 4. every virtual read has a chain and no mask: nothing is selected
        e = rescue(pix, c, run)
        assert (np.diff(e.chain_off.astype(np.int64)) > 0).all() and e.mate_stats == dict.fromkeys(PA.STATS, 0)
        assert (e.mate_which == PA.NO_PAIR).all() and all((getattr(e, f) == NONE).all() for f, _ in TA.READ_FIELDS)
        seeded(pix, c)                                                # 5. the alignment call on the whole set
        al = pix.chains(band=BAND, align=True)
        again = rescue(pix, c, run, align=True)                       # 6. the whole set again, beside the alignment
        TA.same(again, m, "again")
        for f, _ in TA.READ_FIELDS + TA.PAIR_FIELDS:
            assert np.array_equal(getattr(again, f), getattr(first, f)), f
        for f in ("align_row", "edits", "t_start", "t_end"):
            assert np.array_equal(getattr(again, f), getattr(al, f)), f
        assert (al.edits != NONE).sum() >= 500
        # the widest windows, then the narrowest, then none: the buffer of the windows shrinks after the large call
        for after in ((TIERS, NONE, 0, None), (MINUS, NONE, MINUS[1], None), (NOTHING, NONE, 0, "ones"), run):
            TA.same(rescue(pix, c, after), model("a", "plain", *after), after)


@pytest.mark.gpu
def test_tool_prints_the_rescue_of_the_whole_read_set(engine, tmp_path):
    """One fbg_locate --pair-align run over every pair without an empty mate (the tool reads tokens), and one without the flag."""
    from oracle import pyoracle as O
    c = cpu("tool")
    assert len(cpu().pairs) - 6 <= len(c.pairs) < len(cpu().pairs)
    m = model("tool", "adopt", NATURAL, MEDIAN_EDITS)
    assert m.stats["aligned"] >= 400 and m.stats["rejected_edits"] > 0 and m.stats["pairs"] >= 200
    graph, fasta = str(tmp_path / "g.xgfa"), str(tmp_path / "g.fasta")
    O.write_xgfa(c.A, c.b, graph)
    with open(fasta, "wb") as fh:
        for r, row in enumerate(c.A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))
    args = ["--graph=" + graph, "--msa=" + fasta, "--seeds=%d" % L, "--occurrences=%d" % CAP_A, "--chain=%d" % BAND, "--strands", "--rows",
            "--pairs=%d,%d" % NATURAL]
    data = b"".join(r + b"\n" for r in c.reads)
    base = TC.TL.run_locate(args, data)
    got = TC.TL.run_locate(args + ["--pair-align=%d" % MEDIAN_EDITS], data)
    assert base.returncode == 0 and got.returncode == 0, (base.stderr, got.stderr)
    lines = got.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith(b"Y\t")] == TA.y_lines(m, len(c.reads))
    assert [ln for ln in lines if ln.startswith(b"W\t")] == TA.w_lines(m)
    assert [ln for ln in lines if ln[:2] not in (b"Y\t", b"W\t")] == base.stdout.splitlines()
    assert b"Y\t" not in base.stdout and b"W\t" not in base.stdout and any(ln[:2] in (b"Z\t", b"C\t", b"A\t", b"T\t") for ln in lines)
