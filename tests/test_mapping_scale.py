"""Seeds, MSA coordinates, chains, strands and rows on many rows, blocks and reads in one call: the read-mapping calls of
the pattern index (include/fbg_hip.h; csrc/locate.hip and csrc/pindex_*.hip: k_pr_rows / k_pr_chain, pr_walk, the wave-uniform offset searches,
k_px_revcomp, k_pc_key / k_pc_chain, k_pc_strand) between the toy inputs of test_chains.py, test_chain_edges.py,
test_strands.py and test_rows.py and the workload of scripts/gpu_rows_bench.py.

The checkers are the models those modules use (occ_model, seeds_model, msa_model, chain_model, strand_model, rows_model on
heuristic_model.segmentation_graph), and every comparison with the engine is exact.  Every input is seeded, built here and
shared by the CPU and GPU tests:

  founders   200 rows x 1500 columns, copies of twelve founders with private substitutions, segmented by the min-max-length
             DP, about 4000 simulated reads given on both strands;
  repeats    200 rows; 600 columns of the same construction with a tandem repeat of one 16-symbol unit, 80 copies long, in
             every row, and reads long enough to fill the three chain tiers;
  m16, m17, m128   the construction at m x 300 with five founders: the row counts beside PR_SUB and a full last word.

Constraints of the construction:
  * founder 10 occurs only in rows >= 64 and founder 11 only in rows {3} and [130, 136) (they make the cases of the row
    words), so the first rows are founders 0..9 except row 3, which is founder 11, and founder 10 starts at row 64.
  * 80 copies of a 16-symbol unit are 1280 columns: the repeat is inserted between columns 300 and 301 of the 600, so that
    MSA has 1880 columns.  With max_per_seed = 32 a read needs more than 32 seeds of 32 places to leave the LDS tier, hence
    reads of several hundred symbols with an N every 13th symbol.
  * no row is all gaps across whole blocks and has symbols again behind them: the DP makes one block of such a stretch
    (test_a_row_has_a_node_in_every_block_up_to_its_end).  The nearest input is the row that ends early: its walks pass
    the cells without a node up to the last block.

The reads are simulated: cut from the gap-stripped text of a known row at a known offset, every fourth with one symbol
replaced by N, every third reverse-complemented.  That gives the models a ground truth outside themselves: the strand,
the column of a seed's first symbol, the row among the rows of that place, the column of the chain's first anchor.  The
true row need not be in rows(chain), and that is not asserted: a read that starts inside a node is also spelled from
any other node of the block with the same suffix, the chain may pick that place (ties go to the smallest place), and
rows(chain), the intersection over the anchors by the definition of the header, then leaves the true row out.

The two thresholds of the founders input (more than 5000 seeds, more than 10000 start places) are there to pass many
256-thread workgroups and, presumably, more than one tile of the device scans behind seed_off, start_off and chain_off.
Where a tile of those scans ends has not been measured: the tile boundary is not claimed to be covered."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import chain_model as CM  # noqa: E402
import heuristic_model as HM  # noqa: E402
import msa_model as MM  # noqa: E402
import occ_model as OM  # noqa: E402
import rows_model as RM  # noqa: E402
import seeds_model as SDM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chain_edges as TE  # noqa: E402
import test_rows as TR  # noqa: E402
import test_strands as TS  # noqa: E402
import validate_model as VM  # noqa: E402
from conftest import fbg_options, random_msa  # noqa: E402

NONE = RM.NONE
STRAND_NONE = STM.NONE
GAP = ord("-")
TABLE = STM.default_table()
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)
MIN_LENGTH, CAP, BAND = 12, 32, None
PC_SMALL, PC_LDS = 32, 1024                 # chain_stats(): small_max, lds_max
UNIT, COPIES = b"ACGGTCATTGCAGATC", 80
EARLY = 77                                  # founders: the row that ends early
MS = (16, 17, 128)


# ---- the inputs ---------------------------------------------------------------------------------------------------------

def oracle_boundaries(A):
    from oracle import pyoracle as O
    return [int(x) for x in O.minmax_dp(O.compute_f(A))[2]]


def engine_boundaries(engine, A):
    return [int(x) for x in engine.minmax_dp(engine.elastic_f(A))]


def copies(rng, founders, pick, private=0.002):
    """Row r copies founder pick[r]; then a share `private` of the non-gap cells gets another symbol."""
    A = founders[pick].copy()
    at = np.flatnonzero((A != GAP).ravel() & (rng.random(A.size) < private))
    code = np.searchsorted(ALPHA, A.ravel()[at])
    A.ravel()[at] = ALPHA[(code + rng.integers(1, 4, len(at))) % 4]
    return A


def founders_pick(rng, m):
    pick = rng.integers(0, 10, m)
    pick[:10] = np.arange(10)
    late = np.arange(m) >= 64
    pick[late & (rng.random(m) < 0.1)] = 10          # founder 10: rows >= 64 only, in both later words
    pick[[64, 140]] = 10
    pick[EARLY] = 4
    pick[[3] + list(range(130, 136))] = 11           # founder 11: word 1 of its sets is zero between words 0 and 2
    return pick


@functools.lru_cache(maxsize=None)
def founders_msa():
    rng = np.random.default_rng(2026)
    F = random_msa(rng, 12, 1500, gap_p=0.004, gap_run=5, similar=0.93)
    pick = founders_pick(rng, 200)
    A = copies(rng, F, pick)
    A[EARLY, -200:] = GAP
    return A, pick, None


@functools.lru_cache(maxsize=None)
def repeats_msa():
    rng = np.random.default_rng(2027)
    F = random_msa(rng, 12, 600, gap_p=0.004, gap_run=5, similar=0.93)
    pick = rng.integers(0, 12, 200)
    pick[:12] = np.arange(12)
    A = copies(rng, F, pick)
    rep = np.tile(np.frombuffer(UNIT * COPIES, dtype=np.uint8), (200, 1))
    for r, x in ((5, 200), (70, 201), (71, 640), (199, 1100)):          # a few rows carry a substitution inside it
        rep[r, x] = ord("A") if rep[r, x] != ord("A") else ord("C")
    return np.hstack([A[:, :300], rep, A[:, 300:]]), pick, (300, 300 + rep.shape[1])


@functools.lru_cache(maxsize=None)
def small_msa(m):
    rng = np.random.default_rng(3000 + m)
    F = random_msa(rng, 5, 300, gap_p=0.004, gap_run=5, similar=0.93)
    pick = rng.integers(0, 5, m)
    pick[:5] = np.arange(5)
    return copies(rng, F, pick), pick, None


def stripped(A):
    return [r[r != GAP].tobytes() for r in A]


def cut(G, j, r, a, ln, rng):
    """Read j: ln symbols of row r from offset a on, every fourth with an N, every third from the other strand."""
    s = bytearray(G[r][a:a + ln])
    if j % 4 == 3:
        s[int(rng.integers(0, ln))] = ord("N")
    strand = int(j % 3 == 2)
    return (STM.revcomp(bytes(s), TABLE) if strand else bytes(s)), (r, a, ln, strand)


def simulate(rng, A, count, lo=40, hi=120, planted=(), every=400):
    """-> (reads, truth): `planted` (row, offset, length) first, then `count` reads from random rows at random offsets, an
    empty read or a read of N after every `every` of them; truth[R] is (row, offset in the gap-stripped row, length, strand) or None."""
    G = stripped(A)
    reads, truth = [], []
    for j in range(len(planted) + count):
        if j < len(planted):
            r, a, ln = planted[j]
        else:
            r, ln = int(rng.integers(0, len(G))), int(rng.integers(lo, hi + 1))
            a = int(rng.integers(0, len(G[r]) - ln + 1))
        s, t = cut(G, j, r, a, ln, rng)
        reads.append(s)
        truth.append(t)
        if j % every == every - 1:
            reads.append((b"", b"N" * 30, b"", b"N")[(j // every) % 4])
            truth.append(None)
    return reads, truth


def founders_input():
    A, pick, _ = founders_msa()
    G = stripped(A)
    sib = [r for r in range(200) if pick[r] == pick[EARLY] and r != EARLY][:3]
    end = len(G[EARLY])
    planted = [(EARLY, end - 60, 60), (EARLY, end - 45, 45)]          # reads that end with the row
    planted += [(r, end - 30, 70) for r in sib]                       # the row ends before these seeds do
    reads, truth = simulate(np.random.default_rng(41), A, 4000, planted=planted)
    for r in (0, 20, 64, 131, 150, 199):              # a piece and its reverse complement: the same read on either strand
        piece = G[r][100 + 3 * r:125 + 3 * r]
        reads.append(piece + STM.revcomp(piece, TABLE))
        truth.append(None)
    return A, reads, truth, 80


def repeats_input():
    """Reads of the usual lengths anywhere, and long ones cut across and inside the repeat with an N every 13th symbol: 2 ..
    32 seeds of 32 places fill the LDS tier, more than 32 the spill tier."""
    A, _, (x0, x1) = repeats_msa()
    G = stripped(A)
    rng = np.random.default_rng(43)
    reads, truth = simulate(rng, A, 150, every=50)
    at = [int((A[r, :x0] != GAP).sum()) for r in range(len(A))]        # offset of the repeat in every row's text
    for j, (ln, shift) in enumerate([(60, 5), (120, 40), (200, -100), (330, 3), (420, 17), (500, 100), (700, 9), (900, -150),
                                     (1200, -60), (1278, 1), (90, 1270), (300, 1100), (650, 300)]):
        r = (5, 70, 71, 199, 33, 128)[j % 6]
        a = at[r] + shift
        s = bytearray(G[r][a:a + ln])
        s[12::13] = b"N" * len(s[12::13])
        strand = j % 2
        reads.append(STM.revcomp(bytes(s), TABLE) if strand else bytes(s))
        truth.append((r, a, ln, strand))
    return A, reads, truth, 100


def small_input(m):
    A = small_msa(m)[0]
    reads, truth = simulate(np.random.default_rng(50 + m), A, 200, every=40)
    return A, reads, truth, 80


INPUTS = {"founders": founders_input, "repeats": repeats_input}
INPUTS.update({f"m{m}": functools.partial(small_input, m) for m in MS})


# ---- the models, end to end on the CPU ---------------------------------------------------------------------------------

def with_min_score(c, min_score):
    """c with the chains, strands and chain rows that min_score leaves (the dynamic programme does not depend on it)."""
    out = SimpleNamespace(**vars(c))
    out.min_score = min_score
    out.chain_off, out.score, out.anchor_place, out.anchor_seed = CM.assemble(c.solved, min_score)
    n = len(c.reads)
    ln = np.diff(out.chain_off.astype(np.int64))
    picks = [STM.pick(int(out.score[R]), int(out.score[n + R]), ln[R] > 0, ln[n + R] > 0) for R in range(n)]
    out.strand = np.array([p[0] for p in picks], dtype=np.uint8)
    out.best_score = np.array([p[1] for p in picks], dtype=np.uint32)
    s = out.strand.tolist()
    out.strand_counts = dict(forward=s.count(0), reverse=s.count(1), none=s.count(STRAND_NONE))
    out.chain_n_rows, out.chain_first_row, out.row_bits, out.chain_sets = RM.chain_rows(c.rm.m, c.sets, out.chain_off, out.anchor_place)
    return out


@functools.lru_cache(maxsize=None)
def cpu(name, cap=CAP, band=BAND, source=None):
    """What the engine is to return for the stranded call on an input with min_score 0, from the models alone (the shape
    of test_rows.cpu, with the counts, restarts and totals of every seed and the strand of every read).  cap and band:
    max_per_seed and the band of the call; source: the input of another module, a function like those of INPUTS."""
    A, reads, truth, high = (source or INPUTS[name])()
    b = oracle_boundaries(A)
    labels, edges, blocks = HM.segmentation_graph(A, b)
    index, mm, rm = OM.Index(labels, edges), MM.Model(A, b), RM.Model(A, b)
    vreads = STM.virtual_reads(reads, TABLE)
    seed_off, q, k, start_off, places, per_seed = [0], [], [], [0], [], []
    for P in vreads:
        for s in SDM.seeds(index, P, MIN_LENGTH, cap):
            q.append(s.q_start)
            k.append(s.length)
            per_seed.append((s.occ.count, s.occ.restarts, s.occ.end_total, s.occ.start_total))
            places += s.occ.starts.tolist()
            start_off.append(len(places))
        seed_off.append(len(q))
    pl = np.array(places, dtype=np.int64).reshape(-1, 3)
    c = SimpleNamespace(name=name, A=A, b=b, reads=reads, truth=truth, vreads=vreads, L=MIN_LENGTH, cap=cap, band=band, high=high,
                        rm=rm, mm=mm, graph=(labels, edges, blocks), text=index.N)
    c.seed_off, c.start_off = np.array(seed_off, dtype=np.uint64), np.array(start_off, dtype=np.uint64)
    c.q_start, c.length = np.array(q, dtype=np.uint32), np.array(k, dtype=np.uint32)
    ps = np.array(per_seed, dtype=np.int64).reshape(-1, 4)
    c.count, c.restarts, c.end_total, c.start_total = ps[:, 0].astype(np.uint64), ps[:, 1].astype(np.uint32), ps[:, 2].astype(np.uint64), \
        ps[:, 3].astype(np.uint64)
    c.start_src, c.start_dst, c.start_offset = (pl[:, x].astype(np.uint32) for x in range(3))
    c.start_row, c.start_col = (x.astype(np.uint32) for x in mm.coords(pl[:, 0], pl[:, 1], pl[:, 2]))
    c.solved = CM.solve(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, band)
    c.n_rows, c.first_row, c.sets = RM.seed_rows(rm, vreads, c.seed_off, c.q_start, c.length, c.start_off, c.start_src, c.start_dst,
                                                 c.start_offset)
    c.places_per_read = np.diff(c.start_off[c.seed_off.astype(np.int64)].astype(np.int64))
    c.seed_of_place = np.repeat(np.arange(len(q)), np.diff(c.start_off.astype(np.int64)))
    c.cols = [np.flatnonzero(r != GAP) for r in A]                   # MSA column of every symbol of a row's text
    c.palindromes = [R for R, r in enumerate(reads) if truth[R] is None and set(r) - {ord("N")} and r == STM.revcomp(r, TABLE)]
    return with_min_score(c, 0)


@functools.lru_cache(maxsize=None)
def cpu_high(name):
    c = cpu(name)
    return with_min_score(c, c.high)


def model_chain_stats(c):
    return TE.expected_stats((c.seed_off, c.q_start, c.length, c.start_off, c.start_col))


def walk_facts(c):
    """hops: the most blocks a supported row's walk enters after its first; ends_early: walks of row EARLY that match up to
    the end of the row, which comes before the end of the seed; cells: the most cells without a node such a walk passes
    before it arrives at the last block."""
    S = RM.substrings(c.vreads, c.seed_off, c.q_start, c.length)
    rm = c.rm
    nb = len(c.b)
    hops = ends_early = cells = 0
    for g, rows in enumerate(c.sets):
        u, o = rm.node_and_offset(int(c.start_src[g]), int(c.start_dst[g]), int(c.start_offset[g]))
        if not 0 <= o < len(rm.labels[u]):
            continue
        j, s = rm.block_of[u], S[c.seed_of_place[g]]
        for r in rows[:2]:
            x = rm.p[r][j] + o
            hops = max(hops, sum(rm.node_of[r][jj] is not None and x < rm.p[r][jj] < x + len(s) for jj in range(j + 1, nb)))
        if c.name == "founders" and rm.node_of[EARLY][j] == u and EARLY not in rows:
            rest = rm.G[EARLY][rm.p[EARLY][j] + o:]
            if len(rest) < len(s) and s.startswith(rest):
                ends_early += 1
                cells = max(cells, sum(v is None for v in rm.node_of[EARLY][j + 1:]))
    return hops, ends_early, cells


def true_place(c, row, x):
    """(node, offset in its label) of symbol x of the gap-stripped text of `row`."""
    rm = c.rm
    for j in range(len(c.b)):
        u = rm.node_of[row][j]
        if u is not None and rm.p[row][j] <= x < rm.p[row][j] + len(rm.labels[u]):
            return u, x - rm.p[row][j]


def true_span(c, row, x, k):
    """How many nodes of `row` the k symbols of its gap-stripped text from offset x on touch."""
    rm = c.rm
    return sum(rm.node_of[row][j] is not None and rm.p[row][j] < x + k and x < rm.p[row][j] + len(rm.labels[rm.node_of[row][j]])
               for j in range(len(c.b)))


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_founders_input_is_what_it_claims():
    A, pick, _ = founders_msa()
    c = cpu("founders")
    rm = c.rm
    # the hand-laid rows
    assert pick[:10].tolist() == [0, 1, 2, 11, 4, 5, 6, 7, 8, 9] and 3 in pick.tolist()
    assert np.flatnonzero(pick == 10).min() == 64 and (np.flatnonzero(pick == 10) >= 128).any()
    assert np.flatnonzero(pick == 11).tolist() == [3] + list(range(130, 136))
    assert (A[EARLY, -200:] == GAP).all()
    gone = [j for j in range(len(c.b)) if rm.node_of[EARLY][j] is None]
    assert gone and gone == list(range(gone[0], len(c.b)))                      # then no node up to the last block
    assert len(gone) >= 8 and len(c.b) > 100
    # sizes: many 256-thread workgroups of seeds, places, reads
    assert len(c.reads) > 4000 and len(c.q_start) > 5000 and len(c.n_rows) > 10000
    assert (np.diff(c.seed_off.astype(np.int64)) == 0).sum() > len(c.reads) // 2     # most wrong strands have no seed
    assert sum(len(r) == 0 for r in c.reads) >= 4 and sum(len(r) > 0 and set(r) == {ord("N")} for r in c.reads) >= 4
    assert {len(r) % 8 for r in c.reads} == set(range(8))
    assert {int(x) % 8 for x in np.cumsum([len(r) for r in c.reads])} == set(range(8))       # every alignment of a read end
    assert (c.restarts > 0).any() and (c.restarts == 0).any() and (c.start_total > 1).any() and (c.start_total == 1).any()
    # both supported and unsupported places and chains; empty chains next to others
    lens = np.diff(c.chain_off.astype(np.int64))
    assert TR.unsupported(c.n_rows) > 100 and (c.n_rows > 0).sum() > 1000
    assert TR.chains_unsupported(c.chain_off, c.chain_n_rows) > 30 and (c.chain_n_rows > 0).sum() > 1000
    assert (lens == 0).sum() > 1000 and (lens > 0).sum() > 1000 and (lens >= 2).sum() > 100
    assert len({tuple(s) for s in c.chain_sets if s}) > 300                       # hundreds of distinct sets in a launch
    words = c.row_bits
    assert words.shape == (2 * len(c.reads), 4)
    assert ((words[:, 0] != 0) & (words[:, 1] == 0) & (words[:, 2] != 0)).any()   # a zero word between two others
    assert ((words[:, 0] == 0) & (words[:, 1] != 0)).any()                        # empty in word 0, not in word 1
    assert ((c.chain_first_row >= 64) & (c.chain_first_row < 128) & (words[:, 2] != 0)).any()
    assert ((c.chain_first_row >= 128) & (c.chain_first_row != NONE)).any()
    # The walks: over many blocks, and of a row that stops early, over its cells without a node up to the last block.
    hops, ends_early, cells = walk_facts(c)
    assert hops >= 8 and ends_early > 0 and cells >= 8, (hops, ends_early, cells)
    # the strands, and what the higher min_score leaves
    assert all(v > 100 for v in (c.strand_counts["forward"], c.strand_counts["reverse"])) and c.strand_counts["none"] >= 8
    n = len(c.reads)
    assert len(c.palindromes) == 6                  # equal scores on the two strands and a chain: the tie goes forward
    for R in c.palindromes:
        assert c.score[R] == c.score[n + R] >= 25 and lens[R] > 0 and lens[n + R] > 0 and c.strand[R] == 0
    h = cpu_high("founders")
    gone = (lens > 0) & (np.diff(h.chain_off.astype(np.int64)) == 0)
    assert len(c.reads) // 4 < gone.sum() < len(c.reads) and h.strand_counts["none"] > c.strand_counts["none"] + 500
    assert h.strand_counts["forward"] > 100 and h.strand_counts["reverse"] > 100
    # every read in the small chain tier: the other two are the repeats input's
    st = model_chain_stats(c)
    assert st["reads_small"] > 4000 and st["anchors"] > 10000


def test_a_row_has_a_node_in_every_block_up_to_its_end():
    """A row that is all gaps across two whole blocks cannot be had from this construction: where such a row has symbols
    again later, the boundaries of the min-max-length DP on the elastic f make one block of the stretch
    and of columns on either side (blanking two blocks of the founders' segmentation in a row gives it one node there, in
    a block as wide as the stretch and more), so a row is without a node only before its first or after its last symbol.
    The nearest input is row EARLY of the founders: walks of that row pass its cells without a node up to the last block
    (test_founders_input_is_what_it_claims), and test_rows.py has the case on boundaries laid by hand."""
    A, c = founders_msa()[0].copy(), cpu("founders")
    j = len(c.b) // 2
    x0, x1 = c.b[j - 1] + 1, c.b[j + 1] + 1
    A[150, x0:x1] = GAP
    rm = RM.Model(A, oracle_boundaries(A))
    inside = [jj for jj, (a, b) in enumerate(rm.ranges) if a < x1 and x0 < b]
    assert len(inside) == 1 and rm.ranges[inside[0]][1] - rm.ranges[inside[0]][0] > x1 - x0 and None not in rm.node_of[150]
    for r in range(200):
        assert None not in c.rm.node_of[r] or r == EARLY


def test_repeats_input_fills_the_three_chain_tiers():
    c = cpu("repeats")
    p = c.places_per_read
    small, lds, spill = ((p > 0) & (p <= PC_SMALL)).sum(), ((p > PC_SMALL) & (p <= PC_LDS)).sum(), (p > PC_LDS).sum()
    assert small > 100 and lds >= 8 and spill >= 4, (small, lds, spill)
    st = model_chain_stats(c)
    assert (st["reads_small"], st["reads_wave"], st["reads_spill"]) == (small, lds, spill)
    n = len(c.reads)
    assert (p[:n] > PC_LDS).any() and (p[n:] > PC_LDS).any()                      # on either strand
    assert (c.start_total > CAP).any() and (c.start_total <= CAP).any()            # places cut by the cap, and not
    assert (c.n_rows >= 190).any() and (c.n_rows == 1).any() and TR.unsupported(c.n_rows) > 0
    assert c.strand_counts["forward"] > 0 and c.strand_counts["reverse"] > 0 and c.strand_counts["none"] > 0


@pytest.mark.parametrize("m", MS)
def test_small_inputs_are_what_they_claim(m):
    c = cpu(f"m{m}")
    assert c.rm.m == m and c.row_bits.shape == (2 * len(c.reads), (m + 63) // 64)
    sets = {tuple(s) for s in c.chain_sets if s}
    assert len(sets) >= 5 and len({tuple(s) for s in c.sets if s}) >= 5           # the sets differ from place to place
    assert any(m - 1 in s for s in sets) and any(0 in s for s in sets)
    assert TR.unsupported(c.n_rows) > 0 and (np.diff(c.chain_off.astype(np.int64)) == 0).any()
    if m == 128:
        assert (c.row_bits[:, 1] >> np.uint64(63)).any() and ((c.row_bits[:, 0] == 0) & (c.row_bits[:, 1] != 0)).any()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_segmentation_is_semi_repeat_free(name):
    labels, edges, blocks = cpu(name).graph
    status, _, _ = VM.Validator(labels, edges).validate(blocks)
    assert (status != VM.INVALID).all() and (status == VM.VALID).sum() > len(labels) // 2


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_models_find_the_simulated_reads(name):
    """The ground truth of the models alone: (a) the strand a read was cut from; (b) for every seed of that strand whose
    places the cap did not cut, a start place at the column of its first symbol in the true row, with the true row in its
    set; (c) the first anchor of the chosen chain at its true column for at least 99 % of the reads.

    (b) has one exception by the definition of the search (rule 4 of locate_model): it takes the restart only where the
    plain step fails, so a seed found without a restart has its places inside single edges, and if its symbols touch more
    than two nodes of the true row, the true occurrence is not among them (the seed is then spelled inside one edge of
    another row with longer labels there).  Where such a seed has no place that meets (b), none of its places is the true
    row's node at the true offset: the exception is checked, not skipped; these seeds stay below 1 % of the seeds.  In (c) a read whose
    chain begins inside the tandem repeat of the repeats input is left out: its column there is one of eighty."""
    c = cpu(name)
    n = len(c.reads)
    repeat = repeats_msa()[2] if name == "repeats" else (0, 0)
    real = chained = strand_ok = seeds_seen = inside_edges = missed = judged = first_ok = 0
    for R, t in enumerate(c.truth):
        if t is None:
            assert (c.strand[R] == STRAND_NONE and c.best_score[R] == 0) or R in c.palindromes
            continue
        real += 1
        row, a, ln, strand = t
        v = strand * n + R
        for s in range(int(c.seed_off[v]), int(c.seed_off[v + 1])):
            if c.start_total[s] > CAP:
                continue
            x = a + int(c.q_start[s])
            col = c.cols[row][x]
            g = [g for g in range(int(c.start_off[s]), int(c.start_off[s + 1])) if c.start_col[g] == col and row in c.sets[g]]
            seeds_seen += 1
            if c.restarts[s] == 0 and true_span(c, row, x, int(c.length[s])) > 2:
                inside_edges += 1
                if not g:
                    true = true_place(c, row, x)
                    assert all(c.rm.node_and_offset(int(c.start_src[i]), int(c.start_dst[i]), int(c.start_offset[i])) != true
                               for i in range(int(c.start_off[s]), int(c.start_off[s + 1]))), (R, t, s)
                    missed += 1
            else:
                assert g, (R, t, s)
        if c.strand[R] == STRAND_NONE:
            continue
        chained += 1
        strand_ok += int(c.strand[R]) == strand
        if int(c.strand[R]) == strand:
            first = int(c.chain_off[v])
            col = c.cols[row][a + int(c.q_start[c.anchor_seed[first]])]
            if not repeat[0] <= col < repeat[1]:
                judged += 1
                first_ok += int(c.start_col[c.anchor_place[first]]) == col
    print(name, dict(reads=real, chained=chained, strand_ok=strand_ok, seeds=seeds_seen, inside_edges=inside_edges, missed=missed, judged=judged,
                     first_ok=first_ok))
    assert chained >= real - real // 100 and strand_ok == chained, (chained, strand_ok, real)
    assert seeds_seen > real // 2 and inside_edges * 100 <= seeds_seen, (seeds_seen, inside_edges)
    assert judged > real // 4 and first_ok * 100 >= 99 * judged, (first_ok, judged)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

ROW_FIELDS = ("start_n_rows", "start_first_row")
CHAIN_ROW_FIELDS = ("n_rows", "first_row", "row_bits")


def call(pix, c, reads=None, strands=True, **kw):
    return pix.seeds(c.reads if reads is None else reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band,
                     min_score=kw.pop("min_score", 0), strands=strands, rows=True, **kw)


def everything(sd):
    """Every array of a call with msa, chain and rows (and the strands, where there are any), as lists."""
    out = TS.seeds_arrays(sd) + [sd.occ.restarts.tolist(), sd.occ.end_total.tolist(), sd.occ.start_total.tolist()]
    out += [getattr(sd, f).tolist() for f in ROW_FIELDS] + [getattr(sd.chains, f).tolist() for f in CHAIN_ROW_FIELDS]
    if sd.chains.strand is not None:
        out += [sd.chains.strand.tolist(), sd.chains.best_score.tolist(), sd.chains.strand_counts]
    return out


def check_chains(pix, ch, c, nr, what):
    """Chains, strands and chain rows of the engine against c, the models on the CPU; nr: n_rows of the places."""
    for f in TR.CHAIN_FIELDS:
        assert getattr(ch, f).dtype == getattr(c, f).dtype and np.array_equal(getattr(ch, f), getattr(c, f)), (what, f)
    assert ch.strand.dtype == np.uint8 and np.array_equal(ch.strand, c.strand), what
    assert np.array_equal(ch.best_score, c.best_score) and ch.strand_counts == c.strand_counts, what
    for got, want, f in ((ch.n_rows, c.chain_n_rows, "n_rows"), (ch.first_row, c.chain_first_row, "first_row"), (ch.row_bits, c.row_bits, "bits")):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f)
    st = pix.rows_stats()
    assert st["places_unsupported"] == TR.unsupported(nr), what
    assert st["chains_unsupported"] == TR.chains_unsupported(c.chain_off, c.chain_n_rows), what


def run_input(engine, name):
    c = cpu(name)
    assert engine_boundaries(engine, c.A) == c.b                      # the engine's segmentation is the oracle's
    with TR.build(engine, c.A, c.b) as pix:
        assert pix.n_nodes == len(c.graph[0]) and pix.text_length() == c.text + 1
        sd = call(pix, c)
        assert sd.strands and sd.reads == len(c.reads)
        TR.same_as_cpu(sd, c, name)
        for f in ("count", "restarts", "end_total", "start_total"):
            assert np.array_equal(getattr(sd.occ, f), getattr(c, f)), (name, f)
        # the models on the engine's own places and chains, then the all-CPU result
        nr, _ = TR.check_rows(pix, sd, c.rm, c.vreads, name)
        assert np.array_equal(sd.start_n_rows, c.n_rows) and np.array_equal(sd.start_first_row, c.first_row)
        check_chains(pix, sd.chains, c, nr, name)
        st = pix.chain_stats()
        assert {k: st[k] for k in ("anchors", "reads_small", "reads_wave", "reads_spill")} == model_chain_stats(c), name
        assert (st["small_max"], st["lds_max"]) == (PC_SMALL, PC_LDS)
        ms = pix.msa_stats()
        assert ms["gapped_nodes"] == sum(len(lab) != x1 - x0 for lab, (x0, x1) in zip(c.mm.labels, c.mm.ranges))
        assert ms["sample_columns"] % 64 == 0 and ms["sample_columns"] > 0 and ms["map_bytes"] >= 16 * pix.n_nodes
        # a min_score that empties a share of the chains: the same seeds, chained again
        h = cpu_high(name)
        check_chains(pix, pix.chains(band=c.band, min_score=h.min_score, rows=True), h, nr, (name, h.min_score))
        return sd


@pytest.mark.gpu
def test_founders(engine):
    sd = run_input(engine, "founders")
    bits = sd.chains.row_bits
    assert ((bits[:, 0] != 0) & (bits[:, 1] == 0) & (bits[:, 2] != 0)).any()
    assert ((bits[:, 0] == 0) & (bits[:, 1] != 0) & (bits[:, 2] != 0) & (sd.chains.first_row < 128)).any()
    assert not (bits[:, 3] >> np.uint64(200 - 192)).any()             # the padding of the last word


@pytest.mark.gpu
def test_repeats(engine):
    run_input(engine, "repeats")
    c = cpu("repeats")
    assert min(model_chain_stats(c)[k] for k in ("reads_small", "reads_wave", "reads_spill")) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
def test_row_counts_beside_the_lane_switch(engine, m):
    """m = 16: the last with four places a wave; 17: the first with a wave a place; 128: both store conditions of k_pr_chain
    hold in its last iteration.  Option rows_wave gives m = 16 the wave of taller MSAs and changes nothing for the others."""
    sd = run_input(engine, f"m{m}")
    c = cpu(f"m{m}")
    with fbg_options(engine, {"rows_wave": 1}):
        with TR.build(engine, c.A, c.b) as pix:
            wave = call(pix, c)
    assert everything(wave) == everything(sd)
    if m % 64:
        assert not (sd.chains.row_bits[:, -1] >> np.uint64(m % 64)).any()


@pytest.mark.gpu
def test_stranded_call_is_the_plain_call_on_the_virtual_reads(engine):
    c = cpu("founders")
    with TR.build(engine, c.A, c.b) as pix:
        sd = call(pix, c)
        got = everything(sd)[:-3]
        plain = call(pix, c, reads=c.vreads, strands=False)
        assert not plain.strands and plain.reads == 2 * len(c.reads) and plain.chains.strand is None
        assert got == everything(plain)
        assert np.array_equal(sd.chains.strand, c.strand) and sd.chains.strand_counts == c.strand_counts


@pytest.mark.gpu
def test_one_index_across_the_large_batch_and_small_ones(engine):
    """The founders batch, three reads, a locate call (it overwrites the reads on the device: pr_save_reads), the rows of
    the batch before it again, the founders batch again: every array is a fresh index's."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    c = cpu("founders")
    three = [c.reads[0], c.reads[2], c.reads[7]]
    patterns = [r for r in c.vreads[:1500] if r] + [b"ACGT" * 400]

    def rows_again(pix, sd, min_score=0):
        ns = len(sd.start_n_rows)
        a, b = np.zeros(ns, dtype=np.uint32), np.zeros(ns, dtype=np.uint32)
        assert L.fbg_pindex_seeds_rows(pix._h, u32(a), u32(b), None) == 0
        assert np.array_equal(a, sd.start_n_rows) and np.array_equal(b, sd.start_first_row)
        ch = pix.chains(band=c.band, min_score=min_score, rows=True)
        for f in TR.CHAIN_FIELDS + CHAIN_ROW_FIELDS + ("strand", "best_score"):
            assert np.array_equal(getattr(ch, f), getattr(sd.chains, f)), f

    with TR.build(engine, c.A, c.b) as fresh:
        small = everything(call(fresh, c, reads=three))
    with TR.build(engine, c.A, c.b) as pix:
        first = call(pix, c)
        large = everything(first)
        TR.same_as_cpu(first, c, "first")
        count = pix.locate(patterns)[0]
        assert (count > 0).sum() > 500
        rows_again(pix, first)                                        # the saved reads of the large batch
        sd = call(pix, c, reads=three)
        assert everything(sd) == small
        pix.locate(patterns)
        pix.occurrences(patterns[:200], max_per_pattern=8)
        rows_again(pix, sd)                                           # the saved reads of the small one, shorter than the buffer
        assert everything(call(pix, c)) == large
        pix.locate([b"T" * 3000])
        rows_again(pix, first)
