"""Which MSA rows carry a start place and a chain: fbg_pindex_build_segmentation_rows, fbg_pindex_seeds_rows,
fbg_pindex_chains_rows, fbg_pindex_rows_stats, PatternIndex.seeds(rows=True) / .chains(rows=True) / .rows_stats() and
fbg_locate --rows (include/fbg_hip.h, csrc/pindex_rows.hip).

The checker is tests/rows_model.py: node_of and the sets from the MSA bytes and the boundaries alone, by string
comparison on gap-stripped rows.  On the CPU every input of the GPU tests goes through seeds_model, chain_model,
strand_model and rows_model, and the tests assert that the inputs hold what they are meant to hold.  On the GPU the
model takes the places and chains from the engine and every array is compared exactly."""
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import chain_model as CM  # noqa: E402
import heuristic_model as HM  # noqa: E402
import msa_model as MM  # noqa: E402
import occ_model as OM  # noqa: E402
import rows_model as RM  # noqa: E402
import seeds_model as SDM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
from conftest import random_msa  # noqa: E402

LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_build_segmentation_rows", "fbg_pindex_seeds_rows", "fbg_pindex_chains_rows", "fbg_pindex_rows_stats")
NONE = RM.NONE
GAP = ord("-")
TABLE = STM.default_table()


def msa_of(rows):
    return np.array([list(r.encode() if isinstance(r, str) else r) for r in rows], dtype=np.uint8)


def windows(s, length, step):
    return [s[a:a + length] for a in range(0, max(len(s) - length, 0) + 1, step)]


# ---- the inputs (name -> MSA, boundaries, reads, min_length, cap, band, min_score) ----------------------------------

X1, X2, Y1, Z1, Z2 = b"ACGTACGA", b"TTGCAAGC", b"GGATCCTG", b"ATATCGCA", b"CGCGTATT"
SPLICES = [X1[-4:] + Y1 + Z2[:4], X2[-4:] + Y1 + Z1[:4]]


def recombinant_input():
    """Rows X1 Y1 Z1 and X2 Y1 Z2; reads cut from either row, then the two spliced reads the graph spells and no row."""
    rows = [X1 + Y1 + Z1, X2 + Y1 + Z2]
    reads = rows + [w for r in rows for w in windows(r, 10, 3)] + [Y1, Y1[1:7]] + SPLICES
    return msa_of(rows), [7, 15, 24], reads, 4, 8, None, 0


def word_input(m):
    """m rows of two haplotypes: the last row and row 64 (where there is one) carry the second, every other row the first."""
    rng = np.random.default_rng(64)
    hap = ["".join(rng.choice(list("ACGT"), 36)).encode() for _ in range(2)]
    special = {m - 1, 64} & set(range(m))
    rows = [hap[1] if r in special else hap[0] for r in range(m)]
    reads = [hap[1], hap[0]] + windows(hap[1], 14, 9) + windows(hap[0], 14, 11) + [hap[0][:12] + b"T" + hap[1][20:34]]
    return msa_of(rows), [11, 23, 36], reads, 5, 4, None, 0


GAP_ROWS = ["ACGTAC-GGATCCATTA",
            "AC-GTACGGATCCATTA",       # the nodes of row 0 with the gap of block 0 elsewhere
            "ACGTAC-----CCATTA",       # no node in the middle block
            "ACGTAC-GGATCC----",       # ends early
            "ACGTAC-CCATTAGGCA"]       # spells row 2's text through a node of the middle block


def gaps_input():
    G = [r.replace("-", "").encode() for r in GAP_ROWS]
    reads = G + [w for g in G for w in windows(g, 8, 2)] + [b"GTACCCATTA", b"GGATCCAT", b"TACGGATCC"]
    return msa_of(GAP_ROWS), [6, 10, 17], reads, 3, 16, None, 0


def bounds_input():
    """Twelve blocks one column wide in the middle, each with symbols of its own (the search runs through them), between
    wider blocks; gap-free rows that differ in a few cells: whole rows as reads, reads that start in the last block, reads
    that end with a label and with the row."""
    rows = ["ACGTAC" + "BDEFHIJKLMNO" + "GATTAC" + "CCGTGAA",
            "ACGTAC" + "BDEFHIJKLMNO" + "GATTAC" + "CGGTGTA",
            "TCGTCC" + "BDEFhIJKLmNO" + "GCTTAC" + "CCGTGAA",
            "ACGTAC" + "BDEFHIJKLmNO" + "GCTTAC" + "CGGTGTA"]
    A = msa_of(rows)
    b = [5] + list(range(6, 18)) + [23, 31]
    G = [r.tobytes() for r in A]
    reads = G + [g[24:] for g in G] + [g[26:31] for g in G] + [g[2:6] for g in G] + [g[3:24] for g in G] + [g[4:19] for g in G]
    return A, b, reads, 3, 8, None, 0


def chains_input():
    """Reads of two pieces from different rows around a symbol the MSA does not hold, reads without seeds, and reads cut
    from single rows, on a random MSA with gaps whose first two rows come twice; min_score empties some chains."""
    rng = np.random.default_rng(78)
    A = random_msa(rng, 6, 72, gap_p=0.03, gap_run=4, similar=0.93)
    A = np.vstack([A, A[:2]])
    b = [8, 17, 29, 37, 48, 60, 72]
    G = [r[r != GAP].tobytes() for r in A]
    reads = list(G) + [b"NNNN", b""]
    for j in range(len(G)):
        o = G[(j + 1 + j // 3) % len(G)]
        reads.append(G[j][2:22] + b"N" + o[30:52])
        reads.append(G[j][5:30])
    reads.append(STM.revcomp(G[3][4:44], TABLE))          # a read from the other strand
    return A, b, reads, 4, 4, None, 30


def tier_input():
    """test_chains' three-row MSA of one repeated unit: reads with 1, 3 and 65 seeds of 16 places each, one per chain tier."""
    A, b = TC.tier_msa()
    rng = np.random.default_rng(5)
    return A, b, [TC.tier_read(rng, s) for s in (1, 3, 65)] + [b"TT"], 12, 16, 6, 0


INPUTS = {"recombinant": recombinant_input, "gaps": gaps_input, "bounds": bounds_input, "chains": chains_input, "tiers": tier_input}
INPUTS.update({f"m{m}": functools.partial(word_input, m) for m in (1, 63, 64, 65, 129)})


# ---- the models, end to end on the CPU ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def graph_models(name):
    A, b = INPUTS[name]()[:2]
    labels, edges, _ = HM.segmentation_graph(A, b)
    return OM.Index(labels, edges), MM.Model(A, b), RM.Model(A, b)


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False, cap=None):
    """What the engine is to return for an input, from the models alone."""
    A, b, reads, L, cap0, band, min_score = INPUTS[name]()
    cap = cap0 if cap is None else cap
    index, mm, rm = graph_models(name)
    vreads = STM.virtual_reads(reads, TABLE) if strands else [bytes(r) for r in reads]
    seed_off, q, k, start_off, places = [0], [], [], [0], []
    for P in vreads:
        for s in SDM.seeds(index, P, L, cap):
            q.append(s.q_start)
            k.append(s.length)
            places += s.occ.starts.tolist()
            start_off.append(len(places))
        seed_off.append(len(q))
    pl = np.array(places, dtype=np.int64).reshape(-1, 3)
    out = SimpleNamespace(A=A, b=b, reads=reads, vreads=vreads, L=L, cap=cap, band=band, min_score=min_score, rm=rm, mm=mm)
    out.seed_off, out.start_off = np.array(seed_off, dtype=np.uint64), np.array(start_off, dtype=np.uint64)
    out.q_start, out.length = np.array(q, dtype=np.uint32), np.array(k, dtype=np.uint32)
    out.start_src, out.start_dst, out.start_offset = (pl[:, c].astype(np.uint32) for c in range(3))
    out.start_row, out.start_col = (x.astype(np.uint32) for x in mm.coords(pl[:, 0], pl[:, 1], pl[:, 2]))
    out.chain_off, out.score, out.anchor_place, out.anchor_seed = CM.chains(out.seed_off, out.q_start, out.length, out.start_off,
                                                                            out.start_col, band, min_score)
    out.n_rows, out.first_row, out.sets = RM.seed_rows(rm, vreads, out.seed_off, out.q_start, out.length, out.start_off,
                                                       out.start_src, out.start_dst, out.start_offset)
    out.chain_n_rows, out.chain_first_row, out.row_bits, out.chain_sets = RM.chain_rows(rm.m, out.sets, out.chain_off, out.anchor_place)
    out.seed_of_place = np.repeat(np.arange(len(q)), np.diff(out.start_off.astype(np.int64)))
    out.read_of_seed = np.repeat(np.arange(len(vreads)), np.diff(out.seed_off.astype(np.int64)))
    return out


def unsupported(n_rows):
    return int((np.asarray(n_rows) == 0).sum())


def chains_unsupported(chain_off, chain_n_rows):
    return int(((np.diff(chain_off.astype(np.int64)) > 0) & (np.asarray(chain_n_rows) == 0)).sum())


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_row_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    assert "The rows through a node or edge are not reported" in header      # the witness cell still is one row


def test_model_agrees_with_a_scan_of_the_cells():
    """The smallest cases: every start place of every seed, the set by strings against the set by MSA cells."""
    for name in ("recombinant", "gaps"):
        c = cpu(name)
        S = RM.substrings(c.vreads, c.seed_off, c.q_start, c.length)
        assert len(c.sets) > 20
        for g, rows in enumerate(c.sets):
            place = (c.start_src[g], c.start_dst[g], c.start_offset[g])
            assert rows == c.rm.rows_by_cells(place, S[c.seed_of_place[g]]), (name, g)
    # node_of is the numbering of the other models
    for name in ("gaps", "chains"):
        _, mm, rm = graph_models(name)
        assert rm.labels == mm.labels and rm.block_of == mm.blocks
        for u, r in enumerate(mm.rep_row):
            assert rm.node_of[r][mm.blocks[u]] == u


def test_recombinant_input_is_what_it_claims():
    c = cpu("recombinant")
    assert set(c.n_rows.tolist()) == {0, 1, 2}
    assert ((c.n_rows == 0) == (c.first_row == NONE)).all()
    n = len(c.reads)
    for R in (n - 2, n - 1):                  # a splice is one seed, the whole read, and no row carries any of its places
        t = int(c.seed_off[R])
        assert int(c.seed_off[R + 1]) == t + 1 and int(c.length[t]) == len(c.reads[R])
        a, b = int(c.start_off[t]), int(c.start_off[t + 1])
        assert b > a and (c.n_rows[a:b] == 0).all()
        assert c.chain_off[R + 1] - c.chain_off[R] == 1 and c.chain_n_rows[R] == 0 and c.chain_first_row[R] == NONE
    for R in range(n - 2):                    # a read cut from a row: one seed, and a place that its row carries
        t = int(c.seed_off[R])
        assert int(c.seed_off[R + 1]) == t + 1 and int(c.length[t]) == len(c.reads[R])
        a, b = int(c.start_off[t]), int(c.start_off[t + 1])
        assert c.n_rows[a:b].max() >= 1
    assert int(c.length.max()) == 24          # a seed as long as the whole row
    assert unsupported(c.n_rows) >= 2 and chains_unsupported(c.chain_off, c.chain_n_rows) == 2


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_word_inputs_are_what_they_claim(m):
    c = cpu(f"m{m}")
    special = sorted({m - 1, 64} & set(range(m)))
    assert special in [s for s in c.sets] and special in c.chain_sets          # the last row, and row 64, alone in a set
    assert c.row_bits.shape == (len(c.reads), (m + 63) // 64)
    if m > 64:
        assert any(s and s[0] >= 64 for s in c.chain_sets)                      # word 0 empty, first_row from a later word
    if m > 2:                                                                    # both haplotypes are there
        assert max(len(s) for s in c.chain_sets) == m - len(special)
        assert c.chain_sets[-1] == [] and c.chain_off[-1] - c.chain_off[-2] >= 2   # both pieces anchored, no common row


def test_gap_input_is_what_it_claims():
    c = cpu("gaps")
    S = RM.substrings(c.vreads, c.seed_off, c.q_start, c.length)
    other_column = across_none = ends_early = 0
    for g, rows in enumerate(c.sets):
        u, o = c.rm.node_and_offset(int(c.start_src[g]), int(c.start_dst[g]), int(c.start_offset[g]))
        if not 0 <= o < len(c.rm.labels[u]):
            continue
        j, s = c.rm.block_of[u], S[c.seed_of_place[g]]
        x0, x1 = c.rm.ranges[j]
        for r in range(c.rm.m):
            if c.rm.node_of[r][j] != u:
                continue
            col = [x for x in range(x0, x1) if c.A[r, x] != GAP][o]
            x = c.rm.p[r][j] + o
            if r in rows:
                other_column += col != int(c.start_col[g])
                # the seed runs over a block in which the row has no node
                end = x + len(s)
                across_none += any(c.rm.node_of[r][jj] is None and c.rm.p[r][jj] > x and c.rm.p[r][jj] < end
                                   for jj in range(j + 1, len(c.b)))
            else:
                rest = c.rm.G[r][x:]
                ends_early += len(rest) < len(s) and s.startswith(rest)
    assert other_column > 0 and across_none > 0 and ends_early > 0, (other_column, across_none, ends_early)
    assert int(c.n_rows.max()) >= 3 and int(c.n_rows.min()) == 1


def test_bounds_input_is_what_it_claims():
    c = cpu("bounds")
    S = RM.substrings(c.vreads, c.seed_off, c.q_start, c.length)
    last = len(c.b) - 1
    in_last = label_end = row_end = whole = hops = 0
    for g, rows in enumerate(c.sets):
        u, o = c.rm.node_and_offset(int(c.start_src[g]), int(c.start_dst[g]), int(c.start_offset[g]))
        if not rows or not 0 <= o < len(c.rm.labels[u]):
            continue
        j, s = c.rm.block_of[u], S[c.seed_of_place[g]]
        in_last += j == last
        for r in rows:
            end = c.rm.p[r][j] + o + len(s)
            label_end += end in c.rm.p[r][1:]
            row_end += end == len(c.rm.G[r])
            whole += len(s) == len(c.rm.G[r])
            hops = max(hops, sum(c.rm.p[r][j] + o < c.rm.p[r][jj] < end for jj in range(len(c.b))))
    assert in_last > 0 and label_end > 0 and row_end > 0 and whole > 0 and hops >= 12, (in_last, label_end, row_end, whole, hops)


def test_chain_inputs_are_what_they_claim():
    c = cpu("chains")
    lens = np.diff(c.chain_off.astype(np.int64))
    each_supported_none_common = 0
    for R in range(len(c.reads)):
        pl = c.anchor_place[int(c.chain_off[R]):int(c.chain_off[R + 1])]
        each_supported_none_common += len(pl) >= 2 and all(c.sets[g] for g in pl) and not c.chain_sets[R]
    assert each_supported_none_common > 0
    assert ((lens == 0) & (c.score > 0)).any()                        # emptied by min_score
    assert (np.diff(c.seed_off.astype(np.int64)) == 0).sum() >= 2     # reads without seeds
    assert (c.chain_n_rows >= 2).any() and (c.chain_n_rows[lens == 0] == 0).all()
    # seeds without places
    z = cpu("chains", cap=0)
    assert len(z.q_start) > 0 and len(z.n_rows) == 0 and z.chain_off.tolist() == [0] * (len(z.reads) + 1)
    assert (z.chain_n_rows == 0).all() and (z.chain_first_row == NONE).all() and not z.row_bits.any()
    # both strands: the 2n virtual reads are the reads and the model's reverse complements, searched as plain reads
    s = cpu("chains", strands=True)
    n = len(c.reads)
    assert len(s.vreads) == 2 * n and s.vreads[n:] == [STM.revcomp(r, TABLE) for r in c.reads]
    assert np.array_equal(s.n_rows[:len(c.n_rows)], c.n_rows) and np.array_equal(s.chain_n_rows[:n], c.chain_n_rows)
    assert s.chain_n_rows[2 * n - 1] > 0 and s.chain_n_rows[n - 1] == 0      # the read given as its reverse complement


def test_tier_input_is_what_it_claims():
    c = cpu("tiers")
    places = [int(c.start_off[int(c.seed_off[R + 1])] - c.start_off[int(c.seed_off[R])]) for R in range(len(c.reads))]
    assert places[0] <= 32 < places[1] <= 1024 < places[2] and places[3] == 0
    assert (c.chain_n_rows[:3] >= 0).all() and len(c.sets) == sum(places)
    assert int(c.n_rows.max()) >= 2 and int(c.n_rows.min()) <= 1


def test_tool_rows_needs_its_prerequisites():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--rows" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--rows"], input=b"AG\n", capture_output=True,
                       timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--rows needs" in p.stderr and b"usage:" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + TC.SPEC, "--msa=" + TC.GOLDEN[0], "--occurrences=4", "--rows"], input=b"AG\n",
                       capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--rows needs" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

def build(engine, A, b, rows=True):
    engine.msa_load_host(np.ascontiguousarray(A, dtype=np.uint8))
    return engine.pattern_index_of_segmentation(b, rows=rows)


SEED_FIELDS = ("seed_off", "q_start", "length")
PLACE_FIELDS = ("start_off", "start_src", "start_dst", "start_offset", "start_row", "start_col")
CHAIN_FIELDS = ("chain_off", "score", "anchor_place", "anchor_seed")


def same_as_cpu(sd, c, what):
    """The engine's seeds, places and chains are the models': what the CPU tests assert about an input holds here too."""
    for f in SEED_FIELDS:
        assert np.array_equal(getattr(sd, f), getattr(c, f)), (what, f)
    for f in PLACE_FIELDS:
        assert np.array_equal(getattr(sd.occ, f), getattr(c, f)), (what, f)
    for f in CHAIN_FIELDS:
        assert np.array_equal(getattr(sd.chains, f), getattr(c, f)), (what, f)


def check_rows(pix, sd, rm, vreads, what):
    """Every array of seeds(rows=True, chain=True) against the model on the engine's own places and chains."""
    o = sd.occ
    nr, fr, sets = RM.seed_rows(rm, vreads, sd.seed_off, sd.q_start, sd.length, o.start_off, o.start_src, o.start_dst, o.start_offset)
    for got, want, f in ((sd.start_n_rows, nr, "n_rows"), (sd.start_first_row, fr, "first_row")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, f)
    ch = sd.chains
    cnr, cfr, bits, _ = RM.chain_rows(rm.m, sets, ch.chain_off, ch.anchor_place)
    for got, want, f in ((ch.n_rows, cnr, "chain n_rows"), (ch.first_row, cfr, "chain first_row"), (ch.row_bits, bits, "row_bits")):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f)
    for R in range(len(cnr)):
        assert ch.row_set(R).tolist() == np.flatnonzero([(int(bits[R, r // 64]) >> (r % 64)) & 1 for r in range(rm.m)]).tolist()
    st = pix.rows_stats()
    assert st["rows"] == rm.m and st["words_per_set"] == (rm.m + 63) // 64
    assert st["places_unsupported"] == unsupported(nr) and st["chains_unsupported"] == chains_unsupported(ch.chain_off, cnr), what
    return nr, cnr


def run_input(engine, name, strands=False, cap=None):
    c = cpu(name, strands, cap)
    with build(engine, c.A, c.b) as pix:
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band, min_score=c.min_score,
                       strands=strands, rows=True)
        same_as_cpu(sd, c, name)
        check_rows(pix, sd, c.rm, c.vreads, name)
        assert np.array_equal(sd.start_n_rows, c.n_rows) and np.array_equal(sd.chains.row_bits, c.row_bits)
        return sd


@pytest.mark.gpu
def test_recombinant(engine):
    sd = run_input(engine, "recombinant")
    c = cpu("recombinant")
    for R in (len(c.reads) - 2, len(c.reads) - 1):
        a, b = (int(sd.occ.start_off[int(sd.seed_off[R]) + d]) for d in (0, 1))
        assert b > a and (sd.start_n_rows[a:b] == 0).all() and (sd.start_first_row[a:b] == NONE).all()
    cut = sd.start_n_rows[:int(sd.occ.start_off[int(sd.seed_off[len(c.reads) - 2])])]
    assert set(cut.tolist()) <= {0, 1, 2} and (cut == 1).any() and (cut == 2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_row_word_boundaries(engine, m):
    sd = run_input(engine, f"m{m}")
    bits = sd.chains.row_bits
    if m % 64:
        assert not (bits[:, -1] >> np.uint64(m % 64)).any()           # the padding of the last word
    special = sorted({m - 1, 64} & set(range(m)))
    assert any(sd.chains.row_set(R).tolist() == special for R in range(len(bits)))
    if m > 64:
        assert ((bits[:, 0] == 0) & (sd.chains.first_row != NONE) & (sd.chains.first_row >= 64)).any()


@pytest.mark.gpu
def test_gaps(engine):
    run_input(engine, "gaps")


@pytest.mark.gpu
def test_bounds(engine):
    run_input(engine, "bounds")


@pytest.mark.gpu
def test_chains(engine):
    sd = run_input(engine, "chains")
    assert sd.chains.rows_ms > 0 and sd.rows_ms > 0
    z = run_input(engine, "chains", cap=0)                            # seeds without places
    assert len(z.start_n_rows) == 0 and not z.chains.row_bits.any() and (z.chains.first_row == NONE).all()
    # both strands: the stranded call against the plain call on the model's reverse complements
    s = run_input(engine, "chains", strands=True)
    c = cpu("chains")
    with build(engine, c.A, c.b) as pix:
        plain = pix.seeds(STM.virtual_reads(c.reads, TABLE), min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band,
                          min_score=c.min_score, rows=True)
        for f in ("start_n_rows", "start_first_row"):
            assert np.array_equal(getattr(s, f), getattr(plain, f)), f
        for f in ("n_rows", "first_row", "row_bits"):
            assert np.array_equal(getattr(s.chains, f), getattr(plain.chains, f)), f
        # an empty batch and reads without seeds
        e = pix.seeds([], msa=True, chain=True, rows=True)
        assert len(e.start_n_rows) == 0 and len(e.chains.n_rows) == 0 and e.chains.row_bits.shape == (0, 1)
        e = pix.seeds([b"NN", b""], msa=True, chain=True, rows=True)
        assert len(e.start_n_rows) == 0 and e.chains.n_rows.tolist() == [0, 0] and e.chains.first_row.tolist() == [NONE, NONE]
        assert pix.rows_stats()["places_unsupported"] == 0 and pix.rows_stats()["chains_unsupported"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["recombinant", "gaps", "chains", "m1"])
def test_a_wave_per_place_agrees_with_sixteen_lanes(engine, name):
    """Up to 16 rows a place or a chain takes 16 lanes; option rows_wave gives it the wave that taller MSAs get."""
    from conftest import fbg_options
    with fbg_options(engine, {"rows_wave": 1}):
        run_input(engine, name)


@pytest.mark.gpu
def test_all_three_chain_tiers_in_one_call(engine):
    c = cpu("tiers")
    with build(engine, c.A, c.b) as pix:
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, band=c.band, rows=True)
        st = pix.chain_stats()
        assert (st["reads_small"], st["reads_wave"], st["reads_spill"]) == (1, 1, 1)
        same_as_cpu(sd, c, "tiers")
        check_rows(pix, sd, c.rm, c.vreads, "tiers")


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    dummy = np.zeros(4096, dtype=np.uint32)
    c = cpu("chains")
    # a NULL index
    assert L.fbg_pindex_seeds_rows(None, u32(dummy), u32(dummy), None) == _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_chains_rows(None, u32(dummy), u32(dummy), None, None) == _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_rows_stats(None, None, None, None, None, None) == _lib.FBG_ERR_INVALID
    # the plain builder's index has no row table; the new builder's index is the same index otherwise
    with build(engine, c.A, c.b, rows=False) as plain, build(engine, c.A, c.b) as pix:
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True)
        for call in (lambda: plain.seeds(c.reads, rows=True), lambda: plain.chains(rows=True), plain.rows_stats):
            with pytest.raises(FbgError) as ei:
                call()
            assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
        for a, b in zip(plain.download(), pix.download()):
            assert np.array_equal(a, b)
        assert plain.stats()["index_bytes"] == pix.stats()["index_bytes"] and plain.msa_stats() == pix.msa_stats()
        assert np.array_equal(plain.node_block, pix.node_block) and np.array_equal(plain.first_node, pix.first_node)
        st = pix.rows_stats()
        nodes = len(c.rm.labels)
        assert st["table_bytes"] == 4 * c.rm.m * len(c.b) + sum(len(s) for s in c.rm.labels) + 8 * (nodes + 1)
        assert (st["places_unsupported"], st["chains_unsupported"]) == (0, 0)
        # no seeds call yet; then seeds without chains
        assert L.fbg_pindex_seeds_rows(pix._h, u32(dummy), u32(dummy), None) == _lib.FBG_ERR_INVALID
        assert L.fbg_pindex_chains_rows(pix._h, u32(dummy), u32(dummy), None, None) == _lib.FBG_ERR_INVALID
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, rows=True)
        assert L.fbg_pindex_chains_rows(pix._h, u32(dummy), u32(dummy), None, None) == _lib.FBG_ERR_INVALID
        assert np.array_equal(sd.start_n_rows, c.n_rows)
        ch = pix.chains(band=c.band, min_score=c.min_score, rows=True)
        # repeated calls: the same results, with and without the optional arrays, and every other state as it was
        before = TC.seeds_state(pix, len(sd.q_start)), [getattr(ch, f).copy() for f in CHAIN_FIELDS], pix.stats(), pix.chain_stats()
        ns, n = len(sd.start_n_rows), len(c.reads)
        for _ in range(2):
            a, b = np.zeros(ns, dtype=np.uint32), np.zeros(ns, dtype=np.uint32)
            assert L.fbg_pindex_seeds_rows(pix._h, u32(a), u32(b), None) == 0
            assert np.array_equal(a, c.n_rows) and np.array_equal(b, c.first_row)
            assert L.fbg_pindex_seeds_rows(pix._h, None, None, None) == 0
            a, b = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            assert L.fbg_pindex_chains_rows(pix._h, u32(a), u32(b), None, None) == 0
            assert np.array_equal(a, c.chain_n_rows) and np.array_equal(b, c.chain_first_row)
            again = pix.chains(band=c.band, min_score=c.min_score, rows=True)
            assert np.array_equal(again.row_bits, c.row_bits)
        st = pix.rows_stats()
        assert st["places_unsupported"] == unsupported(c.n_rows)
        assert st["chains_unsupported"] == chains_unsupported(c.chain_off, c.chain_n_rows)
        after = TC.seeds_state(pix, len(sd.q_start)), [getattr(again, f) for f in CHAIN_FIELDS], pix.stats(), pix.chain_stats()
        for x, y in zip(before[0], after[0]):
            assert np.array_equal(x, y)
        for x, y in zip(before[1], after[1]):
            assert np.array_equal(x, y)
        assert before[2:] == after[2:]
        # a locate and an occurrences call overwrite the reads on the device: the row calls still see the seeds' reads
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        a, b = np.zeros(ns, dtype=np.uint32), np.zeros(ns, dtype=np.uint32)
        assert L.fbg_pindex_seeds_rows(pix._h, u32(a), u32(b), None) == 0
        assert np.array_equal(a, c.n_rows) and np.array_equal(b, c.first_row)
        assert np.array_equal(pix.chains(band=c.band, min_score=c.min_score, rows=True).row_bits, c.row_bits)
        # a new seeds call invalidates the chains, and with them their rows
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap)
        assert L.fbg_pindex_chains_rows(pix._h, u32(dummy), u32(dummy), None, None) == _lib.FBG_ERR_INVALID


@pytest.mark.gpu
def test_one_index_across_calls_of_very_different_sizes(engine):
    c = cpu("gaps")
    rng = np.random.default_rng(3)
    G = [r[r != GAP].tobytes() for r in c.A]
    big = [G[int(rng.integers(0, len(G)))][int(a):int(a) + int(k)] for a, k in zip(rng.integers(0, 6, 3000), rng.integers(3, 12, 3000))]
    with build(engine, c.A, c.b) as pix:
        for reads in ([G[0]], big, [G[2][2:9]], [], big[:70], [G[4]]):
            sd = pix.seeds(reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, rows=True)
            check_rows(pix, sd, c.rm, [bytes(r) for r in reads], len(reads))


@pytest.mark.gpu
def test_tool_prints_the_rows(engine):
    """fbg_locate --rows appends rows and first to every B line of a seed and to every C line; every other byte of the
    output is what it is without --rows.  The example graph of xGFAspec.md is a segmentation of golden/msa.fasta."""
    from fasta_util import read_fasta
    A, _ = read_fasta(TC.GOLDEN[0])
    data = b"AGCGACTAGATAC AGCAGTT CGACTAX T XX GACTAGTTTCA AGXTTAC AGCGTCTCGTTAC\n"
    reads = data.split()
    args = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain=2"]
    with build(engine, A, [1, 5, 8, 14]) as pix:
        sd = pix.seeds(reads, min_length=3, max_per_seed=4, msa=True, chain=True, band=2, rows=True)
    plain, rows = TC.TL.run_locate(args, data), TC.TL.run_locate(args + ["--rows"], data)
    assert plain.returncode == 0 and rows.returncode == 0, (plain.stderr, rows.stderr)
    fmt = lambda n, f: b"\t%d\t%s\n" % (n, b"*" if f == NONE else b"%d" % f)      # noqa: E731
    want, g, r = [], 0, 0
    for ln in plain.stdout.splitlines(keepends=True):
        if ln.startswith(b"B\t") and not ln.endswith(b" more\n"):
            ln = ln[:-1] + fmt(sd.start_n_rows[g], sd.start_first_row[g])
            g += 1
        elif ln.startswith(b"C\t"):
            ln = ln[:-1] + fmt(sd.chains.n_rows[r], sd.chains.first_row[r])
            r += 1
        want.append(ln)
    assert g == len(sd.start_n_rows) > 0 and r == len(reads)
    assert rows.stdout == b"".join(want)
    assert (sd.start_n_rows == 0).any() and (sd.start_n_rows > 0).any()
    # both strands: the same lines with the two fields appended, nothing else
    plain, rows = TC.TL.run_locate(args + ["--strands"], data), TC.TL.run_locate(args + ["--strands", "--rows"], data)
    assert plain.returncode == 0 and rows.returncode == 0, (plain.stderr, rows.stderr)
    a, b = plain.stdout.splitlines(), rows.stdout.splitlines()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if (x.startswith(b"B\t") and not x.endswith(b" more")) or x.startswith(b"C\t"):
            assert y.startswith(x + b"\t") and len(y[len(x) + 1:].split(b"\t")) == 2, (x, y)
        else:
            assert x == y
