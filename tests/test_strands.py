"""Seeds and chains on both strands: fbg_pindex_seeds_strands / fbg_pindex_chain_strands, PatternIndex.seeds(strands=True),
Chains.strand / .best() and fbg_locate --strands (include/fbg_hip.h, csrc/locate.hip: k_px_revcomp; csrc/pindex_chain.hip: k_pc_strand).

The yardstick is the project's own fbg_pindex_seeds / fbg_pindex_chains: a stranded call on n reads must return, array by
array, what the plain call returns on the 2n reads whose second half strand_model.revcomp made on the host, and that in
turn is pinned by the Python models (seeds_model, msa_model, chain_model through test_chain_edges.HostModel).  Every
input is a function of this file alone; test_inputs_reach_their_classes_in_the_models runs each through the models
without a GPU and asserts the counters the GPU tests end with."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import chain_model as CM  # noqa: E402
import strand_model as SM  # noqa: E402
import test_locate as TL  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta  # noqa: E402
from test_chain_edges import HostModel  # noqa: E402
from test_chains import GOLDEN, build, seeds_state  # noqa: E402
from test_seeds import OCC_FIELDS  # noqa: E402

SPEC, LOCATE = TL.SPEC, TL.LOCATE
CALLS = ("fbg_pindex_seeds_strands", "fbg_pindex_chain_strands")
GAP = ord("-")
NONE = SM.NONE
DEFAULT = SM.default_table()
WORD_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)
PALINDROME = b"ACGTGAATTCACGT"
PROTEIN = "ACDEFGHIKLMNPQRSTVWY"


def table_of(pairs):
    t = bytearray(range(256))
    for a, b in pairs.items():
        t[ord(a)] = ord(b)
    return bytes(t)


# ---- the inputs ------------------------------------------------------------------------------------------------------

def dna_msa():
    """6 similar rows of 180 columns with a few gaps and a palindrome under the default table in every row."""
    A = random_msa(np.random.default_rng(7), 6, 180, gap_p=0.03, gap_run=2, similar=0.9)
    A[:, 100:100 + len(PALINDROME)] = np.frombuffer(PALINDROME, dtype=np.uint8)
    return A, [30, 61, 95, 140, 180]


def protein_msa():
    A = random_msa(np.random.default_rng(9), 5, 150, alphabet=PROTEIN, gap_p=0.02, gap_run=2, similar=0.9)
    return A, [40, 77, 110, 150]


def rows_of(A):
    return [r[r != GAP].tobytes() for r in A]


def word_reads(A, table, alphabet=b"ACGT", seed=3):
    """One read of every length in WORD_LENGTHS: cut from a row, cut and reverse-complemented, or random, in turns, then
    shuffled.  267 bytes in all: the second half of the device buffer starts 3 bytes into a word."""
    rng = np.random.default_rng(seed)
    rows = rows_of(A)
    out = []
    for j, ln in enumerate(WORD_LENGTHS):
        r = rows[j % len(rows)]
        a = int(rng.integers(0, len(r) - ln + 1))
        piece = r[a:a + ln]
        out.append((piece, SM.revcomp(piece, table), bytes(alphabet[i] for i in rng.integers(0, len(alphabet), ln)))[j % 3])
    out = [out[i] for i in rng.permutation(len(out)).tolist()]
    assert sum(len(r) for r in out) % 8 != 0
    return out


def choice_reads(A):
    """Planted forward, planted reverse-complemented, random and palindromic reads; short planted ones score below
    CHOICE[3], the min_score of the test."""
    rng = np.random.default_rng(13)
    rows = rows_of(A)
    out, kind = [], []
    for j in range(12):
        r = rows[j % len(rows)]
        ln = (40, 30, 10)[j % 3]
        a = int(rng.integers(0, len(r) - ln + 1))
        out += [r[a:a + ln], SM.revcomp(r[a:a + ln], DEFAULT)]
        kind += ["forward", "reverse"]
    for ln in (5, 12, 33):
        out.append(bytes(b"ACGT"[i] for i in rng.integers(0, 4, ln)))
        kind.append("random")
    for p in (b"ACGT", b"GAATTC", PALINDROME, b""):
        assert SM.revcomp(p, DEFAULT) == p
        out.append(p)
        kind.append("palindrome")
    order = rng.permutation(len(out)).tolist()
    return [out[i] for i in order], [kind[i] for i in order]


CHOICE = (8, 4, None, 12)            # min_length, max_per_seed, band, min_score of the strand choice

TABLES = {"swap": ("dna", table_of({"A": "C", "C": "A"})),
          "no_involution": ("dna", table_of({"A": "C", "C": "G"})),
          "separator_and_zero": ("dna", table_of({"G": "#", "T": "\0", "A": "T", "C": "G"})),
          "protein": ("protein", table_of({"K": "R", "R": "K", "D": "E", "E": "D", "L": "I", "I": "V"}))}

_HOSTS = {}


def host(name):
    if name not in _HOSTS:
        _HOSTS[name] = HostModel(*(dna_msa() if name == "dna" else protein_msa()))
    return _HOSTS[name]


def table_reads(name):
    which, table = TABLES[name]
    h = host(which)
    return word_reads(h.A, table, alphabet=PROTEIN.encode() if which == "protein" else b"ACGT", seed=len(name))


def model_run(h, reads, table, L, cap, band, min_score):
    """The models on the 2n virtual reads -> (the five seed arrays, (chain_off, score, place, seed), strands, scores, counts)."""
    inp = h.seeds(SM.virtual_reads(reads, table), L, cap)
    ch = CM.chains(*inp, band, min_score)
    n = len(reads)
    ln = np.diff(ch[0].astype(np.int64))
    picks = [SM.pick(int(ch[1][r]), int(ch[1][n + r]), ln[r] > 0, ln[n + r] > 0) for r in range(n)]
    strand = [p[0] for p in picks]
    return inp, ch, strand, [p[1] for p in picks], [strand.count(0), strand.count(1), strand.count(NONE)]


def choice_counters(h, reads, kind):
    """forward / reverse / none: reads by outcome; tie: equal positive scores and a chain; below: a positive score but no
    chain; clean: planted reverse reads whose forward search finds nothing and whose score is their length."""
    L, cap, band, min_score = CHOICE
    _, ch, strand, score, counts = model_run(h, reads, DEFAULT, L, cap, band, min_score)
    n = len(reads)
    seen = dict(forward=counts[0], reverse=counts[1], none=counts[2], tie=0, below=0, clean=0)
    for r in range(n):
        s0, s1 = int(ch[1][r]), int(ch[1][n + r])
        seen["tie"] += s0 == s1 and s0 > 0 and strand[r] == 0
        seen["below"] += score[r] > 0 and strand[r] == NONE
        seen["clean"] += kind[r] == "reverse" and s0 == 0 and s1 == len(reads[r]) and strand[r] == 1
    return seen


def reverse_seeds(inp, n):
    return int(inp[0][2 * n]) - int(inp[0][n])


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_strand_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    assert "#define FBG_STRAND_NONE 0xff" in header and _lib.STRAND_NONE == NONE


def test_model_is_the_definition():
    rng = np.random.default_rng(1)
    tables = [DEFAULT, bytes(rng.permutation(256).astype(np.uint8)), bytes(rng.integers(0, 256, 256, dtype=np.uint8))]
    for ln in [0, 1, 2, 3, 17, 100] * 5:
        P = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        for t in tables:
            out = bytearray(ln)
            for i in range(ln):
                out[i] = t[P[ln - 1 - i]]
            assert SM.revcomp(P, t) == bytes(out)
        assert SM.revcomp(SM.revcomp(P, DEFAULT), DEFAULT) == P
    assert SM.revcomp(b"AACGTtgcN#", DEFAULT) == b"#NgcaACGTT"
    for s0 in range(4):
        for s1 in range(4):
            for c0 in (False, True):
                for c1 in (False, True):
                    if s1 > s0:
                        want = (1 if c1 else NONE, s1)
                    else:
                        want = (0 if c0 else NONE, s0)
                    assert SM.pick(s0, s1, c0, c1) == want


def test_complement_table_helper():
    import founderblockgraphs_amd as F
    assert F.complement_table().tobytes() == DEFAULT == F.complement_table(None).tobytes()
    t = F.complement_table({"A": "C", b"C": b"A", ord("x"): "y"})
    assert t.dtype == np.uint8 and t.tobytes() == table_of({"A": "C", "C": "A", "x": "y"})
    assert F.complement_table(DEFAULT).tobytes() == DEFAULT and F.complement_table(list(DEFAULT)).tobytes() == DEFAULT
    for bad in (b"", DEFAULT[:255], DEFAULT + b"A", list(range(257)), {"AB": "C"}, {"A": ""}, {"A": 256}):
        with pytest.raises(ValueError):
            F.complement_table(bad)


def test_tool_strands_needs_seeds():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--strands" in p.stderr and b"--complement=FROMTO" in p.stderr
    for args in (["--strands"], ["--occurrences=4", "--msa=" + GOLDEN[0], "--strands"]):
        p = subprocess.run([LOCATE, "--graph=" + SPEC] + args, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--strands needs --seeds" in p.stderr and b"usage:" in p.stderr, args
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--seeds", "--complement=ATTA"], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--complement needs --strands" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--seeds", "--strands", "--complement=ATT"], input=b"AG\n", capture_output=True,
                       timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--complement takes pairs" in p.stderr


TOOL_L = 6          # --seeds=6: short enough for seeds on one strand only
TOOL_DATA = b"AGCGACTAGATAC GTATCTAGTCGCT AACTGCT T XX GACTAGTTTCA GTAACGAGACGCT ACGT\n"


def test_inputs_reach_their_classes_in_the_models():
    h = host("dna")
    # word boundaries: every length, seeds on both halves, a reverse-complemented piece found again in one seed
    reads = word_reads(h.A, DEFAULT)
    assert sorted(len(r) for r in reads) == list(WORD_LENGTHS)
    inp, ch, strand, _, counts = model_run(h, reads, DEFAULT, 1, 4, None, 0)
    assert reverse_seeds(inp, len(reads)) > 10 and int(inp[0][len(reads)]) > 10
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0          # the empty read has no chain
    # strand choice
    reads, kind = choice_reads(h.A)
    seen = choice_counters(h, reads, kind)
    assert all(v > 0 for v in seen.values()), seen
    # tables: the complement is applied once, '#' and zero bytes reach the search, the general layout takes part
    for name, (which, table) in TABLES.items():
        reads = table_reads(name)
        inp, _, _, _, counts = model_run(host(which), reads, table, 1, 4, None, 0)
        assert reverse_seeds(inp, len(reads)) > 0, name
        both = b"".join(SM.virtual_reads(reads, table)[len(reads):])
        if name == "separator_and_zero":
            assert b"#" in both and b"\0" in both
        if name == "no_involution":
            assert any(SM.revcomp(SM.revcomp(r, table), table) != r for r in reads)
    assert len(set(host("protein").A.ravel().tolist()) - {GAP}) > 16
    # the tool's reads on the example graph: a pattern found on either strand only, on both, on none
    A, _ = read_fasta(GOLDEN[0])
    hs = HostModel(A, [1, 5, 8, 14])
    reads = TOOL_DATA.split()
    inp, ch, strand, _, counts = model_run(hs, reads, DEFAULT, TOOL_L, 4, 2, 0)
    per = np.diff(inp[0].astype(np.int64))
    n = len(reads)
    assert any(per[r] and not per[n + r] for r in range(n)) and any(per[n + r] and not per[r] for r in range(n))
    assert any(per[r] and per[n + r] for r in range(n)) and any(not per[r] and not per[n + r] for r in range(n))
    assert all(c > 0 for c in counts), counts


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def lib():
    from founderblockgraphs_amd import _lib
    return _lib, _lib.lib()


def raw_run(pix, reads, table, L, cap, band, min_score, stranded, lead=b""):
    """Through the C calls: fbg_pindex_seeds_strands on the reads (stranded) or fbg_pindex_seeds on the virtual reads, then
    fetch, places, msa, chains and its fetch -> every array as a list.  lead: bytes in front of the first read, so that
    pat_off[0] != 0."""
    _lib, L_ = lib()
    u8, u32, u64 = (lambda a: a.ctypes.data_as(_lib.u8p)), (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    given = [bytes(r) for r in reads] if stranded else SM.virtual_reads(reads, table)
    data = np.frombuffer(lead + b"".join(given) + b"\0", dtype=np.uint8).copy()
    off = (len(lead) + np.concatenate(([0], np.cumsum([len(r) for r in given])))).astype(np.uint64)
    nv = 2 * len(reads)
    seed_off = np.full(nv + 1, 77, dtype=np.uint64)
    if stranded:
        t = np.frombuffer(table, dtype=np.uint8).copy() if table is not None else None
        rc = L_.fbg_pindex_seeds_strands(pix._h, u8(data), u64(off), len(reads), u8(t) if t is not None else None, L, cap,
                                         u64(seed_off), None)
    else:
        rc = L_.fbg_pindex_seeds(pix._h, u8(data), u64(off), nv, L, cap, u64(seed_off), None)
    assert rc == 0, pix._eng._chk(rc)
    S = int(seed_off[nv])
    state = seeds_state(pix, S)
    chain_off, score = np.full(nv + 1, 77, dtype=np.uint64), np.full(nv + 1, 77, dtype=np.uint32)
    b = 0xffffffffffffffff if band is None else band
    assert L_.fbg_pindex_chains(pix._h, b, min_score, u64(chain_off), u32(score), None) == 0
    t = int(chain_off[nv])
    place, seed = np.zeros(t + 1, dtype=np.uint32), np.zeros(t + 1, dtype=np.uint32)
    assert L_.fbg_pindex_chains_fetch(pix._h, u32(place), u32(seed), None) == 0
    return [seed_off.tolist()] + state + [chain_off.tolist(), score[:nv].tolist(), place[:t].tolist(), seed[:t].tolist()]


def raw_strands(pix, n):
    """fbg_pindex_chain_strands -> (strand, score, [forward, reverse, none])."""
    _lib, L_ = lib()
    strand, score = np.full(n + 1, 7, dtype=np.uint8), np.full(n + 1, 7, dtype=np.uint32)
    cnt = [ctypes.c_uint64(99) for _ in range(3)]
    ms = ctypes.c_double(-1)
    assert L_.fbg_pindex_chain_strands(pix._h, strand.ctypes.data_as(_lib.u8p), score.ctypes.data_as(_lib.u32p),
                                       *[ctypes.byref(c) for c in cnt], ctypes.byref(ms)) == 0
    assert strand[n] == 7 and score[n] == 7 and ms.value >= 0
    return strand[:n].tolist(), score[:n].tolist(), [c.value for c in cnt]


def seeds_arrays(sd):
    """Every array of a Seeds with msa=True and chain=True."""
    out = [getattr(sd, f) for f in ("seed_off", "q_start", "length", "pattern_of")]
    out += [getattr(sd.occ, f) for f in OCC_FIELDS + ("end_row", "end_col", "start_row", "start_col")]
    out += [getattr(sd.chains, f) for f in ("chain_off", "score", "anchor_place", "anchor_seed")]
    return [np.asarray(a).tolist() for a in out]


def check_equivalence(pix, h, reads, table, L, cap, band, min_score, what):
    """Python layer, C calls with an offset base, and the models -> the Seeds of the stranded call."""
    n = len(reads)
    virt = SM.virtual_reads(reads, table)
    sd = pix.seeds(reads, min_length=L, max_per_seed=cap, msa=True, chain=True, band=band, min_score=min_score, strands=True,
                   complement=table)
    assert sd.strands and sd.reads == n and len(sd.seed_off) == 2 * n + 1
    got = seeds_arrays(sd)
    picked = (sd.chains.strand.tolist(), sd.chains.best_score.tolist(), sd.chains.strand_counts)
    plain = pix.seeds(virt, min_length=L, max_per_seed=cap, msa=True, chain=True, band=band, min_score=min_score)
    assert not plain.strands and plain.reads == 2 * n and plain.chains.strand is None and plain.chains.strand_counts is None
    assert got == seeds_arrays(plain), what
    want = raw_run(pix, reads, table, L, cap, band, min_score, False)
    assert raw_run(pix, reads, table, L, cap, band, min_score, True, lead=b"GATTACA") == want, what
    assert raw_strands(pix, n)[:2] == picked[:2]
    # the models on the virtual reads
    inp, ch, strand, score, counts = model_run(h, reads, table, L, cap, band, min_score)
    for g, w in zip((sd.seed_off, sd.q_start, sd.length, sd.occ.start_off, sd.occ.start_col), inp):
        assert np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)), what
    for g, w in zip((sd.chains.chain_off, sd.chains.score, sd.chains.anchor_place, sd.chains.anchor_seed), ch):
        assert np.array_equal(g, w), what
    assert picked == (strand, score, dict(forward=counts[0], reverse=counts[1], none=counts[2])), what
    # where a seed lies in the given read
    lens = [len(r) for r in reads]
    for j in range(len(sd)):
        v = int(sd.pattern_of[j])
        q, k = int(sd.q_start[j]), int(sd.length[j])
        qf = q if v < n else lens[v - n] - q - k
        assert int(sd.q_forward[j]) == qf and virt[v][q:q + k] == (reads[v][q:q + k] if v < n else SM.revcomp(reads[v - n][qf:qf + k], table))
    for r in range(n):
        assert np.array_equal(sd.of(r, strand=1), sd.of(n + r)) and np.array_equal(sd.of(r), sd.of(r, strand=0))
    return sd, inp, counts


@pytest.mark.gpu
def test_equivalence_at_the_word_boundaries(engine):
    h = host("dna")
    reads = word_reads(h.A, DEFAULT)
    with build(engine, h.A, h.b) as pix:
        for L, cap, band, min_score in ((1, 4, None, 0), (3, 64, 2, 5)):
            sd, inp, counts = check_equivalence(pix, h, reads, DEFAULT, L, cap, band, min_score, (L, cap))
        # a NULL table is the default one
        assert raw_run(pix, reads, None, 1, 4, None, 0, True) == raw_run(pix, reads, DEFAULT, 1, 4, None, 0, False)
        # one read at a time, every length
        for r in reads:
            assert raw_run(pix, [r], DEFAULT, 1, 4, None, 0, True, lead=b"A") == raw_run(pix, [r], DEFAULT, 1, 4, None, 0, False), len(r)
    inp, _, _, _, counts = model_run(h, reads, DEFAULT, 1, 4, None, 0)
    assert reverse_seeds(inp, len(reads)) > 10 and all(c > 0 for c in counts)


@pytest.mark.gpu
def test_strand_choice(engine):
    h = host("dna")
    reads, kind = choice_reads(h.A)
    n = len(reads)
    L, cap, band, min_score = CHOICE
    with build(engine, h.A, h.b) as pix:
        sd = pix.seeds(reads, min_length=L, max_per_seed=cap, msa=True, chain=True, band=band, min_score=min_score, strands=True)
        ch = sd.chains
        ln = np.diff(ch.chain_off.astype(np.int64))
        picks = [SM.pick(int(ch.score[r]), int(ch.score[n + r]), ln[r] > 0, ln[n + r] > 0) for r in range(n)]
        assert ch.strand.dtype == np.uint8 and ch.strand.tolist() == [p[0] for p in picks]
        assert ch.best_score.tolist() == [p[1] for p in picks]
        strand = ch.strand.tolist()
        assert ch.strand_counts == dict(forward=strand.count(0), reverse=strand.count(1), none=strand.count(NONE))
        assert raw_strands(pix, n) == (strand, ch.best_score.tolist(), [strand.count(0), strand.count(1), strand.count(NONE)])
        for r in range(n):
            best = ch.best(r)
            if strand[r] == NONE:
                assert best.shape == (0, 2)
            else:
                assert len(best) > 0 and np.array_equal(best, ch.of(strand[r] * n + r))
                assert set(sd.pattern_of[best[:, 1]].tolist()) == {strand[r] * n + r}
        # the models give the same answer, and its classes are all there
        _, mch, mstrand, mscore, _ = model_run(h, reads, DEFAULT, L, cap, band, min_score)
        assert strand == mstrand and ch.best_score.tolist() == mscore
        for r in range(n):
            if kind[r] == "reverse" and int(ch.score[r]) == 0 and len(reads[r]) >= min_score:
                assert int(ch.best_score[r]) == len(reads[r]) and strand[r] == 1, r
    seen = choice_counters(h, reads, kind)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLES))
def test_tables(engine, name):
    which, table = TABLES[name]
    h = host(which)
    reads = table_reads(name)
    with build(engine, h.A, h.b) as pix:
        _, inp, _ = check_equivalence(pix, h, reads, table, 1, 4, None, 0, name)
    assert reverse_seeds(inp, len(reads)) > 0


@pytest.mark.gpu
def test_degenerate_cases(engine):
    _lib, L_ = lib()
    h = host("dna")
    reads = [b"ACGT", b"", rows_of(h.A)[0][:20], SM.revcomp(rows_of(h.A)[1][5:30], DEFAULT)]
    with build(engine, h.A, h.b) as pix:
        sd = pix.seeds([], msa=True, chain=True, strands=True)                                  # n == 0
        assert sd.seed_off.tolist() == [0] and sd.reads == 0 and sd.strands
        assert sd.chains.chain_off.tolist() == [0] and len(sd.chains.strand) == 0
        assert sd.chains.strand_counts == dict(forward=0, reverse=0, none=0)
        assert raw_strands(pix, 0) == ([], [], [99, 99, 99])                                    # the call writes nothing
        sd = pix.seeds([b"", b"", b""], max_per_seed=4, msa=True, chain=True, strands=True)     # empty reads
        assert sd.seed_off.tolist() == [0] * 7 and sd.chains.strand.tolist() == [NONE] * 3
        assert sd.chains.best_score.tolist() == [0] * 3 and sd.chains.strand_counts == dict(forward=0, reverse=0, none=3)
        sd = pix.seeds(reads, min_length=66, max_per_seed=4, msa=True, chain=True, strands=True)   # min_length above every read
        assert len(sd) == 0 and sd.chains.strand.tolist() == [NONE] * 4 and sd.chains.best_score.tolist() == [0] * 4
        sd = pix.seeds(reads, min_length=1 << 32, max_per_seed=4, chain=True, strands=True)
        assert len(sd) == 0 and sd.seed_off.tolist() == [0] * 9 and sd.chains.strand_counts["none"] == 4
        sd = pix.seeds(reads, max_per_seed=0, msa=True, chain=True, strands=True)               # seeds without places
        assert len(sd) > 0 and sd.chains.strand.tolist() == [NONE] * 4 and sd.chains.best_score.tolist() == [0] * 4
        assert raw_strands(pix, 4) == ([NONE] * 4, [0] * 4, [0, 0, 4])
        sd = pix.seeds(reads, max_per_seed=4, msa=True, chain=True, strands=True)
        top = int(sd.chains.score.max())
        assert sd.chains.strand.tolist() == [0, NONE, 0, 1] and sd.chains.best_score.tolist()[2:] == [20, 25]
        ch = pix.chains(min_score=top + 1)                                                      # min_score above every score
        assert ch.strand.tolist() == [NONE] * 4 and np.array_equal(ch.best_score, sd.chains.best_score)
        assert ch.strand_counts == dict(forward=0, reverse=0, none=4)
        # every output pointer NULL, and the call repeats
        assert L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None) == 0
        assert raw_strands(pix, 4) == ([NONE] * 4, sd.chains.best_score.tolist(), [0, 0, 4])
        assert raw_strands(pix, 4) == ([NONE] * 4, sd.chains.best_score.tolist(), [0, 0, 4])


@pytest.mark.gpu
def test_state_rules(engine):
    import founderblockgraphs_amd as F
    _lib, L_ = lib()
    INVALID = _lib.FBG_ERR_INVALID
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    assert L_.fbg_pindex_chain_strands(None, None, None, None, None, None, None) == INVALID
    assert L_.fbg_pindex_seeds_strands(None, None, None, 0, None, 1, 0, None, None) == INVALID
    h = host("dna")
    rows = rows_of(h.A)
    small = word_reads(h.A, DEFAULT)[:3]
    rng = np.random.default_rng(5)
    large = [rows[j % 6][a:a + 60] for j, a in enumerate(rng.integers(0, 80, 40).tolist())]
    large = [SM.revcomp(r, DEFAULT) if j % 2 else r for j, r in enumerate(large)]
    with build(engine, h.A, h.b) as pix:
        assert L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None) == INVALID     # no seeds at all
        occ = pix.occurrences(large[:10], max_per_pattern=8, msa=True)
        count, pos = pix.locate(large)
        stats = pix.stats()
        val = pix.validate(pix.node_block)
        # a stranded seeds call, but no chains yet
        sd = pix.seeds(large, max_per_seed=4, msa=True, strands=True)
        assert L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None) == INVALID
        with pytest.raises(F.FbgError) as ei:
            pix._eng._chk(L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None))
        assert ei.value.code == INVALID and "fbg_pindex_chains" in str(ei.value)
        before = seeds_state(pix, len(sd))
        ch = pix.chains(band=3, min_score=4)
        assert ch.strand_counts["forward"] > 0 and ch.strand_counts["reverse"] > 0
        chains_before = [a.tolist() for a in (ch.chain_off, ch.score, ch.anchor_place, ch.anchor_seed)]
        first = raw_strands(pix, len(large))
        assert first == (ch.strand.tolist(), ch.best_score.tolist(), [ch.strand_counts[k] for k in ("forward", "reverse", "none")])
        # the strand call leaves the seeds, the chains and everything else alone
        assert seeds_state(pix, len(sd)) == before
        t = len(ch.anchor_place)
        place, seed = np.zeros(t + 1, dtype=np.uint32), np.zeros(t + 1, dtype=np.uint32)
        assert L_.fbg_pindex_chains_fetch(pix._h, u32(place), u32(seed), None) == 0
        assert [place[:t].tolist(), seed[:t].tolist()] == chains_before[2:]
        ends = [np.zeros(len(occ.end_src) + 1, dtype=np.uint32) for _ in range(3)]
        starts = [np.zeros(len(occ.start_src) + 1, dtype=np.uint32) for _ in range(3)]
        assert L_.fbg_pindex_occurrences_fetch(pix._h, *[u32(a) for a in ends + starts], None) == 0
        for a, f in zip(ends + starts, ("end_src", "end_dst", "end_offset", "start_src", "start_dst", "start_offset")):
            assert np.array_equal(a[:-1], getattr(occ, f)), f
        assert pix.stats() == stats
        c2, p2 = pix.locate(large)
        assert np.array_equal(c2, count) and np.array_equal(p2, pos)
        assert np.array_equal(pix.validate(pix.node_block).status, val.status)
        assert raw_strands(pix, len(large)) == first
        # a small stranded call after the large one: stale bytes lie behind its second half
        got = raw_run(pix, small, DEFAULT, 1, 4, None, 0, True)
        got_strands = raw_strands(pix, len(small))
        # a plain seeds call clears the strands
        pix.seeds(large[:5], max_per_seed=4, msa=True)
        assert pix.chains().strand is None
        assert L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None) == INVALID
    with build(engine, h.A, h.b) as fresh:
        assert raw_run(fresh, small, DEFAULT, 1, 4, None, 0, True) == got
        assert raw_strands(fresh, len(small)) == got_strands
        assert got == raw_run(fresh, small, DEFAULT, 1, 4, None, 0, False)
    # an index built on the host knows no MSA: no chains, so no strands
    labels, edges = F.read_xgfa(SPEC)
    with engine.pattern_index(labels, edges) as pix:
        sd = pix.seeds(["AGCGA", "TCGCT"], max_per_seed=4, strands=True)
        assert sd.strands and len(sd.of(0)) > 0 and len(sd.of(1, strand=1)) > 0
        assert L_.fbg_pindex_chain_strands(pix._h, None, None, None, None, None, None) == INVALID


def block_lines(sd, v, ids, chain):
    """The S / E / B (/ C / A) lines of virtual read v, as fbg_locate prints them."""
    o, ch = sd.occ, sd.chains
    lines = []
    for j in range(int(sd.seed_off[v]), int(sd.seed_off[v + 1])):
        lines.append(b"S\t%d\t%d\t%d\t%d\n" % (sd.q_start[j], sd.length[j], o.count[j], o.restarts[j]))
        for tag, w, total in ((b"E", "end", o.end_total), (b"B", "start", o.start_total)):
            off = getattr(o, w + "_off")
            for i in range(int(off[j]), int(off[j + 1])):
                src, dst, at, row, col = (int(getattr(o, f"{w}_{f}")[i]) for f in ("src", "dst", "offset", "row", "col"))
                lines.append(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (tag, ids[src], ids[dst], at, row, col))
            if int(total[j]) > int(off[j + 1] - off[j]):
                lines.append(b"%s\t...\t%d more\n" % (tag, int(total[j]) - int(off[j + 1] - off[j])))
    if chain:
        lines.append(b"C\t%d\t%d\n" % (ch.score[v], len(ch.of(v))))
        lines += [b"A\t%d\t%d\t%d\t%d\n" % (sd.q_start[t], sd.length[t], o.start_row[g], o.start_col[g]) for g, t in ch.of(v)]
    return lines


@pytest.mark.gpu
def test_tool_prints_both_strands(engine):
    A, _ = read_fasta(GOLDEN[0])
    reads = TOOL_DATA.split()
    n = len(reads)
    args = ["--graph=" + SPEC, "--seeds=%d" % TOOL_L, "--occurrences=4", "--msa=" + GOLDEN[0]]
    with build(engine, A, [1, 5, 8, 14]) as pix:
        sd = pix.seeds(reads, min_length=TOOL_L, max_per_seed=4, msa=True, chain=True, band=2, strands=True)
        plain = pix.seeds(reads, min_length=TOOL_L, max_per_seed=4, msa=True, chain=True, band=2)
        swapped = pix.seeds(reads, min_length=TOOL_L, max_per_seed=4, msa=True, chain=True, band=2, strands=True,
                            complement={"A": "C", "C": "A"})
    ids = list(range(1, 10))
    per = np.diff(sd.seed_off.astype(np.int64))

    def expected(sd, chain):
        out, seeded = [], 0
        for r in range(n):
            out.append(b"Pattern? %d seeds found.\n" % per_of(sd)[r])
            out += block_lines(sd, r, ids, chain)
            if sd.strands:
                out.append(b"-\t%d\n" % per_of(sd)[n + r])
                out += block_lines(sd, n + r, ids, chain)
                if chain:
                    t = int(sd.chains.strand[r])
                    out.append(b"T\t%s\t%d\n" % (b"*" if t == NONE else b"+-"[t:t + 1], sd.chains.best_score[r]))
            seeded += bool(per_of(sd)[r] or (sd.strands and per_of(sd)[n + r]))
        return b"".join(out) + b"Pattern? %d out of %d patterns seeded\n" % (seeded, n)

    def per_of(sd):
        return np.diff(sd.seed_off.astype(np.int64))

    p = TL.run_locate(args + ["--chain=2", "--strands"], TOOL_DATA)
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(sd, True)
    marks = [ln[2:3] for ln in p.stdout.splitlines() if ln[:2] == b"T\t"]
    assert len(marks) == n and {b"+", b"-", b"*"} == set(marks)
    # without --chain: no C, A and T lines; without --strands: today's output
    q = TL.run_locate(args + ["--strands"], TOOL_DATA)
    assert q.returncode == 0 and q.stdout == expected(sd, False)
    q = TL.run_locate(args + ["--chain=2"], TOOL_DATA)
    assert q.returncode == 0 and q.stdout == expected(plain, True)
    # a caller's table
    q = TL.run_locate(args + ["--chain=2", "--strands", "--complement=ACCA"], TOOL_DATA)
    assert q.returncode == 0 and q.stdout == expected(swapped, True) and q.stdout != p.stdout
    # --error-on-not-found: a pattern with seeds on the reverse strand only passes, one with none on both fails
    first_none = min(r for r in range(n) if not per[r] and not per[n + r])
    assert any(not per[r] and per[n + r] for r in range(first_none))
    q = TL.run_locate(args + ["--strands", "--error-on-not-found"], TOOL_DATA)
    assert q.returncode == 1 and b"Pattern has no seed." in q.stderr
    assert q.stdout.count(b"Pattern? ") == first_none + 1 and q.stdout.endswith(b"Pattern? 0 seeds found.\n")
    assert expected(sd, False).startswith(q.stdout)
