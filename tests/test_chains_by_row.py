"""Chaining along one MSA row: fbg_pindex_chains_by_row, fbg_pindex_chains_by_row_stats, PatternIndex.chains(by_row=True) /
.seeds(chain=True, by_row=True) / .by_row_stats() and fbg_locate --by-row (include/fbg_hip.h, csrc/pindex_byrow.hip).

The checker is tests/byrow_model.py on what test_rows.cpu() holds of an input.  On the CPU the model is compared with a
row-by-row brute force and with chain_model on the masked columns, the consequences of the definition are asserted, and
the inputs are asserted to hold what they are meant to hold.  On the GPU every array is compared exactly."""
import ctypes
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import byrow_model as BM  # noqa: E402
import chain_model as CM  # noqa: E402
import cigar_model as GM  # noqa: E402
import rows_model as RM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chain_edges as TE  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402

NONE = BM.NONE
LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_chains_by_row", "fbg_pindex_chains_by_row_stats")
BYROW_MS = (65, 129, 130)
PB_LDS = int(re.search(r"^#define PB_LDS (\d+)\b", open(os.path.join(ROOT, "founderblockgraphs_amd", "csrc", "pindex.h")).read(), re.M).group(1))
MIX_MAX = 3 * PB_LDS                      # option byrow_max of the mixed batch


# ---- the inputs of this file ------------------------------------------------------------------------------------------------

def byrow_haps():
    rng = np.random.default_rng(650)
    return ["".join(rng.choice(list("ACGT"), 72)).encode() for _ in range(9)]


def byrow_input(m):
    """m gap-free rows of 72 columns in six blocks.  Every row carries haplotype H0 but these: row m - 1 carries H1, row 3
    H1's first 24 symbols and then a text of its own, row 100 (where there is one) a text of its own and then H1's last
    24; row 10 carries Ha and row 20 Ha's first 24 symbols and then Hb; row 30 Hc and row 40 Hd.  Reads (N is no symbol
    of the MSA, so it ends a seed):
      0  H1[26:46]: the only best row is m - 1, and no row of an earlier chunk supports anything;
      1  H1[2:22]: rows 3 and m - 1 tie, the lower wins;
      2  H1[50:70]: rows 100 and m - 1 tie (m >= 129: rows of the second and third chunk only);
      3  Ha[2:18] N Ha[19:29] N Hb[30:44]: row 10 supports the first two seeds, row 20 the first and the longer third;
      4  Hc[0:12] N Hc[20:32] N Hd[40:58]: row 30 chains two seeds of 12 with a surplus of 7, row 40 has one seed of 18;
      5  H0[5:45]: every other row;   6, 7  without seeds;   8  the reverse complement of read 0."""
    H0, H1, R3, R100, Ha, Hb, Hc, Hd, _ = byrow_haps()
    rows = [H0] * m
    rows[m - 1] = H1
    rows[3] = H1[:24] + R3[24:]
    if m > 100:
        rows[100] = R100[:48] + H1[48:]
    rows[10], rows[20], rows[30], rows[40] = Ha, Ha[:24] + Hb[24:], Hc, Hd
    reads = [H1[26:46], H1[2:22], H1[50:70], Ha[2:18] + b"N" + Ha[19:29] + b"N" + Hb[30:44],
             Hc[0:12] + b"N" + Hc[20:32] + b"N" + Hd[40:58], H0[5:45], b"NNNN", b"", STM.revcomp(H1[26:46], TR.TABLE)]
    return TR.msa_of(rows), [11, 23, 35, 47, 59, 72], reads, 5, 4, 0, 0


def mix_places():
    return (0, PB_LDS, PB_LDS + 1, MIX_MAX, MIX_MAX + 1, 1, PB_LDS - 1)


def mix_input():
    """Reads of 0, PB_LDS, PB_LDS + 1, byrow_max and byrow_max + 1 start places (byrow_max = MIX_MAX) on test_chains'
    tier_msa, built as test_chain_edges.many_reads builds its place counts: rotations of the unit have 16 places each at
    cap 16, a 12-mer of row 2 has one."""
    A, b = TC.tier_msa()
    rng = np.random.default_rng(29)
    reads = []
    for places in mix_places():
        pieces = [TE.rot(int(r)) for r in rng.integers(0, 12, places // 16)] + [b"ACGCAGACCGAA"] * (places % 16)
        reads.append(b"".join(pieces[i] + b"T" for i in rng.permutation(len(pieces)).tolist()) if pieces else b"TT")
    return A, b, reads, 12, 16, 6, 0


OWN = {f"byrow{m}": functools.partial(byrow_input, m) for m in BYROW_MS}
OWN["byrow_mix"] = mix_input
NAMES = list(TR.INPUTS) + [f"byrow{m}" for m in BYROW_MS]


@functools.lru_cache(maxsize=None)
def cpu(name, strands=False):
    """test_rows.cpu() on an input of either file (this file's inputs are in its table for the length of the call)."""
    with mock.patch.dict(TR.INPUTS, OWN):
        return TR.cpu(name, strands)


@functools.lru_cache(maxsize=None)
def model(name, strands=False, band="input", min_score=None, max_places=1024):
    c = cpu(name, strands)
    return BM.by_row(c, c.band if band == "input" else band, c.min_score if min_score is None else min_score, max_places)


def plain_score(c, band):
    return CM.chains(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, band, 0)[1]


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_by_row_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    for words in ("is at most the score fbg_pindex_chains reports", "first_row == row[R]", "1 <= n_rows <= n_best_rows[R]",
                  "`unsupported` statistic is 0", "byrow_max", "byrow_lds"):
        assert words in header, words


@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_brute_force(name, strands):
    """Reads of up to 10 anchors, at the input's band and unbounded: score, row, the number of best rows and the chain."""
    c = cpu(name, strands)
    checked = 0
    for band in dict.fromkeys((c.band, None)):
        m = model(name, strands, band, 0)
        for R in range(len(c.vreads)):
            if len(CM.read_anchors(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, R)) > 10:
                continue
            score, row, nbest, places = BM.brute_by_row(c, R, band)
            got = m.anchor_place[int(m.chain_off[R]):int(m.chain_off[R + 1])].tolist()
            assert (int(m.score[R]), int(m.row[R]), int(m.n_best_rows[R]), got) == (score, row, nbest, places), (name, band, R)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES + ["byrow_mix"])
def test_model_is_the_chain_model_on_the_masked_columns_and_keeps_the_consequences(name, strands):
    c = cpu(name, strands)
    for band in dict.fromkeys((c.band, None)):
        m = model(name, strands, band)
        off, score, place, seed = CM.chains(c.seed_off, c.q_start, c.length, c.start_off, m.col2, band, c.min_score)
        for got, want in ((m.chain_off, off), (m.score, score), (m.anchor_place, place), (m.anchor_seed, seed)):
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, band)
        assert ((m.col2 == NONE) | (m.col2 == c.start_col)).all() and m.anchors_kept == int((m.col2 != NONE).sum())
        # the consequences of the definition
        plain = CM.chains(c.seed_off, c.q_start, c.length, c.start_off, c.start_col, band, 0)
        sets = RM.chain_rows(c.rm.m, c.sets, plain[0], plain[2])[3]
        assert (m.score <= plain[1]).all()
        for R in range(len(c.vreads)):
            if sets[R]:
                assert m.score[R] == plain[1][R], (name, R)
        assert ((m.score == 0) == (m.row == NONE)).all() and ((m.score == 0) == (m.n_best_rows == 0)).all()
        full = np.diff(m.chain_off.astype(np.int64)) > 0
        assert np.array_equal(m.chain_first_row[full], m.row[full])
        assert (m.chain_n_rows[full] >= 1).all() and (m.chain_n_rows[full] <= m.n_best_rows[full]).all()
        assert (m.chain_n_rows[~full] == 0).all()
        assert TR.chains_unsupported(m.chain_off, m.chain_n_rows) == 0          # what align counts as unsupported


def test_inputs_of_test_rows_hold_what_the_by_row_tests_need():
    """The counts are literal: a changed count means a changed model."""
    for strands, want in ((False, 6), (True, 18)):
        c, m = cpu("chains", strands), model("chains", strands)
        assert int(((m.score > 0) & (m.score < plain_score(c, c.band))).sum()) == want
    assert int((np.diff(model("chains").chain_off.astype(np.int64)) == 0).sum()) > 2      # min_score 30 empties chains
    c, m = cpu("recombinant"), model("recombinant")
    assert int(((c.score > 0) & (m.score == 0)).sum()) == 2 and m.no_row == 2
    for mm, rows in ((63, {0, 62}), (64, {0, 63}), (65, {0, 64}), (129, {0, 64})):
        assert set(model(f"m{mm}").row.tolist()) - {NONE} == rows, mm
    c = cpu("tiers")
    places = BM.places_per_read(c)
    assert places.max() == 1040
    R = int(np.argmax(places))
    m = model("tiers")
    assert m.too_many == 1 and m.score[R] == 0 and m.row[R] == NONE
    m = model("tiers", max_places=2048)
    assert m.too_many == 0 and m.score[R] > 0 and m.row[R] != NONE and m.chain_off[R + 1] > m.chain_off[R]


@pytest.mark.parametrize("m", BYROW_MS)
def test_byrow_input_is_what_it_claims(m):
    c, b0, inf = cpu(f"byrow{m}"), model(f"byrow{m}", band=0), model(f"byrow{m}", band=None)
    assert c.rm.m == m and c.band == 0
    of = lambda g: c.sets[g]      # noqa: E731
    for x in (b0, inf):
        # 0: the last row alone, in the last and partial chunk, after chunks that support nothing
        assert (x.row[0], x.n_best_rows[0], x.score[0]) == (m - 1, 1, 20) and (m - 1) % 64 < 63 and m % 64 != 0
        g = range(int(c.start_off[int(c.seed_off[0])]), int(c.start_off[int(c.seed_off[1])]))
        assert all(not of(k) or min(of(k)) >= 64 * ((m - 1) // 64) for k in g) and (m - 1) // 64 >= 1
        # 1: a tie between a row below 64 and a row above
        assert (x.row[1], x.n_best_rows[1]) == (3, 2) and x.chain_sets[1] == [3, m - 1]
        # 2: a tie between rows of the second and third chunk only
        if m >= 129:
            assert (x.row[2], x.n_best_rows[2]) == (100, 2) and x.chain_sets[2] == [100, m - 1] and (m - 1) // 64 == 2
        else:
            assert (x.row[2], x.n_best_rows[2]) == (m - 1, 1)
        # 5: the common haplotype
        assert x.row[5] == 0 and x.n_best_rows[5] == m - (7 if m > 100 else 6)
        assert x.score[6] == 0 and x.score[7] == 0 and x.row[6] == NONE
    # 3: row 10 supports seeds {1, 2}, row 20 seeds {1, 3}, the third is longer, and the higher row wins
    t0 = int(c.seed_off[3])
    assert int(c.seed_off[4]) - t0 == 3 and c.length[t0:t0 + 3].tolist() == [16, 10, 14]
    sup = [set().union(*[of(g) for g in range(int(c.start_off[t]), int(c.start_off[t + 1]))]) for t in range(t0, t0 + 3)]
    assert sup == [{10, 20}, {10}, {20}]
    for x in (b0, inf):
        assert (x.row[3], x.score[3], x.n_best_rows[3]) == (20, 30, 1)
    assert plain_score(c, 0)[3] == 40                                   # the plain chain takes all three and has no row
    # 4: the best row changes with the band
    assert (b0.row[4], b0.score[4]) == (40, 18) and (inf.row[4], inf.score[4]) == (30, 24)
    # 8: the other strand finds read 0's row
    s = model(f"byrow{m}", True)
    n = len(c.reads)
    assert s.row[n + 8] == m - 1 and np.array_equal(s.row[:n], b0.row)


def test_mix_input_is_what_it_claims():
    c = cpu("byrow_mix")
    assert tuple(BM.places_per_read(c).tolist()) == mix_places()
    m = model("byrow_mix", max_places=MIX_MAX)
    assert m.too_many == 1 and m.score[4] == 0 and m.score[3] > 0
    st = BM.stats(m, PB_LDS)
    assert (st["reads_lds"], st["reads_device"], st["reads_too_many"]) == (3, 2, 1)


def test_tool_by_row_needs_its_prerequisites():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--by-row" in p.stderr
    for args in (["--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--rows", "--by-row"],
                 ["--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0], "--chain", "--by-row"]):
        p = subprocess.run([LOCATE, "--graph=" + TC.SPEC] + args, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--by-row needs" in p.stderr and b"usage:" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

ARRAYS = ("chain_off", "score", "row", "n_best_rows", "anchor_place", "anchor_seed")


def by_row_c(pix, n, band, min_score, want=(1, 1, 1)):
    """The C ABI: -> (chain_off, score, row, n_best_rows, anchor_place, anchor_seed), device_ms."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    off = np.full(n + 2, 7, dtype=np.uint64)
    arr = [np.full(n + 1, 7, dtype=np.uint32) for _ in range(3)]
    ms = ctypes.c_double(0)
    rc = L.fbg_pindex_chains_by_row(pix._h, 0xffffffffffffffff if band is None else band, min_score, off.ctypes.data_as(_lib.u64p),
                                    *[a.ctypes.data_as(_lib.u32p) if w else None for a, w in zip(arr, want)], ctypes.byref(ms))
    assert rc == 0, rc
    assert off[n + 1] == 7 and all(a[n] == 7 for a in arr)            # nothing past the n entries
    t = int(off[n])
    place, seed = np.zeros(t + 1, dtype=np.uint32), np.zeros(t + 1, dtype=np.uint32)
    assert L.fbg_pindex_chains_fetch(pix._h, place.ctypes.data_as(_lib.u32p), seed.ctypes.data_as(_lib.u32p), None) == 0
    return (off[:n + 1], arr[0][:n], arr[1][:n], arr[2][:n], place[:t], seed[:t]), ms.value


def of_chains(ch):
    assert ch.by_row is True
    return ch.chain_off, ch.score, ch.chain_row, ch.n_best_rows, ch.anchor_place, ch.anchor_seed


def same(got, m, what):
    for f, g in zip(ARRAYS, got):
        want = getattr(m, f)
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), (what, f, g.tolist(), want.tolist())


def seeded(pix, c, strands, **kw):
    sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=strands, rows=True, **kw)
    for f in TR.SEED_FIELDS:
        assert np.array_equal(getattr(sd, f), getattr(c, f)), f
    for f in TR.PLACE_FIELDS:
        assert np.array_equal(getattr(sd.occ, f), getattr(c, f)), f
    assert np.array_equal(sd.start_n_rows, c.n_rows)
    return sd


def check_stats(pix, m, byrow_lds=0):
    st = pix.by_row_stats()
    assert st == BM.stats(m, PB_LDS, byrow_lds), (st, BM.stats(m, PB_LDS, byrow_lds))
    assert pix.chain_stats()["anchors"] == m.anchors_kept


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_input_through_both_interfaces(engine, name, strands):
    c, m = cpu(name, strands), model(name, strands)
    n = len(c.vreads)
    with TR.build(engine, c.A, c.b) as pix:
        st = pix.by_row_stats()
        assert (st["lds_max"], st["max_places"], st["reads_lds"], st["anchors_kept"]) == (PB_LDS, 1024, 0, 0)
        seeded(pix, c, strands)
        ch = pix.chains(band=c.band, min_score=c.min_score, by_row=True)
        same(of_chains(ch), m, (name, "python"))
        check_stats(pix, m)
        assert ch.device_ms > 0 or len(c.start_col) == 0
        if name in ("chains", "byrow129"):
            got, ms = by_row_c(pix, n, c.band, c.min_score)
            same(got, m, (name, "C"))
            check_stats(pix, m)
            got, _ = by_row_c(pix, n, c.band, c.min_score, want=(0, 0, 0))       # score, row and n_best_rows may be NULL
            assert np.array_equal(got[0], m.chain_off) and np.array_equal(got[4], m.anchor_place)
            un = model(name, strands, None)                                       # and an unbounded band
            same(by_row_c(pix, n, None, c.min_score)[0], un, (name, "unbounded"))
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=strands, chain=True, band=c.band,
                       min_score=c.min_score, by_row=True)
        same(of_chains(sd.chains), m, (name, "seeds"))
        if strands:
            k = len(c.reads)
            ln = np.diff(m.chain_off.astype(np.int64))
            picks = [STM.pick(int(m.score[R]), int(m.score[k + R]), ln[R] > 0, ln[k + R] > 0) for R in range(k)]
            assert sd.chains.strand.tolist() == [p[0] for p in picks] and sd.chains.best_score.tolist() == [p[1] for p in picks]


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_rows_alignment_and_paths_follow_the_by_row_chains(engine, name, strands):
    c, m = cpu(name, strands), model(name, strands)
    cm = BM.as_cpu(c, m)
    am = AM.of_cpu(cm, 16, 0)
    gm = GM.of_align(cm, am)
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, strands)
        ch = pix.chains(band=c.band, min_score=c.min_score, by_row=True, rows=True, align=True, cigar=True)
        same(of_chains(ch), m, name)
        for got, want, f in ((ch.n_rows, m.chain_n_rows, "n_rows"), (ch.first_row, m.chain_first_row, "first_row"),
                             (ch.row_bits, m.row_bits, "row_bits"), (ch.align_row, am.row, "align_row"), (ch.edits, am.edits, "edits"),
                             (ch.t_start, am.t_start, "t_start"), (ch.t_end, am.t_end, "t_end"), (ch.cigar_off, gm.off, "cigar_off"),
                             (ch.cigar_ops, gm.ops, "cigar_ops")):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (name, f)
        full = np.diff(ch.chain_off.astype(np.int64)) > 0
        assert np.array_equal(ch.first_row[full], ch.chain_row[full]) and np.array_equal(ch.align_row[full], ch.chain_row[full])
        assert (ch.align_row[~full] == NONE).all()
        assert (ch.n_rows[full] >= 1).all() and (ch.n_rows[full] <= ch.n_best_rows[full]).all()
        st = pix.align_stats()
        assert st["unsupported"] == 0 and st["aligned"] == am.stats["aligned"]
        assert pix.rows_stats()["chains_unsupported"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_both_tiers_give_the_same_arrays(engine, name):
    from conftest import fbg_options
    c, m = cpu(name, True), model(name, True)
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, True)
        for lds in (-1, 1):
            with fbg_options(engine, {"byrow_lds": lds}):
                same(of_chains(pix.chains(band=c.band, min_score=c.min_score, by_row=True)), m, (name, lds))
                check_stats(pix, m, lds)
                st = pix.by_row_stats()
                assert st["reads_lds"] == int((m.places == 1).sum()) * (lds == 1)


@pytest.mark.gpu
def test_the_tier_limits(engine):
    from conftest import fbg_options
    c = cpu("tiers")
    R = int(np.argmax(BM.places_per_read(c)))
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        m = model("tiers")
        ch = pix.chains(band=c.band, by_row=True)
        same(of_chains(ch), m, "tiers")
        check_stats(pix, m)
        assert pix.by_row_stats()["reads_too_many"] == 1 and ch.chain_row[R] == NONE
        with fbg_options(engine, {"byrow_max": 2048}):
            m = model("tiers", max_places=2048)
            ch = pix.chains(band=c.band, by_row=True)
            same(of_chains(ch), m, "tiers 2048")
            check_stats(pix, m)
            st = pix.by_row_stats()
            assert st["reads_too_many"] == 0 and st["reads_device"] >= 1 and st["max_places"] == 2048 and ch.chain_row[R] != NONE
    # reads of 0, PB_LDS, PB_LDS + 1, byrow_max and byrow_max + 1 start places in one batch
    c = cpu("byrow_mix")
    with TR.build(engine, c.A, c.b) as pix, fbg_options(engine, {"byrow_max": MIX_MAX}):
        seeded(pix, c, False)
        m = model("byrow_mix", max_places=MIX_MAX)
        same(of_chains(pix.chains(band=c.band, by_row=True)), m, "mix")
        check_stats(pix, m)
        st = pix.by_row_stats()
        assert (st["reads_lds"], st["reads_device"], st["reads_too_many"]) == (3, 2, 1)
        for lds in (-1, 1, PB_LDS + 5):
            with fbg_options(engine, {"byrow_lds": lds}):
                same(of_chains(pix.chains(band=c.band, by_row=True)), m, ("mix", lds))
                check_stats(pix, m, lds)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m1", "gaps", "chains"])
def test_rows_wave_changes_nothing(engine, name):
    from conftest import fbg_options
    c, m = cpu(name), model(name)
    out = []
    for wave in (0, 1):
        with fbg_options(engine, {"rows_wave": wave}), TR.build(engine, c.A, c.b) as pix:
            seeded(pix, c, False)
            ch = pix.chains(band=c.band, min_score=c.min_score, by_row=True, rows=True, align=True)
            same(of_chains(ch), m, (name, wave))
            out.append([ch.n_rows, ch.first_row, ch.row_bits, ch.align_row, ch.edits, ch.t_start, ch.t_end])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_min_score_empties_chains(engine):
    c = cpu("chains")
    assert c.min_score == 30
    with TR.build(engine, c.A, c.b) as pix:
        seeded(pix, c, False)
        lens = []
        for ms in (0, 30, 41, 1 << 40):
            m = model("chains", min_score=ms)
            same(of_chains(pix.chains(band=c.band, min_score=ms, by_row=True)), m, ms)
            check_stats(pix, m)
            lens.append(int((np.diff(m.chain_off.astype(np.int64)) > 0).sum()))
        assert lens[0] > lens[1] >= lens[2] > lens[3] == 0
        assert ((model("chains", min_score=30).score > 0) & (model("chains", min_score=30).score < 30)).any()


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    dummy, off = np.zeros(4096, dtype=np.uint32), np.zeros(4096, dtype=np.uint64)
    c, m = cpu("chains"), model("chains")
    n = len(c.reads)
    assert L.fbg_pindex_chains_by_row(None, 0, 0, off.ctypes.data_as(_lib.u64p), None, None, None, None) == _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_chains_by_row_stats(None, None, None, None, None, None, None, None) == _lib.FBG_ERR_INVALID
    with TR.build(engine, c.A, c.b, rows=False) as plain:
        plain.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True)
        for call in (lambda: plain.chains(by_row=True), lambda: plain.seeds(c.reads, chain=True, by_row=True)):
            with pytest.raises(FbgError) as ei:
                call()
            assert ei.value.code == _lib.FBG_ERR_INVALID and "fbg_pindex_build_segmentation_rows" in str(ei.value)
    with TR.build(engine, c.A, c.b) as fresh:
        seeded(fresh, c, False)
        fresh_plain = fresh.chains(band=c.band, min_score=c.min_score, rows=True, align=True)
    with TR.build(engine, c.A, c.b) as pix:
        # no seeds call yet; a NULL chain_off
        assert L.fbg_pindex_chains_by_row(pix._h, 0, 0, off.ctypes.data_as(_lib.u64p), None, None, None, None) == _lib.FBG_ERR_INVALID
        sd = seeded(pix, c, False)
        assert L.fbg_pindex_chains_by_row(pix._h, 0, 0, None, None, None, None, None) == _lib.FBG_ERR_INVALID
        # by-row, then the plain call: a fresh index's plain result, and the by-row statistics are gone
        same(of_chains(pix.chains(band=c.band, min_score=c.min_score, by_row=True, align=True, cigar=True)), m, "first")
        ch = pix.chains(band=c.band, min_score=c.min_score, rows=True, align=True)
        assert ch.by_row is False and ch.chain_row is None
        for f in TR.CHAIN_FIELDS + ("n_rows", "first_row", "row_bits", "align_row", "edits", "t_start", "t_end"):
            assert np.array_equal(getattr(ch, f), getattr(fresh_plain, f)), f
        for f in TR.CHAIN_FIELDS:
            assert np.array_equal(getattr(ch, f), getattr(c, f)), f
        assert pix.by_row_stats()["anchors_kept"] == 0 and pix.chain_stats()["anchors"] == int((c.start_col != NONE).sum())
        before = TC.seeds_state(pix, len(sd.q_start)), pix.stats(), pix.rows_stats()
        # the plain call, then by-row, twice: the model's result; the alignment of the plain chains is invalidated
        for _ in range(2):
            same(of_chains(pix.chains(band=c.band, min_score=c.min_score, by_row=True)), m, "again")
            check_stats(pix, m)
        assert L.fbg_pindex_chains_cigar(pix._h, None, None, None) == _lib.FBG_ERR_INVALID
        after = TC.seeds_state(pix, len(sd.q_start)), pix.stats(), pix.rows_stats()
        for x, y in zip(before[0], after[0]):
            assert np.array_equal(x, y)
        assert before[1:] == after[1:]
        # a locate and an occurrences call overwrite the reads on the device: the call reads the saved ones
        pix.locate([b"ACGT" * 40, b"T"])
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        same(of_chains(pix.chains(band=c.band, min_score=c.min_score, by_row=True)), m, "saved reads")
        # a new seeds call invalidates the chains
        pix.seeds(c.reads[:3], min_length=c.L, max_per_seed=c.cap)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(dummy), u32(dummy), None) == _lib.FBG_ERR_INVALID
        assert pix.by_row_stats()["anchors_kept"] == 0
        # an empty batch, reads without seeds, seeds without places
        e = pix.seeds([], msa=True, chain=True, by_row=True)
        assert e.chains.chain_off.tolist() == [0] and len(e.chains.chain_row) == 0
        e = pix.seeds([b"NN", b""], msa=True, chain=True, by_row=True)
        assert e.chains.score.tolist() == [0, 0] and e.chains.chain_row.tolist() == [NONE, NONE] and e.chains.n_best_rows.tolist() == [0, 0]
        z = cpu("chains").reads
        e = pix.seeds(z, min_length=c.L, max_per_seed=0, msa=True, chain=True, by_row=True)
        assert len(e.q_start) > 0 and not e.chains.score.any() and (e.chains.chain_row == NONE).all()
        assert e.chains.chain_off.tolist() == [0] * (n + 1)


@pytest.mark.gpu
def test_one_index_across_a_large_and_a_small_batch(engine):
    c = cpu("gaps")
    rng = np.random.default_rng(3)
    G = [r[r != TR.GAP].tobytes() for r in c.A]
    big = [G[int(rng.integers(0, len(G)))][int(a):int(a) + int(k)] for a, k in zip(rng.integers(0, 6, 3000), rng.integers(3, 12, 3000))]
    with TR.build(engine, c.A, c.b) as pix:
        for reads in (big, big[:3], [G[4]], big):
            sd = pix.seeds(reads, min_length=c.L, max_per_seed=c.cap, msa=True, rows=True, chain=True, by_row=True)
            o = sd.occ
            x = SimpleNamespace(seed_off=sd.seed_off, q_start=sd.q_start, length=sd.length, start_off=o.start_off, start_col=o.start_col, rm=c.rm)
            x.sets = RM.seed_rows(c.rm, reads, sd.seed_off, sd.q_start, sd.length, o.start_off, o.start_src, o.start_dst, o.start_offset)[2]
            m = BM.by_row(x, None, 0)
            same(of_chains(sd.chains), m, len(reads))
            check_stats(pix, m)


def write_fasta(path, A):
    with open(path, "wb") as fh:
        for r, row in enumerate(A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
def test_tool_prints_the_chosen_rows(engine, strands, tmp_path):
    """fbg_locate --by-row on the `chains` input: every C line ends with the chosen row and the number of best rows, and the
    C / A / T / G lines are those of the model's chains; without --by-row the output is what it is without the option."""
    from oracle import pyoracle as O
    c, m = cpu("chains", strands), model("chains", strands, None, 0)
    cm = BM.as_cpu(c, m)
    am = AM.of_cpu(cm, 16, 0)
    gm = GM.of_align(cm, am)
    graph, fasta = str(tmp_path / "chains.xgfa"), str(tmp_path / "chains.fasta")
    O.write_xgfa(c.A, c.b, graph)
    write_fasta(fasta, c.A)
    data = b"".join(r + b"\n" for r in c.reads if r)                # the tool reads whitespace-separated tokens
    reads = [r for r in c.reads if r]
    keep = [R for R, r in enumerate(c.reads) if r]
    n, k = len(c.reads), len(reads)
    v_of = (lambda i: keep[i // 2] + (i % 2) * n) if strands else (lambda i: keep[i])
    args = ["--graph=" + graph, "--msa=" + fasta, "--seeds=%d" % c.L, "--occurrences=%d" % c.cap, "--chain", "--rows"] + \
        (["--strands"] if strands else [])
    base = TC.TL.run_locate(args, data)
    assert base.returncode == 0, base.stderr
    for extra in ([], ["--align", "--cigar"]):
        got = TC.TL.run_locate(args + extra + ["--by-row"], data)
        assert got.returncode == 0, got.stderr
        want, i = [], 0
        for ln in base.stdout.splitlines(keepends=True):
            if ln[:2] in (b"A\t", b"G\t", b"T\t"):
                continue
            if not ln.startswith(b"C\t"):
                want.append(ln)
                continue
            v = v_of(i)
            i += 1
            a, b = int(m.chain_off[v]), int(m.chain_off[v + 1])
            star = lambda x: b"*" if x == NONE else b"%d" % x      # noqa: E731
            want.append(b"C\t%d\t%d\t%d\t%s\t%s\t%d\n" % (m.score[v], b - a, m.chain_n_rows[v], star(m.chain_first_row[v]), star(m.row[v]),
                                                        m.n_best_rows[v]))
            for g, t in zip(m.anchor_place[a:b], m.anchor_seed[a:b]):
                want.append(b"A\t%d\t%d\t%d\t%d\n" % (c.q_start[t], c.length[t], c.start_row[g], c.start_col[g]))
            if extra:
                want.append(b"G\t*\n" if am.edits[v] == NONE else b"G\t%d\t%d\t%d\t%d\t%s\n" % (
                    am.row[v], am.edits[v], am.t_start[v], am.t_end[v], GM.string_of(gm.runs[v]).encode()))
            if strands and i % 2 == 0:
                R = keep[i // 2 - 1]
                ln2 = np.diff(m.chain_off.astype(np.int64))
                s, best = STM.pick(int(m.score[R]), int(m.score[n + R]), ln2[R] > 0, ln2[n + R] > 0)
                want.append(b"T\t%s\t%d\n" % (b"*" if s == STM.NONE else b"-" if s else b"+", best))
        assert i == (2 * k if strands else k)
        assert got.stdout == b"".join(want)
    assert b"\t*\t0\n" in got.stdout and (m.row != NONE).any()
    # without --by-row: the plain chains of the engine, as before
    with TR.build(engine, c.A, c.b) as pix:
        sd = pix.seeds(reads, min_length=c.L, max_per_seed=c.cap, msa=True, chain=True, strands=strands, rows=True)
    lines = [ln for ln in base.stdout.splitlines() if ln.startswith(b"C\t")]
    assert [int(ln.split(b"\t")[1]) for ln in lines] == [int(sd.chains.score[(i // 2 + (i % 2) * k) if strands else i]) for i in range(len(lines))]
    assert all(len(ln.split(b"\t")) == 5 for ln in lines)
