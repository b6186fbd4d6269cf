"""The second-best chain of every read and the mapping quality: fbg_pindex_chains_mapq / _mapq_fetch,
fbg_pindex_mapq_strands, fbg_pindex_mapq_stats, PatternIndex.chains(mapq=True) / .seeds(chain=True, mapq=True) /
.mapq_stats() and fbg_locate --mapq (include/fbg_hip.h, csrc/pindex_mapq.hip).

The checker is tests/mapq_model.py: the definitions of the header on top of chain_model, applied to what
PatternIndex.seeds(msa=True) returns and to the primary chains a chaining call reports (both pinned by test_seeds,
test_msa_coords, test_chains and test_chains_by_row).  On the CPU the model is compared with chain_model's brute force.
Every GPU comparison is exact.

The golden FASTAs have rows of 14 and 15 symbols: their reads are the rows whole and in pieces (test_chains.chain_reads),
beside the random reads of 30 to 60 symbols and the empty read that every input gets."""
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
import mapq_model as QM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta  # noqa: E402

NONE = CM.NONE
U64 = QM.U64_MAX
GAP = ord("-")
LOCATE = TC.LOCATE
CALLS = ("fbg_pindex_chains_mapq", "fbg_pindex_chains_mapq_fetch", "fbg_pindex_mapq_strands", "fbg_pindex_mapq_stats")
FIELDS = (("second_off", "second_off"), ("second_score", "second"), ("second_lo", "second_lo"), ("second_hi", "second_hi"),
          ("mapq", "mapq"), ("second_place", "second_place"), ("second_seed", "second_seed"))
STATS = ("reads_with_second", "anchors_kept", "anchors_excluded", "mapq0", "mapq60")


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_mapq_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    for words in ("c + k + margin > lo and c < hi + margin", "truth set", "greedy maximal exact matches"):
        assert words in header, words


def test_model_agrees_with_brute_force():
    rng = np.random.default_rng(11)
    seen = dict(none=0, less=0, equal=0, margin_only=0, lo_in=0, lo_out=0, hi_in=0, hi_out=0, astride=0)
    for trial in range(400):
        an = TC.random_anchors(rng)
        for band in (0, 1, 3, None):
            s1, idx = CM.chain_of(an, band)
            span = QM.span_of([an[j] for j in idx])
            for margin in (0, 2, U64):
                if span is None:
                    assert QM.secondary_of(an, span, band, margin) == (0, [], 0)
                    continue
                lo, hi = span
                kept = QM.kept_anchors(an, span, margin)
                assert [a for a in an if a not in kept] == [a for a in an if a[4] + a[3] + margin > lo and a[4] < hi + margin]
                second, sec, n_kept = QM.secondary_of(an, span, band, margin)
                top, at = CM.brute_force(kept, band)
                assert second == top and n_kept == len(kept), (trial, band, margin)
                if sec:
                    # the tie-break minimum among the best: the smallest end, then the smallest predecessor, and so on
                    assert tuple(kept.index(a) for a in sec) == min(at, key=lambda sub: sub[::-1]), (trial, band, margin)
                    # no anchor of the secondary meets the widened span; its span does where the chain has anchors on
                    # either side of it (the definitions allow that: the statement holds per anchor, not for the span)
                    assert all(a[4] + a[3] + margin <= lo or a[4] >= hi + margin for a in sec), (trial, band, margin)
                    lo2, hi2 = QM.span_of(sec)
                    if not (hi2 + margin <= lo or lo2 >= hi + margin):
                        assert sec[0][4] + sec[0][3] + margin <= lo and sec[-1][4] >= hi + margin, (trial, band, margin)
                        seen["astride"] += 1
                    assert sum(a[3] for a in sec) == second
                else:
                    assert second == 0 and at == []
                assert second <= s1
                if margin == U64:
                    assert kept == [] and second == 0
                    continue
                seen["none"] += second == 0
                seen["less"] += 0 < second < s1
                seen["equal"] += second == s1
                if margin == 2:
                    seen["margin_only"] += any(not QM.excluded(a[4], a[3], span, 0) for a in an if a not in kept)
                seen["lo_in"] += any(a[4] + a[3] + margin == lo + 1 and a not in kept for a in an)
                seen["lo_out"] += any(a[4] + a[3] + margin == lo and a in kept for a in an)
                seen["hi_in"] += any(a[4] == hi + margin - 1 and a[4] + a[3] + margin > lo and a not in kept for a in an)
                seen["hi_out"] += any(a[4] == hi + margin and a in kept for a in an)
    assert all(v >= 30 for f, v in seen.items() if f != "astride") and seen["astride"] > 0, seen


def test_formula_edges():
    q, qs = QM.mapq_of, QM.mapq_stranded_of
    assert q(5, 0, 0, True) == 0                                    # L = 0
    assert q(40, 0, 40, False) == 0 and qs(40, 0, 0, 40, False) == 0  # an empty chain
    assert q(40, 0, 40, True) == 60                                 # s1 = L, s2 = 0
    assert q(30, 45, 50, True) == 0                                 # s2 > s1 (after a by-row call)
    assert q(30, 30, 50, True) == 0
    # flooring: 60 * (s1 - s2) = L - 1 and = L
    assert q(1, 0, 61, True) == 0 and q(1, 0, 60, True) == 1 and q(2, 0, 121, True) == 0 and q(2, 0, 120, True) == 1
    assert q(59, 0, 60, True) == 59 and q(60, 1, 60, True) == 59
    assert [q(s, 0, 100, True) for s in (1, 2, 99, 100)] == [0, 1, 59, 60]
    # both strands: the twin competes, ties give 0 on both, a twin below min_score still counts
    assert qs(40, 0, 40, 40, True) == 0 and qs(40, 10, 40, 40, True) == 0
    assert qs(40, 10, 20, 40, True) == 30 and qs(40, 30, 20, 40, True) == 15 and qs(40, 0, 50, 40, True) == 0
    assert qs(40, 0, 3, 40, True) == 55 and qs(3, 0, 40, 40, False) == 0
    # through solve(): two virtual reads with one seed of one place each, scores 8 and 8, then 8 and 5
    for k2, want in ((8, [0, 0]), (5, [22, 0])):
        seed_off, start_off = np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1, 2], dtype=np.uint64)
        qq, kk, col = np.zeros(2, dtype=np.uint32), np.array([8, k2], dtype=np.uint32), np.array([3, 30], dtype=np.uint32)
        off, score, place, seed = CM.chains(seed_off, qq, kk, start_off, col, None, 6)      # min_score empties the chain of 5
        m = QM.solve(seed_off, qq, kk, start_off, col, [8, 8], off, score, place, seed, None, 0, stranded=True)
        assert m.mapq_stranded.tolist() == want and m.second.tolist() == [0, 0]
        assert m.mapq.tolist() == [60, 60 if k2 == 8 else 0]


def test_tool_mapq_needs_chain_and_a_margin():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--mapq[=MARGIN]" in p.stderr
    full = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0]]
    for args in (full + ["--mapq"], full + ["--mapq=3"], ["--graph=" + TC.SPEC, "--mapq"]):
        p = subprocess.run([LOCATE] + args, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--mapq needs --chain" in p.stderr and b"usage:" in p.stderr, args
    for bad in ("x", "", "-1", "3x"):
        p = subprocess.run([LOCATE] + full + ["--chain", "--mapq=" + bad], input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--mapq takes a margin, not '" + bad.encode() + b"'" in p.stderr, bad


# ---- GPU ----------------------------------------------------------------------------------------------------------

def same(ch, m, what):
    for f, g in FIELDS:
        got, want = getattr(ch, f), getattr(m, g)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f, got.tolist(), want.tolist())


def model_of(sd, ch, lens, band, margin, stranded=False, cache=None):
    return QM.solve(*TC.model_inputs(sd), lens, ch.chain_off, ch.score, ch.anchor_place, ch.anchor_seed, band, margin, stranded, cache)


def planted(rng, m, n, gaps):
    A = random_msa(rng, m, n, gap_p=0.02, gap_run=3, similar=0.9) if gaps else random_msa(rng, m, n, similar=0.9)
    A[:, 220:280] = A[:, 40:100]
    return A


def cut_reads(rng, A):
    """About 200 reads of 30 to 60 symbols cut from the rows, gaps stripped, with 0 to 3 substitutions each: inside the
    planted segment [40, 100) or its copy, across one of their four ends, and outside both; then 10 random reads and an
    empty one."""
    n = A.shape[1]
    out = []

    def cut(a, ln, j):
        row = A[int(rng.integers(0, len(A)))]
        s = bytearray(row[a:a + ln][row[a:a + ln] != GAP].tobytes())
        for _ in range(j % 4):
            at = int(rng.integers(0, len(s)))
            s[at] = rng.choice([c for c in b"ACGT" if c != s[at]])
        out.append(bytes(s))

    for j in range(70):                                     # inside
        ln = int(rng.integers(30, 56))
        cut((40, 220)[j % 2] + int(rng.integers(0, 60 - ln + 1)), ln, j)
    for j in range(80):                                     # across an end of the segment or of its copy
        ln, edge = int(rng.integers(36, 61)), (40, 100, 220, 280)[j % 4]
        cut(max(0, min(n - ln, edge - int(rng.integers(12, ln - 11)))), ln, j)
    for j in range(50):                                     # outside
        ln = int(rng.integers(30, 61))
        a = 105 + int(rng.integers(0, 110 - ln + 1)) if j % 2 == 0 or n < 290 + ln else 285 + int(rng.integers(0, n - 285 - ln + 1))
        cut(a, ln, j)
    out += [bytes(rng.choice(list(b"ACGT"), int(rng.integers(30, 61))).astype(np.uint8)) for _ in range(10)]
    return out + [b""]


def fixed_cuts(n):
    return list(range(24, n - 1, 25)) + [n]


def parity(engine, A, reads, bounds, what, seen):
    """Every band, margin and min_score of the issue on one index, after the plain and after the by-row chaining call."""
    lens = [len(r) for r in reads]
    with TR.build(engine, A, bounds) as pix:
        assert pix.mapq_stats() == dict.fromkeys(STATS, 0)
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True)
        cache = {}
        for band in (None, 8):
            for min_score in (0, 20):
                for by_row in (False, True):
                    for margin in (0, 5, U64):
                        ch = pix.chains(band=band, min_score=min_score, by_row=by_row, mapq=True, mapq_margin=margin)
                        m = model_of(sd, ch, lens, band, margin, cache=cache)
                        same(ch, m, (what, band, min_score, by_row, margin))
                        assert pix.mapq_stats() == m.stats, (what, band, min_score, by_row, margin)
                        full = np.diff(ch.chain_off.astype(np.int64)) > 0
                        assert not ch.second_score[~full].any() and not ch.mapq[~full].any()
                        if margin == U64:
                            assert not ch.second_score.any() and ch.second_off[-1] == 0
                        if not by_row:
                            assert (ch.second_score <= ch.score).all()
                        else:
                            seen["above"] += int((ch.second_score > ch.score).sum())
                            assert not ch.mapq[ch.second_score > ch.score].any()
                        if (band, min_score, by_row, margin) == (None, 0, False, 0):
                            L = np.maximum(np.array(lens, dtype=np.int64), 1)
                            seen["equal"] = max(seen["equal"], int((full & (ch.second_score == ch.score) & (ch.mapq == 0)).sum()))
                            seen["less"] = max(seen["less"], int(((ch.second_score > 0) & (ch.second_score < ch.score)).sum()))
                            seen["none"] = max(seen["none"], int((full & (ch.second_score == 0) &
                                                                  (ch.mapq == 60 * ch.score.astype(np.int64) // L)).sum()))
        # through seeds(chain=True, mapq=True): the same object
        sd2 = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, chain=True, band=8, min_score=20, mapq=True, mapq_margin=5)
        same(sd2.chains, model_of(sd2, sd2.chains, lens, 8, 5), (what, "seeds"))
        assert sd2.chains.mapq_ms > 0 or len(sd2.occ.start_col) == 0             # one block: no edge, no start place
        assert pix.seeds(reads, chain=True).chains.mapq is None


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 300), (40, 400)])
@pytest.mark.parametrize("gaps", [False, True])
def test_model_parity_plain_and_by_row_on_planted_copies(engine, shape, gaps):
    rng = np.random.default_rng(shape[0] * 10 + gaps)
    A = planted(rng, *shape, gaps)
    reads = cut_reads(rng, A)
    assert 200 <= len(reads) <= 220 and reads[-1] == b"" and min(len(r) for r in reads[:-1]) >= 20
    seen = dict(equal=0, less=0, none=0, above=0)
    for bounds in ([int(x) for x in engine.minmax_dp(engine.elastic_f(A))], fixed_cuts(A.shape[1])):
        parity(engine, A, reads, bounds, (shape, gaps, len(bounds)), seen)
    assert seen["equal"] >= 20 and seen["less"] >= 20 and seen["none"] >= 20, seen
    # the model decides whether a secondary beats the chain of the chosen row: recorded, not required
    assert seen["above"] >= 0, "reads with second > score after by-row: %d" % seen["above"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", TC.GOLDEN, ids=os.path.basename)
def test_model_parity_plain_and_by_row_on_the_golden_files(engine, path):
    A = read_fasta(path)[0]
    rng = np.random.default_rng(len(A[0]))
    reads = TC.chain_reads(rng, A) + [bytes(rng.choice(list(b"ACGT"), int(rng.integers(30, 61))).astype(np.uint8)) for _ in range(10)] + [b""]
    seen = dict(equal=0, less=0, none=0, above=0)
    for bounds in ([int(x) for x in engine.minmax_dp(engine.elastic_f(A))], fixed_cuts(A.shape[1])):
        parity(engine, A, reads, bounds, (os.path.basename(path), len(bounds)), seen)
    assert seen["none"] > 0, seen


@pytest.mark.gpu
def test_tiers_agree_alone_and_mixed(engine):
    A, b = TC.tier_msa()
    rng = np.random.default_rng(5)
    with TC.build(engine, A, b) as pix:
        st = pix.chain_stats()
        sm, lm = st["small_max"], st["lds_max"]
        counts = [1, 2, sm // 16 + 1, lm // 16 + 1]
        reads = [TC.tier_read(rng, s) for s in counts] + [b"", b"TT"]
        lens = [len(r) for r in reads]
        sd = pix.seeds(reads, min_length=12, max_per_seed=16, msa=True)
        places = [s * 16 for s in counts]
        assert (np.diff(sd.occ.start_off.astype(np.int64)) == 16).all() and places[2] > sm and places[3] > lm
        for band in (None, 6):
            for margin in (0, 5):
                mixed = pix.chains(band=band, mapq=True, mapq_margin=margin)
                st = pix.chain_stats()
                assert [st["reads_small"], st["reads_wave"], st["reads_spill"]] == [2, 1, 1]
                m = model_of(sd, mixed, lens, band, margin)
                same(mixed, m, (band, margin, "mixed"))
                assert pix.mapq_stats() == m.stats
                assert (mixed.second_score[:2] > 0).all()           # another copy of the unit, beyond the margin
        together = [(int(mixed.second_score[r]), int(mixed.second_lo[r]), int(mixed.second_hi[r]), int(mixed.mapq[r])) +
                    tuple(mixed.second(r).T.tolist()) for r in range(len(counts))]
        for r, read in enumerate(reads[:len(counts)]):
            one = pix.seeds([read], min_length=12, max_per_seed=16, msa=True, chain=True, band=6, mapq=True, mapq_margin=5).chains
            base = int(sd.occ.start_off[int(sd.seed_off[r])]), int(sd.seed_off[r])
            pl, se = one.second(0).T.tolist()
            assert (int(one.second_score[0]), int(one.second_lo[0]), int(one.second_hi[0]), int(one.mapq[0]),
                    [x + base[0] for x in pl], [x + base[1] for x in se]) == together[r], r


def palindrome_input():
    """6 x 300, similar rows, with a 30-symbol reverse-complement palindrome planted in every row at [120, 150)."""
    rng = np.random.default_rng(77)
    A = random_msa(rng, 6, 300, similar=0.9)
    A[:, 220:280] = A[:, 40:100]
    w = bytes(rng.choice(list(b"ACGT"), 15).astype(np.uint8))
    pal = w + STM.revcomp(w, TR.TABLE)
    assert pal == STM.revcomp(pal, TR.TABLE)
    A[:, 120:150] = np.frombuffer(pal, dtype=np.uint8)
    return rng, A, pal


@pytest.mark.gpu
def test_strands(engine):
    rng, A, pal = palindrome_input()
    fwd = cut_reads(rng, A)[::4]
    reads = [pal] + fwd + [STM.revcomp(r, TR.TABLE) for r in fwd[:20]]
    k = len(reads)
    lens = [len(r) for r in reads] * 2
    with TR.build(engine, A, fixed_cuts(A.shape[1])) as pix:
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        for band, min_score, by_row, margin in ((None, 0, False, 0), (8, 20, False, 5), (8, 20, True, 0), (None, 0, True, U64)):
            ch = pix.chains(band=band, min_score=min_score, by_row=by_row, mapq=True, mapq_margin=margin)
            m = model_of(sd, ch, lens, band, margin, stranded=True)
            same(ch, m, (band, min_score, by_row, margin))
            assert ch.mapq_stranded.dtype == np.uint8 and np.array_equal(ch.mapq_stranded, m.mapq_stranded)
            assert (ch.mapq_stranded <= ch.mapq).all()
            want = [0 if s == STM.NONE else int(m.mapq_stranded[s * k + R]) for R, s in enumerate(ch.strand.tolist())]
            assert ch.best_mapq.dtype == np.uint8 and ch.best_mapq.tolist() == want
            # the palindrome: the same seeds on both strands, the same score, 0 on both
            assert ch.score[0] == ch.score[k] > 0 and ch.mapq_stranded[0] == 0 and ch.mapq_stranded[k] == 0 and ch.best_mapq[0] == 0
        assert (ch.mapq_stranded > 0).any()


def c_mapq(pix, n, margin, want=(1, 1, 1, 1)):
    """The C ABI: -> rc, (second_off, second, second_lo, second_hi, mapq)."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    off = np.full(n + 2, 7, dtype=np.uint64)
    arr = [np.full(n + 1, 7, dtype=np.uint32) for _ in range(3)]
    mq = np.full(n + 1, 7, dtype=np.uint8)
    rc = L.fbg_pindex_chains_mapq(pix._h, margin, off.ctypes.data_as(_lib.u64p),
                                  *[a.ctypes.data_as(_lib.u32p) if w else None for a, w in zip(arr, want)],
                                  mq.ctypes.data_as(_lib.u8p) if want[3] else None, None)
    if rc == 0:
        assert off[n + 1] == 7 and all(a[n] == 7 for a in arr) and mq[n] == 7        # nothing past the n entries
    return rc, (off[:n + 1], arr[0][:n], arr[1][:n], arr[2][:n], mq[:n])


def fetched(pix, n, given, words, graph):
    """What the fetch calls of the other stages return right now, through the C calls."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32, u64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    big = 1 << 16
    out = [np.zeros(big, dtype=np.uint32) for _ in range(2)]
    assert L.fbg_pindex_chains_fetch(pix._h, u32(out[0]), u32(out[1]), None) == 0
    strand, best = np.zeros(given + 1, dtype=np.uint8), np.zeros(given + 1, dtype=np.uint32)
    cnt = [ctypes.c_uint64(0) for _ in range(3)]
    assert L.fbg_pindex_chain_strands(pix._h, strand.ctypes.data_as(_lib.u8p), u32(best), *[ctypes.byref(x) for x in cnt], None) == 0
    out += [strand, best, np.array([x.value for x in cnt])]
    nr, fr, bits = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32), np.zeros(n * words + 1, dtype=np.uint64)
    assert L.fbg_pindex_chains_rows(pix._h, u32(nr), u32(fr), u64(bits), None) == 0
    out += [nr, fr, bits]
    coff, ops = np.zeros(n + 1, dtype=np.uint64), np.zeros(big, dtype=np.uint32)
    assert L.fbg_pindex_chains_cigar_fetch(pix._h, u64(coff), u32(ops)) == 0
    out += [coff, ops]
    if graph:
        poff, nodes = np.zeros(n + 1, dtype=np.uint64), np.zeros(big, dtype=np.uint32)
        assert L.fbg_pindex_chains_align_graph_fetch(pix._h, u64(poff), u32(nodes)) == 0
        goff, gops = np.zeros(n + 1, dtype=np.uint64), np.zeros(big, dtype=np.uint32)
        assert L.fbg_pindex_chains_graph_cigar_fetch(pix._h, u64(goff), u32(gops)) == 0
        out += [poff, nodes, goff, gops]
    out += [v for v in pix.chain_stats().values()] + [v for v in pix.align_stats().values()] + [v for v in pix.cigar_stats().values()]
    return out


ALIGNED = ("align_row", "edits", "t_start", "t_end", "cigar_off", "cigar_ops")
ON_GRAPH = ("graph_edits", "graph_start", "graph_end", "graph_path_off", "graph_path_nodes", "graph_cigar_off", "graph_cigar_ops")


@pytest.mark.gpu
def test_a_mapq_call_leaves_every_other_state_alone(engine):
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    rng, A, pal = palindrome_input()
    reads = cut_reads(rng, A)[::10][:19] + [pal]
    assert len(reads) == 20
    k, n = len(reads), 2 * len(reads)
    lens = [len(r) for r in reads] * 2
    with TR.build(engine, A, fixed_cuts(A.shape[1])) as pix:
        words = pix.rows_stats()["words_per_set"]
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        seeds0 = TC.seeds_state(pix, len(sd.q_start))
        for by_row in (False, True):
            ch = pix.chains(band=8, by_row=by_row, rows=True, align=True, cigar=True, graph=True, graph_cigar=True)
            assert (ch.edits != NONE).any() and (ch.graph_edits != NONE).any()
            before = fetched(pix, n, k, words, True)
            rc, first = c_mapq(pix, n, 0)
            assert rc == 0
            m0 = model_of(sd, ch, lens, 8, 0)
            for got, f in zip(first, ("second_off", "second", "second_lo", "second_hi", "mapq")):
                assert np.array_equal(got, getattr(m0, f)), f
            # a second call with another margin replaces the first; every output but second_off may be NULL
            rc, second = c_mapq(pix, n, 25, want=(0, 0, 0, 0))
            m25 = model_of(sd, ch, lens, 8, 25)
            assert rc == 0 and np.array_equal(second[0], m25.second_off) and not np.array_equal(m0.second, m25.second)
            t = int(second[0][n])
            place, seed = np.zeros(t + 1, dtype=np.uint32), np.zeros(t + 1, dtype=np.uint32)
            for _ in range(2):                                                  # the fetch may be repeated, either array may be NULL
                assert L.fbg_pindex_chains_mapq_fetch(pix._h, place.ctypes.data_as(_lib.u32p), None, None) == 0
                assert L.fbg_pindex_chains_mapq_fetch(pix._h, None, seed.ctypes.data_as(_lib.u32p), None) == 0
                assert np.array_equal(place[:t], m25.second_place) and np.array_equal(seed[:t], m25.second_seed)
            smq = np.zeros(n, dtype=np.uint8)
            assert L.fbg_pindex_mapq_strands(pix._h, smq.ctypes.data_as(_lib.u8p), None) == 0
            assert np.array_equal(smq, model_of(sd, ch, lens, 8, 25, stranded=True).mapq_stranded)
            assert pix.mapq_stats() == m25.stats
            after = fetched(pix, n, k, words, True)
            for x, y in zip(before, after):
                assert np.array_equal(x, y)
            for x, y in zip(seeds0, TC.seeds_state(pix, len(sd.q_start))):
                assert np.array_equal(x, y)
            # the stages run again on what the mapq call left: the same outputs as before it
            pix.locate([b"ACGT" * 40, b"T"])                                    # and the reads on the device are overwritten
            rc, again = c_mapq(pix, n, 0)
            assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(first, again))
            again = pix.chains(band=8, by_row=by_row, rows=True, align=True, cigar=True, graph=True, graph_cigar=True)
            for f in TR.CHAIN_FIELDS + ("strand", "best_score", "n_rows", "first_row", "row_bits") + ALIGNED + ON_GRAPH:
                assert np.array_equal(getattr(again, f), getattr(ch, f)), f


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    L = _lib.lib()
    INVALID = _lib.FBG_ERR_INVALID
    rng, A, pal = palindrome_input()
    reads = cut_reads(rng, A)[::10]
    n = len(reads)
    lens = [len(r) for r in reads]
    dummy, dummy8 = np.zeros(4096, dtype=np.uint32), np.zeros(4096, dtype=np.uint8)
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    fetch = lambda pix: L.fbg_pindex_chains_mapq_fetch(pix._h, u32(dummy), u32(dummy), None)      # noqa: E731
    strands = lambda pix: L.fbg_pindex_mapq_strands(pix._h, dummy8.ctypes.data_as(_lib.u8p), None)      # noqa: E731
    assert L.fbg_pindex_chains_mapq(None, 0, None, None, None, None, None, None) == INVALID
    assert L.fbg_pindex_chains_mapq_fetch(None, None, None, None) == INVALID
    assert L.fbg_pindex_mapq_strands(None, None, None) == INVALID and L.fbg_pindex_mapq_stats(None, None, None, None, None, None) == INVALID
    # an index not built from a segmentation
    with engine.pattern_index([b"ACGT", b"GGA", b"TTC"], [(0, 1), (0, 2)]) as graph:
        graph.seeds([b"ACGTGGA"], max_per_seed=4)
        assert c_mapq(graph, 1, 0)[0] == INVALID and "fbg_pindex_build_segmentation" in engine_error(engine)
        with pytest.raises(FbgError) as ei:
            graph.chains(mapq=True)
        assert ei.value.code == INVALID
    with TR.build(engine, A, fixed_cuts(A.shape[1]), rows=False) as pix:
        # before any seeds call, and before any chaining call
        assert c_mapq(pix, 0, 0)[0] == INVALID
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True)
        assert c_mapq(pix, n, 0)[0] == INVALID and fetch(pix) == INVALID and strands(pix) == INVALID
        assert pix.mapq_stats() == dict.fromkeys(STATS, 0)
        ch = pix.chains(band=8, mapq=True)
        m = model_of(sd, ch, lens, 8, 0)
        same(ch, m, "first")
        assert L.fbg_pindex_chains_mapq(pix._h, 0, None, None, None, None, None, None) == INVALID         # a NULL second_off
        assert fetch(pix) == INVALID                                                                    # ... fails the state too
        assert c_mapq(pix, n, 0)[0] == 0 and fetch(pix) == 0
        assert strands(pix) == INVALID                                          # the seeds were not stranded
        # an index without the row table keeps the read lengths across a locate call
        pix.occurrences([b"GATTACA" * 30], max_per_pattern=4)
        rc, got = c_mapq(pix, n, 0)
        assert rc == 0 and np.array_equal(got[4], m.mapq) and m.mapq.any()
        # a new chaining call invalidates the fetch, the strands call and the statistics
        pix.chains(band=8)
        assert fetch(pix) == INVALID and strands(pix) == INVALID and pix.mapq_stats() == dict.fromkeys(STATS, 0)
        assert c_mapq(pix, n, 0)[0] == 0 and fetch(pix) == 0
        # a new seeds call invalidates the chains and with them the mapq call
        pix.seeds(reads[:3], min_length=4, max_per_seed=16, strands=True)
        assert fetch(pix) == INVALID and c_mapq(pix, 6, 0)[0] == INVALID and strands(pix) == INVALID
        pix.chains()
        assert strands(pix) == INVALID and c_mapq(pix, 6, 0)[0] == 0 and strands(pix) == 0
        # an empty batch, reads without seeds, seeds without places: zeros, FBG_OK
        e = pix.seeds([], msa=True, chain=True, mapq=True).chains
        assert e.second_off.tolist() == [0] and len(e.mapq) == 0 and len(e.second_place) == 0
        e = pix.seeds([b"NN", b""], msa=True, chain=True, mapq=True, strands=True).chains
        assert e.second_score.tolist() == [0] * 4 and e.mapq.tolist() == [0] * 4 and e.mapq_stranded.tolist() == [0] * 4
        assert e.best_mapq.tolist() == [0, 0] and e.second_lo.tolist() == [NONE] * 4 and e.second_hi.tolist() == [NONE] * 4
        e = pix.seeds(reads, min_length=4, max_per_seed=0, msa=True, chain=True, mapq=True)
        assert len(e.q_start) > 0 and e.chains.second_off.tolist() == [0] * (n + 1)
        assert not e.chains.second_score.any() and not e.chains.mapq.any() and (e.chains.second_lo == NONE).all()
        assert pix.mapq_stats() == dict.fromkeys(STATS, 0) and fetch(pix) == 0


def engine_error(engine):
    from founderblockgraphs_amd import _lib
    return _lib.lib().fbg_last_error(engine._h).decode()


def write_fasta(path, A):
    with open(path, "wb") as fh:
        for r, row in enumerate(A):
            fh.write(b">row%d\n%s\n" % (r, row.tobytes()))


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [False, True])
def test_tool_prints_the_qualities_and_writes_them_to_the_gaf(engine, strands, tmp_path):
    from oracle import pyoracle as O
    A = read_fasta(TC.GOLDEN[0])[0]
    b = [int(x) for x in engine.minmax_dp(engine.elastic_f(A))]
    rng = np.random.default_rng(9)
    reads = [r for r in TC.chain_reads(rng, A) if r]
    k = len(reads)
    graph, gaf0, gaf1 = str(tmp_path / "g.xgfa"), str(tmp_path / "base.gaf"), str(tmp_path / "mapq.gaf")
    O.write_xgfa(A, b, graph)
    data = b"".join(r + b"\n" for r in reads)
    args = ["--graph=" + graph, "--msa=" + TC.GOLDEN[0], "--seeds", "--occurrences", "--chain", "--rows", "--graph-align",
            "--graph-cigar"] + (["--strands"] if strands else [])
    base = TC.TL.run_locate(args + ["--gaf=" + gaf0], data)
    got = TC.TL.run_locate(args + ["--gaf=" + gaf1, "--mapq"], data)
    assert base.returncode == 0 and got.returncode == 0, (base.stderr, got.stderr)
    with TR.build(engine, A, b) as pix:
        ch = pix.seeds(reads, min_length=1, max_per_seed=64, msa=True, chain=True, strands=strands, mapq=True).chains
    value = ch.mapq_stranded if strands else ch.mapq
    # the Q lines, in the order of the chains: pattern by pattern, forward and then reverse
    order = [R + s * k for R in range(k) for s in ((0, 1) if strands else (0,))]
    star = lambda x: b"*" if x == NONE else b"%d" % x      # noqa: E731
    want = [b"Q\t%d\t%d\t%s\t%s" % (value[v], ch.second_score[v], star(ch.second_lo[v]), star(ch.second_hi[v])) for v in order]
    lines = got.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith(b"Q\t")] == want
    assert all(lines[i - 1][:2] in (b"C\t", b"A\t") and lines[i + 1][:2] == b"H\t" for i, ln in enumerate(lines) if ln.startswith(b"Q\t"))
    assert any(v > 0 for v in value.tolist())
    if strands:
        assert [int(ln.split(b"\t")[3]) for ln in lines if ln.startswith(b"T\t")] == ch.best_mapq.tolist()
    # column 12 of every GAF record: the value of that read and strand
    records = open(gaf1, "rb").read().splitlines()
    assert records
    for rec in records:
        f = rec.split(b"\t")
        v = int(f[0][4:]) + (k if f[4] == b"-" else 0)
        assert int(f[11]) == value[v], rec
    # without the Q lines, the T lines' third field and column 12: the run without --mapq, byte for byte
    plain = []
    for ln in got.stdout.splitlines(keepends=True):
        if ln.startswith(b"Q\t"):
            continue
        plain.append(ln.rsplit(b"\t", 1)[0] + b"\n" if ln.startswith(b"T\t") else ln)
    assert b"".join(plain) == base.stdout
    back = [b"\t".join(rec.split(b"\t")[:11] + [b"255"] + rec.split(b"\t")[12:]) for rec in records]
    assert b"".join(r + b"\n" for r in back) == open(gaf0, "rb").read()
