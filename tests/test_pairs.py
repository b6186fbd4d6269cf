"""Paired reads: fbg_pindex_chains_pairs, PatternIndex.chains(pairs=, adopt_pairs=) and fbg_locate --pairs
(include/fbg_hip.h, csrc/pindex_pairs.hip).

The checker is tests/pairs_model.py: the definitions of the header on top of chain_model and mapq_model.span_of, applied
to what PatternIndex.seeds(msa=True, strands=True) returns and to the primary chains a chaining call reports (both pinned
by test_seeds, test_strands, test_chains and test_chains_by_row).  On the CPU the model is compared with chain_model's
brute force, and the inputs of the tier and the truth test are checked to be what they claim with the host models of
test_chain_edges.  Every GPU comparison is exact.

Pairs are interleaved: the given reads 2p and 2p + 1.  The golden FASTAs have rows of 14 and 15 symbols: their reads are
those of test_chains.chain_reads paired up, the second mate reverse-complemented, beside pairs with an empty mate, a mate
without seeds and two identical mates."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import chain_model as CM  # noqa: E402
import mapq_model as QM  # noqa: E402
import pairs_model as PM  # noqa: E402
import rows_model as RM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chain_edges as TE  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta  # noqa: E402

NONE = CM.NONE
U64 = QM.U64_MAX
GAP = ord("-")
LOCATE = TC.LOCATE
CALL = "fbg_pindex_chains_pairs"
INSERTS = ((0, 0), (0, 5), (3, 12), (0, U64))
FIELDS = (("pair_which", "which"), ("pair_score", "pair_score"), ("pair_lo", "t_lo"), ("pair_hi", "t_hi"),
          ("rescue_off", "rescue_off"), ("rescue_score", "rescue_score"), ("rescue_lo", "rescue_lo"), ("rescue_hi", "rescue_hi"),
          ("rescue_place", "rescue_place"), ("rescue_seed", "rescue_seed"))


def rc(s):
    return STM.revcomp(s, TR.TABLE)


def virtual(reads):
    return list(reads) + [rc(r) for r in reads]


def fixed_cuts(n):
    return list(range(24, n - 1, 25)) + [n]


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_pairs_call_and_the_header_declares_it():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    assert hasattr(L, CALL) and f"int {CALL}(" in header and CALL in _lib.SIGNATURES
    for words in ("W = [lo(v), lo(v) + max_insert)", "W = [hi(v) - max_insert, hi(v))", "c >= W.lo and c + k <= W.hi",
                  "lo(F) <= lo(R), hi(F) <= hi(R)", "min_insert <= hi(R) - lo(F) <= max_insert", "the smallest number among equals",
                  "counted in MSA witness columns", "Forward-reverse orientation only", "No mapping quality of the pair",
                  "not rescued by alignment"):
        assert words in header, words


def arrays_of(reads):
    """The five arrays of model_inputs() for reads given as anchor lists [(g, t, q, k, c)] (test_chains.random_anchors):
    seeds and places renumbered in order, a place per anchor."""
    seed_off, q, k, start_off, col = [0], [], [], [0], []
    for an in reads:
        last = None
        for _, t, qq, kk, c in an:
            if t != last:
                if last is not None:
                    start_off.append(len(col))
                q.append(qq)
                k.append(kk)
                last = t
            col.append(c)
        if last is not None:
            start_off.append(len(col))
        seed_off.append(len(q))
    return (np.array(seed_off, dtype=np.uint64), np.array(q, dtype=np.uint32), np.array(k, dtype=np.uint32),
            np.array(start_off, dtype=np.uint64), np.array(col, dtype=np.uint32))


def test_model_agrees_with_brute_force():
    rng = np.random.default_rng(12)
    seen = dict(lo_kept=0, lo_dropped=0, hi_kept=0, hi_dropped=0, clamp=0, empty_window=0, which0=0, which1=0, which2=0, which3=0,
                none=0, tie=0, only_empty=0, only_lo=0, only_hi=0, only_insert=0, emptied=0)
    for trial in range(1500):
        inp = arrays_of([TC.random_anchors(rng) for _ in range(4)])       # one pair: a, b, a + n, b + n
        an = [CM.read_anchors(*inp, v) for v in range(4)]
        band = (0, 1, 3, None)[trial % 4]
        min_score = (0, 4)[trial // 4 % 2]
        lo_ins, hi_ins = ((0, 0), (0, 5), (3, 12), (8, 14), (0, U64))[trial % 5]
        off, score, place, seed = CM.chains(*inp, band, min_score)
        m = PM.solve(*inp, off, score, place, seed, band, lo_ins, hi_ins)
        prim = [[a for a in an[v] if a[0] in place[int(off[v]):int(off[v + 1])].tolist()] for v in range(4)]
        pspan = [QM.span_of(c) for c in prim]
        seen["emptied"] += sum(1 for v in range(4) if pspan[v] is None and score[v] > 0)
        resc = []
        for w in range(4):
            v = PM.partner(w, 2)
            assert PM.partner(v, 2) == w and PM.twin(PM.twin(w, 2), 2) == w and v == PM.twin(w ^ 1 if w < 2 else ((w - 2) ^ 1) + 2, 2)
            # the window in the header's words
            if pspan[v] is None:
                kept = []
                seen["empty_window"] += len(an[w]) > 0
            else:
                lo, hi = pspan[v]
                W = (lo, min(lo + hi_ins, U64)) if v < 2 else (max(hi - hi_ins, 0), hi)
                kept = [a for a in an[w] if W[0] <= a[4] and a[4] + a[3] <= W[1]]
                seen["clamp"] += v >= 2 and hi < hi_ins < U64
                seen["lo_kept"] += any(a[4] == W[0] and a in kept for a in an[w])
                seen["lo_dropped"] += any(a[4] == W[0] - 1 for a in an[w])
                seen["hi_kept"] += any(a[4] + a[3] == W[1] and a in kept for a in an[w])
                seen["hi_dropped"] += any(a[4] + a[3] == W[1] + 1 for a in an[w])
                assert not any(a[4] == W[0] - 1 and a in kept for a in an[w]) and not any(a[4] + a[3] == W[1] + 1 and a in kept for a in an[w])
            assert m.kept[w] == len(kept)
            top, at = CM.brute_force(kept, band)
            got = m.rescue_place[int(m.rescue_off[w]):int(m.rescue_off[w + 1])].tolist()
            assert int(m.rescue_score[w]) == top, (trial, w)
            if got:
                # the tie-break minimum among the best: the smallest end, then the smallest predecessor, and so on
                assert tuple([a[0] for a in kept].index(g) for g in got) == min(at, key=lambda sub: sub[::-1]), (trial, w)
            else:
                assert top == 0 and at == []
            ch = [a for a in kept if a[0] in got]
            resc.append(ch)
            assert (int(m.rescue_lo[w]), int(m.rescue_hi[w])) == (QM.span_of(ch) or (NONE, NONE))
        # the pick, from the table of the header
        table = [((prim[0], int(score[0])), (resc[3], int(m.rescue_score[3]))), ((resc[0], int(m.rescue_score[0])), (prim[3], int(score[3]))),
                 ((prim[1], int(score[1])), (resc[2], int(m.rescue_score[2]))), ((resc[1], int(m.rescue_score[1])), (prim[2], int(score[2])))]
        ok = []
        for i, ((F, sf), (R, sr)) in enumerate(table):
            conds = [bool(F) and bool(R)]
            if conds[0]:
                lf, hf, lr, hr = F[0][4], F[-1][4] + F[-1][3], R[0][4], R[-1][4] + R[-1][3]
                conds += [lf <= lr, hf <= hr, lo_ins <= hr - lf <= hi_ins]
                for j, f in enumerate(("only_lo", "only_hi", "only_insert")):
                    seen[f] += not conds[1 + j] and all(c for jj, c in enumerate(conds[1:]) if jj != j)
            else:
                seen["only_empty"] += 1
            if all(conds):
                ok.append((sf + sr, -i, lf, hr))
        if ok:
            sc, i, lf, hr = max(ok)
            assert (int(m.which[0]), int(m.pair_score[0]), int(m.t_lo[0]), int(m.t_hi[0])) == (-i, sc, lf, hr), trial
            seen["which%d" % -i] += 1
            seen["tie"] += sum(1 for x in ok if x[0] == sc) > 1
            f, r, fr, rr = m.chosen[0]
            want = {f: table[-i][0], r: table[-i][1], PM.twin(f, 2): ([], 0), PM.twin(r, 2): ([], 0)}
        else:
            assert (int(m.which[0]), int(m.pair_score[0]), int(m.t_lo[0]), int(m.t_hi[0])) == (PM.NO_PAIR, 0, NONE, NONE)
            assert m.chosen[0] is None
            seen["none"] += 1
            want = {v: (prim[v], int(score[v])) for v in range(4)}
        # adopt
        for v in range(4):
            a, b = int(m.chain_off[v]), int(m.chain_off[v + 1])
            assert m.anchor_place[a:b].tolist() == [x[0] for x in want[v][0]] and int(m.score[v]) == want[v][1], (trial, v)
            assert all(int(inp[3][t]) <= g < int(inp[3][t + 1]) for g, t in zip(m.anchor_place[a:b].tolist(), m.anchor_seed[a:b].tolist()))
        assert m.stats == dict(which0=int(m.which[0] == 0), which1=int(m.which[0] == 1), which2=int(m.which[0] == 2),
                               which3=int(m.which[0] == 3), none=int(m.which[0] == PM.NO_PAIR), places_kept=sum(m.kept),
                               places_excluded=sum(len(x) for x in an) - sum(m.kept), rescue_differs=m.stats["rescue_differs"])
    assert not {f: v for f, v in seen.items() if v < 30}, seen


def usage_error(args, data=b"AG\nCT\n"):
    p = subprocess.run([LOCATE] + args, input=data, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"usage:" in p.stderr, (args, p.stderr)
    return p.stderr


def test_tool_pairs_needs_its_prerequisites(tmp_path):
    from oracle import pyoracle as O
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--pairs=MIN,MAX" in p.stderr
    head = open(os.path.join(ROOT, "founderblockgraphs_amd", "csrc", "host", "locate_main.cpp")).read().split("#include")[0]
    assert "--pairs=MIN,MAX" in head and "Z <tab> which <tab> pair_score <tab> t_lo <tab> t_hi" in head
    full = ["--graph=" + TC.SPEC, "--seeds=3", "--occurrences=4", "--msa=" + TC.GOLDEN[0]]
    for args in (full + ["--strands", "--pairs=0,9"], full + ["--chain", "--pairs=0,9"], ["--graph=" + TC.SPEC, "--pairs=0,9"]):
        assert b"--pairs needs --chain and --strands" in usage_error(args)
    for bad in ("x", "5", "9,3", "", "1,", ",4", "1,2,3", "-1,4"):
        assert b"--pairs takes MIN,MAX with MIN <= MAX, not '" + bad.encode() + b"'" in usage_error(full + ["--chain", "--strands", "--pairs=" + bad])
    assert b"unknown argument --pairs" in usage_error(full + ["--chain", "--strands", "--pairs"])
    # an odd number of patterns: known once they are read, with a graph that fits the MSA
    A = read_fasta(TC.GOLDEN[0])[0]
    graph = str(tmp_path / "g.xgfa")
    O.write_xgfa(A, [int(x) for x in O.minmax_dp(O.compute_f(A))[2]], graph)
    args = ["--graph=" + graph, "--seeds", "--occurrences", "--msa=" + TC.GOLDEN[0], "--chain", "--strands", "--pairs=0,9"]
    assert b"--pairs takes an even number of patterns" in usage_error(args, b"AG\nCT\nGG\n")


def tier_reads():
    """Two pairs on test_chains.tier_msa, mates of rotations of its unit as test_chain_edges.many_reads builds them: 1280
    start places each in the first pair, 160 in the second.  The second mate is given reverse-complemented, so the
    virtual reads with places are a = 0 (and 2) and b + n = 5 (and 7)."""
    rng = np.random.default_rng(3)
    mk = lambda places: b"".join(TE.rot(int(r)) + b"T" for r in rng.integers(0, 12, places // 16))      # noqa: E731
    X, Y, X2, Y2 = mk(1280), mk(1280), mk(160), mk(160)
    return [X, rc(Y), X2, rc(Y2)]


def test_tier_input_is_what_it_claims():
    inp = TE.host("tier").seeds(virtual(tier_reads()), 12, 16)
    assert TE.places_per_read(inp).tolist() == [1280, 0, 160, 0, 0, 1280, 0, 160]
    off, score, place, seed = CM.chains(*inp, None, 0)
    m = PM.solve(*inp, off, score, place, seed, None, 0, U64)
    assert m.kept[0] > TE.LDS_MAX and m.kept[5] > TE.LDS_MAX and TE.SM_MAX < m.kept[2] <= TE.LDS_MAX and TE.SM_MAX < m.kept[7] <= TE.LDS_MAX
    assert m.which.tolist() == [0, 0] or set(m.which.tolist()) <= {0, 1}
    m2 = PM.solve(*inp, off, score, place, seed, None, 0, 300)
    assert m2.stats["rescue_differs"] + m2.stats["none"] > 0          # a bounded insert cuts the long chains


def truth_input():
    """8 similar rows x 600 columns without gaps, a star phylogeny at 1 %; the 40 columns from 160 on copied to 400 on, 240
    columns away, and either copy altered in one symbol of one row.  64 error-free pairs of 30-symbol mates from fragments
    of 100 .. 150 columns, exactly one mate inside a copy -> (MSA, boundaries, reads, the fragments' columns)."""
    rng = np.random.default_rng(5)
    A = random_msa(rng, 8, 600, similar=0.99)
    A[:, 400:440] = A[:, 160:200]
    for r, c in ((2, 178), (5, 421)):
        A[r, c] = ord("ACGT"["ACGT".index(chr(A[r, c])) - 1])
    reads, frag = [], []
    for p in range(64):
        f, r = int(rng.integers(100, 151)), int(rng.integers(0, 8))
        inside = (160, 400)[p % 2] + int(rng.integers(0, 11))
        a = inside if p % 4 < 2 else inside + 30 - f          # the forward mate inside a copy, or the reverse one
        row = A[r].tobytes()
        m1, m2 = row[a:a + 30], rc(row[a + f - 30:a + f])
        reads += [m1, m2] if p % 3 else [m2, m1]
        frag.append((a, a + f))
        in_copy = [160 <= x and x + 30 <= 200 or 400 <= x and x + 30 <= 440 for x in (a, a + f - 30)]
        touches = [x < 200 and x + 30 > 160 or x < 440 and x + 30 > 400 for x in (a, a + f - 30)]
        assert sum(in_copy) == 1 and sum(touches) == 1 and 0 <= a and a + f <= 600
    return A, fixed_cuts(600), reads, frag


def rescued_wrong_primaries(m, start_col, chain_off, anchor_place):
    """Pairs whose chosen candidate uses a rescue chain while that read's primary chain lies in other columns."""
    count = 0
    for c in m.chosen:
        if c is None:
            continue
        f, r, fr, rr = c
        w = f if fr else r
        prim = start_col[anchor_place[int(chain_off[w]):int(chain_off[w + 1])]].tolist()
        resc = start_col[m.rescue_place[int(m.rescue_off[w]):int(m.rescue_off[w + 1])]].tolist()
        count += prim != resc
    return count


def check_truth(m, frag, start_col, chain_off, anchor_place):
    for p, (lo, hi) in enumerate(frag):
        assert (int(m.pair_score[p]), int(m.t_lo[p]), int(m.t_hi[p])) == (60, lo, hi), p
    wrong = rescued_wrong_primaries(m, start_col, chain_off, anchor_place)
    assert wrong >= 8, wrong
    return wrong


def test_truth_input_is_what_it_claims():
    A, b, reads, frag = truth_input()
    inp = TE.HostModel(A, b).seeds(virtual(reads), 4, 16)
    off, score, place, seed = CM.chains(*inp, None, 0)
    check_truth(PM.solve(*inp, off, score, place, seed, None, 0, 150), frag, inp[4], off, place)


# ---- GPU ----------------------------------------------------------------------------------------------------------

def same(ch, m, what):
    for f, g in FIELDS:
        got, want = getattr(ch, f), getattr(m, g)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f, got.tolist(), want.tolist())
    assert ch.pair_stats == m.stats, (what, ch.pair_stats, m.stats)
    n = len(ch.pair_which) * 2
    for p, c in enumerate(m.chosen):
        assert ch.pair(p) == c, (what, p)
    for v in (0, 2 * n - 1) if n else ():
        a, b = int(m.rescue_off[v]), int(m.rescue_off[v + 1])
        assert ch.rescue(v).tolist() == np.stack((m.rescue_place[a:b], m.rescue_seed[a:b]), axis=1).tolist()


def same_adopted(ch, m, what):
    for f in TR.CHAIN_FIELDS:
        got, want = getattr(ch, f), getattr(m, f)
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, f, got.tolist(), want.tolist())


def model_of(sd, ch0, band, ins, cache=None):
    return PM.solve(*TC.model_inputs(sd), ch0.chain_off, ch0.score, ch0.anchor_place, ch0.anchor_seed, band, ins[0], ins[1], cache)


def strands_of(m, n):
    """What fbg_pindex_chain_strands says of chains (chain_off, score): strand and best score per given read."""
    full = np.diff(m.chain_off.astype(np.int64)) > 0
    t = m.score[n:] > m.score[:n]
    pick = np.where(t, n, 0) + np.arange(n)
    return np.where(full[pick], t.astype(np.uint8), np.uint8(0xff)).astype(np.uint8), np.maximum(m.score[:n], m.score[n:])


def golden_pairs(rng, A):
    rs = TC.chain_reads(rng, A)
    reads = []
    for i in range(0, len(rs) - 1, 2):
        reads += [rs[i], rc(rs[i + 1])] if i % 4 == 0 else [rc(rs[i]), rs[i + 1]]
    x = rs[0]
    return reads + [b"", rc(x), x, b"", b"NN", rc(x), x, x, x, rc(x), x[:7], rc(x[7:])]


@pytest.mark.gpu
@pytest.mark.parametrize("path", TC.GOLDEN, ids=os.path.basename)
def test_model_parity_plain_and_by_row_on_the_golden_files(engine, path):
    A = read_fasta(path)[0]
    reads = golden_pairs(np.random.default_rng(len(A[0])), A)
    assert len(reads) % 2 == 0
    seen = dict(proper=0, none=0, emptied=0, rescue=0)
    for bounds in ([int(x) for x in engine.minmax_dp(engine.elastic_f(A))], fixed_cuts(A.shape[1])):
        with TR.build(engine, A, bounds) as pix:
            sd = pix.seeds(reads, min_length=2, max_per_seed=16, msa=True, strands=True)
            scores = pix.chains().score
            mid = int(scores[scores > 0].min()) + 1 if (scores > 0).any() else 1      # empties the chains of the smallest score
            cache = {}
            for band in (None, 1):
                for min_score in (0, mid):
                    for by_row in (False, True):
                        ch0 = pix.chains(band=band, min_score=min_score, by_row=by_row)
                        seen["emptied"] += int(((np.diff(ch0.chain_off.astype(np.int64)) == 0) & (ch0.score > 0)).sum())
                        for ins in INSERTS:
                            what = (os.path.basename(path), len(bounds), band, min_score, by_row, ins)
                            m = model_of(sd, ch0, band, ins, cache)
                            ch = pix.chains(band=band, min_score=min_score, by_row=by_row, pairs=ins)
                            same(ch, m, what)
                            same_adopted(ch, ch0, what)                       # without adopt the chains are the primaries
                            assert ch.pairs_ms > 0 or len(sd.occ.start_col) == 0
                            if ins == (0, 0):
                                assert (ch.pair_which == PM.NO_PAIR).all() and ch.rescue_off[-1] == 0
                            ad = pix.chains(band=band, min_score=min_score, by_row=by_row, pairs=ins, adopt_pairs=True)
                            same(ad, m, what + ("adopt",))
                            same_adopted(ad, m, what + ("adopt",))
                            seen["proper"] += int((m.which != PM.NO_PAIR).sum())
                            seen["none"] += int((m.which == PM.NO_PAIR).sum())
                            seen["rescue"] += m.stats["rescue_differs"]
    assert all(v > 0 for f, v in seen.items() if f != "rescue"), seen


def random_pairs(rng, A, count=64):
    """`count` pairs of 30-symbol mates from fragments of 40 .. 120 columns of a row, gaps stripped, 0 .. 2 substitutions
    per mate, in either order."""
    reads = []
    while len(reads) < 2 * count:
        f, r = int(rng.integers(40, 121)), int(rng.integers(0, len(A)))
        a = int(rng.integers(0, A.shape[1] - f + 1))
        s = A[r, a:a + f]
        s = s[s != GAP].tobytes()
        if len(s) < 30:
            continue
        mates = []
        for mate in (s[:30], rc(s[-30:])):
            mate = bytearray(mate)
            for _ in range(int(rng.integers(0, 3))):
                at = int(rng.integers(0, 30))
                mate[at] = rng.choice([c for c in b"ACGT" if c != mate[at]])
            mates.append(bytes(mate))
        reads += mates if len(reads) % 4 else mates[::-1]
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [False, True])
def test_model_parity_on_random_msas(engine, gaps):
    rng = np.random.default_rng(40 + gaps)
    A = random_msa(rng, 6, 300, gap_p=0.02, gap_run=3, similar=0.9) if gaps else random_msa(rng, 6, 300, similar=0.9)
    reads = random_pairs(rng, A)
    proper = 0
    with TR.build(engine, A, fixed_cuts(300)) as pix:
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        cache = {}
        for band, min_score, by_row, ins in ((None, 0, False, (30, 130)), (8, 12, False, (0, 60)), (8, 0, True, (30, 130)),
                                             (None, 12, True, (0, U64))):
            ch0 = pix.chains(band=band, min_score=min_score, by_row=by_row)
            m = model_of(sd, ch0, band, ins, cache)
            ch = pix.chains(band=band, min_score=min_score, by_row=by_row, pairs=ins, adopt_pairs=True)
            same(ch, m, (gaps, band, min_score, by_row, ins))
            same_adopted(ch, m, (gaps, band, min_score, by_row, ins))
            proper += int((m.which != PM.NO_PAIR).sum())
    assert proper > 0


@pytest.mark.gpu
def test_rescue_chains_in_the_wave_and_spill_tiers(engine):
    A, b = TC.tier_msa()
    reads = tier_reads()
    with TC.build(engine, A, b) as pix:
        sd = pix.seeds(reads, min_length=12, max_per_seed=16, msa=True, strands=True)
        for band in (None, 6):
            for ins in ((0, U64), (0, 300)):
                ch0 = pix.chains(band=band)
                m = model_of(sd, ch0, band, ins)
                ch = pix.chains(band=band, pairs=ins)
                same(ch, m, (band, ins))
                # a read's tier follows from its start places, kept or not: the rescue run has the tiers of the primary one
                st = pix.chain_stats()
                assert [st["reads_small"], st["reads_wave"], st["reads_spill"]] == [0, 2, 2]
                if ins[1] == U64:
                    assert m.kept[0] > st["lds_max"] and m.kept[5] > st["lds_max"]
                    assert st["small_max"] < m.kept[2] <= st["lds_max"] and st["small_max"] < m.kept[7] <= st["lds_max"]
                    assert ch.pair_stats["places_kept"] == sum(m.kept) > 2 * st["lds_max"]
                ad = pix.chains(band=band, pairs=ins, adopt_pairs=True)
                same_adopted(ad, m, (band, ins, "adopt"))


def c_pairs(pix, V, ins, adopt=False, nseeds=0):
    """The C ABI -> rc, the outputs in the order of the signature (adopt_chain_off and adopt_score last)."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    P = V // 4
    u32, u64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    which = np.full(P + 1, 7, dtype=np.uint8)
    per_pair = [np.full(P + 1, 7, dtype=np.uint32) for _ in range(3)]
    roff = np.full(V + 2, 7, dtype=np.uint64)
    per_read = [np.full(V + 1, 7, dtype=np.uint32) for _ in range(3)]
    anchors = [np.full(nseeds + 1, 7, dtype=np.uint32) for _ in range(2)]
    aoff, asc = np.full(V + 2, 7, dtype=np.uint64), np.full(V + 1, 7, dtype=np.uint32)
    stats = np.full(9, 7, dtype=np.uint64)
    code = L.fbg_pindex_chains_pairs(pix._h, ins[0], ins[1], which.ctypes.data_as(_lib.u8p), *[u32(a) for a in per_pair], u64(roff),
                                     *[u32(a) for a in per_read], *[u32(a) for a in anchors], u64(aoff) if adopt else None,
                                     u32(asc) if adopt else None, u64(stats), None)
    if code == 0:      # nothing past the entries of each array
        assert which[P] == 7 and all(a[P] == 7 for a in per_pair) and roff[V + 1] == 7 and all(a[V] == 7 for a in per_read)
        assert stats[8] == 7 and all(a[nseeds] == 7 for a in anchors) and (not adopt or (aoff[V + 1] == 7 and asc[V] == 7))
    return code, [which[:P]] + [a[:P] for a in per_pair] + [roff[:V + 1]] + [a[:V] for a in per_read] + \
        [a[:int(roff[V]) if code == 0 else 0] for a in anchors] + [aoff[:V + 1], asc[:V]], stats[:8]


def engine_error(engine):
    from founderblockgraphs_amd import _lib
    return _lib.lib().fbg_last_error(engine._h).decode()


@pytest.mark.gpu
def test_errors_leave_the_index_working(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    INVALID = _lib.FBG_ERR_INVALID
    rng = np.random.default_rng(8)
    A = random_msa(rng, 6, 300, similar=0.9)
    reads = random_pairs(rng, A, 8)
    V = 2 * len(reads)

    def fails(pix, V, ins=(0, 100)):
        code = c_pairs(pix, V, ins)[0]
        msg = engine_error(engine)
        assert code == INVALID and CALL in msg, (code, msg)
        return msg

    assert _lib.lib().fbg_pindex_chains_pairs(None, 0, 0, *[None] * 14) == INVALID
    with engine.pattern_index([b"ACGT", b"GGA", b"TTC"], [(0, 1), (0, 2)]) as graph:      # no index of a segmentation
        graph.seeds([b"ACGTGGA", b"TCC"], max_per_seed=4, strands=True)
        assert "fbg_pindex_build_segmentation" in fails(graph, 4)
    with TR.build(engine, A, fixed_cuts(300), rows=False) as pix:
        fails(pix, 0)                                                           # before any seeds call
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True)
        ch0 = pix.chains(band=8)
        assert "fbg_pindex_seeds_strands" in fails(pix, len(reads) // 2 * 2)    # plain seeds, chained
        TC.same(pix.chains(band=8), [getattr(ch0, f) for f in TC.FIELDS], "after a failed call")
        with pytest.raises(ValueError):
            pix.chains(pairs=(0, 100))
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        assert "fbg_pindex_chains" in fails(pix, V)                             # no chaining call
        ch0 = pix.chains(band=8)
        assert "min_insert" in fails(pix, V, (5, 4))
        from founderblockgraphs_amd import _lib as LL
        roff = np.zeros(V + 1, dtype=np.uint64)
        which = np.zeros(V // 4, dtype=np.uint8)
        null_which = LL.lib().fbg_pindex_chains_pairs(pix._h, 0, 9, None, None, None, None, roff.ctypes.data_as(LL.u64p), *[None] * 9)
        null_off = LL.lib().fbg_pindex_chains_pairs(pix._h, 0, 9, which.ctypes.data_as(LL.u8p), *[None] * 13)
        assert null_which == INVALID and null_off == INVALID and CALL in engine_error(engine)
        # after the failed calls the index still works, and no stage went stale
        m = model_of(sd, ch0, 8, (30, 130))
        code, out, stats = c_pairs(pix, V, (30, 130), nseeds=len(sd.q_start))
        assert code == 0 and dict(zip(PM.STATS, stats.tolist())) == m.stats
        for got, f in zip(out, [g for _, g in FIELDS]):
            assert np.array_equal(got, getattr(m, f)), f
        TC.same(pix.chains(band=8), [getattr(ch0, f) for f in TC.FIELDS], "after the calls")
        # an odd number of reads
        pix.seeds(reads[:3], min_length=4, max_per_seed=16, msa=True, strands=True)
        pix.chains()
        assert "even" in fails(pix, 6)
        with pytest.raises(FbgError) as ei:
            pix.chains(pairs=(0, 100))
        assert ei.value.code == INVALID
        assert pix.chains().chain_off.shape == (7,)
        # no reads, reads without seeds, seeds without places: every pair none, every rescue chain empty
        e = pix.seeds([], msa=True, strands=True, chain=True).chains
        e = pix.chains(pairs=(0, 9), adopt_pairs=True)
        assert len(e.pair_which) == 0 and e.rescue_off.tolist() == [0] and e.pair_stats == dict.fromkeys(PM.STATS, 0)
        pix.seeds([b"NN", b"", b"N", b"NNN"], msa=True, strands=True)
        for adopt in (False, True):
            e = pix.chains(pairs=(0, 9), adopt_pairs=adopt)
            assert e.pair_which.tolist() == [0xff] * 2 and e.pair_score.tolist() == [0, 0] and e.pair_lo.tolist() == [NONE] * 2
            assert e.pair_hi.tolist() == [NONE] * 2 and e.rescue_off.tolist() == [0] * 9 and e.rescue_lo.tolist() == [NONE] * 8
            assert e.pair_stats == dict(dict.fromkeys(PM.STATS, 0), none=2) and e.pair(0) is None and e.pairs_ms == 0
            assert e.chain_off.tolist() == [0] * 9 and e.strand.tolist() == [0xff] * 4
        s0 = pix.seeds(reads, min_length=4, max_per_seed=0, msa=True, strands=True)
        e = pix.chains(pairs=(0, U64), adopt_pairs=True)
        assert len(s0.q_start) > 0 and (e.pair_which == 0xff).all() and e.rescue_off.tolist() == [0] * (V + 1)


ALIGNED = ("align_row", "edits", "t_start", "t_end")


@pytest.mark.gpu
@pytest.mark.parametrize("by_row", [False, True])
def test_adopt(engine, by_row):
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    INVALID = _lib.FBG_ERR_INVALID
    rng = np.random.default_rng(21 + by_row)
    A = random_msa(rng, 6, 300, similar=0.9)
    A[:, 200:240] = A[:, 60:100]                     # a copy: some primaries lie at the other one
    reads = random_pairs(rng, A, 30) + [b"", rc(A[0, 10:40].tobytes()), b"NN", b"NNN"]
    n, V = len(reads), 2 * len(reads)
    vreads = virtual(reads)
    lens = [len(r) for r in vreads]
    band, min_score, ins = 8, 14, (30, 130)
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    dummy = [np.zeros(V + 1, dtype=np.uint32) for _ in range(4)]
    with TR.build(engine, A, fixed_cuts(300)) as pix:
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        ch0 = pix.chains(band=band, min_score=min_score, by_row=by_row, align=True, mapq=True)
        m = model_of(sd, ch0, band, ins)
        proper = m.which != PM.NO_PAIR
        assert proper.any() and not proper.all() and (by_row or m.stats["rescue_differs"] > 0)
        assert ((np.diff(ch0.chain_off.astype(np.int64)) == 0) & (ch0.score > 0)).any()           # min_score emptied some
        # without adopt: the chains, their fetch and the done-ness of the align and mapq stages stay
        code, out, _ = c_pairs(pix, V, ins, nseeds=len(sd.q_start))
        assert code == 0
        place, seed = np.zeros(len(sd.q_start) + 1, dtype=np.uint32), np.zeros(len(sd.q_start) + 1, dtype=np.uint32)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(place), u32(seed), None) == 0
        t = int(ch0.chain_off[V])
        assert np.array_equal(place[:t], ch0.anchor_place) and np.array_equal(seed[:t], ch0.anchor_seed)
        assert L.fbg_pindex_chains_mapq_fetch(pix._h, u32(place), u32(seed), None) == 0
        total = ctypes.c_uint64(0)
        assert L.fbg_pindex_chains_cigar(pix._h, None, ctypes.byref(total), None) == 0
        assert pix.mapq_stats()["anchors_kept"] + pix.mapq_stats()["anchors_excluded"] > 0
        # adopt through the C call: the returned arrays and the fetch equal the model
        code, out, stats = c_pairs(pix, V, ins, adopt=True, nseeds=len(sd.q_start))
        assert code == 0 and dict(zip(PM.STATS, stats.tolist())) == m.stats
        assert np.array_equal(out[-2], m.chain_off) and np.array_equal(out[-1], m.score)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(place), u32(seed), None) == 0
        t = int(m.chain_off[V])
        assert np.array_equal(place[:t], m.anchor_place) and np.array_equal(seed[:t], m.anchor_seed)
        # pairs without a candidate keep all four chains bit for bit
        for p in np.flatnonzero(~proper).tolist():
            for v in (2 * p, 2 * p + 1, 2 * p + n, 2 * p + 1 + n):
                a, b, a0, b0 = int(m.chain_off[v]), int(m.chain_off[v + 1]), int(ch0.chain_off[v]), int(ch0.chain_off[v + 1])
                assert place[a:b].tolist() == ch0.anchor_place[a0:b0].tolist() and m.score[v] == ch0.score[v]
        # the strand call returns the chosen strands
        strand, best = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
        assert L.fbg_pindex_chain_strands(pix._h, strand.ctypes.data_as(_lib.u8p), u32(best), None, None, None, None) == 0
        want_strand, want_best = strands_of(m, n)
        assert np.array_equal(strand, want_strand) and np.array_equal(best, want_best)
        for p, c in enumerate(m.chosen):
            if c is not None:
                f, r = c[0], c[1]
                assert strand[f % n] == f // n and strand[r % n] == r // n
        # every stage made from the chains is stale, with px_need's message ...
        for stale in (lambda: L.fbg_pindex_chains_cigar(pix._h, None, ctypes.byref(total), None),
                      lambda: L.fbg_pindex_chains_mapq_fetch(pix._h, u32(place), u32(seed), None)):
            assert stale() == INVALID and "no current" in engine_error(engine)
        assert pix.mapq_stats() == dict.fromkeys(pix.mapq_stats(), 0)
        # ... and run again they equal the models on the adopted chains
        assert L.fbg_pindex_chains_align(pix._h, 16, 0, *[u32(a) for a in dummy], None) == 0
        rm = RM.Model(A, fixed_cuts(300))
        sets = RM.seed_rows(rm, vreads, sd.seed_off, sd.q_start, sd.length, sd.occ.start_off, sd.occ.start_src, sd.occ.start_dst,
                            sd.occ.start_offset)[2]
        chain_sets = RM.chain_rows(rm.m, sets, m.chain_off, m.anchor_place)[3]
        want = AM.chains_align(rm, vreads, m.chain_off, m.anchor_place, m.anchor_seed, chain_sets, sd.q_start, sd.occ.start_src,
                               sd.occ.start_dst, sd.occ.start_offset, 16, 0)
        for got, w in zip(dummy, want[:4]):
            assert np.array_equal(got[:V], w)
        soff = np.zeros(V + 1, dtype=np.uint64)
        mq = np.zeros(V, dtype=np.uint8)
        assert L.fbg_pindex_chains_mapq(pix._h, 0, soff.ctypes.data_as(_lib.u64p), u32(dummy[0]), None, None, mq.ctypes.data_as(_lib.u8p), None) == 0
        qm = QM.solve(*TC.model_inputs(sd), lens, m.chain_off, m.score, m.anchor_place, m.anchor_seed, band, 0)
        assert np.array_equal(soff, qm.second_off) and np.array_equal(dummy[0][:V], qm.second) and np.array_equal(mq, qm.mapq)
        # a second pairs call on the adopted chains: a fixed point for every pair that was proper
        m2 = PM.solve(*TC.model_inputs(sd), m.chain_off, m.score, m.anchor_place, m.anchor_seed, band, ins[0], ins[1])
        code, out2, _ = c_pairs(pix, V, ins, adopt=True, nseeds=len(sd.q_start))
        assert code == 0
        for got, f in zip(out2, [g for _, g in FIELDS]):
            assert np.array_equal(got, getattr(m2, f)), f
        assert np.array_equal(out2[-2], m2.chain_off) and np.array_equal(out2[-1], m2.score)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(place), u32(seed), None) == 0
        # (after the by-row call the rescue chains are not bound to the chosen row: they may score higher than the row's
        # chain, or tie with it on other anchors, so only the chosen reads are required to stay)
        for p in np.flatnonzero(proper).tolist():
            assert m2.chosen[p][:2] == m.chosen[p][:2], p
            if by_row:
                continue
            assert (out2[2][p], out2[3][p], out2[1][p]) == (m.t_lo[p], m.t_hi[p], m.pair_score[p]), p
            for v in m.chosen[p][:2]:
                a, b, a2, b2 = int(m.chain_off[v]), int(m.chain_off[v + 1]), int(out2[-2][v]), int(out2[-2][v + 1])
                assert place[a2:b2].tolist() == m.anchor_place[a:b].tolist() and out2[-1][v] == m.score[v], (p, v)
        # through the Python interface: every field describes the adopted chains
        ch = pix.chains(band=band, min_score=min_score, by_row=by_row, align=True, mapq=True, pairs=ins, adopt_pairs=True)
        same(ch, m, "python")
        same_adopted(ch, m, "python")
        assert np.array_equal(ch.strand, want_strand) and np.array_equal(ch.best_score, want_best)
        for f, w in zip(ALIGNED, want[:4]):
            assert np.array_equal(getattr(ch, f), w), f
        assert np.array_equal(ch.mapq, qm.mapq) and np.array_equal(ch.second_score, qm.second)
        assert ch.by_row == by_row and (not by_row or np.array_equal(ch.chain_row, ch0.chain_row))


@pytest.mark.gpu
def test_truth(engine):
    A, b, reads, frag = truth_input()
    with TR.build(engine, A, b) as pix:
        sd = pix.seeds(reads, min_length=4, max_per_seed=16, msa=True, strands=True)
        ch0 = pix.chains()
        ch = pix.chains(pairs=(0, 150), adopt_pairs=True)
        m = model_of(sd, ch0, None, (0, 150))
        same(ch, m, "truth")
        assert (ch.pair_score == 60).all()
        assert [(int(a), int(b)) for a, b in zip(ch.pair_lo, ch.pair_hi)] == frag
        wrong = check_truth(m, frag, sd.occ.start_col, ch0.chain_off, ch0.anchor_place)
        assert ch.pair_stats["none"] == 0 and wrong >= 8
        # adopted: every given read has its strand, and its chain lies in the fragment
        assert (ch.strand != 0xff).all() and (ch.best_score == 30).all()
        for k in range(len(reads)):
            cols = sd.occ.start_col[ch.best(k)[:, 0]]
            lo, hi = frag[k // 2]
            assert len(cols) and lo <= cols.min() and cols.max() < hi, k


def z_lines(m):
    """The Z line of every pair, as fbg_locate --pairs prints it."""
    return [b"Z\t*" if w == PM.NO_PAIR else b"Z\t%d\t%d\t%d\t%d" % (w, s, lo, hi)
            for w, s, lo, hi in zip(m.which.tolist(), m.pair_score.tolist(), m.t_lo.tolist(), m.t_hi.tolist())]


def chain_lines(sd, m, k):
    """The C / A / T lines of the chains m (chain_off, score, anchor_place, anchor_seed) over the seeds sd of k patterns:
    pattern by pattern, forward and then reverse."""
    want, strand, best = [], *strands_of(m, k)
    for R in range(k):
        for v in (R, R + k):
            a, e = int(m.chain_off[v]), int(m.chain_off[v + 1])
            want.append(b"C\t%d\t%d" % (m.score[v], e - a))
            want += [b"A\t%d\t%d\t%d\t%d" % (sd.q_start[t], sd.length[t], sd.occ.start_row[g], sd.occ.start_col[g])
                     for g, t in zip(m.anchor_place[a:e].tolist(), m.anchor_seed[a:e].tolist())]
        want.append(b"T\t%s\t%d" % ({0: b"+", 1: b"-", 0xff: b"*"}[int(strand[R])], best[R]))
    return want


@pytest.mark.gpu
def test_tool_prints_the_pairs_and_the_adopted_chains(engine, tmp_path):
    from oracle import pyoracle as O
    A = read_fasta(TC.GOLDEN[0])[0]
    b = [int(x) for x in engine.minmax_dp(engine.elastic_f(A))]
    reads = [r for r in golden_pairs(np.random.default_rng(9), A)]
    keep = [p for p in range(len(reads) // 2) if reads[2 * p] and reads[2 * p + 1]]      # the tool reads tokens: no empty pattern
    reads = [reads[2 * p + j] for p in keep for j in (0, 1)]
    k = len(reads)
    graph = str(tmp_path / "g.xgfa")
    O.write_xgfa(A, b, graph)
    data = b"".join(r + b"\n" for r in reads)
    args = ["--graph=" + graph, "--msa=" + TC.GOLDEN[0], "--seeds", "--occurrences", "--chain", "--strands"]
    base = TC.TL.run_locate(args, data)
    got = TC.TL.run_locate(args + ["--pairs=3,15"], data)
    assert base.returncode == 0 and got.returncode == 0, (base.stderr, got.stderr)
    with TR.build(engine, A, b) as pix:
        sd = pix.seeds(reads, min_length=1, max_per_seed=64, msa=True, strands=True)
        ch0 = pix.chains()
        plain = pix.chains(pairs=(3, 15))
        m = model_of(sd, ch0, None, (3, 15))
        same(plain, m, "tool")
    assert (m.which != PM.NO_PAIR).any() and (m.which == PM.NO_PAIR).any() and not np.array_equal(m.chain_off, ch0.chain_off)
    lines = got.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith(b"Z\t")] == z_lines(m)
    assert all(lines[i - 1].startswith(b"T\t") for i, ln in enumerate(lines) if ln.startswith(b"Z\t"))
    # the C / A / T lines: those of the adopted chains, pattern by pattern, forward and then reverse
    assert [ln for ln in lines if ln[:2] in (b"C\t", b"A\t", b"T\t")] == chain_lines(sd, m, k)
    # every other line is that of the run without --pairs, which is the parent's output byte for byte
    other = lambda out: [ln for ln in out.splitlines() if ln[:2] not in (b"C\t", b"A\t", b"T\t", b"Z\t")]      # noqa: E731
    assert other(got.stdout) == other(base.stdout)
    assert [ln for ln in base.stdout.splitlines() if ln[:2] in (b"C\t", b"A\t", b"T\t")] == chain_lines(sd, ch0, k) and b"Z\t" not in base.stdout
