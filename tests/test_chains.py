"""Co-linear chaining of a read's seeds: fbg_pindex_chains / fbg_pindex_chains_fetch / fbg_pindex_chain_stats,
PatternIndex.chains() / .seeds(chain=True) / .chain_stats() and fbg_locate --chain (include/fbg_hip.h, csrc/pindex_chain.hip).

The checker is tests/chain_model.py: the dynamic programme of the header, statement by statement, applied to what
PatternIndex.seeds(msa=True) returns (pinned by test_seeds and test_msa_coords).  Every GPU comparison is exact, on
chain_off, score, anchor_place and anchor_seed."""
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
import test_locate as TL  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta  # noqa: E402

SPEC = TL.SPEC
LOCATE = TL.LOCATE
GOLDEN = [os.path.join(HERE, "golden", f) for f in ("msa.fasta", "test.fasta", "test2.fasta", "test3.fasta")]
CALLS = ("fbg_pindex_chains", "fbg_pindex_chains_fetch", "fbg_pindex_chain_stats")
GAP = ord("-")
NONE = CM.NONE
FIELDS = ("chain_off", "score", "anchor_place", "anchor_seed")


def build(engine, msa, boundaries):
    engine.msa_load_host(np.ascontiguousarray(msa, dtype=np.uint8))
    return engine.pattern_index_of_segmentation(boundaries)


def model_inputs(sd):
    return sd.seed_off, sd.q_start, sd.length, sd.occ.start_off, sd.occ.start_col


def same(ch, want, what):
    for f, w in zip(FIELDS, want):
        g = getattr(ch, f)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, f)


def per_read(ch):
    """[(score, places, seeds)] per read: what must not depend on the batch a read is in."""
    return [(int(ch.score[r]),) + tuple(ch.of(r).T.tolist()) for r in range(len(ch.score))]


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_chain_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    assert "seeds are not chained" not in header


def random_anchors(rng):
    """Up to 10 anchors of one read in g order, [(g, t, q, k, c)]: seeds in read order without overlap, a few places
    each (some seeds none), columns from a range small enough for equal scores and for both signs of the surplus."""
    out, q, g = [], 0, int(rng.integers(0, 50))
    for t in range(int(rng.integers(1, 6))):
        q += int(rng.integers(0, 3))
        k = int(rng.integers(1, 5))
        for _ in range(int(rng.integers(0, 4))):
            if len(out) < 10:
                out.append((g, 7 + t, q, k, int(rng.integers(0, 16))))
            g += int(rng.integers(1, 3))          # places that are no anchor leave holes in g
        q += k
    return out


def test_model_agrees_with_brute_force():
    rng = np.random.default_rng(11)
    ties = longest = holes = 0
    at_band = {(sign, over): 0 for sign in (1, -1) for over in (0, 1)}      # pairs with surplus sign * (band + over)
    for trial in range(400):
        an = random_anchors(rng)
        # the same read as the arrays of a Seeds object: the holes in g are places without a column
        if an:
            g0, t0 = an[0][0], an[0][1]
            col = np.full(an[-1][0] - g0 + 2, NONE, dtype=np.uint32)
            q, k = np.zeros(an[-1][1] - t0 + 1, dtype=np.uint32), np.ones(an[-1][1] - t0 + 1, dtype=np.uint32)
            start_off = np.zeros(len(q) + 1, dtype=np.uint64)
            for g, t, qq, kk, c in an:
                col[g - g0], q[t - t0], k[t - t0] = c, qq, kk
                start_off[t - t0 + 1:] = g - g0 + 1
            start_off[-1] = len(col)
            seed_off = np.array([0, len(q)], dtype=np.uint64)
            assert CM.read_anchors(seed_off, q, k, start_off, col, 0) == [(g - g0, t - t0, qq, kk, c) for g, t, qq, kk, c in an]
            holes += bool((col[:-1] == NONE).any())
        for band in (0, 1, 3, None):
            top, at = CM.brute_force(an, band)
            score, idx = CM.chain_of(an, band)
            assert score == top, (trial, band)
            if an:
                _, score2, place, _ = CM.chains(seed_off, q, k, start_off, col, band, 0)
                assert score2.tolist() == [top] and place.tolist() == [an[j][0] - g0 for j in idx], (trial, band)
            for i, a in enumerate(an if band is not None else []):
                for b in an[i + 1:]:
                    if a[1] < b[1] and b[4] >= a[4] + a[3]:
                        sur = (b[4] - a[4]) - (b[2] - a[2])
                        for sign, over in at_band:
                            at_band[(sign, over)] += sur == sign * (band + over)
            if an:
                assert sum(an[j][3] for j in idx) == score
                # among the best chains: the smallest end, then the smallest predecessor of it, and so on
                assert tuple(idx) == min(at, key=lambda sub: sub[::-1]), (trial, band)
                ties += len(at) > 1
                longest = max(longest, len(idx))
            else:
                assert (score, idx, at) == (0, [], [])
    assert ties > 50 and longest >= 4
    # both signs of the surplus at the band and one beyond it, and places without a column between anchors
    assert holes > 50 and all(v > 20 for v in at_band.values()), (holes, at_band)
    # chains(): CSR assembly, min_score, a read without anchors, a place that is none
    seed_off = np.array([0, 2, 2, 3], dtype=np.uint64)
    q, k = np.array([0, 5, 1], dtype=np.uint32), np.array([4, 3, 2], dtype=np.uint32)
    start_off = np.array([0, 2, 3, 4], dtype=np.uint64)
    col = np.array([NONE, 10, 15, 3], dtype=np.uint32)
    off, score, place, seed = CM.chains(seed_off, q, k, start_off, col, None, 0)
    assert (off.tolist(), score.tolist(), place.tolist(), seed.tolist()) == ([0, 2, 2, 3], [7, 0, 2], [1, 2, 3], [0, 1, 2])
    off, score, place, seed = CM.chains(seed_off, q, k, start_off, col, 0, 3)       # 15 - 10 = 5 - 0: still a chain
    assert (off.tolist(), score.tolist(), place.tolist(), seed.tolist()) == ([0, 2, 2, 2], [7, 0, 2], [1, 2], [0, 1])
    col[2] = 16
    off, score, place, seed = CM.chains(seed_off, q, k, start_off, col, 0, 0)
    assert (off.tolist(), score.tolist(), place.tolist()) == ([0, 1, 1, 2], [4, 0, 2], [1, 3])


def test_tool_chain_needs_its_prerequisites():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--chain[=BAND]" in p.stderr
    full = ["--seeds=3", "--occurrences=4", "--msa=" + GOLDEN[0]]
    for drop in range(3):
        args = ["--graph=" + SPEC] + full[:drop] + full[drop + 1:] + ["--chain=2"]
        p = subprocess.run([LOCATE] + args, input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--chain needs" in p.stderr and b"usage:" in p.stderr, args
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--seeds", "--occurrences=0", "--msa=" + GOLDEN[0], "--chain"], input=b"AG\n",
                       capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--chain needs" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + SPEC] + full + ["--chain=x"], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--chain takes a band" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

def chain_reads(rng, A):
    """Gap-stripped rows whole and in pieces with 0 .. 3 substitutions, and reads spliced from two rows."""
    rows = [r[r != GAP].tobytes() for r in A]
    rows = [r for r in rows if len(r) >= 4]
    out = list(rows)
    for j in range(4 * len(rows)):
        r = rows[j % len(rows)]
        ln = int(rng.integers(max(4, len(r) // 2), len(r) + 1))
        a = int(rng.integers(0, len(r) - ln + 1))
        s = bytearray(r[a:a + ln])
        for _ in range(j % 4):
            at = int(rng.integers(0, ln))
            s[at] = rng.choice([c for c in b"ACGT" if c != s[at]])
        out.append(bytes(s))
    for j in range(2 * len(rows)):
        r, o = rows[j % len(rows)], rows[(j + 1 + j // len(rows)) % len(rows)]
        cut, skip = int(rng.integers(2, len(r) - 1)), int(rng.integers(0, 4))
        out.append(r[:cut] + o[min(cut + skip, len(o) - 2):])
    return out


def chain_inputs(engine=None):
    """(name, MSA, boundaries of the min-max-length DP) of the four golden files and one random MSA with gaps."""
    out = []
    rng = np.random.default_rng(31)
    for path in GOLDEN + [None]:
        A = read_fasta(path)[0] if path else random_msa(rng, 6, 60, gap_p=0.04, gap_run=3, similar=0.9)
        if engine is None:
            from oracle import pyoracle as O
            b = O.minmax_dp(O.compute_f(A))[2]
        else:
            b = engine.minmax_dp(engine.elastic_f(A))
        out.append((os.path.basename(path) if path else "random", A, [int(x) for x in b]))
    return out


@pytest.mark.gpu
def test_golden_and_random_inputs(engine):
    seen = dict(long=0, not_first=0, band=0, below=0, nonempty=0)
    for name, A, b in chain_inputs(engine):
        assert len(b) >= 2, name
        reads = chain_reads(np.random.default_rng(len(A[0])), A)
        with build(engine, A, b) as pix:
            for L in (1, 3):
                for cap in (1, 4, 64):
                    sd = pix.seeds(reads, min_length=L, max_per_seed=cap, msa=True)
                    inp = model_inputs(sd)
                    solved = {band: CM.solve(*inp, band) for band in (0, 2, None)}
                    scores = [sc for _, sc, _ in solved[None]]
                    mid = (min(scores) + max(scores) + 1) // 2
                    assert min(scores) < mid <= max(scores), (name, L, cap)
                    for band in (0, 2, None):
                        for min_score in (0, mid):
                            want = CM.assemble(solved[band], min_score)
                            same(pix.chains(band=band, min_score=min_score), want, (name, L, cap, band, min_score))
                            seen["below"] += int((want[1] < min_score).sum())
                    first = sd.occ.start_off[:-1]
                    for (an, _, idx), (_, _, idx0) in zip(solved[None], solved[0]):
                        seen["long"] += len(idx) >= 3
                        seen["nonempty"] += len(idx) > 0
                        seen["not_first"] += any(an[j][0] != int(first[an[j][1]]) for j in idx)
                        seen["band"] += idx != idx0
            # through seeds(chain=True): the same object
            sd = pix.seeds(reads, min_length=1, max_per_seed=4, msa=True, chain=True, band=2, min_score=3)
            same(sd.chains, CM.chains(*model_inputs(sd), 2, 3), name)
            assert sd.chains.device_ms > 0 and pix.seeds(reads).chains is None
    assert all(v > 0 for v in seen.values()), seen


UNIT = b"ACGGCAGACCGA"


def tier_msa():
    """3 rows of 83 copies of one 12-symbol unit: row 1 with a few gaps, row 2 with a few substitutions; boundaries at
    irregular steps, so that labels and edges start at every phase of the unit."""
    row = np.frombuffer(UNIT * 83, dtype=np.uint8)
    A = np.stack([row, row, row]).copy()
    A[1, [100, 101, 350, 777]] = GAP
    A[2, [60, 410, 800]] = ord("A")
    b, x = [], 30
    while x < len(row) - 40:
        b.append(x)
        x += 31 + (len(b) * 7) % 19
    return A, b + [len(row)]


def tier_read(rng, seeds):
    """`seeds` rotations of the unit, each followed by a symbol the MSA does not hold: one seed per rotation."""
    return b"".join(UNIT[r:] + UNIT[:r] + b"T" for r in rng.integers(0, len(UNIT), seeds).tolist())


@pytest.mark.gpu
def test_tiers_agree_alone_and_mixed(engine):
    A, b = tier_msa()
    rng = np.random.default_rng(5)
    with build(engine, A, b) as pix:
        assert pix.msa_stats()["gapped_nodes"] > 0
        st = pix.chain_stats()
        sm, lm = st["small_max"], st["lds_max"]
        assert 1 <= sm < lm and (st["anchors"], st["reads_small"], st["reads_wave"], st["reads_spill"]) == (0, 0, 0, 0)
        # places per read = seeds * cap, as long as every rotation of the unit has `cap` start places
        plans = {1: [1, 2, sm, sm + 1, lm, lm + 1], 16: [1, sm // 16, sm // 16 + 1, lm // 16, lm // 16 + 1],
                 64: [1, lm // 64, lm // 64 + 1]}
        hit = set()
        for cap, counts in plans.items():
            reads = [tier_read(rng, s) for s in counts] + [b"", b"TT"]
            sd = pix.seeds(reads, min_length=12, max_per_seed=cap, msa=True)
            assert np.diff(sd.seed_off.astype(np.int64)).tolist() == counts + [0, 0]
            assert (np.diff(sd.occ.start_off.astype(np.int64)) == cap).all(), cap
            places = [s * cap for s in counts]
            hit |= set(places)
            tier = [0 if p <= sm else 1 if p <= lm else 2 for p in places]
            for band in (None, 6):
                want = CM.chains(*model_inputs(sd), band, 0)
                mixed = pix.chains(band=band)
                same(mixed, want, (cap, band, "mixed"))
                st = pix.chain_stats()
                assert [st["reads_small"], st["reads_wave"], st["reads_spill"]] == [tier.count(k) for k in range(3)], cap
                assert st["anchors"] == int((sd.occ.start_col != NONE).sum()) == sum(places)
                if cap > 1 and band is None:
                    assert max(len(mixed.of(r)) for r in range(len(counts))) >= 3
                together = per_read(mixed)
                if band is None:
                    continue
                for r, read in enumerate(reads[:len(counts)]):
                    one = pix.seeds([read], min_length=12, max_per_seed=cap, msa=True, chain=True, band=band)
                    base = int(sd.occ.start_off[int(sd.seed_off[r])]), int(sd.seed_off[r])
                    sc, pl, se = per_read(one.chains)[0]
                    assert (sc, [x + base[0] for x in pl], [x + base[1] for x in se]) == together[r], (cap, r)
                    st = pix.chain_stats()
                    assert [st["reads_small"], st["reads_wave"], st["reads_spill"]] == [int(tier[r] == k) for k in range(3)]
        assert {sm, sm + 1, lm, lm + 1} <= hit
        assert all(any((0 if s * cap <= sm else 1 if s * cap <= lm else 2) == k for s in plans[cap]) for cap in (16, 64)
                   for k in ((0, 1, 2) if cap == 16 else (1, 2)))


@pytest.mark.gpu
def test_degenerate_cases(engine):
    A, _ = read_fasta(GOLDEN[0])
    b = engine.minmax_dp(engine.elastic_f(A))
    with build(engine, A, b) as pix:
        sd = pix.seeds([], msa=True, chain=True)                                   # n == 0
        assert sd.chains.chain_off.tolist() == [0] and len(sd.chains.score) == 0 and len(sd.chains.anchor_place) == 0
        sd = pix.seeds([b"", b"", b""], max_per_seed=4, msa=True, chain=True)       # empty reads
        assert sd.chains.chain_off.tolist() == [0, 0, 0, 0] and sd.chains.score.tolist() == [0, 0, 0]
        sd = pix.seeds([b"XX", b"", b"X"], max_per_seed=4, msa=True, chain=True)    # reads without a seed
        assert len(sd) == 0 and sd.chains.chain_off.tolist() == [0, 0, 0, 0] and sd.chains.score.tolist() == [0, 0, 0]
        reads = [b"AGCGACTAGATAC", b"XX", b"AGCXACTAGTT", b""]
        sd = pix.seeds(reads, max_per_seed=0, msa=True, chain=True)                 # seeds without places
        assert len(sd) > 0 and sd.chains.chain_off.tolist() == [0] * 5 and sd.chains.score.tolist() == [0] * 4
        assert pix.chain_stats()["anchors"] == 0
        sd = pix.seeds(reads, max_per_seed=4, msa=True, chain=True)                 # seeded and unseeded reads side by side
        same(sd.chains, CM.chains(*model_inputs(sd), None, 0), "mixed")
        assert sd.chains.score.tolist()[1::2] == [0, 0] and min(sd.chains.score.tolist()[0::2]) > 0
        top = int(sd.chains.score.max())
        ch = pix.chains(min_score=top + 1)                                          # min_score above every score
        assert ch.chain_off.tolist() == [0] * 5 and np.array_equal(ch.score, sd.chains.score) and len(ch.anchor_seed) == 0
        ch = pix.chains(min_score=top)
        assert len(ch.anchor_place) > 0 and set(np.diff(ch.chain_off.astype(np.int64))[sd.chains.score < top]) <= {0}
        # a pattern holding '#': places outside their edge have no column and are no anchor
        from test_msa_coords import MM
        model = MM.Model(A, b)
        S = [model.labels[u] + model.labels[v] for u, v in model.edges]
        pats = [S[e + 1][-2:] + b"#" + S[e][:2] for e in range(len(S) - 1)] + [b"AG#", b"AGCGA"]
        sd = pix.seeds(pats, max_per_seed=64, msa=True, chain=True)
        assert (sd.occ.start_col == NONE).any() and (sd.occ.start_col != NONE).any()
        same(sd.chains, CM.chains(*model_inputs(sd), None, 0), "separator")
        assert (sd.occ.start_col[sd.chains.anchor_place] != NONE).all()
        assert pix.chain_stats()["anchors"] == int((sd.occ.start_col != NONE).sum()) < len(sd.occ.start_col)


def seeds_state(pix, n):
    """What fbg_pindex_seeds_fetch, _places and _msa return right now, through the C calls."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    q, ln, rs = (np.zeros(n + 1, dtype=np.uint32) for _ in range(3))
    cnt, et, st, eo, so = (np.zeros(n + 1, dtype=np.uint64) for _ in range(5))
    assert L.fbg_pindex_seeds_fetch(pix._h, u32(q), u32(ln), u64(cnt), u32(rs), u64(et), u64(st), u64(eo), u64(so), None) == 0
    ne, ns = int(eo[n]), int(so[n])
    six = [np.zeros((ne if k < 3 else ns) + 1, dtype=np.uint32) for k in range(6)]
    four = [np.zeros((ne if k < 2 else ns) + 1, dtype=np.uint32) for k in range(4)]
    assert L.fbg_pindex_seeds_places(pix._h, *[u32(a) for a in six], None) == 0
    assert L.fbg_pindex_seeds_msa(pix._h, *[u32(a) for a in four], None) == 0
    return [a.tolist() for a in [q, ln, rs, cnt, et, st, eo, so] + six + four]


@pytest.mark.gpu
def test_a_chains_call_leaves_every_other_state_alone(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    INVALID = _lib.FBG_ERR_INVALID
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    buf = [np.zeros(1 << 16, dtype=np.uint32) for _ in range(3)]      # room for a chain entry per read symbol
    off = np.zeros(4096, dtype=np.uint64)
    assert L.fbg_pindex_chains(None, 0, 0, u64(off), u32(buf[0]), None) == INVALID
    assert L.fbg_pindex_chains_fetch(None, u32(buf[0]), u32(buf[1]), None) == INVALID
    assert L.fbg_pindex_chain_stats(None, None, None, None, None, None, None) == INVALID
    rng = np.random.default_rng(3)
    A = random_msa(rng, 8, 200, gap_p=0.03, gap_run=3, similar=0.93)
    b = engine.minmax_dp(engine.elastic_f(A))
    reads = chain_reads(rng, A)
    with build(engine, A, b) as pix:
        # before any seeds call; an occurrences search is no seeds result
        assert L.fbg_pindex_chains(pix._h, 0, 0, u64(off), u32(buf[0]), None) == INVALID
        with pytest.raises(F.FbgError) as ei:
            pix.chains()
        assert ei.value.code == INVALID
        occ = pix.occurrences(reads[:20], max_per_pattern=8, msa=True)
        assert L.fbg_pindex_chains(pix._h, 0, 0, u64(off), u32(buf[0]), None) == INVALID
        count, pos = pix.locate(reads)
        stats = pix.stats()
        val = pix.validate(pix.node_block)
        sd = pix.seeds(reads, min_length=2, max_per_seed=8, msa=True)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(buf[0]), u32(buf[1]), None) == INVALID      # seeds, but no chains yet
        assert L.fbg_pindex_chains(pix._h, 0, 0, None, u32(buf[0]), None) == INVALID             # chain_off is required
        before = seeds_state(pix, len(sd))
        ch = pix.chains(band=3, min_score=4)
        same(ch, CM.chains(*model_inputs(sd), 3, 4), "state")
        assert len(ch.anchor_place) > 0
        assert seeds_state(pix, len(sd)) == before
        # the score may be left out, either anchor array too, and the fetch repeats
        assert L.fbg_pindex_chains(pix._h, 3, 4, u64(off), None, None) == 0 and off[:len(reads) + 1].tolist() == ch.chain_off.tolist()
        t = len(ch.anchor_place)
        assert L.fbg_pindex_chains_fetch(pix._h, None, u32(buf[1]), None) == 0 and buf[1][:t].tolist() == ch.anchor_seed.tolist()
        assert L.fbg_pindex_chains_fetch(pix._h, u32(buf[0]), None, None) == 0 and buf[0][:t].tolist() == ch.anchor_place.tolist()
        assert L.fbg_pindex_chains_fetch(pix._h, None, None, None) == 0
        assert seeds_state(pix, len(sd)) == before
        # occurrences, locate's statistics, the validation and a segmentation on the same engine
        ends = [np.zeros(len(occ.end_src) + 1, dtype=np.uint32) for _ in range(3)]
        starts = [np.zeros(len(occ.start_src) + 1, dtype=np.uint32) for _ in range(3)]
        assert L.fbg_pindex_occurrences_fetch(pix._h, *[u32(a) for a in ends + starts], None) == 0
        for a, f in zip(ends + starts, ("end_src", "end_dst", "end_offset", "start_src", "start_dst", "start_offset")):
            assert np.array_equal(a[:-1], getattr(occ, f)), f
        assert pix.stats() == stats
        c2, p2 = pix.locate(reads)
        assert np.array_equal(c2, count) and np.array_equal(p2, pos)
        v2 = pix.validate(pix.node_block)
        assert np.array_equal(v2.status, val.status)
        # a newer seeds call invalidates the chains
        pix.seeds(reads[:5], min_length=2, max_per_seed=8)
        assert L.fbg_pindex_chains_fetch(pix._h, u32(buf[0]), u32(buf[1]), None) == INVALID
        assert pix.chains().chain_off.shape == (6,)
        # the engine's segmentation is what it was
        assert np.array_equal(engine.minmax_dp(engine.elastic_f(A)), b)
    # an index built on the host knows no MSA
    labels, edges = F.read_xgfa(SPEC)
    with engine.pattern_index(labels, edges) as pix:
        pix.seeds(["AGCGA"], max_per_seed=4)
        assert L.fbg_pindex_chains(pix._h, 0, 0, u64(off), u32(buf[0]), None) == INVALID
        with pytest.raises(F.FbgError) as ei:
            pix.chains()
        assert ei.value.code == INVALID
        assert pix.chain_stats()["small_max"] > 0


@pytest.mark.gpu
def test_tool_prints_the_chains(engine):
    """The example graph of xGFAspec.md is a segmentation of golden/msa.fasta (its M and X lines say which)."""
    A, _ = read_fasta(GOLDEN[0])
    data = b"AGCGACTAGATAC AGCAGTT CGACTAX T XX GACTAGTTTCA AGXTTAC AGCGTCTCGTTAC\n"
    reads = data.split()
    args = ["--graph=" + SPEC, "--seeds=3", "--occurrences=4", "--msa=" + GOLDEN[0]]
    with build(engine, A, [1, 5, 8, 14]) as pix:
        sd = pix.seeds(reads, min_length=3, max_per_seed=4, msa=True, chain=True, band=2)
    ch, o = sd.chains, sd.occ
    assert len(ch.anchor_place) >= 3
    ids = list(range(1, 10))                                      # the S ids of the file, ascending
    plain, chained, seeded = [], [], 0
    for r in range(len(reads)):
        a, b = int(sd.seed_off[r]), int(sd.seed_off[r + 1])
        lines = [b"Pattern? %d seeds found.\n" % (b - a)]
        seeded += b > a
        for j in range(a, b):
            lines.append(b"S\t%d\t%d\t%d\t%d\n" % (sd.q_start[j], sd.length[j], o.count[j], o.restarts[j]))
            for tag, w, total in ((b"E", "end", o.end_total), (b"B", "start", o.start_total)):
                off = getattr(o, w + "_off")
                for i in range(int(off[j]), int(off[j + 1])):
                    src, dst, at, row, col = (int(getattr(o, f"{w}_{f}")[i]) for f in ("src", "dst", "offset", "row", "col"))
                    lines.append(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (tag, ids[src], ids[dst], at, row, col))
                if int(total[j]) > int(off[j + 1] - off[j]):
                    lines.append(b"%s\t...\t%d more\n" % (tag, int(total[j]) - int(off[j + 1] - off[j])))
        plain += lines
        chained += lines + [b"C\t%d\t%d\n" % (ch.score[r], len(ch.of(r)))]
        chained += [b"A\t%d\t%d\t%d\t%d\n" % (sd.q_start[t], sd.length[t], o.start_row[g], o.start_col[g]) for g, t in ch.of(r)]
    last = [b"Pattern? %d out of %d patterns seeded\n" % (seeded, len(reads))]
    p = TL.run_locate(args + ["--chain=2"], data)
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"".join(chained + last)
    # without --chain: the output of the unchanged options, and that is the chained output less its C and A lines
    q = TL.run_locate(args, data)
    assert q.returncode == 0 and q.stdout == b"".join(plain + last)
    assert q.stdout == b"".join(ln for ln in p.stdout.splitlines(keepends=True) if ln[:2] not in (b"C\t", b"A\t"))
    # --chain alone is unbounded
    sd_none = None
    with build(engine, A, [1, 5, 8, 14]) as pix:
        sd_none = pix.seeds(reads, min_length=3, max_per_seed=4, msa=True, chain=True)
    p = TL.run_locate(args + ["--chain"], data)
    got = [ln for ln in p.stdout.splitlines() if ln[:2] == b"C\t"]
    assert p.returncode == 0 and got == [b"C\t%d\t%d" % (sd_none.chains.score[r], len(sd_none.chains.of(r))) for r in range(len(reads))]
