"""MSAs over other alphabets than DNA, and texts above 2^24 symbols, bit for bit against the oracle.

Every kernel on the index path packs suffixes into 64-bit key words of K symbols of b bits (suffix_sort.hip
fbg_key_setup), and many branches depend on b, on the coding (compact: no byte below '#', fewer than 128 symbols) and on
how many symbols are frequent (the rank table of the sample sort of pairs, msd_sort_pairs.hip).  Each alphabet class below
is built to reach one such geometry; key_geometry() mirrors the library's arithmetic, the CPU tests pin that every class
reaches its row of the table, and the GPU tests check that the library set up the same keys before comparing results.
The CPU part also pins the oracle itself on these alphabets (its fast scans against its literal ones)."""
import ctypes as C

import numpy as np
import pytest

from conftest import fbg_options
from oracle import pyoracle as O

GAP = ord("-")

# natural amino-acid frequencies (percent, UniProtKB), and two rare codes: X (unknown) and * (stop)
_AA = "ARNDCQEGHILKMFPSTWYV"
_AA_W = [8.25, 5.53, 4.06, 5.45, 1.37, 3.93, 6.75, 7.07, 2.27, 5.96, 9.66, 5.84, 2.42, 3.86, 4.70, 6.56, 5.34, 1.08, 2.92, 6.87]


def _bytes(lo, hi):
    return bytes(range(lo, hi + 1))


_B8 = bytes(c for c in range(1, 256) if c not in (ord("#"), GAP))[:200]

# id -> symbols, weights, generator extras, the ignore character that the class tests, and the geometry it must reach:
# b / compact of the keys of a gap-free MSA, b_pairs / rb of the (key, position) pairs of the record path
CLASSES = {
    # b = 2 with an unused code: the MSD sort's symbols after the key with 3 codes
    "acg": dict(symbols=b"ACG", compact=True, b=2, b_pairs=3, rb=2),
    # 8 frequent symbols: the sample sort's rank table with rb = 3, ew = 4 (16 codes x 4 bits: exactly 64 bits)
    "softmask": dict(symbols=b"ACGT", softmask=0.3, compact=True, b=3, b_pairs=4, rb=3),
    # 4 frequent, 10 rare codes: modes 1 (joins the frequent code above it) and 2 (above T: joins the last one).  V is left
    # out so that the pairs' codes (with '#' and the sentinel) stay at 16: b = 4
    "iupac": dict(symbols=b"ACGTNRYKMSWBDH", weights=[24.25] * 4 + [0.3] * 10, ignore="N", compact=True, b=4, b_pairs=4, rb=2),
    # 20 amino acids at natural skew (18 frequent: no rank table), rare X and *
    "protein": dict(symbols=(_AA + "X*").encode(), weights=_AA_W + [0.1, 0.05], ignore="X", compact=True, b=5, b_pairs=5, rb=0),
    # 4 frequent amino acids, 16 rare: b = 5 with rb = 2, the rank table exactly 64 bits (32 codes x 2 bits)
    "protein4": dict(symbols=b"ALGVRNDCQEHIKMFPSTWY", weights=[22.0] * 4 + [0.75] * 16, compact=True, b=5, b_pairs=5, rb=2),
    # 40 / 100 distinct bytes, some of them 0x80 and above: the shortest keys of the compact coding
    "b6": dict(symbols=_bytes(0x41, 0x5A) + _bytes(0x80, 0x8D), compact=True, b=6, b_pairs=6, rb=0),
    "b7": dict(symbols=_bytes(0x41, 0x7E) + _bytes(0x80, 0xA5), compact=True, b=7, b_pairs=7, rb=0),
    # a byte below '#': no compact coding, (key, position) pairs into the scans of gap-free MSAs
    "bang": dict(symbols=b"ACGT!", weights=[23.0] * 4 + [8.0], compact=False, b=3, b_pairs=3, rb=3),
    # 200 distinct bytes (some below '#'): no compact coding, 8-bit symbols
    "b8": dict(symbols=_B8, compact=False, b=8, b_pairs=8, rb=0),
}


def _runs(rng, m, n, p_cell, run):
    """(m, n) mask of runs of `run` cells that cover about p_cell of the cells."""
    starts = rng.random((m, n)) < p_cell / run
    c = np.cumsum(starts, axis=1, dtype=np.int32)
    before = np.zeros_like(c)
    before[:, run:] = c[:, :-run]
    return (c - before) > 0


def weighted_msa(rng, m, n, symbols, weights=None, similar=0.0, gap_cells=0.0, gap_run=1, softmask=0.0, mask_run=40):
    """Seeded (m, n) uint8 MSA over `symbols` drawn with `weights`.  similar > 0: a star phylogeny (every row a copy of one
    ancestor, each cell redrawn with probability 1 - similar); softmask: that fraction of the cells lies in runs of
    `mask_run` lowercase cells; gap_cells: that fraction in gap runs of `gap_run`."""
    sym = np.frombuffer(bytes(symbols), dtype=np.uint8)
    p = None if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)

    def draw(size):
        return sym[rng.choice(len(sym), size=size, p=p)]

    if similar > 0:
        a = np.tile(draw(n), (m, 1))
        mut = rng.random((m, n)) >= similar
        a[mut] = draw(int(mut.sum()))
    else:
        a = draw((m, n))
    if softmask > 0:
        low = _runs(rng, m, n, softmask, mask_run) & (a >= ord("A")) & (a <= ord("Z"))
        a[low] |= 0x20
    if gap_cells > 0:
        a[_runs(rng, m, n, gap_cells, gap_run)] = GAP
    return a


def class_msa(rng, cls, m, n, **kw):
    c = CLASSES[cls]
    return weighted_msa(rng, m, n, c["symbols"], c.get("weights"), softmask=c.get("softmask", 0.0), **kw)


def key_geometry(msa):
    """What fbg_key_setup and fbg_sample_sort_pairs make of this MSA: the compact coding (gap-free MSAs, rank-order
    scans) and its b; b_pairs of the coding of any alphabet; the sample sort's rb (0: no rank table)."""
    m, n = msa.shape
    hist = np.bincount(msa.ravel(), minlength=256).astype(np.int64)
    hist[GAP] = 0
    hist[ord("#")] += m
    hist[0] += 1
    N = int(hist.sum())
    real = [c for c in range(1, 256) if hist[c] and c != ord("#")]
    compact = 1 <= len(real) < 128 and min(real) > ord("#")

    def bits(s):
        b = 1
        while (1 << b) < s:
            b += 1
        return b

    b_pairs = bits(int((hist > 0).sum()))
    nf = int((hist >= N // 64).sum())
    rb = 1 if nf <= 2 else 2 if nf <= 4 else 3 if nf <= 8 else 0
    ew = 2 if rb <= 2 else 4
    if b_pairs > 5 or (1 << b_pairs) * ew > 64:
        rb = 0
    return dict(N=N, compact=compact, b=bits(len(real)) if compact else b_pairs, b_pairs=b_pairs, rb=rb, ew=ew)


# --------------------------------------------------------------------------------------------------------------------
# CPU part: the generators reach their geometry, and the oracle's fast scans agree with its literal ones
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_class_reaches_its_geometry(cls):
    c = CLASSES[cls]
    rng = np.random.default_rng(7)
    for kw in (dict(), dict(similar=0.99)):
        msa = class_msa(rng, cls, 40, 2500, **kw)
        g = key_geometry(msa)
        assert (g["compact"], g["b"], g["b_pairs"], g["rb"]) == (c["compact"], c["b"], c["b_pairs"], c["rb"]), (kw, g)
    # with gaps: the same symbols, so the same pairs geometry
    g = key_geometry(class_msa(rng, cls, 40, 2500, gap_cells=0.05, gap_run=6))
    assert (g["b_pairs"], g["rb"]) == (c["b_pairs"], c["rb"]), g
    if cls in ("protein4", "softmask"):
        assert (1 << g["b_pairs"]) * g["ew"] == 64                    # the rank table at exactly 64 bits
    if cls in ("b6", "b7"):
        assert any(s >= 0x80 for s in c["symbols"])
    if cls == "b8":
        assert len(set(c["symbols"])) == 200 and min(c["symbols"]) < ord("#")


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_oracle_fast_scans_equal_literal_scans(cls):
    """The GPU tests trust oracle/fbg_oracle.c: its compute_f / segment_v / gapped_v equal its literal forms (the
    reference's statements one by one) on every alphabet class, with and without gaps and ignore characters."""
    rng = np.random.default_rng(sum(map(ord, cls)))
    ign = CLASSES[cls].get("ignore", "")
    for shape in range(20):
        m = int(rng.integers(1, 30))
        n = int(rng.integers(1, 120))
        kw = dict(similar=0.9) if shape % 2 else {}
        gapped = shape % 4 >= 2
        if gapped:
            kw.update(gap_cells=0.1, gap_run=int(rng.integers(1, 6)))
        msa = class_msa(rng, cls, m, n, **kw)
        for ignore in ("", ign) if ign else ("",):
            for tricks_off in (False, True):
                f = O.compute_f(msa, ignore=ignore, disable_tricks=tricks_off)
                assert np.array_equal(f, O.compute_f(msa, ignore=ignore, disable_tricks=tricks_off, literal=True)), (shape, ignore)
        if gapped:
            assert np.array_equal(O.gapped_v(msa), O.gapped_v(msa, literal=True)), shape
        else:
            assert np.array_equal(O.segment_v(msa), O.segment_v(msa, literal=True)), shape


# --------------------------------------------------------------------------------------------------------------------
# GPU: small and medium cases under every switch that picks a path
# --------------------------------------------------------------------------------------------------------------------

SWITCHES = [
    {},
    {"msd_min": 1},
    {"msd_min": 1, "msd_sample_bins": 1},
    {"no_packed": 1},
    {"force_wide": 1},
    {"no_ranked": 1},
    {"pure_scan": 1},
    {"gapped_rank": -1},
    {"span_scan": 1},
    {"span_scan": 3},
    {"rank_no_lean": 1},
]

# (m, n, generator extras): iid and similar rows, gap-free and with gap runs
SHAPES = {
    "iid": (40, 2500, dict()),
    "similar": (64, 1500, dict(similar=0.99)),
    "iid_gaps": (30, 3000, dict(gap_cells=0.03, gap_run=5)),
    "similar_gaps": (100, 2000, dict(similar=0.99, gap_cells=0.02, gap_run=8)),
}


def _check_keys(engine, g):
    """The keys of the last build have the geometry key_geometry() predicts for their coding."""
    b, K = engine.get_option("key_b"), engine.get_option("key_K")
    compact, packed = engine.get_option("key_compact"), engine.get_option("key_packed")
    assert compact in (0, 1) and packed in (0, 1)
    assert not compact or g["compact"]
    assert b == (g["b"] if compact else g["b_pairs"]), (b, compact, g)
    assert 1 <= K <= 64 // b
    assert not packed or compact
    return compact, packed


def _index_matches(engine, msa, ref):
    T, SA, ISA, LCP = ref
    gT, gSA, gISA, gPL, gPR = engine.index_download()
    assert np.array_equal(gT, T)
    assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
    assert np.array_equal(gISA.astype(np.int64), ISA.astype(np.int64))
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
    assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_alphabet_index_and_scans_match_oracle(engine, cls, shape):
    """Index arrays, f (elastic tricks on and off), v, and f with the class's ignore character, under every path switch;
    each path that is expected to run is asserted, each documented decline is named."""
    m, n, kw = SHAPES[shape]
    rng = np.random.default_rng(1000 * sorted(CLASSES).index(cls) + sorted(SHAPES).index(shape))
    msa = class_msa(rng, cls, m, n, **kw)
    g = key_geometry(msa)
    assert g["compact"] == CLASSES[cls]["compact"] and g["b_pairs"] == CLASSES[cls]["b_pairs"]
    gapped = bool((msa == GAP).any())
    ign = CLASSES[cls].get("ignore", "")
    ref_index = O.msa_index(msa)
    f_on, f_off = O.compute_f(msa), O.compute_f(msa, disable_tricks=True)
    v = O.gapped_v(msa) if gapped else O.segment_v(msa)
    f_ign = (O.compute_f(msa, ignore=ign), O.compute_f(msa, ignore=ign, disable_tricks=True)) if ign else None
    for sw in SWITCHES:
        with fbg_options(engine, sw):
            what = (cls, shape, sw)
            engine.msa_load_host(msa)
            engine.index_build()
            kind = engine.get_option("index_kind")
            compact, packed = _check_keys(engine, g)
            if engine.get_option("span_scan_used") == 0:         # (the group-level scan leaves equal keys unordered: no SA)
                _index_matches(engine, msa, ref_index)
            if not gapped:
                if sw.get("no_ranked") or not g["compact"]:
                    # keys in the coding of any alphabet are for the record path only
                    assert kind == 0 and compact == 0, (what, kind)
                    assert engine.get_option("msd_decline") == -1, what
                elif sw.get("force_wide") and shape == "similar":
                    assert kind == 0, what                   # the group-level scan has no wide slot layout (pure_scan.hip)
                else:
                    # compact keys: the rank-order or the group-level scan takes every gap-free MSA
                    assert kind == 1 and compact == 1, (what, kind)
                if sw.get("msd_min") and kind == 1 and packed and shape == "iid":
                    assert engine.get_option("msd_decline") == 0, what
                if kind == 1:
                    assert engine.get_option("pairs_rb") == -1, what
                if sw.get("rank_no_lean"):
                    assert engine.get_option("rank_lean_used") == 0, what
                if sw.get("no_packed") or sw.get("force_wide"):
                    assert packed == 0, what
            else:
                if sw.get("gapped_rank") == -1:
                    assert kind == 0, what
                if sw.get("span_scan") in (1, 3) and shape == "similar_gaps":
                    assert engine.get_option("span_scan_used") == 1, (what, engine.get_option("span_decline"))
                assert compact == 0, what
            if sw.get("msd_min") and shape in ("iid", "iid_gaps") and kind != 1:
                # the record path's sort: the sample sort of pairs with the rank table of its row (msd_sample_bins: none).
                # b8's keys of 3 symbols of 8 bits: the sample sort declines them to rocPRIM (pairs_rb = -1), a fallback
                # whose reason is not pinned down yet -- the results above and below are checked either way
                want = -1 if cls == "b8" else 0 if sw.get("msd_sample_bins") else g["rb"]
                assert engine.get_option("pairs_rb") == want, (what, g)
            got_on = engine.elastic_f(msa)
            assert np.array_equal(got_on, f_on), (what, np.flatnonzero(got_on != f_on)[:8])
            assert np.array_equal(engine.elastic_f(msa, disable_efg_tricks=True), f_off), what
            got_v = engine.gapped_v(msa) if gapped else engine.repeatfree_v(msa)
            assert np.array_equal(got_v, v), (what, np.flatnonzero(got_v != v)[:8])
            if f_ign is not None:
                got = engine.elastic_f(msa, ignorechars=ign)
                assert np.array_equal(got, f_ign[0]), (what, np.flatnonzero(got != f_ign[0])[:8])
                dec = engine.get_option("span_decline")
                assert dec in (0, 10), (what, dec)            # 10: an ignore character the span scan cannot express
                _check_keys(engine, g)
                assert engine.get_option("key_compact") == 0, what
                assert np.array_equal(engine.elastic_f(msa, ignorechars=ign, disable_efg_tricks=True), f_ign[1]), what


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 30), (8, 200), (40, 2500)])
def test_gap_free_keys_without_compact_coding_take_the_record_path(engine, shape):
    """A byte below '#' leaves a gap-free MSA's keys in the coding of any alphabet.  The rank-order and group-level scans
    read keys in the compact coding only; before they declined such keys, the index they left had wrong neighbour LCPs."""
    m, n = shape
    msa = class_msa(np.random.default_rng(m * n), "bang", m, n)
    engine.msa_load_host(msa)
    engine.index_build()
    assert engine.get_option("index_kind") == 0 and engine.get_option("key_compact") == 0
    assert engine.get_option("msd_decline") == -1
    _index_matches(engine, msa, O.msa_index(msa))
    assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("cls", ["protein", "iupac", "bang"])
def test_alphabet_partitioned_index_matches_oracle(cls, P):
    """The key-range partitioned index (multi-GPU path, partitions played by P contexts on one GPU): f with and without
    the elastic tricks, v of the reversed rows, and f of rows with gaps and the class's ignore character."""
    import torch
    from founderblockgraphs_amd import Engine
    from test_gpu_parity import _partitioned
    rng = np.random.default_rng(77 + P + 10 * sorted(CLASSES).index(cls))
    ign = CLASSES[cls].get("ignore", "")
    engines = [Engine() for _ in range(P)]

    def scan_f(n, tricks_off):
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engines[P - 1].scan_f(0, n, d_f.data_ptr(), tricks_off)
        engines[P - 1].sync()
        return d_f.cpu().numpy().astype(np.uint64)

    try:
        for (m, n, kw) in [(24, 2000, {}), (48, 1500, dict(similar=0.5))]:
            msa = class_msa(rng, cls, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
            ok = _partitioned(engines, n)
            if not CLASSES[cls]["compact"]:
                # gap-free rows need the compact coding for the partitioned scan: every partition declines at once
                assert not any(ok[0]), (cls, m, n, ok)
                continue
            assert all(all(v) for v in ok), (cls, m, n, ok)
            for tricks_off in (False, True):
                assert np.array_equal(scan_f(n, tricks_off), O.compute_f(msa, disable_tricks=tricks_off)), (cls, m, n, tricks_off)
            ok = _partitioned(engines, n, reversed=True)
            assert all(all(v) for v in ok), (cls, m, n, ok)
            d_v = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engines[0].scan_v(0, n, d_v.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_v.cpu().numpy().astype(np.uint64), O.segment_v(msa)), (cls, m, n)
        # gaps and the ignore character: one setting of the elastic tricks per build
        msa = class_msa(rng, cls, 40, 1500, gap_cells=0.02, gap_run=5)
        for e in engines:
            e.msa_load_host(msa)
        for tricks_off in (False, True):
            ok = _partitioned(engines, 1500, ignorechars=ign, tricks_off=tricks_off)
            assert all(all(v) for v in ok), (cls, tricks_off, ok)
            assert np.array_equal(scan_f(1500, tricks_off), O.compute_f(msa, ignore=ign, disable_tricks=tricks_off)), (cls, tricks_off)
    finally:
        for e in engines:
            e.close()


# --------------------------------------------------------------------------------------------------------------------
# GPU: above 2^24 symbols with the default options (the thresholds msd_min / bp_min), each case asserting its path
# --------------------------------------------------------------------------------------------------------------------

def _assert_f_v(engine, msa, v_too=True):
    f = engine.elastic_f(msa)
    stats = {k: engine.get_option(k) for k in ("key_b", "key_K", "key_packed", "key_compact", "msd_decline", "rank_lean_launched", "rank_lean_used", "pairs_rb",
                                                "index_kind", "span_scan_used", "ext_pairs", "text_pairs")}
    ref = O.compute_f(msa)
    assert np.array_equal(f, ref), (stats, np.flatnonzero(f != ref)[:8])
    if v_too:
        gapped = bool((msa == GAP).any())
        got = engine.gapped_v(msa) if gapped else engine.repeatfree_v(msa)
        want = O.gapped_v(msa) if gapped else O.segment_v(msa)
        assert np.array_equal(got, want), (stats, np.flatnonzero(got != want)[:8])
    print("path", stats)
    return stats


@pytest.mark.gpu
def test_large_acgt_iid_default_path(engine):
    """1000 x 20000 ACGT (pb = 25): the three-pass MSD sort; f, v, and the suffix array and LCP arrays of the index
    against the oracle.  Here the slot-level scan gives up before its lean form starts and the group-level scan finishes
    (ext_pairs = -1: no slot-level result), so this case does not check the lean scan; test_large_lean_scan_default_path
    does, on rows of which it keeps the result."""
    rng = np.random.default_rng(2_000_000)
    msa = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (1000, 20000))]
    s = _assert_f_v(engine, msa)
    assert s["msd_decline"] == 0 and s["key_b"] == 2 and s["key_packed"] == 1 and s["index_kind"] == 1, s
    assert s["rank_lean_used"] == 0 and s["ext_pairs"] == -1, s
    engine.msa_load_host(msa)
    engine.index_build()
    assert engine.get_option("msd_decline") == 0 and engine.get_option("index_kind") == 1
    _, SA, ISA, LCP = O.msa_index(msa)
    _, gSA, _, gPL, gPR = engine.index_download()
    assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
    assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("planted", [False, True])
def test_large_slot_level_scan_default_path(engine, planted):
    """256 rows, 2 * 10^7 symbols and more (pb = 25), default options: the three-pass MSD sort, then the slot-level
    rank-order scan in its full form (its threshold stays at or below the key length, so the lean form does not apply:
    ext_pairs = text_pairs = 0); f and v against the oracle."""
    from test_sort_ext import planted_repeats
    rng = np.random.default_rng(3_000_000 + planted)
    msa = planted_repeats(rng, 256, 100_000) if planted else np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (256, 80_000))]
    assert msa.size > (1 << 24)
    s = _assert_f_v(engine, msa)
    assert s["msd_decline"] == 0 and s["index_kind"] == 1 and s["key_packed"] == 1, s
    assert s["rank_lean_used"] == 0 and s["ext_pairs"] == 0 and s["text_pairs"] == 0, s


@pytest.mark.gpu
def test_large_lean_scan_default_path(engine):
    """500 x 40000 with planted repeats 40 .. 80 symbols apart (pb = 25), default options: the three-pass MSD sort, the
    lean scan launched and its result kept (rank_lean_used), tied pairs settled both from the 4 symbols after the key
    (msd_ext pair codes) and by the text; f, v, the suffix array and the LCP arrays against the oracle.  (Tied suffixes
    must be frequent enough for a threshold above the key length -- 32 per column -- and rare enough that the slot-level
    scan keeps them: with 1000 rows and more it hands over to the group-level scan, see the next case.)"""
    from test_sort_ext import planted_repeats
    msa = planted_repeats(np.random.default_rng(5), 500, 40000, spacing=80)
    assert msa.size + 501 > (1 << 24)
    s = _assert_f_v(engine, msa)
    assert s["msd_decline"] == 0 and s["key_packed"] == 1 and s["index_kind"] == 1, s
    assert s["rank_lean_launched"] == 1 and s["rank_lean_used"] == 1 and s["ext_pairs"] > 0 and s["text_pairs"] > 0, s
    engine.msa_load_host(msa)
    engine.index_build()
    assert engine.get_option("rank_lean_used") == 1
    _index_matches(engine, msa, O.msa_index(msa))


@pytest.mark.gpu
def test_large_planted_repeats_default_path(engine):
    """1000 x 30000 with planted repeats (pb = 25): the lean scan is launched, then the slot-level scan hands over to the
    group-level scan, whose f and v are compared here (the lean result is discarded: rank_lean_used = 0)."""
    from test_sort_ext import planted_repeats
    msa = planted_repeats(np.random.default_rng(3_000_000), 1000, 30000)
    s = _assert_f_v(engine, msa)
    assert s["msd_decline"] == 0 and s["index_kind"] == 1, s
    assert s["rank_lean_launched"] == 1 and s["rank_lean_used"] == 0, s


@pytest.mark.gpu
def test_large_rows_at_the_lean_filter_limit_hand_over(engine):
    """Rows of 2211 symbols at pb = 25: 2 * delta of the lean filter is 0.00995, just inside its acceptance limit 0.01.
    Above 2^24 symbols such short rows mean 7600 rows and more per column, and there the slot-level scan does not keep its
    result (here, and for planted repeats at 7600 x 2210): the lean kernel is launched, the record path computes f.  So the
    filter's output at its widest eps is not compared with the oracle by any case; this one pins that the hand-over leaves
    a correct f (rank_lean_used = 0, index_kind = 0)."""
    m, n = 14000, 2210
    L, pb = n + 1, 25
    N = m * (n + 1) + 1
    assert (1 << (pb - 1)) < N <= (1 << pb)
    assert 0.0099 < 2 * ((2.0 ** (pb - 25) + 2.0 ** (pb - 22) + 2.0) / L + 1e-6) < 0.01
    rng = np.random.default_rng(2210)
    msa = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, n))]
    s = _assert_f_v(engine, msa, v_too=False)
    assert s["rank_lean_launched"] == 1 and s["rank_lean_used"] == 0 and s["index_kind"] == 0, s


@pytest.mark.gpu
def test_large_protein_default_path(engine):
    """500 x 60000 amino acids: the lean scan with 5-bit symbols, its result kept."""
    msa = class_msa(np.random.default_rng(60000), "protein", 500, 60000)
    s = _assert_f_v(engine, msa)
    assert s["key_b"] == 5 and s["key_compact"] == 1 and s["key_packed"] == 1 and s["index_kind"] == 1, s
    # pass 1 of the MSD sort sizes its stretches for first digits spread over all buckets; with 20 of the 32 codes in use
    # (as with uniform residues, or 40 of 64 codes) a stretch overfills: msd_decline = 2 | 4, rocPRIM sorts the keys
    assert s["msd_decline"] == 6 and s["rank_lean_launched"] == 1 and s["rank_lean_used"] == 1, s


@pytest.mark.gpu
@pytest.mark.parametrize("similar", [0.0, 0.99])
def test_large_iupac_with_gaps_default_path(engine, similar):
    """IUPAC DNA with gap runs, about 2.5 * 10^7 cells: the sample sort of pairs (b = 4, rank table with modes 1 and 2),
    then the slot-level scan (iid rows) or the span scan (star phylogeny); f with and without N as ignore character."""
    m, n = (500, 50000) if similar == 0 else (1000, 25000)
    msa = class_msa(np.random.default_rng(25 + int(similar * 100)), "iupac", m, n, similar=similar, gap_cells=0.02, gap_run=8)
    g = key_geometry(msa)
    assert g["N"] > (1 << 24) and g["b_pairs"] == 4 and g["rb"] == 2
    s = _assert_f_v(engine, msa)
    assert s["key_b"] == 4 and s["key_compact"] == 0 and s["index_kind"] == 2, s
    assert s["span_scan_used"] == (1 if similar else 0), s
    if not similar:
        assert s["pairs_rb"] == 2, s                    # the sample sort of pairs ran with its rank table of 4 symbols
    got = engine.elastic_f(msa, ignorechars="N")
    assert engine.get_option("span_decline") in (0, 10)
    assert np.array_equal(got, O.compute_f(msa, ignore="N"))


@pytest.mark.gpu
def test_large_streamed_upload_variants(engine):
    """fbg_elastic_f from memory of fbg_host_alloc, 64 x 600000: pass 1 of the MSD sort runs during the upload on the
    alphabet of the first chunk.  Variants against the oracle: gaps in the first eighth of the rows (no speculation);
    diverse leading rows with near-duplicate trailing rows (the keys' entropy taken from an unrepresentative chunk); fewer
    than 16 rows (no streaming); a NUL byte in a late chunk (refused as with the whole MSA uploaded first, then a correct
    build on the same context)."""
    from founderblockgraphs_amd import FbgError, _lib
    L = _lib.lib()
    m, n = 64, 600_000
    rng = np.random.default_rng(600_000)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    p = L.fbg_host_alloc(m * n)
    assert p
    try:
        pinned = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(m, n))
        np.copyto(pinned, A[rng.integers(0, 4, (m, n))])
        plain = pinned.copy()
        f_plain = O.compute_f(plain)
        assert np.array_equal(engine.elastic_f(pinned), f_plain)
        assert engine.get_option("pass1_ahead") == 1 and engine.get_option("msd_decline") == 0

        pinned[:m // 8, 1000:1013] = GAP
        assert np.array_equal(engine.elastic_f(pinned), O.compute_f(pinned))
        assert engine.get_option("pass1_ahead") == 0

        anc = A[rng.integers(0, 4, n)]
        np.copyto(pinned, np.tile(anc, (m, 1)))
        pinned[:m // 8] = A[rng.integers(0, 4, (m // 8, n))]
        mut = rng.random((m, n)) < 0.001
        pinned[mut] = A[rng.integers(0, 4, int(mut.sum()))]
        assert np.array_equal(engine.elastic_f(pinned), O.compute_f(pinned))

        small = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(12, m * n // 12))
        np.copyto(small, A[rng.integers(0, 4, small.shape)])
        assert np.array_equal(engine.elastic_f(small), O.compute_f(small))
        assert engine.get_option("pass1_ahead") == 0

        np.copyto(pinned, plain)
        pinned[m - 3, 4321] = 0
        codes = []
        for stream in (0, 1):
            with fbg_options(engine, {"no_stream_upload": 1 - stream}):
                with pytest.raises(FbgError) as err:
                    engine.elastic_f(pinned)
                codes.append(err.value.code)
        assert codes == [1, 1], codes                          # FBG_ERR_INVALID both ways
        np.copyto(pinned, plain)
        assert np.array_equal(engine.elastic_f(pinned), f_plain)
        assert engine.get_option("pass1_ahead") == 1
    finally:
        L.fbg_host_free(C.c_void_p(p))


@pytest.mark.gpu
def test_streamed_upload_refuses_a_late_nul_byte(engine):
    """The smallest streamed upload (16 rows, above 2^24 symbols) with a NUL byte in its last chunk: FBG_ERR_INVALID, as
    with the whole MSA uploaded first.  (Byte 0 occurs in the text either way -- the sentinel -- so the end check of the
    streamed upload compares its count.)"""
    from founderblockgraphs_amd import FbgError, _lib
    L = _lib.lib()
    m, n = 16, 1_100_000
    p = L.fbg_host_alloc(m * n)
    assert p
    try:
        pinned = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(m, n))
        np.copyto(pinned, np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(16).integers(0, 4, (m, n))])
        pinned[m - 1, n - 5] = 0
        with pytest.raises(FbgError) as err:
            engine.elastic_f(pinned)
        assert err.value.code == 1
    finally:
        L.fbg_host_free(C.c_void_p(p))
