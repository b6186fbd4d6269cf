"""The extension scans and the block graph at their capacity boundaries.

The scan in suffix order of an MSA with gaps (csrc/gapped_rank.hip) answers "which columns is this text position the
pointer of its row for" from a table of 16 bytes per 128 text positions (GWin: up to two gap runs, 16-bit run lengths, the
run before the window's first position apart in lo0); a position that points for more than GR_LONG columns leaves the
per-slot path; tie groups of up to GR_MAX_TIE suffixes are ordered in place, larger ones send the MSA to the record path.
The rank-order scan of a gap-free MSA (csrc/rank_scan.hip, rank_tail.hip, rank_common.h) settles tie groups of up to RS_TG inside the
scan, up to 64 from the candidate list, and declines beyond; it walks the slots in chunks of RS_CHUNK with RS_HALO slots
either side, the classification of gapped_rank.hip in stretches of GR_SEG.  fbg_block_graph (csrc/block_graph.hip)
groups a block's labels in LDS up to 4096 rows (above 2048 only with a raised dynamic LDS limit), in device memory up to
FBG_MAX_ROWS.  GR_LONG and RS_TG divide work between two paths that both compute the exact value: moving either by one
changes no result, and what these tests hold fixed there is that both sides of the hand-over agree with the oracle.  The
other limits change a result or the index kind when they move.
The inputs below sit on each of those numbers and one beside them; the CPU tests at the top assert that
the inputs have the run lengths, window contents, text lengths and tie group sizes they were built for, every GPU check
is exact equality with the oracle (oracle/pyoracle.py) or with output_efg's numbering restated in test_gpu_parity."""
import functools

import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O

GAP = ord("-")
GW = 128                                        # text positions per window (gapped_rank.hip: GW_BITS 7)
LONG16 = (65534, 65535, 65536, 65537)           # both sides of GWin::len's 16 bits
NEAR_GR_LONG = (63, 64, 65)                     # a run of L columns makes the next symbol the pointer for L + 1: GR_LONG 64
N_WIDE = 66_400


# ---- what an MSA looks like to the scans ----------------------------------------------------------------------------

def row_starts(msa):
    """text position of every row's first symbol: the rows without their gaps, a '#' behind each, then the sentinel"""
    syms = (msa != GAP).sum(axis=1)
    return np.concatenate([[0], np.cumsum(syms + 1)[:-1]]).astype(np.int64)


def text_length(msa):
    return int((msa != GAP).sum()) + msa.shape[0] + 1


def gap_runs(msa):
    """every maximal gap run as (row, first column, length, text position of what follows it in the row: a symbol or
    the row's '#')"""
    out = []
    starts = row_starts(msa)
    n = msa.shape[1]
    for i, row in enumerate(msa):
        g = np.concatenate([[False], row == GAP, [False]])
        first = np.flatnonzero(g[1:] & ~g[:-1])
        last = np.flatnonzero(g[:-1] & ~g[1:])
        before = np.concatenate([[0], np.cumsum(row != GAP)])
        for c, e in zip(first, last):
            assert e <= n
            out.append((i, int(c), int(e - c), int(starts[i] + before[e])))
    return out


def window_runs(msa):
    """window -> the in-window offsets of the positions that have a gap run right before them, as k_gw_build counts them:
    a run the row starts with is no event (the position is its row's first), nor is a run that ends the row (a '#'
    follows: the window is irregular anyway)"""
    n = msa.shape[1]
    out = {}
    for i, c, length, q in gap_runs(msa):
        if c > 0 and c + length < n:
            out.setdefault(q // GW, []).append(q % GW)
    return out


def insert_runs(row, runs):
    """the row with `length` gap cells put in right before its symbol number k, for every (k, length); cut to its length"""
    parts, last = [], 0
    for k, length in sorted(runs):
        parts += [row[last:k], np.full(length, GAP, dtype=np.uint8)]
        last = k
    parts.append(row[last:])
    return np.concatenate(parts)[:len(row)]


def symbol_at_offset(msa, row, offset, at_least=300):
    """the first symbol number k >= at_least of `row` whose text position lies at `offset` in its window (the rows
    before it are final)"""
    k = at_least + int((offset - (row_starts(msa)[row] + at_least)) % GW)
    assert (row_starts(msa)[row] + k) % GW == offset
    return k


# ---- part 2: gap-run lengths and window shapes ----------------------------------------------------------------------

def _base(seed, n):
    return random_msa(np.random.default_rng(seed), 8, n)


def build_runs_at_300():
    msa = _base(11, N_WIDE)
    lengths = LONG16 + NEAR_GR_LONG
    for i, length in enumerate(lengths):
        msa[i, 300:300 + length] = GAP
    return msa, dict(runs={i: [(300, length)] for i, length in enumerate(lengths)})


def build_rows_start_late():
    msa = _base(12, N_WIDE)
    for i, length in enumerate((64, 65, 65536)):
        msa[i, :length] = GAP
    return msa, dict(runs={i: [(0, length)] for i, length in enumerate((64, 65, 65536))})


def build_rows_end_early():
    msa = _base(13, N_WIDE)
    for i, length in enumerate((64, 65, 65536)):
        msa[i, N_WIDE - length:] = GAP
    return msa, dict(runs={i: [(N_WIDE - length, length)] for i, length in enumerate((64, 65, 65536))})


def _build_in_window(seed, row, offsets, lengths):
    msa = _base(seed, 3000)
    k0 = symbol_at_offset(msa, row, offsets[0])
    runs = [(k0 + o - offsets[0], length) for o, length in zip(offsets, lengths)]
    msa[row] = insert_runs(msa[row], runs)
    q0 = int(row_starts(msa)[row]) + k0
    return msa, dict(runs={row: None}, lengths={row: list(lengths)}, window=(q0 // GW, sorted(offsets)))


def build_two_runs_in_a_window():
    return _build_in_window(14, 2, (10, 50), (5, 9))


def build_three_runs_in_a_window():
    return _build_in_window(15, 2, (10, 50, 110), (5, 9, 3))


def build_run_ends_at_window_start():
    return _build_in_window(16, 3, (0,), (7,))


def build_run_ends_one_later():
    return _build_in_window(17, 3, (1,), (7,))


def build_window_with_a_separator():
    """row 2 has a gap run five symbols before its '#', row 3 one before its fourth symbol: both in the '#' window"""
    msa = _base(18, 3000)
    msa[2] = insert_runs(msa[2], [(3000 - 6 - 5, 6)])
    msa[3] = insert_runs(msa[3], [(3, 4)])
    sep = int(row_starts(msa)[3]) - 1
    return msa, dict(runs={2: None, 3: None}, lengths={2: [6], 3: [4]}, window=(sep // GW, sorted([sep % GW - 5, sep % GW + 4])),
                     separator=sep)


def build_all_gap_columns():
    msa = _base(19, 3000)
    msa[:, 500:503] = GAP
    msa[1, 498:510] = GAP
    msa[4, 500:580] = GAP
    runs = {i: [(500, 3)] for i in range(8)}
    runs[1], runs[4] = [(498, 12)], [(500, 80)]
    return msa, dict(runs=runs, all_gap_columns=3)


GAP_CASES = {
    "runs_at_300": build_runs_at_300,
    "rows_start_late": build_rows_start_late,
    "rows_end_early": build_rows_end_early,
    "two_runs_in_a_window": build_two_runs_in_a_window,
    "three_runs_in_a_window": build_three_runs_in_a_window,
    "run_ends_at_window_start": build_run_ends_at_window_start,
    "run_ends_one_later": build_run_ends_one_later,
    "window_with_a_separator": build_window_with_a_separator,
    "all_gap_columns": build_all_gap_columns,
}


def build_star_long_runs():
    """five noisy copies of one ancestor (1 % substitutions); rows 0 to 3 skip 65534 .. 65537 columns from column 300"""
    rng = np.random.default_rng(20)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    msa = np.tile(alpha[rng.integers(0, 4, N_WIDE)], (5, 1))
    mut = rng.random(msa.shape) < 0.01
    msa[mut] = alpha[rng.integers(0, 4, int(mut.sum()))]
    for i, length in enumerate(LONG16):
        msa[i, 300:300 + length] = GAP
    return msa, dict(runs={i: [(300, length)] for i, length in enumerate(LONG16)})


# ---- part 3: tie groups of exact sizes ------------------------------------------------------------------------------

TIE_PLAIN = (2, 4, 5, 63, 64, 65, 66)           # RS_TG 4; GR_MAX_TIE 64 and the 64 members of k_tie_groups / k_tie_big
TIE_ENTANGLED = (2, 32, 33)                     # groups of 2k whose members share columns pairwise: 4, 64, 66
TIE_CASES = [(k, False) for k in TIE_PLAIN] + [(k, True) for k in TIE_ENTANGLED]
PLANT = 48                                      # symbols the k rows share; a sort key holds 32 at the most


def build_ties(k, entangled, variant):
    """80 x 400 iid; rows 0 .. k-1 share columns 100 .. 147 (entangled: the same 48 symbols at columns 250 .. 297 too).
    variant "gaps": two short gap runs in rows 78 and 79; "ignore": 0.5 % N cells outside the planted columns."""
    rng = np.random.default_rng(3000 + k)
    msa = random_msa(rng, 80, 400)
    msa[1:k, 100:100 + PLANT] = msa[0, 100:100 + PLANT]
    if entangled:
        msa[:k, 250:250 + PLANT] = msa[0, 100:100 + PLANT]
    if variant == "gaps":
        msa[78, 10:15] = GAP
        msa[79, 30:37] = GAP
    if variant == "ignore":
        cells = rng.random(msa.shape) < 0.005
        cells[:, 100:100 + PLANT] = False
        cells[:, 250:250 + PLANT] = False
        msa[cells] = ord("N")
    return msa


def tie_group_sizes(lcp, depth=32):
    """sizes of the maximal groups of suffixes, neighbours in the suffix array, that agree on their first `depth` symbols"""
    tied = np.concatenate([[False], np.asarray(lcp)[1:] >= depth, [False]])
    first = np.flatnonzero(tied[1:] & ~tied[:-1])
    last = np.flatnonzero(tied[:-1] & ~tied[1:])
    return last - first + 1


# ---- part 4: text lengths on chunk edges ----------------------------------------------------------------------------

CHUNK_SHAPES = {1024: (3, 340), 1025: (1, 1023), 2047: (2, 1022), 2048: (1, 2046), 2049: (2, 1023)}     # RS_CHUNK 1024
SEG_LENGTHS = (16384, 16385, 32768)                                                                  # GR_SEG 16384


def build_chunk_edge(N):
    m, n = CHUNK_SHAPES[N]
    return random_msa(np.random.default_rng(N), m, n, alphabet="AC", similar=0.9)


def build_seg_edge(N):
    """8 rows with short gap runs; the last row ends early, by as much as makes the text N symbols long"""
    n = N // 7
    msa = random_msa(np.random.default_rng(N), 8, n, gap_p=0.01, gap_run=6)
    msa[7] = random_msa(np.random.default_rng(N + 1), 1, n)[0]
    keep = N - text_length(msa[:7]) - 1          # symbols of the last row (its '#' is one more)
    assert 0 < keep < n
    msa[7, keep:] = GAP
    return msa


# ---- references, computed once --------------------------------------------------------------------------------------

def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """(msa, claims, oracle results) of one input; the arrays are read-only and shared by the tests"""
    claims, ignore = {}, ""
    if kind == "gaps":
        msa, claims = GAP_CASES[key[0]]()
    elif kind == "star":
        msa, claims = build_star_long_runs()
    elif kind == "ties":
        msa = build_ties(*key)
        ignore = "N" if key[2] == "ignore" else ""
    elif kind == "chunk":
        msa = build_chunk_edge(key[0])
    else:
        msa = build_seg_edge(key[0])
    msa = _frozen(np.ascontiguousarray(msa))
    n = msa.shape[1]
    f0 = np.random.default_rng(n).integers(0, n, n).astype(np.uint64)
    ref = dict(ignore=ignore, f0=_frozen(f0),
               f_on=_frozen(O.compute_f(msa, ignore=ignore)),
               f_off=_frozen(O.compute_f(msa, ignore=ignore, disable_tricks=True)),
               f_merge=_frozen(O.compute_f(msa, ignore=ignore, f_init=f0)),
               index=tuple(_frozen(x) for x in O.msa_index(msa)))
    if kind in ("gaps", "seg"):
        ref["gapped_v"] = _frozen(O.gapped_v(msa))
    if kind in ("ties", "chunk") and key[-1] not in ("gaps", "ignore"):
        ref["v"] = _frozen(O.segment_v(msa))
    return msa, claims, ref


def _has_a_segmentation(msa, ref):
    """with the elastic tricks off f[0] == n means 'no valid segmentation' (fbg.cpp:2004-2013): the engine raises
    instead of returning f, so such an input cannot be compared"""
    assert ref["f_off"][0] != msa.shape[1]


# ---- part 1: the inputs have the properties they were built for (no GPU) ---------------------------------------------

@pytest.mark.parametrize("name", sorted(GAP_CASES) + ["star"])
def test_gap_inputs_have_the_runs_asked_for(name):
    msa, claims, ref = reference("star") if name == "star" else reference("gaps", name)
    m, n = msa.shape
    runs = gap_runs(msa)
    for row in range(m):
        mine = [(c, length) for i, c, length, q in runs if i == row]
        want = claims["runs"].get(row, [])
        if want is None:                         # runs put in by symbol number: their lengths, in order
            assert [length for c, length in mine[:len(claims["lengths"][row])]] == claims["lengths"][row], (name, row, mine)
        else:
            assert mine == want, (name, row, mine)
    per_window = window_runs(msa)
    if "window" in claims:
        w, offsets = claims["window"]
        assert sorted(per_window.get(w, [])) == offsets, (name, w, per_window.get(w))
    if "separator" in claims:
        assert ref["index"][0][claims["separator"]] == ord("#") and claims["separator"] // GW == claims["window"][0]
    if "all_gap_columns" in claims:
        assert int((msa == GAP).all(axis=0).sum()) == claims["all_gap_columns"]
    if name in ("runs_at_300", "star"):          # every run alone in its window, none at a window's first position
        assert all(len(v) == 1 and v[0] != 0 for v in per_window.values()) and len(per_window) == len(claims["runs"])
    assert (msa != GAP).sum(axis=1).min() > 0
    assert len(ref["index"][0]) == text_length(msa) == int((msa != GAP).sum()) + m + 1
    _has_a_segmentation(msa, ref)


def test_window_cases_differ_where_they_should():
    """two against three runs in one window, and a run before offset 0 against one before offset 1"""
    events = {name: window_runs(reference("gaps", name)[0]) for name in GAP_CASES}
    assert max(len(v) for v in events["two_runs_in_a_window"].values()) == 2
    assert max(len(v) for v in events["three_runs_in_a_window"].values()) == 3
    assert list(events["run_ends_at_window_start"].values()) == [[0]]
    assert list(events["run_ends_one_later"].values()) == [[1]]


@pytest.mark.parametrize("variant", ["plain", "gaps", "ignore"])
@pytest.mark.parametrize("k,entangled", TIE_CASES)
def test_tie_inputs_have_groups_of_the_size_asked_for(k, entangled, variant):
    msa, _, ref = reference("ties", k, entangled, variant)
    T, SA, ISA, LCP = ref["index"]
    sizes = tie_group_sizes(LCP)
    want = 2 * k if entangled else k
    # one group per start column 100 .. 100 + PLANT - 32, none larger anywhere
    assert sizes.max() == want and int((sizes == want).sum()) >= PLANT - 32 + 1, (k, entangled, variant, np.bincount(sizes))
    assert 4 * int(sizes.sum()) < len(T)         # far from "a quarter of the slots tie" (rank_scan.hip:33)
    assert len(T) == text_length(msa)
    assert len(T) == 80 * 401 + 1 or variant == "gaps"
    assert (ord("N") in msa) == (variant == "ignore") and (GAP in msa) == (variant == "gaps")
    _has_a_segmentation(msa, ref)


@pytest.mark.parametrize("N", sorted(CHUNK_SHAPES) + list(SEG_LENGTHS))
def test_texts_have_the_lengths_asked_for(N):
    msa, _, ref = reference("chunk", N) if N in CHUNK_SHAPES else reference("seg", N)
    m, n = msa.shape
    assert len(ref["index"][0]) == N == text_length(msa)
    if N in CHUNK_SHAPES:
        assert GAP not in msa and N == m * (n + 1) + 1
        # rows that share stretches tie on whole keys; a single row over AC only repeats itself over a few symbols
        assert tie_group_sizes(ref["index"][3], 32 if m > 1 else 8).size > 0
    else:
        assert GAP in msa[:7] and (msa[7] != GAP).sum() < n
    _has_a_segmentation(msa, ref)


# ---- GPU checks -----------------------------------------------------------------------------------------------------

def _check_index(engine, index, where):
    T, SA, ISA, LCP = index
    gT, gSA, gISA, gPL, gPR = engine.index_download()
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    isa = ISA.astype(np.int64)
    assert np.array_equal(gT, T), (where, "text")
    assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64)), (where, "SA", np.flatnonzero(gSA != SA)[:8])
    assert np.array_equal(gISA.astype(np.int64), isa), (where, "ISA")
    assert np.array_equal(gPL.astype(np.int64), lcp_ext[isa]), (where, "LCP with the suffix before")
    assert np.array_equal(gPR.astype(np.int64), lcp_ext[isa + 1]), (where, "LCP with the suffix after")


def _same(got, want, where):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (where, "columns", bad[:8].tolist(), "got", got[bad[:8]].tolist(), "oracle", want[bad[:8]].tolist())


def _check_scan(engine, msa, ref, kind, where, merge=True):
    """f with the tricks on and off, the max-merge, three column shards, the index arrays: all against the oracle;
    index_kind after every build"""
    import torch
    n, ignore = msa.shape[1], ref["ignore"]
    for off, want in ((False, ref["f_on"]), (True, ref["f_off"])):
        _same(engine.elastic_f(msa, ignorechars=ignore, disable_efg_tricks=off), want, (where, "tricks off" if off else "tricks on"))
        assert engine.get_option("index_kind") == kind, (where, "index_kind", engine.get_option("index_kind"), "expected", kind)
    if merge:
        _same(engine.elastic_f(msa, ignorechars=ignore, f=ref["f0"]), ref["f_merge"], (where, "max-merge"))
    engine.msa_load_host(msa)
    engine.index_build(ignorechars=ignore)
    assert engine.get_option("index_kind") == kind, (where, "index_kind", engine.get_option("index_kind"), "expected", kind)
    for off, want in ((True, ref["f_off"]), (False, ref["f_on"])):
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for r in range(3):
            engine.scan_f(n * r // 3, n * (r + 1) // 3, d_f.data_ptr(), disable_efg_tricks=off)
        engine.sync()
        _same(d_f.cpu().numpy().astype(np.uint64), want, (where, "three shards", "tricks off" if off else "tricks on"))
    _check_index(engine, ref["index"], where)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["suffix_order", "records"])
@pytest.mark.parametrize("name", sorted(GAP_CASES))
def test_gap_run_lengths_and_window_shapes(engine, name, path):
    """gapped_rank.hip: GWin::len is 16 bits (:58-64; k_gw_build's `wide`, :200-201), a window holds two runs (`events > 2`,
    :199-201), the run before a window's first position goes to lo0 (:195-196, :214; read back by gr_span :137-138 and
    gr_win_col :104-111), a window with a '#' is irregular (:194), and a position that points for more than GR_LONG = 64
    columns (:49, :392: a run of 64 and more, the gaps a row starts or ends with) goes to k_grs_long.  Runs of 65534 ..
    65537 and 63 .. 65 columns, rows that start late / end early by 64, 65 and 65536, two and three runs in one window, a
    run that ends at a window's first position and one position later, runs in the window of a '#', columns of gaps only.
    Restates compute_f (fbg.cpp:1579-1695; the pointer that waits through a gap run, 1687-1691; fullrow[], 1605-1608;
    the clamp at the row's end, 1657-1670) and segment2elasticValid's v (fbg.cpp:763-822).  path "records": the same
    inputs under gapped_rank = -1, whose colT and per-cell tables see the same run lengths (index_kind 0)."""
    msa, _, ref = reference("gaps", name)
    with fbg_options(engine, {"gapped_rank": -1 if path == "records" else 0}):
        _check_scan(engine, msa, ref, 0 if path == "records" else 2, (name, path))
        _same(engine.gapped_v(msa), ref["gapped_v"], (name, path, "gapped_v"))


@pytest.mark.gpu
def test_long_gap_runs_in_similar_rows(engine):
    """The runs of 65534 .. 65537 columns in rows that are copies of one ancestor, under span_scan = 1 (span_scan.hip reads
    the same window table through fbg_grs_prepare, gapped_rank.hip:932-951, k_gw_build's `wide` :200): f equals
    compute_f's (fbg.cpp:1579-1695, 1687-1691) whether the group-level scan kept the input or handed it on."""
    msa, _, ref = reference("star")
    with fbg_options(engine, {"span_scan": 1}):
        for off, want in ((False, ref["f_on"]), (True, ref["f_off"])):
            got = engine.elastic_f(msa, disable_efg_tricks=off)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, ("tricks off" if off else "tricks on", "span_scan_used", engine.get_option("span_scan_used"),
                                   "span_decline", engine.get_option("span_decline"), bad[:8].tolist())


def _tie_kind(size, fast, limit=64):
    return fast if size <= limit else 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,entangled", TIE_CASES)
def test_tie_groups_of_exact_sizes_gap_free(engine, k, entangled):
    """rank_scan.hip / rank_common.h: a tie group of up to RS_TG = 4 suffixes is settled inside the scan (rank_common.h:7,
    :189-194, k_tie_simple rank_scan.hip:543-582), up to 64 by k_tie_groups from the candidate list (rank_tail.hip:113-156,
    `s > 64` :126), more go to k_tie_big, which raises the fallback flag for more than 64 members with K real symbols (:166,
    :207).
    Groups of exactly 2, 4, 5, 63, 64, 65 and 66 suffixes, and of 4, 64 and 66 whose members share columns pairwise (the
    runs of k_runs, rank_tail.hip:241).  f (fbg.cpp:1579-1695, the walk 1633-1678), v (fbg.cpp:552-611) and the index arrays.
    index_kind: with pure_scan = -1 the rank-order scan is the only fast path: 1 up to 64 members, 0 (records) from 65 on;
    likewise under force_wide, a layout the group-level scan does not take (pure_scan.hip:315).  With the default options
    a decline of the rank-order scan is followed by the group-level scan (suffix_sort.hip, ranked_path), which holds groups of
    up to 8192 members (pure_scan.hip:33) and keeps index_kind at 1 for 65 and 66 too; so do no_packed and pure_scan = 1."""
    msa, _, ref = reference("ties", k, entangled, "plain")
    size = 2 * k if entangled else k
    for switches, kind in (({"pure_scan": -1}, _tie_kind(size, 1)), ({}, 1), ({"FBG_NO_PACKED": "1"}, 1),
                           ({"FBG_FORCE_WIDE": "1"}, _tie_kind(size, 1)), ({"FBG_PURE_SCAN": "1"}, 1)):
        where = ("tie group of", size, "entangled" if entangled else "plain", tuple(switches))
        with fbg_options(engine, switches):
            _check_scan(engine, msa, ref, kind, where, merge=False)
            _same(engine.repeatfree_v(msa), ref["v"], (where, "repeatfree_v"))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["gaps", "ignore"])
@pytest.mark.parametrize("k,entangled", TIE_CASES)
def test_tie_groups_of_exact_sizes_with_gaps_or_ignore_characters(engine, k, entangled, variant):
    """gapped_rank.hip: gr_order_group orders a tie group of up to GR_MAX_TIE = 64 suffixes in place and raises the decline
    flag for more (:51, :247-248; read by ties_fit :1076-1082), after which the record path builds the index.  The inputs
    of the gap-free test with two short gap runs in rows outside the group, or with 0.5 % N cells under --ignore-chars N
    (the clamp at an ignore character, fbg.cpp:1669-1670): f with the tricks on and off (fbg.cpp:1579-1695) and the index
    arrays.  index_kind: 2 up to 64 members, 0 from 65 on."""
    msa, _, ref = reference("ties", k, entangled, variant)
    size = 2 * k if entangled else k
    _check_scan(engine, msa, ref, _tie_kind(size, 2), ("tie group of", size, "entangled" if entangled else "plain", variant), merge=False)


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(CHUNK_SHAPES))
def test_gap_free_text_lengths_on_chunk_edges(engine, N):
    """rank_scan.hip: k_rank_scan stages RS_CHUNK = 1024 slots and RS_HALO = 8 either side (:50, rank_common.h:159; the
    last chunk's hi_i :77, :96, the first chunk's lo_i :76, :95).  Texts of 1024, 1025, 2047, 2048 and 2049 symbols over
    AC with shared stretches, so that tie groups and runs lie at the chunk ends.  f (fbg.cpp:1579-1695), v
    (fbg.cpp:552-611) and the index arrays."""
    msa, _, ref = reference("chunk", N)
    for switches in ({}, {"FBG_NO_PACKED": "1"}, {"pure_scan": -1}):
        with fbg_options(engine, switches):
            where = ("text of", N, tuple(switches))
            n = msa.shape[1]
            for off, want in ((False, ref["f_on"]), (True, ref["f_off"])):
                _same(engine.elastic_f(msa, disable_efg_tricks=off), want, (where, "tricks off" if off else "tricks on"))
            _same(engine.repeatfree_v(msa), ref["v"], (where, "repeatfree_v"))
            engine.msa_load_host(msa)
            engine.index_build()
            _check_index(engine, ref["index"], where)
            assert engine.text_length() == N and n == CHUNK_SHAPES[N][1]


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0, 4], ids=["every_slot", "classified"])
@pytest.mark.parametrize("N", SEG_LENGTHS)
def test_gapped_text_lengths_on_segment_edges(engine, N, threshold):
    """gapped_rank.hip: k_grs_classify gives a workgroup GR_SEG = 16384 slots and a stretch of the list of that capacity
    (:504, :540-554; nseg :1085).  It runs when the scan has a threshold -- by itself only above 4 * GR_SAMPLE slots
    (:1048), at this size under gapped_rank = 4 ("classified"); "every_slot" is the same text through k_grs_scan_all.
    Texts of 16384, 16385 and 32768 symbols.  f (fbg.cpp:1579-1695), v of segment2elasticValid (fbg.cpp:763-822) and
    the index arrays."""
    msa, _, ref = reference("seg", N)
    with fbg_options(engine, {"gapped_rank": threshold}):
        _check_scan(engine, msa, ref, 2, ("text of", N, "gapped_rank", threshold))
        _same(engine.gapped_v(msa), ref["gapped_v"], (N, threshold, "gapped_v"))
        assert engine.text_length() == N


# ---- part 5: block graph tiers --------------------------------------------------------------------------------------

def _check_block_graph(engine, msa, boundaries, where):
    from test_gpu_parity import _block_graph_reference
    boundaries = np.asarray(boundaries, dtype=np.uint64)
    engine.msa_load_host(msa)
    node_of, first, rep_row, ecount, edges = engine.block_graph(boundaries)
    r_node, r_first, r_reps, r_edges = _block_graph_reference(msa, boundaries)
    assert np.array_equal(first, r_first), (where, "first_node")
    assert np.array_equal(node_of, r_node), (where, "node_of")
    for j in range(len(boundaries)):
        cnt = int(first[j + 1] - first[j])
        assert list(rep_row[j, :cnt]) == r_reps[j], (where, "rep_row of block", j)
        got = [(int(x) >> 32, int(x) & 0xffffffff) for x in edges[j, :int(ecount[j])]]
        assert got == r_edges[j], (where, "edges into block", j)
    return first, ecount


def _cuts(rng, n, nb):
    """nb block ends, the last one n (fbg.cpp:2026-2039)"""
    return np.concatenate([np.sort(rng.choice(np.arange(2, n - 2), size=nb - 1, replace=False)), [n]]).astype(np.uint64)


def _distinct_rows(rng, m, boundaries, n):
    """every row's label differs from every other row's in every block: a permutation of 0 .. m-1 in base 4"""
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    msa = alpha[rng.integers(0, 4, (m, n))]
    start = 0
    for end in boundaries:
        end = min(int(end) + 1, n)
        width = end - start
        assert 4 ** width >= m
        perm = rng.permutation(m)
        for d in range(min(width, 6)):
            msa[:, start + d] = alpha[(perm >> (2 * d)) & 3]
        start = end
    return msa


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2048, 2049, 3000, 4096, 4097])
def test_block_graph_row_tiers(engine, m):
    """block_graph.hip: k_block_group's dynamic LDS is (2 * ts + 2 * m) * 4 bytes, ts the first power of two >= 2 * m (:251-253);
    2049 .. 4096 rows need 80 .. 96 KB and the raised limit of hipFuncSetAttribute (:257-259), 4097 rows the tables in
    device memory (:254-265).  k_block_edges sorts cap = the first power of two >= m pairs (:280-286): at 2048 and 4096
    rows cap == m, no padding entry.  There also: every row distinct in every block (m nodes, m edges per block) and all
    rows identical (one node per block).  Against output_efg's numbering (fbg.cpp:1224-1260)."""
    rng = np.random.default_rng(5000 + m)
    n = 60
    boundaries = _cuts(rng, n, int(rng.integers(5, 9)))
    _check_block_graph(engine, random_msa(rng, m, n, similar=0.9, gap_p=0.01, gap_run=4), boundaries, (m, "similar rows"))
    if m in (2048, 4096):
        wide = np.array([11, 23, 35, 47, n], dtype=np.uint64)           # blocks of 12 columns: room for m distinct labels
        first, ecount = _check_block_graph(engine, _distinct_rows(rng, m, wide, n), wide, (m, "distinct rows"))
        assert np.array_equal(np.diff(first.astype(np.int64)), np.full(len(wide), m)), (m, "cap == m: nodes per block")
        assert list(ecount) == [0] + [m] * (len(wide) - 1), (m, "cap == m: edges per block")
        same = np.tile(random_msa(rng, 1, n), (m, 1))
        first, ecount = _check_block_graph(engine, same, boundaries, (m, "identical rows"))
        assert list(first) == list(range(len(boundaries) + 1)) and list(ecount) == [0] + [1] * (len(boundaries) - 1)


@pytest.mark.gpu
def test_block_graph_block_shapes(engine):
    """block_graph.hip at 300 rows: a block in which every row is gaps (the empty label, h1 == h2 == 0, :63, :103, :112: no
    node, no edge in or out, :159-161), a row that is empty in block j-1 and not in block j, a single block, and a last
    boundary of n against n-1 (bg_block_range clamps like std::string::substr, :38-43).  Against output_efg's numbering
    (fbg.cpp:1224-1260; the last boundary, fbg.cpp:2026-2039)."""
    rng = np.random.default_rng(5300)
    m, n = 300, 60
    msa = random_msa(rng, m, n, similar=0.9, gap_p=0.01, gap_run=4)
    boundaries = np.array([9, 19, 29, 39, 49, n], dtype=np.uint64)
    msa[:, 20:30] = GAP                          # block 2: no label at all
    msa[5, 30:40] = GAP                          # row 5: empty in block 3, back in block 4
    first, ecount = _check_block_graph(engine, msa, boundaries, "all-gap block")
    assert first[3] == first[2] and ecount[2] == 0 and ecount[3] == 0 and ecount[4] > 0
    a = _check_block_graph(engine, msa, [n], "one block")
    assert int(a[0][1]) > 0 and list(a[1]) == [0]
    b = _check_block_graph(engine, msa, boundaries[:-1].tolist() + [n - 1], "last boundary n - 1")
    assert np.array_equal(b[0], first) and np.array_equal(b[1], ecount)


@pytest.mark.gpu
def test_block_graph_row_limit(engine):
    """block_graph.hip:222, include/fbg_hip.h:47: FBG_MAX_ROWS = 32768 rows are taken (the tables in device memory, :254-265)
    and equal output_efg's numbering (fbg.cpp:1224-1260); 32769 rows are refused with an error, after which the engine
    still answers a small call exactly."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(5400)
    n = 24
    boundaries = np.array([7, 15, n], dtype=np.uint64)
    big = random_msa(rng, 32769, n, similar=0.9, gap_p=0.01, gap_run=4)
    _check_block_graph(engine, big[:32768], boundaries, "32768 rows")
    engine.msa_load_host(big)
    with pytest.raises(F.FbgError, match="rows"):
        engine.block_graph(boundaries)
    _check_block_graph(engine, big[:5], boundaries, "5 rows after the refusal")
