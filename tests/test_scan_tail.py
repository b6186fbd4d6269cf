"""The tail of the rank-order scan (rank_scan.hip, rank_tail.hip): coded tied pairs settled inside the lean scan kernel (option
pairs_in_scan), long same-column runs walked by a wave each (k_runs_long; options runs_wave_min, wave_list_cap), the
candidate regions sorted in LDS (cand_local_sort).  Whatever the settings: f, v, the suffix array and the LCPs of the oracle."""
import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

_refs = {}


def _case(name):
    """An input and what the oracle says about it, computed once."""
    if name not in _refs:
        if name == "planted":
            msa = planted_repeats(np.random.default_rng(2024), 256, 20000)
        elif name.startswith("plantedT"):               # the first 256 / 200 rows end in T: one row-end run "T#" of four chunks of 64
            msa = planted_repeats(np.random.default_rng(2024), 256, 20000)
            msa[:int(name[8:]), -1] = ord("T")
        else:
            m, n = (int(x) for x in name.split("x"))
            msa = random_msa(np.random.default_rng(m * 7919 + n), m, n)
        T, SA, ISA, LCP = O.msa_index(msa)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        _refs[name] = {"msa": msa, "f": O.compute_f(msa), "v": O.segment_v(msa), "SA": SA.astype(np.int64), "PL": lcp_ext[ISA],
                       "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    return _refs[name]


def _check_index(engine, ref):
    """The index at hand against the oracle: suffix array and both neighbour LCPs of every text position."""
    gT, gSA, gISA, gPL, gPR = engine.index_download()
    assert np.array_equal(gSA.astype(np.int64), ref["SA"])
    assert np.array_equal(gPL.astype(np.int64), ref["PL"])
    assert np.array_equal(gPR.astype(np.int64), ref["PR"])


def test_pairs_in_scan_same_f_v_and_pair_counts(engine):
    """256 x 20000 with planted repeats (ties beyond the key by 0 .. 4 and more symbols): f and v equal the oracle's with the
    coded pairs settled in the scan kernel and by k_tie_pairs, with and without the MSD sort's extra symbols; the lean scan
    runs every time and counts the same pairs either way."""
    ref = _case("planted")
    seen, seen_v = {}, {}
    for ext in (1, 0):
        for in_scan in (1, 0):
            with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext), "FBG_PAIRS_IN_SCAN": str(in_scan)}):
                assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), (ext, in_scan)
                assert engine.get_option("rank_lean_used") == 1, (ext, in_scan)
                seen[ext, in_scan] = (engine.get_option("ext_pairs"), engine.get_option("text_pairs"))
                assert np.array_equal(engine.repeatfree_v(ref["msa"]), ref["v"]), (ext, in_scan)
                assert engine.get_option("rank_lean_used") == 1, (ext, in_scan)
                seen_v[ext, in_scan] = (engine.get_option("ext_pairs"), engine.get_option("text_pairs"))   # (another index: the text reversed)
    print("pairs (ext, in_scan) -> (by code, by text):", seen, "for v:", seen_v)
    assert seen[1, 1] == seen[1, 0] and seen[0, 1] == seen[0, 0], seen
    assert seen_v[1, 1] == seen_v[1, 0] and seen_v[0, 1] == seen_v[0, 0], seen_v
    assert seen[1, 1][0] > 0 and seen[1, 1][1] > 0, seen
    assert seen[0, 1][0] == 0 and seen[0, 1][1] > 0, seen


WAVE_SETTINGS = {
    "defaults": {},
    "min2": {"FBG_RUNS_WAVE_MIN": "2"},
    "off": {"FBG_RUNS_WAVE_MIN": "0"},
    "defaults_cap1": {"FBG_WAVE_LIST_CAP": "1"},
    "min2_cap1": {"FBG_RUNS_WAVE_MIN": "2", "FBG_WAVE_LIST_CAP": "1"},
}


@pytest.mark.parametrize("setting", list(WAVE_SETTINGS))
@pytest.mark.parametrize("name", ["1000x12", "600x20", "300x40", "planted", "plantedT256", "plantedT200"])
def test_wave_runs_index_equals_oracle(engine, name, setting):
    """f, v, the suffix array and the LCPs equal the oracle's with k_runs_long at its default threshold, at 2, switched off,
    and with a list of one entry (every other run falls back to its thread's own walk).
    The iid inputs have row-end runs of 250, 150 and 75 members, tie groups above and below 64 and rows shorter than the key,
    but rows this short tie almost everywhere: their scan hands over to the group-level scan ("wave_runs" stays -1).
    The planted inputs finish in rank order (the lean scan's result is used), so there the list must have been used as the
    settings say: 256 x 20000 ends its rows in one run of about 64 suffixes "X#" per symbol; with the last column set to T in
    all 256 rows, or in 200 of them, in one run "T#" of exactly four chunks of 64 members, or of three and a part -- the carry
    of both minimum scans from chunk to chunk.  (More rows do not fit a test: '#', "A#", "AA#" ... share the all-zero key, one
    tie group of 4/3 of the rows in one workgroup's candidate region of 256 + 1/8 of its slots, so 600 rows want 3 * 10^7 slots.)"""
    ref = _case(name)
    with fbg_options(engine, dict(WAVE_SETTINGS[setting], FBG_MSD_MIN="1")):
        assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"])
        got = engine.get_option("wave_runs")
        print(name, setting, "index_kind", engine.get_option("index_kind"), "wave_runs", got)
        if name.startswith("planted"):
            assert engine.get_option("rank_lean_used") == 1
            if setting == "off":
                assert got == 0
            elif setting.endswith("cap1"):
                assert got == 1
            else:
                assert got >= 4, got
        _check_index(engine, ref)
        assert np.array_equal(engine.repeatfree_v(ref["msa"]), ref["v"])      # (its index is that of the reversed text)


CAND_SETTINGS = {
    "local": {"FBG_CAND_LOCAL_SORT": "1"},
    "radix": {"FBG_CAND_LOCAL_SORT": "0"},
    "local_cap8": {"FBG_CAND_LOCAL_SORT": "1", "FBG_CAND_LDS_CAP": "8"},
}


@pytest.mark.parametrize("setting", list(CAND_SETTINGS))
@pytest.mark.parametrize("name", ["1000x12", "600x20", "300x40", "planted"])
def test_candidates_sorted_per_region_or_by_radix(engine, name, setting):
    """The candidate list ascends strictly (cand_sort_check) and f equals the oracle's whether the regions are sorted one by
    one in LDS or the radix sort runs.  On the planted 256 x 20000 input the lean scan runs, so the per-region sort must have
    been taken -- and not with its capacity forced to 8 entries, below the count of the regions that hold the row ends."""
    ref = _case(name)
    with fbg_options(engine, dict(CAND_SETTINGS[setting], FBG_MSD_MIN="1", FBG_CAND_SORT_CHECK="1")):
        assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"])
        local = engine.get_option("cand_local_sorted")
        print(name, setting, "index_kind", engine.get_option("index_kind"), "cand_local_sorted", local)
        assert engine.get_option("cand_inversions") == 0
        if name == "planted":
            assert engine.get_option("rank_lean_used") == 1
            assert local == (1 if setting == "local" else 0)
        else:
            assert local in ((0, 1, -1) if setting == "local" else (0, -1))
