"""The lean rank-order scan with the loads of several rows in flight per wave (option scan_rows_ahead, rank_scan.hip), on the
slots of the three-pass MSD sort (msd_sort.hip), k_msd_finish_big included.  Whatever the depth: f, v, the suffix array and the
LCPs of the oracle, and the same tied pairs as one row ahead."""
import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O
from test_scan_tail import _case as _tail_case, _check_index
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

_refs = {}
_pairs1 = {}

# The lean scan wants more than 2^22 slots and ties in every column.  4096 workgroups of four waves share the slots, a wave
# takes rows of 58:
#   planted        256 x 20000, 5.12 * 10^6 slots: six rows per wave -- a full group and a partial one four rows deep, two groups
#                  of three (both register sets), three of two
#   planted16500   256 x 16500, just above 2^22: five rows per wave, waves with nothing left and a partial stretch at the end
#   plantedT256    256 x 20000 with one long run "T#" at the row ends
SHAPES = ["planted", "planted16500", "plantedT256"]


def _case(name):
    """An input and what the oracle says about it, computed once (the 256 x 20000 inputs are test_scan_tail's)."""
    if name != "planted16500":
        return _tail_case(name)
    if name not in _refs:
        msa = planted_repeats(np.random.default_rng(2025), 256, 16500)
        T, SA, ISA, LCP = O.msa_index(msa)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        _refs[name] = {"msa": msa, "f": O.compute_f(msa), "v": O.segment_v(msa), "SA": SA.astype(np.int64), "PL": lcp_ext[ISA],
                       "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    return _refs[name]


def _run(engine, ref, ext, depth):
    """f, the index and v at one depth against the oracle; returns the tied pairs (by code, by text) of the two indexes."""
    with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext), "FBG_SCAN_ROWS_AHEAD": str(depth)}):
        assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"])
        assert engine.get_option("rank_lean_used") == 1
        assert engine.get_option("msd_decline") == 0
        pairs_f = (engine.get_option("ext_pairs"), engine.get_option("text_pairs"))
        _check_index(engine, ref)
        assert np.array_equal(engine.repeatfree_v(ref["msa"]), ref["v"])      # (another index: the text reversed)
        assert engine.get_option("rank_lean_used") == 1
        pairs_v = (engine.get_option("ext_pairs"), engine.get_option("text_pairs"))
    return pairs_f, pairs_v


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("ext", [1, 0])
@pytest.mark.parametrize("name", SHAPES)
def test_rows_ahead_index_equals_oracle(engine, name, ext, depth):
    """Every shape at depth 1 (one row ahead, the loop before this option), 2, 3 (two register sets) and 4 (one set, loaded in
    place), with the extra-symbol bytes and without: f and v equal the oracle's, so do the suffix array and both neighbour
    LCPs, the lean scan's result is the one used, and the scan notes the same tied pairs as at depth 1."""
    ref = _case(name)
    got = _run(engine, ref, ext, depth)
    if (name, ext) not in _pairs1:
        _pairs1[name, ext] = got if depth == 1 else _run(engine, ref, ext, 1)
    print(name, "ext", ext, "depth", depth, "pairs (by code, by text) of f and v:", got, "at depth 1:", _pairs1[name, ext])
    assert got == _pairs1[name, ext]
    if ext == 0:
        assert got[0][0] == 0 and got[0][1] > 0, got
    else:
        assert got[0][0] > 0, got


def test_default_depth_is_a_compiled_one(engine):
    """0 (the default) and values outside 1 .. 4 run the default depth: same f, same pairs."""
    ref = _case("planted")
    base = _run(engine, ref, 1, 0)
    assert engine.get_option("scan_rows_ahead") == 0
    assert _run(engine, ref, 1, 9) == base
    assert _run(engine, ref, 1, -1) == base


def test_sub_bucket_beyond_its_stretch_goes_through_finish_big(engine):
    """4000 rows of 12 columns: '#', "A#", "AA#" ... share the all-zero key, 4/3 of the rows in one sub-bucket of pass 2 -- more
    than its stretch of 4096 slots holds and fewer than k_msd_finish_big's 16384, so the slots beyond the stretch go through
    the arena and that kernel sorts and writes the sub-bucket.  The sort must not decline; suffix array, LCPs and f equal the
    oracle's."""
    m, n = 4000, 12
    msa = random_msa(np.random.default_rng(m * 7919 + n), m, n)
    trailing_a = np.zeros(m, dtype=np.int64)                   # suffixes of a row that are A's up to the row's end, and '#' itself
    alive = np.ones(m, dtype=bool)
    for c in range(n - 1, -1, -1):
        alive &= msa[:, c] == ord("A")
        trailing_a += alive
    zero_key = int((trailing_a + 1).sum())
    assert 4096 < zero_key <= 16384, zero_key
    T, SA, ISA, LCP = O.msa_index(msa)
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    ref = {"SA": SA.astype(np.int64), "PL": lcp_ext[ISA], "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    f_ref = O.compute_f(msa)
    for ext in (1, 0):
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext)}):
            engine.msa_load_host(msa)
            engine.index_build()
            assert engine.get_option("msd_decline") == 0
            _check_index(engine, ref)
            assert np.array_equal(engine.elastic_f(msa), f_ref)
