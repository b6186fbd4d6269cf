"""The short serial steps of the gap-free index build taken off its critical path: the size of a tie group found by galloping
over the sorted keys (tie_gallop, csrc/tie_extent.h), one kernel for the candidate counts (cand_counts_fused) and the sample
of the sorted keys by a fixed grid (tie_sample_loop).  None of them changes a result: f, v, the suffix array and the LCPs of the oracle, whatever the settings."""
import numpy as np
import pytest

from conftest import fbg_options
from oracle import pyoracle as O
from test_scan_tail import _case, _check_index
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

TIE_PROBE = 8          # FBG_TIE_PROBE of csrc/tie_extent.h: the slots looked at one by one before the steps double

_refs = {}


def _tie_case(m):
    """planted_repeats(m, 20000) with the last column T in every row -- no row ends in A, so the all-zero key ('#', "A#",
    "AA#" ... share it) is carried by the separators alone, one group of the m '#' suffixes and the sentinel -- and the last
    two columns AT in the first half of the rows: a run "AT#" next to the run "T#"."""
    key = "tie%d" % m
    if key not in _refs:
        msa = planted_repeats(np.random.default_rng(1000 + m), m, 20000)
        msa[:, -1] = ord("T")
        msa[:(m + 1) // 2, -2] = ord("A")
        T, SA, ISA, LCP = O.msa_index(msa)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        _refs[key] = {"msa": msa, "f": O.compute_f(msa), "v": O.segment_v(msa), "SA": SA.astype(np.int64), "PL": lcp_ext[ISA],
                      "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    return _refs[key]


@pytest.mark.parametrize("m", [TIE_PROBE - 1, TIE_PROBE, TIE_PROBE + 1, 63, 64, 65, 300])
def test_tie_group_sizes_by_gallop_and_by_count(engine, m):
    """Tie groups of m members (and of m / 2, "AT#"; the rows' other ties are pairs and triples) around the length of the
    linear probe, around the 64 members above which a group goes to the list of big groups, and well above: f, v, the suffix
    array and both LCP arrays equal the oracle's with the group sizes found by galloping and by counting.
    The cap of 8192 members cannot be reached on the GPU below about 5 * 10^8 slots: a workgroup's candidate region overflows
    first (see test_scan_tail.test_wave_runs_index_equals_oracle).  The cap and the sizes around it are covered on the CPU
    (test_tie_extent.py)."""
    ref = _tie_case(m)
    for gallop in (1, 0):
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_TIE_GALLOP": str(gallop)}):
            assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), gallop
            print("m", m, "gallop", gallop, "index_kind", engine.get_option("index_kind"), "rank_lean_used", engine.get_option("rank_lean_used"))
            _check_index(engine, ref)
            assert np.array_equal(engine.repeatfree_v(ref["msa"]), ref["v"]), gallop


@pytest.mark.parametrize("name", ["planted", "300x40"])
def test_candidate_counts_and_key_sample_same_results(engine, name):
    """One kernel for the candidate counts or rocPRIM's scan and reduce, the sample of the sorted keys by a fixed grid or a
    workgroup per cluster: same f (the oracle's), a candidate list that ascends, the same scan taken and the same pairs
    counted.  (The planted input has 20 clusters: tie_sample_loop = 3 makes a workgroup walk seven of them.)"""
    ref = _case(name)
    seen = {}
    for fused in (1, 0):
        for loop in (1, 0, 3):
            with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_CAND_SORT_CHECK": "1", "FBG_CAND_COUNTS_FUSED": str(fused),
                                      "FBG_TIE_SAMPLE_LOOP": str(loop)}):
                assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), (fused, loop)
                assert engine.get_option("cand_inversions") == 0, (fused, loop)
                seen[fused, loop] = (engine.get_option("rank_lean_used"), engine.get_option("ext_pairs"), engine.get_option("text_pairs"),
                                     engine.get_option("index_kind"))
    print(name, "(fused, loop) -> (rank_lean_used, ext_pairs, text_pairs, index_kind):", seen)
    assert len(set(seen.values())) == 1, seen
    if name == "planted":
        assert seen[1, 1][0] == 1, seen
