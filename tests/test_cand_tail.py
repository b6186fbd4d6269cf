"""The tail of the rank-order scan worked by member (option cand_tail; rank_tail.hip: k_cand_region, k_cand_lcp, k_cand_runs,
k_cand_runs_long) against the oracle and against the kernels by head (cand_tail = 0), on inputs whose tie groups and same-column
runs are of every size the kernels tell apart and cross the regions of the scan's workgroups.

All inputs are 256 x 20000 (5 * 10^6 slots) with FBG_MSD_MIN = 1, so the lean scan runs: 4096 regions of 1392 slots.
  planted, plantedT256, plantedT200 (test_scan_tail.py): the row ends make one tie group of about 340 members on the all-zero key
    (k_tie_big) and runs "X#"; with the last column set to T in 256 / 200 rows one run "T#" of four chunks of 64 / of three and
    a part, and the '#' alone in that group.
  tiled: the same base; one 40-symbol stretch each copied into g rows at g different columns, g in GROUP_SIZES (tie groups of g
    members on a key of K symbols for each of the stretch's first 41 - K places; the symbol after a copy falls with the row
    number, so text order is not row order; the groups of 65 and 100 have more than 64 members with K real symbols: behind the lean
    scan k_tie_big ranks such a group whole, after the general scan it raises the fallback flag, test_scan_edges.py), and RUN_REPEATS stretches each copied into r rows at one column, r in RUN_SIZES (tied
    members that form a same-column run, below, at and above runs_wave_min = 16).
Before the GPU is used the classes are looked for on the CPU, from the oracle's suffix array: a class that is missing fails."""
import numpy as np
import pytest

from conftest import fbg_options
from oracle import pyoracle as O
from test_scan_tail import _case as _scan_case, _check_index
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

M, N_COLS = 256, 20000
GROUP_SIZES = (3, 4, 5, 9, 33, 64, 65, 100)
RUN_SIZES = (3, 15, 16, 17)
RUN_REPEATS = 12                    # 12 * (3 + 15 + 16 + 17) * 23 = 14 000 run members against regions of 1392 slots: ten crossings expected
STRETCH = 40
KEYS = (17, 18)                     # the key lengths of 2-bit symbols at this text length (asserted below)

_refs = {}
_classes = {}


def tiled_repeats():
    rng = np.random.default_rng(40)
    msa = planted_repeats(np.random.default_rng(2024), M, N_COLS)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)

    taken = np.zeros(msa.shape, dtype=bool)                    # cells of the copies so far, with a margin: no copy touches another

    def free(rows, cols):
        return not any(taken[r, c - STRETCH:c + 2 * STRETCH].any() for r, c in zip(rows, cols))

    def plant(rows, cols):
        stretch = A[rng.integers(0, 4, STRETCH)]
        for i, (r, c) in enumerate(zip(rows, cols)):
            msa[r, c:c + STRETCH] = stretch
            msa[r, c + STRETCH] = A[3 - i % 4]                 # T, G, C, A, T, ... down the rows: text order is not row order
            taken[r, c:c + STRETCH + 1] = True

    for g in GROUP_SIZES:
        rows = np.sort(rng.choice(M, g, replace=False))
        cols = rng.choice(np.arange(200, N_COLS - 200), g, replace=False)
        while not free(rows, cols):
            cols = rng.choice(np.arange(200, N_COLS - 200), g, replace=False)
        plant(rows, cols)
    for _ in range(RUN_REPEATS):
        for r in RUN_SIZES:
            rows = np.sort(rng.choice(M, r, replace=False))
            cols = [int(rng.integers(200, N_COLS - 200))] * r
            while not free(rows, cols):
                cols = [int(rng.integers(200, N_COLS - 200))] * r
            plant(rows, cols)
    return msa


def _case(name):
    if name != "tiled":
        return _scan_case(name)
    if name not in _refs:
        msa = tiled_repeats()
        T, SA, ISA, LCP = O.msa_index(msa)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        _refs[name] = {"msa": msa, "f": O.compute_f(msa), "v": O.segment_v(msa), "SA": SA.astype(np.int64), "PL": lcp_ext[ISA],
                       "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    return _refs[name]


def _run_lengths(v):
    """Starts and lengths of the maximal stretches of equal consecutive values."""
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    return starts, np.diff(np.concatenate([starts, [len(v)]]))


def region_slots(n_slots):
    """Slots of one workgroup of the lean scan (rank_scan.hip: rs_scan_launch's grid, rs_lean_setup's per_wave)."""
    blocks = min(-(-n_slots // 1024), 4096)
    per_wave = -(-(-(-n_slots // (blocks * 4))) // 58) * 58       # a wave's share, rounded up to whole rows of 58 slots
    return 4 * per_wave


def input_classes(name):
    """From the oracle's suffix array: the sizes of the tie groups on K symbols (K in KEYS; separators and what follows them in
    a key are blank, as in the compact keys), the lengths of the same-column runs, and whether a group and a run cross a multiple
    of the region length."""
    if name in _classes:
        return _classes[name]
    ref = _case(name)
    m, n = ref["msa"].shape
    SA = ref["SA"]
    N = len(SA)
    R = region_slots(N)
    p = np.arange(N, dtype=np.int64)
    rem = np.where(p == N - 1, 0, n - p % (n + 1))               # symbols left in the row; 0 for '#' and the sentinel
    code = np.zeros(256, dtype=np.uint64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    text = np.concatenate([np.concatenate([ref["msa"], np.full((m, 1), ord("#"), dtype=np.uint8)], axis=1).ravel(), np.zeros(1 + max(KEYS), dtype=np.uint8)])
    sym = code[text]
    out = {"region": R}
    key = np.zeros(N, dtype=np.uint64)
    for i in range(max(KEYS)):
        key = (key << np.uint64(2)) | np.where(i < rem, sym[i:i + N], np.uint64(0))
        if i + 1 in KEYS:
            starts, lens = _run_lengths(key[SA])
            out["groups", i + 1] = set(np.unique(lens).tolist())
            big = lens >= 2
            out["group_crosses", i + 1] = bool(np.any((starts[big] + lens[big] - 1) // R > starts[big] // R))
    col = np.where(rem == 0, -1 - p, n - rem)                    # ('#' and the sentinel: a column of their own each, never in a run)
    starts, lens = _run_lengths(col[SA])
    out["runs"] = set(np.unique(lens).tolist())
    big = lens >= 2
    out["run_crosses"] = bool(np.any((starts[big] + lens[big] - 1) // R > starts[big] // R))
    _classes[name] = out
    return out


def check_input(name):
    c = input_classes(name)
    assert c["region"] == 1392
    for K in KEYS:
        # the row ends on the all-zero key, k_tie_big: '#', "A#", "AA#" ..., 4/3 of the rows; where the rows end in T the '#' alone
        assert any(s > (64 if "T" in name else 300) for s in c["groups", K]), (name, K)
        assert c["group_crosses", K], (name, K)
        if name == "tiled":
            assert set(GROUP_SIZES) <= c["groups", K], (name, K, sorted(c["groups", K]))
    assert any(16 <= r for r in c["runs"]), name                                  # a run for k_cand_runs_long
    if name == "plantedT256":
        assert 256 in c["runs"]                                                   # four chunks of 64
    if name == "plantedT200":
        assert any(192 < r < 256 for r in c["runs"])                              # three chunks and a part (the 200 rows and those that ended in T before)
    if name == "tiled":
        assert set(RUN_SIZES) <= c["runs"], sorted(c["runs"])
        assert c["run_crosses"]


SETTINGS = {
    "tail": {},
    "by_head": {"FBG_CAND_TAIL": "0"},
    "cap1": {"FBG_WAVE_LIST_CAP": "1"},
    "min0": {"FBG_RUNS_WAVE_MIN": "0"},
    "min2": {"FBG_RUNS_WAVE_MIN": "2"},
    "lds_cap8": {"FBG_CAND_LDS_CAP": "8"},
    # the kernels by head behind the lean scan with the wave-list settings (with cand_tail = 1, the default, those above reach the
    # kernels by member only): k_runs' "list full, walk it yourself" branch, no list at all, and k_runs_long from two members on
    "by_head_cap1": {"FBG_CAND_TAIL": "0", "FBG_WAVE_LIST_CAP": "1"},
    "by_head_min0": {"FBG_CAND_TAIL": "0", "FBG_RUNS_WAVE_MIN": "0"},
    "by_head_min2": {"FBG_CAND_TAIL": "0", "FBG_RUNS_WAVE_MIN": "2"},
}
# the by_head_* settings on the two inputs that hold the run of three chunks and a part and the runs of 3, 15, 16 and 17 that cross regions
CASES = [(name, setting) for name in ("planted", "plantedT256", "plantedT200", "tiled") for setting in SETTINGS
         if not setting.startswith("by_head_") or name in ("plantedT200", "tiled")]


@pytest.mark.parametrize("name,setting", CASES, ids=[f"{name}-{setting}" for name, setting in CASES])
def test_tail_by_member_equals_oracle(engine, name, setting):
    """f, v, the suffix array and both neighbour LCPs equal the oracle's and the sorted candidate list ascends, with the tail by
    member and by head, with a wave list of one entry, with runs_wave_min 0 and 2 (each of the three by member and by head), and
    with the regions' LDS capacity forced to 8 entries (the kernels by head after the radix sort); a second build on the same
    engine gives the same arrays."""
    check_input(name)
    ref = _case(name)
    by_member = not setting.startswith("by_head") and setting != "lds_cap8"
    with fbg_options(engine, dict(SETTINGS[setting], FBG_MSD_MIN="1", FBG_CAND_SORT_CHECK="1")):
        for again in range(2 if setting == "tail" else 1):
            assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), again
            got = {k: engine.get_option(k) for k in ("rank_lean_used", "cand_tail_used", "cand_local_sorted", "cand_inversions", "wave_runs", "key_K")}
            print(name, setting, again, got)
            assert got["rank_lean_used"] == 1
            assert got["key_K"] in KEYS
            assert got["cand_tail_used"] == (1 if by_member else 0)
            assert got["cand_local_sorted"] == (0 if setting == "lds_cap8" else 1)
            assert got["cand_inversions"] == 0
            waves = setting.replace("by_head_", "")
            assert got["wave_runs"] == 0 if waves == "min0" else got["wave_runs"] == 1 if waves == "cap1" else got["wave_runs"] >= (4 if waves == "min2" else 1)
            _check_index(engine, ref)
        assert np.array_equal(engine.repeatfree_v(ref["msa"]), ref["v"])          # (its index is that of the reversed text)
        assert engine.get_option("rank_lean_used") == 1
        assert engine.get_option("cand_tail_used") == (1 if by_member else 0)
