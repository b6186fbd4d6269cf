"""The three segmentation DPs of csrc/dp.hip (dp_bytes.hip, dp_wide.hip) at their sentinels, tiers, tiles and rings.

fbg_repeatfree_dp takes its tier from the longest minimal block (R = 1 / 2 / 4 up to 31 / 63 / 126 columns, the one-lane
kernel above), stores a column's minimal block length in a byte whose 255 also says "no block ends here", and hands an
input over to the one-lane kernel when a value leaves the tier's window.  fbg_minmax_dp climbs a ladder of windows that
max_ext (the longest f[x] + 1 - x) chooses.  fbg_gapped_dp walks tiles of 64 columns in prefetch groups of 8 tiles and
looks back through a ring of the last 8192 values of s.  The backtracks are the lifted one (one table per power of two)
and the one-lane walk of the literal sweep.
The inputs below sit on each of those numbers and one beside them.  Every generator is a small deterministic function
(seeds in this file); its CPU test shows from the oracle alone that the input has the property its GPU test relies on,
every GPU check is exact equality with the oracle (oracle/pyoracle.py): s, prev, minmaxlength, backtrack, boundaries and
the "no segmentation" verdict.  What ran is read from the read-only options dp_kind, ne_dp_kind and dp_attempts."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import fbg_options
from oracle import pyoracle as O


SELFTEST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "founderblockgraphs_amd", "fbg_host_selftest")


def _same(got, want, what):
    assert np.array_equal(got, want), (what, np.flatnonzero(np.asarray(got) != np.asarray(want))[:5])


def _check_v(engine, dp, oracle_dp, v, what):
    s, prev, b = oracle_dp(v)
    gs, gprev, gb = dp(v)
    _same(gs, s, (what, "s"))
    _same(gprev, prev, (what, "prev"))
    assert (b is None) == (gb is None), (what, "verdict")
    if b is not None:
        _same(gb, b, (what, "boundaries"))
    return s, prev, b


def _check_f(engine, f, what):
    mml, bt, b = O.minmax_dp(f)
    gb, gmml, gbt = engine.minmax_dp(f, full=True)
    _same(gmml, mml, (what, "minmaxlength"))
    _same(gbt, bt, (what, "backtrack"))
    _same(gb, b, (what, "boundaries"))
    return mml, bt, b


# ---- 1. non-elastic DP ----------------------------------------------------------------------------------------------

def ne_tier_rule(longest):
    """fbg_dp_repeatfree (dp.hip): bound = 2 * hk[3] + 2; R = bound <= 64 ? 1 : bound <= 128 ? 2 : bound <= 254 ? 4 : 0, hk[3]
    the longest minimal block k_ne_prep found"""
    bound = 2 * longest + 2
    return 1 if bound <= 64 else 2 if bound <= 128 else 4 if bound <= 254 else 0


# longest minimal block -> ne_dp_kind, from the rule above: 2 * 32 + 2 = 66 and 2 * 64 + 2 = 130 are past the 64 and the 128
# of R = 1 and R = 2, so 32 and 64 are the first lengths of the next tier, as 127 (256 > 254) is the first of the one-lane kernel
NE_TIERS = {31: 1, 32: 2, 63: 2, 64: 4, 126: 4, 127: 0}


def ne_tier_sizes(longest):
    wn = 64 * (NE_TIERS[longest] or 4)          # the one-lane kernel has no window: the sizes of the widest tier
    return (wn - 1, wn, wn + 1, 4 * wn - 1, 4 * wn, 4 * wn + 1, 3000)   # the chain's groups are 4 blocks (Fg = 4)


def block_lengths(v):
    """minimal block length of every column that has a valid block (v[j] <= j), 0 for the others"""
    j = np.arange(len(v), dtype=np.int64)
    v = v.astype(np.int64)
    return np.where(v <= j, j + 1 - v, 0)


def ne_tier_v(longest, n, seed=0):
    """lengths drawn from 1 .. longest - 1, 5 % holes, and one column whose minimal block is exactly `longest`"""
    rng = np.random.default_rng([41, longest, n, seed])
    j = np.arange(n, dtype=np.int64)
    v = np.maximum(0, j + 1 - rng.integers(1, longest, n))
    v = np.where(rng.random(n) < 0.05, j + 1, v)
    p = longest - 1 + int(rng.integers(0, n - longest + 1))
    v[p] = p + 1 - longest
    return v.astype(np.uint64), p


@pytest.mark.parametrize("longest", sorted(NE_TIERS))
def test_ne_tier_inputs_have_their_longest_block_once(longest):
    assert NE_TIERS[longest] == ne_tier_rule(longest)
    for n in ne_tier_sizes(longest):
        v, p = ne_tier_v(longest, n)
        lens = block_lengths(v)
        assert lens.max() == longest and (lens == longest).sum() == 1 and lens[p] == longest
        s, _, _ = O.segment_dp(v)
        assert s[p] != p + 2 and s[p] >= longest       # the oracle gives the planted column a value: its block is used
        assert ne_kind_expected(v, s) == NE_TIERS[longest]   # and no value leaves the tier's window: no hand-over


@pytest.mark.gpu
@pytest.mark.parametrize("chain1", [0, 1])
@pytest.mark.parametrize("longest", sorted(NE_TIERS))
def test_ne_tier_boundaries(engine, longest, chain1):
    """Longest minimal block on both sides of every tier limit, n around one and four blocks of the tier's window; the
    tier that ran is the rule's (NE_TIERS; no input here has a value its window cannot hold, ne_kind_expected).
    dp_chain1: the same cases through the older one-wave chain."""
    with fbg_options(engine, {"dp_chain1": chain1}):
        for n in ne_tier_sizes(longest):
            v, _ = ne_tier_v(longest, n)
            _check_v(engine, engine.repeatfree_dp, O.segment_dp, v, (longest, n))
            assert engine.get_option("ne_dp_kind") == NE_TIERS[longest], (longest, n)


def ne_kind_expected(v, s):
    """What fbg_dp_repeatfree runs, from v and the oracle's s.  The tier by ne_tier_rule.  The matrix path looks at
    candidates of ages 1 .. WN = 64 R (k_dp_blockW: age_src <= WN) and keeps its values in bytes with 255 = none, so it is
    exact while every value is at most WN (below 255 for R = 4); k_ne_finish raises the flag at the first column that has
    a valid block but no such value (L >= DPB_INF), and the one-lane kernel redoes the input: 8."""
    lens = block_lengths(v)
    r = ne_tier_rule(int(lens.max())) if (lens < 255).all() else 0
    if r == 0:
        return 0
    valid = lens > 0
    limit = 64 * r if r < 4 else 254
    return 8 if (s[valid] > limit).any() else r


SENTINEL_LENGTHS = (254, 255, 256, 300)
SENTINEL_N = 2000


def ne_sentinel_v(where, length, seed=0):
    """lengths 1 .. 20 (tier R = 1) and a column whose minimal block is `length` columns: in the middle, at the first column
    that can end such a block (the block starts at column 0: the first block of the matrix grid that holds it), at the
    last column, or two of them"""
    n = SENTINEL_N
    rng = np.random.default_rng([42, length, seed])
    j = np.arange(n, dtype=np.int64)
    v = np.maximum(0, j + 1 - rng.integers(1, 21, n))
    cols = {"middle": [(1200, length)], "first": [(length - 1, length)], "last": [(n - 1, length)],
            "two": [(700, length), (1500, 300 if length != 300 else 255)]}[where]
    for p, k in cols:
        v[p] = p + 1 - k
    return v.astype(np.uint64), cols


@pytest.mark.parametrize("where", ["middle", "first", "last", "two"])
@pytest.mark.parametrize("length", SENTINEL_LENGTHS)
def test_ne_sentinel_inputs_have_a_value_at_the_long_block(where, length):
    v, cols = ne_sentinel_v(where, length)
    lens = block_lengths(v)
    assert sorted(lens[lens > 20]) == sorted(k for _, k in cols)
    s, prev, b = O.segment_dp(v)
    for p, k in cols:
        assert s[p] != p + 2 and s[p] == k and prev[p] <= p + 1 - k      # finite, and the long block decides it
    if where == "last":
        assert b is not None and b[-1] == SENTINEL_N - 1 and (len(b) == 1 or b[-2] <= SENTINEL_N - 1 - length)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["middle", "first", "last", "two"])
@pytest.mark.parametrize("length", SENTINEL_LENGTHS)
def test_ne_sentinel_255(engine, where, length):
    """A minimal block of 255 columns or more among short ones.  k_ne_prep keeps min(255, length) in a byte whose 255 also
    means "no valid block ends here".  Before this test the length that sizes the window left every 255 out, so such an
    input took the matrix path with R = 1, k_ne_finish answered s = j + 2, prev = j + 1 for the column without raising the
    flag, and with the block at the last column the library said "No proper segmentation exists." where the oracle has
    one.  Now a block of 255 or more counts as 255 there, beyond every tier (2 * 255 + 2 > 254), and the one-lane kernel
    runs: ne_dp_kind 0, as for 254 (2 * 254 + 2 > 254)."""
    v, _ = ne_sentinel_v(where, length)
    _check_v(engine, engine.repeatfree_dp, O.segment_dp, v, (where, length))
    assert engine.get_option("ne_dp_kind") == 0


HOLE_RUNS = {62: 1, 63: 1, 64: 8, 70: 8}      # run of holes -> ne_dp_kind: a run of h forces a block of h + 1 <= 64 = WN or not
HOLE_N = 1500


def ne_holes_v(run, where, seed=0):
    """lengths 1 .. 3 (R = 1, a window of 64 columns), non-monotone, and one run of `run` columns without a valid block
    (v[j] = j + 1): in the middle, from column 0, or up to the last column"""
    n = HOLE_N
    rng = np.random.default_rng([43, run, seed])
    j = np.arange(n, dtype=np.int64)
    v = np.maximum(0, j + 1 - rng.integers(1, 4, n))
    a = {"middle": 777, "start": 0, "end": n - run}[where]
    v[a:a + run] = j[a:a + run] + 1
    v[a + run:a + run + 4] = j[a + run:a + run + 4]      # one-column blocks behind the run: only the first of them has to span it
    return v.astype(np.uint64), a


@pytest.mark.parametrize("where", ["middle", "start", "end"])
@pytest.mark.parametrize("run", sorted(HOLE_RUNS))
def test_ne_hole_runs_force_a_block_across_them(run, where):
    v, a = ne_holes_v(run, where)
    assert (np.diff(v.astype(np.int64)) < 0).any()                      # non-monotone
    assert block_lengths(v).max() == 3
    s, prev, b = O.segment_dp(v)
    if where == "end":
        assert b is None and ne_kind_expected(v, s) == 1               # nothing behind the run: no value, no flag
        return
    behind = a + run
    assert s[behind] == run + 1 and prev[behind] == a                  # the block over the run, as long as the run + 1
    assert (s[behind] > 64) == (run >= 64)
    assert ne_kind_expected(v, s) == HOLE_RUNS[run]
    assert b is not None


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["middle", "start", "end"])
@pytest.mark.parametrize("run", sorted(HOLE_RUNS))
def test_ne_handover(engine, run, where):
    """A run of h holes forces a block of h + 1 columns behind it.  With R = 1 the matrix path looks at ages 1 .. 64
    (k_dp_blockW: age_src <= WN; k_ne_finish: a <= min(window, jp)), so runs of 62 and 63 (blocks of 63 and 64) stay on it,
    ne_dp_kind 1, and runs of 64 and 70 leave the column behind them without a value: flag, one-lane kernel, 8.  A run up
    to the last column has nothing behind it: no flag, 1, and the verdict "no proper segmentation"."""
    v, _ = ne_holes_v(run, where)
    _check_v(engine, engine.repeatfree_dp, O.segment_dp, v, (run, where))
    assert engine.get_option("ne_dp_kind") == (1 if where == "end" else HOLE_RUNS[run])


# ---- 2. elastic sweep -------------------------------------------------------------------------------------------------

# an extension of E is max_ext = E + 1 to k_dp_keys.  The second row puts max_ext on the limits of DP_LADDER that the first misses:
# 62, 126, 1022, 2046 | 2047, 4094, 8190 | 8191
OUTLIERS = (31, 32, 62, 63, 126, 127, 254, 255, 510, 511, 1022, 1023, 4094, 4095, 16381, 16382, 16383, 16384,
            61, 125, 1021, 2045, 2046, 8189, 8190, 4093)
PLACES = ("x1", "block_last", "block_first", "exact_end", "clipped")
# seed of the base extensions per (place, outlier): the first one with which the base segmentation has a block starting at
# the outlier's column, so that the long extension changes the boundaries (test_outlier_changes_the_boundaries)
OUTLIER_SEEDS = {(place, E): seed for place, seeds in (
    ("x1", (0,) * 26), ("block_last", (2,) * 26), ("block_first", (1,) * 26),
    ("exact_end", (6, 0, 2, 0, 1, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0)),
    ("clipped", (1, 0, 0, 2, 2, 1, 0, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0))) for E, seed in zip(OUTLIERS, seeds)}
assert len(OUTLIER_SEEDS) == 5 * len(OUTLIERS)


def outlier_f(E, place, seed=None):
    """base extensions 0 .. 2, f[0] = 0, and one column with extension E -> (base f, f, the column)"""
    n = max(3000, E + 2000)
    seed = OUTLIER_SEEDS.get((place, E), 0) if seed is None else seed
    rng = np.random.default_rng([44, seed])
    x = np.arange(n, dtype=np.int64)
    base = np.minimum(x + rng.integers(0, 3, n), n - 1)
    base[0] = 0
    col = {"x1": 1, "block_last": 10 * 128 - 1, "block_first": 10 * 128, "exact_end": n - 1 - E, "clipped": n - 1 - E + 7}[place]
    f = base.copy()
    f[col] = min(col + E, n - 1)
    return base.astype(np.uint64), f.astype(np.uint64), col


# fbg_dp_minmax (dp.hip) for f[0] = 0, n >= 2 * DPW_B = 256, default options, by max_ext = the longest f[x] + 1 - x (k_dp_keys):
#   bound = 2 max_ext + 2; R = bound <= 64 ? 1 : <= 128 ? 2 : <= 254 ? 4 : <= 512 ? 8 : <= 1024 ? 16 : 0
#   R != 0 (max_ext <= 511): the byte matrices first, Rt = the smallest of 1, 2, 4 with 64 Rt >= max_ext + 2 (4 beyond) -> dp_kind 1
#   R == 0 and max_ext + 2 <= 16384 (dp_wide_ok, dp_plan.h): the wide rungs, WS = the smallest of 1024 .. 16384 that is >= max_ext + 2 -> dp_kind 3 .. 7
#   else the literal sweep -> dp_kind 0
# each rung settles when no value reaches its limit (k_dp_expand: acc >= 64 R, 255 for R = 4; k_dpw_chain2: v >= WS)
#             (max_ext from, to, dp_kind, the first rung's limit)
DP_LADDER = ((0, 62, 1, 64), (63, 126, 1, 128), (127, 511, 1, 255), (512, 1022, 3, 1024), (1023, 2046, 4, 2048), (2047, 4094, 5, 4096),
             (4095, 8190, 6, 8192), (8191, 16382, 7, 16384), (16383, 1 << 40, 0, None))


def ladder_kind(max_ext):
    return next(kind for lo, hi, kind, _ in DP_LADDER if lo <= max_ext <= hi)


def ladder(f):
    """-> (dp_kind, the first rung's limit) for an f whose entries are all below n"""
    fx = f.astype(np.int64)
    max_ext = int((fx + 1 - np.arange(len(f)))[fx < len(f)].max())     # a column with f = n starts no block and does not count
    return next((kind, limit) for lo, hi, kind, limit in DP_LADDER if lo <= max_ext <= hi)


def test_outliers_sit_on_both_sides_of_every_ladder_limit():
    seen = {int((outlier_f(E, "x1")[1].astype(np.int64) + 1 - np.arange(max(3000, E + 2000))).max()) for E in OUTLIERS}
    for lo, _, _, _ in DP_LADDER[1:]:
        assert lo in seen and lo - 1 in seen, lo


def test_ladder_table_matches_the_rule():
    for lo, hi, kind, limit in DP_LADDER:
        for m in (lo, hi):
            bound = 2 * m + 2
            R = 1 if bound <= 64 else 2 if bound <= 128 else 4 if bound <= 254 else 8 if bound <= 512 else 16 if bound <= 1024 else 0
            if R:
                rt = 1
                while 64 * rt < m + 2 and rt < 4:
                    rt *= 2
                assert kind == 1 and limit == (255 if rt == 4 else 64 * rt), (m, rt)
            elif m + 2 <= 16384:
                ws = 1024
                while ws < m + 2:
                    ws *= 2
                assert kind == 3 + (ws // 1024).bit_length() - 1 and limit == ws, (m, ws)
            else:
                assert kind == 0
    assert all(a[1] + 1 == b[0] for a, b in zip(DP_LADDER, DP_LADDER[1:]))


@pytest.mark.parametrize("place", PLACES)
def test_outlier_changes_the_boundaries(place):
    for E in OUTLIERS:
        base, f, col = outlier_f(E, place)
        n = len(f)
        assert f[0] == 0 and (base.astype(np.int64) - np.arange(n) <= 2).all() and np.flatnonzero(f != base).tolist() == [col]
        reach = col + E
        assert {"x1": col == 1, "block_last": col % 128 == 127, "block_first": col % 128 == 0, "exact_end": reach == n - 1,
                "clipped": reach > n - 1}[place] and (place == "clipped" or reach <= n - 1)
        assert not np.array_equal(O.minmax_dp(base)[2], O.minmax_dp(f)[2]), (place, E)


@pytest.mark.gpu
@pytest.mark.parametrize("place", PLACES)
def test_single_outlier(engine, place, capsys):
    """One long extension among extensions of 0 .. 2, at column 1, on both sides of a 128-column block edge, reaching exactly
    the last column and clipped to it.  dp_kind is the ladder's for the input's max_ext (DP_LADDER), and the first rung
    settles (dp_attempts 1) wherever the oracle's largest minmaxlength is below that rung's limit."""
    seen = []
    for E in OUTLIERS:
        _, f, _ = outlier_f(E, place)
        mml, _, _ = _check_f(engine, f, (place, E))
        kind, limit = ladder(f)
        attempts = engine.get_option("dp_attempts")
        seen.append((E, engine.get_option("dp_kind"), attempts))
        assert engine.get_option("dp_kind") == kind, (place, E, seen[-1])
        assert attempts >= 1
        if limit is None or int(mml.max()) < limit:
            assert attempts == 1, (place, E, attempts)
    with capsys.disabled():
        print(f"\n  {place}: (E, dp_kind, dp_attempts) {seen}")


# (outlier, columns that cannot start a block, the first rung's limit, the next rung's, dp_kind, dp_attempts): the rungs that widen
#   max_ext 3: R = 1, one rung of 64, then neither matrices nor wave sweep are left: the literal sweep
#   max_ext 40: R = 2, rungs of 64 and 128;  max_ext 101: R = 4, rungs of 128 and 256 (values below 255)
#   max_ext 601: R = 0, the wide rungs WS = 1024, then 2048 (dp_kind 4)
WIDENING = ((2, 70, 64, None, 0, 2), (39, 70, 64, 128, 1, 2), (100, 130, 128, 255, 1, 2), (600, 1100, 1024, 2048, 4, 2))


def widening_f(E, run, seed=0):
    """Extensions 0 .. 2, one of E (it sets max_ext = E + 1 and with it the first rung), and `run` columns that cannot start
    a block at all (f = n, a row out of symbols -- only without the elastic tricks): the block over them is run + 1 columns
    long, more than the first rung's window holds."""
    n = 4000
    rng = np.random.default_rng([49, E, seed])
    x = np.arange(n, dtype=np.int64)
    f = np.minimum(x + rng.integers(0, 3, n), n - 1)
    f[0] = 0
    f[500] = 500 + E
    f[2000] = 2000
    f[2001:2001 + run] = n
    return f.astype(np.uint64)


def test_widening_inputs_exceed_the_first_rung_only():
    for E, run, first, second, _, _ in WIDENING:
        f = widening_f(E, run)
        assert ladder(f)[1] == first
        mml, _, b = O.minmax_dp(f)
        assert first <= run + 1 <= int(mml.max()) and (second is None or int(mml.max()) < second) and b[-1] == len(f)


@pytest.mark.gpu
def test_widening_rungs(engine):
    """A value that reaches the first rung's limit: the sweep widens once and settles (dp_attempts 2, dp_kind of the rung that
    settled), or, with no rung left, the literal sweep redoes the input (dp_kind 0)."""
    for E, run, _, _, kind, attempts in WIDENING:
        _check_f(engine, widening_f(E, run), (E, run))
        assert (engine.get_option("dp_kind"), engine.get_option("dp_attempts")) == (kind, attempts), (E, run)


# Sequences the ladder (csrc/dp_plan.h) has beyond those above, n = 4000, one launch each:
#   (E, run, options, the oracle's largest minmaxlength lies in [lo, hi), the plan for this input, (dp_kind, dp_attempts))
#   max_ext 151, R = 8: the byte rung of 4 flags the block over the run (301 >= 255), no wide rung (151 + 2 <= 256), the wave sweep
#   max_ext 301, R = 16: the byte rung of 4, then WIDE(1024)
#   the first input under dp_wave: the wave sweep alone;  max_ext 151 without a run under dp_safe_window: Rt starts at R = 8,
#   above the byte matrices, so no byte rung: the wave sweep
# The pairs are what the commit before the ladder became a plan reported for these inputs on an MI355X (the tests were run
# once on its library: profiles/dp_ladder_summary.txt, section 2); each is also the dp_kind of a rung of the plan and that rung's
# position in it.
LADDER_SEQUENCES = (
    (150, 300, {}, (255, 512), ("B4", "V8", "L"), (2, 2)),
    (300, 300, {}, (255, 1024), ("B4", "W1024", "W2048", "W4096", "W8192", "W16384", "V16", "L"), (3, 2)),
    (150, 300, {"dp_wave": 1}, (255, 512), ("V8", "L"), (2, 1)),
    (150, 0, {"dp_safe_window": 1}, (0, 512), ("V8", "L"), (2, 1)))
RUNG_KIND = {"B": lambda size: 1, "W": lambda size: 3 + (size // 1024).bit_length() - 1, "V": lambda size: 2, "L": lambda size: 0}


@pytest.mark.parametrize("case", range(len(LADDER_SEQUENCES)))
def test_ladder_sequence_inputs_settle_where_the_case_needs(case):
    E, run, options, (lo, hi), plan, (kind, attempts) = LADDER_SEQUENCES[case]
    f = widening_f(E, run)
    assert len(f) == 4000 and f[0] == 0
    fx = f.astype(np.int64)
    assert int((fx + 1 - np.arange(len(f)))[fx < len(f)].max()) == E + 1
    mml, _, b = O.minmax_dp(f)
    assert lo <= int(mml.max()) < hi and b[-1] == len(f)
    rung = plan[attempts - 1]                                   # the pair names a rung of the plan: its kind, its position
    assert RUNG_KIND[rung[0]](int(rung[1:] or 0)) == kind
    line = f"{E + 1} 0 4000 0 {options.get('dp_wave', 0)} {options.get('dp_safe_window', 0)} 0\n"
    r = subprocess.run([SELFTEST, "dp_plan"], input=line, capture_output=True, text=True)      # ... of dp_plan.h's plan
    assert r.returncode == 0 and tuple(w.split(":")[0] for w in r.stdout.split()) == plan, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LADDER_SEQUENCES)))
def test_ladder_sequences(engine, case, capsys):
    E, run, options, _, _, want = LADDER_SEQUENCES[case]
    with fbg_options(engine, options):
        _check_f(engine, widening_f(E, run), (E, run, options))
        got = (engine.get_option("dp_kind"), engine.get_option("dp_attempts"))
    with capsys.disabled():
        print(f"\n  ladder sequence {case}: (dp_kind, dp_attempts) {got}")
    assert got == want, (E, run, options)


def random_f(rng, n, max_ext, style):
    """the three styles of test_gpu_parity.test_dp_sweep_random_f"""
    x = np.arange(n, dtype=np.int64)
    if style == "uniform" or n < 4:
        ext = rng.integers(0, max_ext + 1, n)
    elif style == "plateau":
        ends = np.sort(rng.choice(np.arange(1, n), size=max(1, n // max(2, max_ext)), replace=False))
        ext = np.clip(ends[np.minimum(np.searchsorted(ends, x, side="left"), len(ends) - 1)] - x, 0, max_ext)
    else:
        ext = np.where(rng.random(n) < 0.03, rng.integers(0, max_ext + 1, n), rng.integers(0, 3, n))
    f = np.minimum(x + ext, n - 1)
    f[0] = 0
    return f.astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("max_ext", [5, 40, 100])
@pytest.mark.parametrize("style", ["uniform", "plateau", "spiky"])
def test_dp_safe_window(engine, max_ext, style):
    """dp_safe_window = 1 starts the byte matrices at the window that is provably enough (Rt = R, fbg_dp_minmax): one
    attempt, dp_kind 1."""
    rng = np.random.default_rng([45, max_ext, len(style)])
    with fbg_options(engine, {"dp_safe_window": 1}):
        for n in (1, 2, 63, 64, 65, 1000, 5000):
            _check_f(engine, random_f(rng, n, max_ext, style), (n, max_ext, style))
            assert engine.get_option("dp_kind") == 1 and engine.get_option("dp_attempts") == 1


@pytest.mark.gpu
def test_minmax_refuses_f_outside_its_range(engine):
    """f[x] < x and f[x] > n: FBG_ERR_INVALID with the count of such entries (k_dp_keys, hk[2]); the engine is unharmed."""
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    rng = np.random.default_rng(46)
    n = 700
    good = random_f(rng, n, 9, "uniform")
    for x, value in ((300, 299), (300, n + 1)):
        bad = good.copy()
        bad[x] = value
        with pytest.raises(F.FbgError, match=r"f\[\] has 1 entries outside \[x, n\]") as err:
            engine.minmax_dp(bad)
        assert err.value.code == _lib.FBG_ERR_INVALID and not isinstance(err.value, F.NoSegmentation)
        assert engine.get_option("dp_attempts") == 0
        _check_f(engine, good, ("after the refusal", x, value))


# ---- 3. gapped walk -----------------------------------------------------------------------------------------------------

GD_N = 17_500                                   # the ring of 8192 values wraps twice
GD_RING = 8192
GD_T0 = (8192 + 64, 8192 + 512, 16384 + 128)    # tile starts: second tile of a group, first tile of a group, third tile
GD_DIST = (1, 8191, 8192, 8193, 0)              # t0 - look: newest ring entry, oldest but one, oldest, first from memory, inside the tile
GD_GROUP_N = (511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)


def gapped_base(n):
    """short blocks whose lengths follow a slow sawtooth: 2 .. 7 columns, a step every 37 columns"""
    j = np.arange(n, dtype=np.int64)
    v = np.maximum(0, j + 1 - (2 + (j // 37) % 6))
    v[0] = 0
    return v


def gapped_planted(t0, lane, dist):
    """The base with column j = t0 + lane looking back at look = t0 - dist (v[j] = look + 1), alone in its array.
    s[c] <= c + 1 for every column that has a value, so a lookback can decide s[j] = max(s[look], j - look) through a finite
    value only where look + 1 > j - look.  There ("first") the columns look - 1, look, look + 1 and look + 8192 (where
    they lie in front of j) get v = 0: s[c] = c + 1, all different and all above j - look.  Elsewhere ("hole") the column look
    has no block, s[look] = n + 1, and the others get v = 0: four different values again, and s[j] = n + 1 where any other
    slot gives j - look.  Where look + 8192 is j - 1 that column has to be a hole for the event at j to fire, so the roles
    are swapped ("swap"): s[look] finite, the three others n + 1.  Column j - 1 is a hole wherever it is not one of these
    columns: the walk arrives at j without a block to extend, and the event fires.
    -> (v, j, look, the other columns, the mode); None for lane 0 and dist 0, where look is j itself: v[j] = j + 1 is
    the hole at lane 0 of gapped_others"""
    n = GD_N
    j, look = t0 + lane, t0 - dist
    if look >= j:
        return None
    v = gapped_base(n)
    others = [look - 1] + [c for c in (look + 1, look + GD_RING) if c < j]
    if look > j - look:
        mode = "first"
        v[[look] + others] = 0
    elif look + GD_RING == j - 1:
        mode = "swap"
        v[look] = 0
        for c in others:
            v[c] = c + 1
    else:
        mode = "hole"
        v[look] = look + 1
        v[others] = 0
    if j - 1 not in [look] + others:
        v[j - 1] = j
    v[j] = look + 1
    return v.astype(np.uint64), j, look, others, mode


def _gapped_cases(t0):
    return [(lane, dist, gapped_planted(t0, lane, dist)) for lane in (0, 63) for dist in GD_DIST if gapped_planted(t0, lane, dist)]


@pytest.mark.parametrize("t0", GD_T0)
def test_gapped_planted_lookbacks_decide_their_column(t0):
    assert t0 % 64 == 0 and GD_N > 2 * GD_RING + 64
    cases = _gapped_cases(t0)
    assert len(cases) == 9
    for lane, dist, (v, j, look, others, mode) in cases:
        s, prev, _ = O.segment2_dp(v)
        s = s.astype(np.int64)
        assert j % 64 == lane and j - lane - look == dist and v[j] == look + 1
        assert prev[j] == v[j], (t0, lane, dist)                                        # the event fires
        assert s[j] == max(s[look], j - look)
        cols = [look] + others
        assert (look + GD_RING in others) == (look + GD_RING < j)
        for c in others:                                                                # any other slot gives another s[j]
            assert max(s[c], j - look) != s[j], (t0, lane, dist, c)
        vals = [int(s[c]) for c in cols]
        if mode == "swap":
            # lane 0, look = t0 - 8193 at the two smaller tile starts: s[look] <= look + 1 < j - look, so only n + 1 can
            # differ from it in s[j], and column j - 1 = look + 8192 has to be n + 1 for the event to fire
            assert lane == 0 and dist == 8193 and t0 < 2 * GD_RING and all(x == GD_N + 1 for x in vals[1:]) and vals[0] == look + 1
        else:
            assert len(set(vals)) == len(vals), (t0, lane, dist, vals)                  # pairwise different
        assert mode == ("first" if look > j - look else mode)


@pytest.mark.gpu
@pytest.mark.parametrize("t0", GD_T0)
def test_gapped_ring_edges(engine, t0):
    """A lookback from lane 0 and from lane 63 of the tile at t0 to the newest ring entry (t0 - 1), the oldest but one, the
    oldest (t0 - 8192: k_dp_gapped tests t0 - look <= GD_RING from the tile start), the first column fetched from memory
    (t0 - 8193) and a column of the tile itself (from lane 63)."""
    for lane, dist, (v, j, _, _, _) in _gapped_cases(t0):
        _check_v(engine, engine.gapped_dp, O.segment2_dp, v, (t0, lane, dist))


def gapped_others(kind):
    """-> (v, the tile start) of the further cases on the base input"""
    n, t0 = 2000, 1024
    v = gapped_base(n)
    if kind == "all_fire":
        # the 64 columns before the tile take v = 0: s = t0 - 63 .. t0; lane k looks back at column t0 - 1 - k, 2k + 1 columns:
        # a = t0 - k falls from lane to lane and stays below the b the lane before left
        v[t0 - 64:t0] = 0
        k = np.arange(64)
        v[t0 + k] = t0 - k
    elif kind == "none_fire":
        v[t0 - 2] = t0 - 1                      # a hole, so that column t0 - 1 takes its own block [t0 - 5 .. t0 - 1]
        v[t0 - 1:t0 + 64] = t0 - 5              # and every column of the tile can only extend it
    elif kind == "hole_lane0":
        v[t0] = t0 + 1
    elif kind == "hole_lane63":
        v[t0 + 63] = t0 + 64
    elif kind == "v0_is_1":
        v[0] = 1
    else:
        assert kind == "v0_is_0"
    return v.astype(np.uint64), t0


GD_OTHERS = ("all_fire", "none_fire", "hole_lane0", "hole_lane63", "v0_is_0", "v0_is_1")


def test_gapped_other_inputs_have_their_events():
    tile = np.arange(64)
    v, t0 = gapped_others("all_fire")
    s, prev, b = O.segment2_dp(v)
    assert np.array_equal(prev[t0 + tile], v[t0 + tile]) and len(set(prev[t0 + tile].tolist())) == 64 and b is not None
    assert np.array_equal(s[t0 + tile].astype(np.int64), t0 - tile)
    v, t0 = gapped_others("none_fire")
    s, prev, _ = O.segment2_dp(v)
    assert (v[t0 + tile] <= t0 + tile).all() and (prev[t0 - 1:t0 + 64] == t0 - 5).all() and len(set(s[t0 + tile].tolist())) > 32
    for kind, col in (("hole_lane0", 1024), ("hole_lane63", 1087)):
        v, t0 = gapped_others(kind)
        s, prev, b = O.segment2_dp(v)
        assert col == t0 + (0 if kind == "hole_lane0" else 63) and s[col] == len(v) + 1 and prev[col] == len(v) + 1 and b is not None
        assert prev[col + 1] == v[col + 1]      # the column behind the hole has nothing to extend
    a, b = (O.segment2_dp(gapped_others(k)[0]) for k in ("v0_is_0", "v0_is_1"))
    assert a[0][0] == 2001 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for n in GD_GROUP_N:                        # neighbouring values of the base differ somewhere in every group's last tile
        s, _, b = O.segment2_dp(gapped_base(n).astype(np.uint64))
        assert b is not None and b[-1] == n - 1


@pytest.mark.gpu
def test_gapped_tiles_groups_and_column_0(engine):
    """n on both sides of one, two and eight prefetch groups of 512 columns (k_dp_gapped fetches the next group when
    g0 + 512 < n), a tile in which all 64 columns take a new block, one in which none does, a hole at lane 0 and at lane 63,
    and v[0] = 0 / 1: the walk starts at column 1 (fbg.cpp:830)."""
    for n in GD_GROUP_N:
        _check_v(engine, engine.gapped_dp, O.segment2_dp, gapped_base(n).astype(np.uint64), n)
    for kind in GD_OTHERS:
        _check_v(engine, engine.gapped_dp, O.segment2_dp, gapped_others(kind)[0], kind)


# ---- 4. backtracks ------------------------------------------------------------------------------------------------------

LIFTED_N = (127, 128, 129, 4095, 4096, 4097, 65_535, 65_536, 65_537)


@functools.lru_cache(maxsize=None)
def lifted_case(n):
    """f with extensions 0 .. 2, v with blocks of 1 .. 3 columns, and the oracle's answers to the three DPs (made once)"""
    rng = np.random.default_rng([47, n])
    x = np.arange(n, dtype=np.int64)
    f = np.minimum(x + rng.integers(0, 3, n), n - 1)
    f[0] = 0
    v = np.maximum(0, x + 1 - rng.integers(1, 4, n))
    f, v = f.astype(np.uint64), v.astype(np.uint64)
    return f, v, O.minmax_dp(f), O.segment_dp(v), O.segment2_dp(v)


def lifted_levels(n):
    """fbg_backtrack_lifted: levels = 1; while ((1 << (levels - 1)) <= n) levels++"""
    return n.bit_length() + 1


def test_lifted_sizes_sit_on_the_table_counts():
    assert [lifted_levels(n) for n in LIFTED_N] == [8, 9, 9, 13, 14, 14, 17, 18, 18]
    for n in (127, 128, 129):
        _, _, (_, _, b), (_, _, b1), (_, _, b2) = lifted_case(n)
        assert len(b) > n // 4 and b1 is not None and len(b1) > n // 4 and b2 is not None and len(b2) > n // 8   # many hops to lift


@pytest.mark.gpu
@pytest.mark.parametrize("n", LIFTED_N)
def test_lifted_backtrack_at_powers_of_two(engine, n):
    """fbg_backtrack_lifted keeps one table per power of two up to n; n around 2^7, 2^12 and 2^16, behind all three DPs."""
    f, v, (mml, bt, b), ne, gd = lifted_case(n)
    gb, gmml, gbt = engine.minmax_dp(f, full=True)
    _same(gmml, mml, "minmaxlength"), _same(gbt, bt, "backtrack"), _same(gb, b, "boundaries")
    assert engine.get_option("dp_kind") == 1                    # max_ext <= 3: byte matrices, lifted backtrack
    for dp, want in ((engine.repeatfree_dp, ne), (engine.gapped_dp, gd)):
        gs, gprev, gb = dp(v)
        _same(gs, want[0], "s"), _same(gprev, want[1], "prev")
        assert gb is not None and want[2] is not None
        _same(gb, want[2], "boundaries")
    assert engine.get_option("ne_dp_kind") == 1                 # blocks of up to 3 columns: R = 1, lifted backtrack


WALK_N = 20_000
WALK_HOPS = (8191, 8192, 8193, 9001)


def walk_f(hop, seed=0):
    """Extensions 0 .. 2 up to column p = n - hop, where one block can only run to the end (f[p] = n - 1: an extension of
    hop - 1, 9000 for the longest) and behind which no column can start a block at all (f = n, a row out of symbols): the last
    block is [p, n), the first hop of the backtrack is `hop` columns long and lands on column p.  (In this recurrence nothing
    forces a cut except columns that cannot start a block.)"""
    n = WALK_N
    rng = np.random.default_rng([48, seed])
    x = np.arange(n, dtype=np.int64)
    f = np.minimum(x + rng.integers(0, 3, n), n - 1)
    f[0] = 0
    p = n - hop
    f[p - 3:p] = x[p - 3:p]
    f[p] = n - 1
    f[p + 1:] = n
    return f.astype(np.uint64), p


@pytest.mark.parametrize("hop", WALK_HOPS)
def test_walk_inputs_hop_over_the_window(hop):
    f, p = walk_f(hop)
    mml, bt, b = O.minmax_dp(f)
    assert bt[WALK_N] == p and mml[WALK_N] == hop and b[-1] == WALK_N and b[-2] == p - 1 and len(b) > 1000
    fx = f.astype(np.int64)
    assert int((fx + 1 - np.arange(WALK_N))[fx < WALK_N].max()) == hop and ladder_kind(hop) == 7


@pytest.mark.gpu
@pytest.mark.parametrize("hop", WALK_HOPS)
def test_one_lane_backtrack_long_hops(engine, hop):
    """The literal sweep and its one-lane backtrack (k_dp_minmax, k_dp_backtrack: dp_kind 0) on a first hop of 8191, 8192,
    8193 and 9001 columns -- the edges of, and a hop across, an 8192-column window ending at n, which is what the LDS
    window of k_dp_backtrack_wave would hold; today's k_dp_backtrack reads backtrack[] from memory hop by hop -- then many
    short hops; against the oracle and against the same input on the default path (16-bit matrices, lifted backtrack)."""
    f, _ = walk_f(hop)
    with fbg_options(engine, {"FBG_DP_LITERAL": "1"}):
        mml, bt, b = _check_f(engine, f, ("literal", hop))
        assert engine.get_option("dp_kind") == 0 and engine.get_option("dp_attempts") == 1
    gb, gmml, gbt = engine.minmax_dp(f, full=True)
    _same(gmml, mml, "minmaxlength"), _same(gbt, bt, "backtrack"), _same(gb, b, "boundaries")
    assert engine.get_option("dp_kind") == 7 and engine.get_option("dp_attempts") == 1     # max_ext = hop: the 16384 window
