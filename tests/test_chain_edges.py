"""The chaining kernels of csrc/pindex_chain.hip (k_pc_key, pc_read in its three tiers of k_pc_chain, k_pc_trace) and the host
code of fbg_pindex_chains on the branches that tests/test_chains.py does not provably reach: both signs of the surplus on
either side of the band, places without a column inside reads of the wave and spill tiers, workgroups of the small tier
one read short of full, full and one read over, many workgroups of the large tiers, min_score at a read's score and
beyond 32 bits, buffers that outlive a call, and seeds that give a chain no anchor.

Every input is a function of this file alone (`cases`).  HostModel computes the seeds of an input from the Python models
(occ_model, seeds_model, msa_model); the GPU tests check that PatternIndex.seeds() returns exactly those arrays, so the
class counters that test_inputs_reach_their_classes_in_the_models asserts without a GPU are counters of what the kernels
see.  Every comparison with chain_model is exact, on chain_off, score, anchor_place and anchor_seed, and every GPU test
ends with counters taken from the seeds and the model, never from the kernels' answer."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import chain_model as CM  # noqa: E402
import msa_model as MM  # noqa: E402
import test_seeds as TS  # noqa: E402
from conftest import random_msa  # noqa: E402
from test_chains import UNIT, build, model_inputs, per_read, same, tier_msa  # noqa: E402

NONE = CM.NONE
SURPLUS = (1, 2, 3, 4)              # |surplus| of the junctions: B and B + 1 for B in BANDS_AT
BANDS_AT = (1, 3)                   # the chain under band B differs from the one under B - 1 (B = 1: band 0 against 1)
TIERS = ("small", "wave", "spill")


def source_constants():
    """PX_THREADS, PC_SUB, PC_SMALL and PC_LDS of csrc/pindex.h."""
    text = open(os.path.join(ROOT, "founderblockgraphs_amd", "csrc", "pindex.h")).read()
    return {k: int(re.search(r"^#define %s (\d+)\b" % k, text, re.M).group(1)) for k in ("PX_THREADS", "PC_SUB", "PC_SMALL", "PC_LDS")}


K = source_constants()
SM_MAX, LDS_MAX = K["PC_SMALL"], K["PC_LDS"]
GROUP = K["PX_THREADS"] // K["PC_SUB"]          # reads of the small tier that one workgroup chains


def small_msa():
    """3 rows of 6 copies of the unit of tier_msa, row 2 with one substitution, 3 blocks: a rotation of the unit has 8 to
    11 start places, and the 12-mers of row 2 across its substitution have one."""
    row = np.frombuffer(UNIT * 6, dtype=np.uint8)
    A = np.stack([row, row, row]).copy()
    A[2, 60] = ord("C")
    return A, [20, 47, len(row)]


def rot(r):
    r %= len(UNIT)
    return UNIT[r:] + UNIT[:r]


def junction_read(r0, surplus):
    """Rotations of the unit, one seed each; between two of them the read and the columns advance by amounts that differ
    by `surplus[i]`: 0 is one substituted symbol, s > 0 a substituted symbol and s row symbols left out (a deletion in
    the read), s < 0 a run of -s symbols the MSA does not hold between two adjacent pieces of the row (an insertion)."""
    out, r = [rot(r0)], r0
    for s in surplus:
        if s >= 0:
            out.append(b"T")
            r += 13 + s
        else:
            out.append(b"T" * -s)
            r += 12
        out.append(rot(r))
    return b"".join(out) + b"T"


class HostModel:
    """The Python models of one MSA and segmentation.  seeds() -> the five arrays model_inputs() takes from a Seeds."""

    def __init__(self, A, b):
        self.A, self.b = A, [int(x) for x in b]
        self.mm = MM.Model(A, self.b)
        self.sm = TS.Model(self.mm.labels, self.mm.edges)
        self._seeds = {}

    def seeds(self, reads, L, cap):
        key = (tuple(reads), L, cap)
        if key not in self._seeds:
            e = self.sm.expected(reads, L, cap)
            col = self.mm.coords(e["start_src"], e["start_dst"], e["start_offset"])[1]
            self._seeds[key] = (np.array(e["seed_off"], dtype=np.uint64), np.array(e["q_start"], dtype=np.uint32),
                                np.array(e["length"], dtype=np.uint32), np.array(e["start_off"], dtype=np.uint64), col.astype(np.uint32))
        return self._seeds[key]

    def edge_strings(self):
        return [self.mm.labels[u] + self.mm.labels[v] for u, v in self.mm.edges]


_HOSTS = {}


def host(name):
    if name not in _HOSTS:
        _HOSTS[name] = HostModel(*(tier_msa() if name == "tier" else small_msa()))
    return _HOSTS[name]


def one_place_pieces(h):
    """The 12-mers of row 2 of small_msa that hold its substitution and have exactly one start place."""
    r = h.A[2].tobytes()
    out = [r[a:a + 12] for a in range(49, 60)]
    assert all(h.sm.occ(s, 64).start_total == 1 for s in out)
    return out


# ---- the inputs: name -> (MSA of host(), reads, min_length, max_per_seed) ----------------------------------------------

def surplus_reads(seeds):
    """One read per surplus in +-SURPLUS at the junction in its middle and two with none, `seeds` seeds each."""
    a, b = (seeds - 2) // 2, (seeds - 2) - (seeds - 2) // 2
    return [junction_read(3 * j, [0] * a + [s] + [0] * b) for j, s in enumerate([x * y for x in SURPLUS for y in (1, -1)] + [0, 0])]


def none_reads(h):
    """Reads of pieces that hold '#' (no place of theirs has a column) between rotations of the unit, for cap 16:
    mixed and all-'#' reads of each tier."""
    S = h.edge_strings()
    x = [S[e + 1][-6:] + b"#" + S[e][:6] + b"T" for e in range(4)]            # as test_degenerate_cases: one place, no column
    mix = lambda n: b"".join(b"#T" + rot(5 * j) + b"T" for j in range(n)) + b"#T"      # noqa: E731
    return [x[0] + rot(2) + b"T" + x[1],                                          # small: 1 + 16 + 1
            b"#T",                                                                # small, no column at all
            b"#T" + rot(0) + b"T" + x[0] + rot(3) + b"T#T" + x[1] + rot(6) + b"T#T",    # wave
            b"#T" * 3 + x[2],                                                     # wave, no column at all
            mix(33),                                                              # spill: 67 * 16
            b"#T" * 65 + x[3],                                                    # spill, no column at all
            b"", rot(1) + b"T"]


def occupancy_small_reads(h, count):
    """`count` reads of the small tier: one seed with one place, then SM_MAX places over many seeds, in turns."""
    ones = one_place_pieces(h)
    rng = np.random.default_rng(17)
    cnt = {r: h.sm.occ(rot(r), 64).start_total for r in range(12)}
    out = []
    for j in range(count):
        if j % 2 == 0:
            out.append(ones[(j // 2) % len(ones)] + b"T")
            continue
        pieces, left = [], SM_MAX
        for r in rng.permutation(12).tolist()[:j % 4]:                            # 1 or 3 rotations, the rest one place each
            if cnt[r] <= left:
                pieces.append(rot(r))
                left -= cnt[r]
        pieces += [ones[int(i)] for i in rng.integers(0, len(ones), left)]
        out.append(b"".join(pieces[i] + b"T" for i in rng.permutation(len(pieces)).tolist()))
    return out


def occupancy_batch(h, count):
    """The small reads with a read without a place after every third of them."""
    out = []
    for j, r in enumerate(occupancy_small_reads(h, count)):
        out.append(r)
        if j % 3 == 2:
            out.append((b"", b"TT", b"T")[(j // 3) % 3])
    return out + [b""]


OCCUPANCY = (GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1)
MANY_WAVE = (SM_MAX + 1, 48, 65, 160, 512, 1008, LDS_MAX - 1, LDS_MAX, 300, 999)       # start places of the reads, cap 16
MANY_SPILL = (LDS_MAX + 1, LDS_MAX + 2, LDS_MAX + 16, LDS_MAX + 17, LDS_MAX + 32)
MANY_SMALL = (1, 16, 17, SM_MAX)


def many_reads():
    """Reads of the given numbers of start places for cap 16 on tier_msa: rotations (16 places each) and a 12-mer of
    row 2 that has one place, in an order drawn at random, reads without places between them."""
    rng = np.random.default_rng(23)
    reads = []
    for places in MANY_WAVE + MANY_SPILL + MANY_SMALL:
        pieces = [rot(int(r)) for r in rng.integers(0, 12, places // 16)] + [b"ACGCAGACCGAA"] * (places % 16)
        reads.append(b"".join(pieces[i] + b"T" for i in rng.permutation(len(pieces)).tolist()))
    reads += [b"", b"TT", b"T", b""]
    return [reads[i] for i in rng.permutation(len(reads)).tolist()]


def between_reads(n):
    """A '#' seed first, last and between every two of n rotations whose places line up without a surplus."""
    return b"#T" + b"T#T".join(rot(15 * j) for j in range(n)) + b"T#"


def cases():
    small, tier = host("small"), host("tier")
    out = {"surplus_small": ("small", surplus_reads(2), 12, 64),
           "surplus_large": ("tier", surplus_reads(2) + surplus_reads(6), 12, 256),
           "none": ("tier", none_reads(tier), 1, 16),
           "many": ("tier", many_reads(), 12, 16),
           "between_small": ("small", [between_reads(2), b"#T#", between_reads(1)], 1, 64),
           "between_large": ("tier", [between_reads(2), between_reads(6), b"#T#"], 1, 256)}
    for n in OCCUPANCY:
        out["occupancy_%d" % n] = ("small", occupancy_batch(small, n), 12, 64)
    return out


# ---- counters, all from the seeds and the model ------------------------------------------------------------------------

def places_per_read(inp):
    seed_off, _, _, start_off, _ = inp
    return np.diff(start_off[seed_off.astype(np.int64)].astype(np.int64))


def tier_of(places):
    return None if places == 0 else "small" if places <= SM_MAX else "wave" if places <= LDS_MAX else "spill"


def expected_stats(inp):
    """What chain_stats() must say after chaining these seeds (a call without a start place counts nothing)."""
    tiers = [tier_of(int(p)) for p in places_per_read(inp)]
    return {"anchors": int((inp[4] != NONE).sum()), "reads_small": tiers.count("small"), "reads_wave": tiers.count("wave"),
            "reads_spill": tiers.count("spill")}


def surplus_pairs(an):
    """{surplus: pairs} over the pairs (i, j) of a read's anchors that the band decides: seed(i) < seed(j) and
    c_j >= c_i + k_i."""
    if not an:
        return {}
    _, t, q, k, c = (np.array(x, dtype=np.int64) for x in zip(*an))
    ok = (t[:, None] < t[None, :]) & (c[None, :] >= (c + k)[:, None])
    sur = (c[None, :] - c[:, None]) - (q[None, :] - q[:, None])
    v, n = np.unique(sur[ok], return_counts=True)
    return dict(zip(v.tolist(), n.tolist()))


def surplus_counters(inp, solved):
    """seen[tier]: pairs at each surplus +-SURPLUS, and the reads whose chain under band B differs from the one under
    B - 1 through an insertion (a pair of its chain under B has surplus -B) and through a deletion (+B)."""
    seen = {t: dict(pairs={s * y: 0 for s in SURPLUS for y in (1, -1)}, changed={s * y: 0 for s in BANDS_AT for y in (1, -1)}) for t in TIERS}
    for r, p in enumerate(places_per_read(inp)):
        t = tier_of(int(p))
        if t is None:
            continue
        an = solved[0][r][0]
        for s, n in surplus_pairs(an).items():
            if s in seen[t]["pairs"]:
                seen[t]["pairs"][s] += n
        for B in BANDS_AT:
            idx, below = solved[B][r][2], solved[B - 1][r][2]
            if idx == below:
                continue
            steps = {(an[j][4] - an[i][4]) - (an[j][2] - an[i][2]) for i, j in zip(idx, idx[1:])}
            for s in (B, -B):
                seen[t]["changed"][s] += s in steps
    return seen


def none_counters(inp):
    """Per tier: reads with a no-column place before and one after a place with a column, and reads without any column."""
    seed_off, _, _, start_off, col = inp
    seen = {t: dict(around=0, all_none=0) for t in TIERS}
    for r, p in enumerate(places_per_read(inp)):
        t = tier_of(int(p))
        if t is None:
            continue
        c = col[int(start_off[int(seed_off[r])]):int(start_off[int(seed_off[r + 1])])]
        have, lack = np.nonzero(c != NONE)[0], np.nonzero(c == NONE)[0]
        seen[t]["all_none"] += len(have) == 0
        seen[t]["around"] += len(have) > 0 and len(lack) > 0 and lack[0] < have[0] and lack[-1] > have[-1]
    return seen


def equal_offsets(inp):
    """Seeds without a start place inside reads that have some."""
    seed_off, _, _, start_off, _ = inp
    n = 0
    for r, p in enumerate(places_per_read(inp)):
        if p:
            n += int((np.diff(start_off[int(seed_off[r]):int(seed_off[r + 1]) + 1].astype(np.int64)) == 0).sum())
    return n


def skipped_seeds(inp, solved):
    """Chains that take two seeds with a seed between them that has places, none with a column; reads whose first and
    whose last seed are such seeds."""
    seed_off, _, _, start_off, col = inp
    no_col = lambda t: all(col[g] == NONE for g in range(int(start_off[t]), int(start_off[t + 1])))      # noqa: E731
    seen = dict(between=0, first_and_last=0)
    for r, (an, _, idx) in enumerate(solved):
        for i, j in zip(idx, idx[1:]):
            seen["between"] += an[j][1] == an[i][1] + 2 and no_col(an[i][1] + 1)
        a, b = int(seed_off[r]), int(seed_off[r + 1])
        seen["first_and_last"] += len(idx) > 0 and b - a >= 3 and no_col(a) and no_col(b - 1)
    return seen


_SOLVED = {}


def solved_of(name, inp, band):
    """CM.solve of a case's seeds, once per band for all tests."""
    if (name, band) not in _SOLVED:
        _SOLVED[(name, band)] = CM.solve(*inp, band)
    return _SOLVED[(name, band)]


def case_inputs(name):
    hname, reads, L, cap = cases()[name]
    return host(hname).seeds(reads, L, cap)


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_inputs_reach_their_classes_in_the_models():
    """Every input of the GPU tests below, from the Python models alone, and the classes it is there for."""
    assert (SM_MAX, LDS_MAX, GROUP) == (32, 1024, 16)
    all_cases = cases()
    # 1. surplus: every tier sees a pair at +-B and +-(B + 1), and a chain that the band changes, for either sign
    tiers_seen = set()
    for name in ("surplus_small", "surplus_large"):
        inp = case_inputs(name)
        assert equal_offsets(inp) == 0
        seen = surplus_counters(inp, {band: solved_of(name, inp, band) for band in (0, 1, 2, 3)})
        for t in (("small",) if name == "surplus_small" else ("wave", "spill")):
            assert all(v > 0 for v in seen[t]["pairs"].values()) and all(v > 0 for v in seen[t]["changed"].values()), (t, seen[t])
            tiers_seen.add(t)
    assert tiers_seen == set(TIERS)
    # 2. places without a column around places with one, and reads of nothing else, in every tier
    inp = case_inputs("none")
    seen = none_counters(inp)
    assert all(v > 0 for t in TIERS for v in seen[t].values()), seen
    assert 0 < expected_stats(inp)["anchors"] < len(inp[4])
    for r, (an, sc, idx) in enumerate(solved_of("none", inp, None)):
        assert (sc == 0 and idx == []) == (not an)
    # 3. occupancy: exactly the wanted number of small-tier reads, one place and SM_MAX places in turns, placeless between
    for n in OCCUPANCY:
        inp = case_inputs("occupancy_%d" % n)
        p = places_per_read(inp)
        small = p[p > 0]
        assert len(small) == n and (p == 0).sum() >= 3 and small[0::2].tolist() == [1] * len(small[0::2])
        assert small[1::2].tolist() == [SM_MAX] * len(small[1::2])
        seeds = np.diff(inp[0].astype(np.int64))[p > 0]
        assert (seeds[0::2] == 1).all() and (seeds[1::2] >= 3).all() and seeds.max() >= 20
        assert max(len(idx) for _, _, idx in solved_of("occupancy_%d" % n, inp, None)) >= (2 if n > 3 else 1)
    # 4. many reads of the large tiers: the place counts asked for, and tiers in a mixed order
    inp = case_inputs("many")
    p = places_per_read(inp)
    assert sorted(p[p > 0].tolist()) == sorted(MANY_WAVE + MANY_SPILL + MANY_SMALL) and (p == 0).sum() == 4
    st = expected_stats(inp)
    assert st["reads_wave"] == len(set(MANY_WAVE)) >= 9 and st["reads_spill"] == len(set(MANY_SPILL)) >= 5
    assert {LDS_MAX, LDS_MAX + 1, SM_MAX, SM_MAX + 1} <= set(p.tolist())
    order = [tier_of(int(x)) for x in p]
    assert sum(a != b for a, b in zip(order, order[1:])) >= 10
    # 5. min_score: several distinct scores, among them 0
    scores = {sc for _, sc, _ in solved_of("many", inp, None)}
    assert len(scores) >= 4 and 0 in scores
    # 7. a seed of places without a column between two seeds of a chain, and first and last in a read; the calls give a
    # seed with a match at least one place under any cap above 0, so start_off never repeats inside a read with places
    for name, tiers in (("between_small", {"small"}), ("between_large", {"wave", "spill"})):
        inp = case_inputs(name)
        assert {tier_of(int(x)) for x in places_per_read(inp)} >= tiers
        seen = skipped_seeds(inp, solved_of(name, inp, 0))
        assert seen["between"] >= len(tiers) and seen["first_and_last"] >= len(tiers), seen
        assert equal_offsets(inp) == 0
    for name, (hname, reads, L, cap) in all_cases.items():
        assert equal_offsets(host(hname).seeds(reads, L, cap)) == 0, name
        none = host(hname).seeds(reads, L, 0)
        assert len(none[4]) == 0 and len(none[1]) > 0, name                  # cap 0: every offset equal, and no read with a place


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def seeds_of(pix, name, case=None):
    """PatternIndex.seeds of a case, checked to be what the models say -> (Seeds, model inputs)."""
    hname, reads, L, cap = case or cases()[name]
    sd = pix.seeds(reads, min_length=L, max_per_seed=cap, msa=True)
    inp = model_inputs(sd)
    for got, want, f in zip(inp, host(hname).seeds(reads, L, cap), ("seed_off", "q_start", "length", "start_off", "start_col")):
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, f)
    return sd, inp


def check(pix, inp, solved, band, min_score, what):
    """chains() against the model, chain_stats() against the seeds, every anchor's seed against start_off."""
    ch = pix.chains(band=band, min_score=min_score)
    same(ch, CM.assemble(solved, min_score), what)
    st = pix.chain_stats()
    assert {k: st[k] for k in ("anchors", "reads_small", "reads_wave", "reads_spill")} == expected_stats(inp), what
    start_off, col = inp[3].astype(np.int64), inp[4]
    assert (col[ch.anchor_place] != NONE).all(), what
    seed = ch.anchor_seed.astype(np.int64)
    assert ((start_off[seed] <= ch.anchor_place) & (ch.anchor_place < start_off[seed + 1])).all(), what
    return ch


def build_host(engine, hname):
    return build(engine, host(hname).A, host(hname).b)


@pytest.mark.gpu
def test_both_signs_of_the_surplus_at_the_band(engine):
    seen = {}
    for name in ("surplus_small", "surplus_large"):
        with build_host(engine, cases()[name][0]) as pix:
            assert (pix.chain_stats()["small_max"], pix.chain_stats()["lds_max"]) == (SM_MAX, LDS_MAX)
            _, inp = seeds_of(pix, name)
            solved = {band: solved_of(name, inp, band) for band in (0, 1, 2, 3)}
            for band in (0, 1, 2, 3):
                check(pix, inp, solved[band], band, 0, (name, band))
            got = surplus_counters(inp, solved)
            seen.update({t: got[t] for t in (("small",) if name == "surplus_small" else ("wave", "spill"))})
    assert set(seen) == set(TIERS)
    assert all(v > 0 for t in TIERS for kind in ("pairs", "changed") for v in seen[t][kind].values()), seen


@pytest.mark.gpu
def test_places_without_a_column_in_every_tier(engine):
    with build_host(engine, "tier") as pix:
        sd, inp = seeds_of(pix, "none")
        for band in (None, 2):
            solved = solved_of("none", inp, band)
            ch = check(pix, inp, solved, band, 0, ("none", band))
            assert pix.chain_stats()["anchors"] == int((sd.occ.start_col != NONE).sum()) < len(sd.occ.start_col)
            for r, (an, _, _) in enumerate(solved):
                if not an:
                    assert int(ch.score[r]) == 0 and len(ch.of(r)) == 0, r
    seen = none_counters(inp)
    assert all(v > 0 for t in TIERS for v in seen[t].values()), seen


@pytest.mark.gpu
def test_small_tier_workgroups_short_full_and_over(engine):
    seen = dict(one=0, full=0, placeless=0, chained=0)
    with build_host(engine, "small") as pix:
        for n in OCCUPANCY:
            name = "occupancy_%d" % n
            _, inp = seeds_of(pix, name)
            p = places_per_read(inp)
            for band in (None, 1):
                ch = check(pix, inp, solved_of(name, inp, band), band, 0, (name, band))
            st = pix.chain_stats()
            assert (st["reads_small"], st["reads_wave"], st["reads_spill"]) == (n, 0, 0)
            seen["one"] += int((p == 1).sum())
            seen["full"] += int((p == SM_MAX).sum())
            seen["placeless"] += int((p == 0).sum())
            seen["chained"] += sum(len(idx) >= 2 for _, _, idx in solved_of(name, inp, 1))
        # every read of the largest batch chained alone (band 1: `ch` above)
        hname, reads, L, cap = cases()[name]
        together = per_read(ch)
        for r, read in enumerate(reads):
            one = pix.seeds([read], min_length=L, max_per_seed=cap, msa=True, chain=True, band=1)
            base = int(inp[3][int(inp[0][r])]), int(inp[0][r])
            sc, pl, se = per_read(one.chains)[0]
            assert (sc, [x + base[0] for x in pl], [x + base[1] for x in se]) == together[r], r
    assert all(v > 0 for v in seen.values()) and (seen["one"], seen["full"]) == (sum((n + 1) // 2 for n in OCCUPANCY), sum(n // 2 for n in OCCUPANCY))


@pytest.mark.gpu
def test_many_reads_of_the_wave_and_spill_tiers_in_one_call(engine):
    with build_host(engine, "tier") as pix:
        _, inp = seeds_of(pix, "many")
        for band in (None, 6):
            check(pix, inp, solved_of("many", inp, band), band, 0, ("many", band))
        st = pix.chain_stats()
    assert st["reads_wave"] == len(set(MANY_WAVE)) >= 9 and st["reads_spill"] == len(set(MANY_SPILL)) >= 5
    p = places_per_read(inp)
    assert {LDS_MAX, LDS_MAX + 1} <= set(p.tolist()) and st["reads_small"] == len(MANY_SMALL)


@pytest.mark.gpu
def test_min_score_at_every_score_and_beyond_32_bits(engine):
    seen = dict(at=0, one_below=0, one_above=0)
    with build_host(engine, "tier") as pix:
        _, inp = seeds_of(pix, "many")
        solved = solved_of("many", inp, None)
        score = np.array([sc for _, sc, _ in solved], dtype=np.uint32)
        values = sorted({max(s + d, 0) for s in set(score.tolist()) for d in (-1, 0, 1)}) + [2 ** 32, 2 ** 32 + int(score.max()), 2 ** 64 - 1]
        for v in values:
            ch = check(pix, inp, solved, None, v, ("min_score", v))
            assert np.array_equal(ch.score, score), v
            kept = np.diff(ch.chain_off.astype(np.int64)) > 0
            assert np.array_equal(kept, (score >= v) & (score > 0)), v
            seen["at"] += int((score == v).sum())
            seen["one_below"] += int((score == v - 1).sum())
            seen["one_above"] += int((score == v + 1).sum())
            if v >= 2 ** 32:
                assert not kept.any() and len(ch.anchor_place) == 0
    assert all(v > 0 for v in seen.values()) and len(set(score.tolist())) >= 4, seen


@pytest.mark.gpu
def test_buffers_that_outlive_a_call(engine):
    """One index through calls of very different sizes; after each, chains() is the model's and, for the repeated batch,
    byte for byte what an index that has seen nothing else returns.  Between them: a segmentation on the engine, a second
    index, occurrences() on the first."""
    hname, large, L, cap = cases()["none"]
    tiny = [rot(4) + b"T", b"#T" + rot(7) + b"T"]
    placeless = [b"", b"TT", b"T", b"TTT"]
    rng = np.random.default_rng(29)
    other = random_msa(rng, 8, 200, gap_p=0.03, gap_run=3, similar=0.93)
    other_b = engine.minmax_dp(engine.elastic_f(other))
    h = host(hname)
    steps = []

    def call(pix, reads, cap, band, min_score, what):
        _, inp = seeds_of(pix, what, (hname, reads, L, cap))
        ch = check(pix, inp, CM.solve(*inp, band), band, min_score, what)
        steps.append((what, expected_stats(inp)))
        return [getattr(ch, f).tobytes() for f in ("chain_off", "score", "anchor_place", "anchor_seed")]

    with build_host(engine, hname) as fresh:
        want = call(fresh, large, cap, 2, 12, "fresh")
    with build_host(engine, hname) as pix:
        occ = pix.occurrences(large[:4], max_per_pattern=8, msa=True)
        assert call(pix, large, cap, 2, 12, "1: large") == want
        assert np.array_equal(engine.minmax_dp(engine.elastic_f(other)), other_b)
        call(pix, tiny, cap, None, 0, "2: two small reads")
        with build(engine, other, other_b) as second:
            second.seeds([other[0][other[0] != ord("-")].tobytes()], max_per_seed=4, msa=True, chain=True)
            assert call(pix, large, cap, 2, 12, "3: large") == want
        call(pix, large, 3, None, 0, "4: large, another cap")
        o2 = pix.occurrences(large[:4], max_per_pattern=8, msa=True)
        for f in ("count", "start_off", "start_src", "start_dst", "start_offset", "start_col", "end_col"):
            assert np.array_equal(getattr(o2, f), getattr(occ, f)), f
        call(pix, placeless, cap, None, 0, "5: placeless")
        assert pix.chain_stats()["anchors"] == 0 and pix.chain_stats()["reads_spill"] == 0
        assert np.array_equal(engine.minmax_dp(engine.elastic_f(other)), other_b)
        assert call(pix, large, cap, 2, 12, "6: large") == want
        call(pix, tiny, cap, 0, 0, "7: two small reads")
    stats = dict(steps)
    assert stats["1: large"] == stats["6: large"] == stats["fresh"] and stats["1: large"]["reads_spill"] >= 2
    assert stats["2: two small reads"]["reads_spill"] == stats["4: large, another cap"]["reads_spill"] == 0
    assert stats["4: large, another cap"]["anchors"] not in (0, stats["1: large"]["anchors"])
    assert stats["5: placeless"] == dict(anchors=0, reads_small=0, reads_wave=0, reads_spill=0)
    assert h.seeds(large, L, cap)[4].size > 20 * h.seeds(tiny, L, cap)[4].size


@pytest.mark.gpu
def test_seeds_that_give_the_chain_no_anchor(engine):
    """fbg_pindex_seeds reports a seed only with a match, and a match has a start place; a cap of 0 leaves every seed of
    every read without one.  So no call yields a read in which start_off repeats beside a seed with places (the CPU test
    asserts that of every input here), and the seeds that k_pc_trace's search must pass over are those whose places all
    lack a column: '#' seeds between two seeds of a chain, and first and last in a read."""
    seen = dict(between=0, first_and_last=0)
    tiers = set()
    for name in ("between_small", "between_large"):
        with build_host(engine, cases()[name][0]) as pix:
            _, inp = seeds_of(pix, name)
            for band in (0, None):
                check(pix, inp, solved_of(name, inp, band), band, 0, (name, band))
            assert equal_offsets(inp) == 0
            tiers |= {tier_of(int(x)) for x in places_per_read(inp)}
            for k, v in skipped_seeds(inp, solved_of(name, inp, 0)).items():
                seen[k] += v
    assert tiers >= set(TIERS) and seen["between"] >= 3 and seen["first_and_last"] >= 3, (tiers, seen)
