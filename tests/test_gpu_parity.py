"""GPU parity: every result of libfbg_hip.so (through its C ABI) must be bit-identical to the CPU
oracle (oracle/fbg_oracle.c) on the same inputs.  Integer work: exact equality, no tolerance."""
import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

FIXTURES = {
    "msa": ["AGCGA-CTAGATAC", "AGC--ACTAGTT--", "AGCGA-CTCGTTAC", "AGC--ACT-GTTAC"],
    "test": ["ACCGATGCCGAGCTA", "ACTACTACCGAGCTA"],
    "test2": ["-CCGATGCCGA-CTA", "A-TACTACCGAGCT-"],
    "test3": ["ACCGATGCCGA-CTA", "A-TACTACCGAGCTA"],
}


def test_index_arrays_match_oracle(engine):
    rng = np.random.default_rng(1)
    for (m, n, kw) in [(4, 40, {}), (7, 300, dict(gap_p=0.03, gap_run=5)), (33, 257, dict(similar=0.95)),
                       (3, 1000, dict(alphabet="AC", similar=0.99)), (65, 129, dict(alphabet="ACGTN"))]:
        msa = random_msa(rng, m, n, **kw)
        T, SA, ISA, LCP = O.msa_index(msa)
        engine.msa_load_host(msa)
        engine.index_build()
        gT, gSA, gISA, gPL, gPR = engine.index_download()
        assert np.array_equal(gT, T)
        assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
        assert np.array_equal(gISA.astype(np.int64), ISA.astype(np.int64))
        N = len(T)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
        assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])
        assert N == engine.text_length()


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_fixtures_elastic(engine, name):
    msa = O.msa_array(FIXTURES[name])
    for tricks_off in (False, True):
        f = O.compute_f(msa, disable_tricks=tricks_off)
        try:
            g = engine.elastic_f(msa, disable_efg_tricks=tricks_off)
        except Exception as e:   # NoSegmentation carries no f; compare through the staged path instead
            assert tricks_off and f[0] == msa.shape[1], e
            continue
        assert np.array_equal(g, f)
        mml, bt, b = O.minmax_dp(f)
        gb, gmml, gbt = engine.minmax_dp(g, full=True)
        assert np.array_equal(gb, b) and np.array_equal(gmml, mml) and np.array_equal(gbt, bt)


CASES = [
    (2, 50, {}), (5, 64, {}), (1, 30, {}), (8, 1, {}), (64, 500, {}),
    (16, 400, dict(gap_p=0.02, gap_run=7)), (30, 300, dict(gap_p=0.05, gap_run=3, n_p=0.02)),
    (40, 600, dict(similar=0.97)), (100, 350, dict(similar=0.99, gap_p=0.01, gap_run=10)),
    (257, 200, dict(similar=0.9)), (1000, 120, dict(similar=0.98)), (1025, 70, {}),
    (12, 2000, dict(alphabet="AC", similar=0.995)), (6, 300, dict(alphabet="ACGTN", n_p=0.05)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_elastic_f_and_dp(engine, case):
    m, n, kw = CASES[case]
    rng = np.random.default_rng(100 + case)
    msa = random_msa(rng, m, n, **kw)
    for ignore in ("", "N"):
        f = O.compute_f(msa, ignore=ignore)
        g = engine.elastic_f(msa, ignorechars=ignore)
        assert np.array_equal(g, f), (case, ignore, np.flatnonzero(g != f)[:10])
    mml, bt, b = O.minmax_dp(f)
    gb, gmml, gbt = engine.minmax_dp(g, full=True)
    assert np.array_equal(gmml, mml)
    assert np.array_equal(gbt, bt)
    assert np.array_equal(gb, b)


def test_disable_tricks_and_max_merge(engine):
    rng = np.random.default_rng(7)
    msa = random_msa(rng, 9, 250, gap_p=0.02, gap_run=4)
    f0 = rng.integers(0, 250, 250).astype(np.uint64)
    f = O.compute_f(msa, disable_tricks=True, f_init=f0)
    import founderblockgraphs_amd as F
    try:
        g = engine.elastic_f(msa, disable_efg_tricks=True, f=f0)
        assert np.array_equal(g, f)
    except F.NoSegmentation:
        assert f[0] == 250


@pytest.mark.parametrize("case", range(8))
def test_random_nonelastic(engine, case):
    rng = np.random.default_rng(200 + case)
    m, n, kw = [(2, 15, {}), (4, 200, {}), (64, 700, {}), (10, 500, dict(similar=0.9)),
                (3, 400, dict(alphabet="AC")), (1, 50, {}), (100, 300, dict(similar=0.97)),
                (5, 1, {})][case]
    msa = random_msa(rng, m, n, **kw)
    v = O.segment_v(msa)
    gv = engine.repeatfree_v(msa)
    assert np.array_equal(gv, v)
    s, prev, b = O.segment_dp(v)
    gs, gprev, gb = engine.repeatfree_dp(gv)
    assert np.array_equal(gs, s) and np.array_equal(gprev, prev)
    assert (b is None) == (gb is None)
    if b is not None:
        assert np.array_equal(gb, b)


def test_nonelastic_rejects_gaps(engine):
    import founderblockgraphs_amd as F
    with pytest.raises(F.FbgError):
        engine.repeatfree_v(O.msa_array(FIXTURES["msa"]))


def test_column_shards_equal_whole(engine):
    """compute_f_range semantics (fbg.cpp:1475-1577): any column partition gives the same f."""
    import torch
    rng = np.random.default_rng(5)
    msa = random_msa(rng, 50, 1000, similar=0.95, gap_p=0.01, gap_run=6)
    f = O.compute_f(msa)
    engine.msa_load_host(msa)
    engine.index_build()
    n = msa.shape[1]
    for shards in (1, 2, 3, 8):
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        edges = [n * k // shards for k in range(shards + 1)]
        for k in range(shards):
            engine.scan_f(edges[k], edges[k + 1], d_f.data_ptr())
        engine.sync()
        assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), f)


def _random_f(rng, n, max_ext, style):
    x = np.arange(n, dtype=np.int64)
    if style == "uniform" or n < 4:
        ext = rng.integers(0, max_ext + 1, n)
    elif style == "plateau":      # many columns share one right end (long repeats)
        ends = np.sort(rng.choice(np.arange(1, n), size=max(1, n // max(2, max_ext)), replace=False))
        nxt = ends[np.minimum(np.searchsorted(ends, x, side="left"), len(ends) - 1)]
        ext = np.clip(nxt - x, 0, max_ext)
    else:                         # mostly tiny with rare long extensions
        ext = np.where(rng.random(n) < 0.03, rng.integers(0, max_ext + 1, n), rng.integers(0, 3, n))
    f = np.minimum(x + ext, n - 1)
    f[0] = 0
    return f.astype(np.uint64)


@pytest.mark.parametrize("max_ext", [0, 1, 5, 30, 31, 32, 60, 100, 200, 400, 511, 600])
@pytest.mark.parametrize("style", ["uniform", "plateau", "spiky"])
def test_dp_sweep_random_f(engine, max_ext, style):
    """Both sweeps (wave-parallel for small extensions, literal otherwise) against the literal oracle."""
    rng = np.random.default_rng(max_ext * 7 + len(style))
    for n in (1, 2, 63, 64, 65, 1000, 5000):
        f = _random_f(rng, n, max_ext, style)
        mml, bt, b = O.minmax_dp(f)
        gb, gmml, gbt = engine.minmax_dp(f, full=True)
        assert np.array_equal(gmml, mml), (n, np.flatnonzero(gmml != mml)[:5])
        assert np.array_equal(gbt, bt), (n, np.flatnonzero(gbt != bt)[:5])
        assert np.array_equal(gb, b)


@pytest.mark.parametrize("max_ext", [254, 255, 300, 700, 1021, 1022, 1023, 1500, 2045, 2046, 2047, 3000, 4093, 4094, 5000, 6000, 8189, 8190, 8191,
                                     12000, 16381, 16382, 16383, 20000])
@pytest.mark.parametrize("style", ["uniform", "plateau", "spiky"])
def test_dp_sweep_wide_windows(engine, max_ext, style):
    """Extensions of hundreds to thousands of columns: the 16-bit matrix chain (k_dpw_*), its window sizes 1024 .. 16384,
    and the hand-over to the literal sweep when a value reaches the largest window."""
    rng = np.random.default_rng(max_ext * 11 + len(style))
    kinds = set()
    for n in (255, 256, 257, 1500, 40_000, 40_001):
        f = _random_f(rng, n, max_ext, style)
        if n == 40_001:               # f[0] > 0 (only without the elastic tricks): nothing ends before step f[0] + 1
            f[0] = min(n - 1, int(rng.integers(1, max_ext + 1)))
        mml, bt, b = O.minmax_dp(f)
        gb, gmml, gbt = engine.minmax_dp(f, full=True)
        assert np.array_equal(gmml, mml), (n, np.flatnonzero(gmml != mml)[:5])
        assert np.array_equal(gbt, bt), (n, np.flatnonzero(gbt != bt)[:5])
        assert np.array_equal(gb, b)
        kinds.add(engine.get_option("dp_kind"))
        if n >= 40_000 and style == "uniform" and 512 <= max_ext <= 16381:
            # extensions of every size up to max_ext: beyond the byte matrices, within the 16-bit ones (f[0] > 0 included);
            # the one-lane literal sweep (dp_kind 0) only beyond the 16384 window
            assert engine.get_option("dp_kind") in (3, 4, 5, 6, 7), (n, max_ext, engine.get_option("dp_kind"))
    assert kinds <= {0, 1, 2, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("switches", [{"dpw_matrix": 1}, {"dp_chain1": 1}])
def test_dp_sweep_earlier_methods_stay_exact(engine, switches):
    """The sweep's kernels of rounds 1-3 that round 4 replaced stay reachable through options (A/B timing in one process):
    k_dpw_blockM / k_dpw_chain (one 128 x window matrix per block) behind dpw_matrix, the one-wave walk over the byte
    matrices k_dp_chain behind dp_chain1 -- both against the oracle on every window size."""
    rng = np.random.default_rng(404)
    with fbg_options(engine, switches):
        for max_ext, style in ((40, "uniform"), (100, "plateau"), (200, "spiky"), (700, "plateau"), (1500, "uniform"), (3000, "plateau"),
                               (6000, "plateau"), (12000, "uniform")):
            for n in (300, 40_000):
                f = _random_f(rng, n, max_ext, style)
                mml, bt, b = O.minmax_dp(f)
                gb, gmml, gbt = engine.minmax_dp(f, full=True)
                assert np.array_equal(gmml, mml) and np.array_equal(gbt, bt) and np.array_equal(gb, b), (switches, n, max_ext, style)


def test_dp_sweep_wide_windows_full_size(engine):
    """10^6 columns whose extensions reach 900 columns (rows that resemble each other, with gaps): the 16-bit matrix chain
    against the statement-by-statement sweep, and the properties of a valid segmentation."""
    import torch
    n = 1_000_000
    rng = np.random.default_rng(99)
    f = _random_f(rng, n, 900, "plateau").astype(np.int64)
    d_f = torch.from_numpy(f).cuda()
    out = []
    for literal in (0, 1):
        with fbg_options(engine, {"FBG_DP_LITERAL": str(literal)}):
            d_b = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_mml = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_bt = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            cnt = engine.minmax_dp_device(d_f.data_ptr(), n, d_b.data_ptr(), d_mml.data_ptr(), d_bt.data_ptr())
            assert engine.get_option("dp_kind") == (0 if literal else 3)
            out.append((cnt, d_b[:cnt].clone(), d_mml, d_bt))
    assert out[0][0] == out[1][0] and all(torch.equal(out[0][k], out[1][k]) for k in (1, 2, 3))
    b = out[0][1]
    assert int(b[-1]) == n and bool((b[1:] > b[:-1]).all())
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), b[:-1] + 1])
    ends = torch.cat([b[:-1], torch.tensor([n - 1], device="cuda")])
    assert bool((d_f[starts] <= ends).all())
    assert int((ends - starts + 1).max()) == int(out[0][2][n]) > 256


def test_dp_sweep_window_8192_at_scale(engine):
    """Extensions of up to 6000 columns over 2 * 10^5 columns: the 8192 window of the 16-bit matrix chain (no one-lane sweep
    on the product path: k_dp_minmax only runs under dp_literal, or beyond the 16384 window) against the statement-by-
    statement sweep."""
    import torch
    n = 200_000
    rng = np.random.default_rng(123)
    f = _random_f(rng, n, 6000, "plateau").astype(np.int64)
    d_f = torch.from_numpy(f).cuda()
    out = []
    for literal in (0, 1):
        with fbg_options(engine, {"FBG_DP_LITERAL": str(literal)}):
            d_b = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_mml = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_bt = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            cnt = engine.minmax_dp_device(d_f.data_ptr(), n, d_b.data_ptr(), d_mml.data_ptr(), d_bt.data_ptr())
            assert engine.get_option("dp_kind") == (0 if literal else 6)
            out.append((cnt, d_b[:cnt].clone(), d_mml, d_bt))
    assert out[0][0] == out[1][0] and all(torch.equal(out[0][k], out[1][k]) for k in (1, 2, 3))


def test_dp_sweep_f0_nonzero_uses_literal_semantics(engine):
    """f[0] != 0 (only with --disable-elastic-tricks): lazy-I quirks of fbg.cpp:2004-2013 must survive."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(11)
    for n in (10, 200, 3000):
        for _ in range(5):
            f = _random_f(rng, n, 12, "uniform")
            f[0] = rng.integers(1, min(n - 1, 6) + 1)
            try:
                mml, bt, b = O.minmax_dp(f)
            except O.OracleError:
                with pytest.raises(F.NoSegmentation):
                    engine.minmax_dp(f)
                continue
            gb, gmml, gbt = engine.minmax_dp(f, full=True)
            assert np.array_equal(gmml, mml) and np.array_equal(gbt, bt) and np.array_equal(gb, b)


def test_sharded_pipeline_single_gpu(engine):
    """founderblockgraphs_amd.distributed plumbing on the real engine, world of 1..3 simulated in-process."""
    import torch
    from founderblockgraphs_amd import distributed as D
    rng = np.random.default_rng(6)
    msa = random_msa(rng, 30, 700, similar=0.96, gap_p=0.02, gap_run=5)
    n = msa.shape[1]
    f = O.compute_f(msa)
    b = O.minmax_dp(f)[2]
    engine.msa_load_host(msa)
    engine.index_build()
    scan, sweep = D.engine_scan_shard(engine, n), D.engine_sweep(engine)
    for world in (1, 2, 3):
        parts = [scan(*D.shard_range(n, r, world)).clone() for r in range(world)]
        full = torch.cat(parts)
        assert np.array_equal(full.cpu().numpy().astype(np.uint64), f)
        assert np.array_equal(sweep(full).cpu().numpy().astype(np.uint64), b)


def test_row_group_pairs_single_gpu(engine):
    """Capacity plan for texts beyond 32-bit ranks: max over row-group pairs == whole-MSA f, on the engine."""
    import torch
    from founderblockgraphs_amd import distributed as D
    rng = np.random.default_rng(8)
    m, n = 37, 600
    msa = random_msa(rng, m, n, similar=0.97, gap_p=0.02, gap_run=4, n_p=0.01)
    f = O.compute_f(msa, ignore="N")
    G, groups, plan = D.plan_row_pairs(m, n, 1, limit=20 * (n + 1) + 1)
    d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for a, b in plan[0]:
        rows = list(range(*groups[a])) + list(range(*groups[b]))
        engine.msa_load_host(msa[rows])
        engine.index_build(ignorechars="N")
        engine.scan_f(0, n, d_f.data_ptr())
    engine.sync()
    assert G >= 4 and np.array_equal(d_f.cpu().numpy().astype(np.uint64), f)


def test_committed_oracle_vectors(engine):
    """GPU results against tests/golden/oracle_vectors.json (made by tests/golden/make_golden.py)."""
    import hashlib
    import json
    import os

    def digest(a):
        return hashlib.sha256(np.ascontiguousarray(a, dtype="<u8").tobytes()).hexdigest()
    path = os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.json")
    for c in json.load(open(path)):
        msa = random_msa(np.random.default_rng(c["seed"]), c["m"], c["n"], **c["kw"])
        if c.get("gapped") and c["seed"] == 10:
            msa[:, 0] = np.arange(c["m"]) % 4 + ord("E")
        assert hashlib.sha256(msa.tobytes()).hexdigest() == c["msa_sha256"]
        if c.get("nonelastic"):
            if c.get("gapped"):
                v = engine.gapped_v(msa)
                s, prev, b = engine.gapped_dp(v)
            else:
                v = engine.repeatfree_v(msa)
                s, prev, b = engine.repeatfree_dp(v)
            assert digest(v) == c["v"] and digest(s) == c["s"] and digest(prev) == c["prev"]
            assert (None if b is None else b.tolist()) == c["boundaries"]
        else:
            f = engine.elastic_f(msa, ignorechars=c.get("ignore", ""))
            b, mml, bt = engine.minmax_dp(f, full=True)
            assert (f.tolist() if isinstance(c["f"], list) else digest(f)) == c["f"]
            assert digest(mml) == c["mml"] and digest(bt) == c["bt"] and digest(b) == c["boundaries"]
            assert len(b) == c["n_blocks"] and int(mml[-1]) == c["optimal"]


def test_synthetic_generator_matches_host_spec(engine):
    """fbg_msa_synthetic == the splitmix64 spec of SURVEY.md 8(d), including gap runs and N cells."""
    import torch

    def sm(x):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    m, n, run = 7, 501, 16
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.msa_synthetic(d.data_ptr(), m, n, gap_fraction=0.05, gap_run=run, n_fraction=0.01)
    engine.sync()
    got = d.cpu().numpy().reshape(m, n)
    c = np.arange(m * n, dtype=np.uint64).reshape(m, n)
    with np.errstate(over="ignore"):
        base = np.frombuffer(b"ACGT", dtype=np.uint8)[(sm(np.uint64(0x5EED0001) + c) >> np.uint64(62)).astype(np.int64)]
        start = sm(np.uint64(0x5EED0002) + c) < np.uint64(int((1 << 64) * (0.05 / run)))
        isn = sm(np.uint64(0x5EED0003) + c) < np.uint64(int((1 << 64) * 0.01))
    gap = np.zeros((m, n), dtype=bool)
    for i, j in np.argwhere(start):
        gap[i, j:j + run] = True
    exp = np.where(gap, ord("-"), np.where(isn, ord("N"), base)).astype(np.uint8)
    assert np.array_equal(got, exp)


def test_full_size_properties(engine):
    """BASELINE C3 shape (1000 x 1,000,000, iid) and C2 shape (64 x 100,000 non-elastic) at full size:
    properties that do not need the oracle -- f in range, shards == whole, every block at least its
    minimal valid width, both sweeps (wave-parallel and literal) identical, v[] in range."""
    import os
    import torch
    m, n = 1000, 1_000_000
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    engine.msa_synthetic(d.data_ptr(), m, n)
    engine.msa_set_device(d.data_ptr(), m, n)
    engine.index_build()
    d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_g = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    engine.scan_f(0, n, d_f.data_ptr())
    for k in range(4):                                   # four column shards
        engine.scan_f(n * k // 4, n * (k + 1) // 4, d_g.data_ptr())
    engine.sync()
    assert torch.equal(d_f, d_g)
    x = torch.arange(n, device="cuda")
    assert bool((d_f >= x).all()) and bool((d_f <= n - 1).all()) and int(d_f[0]) == 0
    d_b = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_mml = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_bt = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = engine.minmax_dp_device(d_f.data_ptr(), n, d_b.data_ptr(), d_mml.data_ptr(), d_bt.data_ptr())
    b = d_b[:cnt].clone()
    assert int(b[-1]) == n and bool((b[1:] > b[:-1]).all())
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), b[:-1] + 1])
    ends = torch.cat([b[:-1], torch.tensor([n - 1], device="cuda")])
    assert bool((d_f[starts] <= ends).all())             # every block is semi-repeat-free
    assert int((ends - starts + 1).max()) == int(d_mml[n])
    with fbg_options(engine, {"FBG_DP_LITERAL": "1"}):   # statement-by-statement sweep of fbg.cpp:1968-2014
        d_b2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_mml2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_bt2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        cnt2 = engine.minmax_dp_device(d_f.data_ptr(), n, d_b2.data_ptr(), d_mml2.data_ptr(), d_bt2.data_ptr())
    assert cnt2 == cnt and torch.equal(d_mml, d_mml2) and torch.equal(d_bt, d_bt2) and torch.equal(d_b[:cnt], d_b2[:cnt])
    del d, d_g
    # C2: 64 x 100,000 non-elastic
    m2, n2 = 64, 100_000
    d2 = torch.empty(m2 * n2, dtype=torch.uint8, device="cuda")
    engine.msa_synthetic(d2.data_ptr(), m2, n2)
    engine.msa_set_device(d2.data_ptr(), m2, n2)
    engine.index_build(reversed=True)
    d_v = torch.empty(n2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    engine.scan_v(0, n2, d_v.data_ptr())
    d_b = torch.empty(n2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = engine.repeatfree_dp_device(d_v.data_ptr(), n2, d_b.data_ptr())
    j = torch.arange(n2, device="cuda")
    assert bool((d_v <= j + 1).all())
    vv = d_v[d_v <= j]                                   # where a valid block exists the left end never moves back
    assert vv.numel() > 0 and bool((vv[1:] >= vv[:-1]).all())
    b = d_b[:cnt]
    assert int(b[-1]) == n2 - 1
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), b[:-1] + 1])
    assert bool((starts <= d_v[b]).all())                # block [start..end] is repeat-free iff start <= v[end]


def _scan_whole(eng, n, reversed=False):
    import torch
    d = torch.zeros(n, dtype=torch.int64, device="cuda")        # f is max-merged into (fbg.cpp:1681): start from zeros
    torch.cuda.synchronize()
    (eng.scan_v if reversed else eng.scan_f)(0, n, d.data_ptr())
    eng.sync()
    return d


@pytest.mark.parametrize("config", ["C3", "C5", "C2"])
def test_full_size_independent_paths_agree(config):
    """BASELINE configs at FULL size, each through two structurally different scans that share no scan kernel:
    C3 (1000 x 1,000,000 elastic): rank-order scan of the packed sort words (rank_scan.hip) against the record path
    (prefix-doubling suffix sort, 16-byte records in text order, scan.hip); C5 (256 x 2,000,000, gaps + N): scan in
    suffix order on column spans (gapped_rank.hip) against the record path; C2 (64 x 100,000 non-elastic): v[] likewise
    on the reversed text.  The sampled thresholds, their verification and the regime switches all depend on the size:
    this is the check that they change nothing (fbg.cpp:1579-1695, 552-611).  index_kind: 1 rank order, 2 suffix order
    with gaps, 0 records."""
    import torch
    import founderblockgraphs_amd as F
    with F.Engine(0) as eng:
        if config == "C3":
            m, n, kw, build, fast, alt = 1000, 1_000_000, {}, {}, 1, {"no_ranked": 1}
        elif config == "C5":
            m, n, kw, build, fast, alt = 256, 2_000_000, dict(gap_fraction=0.05, gap_run=16, n_fraction=0.001), dict(ignorechars="N"), 2, {"gapped_rank": -1}
        else:
            m, n, kw, build, fast, alt = 64, 100_000, {}, dict(reversed=True), 1, {"no_ranked": 1}
        rev = bool(build.get("reversed"))
        d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
        eng.msa_synthetic(d.data_ptr(), m, n, **kw)
        eng.msa_set_device(d.data_ptr(), m, n)
        eng.index_build(**build)
        assert eng.get_option("index_kind") == fast
        a = _scan_whole(eng, n, rev)
        with eng.options(**alt):
            eng.index_build(**build)
            assert eng.get_option("index_kind") == 0             # per-position records
            b = _scan_whole(eng, n, rev)
        assert torch.equal(a, b), (config, torch.nonzero(a != b)[:5].flatten().tolist())
        if config == "C5":                                       # ... and with the elastic tricks off (fbg.cpp:1605-1608)
            eng.index_build(**build)
            a2 = torch.zeros(n, dtype=torch.int64, device="cuda")
            b2 = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            eng.scan_f(0, n, a2.data_ptr(), True)
            eng.sync()
            with eng.options(**alt):
                eng.index_build(**build)
                eng.scan_f(0, n, b2.data_ptr(), True)
                eng.sync()
            assert torch.equal(a2, b2) and not torch.equal(a, a2)


@pytest.mark.parametrize("max_len", [1, 3, 20, 31, 40, 100, 126, 200, 400])
def test_nonelastic_dp_random_v(engine, max_len):
    """s[]/prev[]/boundaries of fbg.cpp:616-664 for arbitrary v[] (valid, invalid and non-monotone entries):
    block-matrix path for short blocks, statement-by-statement kernel beyond its window."""
    rng = np.random.default_rng(900 + max_len)
    for n in (1, 2, 64, 65, 700, 3000):
        j = np.arange(n)
        v = np.maximum(0, j + 1 - rng.integers(1, max_len + 1, n))        # block [v..j] of 1..max_len columns
        v = np.where(rng.random(n) < 0.1, j + 1, v).astype(np.uint64)       # 10% of the ends have no valid block
        s, prev, b = O.segment_dp(v)
        gs, gprev, gb = engine.repeatfree_dp(v)
        assert np.array_equal(gs, s), (n, np.flatnonzero(gs != s)[:5])
        assert np.array_equal(gprev, prev), (n, np.flatnonzero(gprev != prev)[:5])
        assert (b is None) == (gb is None)
        if b is not None:
            assert np.array_equal(gb, b)


@pytest.mark.parametrize("kw", [dict(), dict(similar=0.97), dict(gap_p=0.01, gap_run=8), dict(gap_p=0.01, gap_run=8, records=1)],
                         ids=["iid", "similar", "gaps", "gaps-records"])
def test_large_text_index_arrays(engine, kw):
    """Texts above 2^20 symbols (packed compact keys for the iid rows, group-level scan for the similar ones, the scan in
    suffix order of gapped_rank.hip for the rows with gaps, and the record path for them): index arrays and f must
    equal the oracle's."""
    rng = np.random.default_rng(77)
    kw = dict(kw)
    engine.set_option("gapped_rank", -1 if kw.pop("records", 0) else 0)
    msa = random_msa(rng, 48, 24000, **kw)
    T, SA, ISA, LCP = O.msa_index(msa)
    engine.msa_load_host(msa)
    engine.index_build()
    engine.set_option("gapped_rank", 0)
    gT, gSA, gISA, gPL, gPR = engine.index_download()
    assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
    assert np.array_equal(gISA.astype(np.int64), ISA.astype(np.int64))
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
    assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])
    again = engine.index_download()                      # same index, second read-out: must be bit-identical
    assert all(np.array_equal(x, y) for x, y in zip((gT, gSA, gISA, gPL, gPR), again))
    assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa))


ALT_PATHS = [
    {"FBG_NO_RANKED": "1"},                          # record path even for gap-free MSAs
    {"FBG_NO_RANKED": "1", "FBG_LCP_TEXT": "1"},     # ... with Kasai text comparison instead of key-derived LCPs
    {"FBG_FULL_KEYS": "1"},                          # 64-bit keys instead of entropy-sized ones
    {"FBG_RANK_NO_THRESHOLD": "1"},                  # rank-order scan without the sampled threshold
    {"FBG_PURE_SCAN": "1"},                          # group-level scan for similar rows (pure_scan.hip) whatever the input
    {"FBG_PURE_SCAN": "1", "FBG_NO_PACKED": "1"},    # ... on (key, position) pairs
    {"FBG_PURE_SCAN": "1", "FBG_MSD_MIN": "1"},      # ... behind the three-pass MSD sort
    {"FBG_NO_PACKED": "1"},                          # rank-order scan on (key, position) pairs instead of packed words
    {"FBG_NO_PACKED": "1", "FBG_FULL_KEYS": "1"},
    {"FBG_FORCE_WIDE": "1"},                         # ... on wide pairs (the layout for texts beyond 2^32 symbols)
    {"FBG_MSD_MIN": "1"},                            # three-pass MSD sort (msd_sort.hip) also for small texts
    {"FBG_NO_MSD_SORT": "1"},                        # rocPRIM's onesweep instead of it
    {"FBG_MSD_MIN": "1", "FBG_NO_RANKED": "1"},      # record path behind the three-pass sample sort of (key, position) pairs
    {"FBG_BP_MIN": "1"},                             # records reach their text positions through splitting passes ...
    {"FBG_BP_MIN": "1", "FBG_NO_RANKED": "1"},       # ... also for gap-free MSAs
    {"FBG_RECORD_SCATTER": "1"},                     # ... or by a direct scatter whatever the size
    {"FBG_GAPPED_RANK": "-1"},                       # record path for the MSAs with gaps / ignore characters (default: gapped_rank.hip)
    {"FBG_GAPPED_RANK": "-1", "FBG_BP_MIN": "1"},
    {"FBG_GAPPED_RANK": "-1", "FBG_MSD_MIN": "1"},
    {"FBG_MSD_MIN": "1", "FBG_MSD_SAMPLE_BINS": "1"},  # sample sort whose finish bins by sampled keys instead of symbol ranks
    {"FBG_MSD_MIN": "1", "FBG_MSD_MIN_FORCE": "1", "FBG_NO_RANKED": "1"},   # the sample sort of pairs also where rows resemble each other
    {"FBG_GAPPED_RANK": "-1", "FBG_MSD_MIN": "1", "FBG_MSD_SAMPLE_BINS": "1"},
    {"FBG_DP_WAVE": "1"},                            # wave-parallel sweep instead of the matrix chain
    {"FBG_DP_TILE": "1"},                            # 8-steps-per-iteration sweep
    {"FBG_DP_LITERAL": "1"},                         # statement-by-statement sweeps
]


@pytest.mark.parametrize("env", ALT_PATHS, ids=["+".join(sorted(e)) for e in ALT_PATHS])
def test_alternative_paths_stay_bit_identical(engine, env):
    """Every fallback / alternative code path of the engine must give the oracle's answer too."""
    import os
    rng = np.random.default_rng(4242)
    cases = [random_msa(rng, 20, 900, similar=0.96), random_msa(rng, 64, 400), random_msa(rng, 7, 1500, alphabet="AC", similar=0.99),
             random_msa(rng, 15, 700, gap_p=0.02, gap_run=5, n_p=0.01)]
    with fbg_options(engine, env):
        for msa in cases:
            f = O.compute_f(msa, ignore="N")
            g = engine.elastic_f(msa, ignorechars="N")
            assert np.array_equal(g, f)
            mml, bt, b = O.minmax_dp(f)
            gb, gmml, gbt = engine.minmax_dp(g, full=True)
            assert np.array_equal(gmml, mml) and np.array_equal(gbt, bt) and np.array_equal(gb, b)
            if ord("-") not in msa:
                assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa))       # no ignore chars: rank-order scan
                v = O.segment_v(msa)
                gv = engine.repeatfree_v(msa)
                assert np.array_equal(gv, v)
                s, prev, bb = O.segment_dp(v)
                gs, gprev, gbb = engine.repeatfree_dp(gv)
                assert np.array_equal(gs, s) and np.array_equal(gprev, prev)
                assert (bb is None) == (gbb is None) and (bb is None or np.array_equal(gbb, bb))


def _partitioned(engines, n, reversed=False, ignorechars="", tricks_off=False):
    """fbg_part_* with the partitions of a multi-GPU job played by several contexts on one GPU: what
    distributed.partitioned_index does, with torch.cat / torch.maximum standing in for the two collectives.
    Returns the list of per-partition verdicts after each phase."""
    import torch
    from founderblockgraphs_amd._lib import PART_HALO_BYTES
    P = len(engines)
    blobs = torch.zeros(P * PART_HALO_BYTES, dtype=torch.uint8, device="cuda")
    gm = [torch.zeros(n + 1, dtype=torch.int32, device="cuda") for _ in range(P)]
    torch.cuda.synchronize()
    ok1 = [e.part_index_build(r, P, blobs.data_ptr() + r * PART_HALO_BYTES, reversed, ignorechars, tricks_off) for r, e in enumerate(engines)]
    for e in engines:
        e.sync()
    ok2 = [e.part_scan(blobs.data_ptr(), gm[r].data_ptr()) for r, e in enumerate(engines)]
    for e in engines:
        e.sync()
    red = gm[0]
    for g in gm[1:]:
        red = torch.maximum(red, g)
    torch.cuda.synchronize()
    ok3 = [e.part_finish(red.data_ptr()) for e in engines]
    if all(v == 2 for v in ok3):                      # a threshold was not cleared everywhere: exact re-scan, reduce again
        for r, e in enumerate(engines):
            e.part_rescan(gm[r].data_ptr())
            e.sync()
        red = gm[0]
        for g in gm[1:]:
            red = torch.maximum(red, g)
        torch.cuda.synchronize()
        ok3 = [e.part_finish(red.data_ptr()) for e in engines]
    assert all(v in (0, 1) for v in ok3) and len(set(ok3)) == 1, ok3
    return ok1, ok2, [v == 1 for v in ok3]


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_index_matches_oracle(P):
    """Key-range partitioned index (multi-GPU path): f and v from P partitions == the oracle's."""
    import torch
    from founderblockgraphs_amd import Engine
    rng = np.random.default_rng(40 + P)
    engines = [Engine() for _ in range(P)]
    try:
        for (m, n, kw) in [(24, 500, {}), (50, 300, dict(alphabet="AC")), (9, 2500, dict(alphabet="ACGTN")),
                           (40, 400, dict(similar=0.5))]:
            msa = random_msa(rng, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
            ok1, ok2, ok3 = _partitioned(engines, n)
            assert all(ok1) and all(ok2) and all(ok3), (m, n, kw, ok1, ok2, ok3)
            f = O.compute_f(msa)
            for tricks_off in (False, True):
                exp = O.compute_f(msa, disable_tricks=tricks_off)
                d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                engines[P - 1].scan_f(0, n, d_f.data_ptr(), tricks_off)     # any rank can finish: the maxima are global
                engines[P - 1].sync()
                assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), exp)
            # non-elastic: reversed rows
            ok1, ok2, ok3 = _partitioned(engines, n, reversed=True)
            assert all(ok1) and all(ok2) and all(ok3)
            d_v = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engines[0].scan_v(0, n, d_v.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_v.cpu().numpy().astype(np.uint64), O.segment_v(msa))
            del f
    finally:
        for e in engines:
            e.close()


def test_partitioned_index_declines_consistently():
    """Inputs the partitioned path does not take (gaps while the scan in suffix order is switched off, near-identical rows,
    tiny partitions): every partition must report the same verdict after the collectives, and nothing may claim a usable index."""
    import torch
    from founderblockgraphs_amd import Engine, FbgError
    rng = np.random.default_rng(77)
    engines = [Engine() for _ in range(3)]
    try:
        for (m, n, kw) in [(12, 300, dict(gap_p=0.05, gap_run=3)), (100, 300, dict(similar=0.999)), (2, 40, {})]:
            msa = random_msa(rng, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
                e.set_option("gapped_rank", -1 if "gap_p" in kw else 0)
            ok1, ok2, ok3 = _partitioned(engines, n)
            for e in engines:
                e.set_option("gapped_rank", 0)
            assert not any(ok2) and not any(ok3), (kw, ok1, ok2, ok3)
            d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
            with pytest.raises(FbgError):
                engines[0].scan_f(0, n, d_f.data_ptr())
            # the fall-back every rank takes
            engines[0].index_build()
            torch.cuda.synchronize()
            engines[0].scan_f(0, n, d_f.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), O.compute_f(msa))
    finally:
        for e in engines:
            e.close()


def test_partitioned_index_full_size():
    """C3 shape (1000 x 1,000,000): four key-range partitions give exactly the f of the whole index."""
    import torch
    from founderblockgraphs_amd import Engine
    m, n, P = 1000, 1_000_000, 4
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    engines = [Engine() for _ in range(P)]
    try:
        engines[0].msa_synthetic(d.data_ptr(), m, n)
        for e in engines:
            e.msa_set_device(d.data_ptr(), m, n)
        ok1, ok2, ok3 = _partitioned(engines, n)
        assert all(ok1) and all(ok2) and all(ok3)
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_g = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engines[1].scan_f(0, n, d_f.data_ptr())
        engines[1].sync()
        engines[0].index_build()
        engines[0].scan_f(0, n, d_g.data_ptr())
        engines[0].sync()
        assert torch.equal(d_f, d_g)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("env", [{}, {"FBG_NO_PACKED": "1"}, {"FBG_FORCE_WIDE": "1"}, {"FBG_RANK_NO_THRESHOLD": "1"}, {"FBG_MSD_MIN": "1"},
                                 {"FBG_PURE_SCAN": "1"}],
                         ids=["packed", "pairs", "wide", "nothreshold", "msdsort", "purescan"])
def test_rank_scan_sampled_regime_matches_oracle(engine, env):
    """Texts above 2^22 symbols use the sampled threshold and regime test of the rank-order scan: f and v must
    still be the oracle's, for iid rows and for rows with shared stretches (ties, runs, short suffixes)."""
    import os
    rng = np.random.default_rng(99)
    a = random_msa(rng, 150, 30000)
    b = random_msa(rng, 150, 30000, similar=0.6)
    with fbg_options(engine, env):
        for msa in (a, b):
            assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa))
            assert np.array_equal(engine.repeatfree_v(msa), O.segment_v(msa))


@pytest.mark.parametrize("pure", [0, 1], ids=["slots", "groups"])
@pytest.mark.parametrize("alphabet", ["A", "AC", "ACGT", "ACGTN"])
def test_rank_scan_short_rows_and_heavy_ties(engine, alphabet, pure):
    """Rows shorter than a key, tiny alphabets, repeated rows: every suffix is 'short' or tied.  Index arrays and
    f / v against the oracle (exercises the separator coding, tie ordering from the suffix start, runs) -- with the
    slot-level scan and with the group-level one (pure_scan.hip: mixed groups, short members, the key-0 group)."""
    with fbg_options(engine, {"FBG_PURE_SCAN": str(pure)}):
        _short_rows_and_heavy_ties(engine, alphabet)


def _short_rows_and_heavy_ties(engine, alphabet):
    rng = np.random.default_rng(len(alphabet))
    for (m, n, kw) in [(3, 1, {}), (4, 2, {}), (6, 5, {}), (9, 13, {}), (12, 40, {}), (5, 200, dict(similar=0.9)),
                       (40, 30, dict(similar=0.7)), (70, 64, {}), (8, 700, dict(similar=0.98))]:
        msa = random_msa(rng, m, n, alphabet=alphabet, **kw)
        T, SA, ISA, LCP = O.msa_index(msa)
        engine.msa_load_host(msa)
        engine.index_build()
        gT, gSA, gISA, gPL, gPR = engine.index_download()
        assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64)), (alphabet, m, n)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
        assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])
        assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa)), (alphabet, m, n)
        exp = O.compute_f(msa, disable_tricks=True)
        if exp[0] != n:                                  # otherwise the engine reports "no valid segmentation"
            assert np.array_equal(engine.elastic_f(msa, disable_efg_tricks=True), exp)
        assert np.array_equal(engine.repeatfree_v(msa), O.segment_v(msa)), (alphabet, m, n)


@pytest.mark.parametrize("shape", [(200, 20000, 0.01), (1000, 4000, 0.002), (60, 60000, 0.05)], ids=["star200", "star1000", "star60"])
def test_similar_rows_group_scan_matches_oracle(engine, shape):
    """Star phylogeny (one iid ancestor, every cell substituted with probability p): the sample sends these to the
    group-level scan (pure_scan.hip) by itself; f and the sweep against the oracle.  A repeat is planted in the ancestor
    so that mixed groups (members from two columns) of hundreds of suffixes exist too."""
    m, n, p = shape
    rng = np.random.default_rng(m)
    anc = rng.integers(0, 4, n)
    anc[n // 2:n // 2 + 300] = anc[n // 5:n // 5 + 300]           # a 300-symbol repeat
    cells = np.where(rng.random((m, n)) < p, rng.integers(0, 4, (m, n)), anc)
    msa = np.frombuffer(b"ACGT", dtype=np.uint8)[cells]
    f = O.compute_f(msa, threads=8)
    g = engine.elastic_f(msa)
    assert np.array_equal(g, f), np.flatnonzero(g != f)[:10]
    mml, bt, b = O.minmax_dp(f)
    gb, gmml, gbt = engine.minmax_dp(g, full=True)
    assert np.array_equal(gb, b) and np.array_equal(gmml, mml) and np.array_equal(gbt, bt)
    assert np.array_equal(engine.repeatfree_v(msa), O.segment_v(msa))


def test_partitioned_index_wide_layout():
    """The slot layout of texts beyond 2^32 symbols (high position bits in the key word), forced on small inputs."""
    import os
    import torch
    from founderblockgraphs_amd import Engine
    rng = np.random.default_rng(314)
    engines = [Engine() for _ in range(3)]
    for e in engines:
        e.set_option("force_wide", 1)
    try:
        for (m, n, kw) in [(24, 500, {}), (50, 300, dict(alphabet="AC")), (40, 400, dict(similar=0.5))]:
            msa = random_msa(rng, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
            ok1, ok2, ok3 = _partitioned(engines, n)
            assert all(ok1) and all(ok2) and all(ok3), (m, n, kw, ok1, ok2, ok3)
            d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engines[0].scan_f(0, n, d_f.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), O.compute_f(msa))
    finally:
        for e in engines:
            e.close()


def test_partitioned_index_beyond_32bit_positions():
    """550 x 8,000,000: a text of 4.4e9 symbols, more than 32-bit positions hold.  The key-range partitioned index
    (4 partitions, wide slots) must give the f of the row-group-pair plan, whose pair texts fit 32 bits
    (distributed.py: exact by construction, checked against the oracle at small sizes)."""
    import torch
    from founderblockgraphs_amd import Engine
    from founderblockgraphs_amd import distributed as D
    m, n, P = 550, 8_000_000, 4
    assert m * (n + 1) + 1 > (1 << 32)
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    engines = [Engine() for _ in range(P)]
    try:
        engines[0].msa_synthetic(d.data_ptr(), m, n)
        for e in engines:
            e.msa_set_device(d.data_ptr(), m, n)
        ok1, ok2, ok3 = _partitioned(engines, n)
        assert all(ok1) and all(ok2) and all(ok3), (ok1, ok2, ok3)
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engines[2].scan_f(0, n, d_f.data_ptr())
        engines[2].sync()
    finally:
        for e in engines:
            e.close()
    # reference: pairs of row groups, each pair's text below 2^32 symbols
    G, groups, plan = D.plan_row_pairs(m, n, 1)
    d_g = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_rows = torch.empty(max((groups[a][1] - groups[a][0]) + (groups[b][1] - groups[b][0]) for a, b in plan[0]) * n,
                         dtype=torch.uint8, device="cuda")
    eng = Engine()
    try:
        for a, b in plan[0]:
            off = 0
            for g in (a, b):
                r0, r1 = groups[g]
                d_rows[off * n:(off + r1 - r0) * n].copy_(d[r0 * n:r1 * n])
                off += r1 - r0
            torch.cuda.synchronize()
            eng.msa_set_device(d_rows.data_ptr(), off, n)
            eng.index_build()
            eng.scan_f(0, n, d_g.data_ptr())
            eng.sync()
    finally:
        eng.close()
    assert G >= 2 and torch.equal(d_f, d_g)


def test_msd_sort_gives_the_suffix_array(engine):
    """The three-pass MSD sort (forced on a 1.2e6-symbol text): suffix array, inverse, LCPs and f equal the oracle's;
    at C3 size the f it leads to equals the one reached through rocPRIM's sort."""
    import os
    import torch
    rng = np.random.default_rng(123)
    msa = random_msa(rng, 48, 24000)
    T, SA, ISA, LCP = O.msa_index(msa)
    with fbg_options(engine, {"FBG_MSD_MIN": "1"}):
        engine.msa_load_host(msa)
        engine.index_build()
        gT, gSA, gISA, gPL, gPR = engine.index_download()
        assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
        assert np.array_equal(engine.elastic_f(msa), O.compute_f(msa))
    m, n = 1000, 1_000_000
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    engine.msa_synthetic(d.data_ptr(), m, n)
    engine.msa_set_device(d.data_ptr(), m, n)
    fs = []
    for env in ({}, {"FBG_NO_MSD_SORT": "1"}):
        with fbg_options(engine, env):
            engine.index_build()
            d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engine.scan_f(0, n, d_f.data_ptr())
            engine.sync()
            fs.append(d_f)
    assert torch.equal(fs[0], fs[1])


def test_streamed_upload_equals_plain_upload(engine):
    """fbg_elastic_f from memory of fbg_host_alloc sends the rows up in chunks and starts the build on those that are there
    (text, pass 1 of the MSD sort on the alphabet the first chunk promises): same f as with the whole MSA uploaded first --
    also when a later chunk breaks the promise (a new symbol, a gap) and the build starts over."""
    import ctypes as C
    from founderblockgraphs_amd import _lib
    m, n = 64, 600_000
    rng = np.random.default_rng(99)
    L = _lib.lib()
    p = L.fbg_host_alloc(m * n)
    assert p
    try:
        pinned = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(m, n))
        base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, n))]
        for variant in ("plain", "late_symbol", "late_gap"):
            np.copyto(pinned, base)
            if variant == "late_symbol":
                pinned[m - 1, 12345] = ord("N")
            if variant == "late_gap":
                pinned[m - 2, 777:790] = ord("-")
            with fbg_options(engine, {"no_stream_upload": 1}):
                ref = engine.elastic_f(pinned)
                assert engine.get_option("pass1_ahead") == 0
            got = engine.elastic_f(pinned)
            assert np.array_equal(got, ref), variant
            assert engine.get_option("pass1_ahead") == (1 if variant == "plain" else 0), variant
            if variant == "plain":
                assert engine.get_option("msd_decline") == 0
    finally:
        L.fbg_host_free(C.c_void_p(p))


def _block_graph_reference(msa, boundaries):
    """output_efg's numbering (fbg.cpp:1224-1260) with plain Python dicts: node_of, first_node, rep_row, edges."""
    m, n = msa.shape
    nb = len(boundaries)
    node_of = np.full((nb, m), 0xffffffff, dtype=np.uint32)
    first = np.zeros(nb + 1, dtype=np.uint64)
    reps, edges = [], []
    nodecount, prev = 0, 0
    for j, end in enumerate(boundaries):
        cur, r, e = {}, [], set()
        for i in range(m):
            lab = bytes(c for c in msa[i, prev:min(int(end) + 1, n)] if c != ord("-"))
            if not lab:
                continue
            if lab not in cur:
                cur[lab] = nodecount
                nodecount += 1
                r.append(i)
            node_of[j, i] = cur[lab]
            if j > 0 and node_of[j - 1, i] != 0xffffffff:
                e.add((int(node_of[j - 1, i]), cur[lab]))
        first[j + 1] = nodecount
        reps.append(r)
        edges.append(sorted(e))
        prev = int(end) + 1
    return node_of, first, reps, edges


@pytest.mark.parametrize("case", range(8))
def test_block_graph_matches_reference_numbering(engine, case):
    """fbg_block_graph (nodes / edges of the xGFA) against the reference's hashing restated with dicts."""
    rng = np.random.default_rng(900 + case)
    m, n, kw = [(5, 60, {}), (40, 500, dict(similar=0.97)), (64, 300, dict(similar=0.9, gap_p=0.05, gap_run=6)),
                (257, 200, dict(similar=0.99, gap_p=0.02, gap_run=30)), (1000, 150, dict(similar=0.98)),
                (3, 40, dict(gap_p=0.3, gap_run=10)),
                (5000, 90, dict(similar=0.97, gap_p=0.01, gap_run=4)),      # more than 4096 rows: the labels grouped in device memory
                (4097, 60, dict(similar=0.5))][case]
    msa = random_msa(rng, m, n, **kw)
    cuts = np.sort(rng.choice(np.arange(0, n - 1), size=min(n // 4, 40), replace=False)).astype(np.uint64)
    boundaries = np.concatenate([cuts, [n]]).astype(np.uint64)           # last entry is n (fbg.cpp:2026-2039)
    engine.msa_load_host(msa)
    node_of, first, rep_row, ecount, edges = engine.block_graph(boundaries)
    r_node, r_first, r_reps, r_edges = _block_graph_reference(msa, boundaries)
    assert np.array_equal(first, r_first)
    assert np.array_equal(node_of, r_node)
    for j in range(len(boundaries)):
        cnt = int(first[j + 1] - first[j])
        assert list(rep_row[j, :cnt]) == r_reps[j]
        got = [(int(x) >> 32, int(x) & 0xffffffff) for x in edges[j, :int(ecount[j])]]
        assert got == r_edges[j], j


@pytest.mark.parametrize("layout", ["wide", "packed"])
@pytest.mark.parametrize("P", [2, 3])
def test_partitioned_index_msd_sort_of_pairs(P, layout):
    """msd_sort_pairs.hip (the partitions' three-pass sort of 12-byte slots, or of packed 8-byte words), forced on small
    inputs: long keys so that the bucket function has its 27 bits of resolution."""
    import os
    import torch
    from founderblockgraphs_amd import Engine
    rng = np.random.default_rng(555 + P)
    env = {"FBG_FULL_KEYS": "1", "FBG_MSD_MIN": "1"}
    if layout == "wide":
        env["FBG_FORCE_WIDE"] = "1"
    engines = [Engine() for _ in range(P)]
    for e in engines:
        for k, v in env.items():
            e.set_option(k[4:].lower(), int(v))
    try:
        for (m, n, kw) in [(24, 500, {}), (50, 300, dict(alphabet="AC")), (9, 2500, dict(alphabet="ACGTN")), (40, 400, dict(similar=0.5))]:
            msa = random_msa(rng, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
            ok1, ok2, ok3 = _partitioned(engines, n)
            assert all(ok1) and all(ok2) and all(ok3), (m, n, kw, ok1, ok2, ok3)
            d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engines[0].scan_f(0, n, d_f.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), O.compute_f(msa))
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("alphabet", ["AAACGT", "ACGTACGTACGTN", "AC"], ids=["skewed", "rareN", "binary"])
def test_msd_sort_capacity_fallback_is_seamless(engine, alphabet):
    """Texts large enough for the MSD sort whose keys do NOT spread evenly (skewed composition, a rare fifth symbol, a
    binary alphabet): bucket capacities overflow or the geometry does not fit, the engine must end up with the same f
    as with rocPRIM's sort -- and with the oracle's on a smaller cut of the same rows."""
    import os
    import torch
    rng = np.random.default_rng(2024)
    m, n = 180, 100_000                                   # 1.8e7 symbols: above the 2^24 threshold
    msa = random_msa(rng, m, n, alphabet=alphabet)
    got = []
    for env in ({}, {"FBG_NO_MSD_SORT": "1"}):
        with fbg_options(engine, env):
            got.append(engine.elastic_f(msa))
    assert np.array_equal(got[0], got[1])
    small = msa[:40, :4000]
    with fbg_options(engine, {"FBG_MSD_MIN": "1"}):
        assert np.array_equal(engine.elastic_f(small), O.compute_f(small))


def test_sample_sort_decline_on_a_fresh_context():
    """A FRESH context (every run of the host program is one): the sample sort of the (key, position) pairs reserves
    its larger buffers and then declines in its first pass -- one key shared by 1.6e5 suffixes (rows that end in the
    same long run of one symbol) overflows a bucket stretch.  The fall-back must pack into the buffers as they are
    NOW (round 2 packed through pointers taken before the reserve: a write into freed memory that the session-wide
    engine of the other tests, whose buffers no longer move, could not show)."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(606)
    m, n = 40, 8000
    msa = random_msa(rng, m, n, gap_p=0.01, gap_run=3)
    msa[:, n // 2:] = ord("A")
    f_ref = O.compute_f(msa)
    for force in (1, 0):
        with F.Engine(0) as e:
            e.set_option("msd_min", 1)
            e.set_option("msd_min_force", force)
            assert np.array_equal(e.elastic_f(msa), f_ref), force
            T, SA, ISA, LCP = O.msa_index(msa)
            e.set_option("gapped_rank", -1)                       # the record path's arrays: SA as the oracle has it
            e.msa_load_host(msa)
            e.index_build()
            gSA = e.index_download()[1]
            assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64)), force


# ---- non-elastic mode with gaps: segment2elasticValid (fbg.cpp:738-866) ------------------------------------

def _check_gapped(engine, msa, literal=False):
    v = O.gapped_v(msa, literal=literal)
    gv = engine.gapped_v(msa)
    assert np.array_equal(gv, v)
    s, prev, b = O.segment2_dp(v)
    gs, gprev, gb = engine.gapped_dp(gv)
    assert np.array_equal(gs, s) and np.array_equal(gprev, prev)
    assert (b is None) == (gb is None)
    if b is not None:
        assert np.array_equal(gb, b)
    return b


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_fixtures_gapped_nonelastic(engine, name):
    msa = O.msa_array(FIXTURES[name])
    assert _check_gapped(engine, msa, literal=True) is None      # the heuristic finds nothing for the reference's fixtures


@pytest.mark.parametrize("case", range(10))
def test_random_gapped_nonelastic(engine, case):
    rng = np.random.default_rng(700 + case)
    m, n, kw = [(2, 15, dict(gap_p=0.1)), (4, 200, dict(gap_p=0.05, gap_run=3)), (64, 700, dict(gap_p=0.02, gap_run=8)),
                (10, 500, dict(similar=0.9, gap_p=0.03, gap_run=4)), (3, 400, dict(alphabet="AC", gap_p=0.05)),
                (1, 50, dict(gap_p=0.2)), (100, 300, dict(similar=0.97, gap_p=0.01, gap_run=20)), (5, 1, {}),
                (40, 3000, {}), (200, 2500, dict(gap_p=0.004, gap_run=16))][case]
    msa = random_msa(rng, m, n, **kw)
    _check_gapped(engine, msa, literal=m * n <= 4000)


def test_gapped_nonelastic_small_exhaustive(engine):
    """Tiny inputs with many gaps, empty rows and repeats: the cases where a segmentation exists must be among them."""
    rng = np.random.default_rng(77)
    solved = 0
    for it in range(300):
        m, n = int(rng.integers(1, 7)), int(rng.integers(1, 15))
        alpha = ["AC", "ACGT", "A"][it % 3]
        msa = random_msa(rng, m, n, alphabet=alpha, gap_p=[0.0, 0.1, 0.3][it % 3 if it % 2 else 0])
        solved += _check_gapped(engine, msa, literal=True) is not None
    assert solved > 20


def test_gapped_dp_on_arbitrary_v(engine):
    """The recurrence alone, on v arrays the scan would never produce: far lookbacks (beyond the LDS ring of the
    kernel), columns without a block in the middle, n around the tile size, v[0] = 0."""
    rng = np.random.default_rng(78)
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 20000, 70000):
        for mode in range(5):
            j = np.arange(n, dtype=np.int64)
            if mode == 0:      # short blocks, first block from column 0
                v = np.maximum(0, j - rng.integers(0, 6, n))
                v[: min(n, 4)] = 0
            elif mode == 1:    # monotone like the real thing, long blocks
                v = np.maximum.accumulate(np.maximum(0, j - rng.integers(0, 300, n)))
                v[: min(n, 300)] = 0
            elif mode == 2:    # holes: columns where no block ends
                v = np.maximum(0, j - rng.integers(0, 20, n))
                v[rng.random(n) < 0.3] = n + 5
                v[: min(n, 2)] = 0
            elif mode == 3:    # far lookbacks
                v = np.maximum(0, j - rng.integers(0, 30000, n))
            else:              # nothing works
                v = j + 1
            v = v.astype(np.uint64)
            s, prev, b = O.segment2_dp(v)
            gs, gprev, gb = engine.gapped_dp(v)
            assert np.array_equal(gs, s) and np.array_equal(gprev, prev), (n, mode)
            assert (b is None) == (gb is None)
            if b is not None:
                assert np.array_equal(gb, b)


def test_gapped_nonelastic_large(engine):
    """C5-shaped input (gap runs of 16 over 5 % of the cells) at a size the oracle still does in seconds, and the
    v derivation at a larger one against the same derivation in numpy from the engine's own f."""
    rng = np.random.default_rng(79)
    msa = random_msa(rng, 64, 60000, gap_p=0.05 / 16, gap_run=16)
    _check_gapped(engine, msa)
    msa = random_msa(rng, 128, 400000, gap_p=0.05 / 16, gap_run=16)
    n = msa.shape[1]
    gv = engine.gapped_v(msa)
    import founderblockgraphs_amd as Fm
    try:
        F = engine.elastic_f(msa, disable_efg_tricks=True)
    except Fm.NoSegmentation:        # f[0] == n (fbg.cpp:1932-1937): not with this input
        F = None
    assert F is not None
    if F is not None:
        best = np.full(n, -1, dtype=np.int64)
        ok = F < n
        np.maximum.at(best, F[ok].astype(np.int64), np.nonzero(ok)[0])
        run = np.maximum.accumulate(best)
        exp = np.where(run >= 0, run, np.arange(n) + 1).astype(np.uint64)
        assert np.array_equal(gv, exp)
    s, prev, b = O.segment2_dp(gv)
    gs, gprev, gb = engine.gapped_dp(gv)
    assert np.array_equal(gs, s) and np.array_equal(gprev, prev)
    assert (b is None) == (gb is None) and (b is None or np.array_equal(gb, b))


@pytest.mark.parametrize("sort", ["rocprim", "samplesort"])
def test_records_by_position_passes(engine, sort):
    """The record path's way back from suffix order to text order (k_bp_groups0 / k_bp_split / k_bp_leaf): index arrays
    against the oracle with the passes forced on small texts, and a gapped MSA large enough to take them by itself --
    behind rocPRIM's sort and behind the three-pass sample sort of the pairs (msd_sort_pairs.hip, MODE 1)."""
    import os
    rng = np.random.default_rng(31)
    switches = {"FBG_BP_MIN": "1", "FBG_NO_RANKED": "1", "FBG_GAPPED_RANK": "-1"}
    switches["FBG_MSD_MIN" if sort == "samplesort" else "FBG_NO_MSD_SORT"] = "1"
    with fbg_options(engine, switches):
        for (m, n, kw) in [(7, 1300, dict(gap_p=0.03, gap_run=5)), (33, 257, dict(similar=0.95)), (3, 3000, dict(alphabet="AC", similar=0.99)),
                           (65, 1290, dict(alphabet="ACGTN")), (2, 4097, {}), (9, 70000, dict(gap_p=0.01, gap_run=3))]:
            msa = random_msa(rng, m, n, **kw)
            T, SA, ISA, LCP = O.msa_index(msa)
            engine.msa_load_host(msa)
            engine.index_build()
            gT, gSA, gISA, gPL, gPR = engine.index_download()
            assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64)), (m, n)
            assert np.array_equal(gISA.astype(np.int64), ISA.astype(np.int64)), (m, n)
            lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
            assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA]), (m, n)
            assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1]), (m, n)
    msa = random_msa(rng, 24, 800000, gap_p=0.05 / 16, gap_run=16, n_p=0.001)      # 1.9 * 10^7 symbols > 2^24
    want = O.compute_f(msa, ignore="N", threads=8)
    with fbg_options(engine, {"FBG_NO_MSD_SORT": "1", "FBG_GAPPED_RANK": "-1"} if sort == "rocprim" else {"FBG_GAPPED_RANK": "-1"}):
        assert np.array_equal(engine.elastic_f(msa, ignorechars="N"), want)
        assert engine.get_option("index_kind") == 0
    with fbg_options(engine, {"FBG_NO_MSD_SORT": "1"} if sort == "rocprim" else {}):       # and the scan in suffix order behind the same sort
        assert np.array_equal(engine.elastic_f(msa, ignorechars="N"), want)
        assert engine.get_option("index_kind") == 2


def _long_gaps(rng, msa):
    """rows that start late, end early or skip a long stretch"""
    m, n = msa.shape
    for i in rng.choice(m, size=max(1, m // 3), replace=False):
        kind = int(rng.integers(3))
        w = int(rng.integers(1, max(2, n // 2)))
        a0 = 0 if kind == 0 else n - w if kind == 1 else int(rng.integers(0, n - w))
        msa[i, a0:a0 + w] = ord("-")
    return msa


@pytest.mark.parametrize("case", range(8))
def test_gapped_rank_scan_matches_oracle(engine, case):
    """MSAs with gaps and / or ignore characters through the scan in suffix order (gapped_rank.hip): f with and
    without the elastic tricks (the second is a re-scan of the kept slots), the max-merge into a given f, column shards,
    the index arrays read back from the slots, long gap runs (a position that is its row's pointer for hundreds of columns)."""
    import torch
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(900 + case)
    m, n, kw, ign, long_gaps = [
        (12, 900, dict(gap_p=0.02, gap_run=5, n_p=0.01), "N", False),
        (64, 400, dict(gap_p=0.05, gap_run=2), "", True),
        (5, 3000, dict(alphabet="AC", gap_p=0.01, gap_run=30), "", True),
        (30, 700, dict(n_p=0.03), "N", False),                                   # no gaps at all: ignore characters only
        (17, 1200, dict(similar=0.9, gap_p=0.01, gap_run=8, n_p=0.005), "N", True),
        (130, 257, dict(alphabet="ACGTRYKM", gap_p=0.3, gap_run=1), "RY", False),
        (3, 100, dict(gap_p=0.05, gap_run=20), "", True),
        (40, 2000, dict(gap_p=0.005, gap_run=4, n_p=0.001), "N", True)][case]
    msa = random_msa(rng, m, n, **kw)
    if long_gaps:
        msa = _long_gaps(rng, msa)
    assert (msa != ord("-")).sum(axis=1).min() > 0
    for off in (False, True):
        want = O.compute_f(msa, ignore=ign, disable_tricks=off)
        try:
            got = engine.elastic_f(msa, ignorechars=ign, disable_efg_tricks=off)
            assert np.array_equal(got, want), (off, np.flatnonzero(got != want)[:8])
        except F.NoSegmentation:
            assert want[0] == n
        assert engine.get_option("index_kind") == 2
    f0 = rng.integers(0, n, n).astype(np.uint64)
    want = O.compute_f(msa, ignore=ign, f_init=f0)
    assert np.array_equal(engine.elastic_f(msa, ignorechars=ign, f=f0), want)
    # staged calls: one index, both settings of the tricks in turn, shards
    engine.msa_load_host(msa)
    engine.index_build(ignorechars=ign)
    for off in (True, False, True):
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for k in range(3):
            engine.scan_f(n * k // 3, n * (k + 1) // 3, d_f.data_ptr(), disable_efg_tricks=off)
        engine.sync()
        assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), O.compute_f(msa, ignore=ign, disable_tricks=off))
    T, SA, ISA, LCP = O.msa_index(msa)
    gT, gSA, gISA, gPL, gPR = engine.index_download()
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64)) and np.array_equal(gISA.astype(np.int64), ISA.astype(np.int64))
    assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA]) and np.array_equal(gPR.astype(np.int64), lcp_ext[ISA.astype(np.int64) + 1])
    assert np.array_equal(engine.gapped_v(msa), O.gapped_v(msa))       # segment2elasticValid: f without the tricks underneath


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_gapped_index_matches_oracle(P):
    """Key-range partitions of an MSA with gaps / ignore characters (fbg_part_index_build_ignore; the scan in suffix order
    of gapped_rank.hip per partition, edge slots and column maxima exchanged): f with and without the elastic tricks,
    with the threshold forced on (option gapped_rank=4: columns redone through fbg_part_rescan) and without."""
    import torch
    from founderblockgraphs_amd import Engine
    rng = np.random.default_rng(8800 + P)
    engines = [Engine() for _ in range(P)]
    try:
        cases = [(40, 700, dict(gap_p=0.02, gap_run=5, n_p=0.01), "N", False), (64, 400, dict(gap_p=0.05, gap_run=2), "", True),
                 (12, 3000, dict(alphabet="AC", gap_p=0.01, gap_run=30), "", True), (130, 300, dict(n_p=0.03), "N", False),
                 (30, 1500, dict(gap_p=0.005, gap_run=4, n_p=0.002), "N", True)]
        took = 0
        for forced in (0, 4):
            for e in engines:
                e.set_option("gapped_rank", forced)
            for (m, n, kw, ign, long_gaps) in cases:
                msa = random_msa(rng, m, n, **kw)
                if long_gaps:
                    msa = _long_gaps(rng, msa)
                for e in engines:
                    e.msa_load_host(msa)
                for off in (False, True):
                    ok1, ok2, ok3 = _partitioned(engines, n, ignorechars=ign, tricks_off=off)
                    if not (all(ok1) and all(ok2) and all(ok3)):
                        continue                          # declined (a partition of fewer than 128 slots, a run beyond the halo)
                    took += 1
                    want = O.compute_f(msa, ignore=ign, disable_tricks=off)
                    d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    engines[P - 1].scan_f(0, n, d_f.data_ptr(), disable_efg_tricks=off)
                    engines[P - 1].sync()
                    got = d_f.cpu().numpy().astype(np.uint64)
                    assert np.array_equal(got, want), (P, forced, m, n, kw, off, np.flatnonzero(got != want)[:8])
        assert took >= 8
    finally:
        for e in engines:
            e.close()


def test_many_rows_with_gaps_take_the_record_path(engine):
    """More rows than the window table's 16-bit row field holds (65535 and more): the scan in suffix order steps aside,
    the per-cell tables of the record path are built on demand."""
    rng = np.random.default_rng(66)
    msa = random_msa(rng, 66000, 24, gap_p=0.03, gap_run=2)
    assert (msa != ord("-")).sum(axis=1).min() > 0
    got = engine.elastic_f(msa)
    assert engine.get_option("index_kind") == 0
    assert np.array_equal(got, O.compute_f(msa, threads=8))


def test_gapped_v_on_a_partitioned_index():
    """segment2elasticValid's v[] (fbg_scan_gapped_v) from the key-range partitioned index of a multi-GPU job: the
    scan without tricks reads the all-reduced column maxima exactly as fbg_scan_f does."""
    import torch
    from founderblockgraphs_amd import Engine
    rng = np.random.default_rng(4711)
    engines = [Engine() for _ in range(2)]
    try:
        for (m, n, kw) in [(30, 700, {}), (64, 400, dict(alphabet="AC")), (12, 1500, dict(similar=0.5))]:
            msa = random_msa(rng, m, n, **kw)
            for e in engines:
                e.msa_load_host(msa)
            ok1, ok2, ok3 = _partitioned(engines, n)
            if not (all(ok1) and all(ok2) and all(ok3)):
                continue                                  # declined (similar rows): the caller falls back, nothing to check
            d_v = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engines[0].scan_gapped_v(d_v.data_ptr())
            engines[0].sync()
            assert np.array_equal(d_v.cpu().numpy().astype(np.uint64), O.gapped_v(msa)), (m, n, kw)
    finally:
        for e in engines:
            e.close()


# ---- similar rows WITH gaps / ignore characters: the group-level scan on column spans (span_scan.hip) -----------------

def star_msa(rng, m, n, sub=0.01, gap_cells=0.02, gap_run=8, n_p=0.0, shared=0.0, lead=0, alphabet="ACGT"):
    """A star phylogeny: one random ancestor, every row substitutes each position with probability `sub`; `gap_cells` of
    the cells lie in gap runs of `gap_run` (each row its own; `shared`: that fraction of the runs is copied into a third
    of the rows -- deletions common to many rows, as in a real pangenome); `lead`: some rows start / end with gaps."""
    alpha = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    anc = alpha[rng.integers(0, len(alpha), n)]
    a = np.tile(anc, (m, 1))
    mut = rng.random((m, n)) < sub
    a[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    if n_p > 0:
        a[rng.random((m, n)) < n_p] = ord("N")
    if gap_cells > 0:
        for i, j in np.argwhere(rng.random((m, n)) < gap_cells / gap_run):
            a[i, j:j + gap_run] = ord("-")
            if shared > 0 and rng.random() < shared:
                rows = rng.random(m) < 0.33
                a[rows, j:j + gap_run] = ord("-")
    for i in range(m):
        if lead and rng.random() < 0.3:
            a[i, :rng.integers(1, lead + 1)] = ord("-")
        if lead and rng.random() < 0.3:
            a[i, n - rng.integers(1, lead + 1):] = ord("-")
    return a


SPAN_CASES = [
    dict(m=200, n=20000, gap_cells=0.02, gap_run=8),
    dict(m=1000, n=4000, gap_cells=0.03, gap_run=12),
    dict(m=60, n=5000, gap_cells=0.05, gap_run=30, lead=40),
    dict(m=120, n=6000, gap_cells=0.01, gap_run=4, n_p=0.002),
    dict(m=300, n=3000, gap_cells=0.02, gap_run=6, shared=0.5),
    dict(m=40, n=3000, gap_cells=0.0, n_p=0.004),                       # rows without gaps, ignore characters only
    dict(m=25, n=900, gap_cells=0.04, gap_run=5, sub=0.0),              # identical rows up to the gaps
    dict(m=16, n=1200, gap_cells=0.03, gap_run=7, alphabet="AC", sub=0.002, lead=9),   # long repeats by chance: strays in the groups
    dict(m=1, n=700, gap_cells=0.05, gap_run=3),
    dict(m=3, n=64, gap_cells=0.2, gap_run=2, lead=5),
    dict(m=1100, n=1500, gap_cells=0.02, gap_run=6, shared=0.1),         # groups of more than 1024 members: the chains, the slow list
    dict(m=900, n=2500, gap_cells=0.02, gap_run=8, sub=0.003),           # groups of 897 .. 1024 members
    dict(m=2100, n=800, gap_cells=0.01, gap_run=6),                      # groups of 1025 .. 2048 members (k_sp_odd_pairs_big<64, 1024>)
    dict(m=3000, n=400, gap_cells=0.005, gap_run=5, sub=0.002),          # ... 2049 .. 4096 members
    dict(m=4500, n=250, gap_cells=0.004, gap_run=4, sub=0.001),          # ... 4097 .. 8192 members (one workgroup per CU)
]


@pytest.mark.parametrize("key_flags", [0, 1])
@pytest.mark.parametrize("case", range(len(SPAN_CASES)))
def test_span_scan_matches_oracle(engine, case, key_flags):
    """Star-phylogeny rows with gap runs -- the shape of a pangenome MSA -- through the group-level scan on column spans
    (option span_scan = 1 takes it whatever the size; at scale the sample of the sort decides): f with and without
    --ignore-chars, with the elastic tricks on and off, in 3 column shards; against the oracle (fbg.cpp:1579-1695,
    esp. 1687-1691: the pointer that waits through a gap run).  key_flags = 1: in the slot layout of MSAs with 2^30
    cells and more (the reference's size_type is 64 bits wide, fbg.cpp:47: no limit of that kind there)."""
    import torch
    kw = dict(SPAN_CASES[case])
    m, n = kw.pop("m"), kw.pop("n")
    msa = star_msa(np.random.default_rng(9000 + case), m, n, **kw)
    with fbg_options(engine, {"span_scan": 1, "span_key_flags": key_flags}):
        for ignore in ("", "N"):
            if ignore == "" and ord("N") in msa and case != 3:
                continue
            f_on, f_off = O.compute_f(msa, ignore=ignore), O.compute_f(msa, ignore=ignore, disable_tricks=True)
            engine.msa_load_host(msa)
            engine.index_build(ignorechars=ignore)
            if ord("-") in msa or ignore:
                assert engine.get_option("span_scan_used") == 1 and engine.get_option("index_kind") == 2, (case, ignore)
                assert engine.get_option("span_key_flags_used") == key_flags
            for tricks_off, ref in ((False, f_on), (True, f_off), (False, f_on)):
                d = torch.zeros(n, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                for r in range(3):
                    engine.scan_f(n * r // 3, n * (r + 1) // 3, d.data_ptr(), tricks_off)
                engine.sync()
                got = d.cpu().numpy().astype(np.uint64)
                bad = np.flatnonzero(got != ref)
                assert bad.size == 0, (case, ignore, tricks_off, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


def test_one_engine_builds_every_index_kind_in_sequence():
    """One Engine builds, one after the other, a span-scan index with the flags in the key words, a gapped index, a
    gap-free rank-order index and a record-path index: what a build leaves in the context (which index it holds, how
    its sort laid the slots out) must not reach the next one.  Every f against the oracle (fbg.cpp:1579-1695), every
    index_kind against the kind the options ask for."""
    import torch
    import founderblockgraphs_amd as F
    star = star_msa(np.random.default_rng(9100), 16, 1200, gap_cells=0.03, gap_run=7)
    gapped = random_msa(np.random.default_rng(9101), 12, 900, gap_p=0.02, gap_run=5, n_p=0.01)
    gapfree = random_msa(np.random.default_rng(9102), 24, 700)
    steps = [("span", star, "", {"span_scan": 1, "span_key_flags": 1}, 2, 1),
             ("gapped", gapped, "N", {"span_scan": -1}, 2, 0),
             ("ranked", gapfree, "", {}, 1, 0),
             ("record", gapfree, "", {"no_ranked": 1}, 0, 0)]
    with F.Engine(0) as eng:
        for name, msa, ignore, opts, kind, span in steps:
            n = msa.shape[1]
            want = O.compute_f(msa, ignore=ignore)
            with fbg_options(eng, opts):
                eng.msa_load_host(msa)
                eng.index_build(ignorechars=ignore)
                assert eng.get_option("index_kind") == kind, name
                assert eng.get_option("span_scan_used") == span and eng.get_option("span_key_flags_used") == span, name
                d = torch.zeros(n, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                eng.scan_f(0, n, d.data_ptr(), False)
                eng.sync()
            got = d.cpu().numpy().astype(np.uint64)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def test_one_engine_runs_every_owner_of_the_scalar_words_in_two_orders():
    """Every stage that keeps counters or flags in the context's shared scalar words (FbgScalars, fbg_internal.h), on one
    Engine, in two different orders, each result against the oracle both times: a word that two stages share, or that a
    stage reads where another one left something, shows up as a wrong result in one of the orders.  The steps: a gap-free
    build through the MSD sort and the slot-level scan (with the check of the candidate order), similar rows through the
    group-level scan, a key-range partition (the count of the slots it keeps), rows with gaps and ignore characters through
    the sample sort of pairs and the scan in suffix order (counting pass with front_one_fill = 0: its counts in the scalar
    words, its histogram in `small`), the scan on column spans, the record path (records by position, then scan_f with its
    exception columns), the three DPs and the block graph.  Every step asserts from get_option that the path it is
    there for ran.  (The rank scan's histogram and the lean scan's pair statistics exist above 2^22 symbols only:
    test_rank_scan_sampled_regime_matches_oracle, test_scan_tail.py.)"""
    import torch
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(9200)
    unlike = random_msa(rng, 40, 3000)                      # (the smallest shape of test_msd_cursors.py)
    similar = random_msa(rng, 16, 3000, similar=0.97)
    small = random_msa(rng, 16, 2000)
    gapped = random_msa(rng, 12, 3000, gap_p=0.02, gap_run=5, n_p=0.01)
    star = star_msa(rng, 16, 2000, gap_cells=0.03, gap_run=7)
    f_unlike, f_similar, f_small = O.compute_f(unlike), O.compute_f(similar), O.compute_f(small)
    f_gapped, f_star = O.compute_f(gapped, ignore="N"), O.compute_f(star)
    v_unlike, v_gapped = O.segment_v(unlike), O.gapped_v(gapped)
    dp_minmax, dp_repeatfree, dp_gapped = O.minmax_dp(f_unlike), O.segment_dp(v_unlike), O.segment2_dp(v_gapped)
    cuts = np.concatenate([np.arange(40, 2000, 50), [2000]]).astype(np.uint64)
    graph = _block_graph_reference(star, cuts)

    def build_and_scan(eng, msa, ignore, opts, want, check):
        n = msa.shape[1]
        with fbg_options(eng, opts):
            eng.msa_load_host(msa)
            eng.index_build(ignorechars=ignore)
            check()
            d = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            eng.scan_f(0, n, d.data_ptr(), False)
            eng.sync()
        got = d.cpu().numpy().astype(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())

    def kind(eng, want, span=0):
        assert eng.get_option("index_kind") == want and eng.get_option("span_scan_used") == span

    def msd_rank(eng):
        def ran():
            kind(eng, 1)
            assert eng.get_option("msd_decline") == 0 and eng.get_option("cand_inversions") == 0
        build_and_scan(eng, unlike, "", {"msd_min": 1, "pure_scan": -1, "cand_sort_check": 1}, f_unlike, ran)

    def pure(eng):       # (pure_scan = 1: the slot-level scan is not tried, so a ranked index is the group-level scan's)
        build_and_scan(eng, similar, "", {"pure_scan": 1}, f_similar, lambda: kind(eng, 1))

    def partition(eng):
        n = small.shape[1]
        eng.msa_load_host(small)
        ok1, ok2, ok3 = _partitioned([eng], n)
        assert all(ok1) and all(ok2) and all(ok3), (ok1, ok2, ok3)
        assert eng.get_option("index_kind") == 3
        d = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.scan_f(0, n, d.data_ptr())
        eng.sync()
        assert np.array_equal(d.cpu().numpy().astype(np.uint64), f_small)

    def gapped_scan(eng):
        def ran():
            kind(eng, 2)
            assert eng.get_option("pairs_rb") >= 0
        build_and_scan(eng, gapped, "N", {"span_scan": -1, "msd_min": 1, "front_one_fill": 0}, f_gapped, ran)

    def span(eng):
        build_and_scan(eng, star, "", {"span_scan": 1}, f_star, lambda: kind(eng, 2, span=1))

    def record(eng):
        build_and_scan(eng, small, "", {"no_ranked": 1, "bp_min": 1}, f_small, lambda: kind(eng, 0))

    def minmax(eng):
        mml, bt, b = dp_minmax
        gb, gmml, gbt = eng.minmax_dp(f_unlike, full=True)
        assert np.array_equal(gb, b) and np.array_equal(gmml, mml) and np.array_equal(gbt, bt)

    def nonelastic(eng, call, v, want):
        s, prev, b = want
        gs, gprev, gb = call(v)
        assert np.array_equal(gs, s) and np.array_equal(gprev, prev)
        assert (b is None) == (gb is None) and (b is None or np.array_equal(gb, b))

    def repeatfree(eng):
        nonelastic(eng, eng.repeatfree_dp, v_unlike, dp_repeatfree)

    def gapped_dp(eng):
        nonelastic(eng, eng.gapped_dp, v_gapped, dp_gapped)

    def block_graph(eng):
        eng.msa_load_host(star)
        node_of, first, rep_row, ecount, edges = eng.block_graph(cuts)
        r_node, r_first, r_reps, r_edges = graph
        assert np.array_equal(first, r_first) and np.array_equal(node_of, r_node)
        for j in range(len(cuts)):
            assert list(rep_row[j, :int(first[j + 1] - first[j])]) == r_reps[j]
            assert [(int(x) >> 32, int(x) & 0xffffffff) for x in edges[j, :int(ecount[j])]] == r_edges[j], j

    steps = [msd_rank, minmax, record, pure, repeatfree, partition, gapped_scan, gapped_dp, span, block_graph]
    other = [span, gapped_dp, pure, msd_rank, block_graph, record, minmax, gapped_scan, partition, repeatfree]
    assert sorted(s.__name__ for s in steps) == sorted(s.__name__ for s in other)
    with F.Engine(0) as eng:
        for order in (steps, other):
            for step in order:
                step(eng)


def test_span_scan_large_groups_by_chains(engine):
    """Groups of more than 1024 members through the chains along the later keys' groups (option span_scan = 3: the path
    the large instances of k_sp_odd_pairs replaced as the default) -- same f (fbg.cpp:1579-1695)."""
    kw = dict(SPAN_CASES[10])
    m, n = kw.pop("m"), kw.pop("n")
    assert m > 1024
    msa = star_msa(np.random.default_rng(9010), m, n, **kw)
    f_on, f_off = O.compute_f(msa), O.compute_f(msa, disable_tricks=True)
    with fbg_options(engine, {"span_scan": 3}):
        for tricks_off, ref in ((False, f_on), (True, f_off)):
            got = engine.elastic_f(msa, disable_efg_tricks=tricks_off)
            assert (got == ref).all(), (tricks_off, np.flatnonzero(got != ref)[:8].tolist())
        assert engine.get_option("span_scan_used") == 1


def test_span_scan_leaves_many_large_slow_groups_to_the_record_path(engine):
    """More than 1024 identical rows with a few gap runs: every group of the first columns has all its members odd (the
    rows' first symbols) and its chains give up -- thousands of list entries for a few hundred groups, each a second of
    all-pairs comparisons.  By its own choice the library hands such an input to the record path (span_scan_used 0);
    with span_scan = 1 it insists, takes every listed group once, and is still exact (fbg.cpp:1579-1695)."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(424243)
    m, n = 1030, 1200
    anc = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    msa = np.tile(anc, (m, 1))
    for i, j in np.argwhere(rng.random((m, n)) < 0.002):
        msa[i, j:j + 5] = ord("-")
    msa[:, 0] = anc[0]
    f_on, f_off = O.compute_f(msa), O.compute_f(msa, disable_tricks=True)
    for forced in (0, 1):
        with fbg_options(engine, {"span_scan": forced}):
            for tricks_off, ref in ((False, f_on), (True, f_off)):
                try:
                    got = engine.elastic_f(msa, disable_efg_tricks=tricks_off)
                    assert (got == ref).all(), (forced, tricks_off, np.flatnonzero(got != ref)[:8].tolist())
                except F.NoSegmentation:
                    assert tricks_off and ref[0] == n
            if forced:
                assert engine.get_option("span_scan_used") == 1
            else:
                # by its own choice: the record path (no wall-clock bound here -- a busy box would make it flake; what is
                # asserted is the path taken)
                assert engine.get_option("span_scan_used") == 0
                assert engine.get_option("span_slow_groups") <= engine.get_option("span_groups")


def test_span_scan_through_a_group_and_at_scale():
    """(a) the host-buffer group API on a star phylogeny with gaps: two members on one device -- the key-range partitions
    decline such rows, the members scan column shards of the group-level index -- equals the oracle; (b) a text large
    enough that the sample of the sort decides by itself (2^22 symbols and more) and the three-pass sample sort carries the
    cells: equal to the record path's f; (c) the same for 2000 rows."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(515)
    msa = star_msa(rng, 150, 9000, gap_cells=0.02, gap_run=8)
    with F.Group([0, 0]) as grp:
        for mb in range(2):
            grp.member(mb).set_option("span_scan", 1)
        assert np.array_equal(grp.elastic_f(msa), O.compute_f(msa))
        assert grp.plan_used()[0] == "columns"
    big = star_msa(rng, 400, 50000, gap_cells=0.02, gap_run=8)           # 2e7 symbols
    with F.Engine(0) as e:
        a = e.elastic_f(big)
        assert e.get_option("span_scan_used") == 1
        with e.options(span_scan=-1):
            b = e.elastic_f(big)
            assert e.get_option("span_scan_used") == 0
        assert np.array_equal(a, b)
        # (c) more than 1024 rows: groups of 1025 .. 2048 members (k_sp_odd_pairs_big<64, 1024>), the first symbols of 2000
        # rows in one group (nobody coloured with the tricks on, everybody a regular member with the tricks off)
        tall = star_msa(rng, 2000, 12000, gap_cells=0.02, gap_run=8)        # 2.4e7 symbols
        for tricks_off in (False, True):
            a = e.elastic_f(tall, disable_efg_tricks=tricks_off)
            assert e.get_option("span_scan_used") == 1
            with e.options(span_scan=-1):
                b = e.elastic_f(tall, disable_efg_tricks=tricks_off)
                assert e.get_option("span_scan_used") == 0
            assert np.array_equal(a, b), tricks_off


def test_span_scan_beyond_2_30_cells_equals_the_record_path():
    """1000 x 1 100 000 star phylogeny with gaps: 1.1 * 10^9 cells, more than a 30-bit cell number holds.  The reference
    has no limit of that kind (size_type is 64 bits wide, fbg.cpp:47; the pointer that waits through a gap run,
    fbg.cpp:1687-1691, at any size): the group-level scan carries the cell in all 32 bits of the slot's value and the two
    flags in the key word (span_key_flags_used), and gives the f of the record path (option span_scan = -1).  Two columns of
    so long an MSA whose K symbols agree make groups of 2000 members, half of them odd: the slow groups' odd members are
    shared out over 32 workgroups (span_slow_split) -- with 1 the same f."""
    import torch
    import founderblockgraphs_amd as F
    m, n = 1000, 1_100_000
    g = torch.Generator(device="cuda").manual_seed(11)
    anc = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.uint8)
    d = torch.empty((m, n), dtype=torch.uint8, device="cuda")
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    for i0 in range(0, m, 10):
        i1 = min(m, i0 + 10)
        mut = torch.rand((i1 - i0, n), device="cuda", generator=g) < 0.01
        sub = torch.randint(0, 4, (i1 - i0, n), device="cuda", generator=g, dtype=torch.uint8)
        d[i0:i1] = lut[torch.where(mut, sub, anc.expand(i1 - i0, n)).long()]
        start = (torch.rand((i1 - i0, n), device="cuda", generator=g) < 0.02 / 8).float().unsqueeze(1)
        gap = torch.nn.functional.max_pool1d(torch.nn.functional.pad(start, (7, 0)), 8, 1).squeeze(1) > 0
        d[i0:i1][gap] = ord("-")
        del mut, sub, start, gap
    assert (m + 1) * (n + 1) >= 1 << 30
    d = d.reshape(-1)
    got = {}
    with F.Engine(0) as e:
        e.msa_set_device(d.data_ptr(), m, n)
        d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        for name, opts in (("span", {}), ("span, one workgroup per slow group", {"span_slow_split": 1}), ("record path", {"span_scan": -1})):
            with e.options(**opts):
                d_f.zero_()
                torch.cuda.synchronize()
                e.index_build()
                e.scan_f(0, n, d_f.data_ptr())
                e.sync()
                spanned = name != "record path"
                assert e.get_option("span_scan_used") == int(spanned), (name, e.get_option("span_decline"))
                assert e.get_option("span_key_flags_used") == int(spanned), name
                got[name] = d_f.clone()
    for name in got:
        bad = torch.nonzero(got[name] != got["record path"]).flatten()
        assert bad.numel() == 0, (name, bad[:8].tolist())
    assert int(got["span"].max()) > 0
    del d, got
    torch.cuda.empty_cache()


def test_span_scan_decline_hands_the_record_path_a_suffix_array(engine):
    """The group-level scan declines (here: a gap of 5000 columns common to all rows makes a group whose members are coloured
    together over more columns than it walks) AFTER the sort: the cells go back to text positions and the record path goes
    on.  The text has 64 k + 1 symbols, so the sentinel is the first position of its wave in k_sp_cells -- where it took the
    last row's '#' for itself, the suffix array had a position twice, and the text comparison of the record path read beyond
    the text (a memory fault, found by scripts/gpu_fuzz_span.py)."""
    rng = np.random.default_rng(5)
    row = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 63)]
    msa = np.full((3, 5063), ord("-"), dtype=np.uint8)
    msa[:, :10] = row[:10]
    msa[:, 5010:] = row[10:]
    assert (3 * (63 + 1) + 1) % 64 == 1
    for key_flags in (0, 1):           # (1: the declined sort hands back key words without the flag bits, too)
        with fbg_options(engine, {"span_scan": 1, "span_key_flags": key_flags}):
            for tricks_off in (False, True):
                assert np.array_equal(engine.elastic_f(msa, disable_efg_tricks=tricks_off), O.compute_f(msa, disable_tricks=tricks_off))
            assert engine.get_option("span_scan_used") == 0
