"""The symbols after the key that the three-pass MSD sort carries (option msd_ext, msd_sort.hip) and the tied pairs the
lean rank-order scan settles from them (k_tie_pairs): same suffix array, LCPs and f as the oracle, with and without."""
import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu


def planted_repeats(rng, m, n, spacing=40):
    """Random ACGT rows; every odd row receives copies of 16..28-symbol stretches of the row above it at other columns,
    so that tied suffixes extend beyond a 17- or 18-symbol key by 0, 1, 2, 3, 4 and more symbols; its last stretch ends
    at the row's end."""
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    msa = A[rng.integers(0, 4, (m, n))].copy()
    for r in range(0, m - 1, 2):
        src, dst = msa[r], msa[r + 1]
        c = 0
        while c < n - 100:
            L = int(rng.integers(16, 29))
            s = int(rng.integers(0, n - L))
            dst[c:c + L] = src[s:s + L]
            c += L + int(rng.integers(spacing // 2, spacing))
        L = int(rng.integers(16, 29))
        s = int(rng.integers(0, n // 2))
        dst[n - L:] = src[s:s + L]
    return msa


@pytest.mark.parametrize("shape", [(48, 24000), (1000, 12), (600, 20), (40, 3000)])
def test_msd_ext_index_equals_oracle(engine, shape):
    """MSD sort forced on small texts (rows shorter than the key plus its 4 extra symbols among them): suffix array,
    LCPs and f equal the oracle's with the extra symbols on and off."""
    m, n = shape
    rng = np.random.default_rng(m * 7919 + n)
    msa = planted_repeats(rng, m, n) if 200 <= n <= 3000 else random_msa(rng, m, n)
    T, SA, ISA, LCP = O.msa_index(msa)
    lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
    f_ref = O.compute_f(msa)
    for ext in (1, 0):
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext)}):
            engine.msa_load_host(msa)
            engine.index_build()
            assert engine.get_option("msd_decline") == 0
            gT, gSA, gISA, gPL, gPR = engine.index_download()
            assert np.array_equal(gSA.astype(np.int64), SA.astype(np.int64))
            assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA])
            assert np.array_equal(engine.elastic_f(msa), f_ref)


def test_msd_ext_planted_repeats_settle_pairs_both_ways(engine):
    """Tied pairs that part within the 4 extra symbols are settled from them, the others (and all of them with msd_ext
    off) by the text; f equals the oracle's either way.  256 x 20000: large enough for the threshold that lets the lean
    scan run (ties in every column), ties rare enough for the slot-level scan."""
    rng = np.random.default_rng(2024)
    msa = planted_repeats(rng, 256, 20000)
    f_ref = O.compute_f(msa)
    seen = {}
    for ext in (1, 0):
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext)}):
            assert np.array_equal(engine.elastic_f(msa), f_ref)
            assert engine.get_option("msd_decline") == 0
            seen[ext] = (engine.get_option("ext_pairs"), engine.get_option("text_pairs"))
    assert seen[1][0] > 0 and seen[1][1] > 0, seen
    assert seen[0][0] == 0 and seen[0][1] > 0, seen


def test_msd_ext_c3_size_f_unchanged(engine):
    """At C3 size (1000 x 10^6, the benchmark's shape) f is the same with the extra symbols, without them, and behind
    rocPRIM's sort."""
    import torch
    m, n = 1000, 1_000_000
    d = torch.empty(m * n, dtype=torch.uint8, device="cuda")
    engine.msa_synthetic(d.data_ptr(), m, n)
    engine.msa_set_device(d.data_ptr(), m, n)
    fs, stats = [], []
    for env in ({"FBG_MSD_EXT": "1"}, {"FBG_MSD_EXT": "0"}, {"FBG_NO_MSD_SORT": "1"}):
        with fbg_options(engine, env):
            engine.index_build()
            d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            engine.scan_f(0, n, d_f.data_ptr())
            engine.sync()
            fs.append(d_f)
            stats.append((engine.get_option("msd_decline"), engine.get_option("ext_pairs"), engine.get_option("text_pairs")))
    assert stats[0][0] == 0 and stats[0][1] > 0, stats
    assert stats[1][1] == 0, stats
    assert torch.equal(fs[0], fs[1])
    assert torch.equal(fs[0], fs[2])
