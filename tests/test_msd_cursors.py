"""Where pass 1 of the MSD sorts keeps its run cursors (option msd_cursors: 1 the cursors of an XCD's buckets side by side,
0 at the stretch's own number; 32-bit words either way): the index and f equal the oracle's under both placements, with one
stretch per bucket and with eight (msd_xcd), where a capacity of pass 1 does not hold, with pass 1 run in pieces during the
upload, in the sample sort of pairs, and in the sort of a key-range partition."""
import ctypes as C

import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

PLACEMENTS = [(cur, xcd) for cur in (1, 0) for xcd in (0, 1, 2, 3)]      # msd_xcd bit 1: eight stretches per bucket, else one


def _index_and_f_equal_oracle(engine, msa, ref, env):
    SA, ISA, lcp_ext, f_ref = ref
    with fbg_options(engine, env):
        engine.msa_load_host(msa)
        engine.index_build()
        assert engine.get_option("msd_decline") == 0, env
        gT, gSA, gISA, gPL, gPR = engine.index_download()
        assert np.array_equal(gSA.astype(np.int64), SA), env
        assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA]), env
        assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA + 1]), env
        assert np.array_equal(engine.elastic_f(msa), f_ref), env


@pytest.mark.parametrize("shape", [(48, 24000), (1000, 12), (600, 20), (40, 3000)])
def test_msd_cursors_index_equals_oracle(engine, shape):
    """Suffix array, both LCP arrays and f under every placement.  48 x 24000 is 141 tiles of pass 1 -- several per stretch,
    the last one partial -- with planted repeats; 1000 x 12 and 600 x 20 pile their row ends up on few buckets; the smallest
    shape also without the extra symbols (another body of pass 1)."""
    m, n = shape
    rng = np.random.default_rng(m * 7919 + n)
    msa = planted_repeats(rng, m, n) if 200 <= n else random_msa(rng, m, n)
    T, SA, ISA, LCP = O.msa_index(msa)
    ref = (SA.astype(np.int64), ISA.astype(np.int64), np.concatenate([LCP, [0]]).astype(np.int64), O.compute_f(msa))
    for ext in ((1, 0) if shape == (40, 3000) else (1,)):
        for cur, xcd in PLACEMENTS:
            _index_and_f_equal_oracle(engine, msa, ref, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext), "FBG_MSD_CURSORS": str(cur),
                                                         "FBG_MSD_XCD": str(xcd)})


def test_msd_cursors_decline_alike(engine):
    """Rows of 80 % A send a third of the keys to the first bucket: its stretches overflow in pass 1 (msd_decline 2: a run did
    not fit, 4: a cursor beyond its stretch; 6 with the 64-bit cursors before this option, whatever msd_xcd; rows of 90 % A do
    not reach the sort, msd_decline 1).  The 32-bit cursors count the slots that did not fit as well: the same verdict under
    every placement, and f from rocPRIM's sort equals the oracle's."""
    rng = np.random.default_rng(90)
    m, n = 64, 8000
    msa = np.where(rng.random((m, n)) < 0.8, ord("A"), np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, (m, n))]).astype(np.uint8)
    f_ref = O.compute_f(msa)
    seen = []
    for cur, xcd in PLACEMENTS:
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_CURSORS": str(cur), "FBG_MSD_XCD": str(xcd)}):
            assert np.array_equal(engine.elastic_f(msa), f_ref), (cur, xcd)
            seen.append(engine.get_option("msd_decline"))
    print("msd_decline per (msd_cursors, msd_xcd):", dict(zip(PLACEMENTS, seen)))
    assert all(v == 6 for v in seen), seen


def test_msd_cursors_pass1_in_pieces(engine):
    """fbg_elastic_f from memory of fbg_host_alloc, 64 x 525000 (just above the 32 MiB from which the rows go up in chunks):
    pass 1 runs in pieces while the rows arrive (a piece starts at a tile other than 0 and adds to the cursors the earlier
    pieces left).  Same f as with the whole MSA uploaded first, under both placements, and the oracle's."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    m, n = 64, 525_000
    rng = np.random.default_rng(64)
    p = L.fbg_host_alloc(m * n)
    assert p
    try:
        pinned = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(m, n))
        np.copyto(pinned, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, n))])
        fs = {}
        for cur in (1, 0):
            for whole in (1, 0):
                with fbg_options(engine, {"FBG_MSD_CURSORS": str(cur), "FBG_NO_STREAM_UPLOAD": str(whole)}):
                    fs[cur, whole] = engine.elastic_f(pinned)
                    assert engine.get_option("msd_decline") == 0, (cur, whole)
                    assert engine.get_option("pass1_ahead") == 1 - whole, (cur, whole)
        for key, f in fs.items():
            assert np.array_equal(f, fs[1, 1]), key
        assert np.array_equal(fs[1, 1], O.compute_f(pinned))
    finally:
        L.fbg_host_free(C.c_void_p(p))


def test_msd_cursors_pairs_sort(engine):
    """An MSA with gap runs and unlike rows takes the sample sort of (key, position) pairs (k_pp_pack_split; "pairs_rb" says
    that it ran): f and v equal the oracle's under every placement."""
    rng = np.random.default_rng(77)
    msa = random_msa(rng, 60, 3000, gap_p=0.02, gap_run=5)
    f_ref, v_ref = O.compute_f(msa), O.gapped_v(msa)
    for cur, xcd in PLACEMENTS:
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_CURSORS": str(cur), "FBG_MSD_XCD": str(xcd)}):
            assert np.array_equal(engine.elastic_f(msa), f_ref), (cur, xcd)
            assert engine.get_option("pairs_rb") >= 0, (cur, xcd)
            assert np.array_equal(engine.gapped_v(msa), v_ref), (cur, xcd)


def test_msd_cursors_partitions():
    """Two key-range partitions played by two contexts on one GPU (the simulation of test_gpu_parity.py), the MSD sort of a
    partition allowed at this size (no option reports whether a partition took it; the tests of the partitioned index at
    full size take it for certain): f equals the oracle's under both placements."""
    import torch
    from founderblockgraphs_amd import Engine
    from test_gpu_parity import _partitioned
    rng = np.random.default_rng(42)
    m, n = 64, 4000
    msa = random_msa(rng, m, n)
    f_ref = O.compute_f(msa)
    engines = [Engine() for _ in range(2)]
    try:
        for cur in (1, 0):
            with fbg_options(engines, {"FBG_MSD_MIN": "1", "FBG_MSD_CURSORS": str(cur)}):
                for e in engines:
                    e.msa_load_host(msa)
                ok1, ok2, ok3 = _partitioned(engines, n)
                assert all(ok1) and all(ok2) and all(ok3), (cur, ok1, ok2, ok3)
                d_f = torch.zeros(n, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                engines[1].scan_f(0, n, d_f.data_ptr())
                engines[1].sync()
                assert np.array_equal(d_f.cpu().numpy().astype(np.uint64), f_ref), cur
    finally:
        for e in engines:
            e.close()
