"""How a thread of pass 1 of the MSD sort takes its 8 items through LDS (option msd_lds_batch: 1 in phases -- the reads of
all items, then their use -- with the text loads in front of the code table and the whole tiles translated without
end-of-text checks; 0 the earlier loops, item by item; passes 2 and 3 are the same kernels under both values): the index and f equal the oracle's under both values, on several
tiles with a partial last one, where row ends overflow sub-buckets into the arena, with and without the extra symbols and
the XCD placements, on texts shorter than a tile and of a length that is no multiple of 8, where pass 1 overflows in some
lanes only, on similar rows (crowded bins of pass 3) and with pass 1 run in pieces during the upload."""
import ctypes as C

import numpy as np
import pytest

from conftest import fbg_options, random_msa
from oracle import pyoracle as O
from test_sort_ext import planted_repeats

pytestmark = pytest.mark.gpu

BATCH = (1, 0)


def _reference(msa):
    T, SA, ISA, LCP = O.msa_index(msa)
    return SA.astype(np.int64), ISA.astype(np.int64), np.concatenate([LCP, [0]]).astype(np.int64), O.compute_f(msa)


def _index_and_f_equal_oracle(engine, msa, ref, env, decline=0):
    SA, ISA, lcp_ext, f_ref = ref
    with fbg_options(engine, env):
        engine.msa_load_host(msa)
        engine.index_build()
        assert engine.get_option("msd_decline") == decline, env
        gT, gSA, gISA, gPL, gPR = engine.index_download()
        assert np.array_equal(gSA.astype(np.int64), SA), env
        assert np.array_equal(gPL.astype(np.int64), lcp_ext[ISA]), env
        assert np.array_equal(gPR.astype(np.int64), lcp_ext[ISA + 1]), env
        assert np.array_equal(engine.elastic_f(msa), f_ref), env
        return engine.text_length()


@pytest.mark.parametrize("shape", [(48, 24000), (1000, 12), (600, 20), (40, 3000), (8, 1024), (37, 1003)])
def test_msd_lds_batch_index_equals_oracle(engine, shape):
    """Suffix array, both LCP arrays and f under both option values.  48 x 24000 is 141 tiles of pass 1, the last one partial,
    with planted repeats; 1000 x 12 and 600 x 20 pile their row ends up on few keys (arena append, k_msd_finish_big);
    40 x 3000 also without the extra symbols and with the XCD placements off; 8 x 1024 is a text of 8201 symbols, shorter
    than a tile and its lookahead (8256): both its tiles take the checked translate, and all but 9 items of the second lie
    beyond the text; 37 x 1003 is a text whose length is no multiple of 8.  (The shortest text this sort takes has about
    8150 symbols: below that the key has 18 bits, which leaves none for pass 3 -- test_msd_lds_batch_short_text.)"""
    m, n = shape
    rng = np.random.default_rng(m * 7919 + n)
    msa = planted_repeats(rng, m, n) if 200 <= n else random_msa(rng, m, n)
    ref = _reference(msa)
    variants = [(ext, xcd) for ext in (1, 0) for xcd in (0, 3)] if shape == (40, 3000) else [(1, 3)]
    for ext, xcd in variants:
        for batch in BATCH:
            N = _index_and_f_equal_oracle(engine, msa, ref, {"FBG_MSD_MIN": "1", "FBG_MSD_EXT": str(ext), "FBG_MSD_XCD": str(xcd),
                                                             "FBG_MSD_LDS_BATCH": str(batch)})
    if shape == (8, 1024):
        assert N < 8192 + 64, N
    if shape == (37, 1003):
        assert N % 8 != 0, N


def test_msd_lds_batch_short_text(engine):
    """8 x 500, a text of 4009 symbols: its key has 9 symbols, the 18 bits of the first two passes, so the geometry does not
    suit this sort under either option value (msd_decline 1, as before the option) and rocPRIM sorts; index and f equal
    the oracle's all the same."""
    rng = np.random.default_rng(8 * 7919 + 500)
    msa = planted_repeats(rng, 8, 500)
    ref = _reference(msa)
    for batch in BATCH:
        _index_and_f_equal_oracle(engine, msa, ref, {"FBG_MSD_MIN": "1", "FBG_MSD_LDS_BATCH": str(batch)}, decline=1)


def test_msd_lds_batch_decline_alike(engine):
    """The overflow input of test_msd_cursors_decline_alike (rows of 80 % A: the stretches of the first bucket overflow in pass
    1, in some lanes of a wave only): msd_decline is 6 under both option values -- the flag raised once per wave behind the
    stores says what the branch inside the loop said -- and f from rocPRIM's sort equals the oracle's."""
    rng = np.random.default_rng(90)
    m, n = 64, 8000
    msa = np.where(rng.random((m, n)) < 0.8, ord("A"), np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, (m, n))]).astype(np.uint8)
    f_ref = O.compute_f(msa)
    seen = []
    for batch in BATCH:
        with fbg_options(engine, {"FBG_MSD_MIN": "1", "FBG_MSD_LDS_BATCH": str(batch)}):
            assert np.array_equal(engine.elastic_f(msa), f_ref), batch
            seen.append(engine.get_option("msd_decline"))
    print("msd_decline per msd_lds_batch:", dict(zip(BATCH, seen)))
    assert all(v == 6 for v in seen), seen


def test_msd_lds_batch_similar_rows(engine):
    """Similar rows forced through this sort: the crowded-bin path of pass 3.  64 noisy copies (1 % of the cells differ) of an
    ancestor of 34000 columns that carries one stretch of 16 symbols at eight places.  Above 2^21 symbols the key has 18
    symbols, 36 bits: 18 for passes 1 and 2, 11 for the bins of pass 3, 7 below them.  The suffixes that start with the
    stretch -- eight columns in some 55 rows each -- share their first 32 key bits, hence one bin, which so holds more than
    the 192 slots a bin counts through and is split on the bits below.  A column's suffixes tie in at most 64 rows, which
    the slot-level scan (pure_scan = -1) still settles; under pure_scan = 1 the group-level scan reads the same sorted
    slots.  f equals the oracle's under both option values and both scans, this sort is the one that sorted, and under
    pure_scan = 1 the index is a ranked one (index_kind 1), i.e. f came from the slots this sort wrote."""
    rng = np.random.default_rng(320)
    m, n, L = 64, 34000, 16
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = A[rng.integers(0, 4, n)]
    stretch = A[rng.integers(0, 4, L)]
    places = 2000 + 4000 * np.arange(8)
    for c in places:
        anc[c:c + L] = stretch
    msa = np.tile(anc, (m, 1))
    mut = rng.random((m, n)) > 0.99
    msa[mut] = A[rng.integers(0, 4, int(mut.sum()))]
    crowd = sum(int(np.all(msa[:, c:c + 15] == stretch[:15], axis=1).sum()) for c in places)
    assert crowd > 192, crowd                                     # slots of one bin (15 symbols: 30 bits >= the 29 of a bin)
    f_ref = O.compute_f(msa)
    for pure in (-1, 1):
        for batch in BATCH:
            with fbg_options(engine, {"msd_min": 1, "pure_scan": pure, "msd_lds_batch": batch}):
                assert np.array_equal(engine.elastic_f(msa), f_ref), (pure, batch)
                assert engine.get_option("msd_decline") == 0, (pure, batch)
                kind = engine.get_option("index_kind")
                print("pure_scan", pure, "msd_lds_batch", batch, "index_kind", kind)
                if pure == 1:
                    assert kind == 1, (pure, batch, kind)
                    key_bits = engine.get_option("key_K") * engine.get_option("key_b")
                    assert 1 <= key_bits - 18 - 11 <= 10, key_bits    # key bits below the bins: crowded bins are split on them


def test_msd_lds_batch_pass1_in_pieces(engine):
    """fbg_elastic_f from memory of fbg_host_alloc, 64 x 525000: pass 1 runs in pieces while the rows arrive (pass1_ahead = 1;
    a piece starts at a tile other than 0 and holds only tiles whose lookahead has arrived: whole ones, without the checks).
    Same f with the option on and off, and the oracle's."""
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
        for batch in BATCH:
            with fbg_options(engine, {"FBG_MSD_LDS_BATCH": str(batch)}):
                fs[batch] = engine.elastic_f(pinned)
                assert engine.get_option("msd_decline") == 0, batch
                assert engine.get_option("pass1_ahead") == 1, batch
        assert np.array_equal(fs[1], fs[0])
        assert np.array_equal(fs[1], O.compute_f(pinned))
    finally:
        L.fbg_host_free(C.c_void_p(p))
