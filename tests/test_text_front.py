"""The front of the index build (text_build.hip): the counting pass that writes the optimistic text of a gap-free MSA at 16
bytes per lane (k_row_count_fast, option row_count_fast) against the one it replaces, with the fills, the copy and the
sentinel of option front_one_fill either way.  Whatever the settings: the oracle's f, the oracle's text, suffix array and
LCPs, the same kind of index and the same key geometry."""
import ctypes as C

import numpy as np
import pytest

from conftest import fbg_options
from oracle import pyoracle as O
from test_scan_tail import _check_index

pytestmark = pytest.mark.gpu

M = 9                    # rows: the text's row i is shifted by i bytes against the MSA's, so every shift mod 8 occurs
SEG = 65536              # RC_SEG of text_build.hip: a workgroup counts one segment of this many columns of one row
INFO = ("index_kind", "key_b", "key_K", "key_packed", "key_compact")

_refs = {}


def _msa(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    if name.startswith("n"):                    # iid ACGT, n columns
        return alpha[rng.integers(0, 4, (M, int(name[1:])))]
    if name == "late_N":
        # a symbol the first 64 bytes of its segment do not show: it is outside the guess and goes through count()
        a = alpha[rng.integers(0, 4, (M, 2 * SEG + 8))]
        a[2, 100] = a[5, 100] = a[5, SEG + 70] = a[8, SEG + 70] = ord("N")
        return a
    if name == "seven_symbols":
        # seven distinct symbols in the first 64 bytes of every row: more than the candidate list holds
        a = np.frombuffer(b"ACGTNRY", dtype=np.uint8)[rng.integers(0, 7, (M, SEG + 8))]
        a[:, :7] = np.frombuffer(b"ACGTNRY", dtype=np.uint8)
        return a
    if name == "gap_last":
        # one gap in the last row's last column: the optimistic text is discarded and written again
        a = alpha[rng.integers(0, 4, (M, SEG + 8))]
        a[M - 1, -1] = ord("-")
        return a
    raise KeyError(name)


def _case(name):
    if name not in _refs:
        msa = np.ascontiguousarray(_msa(name))
        T, SA, ISA, LCP = O.msa_index(msa)
        lcp_ext = np.concatenate([LCP, [0]]).astype(np.int64)
        _refs[name] = {"msa": msa, "f": O.compute_f(msa), "T": T, "SA": SA.astype(np.int64), "PL": lcp_ext[ISA],
                       "PR": lcp_ext[ISA.astype(np.int64) + 1]}
    return _refs[name]


# below one segment, one word, one exact segment, a segment less / plus one word, two segments plus one word (every n here is
# 8 mod 16 or 0 mod 16: rows that start at odd multiples of 8 bytes and rows that start at multiples of 16); then n = 65532
# and n = 65531, which take the 4-byte and the 1-byte path of k_row_count whatever the option says
CASES = ["n8", "n64", "n65528", "n65536", "n65544", "n131080", "late_N", "seven_symbols", "gap_last", "n65532", "n65531"]


@pytest.mark.parametrize("name", CASES)
def test_counting_pass_fast_and_plain_give_the_oracles_text_and_f(engine, name):
    ref = _case(name)
    seen = {}
    for fast, one_fill in ((1, 1), (0, 1), (1, 0), (0, 0)):
        with fbg_options(engine, {"row_count_fast": fast, "front_one_fill": one_fill}):
            assert np.array_equal(engine.elastic_f(ref["msa"]), ref["f"]), (fast, one_fill)
            seen[fast, one_fill] = tuple(engine.get_option(k) for k in INFO)
            gT = engine.index_download()[0]
            assert np.array_equal(gT, ref["T"]), (fast, one_fill)
            _check_index(engine, ref)
    print(name, "(row_count_fast, front_one_fill) ->", INFO, seen)
    assert len(set(seen.values())) == 1, seen


def test_streamed_upload_from_pinned_memory(engine):
    """16 x 65536 from memory of fbg_host_alloc: the rows go up in eight chunks of two, each counted by a launch of its own
    (row0), with pass 1 of the sort behind it where the sort takes the text; f and the text as the oracle's with either counting kernel."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    m, n = 16, SEG
    rng = np.random.default_rng(16)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, n))]
    want, want_T = O.compute_f(base), O.msa_index(base)[0]
    p = L.fbg_host_alloc(m * n)
    assert p
    try:
        pinned = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(m, n))
        np.copyto(pinned, base)
        seen = {}
        for fast, one_fill in ((1, 1), (0, 1), (1, 0), (0, 0)):
            with fbg_options(engine, {"row_count_fast": fast, "front_one_fill": one_fill, "msd_min": 1}):
                assert np.array_equal(engine.elastic_f(pinned), want), (fast, one_fill)
                seen[fast, one_fill] = tuple(engine.get_option(k) for k in INFO + ("pass1_ahead",))
                assert np.array_equal(engine.index_download()[0], want_T), (fast, one_fill)
        print("streamed (row_count_fast, front_one_fill) ->", seen)
        assert len(set(seen.values())) == 1, seen
    finally:
        L.fbg_host_free(C.c_void_p(p))
