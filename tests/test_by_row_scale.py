"""Chaining along one MSA row (fbg_pindex_chains_by_row) on the inputs of tests/test_mapping_scale.py: 200 rows and
thousands of reads (`founders`), a tandem repeat whose reads have hundreds to thousands of start places (`repeats`, with
option byrow_max raised to 4096: a read of 3106 places in the tier with its state in device memory), and 16 / 17 / 128
rows, all stranded.  The CPU part asserts what the by-row chains gain over the plain ones, with literal counts: a changed
count means a changed model.  On the GPU every array equals tests/byrow_model.py, and on `founders` the reads that
fbg_pindex_chains_align aligns after the by-row call are the model's and outnumber those after the plain call."""
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import byrow_model as BM  # noqa: E402
import test_chains_by_row as TB  # noqa: E402
import test_mapping_scale as MS  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import fbg_options  # noqa: E402

NONE = BM.NONE
MAX_PLACES = {"repeats": 4096}
# input: virtual reads, plain chains non-empty, of these carried by a row, non-empty chains along one row, of these with
# the plain chain's score
TABLE = {"founders": (8042, 4492, 3174, 4205, 4203), "repeats": (332, 164, 120, 163, 152), "m16": (410, 200, 173, 200, 199),
         "m17": (410, 200, 170, 200, 200), "m128": (410, 200, 166, 200, 200)}


@functools.lru_cache(maxsize=None)
def model(name):
    c = MS.cpu(name)
    return BM.by_row(c, c.band, 0, MAX_PLACES.get(name, 1024))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_what_chaining_by_row_gains(name):
    c, m = MS.cpu(name), model(name)
    plain = np.diff(c.chain_off.astype(np.int64)) > 0
    mine = np.diff(m.chain_off.astype(np.int64)) > 0
    got = (len(c.vreads), int(plain.sum()), int((plain & (c.chain_n_rows > 0)).sum()), int(mine.sum()), int((mine & (m.score == c.score)).sum()))
    assert got == TABLE[name]
    assert (m.score <= c.score).all() and (m.score[c.chain_n_rows > 0] == c.score[c.chain_n_rows > 0]).all()
    assert np.array_equal(m.chain_first_row[mine], m.row[mine]) and (m.chain_n_rows[mine] <= m.n_best_rows[mine]).all()
    assert m.no_row == got[1] - got[3]                      # anchors, and none that a row supports
    if name == "founders":
        assert m.no_row == 287 and int((mine & (m.score == c.score) & (c.chain_n_rows == 0)).sum()) == 1029
    if name == "repeats":
        assert m.places.max() == 3106 and m.too_many == 0 and BM.by_row(c, c.band, 0).too_many > 0


def run(engine, name, align=False):
    c, m = MS.cpu(name), model(name)
    with fbg_options(engine, {"byrow_max": MAX_PLACES.get(name, 1024)}), TR.build(engine, c.A, c.b) as pix:
        sd = pix.seeds(c.reads, min_length=c.L, max_per_seed=c.cap, msa=True, strands=True, rows=True)
        for f in TR.SEED_FIELDS:
            assert np.array_equal(getattr(sd, f), getattr(c, f)), (name, f)
        for f in TR.PLACE_FIELDS:
            assert np.array_equal(getattr(sd.occ, f), getattr(c, f)), (name, f)
        ch = pix.chains(band=c.band, by_row=True, rows=True, align=align)
        TB.same(TB.of_chains(ch), m, name)
        TB.check_stats(pix, m)
        for got, want, f in ((ch.n_rows, m.chain_n_rows, "n_rows"), (ch.first_row, m.chain_first_row, "first_row"), (ch.row_bits, m.row_bits, "bits")):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (name, f)
        assert pix.rows_stats()["chains_unsupported"] == 0
        return pix.by_row_stats(), ch, (pix.align_stats() if align else None)


@pytest.mark.gpu
def test_founders(engine):
    c, m = MS.cpu("founders"), model("founders")
    with mock.patch.object(AM, "LITERAL_CELLS", 0):           # the model's DPs a row at a time in numpy
        am = AM.of_cpu(BM.as_cpu(c, m), 16, 0)
    st, ch, al = run(engine, "founders", align=True)
    assert st["reads_lds"] > 0 and st["reads_too_many"] == 0
    for got, want, f in ((ch.align_row, am.row, "row"), (ch.edits, am.edits, "edits"), (ch.t_start, am.t_start, "t_start"), (ch.t_end, am.t_end, "t_end")):
        assert got.dtype == want.dtype and np.array_equal(got, want), f
    assert al["aligned"] == am.stats["aligned"] == int((am.edits != NONE).sum()) and al["unsupported"] == 0
    assert al["aligned"] == TABLE["founders"][3] > TABLE["founders"][2]


@pytest.mark.gpu
def test_repeats(engine):
    st, ch, _ = run(engine, "repeats")
    assert st["reads_device"] > 0 and st["reads_too_many"] == 0 and st["max_places"] == 4096


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS.MS)
def test_small_row_counts(engine, m):
    run(engine, f"m{m}")
