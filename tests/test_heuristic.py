"""The row-chunk mode (--heuristic-subset=ROWNUM): chunked scan, the pattern index of a segmentation built on the device
(fbg_pindex_build_segmentation), validation and repair of a segmentation (fbg_segmentation_validate / _repair), the
Python entry segment_elastic_heuristic and the command line.

CPU part: tests/heuristic_model.py against the definition, and the command-line refusals.
GPU part: everything exact, against the host-assembled index (graph_from_segmentation + pattern_index) and the model.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import heuristic_model as HM
import validate_model as VM
from conftest import random_msa
from fasta_util import write_fasta
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "founderblockgraphs_amd", "founderblockgraph")
VALIDATE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_validate")
GOLD = os.path.join(ROOT, "tests", "golden")

GAPPY = dict(similar=0.95, gap_p=0.02, gap_run=3)
# (m, n, rows per chunk, random_msa arguments, seed, repair rounds the model takes)
CASES = [
    (12, 96, 3, dict(similar=0.9), 93, 0),
    (6, 40, 3, dict(alphabet="AC"), 1, 0),
    (8, 64, 2, {}, 0, 1),
    (16, 128, 4, GAPPY, 0, 1),
    (8, 64, 2, {}, 111, 2),
    (12, 96, 3, dict(similar=0.9), 58, 2),
    (16, 128, 4, GAPPY, 120, 2),
    (6, 40, 3, dict(alphabet="AC"), 140, 2),
]
CASE_IDS = [f"{m}x{n}-R{r}-seed{s}" for m, n, r, _, s, _ in CASES]


@functools.lru_cache(maxsize=None)
def model(case):
    """(msa, initial boundaries, final boundaries, rounds, removed) of CASES[case], computed once."""
    m, n, rows, kw, seed, _ = CASES[case]
    msa = random_msa(np.random.default_rng(seed), m, n, **kw)
    b0, b1, rounds, removed, _ = HM.heuristic(msa, rows)
    msa.setflags(write=False)
    return msa, b0, b1, rounds, removed


# ---- CPU: the model against the definition ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_model_repairs_to_a_valid_graph(case):
    msa, b0, b1, rounds, removed = model(case)
    assert rounds == CASES[case][5]                      # found with this model; a drift shows up here
    assert rounds == len(removed) and all(r > 0 for r in removed)
    assert len(b0) - len(b1) == sum(removed)
    assert set(b1.tolist()) <= set(b0.tolist()) and b1[-1] == b0[-1] == msa.shape[1]
    labels, edges, blocks = HM.segmentation_graph(msa, b1)
    status, bad = VM.naive_validate(labels, edges, blocks)
    assert not bad and not (status == VM.INVALID).any()


@pytest.mark.parametrize("case", [0, 3, 4, 7], ids=[CASE_IDS[c] for c in (0, 3, 4, 7)])
def test_model_with_one_chunk_is_the_unchunked_optimum(case):
    msa = model(case)[0]
    want = O.minmax_dp(O.compute_f(msa))[2]
    for rows in (msa.shape[0], msa.shape[0] + 5):
        assert np.array_equal(O.minmax_dp(HM.chunked_f(msa, rows))[2], want)


def run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True)
    return p.returncode, p.stdout, p.stderr


def test_cli_refuses_the_mode_without_elastic_gfa(tmp_path):
    rc, so, se = run(BIN, "--input", os.path.join(GOLD, "test.fasta"), "--output", str(tmp_path / "o"), "--heuristic-subset=3")
    assert rc == 1 and so == b""
    assert se.decode() == ("--heuristic-subset needs --elastic and --gfa: the row-chunk mode is defined for the elastic "
                           "xGFA output only.\n")
    assert not (tmp_path / "o").exists()


def test_cli_unequal_rows_are_fatal_in_the_mode(tmp_path):
    p = tmp_path / "bad.fasta"
    p.write_bytes(b">a\nACGT\n>b\nACG\n>c\nAC\nGT\n")
    rc, _, se = run(BIN, "--input", str(p), "--output", str(tmp_path / "o"), "--heuristic-subset=3", "--elastic", "--gfa")
    assert rc == 1 and se.decode() == "MSA rows have mismatching size!\n"
    assert not (tmp_path / "o").exists()


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def patterns_of(msa, rng, count=200):
    """Half cut from the rows (gaps stripped), half random over the MSA's symbols."""
    m, n = msa.shape
    syms = np.unique(msa[msa != ord("-")])
    out = []
    for k in range(count):
        ln = int(rng.integers(1, max(2, min(n, 24))))
        if k % 2 == 0:
            i, x = int(rng.integers(0, m)), int(rng.integers(0, max(1, n - ln + 1)))
            out.append(msa[i, x:x + ln].tobytes().replace(b"-", b""))
        else:
            out.append(syms[rng.integers(0, len(syms), ln)].tobytes())
    return out


def same_index(engine, msa, b, ignore="", searches=True):
    """The index built on the device against the host-assembled one of the same segmentation: array for array."""
    import founderblockgraphs_amd as F
    (data, off), edges, blocks = F.graph_from_segmentation(engine, msa, b, packed=True, with_blocks=True)
    with engine.pattern_index((data, off), edges) as ref, engine.pattern_index_of_segmentation(b) as dev:
        assert dev.n_nodes == ref.n_nodes == len(off) - 1
        assert np.array_equal(dev.node_block, blocks)
        assert np.array_equal(dev._label_len, np.diff(off.astype(np.int64)))
        first = np.searchsorted(blocks, np.arange(len(b) + 1))
        assert np.array_equal(dev.first_node.astype(np.int64), first)
        assert dev.text_length() == ref.text_length()
        for x, y, name in zip(dev.download(), ref.download(), ("text", "SA", "B", "E")):
            assert np.array_equal(x, y), name
        va, vb = dev.validate(blocks, ignore), ref.validate(blocks, ignore)
        assert np.array_equal(va.status, vb.status)
        assert np.array_equal(va.witness_node, vb.witness_node) and np.array_equal(va.witness_offset, vb.witness_offset)
        if searches:
            pats = patterns_of(msa, np.random.default_rng(len(b)))
            for x, y in zip(dev.locate(pats), ref.locate(pats)):
                assert np.array_equal(x, y)
            oa, ob = dev.occurrences(pats, 8), ref.occurrences(pats, 8)
            for name in ("count", "pos", "restarts", "end_total", "start_total", "end_off", "start_off", "end_src", "end_dst",
                         "end_offset", "start_src", "start_dst", "start_offset"):
                assert np.array_equal(getattr(oa, name), getattr(ob, name)), name
            assert all(np.array_equal(x, y) for x, y in zip(oa.as_nodes("end"), ob.as_nodes("end")))
        return dev.n_nodes, int(ref.text_length()), va


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_device_index_equals_host_assembled_index(engine, case):
    msa, b0, b1, _, _ = model(case)
    same_index(engine, msa, b0)
    same_index(engine, msa, b1)


def cuts(n, width):
    return np.array(list(range(width - 1, n - 1, width)) + [n], dtype=np.uint64)


@pytest.mark.gpu
def test_shapes_one_row_one_block_one_column(engine):
    rng = np.random.default_rng(7)
    one = random_msa(rng, 1, 20)
    same_index(engine, one, np.array([4, 9, 20], dtype=np.uint64))
    msa = random_msa(rng, 5, 30)
    nodes, n1, _ = same_index(engine, msa, np.array([30], dtype=np.uint64))
    assert n1 == 1 and nodes == 5                         # one block: no edges, a text of one sentinel
    engine.msa_load_host(msa)
    with engine.pattern_index_of_segmentation([30]) as pix:
        assert pix.download()[0].tolist() == [0]
    col = random_msa(rng, 6, 1)
    same_index(engine, col, np.array([1], dtype=np.uint64))


@pytest.mark.gpu
def test_shapes_rows_of_gaps(engine):
    msa = random_msa(np.random.default_rng(8), 5, 16).copy()
    msa[1:3, 4:8] = ord("-")                              # block 1: two rows have no node and no edge across
    msa[:, 8:10] = ord("-")                               # block 2: no node at all
    b = np.array([3, 7, 9, 16], dtype=np.uint64)
    nodes, _, _ = same_index(engine, msa, b)
    labels, edges, blocks = HM.segmentation_graph(msa, b)
    assert nodes == len(labels) and 2 not in blocks.tolist()
    engine.msa_load_host(msa)
    node_of = engine.block_graph(b)[0]
    assert (node_of[1, 1:3] == 0xffffffff).all() and (node_of[2] == 0xffffffff).all()
    allgaps = np.full((3, 6), ord("-"), dtype=np.uint8)
    nodes, n1, _ = same_index(engine, allgaps, np.array([2, 6], dtype=np.uint64), searches=False)
    assert nodes == 0 and n1 == 1


@pytest.mark.gpu
def test_shapes_label_lengths_around_the_padding(engine):
    msa = random_msa(np.random.default_rng(9), 4, 24)
    b = np.array([6, 14, 24], dtype=np.uint64)           # labels of 7, 8 and 9 symbols
    engine.msa_load_host(msa)
    with engine.pattern_index_of_segmentation(b) as pix:
        assert sorted(set(pix._label_len.tolist())) == [7, 8, 9]
    same_index(engine, msa, b)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [65, 257])
def test_shapes_scans_across_workgroups(engine, m):
    msa = random_msa(np.random.default_rng(m), m, 40)
    b = cuts(40, 4)
    nodes, _, _ = same_index(engine, msa, b)
    _, edges, _ = HM.segmentation_graph(msa, b)
    assert nodes > 256 and len(edges) > 256


@pytest.mark.gpu
def test_shapes_ignore_character_and_wide_alphabet(engine):
    msa = random_msa(np.random.default_rng(10), 8, 48, similar=0.8, n_p=0.08)
    b = cuts(48, 6)
    _, _, v = same_index(engine, msa, b, ignore="N")
    assert (v.status == VM.SKIP_IGNORED).any()
    syms = np.array([c for c in range(1, 256) if c not in (ord("#"), ord("-"))], dtype=np.uint8)
    rng = np.random.default_rng(11)
    wide = np.stack([rng.permutation(syms) for _ in range(3)])
    same_index(engine, wide, cuts(len(syms), 11))       # 253 symbols: the occ layout with a count table


@pytest.mark.gpu
def test_separator_in_the_msa_is_refused(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    msa = random_msa(np.random.default_rng(12), 4, 20).copy()
    msa[2, 13] = ord("#")
    engine.msa_load_host(msa)
    with pytest.raises(F.FbgError) as e:
        engine.pattern_index_of_segmentation(cuts(20, 5))
    assert e.value.code == _lib.FBG_ERR_INVALID
    with pytest.raises(F.FbgError) as e:
        engine.validate_segmentation(cuts(20, 5))
    assert e.value.code == _lib.FBG_ERR_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("ignore", ["", "N"])
def test_validate_segmentation_flags_the_models_cuts(engine, ignore):
    msa = random_msa(np.random.default_rng(58), 12, 96, similar=0.9, n_p=0.05)
    b = O.minmax_dp(HM.chunked_f(msa, 3, ignore))[2]
    want, status, (labels, _, _) = HM.cuts_of(msa, b, ignore)
    assert want                                             # the case is not trivially valid
    engine.msa_load_host(msa)
    got = engine.validate_segmentation(b, ignore)
    assert got.bad_cuts.tolist() == want
    assert got.cut_bad[-1] == 0 and got.cut_bad.sum() == len(want)
    assert got.n_nodes == len(labels) and got.n_invalid == int((status == VM.INVALID).sum()) and not got.valid


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_repair_segmentation_equals_the_model(engine, case):
    msa, b0, b1, rounds, removed = model(case)
    engine.msa_load_host(msa)
    got, r, rem = engine.repair_segmentation(b0)
    assert np.array_equal(got, b1) and r == rounds and rem == removed
    assert engine.validate_segmentation(got).valid


@pytest.mark.gpu
def test_repair_leaves_a_valid_segmentation_and_the_context_alone(engine):
    msa, b0, b1, rounds, _ = model(4)
    f = engine.elastic_f(msa)                              # the context now holds the MSA and its index
    best = engine.minmax_dp(f)
    before = engine.index_download()
    pats = patterns_of(msa, np.random.default_rng(3))
    with engine.pattern_index_of_segmentation(b0) as other:
        loc = other.locate(pats)
        occ = other.occurrences(pats, 8)
        got, r, rem = engine.repair_segmentation(best)
        assert np.array_equal(got, best) and r == 0 and rem == []      # the unchunked optimum is valid
        got, r, _ = engine.repair_segmentation(b0)
        assert np.array_equal(got, b1) and r == rounds
        assert engine.validate_segmentation(b0).bad_cuts.tolist() == HM.cuts_of(msa, b0)[0]
        for x, y in zip(engine.index_download(), before):
            assert np.array_equal(x, y)
        for x, y in zip(other.locate(pats), loc):
            assert np.array_equal(x, y)
        again = other.occurrences(pats, 8)
        for name in ("count", "end_off", "start_off", "end_src", "end_dst", "end_offset", "start_src", "start_dst", "start_offset"):
            assert np.array_equal(getattr(again, name), getattr(occ, name)), name
    assert np.array_equal(engine.elastic_f(msa), f)


@pytest.mark.gpu
def test_segment_elastic_heuristic_equals_the_model(engine):
    import founderblockgraphs_amd as F
    msa = model(4)[0]
    for rows in (1, 3, msa.shape[0], msa.shape[0] + 3):
        b0, b1, rounds, removed, f = HM.heuristic(msa, rows)
        got_b, got_f, r, rem = F.segment_elastic_heuristic(msa, rows, engine=engine)
        assert np.array_equal(got_f, f) and np.array_equal(got_b, b1) and r == rounds and rem == removed
    gappy = model(6)[0]
    b0, b1, rounds, removed, f = HM.heuristic(gappy, 4, "", True)
    got_b, got_f, r, rem = F.segment_elastic_heuristic(gappy, 4, disable_efg_tricks=True, engine=engine)
    assert np.array_equal(got_f, f) and np.array_equal(got_b, b1) and r == rounds and rem == removed


@pytest.mark.gpu
def test_segment_elastic_heuristic_without_a_segmentation(engine):
    import founderblockgraphs_amd as F
    msa = random_msa(np.random.default_rng(0), 6, 40, alphabet="A", gap_p=0.3)
    assert O.compute_f(msa[:3], disable_tricks=True)[0] == 40          # the first chunk has no segmentation
    with pytest.raises(F.NoSegmentation):
        F.segment_elastic_heuristic(msa, 3, disable_efg_tricks=True, engine=engine)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [3, 4, 7], ids=[CASE_IDS[c] for c in (3, 4, 7)])
def test_cli_row_chunk_mode(case, tmp_path):
    msa, b0, b1, rounds, removed = model(case)
    msa = msa.copy()
    ids = [f"r{i} sample" for i in range(msa.shape[0])]
    rows = CASES[case][2]
    if (msa[:, 0] == ord("-")).any():                      # every row needs a first block for -p (fbg.cpp:1295)
        msa[:, 0] = np.where(msa[:, 0] == ord("-"), ord("A"), msa[:, 0])
        b0, b1, rounds, removed, _ = HM.heuristic(msa, rows)
    src = tmp_path / "in.fasta"
    write_fasta(src, msa, ids, width=50 if case % 2 else None)
    for paths in (False, True):
        out = tmp_path / f"out{int(paths)}.xgfa"
        rc, _, se = run(BIN, "--input", str(src), "--output", str(out), "--elastic", "--gfa", f"--heuristic-subset={rows}",
                        "--threads=2", *(["-p"] if paths else []))
        text = se.decode()
        assert rc == 0, text
        assert out.read_bytes() == O.write_xgfa(msa, b1, str(tmp_path / "exp.xgfa"), ids=ids if paths else None)
        lines = text.split("\n")
        assert [ln for ln in lines if ln.startswith("Reading MSA[")] == \
            [f"Reading MSA[{r}..{r + rows - 1}]..." for r in range(0, msa.shape[0], rows)]
        assert [ln for ln in lines if ln.endswith("blocks to remove")] == \
            [f"There are {k} blocks to remove" for k in removed + [0]]
        assert f"Graph fixed in {rounds}iterations…\nWriting the xGFA to disk…\n" in text
        assert f"Input MSA[1..{msa.shape[0]},1..{msa.shape[1]}]" in text
        assert not os.path.exists(str(src) + ".transpose")
        rc, so, se = run(VALIDATE, f"--graph={out}")
        assert rc == 0, (so, se)


@pytest.mark.gpu
def test_cli_beyond_the_row_limit_repairs_on_the_host(tmp_path):
    """One row more than fbg_block_graph groups (FBG_MAX_ROWS): the program cuts and numbers the labels itself and
    checks every round with fbg_pindex_build + fbg_pindex_validate.  The model takes one repair round here."""
    msa = random_msa(np.random.default_rng(1), 32769, 32, alphabet="AC", similar=0.99)
    b0, b1, rounds, removed, _ = HM.heuristic(msa, 8192)
    assert rounds == 1 and removed == [1]
    src, out = tmp_path / "in.fasta", tmp_path / "out.xgfa"
    write_fasta(src, msa, [f"r{i}" for i in range(msa.shape[0])])
    rc, _, se = run(BIN, "--input", str(src), "--output", str(out), "--elastic", "--gfa", "--heuristic-subset=8192")
    text = se.decode()
    assert rc == 0, text
    assert out.read_bytes() == O.write_xgfa(msa, b1, str(tmp_path / "exp.xgfa"))
    assert "There are 1 blocks to remove\nThere are 0 blocks to remove\nGraph fixed in 1iterations…\n" in text
