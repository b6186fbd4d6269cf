"""Semi-repeat-free check of a founder graph (fbg_pindex_validate, csrc/pindex_validate.hip, fbg_validate).

The checker is tests/validate_model.py: the four rules and the witness restated in the pattern index's terms, pinned on
CPU against a second, naive formulation and on the example graph of xGFAspec.md.  GPU tests compare status and
witnesses with the model bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import locate_model as LM  # noqa: E402
import validate_model as VM  # noqa: E402
from conftest import random_msa  # noqa: E402
from test_locate import SEG_CASES  # noqa: E402

SPEC = os.path.join(HERE, "golden", "xgfa_spec_example.xgfa")
VALIDATE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_validate")
HOST = os.path.join(ROOT, "founderblockgraphs_amd", "founderblockgraph")
SPEC_BLOCKS = [0, 1, 1, 2, 2, 2, 3, 3, 3]          # B 1 2 3 3


def spec_graph():
    labels, edges = LM.read_xgfa(SPEC)
    return labels, edges, list(SPEC_BLOCKS)


# ---- CPU: the model -----------------------------------------------------------------------------------------------

def test_model_on_the_spec_example():
    labels, edges, blocks = spec_graph()
    st, wn, wo = VM.Validator(labels, edges).validate(blocks)
    # S ids 2 .. 6 are checked and valid, the rest are sources or sinks
    assert st.tolist() == [VM.SKIP_SOURCE_SINK] + [VM.VALID] * 5 + [VM.SKIP_SOURCE_SINK] * 3
    assert (wn == -1).all() and (wo == -1).all()
    assert VM.naive_validate(labels, edges, blocks)[0].tolist() == st.tolist()


def test_model_on_the_spec_example_with_cta_moved():
    labels, edges, blocks = spec_graph()
    assert labels[3] == b"CTA" and labels[5] == b"CT"
    blocks[3] = 3                                    # CTA (S id 4) into the last block
    st, wn, wo = VM.Validator(labels, edges).validate(blocks)
    assert st[5] == VM.INVALID and (wn[5], wo[5]) == (3, 0)          # CT: witness CTA, offset 0
    # the other checked nodes stay valid, CTA included: its own occurrences move with it
    others = [u for u in range(1, 6) if u != 5]
    assert all(st[u] == VM.VALID for u in others)
    assert VM.bad_cuts(st, blocks) == [1]
    naive, bad = VM.naive_validate(labels, edges, blocks)
    assert naive.tolist() == st.tolist() and bad == {5: {(3, 0)}}


def random_graph(rng, n, alphabet=b"AC", max_len=5, edge_factor=3, n_blocks=4, empty_p=0.1):
    labels = [b"" if rng.random() < empty_p else bytes(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(1, max_len + 1))))
              for _ in range(n)]
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(int(rng.integers(0, edge_factor * n + 1)))]
    edges += edges[:len(edges) // 4]                  # duplicates
    rng.shuffle(edges)                                # adjacency in no particular order
    blocks = rng.integers(0, n_blocks, n).tolist()
    return labels, edges, blocks


def test_model_matches_the_naive_formulation_on_random_graphs():
    rng = np.random.default_rng(7)
    seen = np.zeros(5, dtype=int)
    for trial in range(150):
        n = int(rng.integers(1, 14))
        labels, edges, blocks = random_graph(rng, n, alphabet=b"ACN" if trial % 3 == 0 else b"AC")
        ignore = b"N" if trial % 2 == 0 else b""
        st, wn, wo = VM.Validator(labels, edges).validate(blocks, ignore)
        naive, bad = VM.naive_validate(labels, edges, blocks, ignore)
        assert st.tolist() == naive.tolist(), (labels, edges, blocks)
        for u in range(n):
            if st[u] == VM.INVALID:
                assert (int(wn[u]), int(wo[u])) in bad[u]
            else:
                assert wn[u] == -1 and wo[u] == -1
        seen += np.bincount(st, minlength=5)
    assert (seen > 0).all(), seen                     # every status occurs


def test_model_witness_is_the_first_disallowed_slot():
    """The witness is the disallowed occurrence of smallest SA slot: checked against a scan of the whole SA."""
    rng = np.random.default_rng(8)
    for _ in range(40):
        labels, edges, blocks = random_graph(rng, int(rng.integers(2, 12)), empty_p=0.0)
        v = VM.Validator(labels, edges)
        st, wn, wo = v.validate(blocks)
        for u in np.nonzero(st == VM.INVALID)[0]:
            rev = labels[u][::-1]
            first = next(v.occurrence(p, len(rev)) for p in v.SA
                         if v.Tb[p:p + len(rev)] == rev and (v.occurrence(p, len(rev))[1] != 0 or
                                                              blocks[v.occurrence(p, len(rev))[0]] != blocks[u]))
            assert first == (wn[u], wo[u])


# ---- CPU: the ABI and the tool ----------------------------------------------------------------------------------

def test_library_exports_validate_and_header_declares_the_statuses():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "fbg_pindex_validate") and hasattr(L, "fbg_pindex_validate_stats")
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    want = {"FBG_NODE_VALID": 0, "FBG_NODE_INVALID": 1, "FBG_NODE_SKIP_SOURCE_SINK": 2, "FBG_NODE_SKIP_IGNORED": 3,
            "FBG_NODE_SKIP_EMPTY": 4}
    for name, value in want.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (_lib.NODE_VALID, _lib.NODE_INVALID, _lib.NODE_SKIP_SOURCE_SINK, _lib.NODE_SKIP_IGNORED,
            _lib.NODE_SKIP_EMPTY) == (0, 1, 2, 3, 4)


def run_validate(args):
    return subprocess.run([VALIDATE] + args, capture_output=True, timeout=300)


def test_tool_usage_and_input_errors_exit_2(tmp_path):
    assert os.path.exists(VALIDATE), "fbg_validate is built by make -C founderblockgraphs_amd/csrc"
    p = run_validate([])
    assert p.returncode == 2 and p.stdout == b""
    p = run_validate(["--graph=" + str(tmp_path / "missing.xgfa")])
    assert p.returncode == 2 and p.stdout == b""
    p = run_validate(["--graph=" + SPEC, "--bogus"])
    assert p.returncode == 2 and p.stdout == b""
    spec = open(SPEC, "rb").read()
    no_b = tmp_path / "no_b.xgfa"
    no_b.write_bytes(b"".join(x for x in spec.splitlines(True) if not x.startswith(b"B\t")))
    p = run_validate(["--graph=" + str(no_b)])
    assert p.returncode == 2 and p.stdout == b"" and b"B line" in p.stderr
    bad_sum = tmp_path / "bad_sum.xgfa"
    bad_sum.write_bytes(spec.replace(b"B\t1\t2\t3\t3\n", b"B\t1\t2\t3\t2\n"))
    p = run_validate(["--graph=" + str(bad_sum)])
    assert p.returncode == 2 and p.stdout == b"" and b"sum" in p.stderr


def test_read_xgfa_blocks(tmp_path):
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    l2, e2, nb = F.read_xgfa(SPEC, blocks=True)
    assert (l2, e2) == (labels, edges)
    assert nb.dtype == np.int64 and nb.tolist() == SPEC_BLOCKS
    spec = open(SPEC, "rb").read()
    for name, data in (("no_b", spec.replace(b"B\t1\t2\t3\t3\n", b"")), ("bad_sum", spec.replace(b"B\t1\t2\t3\t3\n", b"B\t1\t2\t3\n"))):
        f = tmp_path / (name + ".xgfa")
        f.write_bytes(data)
        assert len(F.read_xgfa(str(f))) == 2           # the default read does not look at B
        with pytest.raises(ValueError):
            F.read_xgfa(str(f), blocks=True)


# ---- GPU ----------------------------------------------------------------------------------------------------------

def check(engine, labels, edges, blocks, ignore=""):
    """Device result == model, bit for bit; returns (result, model status).  `ignore`: str (UTF-8) or bytes as they are."""
    st, wn, wo = VM.Validator(labels, edges).validate(blocks, LM.as_bytes(ignore))
    res = engine.validate_graph(labels, edges, blocks, ignore)
    assert res.status.dtype == np.uint8 and res.witness_node.dtype == np.int64
    assert np.array_equal(res.status, st)
    assert np.array_equal(res.witness_node, wn)
    assert np.array_equal(res.witness_offset, wo)
    assert res.valid == (not (st == VM.INVALID).any())
    assert res.invalid_nodes.tolist() == np.nonzero(st == VM.INVALID)[0].tolist()
    assert res.bad_cuts.tolist() == VM.bad_cuts(st, blocks)
    return res, st


@pytest.mark.gpu
def test_spec_graph_and_its_altered_blocks(engine):
    labels, edges, blocks = spec_graph()
    res, st = check(engine, labels, edges, blocks)
    assert res.valid and st.tolist() == [2, 0, 0, 0, 0, 0, 2, 2, 2]
    blocks[3] = 3
    res, st = check(engine, labels, edges, blocks)
    assert not res.valid and res.invalid_nodes.tolist() == [5]
    assert (res.witness_node[5], res.witness_offset[5]) == (3, 0)
    assert res.bad_cuts.tolist() == [1]


def random_cuts(rng, n, count):
    cuts = np.sort(rng.choice(np.arange(0, n - 1), size=min(count, n - 1), replace=False))
    return np.concatenate([cuts, [n]]).astype(np.uint64)


def case_msa(case):
    rng = np.random.default_rng(case["seed"])
    return rng, random_msa(rng, case["m"], case["n"], gap_p=case.get("gap_p", 0.0), gap_run=case.get("gap_run", 1),
                           similar=case.get("similar", 0.0), n_p=case.get("n_p", 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEG_CASES, ids=[c["name"] for c in SEG_CASES])
def test_dp_segmented_graphs_match_the_model(engine, case):
    import founderblockgraphs_amd as F
    rng, msa = case_msa(case)
    f = engine.elastic_f(msa, ignorechars=case.get("ignore", ""))
    b = engine.minmax_dp(f)
    labels, edges, blocks = F.graph_from_segmentation(engine, msa, b, with_blocks=True)
    assert len(blocks) == len(labels) and blocks[-1] == len(b) - 1
    res, st = check(engine, labels, edges, blocks, case.get("ignore", ""))
    assert (st == VM.VALID).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEG_CASES, ids=[c["name"] for c in SEG_CASES])
def test_randomly_segmented_graphs_match_the_model(engine, case):
    import founderblockgraphs_amd as F
    rng, msa = case_msa(case)
    n = msa.shape[1]
    seen = np.zeros(5, dtype=int)
    for b in (random_cuts(rng, n, n // 4), random_cuts(rng, n, n // 30), random_cuts(rng, n, n - 1)):   # the last: every column
        labels, edges, blocks = F.graph_from_segmentation(engine, msa, b, with_blocks=True)
        res, st = check(engine, labels, edges, blocks, case.get("ignore", ""))
        seen += np.bincount(st, minlength=5)
    assert seen[VM.VALID] > 0 and seen[VM.INVALID] > 0, seen


@pytest.mark.gpu
def test_protein_alphabet_graph(engine):
    rng = np.random.default_rng(21)
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    n = 300
    labels = [bytes(alpha[i] for i in rng.integers(0, 20, int(rng.integers(1, 6)))) for _ in range(n)]
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(900)]
    blocks = rng.integers(0, 6, n)
    assert int(LM.Index(labels, edges).present.sum()) > 16      # the general occ layout
    res, st = check(engine, labels, edges, blocks, "W")
    assert (st == VM.INVALID).any() and (st == VM.VALID).any() and (st == VM.SKIP_IGNORED).any()


@pytest.mark.gpu
def test_text_beyond_a_million_symbols(engine):
    rng = np.random.default_rng(31)
    n = 4000
    anc = rng.integers(0, 4, 120)
    labels = []
    for _ in range(n):
        x = anc[:int(rng.integers(60, 120))].copy()
        mut = rng.random(len(x)) < 0.03
        x[mut] = rng.integers(0, 4, int(mut.sum()))
        labels.append(bytes(b"ACGT"[i] for i in x))
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 8000), rng.integers(0, n, 8000))]
    assert len(LM.edge_text(labels, edges)) > 1_000_000
    blocks = np.arange(n) // 500
    res, st = check(engine, labels, edges, blocks)
    assert (st == VM.INVALID).any() and (st == VM.VALID).any()


@pytest.mark.gpu
def test_prefix_of_many_same_block_labels_takes_the_wave_tier(engine):
    """'AC' is a prefix of 256 labels of its own block and occurs nowhere else: 514 allowed occurrences, VALID."""
    words = [bytes(b"GT"[(k >> i) & 1] for i in range(8)) for k in range(256)]
    labels = [b"TT", b"AC"] + [b"AC" + w for w in words] + [b"GG"]
    n = len(labels)
    edges = [(0, u) for u in range(1, n - 1)] + [(u, n - 1) for u in range(1, n - 1)]
    blocks = [0] + [1] * (n - 2) + [2]
    res, st = check(engine, labels, edges, blocks)
    assert res.valid and st[1] == VM.VALID
    assert res.wave_nodes >= 1
    # and with one of them moved to the next block, 'AC' is INVALID through the wave tier
    blocks[200] = 2
    res, st = check(engine, labels, edges, blocks)
    assert st[1] == VM.INVALID and res.witness_node[1] == 200


@pytest.mark.gpu
def test_periodic_msa_early_exit_keeps_the_witness(engine):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(61)
    m, n = 30, 600
    msa = np.tile(np.frombuffer(b"AC" * (n // 2), dtype=np.uint8), (m, 1)).copy()
    sub = rng.random((m, n)) < 0.01
    msa[sub] = np.frombuffer(b"GT", dtype=np.uint8)[rng.integers(0, 2, int(sub.sum()))]
    for cuts in (n // 10, n // 40):
        labels, edges, blocks = F.graph_from_segmentation(engine, msa, random_cuts(rng, n, cuts), with_blocks=True)
        res, st = check(engine, labels, edges, blocks)
        assert (st == VM.INVALID).sum() > 10
        assert res.slots_scanned > 0


@pytest.mark.gpu
def test_degenerate_graphs(engine):
    res, st = check(engine, [], [], [])
    assert res.valid and len(res.status) == 0
    res, st = check(engine, [b"AC", b"G", b""], [], [0, 1, 2])                      # no edges
    assert st.tolist() == [VM.SKIP_SOURCE_SINK] * 3
    labels = [b"AC", b"CA", b"A", b"C"]
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (1, 0)]
    res, st = check(engine, labels, edges, [0, 0, 0, 0])                           # one block
    check(engine, labels, edges + edges + [(2, 3)] * 3, [0, 1, 1, 2])              # duplicate edges
    labels = [b"AC", b"", b"ACA", b"", b"C"]
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 1), (1, 1)]
    res, st = check(engine, labels, edges, [0, 1, 2, 3, 4])                        # empty labels, a self loop
    assert st[1] == VM.SKIP_EMPTY and st[3] == VM.SKIP_EMPTY


@pytest.mark.gpu
def test_arguments_are_checked(engine):
    import founderblockgraphs_amd as F
    with engine.pattern_index([b"AC", b"G"], [(0, 1)]) as pix:
        with pytest.raises(ValueError):
            pix.validate([0])
        L = engine._L
        st = np.zeros(2, dtype=np.uint8)
        assert L.fbg_pindex_validate(pix._h, None, None, 0, st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, None,
                                     None, None) == 1
        assert L.fbg_pindex_validate(None, None, None, 0, None, None, None, None, None) == 1
        blk = np.zeros(2, dtype=np.uint32)
        assert L.fbg_pindex_validate(pix._h, blk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, 0, None, None, None,
                                     None, None) == 1
        r = pix.validate([0, 1])
        assert r.status.tolist() == [VM.SKIP_SOURCE_SINK] * 2
    assert isinstance(r, F.Validation)


@pytest.mark.gpu
def test_locate_and_segmentation_unchanged_by_validate(engine):
    import founderblockgraphs_amd as F
    from test_locate import sample_patterns
    rng = np.random.default_rng(71)
    msa = random_msa(rng, 24, 900, gap_p=0.01, gap_run=3)
    f1 = engine.elastic_f(msa)
    b1 = engine.minmax_dp(f1)
    labels, edges, blocks = F.graph_from_segmentation(engine, msa, random_cuts(rng, 900, 200), with_blocks=True)
    pats = sample_patterns(rng, msa, 3000)
    with engine.pattern_index(labels, edges) as pix:
        c1, p1 = pix.locate(pats)
        s1 = pix.stats()["search_ms"]
        r1 = pix.validate(blocks)
        assert pix.stats()["search_ms"] == s1
        c2, p2 = pix.locate(pats)
        r2 = pix.validate(blocks)
        f2 = engine.elastic_f(msa)
        b2 = engine.minmax_dp(f2)
    assert np.array_equal(c1, c2) and np.array_equal(p1, p2)
    assert np.array_equal(r1.status, r2.status) and np.array_equal(r1.witness_node, r2.witness_node)
    assert np.array_equal(f1, f2) and np.array_equal(b1, b2)


@pytest.mark.gpu
def test_tool_on_founderblockgraph_output(tmp_path):
    from fasta_util import write_fasta
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(81)
    msa = random_msa(rng, 20, 700, gap_p=0.01, gap_run=3, similar=0.96)
    fa, gfa = tmp_path / "msa.fasta", tmp_path / "efg.xgfa"
    write_fasta(str(fa), msa, [f"row{i}" for i in range(len(msa))])
    p = subprocess.run([HOST, f"--input={fa}", f"--output={gfa}", "--gfa", "--elastic"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr
    labels, edges, blocks = F.read_xgfa(str(gfa), blocks=True)
    want, status = VM.expected_tool_output(labels, edges, VM.xgfa_ids(str(gfa)), blocks)
    p = run_validate(["--graph=" + str(gfa)])
    assert p.stdout == want
    assert p.returncode == status


@pytest.mark.gpu
def test_tool_on_a_randomly_segmented_graph(engine, tmp_path):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(91)
    msa = random_msa(rng, 16, 400, similar=0.9, gap_p=0.01, gap_run=3, n_p=0.01)
    b = random_cuts(rng, 400, 120)
    labels, edges, blocks = F.graph_from_segmentation(engine, msa, b, with_blocks=True)
    ids = list(range(1, len(labels) + 1))
    lines = [b"B\t" + b"\t".join(b"%d" % c for c in np.bincount(blocks, minlength=len(b)))]
    lines += [b"S\t%d\t%s" % (ids[u], labels[u]) for u in range(len(labels))]
    lines += [b"L\t%d\t+\t%d\t+\t0M" % (ids[u] , ids[v]) for u, v in edges]
    g = tmp_path / "random.xgfa"
    g.write_bytes(b"\n".join(lines) + b"\n")
    for ignore in ("", "N"):
        want, status = VM.expected_tool_output(labels, edges, ids, blocks, ignore.encode())
        p = run_validate(["--graph=" + str(g)] + (["--ignore-chars=" + ignore] if ignore else []))
        assert status == 1 and p.returncode == 1, p.stderr
        assert p.stdout == want
