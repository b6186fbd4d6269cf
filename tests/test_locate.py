"""Pattern index of a founder graph and batched pattern search (fbg_pindex_*, csrc/locate.hip, fbg_locate).

The checker is tests/locate_model.py, a numpy restatement of the reference's founder_block_index (text, SA, B / E,
backward search with restarts).  CPU tests pin the model on the example graph of xGFAspec.md and against plain
substring counting; GPU tests compare the device index and searches with the model bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import locate_model as M  # noqa: E402
from conftest import random_msa  # noqa: E402

SPEC = os.path.join(HERE, "golden", "xgfa_spec_example.xgfa")
LOCATE = os.path.join(ROOT, "founderblockgraphs_amd", "fbg_locate")
HOST = os.path.join(ROOT, "founderblockgraphs_amd", "founderblockgraph")

SPEC_TABLE = {
    "AG": (4, 2), "CGACTA": (1, 6), "GACTAG": (2, 6), "AGCGACTAGATAC": (1, 13), "AGCGACTCGTTAC": (1, 13),
    "AGCACTCGTTAC": (1, 12), "AGCAGTT": (0, 4), "GTTACX": (0, 5), "T": (15, 1), "": (0, 0),
}
SPEC_B = [13, 17, 21, 39, 40, 44, 46, 56, 67]
SPEC_E = [15, 19, 24, 39, 41, 45, 49, 63, 69]


# ---- CPU: the model ---------------------------------------------------------------------------------------------

def test_model_reproduces_the_spec_example():
    labels, edges = M.read_xgfa(SPEC)
    assert len(labels) == 9 and len(edges) == 10
    ix = M.Index(labels, edges)
    assert ix.N + 1 == 70
    assert ix.B.tolist() == SPEC_B and ix.E.tolist() == SPEC_E
    for p, want in SPEC_TABLE.items():
        assert ix.locate(p) == want, p


def test_model_suffix_array_is_the_sorted_suffixes():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 300):
        T = np.concatenate((rng.integers(1, 4, n - 1), [0])).astype(np.uint8)
        b = T.tobytes()
        assert M.suffix_array(T).tolist() == sorted(range(n), key=lambda i: b[i:])


def test_model_counts_edge_string_occurrences_without_restarts():
    """A pattern without '#' whose search needs no restart counts its overlapping occurrences in label(u) + label(v)
    summed over the distinct edges."""
    rng = np.random.default_rng(11)
    for trial in range(6):
        n = int(rng.integers(2, 12))
        labels = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(0, 7)))) for _ in range(n)]
        edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(int(rng.integers(0, 3 * n)))]
        ix = M.Index(labels, edges)
        strings = [labels[u] + labels[v] for u, v in sorted(set(edges))]
        checked = 0
        for _ in range(300):
            p = "".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(1, 6))))
            want = sum(sum(1 for i in range(len(s) - len(p) + 1) if s.startswith(p, i)) for s in strings)
            # no restart: every prefix of the pattern is found by a plain backward search
            l, r, plain = 0, ix.N, True
            for c in p.encode():
                cnt, l, r = ix.bs(c, l, r)
                plain = plain and cnt > 0
            if plain:
                assert ix.locate(p) == (want, len(p)), (labels, edges, p)
                checked += 1
            else:
                assert want == 0
        assert checked > 0


def test_model_tokens_follow_cin():
    assert M.tokens(b"A B\n") == [b"A", b"B"]
    assert M.tokens(b"A B") == [b"A"]
    assert M.tokens(b"") == [] and M.tokens(b"  \n") == []


def test_tool_rejects_missing_graph_and_unreadable_file(tmp_path):
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode != 0 and p.stdout == b""
    p = subprocess.run([LOCATE, "--graph=" + str(tmp_path / "missing.xgfa")], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode != 0 and p.stdout == b""
    bad = tmp_path / "bad.xgfa"
    bad.write_bytes(b"S\t1\tAC\nL\t1\t+\t7\t+\t0M\n")          # an edge to a node that does not exist
    p = subprocess.run([LOCATE, "--graph=" + str(bad)], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode != 0 and p.stdout == b""


# ---- GPU --------------------------------------------------------------------------------------------------------

def check_index(pix, model):
    T, sa, B, E = pix.download()
    assert pix.text_length() == model.N + 1
    assert np.array_equal(T, model.T)
    assert np.array_equal(sa.astype(np.int64), model.SA)
    assert np.array_equal(B.astype(np.int64), model.B)
    assert np.array_equal(E.astype(np.int64), model.E)


def check_search(pix, model, patterns):
    count, pos = pix.locate(patterns)
    want = [model.locate(p) for p in patterns]
    assert count.tolist() == [w[0] for w in want]
    assert pos.tolist() == [w[1] for w in want]
    return count


def sample_patterns(rng, msa, n_pat, alphabet=b"ACGT"):
    """Substrings of gap-stripped rows (across blocks), mutated substrings, random strings; lengths 1 .. 300; and
    the empty pattern."""
    rows = [r[r != ord("-")].tobytes() for r in msa]
    rows = [r for r in rows if r]
    out = [b""]
    while len(out) < n_pat:
        kind = rng.integers(0, 4)
        ln = int(min(300, 1 + rng.geometric(1 / 40)))
        if kind == 3:
            out.append(bytes(alphabet[i] for i in rng.integers(0, len(alphabet), ln)))
            continue
        r = rows[int(rng.integers(0, len(rows)))]
        ln = min(ln, len(r))
        a = int(rng.integers(0, len(r) - ln + 1))
        s = bytearray(r[a:a + ln])
        if kind == 2 and s:
            for _ in range(int(rng.integers(1, 3))):
                s[int(rng.integers(0, len(s)))] = alphabet[int(rng.integers(0, len(alphabet)))]
        out.append(bytes(s))
    return out


@pytest.mark.gpu
def test_spec_graph_on_the_gpu(engine):
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    model = M.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        T, sa, B, E = pix.download()
        assert B.tolist() == SPEC_B and E.tolist() == SPEC_E
        pats = list(SPEC_TABLE)
        count, pos = pix.locate(pats)
        assert [(int(c), int(p)) for c, p in zip(count, pos)] == [SPEC_TABLE[p] for p in pats]
        check_search(pix, model, sample_patterns(np.random.default_rng(5), np.array([list(b"AGCGACTAGATAC")], dtype=np.uint8), 3000))


SEG_CASES = [
    dict(name="gapfree", m=24, n=900, seed=1),
    dict(name="gaps", m=24, n=900, seed=2, gap_p=0.02, gap_run=3),
    dict(name="gaps_long_runs", m=16, n=500, seed=3, gap_p=0.08, gap_run=6),
    dict(name="similar", m=40, n=1200, seed=4, similar=0.97),
    dict(name="similar_gaps_N", m=32, n=1000, seed=5, similar=0.95, gap_p=0.01, gap_run=4, n_p=0.01, ignore="N"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEG_CASES, ids=[c["name"] for c in SEG_CASES])
def test_segmented_graphs_match_the_model(engine, case):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(case["seed"])
    msa = random_msa(rng, case["m"], case["n"], gap_p=case.get("gap_p", 0.0), gap_run=case.get("gap_run", 1),
                     similar=case.get("similar", 0.0), n_p=case.get("n_p", 0.0))
    f = engine.elastic_f(msa, ignorechars=case.get("ignore", ""))
    b = engine.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(engine, msa, b)
    model = M.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        count = check_search(pix, model, sample_patterns(rng, msa, 10_000, alphabet=b"ACGTN"))
        assert (count > 0).sum() > 1000


@pytest.mark.gpu
def test_protein_alphabet_takes_the_general_layout(engine):
    rng = np.random.default_rng(21)
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    n = 300
    labels = [bytes(alpha[i] for i in rng.integers(0, 20, int(rng.integers(0, 30)))) for _ in range(n)]
    assert any(len(x) == 0 for x in labels)              # empty labels with edges too
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(900)]
    model = M.Index(labels, edges)
    sigma = int(model.present.sum())
    assert sigma > 16
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        nblk = (model.N + 1) // 128 + 1
        assert pix.stats()["index_bytes"] >= nblk * (128 + 4 * sigma)      # counts in a table of their own
        rows = np.array([list((labels[u] + labels[v]).ljust(60, b"A")[:60]) for u, v in edges[:200]], dtype=np.uint8)
        check_search(pix, model, sample_patterns(rng, rows, 10_000, alphabet=alpha))


@pytest.mark.gpu
def test_text_beyond_a_million_symbols(engine):
    rng = np.random.default_rng(31)
    n = 4000
    anc = rng.integers(0, 4, 120)
    labels = []
    for _ in range(n):       # similar labels: long shared stretches, several doubling rounds
        x = anc[:int(rng.integers(60, 120))].copy()
        mut = rng.random(len(x)) < 0.03
        x[mut] = rng.integers(0, 4, int(mut.sum()))
        labels.append(bytes(b"ACGT"[i] for i in x))
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 8000), rng.integers(0, n, 8000))]
    model = M.Index(labels, edges)
    assert model.N + 1 > 1_000_000
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        rows = np.array([list(x[:60]) for x in labels[:500]], dtype=np.uint8)
        check_search(pix, model, sample_patterns(rng, rows, 4000))


@pytest.mark.gpu
def test_one_block_without_edges(engine):
    labels, edges = [b"ACGT", b"ACGA", b""], []
    model = M.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        assert pix.text_length() == 1
        check_index(pix, model)
        check_search(pix, model, [b"", b"A", b"ACGT", b"#", b"T"])


@pytest.mark.gpu
def test_labels_with_separators_are_refused(engine):
    import founderblockgraphs_amd as F
    for bad in (b"AC#G", b"A\0C"):
        with pytest.raises(F.FbgError) as ei:
            engine.pattern_index([b"ACG", bad], [(0, 1)])
        assert ei.value.code == 1


@pytest.mark.gpu
def test_segmentation_unchanged_by_an_index(engine):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(41)
    msa = random_msa(rng, 32, 1500, gap_p=0.01, gap_run=3)
    f1 = engine.elastic_f(msa)
    b1 = engine.minmax_dp(f1)
    labels, edges = F.graph_from_segmentation(engine, msa, b1)
    with engine.pattern_index(labels, edges) as pix:
        pix.locate(sample_patterns(rng, msa, 2000))
        f2 = engine.elastic_f(msa)
        b2 = engine.minmax_dp(f2)
    f3 = engine.elastic_f(msa)
    b3 = engine.minmax_dp(f3)
    assert np.array_equal(f1, f2) and np.array_equal(f1, f3)
    assert np.array_equal(b1, b2) and np.array_equal(b1, b3)


def run_locate(args, data):
    return subprocess.run([LOCATE] + args, input=data, capture_output=True, timeout=300)


@pytest.mark.gpu
def test_tool_on_the_spec_graph():
    ix = M.Index(*M.read_xgfa(SPEC))
    for data in (b"AGCGACTAGATAC AGCAGTT CGACTA\n", b"AGCGACTAGATAC AGCAGTT CGACTA"):
        p = run_locate(["--graph=" + SPEC], data)
        assert p.returncode == 0, p.stderr
        assert p.stdout == M.expected_stdout(ix, data)[0]
    assert run_locate(["--graph=" + SPEC], b"AGCGACTAGATAC AGCAGTT CGACTA\n").stdout == (
        b"Pattern? 1 occurrences found.\nPattern? 0 occurrences found.\nPattern? 1 occurrences found.\n"
        b"Pattern? 2 out of 3 patterns found\n")
    p = run_locate(["--graph=" + SPEC, "--error-on-not-found"], b"AGCGACTAGATAC AGCAGTT CGACTA\n")
    assert p.returncode == 1
    assert p.stdout == b"Pattern? 1 occurrences found.\nPattern? 0 occurrences found.\n"


@pytest.mark.gpu
def test_founderblockgraph_xgfa_to_fbg_locate(tmp_path):
    from fasta_util import write_fasta
    rng = np.random.default_rng(51)
    msa = random_msa(rng, 20, 700, gap_p=0.01, gap_run=3, similar=0.96)
    fa, gfa = tmp_path / "msa.fasta", tmp_path / "efg.xgfa"
    write_fasta(str(fa), msa, [f"row{i}" for i in range(len(msa))])
    p = subprocess.run([HOST, f"--input={fa}", f"--output={gfa}", "--gfa", "--elastic"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr
    ix = M.Index(*M.read_xgfa(str(gfa)))
    pats = sample_patterns(rng, msa, 400)[1:]
    for data, err in ((b" ".join(pats) + b"\n", False), (b"\n".join(pats), False), (b"\t".join(pats) + b"\n", True)):
        pf = tmp_path / "patterns.txt"
        pf.write_bytes(data)
        args = ["--graph=" + str(gfa), "--patterns=" + str(pf)] + (["--error-on-not-found"] if err else [])
        want, status = M.expected_stdout(ix, data, error_on_not_found=err)
        p = run_locate(args, b"")
        assert p.stdout == want
        assert p.returncode == status
    p = run_locate(["--graph=" + str(gfa)], b" ".join(pats) + b"\n")    # stdin
    assert p.stdout == M.expected_stdout(ix, b" ".join(pats) + b"\n")[0]
