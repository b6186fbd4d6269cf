"""MSA row and column of every reported place: fbg_pindex_occurrences_msa / fbg_pindex_seeds_msa / fbg_pindex_msa_stats,
PatternIndex.occurrences(msa=True) / .seeds(msa=True) / .msa_stats() and fbg_locate --msa (include/fbg_hip.h,
csrc/locate.hip).

The checker is tests/msa_model.py: representative rows and the columns of their non-gap cells straight from (A,
boundaries), applied to the places the existing fetch calls return (those are pinned by test_occurrences / test_seeds).
Every GPU comparison also checks the invariant A[row][col] == S_e[offset] against the MSA itself."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import locate_model as M  # noqa: E402
import msa_model as MM  # noqa: E402
import occ_model as OM  # noqa: E402
import test_locate as TL  # noqa: E402
import test_occurrences as TO  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta, write_fasta  # noqa: E402

SPEC = TL.SPEC
LOCATE = TL.LOCATE
GOLDEN = [os.path.join(HERE, "golden", f) for f in ("msa.fasta", "test.fasta", "test2.fasta", "test3.fasta")]
CALLS = ("fbg_pindex_occurrences_msa", "fbg_pindex_seeds_msa", "fbg_pindex_msa_stats")
NONE = MM.NONE
BIG = 1 << 30                      # a cap above every text length here


def short_patterns(model, longest=6):
    """Every substring of every gap-stripped row of up to `longest` symbols, plus every single symbol of the MSA."""
    pats = set()
    for row in model.A:
        s = row[row != MM.GAP].tobytes()
        pats |= {s[a:a + k] for k in range(1, longest + 1) for a in range(len(s) - k + 1)}
    pats |= {bytes([c]) for c in np.unique(model.A) if c != MM.GAP}
    return sorted(pats)


def check_coords(model, occ, what=""):
    """The four coordinate arrays of an Occurrences object equal the model applied to its places, and every coordinate
    that is not the sentinel names a cell of A that holds the symbol of S_e at the place's offset.  -> sentinels seen."""
    sentinels = 0
    for which in ("end", "start"):
        src, dst, off = (getattr(occ, f"{which}_{f}") for f in ("src", "dst", "offset"))
        row, col = getattr(occ, f"{which}_row"), getattr(occ, f"{which}_col")
        assert row is not None and row.dtype == np.uint32 and col.dtype == np.uint32
        assert len(row) == len(src) and len(col) == len(src), (what, which)
        wrow, wcol = model.coords(src, dst, off)
        assert np.array_equal(row.astype(np.int64), wrow), (what, which, "row")
        assert np.array_equal(col.astype(np.int64), wcol), (what, which, "col")
        sym = model.edge_symbol(src, dst, off)
        ok = wrow != NONE
        assert np.array_equal(sym >= 0, ok), (what, which)
        assert np.array_equal(model.A[wrow[ok], wcol[ok]].astype(np.int64), sym[ok]), (what, which, "A[row][col]")
        sentinels += int((~ok).sum())
    for k in range(min(len(occ.count), 3)):
        a, b = int(occ.end_off[k]), int(occ.end_off[k + 1])
        assert np.array_equal(occ.msa_ends(k), np.stack((occ.end_row[a:b], occ.end_col[a:b]), axis=1).astype(np.int64))
        a, b = int(occ.start_off[k]), int(occ.start_off[k + 1])
        assert np.array_equal(occ.msa_starts(k), np.stack((occ.start_row[a:b], occ.start_col[a:b]), axis=1).astype(np.int64))
    return sentinels


def build(engine, msa, boundaries):
    engine.msa_load_host(np.ascontiguousarray(msa, dtype=np.uint8))
    return engine.pattern_index_of_segmentation(boundaries)


def reached(model, occ):
    """The (node, offset) pairs among the reported ends."""
    node, o = model.node_of(occ.end_src, occ.end_dst, occ.end_offset)
    return set(zip(node.tolist(), o.tolist()))


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_msa_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in CALLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name
    assert "witness row" in header


def test_model_names_the_cell_of_every_label_symbol_on_the_golden_files():
    from oracle import pyoracle as O
    gapped = 0
    for path in GOLDEN:
        A, _ = read_fasta(path)
        b = O.minmax_dp(O.compute_f(A))[2]
        assert len(b) >= 2
        model = MM.Model(A, b)
        for u, lab in enumerate(model.labels):
            x0, x1 = model.ranges[u]
            r, cols = model.rep_row[u], model.cols[u]
            assert len(cols) == len(lab) and (np.diff(cols) > 0).all() and x0 <= cols[0] and cols[-1] < x1
            assert A[r, cols].tobytes() == lab
            assert (A[r, x0:x1] != MM.GAP).sum() == len(lab)
            # the first row with this label
            assert all(A[i, x0:x1][A[i, x0:x1] != MM.GAP].tobytes() != lab for i in range(r))
            gapped += len(lab) != x1 - x0
        # places: source below |label(a)|, destination from there on, the sentinel beyond the edge
        for a, c in model.edges:
            la, lc = len(model.labels[a]), len(model.labels[c])
            offs = np.arange(la + lc + 2)
            row, col = model.coords([a] * len(offs), [c] * len(offs), offs)
            assert row[:la].tolist() == [model.rep_row[a]] * la and col[:la].tolist() == model.cols[a].tolist()
            assert row[la:la + lc].tolist() == [model.rep_row[c]] * lc and col[la:la + lc].tolist() == model.cols[c].tolist()
            assert row[la + lc:].tolist() == [NONE, NONE] and col[la + lc:].tolist() == [NONE, NONE]
    assert gapped > 3


def test_tool_msa_argument_handling(tmp_path):
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--msa=msa.fasta" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--msa="], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"--msa takes" in p.stderr
    # all of these fail before the device is touched: an unreadable FASTA, an M line that disagrees with the FASTA, a
    # graph without M / X lines
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--msa=" + str(tmp_path / "missing.fasta")], input=b"AG\n", capture_output=True,
                       timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"cannot open" in p.stderr
    p = subprocess.run([LOCATE, "--graph=" + SPEC, "--msa=" + GOLDEN[1], "--occurrences"], input=b"AG\n", capture_output=True,
                       timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"does not fit" in p.stderr and b"M line" in p.stderr
    bare = tmp_path / "bare.gfa"
    bare.write_bytes(b"".join(ln for ln in open(SPEC, "rb") if ln[:1] not in (b"M", b"X")))
    p = subprocess.run([LOCATE, "--graph=" + str(bare), "--msa=" + GOLDEN[0]], input=b"AG\n", capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"M and X lines" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_fixtures(engine, path):
    A, _ = read_fasta(path)
    b = engine.minmax_dp(engine.elastic_f(A))
    assert len(b) >= 2
    model = MM.Model(A, b)
    with build(engine, A, b) as pix:
        assert pix.n_nodes == len(model.labels) and pix._label_len.tolist() == model.label_len.tolist()
        occ = pix.occurrences(short_patterns(model), max_per_pattern=BIG, msa=True)
        assert check_coords(model, occ, path) == 0
        assert reached(model, occ) == model.on_edges()
        st = pix.msa_stats()
        assert st["gapped_nodes"] == sum(len(lab) != x1 - x0 for lab, (x0, x1) in zip(model.labels, model.ranges))
        assert st["sample_columns"] % 64 == 0 and st["sample_columns"] > 0 and st["map_bytes"] >= 16 * pix.n_nodes
        plain = pix.occurrences(short_patterns(model), max_per_pattern=BIG)
        assert plain.end_row is None and plain.start_col is None
        with pytest.raises(ValueError):
            plain.msa_ends(0)


WIDTHS = ("63", "64", "65", "127", "128", "129", "S-1", "S", "S+1", "2S+1")


def table_msa(rng, w, lead, gaps_first):
    """4 rows: [a narrow block of `lead` columns,] one wide block of w columns, one narrow block of 3.  In the wide block
    one row has no gap, one has gaps at the relative columns 0, 63, 64 and w - 1, one spells the same label with its
    gaps at the columns 1 .. k instead (the same node: only the first of the two is the witness), and one is all gaps
    (no node there).  gaps_first: the all-gap row is row 0."""
    n = lead + w + 3
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    free, other = alpha[rng.integers(0, 4, (2, n))]
    gapped, dup, none = other.copy(), other.copy(), alpha[rng.integers(0, 4, n)]
    at = sorted({c for c in (0, 63, 64, w - 1) if c < w})
    wide = other[lead:lead + w]
    label = np.delete(wide, at)
    gapped[lead + np.array(at)] = MM.GAP
    dup[lead:lead + w] = np.insert(label, [1] * len(at), MM.GAP)
    none[lead:lead + w] = MM.GAP
    rows = [none, free, gapped, dup] if gaps_first else [free, gapped, dup, none]
    b = ([lead - 1] if lead else []) + [lead + w - 1, n]
    return np.stack(rows), b, at


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_boundaries_of_the_table(engine, width):
    rng = np.random.default_rng(77)
    A0, b0, _ = table_msa(rng, 70, 0, False)
    with build(engine, A0, b0) as pix:
        S = pix.msa_stats()["sample_columns"]
    w = {"S-1": S - 1, "S": S, "S+1": S + 1, "2S+1": 2 * S + 1}.get(width) or int(width)
    for lead, gaps_first in ((0, False), (5, False), (0, True), (37, True)):
        A, b, at = table_msa(rng, w, lead, gaps_first)
        model = MM.Model(A, b)
        j = 1 if lead else 0
        wide = [u for u in range(len(model.labels)) if model.blocks[u] == j]
        assert len(wide) == 2                                      # the gap-free row, and the two gapped rows as one node
        g = [u for u in wide if len(model.labels[u]) != w][0]
        assert model.rep_row[g] == (2 if gaps_first else 1) and len(model.labels[g]) == w - len(at)
        assert all(model.rep_row[u] != 0 for u in wide) == gaps_first
        with build(engine, A, b) as pix:
            assert pix.msa_stats()["gapped_nodes"] == 1
            words = (w + 63) // 64
            assert pix.msa_stats()["map_bytes"] == 16 * pix.n_nodes + 8 * (words + (words * 64 + S - 1) // S)
            occ = pix.occurrences([b"A", b"C", b"G", b"T"], max_per_pattern=BIG, msa=True)
            assert check_coords(model, occ, (w, lead, gaps_first)) == 0
            assert reached(model, occ) == model.on_edges()
            # the gapped node's columns skip exactly the gaps
            node, o = model.node_of(occ.end_src, occ.end_dst, occ.end_offset)
            cols = {int(x): int(c) for x, c in zip(o[node == g], occ.end_col[node == g])}
            assert [cols[x] - lead for x in range(w - len(at))] == [c for c in range(w) if c not in at]


def star_msa(rng, m=40, n=600):
    return random_msa(rng, m, n, gap_p=0.01, gap_run=6, similar=0.96)


def star_reads(rng, A, count=2000):
    rows = [r[r != MM.GAP].tobytes() for r in A]
    out = []
    for k in range(count):
        r = rows[int(rng.integers(0, len(rows)))]
        ln = int(rng.integers(12, 60))
        a = int(rng.integers(0, len(r) - ln))
        s = bytearray(r[a:a + ln])
        if k % 10 == 0:
            at = int(rng.integers(0, ln))
            s[at] = ord(rng.choice([c for c in "ACGT" if ord(c) != s[at]]))
        out.append(bytes(s))
    return out


@pytest.fixture(scope="module")
def star(engine):
    rng = np.random.default_rng(2024)
    A = star_msa(rng)
    b = engine.minmax_dp(engine.elastic_f(A))
    assert len(b) >= 2
    return A, b, MM.Model(A, b), star_reads(rng, A)


@pytest.mark.gpu
def test_random_reads_and_their_seeds(engine, star):
    A, b, model, reads = star
    with build(engine, A, b) as pix:
        assert pix.msa_stats()["gapped_nodes"] > 0
        occ = pix.occurrences(reads, max_per_pattern=64, msa=True)
        assert (occ.count > 0).sum() > 1000 and (occ.restarts > 0).any()
        assert check_coords(model, occ, "occurrences") == 0
        sd = pix.seeds(reads, min_length=8, max_per_seed=16, msa=True)
        assert len(sd) > 1500 and check_coords(model, sd.occ, "seeds") == 0
        # a seed's coordinates are those of occurrences() on its substring
        subs = [reads[int(k)][int(q):int(q) + int(ln)] for k, q, ln in zip(sd.pattern_of, sd.q_start, sd.length)]
        again = pix.occurrences(subs, max_per_pattern=16, msa=True)
        for f in ("end_off", "start_off", "end_row", "end_col", "start_row", "start_col"):
            assert np.array_equal(getattr(sd.occ, f), getattr(again, f)), f
        assert sd.occ.msa_ms > 0 and occ.msa_ms > 0


@pytest.mark.gpu
def test_index_keeps_no_pointer_to_the_msa(engine, star):
    A, b, model, reads = star
    with build(engine, A, b) as pix:
        engine.msa_load_host(star_msa(np.random.default_rng(5), 7, 333))
        occ = pix.occurrences(reads[:500], max_per_pattern=64, msa=True)
        assert check_coords(model, occ) == 0 and len(occ.end_row) > 500


def raw(pix):
    """The C calls one by one, for orders the Python layer does not produce."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p) if a is not None else None      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731

    class Raw:
        def search(self, pats, cap):
            data, off = (np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8).copy(),
                         np.concatenate(([0], np.cumsum([len(p) for p in pats]))).astype(np.uint64))
            k = len(pats)
            z = [np.zeros(k + 1, dtype=np.uint64) for _ in range(6)]
            rs = np.zeros(k + 1, dtype=np.uint32)
            rc = L.fbg_pindex_occurrences(pix._h, data.ctypes.data_as(_lib.u8p), u64(off), k, cap, u64(z[0]), u64(z[1]), u32(rs),
                                          u64(z[2]), u64(z[3]), u64(z[4]), u64(z[5]), None)
            assert rc == 0
            return int(z[2][k]), int(z[3][k])

        def seeds(self, pats, L_min, cap):
            data, off = (np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8).copy(),
                         np.concatenate(([0], np.cumsum([len(p) for p in pats]))).astype(np.uint64))
            so = np.zeros(len(pats) + 1, dtype=np.uint64)
            assert L.fbg_pindex_seeds(pix._h, data.ctypes.data_as(_lib.u8p), u64(off), len(pats), L_min, cap, u64(so), None) == 0
            n = int(so[-1])
            eo, st = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
            assert L.fbg_pindex_seeds_fetch(pix._h, None, None, None, None, None, None, u64(eo), u64(st), None) == 0
            return int(eo[n]), int(st[n])

        def get(self, name, ne, ns, width, ends=True, starts=True):
            arrs = [np.full((ne if k < width else ns) + 1, 0xdeadbeef, dtype=np.uint32) for k in range(2 * width)]
            args = [u32(a) if (ends if k < width else starts) else None for k, a in enumerate(arrs)]
            rc = getattr(L, name)(pix._h, *args, None)
            return rc, [a[:-1] for a in arrs]
    return Raw()


@pytest.mark.gpu
def test_calls_keep_apart(engine, star):
    A, b, model, reads = star
    p1, p2 = reads[:300], reads[300:500]
    with build(engine, A, b) as pix:
        o = pix.occurrences(p1, max_per_pattern=8, msa=True)
        s = pix.seeds(p2, min_length=8, max_per_seed=4, msa=True).occ
        count, pos = pix.locate(p1)
        ms, lines = pix.stats()["search_ms"], pix.stats()["occ_lines"]
        assert ms > 0
        R = raw(pix)
        want = {(which, kind): [getattr(x, f"{w}_{f}") for w in ("end", "start") for f in fields]
                for which, x in (("occ", o), ("seeds", s))
                for kind, fields in (("msa", ("row", "col")), ("places", ("src", "dst", "offset")))}
        ne, ns = R.search(p1, 8)
        se, ss = R.seeds(p2, 8, 4)
        assert (ne, ns, se, ss) == (len(o.end_row), len(o.start_row), len(s.end_row), len(s.start_row))

        def same(name, sizes, which, kind, **kw):
            rc, got = R.get(name, *sizes, 2 if kind == "msa" else 3, **kw)
            assert rc == 0, name
            w = 2 if kind == "msa" else 3
            for k, (g, x) in enumerate(zip(got, want[(which, kind)])):
                used = kw.get("ends", True) if k < w else kw.get("starts", True)
                assert np.array_equal(g, x) if used else (g == 0xdeadbeef).all(), (name, k)

        # coordinates before any fetch, then every order of the four calls, partial lists and repeats
        same("fbg_pindex_occurrences_msa", (ne, ns), "occ", "msa")
        same("fbg_pindex_seeds_msa", (se, ss), "seeds", "msa")
        same("fbg_pindex_occurrences_fetch", (ne, ns), "occ", "places")
        same("fbg_pindex_seeds_msa", (se, ss), "seeds", "msa", starts=False)
        same("fbg_pindex_seeds_places", (se, ss), "seeds", "places")
        same("fbg_pindex_occurrences_msa", (ne, ns), "occ", "msa", ends=False)
        same("fbg_pindex_occurrences_msa", (ne, ns), "occ", "msa")
        same("fbg_pindex_occurrences_fetch", (ne, ns), "occ", "places")
        assert R.get("fbg_pindex_occurrences_msa", ne, ns, 2, ends=False, starts=False)[0] == 0
        # locate's statistics and results are those of the last locate
        assert pix.stats()["search_ms"] == ms and pix.stats()["occ_lines"] == lines
        c2, q2 = pix.locate(p1)
        assert np.array_equal(c2, count) and np.array_equal(q2, pos)
        same("fbg_pindex_seeds_msa", (se, ss), "seeds", "msa")
        same("fbg_pindex_occurrences_msa", (ne, ns), "occ", "msa")


@pytest.mark.gpu
def test_separator_in_a_pattern(engine):
    A, _ = read_fasta(GOLDEN[0])
    b = engine.minmax_dp(engine.elastic_f(A))
    model = MM.Model(A, b)
    S = [model.labels[u] + model.labels[v] for u, v in model.edges]
    # the forward text is S_(E-1) # ... S_1 # S_0 #: a suffix of one edge string, '#', a prefix of the one before it
    pats = [S[e + 1][-2:] + b"#" + S[e][:2] for e in range(len(S) - 1)] + [b"#", b"A#", b"#A", b"AG"]
    with build(engine, A, b) as pix:
        occ = pix.occurrences(pats, max_per_pattern=BIG, msa=True)
        assert (occ.count[:len(S) - 1] > 0).all()
        assert check_coords(model, occ, "separator") > 0
        assert (occ.start_row == NONE).any() and np.array_equal(occ.start_row == NONE, occ.start_col == NONE)
        assert (occ.end_row != NONE).any()


@pytest.mark.gpu
def test_errors(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    INVALID = _lib.FBG_ERR_INVALID
    four = [np.zeros(64, dtype=np.uint32) for _ in range(4)]
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    for name in CALLS[:2]:
        assert getattr(L, name)(None, *[u32(a) for a in four], None) == INVALID
    assert L.fbg_pindex_msa_stats(None, None, None, None) == INVALID
    # an index built on the host knows no MSA
    labels, edges = F.read_xgfa(SPEC)
    with engine.pattern_index(labels, edges) as pix:
        pix.occurrences(["AG"])
        pix.seeds(["AGCGA"])
        for name in CALLS[:2]:
            assert getattr(L, name)(pix._h, *[u32(a) for a in four], None) == INVALID
        with pytest.raises(F.FbgError) as ei:
            pix.occurrences(["AG"], msa=True)
        assert ei.value.code == INVALID
        with pytest.raises(F.FbgError):
            pix.msa_stats()
    A, _ = read_fasta(GOLDEN[0])
    b = engine.minmax_dp(engine.elastic_f(A))
    model = MM.Model(A, b)
    with build(engine, A, b) as pix:
        # before any search
        for name in CALLS[:2]:
            assert getattr(L, name)(pix._h, *[u32(a) for a in four], None) == INVALID
        # an empty batch: nothing to report
        occ = pix.occurrences([], msa=True)
        assert len(occ.end_row) == 0 and len(occ.start_col) == 0
        sd = pix.seeds([], msa=True)
        assert len(sd.occ.end_row) == 0
        occ = pix.occurrences(["XYZ"], msa=True)                  # and a batch that finds nothing
        assert len(occ.end_row) == 0
        # an occurrences search does not make a seeds result, and half a list is refused
        with build(engine, A, b) as other:
            other.occurrences(["AG"])
            assert L.fbg_pindex_seeds_msa(other._h, *[u32(a) for a in four], None) == INVALID
            other.seeds(["AGCGA"])
            assert L.fbg_pindex_seeds_msa(other._h, *[u32(a) for a in four], None) == 0
        pix.occurrences(["AG", "T"], max_per_pattern=3)
        ms = ctypes.c_double(-1)
        assert L.fbg_pindex_occurrences_msa(pix._h, u32(four[0]), None, None, None, ctypes.byref(ms)) == INVALID
        assert L.fbg_pindex_occurrences_msa(pix._h, u32(four[0]), u32(four[1]), None, u32(four[3]), None) == INVALID
        assert L.fbg_pindex_occurrences_msa(pix._h, u32(four[0]), u32(four[1]), None, None, ctypes.byref(ms)) == 0 and ms.value > 0
        assert check_coords(model, pix.occurrences(["AG", "T"], max_per_pattern=3, msa=True)) == 0


@pytest.mark.gpu
def test_index_is_what_it_was(engine):
    """Text, SA, B, E, index_bytes and table_bytes of an index built from a gapped segmentation equal those of the index
    built on the host from the same graph: the coordinate table is counted in neither."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(9)
    A = random_msa(rng, 12, 300, gap_p=0.02, gap_run=4, similar=0.95)
    b = engine.minmax_dp(engine.elastic_f(A))
    assert len(b) >= 2
    labels, edges = F.graph_from_segmentation(engine, A, b)

    def table_bytes(pix):
        tb = ctypes.c_uint64(0)
        assert pix._L.fbg_pindex_validate_stats(pix._h, None, None, ctypes.byref(tb)) == 0
        return tb.value

    with engine.pattern_index(labels, edges) as host, build(engine, A, b) as dev:
        assert dev.msa_stats()["gapped_nodes"] > 0
        for x, y in zip(host.download(), dev.download()):
            assert np.array_equal(x, y)
        assert host.stats()["index_bytes"] == dev.stats()["index_bytes"]
        assert table_bytes(host) == table_bytes(dev)
        pats = TL.sample_patterns(rng, A, 500)
        a, c = host.occurrences(pats), dev.occurrences(pats)
        for f in TO.FIELDS:
            assert np.array_equal(getattr(a, f), getattr(c, f)), f


def tool_lines(model, occ_model, ids, data, cap, msa):
    """What fbg_locate --occurrences=cap [--msa] prints for stdin `data`."""
    out, found = [], 0
    toks = M.tokens(data)
    for t in toks:
        o = occ_model.occurrences(t, cap)
        out.append(b"Pattern? %d occurrences found.\n" % o.count)
        found += o.count != 0
        for tag, places, total in ((b"E", o.ends, o.end_total), (b"B", o.starts, o.start_total)):
            row, col = model.coords(places[:, 0], places[:, 1], places[:, 2])
            for (a, c, off), r, x in zip(TO.rows(places), row.tolist(), col.tolist()):
                line = b"%s\t%d\t%d\t%d" % (tag, ids[a], ids[c], off)
                if msa:
                    line += b"\t*\t*" if r == NONE else b"\t%d\t%d" % (r, x)
                out.append(line + b"\n")
            if total > len(places):
                out.append(b"%s\t...\t%d more\n" % (tag, total - len(places)))
    out.append(b"Pattern? %d out of %d patterns found\n" % (found, len(toks)))
    return b"".join(out)


@pytest.mark.gpu
def test_tool_prints_rows_and_columns(tmp_path):
    """The example graph of xGFAspec.md is a segmentation of golden/msa.fasta (its M and X lines say which)."""
    A, _ = read_fasta(GOLDEN[0])
    model = MM.Model(A, [1, 5, 8, 14])
    labels, edges = M.read_xgfa(SPEC)
    assert [M.as_bytes(s) for s in labels] == model.labels
    occ_model = OM.Index(labels, edges)
    ids = list(range(1, 10))
    data = b"AGCGACTAGATAC AGCAGTT CGACTA T GACTAG AG A#\n"
    for cap in (2, 64):
        p = TL.run_locate(["--graph=" + SPEC, "--msa=" + GOLDEN[0], f"--occurrences={cap}"], data)
        assert p.returncode == 0, p.stderr
        assert p.stdout == tool_lines(model, occ_model, ids, data, cap, True)
        q = TL.run_locate(["--graph=" + SPEC, f"--occurrences={cap}"], data)
        assert q.returncode == 0 and q.stdout == tool_lines(model, occ_model, ids, data, cap, False)
        assert q.stdout == TO.tool_lines(occ_model, ids, data, cap)
    # AGCGACTAGATAC is row 0 of the MSA from its first to its last column
    assert b"E\t4\t7\t7\t0\t13\nB\t1\t2\t0\t0\t0\n" in p.stdout
    # under --seeds, and alone (the index is built from the MSA, the output is the plain one)
    p = TL.run_locate(["--graph=" + SPEC, "--msa=" + GOLDEN[0], "--seeds", "--occurrences"], b"AGCGACTAGATAC\n")
    assert p.returncode == 0 and b"S\t0\t13\t1\t2\nE\t4\t7\t7\t0\t13\nB\t1\t2\t0\t0\t0\n" in p.stdout
    q = TL.run_locate(["--graph=" + SPEC, "--seeds", "--occurrences"], b"AGCGACTAGATAC\n")
    assert q.returncode == 0 and b"S\t0\t13\t1\t2\nE\t4\t7\t7\nB\t1\t2\t0\n" in q.stdout
    for extra in ([], ["--seeds"]):
        p = TL.run_locate(["--graph=" + SPEC, "--msa=" + GOLDEN[0]] + extra, data)
        q = TL.run_locate(["--graph=" + SPEC] + extra, data)
        assert p.returncode == 0 and p.stdout == q.stdout and len(q.stdout) > 0
    # a FASTA of the right shape that is not the graph's MSA
    B = A.copy()
    B[0, 5], B[0, 6] = B[0, 6], B[0, 5]                # the gap moves into the next block: two label lengths change
    bad = tmp_path / "other.fasta"
    write_fasta(str(bad), B, [f"r{i}" for i in range(len(B))])
    p = TL.run_locate(["--graph=" + SPEC, "--msa=" + str(bad), "--occurrences"], data)
    assert p.returncode == 1 and p.stdout == b"" and b"does not fit" in p.stderr
