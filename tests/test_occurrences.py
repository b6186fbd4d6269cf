"""Where each pattern occurs: fbg_pindex_occurrences / fbg_pindex_occurrences_fetch, PatternIndex.occurrences and
fbg_locate --occurrences (include/fbg_hip.h, csrc/locate.hip).

The checker is tests/occ_model.py, a restatement of the definitions over the SA and text of tests/locate_model.py.  CPU
tests pin the model: against locate_model's search, against brute-force substring search that never touches an SA, and
on the example graph of xGFAspec.md.  GPU tests compare every array the device returns with the model."""
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
import occ_model as OM  # noqa: E402
import test_locate as TL  # noqa: E402
from conftest import random_msa  # noqa: E402

SPEC = TL.SPEC
LOCATE = TL.LOCATE

# The model on the example graph of xGFAspec.md (node indices from 0: S id - 1), uncapped:
# pattern -> (restarts, k, t, ends, starts).  Checked by hand against the spec's figure:
#   CGACTA         lies in S_(2,4) = CGA + CTA: it starts at offset 0 and ends at offset 5;
#   AGCGACTAGATAC  is the path 1, 2, 4, 7 (AG CGA CTA GATAC): its first five symbols AGCGA are all of S_(1,2), so the
#                  start is offset 0 of edge (1, 2) and k = 5; the second restart comes after AGCGACTA (t = 8) and the
#                  rest, GATAC, ends with the last symbol of S_(4,7) = CTA + GATAC, offset 7.
SPEC_PLACES = {
    "AG": (0, 0, 0, [(0, 1, 1), (0, 2, 1), (3, 7, 3), (3, 6, 3)], [(0, 1, 0), (0, 2, 0), (3, 7, 2), (3, 6, 2)]),
    "CGACTA": (0, 0, 0, [(1, 3, 5)], [(1, 3, 0)]),
    "GACTAG": (1, 5, 5, [(3, 7, 3), (3, 6, 3)], [(1, 3, 1)]),
    "AGCGACTAGATAC": (2, 5, 8, [(3, 6, 7)], [(0, 1, 0)]),
    "AGCGACTCGTTAC": (2, 5, 8, [(4, 8, 7)], [(0, 1, 0)]),
    "AGCACTCGTTAC": (2, 4, 6, [(4, 8, 7)], [(0, 2, 0)]),
    "AGCAGTT": (0, 0, 0, [], []),
    "GTTACX": (0, 0, 0, [], []),
    "T": (0, 0, 0, [(3, 6, 5), (5, 8, 1), (3, 7, 1), (4, 8, 1), (3, 6, 1), (2, 5, 3), (2, 3, 3), (1, 4, 4), (1, 3, 4),
                    (3, 7, 4), (4, 8, 4), (5, 8, 3), (3, 7, 5), (4, 8, 5), (5, 8, 4)], None),     # starts = ends
    "": (0, 0, 0, [], []),
}


def rows(a):
    return [tuple(int(x) for x in r) for r in a]


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_occurrence_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "fbg_pindex_occurrences") and hasattr(L, "fbg_pindex_occurrences_fetch")
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    assert "int fbg_pindex_occurrences(" in header and "int fbg_pindex_occurrences_fetch(" in header
    assert "fbg_pindex_occurrences" in _lib.SIGNATURES and "fbg_pindex_occurrences_fetch" in _lib.SIGNATURES


def test_model_on_the_spec_example():
    assert set(SPEC_PLACES) == set(TL.SPEC_TABLE)
    ix = OM.Index(*M.read_xgfa(SPEC))
    for p, (restarts, k, t, ends, starts) in SPEC_PLACES.items():
        o = ix.occurrences(p)
        assert (o.count, o.pos) == TL.SPEC_TABLE[p] == ix.locate(p), p
        assert (o.restarts, o.k, o.t) == (restarts, k, t), p
        assert rows(o.ends) == ends and o.end_total == len(ends), p
        want = ends if starts is None else starts
        assert rows(o.starts) == want and o.start_total == len(want), p
        for cap in (0, 1, 3):
            c = ix.occurrences(p, cap)
            assert rows(c.ends) == ends[:cap] and rows(c.starts) == want[:cap], (p, cap)
            assert (c.end_total, c.start_total) == (o.end_total, o.start_total), (p, cap)


def scattered_graph(rng):
    """The generator of test_locate.test_model_counts_edge_string_occurrences_without_restarts."""
    n = int(rng.integers(2, 12))
    labels = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(0, 7)))) for _ in range(n)]
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(int(rng.integers(0, 3 * n)))]
    pats = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(1, 6)))) for _ in range(300)]
    return labels, edges, pats


def chained_graph(rng):
    """Blocks of 1 .. 3 nodes with labels of 2 .. 6 symbols, every node linked to 1 .. 2 nodes of the next block;
    patterns are substrings of the strings spelled by random paths, so that they cross nodes and restart."""
    blocks, labels = [], []
    for _ in range(int(rng.integers(3, 7))):
        size = int(rng.integers(1, 4))
        blocks.append(list(range(len(labels), len(labels) + size)))
        labels += ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(2, 7)))) for _ in range(size)]
    edges = []
    for a, b in zip(blocks, blocks[1:]):
        for u in a:
            edges += [(u, int(v)) for v in rng.choice(b, size=min(len(b), int(rng.integers(1, 3))), replace=False)]
    out = {}
    for u, v in edges:
        out.setdefault(u, []).append(v)
    pats = []
    for _ in range(150):
        u = int(rng.choice(blocks[0]))
        s = labels[u]
        while u in out:
            u = int(rng.choice(out[u]))
            s += labels[u]
        a = int(rng.integers(0, len(s)))
        pats.append(s[a:a + int(rng.integers(1, 16))])
    return labels, edges, pats


def test_model_against_brute_force_on_random_graphs():
    """No SA on the checking side.  Without restarts the places are all substring occurrences in the distinct edge
    strings; with restarts every start holds the first k symbols as a suffix of its edge string and every end holds
    the symbols after the last restart, by string comparison."""
    rng = np.random.default_rng(12)
    plain = restarted = 0
    for trial in range(24):
        labels, edges, pats = scattered_graph(rng) if trial % 2 else chained_graph(rng)
        ix = OM.Index(labels, edges)
        plain_ix = M.Index(labels, edges)
        S = {(u, v): labels[u] + labels[v] for u, v in set(edges)}
        for p in pats:
            o = ix.occurrences(p)
            assert (o.count, o.pos) == plain_ix.locate(p), (labels, edges, p)
            assert o.end_total == len(o.ends) and o.start_total == len(o.starts)
            if o.count == 0:
                assert len(o.ends) == 0 and len(o.starts) == 0
                continue
            ends, starts = rows(o.ends), rows(o.starts)
            assert len(set(ends)) == len(ends) and len(set(starts)) == len(starts)
            if o.restarts == 0:
                want = {(u, v, i) for (u, v), s in S.items() for i in range(len(s) - len(p) + 1) if s.startswith(p, i)}
                assert set(starts) == want, (labels, edges, p)
                assert set(ends) == {(u, v, i + len(p) - 1) for u, v, i in want}, (labels, edges, p)
                assert [(u, v, i + len(p) - 1) for u, v, i in starts] == ends            # slot by slot
                plain += 1
            else:
                assert 0 < o.k <= o.t < len(p)
                for u, v, off in starts:
                    s = S[(u, v)]
                    assert off == len(s) - o.k and s[off:] == p[:o.k], (labels, edges, p)
                for u, v, off in ends:
                    s, rest = S[(u, v)], len(p) - o.t
                    assert off - rest + 1 >= 0 and s[off - rest + 1:off + 1] == p[o.t:], (labels, edges, p)
                restarted += 1
    assert plain > 100 and restarted > 100, (plain, restarted)


def test_tool_occurrences_argument_handling():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    for bad in ("--occurrences=", "--occurrences=x", "--occurrences=-1", "--occurrences=3x", "--occurrences=99999999999999999999999"):
        p = subprocess.run([LOCATE, "--graph=" + SPEC, bad], input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode != 0 and p.stdout == b"" and b"--occurrences" in p.stderr, bad
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--occurrences[=M]" in p.stderr and b"default 64" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

def expected(model, patterns, cap):
    """The arrays of an Occurrences object, from the model."""
    occ = [model.occurrences(p, cap) for p in patterns]
    e = dict(count=[o.count for o in occ], pos=[o.pos for o in occ], restarts=[o.restarts for o in occ],
             end_total=[o.end_total for o in occ], start_total=[o.start_total for o in occ])
    e["end_off"] = np.concatenate(([0], np.cumsum([len(o.ends) for o in occ]))).tolist()
    e["start_off"] = np.concatenate(([0], np.cumsum([len(o.starts) for o in occ]))).tolist()
    ends = np.concatenate([o.ends for o in occ] + [np.zeros((0, 3), dtype=np.int64)])
    starts = np.concatenate([o.starts for o in occ] + [np.zeros((0, 3), dtype=np.int64)])
    for j, f in enumerate(("src", "dst", "offset")):
        e["end_" + f], e["start_" + f] = ends[:, j], starts[:, j]
    return e


FIELDS = ("count", "pos", "restarts", "end_total", "start_total", "end_off", "start_off", "end_src", "end_dst", "end_offset",
          "start_src", "start_dst", "start_offset")


def check_occurrences(pix, model, patterns, cap):
    got = pix.occurrences(patterns, max_per_pattern=cap)
    want = expected(model, patterns, cap)
    for f in FIELDS:
        g = getattr(got, f)
        assert len(g) == len(want[f]), (f, cap)
        assert np.array_equal(np.asarray(g).astype(np.int64), np.asarray(want[f], dtype=np.int64)), (f, cap)
    assert got.search_ms > 0 or len(patterns) == 0
    return got


def check_all_caps(pix, model, patterns):
    """Caps 0, 1, 3, 64 and one above every total; locate before and after is undisturbed.  -> the uncapped result."""
    count0, pos0 = pix.locate(patterns)
    lines0 = pix.stats()["occ_lines"]
    big = None
    for cap in (0, 1, 3, 64, None):
        if cap is None:
            cap = int(max(big.end_total.max(), big.start_total.max())) + 1
        big = check_occurrences(pix, model, patterns, cap)
        assert np.array_equal(big.count, count0) and np.array_equal(big.pos, pos0)
    count1, pos1 = pix.locate(patterns)
    assert np.array_equal(count0, count1) and np.array_equal(pos0, pos1)
    assert pix.stats()["occ_lines"] == lines0
    return big


def assert_every_kind(res, cap_that_cuts=64):
    """The batch holds found patterns with 0, 1 and >= 2 restarts, patterns that are not found, and a list longer than
    the cap: no case passes by being absent."""
    found = res.count > 0
    assert (found & (res.restarts == 0)).any() and (found & (res.restarts == 1)).any() and (found & (res.restarts >= 2)).any()
    assert (~found).any()
    assert (res.end_total > cap_that_cuts).any() and (res.start_total > cap_that_cuts).any()


@pytest.mark.gpu
def test_spec_graph_on_the_gpu(engine):
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    model = OM.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        pats = list(SPEC_PLACES)
        res = check_all_caps(pix, model, pats)
        for k, p in enumerate(pats):
            restarts, _, _, ends, starts = SPEC_PLACES[p]
            assert int(res.restarts[k]) == restarts
            assert rows(res.ends(k)) == ends and rows(res.starts(k)) == (ends if starts is None else starts)
        # as_nodes: AG ends at offset 1 of node 0 (twice, once per edge: one row) and at offset 0 of nodes 6 and 7
        k = pats.index("AG")
        assert rows(res.as_nodes("end")[k]) == [(0, 1), (6, 0), (7, 0)]
        assert rows(res.as_nodes("start")[k]) == [(0, 0), (3, 2)]
        assert rows(res.as_nodes("end")[pats.index("")]) == []
        check_all_caps(pix, model, TL.sample_patterns(np.random.default_rng(5), np.array([list(b"AGCGACTAGATAC")], dtype=np.uint8), 3000))
        assert len(pix.occurrences([]).count) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", TL.SEG_CASES, ids=[c["name"] for c in TL.SEG_CASES])
def test_segmented_graphs_match_the_model(engine, case):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(case["seed"])
    msa = random_msa(rng, case["m"], case["n"], gap_p=case.get("gap_p", 0.0), gap_run=case.get("gap_run", 1),
                     similar=case.get("similar", 0.0), n_p=case.get("n_p", 0.0))
    f = engine.elastic_f(msa, ignorechars=case.get("ignore", ""))
    b = engine.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(engine, msa, b)
    model = OM.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        res = check_all_caps(pix, model, TL.sample_patterns(rng, msa, 10_000, alphabet=b"ACGTN"))
        assert_every_kind(res)


def uneven_patterns(rng, labels, edges):
    """120 patterns of 300 symbols cut from walks through the graph (they cross several nodes, so they restart; a walk
    that ends early is padded and not found), every tenth followed by a 1-symbol pattern and the empty one."""
    out = {}
    for u, v in edges:
        out.setdefault(u, []).append(v)
    pats = []
    for k in range(120):
        u = int(rng.choice(list(out)))
        s = labels[u][int(rng.integers(0, len(labels[u]))):]
        while len(s) < 300 and u in out:
            u = int(rng.choice(out[u]))
            s += labels[u]
        pats.append(s[:300].ljust(300, b"A"))
        if k % 10 == 0:
            pats += [b"ACGT"[(k // 10) % 4:(k // 10) % 4 + 1], b""]
    return pats


@pytest.mark.gpu
def test_uneven_ranges_on_a_text_beyond_a_million_symbols(engine):
    """1-symbol patterns (ranges of about N / 4 slots) next to 300-symbol ones (one slot or none) in one batch, with
    a cap that lets one pattern report more than 10^5 places."""
    rng = np.random.default_rng(31)
    n = 4000
    anc = rng.integers(0, 4, 120)
    labels = []
    for _ in range(n):       # the graph of test_locate.test_text_beyond_a_million_symbols
        x = anc[:int(rng.integers(60, 120))].copy()
        mut = rng.random(len(x)) < 0.03
        x[mut] = rng.integers(0, 4, int(mut.sum()))
        labels.append(bytes(b"ACGT"[i] for i in x))
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 8000), rng.integers(0, n, 8000))]
    model = OM.Index(labels, edges)
    assert model.N + 1 > 1_000_000
    pats = uneven_patterns(rng, labels, model.edges)
    with engine.pattern_index(labels, edges) as pix:
        _, sa, _, _ = pix.download()
        assert np.array_equal(sa.astype(np.int64), model.SA)
        cap = 150_000
        res = check_occurrences(pix, model, pats, cap)
        sizes = np.diff(res.end_off.astype(np.int64))
        assert sizes.max() > 100_000 and (sizes == 1).any() and (sizes == 0).any()
        assert (res.end_total > cap).any()                       # and one list is cut even by this cap
        long_found = np.array([len(p) == 300 for p in pats]) & (res.count > 0)
        assert long_found.sum() > 20 and (res.restarts[long_found] >= 2).any()
        assert ((res.count == 0) & (res.restarts > 0)).any()      # restarts of a search that failed later are reported
        check_occurrences(pix, model, pats, 64)
        # a capped list of 2^32 entries or more: refused after the sizes, before any place is allocated, and it
        # leaves nothing to fetch
        import founderblockgraphs_amd as F
        from founderblockgraphs_amd import _lib
        per = model.occurrences(b"A").end_total
        many = (1 << 32) // per + 1
        with pytest.raises(F.FbgError) as ei:
            pix.occurrences([b"A"] * many, max_per_pattern=1 << 40)
        assert ei.value.code == _lib.FBG_ERR_TOO_LARGE
        six = [np.zeros(8, dtype=np.uint32) for _ in range(6)]
        assert _lib.lib().fbg_pindex_occurrences_fetch(pix._h, *[x.ctypes.data_as(_lib.u32p) for x in six], None) == _lib.FBG_ERR_INVALID
        res = check_occurrences(pix, model, pats, 64)              # and the index still answers
        assert int(res.end_off[-1]) < (1 << 32)


@pytest.mark.gpu
def test_protein_alphabet_takes_the_general_layout(engine):
    rng = np.random.default_rng(21)
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    n = 300
    labels = [bytes(alpha[i] for i in rng.integers(0, 20, int(rng.integers(0, 30)))) for _ in range(n)]
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(900)]
    model = OM.Index(labels, edges)
    assert int(model.present.sum()) > 16
    with engine.pattern_index(labels, edges) as pix:
        seqs = np.array([list((labels[u] + labels[v]).ljust(60, b"A")[:60]) for u, v in edges[:200]], dtype=np.uint8)
        res = check_all_caps(pix, model, TL.sample_patterns(rng, seqs, 10_000, alphabet=alpha))
        assert (res.count > 0).sum() > 1000 and (res.end_total > 64).any()


@pytest.mark.gpu
def test_graph_without_edges_has_no_places(engine):
    labels, edges = [b"ACGT", b"ACGA", b""], []
    model = OM.Index(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        res = check_occurrences(pix, model, [b"", b"A", b"ACGT", b"T"], 64)
        assert res.count.tolist() == [0, 0, 0, 0] and len(res.end_src) == 0


@pytest.mark.gpu
def test_errors_and_partial_fetches(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    labels, edges = F.read_xgfa(SPEC)
    model = OM.Index(labels, edges)
    pats = ["T", "AGCGACTAGATAC", "GACTAG", "AGCAGTT"]
    data = np.frombuffer("".join(pats).encode() + b"\0", dtype=np.uint8).copy()
    off = np.concatenate(([0], np.cumsum([len(p) for p in pats]))).astype(np.uint64)
    k = len(pats)
    cnt, pos, et, st = (np.zeros(k, dtype=np.uint64) for _ in range(4))
    eoff, soff = np.zeros(k + 1, dtype=np.uint64), np.zeros(k + 1, dtype=np.uint64)
    rs = np.zeros(k, dtype=np.uint32)
    ms = ctypes.c_double(0)
    six = [np.zeros(64, dtype=np.uint32) for _ in range(6)]
    INVALID = _lib.FBG_ERR_INVALID
    assert L.fbg_pindex_occurrences(None, _lib.u8p(), u64(off), k, 3, u64(cnt), u64(pos), u32(rs), u64(eoff), u64(soff), u64(et),
                                    u64(st), None) == INVALID
    assert L.fbg_pindex_occurrences_fetch(None, *[u32(a) for a in six], None) == INVALID
    with engine.pattern_index(labels, edges) as pix:
        h = pix._h
        d8 = data.ctypes.data_as(_lib.u8p)
        # a fetch before any search
        assert L.fbg_pindex_occurrences_fetch(h, *[u32(a) for a in six], ctypes.byref(ms)) == INVALID
        # a missing required pointer
        assert L.fbg_pindex_occurrences(h, d8, u64(off), k, 3, u64(cnt), u64(pos), u32(rs), None, u64(soff), u64(et), u64(st),
                                        None) == INVALID
        assert L.fbg_pindex_occurrences(h, d8, None, k, 3, u64(cnt), u64(pos), u32(rs), u64(eoff), u64(soff), u64(et), u64(st),
                                        None) == INVALID
        assert L.fbg_pindex_occurrences(h, d8, u64(off), k, 3, u64(cnt), u64(pos), None, u64(eoff), u64(soff), u64(et), u64(st),
                                        None) == INVALID
        # ... does not leave something to fetch
        assert L.fbg_pindex_occurrences_fetch(h, *[u32(a) for a in six], None) == INVALID
        assert L.fbg_pindex_occurrences(h, d8, u64(off), k, 3, u64(cnt), u64(pos), u32(rs), u64(eoff), u64(soff), u64(et), u64(st),
                                        ctypes.byref(ms)) == 0
        want = expected(model, pats, 3)
        assert eoff.tolist() == want["end_off"] and soff.tolist() == want["start_off"] and rs.tolist() == want["restarts"]
        ne, ns = int(eoff[k]), int(soff[k])
        # one array of a list missing
        assert L.fbg_pindex_occurrences_fetch(h, u32(six[0]), None, u32(six[2]), None, None, None, None) == INVALID
        # only the ends, only the starts, both, and both again: a locate in between does not disturb the ranges
        for a in six:
            a[:] = 0xdeadbeef
        assert L.fbg_pindex_occurrences_fetch(h, u32(six[0]), u32(six[1]), u32(six[2]), None, None, None, ctypes.byref(ms)) == 0
        assert [a[:ne].tolist() for a in six[:3]] == [want["end_" + f].tolist() for f in ("src", "dst", "offset")]
        assert all((a == 0xdeadbeef).all() for a in six[3:]) and all((a[ne:] == 0xdeadbeef).all() for a in six[:3])
        pix.locate(["ACGT" * 20, "T"])
        for a in six:
            a[:] = 0xdeadbeef
        assert L.fbg_pindex_occurrences_fetch(h, None, None, None, u32(six[3]), u32(six[4]), u32(six[5]), None) == 0
        assert [a[:ns].tolist() for a in six[3:]] == [want["start_" + f].tolist() for f in ("src", "dst", "offset")]
        assert all((a == 0xdeadbeef).all() for a in six[:3]) and all((a[ns:] == 0xdeadbeef).all() for a in six[3:])
        for _ in range(2):
            assert L.fbg_pindex_occurrences_fetch(h, *[u32(a) for a in six], None) == 0
            assert [a[:ne].tolist() for a in six[:3]] == [want["end_" + f].tolist() for f in ("src", "dst", "offset")]
            assert [a[:ns].tolist() for a in six[3:]] == [want["start_" + f].tolist() for f in ("src", "dst", "offset")]
        assert L.fbg_pindex_occurrences_fetch(h, None, None, None, None, None, None, None) == 0
        with pytest.raises(ValueError):
            pix.occurrences(pats, max_per_pattern=-1)


def tool_lines(model, ids, data, cap):
    """What fbg_locate --occurrences=cap prints for stdin `data`."""
    out, found = [], 0
    toks = M.tokens(data)
    for t in toks:
        o = model.occurrences(t, cap)
        out.append(b"Pattern? %d occurrences found.\n" % o.count)
        found += o.count != 0
        for tag, places, total in ((b"E", o.ends, o.end_total), (b"B", o.starts, o.start_total)):
            out += [b"%s\t%d\t%d\t%d\n" % (tag, ids[a], ids[b], off) for a, b, off in rows(places)]
            if total > len(places):
                out.append(b"%s\t...\t%d more\n" % (tag, total - len(places)))
    out.append(b"Pattern? %d out of %d patterns found\n" % (found, len(toks)))
    return b"".join(out)


@pytest.mark.gpu
def test_tool_prints_the_places():
    model = OM.Index(*M.read_xgfa(SPEC))
    ids = list(range(1, 10))                                      # the S ids of the file, ascending
    data = b"AGCGACTAGATAC AGCAGTT CGACTA T GACTAG AG\n"
    p = TL.run_locate(["--graph=" + SPEC, "--occurrences=2"], data)
    assert p.returncode == 0, p.stderr
    assert p.stdout == tool_lines(model, ids, data, 2)
    assert b"E\t4\t7\t7\nB\t1\t2\t0\n" in p.stdout and b"E\t...\t13 more\n" in p.stdout
    p = TL.run_locate(["--graph=" + SPEC, "--occurrences"], data)
    assert p.returncode == 0 and p.stdout == tool_lines(model, ids, data, 64)
    p = TL.run_locate(["--graph=" + SPEC, "--occurrences=0"], data)
    assert p.returncode == 0 and p.stdout == tool_lines(model, ids, data, 0)
    # without the flag: what test_locate.test_tool_on_the_spec_graph expects
    p = TL.run_locate(["--graph=" + SPEC], b"AGCGACTAGATAC AGCAGTT CGACTA\n")
    assert p.stdout == (b"Pattern? 1 occurrences found.\nPattern? 0 occurrences found.\nPattern? 1 occurrences found.\n"
                        b"Pattern? 2 out of 3 patterns found\n")
    assert p.stdout == M.expected_stdout(model, b"AGCGACTAGATAC AGCAGTT CGACTA\n")[0]
