"""Maximal exact-match seeds: fbg_pindex_seeds / _fetch / _places, PatternIndex.seeds and fbg_locate --seeds
(include/fbg_hip.h, csrc/locate.hip).

The checker is tests/seeds_model.py: the greedy loop of the definition over locate_model's search, every seed's fields
from occ_model's occurrences of that substring.  CPU tests pin the loop against a brute-force search for the longest
accepted prefix at every start; GPU tests compare every array the device returns with the model, for minimum lengths 1, 2
and 5 and caps 0, 1, 3 and 64.

Of the errors the header lists, "2^32 reported seeds or more" is the one no test provokes: it takes a batch of more than
2^32 symbols."""
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
import seeds_model as SM  # noqa: E402
import test_locate as TL  # noqa: E402
import test_occurrences as TO  # noqa: E402
from conftest import random_msa  # noqa: E402

SPEC = TL.SPEC
LOCATE = TL.LOCATE
LENGTHS = (1, 2, 5)
CAPS = (0, 1, 3, 64)
# the four paths of the example graph of xGFAspec.md (its P lines), spelled out
SPEC_ROWS = [b"AGCGACTAGATAC", b"AGCACTAGTT", b"AGCGACTCGTTAC", b"AGCACTGTTAC"]

OCC_FIELDS = ("count", "pos", "restarts", "end_total", "start_total", "end_off", "start_off", "end_src", "end_dst", "end_offset",
              "start_src", "start_dst", "start_offset")


class Model:
    """occ_model.Index with the cuts of every read and the occurrences of every (substring, cap) computed once."""

    def __init__(self, labels, edges):
        self.ix = OM.Index(labels, edges)
        self._cuts, self._occ = {}, {}

    def cuts(self, read):
        read = M.as_bytes(read)
        if read not in self._cuts:
            self._cuts[read] = SM.cuts(self.ix, read)
        return self._cuts[read]

    def occ(self, sub, cap):
        if (sub, cap) not in self._occ:
            self._occ[(sub, cap)] = self.ix.occurrences(sub, cap)
        return self._occ[(sub, cap)]

    def expected(self, reads, L, cap):
        """The arrays of a Seeds object and of its occ, from the model."""
        reads = [M.as_bytes(r) for r in reads]
        kept = [[(i, k) for i, k in self.cuts(r) if k >= L] for r in reads]
        e = dict(seed_off=np.concatenate(([0], np.cumsum([len(c) for c in kept]))).tolist(),
                 q_start=[i for c in kept for i, _ in c], length=[k for c in kept for _, k in c],
                 pattern_of=[j for j, c in enumerate(kept) for _ in c])
        occ = [self.occ(r[i:i + k], cap) for r, c in zip(reads, kept) for i, k in c]
        assert all(o.count > 0 and o.pos == k for o, k in zip(occ, e["length"]))
        e.update(count=[o.count for o in occ], pos=[o.pos for o in occ], restarts=[o.restarts for o in occ],
                 end_total=[o.end_total for o in occ], start_total=[o.start_total for o in occ])
        e["end_off"] = np.concatenate(([0], np.cumsum([len(o.ends) for o in occ]))).tolist()
        e["start_off"] = np.concatenate(([0], np.cumsum([len(o.starts) for o in occ]))).tolist()
        ends = np.concatenate([o.ends for o in occ] + [np.zeros((0, 3), dtype=np.int64)])
        starts = np.concatenate([o.starts for o in occ] + [np.zeros((0, 3), dtype=np.int64)])
        for j, f in enumerate(("src", "dst", "offset")):
            e["end_" + f], e["start_" + f] = ends[:, j], starts[:, j]
        return e


def same(got, want, what):
    assert len(got) == len(want), what
    assert np.array_equal(np.asarray(got).astype(np.int64), np.asarray(want, dtype=np.int64)), what


def check_seeds(pix, model, reads, L, cap, given=None):
    """given: the reads as the (bytes, offsets) pair handed to the call, when that is not the list itself."""
    got = pix.seeds(reads if given is None else given, min_length=L, max_per_seed=cap)
    want = model.expected(reads, L, cap)
    for f in ("seed_off", "q_start", "length", "pattern_of"):
        same(getattr(got, f), want[f], (f, L, cap))
    for f in OCC_FIELDS:
        same(getattr(got.occ, f), want[f], (f, L, cap))
    assert len(got) == len(want["q_start"])
    return got


def check_all(pix, model, reads):
    """Every minimum length with every cap.  -> the result for L = 1, cap = 64."""
    out = None
    for L in LENGTHS:
        for cap in CAPS:
            res = check_seeds(pix, model, reads, L, cap)
            if (L, cap) == (1, 64):
                out = res
    return out


def substitute(rng, s, at, alphabet):
    """Another symbol of the alphabet at position `at`."""
    s[at] = rng.choice([c for c in alphabet if c != s[at]])


def make_reads(rng, rows, n, alphabet=b"ACGT", max_len=100):
    """Reads cut from the rows: unchanged, with one and with three substitutions, with one at the first and one at the
    last symbol, with two adjacent ones, and with a byte that the text does not hold ('X').  Then the empty read, 'X'
    alone, one symbol of a row alone, and every row whole."""
    rows = [bytes(r) for r in rows if len(r)]
    out = []
    for j in range(n):
        r = rows[int(rng.integers(0, len(rows)))]
        ln = int(rng.integers(1, min(max_len, len(r)) + 1))
        a = int(rng.integers(0, len(r) - ln + 1))
        s = bytearray(r[a:a + ln])
        kind = j % 7
        if kind == 1:
            substitute(rng, s, int(rng.integers(0, ln)), alphabet)
        elif kind == 2:
            for _ in range(3):
                substitute(rng, s, int(rng.integers(0, ln)), alphabet)
        elif kind == 3:
            substitute(rng, s, 0, alphabet)
        elif kind == 4:
            substitute(rng, s, ln - 1, alphabet)
        elif kind == 5 and ln >= 2:
            at = int(rng.integers(0, ln - 1))
            substitute(rng, s, at, alphabet)
            substitute(rng, s, at + 1, alphabet)
        elif kind == 6:
            s[int(rng.integers(0, ln))] = ord("X")
        out.append(bytes(s))
    return out + [b"", b"X", rows[0][:1]] + rows


def assert_every_kind(model, reads):
    """The batch holds a seed found after a restart, a read without a seed, a read that is one whole-read seed, and for
    either minimum length above 1 a seed that it drops: no case passes by being absent."""
    cuts = [model.cuts(r) for r in reads]
    assert any(model.occ(M.as_bytes(r)[i:i + k], 0).restarts > 0 for r, c in zip(reads, cuts) for i, k in c)
    assert any(len(r) > 0 and not c for r, c in zip(reads, cuts))
    assert any(len(r) > 1 and c == [(0, len(r))] for r, c in zip(reads, cuts))
    for L in LENGTHS[1:]:
        assert any(k < L for c in cuts for _, k in c), L
    assert any(len(c) >= 3 for c in cuts)


def spec_reads():
    return make_reads(np.random.default_rng(7), SPEC_ROWS, 140, max_len=13)


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_seed_calls_and_the_header_declares_them():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    for name in ("fbg_pindex_seeds", "fbg_pindex_seeds_fetch", "fbg_pindex_seeds_places"):
        assert hasattr(L, name), name
        assert f"int {name}(" in header, name
        assert name in _lib.SIGNATURES, name


def test_model_is_the_longest_accepted_prefix_at_every_start():
    """Brute force: for every start i of every pattern, the k of the loop (pos of the search of P[i:]) is the largest j
    for which the search of P[i : i + j] alone is found with pos == j, found by trying every j; and every shorter prefix
    is found too (the state after j symbols depends on those symbols only).  The greedy cuts follow from those k."""
    rng = np.random.default_rng(12)
    multi = skipped = 0
    for trial in range(12):
        labels, edges, pats = TO.scattered_graph(rng) if trial % 2 else TO.chained_graph(rng)
        ix = OM.Index(labels, edges)
        for p in pats[:40]:
            P = bytearray(M.as_bytes(p) + M.as_bytes(pats[int(rng.integers(0, len(pats)))]))     # two patterns joined
            if trial % 3 == 0:
                P[int(rng.integers(0, len(P)))] = ord("X")
            P = bytes(P)
            ks = []
            for i in range(len(P)):
                alone = [ix.locate(P[i:i + j]) for j in range(1, len(P) - i + 1)]
                found = [j for j, (count, pos) in enumerate(alone, 1) if count > 0 and pos == j]
                k = ix.locate(P[i:])[1]
                assert k == (max(found) if found else 0), (labels, edges, P, i)
                assert found == list(range(1, k + 1)), (labels, edges, P, i)
                ks.append(k)
            want, i = [], 0
            while i < len(P):
                if ks[i]:
                    want.append((i, ks[i]))
                i += max(ks[i], 1)
            assert SM.cuts(ix, P) == want
            for L in LENGTHS:
                got = SM.seeds(ix, P, L, 3)
                assert [(s.q_start, s.length) for s in got] == [c for c in want if c[1] >= L]
                for s in got:
                    o = ix.occurrences(P[s.q_start:s.q_start + s.length], 3)
                    assert (s.occ.count, s.occ.pos, s.occ.restarts) == (o.count, s.length, o.restarts) and o.count > 0
            multi += len(want) > 1
            skipped += sum(k for _, k in want) < len(P)
    assert multi > 100 and skipped > 20, (multi, skipped)
    assert SM.seeds(OM.Index(["AC", "GT"], [(0, 1)]), b"", 1, 3) == []


def test_spec_batch_holds_every_kind_in_the_model():
    model = Model(*M.read_xgfa(SPEC))
    assert_every_kind(model, spec_reads())
    assert SM.cuts(model.ix, b"AGCGACTAGATAC") == [(0, 13)] and SM.cuts(model.ix, b"AGCAGTT") == [(0, 4), (4, 3)]


def test_tool_seeds_argument_handling():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    missing = os.path.join(HERE, "golden", "no_such_graph.xgfa")          # never read: the arguments fail first
    for bad in ("--seeds=0", "--seeds=x", "--seeds=", "--seeds=-1", "--seeds=3x"):
        p = subprocess.run([LOCATE, "--graph=" + missing, bad], input=b"AG\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--seeds takes" in p.stderr, bad
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--seeds[=L]" in p.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_spec_graph_on_the_gpu(engine):
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    model = Model(labels, edges)
    reads = spec_reads()
    assert_every_kind(model, reads)
    with engine.pattern_index(labels, edges) as pix:
        res = check_all(pix, model, reads)
        k = reads.index(b"AGCGACTAGATAC")
        assert res.of(k).tolist() == [[0, 13, 1]] and int(res.occ.restarts[int(res.seed_off[k])]) == 2
        j = int(res.seed_off[k])
        assert TO.rows(res.occ.ends(j)) == [(3, 6, 7)] and TO.rows(res.occ.starts(j)) == [(0, 1, 0)]
        assert TO.rows(res.occ.as_nodes("end")[j]) == [(6, 4)]
        assert res.of(reads.index(b"")).shape == (0, 3) and res.of(reads.index(b"X")).shape == (0, 3)
        assert res.search_ms > 0
        for bad in (dict(min_length=0), dict(max_per_seed=-1)):
            with pytest.raises(ValueError):
                pix.seeds(reads, **bad)


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
    model = Model(labels, edges)
    rows = [r[r != ord("-")].tobytes() for r in msa]
    reads = make_reads(rng, rows[:6], 350, alphabet=b"ACGT")
    assert_every_kind(model, reads)
    with engine.pattern_index(labels, edges) as pix:
        check_all(pix, model, reads)


@pytest.mark.gpu
def test_reads_and_seeds_at_every_offset_of_a_pattern_word(engine):
    """70 reads of 1 .. 70 symbols back to back: reads start at every offset modulo 8 of the pattern buffer, and with a
    substitution in each of them so do seeds.  Then the same bytes behind 5 bytes that belong to no read (pat_off[0] > 0,
    the rebase), and the empty read alone."""
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    model = Model(labels, edges)
    rng = np.random.default_rng(3)
    long_row = b"".join(SPEC_ROWS[int(i)] for i in rng.integers(0, 4, 12))
    reads = []
    for ln in range(1, 71):
        a = int(rng.integers(0, len(long_row) - ln + 1))
        s = bytearray(long_row[a:a + ln])
        if ln % 3 == 0:
            s[int(rng.integers(0, ln))] = ord("X")
        reads.append(bytes(s))
    starts = np.concatenate(([0], np.cumsum([len(r) for r in reads])))
    seed_at = {(int(starts[j]) + i) % 8 for j, r in enumerate(reads) for i, _ in model.cuts(r)}
    assert {int(x) % 8 for x in starts[:-1]} == set(range(8)) and seed_at == set(range(8))
    with engine.pattern_index(labels, edges) as pix:
        check_all(pix, model, reads)
        data = np.frombuffer(b"#####" + b"".join(reads) + b"\0", dtype=np.uint8).copy()
        off = (starts + 5).astype(np.uint64)
        for L in LENGTHS:
            for cap in CAPS:
                check_seeds(pix, model, reads, L, cap, given=(data[:-1], off))
        for batch in ([b""], [b"", b""], []):
            res = pix.seeds(batch, min_length=1, max_per_seed=3)
            assert res.seed_off.tolist() == [0] * (len(batch) + 1) and len(res) == 0 and len(res.occ.end_src) == 0


@pytest.mark.gpu
def test_a_read_with_a_seed_per_symbol_next_to_reads_with_one(engine):
    """Labels A and C, the one edge A -> C: the text holds both symbols and the bigram AC only.  CACA... of 4096
    symbols has a seed at every other symbol, CCCC... one per symbol; beside them reads of one seed, in one wave.  Then
    300 reads, so that more than one workgroup runs and the lanes of a wave write very different numbers of seeds."""
    labels, edges = [b"A", b"C"], [(0, 1)]
    model = Model(labels, edges)
    fan = [b"CA" * 2048, b"C" * 4096]
    assert len(model.cuts(fan[0])) == 2049 and len(model.cuts(fan[1])) == 4096
    assert model.cuts(b"AC") == [(0, 2)] and model.cuts(b"A") == [(0, 1)]
    small = [fan[0], b"AC", b"A", fan[1], b"C", b"AC", b""]
    rng = np.random.default_rng(9)
    many = []
    for j in range(300):
        ln = int(rng.integers(0, 40)) if j % 50 else 1000 + j
        many.append(bytes(b"ACX"[i] for i in rng.choice(3, ln, p=(0.45, 0.45, 0.1))))
    many[17], many[290] = fan[0], fan[1]
    with engine.pattern_index(labels, edges) as pix:
        res = check_all(pix, model, small)
        assert np.diff(res.seed_off.astype(np.int64)).tolist() == [2049, 1, 1, 4096, 1, 1, 0]
        res = check_all(pix, model, many)
        per = np.diff(res.seed_off.astype(np.int64))
        assert per.max() == 4096 and (per == 0).any() and (per == 1).any() and len(per) > 256


@pytest.mark.gpu
def test_protein_alphabet_takes_the_general_layout(engine):
    rng = np.random.default_rng(21)
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    n = 300
    labels = [bytes(alpha[i] for i in rng.integers(0, 20, int(rng.integers(0, 30)))) for _ in range(n)]
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(900)]
    model = Model(labels, edges)
    assert int(model.ix.present.sum()) > 16
    rows = [(labels[u] + labels[v]) for u, v in edges[:200]]
    reads = make_reads(rng, rows, 350, alphabet=alpha, max_len=60)
    assert_every_kind(model, reads)
    with engine.pattern_index(labels, edges) as pix:
        check_all(pix, model, reads)


@pytest.mark.gpu
def test_a_text_beyond_a_million_symbols(engine):
    """The graph of test_occurrences.test_uneven_ranges_on_a_text_beyond_a_million_symbols: one-symbol seeds with
    ranges of about N / 4 slots next to seeds of hundreds of symbols with one."""
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
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
    model = Model(labels, edges)
    assert model.ix.N + 1 > 1_000_000
    reads = []
    for p in TO.uneven_patterns(rng, labels, model.ix.edges):
        s = bytearray(p)
        for _ in range(len(s) // 100):
            s[int(rng.integers(0, len(s)))] = b"ACGTX"[int(rng.integers(0, 5))]
        reads.append(bytes(s))
    reads += [b"AXCXGXT", b"X"]
    assert len(reads) > 140
    with engine.pattern_index(labels, edges) as pix:
        res = check_all(pix, model, reads)
        assert res.occ.end_total.max() > 200_000 and (res.occ.end_total == 1).any() and (res.occ.restarts >= 2).any()
        # a capped place list of 2^32 entries or more: refused after the sizes, nothing is left to fetch, and the index
        # still answers
        per = model.occ(b"A", 0).end_total
        many = (1 << 32) // per + 1
        with pytest.raises(F.FbgError) as ei:
            pix.seeds([b"AX" * many], max_per_seed=1 << 40)
        assert ei.value.code == _lib.FBG_ERR_TOO_LARGE
        six = [np.zeros(8, dtype=np.uint32) for _ in range(6)]
        L = _lib.lib()
        assert L.fbg_pindex_seeds_places(pix._h, *[x.ctypes.data_as(_lib.u32p) for x in six], None) == _lib.FBG_ERR_INVALID
        assert L.fbg_pindex_seeds_fetch(pix._h, *([None] * 9)) == _lib.FBG_ERR_INVALID
        check_seeds(pix, model, reads, 1, 1)


@pytest.mark.gpu
def test_seeds_are_the_occurrences_of_their_substrings_on_the_gpu(engine):
    """No model: ix.seeds(reads) against ix.occurrences of every seed's substring."""
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(4)
    msa = random_msa(rng, 24, 900, gap_p=0.02, gap_run=3)
    f = engine.elastic_f(msa)
    b = engine.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(engine, msa, b)
    rows = [r[r != ord("-")].tobytes() for r in msa]
    reads = make_reads(rng, rows, 2000)
    with engine.pattern_index(labels, edges) as pix:
        for L, cap in ((1, 64), (2, 3), (5, 0), (5, 1)):
            res = pix.seeds(reads, min_length=L, max_per_seed=cap)
            assert len(res) > 1000 and (res.length.astype(np.int64) >= L).all()
            subs = [reads[int(k)][int(q):int(q) + int(n)] for k, q, n in zip(res.pattern_of, res.q_start, res.length)]
            occ = pix.occurrences(subs, max_per_pattern=cap)
            for fld in OCC_FIELDS:
                same(getattr(res.occ, fld), getattr(occ, fld), (fld, L, cap))
            assert (occ.count > 0).all()
            q, ln, off = res.q_start.astype(np.int64), res.length.astype(np.int64), res.seed_off.astype(np.int64)
            for k in range(len(reads)):                  # a read's seeds are in order and do not overlap
                a, z = off[k], off[k + 1]
                assert (q[a + 1:z] >= q[a:z - 1] + ln[a:z - 1]).all() and (z == a or q[z - 1] + ln[z - 1] <= len(reads[k]))


def raw_places(fn, h, ne, ns):
    from founderblockgraphs_amd import _lib
    six = [np.zeros(max(n, 1), dtype=np.uint32) for n in (ne, ne, ne, ns, ns, ns)]
    assert fn(h, *[a.ctypes.data_as(_lib.u32p) for a in six], None) == 0
    return [a[:n].tolist() for a, n in zip(six, (ne, ne, ne, ns, ns, ns))]


@pytest.mark.gpu
def test_seeds_and_occurrences_keep_their_results_apart(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    labels, edges = F.read_xgfa(SPEC)
    model = Model(labels, edges)
    A = ["T", "AGCGACTAGATAC", "GACTAG", "AGCAGTT", "AG"]
    B = spec_reads()
    with engine.pattern_index(labels, edges) as pix:
        want_a = TO.expected(model.ix, A, 3)
        want_b = model.expected(B, 2, 3)
        places = lambda w: [np.asarray(w[k + "_" + f]).tolist() for k in ("end", "start") for f in ("src", "dst", "offset")]  # noqa: E731
        count0, pos0 = pix.locate(A)
        stats0 = pix.stats()
        # occurrences(A), seeds(B): the occurrence fetch still returns A's places, the seed fetch B's
        pix.occurrences(A, max_per_pattern=3)
        pix.seeds(B, min_length=2, max_per_seed=3)
        assert pix.stats() == stats0
        assert raw_places(L.fbg_pindex_occurrences_fetch, pix._h, len(want_a["end_src"]), len(want_a["start_src"])) == places(want_a)
        assert raw_places(L.fbg_pindex_seeds_places, pix._h, len(want_b["end_src"]), len(want_b["start_src"])) == places(want_b)
        # seeds(B), occurrences(A): the same
        pix.seeds(B, min_length=2, max_per_seed=3)
        pix.occurrences(A, max_per_pattern=3)
        assert raw_places(L.fbg_pindex_seeds_places, pix._h, len(want_b["end_src"]), len(want_b["start_src"])) == places(want_b)
        assert raw_places(L.fbg_pindex_occurrences_fetch, pix._h, len(want_a["end_src"]), len(want_a["start_src"])) == places(want_a)
        # locate and the statistics of the last locate, and a validation, around a seeds call
        v0 = pix.validate([0, 1, 1, 2, 2, 2, 3, 3, 3])
        count1, pos1 = pix.locate(A)
        stats1 = pix.stats()
        pix.seeds(B)
        assert pix.stats() == stats1
        count2, pos2 = pix.locate(A)
        assert np.array_equal(count0, count1) and np.array_equal(count1, count2) and np.array_equal(pos0, pos2)
        assert pix.stats()["occ_lines"] == stats0["occ_lines"]
        assert np.array_equal(pix.validate([0, 1, 1, 2, 2, 2, 3, 3, 3]).status, v0.status)


@pytest.mark.gpu
def test_graph_without_edges_has_no_seeds(engine):
    labels, edges = [b"ACGT", b"ACGA", b""], []
    model = Model(labels, edges)
    with engine.pattern_index(labels, edges) as pix:
        for L in LENGTHS:
            for cap in CAPS:
                res = check_seeds(pix, model, [b"", b"A", b"ACGT", b"T", b"#"], L, cap)
                assert res.seed_off.tolist() == [0] * 6 and len(res.occ.end_src) == 0 and len(res.occ.start_src) == 0


@pytest.mark.gpu
def test_a_pattern_with_a_separator_is_searched_like_any_other(engine):
    import founderblockgraphs_amd as F
    labels, edges = F.read_xgfa(SPEC)
    model = Model(labels, edges)
    reads = [b"AG#CGA", b"#", b"GATAC#AGCGA", b"CTA#", b"A\0G", b"##"]
    with engine.pattern_index(labels, edges) as pix:
        check_all(pix, model, reads)


@pytest.mark.gpu
def test_errors_and_partial_fetches(engine):
    import founderblockgraphs_amd as F
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)      # noqa: E731
    labels, edges = F.read_xgfa(SPEC)
    model = Model(labels, edges)
    reads = ["T", "AGCGACTAGATAC", "GACTAGX", "AGCAGTT", ""]
    data = np.frombuffer("".join(reads).encode() + b"\0", dtype=np.uint8).copy()
    off = np.concatenate(([0], np.cumsum([len(p) for p in reads]))).astype(np.uint64)
    k = len(reads)
    soff = np.zeros(k + 1, dtype=np.uint64)
    ms = ctypes.c_double(0)
    six = [np.zeros(64, dtype=np.uint32) for _ in range(6)]
    INVALID, TOO_LARGE = _lib.FBG_ERR_INVALID, _lib.FBG_ERR_TOO_LARGE
    d8 = data.ctypes.data_as(_lib.u8p)
    assert L.fbg_pindex_seeds(None, d8, u64(off), k, 1, 3, u64(soff), None) == INVALID
    assert L.fbg_pindex_seeds_fetch(None, *([None] * 9)) == INVALID
    assert L.fbg_pindex_seeds_places(None, *[u32(a) for a in six], None) == INVALID
    with engine.pattern_index(labels, edges) as pix:
        h = pix._h
        want = model.expected(reads, 1, 3)
        ns = len(want["q_start"])

        def good():
            soff[:] = 7
            assert L.fbg_pindex_seeds(h, d8, u64(off), k, 1, 3, u64(soff), ctypes.byref(ms)) == 0
            assert soff.tolist() == want["seed_off"] and ms.value > 0

        # a fetch or places call before any search
        assert L.fbg_pindex_seeds_fetch(h, *([None] * 9)) == INVALID
        assert L.fbg_pindex_seeds_places(h, *[u32(a) for a in six], ctypes.byref(ms)) == INVALID
        good()
        bad_off = off.copy()
        bad_off[2] = 0                                                       # decreasing offsets
        huge = np.array([0, 1 << 32], dtype=np.uint64)                       # a pattern of 2^32 symbols (never read)
        for rc, call in (
                (INVALID, lambda: L.fbg_pindex_seeds(h, d8, u64(off), k, 1, 3, None, None)),            # no seed_off
                (INVALID, lambda: L.fbg_pindex_seeds(h, d8, u64(off), k, 0, 3, u64(soff), None)),       # min_length 0
                (INVALID, lambda: L.fbg_pindex_seeds(h, d8, None, k, 1, 3, u64(soff), None)),           # no pat_off
                (INVALID, lambda: L.fbg_pindex_seeds(h, None, u64(off), k, 1, 3, u64(soff), None)),     # no pattern bytes
                (INVALID, lambda: L.fbg_pindex_seeds(h, d8, u64(bad_off), k, 1, 3, u64(soff), None)),
                (TOO_LARGE, lambda: L.fbg_pindex_seeds(h, d8, u64(huge), 1, 1, 3, u64(soff), None)),
                (TOO_LARGE, lambda: L.fbg_pindex_seeds(h, d8, u64(off), 0xffffffff, 1, 3, u64(soff), None))):
            assert call() == rc
            # ... leaves nothing to fetch, and the next call on the same index succeeds
            assert L.fbg_pindex_seeds_fetch(h, *([None] * 9)) == INVALID
            assert L.fbg_pindex_seeds_places(h, None, None, None, None, None, None, None) == INVALID
            good()
        # a minimum length that no pattern can have (2^32 and above: it must not wrap or be clamped to a reachable one)
        for far in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
            soff[:] = 7
            assert L.fbg_pindex_seeds(h, d8, u64(off), k, far, 3, u64(soff), ctypes.byref(ms)) == 0 and not soff.any()
            eo = np.full(1, 9, dtype=np.uint64)
            assert L.fbg_pindex_seeds_fetch(h, None, None, None, None, None, None, u64(eo), None, None) == 0 and eo[0] == 0
            assert L.fbg_pindex_seeds_places(h, *[u32(a) for a in six], None) == 0
        good()
        # no patterns at all
        assert L.fbg_pindex_seeds(h, None, None, 0, 1, 3, u64(soff), None) == 0 and soff[0] == 0
        eo = np.full(1, 9, dtype=np.uint64)
        assert L.fbg_pindex_seeds_fetch(h, None, None, None, None, None, None, u64(eo), None, None) == 0 and eo[0] == 0
        assert L.fbg_pindex_seeds_places(h, *[u32(a) for a in six], None) == 0
        good()
        # the per-seed arrays: all of them, and any subset
        q, ln, rs = (np.zeros(ns, dtype=np.uint32) for _ in range(3))
        cnt, et, st = (np.zeros(ns, dtype=np.uint64) for _ in range(3))
        eoff, stoff = np.zeros(ns + 1, dtype=np.uint64), np.zeros(ns + 1, dtype=np.uint64)
        assert L.fbg_pindex_seeds_fetch(h, u32(q), u32(ln), u64(cnt), u32(rs), u64(et), u64(st), u64(eoff), u64(stoff),
                                        ctypes.byref(ms)) == 0
        for got, f in ((q, "q_start"), (ln, "length"), (cnt, "count"), (rs, "restarts"), (et, "end_total"), (st, "start_total"),
                       (eoff, "end_off"), (stoff, "start_off")):
            assert got.tolist() == list(want[f]), f
        q[:] = 77
        cnt[:] = 0
        assert L.fbg_pindex_seeds_fetch(h, None, None, u64(cnt), None, None, None, None, None, None) == 0
        assert cnt.tolist() == want["count"] and (q == 77).all()
        ne, nst = int(eoff[ns]), int(stoff[ns])
        assert ne > 0 and nst > 0 and ne <= 64 and nst <= 64
        # one array of a list missing
        assert L.fbg_pindex_seeds_places(h, u32(six[0]), None, u32(six[2]), None, None, None, None) == INVALID
        # only the ends, only the starts, both, and both again; searches of the other kinds in between
        for a in six:
            a[:] = 0xdeadbeef
        assert L.fbg_pindex_seeds_places(h, u32(six[0]), u32(six[1]), u32(six[2]), None, None, None, ctypes.byref(ms)) == 0
        assert [a[:ne].tolist() for a in six[:3]] == [want["end_" + f].tolist() for f in ("src", "dst", "offset")]
        assert all((a == 0xdeadbeef).all() for a in six[3:]) and all((a[ne:] == 0xdeadbeef).all() for a in six[:3])
        pix.locate(["ACGT" * 20, "T"])
        pix.occurrences(["AG", "T"], max_per_pattern=5)
        for a in six:
            a[:] = 0xdeadbeef
        assert L.fbg_pindex_seeds_places(h, None, None, None, u32(six[3]), u32(six[4]), u32(six[5]), None) == 0
        assert [a[:nst].tolist() for a in six[3:]] == [want["start_" + f].tolist() for f in ("src", "dst", "offset")]
        assert all((a == 0xdeadbeef).all() for a in six[:3]) and all((a[nst:] == 0xdeadbeef).all() for a in six[3:])
        for _ in range(2):
            assert L.fbg_pindex_seeds_places(h, *[u32(a) for a in six], None) == 0
            assert [a[:ne].tolist() for a in six[:3]] == [want["end_" + f].tolist() for f in ("src", "dst", "offset")]
            assert [a[:nst].tolist() for a in six[3:]] == [want["start_" + f].tolist() for f in ("src", "dst", "offset")]
        assert L.fbg_pindex_seeds_places(h, None, None, None, None, None, None, None) == 0


def tool_lines(model, ids, data, L, cap):
    """What fbg_locate --seeds=L [--occurrences=cap] prints for stdin `data` (cap None: no --occurrences)."""
    out, seeded = [], 0
    toks = M.tokens(data)
    for t in toks:
        ss = SM.seeds(model, t, L, cap or 0)
        out.append(b"Pattern? %d seeds found.\n" % len(ss))
        seeded += len(ss) != 0
        for s in ss:
            o = s.occ
            out.append(b"S\t%d\t%d\t%d\t%d\n" % (s.q_start, s.length, o.count, o.restarts))
            if cap is None:
                continue
            for tag, places, total in ((b"E", o.ends, o.end_total), (b"B", o.starts, o.start_total)):
                out += [b"%s\t%d\t%d\t%d\n" % (tag, ids[a], ids[b], off) for a, b, off in TO.rows(places)]
                if total > len(places):
                    out.append(b"%s\t...\t%d more\n" % (tag, total - len(places)))
    out.append(b"Pattern? %d out of %d patterns seeded\n" % (seeded, len(toks)))
    return b"".join(out)


@pytest.mark.gpu
def test_tool_prints_the_seeds():
    model = OM.Index(*M.read_xgfa(SPEC))
    ids = list(range(1, 10))                                      # the S ids of the file, ascending
    data = b"AGCGACTAGATAC AGCAGTT CGACTAX T XX GACTAGTTTCA AGXTTAC\n"
    p = TL.run_locate(["--graph=" + SPEC, "--seeds=3", "--occurrences=2"], data)
    assert p.returncode == 0, p.stderr
    assert p.stdout == tool_lines(model, ids, data, 3, 2)
    assert b"Pattern? 1 seeds found.\nS\t0\t13\t1\t2\nE\t4\t7\t7\nB\t1\t2\t0\n" in p.stdout
    assert b"Pattern? 0 seeds found.\n" in p.stdout and p.stdout.endswith(b" out of 7 patterns seeded\n")
    p = TL.run_locate(["--graph=" + SPEC, "--seeds"], data)
    assert p.returncode == 0 and p.stdout == tool_lines(model, ids, data, 1, None)
    assert b"E\t" not in p.stdout and b"S\t0\t1\t15\t0\n" in p.stdout
    p = TL.run_locate(["--graph=" + SPEC, "--seeds", "--occurrences"], data)
    assert p.returncode == 0 and p.stdout == tool_lines(model, ids, data, 1, 64)
    p = TL.run_locate(["--graph=" + SPEC, "--seeds=2", "--error-on-not-found"], data)
    want = tool_lines(model, ids, data, 2, None)
    stop = want.index(b"Pattern? 0 seeds found.\n") + len(b"Pattern? 0 seeds found.\n")
    assert p.returncode == 1 and p.stdout == want[:stop]
    # without --seeds: what test_occurrences.test_tool_prints_the_places and test_locate expect, unchanged
    p = TL.run_locate(["--graph=" + SPEC, "--occurrences=2"], data)
    assert p.returncode == 0 and p.stdout == TO.tool_lines(model, ids, data, 2)
    p = TL.run_locate(["--graph=" + SPEC], data)
    assert p.stdout == M.expected_stdout(model, data)[0]
