"""Paired reads, a seedless mate rescued by alignment in the insert window: fbg_pindex_pairs_align,
PatternIndex.chains(pairs=, pair_align=True) and fbg_locate --pair-align (include/fbg_hip.h, csrc/pindex_pairs_align.hip).

The checker is tests/pair_align_model.py: the definitions of the header on top of rows_model (G_r, p(r, block), the rows
that carry a chain), align_model.align and pairs_model.partner.  On the CPU the model is compared with align_model.brute
(the definition by lev) and the inputs are checked to be what they claim with the host models of test_rows: a damaged
mate has no seed of min_length on either strand.  On the GPU the model takes the places and the chains from the engine,
and every array and every counter is compared exactly.

Pairs are interleaved: the given reads 2p and 2p + 1, cut from the two ends of a fragment of one row, the second mate
reverse-complemented, one of the two with a substitution every few symbols; in half of the pairs the mates change places."""
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import align_model as AM  # noqa: E402
import chain_model as CM  # noqa: E402
import heuristic_model as HM  # noqa: E402
import msa_model as MM  # noqa: E402
import occ_model as OM  # noqa: E402
import pair_align_model as PA  # noqa: E402
import pairs_model as PM  # noqa: E402
import rows_model as RM  # noqa: E402
import seeds_model as SDM  # noqa: E402
import strand_model as STM  # noqa: E402
import test_chains as TC  # noqa: E402
import test_rows as TR  # noqa: E402
from conftest import random_msa  # noqa: E402
from fasta_util import read_fasta  # noqa: E402

NONE = PA.NONE
U64 = 0xffffffffffffffff
GAP = ord("-")
LOCATE = TC.LOCATE
CALL = "fbg_pindex_pairs_align"
INSERTS = ((0, 0), (0, 60), (30, 120), (0, U64))
EDITS = (0, 3, 0xffffffff)
READ_FIELDS = (("mate_row", "row"), ("mate_edits", "edits"), ("mate_start", "t_start"), ("mate_end", "t_end"), ("mate_insert", "insert"))
PAIR_FIELDS = (("mate_which", "which"), ("mate_score", "pair_score"), ("mate_lo", "t_lo"), ("mate_hi", "t_hi"))
SEEN = ("aligned", "pairs", "rejected_edits", "rejected_insert", "empty")      # what the parity tests must have met


def rc(s):
    return STM.revcomp(s, TR.TABLE)


def virtual(reads):
    return list(reads) + [rc(r) for r in reads]


def fixed_cuts(n, step=25):
    return list(range(step - 1, n - 1, step)) + [n]


def fast_align(P, W):
    """align_model.align with the DP a row at a time for every window (the CPU test compares the two)."""
    P, W = bytes(P), bytes(W)
    edits, e = AM.smallest_min(AM.last_row_by_rows(P, W, lambda j: 0))
    back, j = AM.smallest_min(AM.last_row_by_rows(P[::-1], W[:e][::-1], lambda j: j))
    assert back == edits
    return edits, e - j, e


def cached(align):
    memo = {}

    def call(P, W):
        key = (bytes(P), bytes(W))
        if key not in memo:
            memo[key] = align(*key)
        return memo[key]
    return call


# ---- the inputs ---------------------------------------------------------------------------------------------------

class Host:
    """The host models of one MSA and segmentation: the index of the graph, rows_model and msa_model."""

    def __init__(self, A, b):
        self.A, self.b = A, [int(x) for x in b]
        labels, edges, _ = HM.segmentation_graph(A, self.b)
        self.index, self.mm, self.rm = OM.Index(labels, edges), MM.Model(A, self.b), RM.Model(A, self.b)

    def n_seeds(self, read, L):
        """Seeds of min_length L of a read, on both strands."""
        return sum(len(SDM.seeds(self.index, P, L, 16)) for P in (bytes(read), rc(read)) if P)

    def run(self, reads, L, cap=16, band=None, min_score=0):
        """What the engine is to return for stranded seeds and chains of `reads` (as test_rows.cpu)."""
        vreads = virtual([bytes(r) for r in reads])
        seed_off, q, k, start_off, places = [0], [], [], [0], []
        for P in vreads:
            for s in SDM.seeds(self.index, P, L, cap):
                q.append(s.q_start)
                k.append(s.length)
                places += s.occ.starts.tolist()
                start_off.append(len(places))
            seed_off.append(len(q))
        pl = np.array(places, dtype=np.int64).reshape(-1, 3)
        o = SimpleNamespace(vreads=vreads, seed_off=np.array(seed_off, dtype=np.uint64), start_off=np.array(start_off, dtype=np.uint64),
                            q_start=np.array(q, dtype=np.uint32), length=np.array(k, dtype=np.uint32))
        o.start_src, o.start_dst, o.start_offset = (pl[:, c].astype(np.uint32) for c in range(3))
        o.start_col = self.mm.coords(pl[:, 0], pl[:, 1], pl[:, 2])[1].astype(np.uint32)
        o.chain_off, o.score, o.anchor_place, o.anchor_seed = CM.chains(o.seed_off, o.q_start, o.length, o.start_off, o.start_col, band,
                                                                       min_score)
        sets = RM.seed_rows(self.rm, vreads, o.seed_off, o.q_start, o.length, o.start_off, o.start_src, o.start_dst, o.start_offset)[2]
        o.chain_sets = RM.chain_rows(self.rm.m, sets, o.chain_off, o.anchor_place)[3]
        return o

    def solve(self, o, ins, max_edits=NONE, max_window=0, select=None, align=AM.align):
        return PA.solve(self.rm, o.vreads, o.chain_off, o.score, o.anchor_place, o.anchor_seed, o.chain_sets, o.q_start, o.start_src,
                        o.start_dst, o.start_offset, ins[0], ins[1], max_edits, max_window, select, align=align)


def damage(rng, host, read, every, L):
    """`read` with a substitution at every `every`-th symbol from `every` // 3 on, the letters drawn again until the host
    models find no seed of L symbols on either strand (every - 1 < L: no stretch of the read survives that long); None
    where twenty draws all left a seed somewhere in the graph."""
    assert every - 1 < L
    for _ in range(20):
        out = bytearray(read)
        for at in range(every // 3, len(out), every):
            out[at] = rng.choice([c for c in b"ACGT" if c != out[at]])
        if host.n_seeds(out, L) == 0:
            return bytes(out)
    return None


def damaged_pairs(rng, host, count, L, lengths, every, frag_max=120):
    """-> (reads, damaged): `count` pairs of mates of lengths[0] .. lengths[1] symbols from the two ends of a fragment of up to
    frag_max columns of one row, gaps stripped; the second mate reverse-complemented; pair p has mate p % 2 damaged, and
    its mates change places where p % 4 >= 2, so every candidate 0 .. 3 has pairs.  damaged: the given reads that were."""
    A = host.A
    reads, bad = [], []
    while len(reads) < 2 * count:
        p = len(reads) // 2
        l1, l2 = (int(rng.integers(lengths[0], lengths[1] + 1)) for _ in range(2))
        f, r = int(rng.integers(max(l1, l2), frag_max + 1)), int(rng.integers(0, len(A)))
        if p % 8 < 2:       # a short fragment of short mates: an insert below a min_insert of 30
            l1, l2 = min(l1, lengths[0] + 8), min(l2, lengths[0] + 8)
            f = max(l1, l2) + 2
        a = int(rng.integers(0, A.shape[1] - f + 1))
        s = A[r, a:a + f]
        s = s[s != GAP].tobytes()
        if len(s) < max(l1, l2):
            continue
        mates = [s[:l1], s[len(s) - l2:]]
        if host.n_seeds(mates[1 - p % 2], L) == 0:      # the other mate is to chain
            continue
        mates[p % 2] = damage(rng, host, mates[p % 2], every, L)
        if mates[p % 2] is None:
            continue
        mates[1] = rc(mates[1])
        if p % 4 >= 2:
            mates = mates[::-1]
        bad.append(2 * p + (p % 2 if p % 4 < 2 else 1 - p % 2))
        reads += mates
    return reads, bad


def spliced(A, b, r1, r2, j, k):
    """k symbols of row r1 up to the end of block j, then k of row r2: a read of the graph that no row spells where the rows differ."""
    c = b[j] + 1
    left, right = A[r1, :c], A[r2, c:]
    return left[left != GAP].tobytes()[-k:] + right[right != GAP].tobytes()[:k]


def extra_pairs(host, x):
    """Beside the damaged pairs: an empty mate, two identical mates, a mate from another row's far end, a spliced mate."""
    A, b = host.A, host.b
    far = A[len(A) - 1, -20:]
    sp = spliced(A, b, 0, len(A) - 1, len(b) // 2, 12)
    return [b"", rc(x), x, b"", x, x, x, rc(far[far != GAP].tobytes()), sp, rc(x), rc(x), sp]


@functools.lru_cache(maxsize=None)
def random_input(gaps):
    rng = np.random.default_rng(70 + gaps)
    A = random_msa(rng, 8, 300, gap_p=0.02, gap_run=3, similar=0.9) if gaps else random_msa(rng, 8, 300, similar=0.9)
    host = Host(A, fixed_cuts(300))
    reads, bad = damaged_pairs(rng, host, 24, 8, (12, 40), 6)
    x = A[1, 100:130]
    return host, reads + extra_pairs(host, x[x != GAP].tobytes()), bad


@functools.lru_cache(maxsize=None)
def golden_input(path):
    A = read_fasta(path)[0]
    rng = np.random.default_rng(len(A[0]))
    host = Host(A, fixed_cuts(A.shape[1], 4))
    reads, bad = damaged_pairs(rng, host, 8, 4, (4, 7), 3, frag_max=A.shape[1])
    x = A[0][A[0] != GAP].tobytes()[:6]
    return host, reads + extra_pairs(host, x), bad


@functools.lru_cache(maxsize=None)
def tier_input():
    """One row of 700 symbols and a near copy.  Pairs whose forward mate (40 symbols, exact) starts in the first 60 symbols,
    so that with max_insert 600 every window is 600 symbols; the reverse mate has 64, 65, 256 or 257 symbols and a
    substitution every 6.  Then one pair whose second mate has 1025 symbols."""
    rng = np.random.default_rng(77)
    A = random_msa(rng, 2, 700, similar=0.97)
    host = Host(A, fixed_cuts(700))
    row = A[0].tobytes()
    reads, bad = [], []
    for i, k in enumerate((64, 65, 256, 257)):
        a = 7 + 13 * i
        end = 600 - 11 * i
        reads += [row[a:a + 40], rc(damage(rng, host, row[end - k:end], 6, 16))]
        bad.append(2 * i + 1)
    long = bytes(rng.choice(list(b"ACGT"), 1025).astype(np.uint8))
    assert host.n_seeds(long, 16) == 0
    reads += [row[20:60], long]
    return host, reads, bad + [9]


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_call_and_the_header_declares_it():
    from founderblockgraphs_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fbg_hip.h")).read()
    assert hasattr(L, CALL) and f"int {CALL}(" in header and CALL in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[CALL][1]) == 17
    for words in ("W = G_r[fs(v) : min(|G_r|, fs(v) + max_insert))", "W = G_r[max(0, fe(v) - max_insert) : fe(v))",
                  "fs(v) = max(0, x_1 - q_1) and fe(v) = min(|G_r|, x_last + L_v - q_last)",
                  "partner without a carrying row; empty, L_w == 0", "too long, L_w > max_read (1024); too wide, max_window != 0 and |W| > max_window",
                  "insert[w] = t_end[w] - fs(v) for v < n and fe(v) - t_start[w] for v >= n",
                  "edits[w] <= max_edits and insert[w] >= min_insert", "0: F = chain(a), R = aligned(b + n)",
                  "1: F = aligned(a), R = chain(b + n)", "2: F = chain(b), R = aligned(a + n)", "3: F = aligned(b), R = chain(a + n)",
                  "score[v] + L_w - edits[w]", "the smallest number among equals", "in symbols of row r"):
        assert words in header, words
    # the sentences that test_pairs pins stay, and point here
    for words in ("not rescued by alignment", "counted in MSA witness columns", "No mapping quality of the pair", "fbg_pindex_pairs_align, below"):
        assert words in header, words


def small_case(rng, trial):
    gaps = trial % 3 == 2
    A = random_msa(rng, 4, 70, gap_p=0.03, gap_run=2, similar=0.85) if gaps else random_msa(rng, 4, 70, similar=0.85)
    host = Host(A, fixed_cuts(70, 10))
    reads, bad = damaged_pairs(rng, host, 6, 7, (9, 16), 5, frag_max=45)
    x = A[1, 20:32]
    return host, reads + extra_pairs(host, x[x != GAP].tobytes()), bad


def test_model_agrees_with_brute_force():
    rng = np.random.default_rng(31)
    seen = dict(clamp0=0, clamp_end=0, short_window=0, empty_window=0, empty_read=0, no_row=0, only_edits=0, only_insert=0, which0=0,
                which1=0, which2=0, which3=0, tie=0, none=0, select_differs=0, cases=0)
    inserts = ((0, 0), (0, 5), (0, 30), (12, 45), (20, 60), (0, U64))
    for trial in range(40):
        host, reads, bad = small_case(rng, trial)
        o = host.run(reads, 7)
        V, n = len(o.vreads), len(reads)
        for v in bad:       # the inputs are what they claim: no seed of min_length on either strand, so no chain
            assert o.seed_off[v + 1] == o.seed_off[v] and o.seed_off[v + n + 1] == o.seed_off[v + n]
            assert o.chain_off[v + 1] == o.chain_off[v] and o.chain_off[v + n + 1] == o.chain_off[v + n]
        ins = inserts[trial % len(inserts)]
        max_edits = (NONE, 2, 0, 4)[trial % 4]
        select = (None, np.ones(V, dtype=np.uint8), (rng.random(V) < 0.5).astype(np.uint8))[trial % 3]
        m = host.solve(o, ins, max_edits, 0, select)
        want = host.solve(o, ins, max_edits, 0, select, align=AM.brute)
        fast = host.solve(o, ins, max_edits, 0, select, align=fast_align)
        for f in ("row", "edits", "t_start", "t_end", "insert", "which", "pair_score", "t_lo", "t_hi"):
            assert np.array_equal(getattr(m, f), getattr(want, f)) and np.array_equal(getattr(m, f), getattr(fast, f)), (trial, f)
        assert m.stats == want.stats == fast.stats
        default = host.solve(o, ins, max_edits, 0, None)
        seen["select_differs"] += select is not None and [s is None for s in default.status] != [s is None for s in m.status]
        # the statements of the header, once more, from the model's own intermediate values
        for w in range(V):
            v = PM.partner(w, n)
            if m.status[w] is None:
                assert all(int(getattr(m, f)[w]) == NONE for f in ("row", "edits", "t_start", "t_end", "insert"))
                continue
            seen["cases"] += 1
            seen["no_row"] += m.status[w] == "no_row"
            if m.status[w] == "no_row":
                assert o.chain_off[v + 1] > o.chain_off[v] and not o.chain_sets[v] and m.row[w] == NONE
                continue
            r, fs, fe = m.frag[v]
            glen, (w0, w1), Lw = len(host.rm.G[r]), m.windows[w], len(o.vreads[w])
            assert m.row[w] == r == o.chain_sets[v][0] and 0 <= fs < fe <= glen and 0 <= w0 <= w1 <= glen and w1 - w0 <= ins[1]
            assert (w0 == fs) if v < n else (w1 == fe)
            seen["clamp0"] += v >= n and fe - min(ins[1], PA.CLAMP) < 0
            seen["clamp_end"] += v < n and fs + min(ins[1], PA.CLAMP) > glen
            seen["empty_window"] += w1 == w0
            seen["empty_read"] += Lw == 0
            assert (m.status[w] == "empty") == (Lw == 0 or w1 == w0)
            if m.status[w] != "aligned":
                assert int(m.edits[w]) == NONE and int(m.insert[w]) == NONE
                continue
            seen["short_window"] += w1 - w0 < Lw
            e, ts, te = int(m.edits[w]), int(m.t_start[w]), int(m.t_end[w])
            assert w0 <= ts <= te <= w1 and AM.lev(o.vreads[w], host.rm.G[r][ts:te]) == e
            insert = te - fs if v < n else fe - ts
            ok_e, ok_i = e <= max_edits, insert >= ins[0]
            assert int(m.insert[w]) == (insert if ok_e and ok_i else NONE)
            seen["only_edits"] += not ok_e and ok_i
            seen["only_insert"] += ok_e and not ok_i
        for p in range(n // 2):
            scores = []
            for i, (v, w) in enumerate(PA.candidates(p, n)):
                if int(m.insert[w]) != NONE:
                    scores.append((int(o.score[v]) + len(o.vreads[w]) - int(m.edits[w]), -i))
            if not scores:
                assert int(m.which[p]) == PA.NO_PAIR and (int(m.pair_score[p]), int(m.t_lo[p]), int(m.t_hi[p])) == (0, NONE, NONE)
                seen["none"] += 1
                continue
            top = max(scores)
            assert (int(m.pair_score[p]), int(m.which[p])) == (top[0], -top[1])
            seen["which%d" % -top[1]] += 1
            seen["tie"] += sum(1 for s in scores if s[0] == top[0]) > 1
        assert m.stats["pairs"] == int((m.which != PA.NO_PAIR).sum())
    assert all(v > 0 for v in seen.values()) and seen["cases"] >= 300, seen


@pytest.mark.parametrize("which", ["random", "gaps", "tier"] + [os.path.basename(p) for p in TC.GOLDEN])
def test_gpu_inputs_are_what_they_claim(which):
    L = 8
    if which in ("random", "gaps"):
        host, reads, bad = random_input(which == "gaps")
    elif which == "tier":
        (host, reads, bad), L = tier_input(), 16
    else:
        (host, reads, bad), L = golden_input([p for p in TC.GOLDEN if os.path.basename(p) == which][0]), 4
    assert len(reads) % 2 == 0 and bad
    o = host.run(reads, L)
    n = len(reads)
    for v in bad:
        assert o.seed_off[v + 1] == o.seed_off[v] and o.seed_off[v + n + 1] == o.seed_off[v + n], v
        mate = v ^ 1
        assert o.chain_off[mate + 1] > o.chain_off[mate] or o.chain_off[mate + n + 1] > o.chain_off[mate + n], v
    m = host.solve(o, (0, 600 if which == "tier" else 120), align=fast_align)
    assert m.stats["aligned"] >= len(bad) - (which == "tier") and m.stats["pairs"] > 0
    if which == "tier":
        assert m.stats["too_long"] == 1 and [len(reads[v]) for v in bad] == [64, 65, 256, 257, 1025]
        assert all(m.windows[v][1] - m.windows[v][0] == 600 for v in range(2 * n) if m.status[v] == "aligned")
        assert m.which.tolist() == [0, 0, 0, 0, 0xff]
    else:
        assert m.stats["empty"] > 0 and len(set(m.which.tolist()) & {0, 1, 2, 3}) == 4
        # what the GPU test counts over its parameters is there to be counted
        seen = dict.fromkeys(SEEN, 0)
        for ins in INSERTS:
            for max_edits in EDITS:
                st = host.solve(o, ins, max_edits, align=fast_align).stats
                for f in SEEN:
                    seen[f] += st[f]
        assert all(v > 0 for v in seen.values()), seen


def test_tool_pair_align_needs_its_prerequisites():
    assert os.path.exists(LOCATE), "fbg_locate is built by make -C founderblockgraphs_amd/csrc"
    p = subprocess.run([LOCATE, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--pair-align" in p.stderr
    base = ["--graph=" + TC.SPEC, "--msa=" + TC.GOLDEN[0], "--seeds", "--occurrences", "--chain", "--strands"]
    for args in (base + ["--rows", "--pair-align"], base + ["--pairs=0,9", "--pair-align=2"], base + ["--rows", "--pairs=0,9", "--pair-align=x"],
                 base + ["--rows", "--pairs=0,9", "--pair-align=4294967296"]):
        p = subprocess.run([LOCATE] + args, input=b"AG\nCT\n", capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"--pair-align" in p.stderr and b"usage:" in p.stderr, args


# ---- GPU ----------------------------------------------------------------------------------------------------------

def model_of(host, sd, ch, vreads, ins, max_edits=NONE, max_window=0, select=None, align=fast_align, cache=None):
    """The model on the engine's own places and on the chains `ch` holds."""
    o = sd.occ
    if cache is None or "sets" not in cache:
        sets = RM.seed_rows(host.rm, vreads, sd.seed_off, sd.q_start, sd.length, o.start_off, o.start_src, o.start_dst, o.start_offset)[2]
        if cache is not None:
            cache["sets"] = sets
    else:
        sets = cache["sets"]
    chain_sets = RM.chain_rows(host.rm.m, sets, ch.chain_off, ch.anchor_place)[3]
    return PA.solve(host.rm, vreads, ch.chain_off, ch.score, ch.anchor_place, ch.anchor_seed, chain_sets, sd.q_start, o.start_src,
                    o.start_dst, o.start_offset, ins[0], ins[1], max_edits, max_window, select, align=align)


def same(ch, m, what):
    for f, g in READ_FIELDS + PAIR_FIELDS:
        got, want = getattr(ch, f), getattr(m, g)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f, got.tolist(), want.tolist())
    assert ch.mate_stats == m.stats, (what, ch.mate_stats, m.stats)


def c_call(pix, V, ins, max_edits=NONE, max_window=0, select=None, null=()):
    """The C ABI -> rc, the nine arrays in the order of the signature, stats.  null: names of outputs passed as NULL."""
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    P = V // 4
    u32, u64 = (lambda a: a.ctypes.data_as(_lib.u32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    per_read = [np.full(V + 1, 7, dtype=np.uint32) for _ in range(5)]
    which = np.full(P + 1, 7, dtype=np.uint8)
    per_pair = [np.full(P + 1, 7, dtype=np.uint32) for _ in range(3)]
    stats = np.full(11, 7, dtype=np.uint64)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
    names = [g for _, g in READ_FIELDS + PAIR_FIELDS]
    args = [u32(a) for a in per_read] + [which.ctypes.data_as(_lib.u8p)] + [u32(a) for a in per_pair]
    args = [None if f in null else a for f, a in zip(names, args)]
    code = L.fbg_pindex_pairs_align(pix._h, ins[0], ins[1], max_edits, max_window, None if sel is None else sel.ctypes.data_as(_lib.u8p),
                                    *args, None if "stats" in null else u64(stats), None)
    if code == 0:      # nothing past the entries of each array
        assert all(a[V] == 7 for a in per_read) and which[P] == 7 and all(a[P] == 7 for a in per_pair) and stats[10] == 7
    return code, [a[:V] for a in per_read] + [which[:P]] + [a[:P] for a in per_pair], stats[:10]


def same_c(got, m, what):
    code, out, stats = got
    assert code == 0, what
    for a, (_, g) in zip(out, READ_FIELDS + PAIR_FIELDS):
        assert np.array_equal(a, getattr(m, g)), (what, g, a.tolist(), getattr(m, g).tolist())
    assert dict(zip(PA.STATS, stats.tolist())) == m.stats, (what, stats.tolist(), m.stats)


def engine_error(engine):
    from founderblockgraphs_amd import _lib
    return _lib.lib().fbg_last_error(engine._h).decode()


MODES = {"plain": dict(), "by_row": dict(by_row=True), "adopt": dict(adopt_pairs=True)}


def run_through_both(engine, host, reads, L, what):
    """Every insert and max_edits, after plain chains, after by_row and after adopt, through the C call and through Python."""
    vreads = virtual(reads)
    V = len(vreads)
    seen = dict.fromkeys(SEEN, 0)
    align = cached(fast_align)
    with TR.build(engine, host.A, host.b) as pix:
        sd = pix.seeds(reads, min_length=L, max_per_seed=16, msa=True, strands=True)
        cache = {}
        for mode, kw in MODES.items():
            for ins in INSERTS:
                for k, max_edits in enumerate(EDITS):
                    select = None if k != 1 else np.ones(V, dtype=np.uint8)
                    ch = pix.chains(pairs=ins, pair_align=True, pair_max_edits=max_edits, pair_select=select, **kw)
                    m = model_of(host, sd, ch, vreads, ins, max_edits, 0, select, align, cache)
                    same(ch, m, (what, mode, ins, max_edits, "python"))
                    same_c(c_call(pix, V, ins, max_edits, 0, select), m, (what, mode, ins, max_edits, "c"))
                    assert ch.mate_ms > 0 or m.stats["selected"] == 0 or ch.chain_off[V] == 0
                    if ins == (0, 0):
                        assert m.stats["aligned"] == 0 and (ch.mate_which == PA.NO_PAIR).all()
                    for f in seen:
                        seen[f] += m.stats[f]
            assert pix.chains(pairs=INSERTS[1], **kw).mate_row is None
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [False, True])
def test_model_parity_on_random_msas(engine, gaps):
    host, reads, _ = random_input(gaps)
    run_through_both(engine, host, reads, 8, ("random", gaps))


@pytest.mark.gpu
@pytest.mark.parametrize("path", TC.GOLDEN, ids=os.path.basename)
def test_model_parity_on_the_golden_files(engine, path):
    host, reads, _ = golden_input(path)
    run_through_both(engine, host, reads, 4, os.path.basename(path))


@pytest.mark.gpu
def test_word_and_tier_boundaries(engine):
    host, reads, bad = tier_input()
    vreads = virtual(reads)
    V, n = len(vreads), len(reads)
    align = cached(fast_align)
    with TR.build(engine, host.A, host.b) as pix:
        sd = pix.seeds(reads, min_length=16, max_per_seed=16, msa=True, strands=True)
        cache = {}
        for max_window, aligned in ((0, 4), (600, 4), (599, 0)):
            ch = pix.chains(pairs=(0, 600), pair_align=True, pair_max_window=max_window)
            m = model_of(host, sd, ch, vreads, (0, 600), NONE, max_window, None, align, cache)
            same(ch, m, ("tiers", max_window))
            same_c(c_call(pix, V, (0, 600), NONE, max_window), m, ("tiers", max_window, "c"))
            assert m.stats["aligned"] == aligned and m.stats["too_wide"] == 4 - aligned and m.stats["too_long"] == 1
            assert ch.mate_edits[n + 9] == NONE and ch.mate_row[n + 9] == 0          # the read of 1025 symbols keeps its row
            if aligned:
                for i, k in enumerate((64, 65, 256, 257)):
                    w = 2 * i + 1 + n      # the damaged mate was given reverse-complemented: its reverse strand is aligned
                    # no more edits than substitutions were made, and a stretch at most that many symbols off k
                    subs, span = len(range(2, k, 6)), int(ch.mate_end[w]) - int(ch.mate_start[w])
                    assert len(vreads[w]) == k and 0 < ch.mate_edits[w] <= subs and abs(span - k) <= int(ch.mate_edits[w])
                assert ch.mate_which.tolist() == [0, 0, 0, 0, 0xff]


@pytest.mark.gpu
def test_state_rules(engine):
    from founderblockgraphs_amd import _lib
    L = _lib.lib()
    host, reads, _ = random_input(False)
    vreads = virtual(reads)
    V = len(vreads)
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)      # noqa: E731
    ins = (30, 120)
    with TR.build(engine, host.A, host.b) as pix:
        sd = pix.seeds(reads, min_length=8, max_per_seed=16, msa=True, strands=True)
        ch0 = pix.chains(band=8)
        assert pix.align_stats()["table_bytes"] == 0
        m = model_of(host, sd, ch0, vreads, ins)
        # before any fbg_pindex_chains_align: the call builds the prefix table itself; and twice the same
        first = c_call(pix, V, ins)
        same_c(first, m, "before align")
        assert pix.align_stats()["table_bytes"] > 0
        same_c(c_call(pix, V, ins), m, "twice")
        # the other stages, fetched before and after, are equal and stay current without being rerun
        ch = pix.chains(band=8, align=True, cigar=True, mapq=True, pairs=ins)
        before = [getattr(ch, f).copy() for f in ("align_row", "edits", "t_start", "t_end", "cigar_off", "cigar_ops", "mapq", "second_score",
                                                  "pair_which", "pair_score", "rescue_off", "rescue_score")]
        astats, cstats, mstats = pix.align_stats(), pix.cigar_stats(), pix.mapq_stats()
        same_c(c_call(pix, V, ins, 3, 0, np.ones(V, dtype=np.uint8)), model_of(host, sd, ch0, vreads, ins, 3, 0, np.ones(V, dtype=np.uint8)),
               "after align")
        coff, ops = np.zeros(V + 1, dtype=np.uint64), np.zeros(len(ch.cigar_ops) + 1, dtype=np.uint32)
        assert L.fbg_pindex_chains_cigar_fetch(pix._h, coff.ctypes.data_as(_lib.u64p), u32(ops)) == 0
        assert np.array_equal(coff, ch.cigar_off) and np.array_equal(ops[:-1], ch.cigar_ops)
        place, seed = (np.zeros(len(sd.q_start) + 1, dtype=np.uint32) for _ in range(2))
        assert L.fbg_pindex_chains_mapq_fetch(pix._h, u32(place), u32(seed), None) == 0
        smq = np.zeros(V, dtype=np.uint8)
        assert L.fbg_pindex_mapq_strands(pix._h, smq.ctypes.data_as(_lib.u8p), None) == 0 and np.array_equal(smq, ch.mapq_stranded)
        total = ctypes.c_uint64(0)
        assert L.fbg_pindex_chains_cigar(pix._h, None, ctypes.byref(total), None) == 0 and total.value == len(ch.cigar_ops)
        assert (pix.align_stats(), pix.cigar_stats(), pix.mapq_stats()) == (astats, cstats, mstats)
        again = pix.chains(band=8, align=True, cigar=True, mapq=True, pairs=ins, pair_align=True)
        after = [getattr(again, f) for f in ("align_row", "edits", "t_start", "t_end", "cigar_off", "cigar_ops", "mapq", "second_score",
                                             "pair_which", "pair_score", "rescue_off", "rescue_score")]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        same(again, m, "beside the other stages")
        # after a new seeds call the chains are stale
        pix.seeds(reads, min_length=8, max_per_seed=16, msa=True, strands=True)
        code = c_call(pix, V, ins)[0]
        assert code == _lib.FBG_ERR_INVALID and CALL in engine_error(engine) and "no current fbg_pindex_chains result" in engine_error(engine)
        pix.chains(band=8)
        same_c(c_call(pix, V, ins), m, "after chains again")


@pytest.mark.gpu
def test_errors_leave_the_index_working(engine):
    from founderblockgraphs_amd import _lib
    from founderblockgraphs_amd.api import FbgError
    INVALID = _lib.FBG_ERR_INVALID
    host, reads, _ = random_input(False)
    vreads = virtual(reads)
    V = len(vreads)

    def fails(pix, V, ins=(0, 100), **kw):
        code = c_call(pix, V, ins, **kw)[0]
        msg = engine_error(engine)
        assert code == INVALID and CALL in msg, (code, msg)
        return msg

    assert _lib.lib().fbg_pindex_pairs_align(None, 0, 0, 0, 0, *[None] * 12) == INVALID
    with TR.build(engine, host.A, host.b, rows=False) as pix:                     # an index built without rows
        pix.seeds(reads, min_length=8, max_per_seed=16, msa=True, strands=True)
        pix.chains()
        assert "fbg_pindex_build_segmentation_rows" in fails(pix, V)
        with pytest.raises(ValueError):
            pix.chains(pairs=(0, 100), pair_align=True)
    with TR.build(engine, host.A, host.b) as pix:
        fails(pix, 0)                                                             # before any seeds call
        pix.seeds(reads, min_length=8, max_per_seed=16, msa=True)
        pix.chains()
        assert "fbg_pindex_seeds_strands" in fails(pix, len(reads) // 2 * 2)      # an unstranded seeds call, chained
        sd = pix.seeds(reads, min_length=8, max_per_seed=16, msa=True, strands=True)
        assert "fbg_pindex_chains" in fails(pix, V)                               # no chaining call
        with pytest.raises(ValueError):
            pix.chains(pair_align=True)                                           # pair_align without pairs
        ch0 = pix.chains(band=8, align=True)
        assert "min_insert" in fails(pix, V, (5, 4))
        assert "which" in fails(pix, V, null=("which",))
        # after the failed calls the index works, no stage went stale, and every optional output may be NULL
        m = model_of(host, sd, ch0, vreads, (30, 120))
        same_c(c_call(pix, V, (30, 120)), m, "after the failed calls")
        code, out, _ = c_call(pix, V, (30, 120), null=("row", "edits", "t_start", "t_end", "insert", "pair_score", "t_lo", "t_hi", "stats"))
        assert code == 0 and np.array_equal(out[5], m.which) and all((a == 7).all() for a in out[:5] + out[6:])
        total = ctypes.c_uint64(0)
        assert _lib.lib().fbg_pindex_chains_cigar(pix._h, None, ctypes.byref(total), None) == 0
        # an odd number of reads
        pix.seeds(reads[:3], min_length=8, max_per_seed=16, msa=True, strands=True)
        pix.chains()
        assert "even" in fails(pix, 6)
        with pytest.raises(FbgError) as ei:
            pix.chains(pairs=(0, 100), pair_align=True)
        assert ei.value.code == INVALID
        # no reads, and reads without a chain: every output none, nothing launched
        pix.seeds([], msa=True, strands=True)
        e = pix.chains(pairs=(0, 9), pair_align=True)
        assert len(e.mate_which) == 0 and len(e.mate_row) == 0 and e.mate_stats == dict.fromkeys(PA.STATS, 0) and e.mate_ms == 0
        pix.seeds([b"NN", b"", b"N", b"NNN"], msa=True, strands=True)
        e = pix.chains(pairs=(0, 9), pair_align=True, pair_select=np.ones(8, dtype=np.uint8))
        assert e.mate_which.tolist() == [0xff] * 2 and e.mate_score.tolist() == [0, 0] and e.mate_lo.tolist() == [NONE] * 2
        assert e.mate_hi.tolist() == [NONE] * 2 and all(getattr(e, f).tolist() == [NONE] * 8 for f, _ in READ_FIELDS)
        assert e.mate_stats == dict.fromkeys(PA.STATS, 0) and e.mate_ms == 0


def y_lines(m, k):
    """The Y line of every virtual read in the tool's order: pattern by pattern, forward and then reverse."""
    out = []
    for R in range(k):
        for v in (R, R + k):
            if int(m.edits[v]) == NONE:
                out.append(b"Y\t*")
            else:
                ins = b"*" if int(m.insert[v]) == NONE else b"%d" % m.insert[v]
                out.append(b"Y\t%d\t%d\t%d\t%d\t" % (m.row[v], m.edits[v], m.t_start[v], m.t_end[v]) + ins)
    return out


def w_lines(m):
    return [b"W\t*" if w == PA.NO_PAIR else b"W\t%d\t%d\t%d\t%d" % (w, s, lo, hi)
            for w, s, lo, hi in zip(m.which.tolist(), m.pair_score.tolist(), m.t_lo.tolist(), m.t_hi.tolist())]


@pytest.mark.gpu
def test_tool_prints_the_alignments_and_the_pairs(engine, tmp_path):
    from oracle import pyoracle as O
    A = read_fasta(TC.GOLDEN[0])[0]
    b = [int(x) for x in engine.minmax_dp(engine.elastic_f(A))]
    host = Host(A, b)
    rng = np.random.default_rng(3)
    reads, bad = damaged_pairs(rng, host, 8, 4, (4, 7), 3, frag_max=A.shape[1])
    k = len(reads)
    graph = str(tmp_path / "g.xgfa")
    O.write_xgfa(A, b, graph)
    data = b"".join(r + b"\n" for r in reads)
    args = ["--graph=" + graph, "--msa=" + TC.GOLDEN[0], "--seeds=4", "--occurrences", "--chain", "--strands", "--rows", "--pairs=3,15"]
    base = TC.TL.run_locate(args, data)
    got = TC.TL.run_locate(args + ["--pair-align=2"], data)
    assert base.returncode == 0 and got.returncode == 0, (base.stderr, got.stderr)
    with TR.build(engine, A, b) as pix:
        sd = pix.seeds(reads, min_length=4, max_per_seed=64, msa=True, strands=True)
        ch = pix.chains(pairs=(3, 15), adopt_pairs=True, pair_align=True, pair_max_edits=2)
        m = model_of(host, sd, ch, virtual(reads), (3, 15), 2)
        same(ch, m, "tool")
    assert m.stats["aligned"] > 0 and (m.which != PA.NO_PAIR).any()
    lines = got.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith(b"Y\t")] == y_lines(m, k)
    assert [ln for ln in lines if ln.startswith(b"W\t")] == w_lines(m)
    assert all(lines[i - 1].startswith(b"Z\t") for i, ln in enumerate(lines) if ln.startswith(b"W\t"))
    # every other line is that of the run without --pair-align, byte for byte
    assert [ln for ln in lines if ln[:2] not in (b"Y\t", b"W\t")] == base.stdout.splitlines()
    assert b"Y\t" not in base.stdout and b"W\t" not in base.stdout
