"""The pattern index and the semi-repeat-free check at their switch points (csrc/pindex_build.hip, locate.hip, pindex_validate.hip).

px_build codes the symbols densely in byte order (the sentinel 0, then '#' unless a label byte sorts below it): at most
16 codes take the compact occ line (4 bit planes, counts inside), more take 8 planes and a count table; the first
doubling round packs K = 64 / ceil(log2 sigma) codes.  An occ query splits its 128-position line at offset 64, and
nblk = N1 / 128 + 1 gives occ(c, N1) a line.  The search reads patterns as 8-byte words in order of length and restarts
at block pair boundaries; the validation finds a text position's edge through a coarse table of every 256th position
and skips labels by a 4 x 64-bit byte mask.  The cases below land on each of those points; every GPU check is exact
equality with tests/locate_model.py and tests/validate_model.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import locate_model as M  # noqa: E402
import validate_model as VM  # noqa: E402
from conftest import random_msa  # noqa: E402
from test_locate import check_index, check_search  # noqa: E402
from test_validate import check  # noqa: E402

SEP = ord("#")
ALL_BYTES = bytes(c for c in range(1, 256) if c != SEP)
SIGMA16 = b"ACGTNRYKMSWBD\x9a"              # 14 label bytes: 16 codes, the last compact alphabet
SIGMA17 = SIGMA16 + b"\xc3"                 # 15 label bytes: 17 codes, the first general one
# sigma (codes: label bytes, '#' and the sentinel) -> label bytes.  The key width b = ceil(log2 sigma) changes at 3, 5,
# 9, 17, 33, 65 and 129; bytes below '#' (sigma 4, 256) move '#' off code 1.
ALPHABETS = {
    2: b"",
    3: b"A",
    4: b"\x01\xff",
    5: b"ACG",
    9: b"ACGTNac",
    16: SIGMA16,
    17: SIGMA17,
    33: bytes(range(0xC0, 0xDF)),
    65: bytes(range(0x24, 0x63)),
    129: bytes(range(0x80, 0xFF)),
    256: ALL_BYTES,
}
IGNORE = b"\x05 Nn\x9a\xc3"                 # one or two bytes in each 64-bit word of the validation's mask


def test_alphabets_have_their_sizes():
    for sigma, alpha in ALPHABETS.items():
        assert len(set(alpha)) == len(alpha) == sigma - 2 and SEP not in alpha and 0 not in alpha
    assert sorted({c >> 6 for c in IGNORE}) == [0, 1, 2, 3]


# ---- inputs -------------------------------------------------------------------------------------------------------

def rand_bytes(rng, alpha, n):
    return np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), n)].tobytes()


def alphabet_graph(rng, alpha, n, max_len, n_edges):
    """Random labels over `alpha` (a tenth of them empty; node 0 holds every byte of it), random edges with self-loops
    and duplicates, in no particular order."""
    labels = [b"" if not alpha or rng.random() < 0.1 else rand_bytes(rng, alpha, int(rng.integers(1, max_len + 1)))
              for _ in range(n)]
    if alpha:
        labels[0] = np.frombuffer(alpha, dtype=np.uint8)[rng.permutation(len(alpha))].tobytes()
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, n_edges), rng.integers(0, n, n_edges))]
    edges += [(int(u), int(u)) for u in rng.integers(0, n, n // 20)]
    edges += [(0, int(rng.integers(0, n))), (int(rng.integers(0, n)), 0)]
    edges += edges[:len(edges) // 5]
    rng.shuffle(edges)
    return labels, edges


def walk(rng, labels, adj, start, steps):
    """label(u0) + label(u1) + ... along a random path of up to `steps` nodes."""
    out, u = [], start
    for _ in range(steps):
        out.append(labels[u])
        if not adj.get(u):
            break
        u = adj[u][int(rng.integers(0, len(adj[u])))]
    return b"".join(out)


def graph_patterns(rng, labels, edges, alpha, n_pat, max_len=40):
    """Substrings of edge strings and of paths through several nodes (restarts), mutated ones, random strings over the
    alphabet, and strings with a byte from outside it: '#', the zero byte, high bytes, absent bytes; the empty
    pattern."""
    adj = {}
    for u, v in edges:
        adj.setdefault(u, []).append(v)
    srcs = sorted(adj)
    odd = b"#\0\x80\xfe\xff" + bytes(c for c in range(1, 256) if c not in alpha and c != SEP)[::17]
    pool = alpha + b"#" if alpha else b"#"
    out = [b""]
    while len(out) < n_pat:
        kind = int(rng.integers(0, 6))
        ln = int(min(max_len, rng.geometric(1 / 10)))
        if kind >= 4:
            out.append(rand_bytes(rng, pool if kind == 4 else pool + odd, ln))
            continue
        u = srcs[int(rng.integers(0, len(srcs)))]
        s = walk(rng, labels, adj, u, 2 if kind == 0 else int(rng.integers(3, 8)))
        if not s:
            continue
        ln = min(ln, len(s))
        a = int(rng.integers(0, len(s) - ln + 1))
        p = bytearray(s[a:a + ln])
        if kind == 2 and alpha:
            p[int(rng.integers(0, ln))] = pool[int(rng.integers(0, len(pool)))]
        elif kind == 3:
            p[int(rng.integers(0, ln))] = odd[int(rng.integers(0, len(odd)))]
        out.append(bytes(p))
    return out


class Probe(M.Index):
    """The model, noting its backward steps once `probe` is set: the in-block offsets of l and r + 1, and how many
    searches went through a restart to the end of their pattern."""

    def __init__(self, labels, edges):
        self.probe = False
        self.off_l, self.off_r1 = set(), set()
        self.seps = self.restarted = 0
        super().__init__(labels, edges)
        self.probe = True

    def bs(self, c, l, r):
        if self.probe:
            self.off_l.add(l % 128)
            self.off_r1.add((r + 1) % 128)
            self.seps += c == SEP
        return super().bs(c, l, r)

    def locate(self, pattern):
        before = self.seps
        cnt, pos = super().locate(pattern)
        if SEP not in M.as_bytes(pattern) and self.seps > before and cnt > 0 and pos == len(pattern):
            self.restarted += 1
        return cnt, pos


def layout_bytes(model):
    """fbg_pindex_stats' index_bytes: occ lines, the count table of a general alphabet, B / E, C and the code table."""
    N1, sigma = model.N + 1, int(model.present.sum())
    nblk = N1 // 128 + 1
    return nblk * 128 + (0 if sigma <= 16 else nblk * sigma * 4) + 4 * (len(model.B) + len(model.E)) + 1536


def text_of_length(rng, alpha, N1):
    """(labels, edges) whose edge text has exactly N1 symbols, the sentinel included: random edges (duplicates among
    them) while they fit, then one edge of two padding labels that makes up the rest."""
    if N1 == 1:
        return [alpha[:3], alpha[:1]], []
    labels, edges, have, total = [], [], set(), 1
    for _ in range(10_000):
        if labels and rng.random() < 0.5:
            u = int(rng.integers(0, len(labels)))
        else:
            labels.append(rand_bytes(rng, alpha, int(rng.integers(0, 30))))
            u = len(labels) - 1
        v = int(rng.integers(0, len(labels)))
        cost = 0 if (u, v) in have else len(labels[u]) + len(labels[v]) + 1
        if total + cost > N1 - 1:
            break
        edges.append((u, v))
        have.add((u, v))
        total += cost
    rest = N1 - total - 1                                   # the padding edge: |a| + |b| = rest
    a = int(rng.integers(0, rest + 1))
    labels += [rand_bytes(rng, alpha, a), rand_bytes(rng, alpha, rest - a)]
    edges.append((len(labels) - 2, len(labels) - 1))
    rng.shuffle(edges)
    return labels, edges


def short_substrings(model, k=4):
    """Every distinct substring of up to k symbols of the forward edge strings (separators included)."""
    fwd = model.T[:-1][::-1].tobytes()
    return sorted({fwd[i:i + j] for j in range(1, k + 1) for i in range(len(fwd) - j + 1)})


def slot_patterns(model, last):
    """One pattern per SA slot that narrows the range to that slot alone and then takes one more step (by `last`): the
    reversed shortest prefix of its suffix that no other suffix shares (the zero sentinel included where it takes
    that).  The occ queries of that step reach every block offset with l and with r + 1."""
    b, sa = model.T.tobytes(), model.SA.tolist()
    lcp = [0] * (len(sa) + 1)
    for i in range(1, len(sa)):
        x, y = b[sa[i - 1]:], b[sa[i]:]
        k = 0
        while k < len(x) and k < len(y) and x[k] == y[k]:
            k += 1
        lcp[i] = k
    return [b[p:p + max(lcp[i], lcp[i + 1]) + 1][::-1] + last for i, p in enumerate(sa)]


# ---- CPU: the models on these alphabets -----------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", sorted(ALPHABETS))
def test_model_suffix_array_is_unsigned_byte_order(sigma):
    rng = np.random.default_rng(200 + sigma)
    labels, edges = alphabet_graph(rng, ALPHABETS[sigma], 60, 12, 90)
    ix = M.Index(labels, edges)
    assert int(ix.present.sum()) == sigma
    b = ix.T.tobytes()
    assert ix.SA.tolist() == sorted(range(len(b)), key=lambda i: b[i:])


def test_validate_model_matches_the_naive_formulation_on_high_bytes():
    rng = np.random.default_rng(9)
    alpha = b"\x05N\x9a\xc3\xfe\x80 "
    seen = np.zeros(5, dtype=int)
    for trial in range(120):
        n = int(rng.integers(1, 14))
        labels = [b"" if rng.random() < 0.1 else rand_bytes(rng, alpha, int(rng.integers(1, 5))) for _ in range(n)]
        edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(int(rng.integers(0, 3 * n + 1)))]
        edges += edges[:len(edges) // 4]
        blocks = rng.integers(0, 4, n).tolist()
        ignore = IGNORE[:int(rng.integers(0, len(IGNORE) + 1))] if trial % 2 else b"\xc3"
        st, wn, wo = VM.Validator(labels, edges).validate(blocks, ignore)
        naive, bad = VM.naive_validate(labels, edges, blocks, ignore)
        assert st.tolist() == naive.tolist(), (labels, edges, blocks, ignore)
        for u in np.nonzero(st == VM.INVALID)[0]:
            assert (int(wn[u]), int(wo[u])) in bad[u]
        seen += np.bincount(st, minlength=5)
    assert (seen > 0).all(), seen


def test_texts_have_the_lengths_asked_for():
    rng = np.random.default_rng(12)
    for N1 in (1, 2, 3, 63, 128, 129, 5121):
        for alpha in (b"ACGT", SIGMA17):
            assert len(M.edge_text(*text_of_length(rng, alpha, N1))) == N1


# ---- GPU: 1. alphabets across the code boundaries -------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sigma", sorted(ALPHABETS))
def test_alphabet_sweep_index_layout_and_search(engine, sigma):
    rng = np.random.default_rng(100 + sigma)
    alpha = ALPHABETS[sigma]
    labels, edges = alphabet_graph(rng, alpha, 300, 40 if sigma > 2 else 0, 700 if sigma > 2 else 3000)
    model = Probe(labels, edges)
    assert int(model.present.sum()) == sigma
    assert (model.N + 1) * sigma <= 10_000_000
    pats = graph_patterns(rng, labels, edges, alpha, 4000)
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        assert pix.stats()["index_bytes"] == layout_bytes(model)          # compact iff sigma <= 16
        count = check_search(pix, model, pats)
    assert (count > 0).sum() > 500
    if sigma > 3:
        assert model.restarted > 0


# ---- GPU: 2. text lengths on occ block edges ----------------------------------------------------------------------

BLOCK_N1 = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 128 * 40 - 1, 128 * 40, 128 * 40 + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [b"ACGT", SIGMA17], ids=["compact", "general"])
@pytest.mark.parametrize("N1", BLOCK_N1)
def test_text_length_on_an_occ_block_edge(engine, N1, alpha):
    rng = np.random.default_rng(N1)
    labels, edges = text_of_length(rng, alpha, N1)
    model = Probe(labels, edges)
    assert model.N + 1 == N1
    single = [bytes([c]) for c in range(256)]                               # the whole text as the range: r + 1 == N1
    pats = [b""] + single + short_substrings(model) + slot_patterns(model, alpha[:1]) + [x for x in labels if x]
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        assert pix.stats()["index_bytes"] == layout_bytes(model)
        count = check_search(pix, model, pats)
    assert count[1:257].tolist() == np.bincount(model.T, minlength=256).tolist()
    if N1 >= 128:                                                           # l and r + 1 at every offset in a line
        for offs in (model.off_l, model.off_r1):
            assert offs == set(range(128)), sorted(set(range(128)) - offs)
    if N1 > 128 and alpha == SIGMA17:
        assert int(model.present.sum()) == 17


# ---- GPU: 3. deep prefix doubling ---------------------------------------------------------------------------------

def periodic_graph(unit, L):
    """Three nodes with the same periodic label of L symbols (one with a self-loop), one with a substitution near its
    end and one with half the label, in a cycle with a chord."""
    P = (unit * (L // len(unit) + 1))[:L]
    V = bytearray(P)
    V[L - 3] = ord("T")
    labels = [P, P, P, bytes(V), P[:L // 2]]
    edges = [(0, 0), (0, 1), (1, 2), (2, 3), (3, 0), (3, 4), (4, 1)]
    return labels, edges


@pytest.mark.gpu
@pytest.mark.parametrize("L", [300, 3000, 20_000])
@pytest.mark.parametrize("unit", [b"A", b"AC", b"ACG"])
def test_deep_doubling_on_periodic_labels(engine, unit, L):
    labels, edges = periodic_graph(unit, L)
    model = M.Index(labels, edges)
    if L <= 300:
        b = model.T.tobytes()
        assert model.SA.tolist() == sorted(range(len(b)), key=lambda i: b[i:])
    P, V = labels[0], labels[3]
    lens = sorted({k for j in range(1, L.bit_length() + 1) for k in (2 ** j - 1, 2 ** j, 2 ** j + 1) if k <= L} |
                  set(range(1, 9)) | {L - 1, L})
    pats = [P[:k] for k in lens] + [P[-k:] for k in lens[::3]]
    pats += [V[L - 3 - k:] for k in (0, 1, 7, 100) if k < L - 3] + [V, V[L // 2:], P + P[:len(unit) * 5], P + P]
    pats += [P[:k] + b"G" for k in (1, 64, L // 3)]
    assert sum(map(len, pats)) <= 400_000
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        count = check_search(pix, model, pats)
    assert count[lens.index(L)] > 0


# ---- GPU: 4. long and awkward patterns ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_long_patterns_along_a_segmented_graph(engine):
    import founderblockgraphs_amd as F
    rng = np.random.default_rng(301)
    msa = random_msa(rng, 8, 21_000, similar=0.97)
    f = engine.elastic_f(msa)
    b = engine.minmax_dp(f)
    labels, edges = F.graph_from_segmentation(engine, msa, b)
    assert len(b) > 500
    model = Probe(labels, edges)
    rows = [r.tobytes() for r in msa]
    along = []
    for k, ln in enumerate((1000, 1500, 2500, 4000, 6000, 9000, 13_000, 20_000)):
        r = rows[k % len(rows)]
        a = int(rng.integers(0, len(r) - ln + 1))
        along.append(r[a:a + ln])
    mutated = []
    for k, p in enumerate(along[:4]):                       # one other base, or an absent byte, half way
        q = bytearray(p)
        q[len(q) // 2] = b"N\xff"[k] if k < 2 else b"CGTA"[b"ACGT".index(q[len(q) // 2])]
        mutated.append(bytes(q))
    # one batch: empty, 1-symbol, short and 20000-symbol patterns in random order, starts at every offset mod 8
    mixed = [b""] * 200 + [bytes([c]) for c in rng.choice(list(b"ACGTN#\x00\xff"), 300)]
    mixed += [rows[int(rng.integers(0, 8))][int(a):int(a) + int(ln)] for a, ln in
              zip(rng.integers(0, 20_000, 100), rng.integers(2, 60, 100))]
    mixed += [rows[k][500:20_500] for k in range(3)]
    order = rng.permutation(len(mixed))
    mixed = [mixed[i] for i in order] + [rows[3][:20_000] + b"AC"]         # the last ends on the buffer's last byte
    starts = np.cumsum([0] + [len(p) for p in mixed[:-1]])
    nonempty = np.array([len(p) > 0 for p in mixed])
    assert set((starts[nonempty] % 8).tolist()) == set(range(8))
    assert sum(map(len, mixed)) % 8 != 0
    with engine.pattern_index(labels, edges) as pix:
        check_index(pix, model)
        count = check_search(pix, model, along + mutated)
        assert all(int(c) > 0 for c in count[:len(along)])
        check_search(pix, model, mixed)
        # a smaller batch after a larger one: the kept pattern buffer holds stale bytes past its end
        small = [p[:37] for p in along[::-1]] + [b"G", b"", rows[5][1:9]]
        check_search(pix, model, small)
    assert model.restarted >= len(along)


# ---- GPU: 5. validation at its lookup edges -----------------------------------------------------------------------

def path_graph(rng, n):
    """A path of n nodes in id order, labels of 1 - 700 symbols (one in twenty of 1 - 3: INVALID), blocks of three
    nodes; last in id order a hub with a unique label and 24 in- and 24 out-edges (VALID through the wave tier)."""
    lens = np.where(rng.random(n) < 0.7, rng.integers(1, 60, n), rng.integers(60, 700, n))
    short = rng.random(n) < 0.05
    lens[short] = rng.integers(1, 4, int(short.sum()))
    labels = [rand_bytes(rng, b"ACGT", int(x)) for x in lens] + [rand_bytes(rng, b"ACGT", 300)]
    hub = n
    edges = [(u, u + 1) for u in range(n - 1)]
    edges += [(int(u), hub) for u in rng.choice(n, 24, replace=False)]
    edges += [(hub, int(v)) for v in rng.choice(n, 24, replace=False)]
    blocks = (np.arange(n + 1) // 3).tolist()
    return labels, edges, blocks


@pytest.mark.gpu
def test_validation_coarse_table_edges(engine):
    rng = np.random.default_rng(401)
    labels, edges, blocks = path_graph(rng, 1500)
    v = VM.Validator(labels, edges)
    starts = np.array(v.estart[:-1])
    assert {0, 1, 254, 255} <= set((starts % 256).tolist())                 # '#' on, after and before a table entry
    assert max(np.diff(v.estart)) > 3 * 256                                 # edges over several table entries
    res, st = check(engine, labels, edges, blocks)
    assert (st == VM.VALID).sum() > 1000 and (st == VM.INVALID).any()
    assert st[-1] == VM.VALID and res.wave_nodes > 0                        # the hub: 48 allowed slots, the wave tier


@pytest.mark.gpu
def test_validation_beyond_65536_edges(engine):
    rng = np.random.default_rng(402)
    n = 1500
    labels = [rand_bytes(rng, b"ACGT", int(x)) for x in rng.integers(3, 10, n)]
    pairs = rng.integers(0, n, (80_000, 2))
    edges = [(int(u), int(v)) for u, v in pairs]
    assert len(set(edges)) > 1 << 16
    blocks = rng.integers(0, 20, n)
    res, st = check(engine, labels, edges, blocks)
    assert (st == VM.INVALID).any() and (st == VM.VALID).any() and res.wave_nodes > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [17, 256])
def test_validation_ignore_mask_words(engine, sigma):
    rng = np.random.default_rng(500 + sigma)
    alpha = ALPHABETS[sigma]
    n = 400
    labels = [b"" if rng.random() < 0.05 else rand_bytes(rng, alpha, int(rng.integers(1, 7))) for _ in range(n)]
    for k, c in enumerate(IGNORE):                                          # labels whose only ignored byte is c
        if c in alpha:
            labels[20 + k] = bytes([c]) + rand_bytes(rng, bytes(x for x in alpha if x not in IGNORE), 4)
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 1200), rng.integers(0, n, 1200))]
    edges += [(0, u) for u in range(1, 40)] + [(u, 0) for u in range(20, 60)]        # node 0: a wave-tier range
    edges += edges[:100]
    blocks = rng.integers(0, 8, n)
    res, st = check(engine, labels, edges, blocks, IGNORE)
    assert (st == VM.INVALID).any() and (st == VM.VALID).any() and res.wave_nodes > 0
    words = {c >> 6 for u in np.nonzero(st == VM.SKIP_IGNORED)[0] for c in set(labels[u]) & set(IGNORE)
             if len(set(labels[u]) & set(IGNORE)) == 1}
    assert words == {c >> 6 for c in IGNORE if c in alpha}
    # the same graph without the mask: those nodes are checked
    res, st2 = check(engine, labels, edges, blocks)
    assert not (st2 == VM.SKIP_IGNORED).any()
