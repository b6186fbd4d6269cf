"""The alignment path of each aligned read (include/fbg_hip.h, fbg_pindex_chains_cigar), restated on byte strings.

For a read with text P of L symbols that fbg_pindex_chains_align laid on T = G_r[t_start : t_end) of N symbols:
  E        E(i, j) = lev(P[i:], T[j:]):  E(L, j) = N - j, E(i, N) = L - i,
           E(i, j) = min(E(i+1, j+1) + [P[i] != T[j]], E(i+1, j) + 1, E(i, j+1) + 1);
  walk     from (0, 0) to (L, N), at every cell the first move that keeps the distance: the diagonal (`=` for equal
           symbols, `X` otherwise), then `I` (a read symbol alone), then `D` (a text symbol alone);
  runs     equal consecutive ops merged, each length << 4 | code with I = 1, D = 2, `=` = 7, X = 8.
suffix_dp holds E as a full matrix, cell by cell; suffix_dp_by_rows is the same recurrence a row at a time in numpy for the
long reads, every row kept, and the CPU tests compare the two on every small input.  brute_path is the independent check:
every alignment of cost edits, enumerated, and the smallest of them position by position in the order (=, X) < I < D.
The model is the checker of the kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import align_model as AM

NONE = AM.NONE
I, D, EQ, X = 1, 2, 7, 8
LETTER = {I: "I", D: "D", EQ: "=", X: "X"}
RANK = {"=": 0, "X": 0, "I": 1, "D": 2}
LDS_WORDS = 4                # reads of up to this many 64-symbol words keep their column history in LDS


def suffix_dp(P, T):
    """E as a list of L + 1 rows of N + 1 values, cell by cell."""
    L, N = len(P), len(T)
    E = [[0] * (N + 1) for _ in range(L + 1)]
    for j in range(N + 1):
        E[L][j] = N - j
    for i in range(L - 1, -1, -1):
        E[i][N] = L - i
        for j in range(N - 1, -1, -1):
            E[i][j] = min(E[i + 1][j + 1] + (P[i] != T[j]), E[i + 1][j] + 1, E[i][j + 1] + 1)
    return E


def suffix_dp_by_rows(P, T):
    """The same matrix a row at a time (align_model.last_row_by_rows mirrored: the running minimum comes from the right)."""
    L, N = len(P), len(T)
    Tn = np.frombuffer(bytes(T), dtype=np.uint8)
    idx = np.arange(N + 1, dtype=np.int64)
    E = np.empty((L + 1, N + 1), dtype=np.int64)
    E[L] = N - idx
    for i in range(L - 1, -1, -1):
        base = np.empty(N + 1, dtype=np.int64)
        base[N] = L - i
        base[:N] = np.minimum(E[i + 1][1:] + (Tn != P[i]), E[i + 1][:N] + 1)
        # E(i, j) = min over k >= j of base[k] + (k - j)
        E[i] = np.minimum.accumulate((base + idx)[::-1])[::-1] - idx
    return E


def walk(P, T, E):
    """The op string of the definition's walk, one character per step."""
    L, N = len(P), len(T)
    i = j = 0
    ops = []
    while i < L or j < N:
        if i < L and j < N and E[i][j] == E[i + 1][j + 1] + (P[i] != T[j]):
            ops.append("=" if P[i] == T[j] else "X")
            i, j = i + 1, j + 1
        elif i < L and E[i][j] == E[i + 1][j] + 1:
            ops.append("I")
            i += 1
        else:
            assert j < N and E[i][j] == E[i][j + 1] + 1, (i, j)
            ops.append("D")
            j += 1
    return "".join(ops)


LITERAL_CELLS = AM.LITERAL_CELLS


def path(P, T):
    """-> (op string, E(0, 0))."""
    P, T = bytes(P), bytes(T)
    E = suffix_dp(P, T) if len(P) * len(T) <= LITERAL_CELLS else suffix_dp_by_rows(P, T)
    return walk(P, T, E), int(E[0][0])


def runs_of(ops):
    """[(code, length)] of an op string."""
    out = []
    for ch in ops:
        code = {"I": I, "D": D, "=": EQ, "X": X}[ch]
        if out and out[-1][0] == code:
            out[-1][1] += 1
        else:
            out.append([code, 1])
    return [(c, n) for c, n in out]


def string_of(runs):
    return "".join(f"{n}{LETTER[c]}" for c, n in runs)


def encode(runs):
    return [n << 4 | c for c, n in runs]


def brute_paths(P, T, edits):
    """Every alignment of P and T of exactly `edits` edits, as op strings."""
    P, T = bytes(P), bytes(T)
    L, N = len(P), len(T)
    out = []

    def go(i, j, cost, ops):
        if cost + abs((L - i) - (N - j)) > edits:
            return
        if i == L and j == N:
            if cost == edits:
                out.append("".join(ops))
            return
        if i < L and j < N:
            go(i + 1, j + 1, cost + (P[i] != T[j]), ops + ["=" if P[i] == T[j] else "X"])
        if i < L:
            go(i + 1, j, cost + 1, ops + ["I"])
        if j < N:
            go(i, j + 1, cost + 1, ops + ["D"])
    go(0, 0, 0, [])
    return out


def brute_path(P, T, edits):
    """-> (the smallest optimal alignment in the order (=, X) < I < D position by position, how many there are).  No
    alignment may be cheaper than edits."""
    assert (len(P) <= 8 and len(T) <= 12) or edits <= 3          # what keeps the enumeration small
    assert all(not brute_paths(P, T, d) for d in range(edits))
    all_ = brute_paths(P, T, edits)
    return min(all_, key=lambda s: [RANK[ch] for ch in s]), len(all_)


def consequences(runs, L, N, edits):
    """What the definition implies for the runs of one aligned read."""
    cnt = {c: 0 for c in LETTER}
    for c, n in runs:
        assert n > 0
        cnt[c] += n
    assert all(a[0] != b[0] for a, b in zip(runs, runs[1:])), runs
    assert cnt[X] + cnt[I] + cnt[D] == edits, (runs, edits)
    assert cnt[EQ] + cnt[X] + cnt[I] == L, (runs, L)
    assert cnt[EQ] + cnt[X] + cnt[D] == N, (runs, N)
    assert len(runs) <= 2 * edits + 1
    if runs:
        assert runs[0][0] != D and runs[-1][0] != D, runs


def history_bytes(L, N):
    """Bytes of column history in device memory for a read of L symbols against N columns."""
    nw = (L + 63) // 64
    return nw * N * 16 if nw > LDS_WORDS else 0


def batches(hist, budget):
    """How many batches reads with these history bytes, in read order, take: consecutive reads from one with a history on
    while the sum fits the budget; a read that alone exceeds it is a batch of its own."""
    count, room = 0, None
    for h in hist:
        if h == 0:
            continue
        if room is None or h > room:
            count, room = count + 1, budget
        room = max(room - h, 0)
    return count


def of_align(c, m, check=None):
    """The model on what test_rows.cpu() made of an input (c) and align_model.of_cpu of its alignment (m) -> off (uint64
    [n + 1]), ops (uint32), runs (per read [(code, length)]), stats (the dict of PatternIndex.cigar_stats).  check: called
    with (P, T, edits, op string) for every aligned read."""
    n = len(c.vreads)
    off, ops, runs, hist = [0], [], [], []
    st = dict(paths=0, ops=0, columns=0, history_bytes=0, batches=0)
    for R in range(n):
        r = []
        if m.edits[R] != NONE:
            P = bytes(c.vreads[R])
            T = c.rm.G[int(m.row[R])][int(m.t_start[R]):int(m.t_end[R])]
            s, e = path(P, T)
            assert e == int(m.edits[R]), (R, e, int(m.edits[R]))
            if check:
                check(P, T, e, s)
            r = runs_of(s)
            consequences(r, len(P), len(T), e)
            st["paths"] += 1
            st["columns"] += len(T)
            hist.append(history_bytes(len(P), len(T)))
        runs.append(r)
        ops += encode(r)
        off.append(len(ops))
    st["ops"] = len(ops)
    st["history_bytes"] = sum(hist)
    st["batches"] = batches(hist, 1 << 30)                    # with the default path_batch_kib
    return SimpleNamespace(hist=hist, off=np.array(off, dtype=np.uint64), ops=np.array(ops, dtype=np.uint32), runs=runs, stats=st,
                           strings=[string_of(r) for r in runs])
