"""Numpy restatement of the pattern index of a founder graph (the founder_block_index of the reference).

Rules (the issue that added fbg_pindex_*):
  1. text T: for every node u in id order and every distinct out-neighbour v in ascending order,
     reverse(label(u) + label(v) + '#'); then one 0 sentinel.  len(T) = N + 1.
  2. SA of T in unsigned byte order; C / occ over the BWT; bs(c, l, r) is one backward step.
  3. B / E: every label, searched left to right from [0, N], sets B[lhs] and E[rhs]; a label whose search finds
     nothing sets no bit.
  4. search of a pattern with the restart at a block pair boundary -> (count, pos).
The model is the checker of the HIP kernels in csrc/locate.hip; nothing here is used by the product.
"""
import bisect

import numpy as np

SEP = ord("#")


def as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def edge_text(labels, edges):
    """labels: list of bytes/str (node id order); edges: iterable of (u, v).  -> uint8 array T with the sentinel."""
    labels = [as_bytes(x) for x in labels]
    out = {}
    for u, v in edges:
        out.setdefault(int(u), set()).add(int(v))
    parts = []
    for u in sorted(out):
        for v in sorted(out[u]):
            parts.append((labels[u] + labels[v] + b"#")[::-1])
    return np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()


def suffix_array(T):
    """Prefix doubling: ranks of the first 2^k symbols, re-sorted by (rank, rank k ahead) until all are distinct."""
    T = np.asarray(T, dtype=np.uint8)
    n = len(T)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    rank = T.astype(np.int64)
    k = 1
    while True:
        nxt = np.full(n, -1, dtype=np.int64)
        if k < n:
            nxt[:n - k] = rank[k:]
        sa = np.lexsort((nxt, rank))
        r1, r2 = rank[sa], nxt[sa]
        new = np.zeros(n, dtype=np.int64)
        new[1:] = np.cumsum((r1[1:] != r1[:-1]) | (r2[1:] != r2[:-1]))
        rank = np.empty(n, dtype=np.int64)
        rank[sa] = new
        if new[-1] == n - 1:
            return sa
        k *= 2


class Index:
    def __init__(self, labels, edges):
        self.labels = [as_bytes(x) for x in labels]
        for x in self.labels:
            if b"#" in x or b"\0" in x:
                raise ValueError("labels may not contain '#' or a zero byte")
        self.T = edge_text(self.labels, edges)
        self.N = len(self.T) - 1
        self.SA = suffix_array(self.T)
        self.bwt = self.T[(self.SA - 1) % len(self.T)]
        hist = np.bincount(self.T, minlength=256)
        self.C = np.concatenate(([0], np.cumsum(hist)[:-1]))
        self.present = hist > 0
        self.occ = {}
        for c in np.nonzero(self.present)[0]:
            self.occ[int(c)] = np.concatenate(([0], np.cumsum(self.bwt == c)))
        B, E = set(), set()
        for lab in self.labels:
            l, r, ok = 0, self.N, True
            for c in lab:
                cnt, l, r = self.bs(c, l, r)
                if cnt == 0:
                    ok = False
                    break
            if ok:
                B.add(l)
                E.add(r)
        self.B = np.array(sorted(B), dtype=np.int64)
        self.E = np.array(sorted(E), dtype=np.int64)
        self._Bl, self._El = self.B.tolist(), self.E.tolist()

    def bs(self, c, l, r):
        if not self.present[c]:
            return 0, l, r
        o = self.occ[int(c)]
        nl = int(self.C[c] + o[l])
        nr = int(self.C[c] + o[r + 1] - 1)
        return nr + 1 - nl, nl, nr

    def locate(self, pattern):
        """-> (count, pos), rule 4."""
        P = as_bytes(pattern)
        l, r, pos, count = 0, self.N, 0, 0
        for c in P:
            count, nl, nr = self.bs(c, l, r)
            if count:
                l, r = nl, nr
            else:
                if self.bs(SEP, l, r)[0] == 0:
                    return 0, pos
                r1 = bisect.bisect_right(self._Bl, l)
                if r1 == 0 or r1 > len(self._El):
                    return 0, pos
                nl, nr = self._Bl[r1 - 1], self._El[r1 - 1]
                if not (nl <= l and r <= nr):
                    return 0, pos
                count, l, r = self.bs(c, nl, nr)
                if count == 0:
                    return 0, pos
            pos += 1
        return count, pos


def read_xgfa(path):
    """(labels, edges) of an xGFA / GFA file: S lines in ascending id order (any base), L lines mapped to 0-based
    indices into labels.  Empty labels are kept."""
    ids, labs, links = [], [], []
    with open(path, "rb") as fh:
        for line in fh:
            f = line.rstrip(b"\r\n").split(b"\t")
            if f[0] == b"S":
                ids.append(int(f[1]))
                labs.append(f[2] if len(f) > 2 else b"")
            elif f[0] == b"L":
                links.append((int(f[1]), int(f[3])))
    order = sorted(range(len(ids)), key=lambda k: ids[k])
    where = {ids[k]: i for i, k in enumerate(order)}
    return [labs[k] for k in order], [(where[u], where[v]) for u, v in links]


def tokens(data):
    """The patterns `std::cin >> pattern` answers in locate_patterns: whitespace-separated tokens, but the last one
    is not answered when the input does not end in whitespace (its read sets EOF)."""
    toks = data.split()
    if toks and not data[-1:].isspace():
        toks = toks[:-1]
    return toks


def expected_stdout(index, data, error_on_not_found=False):
    """The bytes locate_patterns would print for an index of the graph and stdin `data`, and its exit status."""
    out, found = [], 0
    toks = tokens(data)
    for t in toks:
        cnt = index.locate(t)[0]
        out.append(b"Pattern? %d occurrences found.\n" % cnt)
        if cnt == 0 and error_on_not_found:
            return b"".join(out), 1
        found += cnt != 0
    out.append(b"Pattern? %d out of %d patterns found\n" % (found, len(toks)))
    return b"".join(out), 0
