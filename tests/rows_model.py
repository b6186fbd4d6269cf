"""Which MSA rows carry a start place, and which carry a whole chain (include/fbg_hip.h, fbg_pindex_seeds_rows /
fbg_pindex_chains_rows), restated on strings.

Everything comes from the MSA bytes and the boundaries alone:
  G_r            row r with its gap cells removed;
  p(r, j)        the number of non-gap cells of row r before the first column of block j;
  node_of[r][j]  the node of row r in block j (blocks in order, within a block by first appearance by row), None for a
                 row that is all gaps there.
A start place (a, b, offset) of a seed with the read substring S belongs to node u at o: u = a, o = offset if offset <
|label(a)|, else u = b, o = offset - |label(a)|.  Row r supports it iff o < |label(u)|, node_of[r][block(u)] == u and
G_r[x : x + |S|] == S with x = p(r, block(u)) + o (a row whose text ends before x + |S| does not).  rows(place) is the
set of supporting rows; rows(chain) the intersection over the chain's anchors, empty for an empty chain.  Only the
places (and the chains picked among them) are taken from elsewhere: the engine, or occ_model / seeds_model / chain_model
on the CPU.  The model is the checker of the kernels; nothing here is used by the product."""
import numpy as np

NONE = 0xffffffff
GAP = ord("-")


class Model:
    def __init__(self, msa, boundaries):
        A = np.ascontiguousarray(msa, dtype=np.uint8)
        self.A = A
        self.m, n = A.shape
        self.G = [A[r][A[r] != GAP].tobytes() for r in range(self.m)]
        self.ranges, self.labels, self.block_of = [], [], []
        self.node_of = [[None] * len(boundaries) for _ in range(self.m)]
        self.p = [[0] * len(boundaries) for _ in range(self.m)]
        x0 = 0
        for j, b in enumerate(int(x) for x in boundaries):
            x1 = min(b + 1, n)
            x0 = min(x0, x1)
            self.ranges.append((x0, x1))
            ids = {}
            for r in range(self.m):
                self.p[r][j] = int((A[r, :x0] != GAP).sum())
                lab = A[r, x0:x1].tobytes().replace(b"-", b"")
                if not lab:
                    continue
                if lab not in ids:
                    ids[lab] = len(self.labels)
                    self.labels.append(lab)
                    self.block_of.append(j)
                self.node_of[r][j] = ids[lab]
            x0 = b + 1

    def node_and_offset(self, a, b, offset):
        la = len(self.labels[a])
        return (a, offset) if offset < la else (b, offset - la)

    def rows(self, place, S):
        """The ascending list of rows that support the start place (a, b, offset) of a seed with the substring S."""
        u, o = self.node_and_offset(*(int(v) for v in place))
        S = bytes(S)
        if not 0 <= o < len(self.labels[u]):
            return []
        j = self.block_of[u]
        out = []
        for r in range(self.m):
            x = self.p[r][j] + o
            if self.node_of[r][j] == u and self.G[r][x:x + len(S)] == S:       # a short slice is not equal to S
                out.append(r)
        return out

    def rows_by_cells(self, place, S):
        """The same set by a scan of the MSA cells of every row, without G, p or node_of: the row's cells of block(u)
        must spell label(u), and from the o-th of them on the row's non-gap cells must spell S."""
        u, o = self.node_and_offset(*(int(v) for v in place))
        S = bytes(S)
        if not 0 <= o < len(self.labels[u]):
            return []
        x0, x1 = self.ranges[self.block_of[u]]
        out = []
        for r in range(self.m):
            row = self.A[r]
            cells = [x for x in range(x0, x1) if row[x] != GAP]
            if bytes(row[cells].tolist()) != self.labels[u]:
                continue
            x, k = cells[o], 0
            while k < len(S) and x < len(row):
                if row[x] != GAP:
                    if row[x] != S[k]:
                        break
                    k += 1
                x += 1
            if k == len(S):
                out.append(r)
        return out


def substrings(reads, seed_off, q_start, length):
    """The read substring of every seed; reads: the (virtual) reads the seeds call searched, in its order."""
    out = []
    for R in range(len(seed_off) - 1):
        P = bytes(reads[R])
        for t in range(int(seed_off[R]), int(seed_off[R + 1])):
            out.append(P[int(q_start[t]):int(q_start[t]) + int(length[t])])
    return out


def seed_rows(model, reads, seed_off, q_start, length, start_off, start_src, start_dst, start_offset):
    """-> (n_rows uint32[], first_row uint32[], the set of every start place as a list of lists)."""
    S = substrings(reads, seed_off, q_start, length)
    sets = []
    for t in range(len(S)):
        for g in range(int(start_off[t]), int(start_off[t + 1])):
            sets.append(model.rows((start_src[g], start_dst[g], start_offset[g]), S[t]))
    return (np.array([len(s) for s in sets], dtype=np.uint32),
            np.array([s[0] if s else NONE for s in sets], dtype=np.uint32), sets)


def chain_rows(m, sets, chain_off, anchor_place):
    """-> (n_rows uint32[n], first_row uint32[n], row_bits uint64[n, ceil(m / 64)], the sets as sorted lists)."""
    n, words = len(chain_off) - 1, (m + 63) // 64
    bits = np.zeros((n, words), dtype=np.uint64)
    out = []
    for R in range(n):
        places = [int(g) for g in anchor_place[int(chain_off[R]):int(chain_off[R + 1])]]
        rows = set(range(m)) if places else set()
        for g in places:
            rows &= set(sets[g])
        out.append(sorted(rows))
        for r in out[-1]:
            bits[R, r // 64] |= np.uint64(1 << (r % 64))
    return (np.array([len(s) for s in out], dtype=np.uint32), np.array([s[0] if s else NONE for s in out], dtype=np.uint32),
            bits, out)
