"""Plain NumPy restatement of the MSA coordinates of a reported place (include/fbg_hip.h, fbg_pindex_occurrences_msa).

For an MSA A[m][n] and boundaries (inclusive block ends, the last one n):
  block j    covers the columns [x0, x1), x0 = j ? boundaries[j - 1] + 1 : 0, x1 = min(boundaries[j] + 1, n);
  r(u)       the representative row of node u: the first row, by row index, whose gap-stripped label in u's block is
             label(u) (the numbering of heuristic_model.segmentation_graph: blocks in order, labels by first row);
  col(u, o)  the column of the o-th (from 0) non-gap cell of row r(u) in [x0, x1), 0 <= o < |label(u)|.
A place (a, b, offset) belongs to node a at o = offset if offset < |label(a)|, else to node b at o = offset -
|label(a)|; its coordinate is (r(u), col(u, o)), or (NONE, NONE) when o >= |label(u)|.  One witness row per place.
The model is the checker of the kernels; nothing here is used by the product."""
import numpy as np

import heuristic_model as HM

NONE = 0xffffffff
GAP = ord("-")


class Model:
    def __init__(self, msa, boundaries):
        A = np.ascontiguousarray(msa, dtype=np.uint8)
        m, n = A.shape
        self.A = A
        self.boundaries = [int(b) for b in boundaries]
        self.labels, self.rep_row, self.cols, self.blocks, self.ranges = [], [], [], [], []
        x0 = 0
        for j, b in enumerate(self.boundaries):
            x1 = min(b + 1, n)
            x0 = min(x0, x1)
            seen = set()
            for i in range(m):
                keep = np.nonzero(A[i, x0:x1] != GAP)[0] + x0
                lab = A[i, keep].tobytes()
                if not lab or lab in seen:
                    continue
                seen.add(lab)
                self.labels.append(lab)
                self.rep_row.append(i)
                self.cols.append(keep.astype(np.int64))
                self.blocks.append(j)
                self.ranges.append((x0, x1))
            x0 = b + 1
        # the graph the existing models give: the same nodes in the same order
        labels, self.edges, blocks = HM.segmentation_graph(A, self.boundaries)
        assert labels == self.labels and blocks.tolist() == self.blocks
        self.label_len = np.array([len(s) for s in self.labels], dtype=np.int64)

    def node_of(self, src, dst, offset):
        """(node, offset in the node's label) of places, as Occurrences.as_nodes maps them (no duplicates dropped)."""
        src, dst, o = (np.asarray(x).astype(np.int64) for x in (src, dst, offset))
        la = self.label_len[src] if len(src) else src
        in_src = o < la
        return np.where(in_src, src, dst), np.where(in_src, o, o - la)

    def coords(self, src, dst, offset):
        """(row, col) int64 arrays of the places (src, dst, offset); NONE in both where the offset is outside the edge."""
        node, o = self.node_of(src, dst, offset)
        row = np.full(len(node), NONE, dtype=np.int64)
        col = np.full(len(node), NONE, dtype=np.int64)
        for k, (u, x) in enumerate(zip(node.tolist(), o.tolist())):
            if 0 <= x < len(self.cols[u]):
                row[k], col[k] = self.rep_row[u], self.cols[u][x]
        return row, col

    def edge_symbol(self, src, dst, offset):
        """S_e[offset] of every place, -1 where the offset is outside S_e."""
        out = np.full(len(src), -1, dtype=np.int64)
        for k, (a, b, o) in enumerate(zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(offset).tolist())):
            s = self.labels[a] + self.labels[b]
            if 0 <= o < len(s):
                out[k] = s[o]
        return out

    def on_edges(self):
        """Every (node, offset) of a node that some edge touches: what single-symbol patterns reach."""
        touched = sorted({u for e in self.edges for u in e})
        return {(u, o) for u in touched for o in range(len(self.labels[u]))}
