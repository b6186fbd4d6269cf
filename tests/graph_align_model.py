"""The edit distance of each read to a path of the graph around its chain, and that path (include/fbg_hip.h,
fbg_pindex_chains_align_graph), restated cell by cell on byte strings.

The graph comes from heuristic_model.segmentation_graph (labels, distinct edges, the block of every node; node ids ascend
block by block and an edge joins a block to the next), the places from rows_model.Model.node_and_offset; the chains come
from elsewhere (the engine, or the other models on the CPU).  For a (virtual) read with text P of L symbols and a chain
whose anchor i lies in node u_i at offset o_i, block j_i, read offset q_i:
  minlen[j]  the shortest label of block j (0 without nodes), C[j] the sum of minlen over the blocks before j;
  jl         min over the anchors of the largest j <= j_i with C[j_i] - C[j] >= max(0, q_i + pad - o_i), else 0;
  jh         max over the anchors of the smallest j >= j_i with C[j + 1] - C[j_i + 1] >=
             max(0, (L - q_i) + pad - (|label(u_i)| - o_i)), else nb - 1;
  H          the nodes of the blocks jl .. jh and the edges between them; cells = L * sum of |label(v)| over H;
  D_v(i, c)  c = 1 .. |label(v)|, i = 0 .. L: D_v(0, c) = 0, the usual unit-cost recurrence, column 0 of v the row-wise
             minimum of the last columns of v's predecessors in H, or D(i) = i for a node of block jl or without one;
  edits      min D_v(L, c), or L; the end (node, c) is the first cell in (node id, column) order strictly below every
             earlier one and below L, else (first node of block jl, 0);
  path       walking back from the end cell with the reversed read against the reversed suffix (D'(0, x) = x): the first
             offset met inside the current node at which D'(L, .) == edits is the start (the end offset itself and offset
             0 count); otherwise the walk steps to the smallest predecessor u in H with
             min_i (F_u(i) + B(L - i)) == edits, F_u the last column of u, B the walk's column at v's first symbol.
Skipped, with NONE in the five arrays and no path: an empty chain; a read the mask leaves out; L > max_read; then
cells > max_cells (0: no limit).  Every column step exists twice: step_cells, the recurrence cell by cell, and step_rows,
the same a whole column at a time in numpy (forward_blocks: for every node of a block at once), for the long reads and
the large inputs; the CPU tests compare the forms on every small input.  brute() is the
check of the definition over every path of H and every substring of its spelling.  The model is the checker of the
kernels; nothing here is used by the product."""
from types import SimpleNamespace

import numpy as np

import heuristic_model as HM

NONE = 0xffffffff
MAX_READ = 1024
LITERAL_CELLS = 1 << 13      # windows of more cells than this go a column at a time
FIELDS = ("edits", "start_node", "start_offset", "end_node", "end_offset", "n_path")


class Graph:
    def __init__(self, labels, edges, blocks, nb):
        self.labels = [bytes(x) for x in labels]
        self.block_of = [int(j) for j in blocks]
        self.nb = int(nb)
        self.edges = sorted((int(u), int(v)) for u, v in edges)
        n = len(self.labels)
        assert self.block_of == sorted(self.block_of)
        self.first = [sum(1 for j in self.block_of if j < k) for k in range(self.nb + 1)]
        self.preds = [[] for _ in range(n)]
        self.succs = [[] for _ in range(n)]
        for u, v in self.edges:
            assert self.block_of[v] == self.block_of[u] + 1            # strictly layered
            self.preds[v].append(u)
            self.succs[u].append(v)
        self.minlen = [min((len(self.labels[v]) for v in range(self.first[j], self.first[j + 1])), default=0) for j in range(self.nb)]
        self.C = [0]
        for x in self.minlen:
            self.C.append(self.C[-1] + x)

    @classmethod
    def of(cls, msa, boundaries):
        labels, edges, blocks = HM.segmentation_graph(msa, boundaries)
        return cls(labels, edges, blocks, len(boundaries))

    def table_bytes(self):
        return 4 * (len(self.labels) + 1) + 4 * len(self.edges) + 8 * (self.nb + 1)

    def window(self, anchors, L, pad):
        """anchors: (node, offset in the node, q_start) of every anchor -> (jl, jh)."""
        C, jl, jh = self.C, self.nb, 0
        for u, o, q in anchors:
            ji = self.block_of[u]
            left = max(0, q + pad - o)
            right = max(0, (L - q) + pad - (len(self.labels[u]) - o))
            lo = max((j for j in range(ji + 1) if C[ji] - C[j] >= left), default=0)
            hi = min((j for j in range(ji, self.nb) if C[j + 1] - C[ji + 1] >= right), default=self.nb - 1)
            jl, jh = min(jl, lo), max(jh, hi)
        return jl, jh


# ---- one column of the recurrence, twice -------------------------------------------------------------------------------

def step_cells(col, P, c, top):
    """The column after the text symbol c from the column before it; top: its row 0."""
    new = [top] + [0] * len(P)
    for i in range(1, len(P) + 1):
        new[i] = min(col[i - 1] + (P[i - 1] != c), col[i] + 1, new[i - 1] + 1)
    return new


def step_rows(col, P, c, top):
    """step_cells a whole column at a time: new[i] = min over k <= i of (min(diagonal, horizontal) at k) + (i - k)."""
    Pn = np.frombuffer(bytes(P), dtype=np.uint8)
    col = np.asarray(col, dtype=np.int64)
    idx = np.arange(len(P) + 1, dtype=np.int64)
    base = np.empty(len(P) + 1, dtype=np.int64)
    base[0] = top
    base[1:] = np.minimum(col[:-1] + (Pn != c), col[1:] + 1)
    return np.minimum.accumulate(base - idx) + idx


def forward_blocks(g, jl, jh, P):
    """forward() with step_rows on every node of a block at once: one matrix row per node, the nodes whose label has ended
    keep their column.  The first strict minimum in (node id, column) order is found from every node's values of row L."""
    L, n0 = len(P), g.first[jl]
    Pn = np.frombuffer(bytes(P), dtype=np.uint8)
    idx = np.arange(L + 1, dtype=np.int64)
    last, best, end = {}, L, (n0, 0)
    for j in range(jl, jh + 1):
        nodes = list(range(g.first[j], g.first[j + 1]))
        if not nodes:
            continue
        S = np.empty((len(nodes), L + 1), dtype=np.int64)
        for k, v in enumerate(nodes):
            ps = [u for u in g.preds[v] if u >= n0] if j > jl else []
            S[k] = np.minimum.reduce([last[u] for u in ps]) if ps else idx
        lens = np.array([len(g.labels[v]) for v in nodes])
        width = int(lens.max())
        sym = np.zeros((len(nodes), width), dtype=np.uint8)
        for k, v in enumerate(nodes):
            sym[k, :lens[k]] = np.frombuffer(g.labels[v], dtype=np.uint8)
        score = np.full((len(nodes), width), L + 1, dtype=np.int64)
        for t in range(width):
            live = np.flatnonzero(lens > t)
            cur = S[live]
            base = np.empty_like(cur)
            base[:, 0] = 0
            base[:, 1:] = np.minimum(cur[:, :-1] + (Pn[None, :] != sym[live, t][:, None]), cur[:, 1:] + 1)
            S[live] = np.minimum.accumulate(base - idx, axis=1) + idx
            score[live, t] = S[live, L]
        for k, v in enumerate(nodes):
            last[v] = S[k].copy()
            if score[k].min() < best:
                best, end = int(score[k].min()), (v, int(score[k].argmin()) + 1)
    return best, end, last


def forward(g, jl, jh, P, step=step_cells, merges=None):
    """-> (edits, (end_node, end_offset), the last column of every node of H)."""
    L, n0, n1 = len(P), g.first[jl], g.first[jh + 1]
    last, best, end = {}, L, (n0, 0)
    for v in range(n0, n1):
        ps = [u for u in g.preds[v] if u >= n0] if g.block_of[v] > jl else []
        if ps:
            col = [min(last[u][i] for u in ps) for i in range(L + 1)]
            if merges is not None:
                merges.append((v, ps))
        else:
            col = list(range(L + 1))
        for c, ch in enumerate(g.labels[v]):
            col = step(col, P, ch, 0)
            if col[L] < best:
                best, end = col[L], (v, c + 1)
        last[v] = col
    return best, end, last


def trace(g, jl, P, last, edits, end, step=step_cells, steps=None):
    """-> ((start_node, start_offset), the nodes from the start node to the end node)."""
    L, n0 = len(P), g.first[jl]
    Pr = bytes(P)[::-1]
    v, use = end
    if edits == L:
        return (v, use), [v]
    col, x, path = list(range(L + 1)), 0, []
    while True:
        path.append(v)
        lab = g.labels[v]
        for t in range(use):
            x += 1
            col = step(col, Pr, lab[use - 1 - t], x)
            if col[L] == edits:
                return (v, use - 1 - t), path[::-1]
        ps = [u for u in g.preds[v] if u >= n0] if g.block_of[v] > jl else []
        back = np.asarray(col, dtype=np.int64)[::-1]
        ok = [u for u in ps if int((np.asarray(last[u], dtype=np.int64) + back).min()) == edits]
        assert ok, "a node without a start has a predecessor that keeps the distance"
        if steps is not None:
            steps.append((v, ok))
        v = ok[0]
        use = len(g.labels[v])


def lev(a, b):
    col = list(range(len(a) + 1))
    for x, ch in enumerate(b):
        col = step_cells(col, a, ch, x + 1)
    return col[len(a)]


def spell(g, path, start_offset, end_offset):
    s = b"".join(g.labels[v] for v in path)
    return s[start_offset:len(s) - len(g.labels[path[-1]]) + end_offset]


def paths_of(g, jl, jh):
    """Every path of H, as tuples of nodes."""
    n0, n1 = g.first[jl], g.first[jh + 1]
    out = []

    def grow(p):
        out.append(tuple(p))
        for w in g.succs[p[-1]]:
            if w < n1:
                grow(p + [w])
    for v in range(n0, n1):
        grow([v])
    return out


def brute(g, jl, jh, P):
    """The same by the definition's words -> (edits, end, start, path): the minimum of lev over every substring of the
    spelling of every path of H (a substring starts inside the path's first node and ends inside its last), the smallest
    end among those that attain it, then the walk's choices among the paths and starts that attain it with that end."""
    P = bytes(P)
    L, n0 = len(P), g.first[jl]
    val = {}
    for p in paths_of(g, jl, jh):
        text = b"".join(g.labels[v] for v in p)
        head, tail = len(g.labels[p[0]]), len(text) - len(g.labels[p[-1]])
        for s in range(head):
            col = list(range(L + 1))
            for x in range(s, len(text)):
                col = step_cells(col, P, text[x], x - s + 1)
                if x + 1 > tail:
                    val[(p, s, x + 1 - tail)] = col[L]
    edits = min(min(val.values()), L)
    if edits == L:
        return L, (n0, 0), (n0, 0), [n0]
    hits = [k for k, d in val.items() if d == edits]
    end = min((p[-1], e) for p, s, e in hits)
    hits = [(p, s) for p, s, e in hits if (p[-1], e) == end]
    suffix = (end[0],)
    while True:
        here = [s for p, s in hits if p == suffix]
        if here:
            return edits, end, (suffix[0], max(here)), list(suffix)
        suffix = (min(p[-len(suffix) - 1] for p, s in hits if len(p) > len(suffix) and p[-len(suffix):] == suffix),) + suffix


# ---- the call ------------------------------------------------------------------------------------------------------------

def batches_of(sizes, batch_kib):
    """The batches of fbg_pindex_chains_align_graph: consecutive reads from one with scratch on, while the sum fits."""
    budget, n, r0, out = max(int(batch_kib), 1) * 128, len(sizes), 0, 0
    while r0 < n:
        if sizes[r0] == 0:
            r0 += 1
            continue
        r1, total = r0 + 1, sizes[r0]
        while r1 < n and total + sizes[r1] <= budget:
            total += sizes[r1]
            r1 += 1
        out += 1
        r0 = r1
    return out


def align_graph(g, rm, vreads, chain_off, anchor_place, anchor_seed, q_start, start_src, start_dst, start_offset, pad=16, max_cells=0,
                select=None, max_read=MAX_READ, batch_kib=1 << 20, check=None, rows_only=False):
    """-> a namespace with the six arrays (uint32[n]), path_off (uint64[n + 1]) and path_nodes (uint32), stats (the dict of
    PatternIndex.graph_align_stats without table_bytes), and per read its window (jl, jh) and its cells (None, 0 without
    anchors).  check: called with (R, P, jl, jh, result) for every aligned read."""
    n = len(chain_off) - 1
    pad = min(int(pad), 1 << 33)
    out = np.full((6, n), NONE, dtype=np.uint32)
    out[5] = 0
    st = dict(aligned=0, not_selected=0, too_long=0, too_wide=0, cells=0, nodes=0, merges=0, path_nodes=0)
    wins, cells, sizes, paths = [None] * n, [0] * n, [0] * n, [[] for _ in range(n)]
    for R in range(n):
        a, b = int(chain_off[R]), int(chain_off[R + 1])
        if a == b:
            continue
        P = bytes(vreads[R])
        L = len(P)
        anchors = []
        for pl, t in zip(anchor_place[a:b], anchor_seed[a:b]):
            u, o = rm.node_and_offset(int(start_src[pl]), int(start_dst[pl]), int(start_offset[pl]))
            if 0 <= o < len(g.labels[u]):
                anchors.append((u, o, int(q_start[t])))
        if not anchors:
            continue
        jl, jh = g.window(anchors, L, pad)
        n0, n1 = g.first[jl], g.first[jh + 1]
        text = sum(len(g.labels[v]) for v in range(n0, n1))
        wins[R], cells[R] = (jl, jh), L * text
        if select is not None and not select[R]:
            st["not_selected"] += 1
            continue
        if L > max_read:
            st["too_long"] += 1
            continue
        if max_cells and L * text > max_cells:
            st["too_wide"] += 1
            continue
        step = step_rows if rows_only or L * text > LITERAL_CELLS else step_cells
        edits, end, last = forward_blocks(g, jl, jh, P) if step is step_rows else forward(g, jl, jh, P, step)
        start, path = trace(g, jl, P, last, edits, end, step)
        if check:
            check(R, P, jl, jh, (edits, end, start, path))
        out[:, R] = edits, start[0], start[1], end[0], end[1], len(path)
        paths[R] = path
        st["aligned"] += 1
        st["cells"] += L * text
        st["nodes"] += n1 - n0
        st["merges"] += sum(len(g.preds[v]) for v in range(g.first[jl + 1], n1))
        st["path_nodes"] += len(path)
        sizes[R] = (n1 - n0) * 2 * ((L + 63) // 64)
    st["batches"] = batches_of(sizes, batch_kib)
    off = np.concatenate(([0], np.cumsum(out[5].astype(np.uint64)))).astype(np.uint64)
    nodes = np.array([v for p in paths for v in p], dtype=np.uint32)
    res = SimpleNamespace(stats=st, windows=wins, cells=cells, path_off=off, path_nodes=nodes, paths=paths)
    for f, arr in zip(FIELDS, out):
        setattr(res, f, arr)
    return res


def of_cpu(g, c, pad=16, max_cells=0, select=None, **kw):
    """The model on what test_rows.cpu() (or byrow_model.as_cpu) made of an input."""
    return align_graph(g, c.rm, c.vreads, c.chain_off, c.anchor_place, c.anchor_seed, c.q_start, c.start_src, c.start_dst, c.start_offset,
                       pad, max_cells, select, **kw)


def best_edits(edits, strand):
    """Per given read the edits of the strand that Chains.strand picked, NONE where the strand is 0xff."""
    k = len(strand)
    return np.array([NONE if s == 0xff else int(edits[int(s) * k + R]) for R, s in enumerate(strand)], dtype=np.uint32)
