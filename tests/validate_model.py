"""Plain restatement of the semi-repeat-free check of a founder graph (fbg_pindex_validate; the reference's
efg_validate_node).

For every node u the first rule that applies gives its status:
  1. u has no in-edge or no out-edge                      SKIP_SOURCE_SINK
  2. label(u) holds a byte of the ignore set              SKIP_IGNORED
  3. label(u) is empty                                    SKIP_EMPTY
  4. every occurrence of label(u) at offset s of label(a) + label(b), over the distinct edges (a, b), belongs to node a
     at offset s if s < |label(a)|, else to node b at offset s - |label(a)|; it is allowed iff that offset is 0 and
     the node's block is u's.  All allowed: VALID, else INVALID.
Witness of an INVALID node: its disallowed occurrence of smallest SA slot in the pattern index's text (locate_model:
reversed edge strings), i.e. among the suffixes that start with reverse(label(u)).

`Validator` follows the rules in the index's terms (slot order); `naive_validate` is a second formulation by
bytes.find over the forward edge strings, duplicates and adjacency order as given, for the CPU tests.  Nothing here
is used by the product.
"""
import bisect

import numpy as np

import locate_model as LM

VALID, INVALID, SKIP_SOURCE_SINK, SKIP_IGNORED, SKIP_EMPTY = range(5)
STATUS_NAMES = ("valid", "invalid", "source_sink", "ignored", "empty")


def degrees(n, edges):
    has_in, has_out = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for u, v in edges:
        has_out[int(u)] = True
        has_in[int(v)] = True
    return has_in, has_out


def skip_status(label, has_in, has_out, ignore):
    """Rules 1-3: the status, or None when rule 4 decides."""
    if not (has_in and has_out):
        return SKIP_SOURCE_SINK
    if any(c in ignore for c in label):
        return SKIP_IGNORED
    if not label:
        return SKIP_EMPTY
    return None


class Validator:
    def __init__(self, labels, edges):
        self.labels = [LM.as_bytes(x) for x in labels]
        self.edges = sorted({(int(u), int(v)) for u, v in edges})     # the index's order: distinct, ascending
        self.has_in, self.has_out = degrees(len(self.labels), self.edges)
        self.T = LM.edge_text(self.labels, self.edges)
        self.Tb = self.T.tobytes()
        self.SA = LM.suffix_array(self.T).tolist()
        self.estart = [0]                                             # text start ('#') of every edge, then N
        for a, b in self.edges:
            self.estart.append(self.estart[-1] + len(self.labels[a]) + len(self.labels[b]) + 1)

    def label_range(self, label):
        """SA slots [l, r) of the suffixes that start with reverse(label)."""
        rev, m, Tb = label[::-1], len(label), self.Tb
        key = lambda p: Tb[p:p + m]                                   # noqa: E731
        return bisect.bisect_left(self.SA, rev, key=key), bisect.bisect_right(self.SA, rev, key=key)

    def occurrence(self, p, m):
        """(node, offset) of the occurrence of an m-symbol label whose reversed copy starts at text position p."""
        e = bisect.bisect_right(self.estart, p) - 1
        base = self.estart[e] + 1
        ne = self.estart[e + 1] - base                                # |label(a)| + |label(b)|
        a, b = self.edges[e]
        s = ne - (p - base) - m                                       # forward offset in label(a) + label(b)
        la = len(self.labels[a])
        return (a, s) if s < la else (b, s - la)

    def validate(self, blocks, ignore=b""):
        """-> (status uint8[n], witness_node int64[n], witness_offset int64[n]); -1 where there is no witness."""
        ignore = set(LM.as_bytes(ignore))
        n = len(self.labels)
        status = np.zeros(n, dtype=np.uint8)
        wn = np.full(n, -1, dtype=np.int64)
        wo = np.full(n, -1, dtype=np.int64)
        for u in range(n):
            lab = self.labels[u]
            st = skip_status(lab, self.has_in[u], self.has_out[u], ignore)
            if st is not None:
                status[u] = st
                continue
            status[u] = VALID
            l, r = self.label_range(lab)
            for i in range(l, r):
                node, off = self.occurrence(self.SA[i], len(lab))
                if off != 0 or blocks[node] != blocks[u]:
                    status[u], wn[u], wo[u] = INVALID, node, off
                    break
        return status, wn, wo

    def slots(self, u):
        """Size of the SA range of label(u)."""
        l, r = self.label_range(self.labels[u])
        return r - l


def naive_validate(labels, edges, blocks, ignore=b""):
    """Second formulation: bytes.find over label(a) + label(b) for every edge as given (duplicates, any order).
    -> (status, {u: set of disallowed (node, offset)})."""
    labels = [LM.as_bytes(x) for x in labels]
    ignore = set(LM.as_bytes(ignore))
    n = len(labels)
    has_in, has_out = degrees(n, edges)
    status = np.zeros(n, dtype=np.uint8)
    bad = {}
    for u in range(n):
        st = skip_status(labels[u], has_in[u], has_out[u], ignore)
        if st is not None:
            status[u] = st
            continue
        dis = set()
        for a, b in edges:
            s, la = labels[int(a)] + labels[int(b)], len(labels[int(a)])
            k = s.find(labels[u])
            while k >= 0:
                node, off = (int(a), k) if k < la else (int(b), k - la)
                if off != 0 or blocks[node] != blocks[u]:
                    dis.add((node, off))
                k = s.find(labels[u], k + 1)
        status[u] = INVALID if dis else VALID
        if dis:
            bad[u] = dis
    return status, bad


def bad_cuts(status, blocks):
    """The reference's to_remove: b - 1 for every block b > 0 that holds an INVALID node, sorted."""
    blocks = np.asarray(blocks, dtype=np.int64)
    b = blocks[np.asarray(status) == INVALID]
    return sorted({int(x) - 1 for x in b if x > 0})


def expected_tool_output(labels, edges, ids, blocks, ignore=b""):
    """(stdout bytes, exit status) of fbg_validate for a graph whose nodes carry S ids `ids` and blocks from 0."""
    status, wn, wo = Validator(labels, edges).validate(blocks, ignore)
    out = []
    for u in np.nonzero(status == INVALID)[0]:
        w = int(wn[u])
        out.append(b"invalid\t%d\t%d\t%d\t%d\t%d\n" % (ids[u], blocks[u] + 1, ids[w], wo[u], blocks[w] + 1))
    c = np.bincount(status, minlength=5)
    out.append(b"nodes\t%d\tvalid\t%d\tinvalid\t%d\tsource_sink\t%d\tignored\t%d\tempty\t%d\n" %
               (len(labels), c[0], c[1], c[2], c[3], c[4]))
    return b"".join(out), 1 if c[1] else 0


def xgfa_ids(path):
    """The S ids of an xGFA file in ascending order (the node order of read_xgfa)."""
    ids = []
    with open(path, "rb") as fh:
        for line in fh:
            f = line.rstrip(b"\r\n").split(b"\t")
            if f[0] == b"S":
                ids.append(int(f[1]))
    return sorted(ids)
