"""Plain Python restatement of fbg_pindex_occurrences (include/fbg_hip.h): where a pattern's matches end and start.

Notation: distinct edge e = (a, b) in the order of the text (by a, then b), S_e = label(a) + label(b), n_e = |S_e|;
its reversed copy with the leading '#' starts at text position estart[e], base = estart[e] + 1.  A place is
(a, b, offset into S_e).  Rule 4 of locate_model.Index.locate runs unchanged and records
  restarts   the steps that took the restart branch and went on;
  k, [sl, sr]  at the first of them, before the range is replaced: symbols matched so far and the range after the
             '#' step;
  t          symbols matched so far at the last of them;
  [l, r]     the final range, if count > 0.
Found pattern: ends = for slot i in [l, r], p = SA[i], e = the edge holding p: (a, b, n_e - 1 - (p - base)); starts =
the same slots at offset - |P| + 1 when restarts == 0, else for slot i in [sl, sr], e with estart[e] == SA[i]:
(a, b, n_e - k).  Not found: nothing.  Ascending slot order, the first min(total, cap) slots of each range.  Offsets
modulo 2^32.  A graph without edges has no places.  The model is the checker of the kernels; nothing here is used by the
product."""
import bisect
from types import SimpleNamespace

import numpy as np

import locate_model as M

MASK = 0xffffffff


class Index(M.Index):
    def __init__(self, labels, edges):
        edges = [(int(u), int(v)) for u, v in edges]
        super().__init__(labels, edges)
        self.edges = sorted(set(edges))
        self.estart, self.elen = [], []
        at = 0
        for u, v in self.edges:
            self.estart.append(at)
            self.elen.append(len(self.labels[u]) + len(self.labels[v]))
            at += self.elen[-1] + 1
        assert at == self.N
        self._estart = np.array(self.estart, dtype=np.int64)
        self._elen = np.array(self.elen, dtype=np.int64)
        self._pairs = np.array(self.edges, dtype=np.int64).reshape(-1, 2)

    def search(self, pattern):
        """Rule 4 with its record -> namespace(count, pos, restarts, k, t, l, r, sl, sr)."""
        P = M.as_bytes(pattern)
        l, r, pos, count = 0, self.N, 0, 0
        rec = SimpleNamespace(count=0, pos=0, restarts=0, k=0, t=0, l=0, r=-1, sl=0, sr=-1)

        def done(found):
            rec.count, rec.pos = (count if found else 0), pos
            if found and count:
                rec.l, rec.r = l, r
            return rec

        for c in P:
            count, nl, nr = self.bs(c, l, r)
            if count:
                l, r = nl, nr
            else:
                n_sep, sl, sr = self.bs(M.SEP, l, r)
                if n_sep == 0:
                    return done(False)
                r1 = bisect.bisect_right(self._Bl, l)
                if r1 == 0 or r1 > len(self._El):
                    return done(False)
                nl, nr = self._Bl[r1 - 1], self._El[r1 - 1]
                if not (nl <= l and r <= nr):
                    return done(False)
                count, nl, nr = self.bs(c, nl, nr)
                if count == 0:
                    return done(False)
                if rec.restarts == 0:
                    rec.k, rec.sl, rec.sr = pos, sl, sr
                rec.t = pos
                rec.restarts += 1
                l, r = nl, nr
            pos += 1
        return done(True)

    def places(self, slots):
        """int64[len(slots), 4]: (a, b, n_e - 1 - (p - base), n_e) of the text positions p = SA[slots]."""
        p = self.SA[np.asarray(slots, dtype=np.int64)].astype(np.int64)
        e = np.searchsorted(self._estart, p, side="right") - 1
        pairs = self._pairs[e]
        return np.stack((pairs[:, 0], pairs[:, 1], (self._elen[e] - 1 - (p - (self._estart[e] + 1))) & MASK, self._elen[e]), axis=1)

    def occurrences(self, pattern, cap=None):
        """-> namespace(count, pos, restarts, k, t, end_total, start_total, ends, starts); ends / starts are
        int64[rows, 3] arrays of (src, dst, offset) of the first min(total, cap) slots (cap None: all)."""
        P = M.as_bytes(pattern)
        s = self.search(P)
        none = np.zeros((0, 3), dtype=np.int64)
        out = SimpleNamespace(count=s.count, pos=s.pos, restarts=s.restarts, k=s.k, t=s.t, end_total=0, start_total=0,
                              ends=none, starts=none)
        if s.count == 0:
            return out
        out.end_total = s.count
        out.start_total = s.sr - s.sl + 1 if s.restarts else s.count
        if not self.edges:
            return out
        n_end = out.end_total if cap is None else min(cap, out.end_total)
        n_start = out.start_total if cap is None else min(cap, out.start_total)
        out.ends = self.places(np.arange(s.l, s.l + n_end))[:, :3]
        if s.restarts == 0:
            out.starts = self.places(np.arange(s.l, s.l + n_start))[:, :3]
            out.starts[:, 2] = (out.starts[:, 2] - len(P) + 1) & MASK
        else:
            slots = np.arange(s.sl, s.sl + n_start)
            pl = self.places(slots)
            assert np.array_equal(pl[:, 2], pl[:, 3])          # every slot is the '#' of an edge: SA[i] = estart[e]
            out.starts = np.stack((pl[:, 0], pl[:, 1], (pl[:, 3] - s.k) & MASK), axis=1)
        return out
