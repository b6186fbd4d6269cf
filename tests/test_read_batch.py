"""The host state that ties the stages of the pattern index together (csrc/pindex.h, csrc/pindex_stage.h), through the C calls:
the reads of a seeds call stay what they were whatever is searched in between, a newer producing call makes exactly the
results below it stale, and a producing call that fails leaves its stage not done.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import random_msa  # noqa: E402

GAP = ord("-")
PARENT = dict(OCC=None, SEEDS=None, CHAINS="SEEDS", BYROW="CHAINS", ALIGN="CHAINS", CIGAR="ALIGN", GRAPH="CHAINS", GCIGAR="GRAPH",
              MAPQ="CHAINS")
# the calls that read a stage and produce none; ALIGN and BYROW have no such call
READERS = dict(OCC=["occurrences_fetch"], SEEDS=["seeds_fetch", "seeds_places", "seeds_msa", "seeds_rows"],
               CHAINS=["chains_fetch", "chain_strands", "chains_rows"], CIGAR=["cigar_fetch"], GRAPH=["graph_fetch"],
               GCIGAR=["graph_cigar_fetch"], MAPQ=["mapq_fetch", "mapq_strands"])
ALL = 0xffffffffffffffff
EDITED = (3, 8)                                 # the reads that carry a substitution


def below(stage):
    """The stages made from this one, directly or not."""
    return {s for s in PARENT if s != stage and stage in ancestors(s)}


def ancestors(stage):
    return [] if PARENT[stage] is None else [PARENT[stage]] + ancestors(PARENT[stage])


def concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off


class Calls:
    """The C calls on one index, by name.  A call returns (code, the arrays it filled) and remembers the sizes that the calls
    after it take their arrays' lengths from."""

    def __init__(self, pix, reads):
        from founderblockgraphs_amd import _lib
        self.L, self.h, self._lib = _lib.lib(), pix._h, _lib
        self.data, self.off = concat(reads)
        self.given, self.k = len(reads), 2 * len(reads)
        self.words = 1                          # 64-bit words of a row set: the MSA has 6 rows
        self.n = {}

    def u8(self, a): return a.ctypes.data_as(self._lib.u8p)
    def u32(self, a): return a.ctypes.data_as(self._lib.u32p)
    def u64(self, a): return a.ctypes.data_as(self._lib.u64p)

    def z(self, key, dtype, count=1):
        """count arrays with one entry more than the size remembered under key (an int: that many)"""
        size = self.n.get(key, 0) if isinstance(key, str) else key
        out = [np.zeros(size + 1, dtype=dtype) for _ in range(count)]
        return out if count > 1 else out[0]

    # ---- the searches that share nothing with the reads ----
    def locate(self, pats):
        data, off = concat(pats)
        count, pos = self.z(len(pats), np.uint64, 2)
        return self.L.fbg_pindex_locate(self.h, self.u8(data), self.u64(off), len(pats), self.u64(count), self.u64(pos)), [count, pos]

    def occurrences(self, pats):
        data, off = concat(pats)
        k = len(pats)
        count, pos, eo, so, et, st = self.z(k, np.uint64, 6)
        rs = self.z(k, np.uint32)
        rc = self.L.fbg_pindex_occurrences(self.h, self.u8(data), self.u64(off), k, 4, self.u64(count), self.u64(pos), self.u32(rs),
                                           self.u64(eo), self.u64(so), self.u64(et), self.u64(st), None)
        if rc == 0:
            self.n["oe"], self.n["os"] = int(eo[k]), int(so[k])
        return rc, [count, pos, rs, eo, so, et, st]

    def occurrences_fetch(self):
        a = self.z("oe", np.uint32, 3) + self.z("os", np.uint32, 3)
        return self.L.fbg_pindex_occurrences_fetch(self.h, *[self.u32(x) for x in a], None), a

    # ---- seeds(strands=True) ----
    def seeds(self):
        so = self.z(self.k, np.uint64)
        rc = self.L.fbg_pindex_seeds_strands(self.h, self.u8(self.data), self.u64(self.off), self.given, None, 1, 8, self.u64(so), None)
        if rc == 0:
            self.n["S"] = int(so[self.k])
        return rc, [so]

    def seeds_fetch(self):
        S = self.n["S"]
        q, ln, rs = self.z("S", np.uint32, 3)
        cnt, et, st, eo, so = self.z("S", np.uint64, 5)
        rc = self.L.fbg_pindex_seeds_fetch(self.h, self.u32(q), self.u32(ln), self.u64(cnt), self.u32(rs), self.u64(et), self.u64(st),
                                           self.u64(eo), self.u64(so), None)
        if rc == 0:
            self.n["se"], self.n["ss"] = int(eo[S]), int(so[S])
        return rc, [q, ln, rs, cnt, et, st, eo, so]

    def seeds_places(self):
        a = self.z("se", np.uint32, 3) + self.z("ss", np.uint32, 3)
        return self.L.fbg_pindex_seeds_places(self.h, *[self.u32(x) for x in a], None), a

    def seeds_msa(self):
        a = self.z("se", np.uint32, 2) + self.z("ss", np.uint32, 2)
        return self.L.fbg_pindex_seeds_msa(self.h, *[self.u32(x) for x in a], None), a

    def seeds_rows(self):
        a = self.z("ss", np.uint32, 2)
        return self.L.fbg_pindex_seeds_rows(self.h, *[self.u32(x) for x in a], None), a

    # ---- chains(rows, align, cigar, graph, graph_cigar, mapq) ----
    def chains(self):
        off, score = self.z(self.k, np.uint64), self.z(self.k, np.uint32)
        rc = self.L.fbg_pindex_chains(self.h, ALL, 4, self.u64(off), self.u32(score), None)
        if rc == 0:
            self.n["T"] = int(off[self.k])
        return rc, [off, score]

    def chains_by_row(self):
        off = self.z(self.k, np.uint64)
        score, row, nbest = self.z(self.k, np.uint32, 3)
        rc = self.L.fbg_pindex_chains_by_row(self.h, ALL, 4, self.u64(off), self.u32(score), self.u32(row), self.u32(nbest), None)
        if rc == 0:
            self.n["T"] = int(off[self.k])
        return rc, [off, score, row, nbest]

    def by_row_stats(self):
        a = self.z(0, np.uint64, 5)
        return self.L.fbg_pindex_chains_by_row_stats(self.h, *[self.u64(x) for x in a], None, None), a

    def chains_fetch(self):
        a = self.z("T", np.uint32, 2)
        return self.L.fbg_pindex_chains_fetch(self.h, self.u32(a[0]), self.u32(a[1]), None), a

    def chain_strands(self):
        strand, best, cnt = self.z(self.given, np.uint8), self.z(self.given, np.uint32), self.z(3, np.uint64)
        rc = self.L.fbg_pindex_chain_strands(self.h, self.u8(strand), self.u32(best), self.u64(cnt[0:]), self.u64(cnt[1:]),
                                             self.u64(cnt[2:]), None)
        return rc, [strand, best, cnt]

    def mapq(self):
        soff = self.z(self.k, np.uint64)
        sec, lo, hi = self.z(self.k, np.uint32, 3)
        mq = self.z(self.k, np.uint8)
        rc = self.L.fbg_pindex_chains_mapq(self.h, 0, self.u64(soff), self.u32(sec), self.u32(lo), self.u32(hi), self.u8(mq), None)
        if rc == 0:
            self.n["T2"] = int(soff[self.k])
        return rc, [soff, sec, lo, hi, mq]

    def mapq_fetch(self):
        a = self.z("T2", np.uint32, 2)
        return self.L.fbg_pindex_chains_mapq_fetch(self.h, self.u32(a[0]), self.u32(a[1]), None), a

    def mapq_strands(self):
        a = self.z(self.k, np.uint8)
        return self.L.fbg_pindex_mapq_strands(self.h, self.u8(a), None), [a]

    def mapq_stats(self):
        a = self.z(0, np.uint64, 5)
        return self.L.fbg_pindex_mapq_stats(self.h, *[self.u64(x) for x in a]), a

    def chains_rows(self):
        nr, fr = self.z(self.k, np.uint32, 2)
        bits = self.z(self.k * self.words, np.uint64)
        return self.L.fbg_pindex_chains_rows(self.h, self.u32(nr), self.u32(fr), self.u64(bits), None), [nr, fr, bits]

    def align(self):
        a = self.z(self.k, np.uint32, 4)
        return self.L.fbg_pindex_chains_align(self.h, 16, 0, *[self.u32(x) for x in a], None), a

    def _trace(self, call, key):
        nops, total = self.z(self.k, np.uint32), self.z(0, np.uint64)
        rc = call(self.h, self.u32(nops), self.u64(total), None)
        if rc == 0:
            self.n[key] = int(total[0])
        return rc, [nops, total]

    def _trace_fetch(self, call, key):
        off, ops = self.z(self.k, np.uint64), self.z(key, np.uint32)
        return call(self.h, self.u64(off), self.u32(ops)), [off, ops]

    def cigar(self): return self._trace(self.L.fbg_pindex_chains_cigar, "C")
    def cigar_fetch(self): return self._trace_fetch(self.L.fbg_pindex_chains_cigar_fetch, "C")

    def graph(self):
        a = self.z(self.k, np.uint32, 6)
        total = self.z(0, np.uint64)
        rc = self.L.fbg_pindex_chains_align_graph(self.h, 16, 0, None, *[self.u32(x) for x in a], self.u64(total), None)
        if rc == 0:
            self.n["P"] = int(total[0])
        return rc, a + [total]

    def graph_fetch(self): return self._trace_fetch(self.L.fbg_pindex_chains_align_graph_fetch, "P")
    def graph_cigar(self): return self._trace(self.L.fbg_pindex_chains_graph_cigar, "G")
    def graph_cigar_fetch(self): return self._trace_fetch(self.L.fbg_pindex_chains_graph_cigar_fetch, "G")

    def run(self, names, between=None):
        """The calls one after the other, between() between every two of them -> {name: arrays}; every call succeeds."""
        out = {}
        for i, name in enumerate(names):
            if between and i:
                between()
            rc, arrays = getattr(self, name)()
            assert rc == 0, name
            out[name] = [a.tolist() for a in arrays]
        return out


# the C calls of seeds(strands=True, msa=True, rows=True) and of chains() with every output, in the order api.py makes them
WITH_ROWS = ("seeds", "seeds_fetch", "seeds_places", "seeds_msa", "seeds_rows", "chains", "chains_fetch", "chain_strands", "mapq",
             "mapq_fetch", "mapq_strands", "chains_rows", "align", "cigar", "cigar_fetch", "graph", "graph_fetch", "graph_cigar",
             "graph_cigar_fetch")
# what an index without the row table supports of them
WITHOUT_ROWS = ("seeds", "seeds_fetch", "seeds_places", "seeds_msa", "chains", "chains_fetch", "chain_strands", "mapq", "mapq_fetch",
                "mapq_strands")


@pytest.fixture(scope="module")
def setup(engine):
    rng = np.random.default_rng(11)
    A = random_msa(rng, 6, 160, gap_p=0.03, similar=0.93)
    b = engine.minmax_dp(engine.elastic_f(A))
    rows = [bytes(r[r != GAP]) for r in A]
    reads = []
    for j in range(12):                                   # 12 reads of 30 .. 52 symbols, one of every row twice
        a = int(rng.integers(0, 60))
        reads.append(rows[j % 6][a:a + 30 + 2 * j])
    for j in EDITED:                                      # one substitution each, to a read that no row spells
        for c in b"ACGT":
            r = reads[j][:len(reads[j]) // 2] + bytes([c]) + reads[j][len(reads[j]) // 2 + 1:]
            if not any(r in row for row in rows):
                break
        assert not any(r in row for row in rows)
        reads[j] = r
    others = [rows[(j + 1) % 6][100 + j:100 + j + 9 + j] for j in range(7)]      # 7 patterns of 9 .. 15 symbols
    assert len(others) != len(reads) and sum(map(len, others)) != sum(map(len, reads))
    return A, b, reads, others


def build(engine, A, b, rows):
    engine.msa_load_host(np.ascontiguousarray(A, dtype=np.uint8))
    return engine.pattern_index_of_segmentation(b, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [True, False])
def test_other_searches_between_the_calls_change_nothing(engine, setup, rows):
    A, b, reads, others = setup
    names = WITH_ROWS if rows else WITHOUT_ROWS
    with build(engine, A, b, rows) as pix:
        c = Calls(pix, reads)
        want = c.run(names)
        assert len(want["chains_fetch"][0]) > 1 and max(want["mapq"][4]) > 0      # chains, and a mapping quality
        if rows:
            edits = want["align"][1]
            assert 0 in edits and all(1 <= edits[j] <= 3 for j in EDITED)       # the substitutions are aligned over
            assert want["cigar"][1][0] > 0 and want["graph"][6][0] > 0 and want["graph_cigar"][1][0] > 0
        searched = []

        def between():
            for call in (c.locate, c.occurrences):
                rc, arrays = call(others)
                assert rc == 0
                searched.append([a.tolist() for a in arrays])

        got = c.run(names, between)
        for name in names:
            assert got[name] == want[name], name
        assert len(searched) == 2 * (len(names) - 1)
        assert all(s == searched[k % 2] for k, s in enumerate(searched))          # and the reads do not disturb the searches


@pytest.mark.gpu
def test_a_producing_call_makes_exactly_the_results_below_it_stale(engine, setup):
    from founderblockgraphs_amd import _lib
    INVALID = _lib.FBG_ERR_INVALID
    A, b, reads, others = setup
    # every stage done: the chaining call is the one by row
    full = ("seeds", "seeds_fetch", "seeds_places", "chains_by_row", "mapq", "align", "cigar", "graph", "graph_cigar")
    produced = dict(seeds={"SEEDS"}, chains={"CHAINS"}, chains_by_row={"CHAINS", "BYROW"}, align={"ALIGN"}, graph={"GRAPH"})
    with build(engine, A, b, True) as pix:
        c = Calls(pix, reads)
        assert c.occurrences(others)[0] == 0

        def read_all(stages):
            out = {}
            for s in stages:
                for name in READERS.get(s, []):
                    rc, arrays = getattr(c, name)()
                    assert rc == 0, (s, name)
                    out[name] = [a.tolist() for a in arrays]
            if "BYROW" in stages:
                out["by_row_stats"] = [a.tolist() for a in c.by_row_stats()[1]]
            if "MAPQ" in stages:
                out["mapq_stats"] = [a.tolist() for a in c.mapq_stats()[1]]
            return out

        for producer, made in produced.items():
            c.run(full)
            stale = set().union(*[below(s) for s in made]) - made
            kept = set(PARENT) - stale - made
            before = read_all(kept)
            assert "occurrences_fetch" in before and ("BYROW" not in kept or any(x[0] for x in before["by_row_stats"]))
            rc, _ = getattr(c, producer)()
            assert rc == 0, producer
            for s in stale:
                for name in READERS.get(s, []):
                    assert getattr(c, name)()[0] == INVALID, (producer, s, name)
            # the calls that follow a stale stage and would produce the next one
            follow = dict(ALIGN="cigar", GRAPH="graph_cigar", CHAINS="mapq")
            for s, name in follow.items():
                if s in stale:
                    assert getattr(c, name)()[0] == INVALID, (producer, s, name)
            # a stale state reports zeros
            if "BYROW" in stale:
                assert not any(x[0] for x in c.by_row_stats()[1])
            if "MAPQ" in stale:
                assert not any(x[0] for x in c.mapq_stats()[1])
            assert read_all(kept) == before, producer
            read_all(made)                                 # what was produced is there


@pytest.mark.gpu
def test_a_failed_producing_call_leaves_its_stage_not_done(engine, setup):
    from founderblockgraphs_amd import _lib
    INVALID = _lib.FBG_ERR_INVALID
    A, b, reads, _ = setup
    with build(engine, A, b, True) as pix:
        c = Calls(pix, reads)
        c.run(("seeds", "chains", "chains_fetch"))
        score = c.z(c.k, np.uint32)
        assert c.L.fbg_pindex_chains(c.h, ALL, 4, None, c.u32(score), None) == INVALID      # chain_off is required
        assert c.chains_fetch()[0] == INVALID
