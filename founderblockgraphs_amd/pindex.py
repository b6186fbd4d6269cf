"""The pattern index of a founder graph (include/fbg_hip.h, fbg_pindex_*): PatternIndex and the results of its searches.

An index borrows the context of the Engine (api.py) that made it.  Every call goes through the C ABI of libfbg_hip.so;
nothing here computes, beyond picking the entries of a result that belong to a read's chosen strand.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _ignore, _sat64, _u8, _u32, _u64


def _concat(strings):
    """(uint8 bytes, uint64 offsets[len + 1]) of a list of str / bytes, or such a pair passed through."""
    if isinstance(strings, tuple) and len(strings) == 2 and isinstance(strings[1], np.ndarray):
        data = np.concatenate((np.ascontiguousarray(strings[0], dtype=np.uint8).ravel(), np.zeros(1, dtype=np.uint8)))
        return data, np.ascontiguousarray(strings[1], dtype=np.uint64)
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    data = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy()
    return data, off


def complement_table(spec=None):
    """The 256-byte complement table of seeds(strands=True) as a uint8 array.  spec: None for the default (A <-> T,
    C <-> G, a <-> t, c <-> g, every other byte itself); a mapping such as {"A": "T", "T": "A"} of single symbols (str,
    bytes or byte values), every byte not named mapping to itself; or the 256 bytes themselves.  The table is applied
    once per symbol and need not be an involution."""
    if spec is None:
        spec = {"A": "T", "T": "A", "C": "G", "G": "C", "a": "t", "t": "a", "c": "g", "g": "c"}
    if hasattr(spec, "items"):
        def sym(x):
            if isinstance(x, str):
                x = x.encode("latin-1")
            if isinstance(x, (bytes, bytearray)):
                if len(x) != 1:
                    raise ValueError(f"a complement maps single symbols, not {x!r}")
                return x[0]
            if not 0 <= int(x) <= 255:
                raise ValueError(f"a complement maps bytes, not {x!r}")
            return int(x)
        table = np.arange(256, dtype=np.uint8)
        for a, b in spec.items():
            table[sym(a)] = sym(b)
        return table
    if isinstance(spec, str):
        spec = spec.encode("latin-1")
    table = np.array(np.frombuffer(spec, dtype=np.uint8) if isinstance(spec, (bytes, bytearray)) else spec)
    if table.shape != (256,):
        raise ValueError(f"a complement table has 256 entries, not {table.size}")
    if table.dtype != np.uint8 and len(table) and (table.min() < 0 or table.max() > 255):
        raise ValueError("a complement table holds bytes")
    return np.ascontiguousarray(table, dtype=np.uint8)


class PatternIndex:
    """fbg_pindex: the founder_block_index of the reference built on the GPU (include/fbg_hip.h, 'pattern index').
    locate() returns what locate_patterns reports per pattern: the count of the last backward-search range (0: not
    found) and the number of symbols matched."""

    # what the last seeds() call left for chains(): its virtual reads, its seeds, and the given reads after strands=True
    _seed_reads = 0
    _seed_total = 0
    _seed_given = None
    _has_rows = False       # built by Engine.pattern_index_of_segmentation(rows=True)
    _h = None               # the library's handle, until close()

    def __init__(self, engine, labels, edges):
        self._eng = engine
        self._L = engine._L
        self._h = None
        data, loff = _concat(labels)
        n = len(loff) - 1
        e = np.asarray(list(edges) if not isinstance(edges, np.ndarray) else edges, dtype=np.int64).reshape(-1, 2)
        if len(e) and (e.min() < 0 or e.max() >= n):
            raise ValueError("edge endpoints must be node indices 0 .. len(labels) - 1")
        order = np.argsort(e[:, 0], kind="stable")
        dst = np.ascontiguousarray(e[order, 1], dtype=np.uint64)
        eoff = np.zeros(n + 1, dtype=np.uint64)
        if n:
            eoff[1:] = np.cumsum(np.bincount(e[:, 0], minlength=n)[:n], dtype=np.uint64)
        dst = np.concatenate((dst, np.zeros(1, dtype=np.uint64)))
        h = C.c_void_p()
        engine._chk(self._L.fbg_pindex_build(engine._h, _u8(data), _u64(loff), n, _u64(eoff), _u64(dst), C.byref(h)))
        self._h = h
        self.n_nodes = n
        self._label_len = np.diff(loff.astype(np.int64))

    @classmethod
    def _adopt(cls, engine, handle, nb):
        """An index the library built from a segmentation: label lengths and blocks come from the device."""
        self = cls.__new__(cls)
        self._eng, self._L, self._h = engine, engine._L, handle
        n = int(self._L.fbg_pindex_node_count(handle))
        self.n_nodes = n
        ll = np.zeros(max(n, 1), dtype=np.uint32)
        blk = np.zeros(max(n, 1), dtype=np.uint32)
        first = np.zeros(nb + 1, dtype=np.uint64)
        engine._chk(self._L.fbg_pindex_node_info(handle, _u32(ll), _u32(blk), _u64(first)))
        self._label_len = ll[:n].astype(np.int64)
        self.node_block = blk[:n].astype(np.int64)
        self.first_node = first
        return self

    def close(self):
        if self._h:
            self._L.fbg_pindex_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def text_length(self):
        """N + 1: the edge text including its sentinel."""
        return int(self._L.fbg_pindex_text_length(self._h))

    def locate(self, patterns):
        """-> (count, pos), uint64 arrays with one entry per pattern (a list of str / bytes, or a pair (uint8 data,
        uint64 offsets[k + 1]))."""
        data, off = _concat(patterns)
        k = len(off) - 1
        count = np.zeros(max(k, 1), dtype=np.uint64)
        pos = np.zeros(max(k, 1), dtype=np.uint64)
        self._eng._chk(self._L.fbg_pindex_locate(self._h, _u8(data), _u64(off), k, _u64(count), _u64(pos)))
        return count[:k], pos[:k]

    # ---- counters of the last calls: one entry point each, and the names of what it fills ---------------------------
    MSA_STATS = ("map_bytes", "gapped_nodes", "sample_columns")
    ROWS_STATS = ("rows", "table_bytes", "words_per_set", "places_unsupported", "chains_unsupported")
    ALIGN_STATS = ("aligned", "unsupported", "too_long", "too_wide", "cells", "max_read", "table_bytes")
    CIGAR_STATS = ("paths", "ops", "columns", "history_bytes", "batches")
    GRAPH_STATS = ("aligned", "not_selected", "too_long", "too_wide", "cells", "nodes", "merges", "path_nodes", "table_bytes", "batches")
    MAPQ_STATS = ("reads_with_second", "anchors_kept", "anchors_excluded", "mapq0", "mapq60")
    BY_ROW_STATS = ("reads_lds", "reads_device", "reads_too_many", "reads_no_row", "anchors_kept", "lds_max", "max_places")
    CHAIN_STATS = ("anchors", "reads_small", "reads_wave", "reads_spill", "small_max", "lds_max")

    def _stats(self, call, names):
        v = [C.c_uint64(0) for _ in names]
        self._eng._chk(call(self._h, *[C.byref(x) for x in v]))
        return dict(zip(names, (x.value for x in v)))

    def msa_stats(self):
        """{map_bytes, gapped_nodes, sample_columns} of the MSA coordinate table (fbg_pindex_msa_stats; an index built
        by Engine.pattern_index_of_segmentation only)."""
        return self._stats(self._L.fbg_pindex_msa_stats, self.MSA_STATS)

    def rows_stats(self):
        """{rows, table_bytes, words_per_set, places_unsupported, chains_unsupported} of the row table and of the last
        seeds(rows=True) / chains(rows=True) (fbg_pindex_rows_stats; an index built with rows=True only)."""
        return self._stats(self._L.fbg_pindex_rows_stats, self.ROWS_STATS)

    def align_stats(self):
        """{aligned, unsupported, too_long, too_wide, cells, max_read, table_bytes} of the last chains(align=True)
        (fbg_pindex_align_stats; an index built with rows=True only): cells is the sum of read length times window length
        over the aligned reads, max_read the longest read that is aligned, table_bytes the prefix table's."""
        return self._stats(self._L.fbg_pindex_align_stats, self.ALIGN_STATS)

    def cigar_stats(self):
        """{paths, ops, columns, history_bytes, batches} of the last chains(align=True, cigar=True)
        (fbg_pindex_cigar_stats; an index built with rows=True only): the reads traced, their runs, the sum of
        t_end - t_start, the bytes of column history that went to device memory (reads of more than 256 symbols) and
        the batches those reads were worked off in."""
        return self._stats(self._L.fbg_pindex_cigar_stats, self.CIGAR_STATS)

    def graph_align_stats(self):
        """{aligned, not_selected, too_long, too_wide, cells, nodes, merges, path_nodes, table_bytes, batches} of the last
        chains(graph=True) (fbg_pindex_align_graph_stats; an index built with rows=True only): cells is the sum of read
        length times the label symbols of the window's nodes over the aligned reads, nodes the sum of those nodes, merges
        the predecessor columns read on entering them, table_bytes the predecessor lists' and the block table's, batches
        the batches option graph_batch_kib cut the reads into."""
        return self._stats(self._L.fbg_pindex_align_graph_stats, self.GRAPH_STATS)

    def graph_cigar_stats(self):
        """{paths, ops, columns, history_bytes, batches} of the last chains(graph=True, graph_cigar=True)
        (fbg_pindex_graph_cigar_stats; an index built with rows=True only), with the meaning of cigar_stats(): the reads
        traced, their runs, the sum of the lengths of the stretches of the graph they lie on, the bytes of column history
        that went to device memory and the batches those reads were worked off in."""
        return self._stats(self._L.fbg_pindex_graph_cigar_stats, self.CIGAR_STATS)

    def mapq_stats(self):
        """{reads_with_second, anchors_kept, anchors_excluded, mapq0, mapq60} of the last chains(mapq=True), over the reads
        with a non-empty chain: see fbg_pindex_mapq_stats."""
        return self._stats(self._L.fbg_pindex_mapq_stats, self.MAPQ_STATS)

    def by_row_stats(self):
        """{reads_lds, reads_device, reads_too_many, reads_no_row, anchors_kept, lds_max, max_places} of the last
        chains(by_row=True): see fbg_pindex_chains_by_row_stats."""
        return self._stats(self._L.fbg_pindex_chains_by_row_stats, self.BY_ROW_STATS)

    def chain_stats(self):
        """{anchors, reads_small, reads_wave, reads_spill, small_max, lds_max}: see fbg_pindex_chain_stats."""
        return self._stats(self._L.fbg_pindex_chain_stats, self.CHAIN_STATS)

    # ---- searches ---------------------------------------------------------------------------------------------------
    def _msa_coords(self, call, ne, ns):
        """The four arrays of fbg_pindex_occurrences_msa / fbg_pindex_seeds_msa for ne ends and ns starts, and device ms."""
        out = [np.zeros(max(k, 1), dtype=np.uint32) for k in (ne, ne, ns, ns)]
        ms = C.c_double(0)
        self._eng._chk(call(self._h, *[_u32(a) for a in out], C.byref(ms)))
        return [a[:k] for a, k in zip(out, (ne, ne, ns, ns))], ms.value

    def _occurrences(self, fetch, msa_call, per_item, eoff, soff, search_ms, fetch_ms=0.0):
        """The places behind the offsets of a search (`fetch`: fbg_pindex_occurrences_fetch or fbg_pindex_seeds_places), their
        MSA cells if msa_call is given, and with per_item (count, pos, restarts, end_total, start_total) the Occurrences."""
        ne, ns = int(eoff[-1]), int(soff[-1])
        ends = [np.zeros(max(ne, 1), dtype=np.uint32) for _ in range(3)]
        starts = [np.zeros(max(ns, 1), dtype=np.uint32) for _ in range(3)]
        ms = C.c_double(0)
        self._eng._chk(fetch(self._h, *[_u32(a) for a in ends + starts], C.byref(ms)))
        coords, msa_ms = self._msa_coords(msa_call, ne, ns) if msa_call is not None else (None, 0.0)
        return Occurrences(self._label_len, *per_item, eoff, soff, [a[:ne] for a in ends], [a[:ns] for a in starts], search_ms,
                           fetch_ms + ms.value, coords, msa_ms)

    def occurrences(self, patterns, max_per_pattern=64, msa=False):
        """The search of locate() plus the places where each found pattern ends and starts, at most max_per_pattern
        of each per pattern (fbg_pindex_occurrences and fbg_pindex_occurrences_fetch) -> Occurrences.  msa=True (an
        index built by Engine.pattern_index_of_segmentation only): also the MSA row and column of every place
        (fbg_pindex_occurrences_msa)."""
        if max_per_pattern < 0:
            raise ValueError("max_per_pattern must be 0 or more")
        data, off = _concat(patterns)
        k = len(off) - 1
        count, pos, et, st = (np.zeros(max(k, 1), dtype=np.uint64) for _ in range(4))
        rs = np.zeros(max(k, 1), dtype=np.uint32)
        eoff, soff = np.zeros(k + 1, dtype=np.uint64), np.zeros(k + 1, dtype=np.uint64)
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_occurrences(self._h, _u8(data), _u64(off), k, int(max_per_pattern), _u64(count), _u64(pos),
                                                      _u32(rs), _u64(eoff), _u64(soff), _u64(et), _u64(st), C.byref(ms)))
        return self._occurrences(self._L.fbg_pindex_occurrences_fetch, self._L.fbg_pindex_occurrences_msa if msa else None,
                                 (count[:k], pos[:k], rs[:k], et[:k], st[:k]), eoff, soff, ms.value)

    def seeds(self, patterns, min_length=1, max_per_seed=0, msa=False, chain=False, band=None, min_score=0, strands=False,
              complement=None, rows=False, by_row=False, mapq=False, mapq_margin=0):
        """Every read cut greedily into the maximal pieces the search accepts (fbg_pindex_seeds, _fetch and _places):
        seeds of at least min_length symbols, each with what occurrences() reports for that substring, at most
        max_per_seed places per seed and list -> Seeds.  msa=True: as for occurrences() (fbg_pindex_seeds_msa).
        chain=True: also chains(band, min_score) of these seeds, as Seeds.chains.  strands=True: every read is searched
        as given and as its reverse complement under complement_table(complement), made on the device
        (fbg_pindex_seeds_strands): the Seeds then cover 2k virtual reads, the k given ones and then their k reverse
        complements, and chains() also picks a strand per read.  rows=True (an index built with rows=True only): also,
        per start place, the number of MSA rows that carry it and the smallest of them (fbg_pindex_seeds_rows), as
        Seeds.start_n_rows / Seeds.start_first_row; with chain=True the chains get their row sets too.  by_row=True
        (with chain=True): the chains are those of chains(by_row=True).  mapq=True (with chain=True): the chains carry
        their second-best chain and mapping quality, as chains(mapq=True, mapq_margin=mapq_margin)."""
        if mapq and not chain:
            raise ValueError("mapq=True needs chain=True")
        if min_length < 1:
            raise ValueError("min_length must be 1 or more")
        if max_per_seed < 0:
            raise ValueError("max_per_seed must be 0 or more")
        data, off = _concat(patterns)
        given = len(off) - 1
        k = 2 * given if strands else given
        seed_off = np.zeros(k + 1, dtype=np.uint64)
        ms1, ms2 = C.c_double(0), C.c_double(0)
        if strands:
            table = complement_table(complement)
            self._eng._chk(self._L.fbg_pindex_seeds_strands(self._h, _u8(data), _u64(off), given, _u8(table), int(min_length),
                                                            int(max_per_seed), _u64(seed_off), C.byref(ms1)))
        else:
            if complement is not None:
                raise ValueError("complement needs strands=True")
            self._eng._chk(self._L.fbg_pindex_seeds(self._h, _u8(data), _u64(off), k, int(min_length), int(max_per_seed),
                                                    _u64(seed_off), C.byref(ms1)))
        n = int(seed_off[k])
        q, ln, rs = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        count, et, st = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        eoff, soff = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        self._eng._chk(self._L.fbg_pindex_seeds_fetch(self._h, _u32(q), _u32(ln), _u64(count), _u32(rs), _u64(et), _u64(st),
                                                      _u64(eoff), _u64(soff), C.byref(ms2)))
        occ = self._occurrences(self._L.fbg_pindex_seeds_places, self._L.fbg_pindex_seeds_msa if msa else None,
                                (count[:n], ln[:n].astype(np.uint64), rs[:n], et[:n], st[:n]), eoff, soff, ms1.value, ms2.value)
        self._seed_reads, self._seed_total, self._seed_given = k, n, given if strands else None
        out = Seeds(seed_off, q[:n], ln[:n], occ, np.diff(off.astype(np.int64)), strands)
        if rows:
            ns = int(soff[n])
            nr, fr = np.zeros(max(ns, 1), dtype=np.uint32), np.zeros(max(ns, 1), dtype=np.uint32)
            ms5 = C.c_double(0)
            self._eng._chk(self._L.fbg_pindex_seeds_rows(self._h, _u32(nr), _u32(fr), C.byref(ms5)))
            out.start_n_rows, out.start_first_row, out.rows_ms = nr[:ns], fr[:ns], ms5.value
        if chain:
            out.chains = self.chains(band=band, min_score=min_score, rows=rows, by_row=by_row, mapq=mapq, mapq_margin=mapq_margin)
        return out

    def chains(self, band=None, min_score=0, rows=False, align=False, pad=16, max_window=0, cigar=False, by_row=False,
               graph=False, graph_pad=16, max_cells=0, select=None, graph_cigar=False, mapq=False, mapq_margin=0, pairs=None,
               adopt_pairs=False, pair_align=False, pair_max_edits=0xffffffff, pair_max_window=0, pair_select=None):
        """Co-linear chaining of the seeds of the last seeds() call (fbg_pindex_chains and _fetch; an index built by
        Engine.pattern_index_of_segmentation only) -> Chains, whose docstring describes every field named here.

        band, min_score: per read the best-scoring selection of its seeds' start places that ascends in the read and in the
        MSA columns, the surplus of columns over read symbols between two neighbours at most band (None: unbounded); chains
        scoring below min_score come out empty.

        After seeds(strands=True) the chains cover the 2k virtual reads and the strand of every given read is picked from
        their scores on the device (fbg_pindex_chain_strands).

        rows=True (an index built with rows=True only): also the MSA rows that carry every anchor of a read's chain
        (fbg_pindex_chains_rows), as Chains.n_rows, .first_row and .row_set(k).

        align=True, pad, max_window (an index built with rows=True only): also the edit distance of every read to the
        smallest row that carries its chain, in a window of that row's text pad symbols around the chain's diagonals
        (fbg_pindex_chains_align), as Chains.align_row, .edits, .t_start and .t_end; a read whose window is longer than
        max_window (0: no limit) is skipped.  After seeds(strands=True) also Chains.best_edits.

        cigar=True (with align=True): also the alignment path of every aligned read (fbg_pindex_chains_cigar and _fetch),
        as Chains.cigar_off and .cigar_ops, read with .cigar(k) and .cigar_runs(k).

        by_row=True (an index built with rows=True only): chain along one MSA row instead (fbg_pindex_chains_by_row): per
        read the row whose supported anchors chain best, as Chains.chain_row and .n_best_rows, and that row's chain;
        strands, rows=, align= and cigar= then work on these chains, and every non-empty one has a row to be aligned against.

        graph=True, graph_pad, max_cells, select (an index built with rows=True only): also the edit distance of every read
        to a path of the graph through the blocks around its chain, graph_pad symbols beyond the anchors, and that path
        (fbg_pindex_chains_align_graph and _fetch), as Chains.graph_edits, .graph_start, .graph_end, .graph_path_off,
        .graph_path_nodes and .graph_path(k); a read whose window takes more than max_cells cells (0: no limit) is skipped,
        and so is one whose entry of select (one per read of the last seeds() call, None: all) is zero.  After
        seeds(strands=True) also Chains.best_graph_edits.

        graph_cigar=True (with graph=True): also the alignment path of every such read against the stretch of the graph its
        path spells (fbg_pindex_chains_graph_cigar and _fetch), as Chains.graph_cigar_off and .graph_cigar_ops, read with
        .graph_cigar(k) and .graph_cigar_runs(k).

        mapq=True, mapq_margin: also the second-best chain of every read, chained on the anchors outside the MSA columns of
        its chain widened by mapq_margin columns on either side (chains through other alleles in the same columns are the
        same locus), and the mapping quality 60 * (score - min(second, score)) // read length (fbg_pindex_chains_mapq and
        _fetch), as Chains.second_score, .second_lo, .second_hi, .mapq, .second_off, .second_place, .second_seed and
        .second(k); after seeds(strands=True) also Chains.mapq_stranded, where the other strand's score competes too
        (fbg_pindex_mapq_strands), and Chains.best_mapq.  A read matched in one piece has no seed at a shorter copy elsewhere
        and gets second_score 0.

        pairs=(min_insert, max_insert) (after seeds(strands=True) on an even number of reads, mates interleaved): also, per
        virtual read, a rescue chain on the start places inside the insert window that its partner's chain opens, and per
        pair the best valid combination of a chain and a rescue chain on opposite strands (fbg_pindex_chains_pairs), as
        Chains.pair_which, .pair_score, .pair_lo, .pair_hi, .rescue_off, .rescue_score, .rescue_lo, .rescue_hi,
        .rescue_place, .rescue_seed, .rescue(v), .pair(p), .pair_stats and .pairs_ms.

        adopt_pairs=True: the chosen chains replace the chains of their reads and the twins of those reads get the empty
        chain, right after the chaining call: chain_off, score, anchor_place, anchor_seed, the strands and every field of
        rows=, align=, cigar=, graph=, graph_cigar= and mapq= then describe the adopted chains.

        pair_align=True (with pairs=, an index built with rows=True only): after the pairing call, and after its adoption,
        every virtual read without a chain whose partner has one is aligned in the insert window on the row of the partner's
        chain, the insert counted in symbols of that row, and every pair is decided from these alignments
        (fbg_pindex_pairs_align), as Chains.mate_row, .mate_edits, .mate_start, .mate_end, .mate_insert, .mate_which,
        .mate_score, .mate_lo, .mate_hi, .mate_stats and .mate_ms.

        pair_max_edits: the most edits an accepted alignment may have.  pair_max_window (0: no limit): a longer window is
        skipped.  pair_select (one entry per virtual read, None: the reads without a chain): the reads to align where their
        partner has a chain."""
        if adopt_pairs and pairs is None:
            raise ValueError("adopt_pairs=True needs pairs=(min_insert, max_insert)")
        if pairs is not None:
            if self._seed_given is None:
                raise ValueError("pairs= needs seeds(strands=True)")
            lo_ins, hi_ins = (int(x) for x in pairs)
            if not 0 <= lo_ins <= hi_ins:
                raise ValueError("pairs=(min_insert, max_insert) with 0 <= min_insert <= max_insert")
            pairs = (lo_ins, hi_ins)
        if pair_align:
            if pairs is None:
                raise ValueError("pair_align=True needs pairs=(min_insert, max_insert)")
            if not self._has_rows:
                raise ValueError("pair_align=True needs an index built with rows=True")
            if not 0 <= int(pair_max_edits) <= 0xffffffff or pair_max_window < 0:
                raise ValueError("pair_max_edits must fit 32 bits and pair_max_window must be 0 or more")
        if mapq_margin < 0:
            raise ValueError("mapq_margin must be 0 or more")
        if cigar and not align:
            raise ValueError("cigar=True needs align=True")
        if graph_cigar and not graph:
            raise ValueError("graph_cigar=True needs graph=True")
        if band is not None and band < 0:
            raise ValueError("band must be 0 or more, or None")
        if min_score < 0:
            raise ValueError("min_score must be 0 or more")
        if pad < 0 or max_window < 0:
            raise ValueError("pad and max_window must be 0 or more")
        if graph_pad < 0 or max_cells < 0:
            raise ValueError("graph_pad and max_cells must be 0 or more")
        out = self._chain(band, min_score, by_row)
        if pairs is not None:
            self._pairs(out, pairs, adopt_pairs)
        if pair_align:
            self._pair_align(out, pairs, pair_max_edits, pair_max_window, pair_select)
        self._chains_fetch(out)
        if self._seed_given is not None:
            self._chain_strands(out)
        if mapq:
            self._mapq(out, mapq_margin)
        if rows:
            self._chain_rows(out)
        if align:
            self._align(out, pad, max_window)
        if cigar:
            out.cigar_off, out.cigar_ops, out.cigar_ms = self._runs(self._L.fbg_pindex_chains_cigar, self._L.fbg_pindex_chains_cigar_fetch)
        if graph:
            self._graph(out, graph_pad, max_cells, select)
        if graph_cigar:
            out.graph_cigar_off, out.graph_cigar_ops, out.graph_cigar_ms = self._runs(self._L.fbg_pindex_chains_graph_cigar,
                                                                                      self._L.fbg_pindex_chains_graph_cigar_fetch)
        return out

    # ---- the stages of chains(): each allocates, calls and sets its fields of the Chains; k is the number of virtual reads ----
    def _chain(self, band, min_score, by_row):
        k = self._seed_reads
        chain_off = np.zeros(k + 1, dtype=np.uint64)
        score = np.zeros(max(k, 1), dtype=np.uint32)
        ms = C.c_double(0)
        b = 0xffffffffffffffff if band is None else _sat64(band)
        if by_row:
            crow, nbest = np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint32)
            self._eng._chk(self._L.fbg_pindex_chains_by_row(self._h, b, _sat64(min_score), _u64(chain_off), _u32(score), _u32(crow),
                                                            _u32(nbest), C.byref(ms)))
        else:
            self._eng._chk(self._L.fbg_pindex_chains(self._h, b, _sat64(min_score), _u64(chain_off), _u32(score), C.byref(ms)))
        out = Chains(chain_off, score[:k], None, None, ms.value, 0.0)
        if by_row:
            out.chain_row, out.n_best_rows, out.by_row = crow[:k], nbest[:k], True
        return out

    def _pairs(self, out, insert, adopt):
        k = self._seed_reads
        npairs, nseeds = k // 4, self._seed_total
        pw = np.zeros(max(npairs, 1), dtype=np.uint8)
        psc, plo, phi = (np.zeros(max(npairs, 1), dtype=np.uint32) for _ in range(3))
        roff = np.zeros(k + 1, dtype=np.uint64)
        rsc, rlo, rhi = (np.zeros(max(k, 1), dtype=np.uint32) for _ in range(3))
        rplace, rseed = (np.zeros(max(nseeds, 1), dtype=np.uint32) for _ in range(2))
        aoff, asc = np.zeros(k + 1, dtype=np.uint64), np.zeros(max(k, 1), dtype=np.uint32)
        pstats = np.zeros(8, dtype=np.uint64)
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_pairs(self._h, insert[0], _sat64(insert[1]), _u8(pw), _u32(psc), _u32(plo), _u32(phi),
                                                       _u64(roff), _u32(rsc), _u32(rlo), _u32(rhi), _u32(rplace), _u32(rseed),
                                                       _u64(aoff) if adopt else None, _u32(asc) if adopt else None, _u64(pstats),
                                                       C.byref(ms)))
        if adopt:
            out.chain_off, out.score = aoff, asc[:k]
        t = int(roff[k])
        out.pair_which, out.pair_score, out.pair_lo, out.pair_hi = pw[:npairs], psc[:npairs], plo[:npairs], phi[:npairs]
        out.rescue_off, out.rescue_score, out.rescue_lo, out.rescue_hi = roff, rsc[:k], rlo[:k], rhi[:k]
        out.rescue_place, out.rescue_seed = rplace[:t], rseed[:t]
        out.pair_stats, out.pairs_ms = dict(zip(Chains.PAIR_STATS, (int(x) for x in pstats))), ms.value

    def _selection(self, select, message):
        """select= / pair_select= as the uint8 array the library takes, one entry per read of the last seeds() call."""
        if select is None:
            return None
        sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
        if sel.shape != (self._seed_reads,):
            raise ValueError(message)
        return sel

    def _pair_align(self, out, insert, max_edits, max_window, select):
        k, npairs = self._seed_reads, self._seed_reads // 4
        sel = self._selection(select, "pair_select takes one entry per virtual read of the last seeds() call")
        per_read = [np.zeros(max(k, 1), dtype=np.uint32) for _ in range(5)]
        mw = np.zeros(max(npairs, 1), dtype=np.uint8)
        per_pair = [np.zeros(max(npairs, 1), dtype=np.uint32) for _ in range(3)]
        mstats = np.zeros(10, dtype=np.uint64)
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_pairs_align(self._h, insert[0], _sat64(insert[1]), int(max_edits), _sat64(max_window),
                                                      None if sel is None else _u8(sel), *[_u32(a) for a in per_read], _u8(mw),
                                                      *[_u32(a) for a in per_pair], _u64(mstats), C.byref(ms)))
        out.mate_row, out.mate_edits, out.mate_start, out.mate_end, out.mate_insert = (a[:k] for a in per_read)
        out.mate_which = mw[:npairs]
        out.mate_score, out.mate_lo, out.mate_hi = (a[:npairs] for a in per_pair)
        out.mate_stats, out.mate_ms = dict(zip(Chains.MATE_STATS, (int(x) for x in mstats))), ms.value

    def _chains_fetch(self, out):
        t = int(out.chain_off[self._seed_reads])
        place, seed = np.zeros(max(t, 1), dtype=np.uint32), np.zeros(max(t, 1), dtype=np.uint32)
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_fetch(self._h, _u32(place), _u32(seed), C.byref(ms)))
        out.anchor_place, out.anchor_seed, out.fetch_ms = place[:t], seed[:t], ms.value

    def _chain_strands(self, out):
        given = self._seed_given
        strand, best = np.zeros(max(given, 1), dtype=np.uint8), np.zeros(max(given, 1), dtype=np.uint32)
        cnt = [C.c_uint64(0) for _ in range(3)]
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chain_strands(self._h, _u8(strand), _u32(best), *[C.byref(x) for x in cnt], C.byref(ms)))
        out.strand, out.best_score = strand[:given], best[:given]
        out.strand_counts = dict(zip(("forward", "reverse", "none"), (x.value for x in cnt)))
        out.strand_ms = ms.value

    def _of_chosen_strand(self, out, per_read, none):
        """Per given read the entry of per_read (one per virtual read) on the strand that out.strand picked, `none` without one."""
        given = self._seed_given
        pick = np.where(out.strand[:given] == 1, given, 0) + np.arange(given)
        return np.where(out.strand[:given] == _lib.STRAND_NONE, none, per_read[pick] if given else per_read[:0]).astype(none.dtype)

    def _mapq(self, out, margin):
        k = self._seed_reads
        soff = np.zeros(k + 1, dtype=np.uint64)
        sec, slo, shi = (np.zeros(max(k, 1), dtype=np.uint32) for _ in range(3))
        mq = np.zeros(max(k, 1), dtype=np.uint8)
        ms, fetch_ms = C.c_double(0), C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_mapq(self._h, _sat64(margin), _u64(soff), _u32(sec), _u32(slo), _u32(shi), _u8(mq),
                                                      C.byref(ms)))
        t = int(soff[k])
        splace, sseed = np.zeros(max(t, 1), dtype=np.uint32), np.zeros(max(t, 1), dtype=np.uint32)
        self._eng._chk(self._L.fbg_pindex_chains_mapq_fetch(self._h, _u32(splace), _u32(sseed), C.byref(fetch_ms)))
        out.second_off, out.second_score, out.second_lo, out.second_hi, out.mapq = soff, sec[:k], slo[:k], shi[:k], mq[:k]
        out.second_place, out.second_seed, out.mapq_ms = splace[:t], sseed[:t], ms.value
        if self._seed_given is not None:
            smq = np.zeros(max(k, 1), dtype=np.uint8)
            self._eng._chk(self._L.fbg_pindex_mapq_strands(self._h, _u8(smq), None))
            out.mapq_stranded = smq[:k]
            out.best_mapq = self._of_chosen_strand(out, out.mapq_stranded, np.uint8(0))

    def _chain_rows(self, out):
        k = self._seed_reads
        words = self.rows_stats()["words_per_set"]
        nr, fr = np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint32)
        bits = np.zeros(max(k * words, 1), dtype=np.uint64)
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_rows(self._h, _u32(nr), _u32(fr), _u64(bits), C.byref(ms)))
        out.n_rows, out.first_row, out.rows_ms = nr[:k], fr[:k], ms.value
        out.row_bits = bits[:k * words].reshape(k, words)

    def _align(self, out, pad, max_window):
        k = self._seed_reads
        arr = [np.zeros(max(k, 1), dtype=np.uint32) for _ in range(4)]
        ms = C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_align(self._h, _sat64(pad), _sat64(max_window), *[_u32(a) for a in arr], C.byref(ms)))
        out.align_row, out.edits, out.t_start, out.t_end = (a[:k] for a in arr)
        out.align_ms = ms.value
        if self._seed_given is not None:
            out.best_edits = self._of_chosen_strand(out, out.edits, np.uint32(_lib.ALIGN_NONE))

    def _runs(self, trace, fetch):
        """The CIGAR runs of an alignment stage (fbg_pindex_chains_cigar or _graph_cigar, and its _fetch) -> (off, ops, ms)."""
        coff = np.zeros(self._seed_reads + 1, dtype=np.uint64)
        total, ms = C.c_uint64(0), C.c_double(0)
        self._eng._chk(trace(self._h, None, C.byref(total), C.byref(ms)))
        ops = np.zeros(max(total.value, 1), dtype=np.uint32)
        self._eng._chk(fetch(self._h, _u64(coff), _u32(ops)))
        return coff, ops[:total.value], ms.value

    def _graph(self, out, pad, max_cells, select):
        k = self._seed_reads
        sel = self._selection(select, "select takes one entry per read of the last seeds() call")
        arr = [np.zeros(max(k, 1), dtype=np.uint32) for _ in range(6)]
        total, ms = C.c_uint64(0), C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_chains_align_graph(self._h, _sat64(pad), _sat64(max_cells), None if sel is None else _u8(sel),
                                                             *[_u32(a) for a in arr], C.byref(total), C.byref(ms)))
        poff = np.zeros(k + 1, dtype=np.uint64)
        nodes = np.zeros(max(total.value, 1), dtype=np.uint32)
        self._eng._chk(self._L.fbg_pindex_chains_align_graph_fetch(self._h, _u64(poff), _u32(nodes)))
        out.graph_edits = arr[0][:k]
        out.graph_start = np.stack((arr[1][:k], arr[2][:k]), axis=1)
        out.graph_end = np.stack((arr[3][:k], arr[4][:k]), axis=1)
        out.graph_path_off, out.graph_path_nodes, out.graph_ms = poff, nodes[:total.value], ms.value
        if self._seed_given is not None:
            out.best_graph_edits = self._of_chosen_strand(out, out.graph_edits, np.uint32(_lib.ALIGN_NONE))

    def download(self):
        """-> (text with the sentinel, SA, B positions, E positions)."""
        N1 = self.text_length()
        nb, ne = C.c_uint64(0), C.c_uint64(0)
        self._eng._chk(self._L.fbg_pindex_download(self._h, None, None, None, None, C.byref(nb), C.byref(ne)))
        T = np.empty(N1, dtype=np.uint8)
        sa = np.empty(N1, dtype=np.uint32)
        B = np.empty(max(nb.value, 1), dtype=np.uint32)
        E = np.empty(max(ne.value, 1), dtype=np.uint32)
        self._eng._chk(self._L.fbg_pindex_download(self._h, _u8(T), _u32(sa), _u32(B), _u32(E), C.byref(nb), C.byref(ne)))
        return T, sa, B[:nb.value], E[:ne.value]

    def stats(self):
        """{index_bytes, build_ms, search_ms, occ_lines}: see fbg_pindex_stats."""
        ib, ol = C.c_uint64(0), C.c_uint64(0)
        bm, sm = C.c_double(0), C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_stats(self._h, C.byref(ib), C.byref(bm), C.byref(sm), C.byref(ol)))
        return {"index_bytes": ib.value, "build_ms": bm.value, "search_ms": sm.value, "occ_lines": ol.value}

    def validate(self, blocks, ignorechars=""):
        """Semi-repeat-free check of the index's graph (fbg_pindex_validate): `blocks` holds one block id per node
        (0 .. 2^32 - 1; only equality decides a node's status, bad_cuts reads them as block indices from 0).  Nodes
        whose label holds a byte of `ignorechars` are skipped.  -> Validation."""
        n = self.n_nodes
        blk = np.asarray(blocks).ravel()
        if len(blk) != n:
            raise ValueError(f"blocks has {len(blk)} entries for {n} nodes")
        if n and (blk.min() < 0 or blk.max() > 0xffffffff):
            raise ValueError("block ids must lie in 0 .. 2^32 - 1")
        blk32 = np.ascontiguousarray(blk, dtype=np.uint32)
        ig, il = _ignore(ignorechars)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        wn = np.zeros(max(n, 1), dtype=np.uint64)
        wo = np.zeros(max(n, 1), dtype=np.uint64)
        bad, ms = C.c_uint64(0), C.c_double(0)
        self._eng._chk(self._L.fbg_pindex_validate(self._h, _u32(blk32), _u8(ig), il, _u8(status), _u64(wn), _u64(wo), C.byref(bad),
                                                   C.byref(ms)))
        slots, waves, tb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._eng._chk(self._L.fbg_pindex_validate_stats(self._h, C.byref(slots), C.byref(waves), C.byref(tb)))
        return Validation(status[:n], wn[:n], wo[:n], blk.astype(np.int64), ms.value, slots.value, waves.value)


class Occurrences:
    """Result of PatternIndex.occurrences (include/fbg_hip.h, fbg_pindex_occurrences), one entry per pattern:
      count, pos               what locate() returns
      restarts                 uint32, restarts of the search that went on
      end_total, start_total   places the search found (0 for a pattern that was not found)
      end_off, start_off       uint64[k + 1], CSR offsets of the reported (capped) lists
    and one entry per reported place, in ascending SA slot order within a pattern:
      end_src, end_dst, end_offset        the edge (node indices) and the index into label(src) + label(dst) of the
                                          match's last symbol
      start_src, start_dst, start_offset  the same for its first symbol
    and, asked for with msa=True (None otherwise), aligned with them:
      end_row, end_col, start_row, start_col   uint32: the MSA cell of that symbol in the representative row of its node
                                          (one witness row per place; 0xffffffff in both for an offset outside the edge)
    search_ms, fetch_ms: device time of the two calls; msa_ms: of the MSA coordinates.  A (start, end) pair of a pattern
    with restarts is not checked to lie on one path."""

    def __init__(self, label_len, count, pos, restarts, end_total, start_total, end_off, start_off, ends, starts, search_ms,
                 fetch_ms, msa=None, msa_ms=0.0):
        self._label_len = label_len
        self.count, self.pos, self.restarts = count, pos, restarts
        self.end_total, self.start_total = end_total, start_total
        self.end_off, self.start_off = end_off, start_off
        self.end_src, self.end_dst, self.end_offset = ends
        self.start_src, self.start_dst, self.start_offset = starts
        self.search_ms, self.fetch_ms = search_ms, fetch_ms
        self.device_ms = (search_ms, fetch_ms)
        self.end_row, self.end_col, self.start_row, self.start_col = msa if msa is not None else (None,) * 4
        self.msa_ms = msa_ms

    def _rows(self, which, k):
        off = self.end_off if which == "end" else self.start_off
        a, b = int(off[k]), int(off[k + 1])
        return np.stack([getattr(self, f"{which}_{f}")[a:b] for f in ("src", "dst", "offset")], axis=1).astype(np.int64)

    def ends(self, k):
        """int64[rows, 3]: (src, dst, offset) of pattern k's reported ends."""
        return self._rows("end", k)

    def starts(self, k):
        """int64[rows, 3]: (src, dst, offset) of pattern k's reported starts."""
        return self._rows("start", k)

    def _msa_rows(self, which, k):
        if getattr(self, f"{which}_row") is None:
            raise ValueError("no MSA coordinates: ask for them with msa=True")
        off = self.end_off if which == "end" else self.start_off
        a, b = int(off[k]), int(off[k + 1])
        return np.stack([getattr(self, f"{which}_{f}")[a:b] for f in ("row", "col")], axis=1).astype(np.int64)

    def msa_ends(self, k):
        """int64[rows, 2]: (MSA row, MSA column) of pattern k's reported ends, aligned with ends(k)."""
        return self._msa_rows("end", k)

    def msa_starts(self, k):
        """int64[rows, 2]: (MSA row, MSA column) of pattern k's reported starts, aligned with starts(k)."""
        return self._msa_rows("start", k)

    def as_nodes(self, which="end"):
        """Places as (node, offset in the node's label): src where offset < |label(src)|, else dst with the offset
        less |label(src)|; duplicates within a pattern dropped.  -> a list with one sorted int64[rows, 2] array per
        pattern.  which: "end" or "start"."""
        if which not in ("end", "start"):
            raise ValueError('which is "end" or "start"')
        off = self.end_off if which == "end" else self.start_off
        src, dst, o = (getattr(self, f"{which}_{f}").astype(np.int64) for f in ("src", "dst", "offset"))
        la = self._label_len[src] if len(src) else src
        in_src = o < la
        node, noff = np.where(in_src, src, dst), np.where(in_src, o, o - la)
        out = []
        for k in range(len(off) - 1):
            a, b = int(off[k]), int(off[k + 1])
            out.append(np.unique(np.stack((node[a:b], noff[a:b]), axis=1), axis=0).reshape(-1, 2))
        return out


class Seeds:
    """Result of PatternIndex.seeds (include/fbg_hip.h, fbg_pindex_seeds):
      seed_off            uint64[k + 1], CSR offsets of the reported seeds of the k reads (a read's seeds by q_start)
      q_start, length     uint32 per seed: the seed is read[q_start : q_start + length]
      pattern_of          int64 per seed: its read
      occ                 an Occurrences object over the seeds in order, as if every seed had been searched as a pattern
                          of its own (occ.pos equals length; occ.ends(j), occ.starts(j), occ.as_nodes() work per seed)
      chains              the Chains of these seeds when asked for with chain=True, else None
      strands, reads      asked for with strands=True: True and the number k of given reads; seed_off then covers 2k virtual
                          reads, read R as given and read k + R its reverse complement, whose seeds are in the
                          coordinates of the reverse complement.  Otherwise False and the number of reads
      q_forward           int64 per seed: its start in the given read, q_start for a forward seed and
                          L - q_start - length for one of the reverse complement of a read of L symbols
      start_n_rows, start_first_row   asked for with rows=True (None otherwise), uint32 per start place of occ: the number
                          of MSA rows that carry the seed from that place on, and the smallest of them (0xffffffff: none,
                          a place only a recombinant path of the graph spells)
    search_ms: device time of fbg_pindex_seeds; fetch_ms: of the per-seed copies and the expansion of the places."""

    def __init__(self, seed_off, q_start, length, occ, read_len=None, strands=False):
        self.seed_off, self.q_start, self.length, self.occ = seed_off, q_start, length, occ
        self.chains = None
        self.start_n_rows = self.start_first_row = None
        self.pattern_of = np.repeat(np.arange(len(seed_off) - 1, dtype=np.int64), np.diff(seed_off.astype(np.int64)))
        self.search_ms, self.fetch_ms = occ.search_ms, occ.fetch_ms
        self.strands = bool(strands)
        self.reads = (len(seed_off) - 1) // 2 if strands else len(seed_off) - 1
        self.q_forward = q_start.astype(np.int64)
        if strands:
            rev = self.pattern_of >= self.reads
            L = np.asarray(read_len, dtype=np.int64)[self.pattern_of[rev] - self.reads]
            self.q_forward[rev] = L - self.q_forward[rev] - length[rev].astype(np.int64)

    def __len__(self):
        return len(self.q_start)

    def of(self, k, strand=0):
        """int64[rows, 3]: (q_start, length, count) of the seeds of read k; strand=1 (strands=True only): of its reverse
        complement."""
        if strand not in (0, 1) or (strand and not self.strands):
            raise ValueError("strand is 0, or 1 after seeds(strands=True)")
        k += strand * self.reads
        a, b = int(self.seed_off[k]), int(self.seed_off[k + 1])
        return np.stack((self.q_start[a:b], self.length[a:b], self.occ.count[a:b]), axis=1).astype(np.int64)


class Chains:
    """Result of PatternIndex.chains (include/fbg_hip.h, fbg_pindex_chains), for the k reads of the last seeds() call:
      chain_off       uint64[k + 1], CSR offsets of the chains (a read's anchors in ascending q_start)
      score           uint32 per read: read symbols covered by the chain's seeds (0: no anchor); reported also where
                      it is below min_score and the chain therefore empty
      anchor_place    uint32 per chain entry: index into the start arrays of Seeds.occ (start_src .. start_col)
      anchor_seed     uint32 per chain entry: index of its seed (Seeds.q_start, Seeds.length)
    and, after seeds(strands=True) (None otherwise), for the k given reads, whose virtual reads R and k + R these chains cover:
      strand          uint8 per read: 1 if the reverse complement's chain scores higher, else 0; 0xff (_lib.STRAND_NONE) if
                      the chain of that strand is empty
      best_score      uint32 per read: the larger of the two scores
      strand_counts   {forward, reverse, none}: the reads by outcome
    and, asked for with by_row=True (by_row False and the arrays None otherwise; include/fbg_hip.h, fbg_pindex_chains_by_row):
      chain_row       uint32 per read: the smallest MSA row whose supported anchors chain best, 0xffffffff where no row
                      supports an anchor; the chain and the score are then those along this row
      n_best_rows     uint32 per read: how many rows reach that score
    and, asked for with rows=True (None otherwise):
      n_rows, first_row   uint32 per read: how many MSA rows carry every anchor of its chain, and the smallest of them
                      (0 and 0xffffffff for an empty chain, and for one whose anchors no single row carries)
      row_bits        uint64[k, words_per_set]: bit r % 64 of word r // 64 is set for each such row r; row_set(k) lists them
    and, asked for with align=True (None otherwise; include/fbg_hip.h, fbg_pindex_chains_align):
      align_row       uint32 per read: the smallest row that carries its chain, 0xffffffff (_lib.ALIGN_NONE) if none does
      edits           uint32 per read: the fewest edits that turn the read into a stretch of that row's gap-stripped text
                      around the chain; 0xffffffff without a row, and for a read skipped as too long or too wide
      t_start, t_end  uint32 per read: that stretch [t_start, t_end) of the row's text (the smallest end, then the largest
                      start); 0xffffffff where edits is
      best_edits      after seeds(strands=True): uint32 per given read, the edits of the strand that strand picked,
                      0xffffffff where strand is 0xff
      align_ms        device time of fbg_pindex_chains_align: the row choice, the windows and the two passes
    and, asked for with cigar=True beside align=True (None otherwise; include/fbg_hip.h, fbg_pindex_chains_cigar):
      cigar_off       uint64[k + 1], CSR offsets of the reads' runs; a read without an alignment has none
      cigar_ops       uint32 per run: length << 4 | code with BAM's codes I = 1, D = 2, = is 7, X = 8, in read order;
                      cigar(k) gives the string, cigar_runs(k) the (code, length) pairs
      cigar_ms        device time of fbg_pindex_chains_cigar
    and, asked for with graph=True (None otherwise; include/fbg_hip.h, fbg_pindex_chains_align_graph):
      graph_edits     uint32 per read: the fewest edits that turn the read into a stretch of a path of the graph through the
                      blocks around its chain; 0xffffffff for an empty chain and for a read that was not selected, too
                      long or too wide
      graph_start, graph_end   uint32[k, 2]: (node, offset) at which that stretch starts and ends -- the first end cell in
                      (node, offset) order, then the largest start; 0xffffffff where graph_edits is
      graph_path_off  uint64[k + 1], CSR offsets of the reads' paths; a read without an alignment has none
      graph_path_nodes   uint32 per path entry: the nodes from the start node to the end node; graph_path(k) gives read k's
      best_graph_edits   after seeds(strands=True): uint32 per given read, graph_edits of the strand that strand picked
      graph_ms        device time of fbg_pindex_chains_align_graph
    and, asked for with graph_cigar=True beside graph=True (None otherwise; include/fbg_hip.h, fbg_pindex_chains_graph_cigar):
      graph_cigar_off   uint64[k + 1], CSR offsets of the reads' runs; a read without a graph alignment has none
      graph_cigar_ops   uint32 per run, as cigar_ops, in the order of the read and of its path; graph_cigar(k) gives the
                      string, graph_cigar_runs(k) the (code, length) pairs
      graph_cigar_ms  device time of fbg_pindex_chains_graph_cigar
    and, asked for with mapq=True (None otherwise; include/fbg_hip.h, fbg_pindex_chains_mapq):
      second_score    uint32 per read: the score of its best chain on the anchors outside the columns of its chain, widened by
                      the margin; 0 without one, and for an empty chain
      second_lo, second_hi   uint32 per read: the MSA columns [second_lo, second_hi) of that second chain, 0xffffffff without one
      mapq            uint8 per read: 60 * (score - min(second_score, score)) // read length, 0 for an empty chain
      second_off, second_place, second_seed   the second chains, as chain_off, anchor_place and anchor_seed; second(k) gives
                      read k's
      mapq_stranded   after seeds(strands=True): uint8 per virtual read, mapq with the other strand's score as a competitor
      best_mapq       after seeds(strands=True): uint8 per given read, mapq_stranded of the strand that strand picked, 0
                      where strand is 0xff
      mapq_ms         device time of fbg_pindex_chains_mapq
    and, asked for with pairs=(min_insert, max_insert) after seeds(strands=True) on interleaved mates (None otherwise;
    include/fbg_hip.h, fbg_pindex_chains_pairs), for the k / 4 pairs, pair p being the given reads 2p and 2p + 1:
      pair_which      uint8 per pair: the chosen candidate 0 .. 3, 0xff (_lib.PAIR_NONE) without a valid one; pair(p) names
                      its forward and reverse virtual read and says which of the two chains is the rescue
      pair_score      uint32 per pair: the sum of the two chains' scores, 0 without a candidate
      pair_lo, pair_hi   uint32 per pair: the first column of the forward chain and the end of the reverse one, 0xffffffff
                      without a candidate
      rescue_score, rescue_lo, rescue_hi   uint32 per virtual read: score and columns of its rescue chain, the chain on the
                      start places inside the window its partner's chain opens (0 and 0xffffffff where it is empty)
      rescue_off, rescue_place, rescue_seed   the rescue chains, as chain_off, anchor_place and anchor_seed; rescue(v)
                      gives virtual read v's
      pair_stats      {which0 .. which3, none, places_kept, places_excluded, rescue_differs}: stats[] of the call
      pairs_ms        device time of fbg_pindex_chains_pairs
    With adopt_pairs=True every other field describes the adopted chains.
    and, asked for with pair_align=True beside pairs= (None otherwise; include/fbg_hip.h, fbg_pindex_pairs_align):
      mate_row        uint32 per virtual read: the row of its partner's chain on which its window lies, 0xffffffff for a read
                      that is not selected or whose partner's chain no row carries
      mate_edits, mate_start, mate_end   uint32 per virtual read: the edits of the read against its insert window and the
                      stretch of the row's text it lies on, as edits, t_start and t_end; 0xffffffff where nothing was aligned
      mate_insert     uint32 per virtual read: the pair's extent in symbols of the row, 0xffffffff unless accepted
      mate_which, mate_score, mate_lo, mate_hi   per pair: the chosen candidate 0 .. 3 (0xff without one), the chain's score
                      plus the aligned read's length less its edits, and the pair's extent on the row
      mate_stats      {selected, aligned, no_row, empty, too_long, too_wide, rejected_edits, rejected_insert, cells, pairs}
      mate_ms         device time of fbg_pindex_pairs_align
    device_ms: device time of the chaining; fetch_ms: of the copies of the two anchor arrays."""

    def __init__(self, chain_off, score, anchor_place, anchor_seed, device_ms, fetch_ms):
        self.chain_off, self.score = chain_off, score
        self.anchor_place, self.anchor_seed = anchor_place, anchor_seed
        self.device_ms, self.fetch_ms = device_ms, fetch_ms
        self.strand = self.best_score = self.strand_counts = None
        self.n_rows = self.first_row = self.row_bits = None
        self.chain_row = self.n_best_rows = None
        self.by_row = False
        self.align_row = self.edits = self.t_start = self.t_end = self.best_edits = self.align_ms = None
        self.cigar_off = self.cigar_ops = self.cigar_ms = None
        self.graph_edits = self.graph_start = self.graph_end = self.graph_path_off = self.graph_path_nodes = None
        self.best_graph_edits = self.graph_ms = None
        self.graph_cigar_off = self.graph_cigar_ops = self.graph_cigar_ms = None
        self.second_score = self.second_lo = self.second_hi = self.mapq = self.second_off = None
        self.second_place = self.second_seed = self.mapq_stranded = self.best_mapq = self.mapq_ms = None
        self.pair_which = self.pair_score = self.pair_lo = self.pair_hi = self.pair_stats = self.pairs_ms = None
        self.rescue_off = self.rescue_score = self.rescue_lo = self.rescue_hi = self.rescue_place = self.rescue_seed = None
        self.mate_row = self.mate_edits = self.mate_start = self.mate_end = self.mate_insert = None
        self.mate_which = self.mate_score = self.mate_lo = self.mate_hi = self.mate_stats = self.mate_ms = None

    PAIR_STATS = ("which0", "which1", "which2", "which3", "none", "places_kept", "places_excluded", "rescue_differs")
    MATE_STATS = ("selected", "aligned", "no_row", "empty", "too_long", "too_wide", "rejected_edits", "rejected_insert", "cells", "pairs")

    def rescue(self, v):
        """int64[rows, 2]: (anchor_place, anchor_seed) of the rescue chain of virtual read v, as of()."""
        if self.rescue_off is None:
            raise ValueError("no rescue chains: ask for them with pairs=(min_insert, max_insert)")
        a, b = int(self.rescue_off[v]), int(self.rescue_off[v + 1])
        return np.stack((self.rescue_place[a:b], self.rescue_seed[a:b]), axis=1).astype(np.int64)

    def pair(self, p):
        """(forward virtual read, reverse virtual read, forward chain is the rescue, reverse chain is the rescue) of the
        candidate chosen for pair p, the given reads 2p and 2p + 1; None where the pair has no valid candidate."""
        if self.pair_which is None:
            raise ValueError("no pairs: ask for them with pairs=(min_insert, max_insert)")
        i, n = int(self.pair_which[p]), (len(self.chain_off) - 1) // 2
        if i == _lib.PAIR_NONE:
            return None
        a, b = 2 * p, 2 * p + 1
        return (a if i < 2 else b), (b if i < 2 else a) + n, bool(i & 1), not i & 1

    def cigar_runs(self, k):
        """int64[runs, 2]: (code, length) of the runs of read k's alignment path; no rows without an alignment."""
        if self.cigar_off is None:
            raise ValueError("no paths: ask for them with align=True, cigar=True")
        v = self.cigar_ops[int(self.cigar_off[k]):int(self.cigar_off[k + 1])].astype(np.int64)
        return np.stack((v & 15, v >> 4), axis=1)

    def cigar(self, k):
        """The alignment path of read k as a CIGAR string with = and X, such as 25=1X24=; "" without an alignment."""
        return "".join(f"{n}{_lib.CIGAR_OPS[c]}" for c, n in self.cigar_runs(k).tolist())

    def graph_cigar_runs(self, k):
        """int64[runs, 2]: (code, length) of the runs of read k's alignment path in the graph; no rows without one."""
        if self.graph_cigar_off is None:
            raise ValueError("no paths: ask for them with graph=True, graph_cigar=True")
        v = self.graph_cigar_ops[int(self.graph_cigar_off[k]):int(self.graph_cigar_off[k + 1])].astype(np.int64)
        return np.stack((v & 15, v >> 4), axis=1)

    def graph_cigar(self, k):
        """The alignment path of read k against its stretch of the graph as a CIGAR string; "" without an alignment."""
        return "".join(f"{n}{_lib.CIGAR_OPS[c]}" for c, n in self.graph_cigar_runs(k).tolist())

    def graph_path(self, k):
        """int64[n_path]: the nodes of read k's path in the graph, from its start node to its end node."""
        if self.graph_path_off is None:
            raise ValueError("no graph alignment: ask for it with graph=True")
        return self.graph_path_nodes[int(self.graph_path_off[k]):int(self.graph_path_off[k + 1])].astype(np.int64)

    def row_set(self, k):
        """int64[n_rows[k]]: the rows that carry the whole chain of read k, ascending."""
        if self.row_bits is None:
            raise ValueError("no row sets: ask for them with rows=True")
        w = self.row_bits[k]
        return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).astype(np.int64)

    def of(self, k):
        """int64[rows, 2]: (anchor_place, anchor_seed) of the chain of read k."""
        a, b = int(self.chain_off[k]), int(self.chain_off[k + 1])
        return np.stack((self.anchor_place[a:b], self.anchor_seed[a:b]), axis=1).astype(np.int64)

    def second(self, k):
        """int64[rows, 2]: (anchor_place, anchor_seed) of the second-best chain of read k, as of()."""
        if self.second_off is None:
            raise ValueError("no second chains: ask for them with mapq=True")
        a, b = int(self.second_off[k]), int(self.second_off[k + 1])
        return np.stack((self.second_place[a:b], self.second_seed[a:b]), axis=1).astype(np.int64)

    def best(self, k):
        """int64[rows, 2]: the chain of given read k on its chosen strand, as of(); empty where strand[k] is 0xff."""
        if self.strand is None:
            raise ValueError("no strands: ask for them with seeds(strands=True)")
        t = int(self.strand[k])
        if t == _lib.STRAND_NONE:
            return np.zeros((0, 2), dtype=np.int64)
        return self.of(t * len(self.strand) + k)


class Validation:
    """Result of PatternIndex.validate / Engine.validate_graph:
      status          uint8[n], FBG_NODE_* (0 valid, 1 invalid, 2 source / sink, 3 ignored, 4 empty label)
      witness_node    int64[n], the node of an INVALID node's witness occurrence, -1 where there is none
      witness_offset  int64[n], its offset in that node's label, -1 where there is none
      valid           no node is INVALID
      invalid_nodes   int64 indices of the INVALID nodes, ascending
      bad_cuts        sorted distinct b - 1 over the blocks b > 0 that hold an INVALID node (the reference's to_remove)
      device_ms       device time of the validation kernels
      slots_scanned, wave_nodes   SA slots read and nodes scanned by the wave tier (fbg_pindex_validate_stats)"""

    def __init__(self, status, wn, wo, blocks, device_ms, slots_scanned, wave_nodes):
        none = wn == np.uint64(0xffffffffffffffff)
        self.status = status
        self.witness_node = np.where(none, -1, wn.astype(np.int64))
        self.witness_offset = np.where(wo == np.uint64(0xffffffffffffffff), -1, wo.astype(np.int64))
        self.invalid_nodes = np.nonzero(status == _lib.NODE_INVALID)[0].astype(np.int64)
        self.valid = len(self.invalid_nodes) == 0
        cuts = blocks[self.invalid_nodes]
        self.bad_cuts = np.unique(cuts[cuts > 0] - 1).astype(np.int64)
        self.device_ms = device_ms
        self.slots_scanned = slots_scanned
        self.wave_nodes = wave_nodes

    def counts(self):
        """{valid, invalid, source_sink, ignored, empty}: nodes per status."""
        c = np.bincount(self.status, minlength=5)
        return dict(zip(("valid", "invalid", "source_sink", "ignored", "empty"), (int(x) for x in c[:5])))


