"""Host-side mirror of the reference's in-process seam for the segmentation path.

Names and argument meaning follow founderblockgraph.cpp ("fbg.cpp"):
  segment_elastic_minmaxlength  fbg.cpp:1836-2040   (elastic: f[] scan + min-max-length DP)
  segment                       fbg.cpp:526-664     (non-elastic: v[] scan + s/prev DP)
Every call goes through the C ABI of libfbg_hip.so (include/fbg_hip.h); nothing here computes.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import FBG_ERR_NO_SEGMENTATION, FBG_OK, STAGES, _ignore, _sat64, _u8, _u32, _u64  # noqa: F401
from .pindex import Chains, Occurrences, PatternIndex, Seeds, Validation, _concat, complement_table  # noqa: F401


class FbgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfbg_hip error {code}: {msg}")
        self.code = code


class NoSegmentation(FbgError):
    """'No valid segmentation found!' (fbg.cpp:1934) / 'No proper segmentation exists.' (fbg.cpp:650)."""


def as_msa(rows):
    """(m, n) uint8 array from an array or a list of equal-length str/bytes rows."""
    if isinstance(rows, np.ndarray):
        a = np.ascontiguousarray(rows, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("MSA must be 2-D (rows x columns)")
        return a
    rows = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("MSA rows must be non-empty and of equal length")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0])).copy()


class Engine:
    """One fbg_ctx (one GPU, one stream).  Calls on one engine must be serialised by the caller."""

    _h = None               # the library's context, until close()
    _borrowed = False       # a group's member belongs to the group
    _pindexes = None        # the pattern indexes that borrow the context: a WeakSet once there is one

    def __init__(self, device=0):
        self._L = _lib.lib()
        h = C.c_void_p()
        rc = self._L.fbg_ctx_create(int(device), C.byref(h))
        if rc != FBG_OK:
            raise FbgError(rc, self._L.fbg_last_error(None).decode())
        self._h = h
        self.device = int(device)

    def close(self):
        for pix in list(self._pindexes or ()):              # an index borrows the context: it goes first
            pix.close()
        if self._h:
            if not self._borrowed:
                self._L.fbg_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc == FBG_OK:
            return
        msg = self._L.fbg_last_error(self._h).decode()
        raise (NoSegmentation if rc == FBG_ERR_NO_SEGMENTATION else FbgError)(rc, msg)

    # ---- host-buffer entry points --------------------------------------------------------
    def elastic_f(self, msa, ignorechars="", disable_efg_tricks=False, f=None):
        """compute_f: f is max-merged into (zeros if omitted), as fbg.cpp:1681 / 3388."""
        msa = as_msa(msa)
        m, n = msa.shape
        self._msa_rows = m
        ig, il = _ignore(ignorechars)
        f = np.zeros(n, dtype=np.uint64) if f is None else np.ascontiguousarray(f, dtype=np.uint64).copy()
        rc = self._L.fbg_elastic_f(self._h, _u8(msa), m, n, _u8(ig), il, int(disable_efg_tricks), _u64(f))
        if rc == FBG_ERR_NO_SEGMENTATION:
            raise NoSegmentation(rc, self._L.fbg_last_error(self._h).decode())
        self._chk(rc)
        return f

    def minmax_dp(self, f, full=False):
        f = np.ascontiguousarray(f, dtype=np.uint64)
        n = len(f)
        b = np.empty(n + 1, dtype=np.uint64)
        mml = np.empty(n + 1, dtype=np.uint64)
        bt = np.empty(n + 1, dtype=np.uint64)
        cnt = C.c_uint64(0)
        self._chk(self._L.fbg_minmax_dp(self._h, _u64(f), n, _u64(b), C.byref(cnt), _u64(mml), _u64(bt)))
        b = b[:cnt.value].copy()
        return (b, mml, bt) if full else b

    def repeatfree_v(self, msa):
        msa = as_msa(msa)
        m, n = msa.shape
        v = np.empty(n, dtype=np.uint64)
        self._chk(self._L.fbg_repeatfree_v(self._h, _u8(msa), m, n, _u64(v)))
        return v

    def repeatfree_dp(self, v):
        """-> (s, prev, boundaries); boundaries is None when no proper segmentation exists."""
        v = np.ascontiguousarray(v, dtype=np.uint64)
        n = len(v)
        s = np.empty(n, dtype=np.uint64)
        prev = np.empty(n, dtype=np.uint64)
        b = np.empty(n, dtype=np.uint64)
        cnt = C.c_uint64(0)
        rc = self._L.fbg_repeatfree_dp(self._h, _u64(v), n, _u64(s), _u64(prev), _u64(b), C.byref(cnt))
        if rc == FBG_ERR_NO_SEGMENTATION:
            return s, prev, None
        self._chk(rc)
        return s, prev, b[:cnt.value].copy()

    def gapped_v(self, msa):
        """v[] of segment2elasticValid (fbg.cpp:763-822): non-elastic mode, rows may hold gaps."""
        msa = as_msa(msa)
        m, n = msa.shape
        v = np.empty(n, dtype=np.uint64)
        self._chk(self._L.fbg_gapped_v(self._h, _u8(msa), m, n, _u64(v)))
        return v

    def gapped_dp(self, v):
        """fbg.cpp:827-866 -> (s, prev, boundaries); boundaries is None for 'No valid segmentation found!'."""
        v = np.ascontiguousarray(v, dtype=np.uint64)
        n = len(v)
        s = np.empty(n, dtype=np.uint64)
        prev = np.empty(n, dtype=np.uint64)
        b = np.empty(n, dtype=np.uint64)
        cnt = C.c_uint64(0)
        rc = self._L.fbg_gapped_dp(self._h, _u64(v), n, _u64(s), _u64(prev), _u64(b), C.byref(cnt))
        if rc == FBG_ERR_NO_SEGMENTATION:
            return s, prev, None
        self._chk(rc)
        return s, prev, b[:cnt.value].copy()

    def block_graph(self, boundaries):
        """Nodes / edges of the elastic founder graph for a segmentation of the current MSA (fbg_block_graph):
        (node_of[nb, m], first_node[nb + 1], rep_row[nb, m], edge_count[nb], edges[nb, m])."""
        b = np.ascontiguousarray(boundaries, dtype=np.uint64)
        nb = len(b)
        m = self._msa_rows
        node_of = np.empty((nb, m), dtype=np.uint32)
        rep_row = np.empty((nb, m), dtype=np.uint32)
        first = np.empty(nb + 1, dtype=np.uint64)
        ecount = np.empty(nb, dtype=np.uint64)
        edges = np.empty((nb, m), dtype=np.uint64)
        self._chk(self._L.fbg_block_graph(self._h, _u64(b), nb, _u32(node_of), _u64(first), _u32(rep_row), _u64(ecount), _u64(edges)))
        return node_of, first, rep_row, ecount, edges

    # ---- device-resident staged API ------------------------------------------------------
    def msa_load_host(self, msa):
        msa = as_msa(msa)
        self._msa_rows = msa.shape[0]
        self._chk(self._L.fbg_msa_load_host(self._h, _u8(msa), msa.shape[0], msa.shape[1]))

    def msa_set_device(self, ptr, m, n):
        self._msa_rows = m
        self._chk(self._L.fbg_msa_set_device(self._h, C.c_void_p(ptr), m, n))

    def msa_synthetic(self, ptr, m, n, seed=0x5EED0001, seed2=0x5EED0002, gap_fraction=0.0, gap_run=0,
                      seed3=0x5EED0003, n_fraction=0.0):
        gthr = int((1 << 64) * (gap_fraction / gap_run)) if gap_run else 0
        nthr = int((1 << 64) * n_fraction)
        self._chk(self._L.fbg_msa_synthetic(self._h, C.c_void_p(ptr), m, n, seed, seed2, gthr, gap_run, seed3, nthr))

    def index_build(self, reversed=False, ignorechars=""):
        ig, il = _ignore(ignorechars)
        self._chk(self._L.fbg_index_build(self._h, int(reversed), _u8(ig), il))

    # partitioned index (multi-GPU, include/fbg_hip.h): each returns ok; False = use index_build on every rank
    def part_index_build(self, part, nparts, d_blob_ptr, reversed=False, ignorechars="", disable_efg_tricks=False):
        """One key-range partition of the index (fbg_part_index_build_ignore).  MSAs with gaps / ignore characters are
        scanned for ONE setting of the elastic tricks (option part_tricks_off), given here."""
        ok = C.c_int(0)
        ig, il = _ignore(ignorechars)
        self.set_option("part_tricks_off", int(bool(disable_efg_tricks)))
        self._chk(self._L.fbg_part_index_build_ignore(self._h, int(reversed), part, nparts, _u8(ig), il, C.c_void_p(d_blob_ptr), C.byref(ok)))
        return bool(ok.value)

    def part_scan(self, d_blobs_ptr, d_gmax_ptr):
        ok = C.c_int(0)
        self._chk(self._L.fbg_part_scan(self._h, C.c_void_p(d_blobs_ptr), C.c_void_p(d_gmax_ptr), C.byref(ok)))
        return bool(ok.value)

    def part_finish(self, d_gmax_ptr):
        """0: declined, 1: index ready, 2: call part_rescan, reduce again, then part_finish again"""
        ok = C.c_int(0)
        self._chk(self._L.fbg_part_finish(self._h, C.c_void_p(d_gmax_ptr), C.byref(ok)))
        return int(ok.value)

    def part_rescan(self, d_gmax_ptr):
        self._chk(self._L.fbg_part_rescan(self._h, C.c_void_p(d_gmax_ptr)))

    def scan_f(self, x0, x1, d_f_ptr, disable_efg_tricks=False):
        self._chk(self._L.fbg_scan_f(self._h, x0, x1, int(disable_efg_tricks), C.c_void_p(d_f_ptr)))

    def scan_v(self, x0, x1, d_v_ptr):
        self._chk(self._L.fbg_scan_v(self._h, x0, x1, C.c_void_p(d_v_ptr)))

    def minmax_dp_device(self, d_f_ptr, n, d_boundaries_ptr, d_mml_ptr=None, d_bt_ptr=None):
        cnt = C.c_uint64(0)
        self._chk(self._L.fbg_minmax_dp_device(self._h, C.c_void_p(d_f_ptr), n, C.c_void_p(d_boundaries_ptr),
                                               C.byref(cnt), C.c_void_p(d_mml_ptr), C.c_void_p(d_bt_ptr)))
        return cnt.value

    def repeatfree_dp_device(self, d_v_ptr, n, d_boundaries_ptr, d_s_ptr=None, d_prev_ptr=None):
        cnt = C.c_uint64(0)
        self._chk(self._L.fbg_repeatfree_dp_device(self._h, C.c_void_p(d_v_ptr), n, C.c_void_p(d_s_ptr),
                                                   C.c_void_p(d_prev_ptr), C.c_void_p(d_boundaries_ptr),
                                                   C.byref(cnt)))
        return cnt.value

    def scan_gapped_v(self, d_v_ptr):
        self._chk(self._L.fbg_scan_gapped_v(self._h, C.c_void_p(d_v_ptr)))

    def gapped_dp_device(self, d_v_ptr, n, d_boundaries_ptr, d_s_ptr=None, d_prev_ptr=None):
        cnt = C.c_uint64(0)
        rc = self._L.fbg_gapped_dp_device(self._h, C.c_void_p(d_v_ptr), n, C.c_void_p(d_s_ptr),
                                          C.c_void_p(d_prev_ptr), C.c_void_p(d_boundaries_ptr), C.byref(cnt))
        if rc == FBG_ERR_NO_SEGMENTATION:
            return None
        self._chk(rc)
        return cnt.value

    def set_option(self, key, value=1):
        """fbg_set_option: behaviour switch of this context (include/fbg_hip.h lists the keys)."""
        self._chk(self._L.fbg_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._chk(self._L.fbg_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def options(self, **kv):
        """Context manager: set the given options, restore the previous values on exit."""
        eng = self

        class _Scope:
            def __enter__(self_):
                self_.old = {k: eng.get_option(k) for k in kv}
                for k, v in kv.items():
                    eng.set_option(k, v)
                return eng

            def __exit__(self_, *exc):
                for k, v in self_.old.items():
                    eng.set_option(k, v)
        return _Scope()

    def set_stream(self, stream_handle):
        self._chk(self._L.fbg_set_stream(self._h, C.c_void_p(stream_handle)))

    def sync(self):
        self._chk(self._L.fbg_sync(self._h))

    def stage_ms(self):
        out = {}
        for k, name in enumerate(STAGES):
            ms, ln = C.c_float(0), C.c_int(0)
            self._chk(self._L.fbg_stage_ms(self._h, k, C.byref(ms), C.byref(ln)))
            out[name] = (ms.value, ln.value)
        return out

    def release_scratch(self):
        self._chk(self._L.fbg_release_scratch(self._h))

    def device_bytes(self):
        return int(self._L.fbg_device_bytes(self._h))

    def text_length(self):
        return int(self._L.fbg_text_length(self._h))

    def index_download(self):
        N = self.text_length()
        T = np.empty(N, dtype=np.uint8)
        arrs = [np.empty(N, dtype=np.uint32) for _ in range(4)]
        self._chk(self._L.fbg_index_download(self._h, _u8(T), *[_u32(a) for a in arrs]))
        return (T, *arrs)

    def pattern_index(self, labels, edges):
        """Pattern index of a founder graph (fbg_pindex_build): labels in node id order (a list of str / bytes, or a
        pair (uint8 data, uint64 offsets[nodes + 1])), edges as (u, v) pairs of 0-based indices into labels.  Borrows
        this engine's device and stream; closing the engine closes its indexes first."""
        pix = PatternIndex(self, labels, edges)
        if self._pindexes is None:
            self._pindexes = weakref.WeakSet()
        self._pindexes.add(pix)
        return pix

    def pattern_index_of_segmentation(self, boundaries, rows=False):
        """Pattern index of the graph that `boundaries` cuts out of the current MSA, built on the device
        (fbg_pindex_build_segmentation): the index pattern_index(*graph_from_segmentation(...)) gives, without the trip
        of nodes, edges and labels through the host.  node_block / first_node: the block of every node, the first
        node of every block.  rows=True (fbg_pindex_build_segmentation_rows): the same index plus the row table that
        seeds(rows=True), chains(rows=True) and rows_stats() need."""
        b = np.ascontiguousarray(boundaries, dtype=np.uint64)
        h = C.c_void_p()
        build = self._L.fbg_pindex_build_segmentation_rows if rows else self._L.fbg_pindex_build_segmentation
        self._chk(build(self._h, _u64(b), len(b), C.byref(h)))
        pix = PatternIndex._adopt(self, h, len(b))
        pix._has_rows = bool(rows)
        if self._pindexes is None:
            self._pindexes = weakref.WeakSet()
        self._pindexes.add(pix)
        return pix

    def validate_segmentation(self, boundaries, ignorechars=""):
        """Semi-repeat-free check of the graph of a segmentation of the current MSA (fbg_segmentation_validate)
        -> SegmentationCheck: cut_bad uint8[nb] (1: the block after this boundary holds an INVALID node), bad_cuts
        (their indices, the reference's to_remove), n_nodes, n_invalid, valid, device_ms."""
        b = np.ascontiguousarray(boundaries, dtype=np.uint64)
        ig, il = _ignore(ignorechars)
        cut = np.zeros(max(len(b), 1), dtype=np.uint8)
        nn, bad, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        self._chk(self._L.fbg_segmentation_validate(self._h, _u64(b), len(b), _u8(ig), il, _u8(cut), C.byref(nn), C.byref(bad),
                                                    C.byref(ms)))
        return SegmentationCheck(cut[:len(b)], nn.value, bad.value, ms.value)

    def repair_segmentation(self, boundaries, ignorechars="", timing=None):
        """The repair loop of the row-chunk mode (fbg_segmentation_repair; fbg.cpp:3471-3497): validate, drop the
        boundaries before blocks that hold an INVALID node, repeat -> (boundaries, rounds, removed), removed the
        count of dropped boundaries per round.  timing: a dict that receives device_ms."""
        b = np.ascontiguousarray(boundaries, dtype=np.uint64).copy()
        ig, il = _ignore(ignorechars)
        nb, rounds, ms = C.c_uint64(len(b)), C.c_uint64(0), C.c_double(0)
        removed = np.zeros(max(len(b), 1), dtype=np.uint64)
        self._chk(self._L.fbg_segmentation_repair(self._h, _u64(b), C.byref(nb), _u8(ig), il, C.byref(rounds), _u64(removed),
                                                  C.byref(ms)))
        if timing is not None:
            timing["device_ms"] = ms.value
        return b[:nb.value].copy(), int(rounds.value), [int(x) for x in removed[:rounds.value]]

    def validate_graph(self, labels, edges, blocks, ignorechars=""):
        """Semi-repeat-free check of a founder graph (PatternIndex.validate on a temporary index of the graph)."""
        with self.pattern_index(labels, edges) as pix:
            return pix.validate(blocks, ignorechars)


class SegmentationCheck:
    """Result of Engine.validate_segmentation: cut_bad uint8[nb], bad_cuts int64 (indices of the flagged boundaries,
    ascending), n_nodes, n_invalid, valid (nothing flagged), device_ms."""

    def __init__(self, cut_bad, n_nodes, n_invalid, device_ms):
        self.cut_bad = cut_bad
        self.bad_cuts = np.nonzero(cut_bad)[0].astype(np.int64)
        self.n_nodes, self.n_invalid = int(n_nodes), int(n_invalid)
        self.valid = len(self.bad_cuts) == 0
        self.device_ms = device_ms


def read_xgfa(path, blocks=False):
    """(labels, edges) of an xGFA (or GFA) file: S lines sorted by id (0- or 1-based alike), L lines as (u, v) pairs of
    indices into labels.  Empty labels are kept.  blocks=True: (labels, edges, node_block), node_block int64[n] the
    block (from 0) of every node from the B line, whose sizes cover the nodes in ascending S id (xGFAspec.md);
    ValueError when the B line is missing or its sizes do not sum to the node count."""
    ids, labs, links, bline = [], [], [], None
    with open(path, "rb") as fh:
        for line in fh:
            f = line.rstrip(b"\r\n").split(b"\t")
            if f[0] == b"S":
                ids.append(int(f[1]))
                labs.append(f[2] if len(f) > 2 else b"")
            elif f[0] == b"L":
                links.append((int(f[1]), int(f[3])))
            elif f[0] == b"B" and blocks:
                if bline is not None:
                    raise ValueError(f"{path}: a second B line")
                bline = [int(x) for x in f[1:] if x != b""]
    order = sorted(range(len(ids)), key=lambda k: ids[k])
    where = {ids[k]: i for i, k in enumerate(order)}
    out = [labs[k] for k in order], [(where[u], where[v]) for u, v in links]
    if not blocks:
        return out
    if bline is None:
        raise ValueError(f"{path}: no B line (block sizes)")
    sizes = np.array(bline, dtype=np.int64)
    if (sizes < 0).any() or int(sizes.sum()) != len(ids):
        raise ValueError(f"{path}: the B line's block sizes sum to {int(sizes.sum())}, not to the {len(ids)} nodes")
    return out + (np.repeat(np.arange(len(sizes), dtype=np.int64), sizes),)


def graph_from_segmentation(engine, msa, boundaries, packed=False, with_blocks=False):
    """(labels, edges) of the elastic founder graph of a segmentation of `msa` (the nodes and edges of
    Engine.block_graph; the MSA becomes the engine's current one).  Labels are the gap-stripped rows of the blocks:
    a list of bytes, or with packed=True a pair (uint8 data, uint64 offsets); edges an (E, 2) int64 array.
    with_blocks=True: (labels, edges, node_block), node_block int64[n] the block (from 0) of every node."""
    msa = as_msa(msa)
    m, n = msa.shape
    engine.msa_load_host(msa)
    b = np.ascontiguousarray(boundaries, dtype=np.uint64)
    node_of, first, rep_row, ecount, edges = engine.block_graph(b)
    chunks, lens = [], []
    for j in range(len(b)):
        x0 = int(b[j - 1]) + 1 if j else 0
        x1 = min(int(b[j]) + 1, n)
        sub = msa[rep_row[j, :int(first[j + 1] - first[j])], x0:x1]
        keep = sub != ord("-")
        chunks.append(sub[keep])
        lens.append(keep.sum(axis=1))
    data = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    off = np.zeros(int(first[-1]) + 1, dtype=np.uint64)
    if len(off) > 1:
        off[1:] = np.cumsum(np.concatenate(lens), dtype=np.uint64)
    sel = edges[np.arange(m)[None, :] < ecount[:, None].astype(np.int64)]
    pairs = np.stack(((sel >> np.uint64(32)).astype(np.int64), (sel & np.uint64(0xffffffff)).astype(np.int64)), axis=1)
    extra = (np.repeat(np.arange(len(b), dtype=np.int64), np.diff(first.astype(np.int64))),) if with_blocks else ()
    if packed:
        return ((data, off), pairs) + extra
    raw = data.tobytes()
    return ([raw[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)], pairs) + extra


class _DeviceArray:
    """A device pointer dressed up for torch.as_tensor (zero copy): __cuda_array_interface__, version 2."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def device_view(ptr, count, typestr="<i8"):
    """torch view (no copy) of `count` elements of engine-owned device memory; valid as long as the engine keeps it."""
    import torch
    return torch.as_tensor(_DeviceArray(ptr, count, typestr), device="cuda")


class Group:
    """fbg_group: several contexts (one per entry of `devices`; an id may repeat) driven as one engine --
    include/fbg_hip.h, 'several GPUs as one engine'.  The sweep and block_graph run on member(0)."""

    _h = None

    def __init__(self, devices=None):
        self._L = _lib.lib()
        h = C.c_void_p()
        if devices is None:
            rc = self._L.fbg_group_create(0, None, C.byref(h))
        else:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._L.fbg_group_create(len(devices), ids, C.byref(h))
        if rc != FBG_OK:
            raise FbgError(rc, self._L.fbg_group_last_error(None).decode())
        self._h = h
        self._members = {}

    def close(self):
        if self._h:
            for e in self._members.values():
                e._h = None                        # owned by the group
            self._L.fbg_group_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc == FBG_OK:
            return
        msg = self._L.fbg_group_last_error(self._h).decode()
        raise (NoSegmentation if rc == FBG_ERR_NO_SEGMENTATION else FbgError)(rc, msg)

    def size(self):
        return int(self._L.fbg_group_size(self._h))

    def member(self, i=0):
        """Engine view of member i's context (borrowed: closing it is a no-op)."""
        if i not in self._members:
            e = Engine.__new__(Engine)
            e._L = self._L
            e._h = C.c_void_p(self._L.fbg_group_member(self._h, i))
            e.device = None
            e._borrowed = True
            self._members[i] = e
        return self._members[i]

    def set_option(self, key, value=1):
        self._chk(self._L.fbg_group_set_option(self._h, key.encode(), int(value)))

    def plan_used(self):
        parts = C.c_int(0)
        plan = self._L.fbg_group_plan_used(self._h, C.byref(parts))
        return _lib.PLANS[plan], parts.value

    def elastic_f(self, msa, ignorechars="", disable_efg_tricks=False, f=None):
        msa = as_msa(msa)
        m, n = msa.shape
        self.member(0)._msa_rows = m
        ig, il = _ignore(ignorechars)
        f = np.zeros(n, dtype=np.uint64) if f is None else np.ascontiguousarray(f, dtype=np.uint64).copy()
        self._chk(self._L.fbg_group_elastic_f(self._h, _u8(msa), m, n, _u8(ig), il, int(disable_efg_tricks), _u64(f)))
        return f

    def repeatfree_v(self, msa):
        msa = as_msa(msa)
        v = np.empty(msa.shape[1], dtype=np.uint64)
        self._chk(self._L.fbg_group_repeatfree_v(self._h, _u8(msa), msa.shape[0], msa.shape[1], _u64(v)))
        return v

    def gapped_v(self, msa):
        msa = as_msa(msa)
        v = np.empty(msa.shape[1], dtype=np.uint64)
        self._chk(self._L.fbg_group_gapped_v(self._h, _u8(msa), msa.shape[0], msa.shape[1], _u64(v)))
        return v

    def msa_load_host(self, msa):
        msa = as_msa(msa)
        self.member(0)._msa_rows = msa.shape[0]
        self._chk(self._L.fbg_group_msa_load_host(self._h, _u8(msa), msa.shape[0], msa.shape[1]))

    def msa_synthetic(self, m, n, seed=0x5EED0001, seed2=0x5EED0002, gap_fraction=0.0, gap_run=0, seed3=0x5EED0003,
                      n_fraction=0.0):
        gthr = int((1 << 64) * (gap_fraction / gap_run)) if gap_run else 0
        nthr = int((1 << 64) * n_fraction)
        self.member(0)._msa_rows = m
        self._chk(self._L.fbg_group_msa_synthetic(self._h, m, n, seed, seed2, gthr, gap_run, seed3, nthr))

    def scan_f(self, ignorechars="", disable_efg_tricks=False):
        """f of the current MSA -> device pointer (member 0's memory, n uint64 values)."""
        ig, il = _ignore(ignorechars)
        p = C.c_void_p()
        self._chk(self._L.fbg_group_scan_f(self._h, _u8(ig), il, int(disable_efg_tricks), C.byref(p)))
        return p.value


# ---- reference-shaped free functions ---------------------------------------------------------

def segment_elastic_minmaxlength(MSA, ignorechars="", disable_efg_tricks=False, f=None, segment=True,
                                 engine=None):
    """fbg.cpp:1836-2040.  Returns (out_indices, f); out_indices is None when segment=False."""
    eng = engine or Engine()
    try:
        f = eng.elastic_f(MSA, ignorechars, disable_efg_tricks, f)
        if not segment:
            return None, f
        return eng.minmax_dp(f), f
    finally:
        if engine is None:
            eng.close()


def segment_elastic_heuristic(MSA, rows, ignorechars="", disable_efg_tricks=False, engine=None):
    """The row-chunk mode, --heuristic-subset=ROWNUM (fbg.cpp:3400-3433, 3467-3500): f of every chunk of `rows`
    consecutive rows max-merged, the min-max-length DP on the merged f, then the repair loop on the graph of the whole
    MSA.  Returns (boundaries, f, rounds, removed).  NoSegmentation as a chunk raises it (disable_efg_tricks only)."""
    MSA = as_msa(MSA)
    rows = int(rows)
    if rows <= 0:
        raise ValueError("rows must be positive")
    eng = engine or Engine()
    try:
        f = None
        for r in range(0, MSA.shape[0], rows):
            f = eng.elastic_f(MSA[r:r + rows], ignorechars, disable_efg_tricks, f)
        b = eng.minmax_dp(f)
        eng.msa_load_host(MSA)
        b, rounds, removed = eng.repair_segmentation(b, ignorechars)
        return b, f, rounds, removed
    finally:
        if engine is None:
            eng.close()


def segment2elasticValid(MSA, engine=None):
    """fbg.cpp:738-866 up to the boundaries (non-elastic mode with --gap-limit != 1).  Returns
    (status, v, s, prev, boundaries): status 1 = EXIT_FAILURE ('No valid segmentation found!')."""
    eng = engine or Engine()
    try:
        v = eng.gapped_v(MSA)
        s, prev, b = eng.gapped_dp(v)
        return (0 if b is not None else 1), v, s, prev, b
    finally:
        if engine is None:
            eng.close()


def segment(MSA, engine=None):
    """fbg.cpp:526-664 up to the boundaries.  Returns (status, v, s, prev, boundaries):
    status 0 = EXIT_SUCCESS, 1 = EXIT_FAILURE ('No proper segmentation exists.')."""
    eng = engine or Engine()
    try:
        v = eng.repeatfree_v(MSA)
        s, prev, b = eng.repeatfree_dp(v)
        return (0 if b is not None else 1), v, s, prev, b
    finally:
        if engine is None:
            eng.close()
