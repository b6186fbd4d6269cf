"""ctypes loader of libfbg_hip.so (C ABI declared in include/fbg_hip.h).

The library is the product; there is no Python or CPU fallback.  Importing this module
without the built .so raises, and every compute call on a box without a HIP device
returns FBG_ERR_NO_DEVICE (raised as FbgError).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfbg_hip.so")

FBG_OK, FBG_ERR_INVALID, FBG_ERR_NO_SEGMENTATION, FBG_ERR_OOM, FBG_ERR_HIP, FBG_ERR_TOO_LARGE, \
    FBG_ERR_NO_DEVICE, FBG_ERR_HASH_COLLISION = range(8)
# FBG_NODE_* (include/fbg_hip.h, fbg_pindex_validate)
NODE_VALID, NODE_INVALID, NODE_SKIP_SOURCE_SINK, NODE_SKIP_IGNORED, NODE_SKIP_EMPTY = range(5)
STRAND_NONE = 0xff                           # FBG_STRAND_NONE (include/fbg_hip.h)
ALIGN_NONE = 0xffffffff                      # FBG_ALIGN_NONE
PAIR_NONE = 0xff                             # which of fbg_pindex_chains_pairs for a pair without a valid candidate
CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}     # FBG_CIGAR_*: the low four bits of a run, BAM's codes
PART_HALO = 64                               # FBG_PART_HALO (include/fbg_hip.h)
PART_HALO_BYTES = 2 * PART_HALO * 12 + 16    # FBG_PART_HALO_BYTES
STAGES = ("text", "suffix_sort", "lcp", "rank_scan", "scan", "dp", "rank_kernel", "sort_pass1", "sort_pass2", "sort_pass3")

u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)


# a numpy array as a pointer argument
def _u8(a):
    return a.ctypes.data_as(u8p)


def _u32(a):
    return a.ctypes.data_as(u32p)


def _u64(a):
    return a.ctypes.data_as(u64p)


def _sat64(x):
    """A non-negative size, band or limit as a uint64 argument: what does not fit saturates."""
    return min(int(x), 0xffffffffffffffff)


def _ignore(ignorechars):
    if isinstance(ignorechars, str):
        ignorechars = ignorechars.encode()
    ig = np.frombuffer(bytes(ignorechars or b"") + b"\0", dtype=np.uint8).copy()
    return ig, len(ig) - 1


# name -> (restype, argtypes); mirrors include/fbg_hip.h one to one
SIGNATURES = {
    "fbg_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "fbg_ctx_destroy": (None, [vp]),
    "fbg_last_error": (C.c_char_p, [vp]),
    "fbg_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
    "fbg_get_option": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_int64)]),
    "fbg_set_stream": (C.c_int, [vp, vp]),
    "fbg_stage_ms": (C.c_int, [vp, C.c_int, fp, ip]),
    "fbg_device_bytes": (C.c_uint64, [vp]),
    "fbg_release_scratch": (C.c_int, [vp]),
    "fbg_elastic_f": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u8p, C.c_uint64, C.c_int, u64p]),
    "fbg_minmax_dp": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, u64p]),
    "fbg_repeatfree_v": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p]),
    "fbg_repeatfree_dp": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, u64p]),
    "fbg_gapped_v": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p]),
    "fbg_gapped_dp": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, u64p]),
    "fbg_msa_set_device": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
    "fbg_msa_load_host": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64]),
    "fbg_msa_synthetic": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.c_uint32, C.c_uint64, C.c_uint64]),
    "fbg_index_build": (C.c_int, [vp, C.c_int, u8p, C.c_uint64]),
    "fbg_part_index_build": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int)]),
    "fbg_part_index_build_ignore": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_uint64, vp, C.POINTER(C.c_int)]),
    "fbg_part_scan": (C.c_int, [vp, vp, vp, C.POINTER(C.c_int)]),
    "fbg_part_finish": (C.c_int, [vp, vp, C.POINTER(C.c_int)]),
    "fbg_part_rescan": (C.c_int, [vp, vp]),
    "fbg_block_graph": (C.c_int, [vp, u64p, C.c_uint64, u32p, u64p, u32p, u64p, u64p]),
    "fbg_scan_f": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, vp]),
    "fbg_scan_v": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp]),
    "fbg_minmax_dp_device": (C.c_int, [vp, vp, C.c_uint64, vp, u64p, vp, vp]),
    "fbg_repeatfree_dp_device": (C.c_int, [vp, vp, C.c_uint64, vp, vp, vp, u64p]),
    "fbg_scan_gapped_v": (C.c_int, [vp, vp]),
    "fbg_gapped_dp_device": (C.c_int, [vp, vp, C.c_uint64, vp, vp, vp, u64p]),
    "fbg_text_length": (C.c_uint64, [vp]),
    "fbg_index_download": (C.c_int, [vp, u8p, u32p, u32p, u32p, u32p]),
    "fbg_sync": (C.c_int, [vp]),
    "fbg_group_create": (C.c_int, [C.c_int, ip, C.POINTER(vp)]),
    "fbg_group_destroy": (None, [vp]),
    "fbg_group_last_error": (C.c_char_p, [vp]),
    "fbg_group_size": (C.c_int, [vp]),
    "fbg_group_member": (vp, [vp, C.c_int]),
    "fbg_group_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
    "fbg_group_plan_used": (C.c_int, [vp, ip]),
    "fbg_group_elastic_f": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u8p, C.c_uint64, C.c_int, u64p]),
    "fbg_group_repeatfree_v": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p]),
    "fbg_group_gapped_v": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64, u64p]),
    "fbg_group_msa_load_host": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint64]),
    "fbg_group_msa_synthetic": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.c_uint64, C.c_uint64]),
    "fbg_group_scan_f": (C.c_int, [vp, u8p, C.c_uint64, C.c_int, C.POINTER(vp)]),
    "fbg_host_alloc": (vp, [C.c_uint64]),
    "fbg_host_free": (None, [vp]),
    "fbg_pindex_build": (C.c_int, [vp, u8p, u64p, C.c_uint64, u64p, u64p, C.POINTER(vp)]),
    "fbg_pindex_locate": (C.c_int, [vp, u8p, u64p, C.c_uint64, u64p, u64p]),
    "fbg_pindex_text_length": (C.c_uint64, [vp]),
    "fbg_pindex_download": (C.c_int, [vp, u8p, u32p, u32p, u32p, u64p, u64p]),
    "fbg_pindex_stats": (C.c_int, [vp, u64p, C.POINTER(C.c_double), C.POINTER(C.c_double), u64p]),
    "fbg_pindex_destroy": (None, [vp]),
    "fbg_pindex_validate": (C.c_int, [vp, u32p, u8p, C.c_uint64, u8p, u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_validate_stats": (C.c_int, [vp, u64p, u64p, u64p]),
    "fbg_pindex_occurrences": (C.c_int, [vp, u8p, u64p, C.c_uint64, C.c_uint64, u64p, u64p, u32p, u64p, u64p, u64p, u64p,
                                         C.POINTER(C.c_double)]),
    "fbg_pindex_occurrences_fetch": (C.c_int, [vp, u32p, u32p, u32p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_seeds": (C.c_int, [vp, u8p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_seeds_fetch": (C.c_int, [vp, u32p, u32p, u64p, u32p, u64p, u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_seeds_places": (C.c_int, [vp, u32p, u32p, u32p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_build_segmentation": (C.c_int, [vp, u64p, C.c_uint64, C.POINTER(vp)]),
    "fbg_pindex_node_count": (C.c_uint64, [vp]),
    "fbg_pindex_node_info": (C.c_int, [vp, u32p, u32p, u64p]),
    "fbg_pindex_occurrences_msa": (C.c_int, [vp, u32p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_seeds_msa": (C.c_int, [vp, u32p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_msa_stats": (C.c_int, [vp, u64p, u64p, u64p]),
    "fbg_pindex_chains": (C.c_int, [vp, C.c_uint64, C.c_uint64, u64p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_fetch": (C.c_int, [vp, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_chain_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_build_segmentation_rows": (C.c_int, [vp, u64p, C.c_uint64, C.POINTER(vp)]),
    "fbg_pindex_seeds_rows": (C.c_int, [vp, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_rows": (C.c_int, [vp, u32p, u32p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_rows_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_by_row": (C.c_int, [vp, C.c_uint64, C.c_uint64, u64p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_by_row_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_align": (C.c_int, [vp, C.c_uint64, C.c_uint64, u32p, u32p, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_align_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_cigar": (C.c_int, [vp, u32p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_cigar_fetch": (C.c_int, [vp, u64p, u32p]),
    "fbg_pindex_cigar_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_align_graph": (C.c_int, [vp, C.c_uint64, C.c_uint64, u8p, u32p, u32p, u32p, u32p, u32p, u32p, u64p,
                                                C.POINTER(C.c_double)]),
    "fbg_pindex_chains_align_graph_fetch": (C.c_int, [vp, u64p, u32p]),
    "fbg_pindex_align_graph_stats": (C.c_int, [vp] + [u64p] * 10),
    "fbg_pindex_chains_graph_cigar": (C.c_int, [vp, u32p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_graph_cigar_fetch": (C.c_int, [vp, u64p, u32p]),
    "fbg_pindex_graph_cigar_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_mapq": (C.c_int, [vp, C.c_uint64, u64p, u32p, u32p, u32p, u8p, C.POINTER(C.c_double)]),
    "fbg_pindex_chains_mapq_fetch": (C.c_int, [vp, u32p, u32p, C.POINTER(C.c_double)]),
    "fbg_pindex_mapq_strands": (C.c_int, [vp, u8p, C.POINTER(C.c_double)]),
    "fbg_pindex_mapq_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
    "fbg_pindex_chains_pairs": (C.c_int, [vp, C.c_uint64, C.c_uint64, u8p, u32p, u32p, u32p, u64p, u32p, u32p, u32p, u32p, u32p,
                                          u64p, u32p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_pairs_align": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, u8p, u32p, u32p, u32p, u32p, u32p, u8p, u32p,
                                         u32p, u32p, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_seeds_strands": (C.c_int, [vp, u8p, u64p, C.c_uint64, u8p, C.c_uint64, C.c_uint64, u64p, C.POINTER(C.c_double)]),
    "fbg_pindex_chain_strands": (C.c_int, [vp, u8p, u32p, u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "fbg_segmentation_validate": (C.c_int, [vp, u64p, C.c_uint64, u8p, C.c_uint64, u8p, u64p, u64p, C.POINTER(C.c_double)]),
    "fbg_segmentation_repair": (C.c_int, [vp, u64p, u64p, u8p, C.c_uint64, u64p, u64p, C.POINTER(C.c_double)]),
}
PLANS = ("auto", "partitioned", "columns", "row_pairs")   # FBG_PLAN_*

_LIB = None


def build():
    """Compile the HIP sources in csrc/ for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C founderblockgraphs_amd/csrc` "
                              "(or __graft_entry__.build()); there is no fallback path")
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 and a
        # process that loads both that copy and /opt/rocm's ends up with torch seeing no GPU.
        # Loading torch first makes the dynamic loader hand the same (already loaded) runtime to
        # libfbg_hip.so.  The C++ host program never loads torch and uses /opt/rocm's runtime.
        if os.environ.get("FBG_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = header / library mismatch
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB
