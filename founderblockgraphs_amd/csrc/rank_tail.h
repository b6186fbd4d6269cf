// rank_tail.h -- the candidate tail of the rank-order scan (rank_tail.hip): everything between "the scan has listed its
// candidates" and "the column maxima are raised".  The drivers in rank_scan.hip call it in a straight line:
//   rs_scan_launch (rank_scan.hip) -> rs_tail_order -> rs_tail_runs       (partitions: the runs in phase 2, fbg_rank_part_runs)
#pragma once
#include "rank_common.h"

// How the candidates get into suffix-array order, and with it which kernels work the runs (rank_tail.hip's header)
enum class RsTier { none, by_head_radix, by_head_local, by_member };

// What rs_tail_order found and decided; rs_tail_runs goes by it, the diagnostics are written from it
struct RsTail {
    uint64_t T = 0;                  // candidates
    RsTier tier = RsTier::none;      // none: no candidates, or a region overflowed
    bool overflow = false;           // a workgroup's candidate region overflowed (similar rows): the caller takes another path
    int64_t inversions = 0;          // option cand_sort_check: places of the sorted list that do not ascend
};

// The scratch the scan and its tail borrow from other stages, by what it holds here.  One cross-call contract: `sorted` and `pm`
// survive from fbg_rank_part_classify to fbg_rank_part_runs (nothing in between reserves them); everything else is dead once the
// call that filled it returns.
struct RsScratch {
    DevBuf &flat;                    // u32[T]: the candidates of all regions, unsorted (the radix sort's input)
    DevBuf &sorted;                  // u32[T]: the candidates in SA order (RankArgs::cand from rs_tail_order on)
    DevBuf &pm;                      // u32[T]: prefix minima of the forward walks (RankArgs::pm)
    DevBuf &counts;                  // u32[blocks + 1]: candidates per workgroup (RankArgs::blk_count)
    DevBuf &offsets;                 // u32[blocks + 1]: their exclusive scan
    DevBuf &tie_count;               // u32[blocks + 1]: small tie groups per workgroup (RankArgs::tie_count)
    DevBuf &pairs;                   // uint2[blocks * tie_region]: the lean scan's simple tied pairs (RankArgs::pairs)
    DevBuf &pair_count;              // u32[blocks]: ... per workgroup (RankArgs::pair_count)
};
RsScratch rs_scratch(fbg_ctx *ctx);

// Before the scan launches: the list of the big tie groups (a.big) and, without partitions, of the runs that get a wave (a.wl,
// a.wl_cap, a.runs_wave_min)
int rs_tail_prepare(fbg_ctx *ctx, RankArgs &a);
// The scan's candidates, still in the regions of its rs_blocks workgroups (a.cand, a.blk_count, a.region; lean: k_rank_scan_lean
// listed them): counts -> offsets, total and largest (fused or rocPRIM, option cand_counts_fused); picks the tier; compacts /
// sorts; orders the tie groups (k_tie_groups + k_tie_big, or k_cand_region + k_tie_big).  On return a.cand / a.pm name the sorted
// list and its scratch.  Waits for the counts on the host.
int rs_tail_order(fbg_ctx *ctx, RankArgs &a, int layout, bool lean, unsigned rs_blocks, RsTail *t, int *launches);
// The runs of the ordered candidates, by the kernels of t.tier (with the wave list where a.runs_wave_min says so)
int rs_tail_runs(fbg_ctx *ctx, RankArgs &a, int layout, const RsTail &t, int *launches);
// fbg_rank_materialize: every owned slot's tie group ordered (k_tie_groups by slot + k_tie_big exact = 1)
int rs_tail_order_all(fbg_ctx *ctx, RankArgs &a, int layout);
