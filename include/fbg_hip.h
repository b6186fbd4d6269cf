/*
 * fbg_hip.h -- C ABI of libfbg_hip.so, the MI355X (gfx950) segmentation engine.
 *
 * The reference (algbio/founderblockgraphs, founderblockgraph.cpp = "fbg.cpp") has no FFI
 * or plugin seam; the hot path sits behind two in-process C++ calls made from main():
 *
 *   segment_elastic_minmaxlength(MSA, cst, ignorechars, out_indices, disable_efg_tricks, f)
 *                                             fbg.cpp:1836-1844, called at fbg.cpp:3393
 *   segment(MSA, cst, out_labels, out_edges)  fbg.cpp:526-531,   called at fbg.cpp:3437
 *
 * together with the index they consume (load_cst, fbg.cpp:361-436).  The entry points
 * below are what a maintainer binds instead of those calls (INTEGRATION.md shows the
 * patch).  Everything is plain C: pointers + sizes, int status codes, caller-owned
 * buffers, one opaque context, calls on one context serialised by the caller.  All
 * column/row/boundary values are uint64_t because the reference's size_type is
 * (fbg.cpp:47).
 *
 * Limits of this build: one context indexes texts of N = (#non-gap cells) + m + 1 < 2^32 symbols (32-bit suffix
 * ranks); longer texts (below 2^40) go through a group (fbg_group_*, partitioned index); n < 2^31.  Violations return
 * FBG_ERR_TOO_LARGE.
 * There is no CPU fallback: without a HIP device every compute call fails with
 * FBG_ERR_NO_DEVICE / FBG_ERR_HIP.
 */
#ifndef FBG_HIP_H
#define FBG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fbg_ctx fbg_ctx;

enum {
    FBG_OK = 0,
    FBG_ERR_INVALID = 1,         /* bad argument / call order */
    FBG_ERR_NO_SEGMENTATION = 2, /* "No valid segmentation found!" fbg.cpp:1932-1937,
                                    "No proper segmentation exists." fbg.cpp:648-652 */
    FBG_ERR_OOM = 3,
    FBG_ERR_HIP = 4,             /* a HIP runtime call or kernel failed; see fbg_last_error */
    FBG_ERR_TOO_LARGE = 5,
    FBG_ERR_NO_DEVICE = 6,
    FBG_ERR_HASH_COLLISION = 7   /* fbg_block_graph only: use the caller's own label numbering instead */
};

#define FBG_MAX_ROWS 32768  /* fbg_block_graph only: a workgroup groups the labels of a block -- in LDS up to 4096 rows, in a
                               stretch of device memory of its own beyond (exercised at 5000 rows; at this limit 512 workgroups
                               hold 0.4 GB of such stretches and sort 32768 pairs each per block in device memory).  More rows:
                               FBG_ERR_TOO_LARGE, number the labels on the host.  The segmentation itself has no row limit. */

/* stage ids for fbg_stage_ms() */
enum {
    FBG_STAGE_TEXT = 0,      /* MSA -> gap-stripped text + per-row tables (fbg.cpp:372-386,1845-1917) */
    FBG_STAGE_SUFFIX_SORT,   /* suffix array + inverse (sdsl::construct, fbg.cpp:428) */
    FBG_STAGE_LCP,           /* per-position LCP with SA predecessor / successor */
    FBG_STAGE_TILE,          /* rank-order extension scan (gap-free MSAs; runs inside fbg_index_build; its time
                                is also contained in FBG_STAGE_SUFFIX_SORT) */
    FBG_STAGE_SCAN,          /* compute_f / v[] column scan (fbg.cpp:1579-1695, 552-611) */
    FBG_STAGE_DP,            /* bucket pass + DP sweep + backtrack (fbg.cpp:1940-2039, 616-664) */
    FBG_STAGE_RANK_KERNEL,   /* the k_rank_scan / k_rank_scan_lean launch alone (1 launch), for roofline accounting */
    FBG_STAGE_SORT_PASS1,    /* the three kernels of the MSD sort alone, one launch each (k_msd_pack_split, k_msd_split, */
    FBG_STAGE_SORT_PASS2,    /* k_msd_finish), for roofline accounting; 0 launches when another sort ran                */
    FBG_STAGE_SORT_PASS3,
    FBG_STAGE_COUNT
};

/* ---- context ------------------------------------------------------------------------ */
int fbg_ctx_create(int device, fbg_ctx **out);
void fbg_ctx_destroy(fbg_ctx *ctx);
/* Message of the last failing call on this context ("" if none). ctx may be NULL after a
 * failed fbg_ctx_create, in which case a process-wide message is returned. */
const char *fbg_last_error(const fbg_ctx *ctx);
/*
 * Behaviour switches of one context (integers; 0 = default unless stated).  They select between code paths that all
 * give the same results -- tests use them to reach every path; the environment has no influence on the library
 * unless FBG_DEBUG_ENV=1 is set, in which case FBG_<KEY IN CAPITALS>=<integer> presets new contexts.
 *   no_ranked          gap-free MSAs take the record path (text-order scan) instead of the rank-order scan
 *   no_packed, force_wide, full_keys   slot layout / key length of the round-0 sort
 *   no_msd_sort        rocPRIM radix sort instead of the three-pass MSD sort
 *   msd_min, bp_min    text lengths from which the MSD sort / the records-by-position passes are used (-1 = 2^24)
 *   record_scatter     records reach text order by a scatter instead of the by-position passes
 *   lcp_text           neighbour LCPs by text comparison even when the keys would do
 *   pure_scan          1: gap-free MSAs always take the group-level scan for similar rows (pure_scan.hip), -1: never
 *   no_aux_stream      k_tie_simple on the main stream
 *   rank_no_threshold  no extension threshold in the rank-order scan
 *   dp_literal, dp_wave, dp_tile, dp_safe_window   which sweep kernel runs the min-max-length / non-elastic DP
 *   gapped_rank        -1: MSAs with gaps / ignore characters always take the record path (no scan in suffix order)
 *   part_tricks_off    1: the partitioned index of an MSA with gaps / ignore characters is scanned without the elastic tricks
 *   msd_min_force      1: the sample sort of (key, position) pairs also for rows that resemble each other (tests)
 *   msd_sample_bins    1: the finish of the sample sort bins by sampled keys instead of symbol ranks (the earlier method, kept for tests)
 *   gapped_rank also takes 2 (no flag bits in the sort's values), 3 (flag bits, no threshold), 4 (threshold forced: tests)
 *   msd_probe          1: the finish of the sample sort (k_pp_finish) also runs in timing variants (copy only, single phases) before
 *                      the real launch -- for a kernel trace read in launch order (scripts/gpu_trace_order.sh); results
 *                      unchanged.  (The three-pass MSD sort had such variants in round 3: profiles/r03_msd_probe_order.txt)
 *   no_stream_upload   1: fbg_elastic_f copies the whole MSA to the device before the index build starts, also from memory of
 *                      fbg_host_alloc (default: the rows go up in eight chunks while the text is written and pass 1 of the MSD sort
 *                      runs on the rows that are there; results unchanged)
 *   rows_wave          1: fbg_pindex_seeds_rows / _chains_rows give every start place / chain a whole wave also when the MSA
 *                      has at most 16 rows (default: 16 lanes each then); results unchanged (tests, measurements)
 *   rank_no_lean       1: the rank-order scan with k_rank_scan also where its lean form (k_rank_scan_lean: packed slots, threshold
 *                      above the key length) applies; results unchanged
 *   msd_ext            0: the three-pass MSD sort carries no symbols beyond the key (default 1: with 2-bit symbols its words
 *                      carry the 4 symbols after the key, pass 3 writes them out as one byte per slot, and the rank-order
 *                      scan settles most tied pairs from them instead of reading the text); results unchanged
 *   msd_xcd            which passes of the MSD sort place their writes by XCD (-1 = 3): bit 0 pass 2 (the tiles of a bucket
 *                      go to the workgroups of one XCD), bit 1 pass 1 (a stretch per bucket and XCD); 0: neither (the
 *                      layout of rounds 1-3); results unchanged
 *   span_scan          MSAs with gaps / ignore characters whose rows resemble each other take the group-level scan on
 *                      column spans (span_scan.hip); 1: every such MSA takes it, -1: none, 2: as 0, and the sorted slots
 *                      are checked to be the cells in key order (debugging), 3: as 1, with the groups of more than 1024
 *                      members worked off by chains along the later keys' groups (the earlier method, kept for tests)
 *   span_key_flags     1: that scan's slot layout for MSAs of 2^30 cells and more (the two flags of a slot in the key word,
 *                      the cell alone in the value) whatever the size (tests); results unchanged
 *   poison             1 .. 255: every device buffer the context allocates from now on is filled with that byte first
 *                      (debugging aid: reads of memory nobody wrote show up in a fresh process too); results unchanged
 *   dpw_matrix         1: the sweep over windows of 1024 .. 16384 columns with one 128 x window matrix per block (the method of
 *                      rounds 2-3: k_dpw_blockM / k_dpw_chain) instead of the matrix of the 128 columns before a block and the
 *                      closed form for the older ones (k_dpw_blockY / k_dpw_chain2); results unchanged
 *   dp_chain1          1: the walk over the groups of byte matrices on one wave (k_dp_chain, rounds 1-3) instead of six
 *                      (k_dp_chain6); results unchanged
 *   pairs_in_scan      0: the lean rank-order scan hands every simple tied pair to k_tie_pairs (default 1: a pair whose msd_ext
 *                      code says where it parts, 255 in 256, is settled inside the scan kernel; k_tie_pairs takes the rest);
 *                      results, "ext_pairs" and "text_pairs" unchanged
 *   runs_wave_min      the rank-order scan without partitions: a run of same-column slots with this many members and more is
 *                      walked by a wave (k_runs_long) instead of its head's thread (default 16; 0: none is); results unchanged
 *   wave_list_cap      entries the list of such runs holds (0 = 1024, the most); a run that finds the list full stays with
 *                      its thread (tests)
 *   cand_local_sort    0: the candidate list of the rank-order scan always goes through the device-wide radix sort (default 1:
 *                      after the lean scan every workgroup's region is sorted in LDS on its way into the list, where the
 *                      largest region fits); results unchanged
 *   cand_lds_cap       the largest region count that sort takes (0 = 4096, the most; tests)
 *   cand_sort_check    1: the sorted candidate list is checked to ascend ("cand_inversions"; debugging, one more wait)
 *   cand_tail          0: behind the lean scan the sorted regions, their tie groups and the same-column runs are worked by the
 *                      kernels that give a thread to every group's and every run's head (k_cand_sort_compact, k_tie_groups,
 *                      k_runs, k_runs_long).  Default 1, where the regions are sorted in LDS (cand_local_sort): one kernel per
 *                      region sorts it, keeps the candidates' words in LDS and orders the tie groups it heads (k_cand_region);
 *                      every neighbour LCP of a candidate is computed once, by candidate (k_cand_lcp), and the runs' heads take
 *                      their minima over those arrays (k_cand_runs, k_cand_runs_long); results unchanged ("cand_tail_used")
 *   tie_gallop         0: k_tie_groups counts the members of a tie group one by one (default 1: 8 slots one by one, then
 *                      doubling steps and bisection on the sorted keys, tie_extent.h); results unchanged
 *   cand_counts_fused  0: the candidate counts of the rank-order scan's workgroups go through rocPRIM's scan and reduce and two
 *                      copies (default 1: one kernel of one workgroup writes their offsets, their total and the largest, one
 *                      copy brings the two to the host); results unchanged
 *   tie_sample_loop    0: the sample of the sorted keys before the rank-order scan (k_tie_sample) takes one workgroup per
 *                      cluster of 256 slots (default 1: 512 workgroups walk the clusters and add their counts to global memory
 *                      once each; n > 1: n workgroups, tests); same slots, same sums, same threshold and verdict
 *   row_count_fast     0: the counting pass over a gap-free candidate MSA whose rows start at multiples of 8 bytes (k_row_count,
 *                      which also writes the optimistic text) takes 8 bytes per lane and load and tests every word against
 *                      six candidate symbols with 64-bit arithmetic (default 1: k_row_count_fast -- 16 bytes per lane, load and
 *                      store, only the candidates the segment's first 64 bytes showed, three instructions per 32-bit word and
 *                      candidate while all bytes are below 128 and in the guess); same counts, same text
 *   twin_hash          0: the twins among the 2^20 sampled keys before the sort are counted by sorting the sample (rocPRIM,
 *                      22 launches) and the host waits for the count (default 1: one kernel puts the keys into an
 *                      open-addressing table, twin_hash.h, and the count is read behind the sort); same count ("sample_twins")
 *   front_one_fill     0: the counting pass's row totals, byte histogram and counts are cleared by three fills, come back by two
 *                      copies, one of them staged, and the text's sentinel is written after the wait (default 1: one fill, one
 *                      copy into pinned words, the sentinel of a gap-free candidate in front of the counting pass); results unchanged
 *   scan_rows_ahead    the rows of 64 slots whose loads a wave of the lean rank-order scan (k_rank_scan_lean) keeps in flight
 *                      while it works on a row: 1 = one row ahead; 2, 3, 4 = groups of that many rows, the next group's loads
 *                      issued at the top of a group; 0 and any other value = the default, 3; results unchanged
 *   msd_cursors        where pass 1 of the MSD sorts keeps the run cursor of stretch (bucket d, XCD part q of xs, msd_xcd bit 1):
 *                      1 (default) at q * 512 + d, so that the 64 lanes of a reserving wave add to consecutive words; 0 at
 *                      d * xs + q, the stretch's own number (the earlier placement); the words are as wide either way (32 bits
 *                      for texts below 2^32 symbols); results unchanged
 *   msd_lds_batch      0: pass 1 of the three-pass MSD sort takes a thread's 8 items one after the other through LDS, every read
 *                      awaited alone (the earlier loops; default 1: in phases -- the reads of all items, then their use -- with
 *                      the text loads issued before the code table is published and the tiles inside the text translated
 *                      without end-of-text checks; 2: as 1, every tile with the checks, measurements); results unchanged
 *   span_slow_split    workgroups that share the odd members of one large group whose pairs are all compared (0 = 32);
 *                      results unchanged
 *   path_batch_kib     fbg_pindex_chains_cigar and _chains_graph_cigar: the KiB of column history in device memory that
 *                      one batch of reads longer than 256 symbols may take (default 2^20, 1 GiB; values below 1 count as
 *                      1); a read whose own history is larger is a batch of its own; results unchanged
 *   byrow_max          fbg_pindex_chains_by_row: the most start places of a read that is still chained (default 1024;
 *                      negative values count as 0); a read with more gets no row and no chain and is counted
 *   byrow_lds          fbg_pindex_chains_by_row: 0 (default) keeps the state of reads of up to lds_max start places in LDS,
 *                      a positive value below lds_max lowers that limit (larger ones clamp), -1 sends every read to the
 *                      tier with its state in device memory; results unchanged
 *   graph_batch_kib    fbg_pindex_chains_align_graph: the KiB of node columns in device memory that one batch of reads may
 *                      take (default 2^20, 1 GiB, as path_batch_kib: a bound on the scratch that still leaves batches of
 *                      10^5 reads of a few hundred symbols on a dozen founders; values below 1 count as 1); a read whose own
 *                      columns are larger is a batch of its own; results unchanged
 * fbg_get_option also answers "index_kind" (read-only): -1 no index, 0 per-position records, 1 rank-order scan of a
 * gap-free MSA, 2 scan in suffix order of an MSA with gaps / ignore characters (slot by slot, or -- "span_scan_used" = 1 --
 * group by group), 3 one partition of a partitioned index.  "span_groups", "span_odd_groups", "span_irregular",
 * "span_scan_work" (read-only): the group-level scan's table sizes and the text comparisons it expected;
 * "alloc_calls", "alloc_us" (read-only): device buffers the context has allocated or enlarged so far, and the host time
 * that took in microseconds (hipFree + hipMalloc).
 * "span_decline" (read-only): why the group-level scan handed the last build to the record path: 0 it did not, 1 / 3 / 5 /
 * 6 / 8 / 9 a list or table of its kernels was full, 2 more than 32 text comparisons per suffix ahead, 4 / 7 too many groups
 * that need every pair of members compared, 10 an ignore character it cannot express;
 * "span_key_flags_used" (read-only): 1 when the slots at hand have that scan's layout for 2^30 cells and more.
 * "dp_kind" (read-only): the sweep that produced the last fbg_minmax_dp result: -1 none yet, 0 statement by statement,
 * 1 matrix chain with byte entries (windows up to 256 columns), 2 wave-parallel sweep, 3 .. 7 matrix chain with 16-bit
 * entries over windows of 1024 / 2048 / 4096 / 8192 / 16384 columns.
 * "dp_attempts" (read-only): the sweeps the last fbg_minmax_dp launched until one settled: every window it tried, and the
 * statement-by-statement sweep when that ran (1 when the first choice held; 0 before the first call or after a refusal).
 * "ne_dp_kind" (read-only): what produced the last fbg_repeatfree_dp result: -1 none yet, 0 the statement-by-statement
 * kernel, chosen up front (dp_literal, or a minimal block of more than 126 columns), 1 / 2 / 4 the matrix chain over
 * windows of 64 / 128 / 256 columns, 8 the matrix chain met a value its window does not hold and the statement-by-
 * statement kernel redid the input.
 * "msd_decline" (read-only): the three-pass MSD sort of the last index build: -1 not reached, 0 it sorted the slots, 1 the
 * geometry did not suit it (rocPRIM sorted), else the capacity that did not hold (2 / 4 a stretch of pass 1, 8 the arena
 * of pass 2, 16 a sub-bucket beyond the largest finish).  "pass1_ahead" (read-only): 1 when that sort found its pass 1 done
 * during a streamed upload (fbg_elastic_f from memory of fbg_host_alloc).
 * "ext_pairs", "text_pairs" (read-only): the tied pairs the lean rank-order scan of the last index build settled from the
 * MSD sort's symbols after the key (msd_ext) / by comparing the text; -1 when no rank-order scan ran, both 0 when it ran
 * without its lean form.
 * "sample_twins" (read-only): the twins among the keys of the sample drawn before the sort of the last index build (texts
 * of 2^22 symbols and more: 2^20 keys minus the distinct ones among them); -1 when no sample was drawn.
 * "cand_inversions" (read-only): with cand_sort_check, the places of the last scan's sorted candidate list whose successor
 * is not larger (0 also when the scan had no list to sort); -1 without the option.  "cand_local_sorted" (read-only): 1 when
 * that list was sorted region by region, 0 by the radix sort, -1 when no list was sorted.
 * "cand_tail_used" (read-only): 1 when the last rank-order scan worked its candidates by member (option cand_tail), 0 when
 * it ran the kernels by head (the option off, no lean scan, a region above the LDS capacity, partitions, no candidates);
 * -1 when no rank-order scan ran.
 * "wave_runs" (read-only): the runs of the last rank-order scan that a wave each walked; -1 when no rank-order scan
 * finished.
 * "rank_lean_launched" (read-only): 1 when the last rank-order scan launched its lean form (k_rank_scan_lean), whether or
 * not the scan then finished; "rank_lean_used" (read-only): 1 when it also finished, so that the index holds that kernel's
 * column maxima (0 when the scan handed over to the group-level scan or the record path).
 * "pairs_rb" (read-only): the sample sort of (key, position) pairs of the last index build (msd_sort_pairs.hip): -1 it did
 * not sort (not reached, or declined to rocPRIM), else the rank bits of its table of frequent symbols (0: no table, 1 .. 3:
 * 2 / 4 / 8 frequent symbols, entries of 2 bits for 1 .. 2, of 4 bits for 3).
 * "key_b", "key_K", "key_packed", "key_compact" (read-only): the key geometry of the last key setup (suffix_sort.hip
 * fbg_key_setup): bits per symbol, symbols per key, 1 when a key and its position share one 64-bit word, 1 when the
 * separator-free coding of the rank-order scans applies (no byte below '#' in the rows, fewer than 128 distinct symbols);
 * -1 before the first index build.
 * Unknown key: FBG_ERR_INVALID.
 */
int fbg_set_option(fbg_ctx *ctx, const char *key, int64_t value);
int fbg_get_option(const fbg_ctx *ctx, const char *key, int64_t *value);
/* Run all work of this context on an existing hipStream_t (NULL = the context's own). */
int fbg_set_stream(fbg_ctx *ctx, void *hip_stream);
/* Device time of a stage during the most recent call that ran it, in ms (HIP events on the
 * context's stream); launches = number of kernel launches the figure covers. */
int fbg_stage_ms(fbg_ctx *ctx, int stage, float *ms, int *launches);
/* Bytes of device memory currently held by the context's workspaces. */
uint64_t fbg_device_bytes(const fbg_ctx *ctx);
/* Free the suffix-sort / DP scratch buffers (the index itself stays valid).  Called automatically
 * after the suffix sort when the text is longer than 1.5e9 symbols, so that a 4e9-symbol index
 * fits the 288 GB of one MI355X. */
int fbg_release_scratch(fbg_ctx *ctx);

/* ---- host-buffer entry points (what main() of the C++ host calls) -------------------- */

/*
 * Replaces load_cst + compute_f (fbg.cpp:361-436, 1845-1923).  msa: m rows of n bytes,
 * row-major, '-' = gap, any other byte is a symbol.  f[0..n) is MAX-MERGED into, exactly as
 * the reference does (fbg.cpp:1681; main() zero-fills it, fbg.cpp:3388).
 * Returns FBG_ERR_NO_SEGMENTATION iff disable_tricks && f[0] == n (fbg.cpp:1932-1937); f is
 * still written in that case.
 */
int fbg_elastic_f(fbg_ctx *ctx, const uint8_t *msa, uint64_t m, uint64_t n,
                  const uint8_t *ignore_chars, uint64_t ignore_len, int disable_tricks,
                  uint64_t *f);

/*
 * Replaces the sort + DP + backtrack of segment_elastic_minmaxlength (fbg.cpp:1940-2039).
 * boundaries_out: room for n+1 values; *count_out receives the number of blocks.  The last
 * boundary is n (fbg.cpp:2027-2028).  minmaxlength_out / backtrack_out (n+1 values each) may
 * be NULL.  FBG_ERR_NO_SEGMENTATION where the reference would index backtrack[] out of range
 * (only reachable with --disable-elastic-tricks).
 * Device scratch: 64-128 bytes per column; with extensions f[x] - x beyond 254 columns up to 2 * 4096 bytes per column
 * (at most 16 GB) for the 16-bit matrices -- taken only when the device has the room, the statement-by-statement sweep
 * runs otherwise; both give the reference's arrays.
 */
int fbg_minmax_dp(fbg_ctx *ctx, const uint64_t *f, uint64_t n, uint64_t *boundaries_out,
                  uint64_t *count_out, uint64_t *minmaxlength_out, uint64_t *backtrack_out);

/*
 * Replaces load_cst + the v[j] scan of segment() (fbg.cpp:552-611).  Rows must be gap-free
 * (the reference only reaches segment() with --gap-limit=1, which drops rows with gaps,
 * fbg.cpp:176-177, 3436-3437); a gap returns FBG_ERR_INVALID.  v[0..n) is overwritten.
 */
int fbg_repeatfree_v(fbg_ctx *ctx, const uint8_t *msa, uint64_t m, uint64_t n, uint64_t *v);

/*
 * Replaces the s[]/prev[] DP and backtrack of segment() (fbg.cpp:616-664).  s_out, prev_out:
 * n values each (may be NULL); boundaries_out: room for n values, last one is n-1.
 * FBG_ERR_NO_SEGMENTATION iff s[n-1] == n+1 (fbg.cpp:648-652); s/prev are still written.
 */
int fbg_repeatfree_dp(fbg_ctx *ctx, const uint64_t *v, uint64_t n, uint64_t *s_out,
                      uint64_t *prev_out, uint64_t *boundaries_out, uint64_t *count_out);

/*
 * Replaces load_cst + the v[j] scan of segment2elasticValid (fbg.cpp:763-822), the non-elastic
 * mode for --gap-limit != 1: rows may hold gaps.  v[j] = largest jp such that the gap-stripped
 * strings of block [jp..j] occur nowhere but at the m aligned places, j+1 if there is none
 * (fbg.cpp:764, 805-807).  v[0..n) is overwritten.
 */
int fbg_gapped_v(fbg_ctx *ctx, const uint8_t *msa, uint64_t m, uint64_t n, uint64_t *v);

/*
 * Replaces the s[]/prev[] recurrence and backtrack of segment2elasticValid (fbg.cpp:827-866),
 * a heuristic (new block at v[j], or the previous column's solution with its last block
 * extended), reproduced with the reference's unsigned wrap-around; s[0] = prev[0] = n+1 always
 * (the loop starts at 1).  s_out, prev_out: n values each (may be NULL); boundaries_out: room
 * for n values, last one is n-1.  FBG_ERR_NO_SEGMENTATION iff s[n-1] == n+1 (fbg.cpp:850-854);
 * s/prev are still written.
 */
int fbg_gapped_dp(fbg_ctx *ctx, const uint64_t *v, uint64_t n, uint64_t *s_out,
                  uint64_t *prev_out, uint64_t *boundaries_out, uint64_t *count_out);

/* ---- device-resident staged API (bench, multi-GPU column shards) --------------------- */

/* Borrow an MSA already resident in device memory (row-major m x n bytes). */
int fbg_msa_set_device(fbg_ctx *ctx, const uint8_t *d_msa, uint64_t m, uint64_t n);
/* Copy a host MSA into a context-owned device buffer. */
int fbg_msa_load_host(fbg_ctx *ctx, const uint8_t *msa, uint64_t m, uint64_t n);
/*
 * Fill a device buffer with the synthetic MSA of SURVEY.md section 8(d):
 *   cell(i,j) = "ACGT"[splitmix64(seed + i*n + j) >> 62];
 *   gap_run_len > 0: cell (i,j) starts a run of gap_run_len '-' iff
 *                    splitmix64(seed2 + i*n + j) < gap_start_threshold;
 *   n_threshold > 0: a non-gap cell becomes 'N' iff splitmix64(seed3 + i*n + j) < n_threshold.
 */
int fbg_msa_synthetic(fbg_ctx *ctx, uint8_t *d_msa, uint64_t m, uint64_t n, uint64_t seed,
                      uint64_t seed2, uint64_t gap_start_threshold, uint32_t gap_run_len,
                      uint64_t seed3, uint64_t n_threshold);
/*
 * Build the index of the current MSA: text, suffix array, inverse, neighbour LCPs, and the
 * column-tiled tables the scan reads.  reversed = 0 for the elastic scan, 1 for the
 * non-elastic v[] scan (rows written back to front).  ignore_chars only matter for
 * reversed = 0.  Every rank of a multi-GPU job builds the same index (replicas).
 */
int fbg_index_build(fbg_ctx *ctx, int reversed, const uint8_t *ignore_chars, uint64_t ignore_len);
/*
 * Partitioned index for multi-GPU jobs (gap-free MSAs without ignore characters; the only path that accepts texts of
 * 2^32 symbols and more, elastic scan): every rank holds the same
 * MSA, but sorts and scans only the suffixes of key range `part` of `nparts`, so index memory and sort time
 * divide by the number of GPUs.  The caller moves two small things between the ranks:
 *
 *   fbg_part_index_build   text, splitters (identical on every rank), local sort, local classification;
 *                          d_blob (FBG_PART_HALO_BYTES, device) receives this partition's edge slots
 *       -> all-gather the blobs of all ranks, in rank order, into d_blobs (nparts * FBG_PART_HALO_BYTES)
 *   fbg_part_scan          halos in, runs walked; d_gmax (n + 1 words, device) receives the per-column maxima
 *                          of this partition's suffixes, word n its verdict
 *       -> all-reduce(MAX) d_gmax over the ranks
 *   fbg_part_finish        takes the reduced maxima; afterwards fbg_scan_f / fbg_scan_v work as after
 *                          fbg_index_build.  *ok = 2 (the same on every rank): the scan used a threshold that a few
 *                          columns did not clear -- call fbg_part_rescan (maxima without threshold into d_gmax),
 *                          all-reduce(MAX) once more and call fbg_part_finish again.
 *
 * *ok = 0 (from any of the three; the same value on every rank after the collective that follows) means the
 * input does not suit this path (similar rows, long runs): fall back to fbg_index_build on every rank.
 * Replaces the same reference code as fbg_index_build + fbg_scan_f (fbg.cpp:428, 1610-1694).
 */
#define FBG_PART_HALO 64
#define FBG_PART_HALO_BYTES (2 * FBG_PART_HALO * 12 + 16)
int fbg_part_index_build(fbg_ctx *ctx, int reversed, int part, int nparts, void *d_blob, int *ok);
/* The same for MSAs with gaps and / or ignore characters (texts below 2^32 symbols, elastic scan): the partitions are
 * scanned in suffix order like the whole index of such an MSA (gapped_rank.hip).  The scan of fbg_part_scan is for one
 * setting of the elastic tricks -- option part_tricks_off, read at fbg_part_index_build -- and fbg_scan_f must ask for
 * that one.  ignore_chars = NULL, ignore_len = 0: fbg_part_index_build. */
int fbg_part_index_build_ignore(fbg_ctx *ctx, int reversed, int part, int nparts, const uint8_t *ignore_chars, uint64_t ignore_len,
                                void *d_blob, int *ok);
int fbg_part_scan(fbg_ctx *ctx, const void *d_blobs, uint32_t *d_gmax, int *ok);
int fbg_part_finish(fbg_ctx *ctx, const uint32_t *d_gmax, int *ok);
int fbg_part_rescan(fbg_ctx *ctx, uint32_t *d_gmax);
/* Columns [x0, x1) of f, max-merged into d_f[x0..x1) (d_f has n entries, device memory). */
int fbg_scan_f(fbg_ctx *ctx, uint64_t x0, uint64_t x1, int disable_tricks, uint64_t *d_f);
/* Columns [x0, x1) of v, written to d_v[x0..x1). Requires fbg_index_build(reversed = 1). */
int fbg_scan_v(fbg_ctx *ctx, uint64_t x0, uint64_t x1, uint64_t *d_v);
/* DP + backtrack on device arrays; boundaries land in d_boundaries (n+1 values), count on host.
 * d_mml / d_bt (n+1 values each) may be NULL. */
int fbg_minmax_dp_device(fbg_ctx *ctx, const uint64_t *d_f, uint64_t n, uint64_t *d_boundaries,
                         uint64_t *count_out, uint64_t *d_mml, uint64_t *d_bt);
int fbg_repeatfree_dp_device(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s,
                             uint64_t *d_prev, uint64_t *d_boundaries, uint64_t *count_out);
/* v[] of segment2elasticValid (fbg.cpp:763-822) for all n columns into d_v (device).  Requires
 * fbg_index_build(reversed = 0) or a finished partitioned index, without ignore characters. */
int fbg_scan_gapped_v(fbg_ctx *ctx, uint64_t *d_v);
int fbg_gapped_dp_device(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s,
                         uint64_t *d_prev, uint64_t *d_boundaries, uint64_t *count_out);
/*
 * Nodes and edges of the elastic founder graph for a segmentation of the current MSA (the one last given to
 * fbg_elastic_f / fbg_msa_load_host / fbg_msa_set_device): what output_efg computes by hashing the gap-stripped
 * label of every (row, block) twice (fbg.cpp:1210-1260).  boundaries[nb] as produced by fbg_minmax_dp (block j covers
 * columns boundaries[j-1]+1 .. boundaries[j], the last entry is n).  All outputs are host buffers:
 *   node_of[j*m + i]     node of row i in block j in the reference's numbering (blocks in order, within a block by
 *                        first appearance in row order, fbg.cpp:1232-1246); 0xffffffff = the row has only gaps there
 *   first_node[nb + 1]   first node of every block; first_node[j+1] - first_node[j] = entry j of the B line
 *   rep_row[j*m + k]     the row whose label defines node first_node[j] + k (its S line)
 *   edge_count[nb], edges[j*m + e]   the L lines into block j: src << 32 | dst, ascending (std::set order,
 *                        fbg.cpp:1230,1253), e < edge_count[j]; edge_count[0] = 0
 * Exact: rows grouped by a 128-bit hash are compared byte by byte with their group's first row; should two different
 * labels ever collide the call returns FBG_ERR_HASH_COLLISION and the caller numbers the labels itself.
 */
int fbg_block_graph(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, uint32_t *node_of, uint64_t *first_node,
                    uint32_t *rep_row, uint64_t *edge_count, uint64_t *edges);
/* Copy out index arrays for tests: any pointer may be NULL. Host buffers of N entries
 * (N from fbg_text_length). SA / ISA / LCP-with-predecessor / LCP-with-successor by text position. */
uint64_t fbg_text_length(const fbg_ctx *ctx);
int fbg_index_download(fbg_ctx *ctx, uint8_t *text, uint32_t *sa, uint32_t *isa,
                       uint32_t *lcp_prev, uint32_t *lcp_next);
/* Block until all work queued on the context's stream has finished. */
int fbg_sync(fbg_ctx *ctx);

/* ---- several GPUs as one engine (fbg_ctx_create(ndev, dev_ids); 8e) --------------------------------
 *
 * Replaces the std::thread fan-out of segment_elastic_minmaxlength_multithread (fbg.cpp:2180-2289): a group holds one
 * context per entry of dev_ids and drives them from one host thread each.  ndev <= 0 or dev_ids == NULL: all visible
 * devices (the first ndev of them).  An id may repeat: several contexts on one device -- the way to exercise the
 * multi-device code on one GPU and to work a text too long for one index off in partitions.  Plans, tried in this
 * order (fbg_group_plan_used tells which one ran):
 *   FBG_PLAN_PARTITIONED  key-range partitioned index (fbg_part_*): an all-gather of FBG_PART_HALO_BYTES per
 *                         partition and an all-reduce(MAX) of n + 1 words; gap-free MSAs without ignore characters,
 *                         texts of any length below 2^40 symbols (the only way beyond 2^32); partitions may outnumber
 *                         the members (option "partitions", default: as many as keep a partition below ~1e9
 *                         suffixes and within device memory), each member then works several off in turn
 *   FBG_PLAN_COLUMNS      replicated index, member r scans columns [r * ceil(n / W), ...) -- compute_f_range's
 *                         partition, fbg.cpp:2278-2284 -- one all-gather of f
 *   FBG_PLAN_ROW_PAIRS    texts of 2^32 symbols and more that the partitioned index declines (elastic f only): one
 *                         all-reduce(MAX) of f
 * The exchanges are RCCL collectives (ncclAllGather / ncclAllReduce, one communicator per member) when every member
 * has its own device, device-to-device copies otherwise or with option "exchange" = 1.  The result lands in member
 * 0's device memory and, for the host-buffer entry points, in the caller's array; the sweep and fbg_block_graph are
 * then run on fbg_group_member(g, 0).  Group options: "partitions", "plan" (FBG_PLAN_*), "exchange" (0 auto,
 * 1 copies, 2 RCCL); any other key goes to every member (fbg_set_option).
 */
typedef struct fbg_group fbg_group;
enum { FBG_PLAN_AUTO = 0, FBG_PLAN_PARTITIONED = 1, FBG_PLAN_COLUMNS = 2, FBG_PLAN_ROW_PAIRS = 3 };
int fbg_group_create(int ndev, const int *dev_ids, fbg_group **out);
void fbg_group_destroy(fbg_group *g);
const char *fbg_group_last_error(const fbg_group *g);     /* g may be NULL after a failed fbg_group_create */
int fbg_group_size(const fbg_group *g);
fbg_ctx *fbg_group_member(fbg_group *g, int i);
int fbg_group_set_option(fbg_group *g, const char *key, int64_t value);
int fbg_group_plan_used(const fbg_group *g, int *partitions);
/* the same contracts as fbg_elastic_f / fbg_repeatfree_v / fbg_gapped_v */
int fbg_group_elastic_f(fbg_group *g, const uint8_t *msa, uint64_t m, uint64_t n, const uint8_t *ignore_chars,
                        uint64_t ignore_len, int disable_tricks, uint64_t *f);
int fbg_group_repeatfree_v(fbg_group *g, const uint8_t *msa, uint64_t m, uint64_t n, uint64_t *v);
int fbg_group_gapped_v(fbg_group *g, const uint8_t *msa, uint64_t m, uint64_t n, uint64_t *v);
/* staged: the MSA onto every member's device (once per device), then f of all columns into member 0's memory;
 * *d_f (n values, device memory of member 0) stays valid until the next call on the group */
int fbg_group_msa_load_host(fbg_group *g, const uint8_t *msa, uint64_t m, uint64_t n);
int fbg_group_msa_synthetic(fbg_group *g, uint64_t m, uint64_t n, uint64_t seed, uint64_t seed2, uint64_t gap_start_threshold,
                            uint32_t gap_run_len, uint64_t seed3, uint64_t n_threshold);
int fbg_group_scan_f(fbg_group *g, const uint8_t *ignore_chars, uint64_t ignore_len, int disable_tricks, uint64_t **d_f);

/* Pinned host memory: an MSA (or an output array) allocated here moves over PCIe by DMA straight from / into the
 * caller's pages; any other host memory is accepted too and goes through the library's own pinned bounce buffers. */
void *fbg_host_alloc(uint64_t bytes);
void fbg_host_free(void *p);

/* ---- pattern index of a founder graph (pindex.h lists its files) ----------------------------------------------
 *
 * The query side of the reference's founder_block_index (make_index, fbg.cpp:2809-2953; backward_search,
 * founder_block_index.hpp:86-145), built and searched on the GPU.  The graph: n_nodes labels in node id order
 * (labels + label_off[u] .. label_off[u + 1]; '#' and zero bytes are refused with FBG_ERR_INVALID, empty labels are
 * fine) and out-edges as CSR by source (edge_dst[edge_off[u] .. edge_off[u + 1]), node indices; duplicates count
 * once).  All arguments are host buffers.
 *   text   for every node u in id order and every distinct v in its out-edges, ascending: reverse(label(u) +
 *          label(v) + '#'); then one 0 sentinel.  N + 1 < 2^32 symbols (else FBG_ERR_TOO_LARGE).
 *   SA     full suffix array of the text, unsigned byte order; bs(c, l, r) the one-symbol backward step over its BWT.
 *   B / E  every label searched left to right from [0, N] sets B[lhs] and E[rhs] (sorted position lists, each
 *          position once).  A label whose search finds nothing sets nothing (the reference asserts there).
 *   locate each pattern left to right from [0, N]: a step that finds nothing may restart once per symbol at a block
 *          pair boundary ('#' must follow the range, r1 = #B positions <= l > 0, [select_B(r1), select_E(r1)] must
 *          enclose the range -- r1 beyond the E positions: not found -- and the symbol must occur in it); else the
 *          search stops.  count = the size of the last range (what locate_patterns prints: occurrences in the BWT
 *          index, not exact path matches), 0 when the search stopped; pos = symbols matched.  Empty pattern: (0, 0).
 * An index borrows its context's device and stream (destroy it before the context) and owns all of its buffers; the context's MSA, MSA index and
 * every other call are unaffected.  Calls on one index and its context are serialised by the caller.
 */
typedef struct fbg_pindex fbg_pindex;
int fbg_pindex_build(fbg_ctx *ctx, const uint8_t *labels, const uint64_t *label_off, uint64_t n_nodes,
                     const uint64_t *edge_off, const uint64_t *edge_dst, fbg_pindex **out);
/* patterns + pat_off[k] .. pat_off[k + 1]; count, pos: n_patterns values each */
int fbg_pindex_locate(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                      uint64_t *count, uint64_t *pos);
/* N + 1, the text length including the sentinel */
uint64_t fbg_pindex_text_length(const fbg_pindex *ix);
/* For tests; any pointer may be NULL.  text: N + 1 bytes, sa: N + 1 values, b_positions / e_positions: *nb / *ne
 * values (at most n_nodes each; call with NULL lists first to learn the sizes). */
int fbg_pindex_download(fbg_pindex *ix, uint8_t *text, uint32_t *sa, uint32_t *b_positions, uint32_t *e_positions,
                        uint64_t *nb, uint64_t *ne);
/* Measurement (any pointer may be NULL): device bytes of the search structure (occ lines, count table, B / E,
 * symbol tables; the text and SA kept for fbg_pindex_download are not counted), host wall time of the build in ms,
 * device time of the last fbg_pindex_locate in ms (length sort + search kernel, without the copies), and the occ
 * lines its search read. */
int fbg_pindex_stats(const fbg_pindex *ix, uint64_t *index_bytes, double *build_ms, double *search_ms,
                     uint64_t *occ_lines);
void fbg_pindex_destroy(fbg_pindex *ix);

/* Semi-repeat-free check of the index's graph (the reference's efg_validate / efg_validate_node, fbg.cpp:3104-3292,
 * without the repair).  Input: the index as built, node_block[n_nodes] (one block id per node; only equality matters)
 * and an optional set of ignore bytes.  status[u] is given by the first rule that applies:
 *   1. u has no in-edge or no out-edge                                  FBG_NODE_SKIP_SOURCE_SINK
 *   2. label(u) holds a byte of the ignore set                          FBG_NODE_SKIP_IGNORED
 *   3. label(u) is empty                                                FBG_NODE_SKIP_EMPTY (the reference is undefined)
 *   4. every occurrence of label(u) at an offset s of label(a) + label(b), over the distinct edges (a, b) (an
 *      occurrence never crosses the '#'), belongs to node a at offset s if s < |label(a)|, else to node b at offset
 *      s - |label(a)|; it is allowed iff that offset is 0 and the node's block is u's.  All allowed: FBG_NODE_VALID,
 *      else FBG_NODE_INVALID.
 * Witness of an INVALID node: its disallowed occurrence of smallest SA slot in u's range of the index text (the
 * suffixes that start with reverse(label(u))), as (node, offset); UINT64_MAX in both for every other status.  The
 * per-node verdict equals the reference's, which indexes the forward text with duplicate edges in adjacency order:
 * neither changes the set of distinct (edge, offset) occurrences.
 * Device tables the build keeps for this (not counted in index_bytes): per node the SA range of its label (from the
 * B / E walk), a text position, its length and in / out flags (17 bytes); per distinct edge its text start, source
 * and destination (12 bytes, plus one text start); a coarse table of the edge at every 256th text position (4 bytes
 * each).  A call adds 17 bytes per node of scratch, leaves later fbg_pindex_locate results and the context's
 * segmentation results unchanged, and does not change fbg_pindex_stats' search_ms.
 * node_block, status: n_nodes values; witness_* may be NULL; *n_invalid and *device_ms (device time of the
 * validation kernels, without the copies) may be NULL.  A NULL index, or a NULL node_block / status with
 * n_nodes > 0, returns FBG_ERR_INVALID. */
#define FBG_NODE_VALID 0
#define FBG_NODE_INVALID 1
#define FBG_NODE_SKIP_SOURCE_SINK 2
#define FBG_NODE_SKIP_IGNORED 3
#define FBG_NODE_SKIP_EMPTY 4
int fbg_pindex_validate(fbg_pindex *ix, const uint32_t *node_block, const uint8_t *ignore_chars, uint64_t ignore_len,
                        uint8_t *status, uint64_t *witness_node, uint64_t *witness_offset, uint64_t *n_invalid,
                        double *device_ms);
/* Measurement of the last fbg_pindex_validate (any pointer may be NULL): SA slots scanned, nodes whose range went to
 * the wave tier, and the device bytes of the tables the build keeps for validation. */
int fbg_pindex_validate_stats(const fbg_pindex *ix, uint64_t *slots_scanned, uint64_t *wave_nodes, uint64_t *table_bytes);

/* Where each pattern occurs: the search of fbg_pindex_locate ("locate" above, unchanged: the same count and pos), and
 * for every pattern that is found the places of the graph where the match ends and where it starts.
 *
 * Edge e = (a, b) of the build (distinct edges, by source, then destination), S_e = label(a) + label(b),
 * n_e = |S_e|; its reversed copy with the leading '#' starts at text position estart[e], base = estart[e] + 1.  A
 * place is (edge_src, edge_dst, offset): an index into S_e of the edge (edge_src, edge_dst), node indices as given to
 * fbg_pindex_build.  The search of pattern P records on its way:
 *   restarts   the steps that took the restart branch and went on;
 *   at the first of them, before the range is replaced: k = symbols matched so far and [sl, sr] = the range after
 *              the '#' step (every slot i there has SA[i] = estart[e] for one edge e);
 *   at the end, if count > 0: the final range [l, r].
 * For a found pattern (count > 0):
 *   ends       for slot i in [l, r], p = SA[i], e = the edge whose string holds p:
 *              (src(e), dst(e), n_e - 1 - (p - base)), the position of the pattern's last symbol.  end_total = count.
 *   starts     restarts == 0: the same slots, offset = end offset - |P| + 1 (the match lies inside one edge string);
 *              start_total = count.  restarts > 0: for slot i in [sl, sr], e = the edge with estart[e] == SA[i]:
 *              (src(e), dst(e), n_e - k): the first k symbols of P are a suffix of S_e; start_total = sr - sl + 1.
 * A pattern that is not found, the empty one included, has no ends and no starts (both totals 0), whatever was
 * recorded; its restarts are still reported.  Places come in ascending SA slot order.  max_per_pattern = M: only the
 * first min(total, M) slots of each range are reported, the totals say how many there are; M = 0 reports totals and
 * restarts only.  Offsets are computed modulo 2^32: they lie inside S_e for patterns without '#' and zero bytes
 * (others can match across a separator and get offsets outside it).  A graph without edges has no places: its lists
 * are empty.
 *
 * These are the occurrences of the reference's search, with its looseness: after a restart the search goes on from
 * all occurrences of the enclosing node label, which in a semi-repeat-free graph may be a proper prefix of a sibling
 * node of the same block.  The starts and the ends of a pattern with restarts are therefore two independent lists; a
 * (start, end) pair is no proof of a path through the graph.  Paths are not verified here.
 *
 * Two calls, because the size of the lists is known only after the search and the buffers are the caller's:
 *   fbg_pindex_occurrences        search and sizes.  count, pos, end_total, start_total: n_patterns values; restarts:
 *       n_patterns values; end_off, start_off: n_patterns + 1 CSR offsets of the capped lists (pattern k's places are
 *       entries end_off[k] .. end_off[k + 1] of the fetched arrays).  The ranges stay on the device until the next
 *       fbg_pindex_occurrences on this index; fbg_pindex_locate and fbg_pindex_validate in between do not disturb them,
 *       and this call leaves fbg_pindex_stats' search_ms and occ_lines (the last fbg_pindex_locate) alone.
 *       *device_ms (may be NULL): device time of length sort, walk, sizes and scans, without the copies.
 *   fbg_pindex_occurrences_fetch  expands the ranges into end_* (end_off[n_patterns] entries each) and start_*
 *       (start_off[n_patterns] entries each).  Either list may be left out by passing NULL for its three arrays; may be
 *       called again.  *device_ms (may be NULL): device time of the expansion kernels.
 * Errors: a NULL index, a NULL end_off / start_off, or with n_patterns > 0 a NULL pat_off or output array:
 * FBG_ERR_INVALID; a fetch without a successful fbg_pindex_occurrences before it, or with one or two of a list's
 * three arrays NULL: FBG_ERR_INVALID; a capped list of 2^32 entries or more: FBG_ERR_TOO_LARGE (nothing to fetch then).
 * No table is added at build time; the per-call scratch (about 90 bytes per pattern, 12 per reported place) is owned by
 * the index. */
int fbg_pindex_occurrences(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                           uint64_t max_per_pattern, uint64_t *count, uint64_t *pos, uint32_t *restarts,
                           uint64_t *end_off, uint64_t *start_off, uint64_t *end_total, uint64_t *start_total,
                           double *device_ms);
int fbg_pindex_occurrences_fetch(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                                 uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms);

/* Maximal exact-match seeds: every read cut greedily into the pieces the search of the index accepts.
 *
 * search(Q) is "locate" above: it reads Q left to right and returns (count, pos); its state after j symbols depends
 * only on Q[:j].  For a pattern P and a minimum length L >= 1:
 *     i = 0
 *     while i < |P|:
 *         k = search(P[i:]).pos             the longest prefix of P[i:] the search accepts
 *         if k == 0:  i += 1                P[i] cannot be matched from the full range: skipped
 *         else:       seed (i, k); i += k   the failing symbol, if any, starts the next search
 * Seeds with k < L are consumed like the others but not reported.  The empty pattern has no seeds.  For a reported
 * seed (q_start, length) = (i, k), count (> 0 always), restarts, end_total, start_total and the capped end and start
 * place lists, in ascending SA slot order, are what fbg_pindex_occurrences and fbg_pindex_occurrences_fetch report for
 * the pattern P[i : i + k] with max_per_pattern = max_per_seed: a seed adds no notion of a match to the occurrence
 * calls, and it shares their looseness (no path is verified; fbg_pindex_chains below chains a read's seeds).  Patterns holding '#' or zero
 * bytes get no special treatment: whatever the search does with them is what a seed is.
 *
 * Three calls, because the number of seeds is known only after the search and the buffers are the caller's:
 *   fbg_pindex_seeds         search and sizes.  seed_off: n_patterns + 1 CSR offsets of the reported seeds (pattern k's
 *       seeds are entries seed_off[k] .. seed_off[k + 1] of the fetched arrays, in ascending q_start; patterns in input
 *       order).  The device walks every read twice: a pass that counts the reported seeds, a scan, and a pass that
 *       writes one record per seed (56 bytes; nothing is reserved for seeds that are not there); the sizes and scans of
 *       fbg_pindex_occurrences then run over the seeds.  *device_ms (may be NULL): device time from the length sort to
 *       the scans, the host's look at the seed total between the two passes included, without the other copies.
 *   fbg_pindex_seeds_fetch   per seed (seed_off[n_patterns] entries; end_off / start_off one more, the CSR offsets of
 *       the capped place lists): any pointer may be NULL.  *device_ms (may be NULL): device time of the copies.
 *   fbg_pindex_seeds_places  the places of the seeds, as fbg_pindex_occurrences_fetch: end_* take end_off[seeds]
 *       entries each, start_* start_off[seeds]; either list may be left out by passing NULL for its three arrays; may
 *       be called again.  *device_ms (may be NULL): device time of the expansion kernels.
 * The seeds stay on the device until the next fbg_pindex_seeds on this index.  They are kept apart from the ranges of
 * fbg_pindex_occurrences: fbg_pindex_occurrences_fetch after a seeds call still returns the places of the last
 * fbg_pindex_occurrences, and the other way round.  The calls leave fbg_pindex_stats' search_ms and occ_lines,
 * fbg_pindex_validate's results and the context's segmentation results alone.
 * Errors: a NULL index, a NULL seed_off, min_length == 0, a NULL pat_off with n_patterns > 0, missing pattern bytes,
 * decreasing offsets, a fetch or places call without a successful fbg_pindex_seeds before it, one or two of a place
 * list's three arrays NULL: FBG_ERR_INVALID.  A pattern of 2^32 symbols or more, 2^32 - 1 patterns or more, 2^32
 * reported seeds or more, a capped place list of 2^32 entries or more: FBG_ERR_TOO_LARGE (nothing to fetch then).
 * n_patterns == 0: seed_off[0] = 0, FBG_OK.  A min_length of 2^32 or more, which no pattern reaches: no seeds, FBG_OK
 * (the patterns are checked as always).  The per-call scratch (16 bytes per pattern, about 130 per reported seed,
 * 12 per reported place) is owned by the index. */
/* search and sizes: seed_off[n_patterns + 1] = CSR of the reported seeds per pattern */
int fbg_pindex_seeds(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                     uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off, double *device_ms);
/* per seed (seed_off[n_patterns] entries; end_off / start_off one more): any pointer may be NULL */
int fbg_pindex_seeds_fetch(fbg_pindex *ix, uint32_t *q_start, uint32_t *length, uint64_t *count, uint32_t *restarts,
                           uint64_t *end_total, uint64_t *start_total, uint64_t *end_off, uint64_t *start_off,
                           double *device_ms);
/* places of the seeds, as fbg_pindex_occurrences_fetch: either list may be left out, may be called again */
int fbg_pindex_seeds_places(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                            uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms);

/* ---- the pattern index of a segmentation, built on the device; validation and repair of a segmentation ------------
 *
 * fbg_pindex_build_segmentation: the pattern index of the elastic founder graph that `boundaries` (the fbg_minmax_dp
 * convention: inclusive block ends, the last one is n) cuts out of the context's current MSA.  The result is an
 * ordinary fbg_pindex, indistinguishable from fbg_pindex_build given the labels and edges of fbg_block_graph: the same
 * node numbering (blocks in order, within a block by first appearance by row), text, SA, B and E; locate,
 * occurrences, validate, download and stats work on it unchanged.  Nothing but a few sizes and a 256-entry byte
 * histogram goes through the host: the device stage of fbg_block_graph leaves nodes and distinct sorted edges in
 * device memory, the labels are gathered from the resident MSA, and the tables of fbg_pindex_validate are derived
 * there (the label position of a node from the FIRST edge that touches it, as fbg_pindex_build does).  The index
 * also keeps node_block[n_nodes] and first_node[nb + 1] on the device (fbg_pindex_node_info).
 * Errors: FBG_ERR_INVALID for a missing argument, no MSA, boundaries that do not increase or pass n, or a '#' or a
 * zero byte in the MSA (checked on the device); FBG_ERR_TOO_LARGE for more than FBG_MAX_ROWS rows, 2^32 (row, block)
 * cells, or an edge text of 2^32 symbols or more; FBG_ERR_HASH_COLLISION as fbg_block_graph reports it.
 * The call uses the workspaces of fbg_block_graph; the context's MSA, its MSA index and every other fbg_pindex are
 * left as they were. */
int fbg_pindex_build_segmentation(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, fbg_pindex **out);
/* nodes of an index's graph */
uint64_t fbg_pindex_node_count(const fbg_pindex *ix);
/* For tests and the Python layer; any pointer may be NULL.  label_len: n_nodes values (the label lengths, capped at
 * 2^32 - 1; any index).  node_block: n_nodes values, first_node: nb + 1 values (an index built from a segmentation
 * only, else FBG_ERR_INVALID). */
int fbg_pindex_node_info(fbg_pindex *ix, uint32_t *label_len, uint32_t *node_block, uint64_t *first_node);

/* MSA row and column of every reported place (an index built by fbg_pindex_build_segmentation only).
 *
 * A place (edge_src, edge_dst, offset) is private to one segmentation; the MSA column is the one coordinate all rows
 * and all blocks share.  For the MSA A[m][n] and the boundaries the index was built from:
 *   block j    covers the columns [x0, x1), x0 = j ? boundaries[j - 1] + 1 : 0, x1 = min(boundaries[j] + 1, n);
 *   r(u)       the representative row of node u of block j: rep_row of fbg_block_graph, the first row, by row index,
 *              whose gap-stripped label in the block is label(u);
 *   col(u, o)  for 0 <= o < |label(u)|: the column of the o-th (from 0) non-gap cell of row r(u) in [x0, x1).
 * A place (a, b, offset) belongs to node a at o = offset if offset < |label(a)|, else to node b at
 * o = offset - |label(a)| (what Occurrences.as_nodes does); its coordinate is (row, col) = (r(u), col(u, o)), so that
 * A[row][col] == S_e[offset]: the pattern's last symbol for an end, its first symbol for a start.  If o >= |label(u)|,
 * row = col = 0xffffffff; only patterns holding '#' or a zero byte get there (their offsets may lie outside S_e).
 * ONE witness row per place, not the set of rows: other rows that carry the same node may have their gaps elsewhere
 * in the block and so other columns for the same offset.  The rows through a node or edge are not reported.
 *
 * The build keeps a table for this on the device, derived from the resident MSA (the index keeps no pointer to the
 * MSA: replacing the context's MSA later changes no answer): 16 bytes per node (row, x0, bitmap position, x1 - x0),
 * and for every node whose row has a gap in its block a bitmap of the non-gap cells of [x0, x1) in 64-bit words with
 * a running count in front of every 8 words (9/8 bits per column).  A lookup is a search over a node's counts, at
 * most 8 popcounts and one select inside a word, whatever the block's width; a node without gaps is x0 + o.  The
 * table is counted neither in index_bytes nor in table_bytes; fbg_pindex_msa_stats reports it.  With it
 * fbg_pindex_build_segmentation also returns FBG_ERR_TOO_LARGE for an MSA of 2^32 columns or more and for a table of
 * 2^32 - 1 words or more (sizes are summed in 64 bits; nothing wraps).  The rounds of fbg_segmentation_validate and
 * fbg_segmentation_repair report no places and build no table.
 *
 *   fbg_pindex_occurrences_msa   entry i of end_row / end_col is the coordinate of entry i of what
 *       fbg_pindex_occurrences_fetch returns in end_*, and the same for start_*: the same CSR offsets (end_off,
 *       start_off of fbg_pindex_occurrences), order and cap.
 *   fbg_pindex_seeds_msa         the same for fbg_pindex_seeds_places and the offsets of fbg_pindex_seeds_fetch.
 * Either list may be left out by passing NULL for both of its arrays.  A call may come before, after or without the
 * fetch / places call and may be repeated; it expands into a buffer of its own and leaves the other place state, later
 * fetches, fbg_pindex_stats' search_ms and occ_lines, validation results and the context alone.  *device_ms (may be
 * NULL): device time of the expansion kernels.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index not built from a segmentation; no successful search of that
 * kind before the call; one of a list's two arrays NULL.  Nothing to report returns FBG_OK.
 *   fbg_pindex_msa_stats         any pointer may be NULL: device bytes of the table, nodes with a bitmap, and the columns
 *       between two running counts (64 * 8).  FBG_ERR_INVALID for a NULL index or one not built from a segmentation. */
int fbg_pindex_occurrences_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row,
                               uint32_t *start_col, double *device_ms);
int fbg_pindex_seeds_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row, uint32_t *start_col,
                         double *device_ms);
int fbg_pindex_msa_stats(const fbg_pindex *ix, uint64_t *map_bytes, uint64_t *gapped_nodes, uint64_t *sample_columns);

/* Co-linear chaining of a read's seeds (an index built by fbg_pindex_build_segmentation only).
 *
 * The reads are those of the last successful fbg_pindex_seeds on the index: n = its n_patterns, read R has the seeds
 * seed_off[R] .. seed_off[R + 1], seed t has q_start[t], length[t] and the capped start places start_off[t] ..
 * start_off[t + 1], and place g has the column start_col[g] that fbg_pindex_seeds_msa reports.  An anchor of read R is
 * a start place g of one of its seeds t with start_col[g] != 0xffffffff; write q = q_start[t], k = length[t],
 * c = start_col[g].  Anchors are identified and ordered by g: those of earlier seeds first, a seed's in slot order.
 * The witness row and the end places play no part.
 *   i precedes j   iff t_i < t_j, c_j >= c_i + k_i (along any path every symbol sits in a later column than the one
 *                  before, so a seed takes at least k columns from c on) and |(c_j - c_i) - (q_j - q_i)| <= band (the
 *                  surplus of columns over read symbols: gap columns if positive, read insertions if negative), all in
 *                  signed 64-bit; band = UINT64_MAX: unbounded;
 *   best[j]        k_j + max(0, max over the i that precede j of best[i]); pred[j] = the i of that inner maximum, the
 *                  smallest g among equals, none if nothing precedes j;
 *   the chain      of read R ends at its anchor of largest best, the smallest g among equals, and follows pred back;
 *                  score[R] = that best, 0 for a read without an anchor; if score[R] < min_score the score is
 *                  reported and the chain is empty.
 * A chain is a best-scoring co-linear selection among the places the seed calls already report: it adds no notion of
 * a match and inherits their looseness (one witness row per place, the cap, no path is verified).  Scores count covered
 * read symbols only, are at most the read's length and fit uint32_t.
 *
 *   fbg_pindex_chains        the DP and the sizes.  chain_off: n + 1 CSR offsets (read R's chain is entries chain_off[R]
 *       .. chain_off[R + 1] of the fetched arrays, in ascending q_start); score: n values, may be NULL.  On the device:
 *       the start columns are expanded into a buffer of the chain state, the reads are sorted by their number of start
 *       places (known from start_off; at least their number of anchors) and chained in three tiers -- up to small_max
 *       places by a quarter of a wave per read, up to lds_max by a wave with the state of the earlier places in LDS,
 *       beyond by a wave with that state in device memory -- which run the same code and give the same chains; one lane
 *       per read then walks back from the chain's end, a pass that counts, a scan, a pass that writes.  *device_ms (may
 *       be NULL): device time of all of it, the host's look at the tier sizes included, without the copies out.
 *   fbg_pindex_chains_fetch  anchor_place: the g of every chain entry, an index into the start arrays of
 *       fbg_pindex_seeds_places and fbg_pindex_seeds_msa; anchor_seed: its seed t, an index into the arrays of
 *       fbg_pindex_seeds_fetch.  chain_off[n] entries each; either may be NULL; may be called again.
 *   fbg_pindex_chain_stats   any pointer may be NULL: of the last successful fbg_pindex_chains (0 without one) the anchors
 *       of all reads and the reads each tier chained (reads without a start place are in none); small_max and lds_max,
 *       the tiers' limits, at any time.
 * The chains stay on the device until the next fbg_pindex_chains or fbg_pindex_seeds on this index; a new
 * fbg_pindex_seeds invalidates them.  A chains call leaves the seeds (fbg_pindex_seeds_fetch, _places and _msa return
 * what they returned before), the occurrences, fbg_pindex_stats, validation results and the context alone.
 * Errors, all FBG_ERR_INVALID: a NULL index or chain_off; an index not built from a segmentation; no successful
 * fbg_pindex_seeds before the call; a fetch without a successful fbg_pindex_chains since the last fbg_pindex_seeds.
 * n == 0: chain_off[0] = 0, FBG_OK.  Seeds without places (max_per_seed == 0): every score 0, every chain empty, FBG_OK.
 * 2^32 chain entries or more would be FBG_ERR_TOO_LARGE; a chain holds one place per seed at most and a seeds call
 * fewer than 2^32 seeds, so the limit is not reached.  Scratch owned by the index: 12 bytes per start place (16 more
 * when a read takes the third tier), 40 per read, 8 per seed. */
int fbg_pindex_chains(fbg_pindex *ix, uint64_t band, uint64_t min_score, uint64_t *chain_off, uint32_t *score,
                      double *device_ms);
int fbg_pindex_chains_fetch(fbg_pindex *ix, uint32_t *anchor_place, uint32_t *anchor_seed, double *device_ms);
int fbg_pindex_chain_stats(const fbg_pindex *ix, uint64_t *anchors, uint64_t *reads_small, uint64_t *reads_wave,
                           uint64_t *reads_spill, uint64_t *small_max, uint64_t *lds_max);

/* Both strands: seeds and chains of every read and of its reverse complement, from one upload.
 *
 *   complement table   comp: 256 bytes.  NULL stands for the default: A <-> T, C <-> G, a <-> t, c <-> g, every other
 *                      byte maps to itself.
 *   reverse complement for a read P of length L: rc(P)[i] = comp[P[L - 1 - i]].  The table is applied once per symbol; it
 *                      need not be an involution.  Bytes that map to '#' or to zero get no special treatment: whatever
 *                      the search does with them is the answer, as for fbg_pindex_seeds.
 *   virtual reads      the n reads P_0 .. P_{n-1} make 2n virtual reads: read R is the forward read P_R, read n + R is
 *                      rc(P_R).  The layout is blocked, not interleaved.
 *   seed coordinates   the seeds of a reverse virtual read are reported in the coordinates of rc(P_R): a seed (q, k)
 *                      there covers P_R[L - q - k : L - q].
 *
 *   fbg_pindex_seeds_strands   by definition fbg_pindex_seeds on those 2n patterns; seed_off has 2n + 1 entries.
 *       Afterwards fbg_pindex_seeds_fetch, _places, _msa, fbg_pindex_chains, _chains_fetch and fbg_pindex_chain_stats
 *       behave exactly as after that fbg_pindex_seeds call, with 2n reads.  The chains of reverse virtual reads ascend in
 *       the MSA columns like any other: the read is complemented, not the graph.  On the device the given reads are
 *       uploaded once, a kernel appends their reverse complements and the second half of the offsets, and the length
 *       sort, the two walks and the sizes of fbg_pindex_seeds run over the 2n reads.  *device_ms covers that kernel too.
 *       State rules and errors are those of fbg_pindex_seeds, and: FBG_ERR_TOO_LARGE if 2n >= 2^32 - 1 or if twice the
 *       pattern bytes do not fit the 64-bit size sums.  The index remembers that its seeds are stranded and with which
 *       n; a later fbg_pindex_seeds clears that.
 *   fbg_pindex_chain_strands   the strand of every given read.  It needs a successful fbg_pindex_seeds_strands as the
 *       last seeds call and a successful fbg_pindex_chains since it, else FBG_ERR_INVALID.  With s0, s1 the scores that
 *       fbg_pindex_chains reported for the virtual reads R and n + R, and c0, c1 whether their chains are non-empty:
 *       t = 1 if s1 > s0, else 0 (a tie goes to the forward strand); strand[R] = t if chain t is non-empty, else
 *       FBG_STRAND_NONE; score[R] = max(s0, s1) always; *n_forward, *n_reverse and *n_none count the reads by outcome.
 *       Any output pointer may be NULL; with n == 0 the call writes nothing and returns FBG_OK.  The chain of read R is
 *       then entries chain_off[t * n + R] .. chain_off[t * n + R + 1] of what fbg_pindex_chains_fetch returned: nothing
 *       is copied or reordered.  The call leaves every other state alone and may be repeated.  *device_ms (may be NULL):
 *       device time of the kernel. */
#define FBG_STRAND_NONE 0xff
int fbg_pindex_seeds_strands(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                             const uint8_t *complement, uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off,
                             double *device_ms);
int fbg_pindex_chain_strands(fbg_pindex *ix, uint8_t *strand, uint32_t *score, uint64_t *n_forward, uint64_t *n_reverse,
                             uint64_t *n_none, double *device_ms);

/* Which MSA rows carry a start place, and which carry a whole chain (an index built by
 * fbg_pindex_build_segmentation_rows only).
 *
 * A founder graph accepts recombinant paths: the search restarts at block-pair boundaries, so a seed that runs
 * X1 -> Y1 -> Z2 is reported even when no input sequence ever read X1 Y1 Z2.  For an index built from a segmentation
 * the rows of the MSA themselves say which places some input sequence carries.  Take the MSA A[m][n] and the
 * boundaries the index was built from:
 *   G_r            row r with its gap cells removed;
 *   p(r, j)        the number of non-gap cells of row r before the first column of block j;
 *   node_of[r][j]  the node of row r in block j, "none" for a row that is all gaps there (the node numbering of
 *                  fbg_pindex_build_segmentation).
 * A start place g = (a, b, offset) of seed t of (virtual) read R belongs to node u at o exactly as fbg_pindex_seeds_msa
 * decides it (u = a, o = offset if offset < |label(a)|, else u = b, o = offset - |label(a)|) and has the read substring
 * S = P_R[q_start[t] : q_start[t] + length[t]), for a reverse virtual read taken from rc(P_R).
 *   row r supports g   iff o < |label(u)|, node_of[r][block(u)] == u, and G_r[x : x + |S|) == S with
 *                      x = p(r, block(u)) + o; a row whose text ends before x + |S| does not support the place;
 *   rows(g)            the set of supporting rows;
 *   rows(chain of R)   the intersection of rows(g) over the chain's anchors, the empty set for an empty chain.
 * A place with rows(g) empty is a match only the graph has: a recombinant.  This is a statement about rows and so about
 * one path; it replaces neither the witness cell of fbg_pindex_seeds_msa (whose row need not support the place) nor the
 * chain score, and no existing call changes its results.  Sets are reported per chain only, not per place.
 *
 *   fbg_pindex_build_segmentation_rows   fbg_pindex_build_segmentation plus the row table: text, SA, B, E, node tables,
 *       MSA map, fbg_pindex_stats and fbg_pindex_msa_stats are those of the plain build, and so are the errors and limits
 *       (at most FBG_MAX_ROWS rows, fewer than 2^32 (row, block) cells).  The table is a device copy of node_of (4 bytes
 *       per (row, block) cell, block-major, so that 64 lanes read 64 consecutive rows) and of the gathered node labels
 *       with their 64-bit offsets: a node whose rows are all gaps in both neighbouring blocks has no edge and hence no
 *       copy of its label in the index text, yet a row's text runs through it.  The index keeps no pointer to the MSA and
 *       no copy of it.  The plain build and the rounds of fbg_segmentation_validate / _repair build no such table.
 *   fbg_pindex_rows_stats    any pointer may be NULL: m; the device bytes of the table; ceil(m / 64), the 64-bit words of
 *       a set; the places with an empty set in the last fbg_pindex_seeds_rows; the non-empty chains with an empty set in
 *       the last fbg_pindex_chains_rows (0 before the first such call; a call that fails its checks leaves them).
 *   fbg_pindex_seeds_rows    entry g is for start place g of fbg_pindex_seeds_places: the same offsets (start_off of
 *       fbg_pindex_seeds_fetch), order and cap.  n_rows[g] = |rows(g)|, first_row[g] = the smallest supporting row or
 *       0xffffffff.  End places get nothing.  Either array may be NULL.
 *   fbg_pindex_chains_rows   per read of the last seeds call (2n after fbg_pindex_seeds_strands): n_rows[R] = |rows(chain
 *       of R)|, first_row[R] its smallest row or 0xffffffff, and, if row_bits is not NULL, words_per_set 64-bit words per
 *       read: bit r % 64 of word r / 64 is set for each supporting row, bits at m and above are zero.  Any array may be
 *       NULL.
 * On the device: one lane per seed finds the byte its substring starts at, one lane per start place its node, offset,
 * seed and block; then lanes are rows, 64 at a time (16 when the MSA has at most 16 rows): one read of the block's
 * stretch of node_of, the lanes that hold the node compare S with label(u)[o:] and then with the labels of the row's
 * nodes in the following blocks (cells without a node are passed over, block nb ends the row), and a ballot is the word
 * of the set.  For a chain a lane stays with its row from anchor to anchor and the loop ends when the word is zero; no
 * per-place set is kept in device memory.  Scratch owned by the index: 16 bytes per start place, 8 per seed, and what a
 * call copies out.  *device_ms (may be NULL): device time of these kernels.
 * A call may be repeated and leaves the seeds, their places and MSA coordinates, the chains, the occurrences,
 * fbg_pindex_stats, validation results and the context alone.  The reads of the last seeds call stay readable: they
 * lie in buffers of their own, which fbg_pindex_locate and fbg_pindex_occurrences do not write.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index without the row table (the plain builder's included); no
 * successful seeds call before fbg_pindex_seeds_rows; no successful fbg_pindex_chains since the last seeds call before
 * fbg_pindex_chains_rows.  Nothing to report returns FBG_OK. */
int fbg_pindex_build_segmentation_rows(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, fbg_pindex **out);
int fbg_pindex_rows_stats(const fbg_pindex *ix, uint64_t *rows, uint64_t *table_bytes, uint64_t *words_per_set,
                          uint64_t *places_unsupported, uint64_t *chains_unsupported);
int fbg_pindex_seeds_rows(fbg_pindex *ix, uint32_t *n_rows, uint32_t *first_row, double *device_ms);
int fbg_pindex_chains_rows(fbg_pindex *ix, uint32_t *n_rows, uint32_t *first_row, uint64_t *row_bits, double *device_ms);

/* Chaining along one MSA row: which input sequence a read lies on best, and with which anchors (an index built by
 * fbg_pindex_build_segmentation_rows only; after a successful seeds call, plain or stranded).
 *
 * fbg_pindex_chains takes every start place as an anchor, whether or not an input sequence carries it, and breaks ties
 * by the smallest place, so among similar rows its chain often mixes rows: no row then spells every anchor and
 * fbg_pindex_chains_align has nothing to align against.  This call chains per row.  For a (virtual) read R, with the
 * anchors, columns, `precedes`, band and ties of fbg_pindex_chains and rows(g) of the rows section:
 *   chain(R, r)     the chain that fbg_pindex_chains defines on the anchors g of R with r in rows(g).  The columns stay
 *                   the witness columns of fbg_pindex_seeds_msa: nothing is chained in row coordinates;
 *   rowscore(R, r)  the score of chain(R, r), 0 without such an anchor;
 *   score[R]        max over r of rowscore(R, r);
 *   row[R]          the smallest r that attains score[R]; 0xffffffff where score[R] == 0;
 *   n_best_rows[R]  the number of rows that attain score[R]; 0 where score[R] == 0;
 *   the chain       of R is chain(R, row[R]); it is empty where score[R] < min_score or score[R] == 0.
 * Equivalently, the result is what fbg_pindex_chains returns when the start column of every place that row[R] does not
 * support is replaced by 0xffffffff; this is how it is computed.  It follows that
 *   - score[R] is at most the score fbg_pindex_chains reports, and equal to it where that call's chain has a carrying row;
 *   - after the call fbg_pindex_chains_rows gives, for every non-empty chain, first_row == row[R] and
 *     1 <= n_rows <= n_best_rows[R] (a smaller row that carries the whole chain would reach the same score);
 *   - fbg_pindex_chains_align gives row == row[R] for every non-empty chain, and its `unsupported` statistic is 0.
 * A read with more start places than option byrow_max (default 1024) is not chained: score 0, no row, an empty chain;
 * it is counted (reads_too_many).  The work per read is up to A^2 / 2 steps per 64 rows for A start places.
 * Limits: the columns are witness columns; a chain lies on one row only, so a read that truly recombines two input
 * sequences gets the better of its parts and no alignment of the whole against a row (fbg_pindex_chains_align_graph
 * aligns it against the graph); byrow_max.
 *
 *   fbg_pindex_chains_by_row         chain_off (n + 1) and score (n) as for fbg_pindex_chains; row and n_best_rows: n entries
 *       each; score, row and n_best_rows may be NULL.  n = the reads of the last seeds call (2n after
 *       fbg_pindex_seeds_strands).
 *   fbg_pindex_chains_by_row_stats   any pointer may be NULL.  Of the last successful call since the last seeds or
 *       fbg_pindex_chains call (0 without one): the reads whose state stayed in LDS, the reads with their state in device
 *       memory, the reads with more than byrow_max start places, the reads within byrow_max that have an anchor and
 *       score 0, and the start places that keep their column under the mask.  Then lds_max, the compiled capacity of the
 *       LDS tier, and max_places, the value of option byrow_max, at any time.
 * On the device.  The start columns and the per-place records of fbg_pindex_seeds_rows are made as those calls make them;
 * the reads are sorted by their number of start places and binned (none, LDS tier, device tier, too many), which the
 * host reads in one round trip.  A wave per read then takes the rows 64 at a time, a lane per row: per start place a
 * ballot of the rows that support it, then the chain DP in place order, where for each place the lanes test 64 earlier
 * places at a time (a supporting row in common, `precedes`) and every lane folds its own row's scores of the places
 * that pass.  Each lane keeps its best row, and the lanes are merged by (score descending, row ascending).  The state --
 * 280 bytes per start place -- is in LDS for reads of up to lds_max places and otherwise in a slab owned by the index,
 * reserved only when such a read exists.  One lane per start place then masks the columns by the read's row, and the
 * kernels of fbg_pindex_chains run on the masked columns.  The host compares the scores of the two phases; a difference
 * fails the call with FBG_ERR_HIP and names the first read.  *device_ms (may be NULL): device time of all of it, the
 * host's looks at the bins included, without the copies out.
 * The call leaves the chain state as fbg_pindex_chains on the masked columns would: fbg_pindex_chains_fetch,
 * fbg_pindex_chain_strands, fbg_pindex_chain_stats (anchors: the places kept), fbg_pindex_chains_rows, _align, _cigar and
 * _cigar_fetch work on its chains.  Like fbg_pindex_chains it invalidates the alignment and its paths; a later
 * fbg_pindex_chains replaces its result and a seeds call invalidates it.  It may be repeated, reads the reads of the
 * last seeds call also after a later fbg_pindex_locate or fbg_pindex_occurrences, and leaves the seeds, their places and
 * MSA coordinates, what the row calls returned and their statistics, the occurrences, fbg_pindex_stats, validation
 * results and the context alone.
 * Errors, all FBG_ERR_INVALID: a NULL index or chain_off; an index without the row table; no successful seeds call.
 * FBG_ERR_TOO_LARGE for 2^31 reads or more (a workgroup per read).  n == 0: chain_off[0] = 0, FBG_OK.  Seeds without
 * places: every score 0, every row 0xffffffff, every chain empty, FBG_OK, nothing launched. */
int fbg_pindex_chains_by_row(fbg_pindex *ix, uint64_t band, uint64_t min_score, uint64_t *chain_off, uint32_t *score,
                             uint32_t *row, uint32_t *n_best_rows, double *device_ms);
int fbg_pindex_chains_by_row_stats(const fbg_pindex *ix, uint64_t *reads_lds, uint64_t *reads_device, uint64_t *reads_too_many,
                                   uint64_t *reads_no_row, uint64_t *anchors_kept, uint64_t *lds_max, uint64_t *max_places);

/* The second-best chain of every read, and a mapping quality (an index built by fbg_pindex_build_segmentation only; after
 * a successful fbg_pindex_chains or fbg_pindex_chains_by_row since the last seeds call).
 *
 * A chaining call keeps the best chain of a read only, so a read that fits two loci of the MSA equally well looks as
 * certain as a unique one.  In a pangenome the alternative alleles of one locus lie in the same MSA columns: a chain
 * through another allele there is the same mapping and must not count against it.  Only a chain elsewhere in the
 * columns competes.  With the vocabulary of fbg_pindex_chains (anchors g, seed t, q, k, witness column
 * c = start_col[g] of fbg_pindex_seeds_msa, `precedes`, band, ties to the smallest g), for a (virtual) read R of the last
 * seeds call (2n of them after fbg_pindex_seeds_strands):
 *   the primary chain   what the last successful chaining call left, plain or by row: s1 = score[R] and the anchors
 *                       a_1 .. a_len in read order (none where the chain is empty, also where score[R] < min_score);
 *   span                lo = c(a_1), hi = c(a_len) + k(a_len), exclusive, in witness columns;
 *   kept anchors        an anchor g of R is excluded iff [c, c + k) meets [lo - margin, hi + margin), that is iff
 *                       c + k + margin > lo and c < hi + margin, evaluated so that nothing wraps (the sums saturate at
 *                       2^64 - 1); otherwise it is kept.  margin = UINT64_MAX excludes every anchor;
 *   the secondary chain the chain that fbg_pindex_chains defines on the kept anchors of R: the same `precedes`, the band of
 *                       the primary call, the same ties for predecessor and end, no min_score.  It always runs on the
 *                       unmasked witness columns, also after fbg_pindex_chains_by_row: a competing locus on any row
 *                       counts.  second[R] is its score, second_lo[R] and second_hi[R] its span (0xffffffff where it is
 *                       empty); its anchors are reported whenever second[R] > 0.  A read with an empty primary chain has
 *                       no secondary: second[R] = 0;
 *   mapq[R]             with L = |P_R| and s2 = min(second[R], s1): (60 * (s1 - s2)) / L, floored, in 64-bit; 0 where the
 *                       primary chain is empty or L == 0.  Scores are at most L, so the value lies in 0 .. 60;
 *   mapq_stranded[v]    after fbg_pindex_seeds_strands, with w = v +- n the twin of virtual read v: the same formula with
 *                       s2 = min(max(second[v], score[w]), s1).  The other strand's best chain is a competing mapping
 *                       wherever it lies, and its score is used also when it is below min_score: equal scores on both
 *                       strands give 0 on both.
 * It follows that after fbg_pindex_chains second[R] <= score[R]; after fbg_pindex_chains_by_row second[R] may exceed
 * score[R] (the secondary is not bound to a row) and mapq[R] is then 0; no anchor of a secondary chain meets
 * [lo - margin, hi + margin), though its span may reach over it, with anchors on either side.  The constants 60 and the linear shape are a convention in the range other mappers use: no
 * truth set exists to tune them against, and the value is no calibrated probability.
 * Limits.  Seeds are greedy maximal exact matches: a read that matches one locus in a single piece has no seed at a
 * shorter copy elsewhere and gets second = 0; competitors become visible once an edit or a block boundary splits the
 * read.  No gap costs, as in the chains.  Columns are witness columns, one row per place.
 *
 *   fbg_pindex_chains_mapq        the count step.  second_off: n + 1 CSR offsets of the secondary chains; second, second_lo,
 *       second_hi (n uint32_t each) and mapq (n uint8_t) may be NULL.  On the device: the witness columns are expanded into
 *       a buffer of this call's own, one lane per read takes lo and hi from the first and last entry of its primary chain,
 *       one lane per start place finds its read by two searches of the offsets and writes its column or "none", and the
 *       kernels of fbg_pindex_chains (sort, three tiers, trace) run on these columns in a chain state of this call's own;
 *       one lane per read then computes the secondary span and mapq.  *device_ms (may be NULL): device time of all of it,
 *       the host's look at the tier sizes included, without the copies out.
 *   fbg_pindex_chains_mapq_fetch  anchor_place and anchor_seed of the secondary chains, second_off[n] entries each, as
 *       fbg_pindex_chains_fetch; either may be NULL; may be called again.
 *   fbg_pindex_mapq_strands       mapq_stranded: 2n entries, one per virtual read (may be NULL).  It needs a successful
 *       fbg_pindex_seeds_strands as the last seeds call and a successful fbg_pindex_chains_mapq since the last chaining call.
 *   fbg_pindex_mapq_stats         any pointer may be NULL.  Of the last successful fbg_pindex_chains_mapq since the last
 *       chaining call (0 without one), over the reads with a non-empty primary chain: those with second > 0, their anchors
 *       kept and excluded, and the reads with mapq 0 and with mapq 60.
 * The call may be repeated with another margin; the later result replaces the earlier.  It leaves the seeds, their places
 * and columns, the primary chains and their fetch, strands, rows, both alignments, both CIGARs, the graph paths and
 * every statistic of those calls as they were.  A later seeds call, fbg_pindex_chains or fbg_pindex_chains_by_row
 * invalidates the result.  The lengths of the reads stay known after a later fbg_pindex_locate or fbg_pindex_occurrences.
 * Errors, all FBG_ERR_INVALID: a NULL index or second_off; an index not built from a segmentation; no successful
 * chaining call since the last seeds call; a fetch or strands call without a successful fbg_pindex_chains_mapq since the
 * last chaining call; fbg_pindex_mapq_strands after seeds that were not stranded.  n == 0, and seeds without places: every
 * output 0 (the spans 0xffffffff), FBG_OK, nothing launched.  Scratch owned by the index: what fbg_pindex_chains takes,
 * once more, and 4 bytes per start place and 25 per read. */
int fbg_pindex_chains_mapq(fbg_pindex *ix, uint64_t margin, uint64_t *second_off, uint32_t *second, uint32_t *second_lo,
                           uint32_t *second_hi, uint8_t *mapq, double *device_ms);
int fbg_pindex_chains_mapq_fetch(fbg_pindex *ix, uint32_t *anchor_place, uint32_t *anchor_seed, double *device_ms);
int fbg_pindex_mapq_strands(fbg_pindex *ix, uint8_t *mapq_stranded, double *device_ms);
int fbg_pindex_mapq_stats(const fbg_pindex *ix, uint64_t *reads_with_second, uint64_t *anchors_kept, uint64_t *anchors_excluded,
                          uint64_t *mapq0, uint64_t *mapq60);

/* Paired reads: a mate's chain rescued in the insert window of the other mate's chain, and the best combination per pair
 * (an index built by fbg_pindex_build_segmentation only; after a successful fbg_pindex_seeds_strands on an even number of
 * reads and a successful fbg_pindex_chains or fbg_pindex_chains_by_row since it).
 *
 * Two mates come from one fragment, on opposite strands, a bounded distance apart.  A chaining call treats each as a lone
 * read, so a mate that falls into a repeat goes to whichever copy scores a symbol more.  This call lets the other mate
 * decide.  With the vocabulary of fbg_pindex_chains and of fbg_pindex_chains_mapq (anchors, witness column c, seed
 * length k, span):
 *   layout              after fbg_pindex_seeds_strands on n given reads, n even, pair p is the given reads a = 2p and
 *                       b = 2p + 1, interleaved as in an interleaved FASTQ.  Virtual read v < n is read v as given, v >= n
 *                       the reverse complement of read v - n.  twin(v) = v +- n.  partner(v) is the twin of v's mate:
 *                       (v ^ 1) + n for v < n, (v - n) ^ 1 for v >= n; partner is an involution;
 *   the primary chain   of v: what the last chaining call left, plain or by row; non-empty where chain_off[v + 1] >
 *                       chain_off[v]; its span lo(v) = c of its first anchor, hi(v) = c + k of its last; its score score[v];
 *   the window of w     with v = partner(w) and min_insert <= max_insert: empty where v has no primary chain;
 *                       W = [lo(v), lo(v) + max_insert) for v < n (v is the forward mate, w the reverse one);
 *                       W = [hi(v) - max_insert, hi(v)) for v >= n, the lower end clamped at 0.  The sum saturates at
 *                       2^64 - 1.  A start place of w with witness column c and seed length k is kept iff c is a column,
 *                       c >= W.lo and c + k <= W.hi.  Columns are the unmasked witness columns, also after
 *                       fbg_pindex_chains_by_row;
 *   the rescue chain    of w: the chain that fbg_pindex_chains defines on the kept places of w alone, with the band of the
 *                       primary call, min_score 0 and the same ties.  All 2n virtual reads get one;
 *   candidates          of pair p, F the forward chain and R the reverse one, in this order:
 *                         0: F = primary(a), R = rescue(b + n)      1: F = rescue(a), R = primary(b + n)
 *                         2: F = primary(b), R = rescue(a + n)      3: F = rescue(b), R = primary(a + n)
 *                       A candidate is valid iff both chains are non-empty, lo(F) <= lo(R), hi(F) <= hi(R) and
 *                       min_insert <= hi(R) - lo(F) <= max_insert.  Its score is s(F) + s(R).  The pair takes the valid
 *                       candidate of the largest score, the smallest number among equals: which[p] in 0 .. 3, pair_score[p],
 *                       t_lo[p] = lo(F), t_hi[p] = hi(R).  Without a valid candidate which[p] = 0xff, pair_score[p] = 0,
 *                       t_lo[p] = t_hi[p] = 0xffffffff.
 *   fbg_pindex_chains_pairs   one call returns everything.  which, pair_score, t_lo, t_hi: n / 2 entries each (only which
 *       must be given).  rescue_off: 2n + 1 CSR offsets of the rescue chains (must be given); rescue_score, rescue_lo,
 *       rescue_hi: 2n each, may be NULL (score 0 and span 0xffffffff for an empty chain); rescue_place, rescue_seed: the
 *       anchors, as fbg_pindex_chains_fetch reports them; a chain has at most one anchor per seed, so buffers of as many
 *       entries as the seeds call reported seeds hold them; either may be NULL.  stats[8] (may be NULL): the pairs with
 *       which = 0, 1, 2, 3 and without a candidate; start places kept, and start places with a column that were not kept;
 *       pairs whose chosen candidate uses a rescue chain that scores other than the same read's primary chain.  On the
 *       device: one lane per virtual read takes the spans, one lane per start place finds its read by two searches and
 *       writes its column or "none", the kernels of fbg_pindex_chains run on these columns in a chain state of this call's
 *       own, one lane per virtual read takes the rescue spans and one lane per pair picks.  *device_ms (may be NULL): device
 *       time of all of it, adopt included, without the copies out.
 *   adopt               where adopt_chain_off (2n + 1) is given; adopt_score (2n) may be NULL.  For a pair with a
 *       candidate its two chosen virtual reads get the chosen chains as their primary chains and their two twins the empty
 *       chain with score 0; a pair without one keeps all four chains and scores as they were (a chain that min_score had
 *       emptied stays empty).  adopt_chain_off and adopt_score are the new chain_off and score, fbg_pindex_chains_fetch
 *       returns the new anchors, and every result made from the chains (fbg_pindex_chains_rows, _align, _cigar,
 *       _align_graph, _graph_cigar, _mapq; the statistics of fbg_pindex_chains_by_row) is stale as after a chaining call:
 *       run those calls again, and they describe the pair-consistent chains.  fbg_pindex_chain_strands then picks the pair's
 *       strand, the twin being empty.  A second call on chains adopted after fbg_pindex_chains finds every pair that had a
 *       candidate again, with the same two reads and chains, t_lo, t_hi and pair_score (which may name the other candidate of
 *       the same two reads).  After fbg_pindex_chains_by_row it finds the same two reads, but a rescue chain is not bound to
 *       the row and may then score higher than the row's chain, or tie with it on other anchors.  Without adopt nothing of
 *       the chains is written and nothing goes stale.
 * Limits.  The insert is counted in MSA witness columns: a stretch where most rows have gaps counts as long as its columns,
 * not as the fragment's symbols.  Forward-reverse orientation only.  No mapping quality of the pair.  A mate without a seed
 * inside the window is not rescued by alignment.  (fbg_pindex_pairs_align, below, does rescue such a mate, and counts the
 * insert in symbols of a row.)
 * Errors, all FBG_ERR_INVALID: a NULL index, which or rescue_off; an index not built from a segmentation; the last seeds
 * call was not fbg_pindex_seeds_strands, or none succeeded; no successful chaining call since it; n odd;
 * min_insert > max_insert.  A failed check leaves the index as it was.  n == 0, and seeds without places: every pair
 * without a candidate, every rescue chain empty, FBG_OK, nothing launched.  Scratch owned by the index: what
 * fbg_pindex_chains takes, once more, and 4 bytes per start place and 45 per virtual read. */
int fbg_pindex_chains_pairs(fbg_pindex *ix, uint64_t min_insert, uint64_t max_insert, uint8_t *which, uint32_t *pair_score,
                            uint32_t *t_lo, uint32_t *t_hi, uint64_t *rescue_off, uint32_t *rescue_score, uint32_t *rescue_lo,
                            uint32_t *rescue_hi, uint32_t *rescue_place, uint32_t *rescue_seed, uint64_t *adopt_chain_off,
                            uint32_t *adopt_score, uint64_t stats[8], double *device_ms);

/* The edit distance of each read to a row that carries its chain (an index built by
 * fbg_pindex_build_segmentation_rows only; after a successful seeds call, plain or stranded, and a successful
 * fbg_pindex_chains since it).
 *
 * A chain says which pieces of a read match exactly and where; it says nothing about the symbols between and around
 * the anchors.  fbg_pindex_chains_rows names the rows that spell every anchor of a chain, and the row table holds the
 * gap-stripped text G_r of every row, so the whole read can be aligned against one real input sequence around its
 * chain: "this read lies on input sequence r from t_start to t_end with d edits".  For a (virtual) read R let P be its
 * text, for a reverse virtual read rc(P_R), exactly as fbg_pindex_chains_rows reads it, and L = |P|.
 *   r          the smallest row of rows(chain of R).  If the chain is empty or no row carries it,
 *              row[R] = edits[R] = t_start[R] = t_end[R] = FBG_ALIGN_NONE.
 *   x_i, d_i   for anchor i of the chain, a place in node u_i at o_i of a seed (q_i, k_i): x_i = p(r, block(u_i)) + o_i,
 *              its position in G_r (the x of the rows section), and the diagonal d_i = x_i - q_i, signed 64-bit.
 *   W          the window G_r[w0 : w1) with w0 = max(0, min_i d_i - pad) and w1 = min(|G_r|, max_i d_i + L + pad).  It
 *              holds every anchor's stretch of G_r and so is never empty.
 *   D          unit costs, the ends of the row free, the read global: D(0, j) = 0, D(i, 0) = i,
 *              D(i, j) = min(D(i-1, j-1) + [P[i-1] != W[j-1]], D(i-1, j) + 1, D(i, j-1) + 1).  Symbols are compared as
 *              bytes: no case folding, no ignore characters.
 *   edits[R]   min_j D(L, j).  It follows that edits[R] <= L - max_i k_i.
 *   t_end[R]   w0 + e, e the smallest j that attains edits[R].
 *   t_start[R] the largest s in [w0, t_end] with lev(P, G_r[s : t_end)) == edits[R]; one always exists.  It is t_end - j'
 *              for the smallest end j' of a second pass over the reversed read against W[0 : e) reversed, with
 *              D'(0, j) = j.
 * The result is exact: the full recurrence over the window, no band inside it and no early cut-off.  Two per-read skips
 * keep row[R] and set the three other arrays to FBG_ALIGN_NONE; a skipped read is no error:
 *   too long   L > max_read, a constant of the implementation (1024, reported by fbg_pindex_align_stats);
 *   too wide   w1 - w0 > max_window (0: no limit), tested after too long.
 *
 *   fbg_pindex_chains_align   one entry per read of the last seeds call (2n after fbg_pindex_seeds_strands) in each of
 *       the four arrays; any of them may be NULL.  pad is clamped to 2^33, beyond which no window changes, so the sums
 *       stay in 64 bits.
 *   fbg_pindex_align_stats    any pointer may be NULL.  Of the last fbg_pindex_chains_align (0 before the first; a call
 *       that fails its checks leaves them): the reads aligned; the non-empty chains that no row carries; the reads
 *       skipped as too long and as too wide; cells, the sum of L * |W| over the aligned reads, which is the work.  Then
 *       max_read, and the device bytes of the prefix table (0 until the first call builds it).
 * On the device.  The prefix table p(r, j) is uint32[nb * m], block-major like node_of, built by the first call (one
 * lane per row steps over the blocks, so a wave reads 64 consecutive rows at every step) and owned by the index;
 * |G_r| < 2^32 holds because the build takes fewer than 2^32 columns.  A call chooses the rows with the kernel of
 * fbg_pindex_chains_rows; one lane per read then finds the diagonals, the window, the skip status and, by a search of
 * the row's column of the prefix table, the block, node and offset at which the window starts; the window lengths are
 * scanned and their sum sizes the scratch; a wave per read gathers its window label by label (lanes take consecutive
 * bytes, cells without a node are passed over); a wave per read runs Myers' bit-vector recurrence twice.  There lane i
 * holds read symbols i, 64 + i, ..., the window is loaded 64 bytes at a time, each byte is made wave-uniform by a
 * readlane, and the match word of a text byte is one ballot per 64 read symbols: no per-symbol table, any byte
 * alphabet.  The vertical difference words are wave-uniform 64-bit values; the last word is masked to L % 64 bits and
 * the score is followed at bit L - 1.  Reads of 1, 2, 3 and 4 words keep the state in registers (a template on the word
 * count), longer ones up to max_read in LDS with a loop over the words; every tier runs the same recurrence.  Scratch
 * owned by the index: 72 bytes per read, the windows, and what fbg_pindex_chains_rows keeps per seed and start place.
 * *device_ms (may be NULL): device time of these kernels.
 * A call may be repeated and leaves the seeds, their places and MSA coordinates, the chains, what the row calls
 * returned, the occurrences, fbg_pindex_stats, validation results and the context alone; like the row calls it still
 * sees the reads of the last seeds call after a later fbg_pindex_locate or fbg_pindex_occurrences.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index without the row table; no successful fbg_pindex_chains since the
 * last seeds call.  FBG_ERR_TOO_LARGE for 2^31 reads or more (a workgroup per read); the allocator's error if the
 * windows do not fit device memory.  No reads returns FBG_OK. */
#define FBG_ALIGN_NONE 0xffffffffu
int fbg_pindex_chains_align(fbg_pindex *ix, uint64_t pad, uint64_t max_window, uint32_t *row, uint32_t *edits,
                            uint32_t *t_start, uint32_t *t_end, double *device_ms);
int fbg_pindex_align_stats(const fbg_pindex *ix, uint64_t *aligned, uint64_t *unsupported, uint64_t *too_long,
                           uint64_t *too_wide, uint64_t *cells, uint64_t *max_read, uint64_t *table_bytes);

/* Paired reads: a mate without a seed is rescued by alignment in the insert window that the other mate's chain opens on a
 * row (an index built by fbg_pindex_build_segmentation_rows only; after a successful fbg_pindex_seeds_strands on an even
 * number of reads and a current chaining result since it: fbg_pindex_chains, fbg_pindex_chains_by_row, or the chains that
 * fbg_pindex_chains_pairs adopted).
 *
 * fbg_pindex_chains_pairs rescues a mate by chaining the seeds it has inside the window.  A mate with an edit every few
 * symbols has no seed of min_length at all: no chain, no rescue chain, and the pair is lost.  This call aligns such a mate
 * against the text of the row that carries its partner's chain, inside the insert window, with the recurrence of
 * fbg_pindex_chains_align.  Layout, twin and partner as in the pairs section: V = 2n virtual reads, n / 2 pairs; G_r,
 * p(r, j), x_i, D, edits, t_start and t_end as in the align section.
 *   anchored read v     a virtual read whose current chain is non-empty.  r(v) is the smallest row that spells every anchor
 *                       of it: exactly the row fbg_pindex_chains_align chooses.  Where no row does, v opens no window.
 *                       Anchor i has x_i = p(r, block(u_i)) + o_i, read offset q_i and seed length k_i; L_v is the read
 *                       length.  The fragment ends are projected along the first and the last anchor's diagonal:
 *                       fs(v) = max(0, x_1 - q_1) and fe(v) = min(|G_r|, x_last + L_v - q_last);
 *   selected read w     with v = partner(w) anchored: without select, w's own chain is empty; with select (2n bytes),
 *                       select[w] != 0.  Every other w gets "none" in every array and is not counted;
 *   the window of w     W = G_r[fs(v) : min(|G_r|, fs(v) + max_insert)) for v < n (v is the forward mate, w the reverse one);
 *                       W = G_r[max(0, fe(v) - max_insert) : fe(v)) for v >= n.  max_insert is clamped at 2^33, as pad is.
 *                       The insert is counted in symbols of row r, not in MSA columns;
 *   status              of a selected w, tested in this order and counted: partner without a carrying row; empty, L_w == 0
 *                       or |W| == 0; too long, L_w > max_read (1024); too wide, max_window != 0 and |W| > max_window; else
 *                       aligned.  row[w] = r(v) for every status but the first; the other arrays are "none" unless aligned;
 *   aligned             edits[w], t_start[w], t_end[w] follow the definition of fbg_pindex_chains_align for P = the text of
 *                       w over this W, with w0 the window's start: the read global, both ends of W free, unit costs, the
 *                       smallest end, then the largest start;
 *   accepted            insert[w] = t_end[w] - fs(v) for v < n and fe(v) - t_start[w] for v >= n.  w is accepted iff
 *                       edits[w] <= max_edits and insert[w] >= min_insert; insert[w] <= max_insert holds by construction.
 *                       A w that is not accepted keeps row, edits, t_start and t_end and gets insert[w] = 0xffffffff.
 *                       Rejections by edits and by insert are counted apart, edits first;
 *   candidates          of pair p = (a, b), in the order of fbg_pindex_chains_pairs:
 *                         0: F = chain(a), R = aligned(b + n)       1: F = aligned(a), R = chain(b + n)
 *                         2: F = chain(b), R = aligned(a + n)       3: F = aligned(b), R = chain(a + n)
 *                       With v the chained and w the aligned read, a candidate is valid iff w is accepted; its score is
 *                       score[v] + L_w - edits[w].  The largest score wins, the smallest number among equals: which[p] in
 *                       0 .. 3, pair_score[p], and t_lo[p] / t_hi[p] = fs(v) / t_end[w] for the even candidates and
 *                       t_start[w] / fe(v) for the odd ones.  Without a valid candidate which[p] = 0xff, pair_score[p] = 0,
 *                       t_lo[p] = t_hi[p] = 0xffffffff.
 *   fbg_pindex_pairs_align   one call returns everything and nothing outlives it.  row, edits, t_start, t_end, insert: 2n
 *       entries each, "none" is 0xffffffff, each may be NULL.  which (must be given), pair_score, t_lo, t_hi: n / 2 each.
 *       stats[10] (may be NULL): reads selected; aligned; whose partner has no carrying row; empty; too long; too wide;
 *       rejected by edits; rejected by insert; cells, the sum of L_w * |W| over the aligned reads; pairs with a candidate.
 *       *device_ms (may be NULL): device time of the kernels, without the copies out.
 * On the device.  The rows are chosen with the kernel of fbg_pindex_chains_rows, into a buffer of this call's own; one lane
 * per virtual read takes fs and fe from the first and last anchor of its chain; one lane per virtual read takes selection,
 * window and status and finds the block, node and offset at which the window starts by a search of the row's column of
 * the prefix table (built here if no call has built it yet); the window lengths are scanned and their sum sizes the
 * scratch; the gather and bit-vector kernels of fbg_pindex_chains_align run over all 2n reads (the wave of a read that is
 * not aligned returns at once); one lane per pair accepts and picks.  Nothing of the align, CIGAR, graph, mapq, pairs or
 * chain state is written: every current result of those calls stays current and unchanged.
 * Limits.  No CIGAR of the rescued mate and no adoption of the alignment as a chain; rescue against a row, not the graph;
 * forward-reverse orientation only; no mapping quality of the pair.
 * Errors, all FBG_ERR_INVALID and leaving the index as it was: a NULL index or which; an index without the row table; the
 * last seeds call was not fbg_pindex_seeds_strands, or none succeeded; no current chaining result since it; n odd;
 * min_insert > max_insert.  FBG_ERR_TOO_LARGE for 2^31 virtual reads or more (a workgroup per virtual read).  n == 0, and
 * all chains empty: every output "none", FBG_OK, nothing launched.  Scratch owned by the index: 97 bytes per virtual
 * read, the windows, and what fbg_pindex_chains_rows keeps per seed and start place. */
int fbg_pindex_pairs_align(fbg_pindex *ix, uint64_t min_insert, uint64_t max_insert, uint32_t max_edits, uint64_t max_window,
                           const uint8_t *select, uint32_t *row, uint32_t *edits, uint32_t *t_start, uint32_t *t_end,
                           uint32_t *insert, uint8_t *which, uint32_t *pair_score, uint32_t *t_lo, uint32_t *t_hi,
                           uint64_t stats[10], double *device_ms);

/* The alignment path (CIGAR) of each read that the last fbg_pindex_chains_align aligned (after a successful
 * fbg_pindex_chains_align since the last fbg_pindex_chains, and so since the last seeds call).
 *
 * For a read R with edits[R] != FBG_ALIGN_NONE let P be its text as that call read it (rc(P_R) for a reverse virtual
 * read), L = |P|, T = G_r[t_start : t_end) and N = |T|.  With unit costs let
 *   E(i, j) = lev(P[i:], T[j:]):   E(L, j) = N - j,  E(i, N) = L - i,
 *   E(i, j) = min(E(i+1, j+1) + [P[i] != T[j]], E(i+1, j) + 1, E(i, j+1) + 1),
 * so that E(0, 0) == edits[R] by the definition of t_start.  The path is the walk from (0, 0) to (L, N) that takes at
 * every cell the first of these moves that keeps the distance:
 *   1. the diagonal, if i < L, j < N and E(i, j) == E(i+1, j+1) + [P[i] != T[j]]: op `=` for equal symbols, else `X`;
 *   2. `I` (a read symbol with no text symbol), if i < L and E(i, j) == E(i+1, j) + 1;
 *   3. `D` (a text symbol with no read symbol) otherwise.
 * Among the optimal alignments it is the smallest in the order diagonal < I < D, read from the read's first symbol on.
 * Equal consecutive ops are merged into runs; a run is one uint32, length << 4 | code, with BAM's codes FBG_CIGAR_I = 1,
 * FBG_CIGAR_D = 2, FBG_CIGAR_EQ = 7, FBG_CIGAR_X = 8, in the order of P and of ascending positions of the row.  It
 * follows that #X + #I + #D == edits, #= + #X + #I == L, #= + #X + #D == t_end - t_start, that a read has at most
 * 2 * edits + 1 runs, and that its first and last run are never D (t_start is the largest start, t_end the smallest
 * end).  A read without an alignment (empty chain, no carrying row, too long, too wide) has zero runs.
 *
 *   fbg_pindex_chains_cigar        n_ops: the number of runs, one entry per read of that align call; *total_ops: their
 *       sum; *device_ms: device time of the kernels.  Any pointer may be NULL.
 *   fbg_pindex_chains_cigar_fetch  off[n + 1], the scan of n_ops, and ops[off[n]], the runs back to back: the
 *       count-then-fetch pattern of fbg_pindex_seeds / _seeds_fetch.  Either may be NULL.
 *   fbg_pindex_cigar_stats         any pointer may be NULL.  Of the last successful fbg_pindex_chains_cigar (0 before the
 *       first; a failing call leaves them): the reads traced; the total number of runs; columns, the sum of N;
 *       history_bytes, the column history that went to device memory and not to LDS; the batches that took.
 * On the device.  A wave per aligned read runs the second pass of fbg_pindex_chains_align again (the reversed read against
 * T reversed with D'(0, j) = j, so D'(a, b) = E(L - a, N - b)), over exactly the N columns of T, and keeps the two
 * vertical-difference words of every 64 read symbols after every column: 16 bytes per word and column.  It then walks
 * from (L, N) of D' towards (0, 0), which is the walk above from the read's first symbol, so the runs come out in output
 * order.  The three cell values a step needs come from the stored words: the cell above from the column's bit, the cell
 * to the left carried along (one row up: less the bit of the column to the left; one column to the left: rebuilt from
 * D'(0, j) = j and the popcounts of that column's words, one word per lane).  Reads of 1 to 4 words (L <= 256) keep the
 * history in LDS, one launch per word count sized by the widest T of that count (N <= 2 L: at most 32 KiB); longer reads
 * up to max_read keep it in scratch of the index, column-major, nw * N * 16 bytes each, and are worked off in batches of
 * consecutive reads whose history fits option path_batch_kib (a read that alone exceeds it is a batch of its own).
 * The runs are traced into 2 * edits + 1 slots per read and compacted after a scan of the counts.  Every loop is
 * bounded (the history by N columns, the trace by L + N steps); a trace that does not arrive writes zero runs and fails
 * the call with FBG_ERR_HIP.
 * The calls may be repeated and leave every other state alone, the align results and stats included; like the align call
 * they still work after a later fbg_pindex_locate or fbg_pindex_occurrences.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index without the row table; no successful fbg_pindex_chains_align since
 * the last fbg_pindex_chains; _fetch without a successful _cigar since that align call.  No reads returns FBG_OK. */
#define FBG_CIGAR_I 1u
#define FBG_CIGAR_D 2u
#define FBG_CIGAR_EQ 7u
#define FBG_CIGAR_X 8u
int fbg_pindex_chains_cigar(fbg_pindex *ix, uint32_t *n_ops, uint64_t *total_ops, double *device_ms);
int fbg_pindex_chains_cigar_fetch(fbg_pindex *ix, uint64_t *off, uint32_t *ops);
int fbg_pindex_cigar_stats(const fbg_pindex *ix, uint64_t *paths, uint64_t *ops, uint64_t *columns, uint64_t *history_bytes,
                           uint64_t *batches);

/* The edit distance of each read to a path of the graph around its chain, and that path (an index built by
 * fbg_pindex_build_segmentation_rows only; after a successful seeds call, plain or stranded, and a successful
 * fbg_pindex_chains or fbg_pindex_chains_by_row since it).
 *
 * fbg_pindex_chains_align aligns a read against one input sequence.  A founder graph also spells the recombinations of
 * its rows, and a read that recombines two of them has no row to be aligned against, or pays for its other half in edits.
 * This call aligns the whole read against the subgraph of the blocks around its chain and answers "where on the graph
 * does this read lie, through which nodes, with how many edits".  Unit costs, both ends free in the graph, the read
 * global; symbols are compared as bytes.  For a (virtual) read R let P be its text as fbg_pindex_chains_align reads it
 * (rc(P_R) for a reverse virtual read) and L = |P|.
 *   anchors    anchor i of the chain is a place in node u_i at offset o_i, of block j_i, of a seed at read offset q_i.
 *   minlen[j]  the shortest label among the nodes of block j, 0 for a block without nodes; C[j] the sum of minlen over
 *              the blocks before j (C[0] = 0, nb + 1 entries).
 *   window     left need of anchor i: max(0, q_i + pad - o_i); right need: max(0, (L - q_i) + pad - (|label(u_i)| - o_i)).
 *              jl = the minimum over the anchors of the largest j <= j_i with C[j_i] - C[j] >= the left need, or 0 if
 *              there is none; jh = the maximum over the anchors of the smallest j >= j_i with C[j + 1] - C[j_i + 1] >= the
 *              right need, or nb - 1 if there is none.  Every path through the blocks jl .. j_i - 1 spells at least the
 *              left need, so no alignment within pad of the anchors' diagonals is cut off.  pad is clamped to 2^33.
 *   H          every node of the blocks jl .. jh with its whole label, and the index's edges between them.  The graph is
 *              layered: an edge joins a node of a block to a node of the next, and node ids ascend block by block.
 *              cells = L * the sum of |label(v)| over H, which is the work.
 *   D_v(i, c)  for node v of H, columns c = 1 .. |label(v)| and read rows i = 0 .. L: D_v(0, c) = 0, and
 *              D_v(i, c) = min(D_v(i-1, c-1) + [P[i-1] != label(v)[c-1]], D_v(i-1, c) + 1, D_v(i, c-1) + 1), where column 0
 *              of v, the column entering v, is the row-wise minimum of the last columns of v's predecessors in H; a
 *              node of block jl, or one without a predecessor in H, enters with D(i) = i.  (The row-wise minimum of
 *              valid columns is a valid column: neighbouring rows still differ by at most 1.)
 *   edits[R]   the minimum of D_v(L, c) over H, or L if no cell is below L.
 *   end        (end_node, end_offset = c): the first cell in (node id, column) order whose D_v(L, c) is strictly below
 *              every earlier one and below L; without such a cell the empty alignment at (first node of block jl, 0).
 *   path       walk back from the end cell: the reversed read against the reversed text of the suffix chosen so far, with
 *              D'(0, x) = x and D'(i, 0) = i.  Inside the current node v, the first offset met walking back (so the
 *              largest; the end offset itself and offset 0 count) at which D'(L, .) == edits is start_offset and ends
 *              the walk with start_node = v.  Otherwise, at v's first symbol, the walk steps to the smallest
 *              predecessor u in H with min_i (F_u(i) + B(L - i)) == edits, F_u the last column of u and B the walk's
 *              column there.  Such a u exists whenever v holds no start.  The path is the nodes from start_node to
 *              end_node, and lev(P, spell(path)[start_offset : up to end_offset in end_node]) == edits.
 * The result is exact over H: no band, no cut-off.  A read without a result has FBG_ALIGN_NONE in the five arrays and
 * n_path 0, and is no error: an empty chain; a read that select leaves out (not_selected counts those with a chain);
 * too long, L > max_read (1024, as fbg_pindex_chains_align); too wide, max_cells != 0 and cells > max_cells, tested after
 * too long.  An anchor whose place lies outside its node's label (none on a graph of a segmentation) is passed over.
 * Limits: no CIGAR over the path from this call (fbg_pindex_chains_graph_cigar, below, traces it afterwards); unit costs
 * only, no affine gaps; every node of the window's blocks is computed, no
 * pruning inside it, so the cost grows with the distinct nodes per block -- on an MSA of a thousand similar rows a block
 * can hold hundreds -- which is what select is for: graph-align the reads the row alignment left out or left poor.
 *
 *   fbg_pindex_chains_align_graph        one entry per read of the last seeds call (2n after fbg_pindex_seeds_strands) in
 *       each of the six arrays; select: that many bytes, non-zero = aligned, or NULL for all; *total_path: the sum of
 *       n_path.  Any output pointer may be NULL.
 *   fbg_pindex_chains_align_graph_fetch  path_off[n + 1], the scan of n_path, and path_nodes[path_off[n]], the paths back to
 *       back from start_node to end_node: count then fetch, as fbg_pindex_chains_cigar / _cigar_fetch.  Either may be NULL.
 *   fbg_pindex_align_graph_stats         any pointer may be NULL.  Of the last fbg_pindex_chains_align_graph (0 before the
 *       first; a call that fails its checks leaves them): reads aligned, not selected, too long, too wide; cells; nodes, the
 *       sum of |H|; merges, the predecessor columns read on entering nodes; path_nodes; then table_bytes, the device bytes of
 *       the predecessor lists and of C (0 until the first call builds them); batches.
 * On the device.  The first call sorts the edges by (destination, source) into a predecessor CSR and scans minlen into
 * C; the index owns both.  One lane per read finds jl and jh by binary searches in C, the node range, the cells and the
 * skip status.  A read's scratch is the two vertical-difference words of every 64 read symbols of every node's last
 * column, |H| * 2 * ceil(L / 64) words; a scan places the reads and the host forms batches of consecutive reads that fit
 * option graph_batch_kib (a batch always takes at least one read).  Per batch, a wave per read runs Myers' recurrence
 * node by node in id order with the state in registers (1 to 4 words) or LDS (up to 16), the label loaded 64 bytes at a
 * time, each byte made wave-uniform by a readlane and its match word one ballot per 64 read symbols.  On entering a node
 * lane l of word w decodes row 64 w + l + 1 of every predecessor's stored column from popcounts, keeps the minimum, and the
 * merged column is encoded again from each lane's difference to the row below by two ballots per word.  A second wave per
 * read runs the reverse recurrence along the chosen suffix, tests every column for a start, and at a node's first symbol
 * evaluates F_u(i) + B(L - i) per predecessor with lanes as rows and a wave minimum.  It writes the nodes into jh - jl + 1
 * slots per read; a scan of n_path and a compaction serve the fetch.  Every loop is bounded by L, a label, a predecessor
 * list or the node range; a walk that finds no predecessor writes no path and fails the call with FBG_ERR_HIP.
 * *device_ms (may be NULL): device time of the kernels, the host's looks at the sizes included.
 * A call may be repeated and leaves the seeds, their places and MSA coordinates, the chains, what the row calls
 * returned, the row alignment and its paths, the occurrences, fbg_pindex_stats, validation results and the context
 * alone; like the align call it still sees the reads of the last seeds call after a later fbg_pindex_locate or
 * fbg_pindex_occurrences.  A later fbg_pindex_chains, fbg_pindex_chains_by_row or seeds call invalidates the result.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index without the row table; no successful chaining call since the last
 * seeds call; _fetch without a successful call since the last chaining call.  FBG_ERR_TOO_LARGE for 2^31 reads or more
 * (a workgroup per read).  No reads returns FBG_OK. */
int fbg_pindex_chains_align_graph(fbg_pindex *ix, uint64_t pad, uint64_t max_cells, const uint8_t *select, uint32_t *edits,
                                  uint32_t *start_node, uint32_t *start_offset, uint32_t *end_node, uint32_t *end_offset,
                                  uint32_t *n_path, uint64_t *total_path, double *device_ms);
int fbg_pindex_chains_align_graph_fetch(fbg_pindex *ix, uint64_t *path_off, uint32_t *path_nodes);
int fbg_pindex_align_graph_stats(const fbg_pindex *ix, uint64_t *aligned, uint64_t *not_selected, uint64_t *too_long,
                                 uint64_t *too_wide, uint64_t *cells, uint64_t *nodes, uint64_t *merges, uint64_t *path_nodes,
                                 uint64_t *table_bytes, uint64_t *batches);

/* The alignment path (CIGAR) of each read that the last fbg_pindex_chains_align_graph aligned, against the stretch of the
 * graph that its path spells (after a successful fbg_pindex_chains_align_graph since the last chaining call).
 *
 * For a (virtual) read R with edits[R] != FBG_ALIGN_NONE let P be its text as that call read it (rc(P_R) for a reverse
 * virtual read) and L = |P|.  spell(path) is the labels of the path's nodes back to back, and
 *   T = spell(path)[start_offset : |spell(path)| - |label(end_node)| + end_offset],   N = |T|:
 * with start_node == end_node it is label[start_offset : end_offset], and for the empty alignment (edits == L, the end and
 * the start at offset 0 of the first node of block jl) it is empty and the path is the single run L I.  By the
 * definition of the graph call lev(P, T) == edits.  The runs are those of fbg_pindex_chains_cigar's definition with this
 * T: E(i, j) = lev(P[i:], T[j:]), the walk from (0, 0) to (L, N) that prefers the diagonal, then I, then D, equal
 * consecutive ops merged, a run length << 4 | code with the FBG_CIGAR_* codes, in the order of P and of the path (for a
 * reverse virtual read: of rc(P_R), which is PAF's and GAF's convention).  It follows that #X + #I + #D == edits,
 * #= + #X + #I == L, #= + #X + #D == N, that a read has at most 2 * edits + 1 runs, that its first and last run are never
 * D (both ends are free in the graph and edits is the minimum), and that N <= L + edits <= 2 L, so the LDS bound of the
 * row call carries over.  A read without a graph alignment has zero runs.  The CIGAR is one over the whole stretch: it
 * is not split node by node.
 *
 *   fbg_pindex_chains_graph_cigar        n_ops: the number of runs, one entry per read of that graph call; *total_ops:
 *       their sum; *device_ms: device time of the kernels.  Any pointer may be NULL.
 *   fbg_pindex_chains_graph_cigar_fetch  off[n + 1], the scan of n_ops, and ops[off[n]], the runs back to back: count
 *       then fetch, as fbg_pindex_chains_cigar / _cigar_fetch.  Either may be NULL.
 *   fbg_pindex_graph_cigar_stats         any pointer may be NULL.  Of the last successful fbg_pindex_chains_graph_cigar (0
 *       before the first; a failing call leaves them), with the meaning of fbg_pindex_cigar_stats: the reads traced; the
 *       total number of runs; columns, the sum of N; history_bytes, the column history that went to device memory and not
 *       to LDS; the batches that took.
 * On the device, from what the graph call left there (edits, the two offsets, the path CSR, L): only the sizes that the
 * launches need come to the host.  One lane per read sums the label lengths of its path into N and lays the read out as
 * the row call's kernels take it; a path that spells no stretch of at most L + edits symbols fails the call with
 * FBG_ERR_HIP.  After a scan of N a wave per read copies T label by label into one text buffer, the lanes along the
 * bytes, the first node clipped by start_offset and the last by N.  The trace is that of fbg_pindex_chains_cigar, the
 * same kernels on (P, T): run slots and history units per read, the history in LDS for reads of 1 to 4 words (one launch
 * per word count, sized by the widest T of that count) and in scratch for longer reads, in batches of consecutive reads
 * that fit option path_batch_kib (which means here what it means there), a scan of the run counts and the compaction.
 * Every loop is bounded; a trace that does not arrive writes zero runs and fails the call with FBG_ERR_HIP.
 * The calls may be repeated and leave every other state alone, the graph alignment and its path, the row alignment and
 * the row CIGAR (whose buffers they do not share) included; like the align calls they still work after a later
 * fbg_pindex_locate or fbg_pindex_occurrences.  A later seeds call, chaining call or fbg_pindex_chains_align_graph
 * invalidates the result.
 * Errors, all FBG_ERR_INVALID: a NULL index; an index without the row table; no successful fbg_pindex_chains_align_graph
 * since the last chaining call; _fetch without a successful _graph_cigar since that graph call.  No reads, or a graph call
 * that left nothing on the device (every chain empty), returns FBG_OK with zeros. */
int fbg_pindex_chains_graph_cigar(fbg_pindex *ix, uint32_t *n_ops, uint64_t *total_ops, double *device_ms);
int fbg_pindex_chains_graph_cigar_fetch(fbg_pindex *ix, uint64_t *off, uint32_t *ops);
int fbg_pindex_graph_cigar_stats(const fbg_pindex *ix, uint64_t *paths, uint64_t *ops, uint64_t *columns, uint64_t *history_bytes,
                                 uint64_t *batches);

/* fbg_segmentation_validate: the semi-repeat-free check (fbg_pindex_validate's rules) of the graph of a segmentation
 * of the current MSA.  cut_bad[k] = 1 iff block k + 1 holds an INVALID node -- the reference's
 * to_remove[node_blocks[i] - 1] (fbg.cpp:3269-3270, 3194); cut_bad[nb - 1] is always 0.  The index is built by
 * fbg_pindex_build_segmentation, validated against its own device-resident node_block, and the cuts are flagged by a
 * kernel over status and node_block: no per-node array goes to the host.  *n_nodes, *n_invalid (INVALID nodes) and
 * *device_ms may be NULL.  *device_ms: time on the stream from the first to the last device operation of the build and
 * the validation, the waits for the sizes the host reads in between included.
 *
 * fbg_segmentation_repair: the loop of fbg.cpp:3471-3497 -- validate, drop the flagged boundaries, repeat until none is
 * flagged.  boundaries / *nb: in and out (the result is a subsequence of the input and keeps its last entry).
 * *rounds = the rounds that removed something (the reference's iterations - 1); removed[r] = boundaries dropped in
 * round r ("There are K blocks to remove"), room for the incoming *nb values; the final round's 0 is not stored.  The
 * loop ends: a round that flags a cut shortens the list, and the nodes of a single block are sources and sinks.  Every
 * round rebuilds the index into the same buffers.  *device_ms (may be NULL): the sum over the rounds.
 * Errors as fbg_pindex_build_segmentation; on an error boundaries / *nb hold the state before the failing round.
 * Both calls leave the context's MSA, its MSA index and every fbg_pindex untouched. */
int fbg_segmentation_validate(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, const uint8_t *ignore_chars,
                              uint64_t ignore_len, uint8_t *cut_bad, uint64_t *n_nodes, uint64_t *n_invalid, double *device_ms);
int fbg_segmentation_repair(fbg_ctx *ctx, uint64_t *boundaries, uint64_t *nb, const uint8_t *ignore_chars, uint64_t ignore_len,
                            uint64_t *rounds, uint64_t *removed, double *device_ms);

#ifdef __cplusplus
}
#endif
#endif /* FBG_HIP_H */
