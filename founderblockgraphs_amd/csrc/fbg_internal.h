// fbg_internal.h -- shared declarations of the MI355X segmentation engine (libfbg_hip.so).
// gfx950 only: 64-wide wavefronts are assumed throughout.
#pragma once
#include <cstddef>
#include <cstring>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/fbg_hip.h"

#define FBG_WAVE 64

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool listed = false;     // in its owner's list (fbg_reserve)
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Pinned bounce buffers for large host <-> device transfers of pageable memory (ctx.hip: fbg_upload / fbg_download)
struct Stager {
    void *base = nullptr;
    size_t slot_bytes = 0;
    int nslots = 0;
    hipEvent_t *ev = nullptr;
    hipStream_t stream = nullptr;
};

struct StageTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    bool recorded = false;
    int launches = 0;
};

// Behaviour switches of one context (fbg_set_option; include/fbg_hip.h lists the keys).  The environment is never
// consulted by the compute code: fbg_ctx_create copies FBG_<KEY> variables into a new context only when
// FBG_DEBUG_ENV=1 is set (ctx.hip, the library's one getenv site).
struct FbgOptions {
    int64_t no_ranked = 0, no_packed = 0, force_wide = 0, full_keys = 0, no_msd_sort = 0, msd_min = -1, bp_min = -1,
            record_scatter = 0, lcp_text = 0, no_aux_stream = 0, rank_no_threshold = 0, dp_literal = 0, dp_wave = 0,
            dp_safe_window = 0, dp_tile = 0, pure_scan = 0, gapped_rank = 0, part_tricks_off = 0, msd_sample_bins = 0, msd_min_force = 0, msd_probe = 0, msd_xcd = -1, rank_no_lean = 0, no_stream_upload = 0,
            span_scan = 0, span_key_flags = 0, span_slow_split = 0, poison = 0, dpw_matrix = 0, dp_chain1 = 0, msd_ext = 1, rows_wave = 0,
            pairs_in_scan = 1, runs_wave_min = 16, wave_list_cap = 0,
            cand_local_sort = 1, cand_lds_cap = 0, cand_sort_check = 0, cand_tail = 1,
            tie_gallop = 1, cand_counts_fused = 1, tie_sample_loop = 1,
            row_count_fast = 1, twin_hash = 1, front_one_fill = 1,
            scan_rows_ahead = 0, msd_cursors = 1, msd_lds_batch = 1,
            path_batch_kib = 1 << 20, byrow_max = 1024, byrow_lds = 0, graph_batch_kib = 1 << 20;
};

// The index at hand: per-position records, or the sorted slots plus per-column maxima of rank_scan.hip / pure_scan.hip
// (ranked), gapped_rank.hip (gapped) or span_scan.hip (span)
enum class IndexKind { none, record, ranked, gapped, span };

// What describes the index a context holds.  fbg_index_reset (ctx.hip) puts a default-constructed value here at the
// top of every build; the stage that finishes an index sets `kind`, once.
struct IndexState {
    bool index_valid = false;
    IndexKind kind = IndexKind::none;
    bool ranked() const { return kind == IndexKind::ranked; }
    bool granked() const { return kind == IndexKind::gapped || kind == IndexKind::span; }
    bool spanned() const { return kind == IndexKind::span; }
    uint32_t *sa_ptr = nullptr;     // u32[N] suffix array (lives in the sort's value buffer)
    uint64_t *rk_keys = nullptr;    // keys (pairs layout, positions in sa_ptr) or key << rk_pb | position (packed)
    int rk_b = 0, rk_key_bits = 0, rk_K = 0;
    int rk_layout = 0, rk_pb = 0;   // FBG_SLOTS_*
    bool grs_flagged = false;       // bit 31 of the sorted values: an irregular position among the K from there on (gapped_rank.hip)
    bool sp_key_flags_sorted = false;   // span scan: the flags W / I are the two lowest bits of the sorted key words
    bool msd_ext_valid = false;     // msd_ext holds the 4 symbols after the key of every slot the MSD sort sorted
    bool lcp_from_keys = false;     // neighbour LCPs came from the sorted keys (few ties) or from text compares
    bool grs_ties_done = false;     // the tie groups of the kept slots are in text order
    uint32_t n_exc = 0;             // exception columns of a ranked index (rows in `exc`)
    // partitioned index (fbg_part_*): this GPU holds the SA slots of key range `part` of `nparts`
    bool part_active = false;
    bool gpart = false;             // ... of an MSA with gaps / ignore characters (gapped_rank.hip)
    int part = 0, nparts = 1;
    uint64_t part_count = 0;        // owned slots (keys / vals arrays: FBG_PART_HALO + part_count + FBG_PART_HALO)
    uint64_t part_T = 0;            // candidates found by phase 1
    uint32_t part_gmin = 0;         // largest threshold any partition scanned with (0: none, nothing to verify)
};

// What the last build did on its way, as fbg_get_option reports it; reset together with IndexState.
struct BuildDiag {
    int64_t msd_decline = -1;    // fbg_msd_sort: -1 not reached, 0 sorted; 1 not tried (geometry), 2 / 4 a stretch of pass 1, 8 the arena of pass 2, 16 a sub-bucket too large
    int pass1_ahead = 0;         // the MSD sort found its pass 1 done (streamed upload)
    int64_t ext_pairs = -1, text_pairs = -1;   // the rank-order scan: tied pairs settled by the msd_ext symbols / by the text
    int64_t sample_twins = -1;   // twins among the keys of the sample before the sort (suffix_sort.hip); -1: no sample was drawn
    int64_t wave_runs = -1;      // the rank-order scan: runs that a wave each walked (k_runs_long)
    int64_t cand_inversions = -1;  // option cand_sort_check: places of the sorted candidate list that do not ascend
    int cand_local_sorted = -1;  // the candidates were sorted region by region in k_cand_sort_compact (1) / by the radix sort (0)
    int cand_tail_used = -1;     // the scan's tail ran by member: k_cand_region, k_cand_lcp, k_cand_runs (1) / the kernels by head (0)
    int rank_lean_launched = 0;  // the rank-order scan launched k_rank_scan_lean ...
    int rank_lean_used = 0;      // ... and finished with it: the index holds its result
    int pairs_rb = -1;           // the sample sort of pairs: rank bits of its table, -1 it did not sort
    int sp_decline = 0;          // why the group-level scan handed the slots back (0: it did not; include/fbg_hip.h "span_decline")
};

// What the round-0 sort of (key, value) pairs carries besides keys and text positions (built in suffix_sort.hip)
struct SortExtras {
    const uint64_t *ebits = nullptr;    // bitmap the pack kernels fold into bit 31 of the values (gapped_rank.hip)
    const uint32_t *payload = nullptr;  // the value of position p is payload[p] (span_scan.hip: cell | flags)
    bool key_flags = false;             // span scan, 2^30 cells and more: sp_flagT[p] goes below the key, in its two lowest bits
};

struct MsdPlan;                         // msd_sort.hip
struct fbg_ctx {
    int device = 0;
    FbgOptions opt;
    std::string err;
    // ---- streams ----
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second stream for work that only raises column maxima (k_tie_simple) beside the candidate kernels
    hipStream_t aux = nullptr;
    hipEvent_t aux_fork = nullptr, aux_join = nullptr;
    bool aux_pending = false;
    uint32_t *pin_pair = nullptr;  // two pinned words the candidates' total and largest count come back into (rank_tail.hip)
    // the twins among the sampled keys come back into two pinned words; twin_ev follows the copy (suffix_sort.hip sample_launch)
    unsigned long long *pin_twins = nullptr;
    hipEvent_t twin_ev = nullptr;
    bool twin_pending = false;
    unsigned long long *pin_front = nullptr;   // the symbol histogram and the three counts of the counting pass, pinned (text_build.hip)
    Stager stager;
    StageTimer timers[FBG_STAGE_COUNT];

    // ---- current MSA (row-major m x n bytes, device) and its text ----
    const uint8_t *d_msa = nullptr;
    DevBuf msa_own;
    uint64_t m = 0, n = 0;
    int reversed = 0;
    bool gapfree = true;
    bool have_ignore = false;
    uint8_t ignore_tab[256] = {0};
    uint64_t N = 0;            // text length incl. sentinel
    uint64_t byte_hist[256] = {0}; // symbol histogram of the current text (fbg_build_text; read by fbg_key_setup)
    bool allow_wide = false;       // the caller can work with text positions beyond 32 bits (partitioned index only)
    uint32_t mp = 0;           // rows padded to a multiple of 64 (column-tile pitch)
    DevBuf text;               // N + 64 bytes, zero padded
    DevBuf pos, tot;           // u32[m]; behind tot (at the next multiple of 8 bytes): the byte histogram of the counting pass, u64[256],
                               // and its counts, u64[8] -- gaps, ignore cells, N (text_build.hip: one fill clears all three)
    DevBuf segtab;             // u32[3][m][segments]: per 65536-column segment of a row: non-gap cells, prefix, first ignore column
    DevBuf colT;               // u32[N]: MSA column of each text position (gapped MSAs only)
    DevBuf gwin_rows;          // u16 per window of 128 positions: the row of its first position (written with the text)

    // ---- a streamed upload (fbg_elastic_f from pinned host memory; text_build.hip): the MSA still on the host while the index
    // build starts, pass 1 of the MSD sort done ahead on the alphabet the first chunk of rows promised (msd_sort.hip fbg_msd_pre_*)
    const uint8_t *up_host = nullptr;
    hipStream_t up_stream = nullptr;
    hipEvent_t up_ev[9] = {};
    bool pre_pass1 = false;
    uint64_t pre_symbols[4] = {0, 0, 0, 0};   // the symbols (bytes of the text) the speculative keys were set up for
    MsdPlan *pre_plan = nullptr;               // KeyGeom + the sort's arguments between fbg_msd_pre_begin and fbg_msd_sort (owned: fbg_msd_pre_free)
    uint64_t pre_tiles = 0;                    // tiles of pass 1 launched so far

    // ---- index state and the diagnostics of the last build: reset by fbg_index_reset at the top of a build ----
    IndexState ix;
    BuildDiag diag;
    // ---- what outlives a build ----
    int key_b = -1, key_K = -1, key_packed = -1, key_compact = -1;   // geometry of the last key setup (fbg_get_option "key_*")
    int dp_kind = -1;              // which sweep produced the last fbg_dp_minmax result (fbg_get_option "dp_kind")
    int dp_attempts = 0;           // sweeps fbg_dp_minmax launched until one settled, the literal one included ("dp_attempts")
    int ne_dp_kind = -1;           // what produced the last fbg_dp_repeatfree result: 0 literal kernel up front, 1 / 2 / 4 the
                                   // matrix path with that R, 8 the matrix path flagged and the literal kernel redid it ("ne_dp_kind")
    bool grs_skip = false;         // the next build takes the record path: the gapped scan ran out of room (scan.hip)
    bool cells_built = false;      // prow / igrow hold the current MSA (built on demand: only the record path reads them)
    uint64_t held_bytes = 0;
    uint64_t alloc_calls = 0, alloc_us = 0;   // device allocations of the context so far and the host time they took (free + malloc)
    std::vector<DevBuf *> bufs;    // every buffer reserved for this context (fbg_reserve); fbg_ctx_destroy walks it

    // ---- per-stage tables: record path (record_sort.hip, lcp.hip, scan.hip) ----
    DevBuf prow;               // u32[m*n]: text pointer of cell (i,x), row-major (gapped MSAs only)
    DevBuf igrow;              // u32[m*n]: first ignore-char column >= x, row-major (ignore chars only)
    DevBuf rec;                // uint4[N] by text position: {rank, lcp-prev | hint<<31, lcp-next | hint<<31, 0}
    DevBuf xlist;              // u32[n+1]: columns whose coloured ranks may contain consecutive integers
    // rank-order scan (rank_scan.hip, rank_tail.hip): kind ranked
    DevBuf gmax, excol, xslot; // u32[n+1]: column maxima of g, exception flags, exception slots
    DevBuf xbits;              // bitmap of the exception columns
    DevBuf exc_scratch;        // per-workgroup column state of k_scan_exceptions_big (MSAs of more than 4096 rows)
    DevBuf exc;                // uint4[n_exc * m]: (rank, lcp_prev, lcp_next) of the rows of the exception columns
    // rank-order scan of MSAs with gaps / ignore characters (gapped_rank.hip): kind gapped
    int grs_tricks_off = 0;        // the setting of the elastic tricks gmax was computed for
    uint32_t grs_ign_lo = 0, grs_ign_hi = 0;
    DevBuf gwin;                   // 16 bytes per 128 text positions: column, row, gap runs
    DevBuf gbits;                  // 1 bit per text position: not the column after its predecessor's
    bool pairs_similar = false;    // the sample of the (key, position) sort says: rows that resemble each other (ties everywhere)
    bool grs_part_failed = false;  // a partition's exact redo of a few columns ran out of room
    uint32_t grs_t = 1;            // the threshold of the last scan (1: none), the columns it redid exactly
    uint64_t grs_redone = 0;
    // group-level scan on column spans for similar rows with gaps / ignore characters (span_scan.hip): kind span
    DevBuf sp_cells;               // u32[N]: cell | flags of every text position, the payload of the sort
    DevBuf sp_flagT;               // u8[N]: the flags alone where the cells take all 32 bits (SortExtras::key_flags)
    DevBuf sp_cwin;                // 20 bytes per 128 cells of a row: text position of a cell
    DevBuf sp_tiles, sp_gstart, sp_gcol, sp_gflags, sp_rstart, sp_rid, sp_gplo, sp_gphi, sp_gval, sp_odd, sp_irr, sp_chain, sp_slow, sp_mins;
    uint32_t sp_chain_n = 0, sp_slow_n = 0;
    uint64_t sp_G = 0, sp_R = 0, sp_n_irr = 0, sp_work = 0;
    uint32_t sp_n_odd[4] = {0, 0, 0, 0}, sp_odd_cap = 0;

    // ---- scratch ----
    DevBuf keysA, keysB, valsA, valsB, grp, flags, list, tie_list, big_groups, tmp, small, scalars;
    DevBuf msd_ext;            // 1 byte per SA slot: symbols K .. K+3 of its suffix (msd_sort.hip, 2-bit symbols)
    DevBuf wave_list;          // the runs that get a wave each (RankArgs::wl)
    DevBuf cand_cf, cand_lp, cand_ln;   // parallel to the sorted candidates: column | run flags, LCP with the slot before, with the slot after (k_cand_lcp)
    DevBuf kargs;              // arguments a kernel reads from memory (k_rank_scan_lean) ...
    alignas(16) unsigned char kargs_host[512];   // ... and the host copy they are sent from
    uint8_t code_host[256];    // fbg_key_setup's code table on its way to the device (kept here: nothing to wait for)
    DevBuf msd_w, msd_v;       // sub-bucket stretches of the MSD sort of 12-byte slots (msd_sort_pairs.hip)
    DevBuf dp_a, dp_b, dp_c, dp_d, dp_e, dp_f, dp_g, dp_h, io_a, io_b, io_c, io_d;
    DevBuf bt_up, bt_dep;      // binary-lifting tables of the parallel backtrack
    DevBuf ps_a, ps_b, ps_c, ps_d, ps_e, ps_f, ps_g, ps_h;   // group / run tables of the scan for similar rows (pure_scan.hip)
};

// ---- error plumbing ----------------------------------------------------------------------
int fbg_fail(fbg_ctx *ctx, int code, const char *fmt, ...);
#define FBG_HIP_TRY(ctx, expr)                                                              \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fbg_fail((ctx), e_ == hipErrorOutOfMemory ? FBG_ERR_OOM : FBG_ERR_HIP,   \
                            "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                            __LINE__);                                                      \
    } while (0)
#define FBG_TRY(expr)                \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != FBG_OK) return rc_; \
    } while (0)

// Grow-only device allocation.  The buffer joins its owner's list on its first successful reserve; the owner frees
// the list (fbg_release_all).  owner = nullptr: no list, the caller releases the buffer by name (group.hip).  accounted:
// in fbg_device_bytes and alloc_calls / alloc_us, with the poison fill -- the context's buffers and a group member's,
// not those of a pattern index or of its build's scratch.
int fbg_reserve(fbg_ctx *ctx, DevBuf &b, size_t bytes, std::vector<DevBuf *> *owner, bool accounted);
inline int fbg_reserve(fbg_ctx *ctx, DevBuf &b, size_t bytes) { return fbg_reserve(ctx, b, bytes, &ctx->bufs, true); }

// The words of FbgScalars::dp (dp.hip, dp_bytes.hip, dp_wide.hip; host and kernels).  fbg_dp_minmax and fbg_dp_gapped use the
// first block, fbg_dp_repeatfree both: DP_NE is the base of a second block of the same shape, of which only the window
// flag is in use -- k_dp_expand's limit test does not hold for the non-elastic values (k_ne_finish decides there), so its
// flag goes to that block, where nobody reads it.
enum : int {
    DP_COUNT = 0,             // boundaries found (the backtracks)
    DP_NO_SEGMENTATION = 1,   // the backtrack left the array / the last column has no value
    DP_BAD_ENTRIES = 2,       // k_dp_keys: entries of f outside [x, n]
    DP_MAX_EXT = 3,           // k_dp_keys: the longest f[x] + 1 - x; k_ne_prep: the longest minimal block
    DP_WINDOW = 4,            // a value reached the limit of the sweep's window: the rung did not settle
    DP_NE = 8,                // + DP_COUNT .. DP_WINDOW: the non-elastic DP's block
    DP_WORDS = 16
};

// ---- the shared scratch words ---------------------------------------------------------------
// ctx->scalars: the device-side counters and flags of every stage, one member per owner.  The members are disjoint
// whichever stages run together; what a stage does with the words of its own member is its business.  A new counter
// gets a new member here (DESIGN.md 4a lists them).  The blocks that kernels add to start a 64-byte line of their own.
struct FbgScalars {
    alignas(64) unsigned long long front[8];     // text_build.hip, front_one_fill = 0: gaps, ignore cells, N
    unsigned long long sample_count;             // suffix_sort.hip: twins in the key sample; the slots a partition keeps
    alignas(64) unsigned long long dp[DP_WORDS]; // dp*.hip (DP_* above): results and flags of the three DPs and of the lifted backtrack
    unsigned long long scan_exceptions;          // scan.hip: exception columns of the record scan
    alignas(64) unsigned long long rank[8];      // rank_common.h / rank_scan.hip, rank_tail.hip: RankArgs::counters ...
    unsigned long long rank_hist[32];            // ... and right behind them the threshold histogram, 64 x u32 (rs_zero_counters: one fill)
    alignas(64) unsigned long long pure[4];      // pure_scan.hip: PsArgs::counters
    alignas(64) unsigned long long msd[4];       // msd_sort.hip, msd_sort_pairs.hip: decline flag, arena count, total of the pairs sort, sub-buckets left for later
    unsigned long long sample_twins;             // msd_sort_pairs.hip: twins in the sample of the pairs sort
    unsigned long long graph_collision;          // block_graph.hip: two labels share a hash
    unsigned long long pair_stats[2];            // rank_scan.hip: tied pairs of the lean scan settled by the extra symbols / by the text
    unsigned long long cand_inversions;          // rank_tail.hip: option cand_sort_check
    unsigned long long by_position;              // record_sort.hip: the records by position are no permutation
    alignas(64) unsigned long long gapped[8 + 66];   // gapped_rank.hip: GrsArgs::counters and the threshold histogram behind them
    alignas(64) unsigned long long span[34];     // span_scan.hip: SpArgs::counters
};
constexpr size_t FBG_SCALARS_WORDS = 256, FBG_SCALARS_BYTES = FBG_SCALARS_WORDS * sizeof(unsigned long long);
static_assert(sizeof(FbgScalars) <= FBG_SCALARS_BYTES, "the scalar words fit their buffer, whose size is part of fbg_device_bytes");
static_assert(offsetof(FbgScalars, rank_hist) == offsetof(FbgScalars, rank) + sizeof(FbgScalars::rank), "one fill clears counters and histogram");
inline int fbg_reserve_scalars(fbg_ctx *ctx) { return fbg_reserve(ctx, ctx->scalars, FBG_SCALARS_BYTES); }
// the device address of the layout: fbg_scalars(ctx)->dp, &fbg_scalars(ctx)->sample_count (never dereferenced on the host)
inline FbgScalars *fbg_scalars(const fbg_ctx *ctx) { return ctx->scalars.as<FbgScalars>(); }

// ctx->small: the byte tables of a build, 2048 bytes apart
struct FbgSmall {
    alignas(2048) uint8_t ignore_tab[256];       // text_build.hip: 1 for an ignore character (ctx->have_ignore)
    alignas(2048) uint8_t code_tab[256];         // suffix_sort.hip fbg_key_setup: the code of every byte (KeyGeom::d_code)
    alignas(2048) unsigned long long hist[256];  // text_build.hip, front_one_fill = 0: the byte histogram of the counting pass
};
constexpr size_t FBG_SMALL_BYTES = 8192;
static_assert(sizeof(FbgSmall) <= FBG_SMALL_BYTES, "the byte tables fit their buffer");
inline FbgSmall *fbg_small(const fbg_ctx *ctx) { return ctx->small.as<FbgSmall>(); }

// rocPRIM's calling pattern: ask for the temporary size, grow `tmp` (on `owner`'s list, accounted or not: fbg_reserve), call
// again with the buffer.  call(void *tmp, size_t &bytes) holds the one argument list both calls use.
template <class F> int fbg_with_tmp(fbg_ctx *ctx, DevBuf &tmp, std::vector<DevBuf *> *owner, bool accounted, F &&call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return fbg_fail(ctx, FBG_ERR_HIP, "rocprim size query: %s", hipGetErrorString(e));
    FBG_TRY(fbg_reserve(ctx, tmp, bytes, owner, accounted));
    size_t have = tmp.cap;
    e = call(tmp.p, have);
    if (e != hipSuccess)
        return fbg_fail(ctx, e == hipErrorOutOfMemory ? FBG_ERR_OOM : FBG_ERR_HIP, "rocprim call: %s", hipGetErrorString(e));
    return FBG_OK;
}
template <class F> int fbg_with_tmp(fbg_ctx *ctx, F &&call) { return fbg_with_tmp(ctx, ctx->tmp, &ctx->bufs, true, call); }   // the context's own tmp

void fbg_release(fbg_ctx *ctx, DevBuf &b);                         // ctx = nullptr: a buffer outside the context's accounting
void fbg_release_all(fbg_ctx *ctx, std::vector<DevBuf *> &bufs);   // ... every buffer of a list
void fbg_index_reset(fbg_ctx *ctx);                                // ctx.hip: the top of a build, nowhere else
// blocking host <-> device copies; pageable memory of 32 MB and more goes through pinned bounce buffers filled by
// several host threads (the runtime's own staging of pageable memory is a single-threaded memcpy)
int fbg_upload(fbg_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int fbg_download(fbg_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int fbg_stage_begin(fbg_ctx *ctx, int stage);
int fbg_stage_end(fbg_ctx *ctx, int stage, int launches);

#define FBG_SLOTS_PAIRS 0    // keys[k] = key, vals[k] = position (32 bits)
#define FBG_SLOTS_PACKED 1   // keys[k] = key << pb | position
#define FBG_SLOTS_WIDE 2     // keys[k] = key << pb | position >> 32, vals[k] = low 32 bits of the position
// Key geometry of the round-0 sort.  compact: separators ('#', sentinel) share code 0 with the smallest symbol and
// blank the rest of the key (rank_scan.hip undoes the ambiguity with the row arithmetic of gap-free MSAs);
// packed: one 64-bit word per suffix, key << pb | position, sorted by its key bits only.
struct KeyGeom {
    int b = 0, K = 0, key_bits = 0;
    bool compact = false, packed = false;
    bool wide = false;            // (key word, low position word) pairs, key << pb | position >> 32: texts of 2^32 symbols and more
    int pb = 0;
    const uint8_t *d_code = nullptr;
};

// the sorted slots a rank-order index keeps (layout: FBG_SLOTS_*; pb = 0 in the pairs layout)
inline void fbg_remember_slots(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, int layout, const KeyGeom &g)
{
    ctx->ix.rk_keys = keys; ctx->ix.sa_ptr = vals; ctx->ix.rk_layout = layout; ctx->ix.rk_pb = g.pb;
    ctx->ix.rk_b = g.b; ctx->ix.rk_key_bits = g.key_bits; ctx->ix.rk_K = g.K;
}

// the geometry fbg_get_option reports as key_b / key_K / key_packed / key_compact
inline void fbg_note_key_geom(fbg_ctx *ctx, const KeyGeom &g)
{
    ctx->key_b = g.b; ctx->key_K = g.K; ctx->key_packed = g.packed ? 1 : 0; ctx->key_compact = g.compact ? 1 : 0;
}

// ---- stages (each in its own translation unit) ----------------------------------------------
int fbg_build_text(fbg_ctx *ctx, const uint8_t *ignore, uint64_t ignore_len);  // text_build.hip
int fbg_suffix_sort(fbg_ctx *ctx);                                            // suffix_sort.hip
int fbg_neighbour_lcp(fbg_ctx *ctx);                                          // lcp.hip
int fbg_rank_scan_try(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, const KeyGeom &g, int *done);       // rank_scan.hip
int fbg_pure_scan_try(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, const KeyGeom &g, int *done);       // pure_scan.hip
int fbg_rank_finish(fbg_ctx *ctx, uint64_t x0, uint64_t x1, int mode, int disable_tricks, uint64_t *d_out);
int fbg_rank_materialize(fbg_ctx *ctx, uint32_t *d_sa, uint32_t *d_isa, uint32_t *d_pl, uint32_t *d_pr);
#define FBG_STAGE_RANKSCAN FBG_STAGE_TILE
int fbg_grs_prepare(fbg_ctx *ctx, const uint64_t **ebits, int *launches);   // *ebits = nullptr: no flag bit in the values
int fbg_grs_part_classify(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t count, const KeyGeom &g, int eligible, uint8_t *d_blob, int *ok);
int fbg_grs_part_scan(fbg_ctx *ctx, const uint8_t *d_blobs, uint32_t *d_gmax, int *ok);
int fbg_grs_part_unfilled(fbg_ctx *ctx, uint64_t *unfilled);
int fbg_grs_part_rescan(fbg_ctx *ctx);
int fbg_grs_strip(fbg_ctx *ctx, uint32_t *vals);
int fbg_grs_try(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, const KeyGeom &g, int *done);             // gapped_rank.hip
int fbg_grs_finish(fbg_ctx *ctx, uint64_t x0, uint64_t x1, int disable_tricks, uint64_t *d_out, int *ok);
int fbg_grs_materialize(fbg_ctx *ctx, uint32_t *d_sa, uint32_t *d_isa, uint32_t *d_pl, uint32_t *d_pr);
bool fbg_span_eligible(fbg_ctx *ctx, const KeyGeom &g);
bool fbg_span_key_flags(fbg_ctx *ctx, KeyGeom &g);                                                 // span_scan.hip
int fbg_span_prepare(fbg_ctx *ctx, const KeyGeom &g, const SortExtras &x, int *launches);
int fbg_span_try(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, const KeyGeom &g, int *done);
int fbg_span_rescan(fbg_ctx *ctx, int disable_tricks, int *ok);
int fbg_build_cell_tables(fbg_ctx *ctx);                                                                // text_build.hip
int fbg_key_setup(fbg_ctx *ctx, bool compact, KeyGeom *g, int *launches);                                // suffix_sort.hip
int fbg_record_sort(fbg_ctx *ctx, const KeyGeom &g, int *launches);                                      // record_sort.hip
// equal neighbours among the S keys of a sorted sample (suffix_sort.hip), counted in the caller's scalar word and brought back;
// a suffix with a twin somewhere is a sample twin with probability S / N: twins * N / S^2 estimates the fraction that ties
int fbg_count_equal_neighbours(fbg_ctx *ctx, const uint64_t *sorted, uint64_t S, unsigned long long *d_word, unsigned long long *twins);
inline bool fbg_twins_say_similar(uint64_t twins, uint64_t N, uint64_t S) { return (double)twins * (double)N / ((double)S * (double)S) > 0.5; }
int fbg_rank_part_classify(fbg_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t count, const KeyGeom &g, int pre_ok,
                           uint8_t *d_blob, int *ok);                         // rank_scan.hip
int fbg_rank_part_runs(fbg_ctx *ctx, const uint8_t *d_blobs, uint32_t *d_gmax, int *ok);
int fbg_rank_part_unfilled(fbg_ctx *ctx, uint64_t *unfilled);
int fbg_rank_part_rescan(fbg_ctx *ctx);
int fbg_part_sort(fbg_ctx *ctx, int part, int nparts, uint8_t *d_blob, int *ok);
int fbg_msd_sort(fbg_ctx *ctx, const KeyGeom &g, uint64_t **sorted, int *ok, int *launches);         // msd_sort.hip
int fbg_msd_pre_begin(fbg_ctx *ctx, int *ok);                     // pass 1 ahead of the rest, on a text that is still arriving
int fbg_msd_pre_pass1(fbg_ctx *ctx, uint64_t avail);              // ... over the tiles whose positions (and 64 beyond) are below avail
bool fbg_msd_pre_geom(fbg_ctx *ctx, KeyGeom *g);                  // the key geometry it used, if pass 1 was done ahead
void fbg_msd_pre_free(fbg_ctx *ctx);                              // the plan kept between those calls (fbg_ctx_destroy)
int fbg_msd_sort_part(fbg_ctx *ctx, const KeyGeom &g, uint64_t lo, uint64_t hi, int nohi, int nparts, uint64_t out_offset,
                      uint64_t *count, int *ok, int *launches);                                       // msd_sort_pairs.hip
int fbg_sample_sort_pairs(fbg_ctx *ctx, const KeyGeom &g, const SortExtras &x, int *ok, int *launches);                      // msd_sort_pairs.hip
int fbg_scan_columns(fbg_ctx *ctx, uint64_t x0, uint64_t x1, int mode, int disable_tricks,
                     uint64_t *d_out);                                        // scan.hip
int fbg_dp_minmax(fbg_ctx *ctx, const uint64_t *d_f, uint64_t n, uint64_t *d_boundaries,
                  uint64_t *count_out, uint64_t *d_mml, uint64_t *d_bt);      // dp.hip
// k_dp_blockW / k_dp_compose / k_dp_chain6 (k_dp_chain under dp_chain1) / k_dp_expand with R = 1, 2 or 4 (dp_bytes.hip)
int fbg_dp_byte_chain(fbg_ctx *ctx, int R, const uint8_t *ext, const uint8_t *amin, uint64_t n, uint32_t Fg, uint8_t *Sg, uint32_t *out,
                      unsigned long long *flag, uint32_t first_valid);
// block_graph.hip: where the device stage of fbg_block_graph left the graph of a segmentation (the context's dp_* / io_a
// workspaces).  edges: edge_count[j] sorted distinct (source << 32 | destination) at edges[j * m ..], global node numbers.
struct BlockGraphDev {
    const uint64_t *bounds = nullptr;              // [nb]
    const uint32_t *node_of = nullptr, *rep_row = nullptr, *count = nullptr;   // [nb * m], [nb * m], [nb]
    const unsigned long long *first = nullptr, *edge_count = nullptr, *edges = nullptr;   // [nb + 1], [nb], [nb * m]
    uint64_t n_nodes = 0;
    bool collision = false;                        // two different labels share a hash: the numbering is not to be used
};
int fbg_block_graph_device(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, BlockGraphDev *g);
int fbg_dp_repeatfree(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s,
                      uint64_t *d_prev, uint64_t *d_boundaries, uint64_t *count_out);
int fbg_gapped_v_from_f(fbg_ctx *ctx, const uint64_t *d_f, uint64_t n, uint64_t *d_v);
int fbg_dp_gapped(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s, uint64_t *d_prev,
                  uint64_t *d_boundaries, uint64_t *count_out);

#define FBG_SCAN_F 0
#define FBG_SCAN_V 1

static inline unsigned fbg_blocks(uint64_t work, unsigned per_block, unsigned cap = 0x7fffffffu)
{
    uint64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}
