// pindex.h -- what the files of the pattern index (fbg_pindex_*) share: constants, the index object and the state of
// every stage, the kernel argument structs, three host helpers and the few host functions that cross files.
//   pindex_build.hip      edge text, suffix array, occ lines, B / E; the preparation from a segmentation; create, destroy
//   locate.hip            the batched search: locate, occurrences, seeds, and the expansion of places
//   pindex_validate.hip   the semi-repeat-free check of an index; validation and repair of a segmentation
//   pindex_chain.hip      co-linear chaining of a read's seeds, strands
//   pindex_rows.hip       the MSA rows that carry a start place or a chain
//   pindex_byrow.hip      chaining along one row: per read the row whose supported anchors chain best
//   pindex_align.hip      edit distance of a read to a row of its chain, and the alignment path
//   pindex_graph.hip      edit distance of a read to a path of the graph around its chain, and that path
//   pindex_gcigar.hip     the alignment path of a read against the stretch of the graph that path spells
//   pindex_mapq.hip       the second-best chain of a read outside the columns of its best one, and a mapping quality
//   pindex_pairs.hip      paired reads: a mate's chain rescued in the insert window of the other's, the pick per pair, adopt
//   pindex_pairs_align.hip   paired reads: a mate without a chain aligned in the insert window on the row of the other's chain
// Device helpers shared by kernels of several files: pindex_dev.h.  A kernel is defined in one file; another file that
// needs its launch calls a launcher declared at the end of this header.
// Two things tie the stages together.  The reads of the last seeds call lie in buffers of their own (PsState batch), which
// every later stage reads through ps_reads / ps_roff and no other search writes.  Whether a stage's result is current is
// kept in one table (pindex_stage.h, fbg_pindex::done): a producing call begins its stage (px_begin), which makes every
// result made from it stale, and finishes it (px_finish) where it has succeeded; a call that reads a result needs it (px_need).
#pragma once
#include "fbg_internal.h"
#include "pindex_stage.h"
#include <algorithm>
#include <vector>

#define PX_THREADS 256
#define PX_BLK 128            // BWT positions per occ block
#define PX_LINE 128           // bytes per occ line
#define PX_ABSENT 0xffffu     // code of a byte that does not occur in the text
#define PV_OUT 1u             // node flags of the validation tables: has an out-edge / an in-edge
#define PV_IN 2u
#define PV_CSHIFT 8           // the coarse edge table holds the edge of every 2^PV_CSHIFT-th text position
#define PV_SHORT 16           // ranges of at most this many slots are scanned by one lane, longer ones by a wave
#define PV_NONE 0xffffffffu   // no witness
#define PM_W 8                // the MSA coordinate table keeps a running non-gap count every PM_W bitmap words (512 columns)
#define PM_NONE 0xffffffffu   // a node without a bitmap (no gap in its row's stretch); the coordinate of no cell
#define PC_SUB 16             // chaining: lanes that share a read of the small tier
#define PC_SMALL 32           // start places of a read up to which PC_SUB lanes chain it (small_max)
#define PC_LDS 1024           // start places of a read up to which a wave chains it with its state in LDS (lds_max)
#define PC_NONE 0xffffffffu   // no predecessor / no chain end
#define PR_SUB 16             // rows: lanes that share a place (or a chain) when the MSA has at most this many rows
#define PR_NONE 0xffffffffu   // no node in a (row, block) cell (BG_NONE of block_graph.hip); no supporting row
#define PB_LDS 32             // chaining by row: start places of a read up to which its state stays in LDS (lds_max)
#define PB_PLACE 280          // ... bytes of that state per start place: a record, a support word, 64 scores
#define PB_CTR 7              // ... counters: reads without a place, of the LDS tier, of the device tier, with too many;
                              // places of the device tier; reads with an anchor and no row; places kept by the mask
#define PA_MAX_READ 1024      // alignment: the longest read fbg_pindex_chains_align takes (max_read), a multiple of 64
#define PA_REG_WORDS 4        // reads of up to this many 64-symbol words keep the bit-vector state in registers
#define PA_NONE 0xffffffffu   // FBG_ALIGN_NONE
#define PG_CTR 13              // counters of fbg_pindex_chains_cigar: traces that failed, reads traced, columns, reads of 1 .. 4
                              // words and of more, the widest T of each of the five

#define PH_CTR 13             // counters of fbg_pindex_chains_align_graph: traces that failed, reads aligned, not selected, too long,
                              // too wide, cells, nodes, merges, and the reads of 1 .. 4 words and of more
#define PH_NONE 0xffffffffu   // no predecessor chosen
#define PQ_CTR 5              // counters of fbg_pindex_chains_mapq: anchors kept, anchors excluded, reads with a secondary chain,
                              // reads of mapping quality 0 and of 60
#define PQ_NOSPAN 0xffffffffffffffffull   // lo of a read without a primary chain
#define PP_CTR 8              // counters of fbg_pindex_chains_pairs, as its stats[]: pairs of candidate 0 .. 3, pairs without one,
                              // places kept, places excluded, pairs whose rescue chain scores other than that read's primary
#define PP_NOPAIR 0xffu       // which of a pair without a valid candidate
#define PP_KEEP 0             // adopt, per virtual read: its chain stays (pair without a candidate); the chosen primary chain
#define PP_PRIMARY 1          // stays; the chosen rescue chain replaces it; the twin of a chosen read gets the empty chain
#define PP_RESCUE 2
#define PP_TWIN 3
#define PL_CTR 11             // counters of fbg_pindex_pairs_align, as its stats[]: reads selected, aligned, whose partner has no row,
                              // empty, too long, too wide, rejected by edits, rejected by insert; cells; pairs with a candidate;
                              // and, not reported, the non-empty chains without a row (what k_pr_chain counts)

// What k_po_sizes leaves for k_po_expand, for n items (the patterns of fbg_pindex_occurrences, or the seeds of
// fbg_pindex_seeds): totals, capped sizes and their scans, the first slot of either list, k or the length, restarts;
// and the places of the last fetch.  Grow-only, on the index's buffer list.
struct PoState {
    DevBuf etot, stot, esz, ssz, eoff, soff, rs, el, ss, sk, place;
    DevBuf msa;               // the rows and columns of the last fbg_pindex_occurrences_msa / _seeds_msa, apart from place
    uint64_t n = 0, etotal = 0, stotal = 0;
};

// fbg_pindex_chains: per start place of the last fbg_pindex_seeds its MSA row and column (col: rows first, a copy apart
// from sd.msa) and its predecessor; per read the binning keys and ids (before and after the sort), the chain's end
// place, score and length, the scan of the lengths; the chains (places, then seeds); the spill tier's slab (a uint4 per
// start place, reserved when a read needs it); the counters of k_pc_key and k_pc_chain.  fbg_pindex_chain_strands: per
// given read its strand and best score, and the three counters of k_pc_strand.  band: that of the last pc_reserve.
struct PcState {
    DevBuf col, pred, key, id, key2, id2, end, score, len, off, out, slab, ctr;
    DevBuf strand, best, sctr;
    uint64_t n = 0, total = 0, anchors = 0, tier[3] = {0, 0, 0}, band = 0;
};

// The row table of fbg_pindex_build_segmentation_rows: node_of[nb * m], block-major, and the gathered labels with their
// offsets (a node without an edge has no copy of its label in the index text).  sbase: per seed the byte of the reads its
// substring starts at; rec: per start place (node, offset in the node, seed, block) or PR_NONE first; out / cout: what
// the last fbg_pindex_seeds_rows / _chains_rows copied out; ctr: its count of empty sets.
struct PrState {
    DevBuf node_of, labels, loff, sbase, rec, out, cout, ctr;
    uint64_t m = 0, label_bytes = 0, places_unsupported = 0, chains_unsupported = 0;
};

// fbg_pindex_chains_align.  pref: p(r, j) as uint32[nb * m], block-major like node_of, built by the first call.  Per read
// of the last seeds call: nrows / first (what k_pr_chain leaves: the row choice), info = (row, w0, |W| or 0 where nothing
// is aligned, L), start = (block, node, offset in the node) at which w0 falls, wlen and its scan woff (n + 1 each), out
// (row, edits, t_start, t_end: 4 n); win: the windows, back to back; ctr: non-empty chains without a row, reads aligned,
// too long, too wide, and the cells.  A current result (PS_ALIGN) is for n reads; on_device: the call left info, woff, win
// and out for them, which it did not where it returned before its first kernel.
struct PaState {
    DevBuf pref, nrows, info, start, wlen, woff, win, out, ctr;
    bool has_pref = false, on_device = false;
    uint64_t n = 0;
    uint64_t stat[5] = {0, 0, 0, 0, 0};
};

// fbg_pindex_chains_cigar.  Per read of the last align call: sz (history units of 8 bytes, then run slots; n + 1 each)
// and their scans hoff / soff, cnt (runs as u64, n + 1) and its scan off, nops (runs as u32); slots: 2 * edits + 1 runs
// per aligned read; ops: the runs back to back; hist: the column history of one batch of long reads; ctr: PG_CTR
// counters.  A current result (PS_CIGAR; PS_GCIGAR for the state of the graph call) is for n reads and total runs
// (on_device as above).
struct PgState {
    DevBuf sz, hoff, soff, cnt, off, nops, slots, ops, hist, ctr;
    bool on_device = false;
    uint64_t n = 0, total = 0;
    uint64_t stat[5] = {0, 0, 0, 0, 0};      // paths, ops, columns, history_bytes, batches
};

// fbg_pindex_chains_by_row.  Per read of the last seeds call: row, score and nbest (what k_pb_score leaves), the binning
// keys and ids before and after the sort; doff: the scan of the device tier's place counts, slab: that tier's state
// (PB_PLACE bytes per place, reserved when a read needs it); col2: the start columns under the mask of the chosen rows,
// which the chain DP runs on; ctr: PB_CTR counters.
struct PbState {
    DevBuf row, score, nbest, key, id, key2, id2, doff, slab, col2, ctr;
    uint64_t stat[5] = {0, 0, 0, 0, 0};      // reads_lds, reads_device, reads_too_many, reads_no_row, anchors_kept
};

// fbg_pindex_chains_align_graph.  Tables, built by the first call: pin_off (u32[n_nodes + 1]) and pin (u32[E]), the
// predecessors of every node in ascending order; C (u64[nb + 1]), the scan of the shortest label of every block; keys:
// the edges as dst << 32 | src before and after their sort.  Per read of the last chaining call: info = (first node of
// H, one past its last, L or 0 where nothing is aligned, jl); sz (scratch words, then path slots; n + 1 each) and their
// scans soff / poff; out: edits, start node and offset, end node and offset, n_path (6 n); cnt (n_path as u64, n + 1) and
// its scan off; slots: the traced nodes, end first; path: the paths back to back; scratch: the last columns of one
// batch; sel: the caller's mask; ctr: PH_CTR counters.  A current result (PS_GRAPH) is for n reads and total path nodes;
// on_device: the call left off and path for them.
struct PhState {
    DevBuf pin_off, pin, C, keys, info, sz, soff, poff, out, cnt, off, slots, path, scratch, sel, ctr;
    bool has_tab = false, on_device = false;
    uint64_t n = 0, total = 0;
    uint64_t stat[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};     // aligned, not_selected, too_long, too_wide, cells, nodes, merges, path_nodes, batches
};

// fbg_pindex_chains_graph_cigar.  Per read of the last graph call, in the shape k_pg_sizes and k_pg_path read of the row
// call: info = (0, 0, N, L), out (4 n: unused, edits, 0, N), wlen = N or 0 and its scan woff (n + 1 each); text: the
// stretches T, back to back; bad: the count of paths that spell no such stretch; g: the sizes, slots, runs and history
// of the trace, a PgState of this call's own.
struct PjState {
    DevBuf info, out, wlen, woff, text, bad;
    PgState g;
};

// fbg_pindex_chains_mapq.  ch: a chain state of this call's own, in which the chain kernels leave the secondary chains
// (ch.col: the witness rows and columns, expanded again); span: per read lo and hi of its primary chain as u64 (2 n,
// PQ_NOSPAN in lo for an empty chain); mcol: per start place its witness column, or PC_NONE where the anchor is excluded;
// span2: second_lo, then second_hi (2 n); mapq / smapq: the mapping quality per read, and the stranded one; ctr: PQ_CTR
// counters.  A current result (PS_MAPQ) is for n reads and total secondary anchors; on_device: the call left its arrays on
// the device, which it did not where it launched nothing.
struct PqState {
    PcState ch;
    DevBuf span, mcol, span2, mapq, smapq, ctr;
    bool on_device = false;
    uint64_t n = 0, total = 0;
    uint64_t stat[5] = {0, 0, 0, 0, 0};      // reads_with_second, anchors_kept, anchors_excluded, mapq0, mapq60
};

// fbg_pindex_chains_pairs.  ch: a chain state of this call's own, in which the chain kernels leave the rescue chains
// (ch.col: the witness rows and columns, expanded again); span: lo and hi as u64, PQ_NOSPAN in lo for an empty chain, of
// the primary chains (2 V, V the virtual reads) and then of the rescue chains (2 V); mcol: per start place its witness
// column, or PC_NONE outside the window; rspan: rescue_lo, then rescue_hi (2 V u32); pick: per pair pair_score, t_lo,
// t_hi (3 P u32, P = V / 4 pairs); which: per pair the candidate; src: per virtual read what adopt does with it (PP_KEEP
// ..); ctr: PP_CTR counters in the order of stats[].  Nothing outlives the call: it returns all of it.
struct PpState {
    PcState ch;
    DevBuf span, mcol, rspan, pick, which, src, ctr;
};

// fbg_pindex_pairs_align, V virtual reads and P = V / 4 pairs.  nrows / first (2 V, what k_pr_chain leaves: the row choice);
// frag: per virtual read (r, fs, fe, |G_r|), r = PR_NONE without a chain or a row; info, start, wlen, woff, win and out (row,
// edits, t_start, t_end: 4 V) as in PaState, for the selected reads over their insert windows; ins: the insert per read;
// pick: per pair pair_score, t_lo, t_hi (3 P); which: per pair the candidate; sel: the caller's mask; ctr: PL_CTR counters.
// Nothing outlives the call: it returns all of it.
struct PlState {
    DevBuf nrows, frag, info, start, wlen, woff, win, out, ins, pick, which, sel, ctr;
};

// The reads of the last fbg_pindex_seeds / _seeds_strands, in buffers that only a seeds call writes: reads (bytes of them,
// padded as px_front pads) and roff (n + 1 byte offsets).  n: the reads on the device, with _strands the 2 x given virtual
// ones (stranded); comp: the complement table of that call (256 bytes).
struct PsState {
    DevBuf reads, roff, comp;
    uint64_t n = 0, bytes = 0;
    bool stranded = false;
};

struct fbg_pindex {
    fbg_ctx *ctx = nullptr;
    uint64_t N1 = 0;          // text length including the sentinel
    int sigma = 0;            // distinct symbols of the text
    bool compact = false;     // sigma <= 16: counts inside the line
    uint64_t nblk = 0;        // occ blocks: N1 / 128 + 1 (the last one answers occ(c, N1))
    uint64_t n_nodes = 0;
    uint32_t nb = 0, ne = 0;
    DevBuf text, sa, lines, cnt_tab, C, code, bpos, epos;
    DevBuf pats, poff, okey, oval, okey2, oval2, cnt_out, pos_out, lines_ctr, tmp;     // pats / poff: of locate and occurrences
    // kept for fbg_pindex_validate (not in index_bytes): per node the SA range of its label, a text position of the
    // label, its length and in / out flags; per distinct edge its text start (E + 1), source and destination; a
    // coarse table of the edge at every 2^PV_CSHIFT-th text position
    DevBuf vrng, vtpos, vlen, vflag, vestart, vesrc, vedst, vctab;
    DevBuf vblock, vstatus, vwn, vwo, vlist, vctr;      // validation scratch, kept between calls
    // an index built from a segmentation (fbg_pindex_build_segmentation) keeps the block of every node and the first
    // node of every block; scut / sctr: the flagged cuts and the INVALID count of fbg_segmentation_validate
    DevBuf snode_block, sfirst, scut, sctr;
    bool from_segmentation = false;
    uint64_t seg_nb = 0;
    // the MSA coordinate table of fbg_pindex_build_segmentation (not in index_bytes, not in table_bytes): mnode, one
    // uint4 per node (representative row, first column of the block, first unit of the node's bitmap or PM_NONE, width
    // of the block); mbits, u64 units: per gapped node, for every PM_W bitmap words, the non-gap cells before them and
    // then those words
    DevBuf mnode, mbits;
    bool has_map = false;
    uint64_t map_units = 0, map_gapped = 0;
    // fbg_pindex_occurrences: the walk's record per pattern (3 x uint2) and the place state of its patterns;
    // fbg_pindex_seeds: per pattern the number of reported seeds and its scan, per seed what the walk wrote (the same
    // record, count, length as u64 for k_po_sizes, q_start, length) and the place state of the seeds.  The two place
    // states never share a buffer: a fetch of one is not disturbed by a search of the other.
    DevBuf orec;
    PoState occ;
    DevBuf snum, soff, srec, scnt, spos, sq, slen;
    PoState sd;
    PsState batch;
    bool done[PS_COUNT] = {};     // the stages whose result is current: written by px_begin and px_finish only
    PcState ch;
    bool has_rows = false;        // built by fbg_pindex_build_segmentation_rows
    PrState rw;
    PaState al;
    PgState cg;
    PbState pb;
    PhState gr;
    PjState gj;
    PqState pq;
    PpState pp;
    PlState pl;
    uint64_t n_edges = 0, nctab = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, sv0 = nullptr, sv1 = nullptr;   // made with the index (px_new)
    std::vector<DevBuf *> bufs;   // the index's own device buffers: outside the context's workspaces and its accounting
    double build_ms = 0, search_ms = 0, validate_ms = 0;
    uint64_t occ_lines = 0, v_slots = 0, v_wave_nodes = 0;
};

// not in the library's dynamic symbol table: the host functions of the pattern index that cross files
#define PX_LOCAL __attribute__((visibility("hidden")))

// Grow-only, on the index's buffer list, outside the context's accounting
static inline int px_reserve(fbg_pindex *ix, DevBuf &b, size_t bytes) { return fbg_reserve(ix->ctx, b, bytes, &ix->bufs, false); }

template <class F> static int px_with_tmp(fbg_pindex *ix, F &&call) { return fbg_with_tmp(ix->ctx, ix->tmp, &ix->bufs, false, call); }

// The table of pindex_stage.h on the index.  px_need: FBG_OK where stage y and every stage it was made from are current;
// else the call `who` fails, naming the first call on the way to y whose result is missing or stale.
static inline void px_begin(fbg_pindex *ix, PsStage x) { ps_begin(ix->done, x); }
static inline void px_finish(fbg_pindex *ix, PsStage x) { ps_finish(ix->done, x); }
static inline bool px_current(const fbg_pindex *ix, PsStage y) { return ps_missing(ix->done, y) == PS_COUNT; }
static inline int px_need(const fbg_pindex *ix, const char *who, PsStage y)
{
    const int miss = ps_missing(ix->done, y);
    if (miss == PS_COUNT) return FBG_OK;
    return fbg_fail(ix->ctx, FBG_ERR_INVALID, "%s: no current %s result (none yet, or an earlier stage has run again since)", who,
                    ps_table[miss].call);
}

// px_need on an index that must have the row table (fbg_pindex_build_segmentation_rows)
static inline int px_need_rows(const fbg_pindex *ix, const char *who, PsStage y)
{
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation_rows has the row table", who);
    return px_need(ix, who, y);
}

// The reads of the last seeds call, for every stage after it
static inline const uint8_t *ps_reads(const fbg_pindex *ix) { return ix->batch.reads.as<uint8_t>(); }
static inline const uint64_t *ps_roff(const fbg_pindex *ix) { return ix->batch.roff.as<uint64_t>(); }

// The device time of a call lies between ev0 and ev1.  The stage records ev0 where its device work starts and calls
// px_record_end after its last kernel, before it queues the copies to the host, and px_sync_elapsed after them: the
// stream is waited for and the time between the events goes to *ms (may be NULL).
static inline int px_record_end(fbg_pindex *ix) { FBG_HIP_TRY(ix->ctx, hipEventRecord(ix->ev1, ix->ctx->stream)); return FBG_OK; }
static inline int px_sync_elapsed(fbg_pindex *ix, double *ms)
{
    FBG_HIP_TRY(ix->ctx, hipStreamSynchronize(ix->ctx->stream));
    float f = 0;
    FBG_HIP_TRY(ix->ctx, hipEventElapsedTime(&f, ix->ev0, ix->ev1));
    if (ms) *ms = f;
    return FBG_OK;
}

// ---- kernel arguments ---------------------------------------------------------------------------------------------
// what the backward steps read (pindex_dev.h)
struct PxDev {
    const uint8_t *lines;
    const uint32_t *cnt_tab;
    const uint32_t *bpos, *epos;
    uint32_t N, nb, ne, S;
};

// the tables of the validation and of the expansion of places
struct PvDev {
    const uint32_t *sa, *tpos, *len, *estart, *esrc, *edst, *ctab, *block;
    const uint2 *rng;
    const uint8_t *flag, *text;
};

struct PvMask {
    uint64_t w[4];
};

struct PmDev {
    const uint4 *node;
    const uint64_t *bits;
};

// Read R has the seeds seed_off[R] .. seed_off[R + 1] and, as its candidate anchors, their capped start places
// g0 = start_off[seed_off[R]] .. start_off[seed_off[R + 1]]: the places of earlier seeds first, a seed's places in slot
// order.  A place whose column is PC_NONE is no anchor; it keeps its slot with best = 0, which no comparison picks.
struct PcDev {
    const uint64_t *seed_off, *start_off;
    const uint32_t *q, *k, *col;
    uint32_t *pred, *end, *score;
    uint4 *slab;
    unsigned long long *ctr;      // 0 .. 3: reads without a start place, of the small, wave and spill tier; 4: anchors
    uint64_t band;
};

// Row r supports the start place g of seed t iff g belongs to node u at o < |label(u)|, node_of[r][block(u)] == u, and
// the read substring S of t equals the row's gap-stripped text from o inside label(u) on.  That text is label(u)[o:]
// followed by the labels of the row's nodes in the blocks after block(u): cells without a node (the row is all gaps
// there) are passed over, and the text ends with block nb - 1.
struct PrDev {
    const uint32_t *node_of;      // [nb * m], block-major: 64 lanes read 64 consecutive rows of one block
    const uint8_t *labels;
    const uint64_t *loff;         // [n_nodes + 1]
    const uint8_t *reads;
    const uint64_t *sbase;        // [S] byte of reads at which the seed's substring starts
    const uint32_t *slen;         // [S]
    uint64_t m, nb;
};

// Chaining by row.  Read R has the start places g0 = start_off[seed_off[R]] .. start_off[seed_off[R + 1]] as in PcDev;
// col: their start columns (PC_NONE: no anchor), rec: what k_pr_place left per place.  lds / max: the place counts up to
// which a read goes to the LDS tier / is chained at all.
struct PbDev {
    const uint64_t *seed_off, *start_off;
    const uint32_t *q, *k, *col;
    const uint4 *rec;
    uint32_t *row, *score, *nbest;
    unsigned long long *ctr;      // PB_CTR counters
    uint64_t band, lds, max;
};

// The text of row r is the labels of its nodes in block order, so a position x of G_r lies in the last block j with
// p(r, j) <= x (a block without a node of the row has p(r, j) == p(r, j + 1) and is never that last one while x < |G_r|).
struct PaDev {
    const uint32_t *node_of, *pref;   // [nb * m] each, block-major
    const uint8_t *labels;
    const uint64_t *loff;
    const uint8_t *reads;
    const uint64_t *roff;             // [n + 1] byte offsets of the (virtual) reads
    uint64_t m, nb;
};

// The graph of the blocks jl .. jh is the nodes first[jl] .. first[jh + 1] (ids ascend block by block, so id order is a
// topological order) with the edges of pin: the predecessors of v are pin[pin_off[v] .. pin_off[v + 1]), ascending, all
// of the block before v's.  C[j]: the sum of the shortest labels of the blocks before j.
struct PhDev {
    const uint8_t *labels;
    const uint64_t *loff;             // [n_nodes + 1]
    const uint8_t *reads;
    const uint64_t *roff;             // [n + 1] byte offsets of the (virtual) reads
    const uint64_t *first, *C;        // [nb + 1] each
    const uint32_t *pin_off, *pin;
    uint64_t nb;
};

static inline PxDev px_dev(const fbg_pindex *ix)
{
    PxDev d;
    d.lines = ix->lines.as<uint8_t>();
    d.cnt_tab = ix->cnt_tab.as<uint32_t>();
    d.bpos = ix->bpos.as<uint32_t>();
    d.epos = ix->epos.as<uint32_t>();
    d.N = (uint32_t)(ix->N1 - 1);
    d.nb = ix->nb; d.ne = ix->ne;
    d.S = (uint32_t)ix->sigma;
    return d;
}

// The tables of the validation and of the occurrence expansion.  block is the scratch of fbg_pindex_validate (NULL
// before its first call): k_po_expand reads sa, estart, esrc, edst and ctab only.
static inline PvDev pv_dev(const fbg_pindex *ix)
{
    PvDev d;
    d.sa = ix->sa.as<uint32_t>();
    d.tpos = ix->vtpos.as<uint32_t>();
    d.len = ix->vlen.as<uint32_t>();
    d.estart = ix->vestart.as<uint32_t>();
    d.esrc = ix->vesrc.as<uint32_t>();
    d.edst = ix->vedst.as<uint32_t>();
    d.ctab = ix->vctab.as<uint32_t>();
    d.block = ix->vblock.as<uint32_t>();
    d.rng = ix->vrng.as<uint2>();
    d.flag = ix->vflag.as<uint8_t>();
    d.text = ix->text.as<uint8_t>();
    return d;
}

// The scratch of a build; fbg_segmentation_repair keeps one from round to round.
struct PxScratch {
    DevBuf labels, loff, elen, eoff, keysA, keysB, valsA, valsB, cidx, cidx2, rank, headv, hscan, head, keep,
           cntT, cntX, code_u8, count;
    DevBuf nrow, len64, ebase, firstE, nout, nin, hist;     // px_prepare_segmentation
    DevBuf munit, muoff, mctr;                              // ... its MSA coordinate table
    std::vector<DevBuf *> bufs;
    ~PxScratch() { fbg_release_all(nullptr, bufs); }
};

// What k_pg_sizes and k_pg_path read of the call whose alignments they trace, n reads: info[R] = (-, w0, -, L); out (4 n):
// out[n + R] the edits or PA_NONE, then the start and the end of T in the positions that w0 is counted in; T itself at
// win + woff[R] + (start - w0).
struct PgIn {
    const uint4 *info;
    const uint64_t *woff;
    const uint8_t *win;
    const uint32_t *out;
};

// ---- host functions that cross files ---------------------------------------------------------------------------------
PX_LOCAL int px_new(fbg_ctx *ctx, fbg_pindex **out);       // pindex_build.hip: a new index object with its events
PX_LOCAL int px_build_segmentation(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, bool with_map, bool with_rows = false);
PX_LOCAL void px_destroy(fbg_pindex *ix);
// locate.hip: k_px_walk<false> over the labels of a build; off[0 .. n] -= base; k_po_expand_msa over one list of s
PX_LOCAL void px_walk_labels(fbg_pindex *ix, const uint8_t *labels, const uint64_t *loff, uint64_t n_nodes, uint8_t *bflag, uint8_t *eflag);
PX_LOCAL void px_rebase(hipStream_t st, uint64_t *off, uint64_t n, uint64_t base);
PX_LOCAL void po_expand_msa(fbg_pindex *ix, const PoState &s, bool starts, uint32_t *orow, uint32_t *ocol);
// pindex_chain.hip: the checks that fbg_pindex_chains and fbg_pindex_chains_by_row share (what: the caller's name); the
// chain state's buffers for n reads, S seeds and A start places, and d filled for the columns col; then, on those columns,
// k_pc_key, the sort, the host's look at the bins (bin[0 .. 4)), k_pc_chain per tier, k_pc_trace, the scan, k_pc_trace;
// and what ends either call after px_sync_elapsed: the limit on chain_off[n], the statistics (bin[4]: the anchors)
PX_LOCAL int pc_begin(fbg_pindex *ix, uint64_t *chain_off, uint32_t *score, double *device_ms, const char *what, bool *go);
// pc_reserve, pc_launch and pc_finish work on the chain state c: ix->ch for the two chaining calls, the mapq state's own
// for fbg_pindex_chains_mapq (pindex_mapq.hip).  None of them touches the stage table: the caller finishes its stage
PX_LOCAL int pc_reserve(fbg_pindex *ix, PcState &c, PcDev &d, const uint32_t *col, uint64_t band);
PX_LOCAL int pc_launch(fbg_pindex *ix, PcState &c, PcDev &d, uint64_t min_score, uint64_t bin[5], const char *what);
// the tail of pc_launch on its own: k_pc_trace, the scan, k_pc_trace over end, score and pred of c (fbg_pindex_chains_pairs
// runs it on ix->ch after it has put the adopted chains' ends, scores and predecessors there)
PX_LOCAL int pc_trace(fbg_pindex *ix, PcState &c, PcDev &d, uint64_t min_score);
PX_LOCAL int pc_finish(fbg_pindex *ix, PcState &c, const uint64_t *chain_off, const uint64_t bin[5], const char *what);
// pindex_rows.hip: k_pr_seed and k_pr_place (records ev0); k_pr_chain
PX_LOCAL int pr_prepare(fbg_pindex *ix, PrDev &d);
PX_LOCAL void pr_chain_launch(fbg_pindex *ix, const PrDev &d, uint64_t n, uint64_t words, uint32_t *n_rows, uint32_t *first_row,
                              uint64_t *bits, unsigned long long *ctr);
// pindex_align.hip: k_pg_sizes, k_pg_path per tier and batch and k_pg_compact over the alignments of in (NULL: nothing of
// them is on the device, n reads without runs) into g, the state of `stage` (PS_CIGAR or PS_GCIGAR), for the call `who`;
// started: the caller recorded ev0 with kernels of its own.  Ends with px_sync_elapsed.  And the copy of g's offsets and
// runs to the host
PX_LOCAL int pg_trace(fbg_pindex *ix, const PgIn *in, PgState &g, PsStage stage, uint64_t n, bool started, uint32_t *n_ops,
                      uint64_t *total_ops, double *device_ms, const char *who);
PX_LOCAL int pg_fetch(fbg_pindex *ix, const PgState &g, uint64_t *off, uint32_t *ops);
// pindex_align.hip, for fbg_pindex_pairs_align (pindex_pairs_align.hip): the prefix table reserved and, where no call has
// built it yet, k_pa_prefix launched (the caller sets al.has_pref once its call has succeeded); what the alignment kernels
// read, valid after pa_prefix; k_pa_gather and k_pa_edit over n reads on the caller's own info / start / woff / win / out
PX_LOCAL int pa_prefix(fbg_pindex *ix);
PX_LOCAL PaDev pa_dev(const fbg_pindex *ix);
PX_LOCAL void pa_windows(fbg_pindex *ix, const PaDev &a, uint64_t n, const uint4 *info, const uint4 *start, const uint64_t *woff, uint8_t *win,
                         uint32_t *out);
