// locate.hip -- pattern index of a founder graph and batched pattern search (the query side of the reference's
// founder_block_index: make_index, fbg.cpp:2809-2953, and backward_search, founder_block_index.hpp:86-145).
//
// Text: for every node u in id order and every distinct out-neighbour v in ascending order, reverse(label(u) +
// label(v) + '#'), then one 0 sentinel (N + 1 symbols in all).  Built here, all on the device:
//
//   k_px_edge_len / k_px_edge_text   |u| + |v| + 1 per edge, an exclusive scan for the offsets, one wave per edge
//                                    writes its reversed string;
//   suffix array                     prefix doubling: k_px_keys0 packs the first K symbol codes of every suffix,
//                                    a radix sort orders them; every later round re-sorts only the suffixes of
//                                    groups that still tie, by (rank of the group, rank h symbols ahead), and
//                                    doubles h, until no group is left (exact SA, any byte alphabet);
//   k_px_lines                       BWT and the occ structure, one wave per 128 BWT positions;
//   k_px_walk<false>                 B / E: every label searched from [0, N], flags at lhs / rhs, compacted
//                                    into sorted position lists;
//   k_px_walk<true>                  the batched search of rule 4 (restarts included), one lane per pattern,
//                                    patterns handed out in order of length;
//   k_px_walk<true, *, true>         the same search for fbg_pindex_occurrences: it also keeps the final range, the
//                                    range after the '#' step of the first restart and the restart count;
//   k_px_seeds                       fbg_pindex_seeds: that search run to the end of every read, restarted from [0, N]
//                                    wherever it stops; a counting instantiation and a writing one (one record per
//                                    maximal piece, which k_po_sizes / k_po_expand then treat as a pattern);
//   k_po_sizes / k_po_expand         capped list sizes per pattern (scanned into CSR offsets), then one lane per
//                                    reported place: SA slot -> (edge source, edge destination, offset);
//   k_pv_node / k_pv_wave            the semi-repeat-free check (fbg_pindex_validate): the SA range of every label,
//                                    kept from the B / E walk, scanned against the block of each occurrence's node,
//                                    one lane per short range and one wave per long one;
//   k_ps_*                           the index of a segmentation's graph without the host (fbg_pindex_build_segmentation):
//                                    labels gathered from the resident MSA, edges, validation tables and the byte
//                                    histogram from the device stage of fbg_block_graph ("prepare from a segmentation");
//   k_pm_units / k_pm_fill           the MSA coordinate table of such an index: per node its representative row, first
//                                    column and, for a row with gaps in the block, a bitmap of its non-gap cells with a
//                                    running count every PM_W words;
//   k_po_expand_msa                  k_po_expand's walk from a reported place to its edge and offset, then through that
//                                    table to the MSA row and column of the place (fbg_pindex_occurrences_msa / _seeds_msa);
//   k_pc_key / k_pc_chain / k_pc_trace   fbg_pindex_chains: the reads binned by their number of start places, the
//                                    co-linear chaining DP over a read's start places in three tiers, and the walk back
//                                    from the chain's end (a pass that counts, a scan, a pass that writes);
//   k_pr_seed / k_pr_place / k_pr_rows / k_pr_chain   the MSA rows that carry a start place or a whole chain
//                                    (fbg_pindex_seeds_rows / _chains_rows): per seed the byte its substring starts at,
//                                    per start place its node, offset, seed and block, then lanes as rows: one read of
//                                    the row table, a walk along the row's labels, a ballot per 64 rows;
//   k_sv_cuts                        the cuts before blocks that hold an INVALID node (fbg_segmentation_validate / _repair).
//
// occ layout.  Symbols are remapped to dense codes in byte order (the sentinel is code 0, '#' code 1).  With at
// most 16 codes a block of 128 BWT positions is one 128-byte line:
//   bytes   0 ..  63   u32 occ of every code before the block
//   bytes  64 ..  95   bits 0 .. 63 of the positions, bit planes 0 .. 3 (u64 each)
//   bytes  96 .. 127   bits 64 .. 127, bit planes 0 .. 3
// occ(c, i) = count[c] + popcount(AND over the planes of (plane or its complement) below i): one line per query,
// about one byte per text position.  Larger alphabets take 8 bit planes per line (128 bytes) and the counts in a
// table of their own (u32 per block and code): two lines per query.
#include "fbg_internal.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <chrono>
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
#define PA_MAX_READ 1024      // alignment: the longest read fbg_pindex_chains_align takes (max_read), a multiple of 64
#define PA_REG_WORDS 4        // reads of up to this many 64-symbol words keep the bit-vector state in registers
#define PA_NONE 0xffffffffu   // FBG_ALIGN_NONE
#define PG_CTR 13              // counters of fbg_pindex_chains_cigar: traces that failed, reads traced, columns, reads of 1 .. 4
                              // words and of more, the widest T of each of the five

// What k_po_sizes leaves for k_po_expand, for n items (the patterns of fbg_pindex_occurrences, or the seeds of
// fbg_pindex_seeds): totals, capped sizes and their scans, the first slot of either list, k or the length, restarts;
// and the places of the last fetch.  Grow-only, on the index's buffer list.
struct PoState {
    DevBuf etot, stot, esz, ssz, eoff, soff, rs, el, ss, sk, place;
    DevBuf msa;               // the rows and columns of the last fbg_pindex_occurrences_msa / _seeds_msa, apart from place
    bool ready = false;
    uint64_t n = 0, etotal = 0, stotal = 0;
};

// fbg_pindex_chains: per start place of the last fbg_pindex_seeds its MSA row and column (col: rows first, a copy apart
// from sd.msa) and its predecessor; per read the binning keys and ids (before and after the sort), the chain's end
// place, score and length, the scan of the lengths; the chains (places, then seeds); the spill tier's slab (a uint4 per
// start place, reserved when a read needs it); the counters of k_pc_key and k_pc_chain.  fbg_pindex_chain_strands: per
// given read its strand and best score, and the three counters of k_pc_strand.
struct PcState {
    DevBuf col, pred, key, id, key2, id2, end, score, len, off, out, slab, ctr;
    DevBuf strand, best, sctr;
    bool ready = false;
    uint64_t n = 0, total = 0, anchors = 0, tier[3] = {0, 0, 0};
};

// The row table of fbg_pindex_build_segmentation_rows: node_of[nb * m], block-major, and the gathered labels with their
// offsets (a node without an edge has no copy of its label in the index text).  reads / roff: the reads of the last seeds
// call, moved aside when a locate or occurrences call is about to overwrite pats / poff (saved).  sbase: per seed the
// byte of the reads its substring starts at; rec: per start place (node, offset in the node, seed, block) or PR_NONE
// first; out / cout: what the last fbg_pindex_seeds_rows / _chains_rows copied out; ctr: its count of empty sets.
struct PrState {
    DevBuf node_of, labels, loff, reads, roff, sbase, rec, out, cout, ctr;
    bool saved = false;
    uint64_t m = 0, label_bytes = 0, read_bytes = 0, places_unsupported = 0, chains_unsupported = 0;
};

// fbg_pindex_chains_align.  pref: p(r, j) as uint32[nb * m], block-major like node_of, built by the first call.  Per read
// of the last seeds call: nrows / first (what k_pr_chain leaves: the row choice), info = (row, w0, |W| or 0 where nothing
// is aligned, L), start = (block, node, offset in the node) at which w0 falls, wlen and its scan woff (n + 1 each), out
// (row, edits, t_start, t_end: 4 n); win: the windows, back to back; ctr: non-empty chains without a row, reads aligned,
// too long, too wide, and the cells.  valid: a call has succeeded since the last fbg_pindex_chains, for n reads, and
// (on_device) left info, woff, win and out for them; not where it returned before its first kernel.
struct PaState {
    DevBuf pref, nrows, info, start, wlen, woff, win, out, ctr;
    bool has_pref = false, valid = false, on_device = false;
    uint64_t n = 0;
    uint64_t stat[5] = {0, 0, 0, 0, 0};
};

// fbg_pindex_chains_cigar.  Per read of the last align call: sz (history units of 8 bytes, then run slots; n + 1 each)
// and their scans hoff / soff, cnt (runs as u64, n + 1) and its scan off, nops (runs as u32); slots: 2 * edits + 1 runs
// per aligned read; ops: the runs back to back; hist: the column history of one batch of long reads; ctr: PG_CTR
// counters.  ready: a call has succeeded since that align call, for n reads and total runs (on_device as above).
struct PgState {
    DevBuf sz, hoff, soff, cnt, off, nops, slots, ops, hist, ctr;
    bool ready = false, on_device = false;
    uint64_t n = 0, total = 0;
    uint64_t stat[5] = {0, 0, 0, 0, 0};      // paths, ops, columns, history_bytes, batches
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
    DevBuf pats, poff, okey, oval, okey2, oval2, cnt_out, pos_out, lines_ctr, tmp;
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
    hipEvent_t sv0 = nullptr, sv1 = nullptr;
    // fbg_pindex_occurrences: the walk's record per pattern (3 x uint2) and the place state of its patterns;
    // fbg_pindex_seeds: per pattern the number of reported seeds and its scan, per seed what the walk wrote (the same
    // record, count, length as u64 for k_po_sizes, q_start, length) and the place state of the seeds.  The two place
    // states never share a buffer: a fetch of one is not disturbed by a search of the other.
    DevBuf orec;
    PoState occ;
    DevBuf snum, soff, srec, scnt, spos, sq, slen;
    PoState sd;
    uint64_t sd_reads = 0;        // reads of the last successful fbg_pindex_seeds (_strands: the 2n virtual reads)
    bool sd_stranded = false;     // the last seeds call was fbg_pindex_seeds_strands, with sd_reads / 2 given reads
    DevBuf comp;                  // its complement table (256 bytes)
    PcState ch;
    bool has_rows = false;        // built by fbg_pindex_build_segmentation_rows
    PrState rw;
    PaState al;
    PgState cg;
    uint64_t n_edges = 0, nctab = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<DevBuf *> bufs;   // the index's own device buffers: outside the context's workspaces and its accounting
    double build_ms = 0, search_ms = 0, validate_ms = 0;
    uint64_t occ_lines = 0, v_slots = 0, v_wave_nodes = 0;
};

template <class F> static int px_with_tmp(fbg_pindex *ix, F &&call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return fbg_fail(ix->ctx, FBG_ERR_HIP, "rocprim size query: %s", hipGetErrorString(e));
    FBG_TRY(fbg_reserve(ix->ctx, ix->tmp, bytes, &ix->bufs, false));
    size_t have = ix->tmp.cap;
    e = call(ix->tmp.p, have);
    if (e != hipSuccess)
        return fbg_fail(ix->ctx, e == hipErrorOutOfMemory ? FBG_ERR_OOM : FBG_ERR_HIP, "rocprim call: %s", hipGetErrorString(e));
    return FBG_OK;
}

// ---- edge text ------------------------------------------------------------------------------------------------
__global__ void k_px_edge_len(const uint32_t *esrc, const uint32_t *edst, const uint64_t *loff, uint64_t E, uint64_t *len)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t u = esrc[e], v = edst[e];
    len[e] = (loff[u + 1] - loff[u]) + (loff[v + 1] - loff[v]) + 1;
}

// one wave per edge: text[eoff[e] + k] = reverse(label(u) + label(v) + '#')[k] = '#', reverse(v), reverse(u)
__global__ __launch_bounds__(PX_THREADS) void k_px_edge_text(const uint8_t *labels, const uint64_t *loff, const uint32_t *esrc,
                                                            const uint32_t *edst, const uint64_t *eoff, uint64_t E, uint8_t *text)
{
    const uint64_t e = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE;
    const unsigned lane = threadIdx.x % FBG_WAVE;
    if (e >= E) return;
    const uint32_t u = esrc[e], v = edst[e];
    const uint64_t ou = loff[u], lu = loff[u + 1] - ou, ov = loff[v], lv = loff[v + 1] - ov;
    uint8_t *out = text + eoff[e];
    for (uint64_t k = lane; k < lu + lv + 1; k += FBG_WAVE)
        out[k] = k == 0 ? (uint8_t)'#' : k <= lv ? labels[ov + lv - k] : labels[ou + lu - (k - lv)];
}

// ---- suffix array by prefix doubling ----------------------------------------------------------------------------
// round 0: key = the first K symbol codes (b bits each, most significant first; 0 beyond the text, which only
// follows the unique sentinel and so never decides an order), value = position; cidx = identity
__global__ void k_px_keys0(const uint8_t *text, const uint8_t *code_u8, uint64_t N1, int b, int K, uint64_t *keys,
                           uint32_t *vals, uint32_t *cidx)
{
    __shared__ uint8_t cs[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) cs[c] = code_u8[c];
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N1) return;
    uint64_t key = 0;
    for (int j = 0; j < K; j++) {
        const uint64_t q = p + j;
        key = (key << b) | (q < N1 ? cs[text[q]] : 0u);
    }
    keys[p] = key;
    vals[p] = (uint32_t)p;
    cidx[p] = (uint32_t)p;
}

// later rounds: the suffixes of tying groups (SA slots cidx[0 .. cnt), ascending), key = rank << pb | rank h ahead.
// A suffix that still ties has no sentinel among its first h symbols, so p + h < N1.
__global__ void k_px_keysh(const uint32_t *cidx, uint64_t cnt, const uint32_t *sa, const uint32_t *rank, uint64_t h,
                           uint64_t N1, int pb, uint64_t *keys, uint32_t *vals)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t p = sa[cidx[k]];
    const uint64_t r2 = p + h < N1 ? rank[p + h] : 0u;
    keys[k] = ((uint64_t)rank[p] << pb) | r2;
    vals[k] = p;
}

// sorted slots back into the SA; a slot whose key differs from its predecessor's heads a new group
__global__ void k_px_place(const uint64_t *keys, const uint32_t *vals, const uint32_t *cidx, uint64_t cnt, uint32_t *sa,
                           uint32_t *headv, uint8_t *head)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t i = cidx[k];
    sa[i] = vals[k];
    const bool h = k == 0 || keys[k] != keys[k - 1];
    head[k] = h;
    headv[k] = h ? i : 0u;
}

// rank of a suffix = SA slot of its group's head (hscan: inclusive max-scan of headv); groups of one are settled
__global__ void k_px_rank(const uint32_t *vals, const uint32_t *hscan, const uint8_t *head, uint64_t cnt, uint32_t *rank,
                          uint8_t *keep)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    rank[vals[k]] = hscan[k];
    keep[k] = !(head[k] && (k + 1 == cnt || head[k + 1]));
}

// ---- BWT and occ lines ------------------------------------------------------------------------------------------
template <int P> __device__ __forceinline__ uint64_t px_match(uint32_t c, const uint64_t *w)
{
    uint64_t m = ~0ull;
#pragma unroll
    for (int p = 0; p < P; p++) m &= ((c >> p) & 1u) ? w[p] : ~w[p];
    return m;
}

// one wave per block of 128 BWT positions: bit planes into the line, per-code counts into cntT[code * nblk + blk]
template <bool COMPACT>
__global__ __launch_bounds__(PX_THREADS) void k_px_lines(const uint32_t *sa, const uint8_t *text, const uint8_t *code_u8, uint64_t N1,
                                                        uint64_t nblk, int S, uint8_t *lines, uint32_t *cntT)
{
    constexpr int P = COMPACT ? 4 : 8;
    __shared__ uint8_t cs[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) cs[c] = code_u8[c];
    __syncthreads();
    const uint64_t blk = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE;
    const unsigned lane = threadIdx.x % FBG_WAVE;
    if (blk >= nblk) return;
    uint64_t w[2][P], valid[2];
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const uint64_t i = blk * PX_BLK + half * 64 + lane;
        uint32_t c = 0;
        if (i < N1) {
            const uint32_t s = sa[i];
            c = cs[s ? text[s - 1] : 0];    // text[N] is the sentinel: the BWT of slot SA^-1[0] is code 0
        }
        valid[half] = __ballot(i < N1);
#pragma unroll
        for (int p = 0; p < P; p++) w[half][p] = __ballot((c >> p) & 1u);
    }
    uint8_t *ln = lines + blk * PX_LINE;
    if (lane < 2 * P) {
        const int half = lane / P, p = lane % P;
        uint64_t v = 0;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < P; q++)
                if (h == half && q == p) v = w[h][q];
        *(uint64_t *)(ln + (COMPACT ? 64 : 0) + half * (P * 8) + p * 8) = v;
    }
    for (int s = lane; s < S; s += FBG_WAVE)
        cntT[(uint64_t)s * nblk + blk] = __popcll(px_match<P>(s, w[0]) & valid[0]) + __popcll(px_match<P>(s, w[1]) & valid[1]);
}

// exclusive counts (cntX, code-major) into the lines (compact) or the block-major count table
template <bool COMPACT>
__global__ void k_px_counts(const uint32_t *cntX, uint64_t nblk, int S, uint8_t *lines, uint32_t *cnt_tab)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int SS = COMPACT ? 16 : S;
    if (t >= nblk * SS) return;
    const uint64_t blk = t / SS;
    const int s = (int)(t % SS);
    const uint32_t v = s < S ? cntX[(uint64_t)s * nblk + blk] : 0u;
    if (COMPACT) ((uint32_t *)(lines + blk * PX_LINE))[s] = v;
    else cnt_tab[blk * S + s] = v;
}

// ---- backward steps ---------------------------------------------------------------------------------------------
struct PxDev {
    const uint8_t *lines;
    const uint32_t *cnt_tab;
    const uint32_t *bpos, *epos;
    uint32_t N, nb, ne, S;
};

__device__ __forceinline__ uint64_t px_low(uint32_t off) { return off >= 64 ? ~0ull : ((1ull << off) - 1); }

// occ(c, i) of a loaded line: planes w[word][plane]
template <int P> __device__ __forceinline__ uint32_t px_pop(uint32_t c, uint32_t off, const uint64_t (&w)[2][P])
{
    const uint32_t a = __popcll(px_match<P>(c, w[0]) & px_low(off));
    return off > 64 ? a + __popcll(px_match<P>(c, w[1]) & px_low(off - 64)) : a;
}

template <bool COMPACT> __device__ __forceinline__ uint32_t px_load(const PxDev &d, uint32_t c, uint32_t blk,
                                                                    uint64_t (&w)[2][COMPACT ? 4 : 8])
{
    constexpr int P = COMPACT ? 4 : 8;
    const uint8_t *ln = d.lines + (uint64_t)blk * PX_LINE;
    const ulonglong2 *q = (const ulonglong2 *)(ln + (COMPACT ? 64 : 0));
#pragma unroll
    for (int k = 0; k < P; k++) {
        const ulonglong2 v = q[k];
        w[(2 * k) / P][(2 * k) % P] = v.x;
        w[(2 * k + 1) / P][(2 * k + 1) % P] = v.y;
    }
    return COMPACT ? ((const uint32_t *)ln)[c] : d.cnt_tab[(uint64_t)blk * d.S + c];
}

// occ(c, l) and occ(c, r1), l <= r1: both loads issued before either is used; one line when both fall in one block
template <bool COMPACT> __device__ __forceinline__ void px_occ2(const PxDev &d, uint32_t c, uint32_t l, uint32_t r1,
                                                                uint32_t &ol, uint32_t &or1, uint32_t &nlines)
{
    constexpr int P = COMPACT ? 4 : 8;
    const uint32_t bl = l / PX_BLK, br = r1 / PX_BLK;
    uint64_t wl[2][P], wr[2][P];
    const uint32_t cl = px_load<COMPACT>(d, c, bl, wl);
    uint32_t cr = cl;
    const bool two = bl != br;
    if (two) cr = px_load<COMPACT>(d, c, br, wr);
    ol = cl + px_pop<P>(c, l % PX_BLK, wl);
    or1 = two ? cr + px_pop<P>(c, r1 % PX_BLK, wr) : cl + px_pop<P>(c, r1 % PX_BLK, wl);
    nlines += two ? 2u : 1u;
}

// bs(c, l, r) of sdsl: [C[c] + occ(c, l), C[c] + occ(c, r + 1) - 1]; the count, 0 for an absent symbol
template <bool COMPACT> __device__ __forceinline__ uint32_t px_bs(const PxDev &d, const uint16_t *code, const uint32_t *C,
                                                                  uint32_t ch, uint32_t l, uint32_t r, uint32_t &nl,
                                                                  uint32_t &nr, uint32_t &nlines)
{
    const uint32_t c = code[ch];
    if (c == PX_ABSENT) { nl = l; nr = r; return 0; }
    uint32_t ol, or1;
    px_occ2<COMPACT>(d, c, l, r + 1, ol, or1, nlines);
    nl = C[c] + ol;
    nr = C[c] + or1 - 1;
    return or1 - ol;
}

// One lane per pattern.  SEARCH: rule 4 of the index (a failed step may restart at a block pair boundary), results
// count / pos by pattern id, patterns taken in the order `order` (by length).  !SEARCH: B / E of the node labels, no
// restart; a label whose search finds nothing sets no flag (the reference asserts there); every label's range goes to
// rng[id] = (l, r), (1, 0) when nothing was found, for fbg_pindex_validate.  OCC (with SEARCH): the search also records
// rng[3 id] = the final (l, r), rng[3 id + 1] = (sl, sr), the range after the '#' step of the first restart that went
// on, rng[3 id + 2] = (symbols matched at that restart, restarts that went on), for fbg_pindex_occurrences.
template <bool SEARCH, bool COMPACT, bool OCC = false>
__global__ __launch_bounds__(PX_THREADS) void k_px_walk(PxDev d, const uint16_t *code_g, const uint32_t *C_g, const uint8_t *pats,
                                                       const uint64_t *poff, const uint32_t *order, uint64_t n,
                                                       unsigned long long *count_out, unsigned long long *pos_out,
                                                       uint8_t *bflag, uint8_t *eflag, unsigned long long *lines_ctr,
                                                       uint2 *rng)
{
    __shared__ uint16_t code[256];
    __shared__ uint32_t C[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) { code[c] = code_g[c]; C[c] = C_g[c]; }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nlines = 0;
    if (t < n) {
        const uint64_t id = order ? order[t] : t;
        const uint64_t a = poff[id], len = poff[id + 1] - a;
        uint32_t l = 0, r = d.N, cnt = 0;
        uint64_t pos = 0, word = 0;
        bool ok = true;
        uint32_t restarts = 0, fsl = 1, fsr = 0, fk = 0;
        for (uint64_t k = 0; k < len; k++) {
            const uint64_t q = a + k;
            if (k == 0 || (q & 7) == 0) word = *(const uint64_t *)(pats + (q & ~7ull));   // buffer padded to 8 bytes
            const uint32_t ch = (uint32_t)(word >> (8 * (q & 7))) & 0xffu;
            uint32_t nl, nr;
            cnt = px_bs<COMPACT>(d, code, C, ch, l, r, nl, nr, nlines);
            if (cnt) {
                l = nl; r = nr;
            } else {
                if (!SEARCH) { ok = false; break; }
                // restart: the range must be able to step over '#', and B / E must enclose it
                uint32_t sl, sr;
                if (!px_bs<COMPACT>(d, code, C, '#', l, r, sl, sr, nlines)) { ok = false; break; }
                uint32_t lo = 0, hi = d.nb;       // r1 = #B positions <= l
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (d.bpos[mid] <= l) lo = mid + 1; else hi = mid;
                }
                const uint32_t r1 = lo;
                if (r1 == 0 || r1 > d.ne) { ok = false; break; }
                const uint32_t bl = d.bpos[r1 - 1], br = d.epos[r1 - 1];
                if (!(bl <= l && r <= br)) { ok = false; break; }
                cnt = px_bs<COMPACT>(d, code, C, ch, bl, br, nl, nr, nlines);
                if (!cnt) { ok = false; break; }
                if (OCC) {
                    if (!restarts) { fsl = sl; fsr = sr; fk = (uint32_t)pos; }
                    restarts++;
                }
                l = nl; r = nr;
            }
            pos++;
        }
        if (SEARCH) {
            count_out[id] = ok ? cnt : 0u;
            pos_out[id] = pos;
            if (OCC) {
                rng[3 * id] = make_uint2(l, r);
                rng[3 * id + 1] = make_uint2(fsl, fsr);
                rng[3 * id + 2] = make_uint2(fk, restarts);
            }
        } else {
            if (ok) {
                bflag[l] = 1;
                eflag[r] = 1;
            }
            rng[id] = ok ? make_uint2(l, r) : make_uint2(1u, 0u);
        }
    }
    if (SEARCH) {
        unsigned long long s = nlines;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x % FBG_WAVE) == 0 && s) atomicAdd(lines_ctr, s);
    }
}

// fbg_pindex_seeds: the search of k_px_walk<true, *, true>, run to the end of every read.  One lane per read, reads
// taken in the order `order` (by length).  When a step finally fails, or the read ends, after pos > 0 symbols, those
// symbols are a seed: the state is the one the search of exactly those symbols ends in, so (l, r), the record of the
// first restart and the restart count are what fbg_pindex_occurrences keeps for that substring.  The search then starts
// again from [0, N] at the failing symbol, or at the next one when it failed at once (pos == 0).  k moves by at most one
// symbol per step, so the pattern word held is always the one of symbol k, wherever in a word a seed starts.
// !WRITE: num[id] = seeds of at least min_len symbols.  WRITE: seed j of read id goes to entry num[id] + j (num: the
// exclusive scan of the counts) of cnt / len64 (u64, as k_po_sizes reads count and pos), rec (3 x uint2), qs and ln.
template <bool COMPACT, bool WRITE>
__global__ __launch_bounds__(PX_THREADS) void k_px_seeds(PxDev d, const uint16_t *code_g, const uint32_t *C_g, const uint8_t *pats,
                                                        const uint64_t *poff, const uint32_t *order, uint64_t n, uint32_t min_len,
                                                        uint64_t *num, unsigned long long *cnt_out, unsigned long long *len64,
                                                        uint2 *rec, uint32_t *qs, uint32_t *ln)
{
    __shared__ uint16_t code[256];
    __shared__ uint32_t C[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) { code[c] = code_g[c]; C[c] = C_g[c]; }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t id = order[t];
    const uint64_t a = poff[id];
    const uint32_t len = (uint32_t)(poff[id + 1] - a);       // < 2^32: checked by the host
    uint64_t at = WRITE ? num[id] : 0;                        // next entry (WRITE) or seeds counted so far
    uint32_t l = 0, r = d.N, pos = 0, nlines = 0;
    uint32_t restarts = 0, fsl = 1, fsr = 0, fk = 0;
    uint64_t word = 0;
    uint32_t k = 0;
    while (true) {
        bool ok = false;
        if (k < len) {
            const uint64_t q = a + k;
            if (k == 0 || (q & 7) == 0) word = *(const uint64_t *)(pats + (q & ~7ull));   // buffer padded to 8 bytes
            const uint32_t ch = (uint32_t)(word >> (8 * (q & 7))) & 0xffu;
            uint32_t nl, nr;
            ok = px_bs<COMPACT>(d, code, C, ch, l, r, nl, nr, nlines) != 0;
            if (!ok) {
                // restart: the branch of k_px_walk
                uint32_t sl, sr;
                if (px_bs<COMPACT>(d, code, C, '#', l, r, sl, sr, nlines)) {
                    uint32_t lo = 0, hi = d.nb;       // r1 = #B positions <= l
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) / 2;
                        if (d.bpos[mid] <= l) lo = mid + 1; else hi = mid;
                    }
                    const uint32_t r1 = lo;
                    if (r1 != 0 && r1 <= d.ne) {
                        const uint32_t bl = d.bpos[r1 - 1], br = d.epos[r1 - 1];
                        if (bl <= l && r <= br && px_bs<COMPACT>(d, code, C, ch, bl, br, nl, nr, nlines)) {
                            if (!restarts) { fsl = sl; fsr = sr; fk = pos; }
                            restarts++;
                            ok = true;
                        }
                    }
                }
            }
            if (ok) { l = nl; r = nr; pos++; k++; continue; }
        }
        // the search stopped at symbol k (k == len: the read ended)
        if (pos) {
            if (pos >= min_len) {
                if (WRITE) {
                    cnt_out[at] = (unsigned long long)r - l + 1;
                    len64[at] = pos;
                    rec[3 * at] = make_uint2(l, r);
                    rec[3 * at + 1] = make_uint2(fsl, fsr);
                    rec[3 * at + 2] = make_uint2(fk, restarts);
                    qs[at] = k - pos;
                    ln[at] = pos;
                }
                at++;
            }
            l = 0; r = d.N; pos = 0; restarts = 0; fsl = 1; fsr = 0; fk = 0;
        } else {
            if (k < len) k++;                                 // symbol k starts no match: skipped
        }
        if (k >= len) break;
    }
    if (!WRITE) num[id] = at;
}

__global__ void k_px_lenkey(const uint64_t *poff, uint64_t n, uint32_t *key, uint32_t *id)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t len = poff[t + 1] - poff[t];
    key[t] = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;
    id[t] = (uint32_t)t;
}

__global__ void k_px_rebase(uint64_t *off, uint64_t n, uint64_t base)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n) off[t] -= base;
}

// fbg_pindex_seeds_strands: the reverse virtual reads.  pats[0 .. total) and poff[0 .. n] (rebased: poff[0] = 0,
// poff[n] = total) are the given reads; the kernel writes pats[total + j] = comp[pats[poff[R] + poff[R + 1] - 1 - j]]
// for every j in [poff[R], poff[R + 1]) and poff[n + R] = total + poff[R] for R = 1 .. n (R = 0 is poff[n] itself and
// already holds total).  One lane per aligned 8-byte word of the destination: it finds the read of its first byte by
// a search of poff, walks on through poff where reads end inside the word (empty reads are stepped over) and stores
// the word whole; the two words that the range [total, 2 * total) covers only in part are stored byte by byte, so the
// forward bytes that share the first one are left alone.  The table sits in LDS.  The first n lanes of the grid also
// write the offsets.  n > 0.
__global__ __launch_bounds__(PX_THREADS) void k_px_revcomp(const uint8_t *comp_g, uint8_t *pats, uint64_t *poff, uint64_t n,
                                                          uint64_t total)
{
    __shared__ uint8_t comp[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) comp[c] = comp_g[c];
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = (total / 8 + t) * 8;                  // the word's first byte in pats
    const uint64_t lo = b0 > total ? b0 : total, hi = b0 + 8 < 2 * total ? b0 + 8 : 2 * total;
    if (lo < hi) {
        uint64_t j = lo - total;
        uint64_t R = 0, top = n;                              // poff[R] <= j < poff[top]
        while (top - R > 1) {
            const uint64_t mid = R + (top - R) / 2;
            if (poff[mid] <= j) R = mid; else top = mid;
        }
        uint64_t a = poff[R], e = poff[R + 1];
        uint64_t word = 0;
        for (uint64_t b = lo; b < hi; b++, j++) {
            while (j >= e) { R++; a = e; e = poff[R + 1]; }   // j < total = poff[n]: R stays below n
            word |= (uint64_t)comp[pats[a + (e - 1 - j)]] << (8 * (b - b0));
        }
        if (hi - lo == 8) {
            *(uint64_t *)(pats + b0) = word;
        } else {
            for (uint64_t b = lo; b < hi; b++) pats[b] = (uint8_t)(word >> (8 * (b - b0)));
        }
    }
    if (t < n) poff[n + 1 + t] = total + poff[1 + t];
}

// ctab[j] = the last edge e < E with estart[e] <= j << PV_CSHIFT (estart[0] = 0)
__global__ void k_pv_ctab(const uint32_t *estart, uint32_t E, uint64_t nctab, uint32_t *ctab)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nctab) return;
    const uint64_t x = j << PV_CSHIFT;
    uint32_t lo = 0, hi = E - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (estart[mid] <= x) lo = mid; else hi = mid - 1;
    }
    ctab[j] = lo;
}

static PxDev px_dev(const fbg_pindex *ix)
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

// ---- build ----------------------------------------------------------------------------------------------------
struct PxScratch {
    DevBuf labels, loff, elen, eoff, keysA, keysB, valsA, valsB, cidx, cidx2, rank, headv, hscan, head, keep,
           cntT, cntX, code_u8, count;
    DevBuf nrow, len64, ebase, firstE, nout, nin, hist;     // px_prepare_segmentation
    DevBuf munit, muoff, mctr;                              // ... its MSA coordinate table
    std::vector<DevBuf *> bufs;
    ~PxScratch() { fbg_release_all(nullptr, bufs); }
};

// What a prepare step hands to px_build_prepared, besides the device arrays it filled: labels (padded) and loff in the
// scratch; vesrc, vedst, vestart, vtpos, vlen, vflag in the index.
struct PxPrep {
    uint64_t n_nodes = 0, E = 0, N1 = 1;
    uint64_t hist[256] = {0};      // bytes of the text: the sentinel, E times '#', every label byte once per edge of its node
    bool eoff_ready = false;       // scratch.eoff already holds the text offset of every edge
};

struct PxMul {
    uint64_t m;
    __host__ __device__ uint64_t operator()(uint64_t s) const { return s * m; }
};

// Prepare from host arrays (fbg_pindex_build): checks, distinct sorted edges, the validation tables and the byte
// histogram in serial host loops, then the upload.
static int px_prepare_host(fbg_pindex *ix, PxScratch &s, const uint8_t *labels, const uint64_t *label_off, uint64_t n_nodes,
                           const uint64_t *edge_off, const uint64_t *edge_dst, PxPrep &pp)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t L = n_nodes ? label_off[n_nodes] - label_off[0] : 0;
    const uint64_t lbase = n_nodes ? label_off[0] : 0;
    // labels: no '#', no zero byte (both are separators of the text)
    for (uint64_t u = 0; u < n_nodes; u++)
        if (label_off[u + 1] < label_off[u]) return fbg_fail(ctx, FBG_ERR_INVALID, "label offsets decrease at node %llu", (unsigned long long)u);
    for (uint64_t k = 0; k < L; k++) {
        const uint8_t c = labels[lbase + k];
        if (c == '#' || c == 0)
            return fbg_fail(ctx, FBG_ERR_INVALID, "node labels may not contain '#' or a zero byte (byte %llu of the labels)", (unsigned long long)k);
    }
    if (n_nodes >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%llu nodes: at most 2^32 - 2", (unsigned long long)n_nodes);
    // distinct out-edges in ascending order (std::set), the text length and its byte histogram
    std::vector<uint32_t> esrc, edst, tmpv, estart, vtpos(n_nodes, 0), vlen(n_nodes);
    std::vector<uint8_t> vflag(n_nodes, 0);
    std::vector<uint64_t> use(n_nodes, 0);
    uint64_t N1 = 1;
    for (uint64_t u = 0; u < n_nodes; u++) {
        if (edge_off[u + 1] < edge_off[u]) return fbg_fail(ctx, FBG_ERR_INVALID, "edge offsets decrease at node %llu", (unsigned long long)u);
        tmpv.clear();
        for (uint64_t e = edge_off[u]; e < edge_off[u + 1]; e++) {
            if (edge_dst[e] >= n_nodes)
                return fbg_fail(ctx, FBG_ERR_INVALID, "edge %llu -> %llu: no such node", (unsigned long long)u, (unsigned long long)edge_dst[e]);
            tmpv.push_back((uint32_t)edge_dst[e]);
        }
        std::sort(tmpv.begin(), tmpv.end());
        tmpv.erase(std::unique(tmpv.begin(), tmpv.end()), tmpv.end());
        for (uint32_t v : tmpv) {
            esrc.push_back((uint32_t)u);
            edst.push_back(v);
            use[u]++; use[v]++;
            // for validation: the edge's text start ('#'), then reverse(label(v)), then reverse(label(u)); the first
            // edge of a node gives its label's text position
            const uint64_t start = N1 - 1, lv = label_off[v + 1] - label_off[v];
            estart.push_back((uint32_t)start);
            if (!vflag[u]) vtpos[u] = (uint32_t)(start + 1 + lv);
            vflag[u] |= PV_OUT;
            if (!vflag[v]) vtpos[v] = (uint32_t)(start + 1);
            vflag[v] |= PV_IN;
            N1 += (label_off[u + 1] - label_off[u]) + (label_off[v + 1] - label_off[v]) + 1;
            if (N1 >= (1ull << 32))
                return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "the edge text of this graph has 2^32 symbols or more; the pattern index "
                                "takes texts of N + 1 < 2^32 symbols");
        }
    }
    const uint64_t E = esrc.size();
    estart.push_back((uint32_t)(N1 - 1));
    for (uint64_t u = 0; u < n_nodes; u++) {
        const uint64_t len = label_off[u + 1] - label_off[u];
        vlen[u] = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;   // only nodes with edges are read (< N1)
    }
    uint64_t *hist = pp.hist;
    hist[0] = 1;
    hist['#'] = E;
    for (uint64_t u = 0; u < n_nodes; u++)
        if (use[u])
            for (uint64_t k = label_off[u]; k < label_off[u + 1]; k++) hist[labels[k]] += use[u];
    pp.n_nodes = n_nodes; pp.E = E; pp.N1 = N1;
    auto U = [&](std::vector<DevBuf *> &owner, DevBuf &b, const void *h, size_t bytes) -> int {
        FBG_TRY(fbg_reserve(ctx, b, bytes + 8, &owner, false));
        if (bytes) FBG_HIP_TRY(ctx, hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, st));
        return FBG_OK;
    };
    // labels (padded to whole 8-byte words for the walk's reads) and offsets rebased to 0
    FBG_TRY(fbg_reserve(ix->ctx, s.labels, ((L + 7) & ~7ull) + 16, &s.bufs, false));
    FBG_HIP_TRY(ctx, hipMemsetAsync(s.labels.p, 0, s.labels.cap, st));
    if (L) FBG_HIP_TRY(ctx, hipMemcpyAsync(s.labels.p, labels + lbase, L, hipMemcpyHostToDevice, st));
    FBG_TRY(U(s.bufs, s.loff, label_off, (n_nodes + 1) * 8));
    if (lbase) hipLaunchKernelGGL(k_px_rebase, dim3(fbg_blocks(n_nodes + 1, 256)), dim3(256), 0, st, s.loff.as<uint64_t>(), n_nodes, lbase);
    FBG_TRY(U(ix->bufs, ix->vesrc, esrc.data(), E * 4));
    FBG_TRY(U(ix->bufs, ix->vedst, edst.data(), E * 4));
    FBG_TRY(U(ix->bufs, ix->vestart, estart.data(), (E + 1) * 4));
    FBG_TRY(U(ix->bufs, ix->vtpos, vtpos.data(), n_nodes * 4));
    FBG_TRY(U(ix->bufs, ix->vlen, vlen.data(), n_nodes * 4));
    FBG_TRY(U(ix->bufs, ix->vflag, vflag.data(), n_nodes));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));        // the vectors above end with this function
    return FBG_OK;
}

// Build from prepared device arrays, shared by both entry points: symbol tables from the histogram, the text, the
// suffix array, the occ lines, B / E and the label ranges.
static int px_build_prepared(fbg_pindex *ix, PxScratch &s, const PxPrep &pp)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n_nodes = pp.n_nodes, E = pp.E, N1 = pp.N1;
    const uint64_t *hist = pp.hist;
    uint16_t code[256];
    uint8_t code_u8[256];
    uint32_t C[256];
    int sigma = 0;
    uint64_t acc = 0;
    for (int c = 0; c < 256; c++) {
        code[c] = hist[c] ? (uint16_t)sigma : (uint16_t)PX_ABSENT;
        code_u8[c] = hist[c] ? (uint8_t)sigma : 0;
        if (hist[c]) { C[sigma] = (uint32_t)acc; acc += hist[c]; sigma++; }
    }
    for (int s = sigma; s < 256; s++) C[s] = (uint32_t)acc;
    ix->N1 = N1;
    ix->sigma = sigma;
    ix->compact = sigma <= 16;
    ix->n_nodes = n_nodes;
    ix->nblk = N1 / PX_BLK + 1;
    ix->occ.ready = ix->sd.ready = false;

    auto U = [&](std::vector<DevBuf *> &owner, DevBuf &b, const void *h, size_t bytes) -> int {
        FBG_TRY(fbg_reserve(ctx, b, bytes + 8, &owner, false));
        if (bytes) FBG_HIP_TRY(ctx, hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, st));
        return FBG_OK;
    };
    FBG_TRY(fbg_reserve(ix->ctx, ix->vrng, n_nodes * 8, &ix->bufs, false));
    ix->n_edges = E;
    ix->nctab = ((N1 - 1) >> PV_CSHIFT) + 2;
    FBG_TRY(fbg_reserve(ix->ctx, ix->vctab, ix->nctab * 4, &ix->bufs, false));
    if (E) hipLaunchKernelGGL(k_pv_ctab, dim3(fbg_blocks(ix->nctab, 256)), dim3(256), 0, st, ix->vestart.as<uint32_t>(), (uint32_t)E,
                              ix->nctab, ix->vctab.as<uint32_t>());
    FBG_TRY(U(s.bufs, s.code_u8, code_u8, 256));
    FBG_TRY(U(ix->bufs, ix->code, code, sizeof(code)));
    FBG_TRY(U(ix->bufs, ix->C, C, sizeof(C)));

    // text
    FBG_TRY(fbg_reserve(ix->ctx, ix->text, N1 + 64, &ix->bufs, false));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->text.p, 0, ix->text.cap, st));
    if (E) {
        uint64_t *eoff = s.eoff.as<uint64_t>();
        if (!pp.eoff_ready) {
            FBG_TRY(fbg_reserve(ix->ctx, s.elen, E * 8, &s.bufs, false));
            FBG_TRY(fbg_reserve(ix->ctx, s.eoff, E * 8, &s.bufs, false));
            hipLaunchKernelGGL(k_px_edge_len, dim3(fbg_blocks(E, 256)), dim3(256), 0, st, ix->vesrc.as<uint32_t>(), ix->vedst.as<uint32_t>(),
                               s.loff.as<uint64_t>(), E, s.elen.as<uint64_t>());
            uint64_t *elen = s.elen.as<uint64_t>();
            eoff = s.eoff.as<uint64_t>();
            FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
                return rocprim::exclusive_scan(tmp, bytes, elen, eoff, (uint64_t)0, (size_t)E, rocprim::plus<uint64_t>(), st);
            }));
        }
        hipLaunchKernelGGL(k_px_edge_text, dim3(fbg_blocks(E * FBG_WAVE, PX_THREADS)), dim3(PX_THREADS), 0, st, s.labels.as<uint8_t>(),
                           s.loff.as<uint64_t>(), ix->vesrc.as<uint32_t>(), ix->vedst.as<uint32_t>(), eoff, E, ix->text.as<uint8_t>());
    }

    // suffix array
    int b = 1;
    while ((1 << b) < sigma) b++;
    const int K = 64 / b;
    int pb = 1;
    while ((1ull << pb) < N1) pb++;
    FBG_TRY(fbg_reserve(ix->ctx, ix->sa, N1 * 4, &ix->bufs, false));
    for (DevBuf *d : {&s.keysA, &s.keysB}) FBG_TRY(fbg_reserve(ix->ctx, *d, N1 * 8, &s.bufs, false));
    for (DevBuf *d : {&s.valsA, &s.valsB, &s.cidx, &s.cidx2, &s.rank, &s.headv, &s.hscan}) FBG_TRY(fbg_reserve(ix->ctx, *d, N1 * 4, &s.bufs, false));
    for (DevBuf *d : {&s.head, &s.keep}) FBG_TRY(fbg_reserve(ix->ctx, *d, N1, &s.bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, s.count, 8, &s.bufs, false));
    uint64_t *kA = s.keysA.as<uint64_t>(), *kB = s.keysB.as<uint64_t>();
    uint32_t *vA = s.valsA.as<uint32_t>(), *vB = s.valsB.as<uint32_t>();
    uint32_t *sa = ix->sa.as<uint32_t>(), *rank = s.rank.as<uint32_t>(), *headv = s.headv.as<uint32_t>(), *hscan = s.hscan.as<uint32_t>();
    uint8_t *head = s.head.as<uint8_t>(), *keep = s.keep.as<uint8_t>();
    uint32_t *cidx = s.cidx.as<uint32_t>(), *cidx2 = s.cidx2.as<uint32_t>();
    hipLaunchKernelGGL(k_px_keys0, dim3(fbg_blocks(N1, 256)), dim3(256), 0, st, ix->text.as<uint8_t>(), s.code_u8.as<uint8_t>(), N1, b, K,
                       kA, vA, cidx);
    uint64_t cnt = N1, h = (uint64_t)K;
    unsigned end_bit = (unsigned)(K * b);
    for (int round = 0; cnt > 0; round++) {
        if (round > 0) {
            hipLaunchKernelGGL(k_px_keysh, dim3(fbg_blocks(cnt, 256)), dim3(256), 0, st, cidx, cnt, sa, rank, h, N1, pb, kA, vA);
            end_bit = (unsigned)(2 * pb);
            h *= 2;
        }
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, kA, kB, vA, vB, (size_t)cnt, 0u, end_bit, st);
        }));
        hipLaunchKernelGGL(k_px_place, dim3(fbg_blocks(cnt, 256)), dim3(256), 0, st, kB, vB, cidx, cnt, sa, headv, head);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, headv, hscan, (size_t)cnt, rocprim::maximum<uint32_t>(), st);
        }));
        hipLaunchKernelGGL(k_px_rank, dim3(fbg_blocks(cnt, 256)), dim3(256), 0, st, vB, hscan, head, cnt, rank, keep);
        uint64_t *d_count = s.count.as<uint64_t>();
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::select(tmp, bytes, cidx, keep, cidx2, d_count, (size_t)cnt, st);
        }));
        uint64_t next = 0;
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&next, d_count, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
        cnt = next;
        std::swap(cidx, cidx2);
        if (round > 40) return fbg_fail(ctx, FBG_ERR_HIP, "pattern index: the suffix sort did not converge");
    }

    // BWT and occ lines
    const int S = sigma;
    const uint64_t nblk = ix->nblk;
    FBG_TRY(fbg_reserve(ix->ctx, ix->lines, nblk * PX_LINE, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, s.cntT, nblk * S * 4, &s.bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, s.cntX, nblk * S * 4, &s.bufs, false));
    if (!ix->compact) FBG_TRY(fbg_reserve(ix->ctx, ix->cnt_tab, nblk * S * 4, &ix->bufs, false));
    const dim3 gl(fbg_blocks(nblk * FBG_WAVE, PX_THREADS));
    if (ix->compact)
        hipLaunchKernelGGL(k_px_lines<true>, gl, dim3(PX_THREADS), 0, st, sa, ix->text.as<uint8_t>(), s.code_u8.as<uint8_t>(), N1, nblk, S,
                           ix->lines.as<uint8_t>(), s.cntT.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_px_lines<false>, gl, dim3(PX_THREADS), 0, st, sa, ix->text.as<uint8_t>(), s.code_u8.as<uint8_t>(), N1, nblk, S,
                           ix->lines.as<uint8_t>(), s.cntT.as<uint32_t>());
    {
        uint32_t *in = s.cntT.as<uint32_t>(), *out = s.cntX.as<uint32_t>();
        auto begins = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), PxMul{nblk});
        auto ends = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(1), PxMul{nblk});
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::segmented_exclusive_scan(tmp, bytes, in, out, (unsigned)S, begins, ends, (uint32_t)0,
                                                     rocprim::plus<uint32_t>(), st);
        }));
    }
    if (ix->compact)
        hipLaunchKernelGGL(k_px_counts<true>, dim3(fbg_blocks(nblk * 16, 256)), dim3(256), 0, st, s.cntX.as<uint32_t>(), nblk, S,
                           ix->lines.as<uint8_t>(), (uint32_t *)nullptr);
    else
        hipLaunchKernelGGL(k_px_counts<false>, dim3(fbg_blocks(nblk * S, 256)), dim3(256), 0, st, s.cntX.as<uint32_t>(), nblk, S,
                           ix->lines.as<uint8_t>(), ix->cnt_tab.as<uint32_t>());

    // B / E: flags by position, compacted in position order (sorted, each position once)
    uint8_t *bflag = s.head.as<uint8_t>(), *eflag = s.keep.as<uint8_t>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(bflag, 0, N1, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(eflag, 0, N1, st));
    ix->nb = ix->ne = 0;
    PxDev d = px_dev(ix);
    if (n_nodes) {
        const dim3 gw(fbg_blocks(n_nodes, PX_THREADS));
        if (ix->compact)
            hipLaunchKernelGGL((k_px_walk<false, true>), gw, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                               s.labels.as<uint8_t>(), s.loff.as<uint64_t>(), (const uint32_t *)nullptr, n_nodes,
                               (unsigned long long *)nullptr, (unsigned long long *)nullptr, bflag, eflag, (unsigned long long *)nullptr,
                               ix->vrng.as<uint2>());
        else
            hipLaunchKernelGGL((k_px_walk<false, false>), gw, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                               s.labels.as<uint8_t>(), s.loff.as<uint64_t>(), (const uint32_t *)nullptr, n_nodes,
                               (unsigned long long *)nullptr, (unsigned long long *)nullptr, bflag, eflag, (unsigned long long *)nullptr,
                               ix->vrng.as<uint2>());
    }
    FBG_TRY(fbg_reserve(ix->ctx, ix->bpos, N1 * 4 < n_nodes * 4 ? N1 * 4 : n_nodes * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->epos, N1 * 4 < n_nodes * 4 ? N1 * 4 : n_nodes * 4, &ix->bufs, false));
    uint64_t nbe[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        uint8_t *fl = k ? eflag : bflag;
        uint32_t *out = (k ? ix->epos : ix->bpos).as<uint32_t>();
        uint64_t *d_count = s.count.as<uint64_t>();
        auto it = rocprim::make_counting_iterator<uint32_t>(0);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::select(tmp, bytes, it, fl, out, d_count, (size_t)N1, st);
        }));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&nbe[k], d_count, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    ix->nb = (uint32_t)nbe[0];
    ix->ne = (uint32_t)nbe[1];
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    FBG_HIP_TRY(ctx, hipGetLastError());
    fbg_release(nullptr, ix->tmp);
    return FBG_OK;
}

static int px_build(fbg_pindex *ix, const uint8_t *labels, const uint64_t *label_off, uint64_t n_nodes,
                    const uint64_t *edge_off, const uint64_t *edge_dst)
{
    PxScratch s;
    PxPrep pp;
    FBG_TRY(px_prepare_host(ix, s, labels, label_off, n_nodes, edge_off, edge_dst, pp));
    return px_build_prepared(ix, s, pp);
}

// ---- prepare from a segmentation (fbg_pindex_build_segmentation) ------------------------------------------------
// The graph of a segmentation as the device stage of fbg_block_graph leaves it, turned into what px_build_prepared
// reads without a trip through the host:
//   k_ps_nodes        block and representative row of every node (blocks in order, representatives by row: the
//                     reference's numbering);
//   k_ps_labels<0>    one wave per node along its row's bytes: the gap-stripped length, and a flag for '#' / 0;
//   k_ps_labels<1>    the same walk again after the scan of the lengths: the label bytes into the padded buffer;
//   k_ps_edges        the per-block edge lists (distinct, ascending, blocks ascending) compacted with the scan of
//                     edge_count: the (source, destination) order of px_prepare_host;
//   k_ps_touch        per node the first edge that touches it (a min over the edge index: px_prepare_host's rule for
//                     vtpos) and its out- / in-degree over distinct edges;
//   k_ps_estart, k_ps_node_tables   estart from the scanned edge string lengths; vtpos and vflag per node;
//   k_ps_hist         bytes of the labels times the degree of their node, per workgroup in LDS, then global.
#define PS_NONE 0xffffffffu

// the columns [x0, x1) of block j: bg_block_range's clamp (block_graph.hip)
__device__ __forceinline__ void ps_block_range(const uint64_t *bounds, uint64_t n, uint64_t j, uint64_t &x0, uint64_t &x1)
{
    x0 = j ? bounds[j - 1] + 1 : 0;
    x1 = min(bounds[j] + 1, n);
    if (x0 > x1) x0 = x1;
}

__global__ void k_ps_nodes(const uint32_t *rep_row, const uint32_t *count, const unsigned long long *first, uint64_t m, uint64_t nb,
                           uint32_t *node_block, uint32_t *node_row)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * nb) return;
    const uint64_t j = t / m, k = t % m;
    if (k >= count[j]) return;
    const uint64_t u = first[j] + k;
    node_block[u] = (uint32_t)j;
    node_row[u] = rep_row[t];
}

// One wave per node (grid-stride), 64 columns of its row per step; the rank of a kept byte among the kept bytes of
// the step comes from the ballot.  !GATHER: len64[u], vlen[u] and *bad (a '#' or a zero byte in a label).
template <bool GATHER>
__global__ __launch_bounds__(PX_THREADS) void k_ps_labels(const uint8_t *msa, uint64_t n, const uint64_t *bounds, const uint32_t *node_block,
                                                         const uint32_t *node_row, uint64_t n_nodes, uint64_t *len64, uint32_t *vlen,
                                                         unsigned long long *bad, const uint64_t *loff, uint8_t *labels)
{
    const unsigned lane = threadIdx.x % FBG_WAVE;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / FBG_WAVE);
    for (uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE; u < n_nodes; u += nw) {
        uint64_t x0, x1;
        ps_block_range(bounds, n, node_block[u], x0, x1);
        const uint8_t *row = msa + (uint64_t)node_row[u] * n;
        uint8_t *out = GATHER ? labels + loff[u] : nullptr;
        uint64_t base = 0;
        bool sep = false;
        for (uint64_t xb = x0; xb < x1; xb += FBG_WAVE) {
            const uint64_t x = xb + lane;
            const uint8_t c = x < x1 ? row[x] : (uint8_t)'-';
            const bool keep = c != '-';
            const uint64_t bal = __ballot(keep);
            if (GATHER) { if (keep) out[base + __popcll(bal & px_low(lane))] = c; }
            else sep |= keep && (c == '#' || c == 0);
            base += __popcll(bal);
        }
        if (!GATHER) {
            if (lane == 0) {
                len64[u] = base;
                vlen[u] = base > 0xffffffffull ? 0xffffffffu : (uint32_t)base;
            }
            if (sep) *bad = 1;
        }
    }
}

// ---- the MSA coordinate table --------------------------------------------------------------------------------------
// Node u of block [x0, x1) with representative row r: col(u, o) = the column of the o-th non-gap cell of row r in the
// block.  A row without a gap there (|label(u)| == x1 - x0) needs no table: col = x0 + o.  Any other node gets
// nw = ceil((x1 - x0) / 64) bitmap words (bit k of word w: cell x0 + 64 w + k is not '-'), laid out in groups of PM_W
// words, each group headed by one unit that holds the non-gap cells before it: nw + ceil(nw / PM_W) u64 units.
__host__ __device__ __forceinline__ uint64_t pm_units(uint64_t width)
{
    const uint64_t nw = (width + 63) / 64;
    return nw + (nw + PM_W - 1) / PM_W;
}

// units[u] of every node (0 without gaps; units[n_nodes] = 0 for the scan); *gapped: nodes with a bitmap
__global__ void k_pm_units(const uint64_t *bounds, uint64_t n, const uint32_t *node_block, const uint64_t *len64, uint64_t n_nodes,
                           uint64_t *units, unsigned long long *gapped)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool gap = false;
    if (u < n_nodes) {
        uint64_t x0, x1;
        ps_block_range(bounds, n, node_block[u], x0, x1);
        gap = len64[u] != x1 - x0;
        units[u] = gap ? pm_units(x1 - x0) : 0;
    } else if (u == n_nodes) {
        units[u] = 0;
    }
    const uint64_t bal = __ballot(gap);
    if ((threadIdx.x % FBG_WAVE) == 0 && bal) atomicAdd(gapped, (unsigned long long)__popcll(bal));
}

// One wave per node (grid-stride), the walk of k_ps_labels: every step's ballot is one bitmap word.  uoff: the exclusive
// scan of units (uoff[u + 1] - uoff[u] != 0: the node has a bitmap; its last unit is uoff[u] + units - 1 < uoff[u + 1]).
// n < 2^32 and uoff[n_nodes] < 2^32 - 1 are the caller's checks.
__global__ __launch_bounds__(PX_THREADS) void k_pm_fill(const uint8_t *msa, uint64_t n, const uint64_t *bounds, const uint32_t *node_block,
                                                       const uint32_t *node_row, uint64_t n_nodes, const uint64_t *uoff, uint4 *mnode,
                                                       uint64_t *mbits)
{
    const unsigned lane = threadIdx.x % FBG_WAVE;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / FBG_WAVE);
    for (uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE; u < n_nodes; u += nw) {
        uint64_t x0, x1;
        ps_block_range(bounds, n, node_block[u], x0, x1);
        const uint32_t r = node_row[u];
        const uint64_t base = uoff[u];
        const bool gap = uoff[u + 1] != base;
        if (lane == 0) mnode[u] = make_uint4(r, (uint32_t)x0, gap ? (uint32_t)base : PM_NONE, (uint32_t)(x1 - x0));
        if (!gap) continue;
        const uint8_t *row = msa + (uint64_t)r * n;
        uint64_t before = 0, w = 0;
        for (uint64_t xb = x0; xb < x1; xb += FBG_WAVE, w++) {
            const uint64_t x = xb + lane;
            const uint64_t bal = __ballot(x < x1 && row[x] != '-');
            if (lane == 0) {
                uint64_t *grp = mbits + base + (w / PM_W) * (PM_W + 1);
                if (w % PM_W == 0) grp[0] = before;
                grp[1 + w % PM_W] = bal;
            }
            before += __popcll(bal);
        }
    }
}

__global__ void k_ps_edges(const unsigned long long *edges, const unsigned long long *edge_count, const uint64_t *ebase, uint64_t m,
                           uint64_t nb, uint32_t *esrc, uint32_t *edst)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * nb) return;
    const uint64_t j = t / m, k = t % m;
    if (k >= edge_count[j]) return;
    const unsigned long long pr = edges[t];
    const uint64_t e = ebase[j] + k;
    esrc[e] = (uint32_t)(pr >> 32);
    edst[e] = (uint32_t)pr;
}

__global__ void k_ps_touch(const uint32_t *esrc, const uint32_t *edst, uint64_t E, uint32_t *firstE, uint32_t *nout, uint32_t *nin)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t u = esrc[e], v = edst[e];
    atomicMin(&firstE[u], (uint32_t)e);
    atomicMin(&firstE[v], (uint32_t)e);
    atomicAdd(&nout[u], 1u);
    atomicAdd(&nin[v], 1u);
}

__global__ void k_ps_estart(const uint64_t *eoff, uint64_t E, uint32_t *estart)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e <= E) estart[e] = (uint32_t)eoff[e];
}

// the first edge of a node gives its label's text position: after '#' and reverse(label(dst)) when the node is the
// edge's source, right after '#' when it is its destination
__global__ void k_ps_node_tables(const uint32_t *firstE, const uint32_t *nout, const uint32_t *nin, const uint32_t *esrc,
                                 const uint32_t *edst, const uint32_t *estart, const uint32_t *vlen, uint64_t n_nodes,
                                 uint32_t *vtpos, uint8_t *vflag)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_nodes) return;
    const uint32_t e = firstE[u];
    uint32_t tp = 0;
    if (e != PS_NONE) tp = esrc[e] == u ? estart[e] + 1 + vlen[edst[e]] : estart[e] + 1;
    vtpos[u] = tp;
    vflag[u] = (uint8_t)((nout[u] ? PV_OUT : 0u) | (nin[u] ? PV_IN : 0u));
}

// hist[c] += degree(u) for every byte c of label(u): one wave per node, a workgroup's sums in LDS (they stay below the
// text length, which the caller has checked against 2^32), one global add per workgroup and symbol
__global__ __launch_bounds__(PX_THREADS) void k_ps_hist(const uint8_t *labels, const uint64_t *loff, const uint32_t *nout, const uint32_t *nin,
                                                       uint64_t n_nodes, unsigned long long *hist)
{
    __shared__ uint32_t h[256];
    for (int c = threadIdx.x; c < 256; c += blockDim.x) h[c] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x % FBG_WAVE;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / FBG_WAVE);
    for (uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE; u < n_nodes; u += nw) {
        const uint32_t use = nout[u] + nin[u];
        if (!use) continue;
        const uint64_t a = loff[u], b = loff[u + 1];
        for (uint64_t k = a + lane; k < b; k += FBG_WAVE) atomicAdd(&h[labels[k]], use);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 256; c += blockDim.x)
        if (h[c]) atomicAdd(&hist[c], (unsigned long long)h[c]);
}

// with_map: also the MSA coordinate table (fbg_pindex_build_segmentation; the rounds of fbg_segmentation_validate /
// _repair report no places and leave it out).  with_rows: also the row table (fbg_pindex_build_segmentation_rows only):
// copies of node_of and of the gathered labels and their offsets, owned by the index.
static int px_prepare_segmentation(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, PxPrep &pp, bool with_map,
                                   bool with_rows)
{
    fbg_ctx *ctx = ix->ctx;
    BlockGraphDev g;
    FBG_TRY(fbg_block_graph_device(ctx, boundaries, nb, &g));
    if (g.collision)
        return fbg_fail(ctx, FBG_ERR_HASH_COLLISION, "two different block labels share a 128-bit hash; use the host-side numbering");
    hipStream_t st = ctx->stream;
    const uint64_t m = ctx->m, n = ctx->n, cells = m * nb, n_nodes = g.n_nodes;
    if (n_nodes >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%llu nodes: at most 2^32 - 2", (unsigned long long)n_nodes);
    auto R = [&](std::vector<DevBuf *> &owner, DevBuf &b, size_t bytes) { return fbg_reserve(ctx, b, bytes + 8, &owner, false); };
    FBG_TRY(R(ix->bufs, ix->snode_block, n_nodes * 4));
    FBG_TRY(R(ix->bufs, ix->sfirst, (nb + 1) * 8));
    FBG_TRY(R(ix->bufs, ix->vlen, n_nodes * 4));
    FBG_TRY(R(ix->bufs, ix->vtpos, n_nodes * 4));
    FBG_TRY(R(ix->bufs, ix->vflag, n_nodes));
    FBG_TRY(R(s.bufs, s.nrow, n_nodes * 4));
    FBG_TRY(R(s.bufs, s.len64, (n_nodes + 1) * 8));
    FBG_TRY(R(s.bufs, s.loff, (n_nodes + 1) * 8));
    FBG_TRY(R(s.bufs, s.ebase, (nb + 1) * 8));
    FBG_TRY(R(s.bufs, s.firstE, n_nodes * 4));
    FBG_TRY(R(s.bufs, s.nout, n_nodes * 4));
    FBG_TRY(R(s.bufs, s.nin, n_nodes * 4));
    FBG_TRY(R(s.bufs, s.hist, 257 * 8));                 // 256 counts and the separator flag
    uint32_t *node_block = ix->snode_block.as<uint32_t>(), *node_row = s.nrow.as<uint32_t>(), *vlen = ix->vlen.as<uint32_t>();
    uint64_t *len64 = s.len64.as<uint64_t>(), *loff = s.loff.as<uint64_t>(), *ebase = s.ebase.as<uint64_t>();
    auto *hist = s.hist.as<unsigned long long>(), *bad = hist + 256;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->sfirst.p, g.first, (nb + 1) * 8, hipMemcpyDeviceToDevice, st));
    ix->has_rows = false;
    if (with_rows) {
        FBG_TRY(R(ix->bufs, ix->rw.node_of, cells * 4));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->rw.node_of.p, g.node_of, cells * 4, hipMemcpyDeviceToDevice, st));
    }
    FBG_HIP_TRY(ctx, hipMemsetAsync(hist, 0, 257 * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(len64 + n_nodes, 0, 8, st));
    hipLaunchKernelGGL(k_ps_nodes, dim3(fbg_blocks(cells, 256)), dim3(256), 0, st, g.rep_row, g.count, g.first, m, nb, node_block, node_row);
    const dim3 gw(fbg_blocks(n_nodes * FBG_WAVE, PX_THREADS, 4096));
    hipLaunchKernelGGL(k_ps_labels<false>, gw, dim3(PX_THREADS), 0, st, ctx->d_msa, n, g.bounds, (const uint32_t *)node_block,
                       (const uint32_t *)node_row, n_nodes, len64, vlen, bad, (const uint64_t *)nullptr, (uint8_t *)nullptr);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, len64, loff, (uint64_t)0, (size_t)(n_nodes + 1), rocprim::plus<uint64_t>(), st);
    }));
    // edges: the scan of edge_count places every block's list (entry nb of edge_count does not exist: scan nb, add the last)
    const unsigned long long *ecount = g.edge_count;
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, ecount, ebase + 1, (size_t)nb, rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ebase, 0, 8, st));
    uint64_t h_L = 0, h_E = 0, h_units = 0;
    unsigned long long h_bad = 0, h_gapped = 0;
    ix->has_map = false;
    if (with_map) {
        // the units of every node's bitmap and their scan; the host reads the total with the other sizes below
        if (n >= (1ull << 32))
            return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "the MSA has 2^32 columns or more; the MSA coordinates of a pattern index are 32-bit");
        FBG_TRY(R(s.bufs, s.munit, (n_nodes + 1) * 8));
        FBG_TRY(R(s.bufs, s.muoff, (n_nodes + 1) * 8));
        FBG_TRY(R(s.bufs, s.mctr, 8));
        FBG_TRY(R(ix->bufs, ix->mnode, n_nodes * 16));
        uint64_t *munit = s.munit.as<uint64_t>(), *muoff = s.muoff.as<uint64_t>();
        FBG_HIP_TRY(ctx, hipMemsetAsync(s.mctr.p, 0, 8, st));
        hipLaunchKernelGGL(k_pm_units, dim3(fbg_blocks(n_nodes + 1, 256)), dim3(256), 0, st, g.bounds, n, (const uint32_t *)node_block,
                           (const uint64_t *)len64, n_nodes, munit, s.mctr.as<unsigned long long>());
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, munit, muoff, (uint64_t)0, (size_t)(n_nodes + 1), rocprim::plus<uint64_t>(), st);
        }));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_units, muoff + n_nodes, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_gapped, s.mctr.p, 8, hipMemcpyDeviceToHost, st));
    }
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_L, loff + n_nodes, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_E, ebase + nb, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h_bad) return fbg_fail(ctx, FBG_ERR_INVALID, "the MSA may not contain '#' or a zero byte (both are separators of the index text)");
    const uint64_t L = h_L, E = h_E;
    FBG_TRY(fbg_reserve(ctx, s.labels, ((L + 7) & ~7ull) + 16, &s.bufs, false));
    FBG_HIP_TRY(ctx, hipMemsetAsync(s.labels.p, 0, s.labels.cap, st));
    hipLaunchKernelGGL(k_ps_labels<true>, gw, dim3(PX_THREADS), 0, st, ctx->d_msa, n, g.bounds, (const uint32_t *)node_block,
                       (const uint32_t *)node_row, n_nodes, (uint64_t *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr,
                       (const uint64_t *)loff, s.labels.as<uint8_t>());
    if (with_rows) {
        FBG_TRY(R(ix->bufs, ix->rw.labels, L));
        FBG_TRY(R(ix->bufs, ix->rw.loff, (n_nodes + 1) * 8));
        if (L) FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->rw.labels.p, s.labels.p, L, hipMemcpyDeviceToDevice, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->rw.loff.p, loff, (n_nodes + 1) * 8, hipMemcpyDeviceToDevice, st));
        ix->rw.m = m;
        ix->rw.label_bytes = L;
    }
    if (with_map) {
        // unit offsets are kept in 32 bits with PM_NONE set aside; the sums above are 64-bit, so nothing wraps
        if (h_units >= PM_NONE)
            return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "the MSA coordinate table of this segmentation takes %llu 64-bit words; it holds "
                            "fewer than 2^32 - 1", (unsigned long long)h_units);
        FBG_TRY(R(ix->bufs, ix->mbits, h_units * 8));
        hipLaunchKernelGGL(k_pm_fill, gw, dim3(PX_THREADS), 0, st, ctx->d_msa, n, g.bounds, (const uint32_t *)node_block,
                           (const uint32_t *)node_row, n_nodes, (const uint64_t *)s.muoff.as<uint64_t>(), ix->mnode.as<uint4>(),
                           ix->mbits.as<uint64_t>());
        ix->map_units = h_units;
        ix->map_gapped = h_gapped;
    }
    FBG_TRY(R(ix->bufs, ix->vesrc, E * 4));
    FBG_TRY(R(ix->bufs, ix->vedst, E * 4));
    FBG_TRY(R(ix->bufs, ix->vestart, (E + 1) * 4));
    FBG_TRY(R(s.bufs, s.elen, (E + 1) * 8));
    FBG_TRY(R(s.bufs, s.eoff, (E + 1) * 8));
    uint32_t *esrc = ix->vesrc.as<uint32_t>(), *edst = ix->vedst.as<uint32_t>(), *estart = ix->vestart.as<uint32_t>();
    uint32_t *firstE = s.firstE.as<uint32_t>(), *nout = s.nout.as<uint32_t>(), *nin = s.nin.as<uint32_t>();
    uint64_t *elen = s.elen.as<uint64_t>(), *eoff = s.eoff.as<uint64_t>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(firstE, 0xff, n_nodes * 4 + 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(nout, 0, n_nodes * 4 + 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(nin, 0, n_nodes * 4 + 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(elen + E, 0, 8, st));
    if (E) {
        hipLaunchKernelGGL(k_ps_edges, dim3(fbg_blocks(cells, 256)), dim3(256), 0, st, g.edges, g.edge_count, (const uint64_t *)ebase, m, nb,
                           esrc, edst);
        hipLaunchKernelGGL(k_ps_touch, dim3(fbg_blocks(E, 256)), dim3(256), 0, st, (const uint32_t *)esrc, (const uint32_t *)edst, E, firstE,
                           nout, nin);
        hipLaunchKernelGGL(k_px_edge_len, dim3(fbg_blocks(E, 256)), dim3(256), 0, st, (const uint32_t *)esrc, (const uint32_t *)edst,
                           (const uint64_t *)loff, E, elen);
    }
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, elen, eoff, (uint64_t)0, (size_t)(E + 1), rocprim::plus<uint64_t>(), st);
    }));
    uint64_t h_N = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&h_N, eoff + E, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h_N + 1 >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "the edge text of this graph has 2^32 symbols or more; the pattern index "
                        "takes texts of N + 1 < 2^32 symbols");
    hipLaunchKernelGGL(k_ps_estart, dim3(fbg_blocks(E + 1, 256)), dim3(256), 0, st, (const uint64_t *)eoff, E, estart);
    hipLaunchKernelGGL(k_ps_node_tables, dim3(fbg_blocks(n_nodes, 256)), dim3(256), 0, st, (const uint32_t *)firstE, (const uint32_t *)nout,
                       (const uint32_t *)nin, (const uint32_t *)esrc, (const uint32_t *)edst, (const uint32_t *)estart,
                       (const uint32_t *)vlen, n_nodes, ix->vtpos.as<uint32_t>(), ix->vflag.as<uint8_t>());
    if (E)
        hipLaunchKernelGGL(k_ps_hist, dim3(fbg_blocks(n_nodes * FBG_WAVE, PX_THREADS, 1024)), dim3(PX_THREADS), 0, st,
                           (const uint8_t *)s.labels.as<uint8_t>(), (const uint64_t *)loff, (const uint32_t *)nout, (const uint32_t *)nin,
                           n_nodes, hist);
    FBG_HIP_TRY(ctx, hipGetLastError());
    // the 256-entry table is finished on the host
    FBG_HIP_TRY(ctx, hipMemcpyAsync(pp.hist, hist, 256 * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    pp.hist[0] = 1;
    pp.hist['#'] = E;
    pp.n_nodes = n_nodes; pp.E = E; pp.N1 = h_N + 1;
    pp.eoff_ready = true;
    ix->from_segmentation = true;
    ix->has_map = with_map;
    ix->has_rows = with_rows;
    ix->seg_nb = nb;
    return FBG_OK;
}

static int px_build_segmentation(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, bool with_map,
                                 bool with_rows = false)
{
    PxPrep pp;
    FBG_TRY(px_prepare_segmentation(ix, s, boundaries, nb, pp, with_map, with_rows));
    return px_build_prepared(ix, s, pp);
}

static void px_destroy(fbg_pindex *ix)
{
    if (!ix) return;
    if (ix->ctx) {
        (void)hipSetDevice(ix->ctx->device);
        (void)hipStreamSynchronize(ix->ctx->stream);
    }
    fbg_release_all(nullptr, ix->bufs);
    if (ix->ev0) (void)hipEventDestroy(ix->ev0);
    if (ix->ev1) (void)hipEventDestroy(ix->ev1);
    if (ix->sv0) (void)hipEventDestroy(ix->sv0);
    if (ix->sv1) (void)hipEventDestroy(ix->sv1);
    delete ix;
}

// ---- semi-repeat-free validation (fbg_pindex_validate) -----------------------------------------------------------
struct PvDev {
    const uint32_t *sa, *tpos, *len, *estart, *esrc, *edst, *ctab, *block;
    const uint2 *rng;
    const uint8_t *flag, *text;
};

struct PvMask {
    uint64_t w[4];
};

// the edge whose string holds text position p: the last e with estart[e] <= p, searched between two coarse entries
__device__ __forceinline__ uint32_t pv_edge(const PvDev &d, uint32_t p)
{
    uint32_t lo = d.ctab[p >> PV_CSHIFT], hi = d.ctab[(p >> PV_CSHIFT) + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (d.estart[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The occurrence of a label (m symbols, node in block bu) whose reversed copy starts at text position p: the node and
// offset it starts at in label(a) + label(b) of its edge; true iff that is offset 0 of a node of block bu.
__device__ __forceinline__ bool pv_allowed(const PvDev &d, uint32_t p, uint32_t m, uint32_t bu, uint32_t &node, uint32_t &off)
{
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;   // ne = |a| + |b|
    const uint32_t a = d.esrc[e], la = d.len[a];
    const uint32_t s = ne - (p - base) - m;                                 // forward offset in label(a) + label(b)
    if (s < la) { node = a; off = s; } else { node = d.edst[e]; off = s - la; }
    return off == 0 && d.block[node] == bu;
}

__device__ __forceinline__ void pv_add_slots(unsigned long long *ctr, unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x % FBG_WAVE) == 0 && v) atomicAdd(ctr, v);
}

// One lane per node: rules 1-3, then a range of at most PV_SHORT slots scanned in slot order up to its first
// disallowed occurrence; longer ranges go to `list` for k_pv_wave (status VALID until that kernel finds otherwise).
// ctr[0]: list length, ctr[1]: SA slots scanned.
__global__ __launch_bounds__(PX_THREADS) void k_pv_node(PvDev d, uint64_t n, PvMask ig, int has_ig, uint8_t *status, uint32_t *wn,
                                                       uint32_t *wo, uint32_t *list, unsigned long long *ctr)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long slots = 0;
    if (u < n) {
        uint8_t st = FBG_NODE_VALID;
        uint32_t wnode = PV_NONE, woff = PV_NONE;
        const uint32_t m = d.len[u];
        bool ignored = false;
        if ((d.flag[u] & (PV_IN | PV_OUT)) == (PV_IN | PV_OUT) && has_ig) {
            const uint8_t *lab = d.text + d.tpos[u];        // reverse(label(u)): the order does not matter here
            for (uint32_t k = 0; k < m && !ignored; k++) {
                const uint32_t c = lab[k];
                ignored = (ig.w[c >> 6] >> (c & 63)) & 1u;
            }
        }
        if ((d.flag[u] & (PV_IN | PV_OUT)) != (PV_IN | PV_OUT)) st = FBG_NODE_SKIP_SOURCE_SINK;
        else if (ignored) st = FBG_NODE_SKIP_IGNORED;
        else if (m == 0) st = FBG_NODE_SKIP_EMPTY;
        else {
            const uint2 lr = d.rng[u];
            const uint32_t bu = d.block[u];
            if (lr.x <= lr.y && lr.y - lr.x < PV_SHORT) {
                for (uint32_t i = lr.x; i <= lr.y; i++) {
                    slots++;
                    uint32_t node, off;
                    if (!pv_allowed(d, d.sa[i], m, bu, node, off)) {
                        st = FBG_NODE_INVALID; wnode = node; woff = off;
                        break;
                    }
                }
            } else if (lr.x <= lr.y) {
                list[atomicAdd(&ctr[0], 1ull)] = (uint32_t)u;
            }
        }
        status[u] = st;
        wn[u] = wnode;
        wo[u] = woff;
    }
    pv_add_slots(&ctr[1], slots);
}

// One wave per listed node (a grid-stride loop over ctr[0] entries): 64 slots per step in ascending slot order; the
// lowest lane whose occurrence is disallowed is the witness, and the node's scan ends with that step.
__global__ __launch_bounds__(PX_THREADS) void k_pv_wave(PvDev d, const uint32_t *list, unsigned long long *ctr, uint8_t *status,
                                                       uint32_t *wn, uint32_t *wo)
{
    const uint64_t nlist = ctr[0];
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / FBG_WAVE);
    const unsigned lane = threadIdx.x % FBG_WAVE;
    unsigned long long slots = 0;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / FBG_WAVE; k < nlist; k += nw) {
        const uint32_t u = list[k];
        const uint32_t m = d.len[u], bu = d.block[u];
        const uint2 lr = d.rng[u];
        for (uint64_t b = lr.x; b <= lr.y; b += FBG_WAVE) {
            const uint64_t i = b + lane;
            uint32_t node = 0, off = 0;
            bool bad = false;
            if (i <= lr.y) {
                slots++;
                bad = !pv_allowed(d, d.sa[i], m, bu, node, off);
            }
            const uint64_t bal = __ballot(bad);
            if (bal) {
                if (lane == (unsigned)__builtin_ctzll(bal)) {
                    status[u] = FBG_NODE_INVALID;
                    wn[u] = node;
                    wo[u] = off;
                }
                break;
            }
        }
    }
    pv_add_slots(&ctr[1], slots);
}

// ---- occurrences (fbg_pindex_occurrences / _fetch) ---------------------------------------------------------------
// Per pattern: the totals, the capped sizes of both lists (entry n = 0, so that their exclusive scans are the n + 1
// CSR offsets) and what the expansion reads: the first slot of either list, and for the starts k (restarts > 0) or
// |P| (= pos of a found pattern).  A graph without edges has no places: sizes 0, the totals stand.
__global__ void k_po_sizes(const unsigned long long *count, const unsigned long long *pos, const uint2 *rec, uint64_t n, uint64_t cap,
                           int has_edges, uint64_t *etot, uint64_t *stot, uint64_t *esz, uint64_t *ssz, uint32_t *restarts,
                           uint32_t *el, uint32_t *ss, uint32_t *sk)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    if (t == n) { esz[n] = 0; ssz[n] = 0; return; }
    const uint64_t cnt = count[t];
    const uint2 lr = rec[3 * t], s = rec[3 * t + 1], kr = rec[3 * t + 2];
    const uint64_t st = cnt == 0 ? 0 : kr.y ? (uint64_t)s.y - s.x + 1 : cnt;
    etot[t] = cnt;
    stot[t] = st;
    esz[t] = has_edges ? (cnt < cap ? cnt : cap) : 0;
    ssz[t] = has_edges ? (st < cap ? st : cap) : 0;
    restarts[t] = kr.y;
    el[t] = lr.x;
    ss[t] = kr.y ? s.x : lr.x;
    sk[t] = kr.y ? kr.x : (uint32_t)pos[t];
}

__device__ __forceinline__ uint64_t po_uniform(uint64_t v)
{
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}

// the last q in [lo, hi] with off[q] <= x (off[lo] <= x is given)
__device__ __forceinline__ uint64_t po_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One lane per reported place, item i of a list's CSR order (off[n] = total items): the wave finds the patterns of
// its first and last item by a search of all n offsets that is the same in every lane, each lane then searches only
// between those two.  Item j of pattern q is SA slot first[q] + j; the place follows as in pv_allowed.  Lanes write
// consecutive entries: a pattern's places are contiguous and in slot order.  STARTS: offsets of the match's start.
template <bool STARTS>
__global__ __launch_bounds__(PX_THREADS) void k_po_expand(PvDev d, const uint64_t *off, uint64_t n, uint64_t total,
                                                         const uint32_t *first, const uint32_t *sk, const uint32_t *restarts,
                                                         uint32_t *osrc, uint32_t *odst, uint32_t *oofs)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t w0 = po_uniform(i & ~(uint64_t)(FBG_WAVE - 1));
    if (w0 >= total) return;
    const uint64_t w1 = w0 + FBG_WAVE - 1 < total ? w0 + FBG_WAVE - 1 : total - 1;
    const uint64_t q0 = po_uniform(po_find(off, 0, n - 1, w0));
    const uint64_t q1 = po_uniform(po_find(off, q0, n - 1, w1));
    if (i >= total) return;
    const uint64_t q = po_find(off, q0, q1, i);
    const uint32_t p = d.sa[first[q] + (uint32_t)(i - off[q])];
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;
    uint32_t o = ne - 1 - (p - base);                 // of the pattern's last symbol (starts after a restart: p = base - 1)
    if (STARTS) o = restarts[q] ? ne - sk[q] : o - sk[q] + 1;
    osrc[i] = d.esrc[e];
    odst[i] = d.edst[e];
    oofs[i] = o;
}

struct PmDev {
    const uint4 *node;
    const uint64_t *bits;
};

// the position of the k-th (from 0) set bit of w, k < popcount(w): halves narrowed by their popcounts, six steps
__device__ __forceinline__ uint32_t pm_select(uint64_t w, uint32_t k)
{
    uint32_t pos = 0;
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        const uint32_t c = __popcll(w & ((1ull << h) - 1));
        if (k >= c) { k -= c; w >>= h; pos += h; }
    }
    return pos;
}

// col(u, o) of a node with entry nd = (row, x0, first unit, width), o < |label(u)|: the last group whose count is at
// most o (a search over the node's ceil(nw / PM_W) group heads), then at most PM_W words of that group.  A table that
// disagreed with |label(u)| would end the word loop without a hit: PM_NONE then, never a read past the node's units.
__device__ __forceinline__ uint32_t pm_col(const PmDev &m, const uint4 nd, uint32_t o)
{
    if (nd.z == PM_NONE) return nd.y + o;
    const uint64_t *b = m.bits + nd.z;
    const uint32_t nw = (nd.w + 63) / 64;
    uint32_t lo = 0, hi = (nw + PM_W - 1) / PM_W - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (b[(uint64_t)mid * (PM_W + 1)] <= o) lo = mid; else hi = mid - 1;
    }
    const uint64_t *grp = b + (uint64_t)lo * (PM_W + 1);
    uint32_t k = o - (uint32_t)grp[0];
    const uint32_t w0 = lo * PM_W, wn = nw - w0 < PM_W ? nw - w0 : PM_W;
    for (uint32_t j = 0; j < wn; j++) {
        const uint64_t w = grp[1 + j];
        const uint32_t c = __popcll(w);
        if (k < c) return nd.y + (w0 + j) * 64 + pm_select(w, k);
        k -= c;
    }
    return PM_NONE;
}

// k_po_expand for the MSA coordinate of every place: the same lane per place, the same search of the offsets and the
// same SA slot -> edge -> offset; then the node and offset of Occurrences.as_nodes (the source below |label(src)|, else
// the destination), and through the table the row and column of that cell of the node's representative row.  An offset
// outside S_e (a pattern with '#' or a zero byte) gets PM_NONE in both.  Lanes write consecutive entries of orow / ocol.
template <bool STARTS>
__global__ __launch_bounds__(PX_THREADS) void k_po_expand_msa(PvDev d, PmDev m, const uint64_t *off, uint64_t n, uint64_t total,
                                                             const uint32_t *first, const uint32_t *sk, const uint32_t *restarts,
                                                             uint32_t *orow, uint32_t *ocol)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t w0 = po_uniform(i & ~(uint64_t)(FBG_WAVE - 1));
    if (w0 >= total) return;
    const uint64_t w1 = w0 + FBG_WAVE - 1 < total ? w0 + FBG_WAVE - 1 : total - 1;
    const uint64_t q0 = po_uniform(po_find(off, 0, n - 1, w0));
    const uint64_t q1 = po_uniform(po_find(off, q0, n - 1, w1));
    if (i >= total) return;
    const uint64_t q = po_find(off, q0, q1, i);
    const uint32_t p = d.sa[first[q] + (uint32_t)(i - off[q])];
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;
    uint32_t o = ne - 1 - (p - base);
    if (STARTS) o = restarts[q] ? ne - sk[q] : o - sk[q] + 1;
    uint32_t u = d.esrc[e];
    const uint32_t la = d.len[u];
    if (o >= la) { u = d.edst[e]; o -= la; }
    uint32_t row = PM_NONE, col = PM_NONE;
    if (o < d.len[u]) {
        const uint4 nd = m.node[u];
        col = pm_col(m, nd, o);
        row = col == PM_NONE ? PM_NONE : nd.x;
    }
    orow[i] = row;
    ocol[i] = col;
}

// ---- chains (fbg_pindex_chains) ------------------------------------------------------------------------------------
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

// key = start places of the read (what picks its tier), id = the read; reads without one are done here
__global__ void k_pc_key(PcDev d, uint64_t n, uint32_t *key, uint32_t *id)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;
    if (t < n) {
        const uint64_t cnt = d.start_off[d.seed_off[t + 1]] - d.start_off[d.seed_off[t]];
        key[t] = (uint32_t)cnt;
        id[t] = (uint32_t)t;
        tier = cnt == 0 ? 0 : cnt <= PC_SMALL ? 1 : cnt <= PC_LDS ? 2 : 3;
        if (cnt == 0) { d.end[t] = PC_NONE; d.score[t] = 0; }
    }
    for (int b = 0; b < 4; b++) {
        const unsigned long long m = __ballot(tier == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[b], (unsigned long long)__popcll(m));
    }
}

// what a seed's lanes wrote becomes visible to the lanes of the same wave that scan it for the next seed
__device__ __forceinline__ void pc_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The DP of one read on G lanes (lane = 0 .. G - 1), state st[0 .. places of the read) = (best, column, q_start, length).
// Seed by seed: the lanes take the seed's places G at a time, each scans the state of all earlier seeds' places in
// ascending order -- every lane reads the same entry, a broadcast -- and keeps the first of the best predecessors; the
// seed's own entries are written meanwhile (nobody reads them before the next seed) and published by pc_sync.  A lane
// meets its own places in ascending order, so the first maximum it keeps is its smallest; the G lanes' maxima are
// merged by (best descending, place ascending).  live = false: a group without a read, which only takes part in the
// shuffles.
template <int G, class ST>
__device__ __forceinline__ void pc_read(const PcDev &d, bool live, uint32_t R, uint32_t lane, ST st)
{
    const uint64_t s0 = live ? d.seed_off[R] : 0, s1 = live ? d.seed_off[R + 1] : 0;
    const uint64_t g0 = live ? d.start_off[s0] : 0;
    uint32_t bestv = 0, bestj = PC_NONE, valid = 0;
    for (uint64_t t = s0; t < s1; t++) {
        const uint32_t a0 = (uint32_t)(d.start_off[t] - g0), a1 = (uint32_t)(d.start_off[t + 1] - g0);
        const uint32_t q = d.q[t], k = d.k[t];
        for (uint32_t j = a0 + lane; j < a1; j += G) {
            const uint32_t c = d.col[g0 + j];
            uint32_t b = 0, p = PC_NONE;
            if (c != PC_NONE) {
                uint32_t m = 0;
                for (uint32_t i = 0; i < a0; i++) {
                    const uint4 e = st[i];
                    const int64_t dc = (int64_t)c - (int64_t)e.y;
                    const int64_t sur = dc - ((int64_t)q - (int64_t)e.z);
                    const uint64_t mag = sur < 0 ? (uint64_t)-sur : (uint64_t)sur;
                    if (e.x > m && dc >= (int64_t)e.w && mag <= d.band) { m = e.x; p = i; }
                }
                b = k + m;
                valid++;
                if (b > bestv) { bestv = b; bestj = j; }
            }
            d.pred[g0 + j] = p == PC_NONE ? PC_NONE : (uint32_t)(g0 + p);
            st[j] = make_uint4(b, c, q, k);
        }
        pc_sync();
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const uint32_t ov = __shfl_xor(bestv, o, G), oj = __shfl_xor(bestj, o, G);
        valid += __shfl_xor(valid, o, G);
        if (ov > bestv || (ov == bestv && oj < bestj)) { bestv = ov; bestj = oj; }
    }
    if (live && lane == 0) {
        d.end[R] = bestj == PC_NONE ? PC_NONE : (uint32_t)(g0 + bestj);
        d.score[R] = bestv;
        if (valid) atomicAdd(&d.ctr[4], (unsigned long long)valid);
    }
}

// The reads ids[0 .. cnt) of one tier.  TIER 0 (small): PC_SUB lanes per read, PX_THREADS / PC_SUB reads per workgroup,
// PC_SMALL entries of LDS each.  TIER 1 (wave): one wave per workgroup and read, PC_LDS entries of LDS.  TIER 2 (spill):
// the same with the read's stretch of the slab in device memory.  The binning guarantees the capacities; a read beyond
// its tier's would be left without a chain, never written past the array.
template <int TIER>
__global__ __launch_bounds__(TIER == 0 ? PX_THREADS : FBG_WAVE) void k_pc_chain(PcDev d, const uint32_t *ids, uint64_t cnt)
{
    __shared__ uint4 lds[TIER == 0 ? PX_THREADS / PC_SUB * PC_SMALL : TIER == 1 ? PC_LDS : 1];
    if constexpr (TIER == 0) {
        const uint64_t i = (uint64_t)blockIdx.x * (PX_THREADS / PC_SUB) + threadIdx.x / PC_SUB;
        bool live = i < cnt;
        const uint32_t R = live ? ids[i] : 0;
        if (live && d.start_off[d.seed_off[R + 1]] - d.start_off[d.seed_off[R]] > PC_SMALL) live = false;
        pc_read<PC_SUB>(d, live, R, threadIdx.x % PC_SUB, lds + threadIdx.x / PC_SUB * PC_SMALL);
    } else {
        const uint64_t i = blockIdx.x;
        if (i >= cnt) return;
        const uint32_t R = ids[i];
        if constexpr (TIER == 1) {
            if (d.start_off[d.seed_off[R + 1]] - d.start_off[d.seed_off[R]] > PC_LDS) return;
            pc_read<FBG_WAVE>(d, true, R, threadIdx.x, lds);
        } else {
            pc_read<FBG_WAVE>(d, true, R, threadIdx.x, d.slab + d.start_off[d.seed_off[R]]);
        }
    }
}

// One lane per read follows pred back from the chain's end.  The counting pass stores the chain's length (0 below
// min_score or without an anchor; entry n = 0 for the scan); the writing pass fills the read's stretch off[R] ..
// off[R + 1] from its last entry backwards, so that it ascends in q_start: the place, and its seed by a search of the
// read's stretch of start_off.  Either walk ends after as many steps as the read has seeds, whatever pred holds.
template <bool WRITE>
__global__ void k_pc_trace(PcDev d, uint64_t n, uint64_t min_score, uint64_t *len, const uint64_t *off, uint32_t *oplace, uint32_t *oseed)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    if (t == n) { if (!WRITE) len[n] = 0; return; }
    const uint64_t s0 = d.seed_off[t], s1 = d.seed_off[t + 1];
    uint32_t g = d.end[t];
    if (d.score[t] < min_score) g = PC_NONE;
    if (!WRITE) {
        uint64_t c = 0;
        while (g != PC_NONE && c < s1 - s0) { c++; g = d.pred[g]; }
        len[t] = c;
    } else {
        const uint64_t o0 = off[t];
        for (uint64_t i = off[t + 1] - o0; i-- > 0 && g != PC_NONE;) {
            oplace[o0 + i] = g;
            oseed[o0 + i] = (uint32_t)po_find(d.start_off, s0, s1 - 1, g);
            g = d.pred[g];
        }
    }
}

// fbg_pindex_chain_strands: one lane per given read R < n picks between the chains of the virtual reads R and n + R.
// len is what the counting trace left (0 below min_score).  ctr: reads that went forward, reverse, to neither; summed
// per wave before the atomic.
__global__ void k_pc_strand(const uint32_t *score, const uint64_t *len, uint64_t n, uint8_t *strand, uint32_t *best,
                            unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int out = -1;
    if (R < n) {
        const uint32_t s0 = score[R], s1 = score[n + R];
        const int t = s1 > s0;
        out = len[t ? n + R : R] ? t : 2;
        strand[R] = out == 2 ? (uint8_t)FBG_STRAND_NONE : (uint8_t)out;
        best[R] = t ? s1 : s0;
    }
    for (int b = 0; b < 3; b++) {
        const unsigned long long m = __ballot(out == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&ctr[b], (unsigned long long)__popcll(m));
    }
}

// ---- rows (fbg_pindex_seeds_rows / fbg_pindex_chains_rows) ----------------------------------------------------------
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

// sbase[t] = poff[R] + q_start[t] for seed t of read R (a search of the n + 1 seed offsets, as k_pc_trace's)
__global__ void k_pr_seed(const uint64_t *seed_off, const uint64_t *poff, const uint32_t *q, uint64_t n, uint64_t S, uint64_t *sbase)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return;
    sbase[t] = poff[po_find(seed_off, 0, n - 1, t)] + q[t];
}

// k_po_expand_msa<true> up to the node and offset of the place, then rec[i] = (u, o, seed, block(u)); u = PR_NONE where
// o is not below |label(u)| (no row supports such a place).
__global__ __launch_bounds__(PX_THREADS) void k_pr_place(PvDev d, const uint32_t *node_block, const uint64_t *off, uint64_t n, uint64_t total,
                                                        const uint32_t *first, const uint32_t *sk, const uint32_t *restarts, uint4 *rec)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t w0 = po_uniform(i & ~(uint64_t)(FBG_WAVE - 1));
    if (w0 >= total) return;
    const uint64_t w1 = w0 + FBG_WAVE - 1 < total ? w0 + FBG_WAVE - 1 : total - 1;
    const uint64_t q0 = po_uniform(po_find(off, 0, n - 1, w0));
    const uint64_t q1 = po_uniform(po_find(off, q0, n - 1, w1));
    if (i >= total) return;
    const uint64_t q = po_find(off, q0, q1, i);
    const uint32_t p = d.sa[first[q] + (uint32_t)(i - off[q])];
    const uint32_t e = pv_edge(d, p);
    const uint32_t base = d.estart[e] + 1, ne = d.estart[e + 1] - base;
    uint32_t o = restarts[q] ? ne - sk[q] : ne - 1 - (p - base) - sk[q] + 1;
    uint32_t u = d.esrc[e];
    const uint32_t la = d.len[u];
    if (o >= la) { u = d.edst[e]; o -= la; }
    const bool in = o < d.len[u];
    rec[i] = make_uint4(in ? u : PR_NONE, o, (uint32_t)q, in ? node_block[u] : 0u);
}

// Does the text of row r from offset o of its node u in block j on start with S[0 .. k)?  k >= 1, o < |label(u)|.
// Every read is bounded: a label by its length, the row's cells by block nb, S by k.
__device__ __forceinline__ bool pr_walk(const PrDev &d, uint64_t r, uint32_t u, uint32_t o, uint64_t j, const uint8_t *S, uint32_t k)
{
    uint32_t pos = 0;
    uint64_t a = d.loff[u] + o, b = d.loff[u + 1];
    for (;;) {
        const uint64_t take = b - a < (uint64_t)(k - pos) ? b - a : (uint64_t)(k - pos);
        for (uint64_t x = 0; x < take; x++)
            if (d.labels[a + x] != S[pos + x]) return false;
        pos += (uint32_t)take;
        if (pos == k) return true;
        uint32_t v;
        do {
            if (++j >= d.nb) return false;        // the row ends before the seed does
            v = d.node_of[j * d.m + r];
        } while (v == PR_NONE);
        a = d.loff[v];
        b = d.loff[v + 1];
    }
}

// rec of one place and row r: is r in rows(place)?
__device__ __forceinline__ bool pr_supports(const PrDev &d, const uint4 rc, uint64_t r)
{
    if (rc.x == PR_NONE || d.node_of[(uint64_t)rc.w * d.m + r] != rc.x) return false;
    return pr_walk(d, r, rc.x, rc.y, rc.w, d.reads + d.sbase[rc.z], d.slen[rc.z]);
}

// the G bits of a wave-wide ballot that belong to the group whose first lane is sh
template <int G> __device__ __forceinline__ uint64_t pr_group_bits(bool ok, unsigned sh)
{
    const uint64_t bal = __ballot(ok);
    return G == FBG_WAVE ? bal : (bal >> sh) & ((1ull << (G % 64)) - 1);
}

// G lanes per start place, the lanes are rows, G at a time: one coalesced read of the block's stretch of node_of, the
// lanes that hold the place's node walk, the ballot is the chunk of the set.  Every lane of the wave runs the row loop
// (m is the same for all), so the ballots meet; places past the end and rows past m only vote no.
template <int G>
__global__ __launch_bounds__(PX_THREADS) void k_pr_rows(PrDev d, const uint4 *rec, uint64_t total, uint32_t *n_rows, uint32_t *first_row,
                                                       unsigned long long *unsupported)
{
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const unsigned lane = threadIdx.x % FBG_WAVE, gl = lane % G, sh = lane - gl;
    const bool live = i < total;
    const uint4 rc = live ? rec[i] : make_uint4(PR_NONE, 0, 0, 0);
    uint32_t cnt = 0, first = PR_NONE;
    for (uint64_t r0 = 0; r0 < d.m; r0 += G) {
        const uint64_t r = r0 + gl;
        const uint64_t bits = pr_group_bits<G>(r < d.m && pr_supports(d, rc, r), sh);
        if (bits && first == PR_NONE) first = (uint32_t)r0 + (uint32_t)__ffsll((unsigned long long)bits) - 1;
        cnt += __popcll(bits);
    }
    if (live && gl == 0) { n_rows[i] = cnt; first_row[i] = first; }
    const uint64_t none = __ballot(live && gl == 0 && cnt == 0);
    if (lane == 0 && none) atomicAdd(unsupported, (unsigned long long)__popcll(none));
}

// G lanes per read: a lane stays with its row while the row supports anchor after anchor of the read's chain (place:
// the g of every chain entry, off: the n + 1 chain offsets) and drops out at the first that it does not; with a wave
// per read the loop over the anchors ends as soon as no lane is left, that is, when the word of the set is zero.  What
// is left after the last anchor is the chunk of the intersection.  bits (may be NULL): words 64-bit words per read; a
// chunk is shifted into its word, which is stored when it is complete or the rows end, so rows past m stay zero.
template <int G>
__global__ __launch_bounds__(PX_THREADS) void k_pr_chain(PrDev d, const uint4 *rec, const uint32_t *place, const uint64_t *off, uint64_t n,
                                                        uint64_t words, uint32_t *n_rows, uint32_t *first_row, uint64_t *bits_out,
                                                        unsigned long long *unsupported)
{
    const uint64_t R = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const unsigned lane = threadIdx.x % FBG_WAVE, gl = lane % G, sh = lane - gl;
    const bool live = R < n;
    const uint64_t o0 = live ? off[R] : 0, len = live ? off[R + 1] - o0 : 0;
    uint32_t cnt = 0, first = PR_NONE;
    uint64_t word = 0;
    for (uint64_t r0 = 0; r0 < d.m; r0 += G) {
        const uint64_t r = r0 + gl;
        bool ok = len != 0 && r < d.m;
        for (uint64_t a = 0; a < len; a++) {
            if (G == FBG_WAVE && !__any(ok)) break;      // one read per wave: len and this test are the same in every lane
            if (ok) ok = pr_supports(d, rec[place[o0 + a]], r);
        }
        const uint64_t bits = pr_group_bits<G>(ok, sh);
        if (bits && first == PR_NONE) first = (uint32_t)r0 + (uint32_t)__ffsll((unsigned long long)bits) - 1;
        cnt += __popcll(bits);
        word |= bits << (r0 % 64);
        if ((r0 + G) % 64 == 0 || r0 + G >= d.m) {
            if (bits_out && live && gl == 0) bits_out[R * words + r0 / 64] = word;
            word = 0;
        }
    }
    if (live && gl == 0) { n_rows[R] = cnt; first_row[R] = first; }
    const uint64_t none = __ballot(live && gl == 0 && len != 0 && cnt == 0);
    if (lane == 0 && none) atomicAdd(unsupported, (unsigned long long)__popcll(none));
}

// ---- alignment (fbg_pindex_chains_align) ----------------------------------------------------------------------------
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

// pref[j * m + r] = p(r, j): one lane per row steps over the blocks, so a wave reads and writes 64 consecutive rows
__global__ void k_pa_prefix(const uint32_t *node_of, const uint64_t *loff, uint64_t m, uint64_t nb, uint32_t *pref)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    uint32_t run = 0;
    for (uint64_t j = 0; j < nb; j++) {
        pref[j * m + r] = run;
        const uint32_t v = node_of[j * m + r];
        if (v != PR_NONE) run += (uint32_t)(loff[v + 1] - loff[v]);
    }
}

// One lane per read, after k_pr_chain chose the row (first_row; rec, place, off as there; q: q_start per seed): the
// diagonals of the chain's anchors on that row, the window, the skip status and the block, node and offset at which
// the window starts (a search of the row's column of pref).  Writes row and, where nothing is aligned, PA_NONE into
// the three other outputs (out: 4 n); wlen[R] = |W| of an aligned read, else 0, wlen[n] = 0.  ctr[1 .. 4]: reads
// aligned, too long, too wide, and the cells, summed per wave before the atomic.
__global__ void k_pa_prepare(PaDev d, const uint4 *rec, const uint32_t *place, const uint64_t *off, const uint32_t *q,
                             const uint32_t *first_row, uint64_t n, uint64_t pad, uint64_t max_window, uint4 *info, uint4 *start,
                             uint64_t *wlen, uint32_t *out, unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kind = -1;                // 0 aligned, 1 too long, 2 too wide
    unsigned long long cells = 0;
    if (R == n) wlen[n] = 0;
    if (R < n) {
        const uint64_t o0 = off[R], len = off[R + 1] - o0, L = d.roff[R + 1] - d.roff[R];
        const uint32_t r = len ? first_row[R] : PR_NONE;
        uint4 in = make_uint4(r, 0, 0, (uint32_t)L), at = make_uint4(0, 0, 0, 0);
        if (r != PR_NONE) {
            long long dmin = 0, dmax = 0;
            for (uint64_t a = 0; a < len; a++) {
                const uint4 rc = rec[place[o0 + a]];
                const long long dg = (long long)d.pref[(uint64_t)rc.w * d.m + r] + rc.y - (long long)q[rc.z];
                if (a == 0 || dg < dmin) dmin = dg;
                if (a == 0 || dg > dmax) dmax = dg;
            }
            const uint64_t jl = (d.nb - 1) * d.m + r;
            const uint32_t vl = d.node_of[jl];
            const long long glen = (long long)d.pref[jl] + (vl != PR_NONE ? (long long)(d.loff[vl + 1] - d.loff[vl]) : 0);
            const long long lo = dmin - (long long)pad, hi = dmax + (long long)L + (long long)pad;
            const uint64_t w0 = lo > 0 ? (uint64_t)lo : 0, w1 = hi < glen ? (uint64_t)hi : (uint64_t)glen;
            kind = L > PA_MAX_READ ? 1 : max_window && w1 - w0 > max_window ? 2 : 0;
            if (kind == 0) {
                uint64_t a = 0, b = d.nb - 1;
                while (a < b) {
                    const uint64_t mid = a + (b - a + 1) / 2;
                    if (d.pref[mid * d.m + r] <= w0) a = mid; else b = mid - 1;
                }
                in.y = (uint32_t)w0;
                in.z = (uint32_t)(w1 - w0);
                at = make_uint4((uint32_t)a, d.node_of[a * d.m + r], (uint32_t)w0 - d.pref[a * d.m + r], 0);
                cells = (unsigned long long)L * (w1 - w0);
            }
        }
        info[R] = in;
        start[R] = at;
        wlen[R] = in.z;
        out[R] = r;
        if (kind != 0) out[n + R] = out[2 * n + R] = out[3 * n + R] = PA_NONE;
    }
    for (int off2 = FBG_WAVE / 2; off2 > 0; off2 >>= 1) cells += __shfl_xor(cells, off2);
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    for (int b = 0; b < 3; b++) {
        const unsigned long long mk = __ballot(kind == b);
        if (mk && first) atomicAdd(&ctr[1 + b], (unsigned long long)__popcll(mk));
    }
    if (cells && first) atomicAdd(&ctr[4], cells);
}

// A wave per read writes its window W = G_r[w0 : w1) to win + woff[R]: label after label of the row's nodes from the
// start node on, the lanes taking consecutive bytes of a label; cells without a node are passed over.  Every loop is
// bounded: a label by its length, the window by |W|, the row's cells by block nb.
__global__ __launch_bounds__(FBG_WAVE) void k_pa_gather(PaDev d, const uint4 *info, const uint4 *start, const uint64_t *woff, uint8_t *win)
{
    const uint64_t R = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t wl = in.z;
    if (wl == 0) return;
    const uint4 at = start[R];
    if (at.y == PR_NONE) return;
    uint8_t *dst = win + woff[R];
    uint64_t j = at.x, a = d.loff[at.y] + at.z, b = d.loff[at.y + 1];
    uint32_t done = 0;
    for (;;) {
        const uint32_t take = b - a < (uint64_t)(wl - done) ? (uint32_t)(b - a) : wl - done;
        for (uint32_t x = lane; x < take; x += FBG_WAVE) dst[done + x] = d.labels[a + x];
        done += take;
        if (done == wl) return;
        uint32_t v;
        do {
            if (++j >= d.nb) return;
            v = d.node_of[j * d.m + in.x];
        } while (v == PR_NONE);
        a = d.loff[v];
        b = d.loff[v + 1];
    }
}

// One column of Myers' bit-vector recurrence for a word of 64 read symbols (Hyyro's block form).  eq: the rows of the
// word whose read symbol equals the column's text symbol; pv / mv: the rows whose vertical difference D(i, j) -
// D(i - 1, j) is +1 / -1; hin: the horizontal difference D(i0, j) - D(i0, j - 1) of the row below the word's first;
// -> the horizontal difference of the row whose bit is top.  Bits above top never reach the bits below it.
__device__ __forceinline__ int pa_step(uint64_t eq, uint64_t &pv, uint64_t &mv, int hin, uint64_t top)
{
    const uint64_t neg = hin < 0 ? 1 : 0;
    const uint64_t xv = eq | mv;
    eq |= neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
    const int hout = (ph & top) ? 1 : (mh & top) ? -1 : 0;
    ph = (ph << 1) | (hin > 0 ? 1 : 0);
    mh = (mh << 1) | neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// 64 text symbols of a pass per load, lane t takes column j0 + t; REV: the text backwards
template <bool REV> __device__ __forceinline__ int pa_chunk(const uint8_t *W, uint32_t wl, uint32_t j0, unsigned lane)
{
    const uint32_t j = j0 + lane;
    return j < wl ? (int)W[REV ? wl - 1 - j : j] : 0;
}

// One pass of a wave over the text W[0 .. wl) with a read of exactly NW words, the state in registers: lane i holds
// read symbols i, 64 + i, ...  (256: no symbol, equal to no byte, which masks the last word to L % 64 bits), a text byte
// is made wave-uniform by readlane and its match word is one ballot per read word.  D(L, j) is followed at bit L - 1 of
// the last word; -> best = min_j D(L, j) and bestj, the smallest j that attains it (D(L, 0) = L).  REV: the read and the
// text backwards and D(0, j) = j, which is the carry-in 1 of the first word.
// HIST (fbg_pindex_chains_cigar): lane 0 also writes pv and mv of every word after column j to hist[(j * NW + w) * 2].
template <int NW, bool REV, bool HIST = false>
__device__ __forceinline__ void pa_pass_reg(const uint8_t *P, uint32_t L, const uint8_t *W, uint32_t wl, unsigned lane, uint32_t &best,
                                            uint32_t &bestj, uint64_t *hist = nullptr)
{
    int p[NW];
    uint64_t pv[NW], mv[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint32_t i = w * 64 + lane;
        p[w] = i < L ? (int)P[REV ? L - 1 - i : i] : 256;
        pv[w] = ~0ull;
        mv[w] = 0;
    }
    const uint64_t top = 1ull << ((L - 1) & 63);
    uint32_t score = L;
    best = L;
    bestj = 0;
    for (uint32_t j0 = 0; j0 < wl; j0 += 64) {
        const int chunk = pa_chunk<REV>(W, wl, j0, lane);
        const uint32_t cnt = wl - j0 < 64 ? wl - j0 : 64;
        for (uint32_t t = 0; t < cnt; t++) {
            const int c = __builtin_amdgcn_readlane(chunk, t);
            int h = REV ? 1 : 0;
#pragma unroll
            for (int w = 0; w < NW; w++) h = pa_step(__ballot(p[w] == c), pv[w], mv[w], h, w == NW - 1 ? top : 1ull << 63);
            if (HIST && lane == 0) {
                uint64_t *col = hist + (uint64_t)(j0 + t) * (2 * NW);
#pragma unroll
                for (int w = 0; w < NW; w++) { col[2 * w] = pv[w]; col[2 * w + 1] = mv[w]; }
            }
            score += h;
            if (score < best) { best = score; bestj = j0 + t + 1; }
        }
    }
}

// The same pass for a read of nw > PA_REG_WORDS words: the read (rd) and the state (st: pv, then mv) in LDS and a loop
// over the words.  Every lane computes and stores the same state and reads back what it stored itself, and a lane reads
// the read symbols it staged itself: no lane waits for another, so there is no barrier.  HIST: lane w < nw also writes
// word w's pv and mv after column j (which it stored itself) to hist[(j * nw + w) * 2], 16 consecutive bytes per lane.
template <bool REV, bool HIST = false>
__device__ __forceinline__ void pa_pass_lds(const uint8_t *P, uint32_t L, uint32_t nw, const uint8_t *W, uint32_t wl, unsigned lane,
                                            uint8_t *rd, uint64_t *st, uint32_t &best, uint32_t &bestj, uint64_t *hist = nullptr)
{
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t i = w * 64 + lane;
        rd[i] = i < L ? P[REV ? L - 1 - i : i] : 0;
        st[w] = ~0ull;
        st[PA_MAX_READ / 64 + w] = 0;
    }
    const uint64_t top = 1ull << ((L - 1) & 63);
    uint32_t score = L;
    best = L;
    bestj = 0;
    for (uint32_t j0 = 0; j0 < wl; j0 += 64) {
        const int chunk = pa_chunk<REV>(W, wl, j0, lane);
        const uint32_t cnt = wl - j0 < 64 ? wl - j0 : 64;
        for (uint32_t t = 0; t < cnt; t++) {
            const int c = __builtin_amdgcn_readlane(chunk, t);
            int h = REV ? 1 : 0;
            for (uint32_t w = 0; w < nw; w++) {
                const uint32_t i = w * 64 + lane;
                uint64_t pv = st[w], mv = st[PA_MAX_READ / 64 + w];
                h = pa_step(__ballot(i < L && rd[i] == c), pv, mv, h, w == nw - 1 ? top : 1ull << 63);
                st[w] = pv;
                st[PA_MAX_READ / 64 + w] = mv;
            }
            if (HIST && lane < nw) {
                uint64_t *col = hist + ((uint64_t)(j0 + t) * nw + lane) * 2;
                col[0] = st[lane];
                col[1] = st[PA_MAX_READ / 64 + lane];
            }
            score += h;
            if (score < best) { best = score; bestj = j0 + t + 1; }
        }
    }
}

template <bool REV>
__device__ __forceinline__ void pa_pass(const uint8_t *P, uint32_t L, const uint8_t *W, uint32_t wl, unsigned lane, uint8_t *rd, uint64_t *st,
                                        uint32_t &best, uint32_t &bestj)
{
    const uint32_t nw = (L + 63) / 64;         // the tier: the same in every lane
    if (nw == 1) pa_pass_reg<1, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 2) pa_pass_reg<2, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 3) pa_pass_reg<3, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 4) pa_pass_reg<4, REV>(P, L, W, wl, lane, best, bestj);
    else pa_pass_lds<REV>(P, L, nw, W, wl, lane, rd, st, best, bestj);
}

// A wave per aligned read, 1 <= L <= PA_MAX_READ: the forward pass over the window gives edits and the smallest end e,
// the backward pass over W[0 : e) the largest start.  out as in k_pa_prepare.
__global__ __launch_bounds__(FBG_WAVE) void k_pa_edit(PaDev d, const uint4 *info, const uint64_t *woff, const uint8_t *win, uint64_t n,
                                                     uint32_t *out)
{
    __shared__ uint8_t rd[PA_MAX_READ];
    __shared__ uint64_t st[2 * (PA_MAX_READ / 64)];
    const uint64_t R = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t L = in.w;
    if (in.z == 0 || L == 0 || L > PA_MAX_READ) return;
    const uint8_t *P = d.reads + d.roff[R], *W = win + woff[R];
    uint32_t edits, e, back, j;
    pa_pass<false>(P, L, W, in.z, lane, rd, st, edits, e);
    pa_pass<true>(P, L, W, e, lane, rd, st, back, j);
    if (lane == 0) {
        out[n + R] = edits;
        out[2 * n + R] = in.y + e - j;
        out[3 * n + R] = in.y + e;
    }
}

// ---- alignment path (fbg_pindex_chains_cigar) -----------------------------------------------------------------------
// With P' and T' the reversed read and the reversed T = G_r[t_start : t_end), D'(a, b) = lev(P'[:a], T'[:b]) is
// E(L - a, N - b) of the definition, and the second pass of k_pa_edit over exactly the N columns of T' computes it.  The
// history holds, for b = 1 .. N and every word w of the read, pv and mv after column b at hist[((b - 1) * nw + w) * 2]:
// bit a - 1 of the pair is D'(a, b) - D'(a - 1, b).  Column 0 is D'(a, 0) = a and is not stored.

// One lane per read of the last align call (and one for the entry n): units of 8 bytes of history in device memory
// (reads of more than PA_REG_WORDS words) and run slots.  ctr as PG_CTR says, summed per wave before the atomic.
__global__ void k_pg_sizes(const uint4 *info, const uint32_t *out, uint64_t n, uint64_t *hsz, uint64_t *ssz, unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;                // 0 .. 3: 1 .. 4 words, 4: more
    unsigned long long cols = 0;
    if (R <= n) {
        uint64_t h = 0, s = 0;
        if (R < n && out[n + R] != PA_NONE && info[R].w != 0) {
            const uint32_t nw = (info[R].w + 63) / 64;
            cols = out[3 * n + R] - out[2 * n + R];
            tier = nw <= PA_REG_WORDS ? (int)nw - 1 : PA_REG_WORDS;
            if (tier == PA_REG_WORDS) h = 2ull * nw * cols;
            s = 2ull * out[n + R] + 1;
        }
        hsz[R] = h;
        ssz[R] = s;
    }
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    for (int b = 0; b <= PA_REG_WORDS; b++) {
        const unsigned long long mk = __ballot(tier == b);
        if (!mk) continue;                                   // the same in every lane of the wave
        unsigned long long widest = tier == b ? cols : 0;
        for (int off = FBG_WAVE / 2; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(widest, off);
            widest = o > widest ? o : widest;
        }
        if (first) {
            atomicAdd(&ctr[1], (unsigned long long)__popcll(mk));
            atomicAdd(&ctr[3 + b], (unsigned long long)__popcll(mk));
            atomicMax(&ctr[8 + b], widest);
        }
    }
    for (int off = FBG_WAVE / 2; off > 0; off >>= 1) cols += __shfl_xor(cols, off);
    if (cols && first) atomicAdd(&ctr[2], cols);
}

// D'(a, b) from the first row D'(0, b) = b and the column's words: lane w sums the bits of word w below row a, and the
// wave adds the lanes up.  The same value in every lane.
__device__ __forceinline__ int pg_cell(const uint64_t *hist, uint32_t nw, uint32_t a, uint32_t b, unsigned lane)
{
    if (b == 0) return (int)a;
    int part = 0;
    if (lane < nw && lane * 64 < a) {
        const uint64_t *col = hist + ((uint64_t)(b - 1) * nw + lane) * 2;
        const uint32_t rows = a - lane * 64;
        const uint64_t mask = rows >= 64 ? ~0ull : (1ull << rows) - 1;
        part = __popcll(col[0] & mask) - __popcll(col[1] & mask);
    }
    for (int off = FBG_WAVE / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
    return (int)b + part;
}

// D'(a, b) - D'(a - 1, b) for a >= 1
__device__ __forceinline__ int pg_vert(const uint64_t *hist, uint32_t nw, uint32_t a, uint32_t b)
{
    if (b == 0) return 1;
    const uint64_t *col = hist + ((uint64_t)(b - 1) * nw + ((a - 1) >> 6)) * 2;
    const uint64_t bit = 1ull << ((a - 1) & 63);
    return (col[0] & bit) ? 1 : (col[1] & bit) ? -1 : 0;
}

// A wave per read first + blockIdx.x.  NW = 1 .. 4: the reads of exactly NW words, the history in the launch's dynamic
// LDS of cap columns; NW = 0: the reads of more words, the history at scratch + (hoff[R] - hbase) units.  After the
// pass the wave walks from (L, N) to (0, 0), every lane the same walk, and lane 0 writes the runs to slots + soff[R]
// (2 * edits + 1 of them) and their number to cnt[R] and nops[R], which the host cleared.  The walk takes at most L + N
// steps; one that has not arrived by then, or finds a cell that no move explains, or more runs than slots, leaves zero
// runs and adds to ctr[0].
template <int NW>
__global__ __launch_bounds__(FBG_WAVE) void k_pg_path(PaDev d, const uint4 *info, const uint64_t *woff, const uint8_t *win, const uint32_t *out,
                                                     uint64_t n, uint64_t first, uint32_t cap, const uint64_t *hoff, uint64_t hbase,
                                                     uint64_t *scratch, const uint64_t *soff, uint32_t *slots, uint64_t *cnt, uint32_t *nops,
                                                     unsigned long long *ctr)
{
    extern __shared__ uint64_t pg_lds[];
    __shared__ uint8_t rd[NW ? 8 : PA_MAX_READ];
    __shared__ uint64_t st[NW ? 1 : 2 * (PA_MAX_READ / 64)];
    const uint64_t R = first + blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint32_t edits = out[n + R];
    const uint4 in = info[R];
    const uint32_t L = in.w, nw = (L + 63) / 64;
    if (edits == PA_NONE || L == 0 || L > PA_MAX_READ || (NW ? nw != NW : nw <= PA_REG_WORDS)) return;
    const uint32_t ts = out[2 * n + R], N = out[3 * n + R] - ts;
    if (NW && N > cap) {          // the launch's LDS holds cap columns: the host sized it by the widest T of the tier
        if (lane == 0) atomicAdd(&ctr[0], 1ull);
        return;
    }
    const uint8_t *P = d.reads + d.roff[R], *T = win + woff[R] + (ts - in.y);
    uint64_t *hist = NW ? pg_lds : scratch + (hoff[R] - hbase);
    uint32_t best, bestj;
    if constexpr (NW != 0) pa_pass_reg<NW, true, true>(P, L, T, N, lane, best, bestj, hist);
    else pa_pass_lds<true, true>(P, L, nw, T, N, lane, rd, st, best, bestj, hist);
    __syncthreads();              // the history was written by lane 0 (by lane w) and is read by every lane
    uint32_t a = L, b = N, runs = 0, code = 0, len = 0;
    int cur = pg_cell(hist, nw, a, b, lane), left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
    bool bad = cur != (int)edits;
    uint32_t *slot = slots + soff[R];
    for (uint32_t step = 0; step < L + N && (a | b) != 0 && !bad; step++) {
        uint32_t op;
        if (a && b) {
            const int diag = left - pg_vert(hist, nw, a, b - 1);
            const bool eq = P[L - a] == T[N - b];
            if (cur == diag + (eq ? 0 : 1)) {
                op = eq ? 7 : 8;
                a--, b--;
                cur = diag;
                left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
            } else if (pg_vert(hist, nw, a, b) == 1) {
                op = 1;
                a--;
                cur--;
                left = diag;
            } else {
                op = 2;
                bad = cur != left + 1;
                b--;
                cur = left;
                left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
            }
        } else if (a) {           // the text is used up: D'(a, 0) = a
            op = 1;
            a--;
            cur--;
        } else {                  // the read is used up: D'(0, b) = b
            op = 2;
            b--;
            cur--;
        }
        if (op == code) { len++; continue; }
        if (len) {
            if (runs > 2 * edits) bad = true;
            else if (lane == 0) slot[runs] = len << 4 | code;
            runs++;
        }
        code = op;
        len = 1;
    }
    if (len && !bad) {
        if (runs > 2 * edits) bad = true;
        else if (lane == 0) slot[runs] = len << 4 | code;
        runs++;
    }
    if ((a | b) != 0 || cur != 0) bad = true;
    if (lane == 0) {
        if (bad) atomicAdd(&ctr[0], 1ull);
        else { cnt[R] = runs; nops[R] = runs; }
    }
}

// One lane per read copies its runs from their slots to ops + off[R]
__global__ void k_pg_compact(const uint64_t *soff, const uint32_t *slots, const uint64_t *off, uint64_t n, uint32_t *ops)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R >= n) return;
    const uint64_t o = off[R], k = off[R + 1] - o, s = soff[R];
    for (uint64_t x = 0; x < k; x++) ops[o + x] = slots[s + x];
}

// ---- C ABI ------------------------------------------------------------------------------------------------------
extern "C" int fbg_pindex_build(fbg_ctx *ctx, const uint8_t *labels, const uint64_t *label_off, uint64_t n_nodes,
                                const uint64_t *edge_off, const uint64_t *edge_dst, fbg_pindex **out)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!out || (n_nodes && (!label_off || !edge_off)) ||
        (n_nodes && label_off[n_nodes] > label_off[0] && !labels) || (n_nodes && edge_off[n_nodes] > edge_off[0] && !edge_dst))
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_build: missing argument");
    *out = nullptr;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    fbg_pindex *ix = new fbg_pindex();
    ix->ctx = ctx;
    int rc = px_build(ix, labels, label_off, n_nodes, edge_off, edge_dst);
    if (rc != FBG_OK) { px_destroy(ix); return rc; }
    ix->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = ix;
    return FBG_OK;
}

enum PxMode { PX_LOCATE, PX_OCC, PX_SEEDS };

// pats / poff of the last seeds call into buffers of the row state, in stream order before whatever overwrites them
static int pr_save_reads(fbg_pindex *ix)
{
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    FBG_TRY(fbg_reserve(ctx, w.reads, w.read_bytes + 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, w.roff, (ix->sd_reads + 1) * 8, &ix->bufs, false));
    if (w.read_bytes) FBG_HIP_TRY(ctx, hipMemcpyAsync(w.reads.p, ix->pats.p, w.read_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(w.roff.p, ix->poff.p, (ix->sd_reads + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    w.saved = true;
    return FBG_OK;
}

// The per-pattern (or per-seed) buffers of a place state, for n of them.
static int po_reserve(fbg_pindex *ix, PoState &s, uint64_t n)
{
    for (DevBuf *b : {&s.etot, &s.stot}) FBG_TRY(fbg_reserve(ix->ctx, *b, n * 8, &ix->bufs, false));
    for (DevBuf *b : {&s.esz, &s.ssz, &s.eoff, &s.soff}) FBG_TRY(fbg_reserve(ix->ctx, *b, (n + 1) * 8, &ix->bufs, false));
    for (DevBuf *b : {&s.rs, &s.el, &s.ss, &s.sk}) FBG_TRY(fbg_reserve(ix->ctx, *b, n * 4, &ix->bufs, false));
    return FBG_OK;
}

// The front of fbg_pindex_locate, fbg_pindex_occurrences and fbg_pindex_seeds: checks, every allocation of the call
// that depends on n only (after hipSetDevice), patterns onto the device, ev0, and the pattern ids sorted by length into
// oval2.  n > 0.  comp (PX_SEEDS only; NULL: the reads as given): the complement table of fbg_pindex_seeds_strands.
// Everything is then reserved for 2n reads and twice the bytes, k_px_revcomp appends the reverse virtual reads after
// ev0, and the sort runs over the 2n.
static int px_front(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns, PxMode mode,
                    const uint8_t *comp = nullptr)
{
    fbg_ctx *ctx = ix->ctx;
    for (uint64_t k = 0; k < n_patterns; k++)
        if (pat_off[k + 1] < pat_off[k]) return fbg_fail(ctx, FBG_ERR_INVALID, "pattern offsets decrease at pattern %llu", (unsigned long long)k);
    if (mode == PX_SEEDS)
        for (uint64_t k = 0; k < n_patterns; k++)
            if (pat_off[k + 1] - pat_off[k] >= (1ull << 32))
                return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: pattern %llu has 2^32 symbols or more", who, (unsigned long long)k);
    const uint64_t base = pat_off[0], total = pat_off[n_patterns] - base;
    if (total && !patterns) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing patterns", who);
    if (comp && total > (0xffffffffffffffffull - 64) / 2)
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: the patterns and their reverse complements hold 2^64 bytes or more", who);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = comp ? 2 * n_patterns : n_patterns;     // reads on the device
    const uint64_t pbytes = comp ? 2 * total : total;
    // an index with the row table: fbg_pindex_seeds_rows / _chains_rows read the reads of the last seeds call, which a
    // locate or occurrences call is about to overwrite
    if (mode == PX_SEEDS) { ix->rw.saved = false; ix->rw.read_bytes = pbytes; }
    else if (ix->has_rows && ix->sd.ready && ix->sd_reads && !ix->rw.saved) FBG_TRY(pr_save_reads(ix));
    FBG_TRY(fbg_reserve(ix->ctx, ix->pats, ((pbytes + 7) & ~7ull) + 16, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->poff, (n + 1) * 8, &ix->bufs, false));
    for (DevBuf *b : {&ix->okey, &ix->oval, &ix->okey2, &ix->oval2}) FBG_TRY(fbg_reserve(ix->ctx, *b, n * 4, &ix->bufs, false));
    if (mode == PX_SEEDS) {
        for (DevBuf *b : {&ix->snum, &ix->soff}) FBG_TRY(fbg_reserve(ix->ctx, *b, (n + 1) * 8, &ix->bufs, false));
    } else {
        FBG_TRY(fbg_reserve(ix->ctx, ix->cnt_out, n * 8, &ix->bufs, false));
        FBG_TRY(fbg_reserve(ix->ctx, ix->pos_out, n * 8, &ix->bufs, false));
        FBG_TRY(fbg_reserve(ix->ctx, ix->lines_ctr, 8, &ix->bufs, false));
    }
    if (mode == PX_OCC) {
        FBG_TRY(fbg_reserve(ix->ctx, ix->orec, n * 24, &ix->bufs, false));
        FBG_TRY(po_reserve(ix, ix->occ, n));
    }
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    if (comp) FBG_TRY(fbg_reserve(ix->ctx, ix->comp, 256, &ix->bufs, false));
    if (total) FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->pats.p, patterns + base, total, hipMemcpyHostToDevice, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->poff.p, pat_off, (n_patterns + 1) * 8, hipMemcpyHostToDevice, st));
    if (comp) FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->comp.p, comp, 256, hipMemcpyHostToDevice, st));
    if (mode != PX_SEEDS) FBG_HIP_TRY(ctx, hipMemsetAsync(ix->lines_ctr.p, 0, 8, st));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    uint64_t *poff = ix->poff.as<uint64_t>();
    if (base) hipLaunchKernelGGL(k_px_rebase, dim3(fbg_blocks(n_patterns + 1, 256)), dim3(256), 0, st, poff, n_patterns, base);
    if (comp) {
        const uint64_t words = (2 * total + 7) / 8 - total / 8;
        hipLaunchKernelGGL(k_px_revcomp, dim3(fbg_blocks(std::max(words, n_patterns), PX_THREADS)), dim3(PX_THREADS), 0, st,
                           ix->comp.as<uint8_t>(), ix->pats.as<uint8_t>(), poff, n_patterns, total);
    }
    // lanes of a wave take patterns of similar length: pattern ids sorted by length
    uint32_t *ka = ix->okey.as<uint32_t>(), *va = ix->oval.as<uint32_t>(), *kb = ix->okey2.as<uint32_t>(), *vb = ix->oval2.as<uint32_t>();
    hipLaunchKernelGGL(k_px_lenkey, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, poff, n, ka, va);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, va, vb, (size_t)n, 0u, 32u, st);
    }));
    return FBG_OK;
}

// px_front and the walk (occ: the instantiation that records the ranges into orec).  n > 0.
static int px_search(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns, bool occ)
{
    fbg_ctx *ctx = ix->ctx;
    FBG_TRY(px_front(ix, who, patterns, pat_off, n_patterns, occ ? PX_OCC : PX_LOCATE));
    hipStream_t st = ctx->stream;
    const uint64_t n = n_patterns;
    uint64_t *poff = ix->poff.as<uint64_t>();
    uint32_t *vb = ix->oval2.as<uint32_t>();
    PxDev d = px_dev(ix);
    const dim3 g(fbg_blocks(n, PX_THREADS));
    auto *co = ix->cnt_out.as<unsigned long long>(), *po = ix->pos_out.as<unsigned long long>();
    auto *lc = ix->lines_ctr.as<unsigned long long>();
    if (occ && ix->compact)
        hipLaunchKernelGGL((k_px_walk<true, true, true>), g, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                           ix->pats.as<uint8_t>(), poff, vb, n, co, po, (uint8_t *)nullptr, (uint8_t *)nullptr, lc, ix->orec.as<uint2>());
    else if (occ)
        hipLaunchKernelGGL((k_px_walk<true, false, true>), g, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                           ix->pats.as<uint8_t>(), poff, vb, n, co, po, (uint8_t *)nullptr, (uint8_t *)nullptr, lc, ix->orec.as<uint2>());
    else if (ix->compact)
        hipLaunchKernelGGL((k_px_walk<true, true>), g, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                           ix->pats.as<uint8_t>(), poff, vb, n, co, po, (uint8_t *)nullptr, (uint8_t *)nullptr, lc, (uint2 *)nullptr);
    else
        hipLaunchKernelGGL((k_px_walk<true, false>), g, dim3(PX_THREADS), 0, st, d, ix->code.as<uint16_t>(), ix->C.as<uint32_t>(),
                           ix->pats.as<uint8_t>(), poff, vb, n, co, po, (uint8_t *)nullptr, (uint8_t *)nullptr, lc, (uint2 *)nullptr);
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

extern "C" int fbg_pindex_locate(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                 uint64_t *count, uint64_t *pos)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    if (n_patterns && (!pat_off || !count || !pos)) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_locate: missing argument");
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_locate: at most 2^32 - 2 patterns per call");
    ix->search_ms = 0;
    ix->occ_lines = 0;
    if (n_patterns == 0) return FBG_OK;
    FBG_TRY(px_search(ix, "fbg_pindex_locate", patterns, pat_off, n_patterns, false));
    hipStream_t st = ctx->stream;
    const uint64_t n = n_patterns;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(count, ix->cnt_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(pos, ix->pos_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&ix->occ_lines, ix->lines_ctr.p, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    ix->search_ms = ms;
    return FBG_OK;
}

// The tables of the validation and of the occurrence expansion.  block is the scratch of fbg_pindex_validate (NULL
// before its first call): k_po_expand reads sa, estart, esrc, edst and ctab only.
static PvDev pv_dev(const fbg_pindex *ix)
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

// k_po_sizes over n > 0 items (count, pos and rec on the device; s reserved for n) and the scans of the capped sizes
// into the CSR offsets s.eoff / s.soff.  Shared by the occurrence and the seed calls.
static int po_sizes(fbg_pindex *ix, PoState &s, const DevBuf &count, const DevBuf &pos, const DevBuf &rec, uint64_t n, uint64_t cap)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    uint64_t *esz = s.esz.as<uint64_t>(), *ssz = s.ssz.as<uint64_t>(), *eoff = s.eoff.as<uint64_t>(), *soff = s.soff.as<uint64_t>();
    hipLaunchKernelGGL(k_po_sizes, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, count.as<unsigned long long>(),
                       pos.as<unsigned long long>(), (const uint2 *)rec.as<uint2>(), n, cap, ix->n_edges != 0,
                       s.etot.as<uint64_t>(), s.stot.as<uint64_t>(), esz, ssz, s.rs.as<uint32_t>(), s.el.as<uint32_t>(),
                       s.ss.as<uint32_t>(), s.sk.as<uint32_t>());
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, esz, eoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, ssz, soff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

// The places of a place state into the caller's arrays (fbg_pindex_occurrences_fetch, fbg_pindex_seeds_places).
static int po_fetch(fbg_pindex *ix, const char *who, const char *search, PoState &s, uint32_t *end_src, uint32_t *end_dst,
                    uint32_t *end_offset, uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms)
{
    fbg_ctx *ctx = ix->ctx;
    if (device_ms) *device_ms = 0;
    if (!s.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: no %s result to fetch", who, search);
    const bool ends = end_src && end_dst && end_offset, starts = start_src && start_dst && start_offset;
    if ((!ends && (end_src || end_dst || end_offset)) || (!starts && (start_src || start_dst || start_offset)))
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: a list takes all three of its arrays or none", who);
    const uint64_t ne = ends ? s.etotal : 0, ns = starts ? s.stotal : 0, n = s.n;
    if (ne + ns == 0) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ix->ctx, s.place, 3 * (ne + ns) * 4, &ix->bufs, false));
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    // place: src, dst, offset of the ends, then of the starts
    uint32_t *pe = s.place.as<uint32_t>(), *ps = pe + 3 * ne;
    const PvDev d = pv_dev(ix);
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (ne)
        hipLaunchKernelGGL(k_po_expand<false>, dim3(fbg_blocks(ne, PX_THREADS)), dim3(PX_THREADS), 0, st, d, (const uint64_t *)s.eoff.as<uint64_t>(),
                           n, ne, (const uint32_t *)s.el.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                           (const uint32_t *)s.rs.as<uint32_t>(), pe, pe + ne, pe + 2 * ne);
    if (ns)
        hipLaunchKernelGGL(k_po_expand<true>, dim3(fbg_blocks(ns, PX_THREADS)), dim3(PX_THREADS), 0, st, d, (const uint64_t *)s.soff.as<uint64_t>(),
                           n, ns, (const uint32_t *)s.ss.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                           (const uint32_t *)s.rs.as<uint32_t>(), ps, ps + ns, ps + 2 * ns);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    if (ne) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(end_src, pe, ne * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(end_dst, pe + ne, ne * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(end_offset, pe + 2 * ne, ne * 4, hipMemcpyDeviceToHost, st));
    }
    if (ns) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(start_src, ps, ns * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(start_dst, ps + ns, ns * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(start_offset, ps + 2 * ns, ns * 4, hipMemcpyDeviceToHost, st));
    }
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    return FBG_OK;
}

// k_po_expand_msa over one list of a place state (STARTS: its starts, else its ends; the list is not empty) into orow /
// ocol on the device, on the context's stream.
template <bool STARTS> static void po_expand_msa(fbg_pindex *ix, const PoState &s, uint32_t *orow, uint32_t *ocol)
{
    const PvDev d = pv_dev(ix);
    const PmDev m = {ix->mnode.as<uint4>(), ix->mbits.as<uint64_t>()};
    const uint64_t total = STARTS ? s.stotal : s.etotal;
    hipLaunchKernelGGL(k_po_expand_msa<STARTS>, dim3(fbg_blocks(total, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, d, m,
                       (const uint64_t *)(STARTS ? s.soff : s.eoff).as<uint64_t>(), s.n, total,
                       (const uint32_t *)(STARTS ? s.ss : s.el).as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(),
                       (const uint32_t *)s.rs.as<uint32_t>(), orow, ocol);
}

// The MSA coordinates of a place state's places into the caller's arrays (fbg_pindex_occurrences_msa, fbg_pindex_seeds_msa):
// po_fetch with k_po_expand_msa and a buffer of its own, so that neither s.place nor a later fetch sees it.
static int po_fetch_msa(fbg_pindex *ix, const char *who, const char *search, PoState &s, uint32_t *end_row, uint32_t *end_col,
                        uint32_t *start_row, uint32_t *start_col, double *device_ms)
{
    fbg_ctx *ctx = ix->ctx;
    if (device_ms) *device_ms = 0;
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation knows MSA coordinates", who);
    if (!s.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: no %s result to expand", who, search);
    const bool ends = end_row && end_col, starts = start_row && start_col;
    if ((!ends && (end_row || end_col)) || (!starts && (start_row || start_col)))
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: a list takes both of its arrays or none", who);
    const uint64_t ne = ends ? s.etotal : 0, ns = starts ? s.stotal : 0;
    if (ne + ns == 0) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ix->ctx, s.msa, 2 * (ne + ns) * 4, &ix->bufs, false));
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    // msa: row, column of the ends, then of the starts
    uint32_t *pe = s.msa.as<uint32_t>(), *ps = pe + 2 * ne;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (ne) po_expand_msa<false>(ix, s, pe, pe + ne);
    if (ns) po_expand_msa<true>(ix, s, ps, ps + ns);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    if (ne) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(end_row, pe, ne * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(end_col, pe + ne, ne * 4, hipMemcpyDeviceToHost, st));
    }
    if (ns) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(start_row, ps, ns * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(start_col, ps + ns, ns * 4, hipMemcpyDeviceToHost, st));
    }
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    return FBG_OK;
}

extern "C" int fbg_pindex_occurrences(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                      uint64_t max_per_pattern, uint64_t *count, uint64_t *pos, uint32_t *restarts,
                                      uint64_t *end_off, uint64_t *start_off, uint64_t *end_total, uint64_t *start_total,
                                      double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->occ;
    s.ready = false;
    if (device_ms) *device_ms = 0;
    if (!end_off || !start_off || (n_patterns && (!pat_off || !count || !pos || !restarts || !end_total || !start_total)))
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_occurrences: missing argument");
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_occurrences: at most 2^32 - 2 patterns per call");
    end_off[0] = start_off[0] = 0;
    s.n = n_patterns;
    s.etotal = s.stotal = 0;
    if (n_patterns == 0) { s.ready = true; return FBG_OK; }
    const uint64_t n = n_patterns;
    FBG_TRY(px_search(ix, "fbg_pindex_occurrences", patterns, pat_off, n, true));
    hipStream_t st = ctx->stream;
    FBG_TRY(po_sizes(ix, s, ix->cnt_out, ix->pos_out, ix->orec, n, max_per_pattern));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(count, ix->cnt_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(pos, ix->pos_out.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(restarts, s.rs.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(end_total, s.etot.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(start_total, s.stot.p, n * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(end_off, s.eoff.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(start_off, s.soff.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    if (end_off[n] >= (1ull << 32) || start_off[n] >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_occurrences: %llu ends and %llu starts to report; a list takes fewer than 2^32 "
                        "entries (lower max_per_pattern or split the batch)", (unsigned long long)end_off[n], (unsigned long long)start_off[n]);
    s.etotal = end_off[n];
    s.stotal = start_off[n];
    s.ready = true;
    return FBG_OK;
}

extern "C" int fbg_pindex_occurrences_fetch(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                                            uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_occurrences_fetch", "fbg_pindex_occurrences", ix->occ, end_src, end_dst, end_offset, start_src,
                    start_dst, start_offset, device_ms);
}

extern "C" int fbg_pindex_occurrences_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row,
                                          uint32_t *start_col, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch_msa(ix, "fbg_pindex_occurrences_msa", "fbg_pindex_occurrences", ix->occ, end_row, end_col, start_row, start_col,
                        device_ms);
}

// ---- seeds (fbg_pindex_seeds / _fetch / _places) -------------------------------------------------------------------
// Count, then write: k_px_seeds<*, false> counts the reported seeds of every read, an exclusive scan places them (reads
// in input order, a read's seeds contiguous and by q_start), the host learns the total and sizes the per-seed buffers,
// k_px_seeds<*, true> walks again and writes.  From there the seeds are the patterns of po_sizes / po_fetch.
template <bool COMPACT, bool WRITE> static void px_seeds_launch(fbg_pindex *ix, const PxDev &d, uint64_t n, uint32_t min_len)
{
    hipLaunchKernelGGL((k_px_seeds<COMPACT, WRITE>), dim3(fbg_blocks(n, PX_THREADS)), dim3(PX_THREADS), 0, ix->ctx->stream, d,
                       ix->code.as<uint16_t>(), ix->C.as<uint32_t>(), ix->pats.as<uint8_t>(), ix->poff.as<uint64_t>(),
                       ix->oval2.as<uint32_t>(), n, min_len, (WRITE ? ix->soff : ix->snum).as<uint64_t>(),
                       ix->scnt.as<unsigned long long>(), ix->spos.as<unsigned long long>(), ix->srec.as<uint2>(),
                       ix->sq.as<uint32_t>(), ix->slen.as<uint32_t>());
}

// The body of fbg_pindex_seeds (comp == NULL) and fbg_pindex_seeds_strands (comp: the 256-byte table; the device then
// searches the 2 * n_patterns virtual reads and seed_off has that many entries and one).
static int px_seeds(fbg_pindex *ix, const char *who, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                    const uint8_t *comp, uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off, double *device_ms)
{
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->sd;
    s.ready = false;
    ix->ch.ready = false;         // chains belong to the seeds they were made from
    ix->al.valid = ix->cg.ready = false;
    if (device_ms) *device_ms = 0;
    if (!seed_off || (n_patterns && !pat_off)) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing argument", who);
    if (min_length == 0) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: min_length is 1 or more", who);
    if (n_patterns >= 0xffffffffull) return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: at most 2^32 - 2 patterns per call", who);
    if (comp && 2 * n_patterns >= 0xffffffffull)
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: at most 2^31 - 1 patterns per call (both strands: 2^32 - 2 reads)", who);
    seed_off[0] = 0;
    s.n = 0;
    s.etotal = s.stotal = 0;
    const uint64_t n = comp ? 2 * n_patterns : n_patterns;
    ix->sd_reads = n;
    ix->sd_stranded = comp != nullptr;
    if (n == 0) { s.ready = true; return FBG_OK; }
    FBG_TRY(px_front(ix, who, patterns, pat_off, n_patterns, PX_SEEDS, comp));
    hipStream_t st = ctx->stream;
    const bool none = min_length >= (1ull << 32);   // no pattern has 2^32 symbols: nothing can be reported
    const uint32_t L = none ? 0xffffffffu : (uint32_t)min_length;
    const PxDev d = px_dev(ix);
    uint64_t *num = ix->snum.as<uint64_t>(), *soff = ix->soff.as<uint64_t>();
    auto walk = [&](bool write) {
        if (ix->compact) { if (write) px_seeds_launch<true, true>(ix, d, n, L); else px_seeds_launch<true, false>(ix, d, n, L); }
        else { if (write) px_seeds_launch<false, true>(ix, d, n, L); else px_seeds_launch<false, false>(ix, d, n, L); }
    };
    if (none) {
        std::fill(seed_off, seed_off + n + 1, (uint64_t)0);
    } else {
        FBG_HIP_TRY(ctx, hipMemsetAsync(num + n, 0, 8, st));
        walk(false);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, num, soff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
        }));
        FBG_HIP_TRY(ctx, hipGetLastError());
        FBG_HIP_TRY(ctx, hipMemcpyAsync(seed_off, soff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const uint64_t S = seed_off[n];
    if (S >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu seeds to report; a call takes fewer than 2^32 (raise min_length or "
                        "split the batch)", who, (unsigned long long)S);
    uint64_t tot[2] = {0, 0};
    if (S) {
        FBG_TRY(fbg_reserve(ix->ctx, ix->srec, S * 24, &ix->bufs, false));
        for (DevBuf *b : {&ix->scnt, &ix->spos}) FBG_TRY(fbg_reserve(ix->ctx, *b, S * 8, &ix->bufs, false));
        for (DevBuf *b : {&ix->sq, &ix->slen}) FBG_TRY(fbg_reserve(ix->ctx, *b, S * 4, &ix->bufs, false));
        FBG_TRY(po_reserve(ix, s, S));
        walk(true);
        FBG_TRY(po_sizes(ix, s, ix->scnt, ix->spos, ix->srec, S, max_per_seed));
    }
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    if (S) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&tot[0], s.eoff.as<uint64_t>() + S, 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&tot[1], s.soff.as<uint64_t>() + S, 8, hipMemcpyDeviceToHost, st));
    }
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    if (tot[0] >= (1ull << 32) || tot[1] >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu ends and %llu starts to report; a list takes fewer than 2^32 "
                        "entries (lower max_per_seed or split the batch)", who, (unsigned long long)tot[0], (unsigned long long)tot[1]);
    s.n = S;
    s.etotal = tot[0];
    s.stotal = tot[1];
    s.ready = true;
    return FBG_OK;
}

extern "C" int fbg_pindex_seeds(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return px_seeds(ix, "fbg_pindex_seeds", patterns, pat_off, n_patterns, nullptr, min_length, max_per_seed, seed_off, device_ms);
}

extern "C" int fbg_pindex_seeds_strands(fbg_pindex *ix, const uint8_t *patterns, const uint64_t *pat_off, uint64_t n_patterns,
                                        const uint8_t *complement, uint64_t min_length, uint64_t max_per_seed, uint64_t *seed_off,
                                        double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    uint8_t table[256];
    if (!complement) {
        for (int c = 0; c < 256; c++) table[c] = (uint8_t)c;
        const char *pairs = "ATCGatcg";
        for (int k = 0; k < 8; k += 2) { table[(uint8_t)pairs[k]] = pairs[k + 1]; table[(uint8_t)pairs[k + 1]] = pairs[k]; }
        complement = table;
    }
    return px_seeds(ix, "fbg_pindex_seeds_strands", patterns, pat_off, n_patterns, complement, min_length, max_per_seed, seed_off,
                    device_ms);
}

extern "C" int fbg_pindex_seeds_fetch(fbg_pindex *ix, uint32_t *q_start, uint32_t *length, uint64_t *count, uint32_t *restarts,
                                      uint64_t *end_total, uint64_t *start_total, uint64_t *end_off, uint64_t *start_off,
                                      double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    if (!s.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_seeds_fetch: no fbg_pindex_seeds result to fetch");
    const uint64_t S = s.n;
    if (S == 0) {
        if (end_off) end_off[0] = 0;
        if (start_off) start_off[0] = 0;
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    auto get = [&](void *dst, const DevBuf &src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    FBG_HIP_TRY(ctx, get(q_start, ix->sq, S * 4));
    FBG_HIP_TRY(ctx, get(length, ix->slen, S * 4));
    FBG_HIP_TRY(ctx, get(count, ix->scnt, S * 8));
    FBG_HIP_TRY(ctx, get(restarts, s.rs, S * 4));
    FBG_HIP_TRY(ctx, get(end_total, s.etot, S * 8));
    FBG_HIP_TRY(ctx, get(start_total, s.stot, S * 8));
    FBG_HIP_TRY(ctx, get(end_off, s.eoff, (S + 1) * 8));
    FBG_HIP_TRY(ctx, get(start_off, s.soff, (S + 1) * 8));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    return FBG_OK;
}

extern "C" int fbg_pindex_seeds_places(fbg_pindex *ix, uint32_t *end_src, uint32_t *end_dst, uint32_t *end_offset,
                                       uint32_t *start_src, uint32_t *start_dst, uint32_t *start_offset, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch(ix, "fbg_pindex_seeds_places", "fbg_pindex_seeds", ix->sd, end_src, end_dst, end_offset, start_src, start_dst,
                    start_offset, device_ms);
}

extern "C" int fbg_pindex_seeds_msa(fbg_pindex *ix, uint32_t *end_row, uint32_t *end_col, uint32_t *start_row, uint32_t *start_col,
                                    double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    return po_fetch_msa(ix, "fbg_pindex_seeds_msa", "fbg_pindex_seeds", ix->sd, end_row, end_col, start_row, start_col, device_ms);
}

// ---- chains (fbg_pindex_chains / _fetch / _stats) -----------------------------------------------------------------
// The start columns of the seeds' places (k_po_expand_msa<true> into the chain state's own buffer), the reads sorted by
// their number of start places, the host's look at the four bin sizes, one k_pc_chain launch per tier that has reads,
// then count, scan and write as the seeds do.  A chain has at most one anchor per seed: S entries hold every chain.
extern "C" int fbg_pindex_chains(fbg_pindex *ix, uint64_t band, uint64_t min_score, uint64_t *chain_off, uint32_t *score,
                                 double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PcState &c = ix->ch;
    const PoState &s = ix->sd;
    c.ready = false;
    ix->al.valid = ix->cg.ready = false;      // the alignment and its paths belong to the chains
    if (device_ms) *device_ms = 0;
    if (!chain_off) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains: missing chain_off");
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains: only an index built by fbg_pindex_build_segmentation knows MSA columns");
    if (!s.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains: no fbg_pindex_seeds result to chain");
    const uint64_t n = ix->sd_reads, S = s.n, A = s.stotal;
    c.n = n;
    c.total = c.anchors = 0;
    c.tier[0] = c.tier[1] = c.tier[2] = 0;
    std::fill(chain_off, chain_off + n + 1, (uint64_t)0);
    if (score) std::fill(score, score + n, (uint32_t)0);
    if (n == 0 || S == 0 || A == 0) { c.ready = true; return FBG_OK; }   // no start place: every score 0, every chain empty
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ix->ctx, c.col, 2 * A * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, c.pred, A * 4, &ix->bufs, false));
    for (DevBuf *b : {&c.key, &c.id, &c.key2, &c.id2, &c.end, &c.score}) FBG_TRY(fbg_reserve(ix->ctx, *b, n * 4, &ix->bufs, false));
    for (DevBuf *b : {&c.len, &c.off}) FBG_TRY(fbg_reserve(ix->ctx, *b, (n + 1) * 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, c.out, 2 * S * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, c.ctr, 5 * 8, &ix->bufs, false));
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    PcDev d;
    d.seed_off = ix->soff.as<uint64_t>();
    d.start_off = s.soff.as<uint64_t>();
    d.q = ix->sq.as<uint32_t>();
    d.k = ix->slen.as<uint32_t>();
    d.col = c.col.as<uint32_t>() + A;
    d.pred = c.pred.as<uint32_t>();
    d.end = c.end.as<uint32_t>();
    d.score = c.score.as<uint32_t>();
    d.slab = nullptr;
    d.ctr = c.ctr.as<unsigned long long>();
    d.band = band;
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(c.ctr.p, 0, 5 * 8, st));
    po_expand_msa<true>(ix, s, c.col.as<uint32_t>(), c.col.as<uint32_t>() + A);
    uint32_t *ka = c.key.as<uint32_t>(), *va = c.id.as<uint32_t>(), *kb = c.key2.as<uint32_t>(), *vb = c.id2.as<uint32_t>();
    hipLaunchKernelGGL(k_pc_key, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d, n, ka, va);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, va, vb, (size_t)n, 0u, 32u, st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t bin[5] = {0, 0, 0, 0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(bin, c.ctr.p, 4 * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bin[0] + bin[1] + bin[2] + bin[3] != n) return fbg_fail(ctx, FBG_ERR_HIP, "fbg_pindex_chains: the tiers hold %llu of %llu reads",
                                                                (unsigned long long)(bin[0] + bin[1] + bin[2] + bin[3]), (unsigned long long)n);
    if (bin[3]) {
        FBG_TRY(fbg_reserve(ix->ctx, c.slab, A * 16, &ix->bufs, false));
        d.slab = c.slab.as<uint4>();
    }
    const uint32_t *ids = vb + bin[0];
    if (bin[1])
        hipLaunchKernelGGL(k_pc_chain<0>, dim3(fbg_blocks(bin[1], PX_THREADS / PC_SUB)), dim3(PX_THREADS), 0, st, d, ids, bin[1]);
    if (bin[2]) hipLaunchKernelGGL(k_pc_chain<1>, dim3((unsigned)bin[2]), dim3(FBG_WAVE), 0, st, d, ids + bin[1], bin[2]);
    if (bin[3]) hipLaunchKernelGGL(k_pc_chain<2>, dim3((unsigned)bin[3]), dim3(FBG_WAVE), 0, st, d, ids + bin[1] + bin[2], bin[3]);
    uint64_t *len = c.len.as<uint64_t>(), *off = c.off.as<uint64_t>();
    uint32_t *out = c.out.as<uint32_t>();
    hipLaunchKernelGGL(k_pc_trace<false>, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, d, n, min_score, len, (const uint64_t *)off, out, out + S);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, len, off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    hipLaunchKernelGGL(k_pc_trace<true>, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, d, n, min_score, len, (const uint64_t *)off, out, out + S);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(chain_off, off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (score) FBG_HIP_TRY(ctx, hipMemcpyAsync(score, c.score.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bin[4], d.ctr + 4, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    // a chain takes one place per seed at most, and a call has fewer than 2^32 seeds
    if (chain_off[n] >= (1ull << 32))
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_chains: %llu chain entries; a call takes fewer than 2^32", (unsigned long long)chain_off[n]);
    c.total = chain_off[n];
    c.anchors = bin[4];
    c.tier[0] = bin[1];
    c.tier[1] = bin[2];
    c.tier[2] = bin[3];
    c.ready = true;
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_fetch(fbg_pindex *ix, uint32_t *anchor_place, uint32_t *anchor_seed, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (!c.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_fetch: no fbg_pindex_chains result to fetch");
    if (c.total == 0 || (!anchor_place && !anchor_seed)) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t *out = c.out.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (anchor_place) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_place, out, c.total * 4, hipMemcpyDeviceToHost, st));
    if (anchor_seed) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_seed, out + ix->sd.n, c.total * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    return FBG_OK;
}

// The strand of every given read from the scores and lengths fbg_pindex_chains left on the device (k_pc_strand).  Where
// that call found no start place at all it returned before touching the device: every read is then without a chain.
extern "C" int fbg_pindex_chain_strands(fbg_pindex *ix, uint8_t *strand, uint32_t *score, uint64_t *n_forward, uint64_t *n_reverse,
                                        uint64_t *n_none, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (!ix->sd.ready || !ix->sd_stranded)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chain_strands: the last seeds call was no successful fbg_pindex_seeds_strands");
    if (!c.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chain_strands: no fbg_pindex_chains result since that seeds call");
    const uint64_t n = ix->sd_reads / 2;
    if (n == 0) return FBG_OK;
    uint64_t cnt[3] = {0, 0, n};
    if (ix->sd.n == 0 || ix->sd.stotal == 0) {
        if (strand) std::fill(strand, strand + n, (uint8_t)FBG_STRAND_NONE);
        if (score) std::fill(score, score + n, (uint32_t)0);
    } else {
        FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        FBG_TRY(fbg_reserve(ix->ctx, c.strand, n, &ix->bufs, false));
        FBG_TRY(fbg_reserve(ix->ctx, c.best, n * 4, &ix->bufs, false));
        FBG_TRY(fbg_reserve(ix->ctx, c.sctr, 3 * 8, &ix->bufs, false));
        FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
        FBG_HIP_TRY(ctx, hipMemsetAsync(c.sctr.p, 0, 3 * 8, st));
        hipLaunchKernelGGL(k_pc_strand, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, c.score.as<uint32_t>(), c.len.as<uint64_t>(), n,
                           c.strand.as<uint8_t>(), c.best.as<uint32_t>(), c.sctr.as<unsigned long long>());
        FBG_HIP_TRY(ctx, hipGetLastError());
        FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
        if (strand) FBG_HIP_TRY(ctx, hipMemcpyAsync(strand, c.strand.p, n, hipMemcpyDeviceToHost, st));
        if (score) FBG_HIP_TRY(ctx, hipMemcpyAsync(score, c.best.p, n * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(cnt, c.sctr.p, 3 * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
        float ms = 0;
        FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
        if (device_ms) *device_ms = ms;
    }
    if (n_forward) *n_forward = cnt[0];
    if (n_reverse) *n_reverse = cnt[1];
    if (n_none) *n_none = cnt[2];
    return FBG_OK;
}

extern "C" int fbg_pindex_chain_stats(const fbg_pindex *ix, uint64_t *anchors, uint64_t *reads_small, uint64_t *reads_wave,
                                      uint64_t *reads_spill, uint64_t *small_max, uint64_t *lds_max)
{
    if (!ix) return FBG_ERR_INVALID;
    const PcState &c = ix->ch;
    if (anchors) *anchors = c.ready ? c.anchors : 0;
    if (reads_small) *reads_small = c.ready ? c.tier[0] : 0;
    if (reads_wave) *reads_wave = c.ready ? c.tier[1] : 0;
    if (reads_spill) *reads_spill = c.ready ? c.tier[2] : 0;
    if (small_max) *small_max = PC_SMALL;
    if (lds_max) *lds_max = PC_LDS;
    return FBG_OK;
}

extern "C" int fbg_pindex_msa_stats(const fbg_pindex *ix, uint64_t *map_bytes, uint64_t *gapped_nodes, uint64_t *sample_columns)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_msa_stats: only an index built by fbg_pindex_build_segmentation has the table");
    if (map_bytes) *map_bytes = 16 * ix->n_nodes + 8 * ix->map_units;
    if (gapped_nodes) *gapped_nodes = ix->map_gapped;
    if (sample_columns) *sample_columns = 64 * PM_W;
    return FBG_OK;
}

// ---- rows (fbg_pindex_seeds_rows / _chains_rows / _rows_stats) -------------------------------------------------------
// What both calls start with, for S > 0 seeds and A > 0 start places of the last seeds call: sbase per seed and rec per
// start place (k_pr_seed, k_pr_place), into buffers of the row state; d: what the row kernels read.
static int pr_prepare(fbg_pindex *ix, PrDev &d)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    PrState &w = ix->rw;
    const PoState &s = ix->sd;
    const uint64_t n = ix->sd_reads, S = s.n, A = s.stotal;
    FBG_TRY(fbg_reserve(ctx, w.sbase, S * 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, w.rec, A * 16, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, w.ctr, 8, &ix->bufs, false));
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(w.ctr.p, 0, 8, st));
    hipLaunchKernelGGL(k_pr_seed, dim3(fbg_blocks(S, 256)), dim3(256), 0, st, (const uint64_t *)ix->soff.as<uint64_t>(),
                       (const uint64_t *)(w.saved ? w.roff : ix->poff).as<uint64_t>(), (const uint32_t *)ix->sq.as<uint32_t>(), n, S,
                       w.sbase.as<uint64_t>());
    hipLaunchKernelGGL(k_pr_place, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, pv_dev(ix),
                       (const uint32_t *)ix->snode_block.as<uint32_t>(), (const uint64_t *)s.soff.as<uint64_t>(), S, A,
                       (const uint32_t *)s.ss.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(), (const uint32_t *)s.rs.as<uint32_t>(),
                       w.rec.as<uint4>());
    d.node_of = w.node_of.as<uint32_t>();
    d.labels = w.labels.as<uint8_t>();
    d.loff = w.loff.as<uint64_t>();
    d.reads = (w.saved ? w.reads : ix->pats).as<uint8_t>();
    d.sbase = w.sbase.as<uint64_t>();
    d.slen = ix->slen.as<uint32_t>();
    d.m = w.m;
    d.nb = ix->seg_nb;
    return FBG_OK;
}

extern "C" int fbg_pindex_seeds_rows(fbg_pindex *ix, uint32_t *n_rows, uint32_t *first_row, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    const PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    if (!ix->has_rows)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_seeds_rows: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    if (!s.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_seeds_rows: no fbg_pindex_seeds result to expand");
    w.places_unsupported = 0;
    const uint64_t A = s.stotal;
    if (A == 0) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ctx, w.out, 2 * A * 4, &ix->bufs, false));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));
    uint32_t *out = w.out.as<uint32_t>();
    auto *ctr = w.ctr.as<unsigned long long>();
    if (w.m <= PR_SUB && !ctx->opt.rows_wave)
        hipLaunchKernelGGL(k_pr_rows<PR_SUB>, dim3(fbg_blocks(A * PR_SUB, PX_THREADS)), dim3(PX_THREADS), 0, st, d,
                           (const uint4 *)w.rec.as<uint4>(), A, out, out + A, ctr);
    else
        hipLaunchKernelGGL(k_pr_rows<FBG_WAVE>, dim3(fbg_blocks(A * FBG_WAVE, PX_THREADS)), dim3(PX_THREADS), 0, st, d,
                           (const uint4 *)w.rec.as<uint4>(), A, out, out + A, ctr);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    unsigned long long none = 0;
    if (n_rows) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_rows, out, A * 4, hipMemcpyDeviceToHost, st));
    if (first_row) FBG_HIP_TRY(ctx, hipMemcpyAsync(first_row, out + A, A * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&none, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    w.places_unsupported = none;
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_rows(fbg_pindex *ix, uint32_t *n_rows, uint32_t *first_row, uint64_t *row_bits, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (!ix->has_rows)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_rows: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    if (!ix->sd.ready || !c.ready)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_rows: no fbg_pindex_chains result since the last seeds call");
    w.chains_unsupported = 0;
    const uint64_t n = c.n, words = (w.m + 63) / 64;
    if (n == 0) return FBG_OK;
    if (c.total == 0) {          // every chain is empty, and fbg_pindex_chains may have left nothing on the device
        if (n_rows) std::fill(n_rows, n_rows + n, (uint32_t)0);
        if (first_row) std::fill(first_row, first_row + n, (uint32_t)PR_NONE);
        if (row_bits) std::fill(row_bits, row_bits + n * words, (uint64_t)0);
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ctx, w.cout, n * words * 8 + 2 * n * 4, &ix->bufs, false));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));
    uint64_t *bits = w.cout.as<uint64_t>();
    uint32_t *out = (uint32_t *)(bits + n * words);
    auto *ctr = w.ctr.as<unsigned long long>();
    const uint4 *rec = w.rec.as<uint4>();
    const uint32_t *place = c.out.as<uint32_t>();
    const uint64_t *off = c.off.as<uint64_t>();
    if (w.m <= PR_SUB && !ctx->opt.rows_wave)
        hipLaunchKernelGGL(k_pr_chain<PR_SUB>, dim3(fbg_blocks(n * PR_SUB, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n, words,
                           out, out + n, row_bits ? bits : (uint64_t *)nullptr, ctr);
    else
        hipLaunchKernelGGL(k_pr_chain<FBG_WAVE>, dim3(fbg_blocks(n * FBG_WAVE, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n,
                           words, out, out + n, row_bits ? bits : (uint64_t *)nullptr, ctr);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    unsigned long long none = 0;
    if (n_rows) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_rows, out, n * 4, hipMemcpyDeviceToHost, st));
    if (first_row) FBG_HIP_TRY(ctx, hipMemcpyAsync(first_row, out + n, n * 4, hipMemcpyDeviceToHost, st));
    if (row_bits) FBG_HIP_TRY(ctx, hipMemcpyAsync(row_bits, bits, n * words * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&none, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    w.chains_unsupported = none;
    return FBG_OK;
}

extern "C" int fbg_pindex_rows_stats(const fbg_pindex *ix, uint64_t *rows, uint64_t *table_bytes, uint64_t *words_per_set,
                                     uint64_t *places_unsupported, uint64_t *chains_unsupported)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_rows_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    const PrState &w = ix->rw;
    if (rows) *rows = w.m;
    if (table_bytes) *table_bytes = 4 * w.m * ix->seg_nb + w.label_bytes + 8 * (ix->n_nodes + 1);
    if (words_per_set) *words_per_set = (w.m + 63) / 64;
    if (places_unsupported) *places_unsupported = w.places_unsupported;
    if (chains_unsupported) *chains_unsupported = w.chains_unsupported;
    return FBG_OK;
}

// ---- alignment (fbg_pindex_chains_align / _align_stats) ------------------------------------------------------------------
// pr_prepare and k_pr_chain as in fbg_pindex_chains_rows (into buffers of the alignment state, so that call's results
// stay), the prefix table on the first call, k_pa_prepare, a scan of the window lengths, the host's look at their sum,
// the windows gathered into scratch of that size, and a wave per read for the two passes.
extern "C" int fbg_pindex_chains_align(fbg_pindex *ix, uint64_t pad, uint64_t max_window, uint32_t *row, uint32_t *edits,
                                       uint32_t *t_start, uint32_t *t_end, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    PaState &al = ix->al;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (!ix->has_rows)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_align: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    if (!ix->sd.ready || !c.ready)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_align: no fbg_pindex_chains result since the last seeds call");
    std::fill(al.stat, al.stat + 5, (uint64_t)0);
    const uint64_t n = c.n;
    al.valid = al.on_device = ix->cg.ready = false;       // the paths belong to the align call they were traced from
    al.n = n;
    if (n == 0) { al.valid = true; return FBG_OK; }
    if (n > 0x7fffffffull)        // a wave, and so a workgroup, per read
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_chains_align: %llu reads; a call takes fewer than 2^31", (unsigned long long)n);
    uint32_t *host[4] = {row, edits, t_start, t_end};
    if (c.total == 0) {          // every chain is empty, and fbg_pindex_chains may have left nothing on the device
        for (uint32_t *h : host)
            if (h) std::fill(h, h + n, (uint32_t)PA_NONE);
        al.valid = true;
        return FBG_OK;
    }
    if (pad > (1ull << 33)) pad = 1ull << 33;         // positions and read offsets are below 2^32: beyond this nothing changes
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t nb = ix->seg_nb;
    FBG_TRY(fbg_reserve(ctx, al.pref, nb * w.m * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, al.nrows, 2 * n * 4, &ix->bufs, false));
    for (DevBuf *b : {&al.info, &al.start, &al.out}) FBG_TRY(fbg_reserve(ctx, *b, n * 16, &ix->bufs, false));
    for (DevBuf *b : {&al.wlen, &al.woff}) FBG_TRY(fbg_reserve(ctx, *b, (n + 1) * 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, al.ctr, 5 * 8, &ix->bufs, false));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));                       // records ev0
    PaDev a;
    a.node_of = d.node_of;
    a.pref = al.pref.as<uint32_t>();
    a.labels = d.labels;
    a.loff = d.loff;
    a.reads = d.reads;
    a.roff = (w.saved ? w.roff : ix->poff).as<uint64_t>();
    a.m = w.m;
    a.nb = nb;
    if (!al.has_pref)             // the flag is set at the end of the call, once the table is known to be written
        hipLaunchKernelGGL(k_pa_prefix, dim3(fbg_blocks(w.m, 64)), dim3(64), 0, st, a.node_of, a.loff, a.m, a.nb, al.pref.as<uint32_t>());
    auto *ctr = al.ctr.as<unsigned long long>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, 5 * 8, st));
    const uint4 *rec = w.rec.as<uint4>();
    const uint32_t *place = c.out.as<uint32_t>();
    const uint64_t *off = c.off.as<uint64_t>();
    uint32_t *nr = al.nrows.as<uint32_t>(), *out = al.out.as<uint32_t>();
    if (w.m <= PR_SUB && !ctx->opt.rows_wave)
        hipLaunchKernelGGL(k_pr_chain<PR_SUB>, dim3(fbg_blocks(n * PR_SUB, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n,
                           (uint64_t)0, nr, nr + n, (uint64_t *)nullptr, ctr);
    else
        hipLaunchKernelGGL(k_pr_chain<FBG_WAVE>, dim3(fbg_blocks(n * FBG_WAVE, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n,
                           (uint64_t)0, nr, nr + n, (uint64_t *)nullptr, ctr);
    uint64_t *wlen = al.wlen.as<uint64_t>(), *woff = al.woff.as<uint64_t>();
    hipLaunchKernelGGL(k_pa_prepare, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, a, rec, place, off, (const uint32_t *)ix->sq.as<uint32_t>(),
                       (const uint32_t *)(nr + n), n, pad, max_window, al.info.as<uint4>(), al.start.as<uint4>(), wlen, out, ctr);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, wlen, woff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, woff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (total) {
        FBG_TRY(fbg_reserve(ctx, al.win, total, &ix->bufs, false));
        hipLaunchKernelGGL(k_pa_gather, dim3((unsigned)n), dim3(FBG_WAVE), 0, st, a, (const uint4 *)al.info.as<uint4>(),
                           (const uint4 *)al.start.as<uint4>(), (const uint64_t *)woff, al.win.as<uint8_t>());
        hipLaunchKernelGGL(k_pa_edit, dim3((unsigned)n), dim3(FBG_WAVE), 0, st, a, (const uint4 *)al.info.as<uint4>(), (const uint64_t *)woff,
                           (const uint8_t *)al.win.as<uint8_t>(), n, out);
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    uint64_t stat[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 4; k++)
        if (host[k]) FBG_HIP_TRY(ctx, hipMemcpyAsync(host[k], out + k * n, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(stat, ctr, 5 * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    std::copy(stat, stat + 5, al.stat);
    al.has_pref = true;
    al.valid = al.on_device = true;
    return FBG_OK;
}

extern "C" int fbg_pindex_align_stats(const fbg_pindex *ix, uint64_t *aligned, uint64_t *unsupported, uint64_t *too_long,
                                      uint64_t *too_wide, uint64_t *cells, uint64_t *max_read, uint64_t *table_bytes)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_align_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    const PaState &al = ix->al;
    if (aligned) *aligned = al.stat[1];
    if (unsupported) *unsupported = al.stat[0];
    if (too_long) *too_long = al.stat[2];
    if (too_wide) *too_wide = al.stat[3];
    if (cells) *cells = al.stat[4];
    if (max_read) *max_read = PA_MAX_READ;
    if (table_bytes) *table_bytes = al.has_pref ? 4 * ix->rw.m * ix->seg_nb : 0;
    return FBG_OK;
}

// ---- alignment path (fbg_pindex_chains_cigar / _cigar_fetch / _cigar_stats) ----------------------------------------
// Sizes and their scans, the host's look at the history offsets (which form the batches), the slot total and the tier
// counts; one k_pg_path launch per word count that has reads, then one per batch of longer reads, all on the stream and
// so one after the other in the one scratch; a scan of the run counts, the host's look at their sum, the compaction.
static int pg_check(const fbg_pindex *ix, const char *who)
{
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation_rows has the row table", who);
    if (!ix->sd.ready || !ix->ch.ready || !ix->al.valid)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "%s: no fbg_pindex_chains_align result since the last fbg_pindex_chains", who);
    return FBG_OK;
}

template <int NW>
static void pg_launch(hipStream_t st, const PaDev &a, const PaState &al, PgState &g, uint64_t n, uint64_t first, uint64_t reads, uint32_t cap,
                      uint64_t hbase)
{
    hipLaunchKernelGGL(k_pg_path<NW>, dim3((unsigned)reads), dim3(FBG_WAVE), NW ? (size_t)NW * 16 * (cap ? cap : 1) : 0, st, a,
                       (const uint4 *)al.info.as<uint4>(), (const uint64_t *)al.woff.as<uint64_t>(), (const uint8_t *)al.win.as<uint8_t>(),
                       (const uint32_t *)al.out.as<uint32_t>(), n, first, cap, (const uint64_t *)g.hoff.as<uint64_t>(), hbase,
                       g.hist.as<uint64_t>(), (const uint64_t *)g.soff.as<uint64_t>(), g.slots.as<uint32_t>(), g.cnt.as<uint64_t>(),
                       g.nops.as<uint32_t>(), g.ctr.as<unsigned long long>());
}

extern "C" int fbg_pindex_chains_cigar(fbg_pindex *ix, uint32_t *n_ops, uint64_t *total_ops, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PrState &w = ix->rw;
    const PaState &al = ix->al;
    PgState &g = ix->cg;
    FBG_TRY(pg_check(ix, "fbg_pindex_chains_cigar"));
    if (device_ms) *device_ms = 0;
    if (total_ops) *total_ops = 0;
    const uint64_t n = al.n;
    g.ready = false;
    if (n == 0 || !al.on_device) {            // no reads, or every chain empty: nothing of that align call on the device
        if (n_ops) std::fill(n_ops, n_ops + n, (uint32_t)0);
        std::fill(g.stat, g.stat + 5, (uint64_t)0);
        g.n = n;
        g.total = 0;
        g.on_device = false;
        g.ready = true;
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ctx, g.sz, 2 * (n + 1) * 8, &ix->bufs, false));
    for (DevBuf *b : {&g.hoff, &g.soff, &g.cnt, &g.off}) FBG_TRY(fbg_reserve(ctx, *b, (n + 1) * 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, g.nops, n * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, g.ctr, PG_CTR * 8, &ix->bufs, false));
    PaDev a;
    a.node_of = w.node_of.as<uint32_t>();
    a.pref = al.pref.as<uint32_t>();
    a.labels = w.labels.as<uint8_t>();
    a.loff = w.loff.as<uint64_t>();
    a.reads = (w.saved ? w.reads : ix->pats).as<uint8_t>();
    a.roff = (w.saved ? w.roff : ix->poff).as<uint64_t>();
    a.m = w.m;
    a.nb = ix->seg_nb;
    uint64_t *hsz = g.sz.as<uint64_t>(), *ssz = hsz + (n + 1), *hoff = g.hoff.as<uint64_t>(), *soff = g.soff.as<uint64_t>();
    uint64_t *cnt = g.cnt.as<uint64_t>(), *off = g.off.as<uint64_t>();
    auto *ctr = g.ctr.as<unsigned long long>();
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, PG_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (n + 1) * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(g.nops.p, 0, n * 4, st));
    hipLaunchKernelGGL(k_pg_sizes, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, (const uint4 *)al.info.as<uint4>(),
                       (const uint32_t *)al.out.as<uint32_t>(), n, hsz, ssz, ctr);
    for (int k = 0; k < 2; k++)
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, k ? ssz : hsz, k ? soff : hoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
        }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t hunits = 0, nslots = 0, c[PG_CTR];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&hunits, hoff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&nslots, soff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(c, ctr, PG_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    // the batches of the long reads: consecutive reads from one with a history on, while the sum fits the budget; the
    // offsets come to the host only when there is such a read
    std::vector<uint64_t> h;
    if (c[3 + PA_REG_WORDS]) {
        h.resize(n + 1);
        FBG_HIP_TRY(ctx, hipMemcpyAsync(h.data(), hoff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const int64_t kib = ctx->opt.path_batch_kib < 1 ? 1 : ctx->opt.path_batch_kib;
    const uint64_t budget = kib > (int64_t)1 << 50 ? ~0ull : (uint64_t)kib * 128;        // in units
    std::vector<std::pair<uint64_t, uint64_t>> batch;
    uint64_t units = 0;
    for (uint64_t r0 = 0; r0 < n && !h.empty();) {
        if (h[r0 + 1] == h[r0]) { r0++; continue; }
        uint64_t r1 = r0 + 1;
        while (r1 < n && h[r1 + 1] - h[r0] <= budget) r1++;
        batch.emplace_back(r0, r1);
        units = std::max(units, h[r1] - h[r0]);
        r0 = r1;
    }
    FBG_TRY(fbg_reserve(ctx, g.slots, (nslots + 1) * 4, &ix->bufs, false));
    if (units) FBG_TRY(fbg_reserve(ctx, g.hist, units * 8, &ix->bufs, false));
    if (c[3]) pg_launch<1>(st, a, al, g, n, 0, n, (uint32_t)c[8], 0);
    if (c[4]) pg_launch<2>(st, a, al, g, n, 0, n, (uint32_t)c[9], 0);
    if (c[5]) pg_launch<3>(st, a, al, g, n, 0, n, (uint32_t)c[10], 0);
    if (c[6]) pg_launch<4>(st, a, al, g, n, 0, n, (uint32_t)c[11], 0);
    for (const auto &b : batch) pg_launch<0>(st, a, al, g, n, b.first, b.second - b.first, 0, h[b.first]);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, cnt, off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    unsigned long long failed = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&failed, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (failed)
        return fbg_fail(ctx, FBG_ERR_HIP, "fbg_pindex_chains_cigar: the trace of %llu reads did not arrive at the read's start", failed);
    FBG_TRY(fbg_reserve(ctx, g.ops, (total + 1) * 4, &ix->bufs, false));
    if (total) {
        hipLaunchKernelGGL(k_pg_compact, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, (const uint64_t *)soff, (const uint32_t *)g.slots.as<uint32_t>(),
                           (const uint64_t *)off, n, g.ops.as<uint32_t>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    if (n_ops) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_ops, g.nops.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    if (device_ms) *device_ms = ms;
    if (total_ops) *total_ops = total;
    const uint64_t stat[5] = {c[1], total, c[2], hunits * 8, batch.size()};
    std::copy(stat, stat + 5, g.stat);
    g.n = n;
    g.total = total;
    g.on_device = true;
    g.ready = true;
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_cigar_fetch(fbg_pindex *ix, uint64_t *off, uint32_t *ops)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PgState &g = ix->cg;
    FBG_TRY(pg_check(ix, "fbg_pindex_chains_cigar_fetch"));
    if (!g.ready) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chains_cigar_fetch: no fbg_pindex_chains_cigar result since that align call");
    if (!g.on_device) {
        if (off) std::fill(off, off + g.n + 1, (uint64_t)0);
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (off) FBG_HIP_TRY(ctx, hipMemcpyAsync(off, g.off.p, (g.n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (ops && g.total) FBG_HIP_TRY(ctx, hipMemcpyAsync(ops, g.ops.p, g.total * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FBG_OK;
}

extern "C" int fbg_pindex_cigar_stats(const fbg_pindex *ix, uint64_t *paths, uint64_t *ops, uint64_t *columns, uint64_t *history_bytes,
                                      uint64_t *batches)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_cigar_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    uint64_t *o[5] = {paths, ops, columns, history_bytes, batches};
    for (int k = 0; k < 5; k++)
        if (o[k]) *o[k] = ix->cg.stat[k];
    return FBG_OK;
}

extern "C" uint64_t fbg_pindex_text_length(const fbg_pindex *ix) { return ix ? ix->N1 : 0; }

extern "C" int fbg_pindex_download(fbg_pindex *ix, uint8_t *text, uint32_t *sa, uint32_t *b_positions, uint32_t *e_positions,
                                   uint64_t *nb, uint64_t *ne)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (text) FBG_HIP_TRY(ctx, hipMemcpyAsync(text, ix->text.p, ix->N1, hipMemcpyDeviceToHost, st));
    if (sa) FBG_HIP_TRY(ctx, hipMemcpyAsync(sa, ix->sa.p, ix->N1 * 4, hipMemcpyDeviceToHost, st));
    if (b_positions && ix->nb) FBG_HIP_TRY(ctx, hipMemcpyAsync(b_positions, ix->bpos.p, (size_t)ix->nb * 4, hipMemcpyDeviceToHost, st));
    if (e_positions && ix->ne) FBG_HIP_TRY(ctx, hipMemcpyAsync(e_positions, ix->epos.p, (size_t)ix->ne * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nb) *nb = ix->nb;
    if (ne) *ne = ix->ne;
    return FBG_OK;
}

extern "C" int fbg_pindex_stats(const fbg_pindex *ix, uint64_t *index_bytes, double *build_ms, double *search_ms,
                                uint64_t *occ_lines)
{
    if (!ix) return FBG_ERR_INVALID;
    if (index_bytes)
        *index_bytes = ix->nblk * PX_LINE + (ix->compact ? 0 : ix->nblk * ix->sigma * 4) + 4ull * (ix->nb + ix->ne) + 256 * 6;
    if (build_ms) *build_ms = ix->build_ms;
    if (search_ms) *search_ms = ix->search_ms;
    if (occ_lines) *occ_lines = ix->occ_lines;
    return FBG_OK;
}

// The validation kernels over the index's n_nodes > 0 nodes, blocks from d_block (device), between ev0 and ev1; status,
// witnesses and counters stay in vstatus / vwn / vwo / vctr.
static int pv_launch(fbg_pindex *ix, const uint32_t *d_block, const PvMask &ig, int has_ig)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = ix->n_nodes;
    FBG_TRY(fbg_reserve(ix->ctx, ix->vstatus, n, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->vwn, n * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->vwo, n * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->vlist, n * 4, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ix->ctx, ix->vctr, 16, &ix->bufs, false));
    if (!ix->ev0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev0));
    if (!ix->ev1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->ev1));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->vctr.p, 0, 16, st));
    PvDev d = pv_dev(ix);
    d.block = d_block;
    auto *ctr = ix->vctr.as<unsigned long long>();
    uint8_t *dst = ix->vstatus.as<uint8_t>();
    uint32_t *wn = ix->vwn.as<uint32_t>(), *wo = ix->vwo.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    hipLaunchKernelGGL(k_pv_node, dim3(fbg_blocks(n, PX_THREADS)), dim3(PX_THREADS), 0, st, d, n, ig, has_ig, dst, wn, wo,
                       ix->vlist.as<uint32_t>(), ctr);
    const uint64_t wave_blocks = std::min<uint64_t>(fbg_blocks(n * FBG_WAVE, PX_THREADS), 2048);
    hipLaunchKernelGGL(k_pv_wave, dim3(wave_blocks), dim3(PX_THREADS), 0, st, d, (const uint32_t *)ix->vlist.as<uint32_t>(), ctr, dst,
                       wn, wo);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev1, st));
    return FBG_OK;
}

static PvMask pv_mask(const uint8_t *ignore_chars, uint64_t ignore_len, int *has_ig)
{
    PvMask ig = {{0, 0, 0, 0}};
    for (uint64_t k = 0; k < ignore_len; k++) ig.w[ignore_chars[k] >> 6] |= 1ull << (ignore_chars[k] & 63);
    *has_ig = (ig.w[0] | ig.w[1] | ig.w[2] | ig.w[3]) != 0;
    return ig;
}

extern "C" int fbg_pindex_validate(fbg_pindex *ix, const uint32_t *node_block, const uint8_t *ignore_chars, uint64_t ignore_len,
                                   uint8_t *status, uint64_t *witness_node, uint64_t *witness_offset, uint64_t *n_invalid,
                                   double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const uint64_t n = ix->n_nodes;
    if (n && (!node_block || !status)) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_validate: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_validate: missing ignore characters");
    if (n_invalid) *n_invalid = 0;
    if (device_ms) *device_ms = 0;
    ix->validate_ms = 0;
    ix->v_slots = ix->v_wave_nodes = 0;
    if (n == 0) return FBG_OK;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ix->ctx, ix->vblock, n * 4, &ix->bufs, false));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ix->vblock.p, node_block, n * 4, hipMemcpyHostToDevice, st));
    FBG_TRY(pv_launch(ix, ix->vblock.as<uint32_t>(), ig, has_ig));
    auto *ctr = ix->vctr.as<unsigned long long>();
    uint8_t *dst = ix->vstatus.as<uint8_t>();
    uint32_t *wn = ix->vwn.as<uint32_t>(), *wo = ix->vwo.as<uint32_t>();
    std::vector<uint32_t> hwn(witness_node ? n : 0), hwo(witness_offset ? n : 0);
    uint64_t hctr[2] = {0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(status, dst, n, hipMemcpyDeviceToHost, st));
    if (witness_node) FBG_HIP_TRY(ctx, hipMemcpyAsync(hwn.data(), wn, n * 4, hipMemcpyDeviceToHost, st));
    if (witness_offset) FBG_HIP_TRY(ctx, hipMemcpyAsync(hwo.data(), wo, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(hctr, ctr, 16, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    ix->validate_ms = ms;
    ix->v_wave_nodes = hctr[0];
    ix->v_slots = hctr[1];
    uint64_t bad = 0;
    for (uint64_t u = 0; u < n; u++) bad += status[u] == FBG_NODE_INVALID;
    for (uint64_t u = 0; u < hwn.size(); u++) witness_node[u] = hwn[u] == PV_NONE ? UINT64_MAX : hwn[u];
    for (uint64_t u = 0; u < hwo.size(); u++) witness_offset[u] = hwo[u] == PV_NONE ? UINT64_MAX : hwo[u];
    if (n_invalid) *n_invalid = bad;
    if (device_ms) *device_ms = ms;
    return FBG_OK;
}

extern "C" int fbg_pindex_validate_stats(const fbg_pindex *ix, uint64_t *slots_scanned, uint64_t *wave_nodes, uint64_t *table_bytes)
{
    if (!ix) return FBG_ERR_INVALID;
    if (slots_scanned) *slots_scanned = ix->v_slots;
    if (wave_nodes) *wave_nodes = ix->v_wave_nodes;
    if (table_bytes) *table_bytes = 17 * ix->n_nodes + 12 * ix->n_edges + 4 + 4 * ix->nctab;
    return FBG_OK;
}

extern "C" void fbg_pindex_destroy(fbg_pindex *ix) { px_destroy(ix); }

// ---- an index straight from a segmentation; validation and repair of a segmentation ----------------------------------
static int px_new_from_segmentation(fbg_ctx *ctx, const char *who, const uint64_t *boundaries, uint64_t nb, bool with_rows, fbg_pindex **out)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: no MSA set", who);
    if (!out || !boundaries || nb == 0) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing argument", who);
    *out = nullptr;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    fbg_pindex *ix = new fbg_pindex();
    ix->ctx = ctx;
    int rc;
    {
        PxScratch s;
        rc = px_build_segmentation(ix, s, boundaries, nb, true, with_rows);
    }
    if (rc != FBG_OK) { px_destroy(ix); return rc; }
    ix->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = ix;
    return FBG_OK;
}

extern "C" int fbg_pindex_build_segmentation(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, fbg_pindex **out)
{
    return px_new_from_segmentation(ctx, "fbg_pindex_build_segmentation", boundaries, nb, false, out);
}

// ... with the row table of fbg_pindex_seeds_rows / _chains_rows
extern "C" int fbg_pindex_build_segmentation_rows(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, fbg_pindex **out)
{
    return px_new_from_segmentation(ctx, "fbg_pindex_build_segmentation_rows", boundaries, nb, true, out);
}

extern "C" uint64_t fbg_pindex_node_count(const fbg_pindex *ix) { return ix ? ix->n_nodes : 0; }

extern "C" int fbg_pindex_node_info(fbg_pindex *ix, uint32_t *label_len, uint32_t *node_block, uint64_t *first_node)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    if ((node_block || first_node) && !ix->from_segmentation)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_node_info: only an index built from a segmentation knows its blocks");
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ix->n_nodes;
    if (label_len && n) FBG_HIP_TRY(ctx, hipMemcpyAsync(label_len, ix->vlen.p, n * 4, hipMemcpyDeviceToHost, st));
    if (node_block && n) FBG_HIP_TRY(ctx, hipMemcpyAsync(node_block, ix->snode_block.p, n * 4, hipMemcpyDeviceToHost, st));
    if (first_node) FBG_HIP_TRY(ctx, hipMemcpyAsync(first_node, ix->sfirst.p, (ix->seg_nb + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FBG_OK;
}

// cut[b - 1] = 1 for every block b > 0 that holds an INVALID node (the reference's to_remove); *count: INVALID nodes
__global__ void k_sv_cuts(const uint8_t *status, const uint32_t *node_block, uint64_t n, uint8_t *cut, unsigned long long *count)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = u < n && status[u] == FBG_NODE_INVALID;
    if (bad && node_block[u] > 0) cut[node_block[u] - 1] = 1;
    const uint64_t bal = __ballot(bad);
    if ((threadIdx.x % FBG_WAVE) == 0 && bal) atomicAdd(count, (unsigned long long)__popcll(bal));
}

// One round: the index of the segmentation into ix (its buffers and the scratch are reused from round to round), the
// validation kernels on the device's own node_block, the flagged cuts.  The events sv0 / sv1 enclose all of it.
static int sv_round(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, const PvMask &ig, int has_ig,
                    uint8_t *cut_bad, uint64_t *n_invalid, double *ms)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    if (!ix->sv0) FBG_HIP_TRY(ctx, hipEventCreate(&ix->sv0));
    if (!ix->sv1) FBG_HIP_TRY(ctx, hipEventCreate(&ix->sv1));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->sv0, st));
    FBG_TRY(px_build_segmentation(ix, s, boundaries, nb, false));
    const uint64_t n = ix->n_nodes;
    FBG_TRY(fbg_reserve(ctx, ix->scut, nb + 8, &ix->bufs, false));
    FBG_TRY(fbg_reserve(ctx, ix->sctr, 8, &ix->bufs, false));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->scut.p, 0, nb + 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->sctr.p, 0, 8, st));
    if (n) {
        FBG_TRY(pv_launch(ix, ix->snode_block.as<uint32_t>(), ig, has_ig));
        hipLaunchKernelGGL(k_sv_cuts, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, (const uint8_t *)ix->vstatus.as<uint8_t>(),
                           (const uint32_t *)ix->snode_block.as<uint32_t>(), n, ix->scut.as<uint8_t>(), ix->sctr.as<unsigned long long>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_HIP_TRY(ctx, hipEventRecord(ix->sv1, st));
    unsigned long long bad = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(cut_bad, ix->scut.p, nb, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bad, ix->sctr.p, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    float f = 0;
    FBG_HIP_TRY(ctx, hipEventElapsedTime(&f, ix->sv0, ix->sv1));
    *ms += f;
    *n_invalid = bad;
    return FBG_OK;
}

extern "C" int fbg_segmentation_validate(fbg_ctx *ctx, const uint64_t *boundaries, uint64_t nb, const uint8_t *ignore_chars,
                                         uint64_t ignore_len, uint8_t *cut_bad, uint64_t *n_nodes, uint64_t *n_invalid,
                                         double *device_ms)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: no MSA set");
    if (!boundaries || nb == 0 || !cut_bad) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_validate: missing ignore characters");
    if (n_nodes) *n_nodes = 0;
    if (n_invalid) *n_invalid = 0;
    if (device_ms) *device_ms = 0;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    fbg_pindex *ix = new fbg_pindex();
    ix->ctx = ctx;
    uint64_t bad = 0;
    double ms = 0;
    int rc;
    {
        PxScratch s;
        rc = sv_round(ix, s, boundaries, nb, ig, has_ig, cut_bad, &bad, &ms);
    }
    if (rc == FBG_OK) {
        if (n_nodes) *n_nodes = ix->n_nodes;
        if (n_invalid) *n_invalid = bad;
        if (device_ms) *device_ms = ms;
    }
    px_destroy(ix);
    return rc;
}

extern "C" int fbg_segmentation_repair(fbg_ctx *ctx, uint64_t *boundaries, uint64_t *nb, const uint8_t *ignore_chars,
                                       uint64_t ignore_len, uint64_t *rounds, uint64_t *removed, double *device_ms)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: no MSA set");
    if (!boundaries || !nb || *nb == 0 || !rounds || !removed) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: missing argument");
    if (ignore_len && !ignore_chars) return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_segmentation_repair: missing ignore characters");
    *rounds = 0;
    if (device_ms) *device_ms = 0;
    int has_ig = 0;
    const PvMask ig = pv_mask(ignore_chars, ignore_len, &has_ig);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    fbg_pindex *ix = new fbg_pindex();
    ix->ctx = ctx;
    std::vector<uint8_t> cut(*nb);
    double ms = 0;
    int rc = FBG_OK;
    {
        PxScratch s;
        // fbg.cpp:3471-3497: validate, drop the flagged boundaries, again until none is flagged.  Every round with a
        // flagged cut shortens the list, and a single block has no node with both an in- and an out-edge.
        for (;;) {
            uint64_t bad = 0;
            rc = sv_round(ix, s, boundaries, *nb, ig, has_ig, cut.data(), &bad, &ms);
            if (rc != FBG_OK) break;
            uint64_t flagged = 0, keep = 0;
            for (uint64_t k = 0; k < *nb; k++) flagged += cut[k] != 0;
            if (!flagged) break;
            removed[(*rounds)++] = flagged;
            for (uint64_t k = 0; k < *nb; k++)
                if (!cut[k]) boundaries[keep++] = boundaries[k];
            *nb = keep;
        }
    }
    if (rc == FBG_OK && device_ms) *device_ms = ms;
    px_destroy(ix);
    return rc;
}
