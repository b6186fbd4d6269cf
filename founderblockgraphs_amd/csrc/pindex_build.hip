// pindex_build.hip -- the pattern index of a founder graph, built on the device (the reference's make_index,
// fbg.cpp:2809-2953); create, destroy and what an index reports about itself.
//
// Text: for every node u in id order and every distinct out-neighbour v in ascending order, reverse(label(u) +
// label(v) + '#'), then one 0 sentinel (N + 1 symbols in all).
//   k_px_edge_len / k_px_edge_text   |u| + |v| + 1 per edge, an exclusive scan for the offsets, one wave per edge
//                                    writes its reversed string;
//   suffix array                     prefix doubling: k_px_keys0 packs the first K symbol codes of every suffix,
//                                    a radix sort orders them; every later round re-sorts only the suffixes of
//                                    groups that still tie, by (rank of the group, rank h symbols ahead), and
//                                    doubles h, until no group is left (exact SA, any byte alphabet);
//   k_px_lines / k_px_counts         BWT and the occ structure (layout: pindex_dev.h), one wave per 128 BWT positions;
//   B / E                            every label searched from [0, N] (px_walk_labels, locate.hip), flags at lhs / rhs,
//                                    compacted into sorted position lists; k_pv_ctab: the coarse table of pv_edge;
//   k_ps_*                           the index of a segmentation's graph without the host (fbg_pindex_build_segmentation):
//                                    labels gathered from the resident MSA, edges, validation tables and the byte
//                                    histogram from the device stage of fbg_block_graph ("prepare from a segmentation");
//   k_pm_units / k_pm_fill           the MSA coordinate table of such an index: per node its representative row, first
//                                    column and, for a row with gaps in the block, a bitmap of its non-gap cells with a
//                                    running count every PM_W words.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>
#include <chrono>

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

// ---- build ----------------------------------------------------------------------------------------------------
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

// bytes of host memory into b (reserved with 8 bytes to spare, on the owner's list), on the context's stream
static int px_upload(fbg_ctx *ctx, std::vector<DevBuf *> &owner, DevBuf &b, const void *h, size_t bytes)
{
    FBG_TRY(fbg_reserve(ctx, b, bytes + 8, &owner, false));
    if (bytes) FBG_HIP_TRY(ctx, hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return FBG_OK;
}

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
    // labels (padded to whole 8-byte words for the walk's reads) and offsets rebased to 0
    FBG_TRY(fbg_reserve(ix->ctx, s.labels, ((L + 7) & ~7ull) + 16, &s.bufs, false));
    FBG_HIP_TRY(ctx, hipMemsetAsync(s.labels.p, 0, s.labels.cap, st));
    if (L) FBG_HIP_TRY(ctx, hipMemcpyAsync(s.labels.p, labels + lbase, L, hipMemcpyHostToDevice, st));
    FBG_TRY(px_upload(ctx, s.bufs, s.loff, label_off, (n_nodes + 1) * 8));
    if (lbase) px_rebase(st, s.loff.as<uint64_t>(), n_nodes, lbase);
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vesrc, esrc.data(), E * 4));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vedst, edst.data(), E * 4));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vestart, estart.data(), (E + 1) * 4));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vtpos, vtpos.data(), n_nodes * 4));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vlen, vlen.data(), n_nodes * 4));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->vflag, vflag.data(), n_nodes));
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
    for (int s = 0; s < PS_COUNT; s++) px_begin(ix, (PsStage)s);      // no result of the index as it was is current

    FBG_TRY(px_reserve(ix, ix->vrng, n_nodes * 8));
    ix->n_edges = E;
    ix->nctab = ((N1 - 1) >> PV_CSHIFT) + 2;
    FBG_TRY(px_reserve(ix, ix->vctab, ix->nctab * 4));
    if (E) hipLaunchKernelGGL(k_pv_ctab, dim3(fbg_blocks(ix->nctab, 256)), dim3(256), 0, st, ix->vestart.as<uint32_t>(), (uint32_t)E,
                              ix->nctab, ix->vctab.as<uint32_t>());
    FBG_TRY(px_upload(ctx, s.bufs, s.code_u8, code_u8, 256));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->code, code, sizeof(code)));
    FBG_TRY(px_upload(ctx, ix->bufs, ix->C, C, sizeof(C)));

    // text
    FBG_TRY(px_reserve(ix, ix->text, N1 + 64));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ix->text.p, 0, ix->text.cap, st));
    if (E) {
        uint64_t *eoff = s.eoff.as<uint64_t>();
        if (!pp.eoff_ready) {
            for (DevBuf *d : {&s.elen, &s.eoff}) FBG_TRY(fbg_reserve(ix->ctx, *d, E * 8, &s.bufs, false));
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
    FBG_TRY(px_reserve(ix, ix->sa, N1 * 4));
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
    FBG_TRY(px_reserve(ix, ix->lines, nblk * PX_LINE));
    for (DevBuf *d : {&s.cntT, &s.cntX}) FBG_TRY(fbg_reserve(ix->ctx, *d, nblk * S * 4, &s.bufs, false));
    if (!ix->compact) FBG_TRY(px_reserve(ix, ix->cnt_tab, nblk * S * 4));
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
    if (n_nodes) px_walk_labels(ix, s.labels.as<uint8_t>(), s.loff.as<uint64_t>(), n_nodes, bflag, eflag);
    for (DevBuf *d : {&ix->bpos, &ix->epos}) FBG_TRY(px_reserve(ix, *d, N1 * 4 < n_nodes * 4 ? N1 * 4 : n_nodes * 4));
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
    for (DevBuf *b : {&ix->snode_block, &ix->vlen, &ix->vtpos}) FBG_TRY(R(ix->bufs, *b, n_nodes * 4));
    FBG_TRY(R(ix->bufs, ix->sfirst, (nb + 1) * 8));
    FBG_TRY(R(ix->bufs, ix->vflag, n_nodes));
    for (DevBuf *b : {&s.nrow, &s.firstE, &s.nout, &s.nin}) FBG_TRY(R(s.bufs, *b, n_nodes * 4));
    for (DevBuf *b : {&s.len64, &s.loff}) FBG_TRY(R(s.bufs, *b, (n_nodes + 1) * 8));
    FBG_TRY(R(s.bufs, s.ebase, (nb + 1) * 8));
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
        for (DevBuf *b : {&s.munit, &s.muoff}) FBG_TRY(R(s.bufs, *b, (n_nodes + 1) * 8));
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
    for (DevBuf *b : {&ix->vesrc, &ix->vedst}) FBG_TRY(R(ix->bufs, *b, E * 4));
    FBG_TRY(R(ix->bufs, ix->vestart, (E + 1) * 4));
    for (DevBuf *b : {&s.elen, &s.eoff}) FBG_TRY(R(s.bufs, *b, (E + 1) * 8));
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

int px_build_segmentation(fbg_pindex *ix, PxScratch &s, const uint64_t *boundaries, uint64_t nb, bool with_map, bool with_rows)
{
    PxPrep pp;
    FBG_TRY(px_prepare_segmentation(ix, s, boundaries, nb, pp, with_map, with_rows));
    return px_build_prepared(ix, s, pp);
}

// The index object with its events: ev0 / ev1 around the device work of a call, sv0 / sv1 around a whole round of
// fbg_segmentation_validate / _repair.
int px_new(fbg_ctx *ctx, fbg_pindex **out)
{
    fbg_pindex *ix = new fbg_pindex();
    ix->ctx = ctx;
    for (hipEvent_t *ev : {&ix->ev0, &ix->ev1, &ix->sv0, &ix->sv1}) {
        const hipError_t e = hipEventCreate(ev);
        if (e != hipSuccess) {
            px_destroy(ix);
            return fbg_fail(ctx, FBG_ERR_HIP, "pattern index: hipEventCreate failed: %s", hipGetErrorString(e));
        }
    }
    *out = ix;
    return FBG_OK;
}

void px_destroy(fbg_pindex *ix)
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
    fbg_pindex *ix = nullptr;
    FBG_TRY(px_new(ctx, &ix));
    int rc = px_build(ix, labels, label_off, n_nodes, edge_off, edge_dst);
    if (rc != FBG_OK) { px_destroy(ix); return rc; }
    ix->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = ix;
    return FBG_OK;
}

// ---- an index straight from a segmentation ---------------------------------------------------------------------------
static int px_new_from_segmentation(fbg_ctx *ctx, const char *who, const uint64_t *boundaries, uint64_t nb, bool with_rows, fbg_pindex **out)
{
    if (!ctx) return FBG_ERR_INVALID;
    if (!ctx->d_msa) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: no MSA set", who);
    if (!out || !boundaries || nb == 0) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing argument", who);
    *out = nullptr;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    fbg_pindex *ix = nullptr;
    FBG_TRY(px_new(ctx, &ix));
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

extern "C" void fbg_pindex_destroy(fbg_pindex *ix) { px_destroy(ix); }

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
