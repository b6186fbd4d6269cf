// pindex_rows.hip -- the MSA rows that carry a start place or a whole chain (fbg_pindex_seeds_rows / _chains_rows), on
// an index with the row table (fbg_pindex_build_segmentation_rows).
//
//   k_pr_seed / k_pr_place           per seed the byte its substring starts at, per start place its node, offset, seed
//                                    and block;
//   k_pr_rows / k_pr_chain           lanes as rows: one read of the row table, a walk along the row's labels, a ballot per
//                                    64 rows; k_pr_chain keeps the rows that carry every anchor of a chain.
#include "pindex_dev.h"

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

// ---- rows (fbg_pindex_seeds_rows / _chains_rows / _rows_stats) -------------------------------------------------------
// What both calls start with, for S > 0 seeds and A > 0 start places of the last seeds call: sbase per seed and rec per
// start place (k_pr_seed, k_pr_place), into buffers of the row state; d: what the row kernels read.
int pr_prepare(fbg_pindex *ix, PrDev &d)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    PrState &w = ix->rw;
    const PoState &s = ix->sd;
    const uint64_t n = ix->batch.n, S = s.n, A = s.stotal;
    FBG_TRY(px_reserve(ix, w.sbase, S * 8));
    FBG_TRY(px_reserve(ix, w.rec, A * 16));
    FBG_TRY(px_reserve(ix, w.ctr, 8));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(w.ctr.p, 0, 8, st));
    hipLaunchKernelGGL(k_pr_seed, dim3(fbg_blocks(S, 256)), dim3(256), 0, st, (const uint64_t *)ix->soff.as<uint64_t>(),
                       ps_roff(ix), (const uint32_t *)ix->sq.as<uint32_t>(), n, S,
                       w.sbase.as<uint64_t>());
    hipLaunchKernelGGL(k_pr_place, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, pv_dev(ix),
                       (const uint32_t *)ix->snode_block.as<uint32_t>(), (const uint64_t *)s.soff.as<uint64_t>(), S, A,
                       (const uint32_t *)s.ss.as<uint32_t>(), (const uint32_t *)s.sk.as<uint32_t>(), (const uint32_t *)s.rs.as<uint32_t>(),
                       w.rec.as<uint4>());
    d.node_of = w.node_of.as<uint32_t>();
    d.labels = w.labels.as<uint8_t>();
    d.loff = w.loff.as<uint64_t>();
    d.reads = ps_reads(ix);
    d.sbase = w.sbase.as<uint64_t>();
    d.slen = ix->slen.as<uint32_t>();
    d.m = w.m;
    d.nb = ix->seg_nb;
    return FBG_OK;
}

// k_pr_chain over the n chains of the last fbg_pindex_chains (rec of pr_prepare), PR_SUB lanes or a wave per read
void pr_chain_launch(fbg_pindex *ix, const PrDev &d, uint64_t n, uint64_t words, uint32_t *n_rows, uint32_t *first_row, uint64_t *bits,
                     unsigned long long *ctr)
{
    hipStream_t st = ix->ctx->stream;
    const uint4 *rec = ix->rw.rec.as<uint4>();
    const uint32_t *place = ix->ch.out.as<uint32_t>();
    const uint64_t *off = ix->ch.off.as<uint64_t>();
    if (ix->rw.m <= PR_SUB && !ix->ctx->opt.rows_wave)
        hipLaunchKernelGGL(k_pr_chain<PR_SUB>, dim3(fbg_blocks(n * PR_SUB, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n, words,
                           n_rows, first_row, bits, ctr);
    else
        hipLaunchKernelGGL(k_pr_chain<FBG_WAVE>, dim3(fbg_blocks(n * FBG_WAVE, PX_THREADS)), dim3(PX_THREADS), 0, st, d, rec, place, off, n,
                           words, n_rows, first_row, bits, ctr);
}

extern "C" int fbg_pindex_seeds_rows(fbg_pindex *ix, uint32_t *n_rows, uint32_t *first_row, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    const PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_seeds_rows", PS_SEEDS));
    w.places_unsupported = 0;
    const uint64_t A = s.stotal;
    if (A == 0) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, w.out, 2 * A * 4));
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
    FBG_TRY(px_record_end(ix));
    unsigned long long none = 0;
    if (n_rows) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_rows, out, A * 4, hipMemcpyDeviceToHost, st));
    if (first_row) FBG_HIP_TRY(ctx, hipMemcpyAsync(first_row, out + A, A * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&none, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
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
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_rows", PS_CHAINS));
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
    FBG_TRY(px_reserve(ix, w.cout, n * words * 8 + 2 * n * 4));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));
    uint64_t *bits = w.cout.as<uint64_t>();
    uint32_t *out = (uint32_t *)(bits + n * words);
    auto *ctr = w.ctr.as<unsigned long long>();
    pr_chain_launch(ix, d, n, words, out, out + n, row_bits ? bits : (uint64_t *)nullptr, ctr);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    unsigned long long none = 0;
    if (n_rows) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_rows, out, n * 4, hipMemcpyDeviceToHost, st));
    if (first_row) FBG_HIP_TRY(ctx, hipMemcpyAsync(first_row, out + n, n * 4, hipMemcpyDeviceToHost, st));
    if (row_bits) FBG_HIP_TRY(ctx, hipMemcpyAsync(row_bits, bits, n * words * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&none, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
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
