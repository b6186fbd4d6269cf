// pindex_mapq.hip -- the second-best chain of every read, outside the MSA columns of its best one, and an integer mapping
// quality from the two scores (fbg_pindex_chains_mapq / _mapq_fetch, fbg_pindex_mapq_strands, fbg_pindex_mapq_stats).
//
//   k_pq_span                        per read lo and hi of its primary chain, from the first and last entry of the chain output;
//   k_pq_mask                        per start place its witness column, or none where the widened span excludes it;
//   k_pq_final                       per read the secondary chain's span and the mapping quality; STRANDED: the quality with
//                                    the twin's score as a second competitor.
// Between k_pq_mask and k_pq_final the chain kernels of pindex_chain.hip run on the masked columns, in a chain state of
// the mapq state's own (pc_reserve, pc_launch, pc_finish).
#include "pindex_dev.h"

// What the three kernels read of the primary chains (the chain state of the last chaining call) and of the seeds.
struct PqDev {
    const uint64_t *seed_off, *start_off;     // reads -> seeds -> start places
    const uint32_t *k, *col;                  // per seed its length; per start place its witness column (unmasked)
    const uint64_t *off;                      // [n + 1] the scan of the primary chains' lengths
    const uint32_t *place, *seed;             // the primary chains: places, seeds
    const uint32_t *score;                    // [n] the primary scores
    const uint64_t *roff;                     // [n + 1] byte offsets of the (virtual) reads
    uint64_t *span;                           // [2 n] lo, hi per read
    unsigned long long *ctr;                  // PQ_CTR counters
    uint64_t n, S, A, margin;
};

// One lane per read: lo = c(a_1), hi = c(a_len) + k(a_len) of its primary chain; PQ_NOSPAN in lo for an empty chain.
__global__ void k_pq_span(PqDev d)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R >= d.n) return;
    const uint64_t o0 = d.off[R], o1 = d.off[R + 1];
    uint64_t lo = PQ_NOSPAN, hi = 0;
    if (o1 > o0) {
        const uint32_t g0 = d.place[o0], g1 = d.place[o1 - 1], t1 = d.seed[o1 - 1];
        if (g0 < d.A && g1 < d.A && t1 < d.S) {
            lo = d.col[g0];
            hi = (uint64_t)d.col[g1] + d.k[t1];
        }
    }
    d.span[2 * R] = lo;
    d.span[2 * R + 1] = hi;
}

// One lane per start place g: its seed by a search of start_off, its read by a search of seed_off, then mcol[g] = col[g]
// where the read has a primary chain and [c, c + k) does not meet [lo - margin, hi + margin), else none.  The sums
// saturate at 2^64 - 1: c + k and hi stay below 2^33, so a saturated side compares as the exact sum would.  The kept and
// the excluded anchors of reads with a primary chain are counted per wave.
__global__ __launch_bounds__(PX_THREADS) void k_pq_mask(PqDev d, uint32_t *mcol)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int what = -1;                     // 0: kept, 1: excluded
    if (g < d.A) {
        const uint64_t t = po_find(d.start_off, 0, d.S - 1, g);
        const uint64_t R = po_find(d.seed_off, 0, d.n - 1, t);
        const uint32_t c = d.col[g];
        const uint64_t lo = d.span[2 * R], hi = d.span[2 * R + 1];
        bool keep = false;
        if (c != PC_NONE && lo != PQ_NOSPAN) {
            const bool hit = pq_add_sat((uint64_t)c + d.k[t], d.margin) > lo && (uint64_t)c < pq_add_sat(hi, d.margin);
            keep = !hit;
            what = hit ? 1 : 0;
        }
        mcol[g] = keep ? c : PC_NONE;
    }
    for (int b = 0; b < 2; b++) {
        const unsigned long long m = __ballot(what == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[b], (unsigned long long)__popcll(m));
    }
}

// One lane per read.  second / soff / splace / sseed: what the chain kernels left for the masked columns.  Plain: the
// secondary chain's span into span2 (lo, then hi; none where it is empty), mapq = 60 * (s1 - min(second, s1)) / L floored,
// 0 for an empty primary chain or an empty read, and the counters 2 .. 4 over the reads with a primary chain.  STRANDED
// (n even, the twin of v is v +- n / 2): the same quality with max(second, the twin's primary score) for second; nothing
// else is written.
template <bool STRANDED>
__global__ void k_pq_final(PqDev d, const uint32_t *second, const uint64_t *soff, const uint32_t *splace, const uint32_t *sseed,
                           uint32_t *span2, uint8_t *mapq)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b0 = 0, b60 = 0, bsec = 0;
    if (R < d.n) {
        const bool primary = d.off[R + 1] > d.off[R];
        const uint64_t L = d.roff[R + 1] - d.roff[R], s1 = d.score[R];
        uint64_t s2 = second[R];
        if (STRANDED) {
            const uint64_t h = d.n / 2, w = R < h ? R + h : R - h, sw = d.score[w];
            s2 = sw > s2 ? sw : s2;
        } else {
            const uint64_t o0 = soff[R], o1 = soff[R + 1];
            uint32_t lo = PC_NONE, hi = PC_NONE;
            if (o1 > o0) {
                const uint32_t g0 = splace[o0], g1 = splace[o1 - 1], t1 = sseed[o1 - 1];
                if (g0 < d.A && g1 < d.A && t1 < d.S) {
                    lo = d.col[g0];
                    hi = d.col[g1] + d.k[t1];
                }
            }
            span2[R] = lo;
            span2[d.n + R] = hi;
        }
        s2 = s2 < s1 ? s2 : s1;
        const uint64_t q = primary && L ? 60 * (s1 - s2) / L : 0;
        mapq[R] = (uint8_t)q;
        if (!STRANDED && primary) {
            b0 = q == 0;
            b60 = q == 60;
            bsec = second[R] != 0;
        }
    }
    if (!STRANDED) {
        const int flag[3] = {bsec, b0, b60};
        for (int b = 0; b < 3; b++) {
            const unsigned long long m = __ballot(flag[b]);
            if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[2 + b], (unsigned long long)__popcll(m));
        }
    }
}

// What the kernels read, after a successful chaining call with start places.  span and ctr are reserved by the caller.
static PqDev pq_dev(fbg_pindex *ix, uint64_t margin)
{
    PqState &q = ix->pq;
    const PcState &c = ix->ch;
    const uint64_t S = ix->sd.n, A = ix->sd.stotal;
    PqDev d;
    d.seed_off = ix->soff.as<uint64_t>();
    d.start_off = ix->sd.soff.as<uint64_t>();
    d.k = ix->slen.as<uint32_t>();
    d.col = q.ch.col.as<uint32_t>() + A;
    d.off = c.off.as<uint64_t>();
    d.place = c.out.as<uint32_t>();
    d.seed = c.out.as<uint32_t>() + S;
    d.score = c.score.as<uint32_t>();
    d.roff = ps_roff(ix);
    d.span = q.span.as<uint64_t>();
    d.ctr = q.ctr.as<unsigned long long>();
    d.n = ix->batch.n;
    d.S = S;
    d.A = A;
    d.margin = margin;
    return d;
}

// ---- fbg_pindex_chains_mapq / _mapq_fetch / fbg_pindex_mapq_strands / fbg_pindex_mapq_stats ------------------------------
// The witness columns into the mapq state's own buffer (k_po_expand_msa<true>, as fbg_pindex_chains expands them: the
// masked columns that fbg_pindex_chains_by_row chained on play no part), k_pq_span, k_pq_mask, the chain kernels on the
// masked columns with the band of the primary call and min_score 0, k_pq_final.  Nothing of ix->ch is written.
extern "C" int fbg_pindex_chains_mapq(fbg_pindex *ix, uint64_t margin, uint64_t *second_off, uint32_t *second, uint32_t *second_lo,
                                      uint32_t *second_hi, uint8_t *mapq, double *device_ms)
{
    static const char *const what = "fbg_pindex_chains_mapq";
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PqState &q = ix->pq;
    const PcState &c = ix->ch;
    const PoState &s = ix->sd;
    px_begin(ix, PS_MAPQ);
    if (device_ms) *device_ms = 0;
    if (!second_off) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing second_off", what);
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation knows MSA columns", what);
    FBG_TRY(px_need(ix, what, PS_CHAINS));
    const uint64_t n = ix->batch.n, S = s.n, A = s.stotal;
    q.n = n;
    q.total = 0;
    q.on_device = false;
    std::fill(q.stat, q.stat + 5, (uint64_t)0);
    std::fill(second_off, second_off + n + 1, (uint64_t)0);
    if (second) std::fill(second, second + n, (uint32_t)0);
    if (second_lo) std::fill(second_lo, second_lo + n, (uint32_t)PC_NONE);
    if (second_hi) std::fill(second_hi, second_hi + n, (uint32_t)PC_NONE);
    if (mapq) std::fill(mapq, mapq + n, (uint8_t)0);
    if (n == 0 || S == 0 || A == 0) { px_finish(ix, PS_MAPQ); return FBG_OK; }    // no start place: no primary chain, no secondary
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, q.span, 2 * n * 8));
    FBG_TRY(px_reserve(ix, q.mcol, A * 4));
    FBG_TRY(px_reserve(ix, q.span2, 2 * n * 4));
    FBG_TRY(px_reserve(ix, q.mapq, n));
    FBG_TRY(px_reserve(ix, q.ctr, PQ_CTR * 8));
    PcDev pd;
    FBG_TRY(pc_reserve(ix, q.ch, pd, q.mcol.as<uint32_t>(), c.band));
    q.ch.n = n;
    const PqDev d = pq_dev(ix, margin);
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(q.ctr.p, 0, PQ_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(q.ch.ctr.p, 0, 5 * 8, st));
    po_expand_msa(ix, s, true, q.ch.col.as<uint32_t>(), q.ch.col.as<uint32_t>() + A);
    hipLaunchKernelGGL(k_pq_span, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_pq_mask, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, d, q.mcol.as<uint32_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t bin[5] = {0, 0, 0, 0, 0};
    FBG_TRY(pc_launch(ix, q.ch, pd, 0, bin, what));
    const uint32_t *out = q.ch.out.as<uint32_t>();
    hipLaunchKernelGGL(k_pq_final<false>, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d, (const uint32_t *)q.ch.score.as<uint32_t>(),
                       (const uint64_t *)q.ch.off.as<uint64_t>(), out, out + S, q.span2.as<uint32_t>(), q.mapq.as<uint8_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    uint64_t ctr[PQ_CTR] = {0, 0, 0, 0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(second_off, q.ch.off.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (second) FBG_HIP_TRY(ctx, hipMemcpyAsync(second, q.ch.score.p, n * 4, hipMemcpyDeviceToHost, st));
    if (second_lo) FBG_HIP_TRY(ctx, hipMemcpyAsync(second_lo, q.span2.p, n * 4, hipMemcpyDeviceToHost, st));
    if (second_hi) FBG_HIP_TRY(ctx, hipMemcpyAsync(second_hi, q.span2.as<uint32_t>() + n, n * 4, hipMemcpyDeviceToHost, st));
    if (mapq) FBG_HIP_TRY(ctx, hipMemcpyAsync(mapq, q.mapq.p, n, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ctr, q.ctr.p, PQ_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bin[4], pd.ctr + 4, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    FBG_TRY(pc_finish(ix, q.ch, second_off, bin, what));
    q.total = second_off[n];
    q.stat[0] = ctr[2];
    q.stat[1] = ctr[0];
    q.stat[2] = ctr[1];
    q.stat[3] = ctr[3];
    q.stat[4] = ctr[4];
    q.on_device = true;
    px_finish(ix, PS_MAPQ);
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_mapq_fetch(fbg_pindex *ix, uint32_t *anchor_place, uint32_t *anchor_seed, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PqState &q = ix->pq;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need(ix, "fbg_pindex_chains_mapq_fetch", PS_MAPQ));
    if (q.total == 0 || (!anchor_place && !anchor_seed)) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t *out = q.ch.out.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (anchor_place) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_place, out, q.total * 4, hipMemcpyDeviceToHost, st));
    if (anchor_seed) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_seed, out + ix->sd.n, q.total * 4, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_record_end(ix));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    return FBG_OK;
}

// The twin's primary score as a second competitor (k_pq_final<true>), from what the chaining call and the mapq call left
// on the device.  Where the mapq call launched nothing there is no chain on either strand: every quality 0.
extern "C" int fbg_pindex_mapq_strands(fbg_pindex *ix, uint8_t *mapq_stranded, double *device_ms)
{
    static const char *const what = "fbg_pindex_mapq_strands";
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PqState &q = ix->pq;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need(ix, what, PS_SEEDS));
    if (!ix->batch.stranded) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: the last seeds call was no fbg_pindex_seeds_strands", what);
    FBG_TRY(px_need(ix, what, PS_MAPQ));
    const uint64_t n = ix->batch.n;
    if (n == 0 || !mapq_stranded) return FBG_OK;
    if (!q.on_device) { std::fill(mapq_stranded, mapq_stranded + n, (uint8_t)0); return FBG_OK; }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, q.smapq, n));
    const PqDev d = pq_dev(ix, 0);
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    hipLaunchKernelGGL(k_pq_final<true>, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d, (const uint32_t *)q.ch.score.as<uint32_t>(),
                       (const uint64_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                       q.smapq.as<uint8_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(mapq_stranded, q.smapq.p, n, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    return FBG_OK;
}

extern "C" int fbg_pindex_mapq_stats(const fbg_pindex *ix, uint64_t *reads_with_second, uint64_t *anchors_kept, uint64_t *anchors_excluded,
                                     uint64_t *mapq0, uint64_t *mapq60)
{
    if (!ix) return FBG_ERR_INVALID;
    const PqState &q = ix->pq;
    const bool ok = px_current(ix, PS_MAPQ);
    uint64_t *out[5] = {reads_with_second, anchors_kept, anchors_excluded, mapq0, mapq60};
    for (int k = 0; k < 5; k++)
        if (out[k]) *out[k] = ok ? q.stat[k] : 0;
    return FBG_OK;
}
