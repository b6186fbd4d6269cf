// pindex_chain.hip -- co-linear chaining of a read's seeds on the MSA columns of their start places (fbg_pindex_chains)
// and the choice between a read's two strands (fbg_pindex_chain_strands).
//
//   k_pc_key / k_pc_chain / k_pc_trace   the reads binned by their number of start places, the chaining DP over a read's
//                                    start places in three tiers, and the walk back from the chain's end (a pass that
//                                    counts, a scan, a pass that writes);
//   k_pc_strand                      per given read the better of the chains of its two virtual reads.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

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

// ---- chains (fbg_pindex_chains / _fetch / _stats) -----------------------------------------------------------------
// The start columns of the seeds' places (k_po_expand_msa<true> into the chain state's own buffer), the reads sorted by
// their number of start places, the host's look at the four bin sizes, one k_pc_chain launch per tier that has reads,
// then count, scan and write as the seeds do.  A chain has at most one anchor per seed: S entries hold every chain.
// fbg_pindex_chains_by_row (pindex_byrow.hip) runs the same steps on columns of its own, so they are four functions:
// pc_begin, pc_reserve, pc_launch and pc_finish (pindex.h).  The last three take the chain state they work on:
// fbg_pindex_chains_mapq (pindex_mapq.hip) runs them on a state of its own and leaves ix->ch alone, and so does
// fbg_pindex_chains_pairs (pindex_pairs.hip), which with adopt runs pc_launch's tail, pc_trace, on ix->ch once more.

// The checks and trivial cases of a chaining call (what: its name).  *go: there is something to launch; where there is
// not, the caller finishes its stages at once.
int pc_begin(fbg_pindex *ix, uint64_t *chain_off, uint32_t *score, double *device_ms, const char *what, bool *go)
{
    fbg_ctx *ctx = ix->ctx;
    PcState &c = ix->ch;
    const PoState &s = ix->sd;
    *go = false;
    px_begin(ix, PS_CHAINS);      // with the row choice, the alignments, their paths and the mapping quality made from the chains
    if (device_ms) *device_ms = 0;
    if (!chain_off) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing chain_off", what);
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation knows MSA columns", what);
    FBG_TRY(px_need(ix, what, PS_SEEDS));
    const uint64_t n = ix->batch.n, S = s.n, A = s.stotal;
    c.n = n;
    c.total = c.anchors = 0;
    c.tier[0] = c.tier[1] = c.tier[2] = 0;
    std::fill(chain_off, chain_off + n + 1, (uint64_t)0);
    if (score) std::fill(score, score + n, (uint32_t)0);
    if (n == 0 || S == 0 || A == 0) return FBG_OK;      // no start place: every score 0, every chain empty
    *go = true;
    return FBG_OK;
}

int pc_reserve(fbg_pindex *ix, PcState &c, PcDev &d, const uint32_t *col, uint64_t band)
{
    const PoState &s = ix->sd;
    const uint64_t n = ix->batch.n, S = s.n, A = s.stotal;
    FBG_TRY(px_reserve(ix, c.col, 2 * A * 4));
    FBG_TRY(px_reserve(ix, c.pred, A * 4));
    for (DevBuf *b : {&c.key, &c.id, &c.key2, &c.id2, &c.end, &c.score}) FBG_TRY(px_reserve(ix, *b, n * 4));
    for (DevBuf *b : {&c.len, &c.off}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    FBG_TRY(px_reserve(ix, c.out, 2 * S * 4));
    FBG_TRY(px_reserve(ix, c.ctr, 5 * 8));
    d.seed_off = ix->soff.as<uint64_t>();
    d.start_off = s.soff.as<uint64_t>();
    d.q = ix->sq.as<uint32_t>();
    d.k = ix->slen.as<uint32_t>();
    d.col = col ? col : c.col.as<uint32_t>() + A;
    d.pred = c.pred.as<uint32_t>();
    d.end = c.end.as<uint32_t>();
    d.score = c.score.as<uint32_t>();
    d.slab = nullptr;
    d.ctr = c.ctr.as<unsigned long long>();
    d.band = c.band = band;
    return FBG_OK;
}

int pc_launch(fbg_pindex *ix, PcState &c, PcDev &d, uint64_t min_score, uint64_t bin[5], const char *what)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = ix->batch.n, A = ix->sd.stotal;
    uint32_t *ka = c.key.as<uint32_t>(), *va = c.id.as<uint32_t>(), *kb = c.key2.as<uint32_t>(), *vb = c.id2.as<uint32_t>();
    hipLaunchKernelGGL(k_pc_key, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d, n, ka, va);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, va, vb, (size_t)n, 0u, 32u, st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_HIP_TRY(ctx, hipMemcpyAsync(bin, c.ctr.p, 4 * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bin[0] + bin[1] + bin[2] + bin[3] != n) return fbg_fail(ctx, FBG_ERR_HIP, "%s: the tiers hold %llu of %llu reads", what,
                                                                (unsigned long long)(bin[0] + bin[1] + bin[2] + bin[3]), (unsigned long long)n);
    if (bin[3]) {
        FBG_TRY(px_reserve(ix, c.slab, A * 16));
        d.slab = c.slab.as<uint4>();
    }
    const uint32_t *ids = vb + bin[0];
    if (bin[1])
        hipLaunchKernelGGL(k_pc_chain<0>, dim3(fbg_blocks(bin[1], PX_THREADS / PC_SUB)), dim3(PX_THREADS), 0, st, d, ids, bin[1]);
    if (bin[2]) hipLaunchKernelGGL(k_pc_chain<1>, dim3((unsigned)bin[2]), dim3(FBG_WAVE), 0, st, d, ids + bin[1], bin[2]);
    if (bin[3]) hipLaunchKernelGGL(k_pc_chain<2>, dim3((unsigned)bin[3]), dim3(FBG_WAVE), 0, st, d, ids + bin[1] + bin[2], bin[3]);
    return pc_trace(ix, c, d, min_score);
}

// The tail of pc_launch: from end, score and pred of c the lengths (0 below min_score), their scan, the chains.
int pc_trace(fbg_pindex *ix, PcState &c, PcDev &d, uint64_t min_score)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = ix->batch.n, S = ix->sd.n;
    uint64_t *len = c.len.as<uint64_t>(), *off = c.off.as<uint64_t>();
    uint32_t *out = c.out.as<uint32_t>();
    hipLaunchKernelGGL(k_pc_trace<false>, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, d, n, min_score, len, (const uint64_t *)off, out, out + S);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, len, off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    hipLaunchKernelGGL(k_pc_trace<true>, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, d, n, min_score, len, (const uint64_t *)off, out, out + S);
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

int pc_finish(fbg_pindex *ix, PcState &c, const uint64_t *chain_off, const uint64_t bin[5], const char *what)
{
    const uint64_t n = c.n;
    // a chain takes one place per seed at most, and a call has fewer than 2^32 seeds
    if (chain_off[n] >= (1ull << 32))
        return fbg_fail(ix->ctx, FBG_ERR_TOO_LARGE, "%s: %llu chain entries; a call takes fewer than 2^32", what, (unsigned long long)chain_off[n]);
    c.total = chain_off[n];
    c.anchors = bin[4];
    c.tier[0] = bin[1];
    c.tier[1] = bin[2];
    c.tier[2] = bin[3];
    return FBG_OK;
}

extern "C" int fbg_pindex_chains(fbg_pindex *ix, uint64_t band, uint64_t min_score, uint64_t *chain_off, uint32_t *score,
                                 double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PcState &c = ix->ch;
    const PoState &s = ix->sd;
    bool go = false;
    FBG_TRY(pc_begin(ix, chain_off, score, device_ms, "fbg_pindex_chains", &go));
    if (!go) { px_finish(ix, PS_CHAINS); return FBG_OK; }
    const uint64_t n = ix->batch.n, A = s.stotal;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PcDev d;
    FBG_TRY(pc_reserve(ix, c, d, nullptr, band));
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(c.ctr.p, 0, 5 * 8, st));
    po_expand_msa(ix, s, true, c.col.as<uint32_t>(), c.col.as<uint32_t>() + A);
    uint64_t bin[5] = {0, 0, 0, 0, 0};
    FBG_TRY(pc_launch(ix, c, d, min_score, bin, "fbg_pindex_chains"));
    FBG_TRY(px_record_end(ix));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(chain_off, c.off.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (score) FBG_HIP_TRY(ctx, hipMemcpyAsync(score, c.score.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bin[4], d.ctr + 4, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    FBG_TRY(pc_finish(ix, c, chain_off, bin, "fbg_pindex_chains"));
    px_finish(ix, PS_CHAINS);
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_fetch(fbg_pindex *ix, uint32_t *anchor_place, uint32_t *anchor_seed, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need(ix, "fbg_pindex_chains_fetch", PS_CHAINS));
    if (c.total == 0 || (!anchor_place && !anchor_seed)) return FBG_OK;
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t *out = c.out.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    if (anchor_place) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_place, out, c.total * 4, hipMemcpyDeviceToHost, st));
    if (anchor_seed) FBG_HIP_TRY(ctx, hipMemcpyAsync(anchor_seed, out + ix->sd.n, c.total * 4, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_record_end(ix));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
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
    FBG_TRY(px_need(ix, "fbg_pindex_chain_strands", PS_SEEDS));
    if (!ix->batch.stranded)
        return fbg_fail(ctx, FBG_ERR_INVALID, "fbg_pindex_chain_strands: the last seeds call was no fbg_pindex_seeds_strands");
    FBG_TRY(px_need(ix, "fbg_pindex_chain_strands", PS_CHAINS));
    const uint64_t n = ix->batch.n / 2;
    if (n == 0) return FBG_OK;
    uint64_t cnt[3] = {0, 0, n};
    if (ix->sd.n == 0 || ix->sd.stotal == 0) {
        if (strand) std::fill(strand, strand + n, (uint8_t)FBG_STRAND_NONE);
        if (score) std::fill(score, score + n, (uint32_t)0);
    } else {
        FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        FBG_TRY(px_reserve(ix, c.strand, n));
        FBG_TRY(px_reserve(ix, c.best, n * 4));
        FBG_TRY(px_reserve(ix, c.sctr, 3 * 8));
        FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
        FBG_HIP_TRY(ctx, hipMemsetAsync(c.sctr.p, 0, 3 * 8, st));
        hipLaunchKernelGGL(k_pc_strand, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, c.score.as<uint32_t>(), c.len.as<uint64_t>(), n,
                           c.strand.as<uint8_t>(), c.best.as<uint32_t>(), c.sctr.as<unsigned long long>());
        FBG_HIP_TRY(ctx, hipGetLastError());
        FBG_TRY(px_record_end(ix));
        if (strand) FBG_HIP_TRY(ctx, hipMemcpyAsync(strand, c.strand.p, n, hipMemcpyDeviceToHost, st));
        if (score) FBG_HIP_TRY(ctx, hipMemcpyAsync(score, c.best.p, n * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(cnt, c.sctr.p, 3 * 8, hipMemcpyDeviceToHost, st));
        FBG_TRY(px_sync_elapsed(ix, device_ms));
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
    const bool ok = px_current(ix, PS_CHAINS);
    if (anchors) *anchors = ok ? c.anchors : 0;
    if (reads_small) *reads_small = ok ? c.tier[0] : 0;
    if (reads_wave) *reads_wave = ok ? c.tier[1] : 0;
    if (reads_spill) *reads_spill = ok ? c.tier[2] : 0;
    if (small_max) *small_max = PC_SMALL;
    if (lds_max) *lds_max = PC_LDS;
    return FBG_OK;
}
