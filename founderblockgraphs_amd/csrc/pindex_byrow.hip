// pindex_byrow.hip -- chaining along one MSA row (fbg_pindex_chains_by_row): per read the row whose supported anchors
// chain best, then the chain DP of pindex_chain.hip on the start columns that this row leaves.
//
//   k_pb_key                         the reads binned by their number of start places: none, LDS tier, device tier, too many;
//   k_pb_sizes                       the device tier's place counts as 64-bit sizes for the scan that lays out its slab;
//   k_pb_score                       a wave per read, lanes as rows, 64 at a time: a support word per place, the chain DP of
//                                    every row on the places it supports, the best row;
//   k_pb_mask                        per start place its column, or none where the read's row does not support it.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

// key = start places of the read, id = the read; every read starts without a row (k_pb_score overwrites its reads)
__global__ void k_pb_key(PbDev d, uint64_t n, uint32_t *key, uint32_t *id)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;
    if (t < n) {
        const uint64_t cnt = d.start_off[d.seed_off[t + 1]] - d.start_off[d.seed_off[t]];
        key[t] = (uint32_t)cnt;
        id[t] = (uint32_t)t;
        tier = cnt == 0 ? 0 : cnt > d.max ? 3 : cnt <= d.lds ? 1 : 2;
        d.row[t] = PR_NONE;
        d.score[t] = 0;
        d.nbest[t] = 0;
        if (tier == 2) atomicAdd(&d.ctr[4], (unsigned long long)cnt);
    }
    for (int b = 0; b < 4; b++) {
        const unsigned long long m = __ballot(tier == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[b], (unsigned long long)__popcll(m));
    }
}

// sz[i] = places of the i-th read of the device tier (key: the sorted keys from that tier on), sz[cnt] = 0 for the scan
__global__ void k_pb_sizes(const uint32_t *key, uint64_t cnt, uint64_t *sz)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= cnt) sz[i] = i < cnt ? key[i] : 0;
}

__device__ __forceinline__ uint32_t pb_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
// a support word: both halves as unsigned values (readfirstlane returns an int, and bit 31 of the low half is a row)
__device__ __forceinline__ uint64_t pb_uniform64(uint64_t v) { return ((uint64_t)pb_uniform((uint32_t)(v >> 32)) << 32) | pb_uniform((uint32_t)v); }

// One wave per read of ids[0 .. cnt), one read per workgroup.  State per start place a of the read: rec[a] = (column,
// q_start, length, seed), sup[a] = the rows of the current chunk that support it as a ballot word (0 for a place without
// a column), best[a * 64 + lane] = the best chain of row r0 + lane that ends in a (0 where the row does not support it):
// a lane reads and writes its own column of best only, so these need no fence, and a wave's access is 256 consecutive
// bytes.  TIER 0 keeps the state in LDS, for reads of up to PB_LDS places; TIER 1 in the read's stretch doff[i] ..
// doff[i + 1] of the slab (T places in all: records, then words, then scores).  A read whose places do not fit what the
// binning promised is left without a row, never written past its state.
//
// Per chunk of 64 rows: the support words, place by place (the lanes walk their rows' labels; a chunk that supports
// nothing is passed over); then the DP in place order, which is seed order.  For place j the lanes test 64 places of
// earlier seeds at a time -- a row in common and `precedes`, in the signed 64-bit arithmetic of pc_read -- and the
// ballot of the test lists the predecessors; every lane folds its own score of each into a maximum.  Rows ascend from
// chunk to chunk, so the first maximum a lane keeps is its smallest row; the lanes are merged at the end by (score
// descending, row ascending), the counts of equal scores added.  Every loop is bounded by the read's places or by m.
template <int TIER>
__global__ __launch_bounds__(FBG_WAVE) void k_pb_score(PbDev d, PrDev w, const uint32_t *ids, uint64_t cnt, const uint64_t *doff,
                                                      uint8_t *slab, uint64_t T)
{
    __shared__ uint4 l_rec[TIER == 0 ? PB_LDS : 1];
    __shared__ uint64_t l_sup[TIER == 0 ? PB_LDS : 1];
    __shared__ uint32_t l_best[TIER == 0 ? PB_LDS * FBG_WAVE : 1];
    const uint64_t i = blockIdx.x;
    if (i >= cnt) return;
    const uint32_t R = ids[i], lane = threadIdx.x;
    const uint64_t s0 = d.seed_off[R], s1 = d.seed_off[R + 1];
    const uint64_t g0 = d.start_off[s0], A64 = d.start_off[s1] - g0;
    uint4 *rec;
    uint64_t *sup;
    uint32_t *best;
    if constexpr (TIER == 0) {
        if (A64 == 0 || A64 > PB_LDS) return;
        rec = l_rec; sup = l_sup; best = l_best;
    } else {
        const uint64_t o = doff[i];
        if (A64 == 0 || A64 > 0xffffffffull || doff[i + 1] - o != A64 || o + A64 > T) return;
        rec = (uint4 *)slab + o;
        sup = (uint64_t *)(slab + T * 16) + o;
        best = (uint32_t *)(slab + T * 24) + o * FBG_WAVE;
    }
    const uint32_t A = (uint32_t)A64;
    bool mine = false;
    for (uint32_t a = lane; a < A; a += FBG_WAVE) {
        const uint32_t t = d.rec[g0 + a].z, c = d.col[g0 + a];
        rec[a] = make_uint4(c, d.q[t], d.k[t], t);
        mine |= c != PC_NONE;
    }
    const bool anchored = __any(mine);
    pc_sync();
    uint32_t top = 0, trow = PR_NONE, tcnt = 0;
    for (uint64_t r0 = 0; r0 < w.m; r0 += FBG_WAVE) {
        const uint64_t r = r0 + lane;
        uint64_t any = 0;
        for (uint32_t a = 0; a < A; a++) {
            const uint4 rc = d.rec[g0 + a];
            const uint64_t bits = __ballot(pb_uniform(rec[a].x) != PC_NONE && r < w.m && pr_supports(w, rc, r));
            if (lane == 0) sup[a] = bits;
            any |= bits;
        }
        if (any == 0) continue;
        pc_sync();
        uint32_t ctop = 0;
        for (uint32_t j = 0; j < A; j++) {
            const uint64_t sj = pb_uniform64(sup[j]);
            if (sj == 0) continue;
            const uint4 ej = rec[j];
            const uint32_t cj = pb_uniform(ej.x), qj = pb_uniform(ej.y), kj = pb_uniform(ej.z), tj = pb_uniform(ej.w);
            const uint32_t a0 = (uint32_t)(d.start_off[tj] - g0);        // the places of earlier seeds
            uint32_t m = 0;
            for (uint32_t b0 = 0; b0 < a0; b0 += FBG_WAVE) {
                const uint32_t x = b0 + lane;
                bool ok = false;
                if (x < a0 && (sup[x] & sj) != 0) {
                    const uint4 e = rec[x];
                    const int64_t dc = (int64_t)cj - (int64_t)e.x;
                    const int64_t sur = dc - ((int64_t)qj - (int64_t)e.y);
                    const uint64_t mag = sur < 0 ? (uint64_t)-sur : (uint64_t)sur;
                    ok = dc >= (int64_t)e.z && mag <= d.band;
                }
                for (uint64_t pre = __ballot(ok); pre; pre &= pre - 1) {
                    const uint32_t v = best[(size_t)(b0 + (uint32_t)__ffsll((unsigned long long)pre) - 1) * FBG_WAVE + lane];
                    m = v > m ? v : m;
                }
            }
            const uint32_t v = (sj >> lane) & 1 ? kj + m : 0;
            best[(size_t)j * FBG_WAVE + lane] = v;
            ctop = v > ctop ? v : ctop;
        }
        if (ctop > top) { top = ctop; trow = (uint32_t)r; tcnt = 1; }
        else if (ctop == top && ctop != 0) tcnt++;
        pc_sync();               // the words of this chunk are read before those of the next are written
    }
#pragma unroll
    for (int o = FBG_WAVE / 2; o > 0; o >>= 1) {
        const uint32_t ot = __shfl_xor(top, o), orow = __shfl_xor(trow, o), oc = __shfl_xor(tcnt, o);
        if (ot > top) { top = ot; trow = orow; tcnt = oc; }
        else if (ot == top) { trow = orow < trow ? orow : trow; tcnt += oc; }
    }
    if (lane == 0) {
        d.row[R] = top ? trow : PR_NONE;
        d.score[R] = top;
        d.nbest[R] = top ? tcnt : 0;
        if (anchored && top == 0) atomicAdd(&d.ctr[5], 1ull);
    }
}

// One lane per start place g: its read from the seed of rec[g] by a search of seed_off, then col2[g] = col[g] where the
// read has a row and that row supports g, else none.  The kept places are counted per wave.
__global__ __launch_bounds__(PX_THREADS) void k_pb_mask(PbDev d, PrDev w, uint64_t n, uint64_t total, uint32_t *col2)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (g < total) {
        const uint4 rc = d.rec[g];
        const uint32_t c = d.col[g], row = d.row[po_find(d.seed_off, 0, n - 1, rc.z)];
        keep = row != PR_NONE && row < w.m && c != PC_NONE && pr_supports(w, rc, row);
        col2[g] = keep ? c : PC_NONE;
    }
    const unsigned long long m = __ballot(keep);
    if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[6], (unsigned long long)__popcll(m));
}

// ---- chaining by row (fbg_pindex_chains_by_row / _stats) -------------------------------------------------------------------
// pr_prepare (sbase, rec; records ev0), the start columns into the chain state's own buffer as fbg_pindex_chains leaves
// them, the reads sorted by their number of start places, the host's look at the bins, k_pb_score per tier that has
// reads, k_pb_mask, then pc_launch on the masked columns: the chain state is what fbg_pindex_chains leaves for them.  The
// host then compares the scores of the two phases.
extern "C" int fbg_pindex_chains_by_row(fbg_pindex *ix, uint64_t band, uint64_t min_score, uint64_t *chain_off, uint32_t *score,
                                        uint32_t *row, uint32_t *n_best_rows, double *device_ms)
{
    static const char *const what = "fbg_pindex_chains_by_row";
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PbState &b = ix->pb;
    PcState &c = ix->ch;
    const PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    if (!ix->has_rows)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation_rows has the row table", what);
    bool go = false;
    FBG_TRY(pc_begin(ix, chain_off, score, device_ms, what, &go));
    const uint64_t n = ix->batch.n, A = s.stotal;
    std::fill(b.stat, b.stat + 5, (uint64_t)0);
    if (row) std::fill(row, row + n, (uint32_t)PR_NONE);
    if (n_best_rows) std::fill(n_best_rows, n_best_rows + n, (uint32_t)0);
    if (!go) { px_finish(ix, PS_CHAINS); px_finish(ix, PS_BYROW); return FBG_OK; }
    if (n > 0x7fffffffull)        // a wave, and so a workgroup, per read
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu reads; a call takes fewer than 2^31", what, (unsigned long long)n);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t omax = ctx->opt.byrow_max, olds = ctx->opt.byrow_lds;
    const uint64_t maxp = omax < 0 ? 0 : std::min<uint64_t>((uint64_t)omax, 0xffffffffull);
    const uint64_t ldsp = std::min<uint64_t>(olds < 0 ? 0 : olds == 0 ? PB_LDS : std::min<uint64_t>((uint64_t)olds, PB_LDS), maxp);
    FBG_TRY(px_reserve(ix, b.col2, A * 4));
    for (DevBuf *x : {&b.row, &b.score, &b.nbest, &b.key, &b.id, &b.key2, &b.id2}) FBG_TRY(px_reserve(ix, *x, n * 4));
    FBG_TRY(px_reserve(ix, b.ctr, PB_CTR * 8));
    PcDev pd;
    FBG_TRY(pc_reserve(ix, c, pd, b.col2.as<uint32_t>(), band));
    PrDev w;
    FBG_TRY(pr_prepare(ix, w));                       // records ev0
    FBG_HIP_TRY(ctx, hipMemsetAsync(b.ctr.p, 0, PB_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(c.ctr.p, 0, 5 * 8, st));
    po_expand_msa(ix, s, true, c.col.as<uint32_t>(), c.col.as<uint32_t>() + A);
    PbDev d;
    d.seed_off = pd.seed_off;
    d.start_off = pd.start_off;
    d.q = pd.q;
    d.k = pd.k;
    d.col = c.col.as<uint32_t>() + A;
    d.rec = ix->rw.rec.as<uint4>();
    d.row = b.row.as<uint32_t>();
    d.score = b.score.as<uint32_t>();
    d.nbest = b.nbest.as<uint32_t>();
    d.ctr = b.ctr.as<unsigned long long>();
    d.band = band;
    d.lds = ldsp;
    d.max = maxp;
    uint32_t *ka = b.key.as<uint32_t>(), *va = b.id.as<uint32_t>(), *kb = b.key2.as<uint32_t>(), *vb = b.id2.as<uint32_t>();
    hipLaunchKernelGGL(k_pb_key, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d, n, ka, va);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, ka, kb, va, vb, (size_t)n, 0u, 32u, st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t bin[PB_CTR] = {0, 0, 0, 0, 0, 0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(bin, b.ctr.p, 5 * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bin[0] + bin[1] + bin[2] + bin[3] != n)
        return fbg_fail(ctx, FBG_ERR_HIP, "%s: the tiers hold %llu of %llu reads", what,
                        (unsigned long long)(bin[0] + bin[1] + bin[2] + bin[3]), (unsigned long long)n);
    const uint32_t *ids = vb + bin[0];
    if (bin[1])
        hipLaunchKernelGGL(k_pb_score<0>, dim3((unsigned)bin[1]), dim3(FBG_WAVE), 0, st, d, w, ids, bin[1], (const uint64_t *)nullptr,
                           (uint8_t *)nullptr, (uint64_t)0);
    if (bin[2]) {
        const uint64_t T = bin[4];
        if (T > (1ull << 63) / PB_PLACE)
            return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu start places in the device tier", what, (unsigned long long)T);
        FBG_TRY(px_reserve(ix, b.doff, 2 * (bin[2] + 1) * 8));
        FBG_TRY(px_reserve(ix, b.slab, T * PB_PLACE));
        uint64_t *sz = b.doff.as<uint64_t>(), *doff = sz + bin[2] + 1;
        hipLaunchKernelGGL(k_pb_sizes, dim3(fbg_blocks(bin[2] + 1, 256)), dim3(256), 0, st, (const uint32_t *)(kb + bin[0] + bin[1]), bin[2], sz);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, sz, doff, (uint64_t)0, (size_t)(bin[2] + 1), rocprim::plus<uint64_t>(), st);
        }));
        hipLaunchKernelGGL(k_pb_score<1>, dim3((unsigned)bin[2]), dim3(FBG_WAVE), 0, st, d, w, ids + bin[1], bin[2], (const uint64_t *)doff,
                           b.slab.as<uint8_t>(), T);
    }
    hipLaunchKernelGGL(k_pb_mask, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, d, w, n, A, b.col2.as<uint32_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t cbin[5] = {0, 0, 0, 0, 0};
    FBG_TRY(pc_launch(ix, c, pd, min_score, cbin, what));
    FBG_TRY(px_record_end(ix));
    std::vector<uint32_t> first(n), second(n);
    FBG_HIP_TRY(ctx, hipMemcpyAsync(chain_off, c.off.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(first.data(), b.score.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(second.data(), c.score.p, n * 4, hipMemcpyDeviceToHost, st));
    if (row) FBG_HIP_TRY(ctx, hipMemcpyAsync(row, b.row.p, n * 4, hipMemcpyDeviceToHost, st));
    if (n_best_rows) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_best_rows, b.nbest.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&cbin[4], pd.ctr + 4, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bin[5], d.ctr + 5, 2 * 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    // the chain of the chosen row, found again by the chain DP on the masked columns, has the score the row was chosen for
    for (uint64_t R = 0; R < n; R++)
        if (first[R] != second[R])
            return fbg_fail(ctx, FBG_ERR_HIP, "%s: read %llu scores %u along its row and %u on the masked columns", what,
                            (unsigned long long)R, first[R], second[R]);
    if (score) std::copy(first.begin(), first.end(), score);
    FBG_TRY(pc_finish(ix, c, chain_off, cbin, what));
    b.stat[0] = bin[1];
    b.stat[1] = bin[2];
    b.stat[2] = bin[3];
    b.stat[3] = bin[5];
    b.stat[4] = bin[6];
    px_finish(ix, PS_CHAINS);
    px_finish(ix, PS_BYROW);
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_by_row_stats(const fbg_pindex *ix, uint64_t *reads_lds, uint64_t *reads_device, uint64_t *reads_too_many,
                                              uint64_t *reads_no_row, uint64_t *anchors_kept, uint64_t *lds_max, uint64_t *max_places)
{
    if (!ix) return FBG_ERR_INVALID;
    const PbState &b = ix->pb;
    uint64_t *out[5] = {reads_lds, reads_device, reads_too_many, reads_no_row, anchors_kept};
    for (int k = 0; k < 5; k++)
        if (out[k]) *out[k] = px_current(ix, PS_BYROW) ? b.stat[k] : 0;
    if (lds_max) *lds_max = PB_LDS;
    if (max_places) *max_places = ix->ctx->opt.byrow_max < 0 ? 0 : (uint64_t)ix->ctx->opt.byrow_max;
    return FBG_OK;
}
