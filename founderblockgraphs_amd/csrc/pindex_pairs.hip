// pindex_pairs.hip -- paired reads: per virtual read a rescue chain on the start places inside the insert window that its
// partner's primary chain opens, per pair the best of four candidate combinations, and optionally the chosen chains put
// into ix->ch, so that every later stage runs on pair-consistent chains (fbg_pindex_chains_pairs).
//
// After fbg_pindex_seeds_strands on n given reads, n even, pair p is the given reads a = 2p and b = 2p + 1.  Virtual read
// v < n is read v as given, v >= n the reverse complement of read v - n; twin(v) = v +- n; partner(v), the twin of v's
// mate, is (v ^ 1) + n for v < n and (v - n) ^ 1 for v >= n.  V = 2n virtual reads, P = n / 2 pairs.
//
//   k_pp_span                        per virtual read lo and hi of a chain, from the first and last entry of a chain output
//                                    (k_pq_span's like; run on the primary chains and on the rescue chains);
//   k_pp_mask                        per start place its witness column, or none outside the window of its read;
//   k_pp_pick                        per pair the valid candidate of the largest score, and what adopt does with its four reads;
//   k_pp_adopt_read / _adopt_pred    adopt: end and score per virtual read, pred per start place, into ix->ch.
// Between k_pp_mask and the second k_pp_span the chain kernels of pindex_chain.hip run on the masked columns, in a chain
// state of the pairs state's own (pc_reserve, pc_launch, pc_finish); after the adopt kernels pc_trace runs on ix->ch.
#include "pindex_dev.h"

struct PpDev {
    const uint64_t *seed_off, *start_off;     // reads -> seeds -> start places
    const uint32_t *k, *col;                  // per seed its length; per start place its witness column (unmasked)
    const uint32_t *pscore, *rscore;          // [V] the primary and the rescue scores
    uint64_t *span;                           // [4 V] lo, hi per virtual read: the primary chains, then the rescue chains
    unsigned long long *ctr;                  // PP_CTR counters
    uint64_t V, S, A, min_insert, max_insert;
};

__device__ __forceinline__ uint64_t pp_partner(uint64_t v, uint64_t n) { return v < n ? (v ^ 1) + n : (v - n) ^ 1; }

// One lane per virtual read: lo = c(a_1), hi = c(a_len) + k(a_len) of its chain in (off, place, seed); PQ_NOSPAN in lo for
// an empty chain.  lo32 / hi32 (may be NULL): the same as u32, PC_NONE in both for an empty chain.
__global__ void k_pp_span(PpDev d, const uint64_t *off, const uint32_t *place, const uint32_t *seed, uint64_t *span, uint32_t *lo32,
                          uint32_t *hi32)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R >= d.V) return;
    const uint64_t o0 = off[R], o1 = off[R + 1];
    uint64_t lo = PQ_NOSPAN, hi = 0;
    if (o1 > o0) {
        const uint32_t g0 = place[o0], g1 = place[o1 - 1], t1 = seed[o1 - 1];
        if (g0 < d.A && g1 < d.A && t1 < d.S) {
            lo = d.col[g0];
            hi = (uint64_t)d.col[g1] + d.k[t1];
        }
    }
    span[2 * R] = lo;
    span[2 * R + 1] = hi;
    if (lo32) {
        lo32[R] = lo == PQ_NOSPAN ? PC_NONE : (uint32_t)lo;
        hi32[R] = lo == PQ_NOSPAN ? PC_NONE : (uint32_t)hi;
    }
}

// One lane per start place g of virtual read w: its seed by a search of start_off, w by a search of seed_off, v = partner(w).
// The window W of w is empty where v has no primary chain, [lo(v), lo(v) + max_insert) for v < n (v is the forward mate)
// and [hi(v) - max_insert, hi(v)) with the lower end clamped at 0 for v >= n; the sum saturates at 2^64 - 1, above every
// c + k.  mcol[g] = col[g] iff col[g] is a column, c >= W.lo and c + k <= W.hi, else none.  Places kept, and places with a
// column that are not kept, are counted per wave.
__global__ __launch_bounds__(PX_THREADS) void k_pp_mask(PpDev d, uint32_t *mcol)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int what = -1;                     // 0: kept, 1: excluded
    if (g < d.A) {
        const uint64_t n = d.V / 2;
        const uint64_t t = po_find(d.start_off, 0, d.S - 1, g);
        const uint64_t w = po_find(d.seed_off, 0, d.V - 1, t);
        const uint64_t v = pp_partner(w, n);
        const uint32_t c = d.col[g];
        const uint64_t lo = d.span[2 * v], hi = d.span[2 * v + 1];
        bool keep = false;
        if (c != PC_NONE) {
            if (lo != PQ_NOSPAN) {
                const uint64_t wlo = v < n ? lo : hi > d.max_insert ? hi - d.max_insert : 0;
                const uint64_t whi = v < n ? pq_add_sat(lo, d.max_insert) : hi;
                keep = (uint64_t)c >= wlo && (uint64_t)c + d.k[t] <= whi;
            }
            what = keep ? 0 : 1;
        }
        mcol[g] = keep ? c : PC_NONE;
    }
    for (int b = 0; b < 2; b++) {
        const unsigned long long m = __ballot(what == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[5 + b], (unsigned long long)__popcll(m));
    }
}

// One lane per pair p, a = 2p, b = 2p + 1.  Candidate i = 0 .. 3 is (F, R) = (primary(a), rescue(b + n)), (rescue(a),
// primary(b + n)), (primary(b), rescue(a + n)), (rescue(b), primary(a + n)); it is valid iff both chains are non-empty,
// lo(F) <= lo(R), hi(F) <= hi(R) and min_insert <= hi(R) - lo(F) <= max_insert, and scores s(F) + s(R).  The valid one of
// the largest score wins, the smallest i among equals.  pick: pair_score, then t_lo = lo(F), then t_hi = hi(R) (P each).
// src: the chosen reads get PP_PRIMARY or PP_RESCUE, their twins PP_TWIN; all four PP_KEEP without a valid candidate.
__global__ void k_pp_pick(PpDev d, uint8_t *which, uint32_t *pick, uint8_t *src)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = d.V / 2, P = d.V / 4;
    int out = -1, differs = 0;
    if (p < P) {
        const uint64_t a = 2 * p, b = 2 * p + 1;
        uint64_t best = 0, blo = 0, bhi = 0;
        int bi = -1;
        for (int i = 0; i < 4; i++) {
            const uint64_t fv = i < 2 ? a : b, rv = (i < 2 ? b : a) + n;
            const uint64_t *sf = d.span + ((i & 1) ? 2 * d.V : 0) + 2 * fv, *sr = d.span + ((i & 1) ? 0 : 2 * d.V) + 2 * rv;
            const uint64_t flo = sf[0], fhi = sf[1], rlo = sr[0], rhi = sr[1];
            if (flo == PQ_NOSPAN || rlo == PQ_NOSPAN) continue;
            if (flo > rlo || fhi > rhi || rhi < flo) continue;
            const uint64_t ins = rhi - flo;
            if (ins < d.min_insert || ins > d.max_insert) continue;
            const uint64_t sc = (uint64_t)((i & 1) ? d.rscore[fv] : d.pscore[fv]) + ((i & 1) ? d.pscore[rv] : d.rscore[rv]);
            if (bi < 0 || sc > best) { best = sc; bi = i; blo = flo; bhi = rhi; }
        }
        out = bi < 0 ? 4 : bi;
        which[p] = bi < 0 ? (uint8_t)PP_NOPAIR : (uint8_t)bi;
        pick[p] = bi < 0 ? 0 : (uint32_t)best;
        pick[P + p] = bi < 0 ? PC_NONE : (uint32_t)blo;
        pick[2 * P + p] = bi < 0 ? PC_NONE : (uint32_t)bhi;
        if (bi < 0) {
            src[a] = src[b] = src[a + n] = src[b + n] = PP_KEEP;
        } else {
            const uint64_t fv = bi < 2 ? a : b, rv = (bi < 2 ? b : a) + n, w = (bi & 1) ? fv : rv;
            src[fv] = (bi & 1) ? PP_RESCUE : PP_PRIMARY;
            src[rv] = (bi & 1) ? PP_PRIMARY : PP_RESCUE;
            src[fv + n] = src[rv - n] = PP_TWIN;
            differs = d.rscore[w] != d.pscore[w];
        }
    }
    for (int b = 0; b < 5; b++) {
        const unsigned long long m = __ballot(out == b);
        if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[b], (unsigned long long)__popcll(m));
    }
    const unsigned long long m = __ballot(differs);
    if (m && (threadIdx.x & (FBG_WAVE - 1)) == 0) atomicAdd(&d.ctr[7], (unsigned long long)__popcll(m));
}

// Adopt, one lane per virtual read: end and score of ix->ch by src.  PP_KEEP: a chain that min_score had emptied (old off)
// loses its end, so that the trace with min_score 0 leaves it empty; its score stays.  PP_PRIMARY: nothing.  PP_RESCUE:
// end and score of the rescue chain.  PP_TWIN: no end, score 0.
__global__ void k_pp_adopt_read(uint64_t V, const uint8_t *src, const uint64_t *poff, const uint32_t *rend, const uint32_t *rscore,
                                uint32_t *cend, uint32_t *cscore)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint8_t s = src[v];
    if (s == PP_KEEP) {
        if (poff[v + 1] == poff[v]) cend[v] = PC_NONE;
    } else if (s == PP_RESCUE) {
        cend[v] = rend[v];
        cscore[v] = rscore[v];
    } else if (s == PP_TWIN) {
        cend[v] = PC_NONE;
        cscore[v] = 0;
    }
}

// Adopt, one lane per start place: the predecessor of the rescue run where its read takes the rescue chain.
__global__ __launch_bounds__(PX_THREADS) void k_pp_adopt_pred(PpDev d, const uint8_t *src, const uint32_t *rpred, uint32_t *cpred)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.A) return;
    const uint64_t t = po_find(d.start_off, 0, d.S - 1, g);
    const uint64_t w = po_find(d.seed_off, 0, d.V - 1, t);
    if (src[w] == PP_RESCUE) cpred[g] = rpred[g];
}

// ---- fbg_pindex_chains_pairs -----------------------------------------------------------------------------------------
// The witness columns into the pairs state's own buffer (k_po_expand_msa<true>: the masked columns of a by-row call play
// no part), k_pp_span on the primary chains, k_pp_mask, the chain kernels on the masked columns with the band of the primary
// call and min_score 0, k_pp_span on the rescue chains, k_pp_pick.  Without adopt nothing of ix->ch is written and no stage
// goes stale.  With adopt: px_begin(PS_CHAINS), the two adopt kernels, pc_trace on ix->ch with min_score 0, px_finish.
extern "C" int fbg_pindex_chains_pairs(fbg_pindex *ix, uint64_t min_insert, uint64_t max_insert, uint8_t *which, uint32_t *pair_score,
                                       uint32_t *t_lo, uint32_t *t_hi, uint64_t *rescue_off, uint32_t *rescue_score, uint32_t *rescue_lo,
                                       uint32_t *rescue_hi, uint32_t *rescue_place, uint32_t *rescue_seed, uint64_t *adopt_chain_off,
                                       uint32_t *adopt_score, uint64_t stats[8], double *device_ms)
{
    static const char *const what = "fbg_pindex_chains_pairs";
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PpState &q = ix->pp;
    PcState &c = ix->ch;
    const PoState &s = ix->sd;
    if (device_ms) *device_ms = 0;
    if (!which || !rescue_off) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing which or rescue_off", what);
    if (!ix->from_segmentation || !ix->has_map)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation knows MSA columns", what);
    FBG_TRY(px_need(ix, what, PS_SEEDS));
    if (!ix->batch.stranded) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: the last seeds call was no fbg_pindex_seeds_strands", what);
    FBG_TRY(px_need(ix, what, PS_CHAINS));
    const uint64_t V = ix->batch.n, n = V / 2, P = n / 2, S = s.n, A = s.stotal;
    if (n % 2) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: %llu reads; pairs take an even number, mates interleaved", what, (unsigned long long)n);
    if (min_insert > max_insert)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: min_insert %llu above max_insert %llu", what, (unsigned long long)min_insert,
                        (unsigned long long)max_insert);
    const bool adopt = adopt_chain_off != nullptr;
    if (adopt) px_begin(ix, PS_CHAINS);      // with everything made from the chains
    std::fill(which, which + P, (uint8_t)PP_NOPAIR);
    if (pair_score) std::fill(pair_score, pair_score + P, (uint32_t)0);
    if (t_lo) std::fill(t_lo, t_lo + P, (uint32_t)PC_NONE);
    if (t_hi) std::fill(t_hi, t_hi + P, (uint32_t)PC_NONE);
    std::fill(rescue_off, rescue_off + V + 1, (uint64_t)0);
    if (rescue_score) std::fill(rescue_score, rescue_score + V, (uint32_t)0);
    if (rescue_lo) std::fill(rescue_lo, rescue_lo + V, (uint32_t)PC_NONE);
    if (rescue_hi) std::fill(rescue_hi, rescue_hi + V, (uint32_t)PC_NONE);
    if (stats) { std::fill(stats, stats + PP_CTR, (uint64_t)0); stats[4] = P; }
    if (n == 0 || S == 0 || A == 0) {        // no start place: every chain is empty, and stays so
        if (adopt) {
            std::fill(adopt_chain_off, adopt_chain_off + V + 1, (uint64_t)0);
            if (adopt_score) std::fill(adopt_score, adopt_score + V, (uint32_t)0);
            px_finish(ix, PS_CHAINS);
        }
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, q.span, 4 * V * 8));
    FBG_TRY(px_reserve(ix, q.mcol, A * 4));
    FBG_TRY(px_reserve(ix, q.rspan, 2 * V * 4));
    FBG_TRY(px_reserve(ix, q.pick, 3 * P * 4));
    FBG_TRY(px_reserve(ix, q.which, P));
    FBG_TRY(px_reserve(ix, q.src, V));
    FBG_TRY(px_reserve(ix, q.ctr, PP_CTR * 8));
    PcDev pd;
    FBG_TRY(pc_reserve(ix, q.ch, pd, q.mcol.as<uint32_t>(), c.band));
    q.ch.n = V;
    PpDev d;
    d.seed_off = ix->soff.as<uint64_t>();
    d.start_off = s.soff.as<uint64_t>();
    d.k = ix->slen.as<uint32_t>();
    d.col = q.ch.col.as<uint32_t>() + A;
    d.pscore = c.score.as<uint32_t>();
    d.rscore = q.ch.score.as<uint32_t>();
    d.span = q.span.as<uint64_t>();
    d.ctr = q.ctr.as<unsigned long long>();
    d.V = V;
    d.S = S;
    d.A = A;
    d.min_insert = min_insert;
    d.max_insert = max_insert;
    const uint32_t *pout = c.out.as<uint32_t>(), *rout = q.ch.out.as<uint32_t>();
    uint32_t *rspan = q.rspan.as<uint32_t>(), *pick = q.pick.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(q.ctr.p, 0, PP_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(q.ch.ctr.p, 0, 5 * 8, st));
    po_expand_msa(ix, s, true, q.ch.col.as<uint32_t>(), q.ch.col.as<uint32_t>() + A);
    hipLaunchKernelGGL(k_pp_span, dim3(fbg_blocks(V, 256)), dim3(256), 0, st, d, (const uint64_t *)c.off.as<uint64_t>(), pout, pout + S,
                       d.span, (uint32_t *)nullptr, (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_pp_mask, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, d, q.mcol.as<uint32_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t bin[5] = {0, 0, 0, 0, 0};
    FBG_TRY(pc_launch(ix, q.ch, pd, 0, bin, what));
    hipLaunchKernelGGL(k_pp_span, dim3(fbg_blocks(V, 256)), dim3(256), 0, st, d, (const uint64_t *)q.ch.off.as<uint64_t>(), rout, rout + S,
                       d.span + 2 * V, rspan, rspan + V);
    hipLaunchKernelGGL(k_pp_pick, dim3(fbg_blocks(P, 256)), dim3(256), 0, st, d, q.which.as<uint8_t>(), pick, q.src.as<uint8_t>());
    FBG_HIP_TRY(ctx, hipGetLastError());
    if (adopt) {
        PcDev cd;
        FBG_TRY(pc_reserve(ix, c, cd, nullptr, c.band));
        hipLaunchKernelGGL(k_pp_adopt_read, dim3(fbg_blocks(V, 256)), dim3(256), 0, st, V, (const uint8_t *)q.src.as<uint8_t>(),
                           (const uint64_t *)c.off.as<uint64_t>(), (const uint32_t *)q.ch.end.as<uint32_t>(), d.rscore,
                           c.end.as<uint32_t>(), c.score.as<uint32_t>());
        hipLaunchKernelGGL(k_pp_adopt_pred, dim3(fbg_blocks(A, PX_THREADS)), dim3(PX_THREADS), 0, st, d, (const uint8_t *)q.src.as<uint8_t>(),
                           (const uint32_t *)q.ch.pred.as<uint32_t>(), c.pred.as<uint32_t>());
        FBG_HIP_TRY(ctx, hipGetLastError());
        FBG_TRY(pc_trace(ix, c, cd, 0));
    }
    FBG_TRY(px_record_end(ix));
    uint64_t ctr[PP_CTR] = {0, 0, 0, 0, 0, 0, 0, 0};
    FBG_HIP_TRY(ctx, hipMemcpyAsync(which, q.which.p, P, hipMemcpyDeviceToHost, st));
    if (pair_score) FBG_HIP_TRY(ctx, hipMemcpyAsync(pair_score, pick, P * 4, hipMemcpyDeviceToHost, st));
    if (t_lo) FBG_HIP_TRY(ctx, hipMemcpyAsync(t_lo, pick + P, P * 4, hipMemcpyDeviceToHost, st));
    if (t_hi) FBG_HIP_TRY(ctx, hipMemcpyAsync(t_hi, pick + 2 * P, P * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_off, q.ch.off.p, (V + 1) * 8, hipMemcpyDeviceToHost, st));
    if (rescue_score) FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_score, q.ch.score.p, V * 4, hipMemcpyDeviceToHost, st));
    if (rescue_lo) FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_lo, rspan, V * 4, hipMemcpyDeviceToHost, st));
    if (rescue_hi) FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_hi, rspan + V, V * 4, hipMemcpyDeviceToHost, st));
    if (adopt) {
        FBG_HIP_TRY(ctx, hipMemcpyAsync(adopt_chain_off, c.off.p, (V + 1) * 8, hipMemcpyDeviceToHost, st));
        if (adopt_score) FBG_HIP_TRY(ctx, hipMemcpyAsync(adopt_score, c.score.p, V * 4, hipMemcpyDeviceToHost, st));
    }
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ctr, q.ctr.p, PP_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&bin[4], pd.ctr + 4, 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    FBG_TRY(pc_finish(ix, q.ch, rescue_off, bin, what));
    const uint64_t total = rescue_off[V];
    if (total && (rescue_place || rescue_seed)) {
        if (rescue_place) FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_place, rout, total * 4, hipMemcpyDeviceToHost, st));
        if (rescue_seed) FBG_HIP_TRY(ctx, hipMemcpyAsync(rescue_seed, rout + S, total * 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (stats) std::copy(ctr, ctr + PP_CTR, stats);
    if (adopt) {
        if (adopt_chain_off[V] >= (1ull << 32))
            return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu chain entries; a call takes fewer than 2^32", what,
                            (unsigned long long)adopt_chain_off[V]);
        c.total = adopt_chain_off[V];
        px_finish(ix, PS_CHAINS);
    }
    return FBG_OK;
}
