// pindex_pairs_align.hip -- paired reads: a mate without a chain is aligned in the insert window that its partner's chain
// opens on the smallest row carrying that chain, and the pair is decided from the alignment (fbg_pindex_pairs_align).
//
// V = 2n virtual reads and P = n / 2 pairs, twin and partner as in pindex_pairs.hip.
//
//   k_pl_frag                        per virtual read the row r of its chain (what k_pr_chain chose) and the fragment ends
//                                    fs, fe along the diagonals of its first and last anchor;
//   k_pl_window                      per virtual read w the selection, the window of partner(w), the status and the block,
//                                    node and offset at which the window starts (k_pa_prepare's search);
//   k_pl_pick                        per pair the acceptance of its four possible aligned reads and the pick.
// Between k_pl_window and k_pl_pick the windows are gathered and aligned by k_pa_gather and k_pa_edit of pindex_align.hip
// (pa_windows), on buffers of this call's own.  Nothing of ix->al but the prefix table is written, and nothing of ix->ch,
// ix->pp or the row calls' outputs: no stage goes stale.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

struct PlDev {
    const uint64_t *off;              // [V + 1] the chains of ix->ch: offsets, places, and per start place its record
    const uint32_t *place;
    const uint4 *rec;
    const uint32_t *q, *score;        // per seed q_start; per virtual read the chain's score
    const uint8_t *select;            // [V] or NULL
    unsigned long long *ctr;          // PL_CTR counters
    uint64_t V, min_insert, max_insert, max_window;
    uint32_t max_edits;
};

__device__ __forceinline__ uint64_t pl_partner(uint64_t v, uint64_t n) { return v < n ? (v ^ 1) + n : (v - n) ^ 1; }

// One lane per virtual read v with a chain and a row r = first_row[v]: x = p(r, block(u)) + o of its first and last
// anchor, fs = max(0, x_1 - q_1), fe = min(|G_r|, x_last + L - q_last).  frag[v] = (r, fs, fe, |G_r|); r = PR_NONE for an
// empty chain and for a chain that no row carries.
__global__ void k_pl_frag(PaDev d, PlDev p, const uint32_t *first_row, uint4 *frag)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= p.V) return;
    const uint64_t o0 = p.off[v], len = p.off[v + 1] - o0;
    const uint32_t r = len ? first_row[v] : PR_NONE;
    uint4 f = make_uint4(r, 0, 0, 0);
    if (r != PR_NONE) {
        const uint4 a = p.rec[p.place[o0]], b = p.rec[p.place[o0 + len - 1]];
        const long long L = (long long)(d.roff[v + 1] - d.roff[v]);
        const long long x1 = (long long)d.pref[(uint64_t)a.w * d.m + r] + a.y - (long long)p.q[a.z];
        const long long x2 = (long long)d.pref[(uint64_t)b.w * d.m + r] + b.y - (long long)p.q[b.z] + L;
        const uint64_t jl = (d.nb - 1) * d.m + r;
        const uint32_t vl = d.node_of[jl];
        const long long glen = (long long)d.pref[jl] + (vl != PR_NONE ? (long long)(d.loff[vl + 1] - d.loff[vl]) : 0);
        f.y = x1 > 0 ? (uint32_t)x1 : 0;
        f.z = (uint32_t)(x2 < glen ? (x2 > 0 ? x2 : 0) : glen);
        f.w = (uint32_t)glen;
    }
    frag[v] = f;
}

// One lane per virtual read w (and one for the entry V of wlen), v = partner(w).  w is selected iff v's chain is non-empty
// and select[w] != 0, without select iff w's own chain is empty.  The window of a selected w on v's row r is
// [fs, min(|G_r|, fs + max_insert)) for v < n and [max(0, fe - max_insert), fe) for v >= n; kind: 0 aligned, 1 no row, 2 empty,
// 3 too long, 4 too wide, tested in this order.  info, start, wlen and out as k_pa_prepare leaves them: info.z = |W| for
// kind 0 and 0 else, out[w] = r for kinds 0 and 2 .. 4, PA_NONE in the three other outputs unless kind is 0.  ctr[0]: the
// selected reads, ctr[1 + kind], ctr[8]: the cells; summed per wave before the atomic.
__global__ void k_pl_window(PaDev d, PlDev p, const uint4 *frag, uint4 *info, uint4 *start, uint64_t *wlen, uint32_t *out)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t V = p.V, n = V / 2;
    int kind = -1;
    unsigned long long cells = 0;
    if (w == V) wlen[V] = 0;
    if (w < V) {
        const uint64_t v = pl_partner(w, n);
        const uint64_t L = d.roff[w + 1] - d.roff[w];
        const bool anchored = p.off[v + 1] != p.off[v];
        const bool sel = anchored && (p.select ? p.select[w] != 0 : p.off[w + 1] == p.off[w]);
        uint4 in = make_uint4(PR_NONE, 0, 0, (uint32_t)L), at = make_uint4(0, 0, 0, 0);
        if (sel) {
            const uint4 f = frag[v];
            const uint32_t r = f.x;
            if (r == PR_NONE) kind = 1;
            else {
                const uint64_t fs = f.y, fe = f.z, glen = f.w;
                const uint64_t w0 = v < n ? fs : fe > p.max_insert ? fe - p.max_insert : 0;
                const uint64_t w1 = v < n ? (fs + p.max_insert < glen ? fs + p.max_insert : glen) : fe;      // max_insert <= 2^33
                const uint64_t wl = w1 - w0;
                kind = L == 0 || wl == 0 ? 2 : L > PA_MAX_READ ? 3 : p.max_window && wl > p.max_window ? 4 : 0;
                in.x = r;
                if (kind == 0) {
                    uint64_t a = 0, b = d.nb - 1;
                    while (a < b) {
                        const uint64_t mid = a + (b - a + 1) / 2;
                        if (d.pref[mid * d.m + r] <= w0) a = mid; else b = mid - 1;
                    }
                    in.y = (uint32_t)w0;
                    in.z = (uint32_t)wl;
                    at = make_uint4((uint32_t)a, d.node_of[a * d.m + r], (uint32_t)w0 - d.pref[a * d.m + r], 0);
                    cells = (unsigned long long)L * wl;
                }
            }
        }
        info[w] = in;
        start[w] = at;
        wlen[w] = in.z;
        out[w] = in.x;
        if (kind != 0) out[V + w] = out[2 * V + w] = out[3 * V + w] = PA_NONE;
    }
    for (int o = FBG_WAVE / 2; o > 0; o >>= 1) cells += __shfl_xor(cells, o);
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    const unsigned long long any = __ballot(kind >= 0);
    if (any && first) atomicAdd(&p.ctr[0], (unsigned long long)__popcll(any));
    for (int b = 0; b < 5; b++) {
        const unsigned long long mk = __ballot(kind == b);
        if (mk && first) atomicAdd(&p.ctr[1 + b], (unsigned long long)__popcll(mk));
    }
    if (cells && first) atomicAdd(&p.ctr[8], cells);
}

// One lane per pair p, a = 2p, b = 2p + 1.  Candidate i = 0 .. 3 has the chained read v and the aligned read w: (a, b + n),
// (b + n, a), (b, a + n), (a + n, b); v < n for the even ones.  An aligned w has insert = t_end(w) - fs(v) for v < n and
// fe(v) - t_start(w) for v >= n, and is accepted iff edits <= max_edits and insert >= min_insert (rejections counted in
// this order: ctr[6], ctr[7]); ins[w] = insert where accepted, else PA_NONE.  A candidate is valid iff its w is accepted and
// scores score[v] + L_w - edits[w]; the largest score wins, the smallest i among equals.  pick: pair_score, then t_lo, then
// t_hi (P each): fs(v), t_end(w) for even i and t_start(w), fe(v) for odd i.  ctr[9]: pairs with a candidate.
__global__ void k_pl_pick(PaDev d, PlDev p, const uint4 *frag, const uint32_t *out, uint32_t *ins, uint8_t *which, uint32_t *pick)
{
    const uint64_t pr = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t V = p.V, n = V / 2, P = V / 4;
    unsigned long long by_edits = 0, by_insert = 0;
    bool found = false;
    if (pr < P) {
        const uint64_t a = 2 * pr, b = 2 * pr + 1;
        uint64_t best = 0;
        uint32_t blo = 0, bhi = 0;
        int bi = -1;
        for (int i = 0; i < 4; i++) {
            const uint64_t fwd = i < 2 ? a : b, rev = (i < 2 ? b : a) + n;
            const uint64_t v = (i & 1) ? rev : fwd, w = (i & 1) ? fwd : rev;
            const uint32_t e = out[V + w];
            uint32_t insert = PA_NONE;
            if (e != PA_NONE) {
                const uint4 f = frag[v];
                const uint32_t ts = out[2 * V + w], te = out[3 * V + w];
                const uint32_t got = (i & 1) ? f.z - ts : te - f.y;
                if (e > p.max_edits) by_edits++;
                else if (got < p.min_insert) by_insert++;
                else {
                    insert = got;
                    const uint64_t sc = (uint64_t)p.score[v] + (d.roff[w + 1] - d.roff[w]) - e;
                    if (bi < 0 || sc > best) {
                        best = sc;
                        bi = i;
                        blo = (i & 1) ? ts : f.y;
                        bhi = (i & 1) ? f.z : te;
                    }
                }
            }
            ins[w] = insert;
        }
        found = bi >= 0;
        which[pr] = found ? (uint8_t)bi : (uint8_t)PP_NOPAIR;
        pick[pr] = found ? (uint32_t)best : 0;
        pick[P + pr] = found ? blo : PC_NONE;
        pick[2 * P + pr] = found ? bhi : PC_NONE;
    }
    for (int o = FBG_WAVE / 2; o > 0; o >>= 1) {
        by_edits += __shfl_xor(by_edits, o);
        by_insert += __shfl_xor(by_insert, o);
    }
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    const unsigned long long mk = __ballot(found);
    if (by_edits && first) atomicAdd(&p.ctr[6], by_edits);
    if (by_insert && first) atomicAdd(&p.ctr[7], by_insert);
    if (mk && first) atomicAdd(&p.ctr[9], (unsigned long long)__popcll(mk));
}

// ---- fbg_pindex_pairs_align ------------------------------------------------------------------------------------------
// pr_prepare and k_pr_chain as in fbg_pindex_chains_align (into buffers of this state, so that call's results stay), the
// prefix table where no call has built it, k_pl_frag, k_pl_window, a scan of the window lengths, the host's look at their
// sum, the windows gathered and aligned over all V reads (a wave of a read that is not aligned returns at once), k_pl_pick.
extern "C" int fbg_pindex_pairs_align(fbg_pindex *ix, uint64_t min_insert, uint64_t max_insert, uint32_t max_edits, uint64_t max_window,
                                      const uint8_t *select, uint32_t *row, uint32_t *edits, uint32_t *t_start, uint32_t *t_end,
                                      uint32_t *insert, uint8_t *which, uint32_t *pair_score, uint32_t *t_lo, uint32_t *t_hi,
                                      uint64_t stats[10], double *device_ms)
{
    static const char *const what = "fbg_pindex_pairs_align";
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PlState &s = ix->pl;
    PaState &al = ix->al;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (!which) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: missing which", what);
    if (!ix->has_rows)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: only an index built by fbg_pindex_build_segmentation_rows has the row table", what);
    FBG_TRY(px_need(ix, what, PS_SEEDS));
    if (!ix->batch.stranded) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: the last seeds call was no fbg_pindex_seeds_strands", what);
    FBG_TRY(px_need(ix, what, PS_CHAINS));
    const uint64_t V = ix->batch.n, n = V / 2, P = n / 2;
    if (n % 2) return fbg_fail(ctx, FBG_ERR_INVALID, "%s: %llu reads; pairs take an even number, mates interleaved", what, (unsigned long long)n);
    if (min_insert > max_insert)
        return fbg_fail(ctx, FBG_ERR_INVALID, "%s: min_insert %llu above max_insert %llu", what, (unsigned long long)min_insert,
                        (unsigned long long)max_insert);
    if (V > 0x7fffffffull)        // a wave, and so a workgroup, per virtual read
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "%s: %llu virtual reads; a call takes fewer than 2^31", what, (unsigned long long)V);
    uint32_t *host[5] = {row, edits, t_start, t_end, insert};
    for (uint32_t *h : host)
        if (h) std::fill(h, h + V, (uint32_t)PA_NONE);
    std::fill(which, which + P, (uint8_t)PP_NOPAIR);
    if (pair_score) std::fill(pair_score, pair_score + P, (uint32_t)0);
    if (t_lo) std::fill(t_lo, t_lo + P, (uint32_t)PC_NONE);
    if (t_hi) std::fill(t_hi, t_hi + P, (uint32_t)PC_NONE);
    if (stats) std::fill(stats, stats + 10, (uint64_t)0);
    if (n == 0 || c.total == 0) return FBG_OK;        // every chain is empty: nobody opens a window
    if (max_insert > (1ull << 33)) max_insert = 1ull << 33;      // positions are below 2^32: beyond this no window changes
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, al.pref, ix->seg_nb * ix->rw.m * 4));
    FBG_TRY(px_reserve(ix, s.nrows, 2 * V * 4));
    for (DevBuf *b : {&s.frag, &s.info, &s.start, &s.out}) FBG_TRY(px_reserve(ix, *b, V * 16));
    for (DevBuf *b : {&s.wlen, &s.woff}) FBG_TRY(px_reserve(ix, *b, (V + 1) * 8));
    FBG_TRY(px_reserve(ix, s.ins, V * 4));
    FBG_TRY(px_reserve(ix, s.pick, 3 * P * 4));
    FBG_TRY(px_reserve(ix, s.which, P));
    FBG_TRY(px_reserve(ix, s.ctr, PL_CTR * 8));
    if (select) FBG_TRY(px_reserve(ix, s.sel, V));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));                       // records ev0
    FBG_TRY(pa_prefix(ix));
    const PaDev a = pa_dev(ix);
    if (select) FBG_HIP_TRY(ctx, hipMemcpyAsync(s.sel.p, select, V, hipMemcpyHostToDevice, st));
    PlDev p;
    p.off = c.off.as<uint64_t>();
    p.place = c.out.as<uint32_t>();
    p.rec = ix->rw.rec.as<uint4>();
    p.q = ix->sq.as<uint32_t>();
    p.score = c.score.as<uint32_t>();
    p.select = select ? s.sel.as<uint8_t>() : nullptr;
    p.ctr = s.ctr.as<unsigned long long>();
    p.V = V;
    p.min_insert = min_insert;
    p.max_insert = max_insert;
    p.max_window = max_window;
    p.max_edits = max_edits;
    FBG_HIP_TRY(ctx, hipMemsetAsync(p.ctr, 0, PL_CTR * 8, st));
    uint32_t *nr = s.nrows.as<uint32_t>(), *out = s.out.as<uint32_t>(), *pick = s.pick.as<uint32_t>();
    uint4 *frag = s.frag.as<uint4>();
    uint64_t *wlen = s.wlen.as<uint64_t>(), *woff = s.woff.as<uint64_t>();
    pr_chain_launch(ix, d, V, 0, nr, nr + V, nullptr, p.ctr + 10);
    hipLaunchKernelGGL(k_pl_frag, dim3(fbg_blocks(V, 256)), dim3(256), 0, st, a, p, (const uint32_t *)(nr + V), frag);
    hipLaunchKernelGGL(k_pl_window, dim3(fbg_blocks(V + 1, 256)), dim3(256), 0, st, a, p, (const uint4 *)frag, s.info.as<uint4>(),
                       s.start.as<uint4>(), wlen, out);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, wlen, woff, (uint64_t)0, (size_t)(V + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, woff + V, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (total) {
        FBG_TRY(px_reserve(ix, s.win, total));
        pa_windows(ix, a, V, s.info.as<uint4>(), s.start.as<uint4>(), woff, s.win.as<uint8_t>(), out);
    }
    hipLaunchKernelGGL(k_pl_pick, dim3(fbg_blocks(P, 256)), dim3(256), 0, st, a, p, (const uint4 *)frag, (const uint32_t *)out,
                       s.ins.as<uint32_t>(), s.which.as<uint8_t>(), pick);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(px_record_end(ix));
    uint64_t ctr[PL_CTR] = {};
    for (int k = 0; k < 4; k++)
        if (host[k]) FBG_HIP_TRY(ctx, hipMemcpyAsync(host[k], out + k * V, V * 4, hipMemcpyDeviceToHost, st));
    if (insert) FBG_HIP_TRY(ctx, hipMemcpyAsync(insert, s.ins.p, V * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(which, s.which.p, P, hipMemcpyDeviceToHost, st));
    if (pair_score) FBG_HIP_TRY(ctx, hipMemcpyAsync(pair_score, pick, P * 4, hipMemcpyDeviceToHost, st));
    if (t_lo) FBG_HIP_TRY(ctx, hipMemcpyAsync(t_lo, pick + P, P * 4, hipMemcpyDeviceToHost, st));
    if (t_hi) FBG_HIP_TRY(ctx, hipMemcpyAsync(t_hi, pick + 2 * P, P * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(ctr, p.ctr, PL_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    if (stats) std::copy(ctr, ctr + 10, stats);
    al.has_pref = true;
    return FBG_OK;
}
