// pindex_gcigar.hip -- the alignment path of each read against the stretch of the graph that its path spells
// (fbg_pindex_chains_graph_cigar / _graph_cigar_fetch / fbg_pindex_graph_cigar_stats).
//
//   k_pj_sizes    per read of the last graph call N, the length of T = spell(path)[start_offset : up to end_offset in
//                 the end node], from the label lengths of its path, and the read in the shape the row call's kernels take;
//   k_pj_gather   a wave per read: T label by label, the first and the last node clipped, into one text buffer;
// then pg_trace of pindex_align.hip on these (P, T): k_pg_sizes, k_pg_path per tier and batch, k_pg_compact.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

// One lane per read of the last graph call (and one for the entry n of wlen).  gout, goff, gpath, ginfo: what that call
// left (PhState out, off, path, info).  A read with a result gets info = (0, 0, N, L), out[n + R] = edits, out[2 n + R] = 0,
// out[3 n + R] = N and wlen[R] = N; every other read info.w = 0, out[n + R] = PA_NONE and wlen[R] = 0.  A path that spells no
// stretch between its two offsets, or one of more than L + edits symbols (lev(P, T) == edits allows no more), is counted in
// *bad and treated as no result: the LDS of k_pg_path is sized by N <= 2 L.  The loop is bounded by n_path.
__global__ void k_pj_sizes(const uint64_t *loff, const uint4 *ginfo, const uint32_t *gout, const uint64_t *goff, const uint32_t *gpath,
                           uint64_t n, uint4 *info, uint32_t *out, uint64_t *wlen, unsigned long long *bad)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R > n) return;
    if (R == n) { wlen[n] = 0; return; }
    const uint32_t edits = gout[R], L = ginfo[R].z;
    const uint64_t o = goff[R], k = goff[R + 1] - o;
    uint32_t N = 0;
    bool have = edits != PA_NONE && L != 0 && k != 0;
    if (have) {
        uint64_t sum = 0, head = 0, tail = 0;
        for (uint64_t x = 0; x < k; x++) {
            const uint32_t v = gpath[o + x];
            tail = loff[v + 1] - loff[v];
            if (x == 0) head = tail;
            sum += tail;
        }
        const uint64_t so = gout[2 * n + R], eo = gout[4 * n + R], end = sum - tail + eo;
        if (so > head || eo > tail || end < so || end - so > (uint64_t)L + edits) {
            atomicAdd(bad, 1ull);
            have = false;
        } else
            N = (uint32_t)(end - so);
    }
    info[R] = make_uint4(0, 0, N, have ? L : 0);
    out[R] = 0;
    out[n + R] = have ? edits : PA_NONE;
    out[2 * n + R] = 0;
    out[3 * n + R] = N;
    wlen[R] = N;
}

// A wave per read writes its T to text + woff[R]: the labels of its path one after the other, the lanes along the bytes
// of a label; the first label from start_offset on, and the last cut where N symbols are written.  Bounded by n_path
// labels and N symbols.
__global__ __launch_bounds__(FBG_WAVE) void k_pj_gather(const uint8_t *labels, const uint64_t *loff, const uint4 *info, const uint32_t *gout,
                                                       const uint64_t *goff, const uint32_t *gpath, uint64_t n, const uint64_t *woff,
                                                       uint8_t *text)
{
    const uint64_t R = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint32_t N = info[R].z;
    if (N == 0) return;
    const uint64_t o = goff[R], k = goff[R + 1] - o;
    uint8_t *dst = text + woff[R];
    uint32_t done = 0;
    for (uint64_t x = 0; x < k && done < N; x++) {
        const uint32_t v = gpath[o + x];
        const uint64_t a = loff[v] + (x == 0 ? gout[2 * n + R] : 0), b = loff[v + 1];
        if (a >= b) continue;
        const uint32_t take = b - a < (uint64_t)(N - done) ? (uint32_t)(b - a) : N - done;
        for (uint32_t t = lane; t < take; t += FBG_WAVE) dst[done + t] = labels[a + t];
        done += take;
    }
}

// k_pj_sizes, a scan of N, the host's look at its sum and at the bad paths, the gather into a text of that size, and
// pg_trace on the result, which ends the device time that ev0 starts here.
extern "C" int fbg_pindex_chains_graph_cigar(fbg_pindex *ix, uint32_t *n_ops, uint64_t *total_ops, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PhState &gr = ix->gr;
    PjState &j = ix->gj;
    const char *who = "fbg_pindex_chains_graph_cigar";
    FBG_TRY(px_need_rows(ix, who, PS_GRAPH));
    const uint64_t n = gr.n;
    if (n == 0 || !gr.on_device)              // no reads, or every chain empty: nothing of that graph call on the device
        return pg_trace(ix, nullptr, j.g, PS_GCIGAR, n, false, n_ops, total_ops, device_ms, who);
    if (device_ms) *device_ms = 0;
    if (total_ops) *total_ops = 0;
    px_begin(ix, PS_GCIGAR);
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, j.info, n * 16));
    FBG_TRY(px_reserve(ix, j.out, 4 * n * 4));
    for (DevBuf *b : {&j.wlen, &j.woff}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    FBG_TRY(px_reserve(ix, j.bad, 8));
    const uint8_t *labels = ix->rw.labels.as<uint8_t>();
    const uint64_t *loff = ix->rw.loff.as<uint64_t>(), *goff = gr.off.as<uint64_t>();
    const uint32_t *gout = gr.out.as<uint32_t>(), *gpath = gr.path.as<uint32_t>();
    uint64_t *wlen = j.wlen.as<uint64_t>(), *woff = j.woff.as<uint64_t>();
    auto *bad = j.bad.as<unsigned long long>();
    FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(bad, 0, 8, st));
    hipLaunchKernelGGL(k_pj_sizes, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, loff, (const uint4 *)gr.info.as<uint4>(), gout, goff, gpath, n,
                       j.info.as<uint4>(), j.out.as<uint32_t>(), wlen, bad);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, wlen, woff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    unsigned long long nbad = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, woff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&nbad, bad, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nbad)
        return fbg_fail(ctx, FBG_ERR_HIP, "%s: the paths of %llu reads spell no stretch of at most L + edits symbols", who, nbad);
    FBG_TRY(px_reserve(ix, j.text, total + 1));
    if (total) {
        hipLaunchKernelGGL(k_pj_gather, dim3((unsigned)n), dim3(FBG_WAVE), 0, st, labels, loff, (const uint4 *)j.info.as<uint4>(), gout, goff, gpath,
                           n, (const uint64_t *)woff, j.text.as<uint8_t>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    const PgIn in = {j.info.as<uint4>(), woff, j.text.as<uint8_t>(), j.out.as<uint32_t>()};
    return pg_trace(ix, &in, j.g, PS_GCIGAR, n, true, n_ops, total_ops, device_ms, who);
}

extern "C" int fbg_pindex_chains_graph_cigar_fetch(fbg_pindex *ix, uint64_t *off, uint32_t *ops)
{
    if (!ix) return FBG_ERR_INVALID;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_graph_cigar_fetch", PS_GCIGAR));
    return pg_fetch(ix, ix->gj.g, off, ops);
}

extern "C" int fbg_pindex_graph_cigar_stats(const fbg_pindex *ix, uint64_t *paths, uint64_t *ops, uint64_t *columns, uint64_t *history_bytes,
                                            uint64_t *batches)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_graph_cigar_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    uint64_t *o[5] = {paths, ops, columns, history_bytes, batches};
    for (int k = 0; k < 5; k++)
        if (o[k]) *o[k] = ix->gj.g.stat[k];
    return FBG_OK;
}
