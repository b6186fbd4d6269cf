// dp.hip -- the three segmentation recurrences and their backtracks, on the device.
//
//  * fbg_dp_minmax:     sort of (x, f[x]+1) by second + min-max-length sweep + backtrack of
//                       segment_elastic_minmaxlength (fbg.cpp:1940-2039);
//  * fbg_dp_repeatfree: s[]/prev[] recurrence + backtrack of segment() (fbg.cpp:616-664);
//  * fbg_dp_gapped:     segment2elasticValid (fbg.cpp:738-866).
//
// Where the families of sweeps live:
//   dp_plan.h      which sweeps fbg_dp_minmax tries and in which order (host only; the rule of DESIGN.md 6)
//   dp_bytes.hip   byte matrices, windows of 64 .. 256 columns: the BYTES rungs, and the chain fbg_dp_repeatfree runs on
//   dp_wide.hip    16-bit matrices, windows of 1024 .. 16384 columns: the WIDE rungs
//   dp.hip         keys and buckets, the wave and the literal sweep (WAVE, LITERAL), the backtracks, the three entry points,
//                  the non-elastic and the gapped kernels
//   dp_dev.h       the device pieces two of these files share
//   dp_host.h      the host pieces they share: the state of a sweep, the rungs' declarations, dp_for_R
// The words of the DPs' scratch (FbgScalars::dp) are named in fbg_internal.h (DP_COUNT .. DP_NE).
//
// The std::sort (fbg.cpp:1953) is a counting sort here: a histogram of f[x]+1, an exclusive scan
// and a scatter.  Ties may land in any order; the sweep's outcome does not depend on it, because
// every update inside one step j is a strict min/max over distinct x or a counter.
// The literal sweep itself is inherently sequential (step j reads minmaxlength[] of earlier columns); one
// lane walks it with all state in device memory, exactly the statements of fbg.cpp:1968-2014.
#include "dp_host.h"
#include "dp_dev.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>

// e[x] = f[x] + 1, the count of entries outside [x, n] and the longest minimal extension (one atomic each per workgroup)
__global__ __launch_bounds__(256) void k_dp_keys(const uint64_t *__restrict__ f, uint64_t n, uint32_t *__restrict__ e,
                                                 unsigned long long *__restrict__ bad)
{
    __shared__ unsigned long long s_ext[4], s_bad[4];
    unsigned long long ext = 0, nbad = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t fx = f[x];
        if (fx > n || fx < x) { nbad++; fx = fx > n ? n : x; }            // f[x] in [x, n] by construction
        e[x] = (uint32_t)(fx + 1);
        // longest minimal extension f[x]+1-x.  A column with f[x] = n (a row runs out of symbols; only without the elastic
        // tricks, fbg.cpp:1659-1663) can start no block at all -- its entry would be read at step n+1 -- and does not count
        if (fx < n) ext = max(ext, (unsigned long long)(fx + 1 - x));
    }
    for (int d = 32; d >= 1; d >>= 1) {
        ext = max(ext, (unsigned long long)__shfl_down(ext, d, 64));
        nbad += (unsigned long long)__shfl_down(nbad, d, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_ext[threadIdx.x >> 6] = ext; s_bad[threadIdx.x >> 6] = nbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long mx = max(max(s_ext[0], s_ext[1]), max(s_ext[2], s_ext[3])), nb = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        if (nb) atomicAdd(bad, nb);
        if (mx) atomicMax(bad + (DP_MAX_EXT - DP_BAD_ENTRIES), mx);
    }
}

// hist[e]++ : the counting sort of fbg.cpp:1941-1953 (only the wave-parallel and the literal sweep read its order)
__global__ void k_dp_hist(const uint32_t *__restrict__ e, uint64_t n, uint32_t *__restrict__ hist)
{
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) atomicAdd(&hist[e[x]], 1u);
}

__global__ void k_dp_scatter(const uint32_t *__restrict__ e, uint64_t n, uint32_t *__restrict__ cursor,
                             uint32_t *__restrict__ items)
{
    uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    uint32_t slot = atomicAdd(&cursor[e[x]], 1u);
    items[slot] = (uint32_t)x;
}

// fbg.cpp:1960-2014, one lane.  bstart[j]..bstart[j+1] delimit the entries with f[x]+1 == j.
__global__ void k_dp_minmax(const uint32_t *__restrict__ bstart, const uint32_t *__restrict__ items, uint32_t n,
                            uint32_t *__restrict__ count, uint32_t *__restrict__ bcount,
                            uint32_t *__restrict__ thead, uint32_t *__restrict__ tnext,
                            uint32_t *__restrict__ mml, uint32_t *__restrict__ bt)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    // count[], bcount[], mml[0], bt[0] arrive zeroed; thead[] arrives filled with DP_NONE
    uint32_t I = 0, S = n + 1, bS = DP_NONE;                                    // 1967
    for (uint32_t j = 1; j <= n; j++) {
        const uint32_t b0 = bstart[j], b1 = bstart[j + 1];
        for (uint32_t y = b0; y < b1; y++) {                                     // 1969
            const uint32_t xy = items[y];
            const uint32_t rec = mml[xy];
            if (rec > n) {
                // no recursive solution (1973)
            } else if (j <= xy + rec) {                                          // 1975
                count[rec] += 1;
                I = min(I, rec);
                const uint32_t cx = bcount[rec];
                if (xy + rec > cx + mml[cx]) bcount[rec] = xy;                   // 1979
                if (xy + rec + 1 <= n) {                                         // 1982
                    const uint32_t slot = xy + rec + 1;
                    tnext[xy] = thead[slot];
                    thead[slot] = xy;
                }
            } else {
                if (j - xy < S) { bS = xy; S = j - xy; }                         // 1986-1989
            }
        }
        for (uint32_t x = thead[j]; x != DP_NONE; x = tnext[x]) {                // 1993
            const uint32_t v = mml[x];
            const uint32_t c = count[v] - 1;
            count[v] = c;
            if (j - x < S) { S = j - x; bS = x; }
            if (c == 0) bcount[v] = 0;
        }
        const uint32_t cI = count[I];
        if (cI > 0 && I < S) { mml[j] = I; bt[j] = bcount[I]; }                  // 2004
        else { mml[j] = S; bt[j] = bS; }
        S += 1;
        if (cI == 0) I += 1;                                                     // 2012
    }
}


// ---- wave-parallel sweep ---------------------------------------------------------------------------
//
// Equivalent statement of fbg.cpp:1968-2014 used when f[0] == 0 (always true with the elastic
// "tricks", fbg.cpp:1605-1608: no row is active at column 0).  Then S == 1 after step 1 and the lazy
// index I of the reference can never hide a live count (whenever count[I] == 0, S <= I+1 holds, so the
// S branch it takes is the true minimum), hence
//     minmaxlength[j] = min over x with f[x]+1 <= j of max(minmaxlength[x], j - x),
// ties resolved towards the "S" candidate exactly as the strict `I < S` test does (fbg.cpp:2004).
// Lane L of the wave keeps cand[L] = max{ x : f[x]+1 <= j, minmaxlength[x] <= L }; then
//     minmaxlength[j] = min{ L : cand[L] + L >= j }                       (one ballot + find-first)
//     backtrack[j]    = j - L*      if cand[L*-1] == j - L*   (the reference's S / backtrack_S branch)
//                     = cand[L*]    otherwise                 (its count_solutions / backtrack_count branch)
// R registers per lane cover block lengths up to 64*R-1; minmaxlength never exceeds twice the longest
// minimal extension + 1, which is how R is chosen.  A step that finds no feasible lane raises `flag`
// and the host reruns the literal kernel (never observed; it guards the bound).
// DPW (dp_dev.h): steps / items staged in LDS per refill.

template <int R>
__global__ __launch_bounds__(64) void k_dp_wave(const uint32_t *__restrict__ bstart, const uint32_t *__restrict__ items,
                                                uint32_t n, uint32_t *__restrict__ mml, uint32_t *__restrict__ bt,
                                                unsigned long long *__restrict__ flag)
{
    constexpr int RING = 64 * R;              // covers x in (j - 64R, j): extensions are < 32R
    __shared__ uint32_t ring[RING];
    __shared__ uint32_t s_bs[DPW];            // bstart[jb+1 .. jb+DPW]: bucket end of each staged step
    __shared__ uint32_t s_it[DPW];            // items[itbase .. itbase+DPW)
    const int lane = threadIdx.x;
    int cand[R];
#pragma unroll
    for (int r = 0; r < R; r++) cand[r] = 0;  // f[0] == 0: column 0 is a candidate for every length from step 1 on
    if (R > 1) { for (int k = lane; k < RING; k += 64) ring[k] = 0; }
    int minLs = 1 << 30;

    // items reach the steps through two windows: DPW entries in LDS, 64 of them in one VGPR
    uint32_t y = 0, itbase = 0, itw = 0;      // itw: items index of lane 0 of the register window
    for (int k = lane; k < DPW; k += 64) s_it[k] = (uint32_t)k < n ? items[k] : 0;
    __syncthreads();
    uint32_t itv = s_it[lane];
    // steps are walked in 64-aligned groups so that lane (j & 63) of one register holds minmaxlength[j]
    int ringv = 0, outb = 0;                  // lane 0 of the first group is column 0: both 0
    for (uint32_t jb = 0; jb <= n; jb += DPW) {
        for (uint32_t k = lane; k < DPW; k += 64) s_bs[k] = jb + k + 1 <= n + 1 ? bstart[jb + k + 1] : 0;
        __syncthreads();
        for (uint32_t g = 0; g < DPW && jb + g <= n; g += 64) {
            const uint32_t bsv = s_bs[g + lane];
            const uint32_t k0 = (jb + g == 0) ? 1u : 0u;
            const uint32_t k1 = min(64u, n - (jb + g) + 1);
            for (uint32_t k = k0; k < k1; k++) {
                const uint32_t j = jb + g + k;
                const uint32_t b1 = (uint32_t)__builtin_amdgcn_readlane((int)bsv, (int)k);
                // ---- entries with f[x]+1 == j (fbg.cpp:1969) ----
                while (y < b1) {
                    if (y - itw >= 64) {          // next register window
                        itw += 64;
                        if (itw - itbase >= DPW) {   // next LDS window
                            itbase += DPW;
                            __syncthreads();
                            for (int q = lane; q < DPW; q += 64) s_it[q] = itbase + q < n ? items[itbase + q] : 0;
                            __syncthreads();
                        }
                        itv = s_it[itw - itbase + lane];
                    }
                    const int x = __builtin_amdgcn_readlane((int)itv, (int)(y - itw));
                    y++;
                    int v;
                    if (R == 1) v = __builtin_amdgcn_readlane(ringv, x & 63);
                    else v = __builtin_amdgcn_readfirstlane((int)ring[x & (RING - 1)]);
#pragma unroll
                    for (int r = 0; r < R; r++) cand[r] = (64 * r + lane >= v) ? max(cand[r], x) : cand[r];
                }
                // ---- smallest feasible block length: cand[L] + L is increasing in L ----
                int Ls = -1;
#pragma unroll
                for (int r = R - 1; r >= 0; r--) {
                    const unsigned long long bal = __builtin_amdgcn_ballot_w64((uint32_t)(cand[r] + 64 * r + lane) >= j);
                    if (bal) Ls = 64 * r + (int)__builtin_ctzll(bal);
                }
                minLs = min(minLs, Ls);
                int cprev, ccur;
                if (R == 1) {
                    cprev = __builtin_amdgcn_readlane(cand[0], (Ls - 1) & 63);
                    ccur = __builtin_amdgcn_readlane(cand[0], Ls & 63);
                } else {
                    cprev = ccur = 0;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int a = __builtin_amdgcn_readlane(cand[r], (Ls - 1) & 63);
                        const int b = __builtin_amdgcn_readlane(cand[r], Ls & 63);
                        if (((Ls - 1) >> 6) == r) cprev = a;
                        if ((Ls >> 6) == r) ccur = b;
                    }
                }
                const int jl = (int)j - Ls;
                const int back = cprev == jl ? jl : ccur;
                const bool mine = lane == (int)k;
                ringv = mine ? Ls : ringv;
                outb = mine ? back : outb;
                if (R > 1 && lane == 0) ring[j & (RING - 1)] = (uint32_t)Ls;
            }
            if ((uint32_t)lane < k1) { mml[jb + g + lane] = (uint32_t)ringv; bt[jb + g + lane] = (uint32_t)outb; }
        }
        __syncthreads();
    }
    if (minLs < 1 && lane == 0) flag[DP_WINDOW] = 1;
}

// backtrack (fbg.cpp:2026-2039): walks backtrack[] backwards through an 8192-column LDS window (one bulk
// load per window instead of one global round trip per hop); the boundaries are collected in reverse in
// LDS and flushed 1024 at a time.  rev[] receives them, result[DP_COUNT] the count.
__global__ __launch_bounds__(64) void k_dp_backtrack_wave(const uint32_t *__restrict__ bt, uint32_t n,
                                                          uint32_t *__restrict__ rev,
                                                          unsigned long long *__restrict__ result)
{
    constexpr uint32_t WIN = 8192;           // backtrack[] window held in LDS, reloaded when walked out of
    __shared__ uint32_t s_bt[WIN];
    __shared__ uint32_t obuf[1024];
    const uint32_t lane = threadIdx.x;
    uint32_t j = n, cnt = 1, flushed = 0;
    uint32_t wlo = 0xffffffffu, whi = 0;      // window covers columns [wlo, whi]
    if (lane == 0) obuf[0] = n;
    bool err = false;
    for (;;) {
        if (j < wlo || j > whi) {             // (re)load the window ending at j
            __syncthreads();
            whi = j;
            wlo = j >= WIN - 1 ? j - (WIN - 1) : 0;
            for (uint32_t k = lane; k <= whi - wlo; k += 64) s_bt[k] = bt[wlo + k];
            __syncthreads();
        }
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_bt[j - wlo]);
        if (b == 0) break;
        if (b > n || cnt > n + 1) { err = true; break; }
        if (cnt - flushed == 1024) {
            __syncthreads();
            for (uint32_t k = lane; k < 1024; k += 64) rev[flushed + k] = obuf[k];
            flushed += 1024;
            __syncthreads();
        }
        if (lane == 0) obuf[cnt - flushed] = b - 1;
        cnt++;
        j = b;
    }
    __syncthreads();
    for (uint32_t k = lane; k < cnt - flushed; k += 64) rev[flushed + k] = obuf[k];
    if (lane == 0) { result[DP_COUNT] = err ? 0 : cnt; result[DP_NO_SEGMENTATION] = err ? 1 : 0; }
}

// ---- parallel backtrack (fbg.cpp:2026-2039) by binary lifting --------------------------------------
// backtrack[] is a forest towards column 0.  up[k][j] = the column reached from j after 2^k hops (0 absorbs),
// dep[j] = number of hops from j to 0.  The boundary list of the reference, [.., backtrack-1, .., n], has
// dep[n] entries; entry t is found independently by jumping dep[n]-1-t hops from n.
__global__ void k_bt_lift0(const uint32_t *__restrict__ bt, uint32_t n, uint32_t *__restrict__ up0,
                           uint32_t *__restrict__ dep)
{
    // index n+1 is a dead end that absorbs every pointer that is not a backward pointer (columns without a
    // value, fbg.cpp:2004-2009 with backtrack_S still -1, or the non-elastic "no valid range" marker)
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n + 1) return;
    if (j == n + 1) { up0[j] = j; dep[j] = 0; return; }
    const uint32_t b = j == 0 ? 0u : bt[j];
    up0[j] = (b >= j && j != 0) ? n + 1 : b;
    dep[j] = j == 0 ? 0u : 1u;
}

__global__ void k_bt_lift(const uint32_t *__restrict__ up_prev, const uint32_t *__restrict__ dep_prev, uint32_t n,
                          uint32_t *__restrict__ up_next, uint32_t *__restrict__ dep_next)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n + 1) return;
    const uint32_t a = up_prev[j];
    up_next[j] = up_prev[a];
    dep_next[j] = dep_prev[j] + dep_prev[a];      // hops counted so far: exact once the chain reaches 0
}

__global__ void k_bt_emit(const uint32_t *__restrict__ up, const uint32_t *__restrict__ dep_final, uint32_t n,
                          uint32_t levels, uint64_t *__restrict__ boundaries, unsigned long long *__restrict__ result)
{
    // the chain from n is valid iff it ends in column 0 and not in the dead end
    uint32_t e = n;
    for (uint32_t k = 0; k < levels; k++) e = up[(size_t)k * (n + 2) + e];
    const bool ok = e == 0;
    const uint32_t cnt = dep_final[n];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { result[DP_COUNT] = ok ? cnt : 0; result[DP_NO_SEGMENTATION] = ok ? 0 : 1; }
    if (!ok || t >= cnt) return;
    uint32_t hops = cnt - 1 - t, j = n;
    for (uint32_t k = 0; k < levels && hops; k++, hops >>= 1)
        if (hops & 1u) j = up[(size_t)k * (n + 2) + j];
    boundaries[t] = t == cnt - 1 ? (uint64_t)n : (uint64_t)j - 1;
}

__global__ void k_reverse_widen(const uint32_t *__restrict__ rev, const unsigned long long *__restrict__ result,
                                uint64_t *__restrict__ boundaries)
{
    const unsigned long long cnt = result[DP_COUNT];
    const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < cnt) boundaries[k] = rev[cnt - 1 - k];
}

// fbg.cpp:2026-2039.  status: 0 ok, 1 = backtrack left the array (reference: out-of-bounds read)
__global__ void k_dp_backtrack(const uint32_t *__restrict__ bt, uint32_t n, uint64_t *__restrict__ boundaries,
                               unsigned long long *__restrict__ result)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t cnt = 1;
    uint32_t j = n;
    while (bt[j] != 0) {
        if (bt[j] > n || cnt > (uint64_t)n + 1) { result[DP_COUNT] = 0; result[DP_NO_SEGMENTATION] = 1; return; }
        cnt++; j = bt[j];
    }
    uint64_t k = cnt - 1;
    j = n;
    boundaries[k--] = n;
    while (bt[j] != 0) { boundaries[k--] = (uint64_t)bt[j] - 1; j = bt[j]; }
    result[DP_COUNT] = cnt; result[DP_NO_SEGMENTATION] = 0;
}

__global__ void k_widen(const uint32_t *__restrict__ src, uint64_t cnt, uint64_t *__restrict__ dst, int none_is_minus1)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    uint32_t v = src[k];
    dst[k] = (none_is_minus1 && v == DP_NONE) ? ~0ull : (uint64_t)v;
}

static int fbg_backtrack_lifted(fbg_ctx *ctx, const uint32_t *bt, uint32_t n, uint64_t *d_boundaries,
                                unsigned long long *sc)
{
    hipStream_t st = ctx->stream;
    uint32_t levels = 1;
    while ((1ull << (levels - 1)) <= (uint64_t)n) levels++;   // the last table spans 2^(levels-1) > n hops
    const size_t stride = (size_t)n + 2;
    FBG_TRY(fbg_reserve(ctx, ctx->bt_up, (size_t)levels * stride * 4));
    FBG_TRY(fbg_reserve(ctx, ctx->bt_dep, 2 * stride * 4));
    uint32_t *up = ctx->bt_up.as<uint32_t>(), *dep0 = ctx->bt_dep.as<uint32_t>(), *dep1 = dep0 + stride;
    const unsigned grid = fbg_blocks(stride, 256);
    hipLaunchKernelGGL(k_bt_lift0, dim3(grid), dim3(256), 0, st, bt, n, up, dep0);
    uint32_t *dp = dep0, *dn = dep1;
    for (uint32_t k = 1; k < levels; k++) {
        hipLaunchKernelGGL(k_bt_lift, dim3(grid), dim3(256), 0, st, up + (size_t)(k - 1) * stride, dp, n,
                           up + (size_t)k * stride, dn);
        uint32_t *t = dp; dp = dn; dn = t;
    }
    hipLaunchKernelGGL(k_bt_emit, dim3(grid), dim3(256), 0, st, up, dp, n, levels, d_boundaries, sc);
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

// ---- fbg_dp_minmax: a ladder of sweeps (dp_plan.h), the first that settles gives the result --------------------------------

// The window word of a rung: cleared before the rung's own launches (each rung with a window begins with it; the literal sweep
// has none), and after them copied, waited for and tested -- the one wait of a rung.
int fbg_dp_clear_window(fbg_ctx *ctx, unsigned long long *sc)
{
    FBG_HIP_TRY(ctx, hipMemsetAsync(sc + DP_WINDOW, 0, sizeof(unsigned long long), ctx->stream));
    return FBG_OK;
}

int fbg_dp_settled(fbg_ctx *ctx, unsigned long long *sc, bool *settled)
{
    unsigned long long raised = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&raised, sc + DP_WINDOW, sizeof(raised), hipMemcpyDeviceToHost, ctx->stream));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *settled = raised == 0;
    return FBG_OK;
}

// the bucket order of fbg.cpp:1941-1953 (counting sort of x by f[x]+1): only the wave-parallel and the literal sweep
// read it -- built when the first of them is about to run.  Also zeroes what the abandoned rungs left in count / bcount / mml / bt
static int dp_build_buckets(fbg_ctx *ctx, DpSweep &sw)
{
    if (sw.buckets_ready) return FBG_OK;
    hipStream_t st = ctx->stream;
    const uint64_t n = sw.n;
    const size_t w = (n + 2) * 4;
    uint32_t *bstart = ctx->dp_b.as<uint32_t>(), *cur = ctx->dp_c.as<uint32_t>(), *items = ctx->dp_d.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(bstart, 0, w, st));
    hipLaunchKernelGGL(k_dp_hist, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, sw.e, n, bstart);
    // ctx->tmp may hold the block matrices of an abandoned rung: they are dead by now
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, bstart, bstart, 0u, (size_t)(n + 2), rocprim::plus<uint32_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(cur, bstart, w, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_dp_scatter, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, sw.e, n, cur, items);
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctx->dp_e.p, 0, w, st));   // count
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctx->dp_f.p, 0, w, st));   // bcount
    FBG_HIP_TRY(ctx, hipMemsetAsync(sw.mml, 0, w, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(sw.bt, 0, w, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(cur, 0xff, w, st));        // thead = DP_NONE
    sw.buckets_ready = true;
    return FBG_OK;
}

// WAVE(R): k_dp_wave, from column 0 being a candidate at once (f[0] == 0)
static int rung_wave(fbg_ctx *ctx, DpSweep &sw, const DpRung &r, bool *settled)
{
    FBG_TRY(fbg_dp_clear_window(ctx, sw.sc));
    FBG_TRY(dp_build_buckets(ctx, sw));
    ctx->dp_attempts++;
    FBG_TRY(dp_for_R<16>((int)r.size, [&](auto R) {
        hipLaunchKernelGGL((k_dp_wave<decltype(R)::value>), dim3(1), dim3(64), 0, ctx->stream, ctx->dp_b.as<uint32_t>(), ctx->dp_d.as<uint32_t>(),
                           (uint32_t)sw.n, sw.mml, sw.bt, sw.sc);
        return FBG_OK;
    }));
    return fbg_dp_settled(ctx, sw.sc, settled);
}

// LITERAL: the statements of fbg.cpp:1960-2014 on one lane.  It has no window and always settles.
static int rung_literal(fbg_ctx *ctx, DpSweep &sw, bool *settled)
{
    hipStream_t st = ctx->stream;
    const size_t w = (sw.n + 2) * 4;
    uint32_t *count = ctx->dp_e.as<uint32_t>(), *bcount = ctx->dp_f.as<uint32_t>();
    ctx->dp_attempts++;
    FBG_TRY(dp_build_buckets(ctx, sw));
    FBG_HIP_TRY(ctx, hipMemsetAsync(count, 0, w, st));         // again: a wave sweep that did not settle has been here
    FBG_HIP_TRY(ctx, hipMemsetAsync(bcount, 0, w, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(sw.mml, 0, w, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(sw.bt, 0, w, st));
    hipLaunchKernelGGL(k_dp_minmax, dim3(1), dim3(64), 0, st, ctx->dp_b.as<uint32_t>(), ctx->dp_d.as<uint32_t>(), (uint32_t)sw.n, count, bcount,
                       ctx->dp_c.as<uint32_t>(), ctx->list.as<uint32_t>(), sw.mml, sw.bt);
    *settled = true;
    return FBG_OK;
}

int fbg_dp_minmax(fbg_ctx *ctx, const uint64_t *d_f, uint64_t n, uint64_t *d_boundaries, uint64_t *count_out,
                  uint64_t *d_mml, uint64_t *d_bt)
{
    hipStream_t st = ctx->stream;
    ctx->dp_attempts = 0;
    FBG_TRY(fbg_stage_begin(ctx, FBG_STAGE_DP));
    const size_t w = (n + 2) * 4;
    FBG_TRY(fbg_reserve(ctx, ctx->dp_a, w));   // e
    FBG_TRY(fbg_reserve(ctx, ctx->dp_b, w));   // hist -> bstart
    FBG_TRY(fbg_reserve(ctx, ctx->dp_c, w));   // cursor / thead; the byte chain's group states
    FBG_TRY(fbg_reserve(ctx, ctx->dp_d, w));   // items
    FBG_TRY(fbg_reserve(ctx, ctx->dp_e, w));   // count; the extensions of the byte and the wide rungs
    FBG_TRY(fbg_reserve(ctx, ctx->dp_f, w));   // bcount; clen of the byte rungs
    FBG_TRY(fbg_reserve(ctx, ctx->dp_g, w));   // mml
    FBG_TRY(fbg_reserve(ctx, ctx->dp_h, w));   // bt
    FBG_TRY(fbg_reserve(ctx, ctx->list, w));   // tnext
    FBG_TRY(fbg_reserve_scalars(ctx));
    DpSweep sw;
    sw.n = n;
    sw.e = ctx->dp_a.as<uint32_t>();
    sw.mml = ctx->dp_g.as<uint32_t>();
    sw.bt = ctx->dp_h.as<uint32_t>();
    unsigned long long *sc = sw.sc = fbg_scalars(ctx)->dp;
    FBG_HIP_TRY(ctx, hipMemsetAsync(sc, 0, DP_NE * sizeof(unsigned long long), st));   // the first block: the DP_NE words before the non-elastic one
    hipLaunchKernelGGL(k_dp_keys, dim3(fbg_blocks(n, 256, 2048)), dim3(256), 0, st, d_f, n, ctx->dp_a.as<uint32_t>(), sc + DP_BAD_ENTRIES);
    unsigned long long hk[DP_MAX_EXT + 1];
    uint64_t f0 = 1;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(hk, sc, sizeof(hk), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&f0, d_f, sizeof(f0), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hk[DP_BAD_ENTRIES] != 0) return fbg_fail(ctx, FBG_ERR_INVALID, "f[] has %llu entries outside [x, n]", hk[DP_BAD_ENTRIES]);
    // f[0] > 0 (only without the elastic tricks): nothing ends before step f[0] + 1, where the sweep stands exactly as
    // it does after step 1 otherwise (S = f[0] + 1, I = f[0], no counts: the invariant of the derivation above holds
    // from there on); the steps before it keep the running S of fbg.cpp:1967 and are filled in closed form.  The wave
    // sweep (k_dp_wave) starts from column 0 being a candidate at once and keeps its f[0] = 0 condition.
    sw.first_valid = (uint32_t)std::min<uint64_t>(f0 + 1, n + 1);
    const DpPlanOptions po = {ctx->opt.dp_literal != 0, ctx->opt.dp_wave != 0, ctx->opt.dp_safe_window != 0, ctx->opt.dp_tile != 0};
    const DpPlan plan = dp_plan(hk[DP_MAX_EXT], f0, n, po);
    bool settled = false;
    DpRung last = plan.rung[0];
    for (int i = 0; i < plan.count && !settled; i++) {
        last = plan.rung[i];
        switch (last.family) {
        case DP_BYTES: FBG_TRY(fbg_rung_bytes(ctx, sw, last, &settled)); break;
        case DP_WIDE: FBG_TRY(fbg_rung_wide(ctx, sw, last, &settled)); break;
        case DP_WAVE: FBG_TRY(rung_wave(ctx, sw, last, &settled)); break;
        case DP_LITERAL: FBG_TRY(rung_literal(ctx, sw, &settled)); break;
        }
    }
    ctx->dp_kind = dp_kind_of(last);
    // the byte and the wide rungs leave backtrack[] of every column at once: lifted; the two sweeps along the columns are walked
    if (last.family == DP_BYTES || last.family == DP_WIDE) FBG_TRY(fbg_backtrack_lifted(ctx, sw.bt, (uint32_t)n, d_boundaries, sc));
    else hipLaunchKernelGGL(k_dp_backtrack, dim3(1), dim3(64), 0, st, sw.bt, (uint32_t)n, d_boundaries, sc);
    if (d_mml) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, sw.mml, n + 1, d_mml, 0);
    if (d_bt) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, sw.bt, n + 1, d_bt, 1);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(fbg_stage_end(ctx, FBG_STAGE_DP, 6));
    unsigned long long h[DP_NO_SEGMENTATION + 1];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *count_out = h[DP_COUNT];
    if (h[DP_NO_SEGMENTATION] != 0) return fbg_fail(ctx, FBG_ERR_NO_SEGMENTATION, "No valid segmentation found!");
    return FBG_OK;
}

// ---- non-elastic recurrence (fbg.cpp:616-664), one lane ----------------------------------------

__global__ void k_dp_repeatfree(const uint64_t *__restrict__ v, uint32_t n, uint32_t *__restrict__ s,
                                uint32_t *__restrict__ prev, uint64_t *__restrict__ boundaries,
                                unsigned long long *__restrict__ result)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (uint32_t j = 0; j < n; j++) {
        uint32_t sj = j + 2, pj = j + 1;                                          // 623-624
        const uint64_t vj = v[j];
        if (vj <= j) {
            uint32_t jp = (uint32_t)vj;
            for (;;) {
                if (jp != 0 && s[jp - 1] == jp + 1) { jp--; continue; }          // 629-632
                const uint32_t a = jp == 0 ? 0u : s[jp - 1], b = j - jp + 1;
                const uint32_t cand = max(a, b);
                if (sj > cand) { sj = cand; pj = jp; }                            // 633-636
                if (sj == j - jp + 1) break;
                if (jp == 0) break;
                jp--;
            }
        }
        s[j] = sj; prev[j] = pj;
    }
    if (s[n - 1] == n + 1) { result[DP_COUNT] = 0; result[DP_NO_SEGMENTATION] = 1; return; }              // 648-652
    uint64_t cnt = 1;
    uint32_t j = n - 1;
    while (prev[j] != 0) { cnt++; j = prev[j] - 1; }                              // 657-660
    uint64_t k = cnt - 1;
    j = n - 1;
    boundaries[k--] = j;
    while (prev[j] != 0) { boundaries[k--] = (uint64_t)prev[j] - 1; j = prev[j] - 1; }
    result[DP_COUNT] = cnt; result[DP_NO_SEGMENTATION] = 0;
}

// ---- non-elastic recurrence on the block-matrix machinery ---------------------------------------------
// In prefix lengths (j' = j+1, x' = jp): s'[j'] = min over x' <= v[j'-1] of max(s'[x'], j' - x') for steps
// with a valid block (v[j'-1] <= j'-1), no value otherwise (fbg.cpp:622-643).  A candidate is valid at a
// step iff its age j'-x' is at least j' - v[j'-1]: a per-step threshold instead of a per-candidate one.
__global__ void k_ne_prep(const uint64_t *__restrict__ v, uint32_t n, uint8_t *__restrict__ ext1, uint8_t *__restrict__ amin,
                          unsigned long long *__restrict__ sc)
{
    const uint32_t jp = blockIdx.x * blockDim.x + threadIdx.x;   // prefix length 0..n
    if (jp > n) return;
    ext1[jp] = 1;
    uint32_t am = 255;
    bool valid = false;
    if (jp >= 1) {
        const uint64_t vj = v[jp - 1];
        valid = vj <= jp - 1;
        if (valid) am = (uint32_t)min((uint64_t)255, (uint64_t)jp - vj);
    }
    amin[jp] = (uint8_t)am;
    // longest minimal block, to size the window.  In the byte 255 also says "no valid block ends here", so a minimal block
    // of 255 columns or more must not reach the matrix path as that byte: it counts with 255 here, which is beyond every
    // tier (fbg_dp_repeatfree: 2 * 255 + 2 > 254), and the statement-by-statement kernel takes the input
    unsigned long long e = valid ? am : 0;
    for (int d = 32; d >= 1; d >>= 1) e = max(e, (unsigned long long)__shfl_down(e, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(sc + DP_MAX_EXT, e);
}

// s[j], prev[j] (fbg.cpp:623-636) from the prefix values: first (largest jp) candidate reaching the minimum
__global__ void k_ne_finish(const uint32_t *__restrict__ sp, const uint8_t *__restrict__ amin, uint32_t n, uint32_t window,
                            uint32_t *__restrict__ s, uint32_t *__restrict__ prev, uint32_t *__restrict__ btp,
                            unsigned long long *__restrict__ flag)
{
    const uint32_t jp = blockIdx.x * blockDim.x + threadIdx.x;   // prefix length 1..n  <->  column j = jp-1
    if (jp == 0) { if (blockIdx.x == 0) btp[0] = 0; return; }
    if (jp > n) return;
    const uint32_t L = sp[jp], am = amin[jp], j = jp - 1;
    if (am == 255) { s[j] = j + 2; prev[j] = j + 1; btp[jp] = DP_NONE; return; }       // no valid block ends here
    if (L >= DPB_INF) {   // no value inside the window: undecidable here, let the literal kernel do this input
        flag[DP_WINDOW] = 1; s[j] = j + 2; prev[j] = j + 1; btp[jp] = DP_NONE; return;
    }
    uint32_t best = 0;
    const uint32_t amax = min(window, jp);
    for (uint32_t a = am; a <= amax; a++) {
        const uint32_t v = sp[jp - a];
        if (v < DPB_INF && max(v, a) == L) { best = a; break; }
    }
    if (!best) { flag[DP_WINDOW] = 1; best = am; }
    s[j] = L;
    prev[j] = jp - best;
    btp[jp] = jp - best;
}

__global__ void k_ne_fix_last(uint64_t *__restrict__ boundaries, const unsigned long long *__restrict__ result)
{
    // the shared backtrack emits n as last boundary (elastic convention); segment() ends at n-1 (fbg.cpp:655-656)
    if (blockIdx.x == 0 && threadIdx.x == 0 && result[DP_COUNT] > 0) boundaries[result[DP_COUNT] - 1] -= 1;
}

int fbg_dp_repeatfree(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s, uint64_t *d_prev,
                      uint64_t *d_boundaries, uint64_t *count_out)
{
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_stage_begin(ctx, FBG_STAGE_DP));
    FBG_TRY(fbg_reserve(ctx, ctx->dp_g, (n + 2) * 4));
    FBG_TRY(fbg_reserve(ctx, ctx->dp_h, (n + 2) * 4));
    FBG_TRY(fbg_reserve_scalars(ctx));
    uint32_t *s = ctx->dp_g.as<uint32_t>(), *prev = ctx->dp_h.as<uint32_t>();
    unsigned long long *sc = fbg_scalars(ctx)->dp, *sc_ne = sc + DP_NE;
    FBG_HIP_TRY(ctx, hipMemsetAsync(sc, 0, DP_WORDS * sizeof(unsigned long long), st));
    bool literal = ctx->opt.dp_literal != 0;
    ctx->ne_dp_kind = 0;
    if (!literal) {
        const size_t w = (n + 2) * 4;
        FBG_TRY(fbg_reserve(ctx, ctx->dp_a, w));
        FBG_TRY(fbg_reserve(ctx, ctx->dp_b, w));
        FBG_TRY(fbg_reserve(ctx, ctx->dp_c, w));
        FBG_TRY(fbg_reserve(ctx, ctx->dp_e, w));
        FBG_TRY(fbg_reserve(ctx, ctx->dp_f, w));
        uint8_t *ext1 = ctx->dp_e.as<uint8_t>(), *amin = ctx->dp_f.as<uint8_t>();
        uint32_t *sp = ctx->dp_a.as<uint32_t>(), *btp = ctx->dp_b.as<uint32_t>();
        uint8_t *Sg = ctx->dp_c.as<uint8_t>();
        hipLaunchKernelGGL(k_ne_prep, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, d_v, (uint32_t)n, ext1, amin, sc);
        unsigned long long hk[DP_MAX_EXT + 1];
        FBG_HIP_TRY(ctx, hipMemcpyAsync(hk, sc, sizeof(hk), hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
        const int R = dp_tier(2 * hk[DP_MAX_EXT] + 2, /* no wave sweep here: the cap of an f[0] != 0 */ 1);
        if (R == 0) {
            literal = true;
        } else {
            // the byte chain in groups of 4 blocks; k_dp_expand's flag goes to the non-elastic block (DP_NE, fbg_internal.h)
            FBG_TRY(fbg_dp_byte_chain(ctx, R, ext1, amin, n, 4, Sg, sp, sc_ne, 0));
            hipLaunchKernelGGL(k_ne_finish, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, sp, amin, (uint32_t)n, 64u * R, s, prev,
                               btp, sc);
            bool settled = false;
            FBG_TRY(fbg_dp_settled(ctx, sc, &settled));
            ctx->ne_dp_kind = settled ? R : 8;
            if (!settled) {
                literal = true;   // window too small for this input: statement-by-statement kernel
                FBG_HIP_TRY(ctx, hipMemsetAsync(sc, 0, DP_NE * sizeof(unsigned long long), st));   // the first block, as at the start
            } else {
                // no proper segmentation <=> the last prefix has no value (fbg.cpp:648-652)
                FBG_TRY(fbg_backtrack_lifted(ctx, btp, (uint32_t)n, d_boundaries, sc));
                hipLaunchKernelGGL(k_ne_fix_last, dim3(1), dim3(64), 0, st, d_boundaries, sc);
            }
        }
    }
    if (literal)
        hipLaunchKernelGGL(k_dp_repeatfree, dim3(1), dim3(64), 0, st, d_v, (uint32_t)n, s, prev, d_boundaries, sc);
    if (d_s) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, s, n, d_s, 0);
    if (d_prev) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, prev, n, d_prev, 0);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(fbg_stage_end(ctx, FBG_STAGE_DP, 3));
    unsigned long long h[DP_NO_SEGMENTATION + 1];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *count_out = h[DP_COUNT];
    if (h[DP_NO_SEGMENTATION] != 0) return fbg_fail(ctx, FBG_ERR_NO_SEGMENTATION, "No proper segmentation exists.");
    return FBG_OK;
}

// ---- non-elastic mode with gaps: segment2elasticValid (fbg.cpp:738-866) ---------------------------------------
// v[] from the f of the elastic scan without tricks: block [jp..j] passes the interval-union test of fbg.cpp:786-808
// iff F[jp] <= j (all rows have a symbol in it and every occurrence of every row's string starts at some row's first
// symbol at or after jp -- what compute_f evaluates with all rows coloured).  The reference's left-moving pointer
// (763-822) never binds, because the largest passing jp cannot decrease as j grows: v[j] = max{jp : F[jp] <= j}.

__global__ void k_gv_scatter(const uint64_t *__restrict__ f, uint32_t n, uint32_t *__restrict__ best)
{
    const uint32_t jp = blockIdx.x * blockDim.x + threadIdx.x;
    if (jp >= n) return;
    const uint64_t F = f[jp];
    if (F < n) atomicMax(best + F, jp + 1);          // 0 = no block ends here
}

__global__ void k_gv_finish(const uint32_t *__restrict__ best, uint32_t n, uint64_t *__restrict__ v)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t b = best[j];                      // running maximum by now
    v[j] = b ? (uint64_t)b - 1 : (uint64_t)j + 1;   // 764, 806
}

int fbg_gapped_v_from_f(fbg_ctx *ctx, const uint64_t *d_f, uint64_t n, uint64_t *d_v)
{
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_reserve(ctx, ctx->dp_a, (n + 2) * 4));
    uint32_t *best = ctx->dp_a.as<uint32_t>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(best, 0, (n + 2) * 4, st));
    hipLaunchKernelGGL(k_gv_scatter, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, d_f, (uint32_t)n, best);
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, best, best, (size_t)n, rocprim::maximum<uint32_t>(), st);
    }));
    hipLaunchKernelGGL(k_gv_finish, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, best, (uint32_t)n, d_v);
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

// The recurrence of fbg.cpp:830-846 is a chain: column j takes either a new block [v[j]..j] on top of s[v[j]-1] or the
// solution of column j-1 with its last block extended, so one wave walks the columns -- but it walks from event to event,
// not from column to column.  Between two events (a new block taken at 838-841 or 834-837, or a column without a block,
// 832) the state is the last event's (a, P) with the last block growing: s[j] = max(a, j - P + 1), prev[j] = P.  A tile of
// 64 columns sits in the lanes; every lane evaluates its column under the assumption that nothing happens between the
// last event and itself (its lookback s[v-1] is then either a finished value or the same closed form), a ballot finds
// the first lane whose test fires -- for that lane the assumption is true -- and the walk jumps there.  Lookbacks in
// front of the tile come from a ring of the last GD_RING values of s in LDS (or, beyond it, from memory), fetched by
// all lanes at once before the walk.  INV = n+1 is the reference's initial value of both arrays; with prev[j-1] = n+1
// the reference's j - prev[j-1] + 1 wraps around to something larger than any score (838, 843), spelled GD_HUGE here.
#define GD_RING 8192u
#define GD_HUGE 0xffffffffu
#define GD_TILES 8u          // tiles per prefetch group

__global__ __launch_bounds__(64) void k_dp_gapped(const uint64_t *__restrict__ v, uint32_t n, uint32_t *__restrict__ s,
                                                 uint32_t *__restrict__ prev, uint32_t *__restrict__ btp)
{
    __shared__ uint32_t ring[GD_RING];
    const uint32_t lane = threadIdx.x, INV = n + 1;
    uint32_t sa = INV, sp = INV;                               // the last event: s and prev it left behind
    auto fetch = [&](uint32_t t0) -> uint32_t {                // v of column t0 + lane; INV = no block ends here (832)
        const uint32_t j = t0 + lane;
        if (j >= n || j == 0) return INV;                      // the loop starts at 1 (830)
        const uint64_t x = v[j];
        return x > j ? INV : (uint32_t)x;
    };
    if (lane == 0) btp[0] = 0;
    uint32_t cur[GD_TILES], nxt[GD_TILES];
#pragma unroll
    for (uint32_t q = 0; q < GD_TILES; q++) nxt[q] = fetch(q * 64);
    for (uint32_t g0 = 0; g0 < n; g0 += 64 * GD_TILES) {
        // the prefetched columns are settled here, once per group: left to the compiler, the wait for them lands in front
        // of every tile's walk, and a wait for loads is a wait for the previous tile's stores as well
#pragma unroll
        for (uint32_t q = 0; q < GD_TILES; q++) { cur[q] = nxt[q]; asm volatile("" : "+v"(cur[q])); }
        if (g0 + 64 * GD_TILES < n) {
#pragma unroll
            for (uint32_t q = 0; q < GD_TILES; q++) nxt[q] = fetch(g0 + 64 * GD_TILES + q * 64);
        }
#pragma unroll
        for (uint32_t q = 0; q < GD_TILES; q++) {
            const uint32_t t0 = g0 + q * 64;
            if (t0 >= n) break;
            const uint32_t vj = cur[q], j = t0 + lane;
            const bool skip = vj == INV, first = vj == 0;
            const uint32_t look = vj - 1;                      // column whose s the new block builds on
            // s[v-1] for lookbacks that land in front of this tile
            uint32_t aext = INV;
            bool far = false;
            if (!skip && !first && look < t0) {
                if (t0 - look <= GD_RING) aext = ring[look % GD_RING]; else far = true;
            }
            if (__ballot(far)) {
                __threadfence();
                if (far) aext = __hip_atomic_load(s + look, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0) here, in the rare branch, not in the walk below
            }
            const uint32_t len_new = j - vj + 1;
            uint32_t s_vec = INV, p_vec = INV;
            const uint32_t cnt = min(64u, n - t0);
            uint32_t k0 = 0;                                   // lanes below k0 are finished
            while (k0 < cnt) {
                // the state of column j-1 if nothing happens between the last event and j
                const uint32_t b = sp == INV ? GD_HUGE : max(sa, j - sp + 1);
                // every lane takes part in the exchange (a lane switched off would hand out nothing)
                const uint32_t fin = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((look - t0) & 63u) << 2), (int)s_vec);
                const uint32_t A = look < t0 ? aext : look - t0 < k0 ? fin : max(sa, look - sp + 1);
                const uint32_t a = max(A, len_new);
                const bool fire = skip || first || a < b;                                   // 832, 834, 838
                const unsigned long long mask = __ballot(fire && lane >= k0 && lane < cnt);
                const uint32_t ks = mask ? (uint32_t)__builtin_ctzll(mask) : cnt;
                if (lane >= k0 && lane < ks) { s_vec = b; p_vec = sp; }                     // 842-845
                if (ks >= cnt) break;
                const uint32_t ns = skip ? INV : first ? j + 1 : a;                         // 836, 839
                const uint32_t np = skip ? INV : vj;                                        // 837, 840
                if (lane == ks) { s_vec = ns; p_vec = np; }
                sa = (uint32_t)__builtin_amdgcn_readlane((int)ns, (int)ks);
                sp = (uint32_t)__builtin_amdgcn_readlane((int)np, (int)ks);
                k0 = ks + 1;
            }
            if (j < n) {
                s[j] = s_vec; prev[j] = p_vec;
                btp[j + 1] = p_vec;                // in prefix lengths: the block that ends prefix j+1 starts after prefix prev[j]
                ring[j % GD_RING] = s_vec;
            }
            __syncthreads();
        }
    }
}

// "No valid segmentation found!" is decided on s[n-1] (fbg.cpp:850-854)
__global__ void k_gd_verdict(const uint32_t *__restrict__ s, uint32_t n, uint64_t *__restrict__ boundaries,
                             unsigned long long *__restrict__ result)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (s[n - 1] == n + 1) { result[DP_COUNT] = 0; result[DP_NO_SEGMENTATION] = 1; return; }
    if (result[DP_COUNT] > 0) boundaries[result[DP_COUNT] - 1] -= 1;          // the shared backtrack ends at n; this one at n-1 (857-858)
}

int fbg_dp_gapped(fbg_ctx *ctx, const uint64_t *d_v, uint64_t n, uint64_t *d_s, uint64_t *d_prev,
                  uint64_t *d_boundaries, uint64_t *count_out)
{
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_stage_begin(ctx, FBG_STAGE_DP));
    const size_t w = (n + 2) * 4;
    FBG_TRY(fbg_reserve(ctx, ctx->dp_g, w));
    FBG_TRY(fbg_reserve(ctx, ctx->dp_h, w));
    FBG_TRY(fbg_reserve(ctx, ctx->dp_b, w));
    FBG_TRY(fbg_reserve_scalars(ctx));
    uint32_t *s = ctx->dp_g.as<uint32_t>(), *prev = ctx->dp_h.as<uint32_t>(), *btp = ctx->dp_b.as<uint32_t>();
    unsigned long long *sc = fbg_scalars(ctx)->dp;
    FBG_HIP_TRY(ctx, hipMemsetAsync(sc, 0, DP_WORDS * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_dp_gapped, dim3(1), dim3(64), 0, st, d_v, (uint32_t)n, s, prev, btp);
    FBG_TRY(fbg_backtrack_lifted(ctx, btp, (uint32_t)n, d_boundaries, sc));
    hipLaunchKernelGGL(k_gd_verdict, dim3(1), dim3(64), 0, st, s, (uint32_t)n, d_boundaries, sc);
    if (d_s) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, s, n, d_s, 0);
    if (d_prev) hipLaunchKernelGGL(k_widen, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, prev, n, d_prev, 0);
    FBG_HIP_TRY(ctx, hipGetLastError());
    FBG_TRY(fbg_stage_end(ctx, FBG_STAGE_DP, 3));
    unsigned long long h[DP_NO_SEGMENTATION + 1];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *count_out = h[DP_NO_SEGMENTATION] ? 0 : h[DP_COUNT];
    if (h[DP_NO_SEGMENTATION] != 0) return fbg_fail(ctx, FBG_ERR_NO_SEGMENTATION, "No valid segmentation found!");
    return FBG_OK;
}
