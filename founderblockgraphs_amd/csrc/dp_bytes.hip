// dp_bytes.hip -- the min-max-length recurrence on byte entries: windows of 64, 128 and 256 columns.
//
//  * the tiled sweep k_dp_tile (option dp_tile) and the block-matrix chain k_dp_blockW / k_dp_compose / k_dp_chain6 (k_dp_chain
//    under dp_chain1) / k_dp_expand, with k_dp_prep in front and k_dp_bt behind;
//  * fbg_dp_byte_chain: the one launcher of that chain, for the BYTES rungs of fbg_dp_minmax and for fbg_dp_repeatfree (dp.hip);
//  * fbg_rung_bytes: a BYTES rung of the ladder (dp_plan.h).
#include "dp_host.h"
#include "dp_dev.h"

// ---- tiled sweep: 8 steps per iteration (block lengths < 64) ---------------------------------------
//
// Same recurrence as k_dp_wave, arranged so that one wave instruction works on 8 steps x 8 candidates:
//     minmaxlength[j] = min over candidates x < j with f[x]+1 <= j of max(minmaxlength[x], j - x).
// A chunk of c <= 8 consecutive steps j..j+c-1 can be evaluated together when no column inside the chunk
// is itself a usable candidate inside it, i.e. f[x]+1 >= j+c for every x >= j (clen[], precomputed).
// Lane (t, c8) scores candidates of age 8*c8+1 .. 8*c8+8 (relative to j) for step j+t; the eight partial
// minima of a step are combined with three DPP row operations.  The reference's tie-breaking is folded
// into the key: cost*128 + 0 for a candidate of its "S" kind (age > minmaxlength[x], fbg.cpp:1985-1989,
// 1996-1999), cost*128 + 1 + age for its count_solutions kind (youngest first = backtrack_count's
// largest x, fbg.cpp:1976-1981); S wins ties like the strict `I < S` (fbg.cpp:2004).
// The last 64 columns' (extension, minmaxlength) pairs live in an LDS ring; ages beyond 64 cannot win
// because minmaxlength <= 63 here (checked: a step without a feasible candidate raises the flag).
#define DPT_BIG 0xffffu

__global__ void k_dp_prep(const uint32_t *__restrict__ e, uint32_t n, uint32_t ext_cap, uint8_t *__restrict__ ext7,
                          uint8_t *__restrict__ clen)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    ext7[j] = j < n ? (uint8_t)min(e[j] - j, ext_cap) : (uint8_t)ext_cap;
    uint32_t c = 8;
    for (uint32_t s = 0; s < 8 && j + s < n; s++) c = min(c, e[j + s] - j);   // e[j+s] - j >= s + 1 >= 1
    clen[j] = (uint8_t)c;
}

__device__ __forceinline__ uint32_t dpp_min8(uint32_t v)
{
    // minimum over each group of 8 consecutive lanes (half a DPP row)
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    return v;
}

__global__ __launch_bounds__(64) void k_dp_tile(const uint8_t *__restrict__ ext7, const uint8_t *__restrict__ clen,
                                                uint32_t n, uint32_t *__restrict__ mml, uint32_t *__restrict__ bt,
                                                unsigned long long *__restrict__ flag)
{
    __shared__ uint16_t ring[64];            // (extension << 7) | minmaxlength of column (x & 63)
    __shared__ uint8_t s_ext[DPW + 16], s_len[DPW + 16];
    const uint32_t lane = threadIdx.x, t = lane >> 3, c8 = lane & 7;
    ring[lane] = (uint16_t)(127u << 7);      // columns < 0 do not exist: never valid
    if (lane == 0) { mml[0] = 0; bt[0] = 0; }
    uint32_t wbase = 0xffffffffu, j = 1;
    uint32_t bad = 0;
    while (j <= n) {
        if (wbase == 0xffffffffu || j + 8 > wbase + DPW) {           // stage the next window of inputs
            __syncthreads();
            wbase = j;
            for (uint32_t k = lane; k < DPW + 8; k += 64) {
                const uint32_t x = wbase + k;
                s_ext[k] = x <= n ? ext7[x] : (uint8_t)127;
                s_len[k] = x <= n ? clen[x] : (uint8_t)1;
            }
            if (j == 1 && lane == 0) ring[0] = (uint16_t)(((uint32_t)ext7[0] << 7) | 0u);   // column 0, minmaxlength 0
            __syncthreads();
        }
        uint32_t cl = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_len[j - wbase]);
        cl = min(cl, n - j + 1);
        uint32_t best = DPT_BIG;
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            const uint32_t a0 = 1 + 8 * c8 + u;                      // age of the candidate at step j
            const uint32_t pk = ring[(j - a0) & 63];
            const uint32_t v = pk & 127u, ext = pk >> 7;
            const uint32_t age = a0 + t;                             // its age at this lane's step j + t
            const uint32_t key = (max(v, age) << 7) | (age > v ? 0u : age + 1);
            best = min(best, ext <= age ? key : DPT_BIG);
        }
        best = dpp_min8(best);
        const uint32_t jt = j + t;
        const uint32_t cost = best >> 7, tb = best & 127u;
        const uint32_t back = tb == 0 ? jt - cost : jt - (tb - 1);
        const bool live = t < cl;
        bad |= (live && best == DPT_BIG) ? 1u : 0u;
        if (live && c8 == 0) {
            mml[jt] = cost;
            bt[jt] = back;
            if (jt < n) ring[jt & 63] = (uint16_t)(((uint32_t)s_ext[jt - wbase] << 7) | (cost & 127u));
        }
        j += cl;
    }
    if (__ballot(bad != 0) && lane == 0) flag[DP_WINDOW] = 1;
}

// ---- block-matrix sweep: the recurrence as a (min,max) matrix chain ----------------------------------
//
// minmaxlength[j] = min_x max(minmaxlength[x], j-x) is a product in the (min,max) semiring, so a block of 64
// steps acts on the 64 values before it through a 64x64 matrix W_b:
//     minmaxlength[64b+1+t] = min_k max( minmaxlength[64b-63+k], W_b[k][t] ),
// W_b[k][t] = the smallest achievable longest block over all ways of cutting [64b-63+k, 64b+1+t) into valid
// blocks (first block starting at the old column, the rest inside the new 64 columns).  Only candidates of
// age <= 64 are considered, which is exact while minmaxlength <= 63 (flagged otherwise).
//   k_dp_blockW  builds every W_b independently: one wave per block, lane = old column k, 64 sequential
//                steps of the same recurrence started from a one-hot state.  Embarrassingly parallel.
//   k_dp_chain   the only sequential part left: one (min,max) matrix-vector product per block.
//   k_dp_bt      backtrack[j] from minmaxlength[] alone, one thread per column, with the reference's
//                tie-breaking (S kind first, else the youngest count_solutions kind; fbg.cpp:1976-2009).
// R = window / 64: candidates up to 64R columns back, blocks of 64R steps, matrices of (64R)^2 bytes.
// Step t of source k: w = min over the inside candidates tp < t of max(W[tp][k], t - tp), a candidate counting from the
// step on at which its block is long enough (t >= tp + ext[tp]) -- 64R steps x 64R candidates x 64R sources per block.
// The thread's row of W lies along tp in LDS (rows padded by 4 bytes: the lanes' rows start in different banks), so one
// load brings 4 candidates; their bytes as two pairs of 16-bit lanes go through packed max (with the ages, which are
// the same for all sources) and packed min; which candidates count is a byte mask per wave, kept up to date by the
// lanes themselves (lane j clears the bytes of its candidates at the step they become usable): 0xff on a byte makes
// the maximum at least 255 = no solution.  11 vector operations per 4 candidates instead of 24.
#define DPB_PADDED(WN) ((WN) + 4)
template <int R>
__global__ __launch_bounds__(64 * R) void k_dp_blockW(const uint8_t *__restrict__ ext7, const uint8_t *__restrict__ amin,
                                                      uint32_t n, uint32_t nblocks, uint8_t *__restrict__ Wt)
{
    // amin (optional): per-step minimal block length -- the non-elastic recurrence, where a block ending at
    // step j is valid iff it is at least j - v[j-1] long (fbg.cpp:625-627); 255 = no valid block ends there
    // one thread per source column k; the R waves of a block never need each other's values
    constexpr uint32_t WN = 64 * R, WP = DPB_PADDED(WN);
    extern __shared__ uint8_t dyn_lds[];
    uint8_t *wl = dyn_lds;                   // wl[k * WP + t]: W of inside column (block start + 1 + t) for source k
    uint8_t *s_ext = dyn_lds + WN * WP;      // extensions of the inside columns
    uint8_t *s_amin = s_ext + WN;            // minimal block length per step
    uint8_t *mk = s_amin + WN + (threadIdx.x >> 6) * 2 * WN;   // this wave's masks: per group of 4 candidates two words (even / odd candidates as 16-bit lanes)
    const uint32_t k = threadIdx.x, lane = threadIdx.x & 63;
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint32_t jb = WN * b;
        const int64_t xs = (int64_t)jb - (WN - 1) + k;                    // old column of source k
        const uint32_t ext_src = xs >= 0 ? ext7[xs] : 255u;
        __syncthreads();
        s_ext[k] = jb + 1 + k < n ? ext7[jb + 1 + k] : (uint8_t)255;
        s_amin[k] = amin ? (jb + 1 + k <= n ? amin[jb + 1 + k] : (uint8_t)255) : (uint8_t)1;
        __syncthreads();
        uint32_t minext = 255;
        for (uint32_t q = 0; q < WN; q++) minext = min(minext, (uint32_t)s_ext[q]);
        // all candidates masked out; candidate tp = 4g + j sits in byte 8g + 4(j & 1) + 2(j >> 1)
        for (uint32_t q = lane; q < WN / 4; q += 64) reinterpret_cast<uint2 *>(mk)[q] = make_uint2(0x00ff00ffu, 0x00ff00ffu);
        uint32_t ready[R];                                                // the step from which the lane's candidates count
#pragma unroll
        for (int r = 0; r < R; r++) { const uint32_t tp = lane + 64 * r; ready[r] = tp + max(1u, (uint32_t)s_ext[tp]); }
        uint8_t *row = wl + k * WP;
        uint8_t *out = Wt + (size_t)b * WN * WN;
        for (uint32_t t = 0; t < WN; t++) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (ready[r] == t) { const uint32_t tp = lane + 64 * r; mk[8 * (tp >> 2) + 4 * (tp & 1) + 2 * ((tp >> 1) & 1)] = 0; }
            __builtin_amdgcn_wave_barrier();
            const uint32_t age_src = t + WN - k;                          // (jb+1+t) - xs
            const uint32_t am = s_amin[t];
            uint32_t w = (ext_src <= age_src && age_src <= WN && age_src >= am) ? age_src : DPB_INF;
            // inside candidates need age >= their extension >= minext and age >= the step's minimum
            const uint32_t need = max(minext, am);
            const uint32_t tp_end = t >= need ? t - need + 1 : 0;
            dp_u16x2 acc_e = dp_pair(0xffffu), acc_o = acc_e;
            uint32_t g4 = 0;
            // sixteen candidates a turn without a bound check in between (round 4: the compiler's own unrolling kept a compare
            // and a branch after every four), then the rest four at a time
            for (; g4 + 16 <= tp_end; g4 += 16) {
#pragma unroll
                for (uint32_t h = 0; h < 16; h += 4) {
                    const uint32_t word = *reinterpret_cast<const uint32_t *>(row + g4 + h);
                    const uint2 m = *reinterpret_cast<const uint2 *>(mk + 2 * (g4 + h));
                    const uint32_t base = t - g4 - h;
                    const dp_u16x2 age_e = dp_bits(base | ((base - 2) << 16)), age_o = dp_bits((base - 1) | ((base - 3) << 16));
                    acc_e = __builtin_elementwise_min(acc_e, __builtin_elementwise_max(dp_bits((word & 0x00ff00ffu) | m.x), age_e));
                    acc_o = __builtin_elementwise_min(acc_o, __builtin_elementwise_max(dp_bits(((word >> 8) & 0x00ff00ffu) | m.y), age_o));
                }
            }
            for (; g4 + 4 <= tp_end; g4 += 4) {
                const uint32_t word = *reinterpret_cast<const uint32_t *>(row + g4);
                const uint2 m = *reinterpret_cast<const uint2 *>(mk + 2 * g4);
                const uint32_t base = t - g4;
                const dp_u16x2 age_e = dp_bits(base | ((base - 2) << 16)), age_o = dp_bits((base - 1) | ((base - 3) << 16));
                acc_e = __builtin_elementwise_min(acc_e, __builtin_elementwise_max(dp_bits((word & 0x00ff00ffu) | m.x), age_e));
                acc_o = __builtin_elementwise_min(acc_o, __builtin_elementwise_max(dp_bits(((word >> 8) & 0x00ff00ffu) | m.y), age_o));
            }
            if (g4 < tp_end) {                                            // the last, partial group: candidates from tp_end on do not count
                const uint32_t word = *reinterpret_cast<const uint32_t *>(row + g4);
                uint2 m = *reinterpret_cast<const uint2 *>(mk + 2 * g4);
                const uint32_t live = tp_end - g4;                        // 1 .. 3
                if (live < 2) m.y |= 0x000000ffu;
                if (live < 3) m.x |= 0x00ff0000u;
                m.y |= 0x00ff0000u;
                const uint32_t base = t - g4;
                const dp_u16x2 age_e = dp_bits((base & 0xffffu) | ((base - 2) << 16)), age_o = dp_bits(((base - 1) & 0xffffu) | ((base - 3) << 16));
                acc_e = __builtin_elementwise_min(acc_e, __builtin_elementwise_max(dp_bits((word & 0x00ff00ffu) | m.x), age_e));
                acc_o = __builtin_elementwise_min(acc_o, __builtin_elementwise_max(dp_bits(((word >> 8) & 0x00ff00ffu) | m.y), age_o));
            }
            const dp_u16x2 acc = __builtin_elementwise_min(acc_e, acc_o);
            w = min(w, min((uint32_t)acc.x, (uint32_t)acc.y));
            w = min(w, DPB_INF);
            row[t] = (uint8_t)w;
            out[(size_t)t * WN + k] = (uint8_t)w;                         // Wt[b][t][k]
        }
    }
}

template <int R>
__global__ __launch_bounds__(64) void k_dp_chain(const uint8_t *__restrict__ Wt, uint32_t n, uint32_t nblocks,
                                                 uint32_t F, uint8_t *__restrict__ Sg,
                                                 uint32_t *__restrict__ mml, unsigned long long *__restrict__ flag)
{
    // steps from group to group: block index of step g is the last block of group g (its matrix holds the
    // product of the whole group after k_dp_compose); Sg[g] receives the state entering group g
    constexpr uint32_t WN = 64 * R;
    constexpr bool PREFETCH = R <= 2;        // next block's rows held in registers (16 R^2 VGPRs)
    constexpr int NQ = R * R * 4;             // uint4 loads per lane per block
    const uint32_t lane = threadIdx.x;
    uint32_t S[R];                                                        // S[r]: state of source k = 64r + lane
#pragma unroll
    for (int r = 0; r < R; r++) S[r] = (r == R - 1 && lane == 63) ? 0u : DPB_INF;   // before block 0: only column 0
    if (lane == 0) mml[0] = 0;
    uint32_t bad = 0;
    uint4 nx[PREFETCH ? NQ : 1];
    const uint32_t ngroups = (nblocks + F - 1) / F;
    auto row_ptr = [&](uint32_t g, int rt) {
        const uint32_t b = min(g * F + F - 1, nblocks - 1);
        return reinterpret_cast<const uint4 *>(Wt + (size_t)b * WN * WN + (size_t)(64 * rt + lane) * WN);
    };
    if (PREFETCH) {
#pragma unroll
        for (int rt = 0; rt < R; rt++)
#pragma unroll
            for (int i = 0; i < 4 * R; i++) nx[rt * 4 * R + i] = row_ptr(0, rt)[i];
    }
    for (uint32_t b = 0; b < ngroups; b++) {
#pragma unroll
        for (int r = 0; r < R; r++) Sg[(size_t)b * WN + 64 * r + lane] = (uint8_t)min(S[r], DPB_INF);
        uint4 cur[NQ];
        if (PREFETCH) {
#pragma unroll
            for (int i = 0; i < NQ; i++) cur[i] = nx[i];
            if (b + 1 < ngroups) {
#pragma unroll
                for (int rt = 0; rt < R; rt++)
#pragma unroll
                    for (int i = 0; i < 4 * R; i++) nx[rt * 4 * R + i] = row_ptr(b + 1, rt)[i];
            }
        } else {
#pragma unroll
            for (int rt = 0; rt < R; rt++)
#pragma unroll
                for (int i = 0; i < 4 * R; i++) cur[rt * 4 * R + i] = row_ptr(b, rt)[i];
        }
        uint32_t best[R];
#pragma unroll
        for (int rt = 0; rt < R; rt++) {                                   // target t = 64*rt + lane
            uint32_t acc = DPB_INF;
#pragma unroll
            for (int rs = 0; rs < R; rs++) {                               // sources 64*rs .. 64*rs+63
#pragma unroll
                for (int k = 0; k < 64; k++) {
                    const uint4 q = cur[rt * 4 * R + rs * 4 + (k >> 4)];
                    const uint32_t word = ((k >> 2) & 3) == 0 ? q.x : ((k >> 2) & 3) == 1 ? q.y : ((k >> 2) & 3) == 2 ? q.z : q.w;
                    const uint32_t sk = (uint32_t)__builtin_amdgcn_readlane((int)S[rs], k);
                    acc = min(acc, max(sk, (word >> (8 * (k & 3))) & 255u));
                }
            }
            best[rt] = acc;
        }
#pragma unroll
        for (int rt = 0; rt < R; rt++) S[rt] = best[rt];   // minmaxlength values are written by k_dp_expand
    }
    if (__ballot(bad != 0) && lane == 0) flag[DP_WINDOW] = 1;
}

// The same walk on six waves (round 4).  One wave alone spends 4 instructions per (source, target) pair -- 1.2 us per group of
// 128 x 128, all of it instruction issue.  Waves 0..3 take a quarter of the sources each (their part of every target's row,
// fetched a group ahead), leave their partial minima in LDS and, behind ONE barrier per group (the table alternates between
// two copies), every wave folds the four parts into the next state.  Wave 4 keeps the state too and is the only one that stores
// (Sg): a store in flight would make every use of a fetched row wait for all of the wave's loads (one counter for both).
// Wave 5 touches the lines of the matrix PF groups ahead (see k_dpw_chain2).
template <int R>
__global__ __launch_bounds__(384) void k_dp_chain6(const uint8_t *__restrict__ Wt, uint32_t n, uint32_t nblocks, uint32_t F, uint8_t *__restrict__ Sg,
                                                   uint32_t *__restrict__ mml)
{
    constexpr uint32_t WN = 64 * R, PF = 6;
    __shared__ uint32_t part[2][4][WN];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ngroups = (nblocks + F - 1) / F;
    auto last_block = [&](uint32_t g) { return min(g * F + F - 1, nblocks - 1); };
    if (wv == 5) {
        constexpr uint32_t NL = R == 1 ? 1 : R * R / 2;          // loads of 64 lines each that cover WN * WN bytes
        for (uint32_t g = 0; g < ngroups; g++) {   // role "touch": one barrier per group (dp_dev.h, THE BARRIER COUNT)
            const char *p = reinterpret_cast<const char *>(Wt) + (size_t)last_block(min(g + PF, ngroups - 1)) * WN * WN + (size_t)(R == 1 ? lane & 31 : lane) * 128;
            for (uint32_t i = 0; i < NL; i++) asm volatile("global_load_dword v127, %0, off" : : "v"(p + (size_t)i * 8192) : "v127", "memory");
            dpw_lds_barrier();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    uint32_t S[R];                                                        // S[r]: state of source k = 64r + lane
#pragma unroll
    for (int r = 0; r < R; r++) S[r] = (r == R - 1 && lane == 63) ? 0u : DPB_INF;   // before block 0: only column 0
    if (wv == 4) {
        if (lane == 0) mml[0] = 0;
        for (uint32_t g = 0; g < ngroups; g++) {   // role "store": one barrier per group (dp_dev.h, THE BARRIER COUNT)
#pragma unroll
            for (int r = 0; r < R; r++) Sg[(size_t)g * WN + 64 * r + lane] = (uint8_t)min(S[r], DPB_INF);
            dpw_lds_barrier();
#pragma unroll
            for (int r = 0; r < R; r++)
                S[r] = min(min(part[g & 1][0][64 * r + lane], part[g & 1][1][64 * r + lane]), min(part[g & 1][2][64 * r + lane], part[g & 1][3][64 * r + lane]));
        }
        return;
    }
    // waves 0..3: sources 16 R wv .. 16 R wv + 16 R - 1, i.e. the uint4 words R wv .. R wv + R - 1 of every target's row
    auto row_ptr = [&](uint32_t g, int rt) {
        return reinterpret_cast<const uint4 *>(Wt + (size_t)last_block(g) * WN * WN + (size_t)(64 * rt + lane) * WN) + R * wv;
    };
    uint4 nx[R * R];
#pragma unroll
    for (int rt = 0; rt < R; rt++)
#pragma unroll
        for (int i = 0; i < R; i++) nx[rt * R + i] = row_ptr(0, rt)[i];
    const uint32_t k0 = 16 * R * wv;                                      // first source of the wave: lane (k0 & 63) of S[k0 >> 6]
    for (uint32_t g = 0; g < ngroups; g++) {   // role "compute": one barrier per group (dp_dev.h, THE BARRIER COUNT)
        uint4 cur[R * R];
#pragma unroll
        for (int i = 0; i < R * R; i++) cur[i] = nx[i];
        {
            const uint32_t gn = min(g + 1, ngroups - 1);
#pragma unroll
            for (int rt = 0; rt < R; rt++)
#pragma unroll
                for (int i = 0; i < R; i++) nx[rt * R + i] = row_ptr(gn, rt)[i];
        }
        uint32_t Ssel = S[0];                                             // the state register that holds the wave's sources
#pragma unroll
        for (int r = 1; r < R; r++) Ssel = (k0 >> 6) == (uint32_t)r ? S[r] : Ssel;
        const uint32_t l0 = k0 & 63;
#pragma unroll
        for (int rt = 0; rt < R; rt++) {
            uint32_t acc = DPB_INF;
#pragma unroll
            for (int j = 0; j < 16 * R; j++) {
                const uint4 q = cur[rt * R + (j >> 4)];
                const uint32_t word = ((j >> 2) & 3) == 0 ? q.x : ((j >> 2) & 3) == 1 ? q.y : ((j >> 2) & 3) == 2 ? q.z : q.w;
                const uint32_t sk = (uint32_t)__builtin_amdgcn_readlane((int)Ssel, (int)(l0 + j));
                acc = min(acc, max(sk, (word >> (8 * (j & 3))) & 255u));
            }
            part[g & 1][wv][64 * rt + lane] = acc;
        }
        dpw_lds_barrier();
#pragma unroll
        for (int r = 0; r < R; r++)
            S[r] = min(min(part[g & 1][0][64 * r + lane], part[g & 1][1][64 * r + lane]), min(part[g & 1][2][64 * r + lane], part[g & 1][3][64 * r + lane]));
    }
}

// Shorten the sequential chain: inside every group of F consecutive blocks the matrices are replaced by
// their running (min,max) products P_i = W_first (x) ... (x) W_i (in place, all groups in parallel), so the
// chain only has to step from group to group (through the last product) and every block's values follow
// from its group's entry state with one independent matrix-vector product (k_dp_expand).
//     (P (x) W)[t][k] = min_u max( P[u][k], W[t][u] )      t: target of W, k: source of P
template <int R>
__global__ __launch_bounds__(256) void k_dp_compose(uint8_t *__restrict__ Wt, uint32_t nblocks, uint32_t F)
{
    constexpr uint32_t WN = 64 * R;
    extern __shared__ uint8_t dyn_lds[];
    uint8_t *P = dyn_lds, *W = dyn_lds + WN * WN;       // [row][col] = [target][source]
    const uint32_t tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * F;
    if (b0 >= nblocks) return;
    const uint32_t b1 = min(b0 + F, nblocks);
    for (uint32_t q = tid * 16; q < WN * WN; q += 256 * 16)
        *reinterpret_cast<uint4 *>(P + q) = *reinterpret_cast<const uint4 *>(Wt + (size_t)b0 * WN * WN + q);
    for (uint32_t b = b0 + 1; b < b1; b++) {
        uint8_t *G = Wt + (size_t)b * WN * WN;
        __syncthreads();
        for (uint32_t q = tid * 16; q < WN * WN; q += 256 * 16)
            *reinterpret_cast<uint4 *>(W + q) = *reinterpret_cast<const uint4 *>(G + q);
        __syncthreads();
        // thread -> a tile of 4 rows t x 8 consecutive sources k, four u per step: the four W words (4 u each) and the four P
        // rows' 8 bytes are read once for 128 (t, k, u) triples; bytes as two pairs of 16-bit lanes per word (even / odd bytes:
        // packed 16-bit max / min do two sources per instruction), a W byte in both lanes by one v_perm.  1.4 instructions per
        // triple (round 4; a row t x 8 sources per thread, one u per step: 2.1)
        for (uint32_t tile = tid; tile < WN * WN / 32; tile += 256) {
            const uint32_t t0 = 4 * (tile / (WN / 8)), k8 = (tile % (WN / 8)) * 8;
            dp_u16x2 acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[a][c] = dp_pair(DPB_INF);
#pragma unroll 2
            for (uint32_t u = 0; u < WN; u += 4) {
                uint32_t w[4];
#pragma unroll
                for (int a = 0; a < 4; a++) w[a] = *reinterpret_cast<const uint32_t *>(W + (t0 + a) * WN + u);
#pragma unroll
                for (int uu = 0; uu < 4; uu++) {
                    const uint2 p8 = *reinterpret_cast<const uint2 *>(P + (u + uu) * WN + k8);
                    const dp_u16x2 pe0 = dp_bits(p8.x & 0x00ff00ffu), po0 = dp_bits((p8.x >> 8) & 0x00ff00ffu),
                                   pe1 = dp_bits(p8.y & 0x00ff00ffu), po1 = dp_bits((p8.y >> 8) & 0x00ff00ffu);
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        const dp_u16x2 ww = dp_bits(__builtin_amdgcn_perm(w[a], w[a], 0x0c000c00u | (uint32_t)uu | ((uint32_t)uu << 16)));
                        acc[a][0] = __builtin_elementwise_min(acc[a][0], __builtin_elementwise_max(ww, pe0));
                        acc[a][1] = __builtin_elementwise_min(acc[a][1], __builtin_elementwise_max(ww, po0));
                        acc[a][2] = __builtin_elementwise_min(acc[a][2], __builtin_elementwise_max(ww, pe1));
                        acc[a][3] = __builtin_elementwise_min(acc[a][3], __builtin_elementwise_max(ww, po1));
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                uint2 o;
                o.x = dp_word(acc[a][0]) | (dp_word(acc[a][1]) << 8);
                o.y = dp_word(acc[a][2]) | (dp_word(acc[a][3]) << 8);
                *reinterpret_cast<uint2 *>(G + (t0 + a) * WN + k8) = o;
            }
        }
        __syncthreads();
        // the product becomes P for the next block of the group
        for (uint32_t q = tid * 16; q < WN * WN; q += 256 * 16)
            *reinterpret_cast<uint4 *>(P + q) = *reinterpret_cast<const uint4 *>(G + q);
    }
}

// state entering block b (64R values) (x) matrix of block b -> minmaxlength of the block's columns
template <int R>
__global__ __launch_bounds__(64) void k_dp_expand(const uint8_t *__restrict__ Wt, const uint8_t *__restrict__ Sg,
                                                  uint32_t n, uint32_t nblocks, uint32_t F, uint32_t *__restrict__ mml,
                                                  unsigned long long *__restrict__ flag, uint32_t first_valid)
{
    // first_valid = f[0] + 1: no block ends before that step, and the reference's sweep leaves its running S there:
    // minmaxlength[j] = n + j, backtrack[j] = -1 (fbg.cpp:1967, 2007-2010 with backtrack_S still size_type(-1))
    constexpr uint32_t WN = 64 * R;
    __shared__ uint8_t s_state[WN];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        __syncthreads();
        for (uint32_t q = lane; q < WN; q += 64) s_state[q] = Sg[(size_t)(b / F) * WN + q];
        __syncthreads();
        const uint8_t *Wb = Wt + (size_t)b * WN * WN;
#pragma unroll
        for (int rt = 0; rt < R; rt++) {
            const uint32_t t = 64 * rt + lane;
            const uint4 *row = reinterpret_cast<const uint4 *>(Wb + (size_t)t * WN);
            uint32_t acc = DPB_INF;
            for (uint32_t q = 0; q < WN / 16; q++) {
                const uint4 w4 = row[q];
                const uint32_t ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int i = 0; i < 16; i++)
                    acc = min(acc, max((uint32_t)s_state[16 * q + i], (ws[i >> 2] >> (8 * (i & 3))) & 255u));
            }
            const uint32_t j = WN * b + 1 + t;
            if (j <= n) {
                if (j < first_valid) mml[j] = n + j;
                else {
                    mml[j] = acc;
                    // exact as long as every value stays below the window: a block longer than the window, or one that
                    // starts at a column whose minimal extension exceeds it, costs more than any value seen (fbg_dp_minmax)
                    if (acc >= (R == 4 ? 255u : 64u * R)) flag[DP_WINDOW] = 1;
                }
            }
        }
    }
}

__global__ void k_dp_bt(const uint32_t *__restrict__ mml, const uint8_t *__restrict__ ext7, uint32_t n, uint32_t window,
                        uint32_t *__restrict__ bt, unsigned long long *__restrict__ flag, uint32_t first_valid)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == 0) { bt[0] = 0; return; }
    if (j < first_valid) { bt[j] = DP_NONE; return; }
    const uint32_t L = mml[j];
    uint32_t best_age = 0;                    // youngest count_solutions-kind candidate (age <= its value == L)
    bool s_kind = false;                      // candidate of age L with a smaller value: the S / backtrack_S branch
    const uint32_t amax = min(window, j);
    for (uint32_t a = 1; a <= amax; a++) {
        const uint32_t x = j - a;
        if (ext7[x] > a) continue;            // block [x, j) not valid yet: f[x]+1 > j
        const uint32_t v = mml[x];
        if (v > n) continue;                  // a column before first_valid: no solution ends there (fbg.cpp:1973)
        if (a > v) { if (a == L) s_kind = true; }
        else if (v == L && best_age == 0) best_age = a;
    }
    if (s_kind) bt[j] = j - L;
    else if (best_age) bt[j] = j - best_age;
    else { bt[j] = 0; flag[DP_WINDOW] = 1; }
}

// ---- host: the one launcher of the chain, and the BYTES rung ---------------------------------------------------------------

// ext / amin / out / flag / first_valid: k_dp_blockW and k_dp_expand.  Fg: blocks per group of the chain (a chain step costs
// ~0.5 us).  Sg: ngroups * 64 R bytes, the state entering each group.  The matrices go to ctx->tmp.
template <int R>
static int dp_byte_chain(fbg_ctx *ctx, const uint8_t *ext, const uint8_t *amin, uint64_t n, uint32_t Fg, uint8_t *Sg, uint32_t *out,
                         unsigned long long *flag, uint32_t first_valid)
{
    hipStream_t st = ctx->stream;
    constexpr uint32_t WN = 64u * R;
    const uint32_t nblocks = (uint32_t)((n + WN - 1) / WN), ngroups = (nblocks + Fg - 1) / Fg;
    FBG_TRY(fbg_reserve(ctx, ctx->tmp, (size_t)nblocks * WN * WN));
    uint8_t *Wt = ctx->tmp.as<uint8_t>();
    const size_t lds = (size_t)WN * DPB_PADDED(WN) + 2 * WN + 2 * WN * (WN / 64), lds2 = 2 * (size_t)WN * WN;
    const unsigned grid = fbg_blocks(nblocks, 1, 256 * 16);
    if (lds > 64 * 1024)
        FBG_HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_dp_blockW<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (lds2 > 64 * 1024)
        FBG_HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_dp_compose<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    hipLaunchKernelGGL((k_dp_blockW<R>), dim3(grid), dim3(64 * R), lds, st, ext, amin, (uint32_t)n, nblocks, Wt);
    hipLaunchKernelGGL((k_dp_compose<R>), dim3(ngroups), dim3(256), lds2, st, Wt, nblocks, Fg);
    if (ctx->opt.dp_chain1) hipLaunchKernelGGL((k_dp_chain<R>), dim3(1), dim3(64), 0, st, Wt, (uint32_t)n, nblocks, Fg, Sg, out, flag);
    else hipLaunchKernelGGL((k_dp_chain6<R>), dim3(1), dim3(384), 0, st, Wt, (uint32_t)n, nblocks, Fg, Sg, out);
    hipLaunchKernelGGL((k_dp_expand<R>), dim3(grid), dim3(64), 0, st, Wt, Sg, (uint32_t)n, nblocks, Fg, out, flag, first_valid);
    return FBG_OK;
}

int fbg_dp_byte_chain(fbg_ctx *ctx, int R, const uint8_t *ext, const uint8_t *amin, uint64_t n, uint32_t Fg, uint8_t *Sg, uint32_t *out,
                      unsigned long long *flag, uint32_t first_valid)
{
    return dp_for_R<4>(R, [&](auto r) { return dp_byte_chain<decltype(r)::value>(ctx, ext, amin, n, Fg, Sg, out, flag, first_valid); });
}

// BYTES(Rt): a sweep that works straight from f (no bucket order needed), in a window of 64 Rt columns.
// Exactness of a window: columns whose minimal extension does not fit it are no candidates inside it, and a
// block longer than the window is not looked at -- both cost more than the window, so as long as every
// minmaxlength found stays BELOW the window (the flag k_dp_expand raises otherwise) no such block could have
// improved on it and the values are the reference's.  (Induction over j: the first column where the windowed
// value exceeds the true one would need a true optimum through a dead candidate or a long block, i.e. a true
// value above the window, yet the windowed value is below it and never smaller than the true one.)
int fbg_rung_bytes(fbg_ctx *ctx, DpSweep &sw, const DpRung &r, bool *settled)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)sw.n;
    uint8_t *ext7 = ctx->dp_e.as<uint8_t>(), *clen = ctx->dp_f.as<uint8_t>();   // count / bcount of the literal sweep: free on this path
    ctx->dp_attempts++;
    FBG_TRY(fbg_dp_clear_window(ctx, sw.sc));
    hipLaunchKernelGGL(k_dp_prep, dim3(fbg_blocks(sw.n + 1, 256)), dim3(256), 0, st, sw.e, n, r.tile ? 127u : 255u, ext7, clen);
    if (r.tile) {
        hipLaunchKernelGGL(k_dp_tile, dim3(1), dim3(64), 0, st, ext7, clen, n, sw.mml, sw.bt, sw.sc);
    } else {
        uint8_t *Sg = ctx->dp_c.as<uint8_t>();                                  // (n + 2) * 4 bytes >= ngroups * WN: free on this path
        FBG_TRY(fbg_dp_byte_chain(ctx, (int)r.size, ext7, nullptr, sw.n, 16, Sg, sw.mml, sw.sc, sw.first_valid));
        hipLaunchKernelGGL(k_dp_bt, dim3(fbg_blocks(sw.n + 1, 256)), dim3(256), 0, st, sw.mml, ext7, n, 64u * r.size, sw.bt, sw.sc, sw.first_valid);
    }
    return fbg_dp_settled(ctx, sw.sc, settled);
}
