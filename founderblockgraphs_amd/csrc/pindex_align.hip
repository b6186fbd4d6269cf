// pindex_align.hip -- the edit distance of each read to a row that carries its chain (fbg_pindex_chains_align) and the
// alignment path behind it (fbg_pindex_chains_cigar).
//
//   k_pa_prefix / k_pa_prepare / k_pa_gather   per (row, block) the row's text position; per read the window of its chain
//                                    on the chosen row; the windows gathered back to back;
//   k_pa_edit                        a wave per read: Myers' bit-vector recurrence forwards, then backwards, the state in
//                                    registers (up to PA_REG_WORDS words of 64 read symbols) or in LDS;
//   k_pg_sizes / k_pg_path / k_pg_compact   the backward pass again with its column history kept, the walk from (L, N)
//                                    to (0, 0) along it, and the runs of the path back to back.
// pa_prefix and pa_windows launch k_pa_prefix, k_pa_gather and k_pa_edit for fbg_pindex_pairs_align (pindex_pairs_align.hip)
// too, on that call's own buffers.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

// pref[j * m + r] = p(r, j): one lane per row steps over the blocks, so a wave reads and writes 64 consecutive rows
__global__ void k_pa_prefix(const uint32_t *node_of, const uint64_t *loff, uint64_t m, uint64_t nb, uint32_t *pref)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    uint32_t run = 0;
    for (uint64_t j = 0; j < nb; j++) {
        pref[j * m + r] = run;
        const uint32_t v = node_of[j * m + r];
        if (v != PR_NONE) run += (uint32_t)(loff[v + 1] - loff[v]);
    }
}

// One lane per read, after k_pr_chain chose the row (first_row; rec, place, off as there; q: q_start per seed): the
// diagonals of the chain's anchors on that row, the window, the skip status and the block, node and offset at which
// the window starts (a search of the row's column of pref).  Writes row and, where nothing is aligned, PA_NONE into
// the three other outputs (out: 4 n); wlen[R] = |W| of an aligned read, else 0, wlen[n] = 0.  ctr[1 .. 4]: reads
// aligned, too long, too wide, and the cells, summed per wave before the atomic.
__global__ void k_pa_prepare(PaDev d, const uint4 *rec, const uint32_t *place, const uint64_t *off, const uint32_t *q,
                             const uint32_t *first_row, uint64_t n, uint64_t pad, uint64_t max_window, uint4 *info, uint4 *start,
                             uint64_t *wlen, uint32_t *out, unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kind = -1;                // 0 aligned, 1 too long, 2 too wide
    unsigned long long cells = 0;
    if (R == n) wlen[n] = 0;
    if (R < n) {
        const uint64_t o0 = off[R], len = off[R + 1] - o0, L = d.roff[R + 1] - d.roff[R];
        const uint32_t r = len ? first_row[R] : PR_NONE;
        uint4 in = make_uint4(r, 0, 0, (uint32_t)L), at = make_uint4(0, 0, 0, 0);
        if (r != PR_NONE) {
            long long dmin = 0, dmax = 0;
            for (uint64_t a = 0; a < len; a++) {
                const uint4 rc = rec[place[o0 + a]];
                const long long dg = (long long)d.pref[(uint64_t)rc.w * d.m + r] + rc.y - (long long)q[rc.z];
                if (a == 0 || dg < dmin) dmin = dg;
                if (a == 0 || dg > dmax) dmax = dg;
            }
            const uint64_t jl = (d.nb - 1) * d.m + r;
            const uint32_t vl = d.node_of[jl];
            const long long glen = (long long)d.pref[jl] + (vl != PR_NONE ? (long long)(d.loff[vl + 1] - d.loff[vl]) : 0);
            const long long lo = dmin - (long long)pad, hi = dmax + (long long)L + (long long)pad;
            const uint64_t w0 = lo > 0 ? (uint64_t)lo : 0, w1 = hi < glen ? (uint64_t)hi : (uint64_t)glen;
            kind = L > PA_MAX_READ ? 1 : max_window && w1 - w0 > max_window ? 2 : 0;
            if (kind == 0) {
                uint64_t a = 0, b = d.nb - 1;
                while (a < b) {
                    const uint64_t mid = a + (b - a + 1) / 2;
                    if (d.pref[mid * d.m + r] <= w0) a = mid; else b = mid - 1;
                }
                in.y = (uint32_t)w0;
                in.z = (uint32_t)(w1 - w0);
                at = make_uint4((uint32_t)a, d.node_of[a * d.m + r], (uint32_t)w0 - d.pref[a * d.m + r], 0);
                cells = (unsigned long long)L * (w1 - w0);
            }
        }
        info[R] = in;
        start[R] = at;
        wlen[R] = in.z;
        out[R] = r;
        if (kind != 0) out[n + R] = out[2 * n + R] = out[3 * n + R] = PA_NONE;
    }
    for (int off2 = FBG_WAVE / 2; off2 > 0; off2 >>= 1) cells += __shfl_xor(cells, off2);
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    for (int b = 0; b < 3; b++) {
        const unsigned long long mk = __ballot(kind == b);
        if (mk && first) atomicAdd(&ctr[1 + b], (unsigned long long)__popcll(mk));
    }
    if (cells && first) atomicAdd(&ctr[4], cells);
}

// A wave per read writes its window W = G_r[w0 : w1) to win + woff[R]: label after label of the row's nodes from the
// start node on, the lanes taking consecutive bytes of a label; cells without a node are passed over.  Every loop is
// bounded: a label by its length, the window by |W|, the row's cells by block nb.
__global__ __launch_bounds__(FBG_WAVE) void k_pa_gather(PaDev d, const uint4 *info, const uint4 *start, const uint64_t *woff, uint8_t *win)
{
    const uint64_t R = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t wl = in.z;
    if (wl == 0) return;
    const uint4 at = start[R];
    if (at.y == PR_NONE) return;
    uint8_t *dst = win + woff[R];
    uint64_t j = at.x, a = d.loff[at.y] + at.z, b = d.loff[at.y + 1];
    uint32_t done = 0;
    for (;;) {
        const uint32_t take = b - a < (uint64_t)(wl - done) ? (uint32_t)(b - a) : wl - done;
        for (uint32_t x = lane; x < take; x += FBG_WAVE) dst[done + x] = d.labels[a + x];
        done += take;
        if (done == wl) return;
        uint32_t v;
        do {
            if (++j >= d.nb) return;
            v = d.node_of[j * d.m + in.x];
        } while (v == PR_NONE);
        a = d.loff[v];
        b = d.loff[v + 1];
    }
}

// 64 text symbols of a pass per load, lane t takes column j0 + t; REV: the text backwards
template <bool REV> __device__ __forceinline__ int pa_chunk(const uint8_t *W, uint32_t wl, uint32_t j0, unsigned lane)
{
    const uint32_t j = j0 + lane;
    return j < wl ? (int)W[REV ? wl - 1 - j : j] : 0;
}

// One pass of a wave over the text W[0 .. wl) with a read of exactly NW words, the state in registers: lane i holds
// read symbols i, 64 + i, ...  (256: no symbol, equal to no byte, which masks the last word to L % 64 bits), a text byte
// is made wave-uniform by readlane and its match word is one ballot per read word.  D(L, j) is followed at bit L - 1 of
// the last word; -> best = min_j D(L, j) and bestj, the smallest j that attains it (D(L, 0) = L).  REV: the read and the
// text backwards and D(0, j) = j, which is the carry-in 1 of the first word.
// HIST (fbg_pindex_chains_cigar): lane 0 also writes pv and mv of every word after column j to hist[(j * NW + w) * 2].
template <int NW, bool REV, bool HIST = false>
__device__ __forceinline__ void pa_pass_reg(const uint8_t *P, uint32_t L, const uint8_t *W, uint32_t wl, unsigned lane, uint32_t &best,
                                            uint32_t &bestj, uint64_t *hist = nullptr)
{
    int p[NW];
    uint64_t pv[NW], mv[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint32_t i = w * 64 + lane;
        p[w] = i < L ? (int)P[REV ? L - 1 - i : i] : 256;
        pv[w] = ~0ull;
        mv[w] = 0;
    }
    const uint64_t top = 1ull << ((L - 1) & 63);
    uint32_t score = L;
    best = L;
    bestj = 0;
    for (uint32_t j0 = 0; j0 < wl; j0 += 64) {
        const int chunk = pa_chunk<REV>(W, wl, j0, lane);
        const uint32_t cnt = wl - j0 < 64 ? wl - j0 : 64;
        for (uint32_t t = 0; t < cnt; t++) {
            const int c = __builtin_amdgcn_readlane(chunk, t);
            int h = REV ? 1 : 0;
#pragma unroll
            for (int w = 0; w < NW; w++) h = pa_step(__ballot(p[w] == c), pv[w], mv[w], h, w == NW - 1 ? top : 1ull << 63);
            if (HIST && lane == 0) {
                uint64_t *col = hist + (uint64_t)(j0 + t) * (2 * NW);
#pragma unroll
                for (int w = 0; w < NW; w++) { col[2 * w] = pv[w]; col[2 * w + 1] = mv[w]; }
            }
            score += h;
            if (score < best) { best = score; bestj = j0 + t + 1; }
        }
    }
}

// The same pass for a read of nw > PA_REG_WORDS words: the read (rd) and the state (st: pv, then mv) in LDS and a loop
// over the words.  Every lane computes and stores the same state and reads back what it stored itself, and a lane reads
// the read symbols it staged itself: no lane waits for another, so there is no barrier.  HIST: lane w < nw also writes
// word w's pv and mv after column j (which it stored itself) to hist[(j * nw + w) * 2], 16 consecutive bytes per lane.
template <bool REV, bool HIST = false>
__device__ __forceinline__ void pa_pass_lds(const uint8_t *P, uint32_t L, uint32_t nw, const uint8_t *W, uint32_t wl, unsigned lane,
                                            uint8_t *rd, uint64_t *st, uint32_t &best, uint32_t &bestj, uint64_t *hist = nullptr)
{
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t i = w * 64 + lane;
        rd[i] = i < L ? P[REV ? L - 1 - i : i] : 0;
        st[w] = ~0ull;
        st[PA_MAX_READ / 64 + w] = 0;
    }
    const uint64_t top = 1ull << ((L - 1) & 63);
    uint32_t score = L;
    best = L;
    bestj = 0;
    for (uint32_t j0 = 0; j0 < wl; j0 += 64) {
        const int chunk = pa_chunk<REV>(W, wl, j0, lane);
        const uint32_t cnt = wl - j0 < 64 ? wl - j0 : 64;
        for (uint32_t t = 0; t < cnt; t++) {
            const int c = __builtin_amdgcn_readlane(chunk, t);
            int h = REV ? 1 : 0;
            for (uint32_t w = 0; w < nw; w++) {
                const uint32_t i = w * 64 + lane;
                uint64_t pv = st[w], mv = st[PA_MAX_READ / 64 + w];
                h = pa_step(__ballot(i < L && rd[i] == c), pv, mv, h, w == nw - 1 ? top : 1ull << 63);
                st[w] = pv;
                st[PA_MAX_READ / 64 + w] = mv;
            }
            if (HIST && lane < nw) {
                uint64_t *col = hist + ((uint64_t)(j0 + t) * nw + lane) * 2;
                col[0] = st[lane];
                col[1] = st[PA_MAX_READ / 64 + lane];
            }
            score += h;
            if (score < best) { best = score; bestj = j0 + t + 1; }
        }
    }
}

template <bool REV>
__device__ __forceinline__ void pa_pass(const uint8_t *P, uint32_t L, const uint8_t *W, uint32_t wl, unsigned lane, uint8_t *rd, uint64_t *st,
                                        uint32_t &best, uint32_t &bestj)
{
    const uint32_t nw = (L + 63) / 64;         // the tier: the same in every lane
    if (nw == 1) pa_pass_reg<1, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 2) pa_pass_reg<2, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 3) pa_pass_reg<3, REV>(P, L, W, wl, lane, best, bestj);
    else if (nw == 4) pa_pass_reg<4, REV>(P, L, W, wl, lane, best, bestj);
    else pa_pass_lds<REV>(P, L, nw, W, wl, lane, rd, st, best, bestj);
}

// A wave per aligned read, 1 <= L <= PA_MAX_READ: the forward pass over the window gives edits and the smallest end e,
// the backward pass over W[0 : e) the largest start.  out as in k_pa_prepare.
__global__ __launch_bounds__(FBG_WAVE) void k_pa_edit(PaDev d, const uint4 *info, const uint64_t *woff, const uint8_t *win, uint64_t n,
                                                     uint32_t *out)
{
    __shared__ uint8_t rd[PA_MAX_READ];
    __shared__ uint64_t st[2 * (PA_MAX_READ / 64)];
    const uint64_t R = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t L = in.w;
    if (in.z == 0 || L == 0 || L > PA_MAX_READ) return;
    const uint8_t *P = d.reads + d.roff[R], *W = win + woff[R];
    uint32_t edits, e, back, j;
    pa_pass<false>(P, L, W, in.z, lane, rd, st, edits, e);
    pa_pass<true>(P, L, W, e, lane, rd, st, back, j);
    if (lane == 0) {
        out[n + R] = edits;
        out[2 * n + R] = in.y + e - j;
        out[3 * n + R] = in.y + e;
    }
}

// ---- alignment path (fbg_pindex_chains_cigar) -----------------------------------------------------------------------
// With P' and T' the reversed read and the reversed T = G_r[t_start : t_end), D'(a, b) = lev(P'[:a], T'[:b]) is
// E(L - a, N - b) of the definition, and the second pass of k_pa_edit over exactly the N columns of T' computes it.  The
// history holds, for b = 1 .. N and every word w of the read, pv and mv after column b at hist[((b - 1) * nw + w) * 2]:
// bit a - 1 of the pair is D'(a, b) - D'(a - 1, b).  Column 0 is D'(a, 0) = a and is not stored.

// One lane per read of the last align call (and one for the entry n): units of 8 bytes of history in device memory
// (reads of more than PA_REG_WORDS words) and run slots.  ctr as PG_CTR says, summed per wave before the atomic.
__global__ void k_pg_sizes(const uint4 *info, const uint32_t *out, uint64_t n, uint64_t *hsz, uint64_t *ssz, unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;                // 0 .. 3: 1 .. 4 words, 4: more
    unsigned long long cols = 0;
    if (R <= n) {
        uint64_t h = 0, s = 0;
        if (R < n && out[n + R] != PA_NONE && info[R].w != 0) {
            const uint32_t nw = (info[R].w + 63) / 64;
            cols = out[3 * n + R] - out[2 * n + R];
            tier = nw <= PA_REG_WORDS ? (int)nw - 1 : PA_REG_WORDS;
            if (tier == PA_REG_WORDS) h = 2ull * nw * cols;
            s = 2ull * out[n + R] + 1;
        }
        hsz[R] = h;
        ssz[R] = s;
    }
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    for (int b = 0; b <= PA_REG_WORDS; b++) {
        const unsigned long long mk = __ballot(tier == b);
        if (!mk) continue;                                   // the same in every lane of the wave
        unsigned long long widest = tier == b ? cols : 0;
        for (int off = FBG_WAVE / 2; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(widest, off);
            widest = o > widest ? o : widest;
        }
        if (first) {
            atomicAdd(&ctr[1], (unsigned long long)__popcll(mk));
            atomicAdd(&ctr[3 + b], (unsigned long long)__popcll(mk));
            atomicMax(&ctr[8 + b], widest);
        }
    }
    for (int off = FBG_WAVE / 2; off > 0; off >>= 1) cols += __shfl_xor(cols, off);
    if (cols && first) atomicAdd(&ctr[2], cols);
}

// D'(a, b) from the first row D'(0, b) = b and the column's words: lane w sums the bits of word w below row a, and the
// wave adds the lanes up.  The same value in every lane.
__device__ __forceinline__ int pg_cell(const uint64_t *hist, uint32_t nw, uint32_t a, uint32_t b, unsigned lane)
{
    if (b == 0) return (int)a;
    int part = 0;
    if (lane < nw && lane * 64 < a) {
        const uint64_t *col = hist + ((uint64_t)(b - 1) * nw + lane) * 2;
        const uint32_t rows = a - lane * 64;
        const uint64_t mask = rows >= 64 ? ~0ull : (1ull << rows) - 1;
        part = __popcll(col[0] & mask) - __popcll(col[1] & mask);
    }
    for (int off = FBG_WAVE / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
    return (int)b + part;
}

// D'(a, b) - D'(a - 1, b) for a >= 1
__device__ __forceinline__ int pg_vert(const uint64_t *hist, uint32_t nw, uint32_t a, uint32_t b)
{
    if (b == 0) return 1;
    const uint64_t *col = hist + ((uint64_t)(b - 1) * nw + ((a - 1) >> 6)) * 2;
    const uint64_t bit = 1ull << ((a - 1) & 63);
    return (col[0] & bit) ? 1 : (col[1] & bit) ? -1 : 0;
}

// A wave per read first + blockIdx.x.  NW = 1 .. 4: the reads of exactly NW words, the history in the launch's dynamic
// LDS of cap columns; NW = 0: the reads of more words, the history at scratch + (hoff[R] - hbase) units.  After the
// pass the wave walks from (L, N) to (0, 0), every lane the same walk, and lane 0 writes the runs to slots + soff[R]
// (2 * edits + 1 of them) and their number to cnt[R] and nops[R], which the host cleared.  The walk takes at most L + N
// steps; one that has not arrived by then, or finds a cell that no move explains, or more runs than slots, leaves zero
// runs and adds to ctr[0].
template <int NW>
__global__ __launch_bounds__(FBG_WAVE) void k_pg_path(PaDev d, const uint4 *info, const uint64_t *woff, const uint8_t *win, const uint32_t *out,
                                                     uint64_t n, uint64_t first, uint32_t cap, const uint64_t *hoff, uint64_t hbase,
                                                     uint64_t *scratch, const uint64_t *soff, uint32_t *slots, uint64_t *cnt, uint32_t *nops,
                                                     unsigned long long *ctr)
{
    extern __shared__ uint64_t pg_lds[];
    __shared__ uint8_t rd[NW ? 8 : PA_MAX_READ];
    __shared__ uint64_t st[NW ? 1 : 2 * (PA_MAX_READ / 64)];
    const uint64_t R = first + blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint32_t edits = out[n + R];
    const uint4 in = info[R];
    const uint32_t L = in.w, nw = (L + 63) / 64;
    if (edits == PA_NONE || L == 0 || L > PA_MAX_READ || (NW ? nw != NW : nw <= PA_REG_WORDS)) return;
    const uint32_t ts = out[2 * n + R], N = out[3 * n + R] - ts;
    if (NW && N > cap) {          // the launch's LDS holds cap columns: the host sized it by the widest T of the tier
        if (lane == 0) atomicAdd(&ctr[0], 1ull);
        return;
    }
    const uint8_t *P = d.reads + d.roff[R], *T = win + woff[R] + (ts - in.y);
    uint64_t *hist = NW ? pg_lds : scratch + (hoff[R] - hbase);
    uint32_t best, bestj;
    if constexpr (NW != 0) pa_pass_reg<NW, true, true>(P, L, T, N, lane, best, bestj, hist);
    else pa_pass_lds<true, true>(P, L, nw, T, N, lane, rd, st, best, bestj, hist);
    __syncthreads();              // the history was written by lane 0 (by lane w) and is read by every lane
    uint32_t a = L, b = N, runs = 0, code = 0, len = 0;
    int cur = pg_cell(hist, nw, a, b, lane), left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
    bool bad = cur != (int)edits;
    uint32_t *slot = slots + soff[R];
    for (uint32_t step = 0; step < L + N && (a | b) != 0 && !bad; step++) {
        uint32_t op;
        if (a && b) {
            const int diag = left - pg_vert(hist, nw, a, b - 1);
            const bool eq = P[L - a] == T[N - b];
            if (cur == diag + (eq ? 0 : 1)) {
                op = eq ? 7 : 8;
                a--, b--;
                cur = diag;
                left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
            } else if (pg_vert(hist, nw, a, b) == 1) {
                op = 1;
                a--;
                cur--;
                left = diag;
            } else {
                op = 2;
                bad = cur != left + 1;
                b--;
                cur = left;
                left = b ? pg_cell(hist, nw, a, b - 1, lane) : 0;
            }
        } else if (a) {           // the text is used up: D'(a, 0) = a
            op = 1;
            a--;
            cur--;
        } else {                  // the read is used up: D'(0, b) = b
            op = 2;
            b--;
            cur--;
        }
        if (op == code) { len++; continue; }
        if (len) {
            if (runs > 2 * edits) bad = true;
            else if (lane == 0) slot[runs] = len << 4 | code;
            runs++;
        }
        code = op;
        len = 1;
    }
    if (len && !bad) {
        if (runs > 2 * edits) bad = true;
        else if (lane == 0) slot[runs] = len << 4 | code;
        runs++;
    }
    if ((a | b) != 0 || cur != 0) bad = true;
    if (lane == 0) {
        if (bad) atomicAdd(&ctr[0], 1ull);
        else { cnt[R] = runs; nops[R] = runs; }
    }
}

// One lane per read copies its runs from their slots to ops + off[R]
__global__ void k_pg_compact(const uint64_t *soff, const uint32_t *slots, const uint64_t *off, uint64_t n, uint32_t *ops)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R >= n) return;
    const uint64_t o = off[R], k = off[R + 1] - o, s = soff[R];
    for (uint64_t x = 0; x < k; x++) ops[o + x] = slots[s + x];
}

// what the alignment kernels read: the row table, the prefix table and the reads of the last seeds call
PaDev pa_dev(const fbg_pindex *ix)
{
    const PrState &w = ix->rw;
    PaDev a;
    a.node_of = w.node_of.as<uint32_t>();
    a.pref = ix->al.pref.as<uint32_t>();
    a.labels = w.labels.as<uint8_t>();
    a.loff = w.loff.as<uint64_t>();
    a.reads = ps_reads(ix);
    a.roff = ps_roff(ix);
    a.m = w.m;
    a.nb = ix->seg_nb;
    return a;
}

// The prefix table for the call that is running: reserved, and built where no successful call has built it
int pa_prefix(fbg_pindex *ix)
{
    PaState &al = ix->al;
    const PrState &w = ix->rw;
    FBG_TRY(px_reserve(ix, al.pref, ix->seg_nb * w.m * 4));
    if (!al.has_pref)             // the flag is set at the end of the call, once the table is known to be written
        hipLaunchKernelGGL(k_pa_prefix, dim3(fbg_blocks(w.m, 64)), dim3(64), 0, ix->ctx->stream, (const uint32_t *)w.node_of.as<uint32_t>(),
                           (const uint64_t *)w.loff.as<uint64_t>(), w.m, ix->seg_nb, al.pref.as<uint32_t>());
    return FBG_OK;
}

// A wave per read gathers its window, a wave per read runs the two passes: n reads, n below 2^31
void pa_windows(fbg_pindex *ix, const PaDev &a, uint64_t n, const uint4 *info, const uint4 *start, const uint64_t *woff, uint8_t *win, uint32_t *out)
{
    hipStream_t st = ix->ctx->stream;
    hipLaunchKernelGGL(k_pa_gather, dim3((unsigned)n), dim3(FBG_WAVE), 0, st, a, info, start, woff, win);
    hipLaunchKernelGGL(k_pa_edit, dim3((unsigned)n), dim3(FBG_WAVE), 0, st, a, info, woff, (const uint8_t *)win, n, out);
}

// ---- alignment (fbg_pindex_chains_align / _align_stats) ------------------------------------------------------------------
// pr_prepare and k_pr_chain as in fbg_pindex_chains_rows (into buffers of the alignment state, so that call's results
// stay), the prefix table on the first call, k_pa_prepare, a scan of the window lengths, the host's look at their sum,
// the windows gathered into scratch of that size, and a wave per read for the two passes.
extern "C" int fbg_pindex_chains_align(fbg_pindex *ix, uint64_t pad, uint64_t max_window, uint32_t *row, uint32_t *edits,
                                       uint32_t *t_start, uint32_t *t_end, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    PaState &al = ix->al;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_align", PS_CHAINS));
    std::fill(al.stat, al.stat + 5, (uint64_t)0);
    const uint64_t n = c.n;
    px_begin(ix, PS_ALIGN);                               // the paths belong to the align call they were traced from
    al.on_device = false;
    al.n = n;
    if (n == 0) { px_finish(ix, PS_ALIGN); return FBG_OK; }
    if (n > 0x7fffffffull)        // a wave, and so a workgroup, per read
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_chains_align: %llu reads; a call takes fewer than 2^31", (unsigned long long)n);
    uint32_t *host[4] = {row, edits, t_start, t_end};
    if (c.total == 0) {          // every chain is empty, and fbg_pindex_chains may have left nothing on the device
        for (uint32_t *h : host)
            if (h) std::fill(h, h + n, (uint32_t)PA_NONE);
        px_finish(ix, PS_ALIGN);
        return FBG_OK;
    }
    if (pad > (1ull << 33)) pad = 1ull << 33;         // positions and read offsets are below 2^32: beyond this nothing changes
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, al.pref, ix->seg_nb * w.m * 4));      // before ev0; pa_prefix then finds it there
    FBG_TRY(px_reserve(ix, al.nrows, 2 * n * 4));
    for (DevBuf *b : {&al.info, &al.start, &al.out}) FBG_TRY(px_reserve(ix, *b, n * 16));
    for (DevBuf *b : {&al.wlen, &al.woff}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    FBG_TRY(px_reserve(ix, al.ctr, 5 * 8));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));                       // records ev0
    FBG_TRY(pa_prefix(ix));
    const PaDev a = pa_dev(ix);
    auto *ctr = al.ctr.as<unsigned long long>();
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, 5 * 8, st));
    const uint4 *rec = w.rec.as<uint4>();
    const uint32_t *place = c.out.as<uint32_t>();
    const uint64_t *off = c.off.as<uint64_t>();
    uint32_t *nr = al.nrows.as<uint32_t>(), *out = al.out.as<uint32_t>();
    pr_chain_launch(ix, d, n, 0, nr, nr + n, nullptr, ctr);
    uint64_t *wlen = al.wlen.as<uint64_t>(), *woff = al.woff.as<uint64_t>();
    hipLaunchKernelGGL(k_pa_prepare, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, a, rec, place, off, (const uint32_t *)ix->sq.as<uint32_t>(),
                       (const uint32_t *)(nr + n), n, pad, max_window, al.info.as<uint4>(), al.start.as<uint4>(), wlen, out, ctr);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, wlen, woff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, woff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (total) {
        FBG_TRY(px_reserve(ix, al.win, total));
        pa_windows(ix, a, n, al.info.as<uint4>(), al.start.as<uint4>(), woff, al.win.as<uint8_t>(), out);
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_TRY(px_record_end(ix));
    uint64_t stat[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 4; k++)
        if (host[k]) FBG_HIP_TRY(ctx, hipMemcpyAsync(host[k], out + k * n, n * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(stat, ctr, 5 * 8, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    std::copy(stat, stat + 5, al.stat);
    al.has_pref = true;
    al.on_device = true;
    px_finish(ix, PS_ALIGN);
    return FBG_OK;
}

extern "C" int fbg_pindex_align_stats(const fbg_pindex *ix, uint64_t *aligned, uint64_t *unsupported, uint64_t *too_long,
                                      uint64_t *too_wide, uint64_t *cells, uint64_t *max_read, uint64_t *table_bytes)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_align_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    const PaState &al = ix->al;
    if (aligned) *aligned = al.stat[1];
    if (unsupported) *unsupported = al.stat[0];
    if (too_long) *too_long = al.stat[2];
    if (too_wide) *too_wide = al.stat[3];
    if (cells) *cells = al.stat[4];
    if (max_read) *max_read = PA_MAX_READ;
    if (table_bytes) *table_bytes = al.has_pref ? 4 * ix->rw.m * ix->seg_nb : 0;
    return FBG_OK;
}

// ---- alignment path (fbg_pindex_chains_cigar / _cigar_fetch / _cigar_stats) ----------------------------------------
// pg_trace, which fbg_pindex_chains_graph_cigar (pindex_gcigar.hip) runs too, on alignments and a state of its own: sizes
// and their scans, the host's look at the history offsets (which form the batches), the slot total and the tier counts; one k_pg_path launch per word count that has reads, then one per batch of longer reads, all on the stream and
// so one after the other in the one scratch; a scan of the run counts, the host's look at their sum, the compaction.
template <int NW>
static void pg_launch(hipStream_t st, const PaDev &a, const PgIn &in, PgState &g, uint64_t n, uint64_t first, uint64_t reads, uint32_t cap,
                      uint64_t hbase)
{
    hipLaunchKernelGGL(k_pg_path<NW>, dim3((unsigned)reads), dim3(FBG_WAVE), NW ? (size_t)NW * 16 * (cap ? cap : 1) : 0, st, a, in.info, in.woff,
                       in.win, in.out, n, first, cap, (const uint64_t *)g.hoff.as<uint64_t>(), hbase, g.hist.as<uint64_t>(),
                       (const uint64_t *)g.soff.as<uint64_t>(), g.slots.as<uint32_t>(), g.cnt.as<uint64_t>(), g.nops.as<uint32_t>(),
                       g.ctr.as<unsigned long long>());
}

int pg_trace(fbg_pindex *ix, const PgIn *in, PgState &g, PsStage stage, uint64_t n, bool started, uint32_t *n_ops, uint64_t *total_ops,
             double *device_ms, const char *who)
{
    fbg_ctx *ctx = ix->ctx;
    if (device_ms) *device_ms = 0;
    if (total_ops) *total_ops = 0;
    px_begin(ix, stage);
    if (n == 0 || !in) {
        if (n_ops) std::fill(n_ops, n_ops + n, (uint32_t)0);
        std::fill(g.stat, g.stat + 5, (uint64_t)0);
        g.n = n;
        g.total = 0;
        g.on_device = false;
        px_finish(ix, stage);
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, g.sz, 2 * (n + 1) * 8));
    for (DevBuf *b : {&g.hoff, &g.soff, &g.cnt, &g.off}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    FBG_TRY(px_reserve(ix, g.nops, n * 4));
    FBG_TRY(px_reserve(ix, g.ctr, PG_CTR * 8));
    const PaDev a = pa_dev(ix);
    uint64_t *hsz = g.sz.as<uint64_t>(), *ssz = hsz + (n + 1), *hoff = g.hoff.as<uint64_t>(), *soff = g.soff.as<uint64_t>();
    uint64_t *cnt = g.cnt.as<uint64_t>(), *off = g.off.as<uint64_t>();
    auto *ctr = g.ctr.as<unsigned long long>();
    if (!started) FBG_HIP_TRY(ctx, hipEventRecord(ix->ev0, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, PG_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (n + 1) * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(g.nops.p, 0, n * 4, st));
    hipLaunchKernelGGL(k_pg_sizes, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, in->info, in->out, n, hsz, ssz, ctr);
    for (int k = 0; k < 2; k++)
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, k ? ssz : hsz, k ? soff : hoff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
        }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t hunits = 0, nslots = 0, c[PG_CTR];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&hunits, hoff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&nslots, soff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(c, ctr, PG_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    // the batches of the long reads: consecutive reads from one with a history on, while the sum fits the budget; the
    // offsets come to the host only when there is such a read
    std::vector<uint64_t> h;
    if (c[3 + PA_REG_WORDS]) {
        h.resize(n + 1);
        FBG_HIP_TRY(ctx, hipMemcpyAsync(h.data(), hoff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const int64_t kib = ctx->opt.path_batch_kib < 1 ? 1 : ctx->opt.path_batch_kib;
    const uint64_t budget = kib > (int64_t)1 << 50 ? ~0ull : (uint64_t)kib * 128;        // in units
    std::vector<std::pair<uint64_t, uint64_t>> batch;
    uint64_t units = 0;
    for (uint64_t r0 = 0; r0 < n && !h.empty();) {
        if (h[r0 + 1] == h[r0]) { r0++; continue; }
        uint64_t r1 = r0 + 1;
        while (r1 < n && h[r1 + 1] - h[r0] <= budget) r1++;
        batch.emplace_back(r0, r1);
        units = std::max(units, h[r1] - h[r0]);
        r0 = r1;
    }
    FBG_TRY(px_reserve(ix, g.slots, (nslots + 1) * 4));
    if (units) FBG_TRY(px_reserve(ix, g.hist, units * 8));
    if (c[3]) pg_launch<1>(st, a, *in, g, n, 0, n, (uint32_t)c[8], 0);
    if (c[4]) pg_launch<2>(st, a, *in, g, n, 0, n, (uint32_t)c[9], 0);
    if (c[5]) pg_launch<3>(st, a, *in, g, n, 0, n, (uint32_t)c[10], 0);
    if (c[6]) pg_launch<4>(st, a, *in, g, n, 0, n, (uint32_t)c[11], 0);
    for (const auto &b : batch) pg_launch<0>(st, a, *in, g, n, b.first, b.second - b.first, 0, h[b.first]);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, cnt, off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    unsigned long long failed = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&failed, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (failed) return fbg_fail(ctx, FBG_ERR_HIP, "%s: the trace of %llu reads did not arrive at the read's start", who, failed);
    FBG_TRY(px_reserve(ix, g.ops, (total + 1) * 4));
    if (total) {
        hipLaunchKernelGGL(k_pg_compact, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, (const uint64_t *)soff, (const uint32_t *)g.slots.as<uint32_t>(),
                           (const uint64_t *)off, n, g.ops.as<uint32_t>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_TRY(px_record_end(ix));
    if (n_ops) FBG_HIP_TRY(ctx, hipMemcpyAsync(n_ops, g.nops.p, n * 4, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    if (total_ops) *total_ops = total;
    const uint64_t stat[5] = {c[1], total, c[2], hunits * 8, batch.size()};
    std::copy(stat, stat + 5, g.stat);
    g.n = n;
    g.total = total;
    g.on_device = true;
    px_finish(ix, stage);
    return FBG_OK;
}

int pg_fetch(fbg_pindex *ix, const PgState &g, uint64_t *off, uint32_t *ops)
{
    fbg_ctx *ctx = ix->ctx;
    if (!g.on_device) {
        if (off) std::fill(off, off + g.n + 1, (uint64_t)0);
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (off) FBG_HIP_TRY(ctx, hipMemcpyAsync(off, g.off.p, (g.n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (ops && g.total) FBG_HIP_TRY(ctx, hipMemcpyAsync(ops, g.ops.p, g.total * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_cigar(fbg_pindex *ix, uint32_t *n_ops, uint64_t *total_ops, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    const PaState &al = ix->al;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_cigar", PS_ALIGN));
    // no reads, or every chain empty: nothing of that align call on the device
    const PgIn in = {al.info.as<uint4>(), al.woff.as<uint64_t>(), al.win.as<uint8_t>(), al.out.as<uint32_t>()};
    return pg_trace(ix, al.on_device ? &in : nullptr, ix->cg, PS_CIGAR, al.n, false, n_ops, total_ops, device_ms, "fbg_pindex_chains_cigar");
}

extern "C" int fbg_pindex_chains_cigar_fetch(fbg_pindex *ix, uint64_t *off, uint32_t *ops)
{
    if (!ix) return FBG_ERR_INVALID;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_cigar_fetch", PS_CIGAR));
    return pg_fetch(ix, ix->cg, off, ops);
}

extern "C" int fbg_pindex_cigar_stats(const fbg_pindex *ix, uint64_t *paths, uint64_t *ops, uint64_t *columns, uint64_t *history_bytes,
                                      uint64_t *batches)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_cigar_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    uint64_t *o[5] = {paths, ops, columns, history_bytes, batches};
    for (int k = 0; k < 5; k++)
        if (o[k]) *o[k] = ix->cg.stat[k];
    return FBG_OK;
}
