// pindex_graph.hip -- the edit distance of each read to a path of the graph around its chain, and that path
// (fbg_pindex_chains_align_graph / _align_graph_fetch / fbg_pindex_align_graph_stats).
//
//   k_ph_keys / k_ph_pin / k_ph_minlen   the tables of the first call: the edges sorted by (destination, source) as a
//                                    predecessor CSR, and per block its shortest label, scanned into C;
//   k_ph_prepare                     per read the blocks jl .. jh around its chain, the node range, the cells, the skip
//                                    status, the scratch and the path slots;
//   k_ph_forward                     a wave per read: Myers' bit-vector recurrence node by node in id order, the column
//                                    entering a node merged from the stored last columns of its predecessors;
//   k_ph_trace / k_ph_compact        the reverse recurrence from the end cell back through the merges, and the paths back
//                                    to back.
#include "pindex_dev.h"
#include <rocprim/rocprim.hpp>

// ---- tables -----------------------------------------------------------------------------------------------------------
__global__ void k_ph_keys(const uint32_t *esrc, const uint32_t *edst, uint64_t E, uint64_t *keys)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) keys[e] = (uint64_t)edst[e] << 32 | esrc[e];
}

// pin[e]: the source of the e-th sorted edge; pin_off[v]: the first sorted edge whose destination is at least v
__global__ void k_ph_pin(const uint64_t *keys, uint64_t E, uint64_t n_nodes, uint32_t *pin_off, uint32_t *pin)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) pin[i] = (uint32_t)keys[i];
    if (i <= n_nodes) {
        uint64_t lo = 0, hi = E;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((keys[mid] >> 32) < i) lo = mid + 1; else hi = mid;
        }
        pin_off[i] = (uint32_t)lo;
    }
}

// minlen[j] for j < nb, 0 for j == nb: one lane per block steps over its nodes
__global__ void k_ph_minlen(const uint64_t *first, const uint64_t *loff, uint64_t nb, uint64_t *minlen)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nb) return;
    uint64_t best = 0;
    if (j < nb)
        for (uint64_t v = first[j]; v < first[j + 1]; v++) {
            const uint64_t len = loff[v + 1] - loff[v];
            if (v == first[j] || len < best) best = len;
        }
    minlen[j] = best;
}

// ---- prepare ----------------------------------------------------------------------------------------------------------
// One lane per read (and one for the entry n of the sizes), after pr_prepare left rec (place, off: the chains; q: q_start
// per seed).  info[R] = (first node of H, one past its last, L or 0 where nothing is aligned, jl); ssz[R]: the scratch
// words, psz[R]: the path slots, both 0 where nothing is aligned; out (6 n): FBG_ALIGN_NONE five times and n_path 0.
// ctr as PH_CTR says, summed per wave before the atomic.
__global__ void k_ph_prepare(PhDev d, const uint4 *rec, const uint32_t *place, const uint64_t *off, const uint32_t *q,
                             const uint8_t *select, uint64_t n, uint64_t pad, uint64_t max_cells, uint4 *info, uint64_t *ssz,
                             uint64_t *psz, uint32_t *out, unsigned long long *ctr)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kind = -1;                // 0 aligned, 1 not selected, 2 too long, 3 too wide
    int tier = -1;                // 0 .. 3: 1 .. 4 words, 4: more
    unsigned long long cells = 0, nodes = 0, merges = 0;
    if (R <= n) {
        uint64_t s = 0, p = 0;
        if (R < n) {
            const uint64_t o0 = off[R], len = off[R + 1] - o0, L = d.roff[R + 1] - d.roff[R];
            uint64_t jl = d.nb, jh = 0;
            bool any = false;
            for (uint64_t a = 0; a < len; a++) {
                const uint4 rc = rec[place[o0 + a]];
                if (rc.x == PR_NONE) continue;
                const uint64_t ji = rc.w, qi = q[rc.z], lab = d.loff[rc.x + 1] - d.loff[rc.x];
                const uint64_t left = qi + pad > rc.y ? qi + pad - rc.y : 0;
                const uint64_t have = lab - rc.y, want = (L - qi) + pad, right = want > have ? want - have : 0;
                const uint64_t lo = d.C[ji] < left ? 0 : po_find(d.C, 0, ji, d.C[ji] - left);
                const uint64_t target = d.C[ji + 1] + right;
                uint64_t a2 = ji, b2 = d.nb - 1;
                while (a2 < b2) {
                    const uint64_t mid = a2 + (b2 - a2) / 2;
                    if (d.C[mid + 1] >= target) b2 = mid; else a2 = mid + 1;
                }
                if (lo < jl) jl = lo;
                if (a2 > jh) jh = a2;
                any = true;
            }
            uint4 in = make_uint4(0, 0, 0, 0);
            if (any) {
                const uint64_t n0 = d.first[jl], n1 = d.first[jh + 1], text = d.loff[n1] - d.loff[n0];
                kind = select && !select[R] ? 1 : L > PA_MAX_READ ? 2 : max_cells && L * text > max_cells ? 3 : 0;
                in = make_uint4((uint32_t)n0, (uint32_t)n1, 0, (uint32_t)jl);
                if (kind == 0) {
                    const uint32_t nw = (uint32_t)((L + 63) / 64);
                    in.z = (uint32_t)L;
                    cells = L * text;
                    nodes = n1 - n0;
                    merges = d.pin_off[n1] - d.pin_off[d.first[jl + 1]];
                    s = nodes * 2 * nw;
                    p = jh - jl + 1;
                    tier = nw <= PA_REG_WORDS ? (int)nw - 1 : PA_REG_WORDS;
                }
            }
            info[R] = in;
            for (int k = 0; k < 5; k++) out[k * n + R] = PA_NONE;
            out[5 * n + R] = 0;
        }
        ssz[R] = s;
        psz[R] = p;
    }
    const bool first = (threadIdx.x & (FBG_WAVE - 1)) == 0;
    for (int b = 0; b < 4; b++) {
        const unsigned long long mk = __ballot(kind == b);
        if (mk && first) atomicAdd(&ctr[1 + b], (unsigned long long)__popcll(mk));
    }
    for (int b = 0; b <= PA_REG_WORDS; b++) {
        const unsigned long long mk = __ballot(tier == b);
        if (mk && first) atomicAdd(&ctr[8 + b], (unsigned long long)__popcll(mk));
    }
    for (int o = FBG_WAVE / 2; o > 0; o >>= 1) {
        cells += __shfl_xor(cells, o);
        nodes += __shfl_xor(nodes, o);
        merges += __shfl_xor(merges, o);
    }
    if (first && cells) atomicAdd(&ctr[5], cells);
    if (first && nodes) atomicAdd(&ctr[6], nodes);
    if (first && merges) atomicAdd(&ctr[7], merges);
}

// ---- the wave's state -----------------------------------------------------------------------------------------------------
// lane l of a wave-uniform 64-bit value held one per lane; the halves unsigned, so that neither extends its sign
__device__ __forceinline__ uint64_t ph_lane64(uint64_t x, uint32_t l)
{
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)l);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)l);
    return (uint64_t)hi << 32 | lo;
}

// The read and the two vertical-difference words of every 64 read symbols, as pa_pass_reg (NW = 1 .. PA_REG_WORDS: in
// registers, lane i holds read symbols i, 64 + i, ..., 256 for none) and pa_pass_lds (NW = 0: rd and st in LDS, every lane
// stores the same state and reads back what it stored itself) keep them.  REV: the read backwards.
template <int NW, bool REV> struct PhWave {
    uint64_t pv[NW ? NW : 1], mv[NW ? NW : 1];
    int p[NW ? NW : 1];
    uint8_t *rd;
    uint64_t *st;
    uint32_t L, nw;
    unsigned lane;
    uint64_t top;

    __device__ __forceinline__ void init(const uint8_t *P, uint32_t L_, unsigned lane_, uint8_t *rd_, uint64_t *st_)
    {
        L = L_; lane = lane_; rd = rd_; st = st_;
        nw = NW ? NW : (L + 63) / 64;
        top = 1ull << ((L - 1) & 63);
        if constexpr (NW != 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t i = w * 64 + lane;
                p[w] = i < L ? (int)P[REV ? L - 1 - i : i] : 256;
            }
        } else {
            for (uint32_t w = 0; w < nw; w++) {
                const uint32_t i = w * 64 + lane;
                rd[i] = i < L ? P[REV ? L - 1 - i : i] : 0;
            }
        }
    }
    __device__ __forceinline__ uint64_t get_pv(uint32_t w) const { if constexpr (NW != 0) return pv[w]; else return st[w]; }
    __device__ __forceinline__ uint64_t get_mv(uint32_t w) const { if constexpr (NW != 0) return mv[w]; else return st[PA_MAX_READ / 64 + w]; }
    __device__ __forceinline__ void set(uint32_t w, uint64_t a, uint64_t b)
    {
        if constexpr (NW != 0) { pv[w] = a; mv[w] = b; }
        else { st[w] = a; st[PA_MAX_READ / 64 + w] = b; }
    }
    // D(i) = i
    __device__ __forceinline__ void fresh()
    {
        if constexpr (NW != 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) set(w, ~0ull, 0);
        } else
            for (uint32_t w = 0; w < nw; w++) set(w, ~0ull, 0);
    }
    // one column for the text symbol c; h: the horizontal difference of row 0 -> that of row L
    __device__ __forceinline__ int column(int c, int h)
    {
        if constexpr (NW != 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) h = pa_step(__ballot(p[w] == c), pv[w], mv[w], h, w == NW - 1 ? top : 1ull << 63);
        } else {
            for (uint32_t w = 0; w < nw; w++) {
                const uint32_t i = w * 64 + lane;
                uint64_t a = st[w], b = st[PA_MAX_READ / 64 + w];
                h = pa_step(__ballot(i < L && rd[i] == c), a, b, h, w == nw - 1 ? top : 1ull << 63);
                st[w] = a;
                st[PA_MAX_READ / 64 + w] = b;
            }
        }
        return h;
    }
    // lane t < 2 nw: word t of the column as it is stored, pv of every word and then mv
    __device__ __forceinline__ uint64_t stored() const
    {
        uint64_t x = 0;
        if constexpr (NW != 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) {
                if (lane == (unsigned)w) x = pv[w];
                if (lane == (unsigned)(NW + w)) x = mv[w];
            }
        } else if (lane < 2 * nw)
            x = lane < nw ? st[lane] : st[PA_MAX_READ / 64 + lane - nw];
        return x;
    }
};

// the bits of the rows up to this lane's
__device__ __forceinline__ uint64_t ph_below(unsigned lane) { return lane >= 63 ? ~0ull : (1ull << (lane + 1)) - 1; }

// ---- forward ----------------------------------------------------------------------------------------------------------
// The nodes n0 .. n1 of H in id order.  col: the read's scratch, 2 nw words per node; mn: per lane its NW minima (NW = 0: in
// LDS at w * 64 + lane, a slot that only this lane touches).  -> best, and the first cell (bnode, bcol) that attains it.
template <int NW>
__device__ __forceinline__ void ph_forward(const PhDev &d, const uint4 in, const uint8_t *P, uint64_t *col, unsigned lane, uint8_t *rd,
                                           uint64_t *st, int *mnl, uint32_t &best, uint32_t &bnode, uint32_t &bcol)
{
    PhWave<NW, false> s;
    const uint32_t n0 = in.x, n1 = in.y, L = in.z;
    s.init(P, L, lane, rd, st);
    const uint32_t nw = s.nw, inner = (uint32_t)d.first[in.w + 1];      // the nodes below inner are of block jl
    const uint64_t below = ph_below(lane);
    int mn[NW ? NW : 1];
    best = L;
    bnode = n0;
    bcol = 0;
    for (uint32_t v = n0; v < n1; v++) {
        uint32_t score = L;
        bool merged = false;
        const uint32_t e0 = d.pin_off[v], e1 = d.pin_off[v + 1];
        if (v >= inner && e0 < e1) {
            if constexpr (NW != 0) {
#pragma unroll
                for (int w = 0; w < NW; w++) mn[w] = 0x7fffffff;
            } else
                for (uint32_t w = 0; w < nw; w++) mnl[w * 64 + lane] = 0x7fffffff;
            for (uint32_t e = e0; e < e1; e++) {
                const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.pin[e]);
                if (u < n0 || u >= v) continue;
                merged = true;
                const uint64_t *cu = col + (uint64_t)(u - n0) * 2 * nw;
                const uint64_t x = lane < 2 * nw ? cu[lane] : 0;
                int base = 0;
                if constexpr (NW != 0) {
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const uint64_t a = ph_lane64(x, w), b = ph_lane64(x, NW + w);
                        const int val = base + __popcll(a & below) - __popcll(b & below);
                        mn[w] = val < mn[w] ? val : mn[w];
                        base += __popcll(a) - __popcll(b);
                    }
                } else {
                    for (uint32_t w = 0; w < nw; w++) {
                        const uint64_t a = ph_lane64(x, w), b = ph_lane64(x, nw + w);
                        const int val = base + __popcll(a & below) - __popcll(b & below);
                        const int old = mnl[w * 64 + lane];
                        mnl[w * 64 + lane] = val < old ? val : old;
                        base += __popcll(a) - __popcll(b);
                    }
                }
            }
        }
        if (merged) {
            // the merged column from each row's difference to the row below: lane l - 1, lane 63 of the word before, or row 0
            int carry = 0, last = 0;
            if constexpr (NW != 0) {
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const int m = mn[w], up = __shfl_up(m, 1), dl = m - (lane ? up : carry);
                    const bool in_read = w * 64 + lane < L;
                    s.set(w, __ballot(in_read && dl == 1), __ballot(in_read && dl == -1));
                    carry = __builtin_amdgcn_readlane(m, 63);
                    last = m;
                }
            } else {
                for (uint32_t w = 0; w < nw; w++) {
                    const int m = mnl[w * 64 + lane], up = __shfl_up(m, 1), dl = m - (lane ? up : carry);
                    const bool in_read = w * 64 + lane < L;
                    s.set(w, __ballot(in_read && dl == 1), __ballot(in_read && dl == -1));
                    carry = __builtin_amdgcn_readlane(m, 63);
                    last = m;
                }
            }
            score = (uint32_t)__builtin_amdgcn_readlane(last, (int)((L - 1) & 63));
        } else
            s.fresh();
        const uint64_t la = d.loff[v];
        const uint32_t len = (uint32_t)(d.loff[v + 1] - la);
        for (uint32_t j0 = 0; j0 < len; j0 += 64) {
            const uint32_t j = j0 + lane;
            const int chunk = j < len ? (int)d.labels[la + j] : 0;
            const uint32_t cnt = len - j0 < 64 ? len - j0 : 64;
            for (uint32_t t = 0; t < cnt; t++) {
                const int c = __builtin_amdgcn_readlane(chunk, t);
                score += s.column(c, 0);
                if (score < best) { best = score; bnode = v; bcol = j0 + t + 1; }
            }
        }
        const uint64_t x = s.stored();
        if (lane < 2 * nw) col[(uint64_t)(v - n0) * 2 * nw + lane] = x;
        pc_sync();                // lanes 0 .. 2 nw - 1 wrote what every lane reads when a later node merges
    }
}

// A wave per read first + blockIdx.x of a batch whose scratch starts at unit sbase.  1 <= L <= PA_MAX_READ.
__global__ __launch_bounds__(FBG_WAVE) void k_ph_forward(PhDev d, const uint4 *info, const uint64_t *soff, uint64_t sbase, uint64_t *scratch,
                                                        uint64_t n, uint64_t first, uint32_t *out)
{
    __shared__ uint8_t rd[PA_MAX_READ];
    __shared__ uint64_t st[2 * (PA_MAX_READ / 64)];
    __shared__ int mn[PA_MAX_READ];
    const uint64_t R = first + blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t L = in.z;
    if (L == 0 || L > PA_MAX_READ || in.x >= in.y) return;
    const uint8_t *P = d.reads + d.roff[R];
    uint64_t *col = scratch + (soff[R] - sbase);
    const uint32_t nw = (L + 63) / 64;         // the tier: the same in every lane
    uint32_t best, bnode, bcol;
    if (nw == 1) ph_forward<1>(d, in, P, col, lane, rd, st, mn, best, bnode, bcol);
    else if (nw == 2) ph_forward<2>(d, in, P, col, lane, rd, st, mn, best, bnode, bcol);
    else if (nw == 3) ph_forward<3>(d, in, P, col, lane, rd, st, mn, best, bnode, bcol);
    else if (nw == 4) ph_forward<4>(d, in, P, col, lane, rd, st, mn, best, bnode, bcol);
    else ph_forward<0>(d, in, P, col, lane, rd, st, mn, best, bnode, bcol);
    if (lane == 0) {
        out[R] = best;
        out[3 * n + R] = bnode;
        out[4 * n + R] = bcol;
    }
}

// ---- trace ------------------------------------------------------------------------------------------------------------
// From the end cell (v, use) back.  bv: L + 1 values in LDS, the walk's column at a node's first symbol.  slot: cap slots,
// the nodes end first.  -> the number of nodes, 0 for a walk that found no predecessor or ran out of slots.
template <int NW>
__device__ __forceinline__ uint32_t ph_trace(const PhDev &d, const uint4 in, const uint8_t *P, const uint64_t *col, unsigned lane, uint8_t *rd,
                                             uint64_t *st, int *bv, uint32_t edits, uint32_t v, uint32_t use, uint32_t *slot, uint32_t cap,
                                             uint32_t &snode, uint32_t &soffs)
{
    PhWave<NW, true> s;
    const uint32_t n0 = in.x, L = in.z;
    s.init(P, L, lane, rd, st);
    s.fresh();
    const uint32_t nw = s.nw, inner = (uint32_t)d.first[in.w + 1];
    const uint64_t below = ph_below(lane);
    uint32_t score = L, x = 0, k = 0;
    bool found = score == edits;      // the empty alignment: the start is the end
    soffs = use;
    for (;;) {
        if (k >= cap) return 0;
        if (lane == 0) slot[k] = v;
        k++;
        const uint64_t la = d.loff[v];
        for (uint32_t j0 = 0; j0 < use && !found; j0 += 64) {
            const uint32_t j = j0 + lane;
            const int chunk = j < use ? (int)d.labels[la + (use - 1 - j)] : 0;
            const uint32_t cnt = use - j0 < 64 ? use - j0 : 64;
            for (uint32_t t = 0; t < cnt; t++) {
                const int c = __builtin_amdgcn_readlane(chunk, t);
                score += s.column(c, 1);
                x++;
                if (score == edits) { found = true; soffs = use - (j0 + t + 1); break; }
            }
        }
        if (found) { snode = v; return k; }
        if (v < inner) return 0;          // a node of block jl enters with D(i) = i: its first symbol would have been a start
        // B(r) = D'(r, x) for r = 0 .. L
        if (lane == 0) bv[0] = (int)x;
        int base = (int)x;
        if constexpr (NW != 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint64_t a = s.get_pv(w), b = s.get_mv(w);
                const uint32_t r = w * 64 + lane + 1;
                if (r <= L) bv[r] = base + __popcll(a & below) - __popcll(b & below);
                base += __popcll(a) - __popcll(b);
            }
        } else {
            for (uint32_t w = 0; w < nw; w++) {
                const uint64_t a = s.get_pv(w), b = s.get_mv(w);
                const uint32_t r = w * 64 + lane + 1;
                if (r <= L) bv[r] = base + __popcll(a & below) - __popcll(b & below);
                base += __popcll(a) - __popcll(b);
            }
        }
        pc_sync();
        uint32_t pick = PH_NONE;
        const uint32_t e0 = d.pin_off[v], e1 = d.pin_off[v + 1];
        for (uint32_t e = e0; e < e1 && pick == PH_NONE; e++) {
            const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.pin[e]);
            if (u < n0 || u >= v) continue;
            const uint64_t *cu = col + (uint64_t)(u - n0) * 2 * nw;
            const uint64_t xw = lane < 2 * nw ? cu[lane] : 0;
            int m = (int)score, fb = 0;          // row 0 of F_u is 0, and B(L) is the walk's score
            for (uint32_t w = 0; w < nw; w++) {
                const uint64_t a = ph_lane64(xw, w), b = ph_lane64(xw, nw + w);
                const uint32_t i = w * 64 + lane + 1;
                if (i <= L) {
                    const int val = fb + __popcll(a & below) - __popcll(b & below) + bv[L - i];
                    m = val < m ? val : m;
                }
                fb += __popcll(a) - __popcll(b);
            }
            for (int o = FBG_WAVE / 2; o > 0; o >>= 1) {
                const int other = __shfl_xor(m, o);
                m = other < m ? other : m;
            }
            if (m == (int)edits) pick = u;
        }
        pc_sync();                        // bv is written again at the next node
        if (pick == PH_NONE) return 0;
        v = pick;
        use = (uint32_t)(d.loff[v + 1] - d.loff[v]);
    }
}

__global__ __launch_bounds__(FBG_WAVE) void k_ph_trace(PhDev d, const uint4 *info, const uint64_t *soff, uint64_t sbase, const uint64_t *scratch,
                                                      const uint64_t *poff, uint32_t *slots, uint64_t n, uint64_t first, uint32_t *out,
                                                      uint64_t *cnt, unsigned long long *ctr)
{
    __shared__ uint8_t rd[PA_MAX_READ];
    __shared__ uint64_t st[2 * (PA_MAX_READ / 64)];
    __shared__ int bv[PA_MAX_READ + 1];
    const uint64_t R = first + blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint4 in = info[R];
    const uint32_t L = in.z;
    if (L == 0 || L > PA_MAX_READ || in.x >= in.y) return;
    const uint8_t *P = d.reads + d.roff[R];
    const uint64_t *col = scratch + (soff[R] - sbase);
    uint32_t *slot = slots + poff[R];
    const uint32_t cap = (uint32_t)(poff[R + 1] - poff[R]);
    const uint32_t edits = out[R], ve = out[3 * n + R], ce = out[4 * n + R];
    const uint32_t nw = (L + 63) / 64;
    uint32_t snode = 0, so = 0, k;
    if (ve < in.x || ve >= in.y || ce > d.loff[ve + 1] - d.loff[ve]) k = 0;
    else if (nw == 1) k = ph_trace<1>(d, in, P, col, lane, rd, st, bv, edits, ve, ce, slot, cap, snode, so);
    else if (nw == 2) k = ph_trace<2>(d, in, P, col, lane, rd, st, bv, edits, ve, ce, slot, cap, snode, so);
    else if (nw == 3) k = ph_trace<3>(d, in, P, col, lane, rd, st, bv, edits, ve, ce, slot, cap, snode, so);
    else if (nw == 4) k = ph_trace<4>(d, in, P, col, lane, rd, st, bv, edits, ve, ce, slot, cap, snode, so);
    else k = ph_trace<0>(d, in, P, col, lane, rd, st, bv, edits, ve, ce, slot, cap, snode, so);
    if (lane == 0) {
        if (k == 0) atomicAdd(&ctr[0], 1ull);
        else {
            out[n + R] = snode;
            out[2 * n + R] = so;
            out[5 * n + R] = k;
            cnt[R] = k;
        }
    }
}

// One lane per read copies its nodes from their slots, where the end node comes first, to path + off[R], start node first
__global__ void k_ph_compact(const uint64_t *poff, const uint32_t *slots, const uint64_t *off, uint64_t n, uint32_t *path)
{
    const uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (R >= n) return;
    const uint64_t o = off[R], k = off[R + 1] - o, s = poff[R];
    for (uint64_t x = 0; x < k; x++) path[o + x] = slots[s + k - 1 - x];
}

// ---- the calls --------------------------------------------------------------------------------------------------------
// the predecessor CSR and C, once per index
static int ph_tables(fbg_pindex *ix)
{
    fbg_ctx *ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    PhState &g = ix->gr;
    const uint64_t E = ix->n_edges, nn = ix->n_nodes, nb = ix->seg_nb;
    FBG_TRY(px_reserve(ix, g.pin_off, (nn + 1) * 4));
    FBG_TRY(px_reserve(ix, g.pin, (E + 1) * 4));
    FBG_TRY(px_reserve(ix, g.C, 2 * (nb + 1) * 8));
    FBG_TRY(px_reserve(ix, g.keys, 2 * (E + 1) * 8));
    uint64_t *keys = g.keys.as<uint64_t>(), *sorted = keys + (E + 1), *C = g.C.as<uint64_t>(), *minlen = C + (nb + 1);
    if (E) {
        hipLaunchKernelGGL(k_ph_keys, dim3(fbg_blocks(E, 256)), dim3(256), 0, st, (const uint32_t *)ix->vesrc.as<uint32_t>(),
                           (const uint32_t *)ix->vedst.as<uint32_t>(), E, keys);
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, keys, sorted, (size_t)E, 0, 64, st);
        }));
    }
    hipLaunchKernelGGL(k_ph_pin, dim3(fbg_blocks(std::max(E, nn + 1), 256)), dim3(256), 0, st, (const uint64_t *)sorted, E, nn,
                       g.pin_off.as<uint32_t>(), g.pin.as<uint32_t>());
    hipLaunchKernelGGL(k_ph_minlen, dim3(fbg_blocks(nb + 1, 256)), dim3(256), 0, st, (const uint64_t *)ix->sfirst.as<uint64_t>(),
                       (const uint64_t *)ix->rw.loff.as<uint64_t>(), nb, minlen);
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, minlen, C, (uint64_t)0, (size_t)(nb + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    return FBG_OK;
}

static uint64_t ph_table_bytes(const fbg_pindex *ix)
{
    return ix->gr.has_tab ? 4 * (ix->n_nodes + 1) + 4 * ix->n_edges + 8 * (ix->seg_nb + 1) : 0;
}

// pr_prepare as in fbg_pindex_chains_align, the tables on the first call, k_ph_prepare, the scans of the scratch and slot
// sizes, the host's look at the scratch offsets (which form the batches), per batch k_ph_forward and k_ph_trace on the
// stream and so one after the other in the one scratch, a scan of n_path, the host's look at its sum, the compaction.
extern "C" int fbg_pindex_chains_align_graph(fbg_pindex *ix, uint64_t pad, uint64_t max_cells, const uint8_t *select, uint32_t *edits,
                                             uint32_t *start_node, uint32_t *start_offset, uint32_t *end_node, uint32_t *end_offset,
                                             uint32_t *n_path, uint64_t *total_path, double *device_ms)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    PrState &w = ix->rw;
    PhState &g = ix->gr;
    const PcState &c = ix->ch;
    if (device_ms) *device_ms = 0;
    if (total_path) *total_path = 0;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_align_graph", PS_CHAINS));
    std::fill(g.stat, g.stat + 9, (uint64_t)0);
    const uint64_t n = c.n;
    px_begin(ix, PS_GRAPH);                               // the CIGARs belong to the graph call they were traced from
    g.on_device = false;
    g.n = n;
    g.total = 0;
    if (n == 0) { px_finish(ix, PS_GRAPH); return FBG_OK; }
    if (n > 0x7fffffffull)        // a wave, and so a workgroup, per read
        return fbg_fail(ctx, FBG_ERR_TOO_LARGE, "fbg_pindex_chains_align_graph: %llu reads; a call takes fewer than 2^31", (unsigned long long)n);
    uint32_t *host[6] = {edits, start_node, start_offset, end_node, end_offset, n_path};
    if (c.total == 0) {          // every chain is empty, and the chaining call may have left nothing on the device
        for (int k = 0; k < 6; k++)
            if (host[k]) std::fill(host[k], host[k] + n, k < 5 ? (uint32_t)PA_NONE : 0u);
        px_finish(ix, PS_GRAPH);
        return FBG_OK;
    }
    if (pad > (1ull << 33)) pad = 1ull << 33;         // offsets and read lengths are below 2^32: beyond this nothing changes
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FBG_TRY(px_reserve(ix, g.info, n * 16));
    FBG_TRY(px_reserve(ix, g.sz, 2 * (n + 1) * 8));
    for (DevBuf *b : {&g.soff, &g.poff, &g.cnt, &g.off}) FBG_TRY(px_reserve(ix, *b, (n + 1) * 8));
    FBG_TRY(px_reserve(ix, g.out, 6 * n * 4));
    FBG_TRY(px_reserve(ix, g.sel, n));
    FBG_TRY(px_reserve(ix, g.ctr, PH_CTR * 8));
    PrDev d;
    FBG_TRY(pr_prepare(ix, d));                       // records ev0
    if (!g.has_tab) FBG_TRY(ph_tables(ix));           // the flag is set at the end of the call, once the tables are known to be written
    PhDev h;
    h.labels = w.labels.as<uint8_t>();
    h.loff = w.loff.as<uint64_t>();
    h.reads = ps_reads(ix);
    h.roff = ps_roff(ix);
    h.first = ix->sfirst.as<uint64_t>();
    h.C = g.C.as<uint64_t>();
    h.pin_off = g.pin_off.as<uint32_t>();
    h.pin = g.pin.as<uint32_t>();
    h.nb = ix->seg_nb;
    auto *ctr = g.ctr.as<unsigned long long>();
    uint64_t *ssz = g.sz.as<uint64_t>(), *psz = ssz + (n + 1), *soff = g.soff.as<uint64_t>(), *poff = g.poff.as<uint64_t>();
    uint64_t *cnt = g.cnt.as<uint64_t>(), *off = g.off.as<uint64_t>();
    uint32_t *out = g.out.as<uint32_t>();
    if (select) FBG_HIP_TRY(ctx, hipMemcpyAsync(g.sel.p, select, n, hipMemcpyHostToDevice, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, PH_CTR * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (n + 1) * 8, st));
    hipLaunchKernelGGL(k_ph_prepare, dim3(fbg_blocks(n + 1, 256)), dim3(256), 0, st, h, (const uint4 *)w.rec.as<uint4>(),
                       (const uint32_t *)c.out.as<uint32_t>(), (const uint64_t *)c.off.as<uint64_t>(), (const uint32_t *)ix->sq.as<uint32_t>(),
                       select ? (const uint8_t *)g.sel.as<uint8_t>() : (const uint8_t *)nullptr, n, pad, max_cells, g.info.as<uint4>(), ssz, psz,
                       out, ctr);
    for (int k = 0; k < 2; k++)
        FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, k ? psz : ssz, k ? poff : soff, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
        }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t nslots = 0, cv[PH_CTR];
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&nslots, poff + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(cv, ctr, PH_CTR * 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    // the batches: consecutive reads from an aligned one on, while their columns fit the budget
    std::vector<uint64_t> so;
    if (cv[1]) {
        so.resize(n + 1);
        FBG_HIP_TRY(ctx, hipMemcpyAsync(so.data(), soff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const int64_t kib = ctx->opt.graph_batch_kib < 1 ? 1 : ctx->opt.graph_batch_kib;
    const uint64_t budget = kib > (int64_t)1 << 50 ? ~0ull : (uint64_t)kib * 128;        // in words
    std::vector<std::pair<uint64_t, uint64_t>> batch;
    uint64_t units = 0;
    for (uint64_t r0 = 0; r0 < n && !so.empty();) {
        if (so[r0 + 1] == so[r0]) { r0++; continue; }
        uint64_t r1 = r0 + 1;
        while (r1 < n && so[r1 + 1] - so[r0] <= budget) r1++;
        batch.emplace_back(r0, r1);
        units = std::max(units, so[r1] - so[r0]);
        r0 = r1;
    }
    FBG_TRY(px_reserve(ix, g.slots, (nslots + 1) * 4));
    if (units) FBG_TRY(px_reserve(ix, g.scratch, units * 8));
    for (const auto &b : batch) {
        const unsigned reads = (unsigned)(b.second - b.first);
        hipLaunchKernelGGL(k_ph_forward, dim3(reads), dim3(FBG_WAVE), 0, st, h, (const uint4 *)g.info.as<uint4>(), (const uint64_t *)soff,
                           so[b.first], g.scratch.as<uint64_t>(), n, b.first, out);
        hipLaunchKernelGGL(k_ph_trace, dim3(reads), dim3(FBG_WAVE), 0, st, h, (const uint4 *)g.info.as<uint4>(), (const uint64_t *)soff,
                           so[b.first], (const uint64_t *)g.scratch.as<uint64_t>(), (const uint64_t *)poff, g.slots.as<uint32_t>(), n, b.first,
                           out, cnt, ctr);
    }
    FBG_TRY(px_with_tmp(ix, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, cnt, off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
    }));
    FBG_HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    unsigned long long failed = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&failed, ctr, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    g.has_tab = true;
    if (failed)
        return fbg_fail(ctx, FBG_ERR_HIP, "fbg_pindex_chains_align_graph: the trace of %llu reads found no predecessor to step to", failed);
    FBG_TRY(px_reserve(ix, g.path, (total + 1) * 4));
    if (total) {
        hipLaunchKernelGGL(k_ph_compact, dim3(fbg_blocks(n, 256)), dim3(256), 0, st, (const uint64_t *)poff, (const uint32_t *)g.slots.as<uint32_t>(),
                           (const uint64_t *)off, n, g.path.as<uint32_t>());
        FBG_HIP_TRY(ctx, hipGetLastError());
    }
    FBG_TRY(px_record_end(ix));
    for (int k = 0; k < 6; k++)
        if (host[k]) FBG_HIP_TRY(ctx, hipMemcpyAsync(host[k], out + k * n, n * 4, hipMemcpyDeviceToHost, st));
    FBG_TRY(px_sync_elapsed(ix, device_ms));
    if (total_path) *total_path = total;
    const uint64_t stat[9] = {cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7], total, batch.size()};
    std::copy(stat, stat + 9, g.stat);
    g.total = total;
    g.on_device = true;
    px_finish(ix, PS_GRAPH);
    return FBG_OK;
}

extern "C" int fbg_pindex_chains_align_graph_fetch(fbg_pindex *ix, uint64_t *path_off, uint32_t *path_nodes)
{
    if (!ix) return FBG_ERR_INVALID;
    fbg_ctx *ctx = ix->ctx;
    const PhState &g = ix->gr;
    FBG_TRY(px_need_rows(ix, "fbg_pindex_chains_align_graph_fetch", PS_GRAPH));
    if (!g.on_device) {
        if (path_off) std::fill(path_off, path_off + g.n + 1, (uint64_t)0);
        return FBG_OK;
    }
    FBG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (path_off) FBG_HIP_TRY(ctx, hipMemcpyAsync(path_off, g.off.p, (g.n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (path_nodes && g.total) FBG_HIP_TRY(ctx, hipMemcpyAsync(path_nodes, g.path.p, g.total * 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return FBG_OK;
}

extern "C" int fbg_pindex_align_graph_stats(const fbg_pindex *ix, uint64_t *aligned, uint64_t *not_selected, uint64_t *too_long,
                                            uint64_t *too_wide, uint64_t *cells, uint64_t *nodes, uint64_t *merges, uint64_t *path_nodes,
                                            uint64_t *table_bytes, uint64_t *batches)
{
    if (!ix) return FBG_ERR_INVALID;
    if (!ix->has_rows)
        return fbg_fail(ix->ctx, FBG_ERR_INVALID, "fbg_pindex_align_graph_stats: only an index built by fbg_pindex_build_segmentation_rows has the row table");
    const PhState &g = ix->gr;
    uint64_t *o[8] = {aligned, not_selected, too_long, too_wide, cells, nodes, merges, path_nodes};
    for (int k = 0; k < 8; k++)
        if (o[k]) *o[k] = g.stat[k];
    if (table_bytes) *table_bytes = ph_table_bytes(ix);
    if (batches) *batches = g.stat[8];
    return FBG_OK;
}
