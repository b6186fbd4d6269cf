// pindex_dev.h -- device helpers of the pattern index that kernels of more than one file inline (no relocatable device code).
//
// occ layout.  Symbols are remapped to dense codes in byte order (the sentinel is code 0, '#' code 1).  With at
// most 16 codes a block of 128 BWT positions is one 128-byte line:
//   bytes   0 ..  63   u32 occ of every code before the block
//   bytes  64 ..  95   bits 0 .. 63 of the positions, bit planes 0 .. 3 (u64 each)
//   bytes  96 .. 127   bits 64 .. 127, bit planes 0 .. 3
// occ(c, i) = count[c] + popcount(AND over the planes of (plane or its complement) below i): one line per query,
// about one byte per text position.  Larger alphabets take 8 bit planes per line (128 bytes) and the counts in a
// table of their own (u32 per block and code): two lines per query.  k_px_lines / k_px_counts (pindex_build.hip) write
// the lines, px_load reads them.
#pragma once
#include "pindex.h"

// ---- backward steps ---------------------------------------------------------------------------------------------
// the positions of a block whose code is c, from the block's bit planes
template <int P> __device__ __forceinline__ uint64_t px_match(uint32_t c, const uint64_t *w)
{
    uint64_t m = ~0ull;
#pragma unroll
    for (int p = 0; p < P; p++) m &= ((c >> p) & 1u) ? w[p] : ~w[p];
    return m;
}

__device__ __forceinline__ uint64_t px_low(uint32_t off) { return off >= 64 ? ~0ull : ((1ull << off) - 1); }

// occ(c, i) of a loaded line: planes w[word][plane]
template <int P> __device__ __forceinline__ uint32_t px_pop(uint32_t c, uint32_t off, const uint64_t (&w)[2][P])
{
    const uint32_t a = __popcll(px_match<P>(c, w[0]) & px_low(off));
    return off > 64 ? a + __popcll(px_match<P>(c, w[1]) & px_low(off - 64)) : a;
}

template <bool COMPACT> __device__ __forceinline__ uint32_t px_load(const PxDev &d, uint32_t c, uint32_t blk,
                                                                    uint64_t (&w)[2][COMPACT ? 4 : 8])
{
    constexpr int P = COMPACT ? 4 : 8;
    const uint8_t *ln = d.lines + (uint64_t)blk * PX_LINE;
    const ulonglong2 *q = (const ulonglong2 *)(ln + (COMPACT ? 64 : 0));
#pragma unroll
    for (int k = 0; k < P; k++) {
        const ulonglong2 v = q[k];
        w[(2 * k) / P][(2 * k) % P] = v.x;
        w[(2 * k + 1) / P][(2 * k + 1) % P] = v.y;
    }
    return COMPACT ? ((const uint32_t *)ln)[c] : d.cnt_tab[(uint64_t)blk * d.S + c];
}

// occ(c, l) and occ(c, r1), l <= r1: both loads issued before either is used; one line when both fall in one block
template <bool COMPACT> __device__ __forceinline__ void px_occ2(const PxDev &d, uint32_t c, uint32_t l, uint32_t r1,
                                                                uint32_t &ol, uint32_t &or1, uint32_t &nlines)
{
    constexpr int P = COMPACT ? 4 : 8;
    const uint32_t bl = l / PX_BLK, br = r1 / PX_BLK;
    uint64_t wl[2][P], wr[2][P];
    const uint32_t cl = px_load<COMPACT>(d, c, bl, wl);
    uint32_t cr = cl;
    const bool two = bl != br;
    if (two) cr = px_load<COMPACT>(d, c, br, wr);
    ol = cl + px_pop<P>(c, l % PX_BLK, wl);
    or1 = two ? cr + px_pop<P>(c, r1 % PX_BLK, wr) : cl + px_pop<P>(c, r1 % PX_BLK, wl);
    nlines += two ? 2u : 1u;
}

// bs(c, l, r) of sdsl: [C[c] + occ(c, l), C[c] + occ(c, r + 1) - 1]; the count, 0 for an absent symbol
template <bool COMPACT> __device__ __forceinline__ uint32_t px_bs(const PxDev &d, const uint16_t *code, const uint32_t *C,
                                                                  uint32_t ch, uint32_t l, uint32_t r, uint32_t &nl,
                                                                  uint32_t &nr, uint32_t &nlines)
{
    const uint32_t c = code[ch];
    if (c == PX_ABSENT) { nl = l; nr = r; return 0; }
    uint32_t ol, or1;
    px_occ2<COMPACT>(d, c, l, r + 1, ol, or1, nlines);
    nl = C[c] + ol;
    nr = C[c] + or1 - 1;
    return or1 - ol;
}

// ---- from a text position to its edge; searches of CSR offsets ----------------------------------------------------------
// the edge whose string holds text position p: the last e with estart[e] <= p, searched between two coarse entries
__device__ __forceinline__ uint32_t pv_edge(const PvDev &d, uint32_t p)
{
    uint32_t lo = d.ctab[p >> PV_CSHIFT], hi = d.ctab[(p >> PV_CSHIFT) + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (d.estart[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint64_t po_uniform(uint64_t v)
{
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}

// the last q in [lo, hi] with off[q] <= x (off[lo] <= x is given)
__device__ __forceinline__ uint64_t po_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the MSA coordinate table (written by k_pm_units / k_pm_fill, pindex_build.hip) --------------------------------------
// the position of the k-th (from 0) set bit of w, k < popcount(w): halves narrowed by their popcounts, six steps
__device__ __forceinline__ uint32_t pm_select(uint64_t w, uint32_t k)
{
    uint32_t pos = 0;
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        const uint32_t c = __popcll(w & ((1ull << h) - 1));
        if (k >= c) { k -= c; w >>= h; pos += h; }
    }
    return pos;
}

// col(u, o) of a node with entry nd = (row, x0, first unit, width), o < |label(u)|: the last group whose count is at
// most o (a search over the node's ceil(nw / PM_W) group heads), then at most PM_W words of that group.  A table that
// disagreed with |label(u)| would end the word loop without a hit: PM_NONE then, never a read past the node's units.
__device__ __forceinline__ uint32_t pm_col(const PmDev &m, const uint4 nd, uint32_t o)
{
    if (nd.z == PM_NONE) return nd.y + o;
    const uint64_t *b = m.bits + nd.z;
    const uint32_t nw = (nd.w + 63) / 64;
    uint32_t lo = 0, hi = (nw + PM_W - 1) / PM_W - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (b[(uint64_t)mid * (PM_W + 1)] <= o) lo = mid; else hi = mid - 1;
    }
    const uint64_t *grp = b + (uint64_t)lo * (PM_W + 1);
    uint32_t k = o - (uint32_t)grp[0];
    const uint32_t w0 = lo * PM_W, wn = nw - w0 < PM_W ? nw - w0 : PM_W;
    for (uint32_t j = 0; j < wn; j++) {
        const uint64_t w = grp[1 + j];
        const uint32_t c = __popcll(w);
        if (k < c) return nd.y + (w0 + j) * 64 + pm_select(w, k);
        k -= c;
    }
    return PM_NONE;
}

// ---- sums of columns and margins that must not wrap (pindex_mapq.hip, pindex_pairs.hip) ---------------------------------
__device__ __forceinline__ uint64_t pq_add_sat(uint64_t a, uint64_t b) { return b > 0xffffffffffffffffull - a ? 0xffffffffffffffffull : a + b; }

// ---- one wave's own traffic through LDS or device memory (the chain DPs) ------------------------------------------------
// what a seed's lanes wrote becomes visible to the lanes of the same wave that scan it for the next seed
__device__ __forceinline__ void pc_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- the row table: does a row spell a seed from a start place on (pindex_rows.hip, pindex_byrow.hip) ---------------------
// Does the text of row r from offset o of its node u in block j on start with S[0 .. k)?  k >= 1, o < |label(u)|.
// Every read is bounded: a label by its length, the row's cells by block nb, S by k.
__device__ __forceinline__ bool pr_walk(const PrDev &d, uint64_t r, uint32_t u, uint32_t o, uint64_t j, const uint8_t *S, uint32_t k)
{
    uint32_t pos = 0;
    uint64_t a = d.loff[u] + o, b = d.loff[u + 1];
    for (;;) {
        const uint64_t take = b - a < (uint64_t)(k - pos) ? b - a : (uint64_t)(k - pos);
        for (uint64_t x = 0; x < take; x++)
            if (d.labels[a + x] != S[pos + x]) return false;
        pos += (uint32_t)take;
        if (pos == k) return true;
        uint32_t v;
        do {
            if (++j >= d.nb) return false;        // the row ends before the seed does
            v = d.node_of[j * d.m + r];
        } while (v == PR_NONE);
        a = d.loff[v];
        b = d.loff[v + 1];
    }
}

// rec of one place and row r: is r in rows(place)?
__device__ __forceinline__ bool pr_supports(const PrDev &d, const uint4 rc, uint64_t r)
{
    if (rc.x == PR_NONE || d.node_of[(uint64_t)rc.w * d.m + r] != rc.x) return false;
    return pr_walk(d, r, rc.x, rc.y, rc.w, d.reads + d.sbase[rc.z], d.slen[rc.z]);
}

// the G bits of a wave-wide ballot that belong to the group whose first lane is sh
template <int G> __device__ __forceinline__ uint64_t pr_group_bits(bool ok, unsigned sh)
{
    const uint64_t bal = __ballot(ok);
    return G == FBG_WAVE ? bal : (bal >> sh) & ((1ull << (G % 64)) - 1);
}

// ---- the bit-vector edit distance (pindex_align.hip, pindex_graph.hip) -----------------------------------------------------
// One column of Myers' bit-vector recurrence for a word of 64 read symbols (Hyyro's block form).  eq: the rows of the
// word whose read symbol equals the column's text symbol; pv / mv: the rows whose vertical difference D(i, j) -
// D(i - 1, j) is +1 / -1; hin: the horizontal difference D(i0, j) - D(i0, j - 1) of the row below the word's first;
// -> the horizontal difference of the row whose bit is top.  Bits above top never reach the bits below it.
__device__ __forceinline__ int pa_step(uint64_t eq, uint64_t &pv, uint64_t &mv, int hin, uint64_t top)
{
    const uint64_t neg = hin < 0 ? 1 : 0;
    const uint64_t xv = eq | mv;
    eq |= neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
    const int hout = (ph & top) ? 1 : (mh & top) ? -1 : 0;
    ph = (ph << 1) | (hin > 0 ? 1 : 0);
    mh = (mh << 1) | neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}
