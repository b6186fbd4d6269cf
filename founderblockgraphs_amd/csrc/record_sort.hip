// record_sort.hip -- the record path: from the sorted round-0 (key, position) pairs to the suffix array and one 16-byte
// record per text position.  Taken when no scan in suffix order finished the index (suffix_sort.hip chooses the path).
//
// Method: prefix doubling with early discard.  Round 0: suffix_sort.hip has sorted all N pairs by the first K symbols of every
// suffix (keys.h).  Round k: only suffixes still sharing their key with a neighbour are re-sorted, by (rank of their group,
// rank of the suffix h symbols further on), h = K, 2K, 4K, ...  rank[p] is always the SA index of the first member of p's
// group, so it is final as soon as the group is a singleton.  Device-wide sort / scan primitives come from rocPRIM.
//
// Ranks live in a 16-byte record per text position, rec[p] = {rank, lcp_prev, lcp_next, 0}, so that the one unavoidable random
// scatter of the sort (SA order -> text order) also delivers the two neighbour LCPs the scan needs: for suffixes whose round-0
// keys differ the LCP is the number of equal leading symbols of the two keys -- no text access.  Bit 31 of an LCP word is the
// run hint: the SA neighbour sits in the same MSA column, i.e. the two ranks can be coloured together (fbg.cpp:1633-1641).
// Suffixes that tie on their whole key (round-0 groups) are patched after the last doubling round (k_fix_dirty: text comparison
// from symbol K on).  When ties are common (similar rows) or the MSA has gaps, lcp.hip recomputes both LCP words instead.
#include "fbg_internal.h"
#include "keys.h"
#include "sort_config.h"
#include "text_cmp.h"
#include <rocprim/rocprim.hpp>

// grp[r] = r if key[r] starts a group, else 0  (max-scan turns it into the group head index)
__global__ void k_mark_heads(const uint64_t *__restrict__ keys, uint64_t cnt, const uint32_t *__restrict__ where,
                             uint32_t *__restrict__ grp)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    bool head = k == 0 || keys[k] != keys[k - 1];
    uint32_t r = where ? where[k] : (uint32_t)k;
    grp[k] = head ? r : 0u;
}

// Run hint of two SA-adjacent positions: can both be the pointer of an active row in one column?
// Row pointer p is current for the columns (column of the previous symbol of its row, column of p]
// (fbg.cpp:1687-1691); gap-free MSAs: exactly one column, p mod (n+1).
struct ColTest {
    const uint32_t *colT;  // MSAs with gaps: column of every text position ('#', sentinel: n); else nullptr
    uint32_t row_len;      // gap-free: n + 1
    uint32_t n;
    uint32_t last;         // N - 1, the sentinel, never a row pointer
    __device__ __forceinline__ uint2 span(uint32_t p) const
    {
        if (p == last) return make_uint2(1u, 0u);                        // empty
        if (!colT) { const uint32_t c = p % row_len; return make_uint2(c, c); }
        const uint32_t c = colT[p];
        uint32_t lo = 0;
        if (p > 0) { const uint32_t cp = colT[p - 1]; lo = cp >= n ? 0u : cp + 1; }
        return make_uint2(lo, c < n ? c : n - 1);
    }
    static __device__ __forceinline__ uint32_t meet(uint2 a, uint2 c)
    {
        return max(a.x, c.x) <= min(a.y, c.y) ? 0x80000000u : 0u;
    }
    __device__ __forceinline__ uint32_t same(uint32_t p, uint32_t q) const { return meet(span(p), span(q)); }
};

// round 0, after the max-scan: one 16-byte record per text position (rank, key-derived neighbour LCPs
// with run hints), unresolved flags.  vals[] doubles as the suffix array.
__global__ void k_apply_groups0(const uint32_t *__restrict__ grp, const uint32_t *__restrict__ vals,
                                const uint64_t *__restrict__ keys, uint64_t N, int b, int key_bits, ColTest ct,
                                uint4 *__restrict__ rec, uint8_t *__restrict__ flags)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < N;
    const int lane = threadIdx.x & 63;
    const uint32_t g = in ? grp[k] : 0u, p = in ? vals[k] : ct.last;
    const uint64_t key = in ? keys[k] : 0ull;
    // column span of this suffix's position; the neighbours' spans come from the adjacent lanes
    const uint2 sp = ct.span(p);
    uint2 sprev = make_uint2(__shfl_up(sp.x, 1, 64), __shfl_up(sp.y, 1, 64));
    uint2 snext = make_uint2(__shfl_down(sp.x, 1, 64), __shfl_down(sp.y, 1, 64));
    if (!in) return;
    uint32_t lp = 0, ln = 0;
    bool head = g == (uint32_t)k, next_head = true;
    if (k > 0) {
        const uint64_t kp = keys[k - 1];
        if (kp != key) {
            if (lane == 0) sprev = ct.span(vals[k - 1]);
            lp = fbg_key_lcp_inv(kp, key, fbg_key_inv(b), key_bits) | ColTest::meet(sprev, sp);
        }
    }
    if (k + 1 < N) {
        const uint64_t kn = keys[k + 1];
        next_head = kn != key;
        if (next_head) {
            if (lane == 63) snext = ct.span(vals[k + 1]);
            ln = fbg_key_lcp_inv(key, kn, fbg_key_inv(b), key_bits) | ColTest::meet(sp, snext);
        }
    }
    rec[p] = make_uint4(g, lp, ln, 0u);
    flags[k] = !(head && next_head);
}

// ---- the same records without a random scatter -------------------------------------------------------------
// rec[p] = ... above writes 16 bytes at a random place per suffix: every one of them a read-modify-write of a memory
// line (36 ms for 5*10^8 suffixes).  The positions are a permutation of 0..N-1, so the way back to text order is a
// sort whose bucket sizes are known exactly beforehand: two splitting passes on the leading bits of p (tiles
// regrouped in LDS and written in runs, as msd_sort.hip does; every bucket owns precisely the stretch of the
// positions it covers, no capacities to bet on) and a last pass that drops each leaf of 4096 positions into place
// inside LDS and writes it out whole.  5 x 16 bytes of streamed traffic per suffix instead: 18 ms for the same input.
#define BP_THREADS 1024                        // 512-thread tiles (two workgroups per CU) were 30 % slower: shorter runs
#define BP_ITEMS 8
#define BP_TILE (BP_THREADS * BP_ITEMS)
#define BP_MAXD 1024
#define BP_LEAF_BITS 12
#define BP_LEAF (1u << BP_LEAF_BITS)

struct BpArgs {
    uint64_t N;
    int shift;                       // bucket of an element = p >> shift; its stretch starts at bucket << shift
    uint32_t nd;                     // buckets a tile can meet (power of two): LDS digit = bucket & (nd - 1)
    const uint4 *in;                 // pass B: stretches of 1 << seg_shift elements
    int seg_shift;
    uint32_t tiles_per_seg;
    uint4 *out;
    unsigned long long *cursor;      // [N >> shift + 1], zeroed: fill of every bucket
    unsigned long long *flag;
    // pass A makes its elements from the sorted keys (k_apply_groups0)
    const uint32_t *grp, *vals;
    const uint64_t *keys;
    int b, key_bits;
    ColTest ct;
    uint8_t *flags;
    // MSAs with gaps: first column and number of gaps of every window of BP_WIN text positions (no row end inside),
    // from which a position's column span is bounded without touching colT
    const uint2 *win;
    const uint32_t *win_lo;          // exact lower end of the span of every window's first position
};

#define BP_WIN_BITS 10
#define BP_WIN (1u << BP_WIN_BITS)
#define BP_WIN_NONE 0xffffffffu

// one wave per window: a window that holds a '#' or the sentinel (column n) bounds nothing
__global__ __launch_bounds__(256) void k_bp_windows(const uint32_t *__restrict__ colT, uint64_t N, uint32_t n,
                                                    uint2 *__restrict__ win, uint32_t *__restrict__ win_lo)
{
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t lo = w << BP_WIN_BITS;
    if (lo >= N) return;
    const uint64_t hi = min(N, lo + BP_WIN);
    bool bad = false;
    for (uint64_t q = lo + lane; q < hi; q += 64) bad = bad || colT[q] >= n;
    if (lane == 0) { const uint32_t cp = lo > 0 ? colT[lo - 1] : n; win_lo[w] = cp >= n ? 0u : cp + 1; }   // as ColTest::span
    if (__ballot(bad)) { if (lane == 0) win[w] = make_uint2(BP_WIN_NONE, 0u); return; }
    if (lane == 0) {
        const uint32_t first = colT[lo], last = colT[hi - 1];
        win[w] = make_uint2(first, last - first - (uint32_t)(hi - 1 - lo));
    }
}

// an interval that contains the column span of text position p (ColTest::span), from the window tables alone
__device__ __forceinline__ uint2 bp_span_bound(const BpArgs &a, uint32_t p)
{
    if (p == a.ct.last) return make_uint2(1u, 0u);
    const uint32_t o = p & (BP_WIN - 1);
    const uint2 w = a.win[p >> BP_WIN_BITS];
    if (w.x == BP_WIN_NONE) return make_uint2(0u, a.ct.n);
    // the window's first position is every 1024th: with a loose lower end half of them would go on to the exact test
    return make_uint2(o ? w.x + o : a.win_lo[p >> BP_WIN_BITS], w.x + o + w.y);
}

// e[r] (valid for r with j = threadIdx.x + r * BP_THREADS < have; e.x = position) -> runs in the buckets' stretches
__device__ __forceinline__ void bp_regroup_write(const BpArgs &a, uint4 (&e)[BP_ITEMS], uint32_t have, uint4 *buf, uint32_t *cnt,
                                                 uint32_t *loff, unsigned long long *gbase, uint32_t *wsum)
{
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t rk[BP_ITEMS];
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        rk[r] = j < have ? atomicAdd(&cnt[(e[r].x >> a.shift) & (a.nd - 1)], 1u) : 0u;
    }
    __syncthreads();
    {   // exclusive offsets of the digit counts; one global atomic per non-empty digit reserves its run
        const uint32_t c = cnt[threadIdx.x];                       // BP_THREADS == BP_MAXD
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += o; }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t q = 0; q < wv; q++) pre += wsum[q];
        loff[threadIdx.x] = pre + inc - c;
        gbase[threadIdx.x] = 0;
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        if (j < have) {
            const uint32_t d = (e[r].x >> a.shift) & (a.nd - 1);
            buf[loff[d] + rk[r]] = e[r];
            if (rk[r] == 0) {                                      // first of its digit in this tile: reserve the run
                const uint64_t bucket = (uint64_t)e[r].x >> a.shift;
                gbase[d] = (bucket << a.shift) + atomicAdd(&a.cursor[bucket], (unsigned long long)cnt[d]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        if (j < have) {
            const uint4 x = buf[j];
            const uint32_t d = (x.x >> a.shift) & (a.nd - 1);
            const uint64_t at = gbase[d] + (j - loff[d]);
            const uint64_t end = min(a.N, (((uint64_t)x.x >> a.shift) + 1) << a.shift);
            if (at < end) a.out[at] = x;
            else *a.flag = 1;                                      // cannot happen for a permutation
        }
    }
}

// first splitting pass: k_apply_groups0's record of every suffix, sent towards its position instead of written there.
// (As two kernels -- a streaming one that writes the records in suffix order, then k_bp_split over the whole array --
// the same work took 15 ms instead of 12.)
__global__ __launch_bounds__(BP_THREADS) void k_bp_groups0(BpArgs a)
{
    __shared__ uint4 buf[BP_TILE];
    __shared__ uint32_t cnt[BP_MAXD], loff[BP_MAXD];
    __shared__ unsigned long long gbase[BP_MAXD];
    __shared__ uint32_t wsum[BP_THREADS / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BP_TILE;
    const uint32_t have = (uint32_t)min((uint64_t)BP_TILE, a.N - first);
    cnt[threadIdx.x] = 0;
    uint4 e[BP_ITEMS];
    // all loads of the tile first, then the window tables, then keys and spans of the whole tile into LDS, where every
    // element finds its two SA neighbours (the tile's first and last element fetch theirs from memory)
    const bool bounded = a.ct.colT != nullptr;
    const uint32_t inv_b = fbg_key_inv(a.b);
    uint32_t gg[BP_ITEMS], pp[BP_ITEMS];
    uint64_t key[BP_ITEMS];
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        const uint64_t k = first + j;
        const bool in = j < have;
        gg[r] = in ? a.grp[k] : 0u;
        pp[r] = in ? a.vals[k] : a.ct.last;
        key[r] = in ? a.keys[k] : 0ull;
    }
    uint2 sp[BP_ITEMS];
    if (bounded) {
        // the run hints need the column spans of SA neighbours.  With gaps a span costs two reads of colT at a random
        // place: bounds from the window tables (small enough to stay in L2) rule nearly every pair out first.  The
        // table reads of the thread's eight slots go out together -- one after the other (the branches of
        // bp_span_bound between them) this kernel spent 88 % of its wave cycles waiting for them
        uint2 wv[BP_ITEMS];
        uint32_t wl[BP_ITEMS];
#pragma unroll
        for (int r = 0; r < BP_ITEMS; r++) wv[r] = a.win[pp[r] >> BP_WIN_BITS];
#pragma unroll
        for (int r = 0; r < BP_ITEMS; r++) wl[r] = (pp[r] & (BP_WIN - 1)) ? 0u : a.win_lo[pp[r] >> BP_WIN_BITS];
#pragma unroll
        for (int r = 0; r < BP_ITEMS; r++) {
            const uint32_t p = pp[r], o = p & (BP_WIN - 1);
            if (p == a.ct.last) sp[r] = make_uint2(1u, 0u);
            else if (wv[r].x == BP_WIN_NONE) sp[r] = make_uint2(0u, a.ct.n);
            else sp[r] = make_uint2(o ? wv[r].x + o : wl[r], wv[r].x + o + wv[r].y);
        }
    } else {
#pragma unroll
        for (int r = 0; r < BP_ITEMS; r++) sp[r] = a.ct.span(pp[r]);
    }
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++)
        buf[threadIdx.x + r * BP_THREADS] = make_uint4((uint32_t)key[r], (uint32_t)(key[r] >> 32), sp[r].x, sp[r].y);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        const uint64_t k = first + j;
        const bool in = j < have;
        const uint32_t p = pp[r];
        uint32_t lp = 0, ln = 0;
        const bool head = gg[r] == (uint32_t)k;
        bool next_head = true;
        if (in && k > 0) {
            uint64_t kp;
            uint2 sprev;
            if (j > 0) { const uint4 q = buf[j - 1]; kp = (uint64_t)q.y << 32 | q.x; sprev = make_uint2(q.z, q.w); }
            else { kp = a.keys[k - 1]; const uint32_t pq = a.vals[k - 1]; sprev = bounded ? bp_span_bound(a, pq) : a.ct.span(pq); }
            if (kp != key[r]) {
                uint32_t hint = ColTest::meet(sprev, sp[r]);
                if (hint && bounded) hint = a.ct.same(a.vals[k - 1], p);
                lp = fbg_key_lcp_inv(kp, key[r], inv_b, a.key_bits) | hint;
            }
        }
        if (in && k + 1 < a.N) {
            uint64_t kn;
            uint2 snext;
            if (j + 1 < have) { const uint4 q = buf[j + 1]; kn = (uint64_t)q.y << 32 | q.x; snext = make_uint2(q.z, q.w); }
            else { kn = a.keys[k + 1]; const uint32_t pq = a.vals[k + 1]; snext = bounded ? bp_span_bound(a, pq) : a.ct.span(pq); }
            next_head = kn != key[r];
            if (next_head) {
                uint32_t hint = ColTest::meet(sp[r], snext);
                if (hint && bounded) hint = a.ct.same(p, a.vals[k + 1]);
                ln = fbg_key_lcp_inv(key[r], kn, inv_b, a.key_bits) | hint;
            }
        }
        e[r] = make_uint4(p, gg[r], lp, ln);
        if (in) a.flags[k] = !(head && next_head);
    }
    bp_regroup_write(a, e, have, buf, cnt, loff, gbase, wsum);
}

// second splitting pass: a stretch of the first, tile by tile, by the next bits of the position
__global__ __launch_bounds__(BP_THREADS) void k_bp_split(BpArgs a)
{
    __shared__ uint4 buf[BP_TILE];
    __shared__ uint32_t cnt[BP_MAXD], loff[BP_MAXD];
    __shared__ unsigned long long gbase[BP_MAXD];
    __shared__ uint32_t wsum[BP_THREADS / 64];
    const uint64_t seg = blockIdx.x / a.tiles_per_seg;
    const uint64_t seg_lo = seg << a.seg_shift, seg_hi = min(a.N, (seg + 1) << a.seg_shift);
    const uint64_t first = seg_lo + (uint64_t)(blockIdx.x % a.tiles_per_seg) * BP_TILE;
    cnt[threadIdx.x] = 0;
    uint4 e[BP_ITEMS];
    const uint32_t have = first < seg_hi ? (uint32_t)min((uint64_t)BP_TILE, seg_hi - first) : 0u;
#pragma unroll
    for (int r = 0; r < BP_ITEMS; r++) {
        const uint32_t j = threadIdx.x + r * BP_THREADS;
        e[r] = j < have ? a.in[first + j] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (have == 0) return;                                         // uniform
    bp_regroup_write(a, e, have, buf, cnt, loff, gbase, wsum);
}

// last pass: the BP_LEAF positions of a leaf, each dropped at its own place in LDS, leave as finished records
__global__ __launch_bounds__(512) void k_bp_leaf(const uint4 *__restrict__ in, uint64_t N, uint4 *__restrict__ rec,
                                                 unsigned long long *__restrict__ flag)
{
    __shared__ uint32_t sg[BP_LEAF], sl[BP_LEAF], sn[BP_LEAF];
    const uint64_t lo = (uint64_t)blockIdx.x << BP_LEAF_BITS;
    const uint32_t have = (uint32_t)min((uint64_t)BP_LEAF, N - lo);
    for (uint32_t j = threadIdx.x; j < have; j += blockDim.x) {
        const uint4 x = in[lo + j];
        const uint32_t i = x.x - (uint32_t)lo;
        if (i < have) { sg[i] = x.y; sl[i] = x.z; sn[i] = x.w; }
        else *flag = 1;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < have; j += blockDim.x) rec[lo + j] = make_uint4(sg[j], sl[j], sn[j], 0u);
}

// doubling rounds: new group heads -> rank word of the records, suffix array slots, unresolved flags
__global__ void k_apply_groups(const uint32_t *__restrict__ grp, const uint32_t *__restrict__ vals, uint64_t cnt,
                               const uint32_t *__restrict__ where, uint4 *__restrict__ rec,
                               uint32_t *__restrict__ sa, uint8_t *__restrict__ flags)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t r = where[k], g = grp[k], p = vals[k];
    rec[p].x = g;
    sa[r] = p;
    const bool head = g == r;
    const bool next_head = (k + 1 == cnt) || (grp[k + 1] == where[k + 1]);
    flags[k] = !(head && next_head);
}

// After the last round: members of round-0 tie groups get their final neighbour LCPs and hints.
// dirty[] = SA indices of those members.  A neighbour with a different round-0 key keeps its key-derived
// LCP, but its hint depends on who finally sits next to it, so that word is rewritten from here too
// (both sides compute the identical word).
__global__ void k_fix_dirty(const uint32_t *__restrict__ dirty, uint64_t cnt, const uint32_t *__restrict__ sa,
                            const uint64_t *__restrict__ key0, const uint8_t *__restrict__ T, uint64_t N, int b,
                            int key_bits, int K, ColTest ct, uint4 *__restrict__ rec)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t r = dirty[k], p = sa[r];
    const uint64_t key = key0[r];
    uint32_t lp = 0, ln = 0;
    if (r > 0) {
        const uint32_t q = sa[r - 1];
        const uint64_t kq = key0[r - 1];
        if (kq == key) {
            lp = fbg_clamp_lcp(fbg_extend_match(T, (uint64_t)q + K, (uint64_t)p + K, 0) + (uint32_t)K) | ct.same(q, p);
        } else {
            lp = fbg_key_lcp_inv(kq, key, fbg_key_inv(b), key_bits) | ct.same(q, p);
            rec[q].z = lp;
        }
    }
    if ((uint64_t)r + 1 < N) {
        const uint32_t q = sa[r + 1];
        const uint64_t kq = key0[r + 1];
        if (kq == key) {
            ln = fbg_clamp_lcp(fbg_extend_match(T, (uint64_t)p + K, (uint64_t)q + K, 0) + (uint32_t)K) | ct.same(p, q);
        } else {
            ln = fbg_key_lcp_inv(key, kq, fbg_key_inv(b), key_bits) | ct.same(p, q);
            rec[q].y = ln;
        }
    }
    rec[p].y = lp;
    rec[p].z = ln;
}

// indices of the set flags (bytes), ascending: per tile of 16 KiB of flags a count, an exclusive scan of the counts
// (small), then every tile writes its indices at its offset.  (rocPRIM's select over a byte array took 5 ms for
// 5 * 10^8 flags: these two passes read 1 byte per element at full width, 0.3 ms.)
#define FC_THREADS 256
#define FC_TILE (FC_THREADS * 64)
template <bool WRITE>
__global__ __launch_bounds__(FC_THREADS) void k_flag_compact(const uint8_t *__restrict__ flags, uint64_t cnt, uint32_t *__restrict__ tile_cnt,
                                                             uint32_t *__restrict__ sel)
{
    __shared__ uint32_t lds[FC_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * FC_TILE + (uint64_t)threadIdx.x * 64;
    // 64 flags per thread: four 16-byte loads (flags[] is allocated in whole tiles)
    uint32_t bits[2] = {0, 0};
    const uint4 *src = reinterpret_cast<const uint4 *>(flags + base);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (base + 16 * q < cnt) v = src[q];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const bool set = ((w4[i >> 2] >> (8 * (i & 3))) & 0xffu) != 0 && base + 16 * q + i < cnt;
            bits[(16 * q + i) >> 5] |= (set ? 1u : 0u) << ((16 * q + i) & 31);
        }
    }
    const uint32_t mine = (uint32_t)__popc(bits[0]) + (uint32_t)__popc(bits[1]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (int k = 0; k < FC_THREADS / 64; k++) { if (k < w) pre += lds[k]; tot += lds[k]; }
    if (!WRITE) {
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
        return;
    }
    uint32_t at = tile_cnt[blockIdx.x] + pre + inc - mine;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t b = bits[h];
        while (b) {
            const int i = __ffs((int)b) - 1;
            b &= b - 1;
            sel[at++] = (uint32_t)(base + 32 * h + i);
        }
    }
}

// compact the unresolved members: (SA index, position, group head) triples in SA order
__global__ void k_gather_unresolved(const uint32_t *__restrict__ sel, uint64_t cnt, const uint32_t *__restrict__ where_old,
                                    const uint32_t *__restrict__ vals_old, const uint32_t *__restrict__ grp_old,
                                    uint32_t *__restrict__ where_new, uint32_t *__restrict__ vals_new,
                                    uint32_t *__restrict__ grp_new)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    uint32_t s = sel[k];
    where_new[k] = where_old ? where_old[s] : s;
    vals_new[k] = vals_old[s];
    grp_new[k] = grp_old[s];
}

// key = (group head, rank of the suffix h further on)
__global__ void k_doubling_keys(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ grp, uint64_t cnt,
                                const uint4 *__restrict__ rec, uint64_t h, uint64_t N, int nb,
                                uint64_t *__restrict__ keys)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    uint64_t q = (uint64_t)vals[k] + h;
    uint32_t r2 = q < N ? rec[q].x : 0u;   // q < N always holds for unresolved suffixes (unique sentinel)
    keys[k] = ((uint64_t)grp[k] << nb) | r2;                  // both below 2^nb: 2 nb key bits to sort, not 64
}


// ---- host side -----------------------------------------------------------------------------------------------------------------
static ColTest col_test(const fbg_ctx *ctx)
{
    return ColTest{ctx->gapfree ? nullptr : ctx->colT.as<uint32_t>(), (uint32_t)(ctx->n + 1), (uint32_t)ctx->n, (uint32_t)(ctx->N - 1)};
}

// round 0: groups of equal keys among the sorted pairs (keysB / valsB) -> records (rank = SA index of the group head,
// key-derived LCPs), unresolved flags
static int records_round0(fbg_ctx *ctx, const KeyGeom &g, int *launches)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    const uint64_t *keys = ctx->keysB.as<uint64_t>();
    const uint32_t *vals = ctx->valsB.as<uint32_t>();
    uint32_t *grp = ctx->grp.as<uint32_t>();
    uint4 *rec = ctx->rec.as<uint4>();
    uint8_t *flags = ctx->flags.as<uint8_t>();
    const ColTest ct = col_test(ctx);
    hipLaunchKernelGGL(k_mark_heads, dim3(fbg_blocks(N, 256)), dim3(256), 0, st, keys, N, (const uint32_t *)nullptr, grp);
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, grp, grp, (size_t)N, rocprim::maximum<uint32_t>(), st);
    }));
    // FBG_BP_MIN lowers the size from which the records travel to their positions in passes (tests); FBG_RECORD_SCATTER
    // keeps the direct scatter
    const uint64_t bp_min = ctx->opt.bp_min >= 0 ? (uint64_t)ctx->opt.bp_min : (1ull << 24);
    if (N < bp_min || N <= 2 * BP_LEAF || N > 1500000000ull || ctx->opt.record_scatter) {
        hipLaunchKernelGGL(k_apply_groups0, dim3(fbg_blocks(N, 256)), dim3(256), 0, st, grp, vals, keys, N, g.b, g.key_bits, ct, rec, flags);
        *launches += 4;
        return FBG_OK;
    }
    int bits = 0;
    while ((1ull << bits) < N) bits++;
    const int S = bits - BP_LEAF_BITS, d1 = (S + 1) / 2, d2 = S - d1;      // two splitting passes, then leaves
    FBG_TRY(fbg_reserve(ctx, ctx->msd_w, N * 16));
    FBG_TRY(fbg_reserve(ctx, ctx->msd_v, N * 16));
    const uint64_t nleaf = (N + BP_LEAF - 1) >> BP_LEAF_BITS, ntop = (N >> (d2 + BP_LEAF_BITS)) + 1, nwin = (N >> BP_WIN_BITS) + 1;
    FBG_TRY(fbg_reserve(ctx, ctx->list, (ntop + nleaf + 2) * 8 + 3 * nwin * 4));
    unsigned long long *cur1 = ctx->list.as<unsigned long long>(), *cur2 = cur1 + ntop + 1;
    uint2 *win = reinterpret_cast<uint2 *>(cur1 + ntop + nleaf + 2);
    uint32_t *win_lo = reinterpret_cast<uint32_t *>(win + nwin);
    if (ct.colT) {
        hipLaunchKernelGGL(k_bp_windows, dim3(fbg_blocks(nwin, 4)), dim3(256), 0, st, ct.colT, N, ct.n, win, win_lo);
        *launches += 1;
    }
    unsigned long long *bflag = &fbg_scalars(ctx)->by_position;
    FBG_HIP_TRY(ctx, hipMemsetAsync(cur1, 0, (ntop + nleaf + 2) * 8, st));
    FBG_HIP_TRY(ctx, hipMemsetAsync(bflag, 0, 8, st));
    BpArgs a;
    a.N = N; a.flag = bflag;
    a.grp = grp; a.vals = vals; a.keys = keys; a.b = g.b; a.key_bits = g.key_bits; a.ct = ct; a.flags = flags;
    a.win = win; a.win_lo = win_lo;
    a.shift = d2 + BP_LEAF_BITS; a.nd = 1u << d1; a.in = nullptr; a.seg_shift = 0; a.tiles_per_seg = 0;
    a.out = ctx->msd_w.as<uint4>(); a.cursor = cur1;
    hipLaunchKernelGGL(k_bp_groups0, dim3(fbg_blocks(N, BP_TILE)), dim3(BP_THREADS), 0, st, a);
    a.in = ctx->msd_w.as<uint4>(); a.seg_shift = d2 + BP_LEAF_BITS;
    a.tiles_per_seg = (uint32_t)(((1ull << a.seg_shift) + BP_TILE - 1) / BP_TILE);
    a.shift = BP_LEAF_BITS; a.nd = 1u << d2; a.out = ctx->msd_v.as<uint4>(); a.cursor = cur2;
    hipLaunchKernelGGL(k_bp_split, dim3((unsigned)(ntop * a.tiles_per_seg)), dim3(BP_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_bp_leaf, dim3((unsigned)nleaf), dim3(512), 0, st, ctx->msd_v.as<uint4>(), N, rec, bflag);
    unsigned long long hf = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&hf, bflag, 8, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *launches += 6;
    if (hf != 0) return fbg_fail(ctx, FBG_ERR_HIP, "records by position: the sorted positions are not a permutation");
    return FBG_OK;
}

// the unresolved among the first cnt entries of the current list: their indices, ascending, into ctx->list; *count of them
static int select_unresolved(fbg_ctx *ctx, uint64_t cnt, uint64_t *count, int *launches)
{
    hipStream_t st = ctx->stream;
    const uint8_t *flags = ctx->flags.as<uint8_t>();
    uint32_t *sel = ctx->list.as<uint32_t>();
    const unsigned ftiles = fbg_blocks(cnt, FC_TILE);
    FBG_TRY(fbg_reserve(ctx, ctx->ps_a, ((size_t)ftiles + 1) * 4));
    uint32_t *tile_cnt = ctx->ps_a.as<uint32_t>();
    hipLaunchKernelGGL((k_flag_compact<false>), dim3(ftiles), dim3(FC_THREADS), 0, st, flags, cnt, tile_cnt, sel);
    FBG_HIP_TRY(ctx, hipMemsetAsync(tile_cnt + ftiles, 0, 4, st));
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, tile_cnt, tile_cnt, 0u, (size_t)ftiles + 1, rocprim::plus<uint32_t>(), st);
    }));
    hipLaunchKernelGGL((k_flag_compact<true>), dim3(ftiles), dim3(FC_THREADS), 0, st, flags, cnt, tile_cnt, sel);
    uint32_t h32 = 0;
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&h32, tile_cnt + ftiles, 4, hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *count = h32;
    *launches += 3;
    return FBG_OK;
}

// the compacted list of the unresolved, in SA order: where[k] = SA index (nullptr: k itself, round 0), vals[k] = position
struct Unresolved { uint64_t cnt; const uint32_t *where; uint32_t *vals, *grp; };

// one doubling round: the ncnt selected members of `cur` (ctx->list) become the new list in the buffers of parity pp, are
// sorted by (group, rank of the suffix h further on) and regrouped
static int doubling_round(fbg_ctx *ctx, Unresolved &cur, uint64_t ncnt, int pp, uint64_t h, uint64_t *dkeys_in, uint64_t *dkeys_out, int *launches)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    DevBuf *nbuf[3] = {pp ? &ctx->dp_b : &ctx->dp_a, pp ? &ctx->dp_d : &ctx->dp_c, pp ? &ctx->dp_f : &ctx->dp_e};
    for (DevBuf *d : nbuf) FBG_TRY(fbg_reserve(ctx, *d, ncnt * 4));
    uint32_t *where_new = nbuf[0]->as<uint32_t>(), *vals_new = nbuf[1]->as<uint32_t>(), *grp_new = nbuf[2]->as<uint32_t>();
    uint32_t *valsA = ctx->valsA.as<uint32_t>();
    uint4 *rec = ctx->rec.as<uint4>();
    hipLaunchKernelGGL(k_gather_unresolved, dim3(fbg_blocks(ncnt, 256)), dim3(256), 0, st, ctx->list.as<uint32_t>(), ncnt, cur.where,
                       cur.vals, cur.grp, where_new, vals_new, grp_new);
    int nb = 1;
    while ((1ull << nb) < N) nb++;
    hipLaunchKernelGGL(k_doubling_keys, dim3(fbg_blocks(ncnt, 256)), dim3(256), 0, st, vals_new, grp_new, ncnt, rec, h, N, nb, dkeys_in);
    // sort by (group, rank at +h); the sorted positions go back to the same SA slots
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        if (ncnt >= (1u << 23))
            return rocprim::radix_sort_pairs<fbg_sort_config>(tmp, bytes, dkeys_in, dkeys_out, vals_new, valsA, (size_t)ncnt, 0u, (unsigned)(2 * nb), st);
        return rocprim::radix_sort_pairs(tmp, bytes, dkeys_in, dkeys_out, vals_new, valsA, (size_t)ncnt, 0u, (unsigned)(2 * nb), st);
    }));
    hipLaunchKernelGGL(k_mark_heads, dim3(fbg_blocks(ncnt, 256)), dim3(256), 0, st, dkeys_out, ncnt, where_new, grp_new);
    FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, grp_new, grp_new, (size_t)ncnt, rocprim::maximum<uint32_t>(), st);
    }));
    hipLaunchKernelGGL(k_apply_groups, dim3(fbg_blocks(ncnt, 256)), dim3(256), 0, st, grp_new, valsA, ncnt, where_new, rec,
                       ctx->valsB.as<uint32_t>(), ctx->flags.as<uint8_t>());
    // the sorted positions become the list's values for the next round
    FBG_HIP_TRY(ctx, hipMemcpyAsync(vals_new, valsA, ncnt * 4, hipMemcpyDeviceToDevice, st));
    *launches += 7;
    cur = Unresolved{ncnt, where_new, vals_new, grp_new};
    return FBG_OK;
}

// The sorted (key, position) pairs in keysB / valsB, keys of geometry g: valsB becomes the suffix array, rec the records.
int fbg_record_sort(fbg_ctx *ctx, const KeyGeom &g, int *launches)
{
    const uint64_t N = ctx->N;
    hipStream_t st = ctx->stream;
    FBG_TRY(fbg_build_cell_tables(ctx));       // the per-cell tables of the record path's column scan
    FBG_TRY(fbg_reserve(ctx, ctx->grp, N * 4));
    FBG_TRY(fbg_reserve(ctx, ctx->flags, (N + FC_TILE - 1) / FC_TILE * FC_TILE));   // whole tiles: k_flag_compact loads 16 bytes at a time
    FBG_TRY(fbg_reserve(ctx, ctx->rec, N * 16));
    FBG_TRY(records_round0(ctx, g, launches));
    FBG_TRY(fbg_reserve(ctx, ctx->list, N * 4));
    Unresolved cur = {N, nullptr, ctx->valsB.as<uint32_t>(), ctx->grp.as<uint32_t>()};
    uint64_t dirty_cnt = 0, h = (uint64_t)g.K;
    uint64_t *dkeys_in = ctx->keysA.as<uint64_t>(), *dkeys_out = ctx->keysB.as<uint64_t>();
    ctx->ix.lcp_from_keys = false;
    for (int round = 1;; round++, h *= 2) {
        uint64_t hc = 0;
        FBG_TRY(select_unresolved(ctx, cur.cnt, &hc, launches));
        if (round == 1) {
            // few ties: the key-derived LCPs stand, only the tie groups are patched afterwards;
            // the round-0 keys (keysB) must then survive the doubling rounds
            ctx->ix.lcp_from_keys = hc <= N / 32 && !ctx->opt.lcp_text;
            if (ctx->ix.lcp_from_keys && hc > 0) {
                dirty_cnt = hc;
                FBG_TRY(fbg_reserve(ctx, ctx->io_d, hc * 4));
                FBG_HIP_TRY(ctx, hipMemcpyAsync(ctx->io_d.p, ctx->list.p, hc * 4, hipMemcpyDeviceToDevice, st));
                FBG_TRY(fbg_reserve(ctx, ctx->dp_g, hc * 8));
                FBG_TRY(fbg_reserve(ctx, ctx->dp_h, hc * 8));
                dkeys_in = ctx->dp_g.as<uint64_t>();
                dkeys_out = ctx->dp_h.as<uint64_t>();
            }
        }
        if (hc == 0) break;
        if (round > 64) return fbg_fail(ctx, FBG_ERR_HIP, "suffix sort did not converge");
        FBG_TRY(doubling_round(ctx, cur, hc, (round - 1) & 1, h, dkeys_in, dkeys_out, launches));
    }
    if (ctx->ix.lcp_from_keys && dirty_cnt > 0) {
        hipLaunchKernelGGL(k_fix_dirty, dim3(fbg_blocks(dirty_cnt, 256)), dim3(256), 0, st, ctx->io_d.as<uint32_t>(), dirty_cnt,
                           ctx->valsB.as<uint32_t>(), ctx->keysB.as<uint64_t>(), ctx->text.as<uint8_t>(), N, g.b, g.key_bits, g.K,
                           col_test(ctx), ctx->rec.as<uint4>());
        *launches += 1;
    }
    ctx->ix.kind = IndexKind::record;          // the index is the records by text position
    return FBG_OK;
}
