// rank_tail.hip -- the candidate tail of the rank-order scan (rank_scan.hip): from "the scan has listed its candidates" to "the
// column maxima are raised".  Candidates are the SA slots the scan could not settle by looking at their nearest neighbours: slots
// with a same-column neighbour, members of larger or entangled tie groups.  The scan's workgroups list them in regions of their
// own.  The tail (1) puts them in SA order, (2) puts the tie groups they belong to in text order, which is final SA order, and
// (3) gives every maximal run of same-column neighbouring slots its extensions,
//     g = 1 + max(min LCP towards the run head, min LCP towards the run tail) per member   (fbg.cpp:1644-1678).
// Three tiers, picked once (rs_tail_order) from the scan that ran and the largest region's count:
//   by head, radix   after k_rank_scan (a workgroup's chunks are scattered over the slots), or a region beyond the LDS capacity
//                    (RS_CAND_LDS, option cand_lds_cap), or option cand_local_sort off: k_cand_compact, rocPRIM's radix sort,
//                    k_tie_groups + k_tie_big; then k_runs, a thread per run head walking its run, and k_runs_long, a wave for
//                    every run of runs_wave_min members and more.
//   by head, local   after k_rank_scan_lean, every region within the LDS capacity: the regions ascend with the workgroups, so
//                    k_cand_sort_compact sorts each in LDS on its way out; the rest as above.
//   by member        the same condition with option cand_tail (the default) and columns below 2^30: k_cand_region sorts a region
//                    and orders the tie groups it heads in one kernel, + k_tie_big; k_cand_lcp computes every LCP once, by
//                    candidate; k_cand_runs and k_cand_runs_long take the runs' minima over those arrays (cand_tail.h).
// With partitions (fbg_rank_part_classify / fbg_rank_part_runs) the runs wait for the neighbours' edge slots: order in phase 1,
// runs in phase 2, by head.  fbg_rank_materialize orders the tie groups of every slot (rs_tail_order_all).
#include <algorithm>
#include "fbg_internal.h"
#include "text_cmp.h"
#include <rocprim/rocprim.hpp>

#include "rank_common.h"
#include "tie_extent.h"
#include "cand_tail.h"
#include "rank_tail.h"

// candidate regions of the workgroups -> one contiguous list (offsets = exclusive scan of the counts)
__global__ void k_cand_compact(const uint32_t *__restrict__ regions, const uint32_t *__restrict__ counts,
                               const uint32_t *__restrict__ offsets, uint32_t region, uint32_t *__restrict__ out)
{
    const uint32_t c = counts[blockIdx.x] < region ? counts[blockIdx.x] : region, o = offsets[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) out[o + i] = regions[(size_t)blockIdx.x * region + i];
}

// The same after k_rank_scan_lean, where a workgroup owns one contiguous stretch of the slots and the stretches ascend with the
// workgroups: what a region holds lies in its workgroup's stretch -- but for the tail of a pair whose head is the stretch's last
// slot, the first slot of the next stretch, which its owner never lists (a row's lane 3 that ties with lane 2 and not with lane 4
// is neither head of a pair, nor member of a longer group, nor "not tied": none of the masks Q is made of) -- so regions sorted
// one by one and written out at their offsets are the sorted list: no device-wide sort.  Bitonic sort in LDS, counts up to
// RS_CAND_LDS (the host knows the largest).
#define RS_CAND_LDS 4096
__global__ __launch_bounds__(256) void k_cand_sort_compact(const uint32_t *__restrict__ regions, const uint32_t *__restrict__ counts,
                                                           const uint32_t *__restrict__ offsets, uint32_t region, uint32_t *__restrict__ out)
{
    __shared__ uint32_t buf[RS_CAND_LDS];
    const uint32_t c = min(min(counts[blockIdx.x], region), (uint32_t)RS_CAND_LDS), o = offsets[blockIdx.x];
    if (c == 0) return;
    uint32_t P = 2;
    while (P < c) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) buf[i] = i < c ? regions[(size_t)blockIdx.x * region + i] : 0xffffffffu;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t x = buf[i], y = buf[l];
                    if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[l] = x; }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) out[o + i] = buf[i];
}

// The candidate counts of the workgroups (nb of them, 4096 at most) -> their exclusive offsets offs[0 .. nb] (offs[nb]: the total),
// and the total and the largest count side by side in tot_max[0 .. 1], for one copy to the host.  One workgroup: a thread
// takes a stretch of counts, the stretches' sums are scanned across the wave and then across the 16 waves.
#define RS_COUNTS_THREADS 1024
__global__ __launch_bounds__(RS_COUNTS_THREADS) void k_cand_counts(const uint32_t *__restrict__ counts, uint32_t nb, uint32_t *__restrict__ offs,
                                                                   uint32_t *__restrict__ tot_max)
{
    __shared__ uint32_t wsum[RS_COUNTS_THREADS / 64], wmax[RS_COUNTS_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t per = (nb + RS_COUNTS_THREADS - 1) / RS_COUNTS_THREADS;
    const uint32_t i0 = min(threadIdx.x * per, nb), i1 = min(i0 + per, nb);
    uint32_t sum = 0, mx = 0;
    for (uint32_t i = i0; i < i1; i++) { const uint32_t c = counts[i]; sum += c; mx = max(mx, c); }
    uint32_t inc = sum;                                                // inclusive scan of the stretches' sums in the wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += o;
    }
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    if (lane == 63) wsum[wv] = inc;
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    uint32_t before = inc - sum, total = 0, largest = 0;
    for (uint32_t v = 0; v < RS_COUNTS_THREADS / 64; v++) {
        if (v < wv) before += wsum[v];
        total += wsum[v];
        largest = max(largest, wmax[v]);
    }
    for (uint32_t i = i0; i < i1; i++) { offs[i] = before; before += counts[i]; }
    if (threadIdx.x == 0) { offs[nb] = total; tot_max[0] = total; tot_max[1] = largest; }
}

// debugging aid (option cand_sort_check): places of the sorted candidate list that do not ascend
__global__ void k_cand_inversions(const uint32_t *__restrict__ cand, uint64_t T, unsigned long long *__restrict__ count)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long mask = __ballot(t + 1 < T && cand[t] >= cand[t + 1]);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(count, (unsigned long long)__popcll(mask));
}

// a slot whose key equals its successor's but not its predecessor's heads a tie group: put the group in text
// order.  by_list: t indexes the sorted candidates; otherwise every owned slot (fbg_rank_materialize).
// Groups of more than 64 go to k_tie_big.
#define RS_BIG_GROUPS 1024
#define RS_BIG_MEMBERS 8192
template <int L> __global__ void k_tie_groups(RankArgs a, uint64_t T, int by_list, int gallop)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t k0 = by_list ? (uint64_t)a.cand[t] : a.own_lo + t;
    const uint64_t key = rs_key<L>(a, k0);
    if (k0 > a.own_lo && rs_key<L>(a, k0 - 1) == key) return;                      // inside a group
    if (k0 + 1 >= a.own_hi || rs_key<L>(a, k0 + 1) != key) return;                 // not a tie (ties never cross partitions)
    // the group's size, RS_BIG_MEMBERS + 1 for anything larger.  Counting member by member is one dependent load each: the
    // row ends make groups of a thousand and more, and the whole kernel is as long as that one thread (gallop: tie_extent.h)
    uint32_t s = 1;
    if (gallop) s = fbg_tie_extent(k0, a.own_hi, RS_BIG_MEMBERS, key, [&](uint64_t k) { return rs_key<L>(a, k); });
    else while (k0 + s < a.own_hi && s <= RS_BIG_MEMBERS && rs_key<L>(a, k0 + s) == key) s++;
    if (s > 64) {
        if (s > RS_BIG_MEMBERS) { a.counters[1] = 1; return; }
        const unsigned long long e = atomicAdd(&a.counters[5], 1ull);
        if (e >= RS_BIG_GROUPS) { a.counters[1] = 1; return; }
        a.big[2 * e] = (uint32_t)k0;
        a.big[2 * e + 1] = s;
        return;
    }
    // order the s suffixes by their text (insertion sort, s is tiny).  The first K symbols agree -- unless a member
    // has fewer than K symbols left in its row: then the keys agree only up to the separator coding
    typedef typename PosT<L>::type pos_t;
    pos_t pos[64];
    uint32_t from = (uint32_t)a.K;
    for (uint32_t i = 0; i < s; i++) {
        pos[i] = (pos_t)rs_pos<L>(a, k0 + i);
        if (rs_rem<L>(a, pos[i]) < (uint32_t)a.K) from = 0;
    }
    for (uint32_t i = 1; i < s; i++) {
        const pos_t cur = pos[i];
        uint32_t j = i;
        while (j > 0) {
            const pos_t o = pos[j - 1];
            const uint32_t h = fbg_extend_match(a.T, (uint64_t)o + from, (uint64_t)cur + from, 0);
            if (a.T[(uint64_t)o + from + h] < a.T[(uint64_t)cur + from + h]) break;      // o < cur: in place
            pos[j] = o;
            j--;
        }
        pos[j] = cur;
    }
    for (uint32_t i = 0; i < s; i++) rs_set_pos<L>(a, k0 + i, pos[i]);
}

// Long tie groups exist where many rows end alike: the members of a group share their real symbols and differ in
// how many they have left (r#, rA#, rAA#, ... and the suffixes with K real symbols), '#' being the smallest
// symbol.  Text order is therefore: by symbols left (capped at K) first.  Members with the same number left sit in
// one MSA column: a run whose inner order has no influence on any extension (the LCPs inside exceed those at its
// two ends, fbg.cpp:1644-1656) -- left as it is unless `exact` (fbg_index_download wants the true suffix array).
// The members with K real symbols are ordered by their text; more than 64 of those -> fallback flag, or with exact = 2 the
// whole group as under exact = 1.
// One workgroup per group.
template <int L> __global__ __launch_bounds__(256) void k_tie_big(RankArgs a, int exact)
{
    __shared__ uint32_t pos_lo[RS_BIG_MEMBERS];
    __shared__ uint8_t pos_hi[L == FBG_SLOTS_WIDE ? RS_BIG_MEMBERS : 1];     // positions beyond 32 bits: their top byte
    __shared__ uint8_t cls[RS_BIG_MEMBERS];
    __shared__ uint32_t offs[66];
    __shared__ uint32_t q_start, q_count;
    if (blockIdx.x >= a.counters[5]) return;
    const uint64_t k0 = a.big[2 * blockIdx.x];
    const uint32_t s = a.big[2 * blockIdx.x + 1];
    auto member = [&](uint32_t i) -> uint64_t {
        return L == FBG_SLOTS_WIDE ? ((uint64_t)pos_hi[L == FBG_SLOTS_WIDE ? i : 0] << 32) | pos_lo[i] : (uint64_t)pos_lo[i];
    };
    if (threadIdx.x < 66) offs[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < s; i += blockDim.x) {
        const uint64_t p = rs_pos<L>(a, k0 + i);
        const uint32_t c = min(rs_rem<L>(a, p), (uint32_t)a.K);
        pos_lo[i] = (uint32_t)p;
        if (L == FBG_SLOTS_WIDE) pos_hi[L == FBG_SLOTS_WIDE ? i : 0] = (uint8_t)(p >> 32);
        cls[i] = (uint8_t)c;
        atomicAdd(&offs[c + 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        q_count = offs[a.K + 1];
        for (int c = 1; c <= a.K + 1; c++) offs[c] += offs[c - 1];      // offs[c] = first slot of class c
        q_start = offs[a.K];
    }
    __syncthreads();
    // exact = 2 (behind the lean scan): more than 64 members with K real symbols -- a stretch that many rows share -- are no
    // reason to give the scan up: the ranks below order such a group like any other
    if (exact == 0 || (exact == 2 && q_count <= 64)) {
        for (uint32_t i = threadIdx.x; i < s; i += blockDim.x) {
            const uint32_t dst = atomicAdd(&offs[cls[i]], 1u);
            rs_set_pos<L>(a, k0 + dst, member(i));
        }
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t q = q_count;
            if (q > 64) { a.counters[1] = 1; return; }
            const uint64_t kq = k0 + q_start;
            for (uint32_t i = 1; i < q; i++) {                          // insertion sort by the text beyond the key
                const uint64_t cur = rs_pos<L>(a, kq + i);
                uint32_t j = i;
                while (j > 0) {
                    const uint64_t o = rs_pos<L>(a, kq + j - 1);
                    const uint32_t h = fbg_extend_match(a.T, o + a.K, cur + a.K, 0);
                    if (a.T[o + a.K + h] < a.T[cur + a.K + h]) break;
                    rs_set_pos<L>(a, kq + j, o);
                    j--;
                }
                rs_set_pos<L>(a, kq + j, cur);
            }
        }
        return;
    }
    // exact: rank of every member among all members by text comparison (distinct suffixes: ranks are a permutation)
    for (uint32_t i = threadIdx.x; i < s; i += blockDim.x) {
        const uint64_t p = member(i);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < s; j++) {
            if (j == i) continue;
            const uint64_t o = member(j);
            const uint32_t h = fbg_extend_match(a.T, o, p, 0);
            rank += a.T[o + h] < a.T[p + h] ? 1u : 0u;
        }
        rs_set_pos<L>(a, k0 + rank, p);
    }
}

// candidates (sorted, final SA order): one thread per run head walks its run of same-column slots.  With
// partitions a run may begin or end in a halo (copies of the neighbouring partition's edge slots): it is walked
// in full, but only owned members update the column maxima -- the neighbour does the same from its side.
template <int L> __global__ void k_runs(RankArgs a, uint64_t T)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t k0 = a.cand[t];
    const uint32_t col = rs_col<L>(a, k0);
    if (col == a.n) return;                                            // '#' / sentinel: not a row pointer
    if (k0 > a.own_lo && rs_col<L>(a, k0 - 1) == col) return;         // an owned predecessor heads this run
    const uint64_t lo_slot = a.first_part ? a.own_lo : 0, hi_slot = a.last_part ? a.own_hi : a.N;
    uint64_t ks = k0;                                                  // true head: possibly inside the previous halo
    while (ks > lo_slot && rs_col<L>(a, ks - 1) == col) ks--;
    if (ks == 0 && !a.first_part) { a.counters[1] = 1; return; }       // run longer than the halo
    // forward: running minimum of LCP[lb..r]   (owned members of a run are contiguous in cand[])
    uint32_t run = rs_slot_lcp<L>(a, ks);
    uint64_t s = ks;
    for (;;) {
        if (s >= k0 && s < a.own_hi) a.pm[t + (s - k0)] = run;
        if (s + 1 >= hi_slot || rs_col<L>(a, s + 1) != col) break;
        s++;
        if (a.runs_wave_min && s - ks + 1 == a.runs_wave_min) {        // a long run: a wave walks it (k_runs_long), unless the list is full
            const unsigned long long e = atomicAdd(&a.counters[7], 1ull);
            if (e < a.wl_cap) { a.wl[2 * e] = (uint32_t)t; a.wl[2 * e + 1] = (uint32_t)ks; return; }
        }
        run = min(run, rs_slot_lcp<L>(a, s));
    }
    if (s + 1 == a.N && !a.last_part) { a.counters[1] = 1; return; }   // ran through the next halo
    // backward: running minimum of LCP[r+1..rb+1], extension, column maximum   (fbg.cpp:1656)
    uint32_t rmin = 0xffffffffu;
    for (;; s--) {
        rmin = min(rmin, rs_slot_lcp<L>(a, s + 1));
        if (s >= k0 && s < a.own_hi) rs_update(a, col, max(a.pm[t + (s - k0)], rmin) + 1);
        if (s == ks || s <= k0) break;                                 // members before k0 belong to the neighbour
    }
}

// ---- a long run walked by a wave (k_runs_long, k_cand_runs_long) ----
// The last column of 1000 rows holds 250 suffixes "X#" per symbol, one run: 500 text comparisons one after the other for a
// thread.  One wave per run, 64 members at a time, a lane each: the members' LCPs side by side, an inclusive minimum scan across
// the wave with a carry from chunk to chunk -- forward into pm, then backward from the tail; the arithmetic is k_runs'
// (fbg.cpp:1644-1678).  The members share their column: one update of its maximum.

// the inclusive minimum across the wave: lane l gets the minimum of lanes 0 .. l (UP) or of lanes l .. 63
template <bool UP> __device__ __forceinline__ uint32_t rt_wave_min(uint32_t v, uint32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = UP ? __shfl_up(v, d, 64) : __shfl_down(v, d, 64);
        if (UP ? lane >= (uint32_t)d : lane + (uint32_t)d < 64) v = min(v, o);
    }
    return v;
}

// The walk.  pm: the prefix minima of the run's members, member 0 first.  The kernels say where a member's facts come from:
//   member(i)      is slot / candidate i, counted from the run's head, still in the run?  (true for 0; once false, never asked again)
//   before(i)      the LCP of member i with the slot before it
//   after(i, len)  the LCP of member i with the slot after it, in a run of len members
// Idx: what the members are counted in -- slots in 64 bits, candidates in 32.
template <class Idx, class Member, class Before, class After>
__device__ __forceinline__ void rt_wave_walk(const RankArgs &a, uint32_t col, uint32_t *pm, Member member, Before before, After after)
{
    const uint32_t lane = threadIdx.x;
    Idx len = 0;
    uint32_t carry = FBG_CT_NONE;
    for (Idx c0 = 0;; c0 += 64) {                                      // forward: minimum of LCP[head .. member]
        const unsigned long long out = ~__ballot(member(c0 + lane));
        const uint32_t cnt = out ? (uint32_t)__ffsll((long long)out) - 1 : 64u;       // members among these 64
        uint32_t v = lane < cnt ? before(c0 + lane) : FBG_CT_NONE;
        v = min(rt_wave_min<true>(v, lane), carry);
        if (lane < cnt) pm[c0 + lane] = v;
        carry = __shfl(v, 63, 64);
        len += cnt;
        if (cnt < 64) break;
    }
    if (len == 0) return;
    uint32_t best = 0;
    carry = FBG_CT_NONE;
    for (Idx c0 = (len - 1) / 64 * 64;; c0 -= 64) {                    // backward: minimum of LCP[member + 1 .. tail + 1], extension
        const Idx i = c0 + lane;
        uint32_t v = after(min(i, (Idx)(len - 1)), len);               // (lanes past the run repeat its last member: every lane asks,
        if (i >= len) v = FBG_CT_NONE;                                 // so what does not depend on the lane stays in scalar registers)
        v = min(rt_wave_min<false>(v, lane), carry);
        if (i < len) best = max(best, max(pm[i], v) + 1);              // (pm[i]: this lane's own store)
        carry = __shfl(v, 0, 64);
        if (c0 == 0) break;
    }
    for (int d = 32; d > 0; d >>= 1) best = max(best, (uint32_t)__shfl_xor(best, d, 64));
    if (lane == 0) rs_update(a, col, best);
}

// The runs k_runs noted (runs_wave_min members and more; no partitions: the head is the candidate itself and every slot is
// owned): the LCPs from the slots, as k_runs computes them.
template <int L> __global__ __launch_bounds__(64) void k_runs_long(RankArgs a)
{
    if (blockIdx.x >= a.counters[7]) return;                            // (the grid is wl_cap blocks)
    const uint64_t t = a.wl[2 * blockIdx.x], ks = a.wl[2 * blockIdx.x + 1];
    const uint32_t col = rs_col<L>(a, ks);
    rt_wave_walk<uint64_t>(a, col, a.pm + t,
                           [&](uint64_t i) { return ks + i < a.own_hi && rs_col<L>(a, ks + i) == col; },
                           [&](uint64_t i) { return rs_slot_lcp<L>(a, ks + i); },
                           [&](uint64_t i, uint64_t) { return rs_slot_lcp<L>(a, ks + i + 1); });
}

// ---- the tail by member (option cand_tail; packed slots, no partitions, regions sorted in LDS; the logic is cand_tail.h's) ----
// k_cand_sort_compact and k_tie_groups in one kernel, a workgroup per region: the region sorted in LDS and written out, the
// word of every candidate kept beside it, a head's group measured on those (fbg_ct_key_from: the slots themselves answer past
// the region's end -- groups span regions, the head's workgroup owns the whole group and is the only one to write its
// positions; other workgroups read the keys of those slots only, which no write changes).  Groups of up to RC_SMALL members
// are ordered by their head's thread in registers, those of up to 64 by a wave with a lane per member (rank = number of
// smaller members, as k_tie_big's exact mode), larger ones go to k_tie_big as from k_tie_groups.  No private array is indexed
// at run time: no scratch.  Every loop is bounded by the region's count, a group's cap or the text's end.
#define RC_SMALL 4

// is the suffix at po smaller than the one at pc?  wo / wc: their first 8 bytes (fbg_load8), loaded by the caller ahead of use
__device__ __forceinline__ bool rc_text_less(const uint8_t *__restrict__ T, uint64_t po, uint64_t pc, uint64_t wo, uint64_t wc)
{
    const uint64_t x = wo ^ wc;
    if (x == 0) {
        const uint32_t h = fbg_extend_match(T, po, pc, 8);
        return T[po + h] < T[pc + h];
    }
    const uint32_t sh = (uint32_t)(__ffsll((unsigned long long)x) - 1) & ~7u;      // the first byte that differs
    return ((wo >> sh) & 0xff) < ((wc >> sh) & 0xff);
}

// a wave's own LDS writes, visible to its other lanes' reads that follow
__device__ __forceinline__ void rc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one compare-exchange stage of the bitonic network over pairs [t0, t1) step `step`: pair t is (i, i + j), i = t with a zero bit
// put in at j's place
__device__ __forceinline__ void rc_bitonic_pairs(uint32_t *buf, uint32_t base, uint32_t t0, uint32_t t1, uint32_t step, uint32_t j, uint32_t k)
{
    for (uint32_t t = t0; t < t1; t += step) {
        const uint32_t i = base + (((t & ~(j - 1)) << 1) | (t & (j - 1))), l = i + j;
        const uint32_t x = buf[i], y = buf[l];
        if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[l] = x; }
    }
}

// LDS (dynamic; the host knows the largest count, cap): the words of a region's first wcap entries, its slots padded to a power
// of two (pmax at most), the entries that head a group (at most every other one) and the groups that get a wave (lcap).  An
// entry past wcap -- the few regions that hold the row ends -- finds its word among the slots, like a slot past the region.
#define RC_WORDS 1024
__global__ __launch_bounds__(256) void k_cand_region(RankArgs a, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                     uint32_t *__restrict__ out, int gallop, uint32_t cap, uint32_t pmax, uint32_t wcap, uint32_t lcap)
{
    constexpr int L = FBG_SLOTS_PACKED;
    extern __shared__ uint64_t rc_lds[];
    uint64_t *wbuf = rc_lds;
    uint32_t *buf = reinterpret_cast<uint32_t *>(wbuf + wcap);
    uint32_t *glist = buf + pmax;
    uint16_t *hlist = reinterpret_cast<uint16_t *>(glist + lcap);
    __shared__ uint32_t gcount, hcount;
    const uint32_t c = min(min(counts[blockIdx.x], a.region), cap), o = offsets[blockIdx.x];
    if (c == 0) return;
    const uint32_t wc = min(c, wcap), hcap = cap / 2 + 2;
    uint32_t P = 2;
    while (P < c) P <<= 1;                                              // (<= pmax: the power of two at or above cap)
    for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) buf[i] = i < c ? a.cand[(size_t)blockIdx.x * a.region + i] : 0xffffffffu;
    if (threadIdx.x == 0) { gcount = 0; hcount = 0; }
    __syncthreads();
    // k_cand_sort_compact's network, scheduled by wave: a wave owns a quarter of the slots (all of them below 256), and only the
    // stages whose partners lie a quarter and more apart -- three of them -- go across the workgroup, between barriers
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t Q = P >= 256 ? P >> 2 : P;
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j >= Q) {
                __syncthreads();
                rc_bitonic_pairs(buf, 0, threadIdx.x, P >> 1, blockDim.x, j, k);
                __syncthreads();
            } else if (wv * Q < P) {
                rc_bitonic_pairs(buf, wv * Q, lane, Q >> 1, 64, j, k);
                rc_wave_sync();
            }
        }
    __syncthreads();
    // the sorted slots out; a candidate's word and its two neighbours', four entries' twelve loads in flight together (an entry
    // past the count repeats the last, a neighbour past the array the slot itself); the heads of groups onto a list
    for (uint32_t i0 = threadIdx.x; i0 < c; i0 += 4 * blockDim.x) {
        uint64_t k[4], w[4], wp[4], wn[4];
#pragma unroll
        for (int q = 0; q < 4; q++) k[q] = buf[min(i0 + (uint32_t)q * blockDim.x, c - 1)];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            w[q] = a.keys[k[q]];
            wp[q] = a.keys[k[q] > 0 ? k[q] - 1 : k[q]];
            wn[q] = a.keys[k[q] + 1 < a.N ? k[q] + 1 : k[q]];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = i0 + (uint32_t)q * blockDim.x;
            if (i >= c) continue;
            out[o + i] = (uint32_t)k[q];
            if (i < wc) wbuf[i] = w[q];
            const uint64_t key = w[q] >> a.pb;
            if (!(k[q] > 0 && (wp[q] >> a.pb) == key) && k[q] + 1 < a.N && (wn[q] >> a.pb) == key) {
                const uint32_t e = atomicAdd(&hcount, 1u);
                if (e < hcap) hlist[e] = (uint16_t)i;
                else a.counters[1] = 1;                                     // (cannot be: a head's successor is no head)
            }
        }
    }
    __syncthreads();
    const uint32_t n_heads = min(hcount, hcap);
    for (uint32_t h = threadIdx.x; h < n_heads; h += blockDim.x) {
        const uint32_t i = hlist[h];
        const uint64_t k0 = buf[i], w0 = i < wc ? wbuf[i] : a.keys[k0], key = w0 >> a.pb;
        auto word_at = [&](uint32_t d) -> uint64_t {                    // the word of slot k0 + d
            const uint32_t j = i + d;
            return j < wc && buf[j] == k0 + d ? wbuf[j] : a.keys[k0 + d];
        };
        auto key_at = [&](uint64_t k) -> uint64_t {
            return fbg_ct_key_from(i, wc, k0, k, [&](uint32_t j) { return (uint64_t)buf[j]; }, [&](uint32_t j) { return wbuf[j] >> a.pb; },
                                   [&](uint64_t s) { return a.keys[s] >> a.pb; });
        };
        uint32_t s = 1;
        if (gallop) s = fbg_tie_extent(k0, a.N, RS_BIG_MEMBERS, key, key_at);
        else while (k0 + s < a.N && s <= RS_BIG_MEMBERS && key_at(k0 + s) == key) s++;
        if (s > 64) {
            if (s > RS_BIG_MEMBERS) { a.counters[1] = 1; continue; }
            const unsigned long long e = atomicAdd(&a.counters[5], 1ull);
            if (e >= RS_BIG_GROUPS) { a.counters[1] = 1; continue; }
            a.big[2 * e] = (uint32_t)k0;
            a.big[2 * e + 1] = s;
            continue;
        }
        if (s > RC_SMALL) {
            const uint32_t e = atomicAdd(&gcount, 1u);
            if (e < lcap) glist[e] = i | s << 16;
            else a.counters[1] = 1;                                         // (cannot be: such groups do not overlap)
            continue;
        }
        // 2 .. RC_SMALL members, in registers: positions, where the comparison starts, the first 8 bytes of every member ahead
        // of the comparisons, every pair compared once
        uint32_t p[RC_SMALL];
        uint64_t w8[RC_SMALL];
#pragma unroll
        for (int d = 0; d < RC_SMALL; d++) p[d] = (uint32_t)(((uint32_t)d < s ? word_at(d) : w0) & a.pmask);
        uint32_t from = (uint32_t)a.K;
#pragma unroll
        for (int d = 0; d < RC_SMALL; d++)
            if (rs_rem<L>(a, p[d]) < (uint32_t)a.K) from = 0;               // (fbg_ct_from; slots past the group repeat the head)
#pragma unroll
        for (int d = 0; d < RC_SMALL; d++) w8[d] = fbg_load8(a.T, (uint64_t)p[d] + from);
        uint32_t rank[RC_SMALL];
        fbg_ct_small_ranks<RC_SMALL>(s, [&](int x, int y) { return rc_text_less(a.T, (uint64_t)p[x] + from, (uint64_t)p[y] + from, w8[x], w8[y]); }, rank);
#pragma unroll
        for (int d = 0; d < RC_SMALL; d++)
            if ((uint32_t)d < s) a.keys[k0 + rank[d]] = key << a.pb | p[d];
    }
    __syncthreads();
    // the groups of RC_SMALL + 1 .. 64 members: a wave each, a lane per member
    const uint32_t groups = min(gcount, lcap);
    for (uint32_t e = threadIdx.x >> 6; e < groups; e += blockDim.x >> 6) {
        const uint32_t i = glist[e] & 0xffffu, s = glist[e] >> 16;
        const uint64_t k0 = buf[i];
        const uint32_t d = lane < s ? lane : 0u, j = i + d;                // (lanes past the group repeat the head: every load is valid)
        const uint64_t w = j < wc && buf[j] == k0 + d ? wbuf[j] : a.keys[k0 + d];
        const uint32_t p = (uint32_t)(w & a.pmask);
        const uint32_t from = __ballot(rs_rem<L>(a, p) < (uint32_t)a.K) ? 0u : (uint32_t)a.K;
        const uint64_t w8 = fbg_load8(a.T, (uint64_t)p + from);
        const uint32_t rank = fbg_ct_rank(lane, s, [&](uint32_t x, uint32_t) {
            const uint32_t px = (uint32_t)__shfl((int)p, (int)x, 64);
            const uint64_t wx = (uint64_t)(uint32_t)__shfl((int)(uint32_t)w8, (int)x, 64) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(w8 >> 32), (int)x, 64) << 32;
            return lane < s && x != lane && rc_text_less(a.T, (uint64_t)px + from, (uint64_t)p + from, wx, w8);   // (after the exchange: all lanes take part in it)
        });
        if (lane < s) a.keys[k0 + rank] = (w & ~a.pmask) | p;
    }
}

// One thread per candidate: the column of its slot, whether it begins and ends a same-column run, and its LCP with the slot
// before it, into arrays parallel to cand[]; the LCP with the slot after it only where that slot is not the next candidate
// (there it is that candidate's).  Every LCP of the tail is computed here, once.
#define RC_HEAD 0x80000000u
#define RC_TAIL 0x40000000u
#define RC_COL 0x3fffffffu
__global__ __launch_bounds__(256) void k_cand_lcp(RankArgs a, uint64_t T, uint32_t *__restrict__ cf, uint32_t *__restrict__ lp, uint32_t *__restrict__ ln)
{
    constexpr int L = FBG_SLOTS_PACKED;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t k = a.cand[t];
    const uint64_t next_cand = t + 1 < T ? (uint64_t)a.cand[t + 1] : ~0ull;
    const bool has_p = k > 0, has_n = k + 1 < a.N;
    const uint64_t w = a.keys[k], wp = has_p ? a.keys[k - 1] : 0ull, wn = has_n ? a.keys[k + 1] : 0ull;
    auto slot_of = [&](uint64_t word) {
        Slot s;
        s.key = word >> a.pb;
        s.pos = word & a.pmask;
        s.rem = rs_rem<L>(a, s.pos);
        s.col = rs_col_of_rem(a, s.rem);
        return s;
    };
    const Slot y = slot_of(w), x = slot_of(wp), z = slot_of(wn);
    uint32_t f = y.col;
    if (!(has_p && x.col == y.col)) f |= RC_HEAD;
    if (!(has_n && z.col == y.col)) f |= RC_TAIL;
    cf[t] = f;
    lp[t] = has_p ? rs_pair_lcp(a, x, y) : 0u;
    if (next_cand != k + 1) ln[t] = has_n ? rs_pair_lcp(a, y, z) : 0u;
}

// the LCP of the run's last member (candidate t + len - 1) with the slot after it
__device__ __forceinline__ uint32_t rc_end_lcp(const RankArgs &a, uint64_t T, uint64_t t, uint64_t len, const uint32_t *__restrict__ lp,
                                               const uint32_t *__restrict__ ln)
{
    const uint64_t e = t + len;
    return e < T && a.cand[e] == a.cand[e - 1] + 1 ? lp[e] : ln[e - 1];
}

// One thread per candidate; the head of a same-column run (its members are consecutive candidates) takes the two running minima
// over lp[] (fbg_ct_min_forward / _backward) and raises the column's maximum, as k_runs does.  A run of runs_wave_min members
// and more is noted for k_cand_runs_long while the list has room.
__global__ __launch_bounds__(256) void k_cand_runs(RankArgs a, uint64_t T, const uint32_t *__restrict__ cf, const uint32_t *__restrict__ lp,
                                                   const uint32_t *__restrict__ ln, uint32_t *__restrict__ pm)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint32_t f0 = cf[t], col = f0 & RC_COL;
    if (col == (uint32_t)a.n || !(f0 & RC_HEAD)) return;             // '#' / sentinel: not a row pointer; inside a run
    // the run's length: the tail flags, four candidates at a time
    const uint64_t room = T - t;
    uint64_t len = 0;
    bool tried = false;
    for (uint64_t i0 = 0; i0 < room && !len; i0 += 4) {
        uint32_t g[4];
#pragma unroll
        for (int q = 0; q < 4; q++) g[q] = cf[min(t + i0 + q, T - 1)];
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (!len && i0 + q < room && (g[q] & RC_TAIL)) len = i0 + q + 1;
        const uint64_t known = len ? len : i0 + 5;                     // members the run is known to have by now
        if (!tried && a.runs_wave_min >= 2 && known >= a.runs_wave_min) {
            tried = true;                                              // a long run: a wave walks it, unless the list is full
            const unsigned long long e = atomicAdd(&a.counters[7], 1ull);
            if (e < a.wl_cap) { a.wl[2 * e] = (uint32_t)t; a.wl[2 * e + 1] = a.cand[t]; return; }
        }
    }
    if (!len) len = room;
    const uint32_t n_mem = (uint32_t)len;
    fbg_ct_min_forward(0u, n_mem, FBG_CT_NONE, [&](uint32_t i) { return lp[t + i]; }, [&](uint32_t i, uint32_t v) { pm[t + i] = v; });
    const uint32_t end = rc_end_lcp(a, T, t, len, lp, ln);
    uint32_t best = 0;
    fbg_ct_min_backward(0u, n_mem, FBG_CT_NONE, [&](uint32_t i) { return i + 1 < n_mem ? lp[t + i + 1] : end; },
                        [&](uint32_t i) { return pm[t + i]; }, [&](uint32_t, uint32_t g) { best = max(best, g); });
    rs_update(a, col, best);                                           // (the members share their column)
}

// The runs k_cand_runs noted, a wave each: the walk over the LCP arrays (no LCP computed again).  Candidate t + i belongs to the
// run of head t while no candidate before it carries the tail flag.
__global__ __launch_bounds__(64) void k_cand_runs_long(RankArgs a, uint64_t T, const uint32_t *__restrict__ cf, const uint32_t *__restrict__ lp,
                                                       const uint32_t *__restrict__ ln, uint32_t *__restrict__ pm)
{
    if (blockIdx.x >= a.counters[7]) return;                            // (the grid is wl_cap blocks)
    const uint64_t t = a.wl[2 * blockIdx.x];
    rt_wave_walk<uint32_t>(a, cf[t] & RC_COL, pm + t,
                           [&](uint32_t i) { return t + i < T && !(i > 0 && (cf[t + i - 1] & RC_TAIL)); },
                           [&](uint32_t i) { return lp[t + i]; },
                           [&](uint32_t i, uint32_t len) {
                               const uint32_t end = rc_end_lcp(a, T, t, len, lp, ln);         // (the same for every lane)
                               return i + 1 < len ? lp[t + i + 1] : end;
                           });
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
RsScratch rs_scratch(fbg_ctx *ctx)
{
    return RsScratch{ctx->dp_e, ctx->dp_a, ctx->dp_b, ctx->dp_c, ctx->dp_d, ctx->dp_f, ctx->ps_g, ctx->ps_h};
}

// where k_tie_groups / k_cand_region note the tie groups of more than 64 members (their count is counters[5])
static int rs_big_list(fbg_ctx *ctx, RankArgs &a)
{
    FBG_TRY(fbg_reserve(ctx, ctx->big_groups, RS_BIG_GROUPS * 8));
    a.big = ctx->big_groups.as<uint32_t>();
    return FBG_OK;
}

// ... and, without partitions, the list of the runs that get a wave each (its count is counters[7], zeroed with the other
// counters); which runs go there
int rs_tail_prepare(fbg_ctx *ctx, RankArgs &a)
{
    FBG_TRY(rs_big_list(ctx, a));
    if (a.part_mode) return FBG_OK;
    FBG_TRY(fbg_reserve(ctx, ctx->wave_list, (size_t)2 * RS_WAVE_LIST * 4));
    a.wl = ctx->wave_list.as<uint32_t>();
    const int64_t cap = ctx->opt.wave_list_cap;
    a.wl_cap = cap > 0 && cap < RS_WAVE_LIST ? (uint32_t)cap : RS_WAVE_LIST;
    a.runs_wave_min = ctx->opt.runs_wave_min > 0 ? (uint32_t)ctx->opt.runs_wave_min : 0u;
    return FBG_OK;
}

// option cand_sort_check: count the places of the sorted list that do not ascend (a host round trip)
static int rs_check_sorted(fbg_ctx *ctx, const uint32_t *sorted, uint64_t T, int64_t *inversions)
{
    hipStream_t st = ctx->stream;
    unsigned long long *d_inv = &fbg_scalars(ctx)->cand_inversions, inv = 0;
    FBG_HIP_TRY(ctx, hipMemsetAsync(d_inv, 0, sizeof(inv), st));
    hipLaunchKernelGGL(k_cand_inversions, dim3(fbg_blocks(T, 256)), dim3(256), 0, st, sorted, T, d_inv);
    FBG_HIP_TRY(ctx, hipMemcpyAsync(&inv, d_inv, sizeof(inv), hipMemcpyDeviceToHost, st));
    FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *inversions = (int64_t)inv;
    return FBG_OK;
}

// the sorted candidates and their scratch, where rs_tail_order left them
static void rs_bind_sorted(fbg_ctx *ctx, RankArgs &a)
{
    const RsScratch s = rs_scratch(ctx);
    a.cand = s.sorted.as<uint32_t>();
    a.pm = s.pm.as<uint32_t>();
}

static int rs_order(fbg_ctx *ctx, RankArgs &a, int layout, bool lean, unsigned rs_blocks, RsTail *t, int *launches)
{
    hipStream_t st = ctx->stream;
    const RsScratch s = rs_scratch(ctx);
    // candidate counts per workgroup -> offsets; total and the largest count come back to the host
    uint32_t *d_counts = a.blk_count, *d_offs = s.offsets.as<uint32_t>();
    uint32_t *d_max = reinterpret_cast<uint32_t *>(a.counters + 6);           // (the fused kernel: total, largest)
    uint32_t tot = 0, mx = 0;
    if (ctx->opt.cand_counts_fused) {
        // one small kernel and one copy into pinned memory instead of a scan (two launches), a reduce and two copies
        if (!ctx->pin_pair) FBG_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->pin_pair), 2 * sizeof(uint32_t), hipHostMallocDefault));
        hipLaunchKernelGGL(k_cand_counts, dim3(1), dim3(RS_COUNTS_THREADS), 0, st, d_counts, (uint32_t)rs_blocks, d_offs, d_max);
        FBG_HIP_TRY(ctx, hipMemcpyAsync(ctx->pin_pair, d_max, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
        tot = ctx->pin_pair[0]; mx = ctx->pin_pair[1];
    } else {
        FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
            return rocprim::exclusive_scan(tmp, bytes, d_counts, d_offs, 0u, (size_t)(rs_blocks + 1), rocprim::plus<uint32_t>(), st);
        }));
        FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
            return rocprim::reduce(tmp, bytes, d_counts, d_max, 0u, (size_t)rs_blocks, rocprim::maximum<uint32_t>(), st);
        }));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&tot, d_offs + rs_blocks, 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipMemcpyAsync(&mx, d_max, 4, hipMemcpyDeviceToHost, st));
        FBG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    const uint64_t T = t->T = tot;
    if (mx > a.region) { t->overflow = true; return FBG_OK; }
    if (T == 0) return FBG_OK;
    // k_rank_scan: workgroup b owns chunks b, b+G, ...: not contiguous -> compact, then sort.  k_rank_scan_lean: one
    // stretch per workgroup -> every region sorted in LDS on its way out, where the largest fits
    const int64_t cap_opt = ctx->opt.cand_lds_cap;
    const uint32_t lds_cap = cap_opt > 0 && cap_opt < RS_CAND_LDS ? (uint32_t)cap_opt : RS_CAND_LDS;
    const bool local = lean && ctx->opt.cand_local_sort && mx <= lds_cap;
    // the tail by member: packed slots (the lean scan's), columns that leave the two flag bits of k_cand_lcp free
    const bool by_member = local && ctx->opt.cand_tail != 0 && a.n <= RC_COL;
    t->tier = by_member ? RsTier::by_member : local ? RsTier::by_head_local : RsTier::by_head_radix;
    if (t->tier == RsTier::by_head_radix) FBG_TRY(fbg_reserve(ctx, s.flat, T * 4));
    FBG_TRY(fbg_reserve(ctx, s.sorted, T * 4));
    FBG_TRY(fbg_reserve(ctx, s.pm, T * 4));
    uint32_t *sorted = s.sorted.as<uint32_t>();
    const int gallop = ctx->opt.tie_gallop != 0 ? 1 : 0;
    switch (t->tier) {
    case RsTier::by_member: {
        // sorted, written out at their offsets and the tie groups put in final order by one kernel.  LDS by the largest region:
        // the slots padded to a power of two, the words of the first RC_WORDS entries, the heads (every other entry at most) and
        // a list that holds every group of more than RC_SMALL members a region can head
        uint32_t pmax = 2;
        while (pmax < mx) pmax <<= 1;
        const uint32_t wcap = std::min<uint32_t>(mx, RC_WORDS), lcap = mx / (RC_SMALL + 1) + 1;
        const size_t lds = (size_t)wcap * 8 + (size_t)pmax * 4 + (size_t)lcap * 4 + (size_t)(mx / 2 + 2) * 2;
        hipLaunchKernelGGL(k_cand_region, dim3(rs_blocks), dim3(256), lds, st, a, d_counts, d_offs, sorted, gallop, mx, pmax, wcap, lcap);
        break;
    }
    case RsTier::by_head_local:
        hipLaunchKernelGGL(k_cand_sort_compact, dim3(rs_blocks), dim3(256), 0, st, a.cand, d_counts, d_offs, a.region, sorted);
        break;
    default: {
        uint32_t *flat = s.flat.as<uint32_t>();
        hipLaunchKernelGGL(k_cand_compact, dim3(rs_blocks), dim3(256), 0, st, a.cand, d_counts, d_offs, a.region, flat);
        FBG_TRY(fbg_with_tmp(ctx, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, flat, sorted, (size_t)T, 0u, 32u, st);
        }));
    }
    }
    if (ctx->opt.cand_sort_check) FBG_TRY(rs_check_sorted(ctx, sorted, T, &t->inversions));
    rs_bind_sorted(ctx, a);
    // tie groups in final order (k_cand_region has done those of up to 64 members); k_tie_big's `exact`: 0, or 2 behind the lean scan
    if (t->tier != RsTier::by_member) {
        RS_LAUNCH(k_tie_groups, layout, dim3(fbg_blocks(T, 64)), dim3(64), st, a, T, 1, gallop);
        (*launches)++;
    }
    RS_LAUNCH(k_tie_big, layout, dim3(RS_BIG_GROUPS), dim3(256), st, a, lean ? 2 : 0);
    *launches += 2;
    return FBG_OK;
}

int rs_tail_order(fbg_ctx *ctx, RankArgs &a, int layout, bool lean, unsigned rs_blocks, RsTail *t, int *launches)
{
    *t = RsTail{};
    const int rc = rs_order(ctx, a, layout, lean, rs_blocks, t, launches);
    // what the tail did, as fbg_get_option reports it: written here and nowhere else, from the value that steers the tail
    ctx->diag.cand_tail_used = t->tier == RsTier::by_member ? 1 : 0;
    if (t->tier != RsTier::none) ctx->diag.cand_local_sorted = t->tier == RsTier::by_head_radix ? 0 : 1;
    if (ctx->opt.cand_sort_check) ctx->diag.cand_inversions = t->inversions;
    return rc;
}

int rs_tail_runs(fbg_ctx *ctx, RankArgs &a, int layout, const RsTail &t, int *launches)
{
    if (t.tier == RsTier::none) return FBG_OK;
    hipStream_t st = ctx->stream;
    const uint64_t T = t.T;
    rs_bind_sorted(ctx, a);
    if (t.tier == RsTier::by_member) {
        // every LCP once, by candidate; then the runs' minima over those arrays
        FBG_TRY(fbg_reserve(ctx, ctx->cand_cf, T * 4));
        FBG_TRY(fbg_reserve(ctx, ctx->cand_lp, T * 4));
        FBG_TRY(fbg_reserve(ctx, ctx->cand_ln, T * 4));
        uint32_t *cf = ctx->cand_cf.as<uint32_t>(), *lp = ctx->cand_lp.as<uint32_t>(), *ln = ctx->cand_ln.as<uint32_t>();
        hipLaunchKernelGGL(k_cand_lcp, dim3(fbg_blocks(T, 256)), dim3(256), 0, st, a, T, cf, lp, ln);
        hipLaunchKernelGGL(k_cand_runs, dim3(fbg_blocks(T, 256)), dim3(256), 0, st, a, T, cf, lp, ln, a.pm);
        *launches += 2;
        if (a.runs_wave_min) { hipLaunchKernelGGL(k_cand_runs_long, dim3(a.wl_cap), dim3(64), 0, st, a, T, cf, lp, ln, a.pm); (*launches)++; }
    } else {
        RS_LAUNCH(k_runs, layout, dim3(fbg_blocks(T, 64)), dim3(64), st, a, T);
        (*launches)++;
        if (a.runs_wave_min) { RS_LAUNCH(k_runs_long, layout, dim3(a.wl_cap), dim3(64), st, a); (*launches)++; }
    }
    return FBG_OK;
}

int rs_tail_order_all(fbg_ctx *ctx, RankArgs &a, int layout)
{
    hipStream_t st = ctx->stream;
    const uint64_t own = a.own_hi - a.own_lo;
    FBG_TRY(rs_big_list(ctx, a));
    FBG_HIP_TRY(ctx, hipMemsetAsync(a.counters + 5, 0, sizeof(unsigned long long), st));
    RS_LAUNCH(k_tie_groups, layout, dim3(fbg_blocks(own, 256)), dim3(256), st, a, own, 0, ctx->opt.tie_gallop != 0 ? 1 : 0);
    RS_LAUNCH(k_tie_big, layout, dim3(RS_BIG_GROUPS), dim3(256), st, a, 1);
    return FBG_OK;
}
