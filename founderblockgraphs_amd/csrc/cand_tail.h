// cand_tail.h -- the logic of the rank-order scan's tail that works member by member (rank_tail.hip: k_cand_region, k_cand_lcp,
// k_cand_runs): where a tie group begins in a sorted candidate list and where its keys are found, the order of a group's
// members as ranks, and the two running minima of a same-column run over arrays of neighbour LCPs.
// Plain C++ (no HIP types), templated on accessors like tie_extent.h: the kernels and the CPU check in host/host_selftest.cpp
// (mode cand-tail) share it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FBG_CT_HD __host__ __device__ __forceinline__
#define FBG_CT_UNROLL _Pragma("unroll")
#else
#define FBG_CT_HD inline
#define FBG_CT_UNROLL
#endif

#define FBG_CT_NONE 0xffffffffu

// ---- tie groups ------------------------------------------------------------------------------------------------------------
// Slot k of the sorted slots [lo, hi) heads a tie group when its key equals its successor's and not its predecessor's.
template <class KeyAt> FBG_CT_HD bool fbg_ct_heads_group(uint64_t k, uint64_t lo, uint64_t hi, KeyAt key_at)
{
    const uint64_t key = key_at(k);
    if (k > lo && key_at(k - 1) == key) return false;                  // inside a group
    return k + 1 < hi && key_at(k + 1) == key;
}

// The key of slot k >= k0, where k0 is entry i of a region's c ascending candidate slots: the members of a group that is not
// "simple" are candidates with consecutive slot numbers, so as long as the entries go on consecutively the region's own copy
// (key_local, by entry) answers; past a gap or the region's end the slots themselves do (key_slot, by slot).
template <class SlotAt, class KeyLocal, class KeySlot>
FBG_CT_HD uint64_t fbg_ct_key_from(uint32_t i, uint32_t c, uint64_t k0, uint64_t k, SlotAt slot_at, KeyLocal key_local, KeySlot key_slot)
{
    const uint64_t j = (uint64_t)i + (k - k0);
    return j < c && slot_at((uint32_t)j) == k ? key_local((uint32_t)j) : key_slot(k);
}

// Where the text comparison of a group's members starts: the first K symbols agree -- unless a member has fewer than K symbols
// left in its row, then the keys agree only up to the separator coding and the comparison starts at the suffixes' first symbol.
template <class RemAt> FBG_CT_HD uint32_t fbg_ct_from(uint32_t s, uint32_t K, RemAt rem_at)
{
    uint32_t from = K;
    for (uint32_t i = 0; i < s; i++)
        if (rem_at(i) < K) from = 0;
    return from;
}

// The place of member `me` in the text order of the group's s members: how many are smaller (less(j, me): member j's suffix is
// smaller than member me's; the suffixes are distinct, so the places of all members are a permutation).  less is called for
// every j, j == me included, where it returns false: on the GPU the lanes of a wave call it side by side and exchange their
// members inside it, so no lane may skip a call.
template <class Less> FBG_CT_HD uint32_t fbg_ct_rank(uint32_t me, uint32_t s, Less less)
{
    uint32_t rank = 0;
    for (uint32_t j = 0; j < s; j++) rank += less(j, me) ? 1u : 0u;
    return rank;
}

// The same for all members of a group of at most S at once, every pair compared once and no array indexed at run time: S is a
// small constant, the loops unroll, rank[] stays in registers.  rank[i] for i >= s is not meaningful.
template <int S, class Less> FBG_CT_HD void fbg_ct_small_ranks(uint32_t s, Less less, uint32_t (&rank)[S])
{
FBG_CT_UNROLL
    for (int i = 0; i < S; i++) rank[i] = 0;
FBG_CT_UNROLL
    for (int i = 0; i < S; i++)
FBG_CT_UNROLL
        for (int j = i + 1; j < S; j++)
            if ((uint32_t)j < s) {
                if (less(i, j)) rank[j]++;
                else rank[i]++;
            }
}

// ---- same-column runs --------------------------------------------------------------------------------------------------------
// A run's members 0 .. len-1 are consecutive SA slots; lp(i) is the LCP of member i with the slot before it, nx(i) the LCP of
// member i with the slot after it (nx(i) = lp(i + 1) inside the run).  Member i extends by
//     max(min(lp(0 .. i)), min(nx(i .. len-1))) + 1.
// Both minima run in pieces [i0, i1) with a carry from piece to piece (FBG_CT_NONE to start with), so a run may be worked in
// chunks: forward in ascending pieces, backward in descending ones.

// Both read their arrays four members at a time ahead of use: the reads of a batch do not wait for one another.

// forward: pm(i) = min(carry, lp(i0 .. i)) for i in [i0, i1); returns the carry for the next piece
template <class LpAt, class PmSet> FBG_CT_HD uint32_t fbg_ct_min_forward(uint32_t i0, uint32_t i1, uint32_t carry, LpAt lp_at, PmSet pm_set)
{
    uint32_t i = i0;
    for (; i1 - i >= 4; i += 4) {
        uint32_t v[4];
FBG_CT_UNROLL
        for (int q = 0; q < 4; q++) v[q] = lp_at(i + (uint32_t)q);
FBG_CT_UNROLL
        for (int q = 0; q < 4; q++) {
            carry = v[q] < carry ? v[q] : carry;
            pm_set(i + (uint32_t)q, carry);
        }
    }
    for (; i < i1; i++) {
        const uint32_t v = lp_at(i);
        carry = v < carry ? v : carry;
        pm_set(i, carry);
    }
    return carry;
}

// backward: for i = i1-1 down to i0, emit(i, max(pm(i), min(carry, nx(i .. i1-1))) + 1); returns the carry for the piece below
template <class NxAt, class PmAt, class Emit>
FBG_CT_HD uint32_t fbg_ct_min_backward(uint32_t i0, uint32_t i1, uint32_t carry, NxAt nx_at, PmAt pm_at, Emit emit)
{
    uint32_t i = i1;
    for (; i - i0 >= 4; i -= 4) {
        uint32_t v[4], p[4];
FBG_CT_UNROLL
        for (int q = 0; q < 4; q++) { v[q] = nx_at(i - 1 - (uint32_t)q); p[q] = pm_at(i - 1 - (uint32_t)q); }
FBG_CT_UNROLL
        for (int q = 0; q < 4; q++) {
            carry = v[q] < carry ? v[q] : carry;
            emit(i - 1 - (uint32_t)q, (p[q] > carry ? p[q] : carry) + 1);
        }
    }
    for (; i > i0; i--) {
        const uint32_t v = nx_at(i - 1);
        carry = v < carry ? v : carry;
        const uint32_t p = pm_at(i - 1);
        emit(i - 1, (p > carry ? p : carry) + 1);
    }
    return carry;
}
