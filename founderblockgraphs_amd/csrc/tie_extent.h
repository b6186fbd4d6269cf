// tie_extent.h -- how many consecutive slots of a sorted array carry one key, in O(log s) reads.
// Plain C++ (no HIP types): rank_tail.hip's k_tie_groups and k_cand_region and the CPU check in host/host_selftest.cpp share it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FBG_TIE_HD __host__ __device__
#else
#define FBG_TIE_HD
#endif

// Most tie groups are pairs and triples: the first slots are looked at one by one, as a plain count would.
#define FBG_TIE_PROBE 8

// The slots are sorted by key and slot k0 carries `key`: the number of slots from k0 on that carry it, looking no further than
// slot hi - 1 and counting no further than cap + 1 -- what
//     s = 1; while (k0 + s < hi && s <= cap && key_at(k0 + s) == key) s++;
// returns.  A group ends at the first slot whose key differs: FBG_TIE_PROBE slots one by one, then steps that double until a
// slot differs (or the limit is reached), then bisection between the last slot known to carry the key and that one.
template <class KeyAt> FBG_TIE_HD inline uint32_t fbg_tie_extent(uint64_t k0, uint64_t hi, uint32_t cap, uint64_t key, KeyAt key_at)
{
    const uint64_t room = hi - k0;
    const uint32_t limit = room < (uint64_t)cap + 1 ? (uint32_t)room : cap + 1;     // the most the answer can be (>= 1)
    uint32_t lo = 1;                                                                // slots k0 .. k0 + lo - 1 carry the key
    while (lo < limit && lo < FBG_TIE_PROBE) {
        if (key_at(k0 + lo) != key) return lo;
        lo++;
    }
    if (lo >= limit) return limit;
    uint32_t end = limit;                                                           // slot k0 + end differs, or end == limit
    for (uint32_t step = FBG_TIE_PROBE;; step <<= 1) {
        const uint32_t probe = limit - lo > step ? lo + step - 1 : limit - 1;
        if (key_at(k0 + probe) != key) { end = probe; break; }
        lo = probe + 1;
        if (lo >= limit) return limit;
    }
    while (lo < end) {
        const uint32_t mid = lo + (end - lo) / 2;
        if (key_at(k0 + mid) == key) lo = mid + 1;
        else end = mid;
    }
    return lo;
}
