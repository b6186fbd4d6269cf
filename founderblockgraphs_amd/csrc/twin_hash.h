// twin_hash.h -- twins among a sample of keys, counted with an open-addressing table instead of a sort.
// Plain C++ (no HIP types): suffix_sort.hip's k_sample_twins and the CPU check in host/host_selftest.cpp share the slot
// choice, the probe step and the way the counters are read.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FBG_TWIN_HD __host__ __device__
#else
#define FBG_TWIN_HD
#endif

// An empty word of the table.  A key of this value cannot be stored: such keys are counted in a word of their own.
#define FBG_TWIN_EMPTY 0xffffffffffffffffull
// The table has 2^(FBG_TWIN_SPARE + log2 S) words for S keys: at most half of them are ever taken, a probe always ends.
#define FBG_TWIN_SPARE 1

// first slot of a key in a table of 2^bits words (bits >= 1): the top bits of a multiplicative hash, into which every bit
// of the key goes (neighbouring keys -- texts of few symbols make keys that differ in their low bits only -- part at once)
FBG_TWIN_HD inline uint64_t fbg_twin_slot(uint64_t key, int bits)
{
    return ((key ^ (key >> 29)) * 0x9E3779B97F4A7C15ull) >> (64 - bits);
}

// the slot looked at after `slot`: linear probing, the table is a ring
FBG_TWIN_HD inline uint64_t fbg_twin_next(uint64_t slot, int bits) { return (slot + 1) & ((1ull << bits) - 1); }

// One insertion.  cas(slot, key): the word of `slot` before the call, which stores `key` there when the word was empty
// (atomicCAS on the device).  Returns 1 when the key was in the table already (a twin), 0 when it was stored -- or when
// the table is full, which a table of more words than keys never is.
template <class Cas> FBG_TWIN_HD inline uint32_t fbg_twin_insert(uint64_t key, int bits, Cas cas)
{
    uint64_t slot = fbg_twin_slot(key, bits);
    for (uint64_t probe = 0; probe < (1ull << bits); probe++) {
        const uint64_t seen = cas(slot, key);
        if (seen == FBG_TWIN_EMPTY) return 0;
        if (seen == key) return 1;
        slot = fbg_twin_next(slot, bits);
    }
    return 0;
}

// The two counter words lie behind the table and are filled with all-ones like it (one fill for everything), so each
// reads one less than was added to it.  counters[0]: twins found by insertion; counters[1]: keys equal to FBG_TWIN_EMPTY,
// all but the first of which are twins.  Together: S minus the number of distinct keys.
FBG_TWIN_HD inline uint64_t fbg_twin_total(uint64_t counter0, uint64_t counter1)
{
    const uint64_t found = counter0 + 1, ones = counter1 + 1;
    return found + (ones ? ones - 1 : 0);
}
