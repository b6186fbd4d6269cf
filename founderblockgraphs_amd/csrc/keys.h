// keys.h -- what a sort key is, once: the first K symbol codes of a suffix, b bits each, most significant first, right aligned
// in a 64-bit word.  In the compact coding (rank-order scans) the code table flags separators ('#', the sentinel, positions
// beyond the text) with FBG_SEP, and a separator and everything behind it inside a key count as code 0; in the plain coding
// every byte value is an ordinary code.  The number of equal leading symbols of two different keys comes from a count of
// leading zeros.
// Plain C++ (no HIP types) like twin_hash.h, tie_extent.h and cand_tail.h: k_pack and the samples (suffix_sort.hip), the MSD
// sorts (msd_keys.h), the scans and the CPU check in host/host_selftest.cpp (mode keys) share it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FBG_KEY_HD __host__ __device__ __forceinline__
#define FBG_KEY_UNROLL _Pragma("unroll")
#else
#define FBG_KEY_HD inline
#define FBG_KEY_UNROLL
#endif

#define FBG_SEP 0x80
#define FBG_KEY_ITEMS 8                        // consecutive positions a thread builds the keys of

// ---- LCP of two keys ---------------------------------------------------------------------------------------------------------
// number of equal leading symbols of two different K-symbol keys (b bits per symbol, right aligned in key_bits = K * b bits);
// inv_b = fbg_key_inv(b), hoisted by callers with many pairs
FBG_KEY_HD uint32_t fbg_key_inv(int b) { return (65536u + (uint32_t)b - 1) / (uint32_t)b; }    // exact for numerators <= 64
FBG_KEY_HD uint32_t fbg_key_equal_bits(uint64_t a, uint64_t c, int key_bits)
{
    const uint64_t d = a ^ c;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(__clzll((long long)d) - (64 - key_bits));
#else
    return (uint32_t)(__builtin_clzll(d) - (64 - key_bits));
#endif
}
FBG_KEY_HD uint32_t fbg_key_lcp_inv(uint64_t a, uint64_t c, uint32_t inv_b, int key_bits)
{
    return (fbg_key_equal_bits(a, c, key_bits) * inv_b) >> 16;
}
FBG_KEY_HD uint32_t fbg_key_lcp(uint64_t a, uint64_t c, int b, int key_bits)
{
    return (fbg_key_equal_bits(a, c, key_bits) * fbg_key_inv(b)) >> 16;
}

// ---- one symbol ----------------------------------------------------------------------------------------------------------------
// The code that symbol code c adds to a key: a separator kills the rest of the key (compact coding only; dead is carried from
// symbol to symbol of one key).
FBG_KEY_HD uint32_t fbg_key_symbol(uint32_t c, int compact, bool &dead)
{
    dead = dead || (compact && (c & FBG_SEP));
    return dead ? 0u : c;
}

// ---- the keys of FBG_KEY_ITEMS consecutive positions ---------------------------------------------------------------------------
// tile[] holds the symbol codes of a stretch of text; w[i] = key of position t0 + i.  The builders read tile[t0 .. t0 + K + 6].
// rolling: the first key symbol by symbol, the following ones drop the leading symbol and append one -- one byte read per
// position.  Separators are not looked at; returns the OR of the codes read, from which the caller sees whether there was one.
FBG_KEY_HD uint32_t fbg_keys_rolling(const uint8_t *tile, int t0, int b, int K, uint64_t *w)
{
    const uint64_t mask = (K * b) >= 64 ? ~0ull : ((1ull << (K * b)) - 1);
    uint64_t key = 0;
    uint32_t seen = 0;
    for (int k = 0; k < K; k++) { const uint32_t c = tile[t0 + k]; seen |= c; key = (key << b) | c; }
FBG_KEY_UNROLL
    for (int i = 0; i < FBG_KEY_ITEMS; i++) {
        w[i] = key;
        const uint32_t c = tile[t0 + K + i];
        seen |= c;
        key = ((key << b) | c) & mask;
    }
    return seen;
}

// symbol by symbol, compact coding: for the positions with a row end in reach
FBG_KEY_HD void fbg_keys_by_symbol(const uint8_t *tile, int t0, int b, int K, uint64_t *w)
{
FBG_KEY_UNROLL
    for (int i = 0; i < FBG_KEY_ITEMS; i++) {
        uint64_t kk = 0;
        bool dead = false;
        for (int k = 0; k < K; k++) kk = (kk << b) | fbg_key_symbol(tile[t0 + i + k], 1, dead);
        w[i] = kk;
    }
}

// 2-bit symbols, K + FBG_KEY_ITEMS - 1 <= 32: the 32 symbols from t0 on packed into one word (four 8-byte reads, t0 a multiple
// of 8; two multiplies per 8 bytes gather the low two bits of every byte), every key a shift of it.  Separators are not looked
// at; returns whether there was one among the 32 symbols.
FBG_KEY_HD bool fbg_keys_gather2(const uint8_t *tile, int t0, int K, uint64_t *w)
{
    uint64_t P = 0, any = 0;
FBG_KEY_UNROLL
    for (int q = 0; q < 4; q++) {
        const uint64_t x = *reinterpret_cast<const uint64_t *>(tile + t0 + 8 * q);
        any |= x;
        const uint32_t lo = (uint32_t)x & 0x03030303u, hi = (uint32_t)(x >> 32) & 0x03030303u;
        const uint32_t g = (((lo * 0x40100401u) >> 24) << 8) | ((hi * 0x40100401u) >> 24);    // 8 symbols, first one on top
        P |= (uint64_t)g << (48 - 16 * q);
    }
    const bool sep = (any & 0x8080808080808080ull) != 0;
FBG_KEY_UNROLL
    for (int i = 0; i < FBG_KEY_ITEMS; i++) w[i] = (P << (2 * i)) >> (64 - 2 * K);
    return sep;
}

// compact coding, any geometry: the fast builder that fits, then symbol by symbol where a row ends nearby (the MSD sorts)
FBG_KEY_HD void msd_build_keys(const uint8_t *tile, int t0, int b, int K, uint64_t *w)
{
    bool slow = true;
    if (b == 2 && K + FBG_KEY_ITEMS - 1 <= 32) slow = fbg_keys_gather2(tile, t0, K, w);
    if (b != 2 || K + FBG_KEY_ITEMS - 1 > 32) slow = (fbg_keys_rolling(tile, t0, b, K, w) & FBG_SEP) != 0;
    if (slow) fbg_keys_by_symbol(tile, t0, b, K, w);
}
