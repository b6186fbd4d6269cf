// msd_keys.h -- the tiles of the MSD sorts (msd_sort.hip, msd_sort_pairs.hip): the symbol codes of a tile of text into
// LDS, from which msd_build_keys (keys.h) makes the keys of a thread's 8 consecutive positions; cursors and wave sums.
#pragma once
#include <stdint.h>
#include "keys.h"

#define MSD_ITEMS FBG_KEY_ITEMS

// Pass 1 of both sorts keeps one run cursor per stretch (bucket d of nb, part xq of xs: one part per XCD).  The stretch's
// number d * xs + xq says where it lies in the pass-1 buffer and in tile_start; its cursor lies at xq * nb + d (contig,
// option msd_cursors, the default), so that the 64 lanes of a reserving wave -- 64 buckets, one part -- add to consecutive
// words, one 256-byte request; at the stretch's own number (contig = false, the earlier placement) they lie xs words apart.
__host__ __device__ __forceinline__ uint32_t msd_cursor_index(uint32_t d, uint32_t xq, uint32_t xs, uint32_t nb, bool contig)
{
    return contig ? xq * nb + d : d * xs + xq;
}

// The symbol codes of text positions base .. base + TILE + 64 go to LDS in two steps, so that a kernel walking several
// tiles can have the next tile's loads in flight: msd_fetch_raw (8 text bytes per thread, threads 0..7 also the 64
// bytes of lookahead; T is padded beyond N, base is a multiple of 8) and msd_store_tile (code table cd in LDS).
template <int TILE>
__device__ __forceinline__ void msd_fetch_raw(const uint8_t *__restrict__ T, uint64_t N, uint64_t base, uint64_t &raw, uint64_t &raw2)
{
    const uint64_t p = base + threadIdx.x * 8;
    raw = p < N + 56 ? *reinterpret_cast<const uint64_t *>(T + p) : 0ull;
    raw2 = 0;
    if (threadIdx.x < 8) {
        const uint64_t q = base + TILE + threadIdx.x * 8;
        raw2 = q < N + 56 ? *reinterpret_cast<const uint64_t *>(T + q) : 0ull;
    }
}
// FULL: the tile and its lookahead lie inside the text (base + TILE + 64 <= N): no end-of-text checks
template <int TILE, bool FULL = false>
__device__ __forceinline__ void msd_store_tile(uint8_t *tile, const uint8_t *cd, uint64_t N, uint64_t base, uint64_t raw, uint64_t raw2)
{
    const int k8 = threadIdx.x * 8;
    const uint64_t p = base + k8;
    uint64_t codes = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t c = (FULL || p + j < N) ? cd[(raw >> (8 * j)) & 255u] : (uint32_t)FBG_SEP;
        codes |= (uint64_t)c << (8 * j);
    }
    *reinterpret_cast<uint64_t *>(tile + k8) = codes;
    if (threadIdx.x < 8) {
        const int kk = TILE + threadIdx.x * 8;
        const uint64_t q = base + kk;
        uint64_t codes2 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t c = (FULL || q + j < N) ? cd[(raw2 >> (8 * j)) & 255u] : (uint32_t)FBG_SEP;
            codes2 |= (uint64_t)c << (8 * j);
        }
        *reinterpret_cast<uint64_t *>(tile + kk) = codes2;
    }
}
// msd_store_tile with the table lookups of a thread issued as one batch (option msd_lds_batch): at the text's end every
// byte is still looked up -- any byte is a valid index of cd -- and the end-of-text check is a select behind the reads,
// so that no lookup sits in a branch of its own and is awaited alone.  FULL as above; the caller's choice must be the
// same in all threads of the workgroup only where it wraps barriers (it does not here).
template <int TILE, bool FULL>
__device__ __forceinline__ void msd_store_tile_batched(uint8_t *tile, const uint8_t *cd, uint64_t N, uint64_t base, uint64_t raw, uint64_t raw2)
{
    const int k8 = threadIdx.x * 8;
    const uint64_t p = base + k8;
    uint32_t c[8];
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = cd[(raw >> (8 * j)) & 255u];
    uint64_t codes = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) codes |= (uint64_t)((FULL || p + j < N) ? c[j] : (uint32_t)FBG_SEP) << (8 * j);
    *reinterpret_cast<uint64_t *>(tile + k8) = codes;
    // the 64 bytes of lookahead: threads 0 .. 7 hold them (msd_fetch_raw); their wave does 8 more lookups, in one batch too
    if (threadIdx.x < 8) {
        const int kk = TILE + threadIdx.x * 8;
        const uint64_t q = base + kk;
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = cd[(raw2 >> (8 * j)) & 255u];
        uint64_t codes2 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) codes2 |= (uint64_t)((FULL || q + j < N) ? c[j] : (uint32_t)FBG_SEP) << (8 * j);
        *reinterpret_cast<uint64_t *>(tile + kk) = codes2;
    }
}

// sum of wsum[0 .. wv - 1], wv < NW <= 16 (the scan totals of the waves in front of this one; all 64 lanes call): lane q
// reads wsum[q], one LDS read, and the lanes below wv are added up along their row of 16 lanes (three or four DPP
// shifts, no LDS), instead of a loop of up to wv reads that are awaited one by one
template <int NW>
__device__ __forceinline__ uint32_t msd_waves_before(const uint32_t *wsum, uint32_t wv)
{
    static_assert(NW == 8 || NW == 16, "one row of 16 lanes");
    const uint32_t lane = threadIdx.x & 63;
    uint32_t v = wsum[lane & (NW - 1)];
    v = lane < wv ? v : 0u;
    // row_shr:d with zero fill: lane l adds lane l - d of its row
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    if (NW > 8) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, NW - 1);
}

template <int TILE, bool FULL = false>
__device__ __forceinline__ void msd_load_tile(uint8_t *tile, const uint8_t *cd, const uint8_t *__restrict__ T, uint64_t N, uint64_t base)
{
    uint64_t raw, raw2;
    msd_fetch_raw<TILE>(T, N, base, raw, raw2);
    msd_store_tile<TILE, FULL>(tile, cd, N, base, raw, raw2);
}
